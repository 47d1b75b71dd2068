"""Boundary counters on the GPU: dupl_seg_boundary (csrc/boundary.hip) and ops.seg_boundary against tests/boundary_ref.py (scipy
filters / erosions, not the kernel's separable search).  Everything is an integer: every comparison is exact equality.  The int64
maps sit in sentinel-slack buffers (a sentinel read as a label is out of range and would change the distances next to it), the
counters and, in the raw calls, the distance maps too (tests/kernel_guard.py).

  1. band_hist, biou, dist_gt and dist_pred equal the reference over shapes x R; band_hist.sum(0) is confusion_accum's matrix; a
     second update doubles the counts; a repeated call is bit-identical;
  2. the special maps: uniform, checkerboard, all-ignored gt, label changes on the tile seams and R / R + 1 away from them;
  3. out-of-range predictions are skipped; non-contiguous views; the distance maps stay inside their buffers;
  4. every ValueError and every DUPL_ERR_ARG comes before anything is written."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import boundary_ref as BR
import kernel_guard as KG

pytestmark = pytest.mark.gpu

TH, TW = 16, 64              # the column kernel's tile (BD_TH, BD_TW); the row kernel works on 64-pixel chunks of a row
SHAPES = [(1, 1), (1, 9), (9, 1), (TH, TW), (TH + 1, TW), (TH, TW + 1), (TH + 1, TW + 1), (5, 257), (33, 130)]
RS = [1, 3, TH + 1, 64]
NCS = [3, 21, 81]


def blocky(H, W, nc, seed, void):
    """(gt, pred): low-resolution random maps, Kronecker-upsampled by 8; pred is gt shifted, with a fifth of its 4 x 4 blocks redrawn;
    void "sprinkle": 3 % of gt is 255, "contour": the gt pixels next to a label change are 255 (VOC's outline)."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, nc, ((H + 7) // 8, (W + 7) // 8))
    gt = np.kron(low, np.ones((8, 8), dtype=np.int64))[:H, :W]
    pred = np.roll(gt, (2, 3), axis=(0, 1))
    noise = np.kron(rng.integers(0, nc, ((H + 3) // 4, (W + 3) // 4)), np.ones((4, 4), dtype=np.int64))[:H, :W]
    redraw = np.kron(rng.random(((H + 3) // 4, (W + 3) // 4)) < 0.2, np.ones((4, 4), dtype=bool))[:H, :W]
    pred = np.where(redraw, noise, pred)
    if void == "sprinkle":
        gt = np.where(rng.random((H, W)) < 0.03, 255, gt)
    elif void == "contour":
        edge = np.zeros((H, W), dtype=bool)
        edge[:, 1:] |= gt[:, 1:] != gt[:, :-1]
        edge[1:, :] |= gt[1:, :] != gt[:-1, :]
        gt = np.where(edge, 255, gt)
    return np.ascontiguousarray(gt, dtype=np.int64), np.ascontiguousarray(pred, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def blocky_case(shape, R):
    """one (shape, R) case with its reference, computed once and shared; treat as read-only"""
    i = SHAPES.index(shape) * len(RS) + RS.index(R)
    nc = NCS[i % 3]
    d = [BR.biou_dist(*shape), 5, 64, R][i % 4]
    gt, pred = blocky(shape[0], shape[1], nc, seed=i, void=("sprinkle", "contour")[i % 2])
    return gt, pred, nc, d, BR.reference(gt, pred, nc, R, d)


def guarded(arr, dev):
    return KG.Guard(arr.shape, dev, torch.int64, init=torch.from_numpy(arr)).view


def run(gt, pred, nc, R, d, dev, hist=None, biou=None, want_dist=True):
    from dupl_amd import ops
    return ops.seg_boundary(guarded(gt, dev), guarded(pred, dev), num_classes=nc, max_dist=R, biou_dist=d, band_hist=hist, biou=biou,
                            want_dist=want_dist)


def check(gt, pred, nc, R, d, ref, dev):
    """one call into guarded counters equals ref; returns the counters' Guards"""
    from dupl_amd import ops
    hist = KG.Guard((R + 1, nc, nc), dev, torch.int64, init=torch.zeros((R + 1, nc, nc), dtype=torch.int64))
    biou = KG.Guard((3, nc), dev, torch.int64, init=torch.zeros((3, nc), dtype=torch.int64))
    _, b, dg, dp = run(gt, pred, nc, R, d, dev, hist.view, biou.view)
    assert np.array_equal(hist.cpu().numpy(), ref[0])
    if d > 0:
        assert b is biou.view and np.array_equal(biou.cpu().numpy(), ref[1])
    else:
        assert b is None and not biou.cpu().any()
    assert np.array_equal(dg.cpu().numpy(), ref[2]) and np.array_equal(dp.cpu().numpy(), ref[3])
    conf = torch.zeros((nc, nc), device=dev, dtype=torch.int64)
    ops.confusion_accum(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev), conf)
    assert torch.equal(hist.view.sum(0), conf)
    return hist, biou


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blocky_maps_equal_the_reference(dev, shape, R):
    gt, pred, nc, d, ref = blocky_case(shape, R)
    if min(shape) >= TH and R <= 3:          # the case is meant to discriminate: pixels at a label change and pixels farther than R
        assert ref[0][0].sum() > 0 and ref[0][R].sum() > 0
        assert ref[1][1].sum() > 0
    hist, biou = check(gt, pred, nc, R, d, ref, dev)
    # a second update adds the same counts again; a fresh call is bit-identical to the first
    run(gt, pred, nc, R, d, dev, hist.view, biou.view, want_dist=False)
    assert np.array_equal(hist.cpu().numpy(), 2 * ref[0]) and np.array_equal(biou.cpu().numpy(), 2 * ref[1])
    again = run(gt, pred, nc, R, d, dev)
    assert np.array_equal(again[0].cpu().numpy(), ref[0]) and np.array_equal(again[1].cpu().numpy(), ref[1])
    assert np.array_equal(again[2].cpu().numpy(), ref[2]) and np.array_equal(again[3].cpu().numpy(), ref[3])


@pytest.mark.parametrize("nc", NCS)
def test_uniform_checkerboard_and_all_ignored(dev, nc):
    H, W, R, d = 33, 130, 3, 2
    c = nc - 1
    uni = np.full((H, W), c, dtype=np.int64)
    ref = BR.reference(uni, uni, nc, R, d)
    assert ref[0][R, c, c] == H * W and ref[0][:R].sum() == 0                      # everything in bin R
    frame = H * W - (H - 2 * d) * (W - 2 * d)                                      # with the border counted the band is the frame
    assert ref[1][:, c].tolist() == [frame, frame, frame]
    check(uni, uni, nc, R, d, ref, dev)
    ys, xs = np.mgrid[0:H, 0:W]
    chk = ((ys + xs) % 2).astype(np.int64) * c
    ref = BR.reference(chk, uni, nc, R, d)
    assert ref[0][0].sum() == H * W and ref[0][1:].sum() == 0                      # everything in bin 0
    check(chk, uni, nc, R, d, ref, dev)
    ign = np.full((H, W), 255, dtype=np.int64)
    ref = BR.reference(ign, chk, nc, R, d)
    assert ref[0].sum() == 0 and ref[1].sum() == 0                                 # nothing counted
    check(ign, chk, nc, R, d, ref, dev)


@pytest.mark.parametrize("R", [3, TH + 1])
def test_label_changes_on_and_near_the_tile_seams(dev, R):
    """gt: one vertical and one horizontal label change at a time, exactly on a tile seam of the column kernel (x = 64, y = 16) and of
    the row kernel's chunks (x = 256) and a row that is no multiple of anything (y = 4), and R and R + 1 before and behind it; pred has its changes three pixels further."""
    H, W, nc = 3 * TH, 256 + 2 * R + 8, 4
    ys, xs = np.mgrid[0:H, 0:W]
    for seam_x, seam_y in ((TW, TH), (256, 4)):
        for off in (0, R, R + 1, -R, -R - 1):
            bx, by = seam_x + off, seam_y + off
            if not (0 < by < H and 0 < bx < W):
                continue
            gt = ((xs >= bx) + 2 * (ys >= by)).astype(np.int64)
            pred = ((xs >= bx + 3) + 2 * (ys >= by - 3)).astype(np.int64)
            d = R + 1 if off else 2
            ref = BR.reference(gt, pred, nc, R, d)
            assert ref[0][0].sum() > 0 and ref[0][R].sum() > 0 and ref[0][R - 1].sum() > 0
            check(gt, pred, nc, R, d, ref, dev)


def test_out_of_range_predictions_are_skipped(dev):
    nc, R, d = 21, 3, 2
    gt, pred = blocky(33, 130, nc, seed=99, void="sprinkle")
    for bad in (-1, nc, 255, 1 << 40):
        p = pred.copy()
        p[5:9, 60:70] = bad
        p[20, :] = bad
        ref = BR.reference(gt, p, nc, R, d)
        assert ref[0].sum() < BR.band_hist(gt, pred, nc, R).sum()
        check(gt, p, nc, R, d, ref, dev)


def test_non_contiguous_views(dev):
    from dupl_amd import ops
    nc, R, d = 21, 3, 2
    gt, pred = blocky(33, 130, nc, seed=7, void="contour")
    ref = BR.reference(gt, pred, nc, R, d)
    big = torch.full((66, 260), 255, dtype=torch.int64, device=dev)
    big[::2, ::2] = torch.from_numpy(gt).to(dev)
    pt = torch.from_numpy(np.ascontiguousarray(pred.T)).to(dev).t()
    assert not big[::2, ::2].is_contiguous() and not pt.is_contiguous()
    h, b, dg, dp = ops.seg_boundary(big[::2, ::2], pt, num_classes=nc, max_dist=R, biou_dist=d, want_dist=True)
    got = (h.cpu().numpy(), b.cpu().numpy(), dg.cpu().numpy(), dp.cpu().numpy())
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))


class Raw:
    """One raw dupl_seg_boundary call on guarded buffers."""

    def __init__(self, gt, pred, nc, R, d, dev, ws_short=0, over=None):
        from dupl_amd import _lib, ops
        H, W = gt.shape
        self.gt, self.pred = guarded(gt, dev), guarded(pred, dev)
        self.hist = KG.Guard((R + 1, nc, nc), dev, torch.int64)
        self.biou = KG.Guard((3, nc), dev, torch.int64)
        self.dg, self.dp = KG.Guard((H, W), dev, torch.uint8, front=KG.PAD_U8 + 3), KG.Guard((H, W), dev, torch.uint8, front=KG.PAD_U8 + 1)
        good = _lib.SegBoundaryDesc(H=H, W=W, num_classes=nc, max_dist=R, biou_dist=d)
        nbytes = _lib.lib().dupl_seg_boundary_workspace(ctypes.byref(good))
        assert nbytes >= 6 * H * W
        self.ws = KG.Guard((nbytes - ws_short,), dev, torch.uint8)
        desc = _lib.SegBoundaryDesc(H=H, W=W, num_classes=nc, max_dist=R, biou_dist=d, gt=self.gt.data_ptr(), pred=self.pred.data_ptr(),
                                    band_hist=self.hist.ptr, biou=self.biou.ptr, dist_gt=self.dg.ptr, dist_pred=self.dp.ptr,
                                    workspace=self.ws.ptr, workspace_bytes=nbytes - ws_short)
        for k, v in (over or {}).items():
            setattr(desc, k, v)
        self.size_query = _lib.lib().dupl_seg_boundary_workspace(ctypes.byref(desc))
        self.status = _lib.lib().dupl_seg_boundary.raw(ctypes.byref(desc), ops._stream())
        torch.cuda.synchronize()

    def outputs_untouched(self):
        return all(g.untouched() for g in (self.hist, self.biou, self.dg, self.dp, self.ws))


@pytest.mark.parametrize("shape", [(1, 1), (TH + 1, TW + 1), (5, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_raw_call_stays_inside_its_buffers(dev, shape):
    gt, pred, nc, d, ref = blocky_case(shape, 3)
    r = Raw(gt, pred, nc, 3, d, dev)
    assert r.status == 0
    assert np.array_equal(r.dg.cpu().numpy(), ref[2]) and np.array_equal(r.dp.cpu().numpy(), ref[3])
    assert r.hist.intact() and r.biou.intact() and r.ws.intact()


def test_bad_descriptors_are_refused_before_any_launch(dev):
    gt, pred, nc, d, _ = blocky_case((TH + 1, TW + 1), 3)
    bad = [dict(gt=None), dict(pred=None), dict(band_hist=None), dict(biou=None), dict(workspace=None), dict(max_dist=0), dict(max_dist=65),
           dict(biou_dist=-1), dict(biou_dist=65), dict(H=0), dict(W=0), dict(H=-3), dict(num_classes=0), dict(num_classes=256),
           dict(struct_size=8)]
    for over in bad:
        r = Raw(gt, pred, nc, 3, d, dev, over=over)
        assert r.status == -1 and r.outputs_untouched(), over
        if not any(k in over for k in ("gt", "pred", "band_hist", "biou", "workspace")):
            assert r.size_query <= 0, over
    r = Raw(gt, pred, nc, 3, d, dev, ws_short=1)
    assert r.status == -1 and r.outputs_untouched()
    assert Raw(gt, pred, nc, 3, 0, dev, over=dict(biou=None)).status == 0                   # no Boundary IoU counters asked for: biou may be NULL


def test_value_errors_come_before_anything_is_written(dev):
    from dupl_amd import ops
    gt, pred, nc, d, _ = blocky_case((TH + 1, TW + 1), 3)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    hist, biou = KG.Guard((4, nc, nc), dev, torch.int64), KG.Guard((3, nc), dev, torch.int64)
    ok = dict(num_classes=nc, max_dist=3, biou_dist=d, band_hist=hist.view, biou=biou.view)
    calls = [((g, p), dict(num_classes=0), "0"), ((g, p), dict(num_classes=256), "256"), ((g, p), dict(max_dist=0), "0"),
             ((g, p), dict(max_dist=65), "65"), ((g, p), dict(biou_dist=-1), "-1"), ((g, p), dict(biou_dist=65), "65"),
             ((g.int(), p), {}, "int32"), ((g, p.cpu()), {}, "cpu"), ((g, p[:, :-1]), {}, "64"), ((g[None], p[None]), {}, "gt"),
             ((g, p), dict(band_hist=torch.zeros((3, nc, nc), device=dev, dtype=torch.int64)), "band_hist"),
             ((g, p), dict(biou=torch.zeros((3, nc), device=dev, dtype=torch.int32)), "biou"),
             ((g, p), dict(max_dist=4), "band_hist")]
    for args, over, word in calls:
        with pytest.raises(ValueError, match=word):
            ops.seg_boundary(*args, **{**ok, **over})
    torch.cuda.synchronize()
    assert hist.untouched() and biou.untouched()
