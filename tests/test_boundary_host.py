"""Boundary scores, the host side (no GPU): tests/boundary_ref.py's filter / erosion formulation against the brute-force definition,
evaluate.BoundaryMatrix's arithmetic on hand-written counters, evaluate.biou_dist, eval_seg's new flags, and the library's exports."""
import ctypes

import numpy as np
import pytest
import torch

import boundary_ref as BR


def _maps(H, W, nc, seed):
    rng = np.random.default_rng(seed)
    gt = np.kron(rng.integers(0, nc, ((H + 2) // 3, (W + 2) // 3)), np.ones((3, 3), dtype=np.int64))[:H, :W]
    pred = np.kron(rng.integers(0, nc, ((H + 3) // 4, (W + 3) // 4)), np.ones((4, 4), dtype=np.int64))[:H, :W]
    gt = np.where(rng.random((H, W)) < 0.03, 255, gt)
    return gt, pred


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (9, 11)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_is_the_brute_force_definition(shape):
    for seed, (R, d) in enumerate([(1, 1), (2, 3), (3, 2), (8, 1), (64, 64)]):
        gt, pred = _maps(shape[0], shape[1], 4, seed)
        hist, cnt, dg, dp = BR.brute(gt, pred, 4, R, d)
        ref = BR.reference(gt, pred, 4, R, d)
        assert np.array_equal(ref[0], hist) and np.array_equal(ref[1], cnt)
        assert np.array_equal(ref[2], dg) and np.array_equal(ref[3], dp)
        assert ref[0].sum() == ((gt < 4) & (pred < 4)).sum()


def test_reference_on_maps_read_off_by_hand():
    # one row, labels 0 0 0 1 1: distances to the label change 3 2 1 1 2
    gt = np.array([[0, 0, 0, 1, 1]])
    assert BR.dist_map(gt, 2).tolist() == [[3, 2, 1, 1, 2]]
    h = BR.band_hist(gt, gt, 2, 2)
    assert h[:, 0, 0].tolist() == [1, 1, 1] and h[:, 1, 1].tolist() == [1, 1, 0] and h.sum() == 5
    # the border counts for the Boundary IoU band: at d = 1 every pixel of a one-row map is in its class's band
    assert BR.biou_counts(gt, gt, 2, 1).tolist() == [[3, 2], [3, 2], [3, 2]]
    # a uniform 5 x 7 map: nothing within R, the band at d = 1 is the frame
    uni = np.zeros((5, 7), dtype=np.int64)
    assert (BR.dist_map(uni, 3) == 4).all() and BR.biou_counts(uni, uni, 1, 1).tolist() == [[20], [20], [20]]
    # an ignored pixel is a label like any other to its neighbours, and is not counted itself
    gt = np.array([[0, 0, 255, 0, 0]])
    assert BR.dist_map(gt, 2).tolist() == [[2, 1, 1, 1, 2]] and BR.band_hist(gt, np.zeros_like(gt), 1, 2)[:, 0, 0].tolist() == [2, 2, 0]


def test_biou_dist():
    from dupl_amd.utils import evaluate
    for fn in (evaluate.biou_dist, BR.biou_dist):
        assert fn(375, 500) == 13 and fn(480, 640) == 16 and fn(1, 1) == 1
        assert fn(100, 75) == 3 and fn(4000, 4000) == 64                        # 2.5 rounds up; clipped to the kernel's maximum


def test_boundary_matrix_arithmetic():
    from dupl_amd.utils import evaluate
    bm = evaluate.BoundaryMatrix(3, "cpu", max_dist=2)
    assert bm.hist.shape == (3, 3, 3) and bm.biou.shape == (3, 3) and bm.hist.dtype == torch.int64 and bm.biou.dtype == torch.int64
    assert np.isnan(bm.boundary_iou()["biou"])
    hist = np.zeros((3, 3, 3), dtype=np.int64)
    hist[0] = [[2, 2, 0], [0, 4, 0], [0, 0, 0]]                                 # at the label change: class 0 half right, class 1 right
    hist[1] = [[6, 0, 0], [2, 2, 0], [0, 0, 0]]
    hist[2] = [[50, 0, 0], [0, 40, 0], [0, 0, 0]]                               # farther than 2: all right
    bm.hist.copy_(torch.from_numpy(hist))
    tri = bm.trimap_scores([1, 2])
    assert sorted(tri) == [1, 2]
    # width 1: IoU 2 / 4 and 4 / 6, class 2 absent from the ground truth and left out of the mean
    assert tri[1]["miou"] == pytest.approx((2 / 4 + 4 / 6) / 2) and tri[1]["pAcc"] == pytest.approx(6 / 8)
    # width 2 is cumulative: bins 0 and 1 together
    assert tri[2]["miou"] == pytest.approx((8 / 12 + 6 / 10) / 2) and tri[2]["pAcc"] == pytest.approx(14 / 18)
    full = bm.scores()
    assert full["miou"] == pytest.approx((58 / 62 + 46 / 50) / 2) == evaluate.scores_from_hist(hist.sum(0))["miou"]
    with pytest.raises(ValueError, match="3"):
        bm.trimap_scores([3])
    with pytest.raises(ValueError, match="0"):
        bm.trimap_scores([0])
    # I, G, P: class 0 -> 3 / (4 + 5 - 3), class 1 has no ground-truth boundary (G = 0) but predictions: out of the mean; class 2 -> 0 / 3
    bm.biou.copy_(torch.tensor([[3, 0, 0], [4, 0, 2], [5, 7, 1]]))
    b = bm.boundary_iou()
    assert b["iou"][0] == pytest.approx(0.5) and b["iou"][1] == 0.0 and b["iou"][2] == 0.0
    assert b["biou"] == pytest.approx((0.5 + 0.0) / 2)
    with pytest.raises(ValueError, match="65"):
        evaluate.BoundaryMatrix(3, "cpu", max_dist=65)


def test_eval_seg_flags():
    from dupl_amd.tools import eval_seg
    for ds in ("voc", "coco"):
        p = eval_seg.build_parser(ds)
        a = p.parse_args([])
        assert a.boundary == 0 and a.trimap_widths == (1, 2, 4, 8, 16, 32) and a.crf_method is None
        a = p.parse_args(["--boundary", "1", "--trimap_widths", "3,64", "--crf_method", "lattice"])
        assert a.boundary == 1 and a.trimap_widths == (3, 64) and a.crf_method == "lattice"
        for bad in (["--trimap_widths", "0"], ["--trimap_widths", "65"], ["--trimap_widths", "4,2"], ["--trimap_widths", "2,2"],
                    ["--trimap_widths", "x"], ["--boundary", "2"], ["--crf_method", "pydensecrf"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)


def test_format_boundary_and_scores_dict():
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    bm = evaluate.BoundaryMatrix(2, "cpu", max_dist=4)
    bm.hist[0, 0, 0], bm.hist[0, 1, 0], bm.hist[3, 1, 1] = 3, 1, 5
    bm.biou.copy_(torch.tensor([[1, 2], [2, 2], [1, 4]]))
    s = eval_seg.boundary_scores(bm, (1, 4))
    assert sorted(s) == ["biou", "biou_iou", "trimap"] and sorted(s["trimap"]) == [1, 4] and sorted(s["trimap"][1]) == ["miou", "pAcc"]
    assert s["biou"] == pytest.approx((0.5 + 0.5) / 2) and s["trimap"][1]["pAcc"] == pytest.approx(0.75)
    line = eval_seg.format_boundary([{"boundary": s}], ["Seg_1"])
    assert line.startswith("boundary Seg_1: BIoU 50.000 | trimap mIoU @1 ") and " @4 " in line and "\n" not in line


def test_library_exports_the_boundary_entry_points():
    from dupl_amd import _lib
    L = _lib.lib()
    assert L.dupl_abi_version() == 4                                           # the exports are additive
    assert "dupl_seg_boundary" in L.protos and hasattr(L.cdll, "dupl_seg_boundary_workspace")
    d = _lib.SegBoundaryDesc(H=375, W=500, num_classes=21, max_dist=32, biou_dist=13)
    assert d.struct_size == ctypes.sizeof(_lib.SegBoundaryDesc) == 88
    n = L.dupl_seg_boundary_workspace(ctypes.byref(d))
    assert 6 * 375 * 500 <= n < 6 * 375 * 500 + 4 * 256 and n % 256 == 0
    for over in (dict(H=0), dict(max_dist=65), dict(biou_dist=-1), dict(num_classes=256), dict(struct_size=4)):
        bad = _lib.SegBoundaryDesc(H=375, W=500, num_classes=21, max_dist=32, biou_dist=13)
        for k, v in over.items():
            setattr(bad, k, v)
        assert L.dupl_seg_boundary_workspace(ctypes.byref(bad)) <= 0
        assert L.dupl_seg_boundary.raw(ctypes.byref(bad), None) == -1          # refused before any launch: no GPU is needed to ask
