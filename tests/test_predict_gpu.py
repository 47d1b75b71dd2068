"""Label-less inference on the GPU: dupl_seg_decide (csrc/seg_ens.hip), dupl_seg_paint / dupl_window_gather / dupl_window_merge
(csrc/seg_render.hip) at their edges, their ops.* wrappers, tools/predict.  Every input lives in a NaN-slack buffer, every output in
a sentinel-slack buffer (tests/kernel_guard.py; the uint8 outputs in tests/seg_render_ref.py's U8Guard, on an odd address).

  1. seg_decide's labels at min_conf 0 are the bits of the existing kernels: upsample_argmax / argmax_channels (one student),
     seg_ensemble's pred (two);
  2. conf is within 2 x the error of the composed fp32 path (ops.resize_bilinear -> torch.softmax -> mean -> max) + 1e-7 of float64;
  3. rejection and stats are exact against numpy on the returned conf; stats accumulate; every subset of the outputs gives the bits
     of the full call; two runs are bit-identical;
  4. is_prob on seg_ensemble's prob gives the bits of the two-student logits call;
  5. seg_paint, 6. window_gather, 7. window_merge are bit-equal to their references;
  8. bad arguments return -1 and touch nothing;
  9. msc_seg_logits_windowed against msc_seg_logits and against the assembled reference; the command line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_guard as KG
import seg_ensemble_ref as ER
import seg_render_ref as R

pytestmark = pytest.mark.gpu

IDS = ["x".join(map(str, s)) for s in R.SHAPES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Decide:
    """One raw dupl_seg_decide call on guarded buffers; outputs not in `want` are NULL."""

    def __init__(self, shape, dev, two, want=("conf", "label", "stats"), into=None, probs=None, **over):
        from dupl_amd import _lib, ops
        C, h, w, H, W = shape
        if probs is not None:
            ins = probs
        else:
            a, b, _, _ = ER.case(shape)
            ins = (a[0], b[0]) if two else (a[0],)
        self.ins = [KG.nan_in(t, dev) for t in ins]
        self.conf = KG.Guard((H, W), dev, torch.float32)
        self.label = R.U8Guard((H, W), dev)
        self.stats = into.stats if into is not None else KG.Guard((2, C + 1), dev, torch.int64, init=torch.zeros((2, C + 1), dtype=torch.int64))
        kw = dict(C=C, h=h, w=w, H=H, W=W, is_prob=int(probs is not None), ignore_index=255, min_conf=0.0,
                  a=self.ins[0].data_ptr(), b=self.ins[1].data_ptr() if len(self.ins) > 1 else None)
        for k in want:
            kw[k] = getattr(self, k).ptr
        kw.update(over)
        d = _lib.SegDecideDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        self.status = _lib.lib().dupl_seg_decide.raw(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()

    def outputs_untouched(self, but=()):
        return all(getattr(self, k).untouched() for k in ("conf", "label") if k not in but)


@pytest.fixture(scope="module")
def full(dev):
    """The call that asks for everything at min_conf 0, once per shape and student count."""
    return {(s, two): Decide(s, dev, two) for s in R.SHAPES for two in (False, True)}


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_labels_are_the_existing_kernels_bits(dev, full, shape):
    from dupl_amd import ops
    C, h, w, H, W = shape
    a, b, _, _ = ER.case(shape)
    one, two = full[(shape, False)], full[(shape, True)]
    assert one.status == 0 and two.status == 0
    t = a.to(dev)
    want1 = ops.argmax_channels(t)[0] if (h, w) == (H, W) else ops.upsample_argmax(t, H, W)[0]
    assert torch.equal(one.label.cpu().long(), want1.cpu())
    want2 = ops.seg_ensemble(a.to(dev), b.to(dev), (H, W), want_pred=True)[0]
    assert torch.equal(two.label.cpu().long(), want2.cpu())
    if H * W >= 100:
        assert float((want1 != want2).double().mean()) > 0.3          # the two calls do not answer the same question


@pytest.mark.parametrize("two", (False, True), ids=("one", "two"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_conf_holds_the_composed_paths_bar(dev, full, shape, two):
    from dupl_amd import ops
    C, h, w, H, W = shape
    a, b, _, _ = ER.case(shape)
    _, conf64, _ = R.decide_case(shape, two)
    conf64 = torch.from_numpy(conf64)
    p = torch.softmax(ops.resize_bilinear(a.to(dev), H, W), 1)
    if two:
        p = 0.5 * (p + torch.softmax(ops.resize_bilinear(b.to(dev), H, W), 1))
    comp = p[0].max(0).values
    err_comp = float((comp.cpu().double() - conf64).abs().max())
    conf = full[(shape, two)].conf.cpu()
    err = float((conf.double() - conf64).abs().max())
    print(f"{shape} {'two' if two else 'one'}: conf max-abs error {err:.3e}, composed fp32 path {err_comp:.3e} (bar {2 * err_comp + 1e-7:.3e})")
    assert bool(torch.isfinite(conf).all()) and float(conf.max()) <= 1.0 and float(conf.min()) > 0.0
    assert err <= 2.0 * err_comp + 1e-7


@pytest.mark.parametrize("two", (False, True), ids=("one", "two"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_rejection_stats_subsets_and_reproducibility(dev, full, shape, two):
    C, h, w, H, W = shape
    base = full[(shape, two)]
    winner, conf0 = base.label.cpu().numpy(), base.conf.cpu()
    c32 = conf0.numpy()
    st0 = R.stats_ref(winner, c32, np.zeros((H, W), dtype=bool), C)
    assert np.array_equal(base.stats.cpu().numpy(), st0) and int(st0[0, C]) == 0 and int(st0[0].sum()) == H * W
    for min_conf in (0.3, 0.6):
        ign = 255 if C > 200 else 201
        r = Decide(shape, dev, two, min_conf=min_conf, ignore_index=ign)
        assert r.status == 0
        assert KG.same_bits(r.conf.cpu(), conf0)
        lab, rej = R.labels_of(winner, c32, min_conf, ign)
        assert np.array_equal(r.label.cpu().numpy(), lab)
        want = R.stats_ref(winner, c32, rej, C)
        assert np.array_equal(r.stats.cpu().numpy(), want)
        print(f"{shape} {'two' if two else 'one'} min_conf {min_conf}: {int(rej.sum())} of {H * W} pixels rejected")
        # a second call into the same stats adds; the same bits again
        again = Decide(shape, dev, two, min_conf=min_conf, ignore_index=ign, into=r)
        assert again.status == 0 and np.array_equal(r.stats.cpu().numpy(), 2 * want)
        assert KG.same_bits(again.conf.cpu(), conf0) and torch.equal(again.label.cpu(), r.label.cpu())
        # every subset of the outputs: the bits of the full call, nothing else written
        for sub in (("conf",), ("label",), ("stats",), ("conf", "label"), ("label", "stats")):
            s = Decide(shape, dev, two, want=sub, min_conf=min_conf, ignore_index=ign)
            assert s.status == 0 and s.outputs_untouched(but=sub), sub
            if "conf" in sub:
                assert KG.same_bits(s.conf.cpu(), conf0)
            if "label" in sub:
                assert np.array_equal(s.label.cpu().numpy(), lab)
            assert np.array_equal(s.stats.cpu().numpy(), want if "stats" in sub else np.zeros_like(want)), sub
    if H * W >= 1000:
        assert int((c32 < 0.6).sum()) > 0                             # pixels were rejected (and at min_conf 0 above, none)


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[1:3] == s[3:5]], ids=lambda s: "x".join(map(str, s)))
def test_is_prob_on_the_ensembles_probabilities(dev, full, shape):
    from dupl_amd import ops
    C, h, w, H, W = shape
    a, b, _, _ = ER.case(shape)
    prob = ops.seg_ensemble(a.to(dev), b.to(dev), (H, W), want_prob=True)[1].cpu()
    two = full[(shape, True)]
    for probs in ((prob,), (prob, prob)):                             # the mean of a vector with itself is the vector
        r = Decide(shape, dev, False, probs=probs, min_conf=0.6)
        assert r.status == 0
        assert KG.same_bits(r.conf.cpu(), two.conf.cpu())
        lab, rej = R.labels_of(two.label.cpu().numpy(), two.conf.cpu().numpy(), 0.6, 255)
        assert np.array_equal(r.label.cpu().numpy(), lab)
        assert np.array_equal(r.stats.cpu().numpy(), R.stats_ref(two.label.cpu().numpy(), two.conf.cpu().numpy(), rej, C))
    # the mean of two different maps, against numpy in fp32
    q = torch.softmax(a[0], 0)
    r = Decide(shape, dev, False, probs=(prob, q))
    mean = (0.5 * (prob + q)).numpy()
    assert np.array_equal(r.conf.cpu().numpy(), mean.max(0)) and np.array_equal(r.label.cpu().numpy(), mean.argmax(0).astype(np.uint8))


class Paint:
    def __init__(self, size, dev, with_image=True, front=67, **over):
        H, W = size
        from dupl_amd import _lib, ops
        from dupl_amd.utils import imutils
        self.lab_np, self.img_np = R.paint_inputs(H, W)
        self.pal_np = imutils.colormap()
        self.label = R.U8Guard((H, W), dev, init=self.lab_np, front=5)
        self.image = R.U8Guard((H, W, 3), dev, init=self.img_np, front=3)
        self.palette = R.U8Guard((256, 3), dev, init=self.pal_np, front=1)
        self.out = R.U8Guard((H, W, 3), dev, front=front)
        kw = dict(H=H, W=W, alpha256=154, tint_background=0, contour=0, label=self.label.ptr, image=self.image.ptr if with_image else None,
                  palette=self.palette.ptr, out=self.out.ptr)
        kw.update(over)
        d = _lib.SegPaintDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        self.status = _lib.lib().dupl_seg_paint.raw(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", R.PAINT_SHAPES)
def test_paint_is_the_integer_reference(dev, H, W):
    from dupl_amd import ops
    n = 0
    for front in (64, 65, 66, 67):                                    # every alignment of the output's first byte
        r = Paint((H, W), dev, with_image=False, front=front)
        assert r.status == 0 and np.array_equal(r.out.cpu().numpy(), R.paint_ref(r.lab_np, r.pal_np))
    for alpha in R.PAINT_ALPHAS:
        for tint in (0, 1):
            for contour in (0, 1):
                r = Paint((H, W), dev, alpha256=alpha, tint_background=tint, contour=contour, contour_rgb=(ctypes.c_uint8 * 3)(250, 3, 77),
                          front=64 + (n % 4))
                n += 1
                want = R.paint_ref(r.lab_np, r.pal_np, r.img_np, alpha, bool(tint), bool(contour), (250, 3, 77))
                assert r.status == 0 and np.array_equal(r.out.cpu().numpy(), want), (alpha, tint, contour)
    r = Paint((H, W), dev, with_image=False, contour=1, contour_rgb=(ctypes.c_uint8 * 3)(9, 8, 7))
    assert np.array_equal(r.out.cpu().numpy(), R.paint_ref(r.lab_np, r.pal_np, None, 154, False, True, (9, 8, 7)))
    lab, img, pal = (torch.from_numpy(t).to(dev) for t in (r.lab_np, r.img_np, r.pal_np))
    got = ops.seg_paint(lab, pal, img, alpha256=128, contour=True, contour_rgb=(1, 2, 3))
    assert np.array_equal(got.cpu().numpy(), R.paint_ref(r.lab_np, r.pal_np, r.img_np, 128, False, True, (1, 2, 3)))
    with pytest.raises(ValueError):
        ops.seg_paint(lab, pal, img, alpha256=257)


def _gather_raw(x_dev, size, org, win, dev, **over):
    """one raw dupl_window_gather call: size = (Hs, Ws), win = (wh, ww); `over` replaces descriptor fields"""
    from dupl_amd import _lib, ops
    out = KG.Guard((2 * len(org), 3, win[0], win[1]), dev, torch.float32)
    tab = np.ascontiguousarray(np.asarray(org, dtype=np.int32).reshape(-1, 2))
    kw = dict(h=x_dev.shape[2], w=x_dev.shape[3], Hs=size[0], Ws=size[1], nW=len(org), wh=win[0], ww=win[1], x=x_dev.data_ptr(),
              origins=tab.ctypes.data, out=out.ptr)
    kw.update(over)
    d = _lib.WindowGatherDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    status = _lib.lib().dupl_window_gather.raw(ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    return status, out


@pytest.mark.parametrize("scale", (1.0, 1.5))
@pytest.mark.parametrize("window", (32, 48))
def test_window_gather_is_the_sliced_resize(dev, scale, window):
    from dupl_amd import ops
    h, w = 75, 100
    x = KG.nan_in(KG.rnd(1, 3, h, w, seed=21), dev)
    Hs, Ws = int(h * scale), int(w * scale)
    th, tw, wt = Hs // 16, Ws // 16, window // 16
    org = [(16 * r, 16 * c) for r, c in R.grid_origins(th, tw, wt, max(1, wt - 1))]
    assert org[-1] == (16 * (th - wt), 16 * (tw - wt)) and len(org) > 2       # the last aligned window
    org += [(Hs - window, Ws - window), (3, 5)]                                  # and windows off the token grid
    status, out = _gather_raw(x, (Hs, Ws), org, (window, window), dev)
    assert status == 0
    got = out.cpu()
    full = ops.resize_bilinear(x, Hs, Ws, flip_cat=True).cpu()
    for k, (r0, c0) in enumerate(org):
        for f in range(2):
            assert KG.same_bits(got[f * len(org) + k], full[f, :, r0:r0 + window, c0:c0 + window]), (k, f)
    assert bool(torch.isfinite(got).all())
    assert KG.same_bits(ops.window_gather(x, Hs, Ws, org, window, window).cpu(), got)
    with pytest.raises(ValueError):
        ops.window_gather(x, Hs, Ws, [(Hs - window + 1, 0)], window, window)


def _merge_raw(lg_dev, org, size, dev, **over):
    """one raw dupl_window_merge call onto a size = (hs, ws) canvas; `over` replaces descriptor fields"""
    from dupl_amd import _lib, ops
    C = lg_dev.shape[1]
    out = KG.Guard((2, C, size[0], size[1]), dev, torch.float32)
    tab = np.ascontiguousarray(np.asarray(org, dtype=np.int32).reshape(-1, 2))
    kw = dict(C=C, hs=size[0], ws=size[1], nW=len(org), wth=lg_dev.shape[2], wtw=lg_dev.shape[3], logits=lg_dev.data_ptr(), origins=tab.ctypes.data,
              canvas=out.ptr)
    kw.update(over)
    d = _lib.WindowMergeDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    status = _lib.lib().dupl_window_merge.raw(ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    return status, out


@pytest.mark.parametrize("case", R.MERGE_CASES, ids=lambda c: f"C{c[0]}-{c[1][0]}x{c[1][1]}-w{c[2]}s{c[3]}")
def test_window_merge_is_the_fixed_order_reference(dev, case):
    from dupl_amd import ops
    C, (hs, ws), win, stride = case
    lg, org = R.merge_inputs(C, hs, ws, win, stride)
    lg_dev = KG.nan_in(lg, dev)
    want = torch.from_numpy(R.merge_ref(lg.numpy(), org, hs, ws))
    status, out = _merge_raw(lg_dev, org, (hs, ws), dev)
    assert status == 0 and KG.same_bits(out.cpu(), want)
    status, again = _merge_raw(lg_dev, org, (hs, ws), dev)
    assert KG.same_bits(again.cpu(), out.cpu())
    assert KG.same_bits(ops.window_merge(lg_dev, org, hs, ws).cpu(), want)


def test_bad_arguments_are_refused_and_launch_nothing(dev):
    from dupl_amd import _lib, ops
    shape = R.SHAPES[1]
    size = ctypes.sizeof(_lib.SegDecideDesc)
    for kw in (dict(struct_size=size - 8), dict(struct_size=size + 8), dict(struct_size=0), dict(C=0), dict(C=256), dict(C=-1), dict(h=0),
               dict(W=0), dict(H=-2), dict(a=None), dict(ignore_index=256), dict(ignore_index=-1), dict(is_prob=1)):   # is_prob: h != H
        r = Decide(shape, dev, True, **kw)
        assert r.status == -1 and r.outputs_untouched() and not bool(r.stats.cpu().any()), kw
    r = Decide(shape, dev, True, want=())                                        # all outputs NULL
    assert r.status == -1 and r.outputs_untouched()
    assert Decide(shape, dev, True).status == 0
    with pytest.raises(ValueError):
        ops.seg_decide(ER.case(shape)[0].to(dev), want_label=False, want_conf=False)
    with pytest.raises(ValueError):
        ops.seg_decide(ER.case(shape)[0].to(dev), size=(37, 53), is_prob=True)
    psize = ctypes.sizeof(_lib.SegPaintDesc)
    for kw in (dict(struct_size=psize + 8), dict(struct_size=0), dict(alpha256=257), dict(alpha256=-1), dict(H=0), dict(W=-1), dict(label=None),
               dict(palette=None), dict(out=None), dict(contour=2), dict(tint_background=2)):
        r = Paint((5, 3), dev, **kw)
        assert r.status == -1, kw
        if "out" not in kw:
            assert r.out.untouched(), kw
    assert Paint((5, 3), dev).status == 0
    x = KG.nan_in(KG.rnd(1, 3, 40, 50, seed=2), dev)
    gsize = ctypes.sizeof(_lib.WindowGatherDesc)
    for kw, org in ((dict(), [(0, 0), (9, 19)]), (dict(), [(0, 0), (8, 20)]), (dict(), [(-1, 0)]), (dict(), [(0, -16)]),
                    (dict(struct_size=gsize - 4), [(0, 0)]), (dict(nW=0), [(0, 0)]), (dict(nW=_lib.WINDOW_MAX + 1), [(0, 0)]), (dict(wh=0), [(0, 0)]),
                    (dict(x=None), [(0, 0)]), (dict(origins=None), [(0, 0)]), (dict(Hs=0), [(0, 0)])):
        status, out = _gather_raw(x, (40, 50), org, (32, 32), dev, **kw)             # a 32 x 32 window must start at or before (8, 18)
        assert status == -1 and out.untouched(), (kw, org)
    assert _gather_raw(x, (40, 50), [(8, 18)], (32, 32), dev)[0] == 0
    lg = KG.nan_in(KG.rnd(4, 5, 2, 2, seed=1), dev)
    msize = ctypes.sizeof(_lib.WindowMergeDesc)
    for kw, org in ((dict(), [(0, 0), (3, 4)]), (dict(), [(0, 0), (2, 5)]), (dict(), [(0, 0), (0, -1)]), (dict(struct_size=msize + 4), [(0, 0), (1, 1)]),
                    (dict(C=0), [(0, 0), (1, 1)]), (dict(nW=0), [(0, 0), (1, 1)]), (dict(logits=None), [(0, 0), (1, 1)]), (dict(hs=0), [(0, 0), (1, 1)])):
        status, out = _merge_raw(lg, org, (4, 6), dev, **kw)
        assert status == -1 and out.untouched(), (kw, org)
    assert _merge_raw(lg, [(0, 0), (2, 4)], (4, 6), dev)[0] == 0


# ------------------------------------------------------------------------------------------------------------- the model level
@pytest.fixture(scope="module")
def tiny(dev):
    from test_eval_gpu import _tiny_model
    model, _ = _tiny_model(dev)
    model.eval()
    return model


def test_windows_at_or_above_the_image_are_msc_seg_logits(dev, tiny):
    from dupl_amd.tools import eval_seg, predict
    x = KG.rnd(1, 3, 75, 100, seed=31).to(dev)
    scales = (1.0, 1.5, 1.25)
    want = eval_seg.msc_seg_logits(tiny, x, (75, 100), scales)
    for window, stride in ((160, 160), (160, 96), (1024, 16)):                   # 100 * 1.5 = 150 pixels: 9 tokens <= 10
        got = predict.msc_seg_logits_windowed(tiny, x, (75, 100), scales, window, stride, window_batch=3)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert predict.windows_per_scale(75, 100, scales, window, stride) == [1, 1, 1]
    with pytest.raises(ValueError):
        predict.msc_seg_logits_windowed(tiny, x, (75, 100), scales, 100, 64)
    with pytest.raises(ValueError):
        predict.msc_seg_logits_windowed(tiny, x, (75, 100), scales, 64, 80)


def test_windowed_inference_is_the_assembled_reference(dev, tiny):
    """Gather, chunking, merge and glue: the same chunks of resize_bilinear(flip_cat) slices through the model, merged by the numpy
    reference, then msc_seg_accum_.  (Not asserted: that a window's logits do not depend on which windows share its batch.)"""
    from dupl_amd import ops
    from dupl_amd.tools import predict
    h, w, window, stride, wb = 160, 208, 64, 48, 4
    x = KG.rnd(1, 3, h, w, seed=32).to(dev)
    scales = (1.0, 1.5)
    got = predict.msc_seg_logits_windowed(tiny, x, (h, w), scales, window, stride, window_batch=wb)
    accs = [torch.empty((1, 21, h, w), device=dev) for _ in range(2)]
    with torch.no_grad():
        for i, sc in enumerate(scales):
            Hs, Ws = int(h * sc), int(w * sc)
            th, tw, wt = Hs // 16, Ws // 16, window // 16
            org = R.grid_origins(th, tw, wt, stride // 16)
            assert len(org) == predict.windows_per_scale(h, w, scales, window, stride)[i] > wb
            full = ops.resize_bilinear(x, Hs, Ws, flip_cat=True)
            batch = torch.stack([full[f, :, 16 * r:16 * r + window, 16 * c:16 * c + window] for f in range(2) for r, c in org]).contiguous()
            outs = [[], []]
            for j in range(0, batch.shape[0], wb):
                res = tiny(batch[j:j + wb].contiguous())
                for k, name in enumerate(("branch1", "branch2")):
                    outs[k].append(res[name][1].cpu())
            for k in range(2):
                canvas = torch.from_numpy(R.merge_ref(torch.cat(outs[k]).numpy(), org, th, tw)).to(dev)
                ops.msc_seg_accum_(accs[k], canvas, mode=(0 if i == 0 else 1))
    assert got[0].shape == (1, 21, h, w)
    assert torch.equal(got[0], accs[0]) and torch.equal(got[1], accs[1])
    assert bool(torch.isfinite(got[0]).all()) and not torch.equal(got[0], got[1])


def test_predict_command_line(dev, tiny, tmp_path):
    """`python -m dupl_amd.tools.predict` on a folder of four JPEGs of different sizes, one larger than the window, from a
    `module.`-prefixed checkpoint: index PNGs of the images' sizes, a summary that agrees with them, and a second run (in this
    process) that writes the same files; --branch ens --crf 1 --min_conf 0.9 on the smallest image."""
    from PIL import Image
    from dupl_amd.tools import predict
    imgs = tmp_path / "photos"
    imgs.mkdir()
    sizes = {"a": (48, 64), "b": (75, 100), "c": (96, 64), "d": (160, 208)}
    g = np.random.RandomState(5)
    for nm, (H, W) in sizes.items():
        base = g.randint(0, 256, size=((H + 15) // 16, (W + 15) // 16, 3)).astype(np.uint8).repeat(16, 0).repeat(16, 1)[:H, :W]
        Image.fromarray(base).save(imgs / (nm + ".jpg"), quality=95)
    ckpt = str(tmp_path / "checkpoint.pth")
    torch.save({"module." + k: v.detach().cpu() for k, v in tiny.state_dict().items()}, ckpt)
    common = ["--model_path", ckpt, "--backbone", "tiny_test", "--num_classes", "21", "--input", str(imgs), "--scales", "1.0,1.5",
              "--window", "64", "--stride", "48", "--window_batch", "4", "--save_conf", "1", "--branch", "1"]
    r = subprocess.run([sys.executable, "-m", "dupl_amd.tools.predict"] + common + ["--out_dir", str(tmp_path / "o1")], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines[-5:-1]] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"] and "images/s" in lines[-1]
    predict.main(common + ["--out_dir", str(tmp_path / "o2")])
    summ = json.load(open(tmp_path / "o1" / "summary.json"))
    assert [e["image"] for e in summ["images"]] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"]
    for e in summ["images"]:
        H, W = sizes[e["image"][0]]
        png = Image.open(tmp_path / "o1" / "labels" / (e["image"][0] + ".png"))
        lab = np.array(png)
        assert png.mode == "P" and lab.shape == (H, W) and e["size"] == [H, W]
        assert bool(((lab < 21) | (lab == 255)).all())
        assert png.getpalette()[:9] == [0, 0, 0, 128, 0, 0, 0, 128, 0]
        assert sum(c["pixels"] for c in e["classes"]) + e["rejected_pixels"] == H * W
        for c in e["classes"]:
            assert c["pixels"] == int((lab == c["id"]).sum()) and c["name"] == predict.class_names("voc")[c["id"]]
            assert 1.0 / 21 <= c["mean_conf"] <= 1.0 and abs(c["share"] - c["pixels"] / (H * W)) < 1e-12
        assert e["rejected_pixels"] == int((lab == 255).sum()) == 0
        assert e["windows_per_scale"] == predict.windows_per_scale(H, W, (1.0, 1.5), 64, 48)
        ov = np.array(Image.open(tmp_path / "o1" / "overlay" / (e["image"][0] + ".png")))
        cf = np.array(Image.open(tmp_path / "o1" / "conf" / (e["image"][0] + ".png")))
        assert ov.shape == (H, W, 3) and cf.shape == (H, W) and cf.dtype == np.uint8 and int(cf.min()) >= 255 // 21
    assert summ["images"][3]["windows_per_scale"] == [12, 30] and summ["images"][0]["windows_per_scale"] == [1, 2]
    for sub in ("labels", "overlay", "conf"):
        for nm in sizes:
            assert (tmp_path / "o1" / sub / (nm + ".png")).read_bytes() == (tmp_path / "o2" / sub / (nm + ".png")).read_bytes(), (sub, nm)
    assert (tmp_path / "o1" / "summary.json").read_bytes() == (tmp_path / "o2" / "summary.json").read_bytes()
    # the ensemble through DenseCRF with rejection, on the smallest image, whole-image route
    out = predict.main(["--model_path", ckpt, "--backbone", "tiny_test", "--input", str(imgs / "a.jpg"), "--out_dir", str(tmp_path / "o3"),
                        "--branch", "ens", "--crf", "1", "--min_conf", "0.9", "--contour", "1"])
    lab = np.array(Image.open(tmp_path / "o3" / "labels" / "a.png"))
    assert lab.shape == (48, 64) and bool(((lab < 21) | (lab == 255)).all())
    assert out[0]["rejected_pixels"] == int((lab == 255).sum()) and out[0]["windows_per_scale"] == [1, 1, 1]
    assert sum(c["pixels"] for c in out[0]["classes"]) + out[0]["rejected_pixels"] == 48 * 64
    assert all(c["mean_conf"] >= 0.9 for c in out[0]["classes"])
