"""The two-student ensemble on the GPU: dupl_seg_ensemble (csrc/seg_ens.hip) at its edges, ops.seg_ensemble, evaluate.EnsembleMatrix
and eval_seg --ensemble / --crf_branch.  The inputs live inside guarded buffers (tests/kernel_guard.py): NaN slack around what the
kernel reads, sentinel slack around what it writes.  The float64 reference is tests/seg_ensemble_ref.py (pinned against torch in
tests/test_seg_ensemble_host.py).

  1. the students' rows of the histogram and the agreement counters are bit-equal to the existing kernels (upsample_argmax /
     argmax_channels -> ConfusionMatrix);
  2. the ensemble's row and pred match float64 on every pixel whose float64 top-2 margin of e is >= 1e-5; the excused pixels (set to
     255 in gt on both sides) are at most 0.2 % per shape -- the reference alone gives 0, 0, 0, 3 of 12 707, 0, 2 of 16 448, 0, 0;
  3. prob is within 2 x the error of the composed fp32 path (ops.resize_bilinear -> torch.softmax -> mean) + 1e-7 of the float64 e;
  4. hist / counts accumulate, every subset of the outputs gives the bits of the full call, two runs are bit-identical;
  5. bad arguments return -1 and touch nothing;
  6. the command line: --ensemble 1, --crf_branch ens, and validate_coco(..., ensemble=True) on low-resolution logits."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import kernel_guard as KG
import seg_ensemble_ref as R

pytestmark = pytest.mark.gpu

IDS = ["x".join(map(str, s)) for s in R.SHAPES]


def _masked_gt(shape):
    """gt of the case with the proven ties of the float64 ensemble set to 255 (on both sides of every comparison)."""
    _, _, gt, ref = R.case(shape)
    tie = torch.from_numpy(ref["margin"] < R.MARGIN)
    g = gt.clone()
    g[tie] = 255
    return g, tie


class Call:
    """One raw dupl_seg_ensemble call on guarded buffers; outputs not in `want` are NULL."""

    def __init__(self, shape, dev, gt=None, want=("hist", "counts", "pred", "prob"), into=None, **over):
        from dupl_amd import _lib, ops
        C, h, w, H, W = shape
        a, b, _, _ = R.case(shape)
        self.a, self.b = KG.nan_in(a[0], dev), KG.nan_in(b[0], dev)
        self.gt = KG.Guard((H, W), dev, torch.int64, init=gt) if gt is not None else None
        if into is not None:
            self.hist, self.counts = into.hist, into.counts
        else:
            self.hist = KG.Guard((3, C, C), dev, torch.int64, init=torch.zeros((3, C, C), dtype=torch.int64))
            self.counts = KG.Guard((2,), dev, torch.int64, init=torch.zeros(2, dtype=torch.int64))
        self.pred = KG.Guard((H, W), dev, torch.int64)
        self.prob = KG.Guard((C, H, W), dev, torch.float32)
        kw = dict(C=C, h=h, w=w, H=H, W=W, a=self.a.data_ptr(), b=self.b.data_ptr(),
                  gt=self.gt.ptr if self.gt is not None else None)
        for k in want:
            kw[k] = getattr(self, k).ptr
        kw.update(over)
        d = _lib.SegEnsembleDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        self.status = _lib.lib().dupl_seg_ensemble.raw(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()

    def outputs_untouched(self, but=()):
        return all(getattr(self, k).untouched() for k in ("pred", "prob") if k not in but)


@pytest.fixture(scope="module")
def full(dev):
    """The call that asks for everything, once per shape, on the tie-masked gt."""
    return {s: Call(s, dev, gt=_masked_gt(s)[0]) for s in R.SHAPES}


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_student_rows_and_counts_are_the_existing_kernels(dev, full, shape):
    from dupl_amd import ops
    from dupl_amd.utils import evaluate
    C, h, w, H, W = shape
    a, b, _, _ = R.case(shape)
    gt = _masked_gt(shape)[0].to(dev)
    r = full[shape]
    assert r.status == 0
    hist, counts = r.hist.cpu(), r.counts.cpu()
    preds = []
    for k, t in enumerate((a, b)):
        t = t.to(dev)
        p = ops.argmax_channels(t)[0] if (h, w) == (H, W) else ops.upsample_argmax(t, H, W)[0]
        cm = evaluate.ConfusionMatrix(C, dev)
        cm.update(gt, p)
        assert torch.equal(hist[k], cm.hist.cpu()), f"student {k + 1}"
        preds.append(p)
    valid = (gt >= 0) & (gt < C)
    want = [int(valid.sum()), int((valid & (preds[0] == preds[1])).sum())]
    assert counts.tolist() == want and want[0] > 0
    assert int(hist[0].sum()) == want[0] and int(hist[1].sum()) == want[0] and int(hist[2].sum()) == want[0]


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_ensemble_row_and_pred_match_float64_off_the_ties(dev, full, shape):
    from dupl_amd.utils import evaluate
    C, h, w, H, W = shape
    _, _, _, ref = R.case(shape)
    gt, tie = _masked_gt(shape)
    share = float(tie.double().mean())
    print(f"{shape}: {int(tie.sum())} of {H * W} pixels excused (float64 top-2 margin of e < {R.MARGIN}): {100 * share:.3f} %")
    assert share <= R.TIE_SHARE
    r = full[shape]
    pred = r.pred.cpu()
    want = torch.from_numpy(ref["pred"])
    differ = pred != want
    print(f"{shape}: {int(differ.sum())} ensemble predictions differ from float64, {int((differ & ~tie).sum())} of them off the ties")
    assert not bool((differ & ~tie).any())
    assert np.array_equal(r.hist.cpu()[2].numpy(), evaluate._fast_hist(gt.numpy().flatten(), ref["pred"].flatten(), C))
    if H * W >= 100:                  # the ensemble is not a student: a kernel that returned one could not get here
        for k in ("pred1", "pred2"):
            assert float((pred != torch.from_numpy(ref[k])).double().mean()) > 0.3


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_prob_holds_the_composed_paths_bar(dev, full, shape):
    from dupl_amd import ops
    C, h, w, H, W = shape
    a, b, _, ref = R.case(shape)
    e64 = torch.from_numpy(ref["e"])
    comp = 0.5 * (torch.softmax(ops.resize_bilinear(a.to(dev), H, W), 1) + torch.softmax(ops.resize_bilinear(b.to(dev), H, W), 1))[0]
    err_comp = float((comp.cpu().double() - e64).abs().max())
    prob = full[shape].prob.cpu()
    err = float((prob.double() - e64).abs().max())
    sums = float((prob.double().sum(0) - 1.0).abs().max())
    print(f"{shape}: prob max-abs error {err:.3e}, composed fp32 path {err_comp:.3e} (bar {2 * err_comp + 1e-7:.3e}); "
          f"channel sums off 1 by {sums:.2e}")
    assert bool(torch.isfinite(prob).all())
    assert err <= 2.0 * err_comp + 1e-7
    assert sums <= 1e-6


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_accumulation_optional_outputs_and_reproducibility(dev, full, shape):
    C, h, w, H, W = shape
    gt = _masked_gt(shape)[0]
    gt2 = torch.roll(gt, shifts=(1, 2), dims=(0, 1))
    r = full[shape]
    h0, c0, p0, q0 = r.hist.cpu(), r.counts.cpu(), r.pred.cpu(), r.prob.cpu()
    # two calls into the same hist / counts = the sum of two single calls
    one = Call(shape, dev, gt=gt2)
    two = Call(shape, dev, gt=gt)
    again = Call(shape, dev, gt=gt2, into=two)
    assert one.status == 0 and two.status == 0 and again.status == 0
    assert torch.equal(two.hist.cpu(), h0 + one.hist.cpu()) and torch.equal(two.counts.cpu(), c0 + one.counts.cpu())
    # two runs of the same call: the same bits
    assert KG.same_bits(one.pred.cpu(), again.pred.cpu()) and KG.same_bits(one.prob.cpu(), again.prob.cpu())
    assert KG.same_bits(two.pred.cpu(), p0) and KG.same_bits(two.prob.cpu(), q0)
    # every subset of the outputs: the bits of the full call, nothing else written
    for want in (("pred",), ("prob",), ("hist",), ("counts",), ("hist", "counts")):
        s = Call(shape, dev, gt=gt if ("hist" in want or "counts" in want) else None, want=want)
        assert s.status == 0, want
        assert s.outputs_untouched(but=want), want
        if "pred" in want:
            assert KG.same_bits(s.pred.cpu(), p0)
        if "prob" in want:
            assert KG.same_bits(s.prob.cpu(), q0)
        assert torch.equal(s.hist.cpu(), h0 if "hist" in want else torch.zeros_like(h0)), want
        assert torch.equal(s.counts.cpu(), c0 if "counts" in want else torch.zeros_like(c0)), want


def test_bad_arguments_are_refused_and_launch_nothing(dev):
    from dupl_amd import _lib
    shape = R.SHAPES[1]
    gt = R.case(shape)[2]
    size = ctypes.sizeof(_lib.SegEnsembleDesc)
    bad = [dict(struct_size=size - 8), dict(struct_size=size + 8), dict(struct_size=0), dict(C=0), dict(C=256), dict(C=-1),
           dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(h=-3), dict(W=-1), dict(a=None), dict(b=None)]
    for kw in bad:
        r = Call(shape, dev, gt=gt, **kw)
        assert r.status == -1, kw
        assert r.outputs_untouched() and not bool(r.hist.cpu().any()) and not bool(r.counts.cpu().any()), kw
    for want in (("hist",), ("counts",), ("hist", "counts", "pred", "prob")):       # hist or counts without gt
        r = Call(shape, dev, gt=None, want=want)
        assert r.status == -1 and r.outputs_untouched() and not bool(r.hist.cpu().any()) and not bool(r.counts.cpu().any()), want
    r = Call(shape, dev, gt=gt, want=())                                             # nothing asked for
    assert r.status == -1 and r.outputs_untouched()
    assert Call(shape, dev, gt=gt).status == 0


def test_python_wrappers(dev):
    """ops.seg_ensemble and evaluate.EnsembleMatrix are the raw call; what they cannot serve raises."""
    from dupl_amd import ops
    from dupl_amd.utils import evaluate
    shape = R.SHAPES[1]
    C, h, w, H, W = shape
    a, b, _, _ = R.case(shape)
    gt = _masked_gt(shape)[0].to(dev)
    r = Call(shape, dev, gt=gt.cpu())
    em = evaluate.EnsembleMatrix(C, dev)
    assert em.hist.shape == (3, C, C) and em.counts.shape == (2,) and np.isnan(em.agreement())
    em.update(a.to(dev), b.to(dev), gt[None])
    em.update(a.to(dev), b.to(dev), gt[None])
    assert torch.equal(em.hist.cpu(), 2 * r.hist.cpu()) and torch.equal(em.counts.cpu(), 2 * r.counts.cpu())
    sc = em.scores()
    assert len(sc) == 3 and all(0.0 <= s["miou"] <= 1.0 for s in sc)
    for k in range(3):
        assert sc[k]["miou"] == evaluate.scores_from_hist(r.hist.cpu()[k].numpy())["miou"]
    assert em.agreement() == int(r.counts.cpu()[1]) / int(r.counts.cpu()[0])
    pred, prob = ops.seg_ensemble(a.to(dev), b.to(dev), (H, W), want_pred=True, want_prob=True)
    assert KG.same_bits(pred.cpu(), r.pred.cpu()) and KG.same_bits(prob.cpu(), r.prob.cpu())
    assert ops.seg_ensemble(a[0].to(dev), b[0].to(dev), (H, W), want_pred=True)[1] is None
    with pytest.raises(ValueError):
        ops.seg_ensemble(a.to(dev), b.to(dev), (H, W))
    with pytest.raises(AssertionError):
        ops.seg_ensemble(a.to(dev), b.to(dev), (H, W), hist=em.hist)


def test_eval_seg_cli_ensemble_and_crf_on_it(dev, tmp_path):
    """`python -m dupl_amd.tools.eval_seg --ensemble 1 --crf 1 --crf_branch ens`: the students' scores are the plain run's, the
    ensemble's score and the agreement are those of predictions recomputed here from the saved per-student logits, and every PNG is
    the argmax of DenseCRF(10, 1, 1, 4, 121, 5) on the ensemble's probabilities of those logits."""
    from PIL import Image
    from dupl_amd import ops
    from dupl_amd.utils import evaluate, imutils
    from dupl_amd.utils.dcrf import DenseCRF
    from test_crf_gpu import _run_cli, _voc_folder
    root, names, argv = _voc_folder(tmp_path, dev)
    out0, plain = _run_cli(argv)
    assert sorted(plain) == ["Seg_1 mIoU", "Seg_2 mIoU", "next"] and "Seg_ens" not in out0
    out1, last = _run_cli(argv + ["--ensemble", "1", "--crf", "1", "--crf_branch", "ens"])
    assert sorted(last) == ["Seg_1 mIoU", "Seg_2 mIoU", "Seg_ens mIoU", "agree", "seg_crf mIoU"]
    assert last["Seg_1 mIoU"] == plain["Seg_1 mIoU"] and last["Seg_2 mIoU"] == plain["Seg_2 mIoU"]
    head = out1[:out1.index("crf post-processing...")]
    assert "Seg_1" in head and "Seg_2" in head and "Seg_ens" in head and "aeroplane" in head
    logits = tmp_path / "run" / "segs" / "logits" / "val"
    assert sorted(p.name for p in logits.iterdir()) == ["branch1", "branch2"]            # no new files for the ensemble
    post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=1, bi_xy_std=121, bi_rgb_std=5, bi_w=4)
    gts, preds, crfs, n_valid, n_agree = [], [], [], 0, 0
    for nm in names:
        z = [torch.from_numpy(np.load(logits / b / (nm + ".npy"), allow_pickle=True).item()["msc_seg"]).to(dev)
             for b in ("branch1", "branch2")]
        gt = np.array(Image.open(root / "SegmentationClassAug" / (nm + ".png")))
        image = np.array(Image.open(root / "JPEGImages" / (nm + ".jpg")).convert("RGB"))
        H, W, _ = image.shape
        assert gt.shape == (H, W)
        pred, prob = ops.seg_ensemble(z[0], z[1], (H, W), want_pred=True, want_prob=True)
        gts.append(gt)
        preds.append(pred.cpu().numpy())
        p1, p2 = z[0].argmax(1)[0].cpu().numpy(), z[1].argmax(1)[0].cpu().numpy()
        n_valid += int((gt < 21).sum())
        n_agree += int(((gt < 21) & (p1 == p2)).sum())
        want = post(torch.from_numpy(image).to(dev), prob).argmax(0).cpu().numpy()
        png = np.array(Image.open(tmp_path / "run" / "segs" / "seg_preds" / "val" / (nm + ".png")))
        rgb = np.array(Image.open(tmp_path / "run" / "segs" / "seg_preds_rgb" / "val" / (nm + ".png")))
        assert png.shape == (H, W) and png.dtype == np.uint8 and np.array_equal(png, want)
        assert np.array_equal(rgb, imutils.encode_cmap(png))
        crfs.append(png)
    assert last["Seg_ens mIoU"] == evaluate.scores(gts, preds)["miou"] and 0.0 <= last["Seg_ens mIoU"] <= 1.0
    assert last["agree"] == n_agree / n_valid
    assert last["seg_crf mIoU"] == evaluate.scores(gts, crfs)["miou"]


def test_validate_coco_ensemble_on_low_resolution_logits(dev, golden_dir):
    """validate_coco(..., ensemble=True): the summed (size / 16)^2 logits of both students go through one fused pass per image; the
    students' scores are those of the plain call and the ensemble's those of predictions recomputed here."""
    from dupl_amd import ops
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    from test_eval_gpu import _loader, _tiny_model
    model, _ = _tiny_model(dev)
    loader = _loader()
    g = np.load(os.path.join(golden_dir, "val_tiny.npz"))                                 # the scales and size of tests/test_eval_gpu.py
    args = types.SimpleNamespace(scales=tuple(float(v) for v in g["coco_scales"]), crop_size=int(g["coco_size"]))
    kept = []
    s1, s2 = eval_seg.validate_coco(model, loader, args, num_classes=21)
    e1, e2, ens = eval_seg.validate_coco(model, loader, args, num_classes=21, keep_logits=lambda n, k, t: kept.append((n[0], k)),
                                         ensemble=True)
    assert e1["miou"] == s1["miou"] and e2["miou"] == s2["miou"]
    assert kept == [(d[0][0], k) for d in loader for k in (1, 2)]                        # keep_logits per student, as before
    gts, preds, n_valid, n_agree = [], [], 0, 0
    for data in loader:
        seg = eval_seg.msc_seg_logits_coco(model, data[1].to(dev), args.scales, args.crop_size)
        H, W = data[2].shape[1:]
        assert tuple(seg[0].shape[2:]) != (H, W)
        preds.append(ops.seg_ensemble(seg[0], seg[1], (H, W), want_pred=True)[0].cpu().numpy())
        gts.append(data[2][0].numpy())
        p = [ops.upsample_argmax(s, H, W)[0].cpu().numpy() for s in seg]
        ok = (gts[-1] >= 0) & (gts[-1] < 21)
        n_valid += int(ok.sum())
        n_agree += int((ok & (p[0] == p[1])).sum())
    assert ens["miou"] == evaluate.scores(gts, preds)["miou"] and 0.0 <= ens["miou"] <= 1.0
    assert ens["agree"] == n_agree / n_valid
