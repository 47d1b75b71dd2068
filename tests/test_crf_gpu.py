"""DenseCRF post-processing on the device (csrc/crf.hip, ops.crf_message / ops.dense_crf, utils/dcrf.py, eval_seg --crf)
against the brute-force fp64 mean-field of tests/crf_ref.py.

The bar for "fp32-equivalent": in the same test a plain fp32 torch evaluation of the same formulas (tests/crf_ref.py with
dtype=float32 -- the reference, not the code under test) is measured against fp64, and the device result may be at most 4x
that far from fp64 (the project's "2x the exact-f32 kernel's error" rule, doubled because the device exp and a different
summation order stack).  The fp32 yardstick is floored at 2^-24: the exact result rounded to fp32 is already that far
from fp64, and on degenerate inputs (a 1 x 1 image) the host evaluation happens to be exact, which no fp32 output can be held to.
Message errors are relative to the row's fp64 value (a pixel's row of C channel values, measured against its largest entry)."""
import ctypes
import functools
import os
import numpy as np
import pytest
import torch

import crf_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0
KERNELS = (("gauss sxy=1", False, 1.0, 1.0), ("gauss sxy=3", False, 3.0, 1.0), ("bilateral 121/5", True, 121.0, 5.0),
           ("bilateral 80/13", True, 80.0, 13.0))


def _bar(err32):
    return FACTOR * max(err32, R.EPS32)


@functools.lru_cache(maxsize=None)
def _case(H, W, C):
    return R.make_case(H, W, C, seed=R.case_seed(H, W))


@functools.lru_cache(maxsize=None)
def _mean_field(H, W, C, pset, dtype):
    img, _, logits = _case(H, W, C)
    U = R.unary_from_softmax(torch.softmax(logits, 0))
    return R.mean_field(img, U, 10, dtype=dtype, **R.PARAMS[pset])


@pytest.mark.parametrize("H,W", [(48, 64), (61, 83), (1, 37), (33, 1), (1, 1)])
def test_crf_message_against_fp64(dev, H, W):
    """(a) one application of each kernel, C in {2, 21, 81}, normalised and not, and the normaliser n itself."""
    from dupl_amd import ops
    img, _, logits = _case(H, W, 81)
    img_d = img.to(dev)
    worst = 0.0
    for name, bilateral, sxy, srgb in KERNELS:
        im, im_d = (img, img_d) if bilateral else (None, None)
        K64 = R.kernel_rows(R.features(H, W, im, sxy, srgb, torch.float64))
        K32 = R.kernel_rows(R.features(H, W, im, sxy, srgb, torch.float32))
        n64, n32 = R.norm_of(K64), R.norm_of(K32)
        n_d = ops.crf_norm(im_d, H, W, sxy, srgb, device=dev)
        e32, e = R.rel_err(n32, n64), R.rel_err(n_d.cpu().reshape(-1), n64)
        print(f"({H},{W}) {name}: n rel err {e:.2e}, fp32 torch {e32:.2e}, ratio {e / max(e32, R.EPS32):.2f}")
        worst = max(worst, e / max(e32, R.EPS32))
        assert e <= _bar(e32)
        for C in (2, 21, 81):
            Q = torch.softmax(logits[:C], 0).reshape(C, -1)
            for normalize in (True, False):
                ref = R.message(K64, Q.double(), n64 if normalize else None)
                t32 = R.message(K32, Q, n32 if normalize else None)
                out = ops.crf_message(im_d, Q.reshape(C, H, W).to(dev), sxy, srgb, normalize=normalize)
                assert out.shape == (C, H, W) and out.dtype == torch.float32
                e32, e = R.row_rel_err(t32, ref), R.row_rel_err(out.cpu(), ref)
                print(f"({H},{W},{C}) {name} normalize={normalize}: row rel err {e:.2e}, fp32 torch {e32:.2e}, "
                      f"ratio {e / max(e32, R.EPS32):.2f}")
                worst = max(worst, e / max(e32, R.EPS32))
                assert e <= _bar(e32)
    print(f"({H},{W}): worst device / fp32-torch error ratio {worst:.2f} (bar {FACTOR})")


@pytest.mark.parametrize("H,W,C", R.CASES)
@pytest.mark.parametrize("pset", sorted(R.PARAMS))
def test_dense_crf_against_fp64(dev, H, W, C, pset):
    """(b) ten iterations: Q within 4x the fp32 evaluation's error, labels equal to the fp64 labels except at pixels whose fp64
    top-2 margin is under 1e-4, and at most 0.2 % of the pixels are so excused."""
    from dupl_amd import ops
    img, _, logits = _case(H, W, C)
    U = R.unary_from_softmax(torch.softmax(logits, 0))
    Q64, Q32 = _mean_field(H, W, C, pset, torch.float64), _mean_field(H, W, C, pset, torch.float32)
    p = R.PARAMS[pset]
    Q = ops.dense_crf(U.to(dev), img.to(dev), 10, p["w_g"], p["sxy_g"], p["w_b"], p["sxy_b"], p["srgb_b"]).cpu()
    e32, e = float((Q32.double() - Q64).abs().max()), float((Q.double() - Q64).abs().max())
    close = R.top2_margin(Q64) < R.MARGIN
    differ = Q.argmax(0) != Q64.argmax(0)
    print(f"({H},{W},{C}) {pset}: max |Q - Q64| {e:.2e}, fp32 torch {e32:.2e}, ratio {e / max(e32, R.EPS32):.2f}; "
          f"{int(differ.sum())} labels differ, {int(close.sum())} of {close.numel()} pixels have margin < {R.MARGIN}")
    assert e <= _bar(e32)
    assert not bool((differ & ~close).any())
    assert float(close.float().mean()) <= R.TIE_SHARE
    assert float((Q.sum(0) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("H,W,C", [(375, 500, 21), (480, 640, 81)])
def test_full_size(dev, H, W, C):
    """(c) image-sized inputs: n and the messages at 512 seeded random pixels plus the four corners against chunked fp64 rows
    (the message takes the device's n as a given input on both sides, so that the reference needs no N x N pass; n itself is
    checked at the same rows); dense_crf against the same ten iterations composed from crf_message and torch's softmax; two
    calls bit-identical.  The composition differs from dense_crf only in the softmax's rounding, which the iterations amplify like
    any fp32 rounding: the bar is 4x the largest fp32-vs-fp64 error in Q seen on the small inputs (1.3e-6, tests/test_crf_host.py
    prints it per case)."""
    from dupl_amd import ops
    img, _, logits = R.make_case(H, W, C, seed=R.case_seed(H, W))
    N = H * W
    g = torch.Generator().manual_seed(7)
    rows = torch.cat([torch.randint(0, N, (512,), generator=g), torch.tensor([0, W - 1, N - W, N - 1])])
    img_d = img.to(dev)
    Qh = torch.softmax(logits, 0).reshape(C, N)
    Q_d = Qh.reshape(C, H, W).to(dev)
    p = R.PARAMS["eval"]
    norms = {}
    for name, im, im_d, sxy, srgb in (("gauss", None, None, p["sxy_g"], 1.0), ("bilateral", img, img_d, p["sxy_b"], p["srgb_b"])):
        f64, f32 = R.features(H, W, im, sxy, srgb, torch.float64), R.features(H, W, im, sxy, srgb, torch.float32)
        n_d = ops.crf_norm(im_d, H, W, sxy, srgb, device=dev)
        norms[name] = n_d
        n64 = 1.0 / torch.sqrt(R.rowsum_rows(f64, rows) + 1e-20)
        n32 = 1.0 / torch.sqrt(R.rowsum_rows(f32, rows) + 1e-20)
        e32, e = R.rel_err(n32, n64), R.rel_err(n_d.cpu().reshape(-1)[rows], n64)
        print(f"({H},{W}) {name}: n rel err at {len(rows)} rows {e:.2e}, fp32 torch {e32:.2e}, ratio {e / max(e32, R.EPS32):.2f}")
        assert e <= _bar(e32)
        nh = n_d.cpu().reshape(-1)
        ref = R.message_rows(f64, Qh.double(), rows, nh.double())
        t32 = R.message_rows(f32, Qh, rows, nh)
        out = ops.crf_message(im_d, Q_d, sxy, srgb, normalize=n_d).cpu().reshape(C, N)[:, rows]
        e32, e = R.row_rel_err(t32, ref), R.row_rel_err(out, ref)
        print(f"({H},{W},{C}) {name}: message row rel err {e:.2e}, fp32 torch {e32:.2e}, ratio {e / max(e32, R.EPS32):.2f}")
        assert e <= _bar(e32)
    U = ops.crf_unary(Q_d)
    Q1 = ops.dense_crf(U, img_d, 10, p["w_g"], p["sxy_g"], p["w_b"], p["sxy_b"], p["srgb_b"])
    Q2 = ops.dense_crf(U, img_d, 10, p["w_g"], p["sxy_g"], p["w_b"], p["sxy_b"], p["srgb_b"])
    assert torch.equal(Q1, Q2)
    Qc = torch.softmax(-U, 0)
    for _ in range(10):
        Mg = ops.crf_message(None, Qc, p["sxy_g"], normalize=norms["gauss"])
        Mb = ops.crf_message(img_d, Qc, p["sxy_b"], p["srgb_b"], normalize=norms["bilateral"])
        Qc = torch.softmax(-U + p["w_g"] * Mg + p["w_b"] * Mb, 0)
    e = float((Q1 - Qc).abs().max())
    changed = float((Q1.argmax(0) != Q_d.argmax(0)).float().mean())
    print(f"({H},{W},{C}): dense_crf vs composed iterations max |dQ| {e:.2e}; the CRF changes {100 * changed:.1f} % of the labels")
    assert e <= FACTOR * 1.3e-6
    assert changed > 0.02


def test_dcrf_module(dev):
    """(d) utils/dcrf.py: numpy in / numpy out and device in / device out agree bit for bit; the unaries follow their formulas;
    crf_inference_label against fp64."""
    from dupl_amd.utils import dcrf
    H, W, C = 48, 64, 21
    img, labels, logits = _case(H, W, C)
    prob = torch.softmax(logits, 0)
    post = dcrf.DenseCRF(10, 1, 1, 4, 121, 5)
    q_np = post(img.numpy(), prob.numpy())
    q_d = post(img.to(dev), prob.to(dev))
    assert isinstance(q_np, np.ndarray) and q_np.shape == (C, H, W) and q_d.is_cuda
    assert np.array_equal(q_np, q_d.cpu().numpy())
    assert float((torch.from_numpy(q_np).double() - _mean_field(H, W, C, "eval", torch.float64)).abs().max()) <= \
        _bar(float((_mean_field(H, W, C, "eval", torch.float32).double() - _mean_field(H, W, C, "eval", torch.float64)).abs().max()))
    q_l = post.from_logits(img.to(dev), logits.to(dev))                       # softmax fused into the unary launch
    assert float((q_l - q_d).abs().max()) <= FACTOR * 1.3e-6                  # differs by the softmax's rounding only (see test_full_size)
    i_np = dcrf.crf_inference(img.numpy(), prob.numpy(), t=10, scale_factor=1, labels=C)
    i_d = dcrf.crf_inference(img.to(dev), prob.to(dev), labels=C)
    assert np.array_equal(i_np, i_d.cpu().numpy())
    e = float((torch.from_numpy(i_np).double() - _mean_field(H, W, C, "helper", torch.float64)).abs().max())
    assert e <= _bar(float((_mean_field(H, W, C, "helper", torch.float32).double() - _mean_field(H, W, C, "helper", torch.float64)).abs().max()))
    # unaries
    u = dcrf.unary_from_softmax(prob.to(dev)).cpu()
    assert float((u - R.unary_from_softmax(prob)).abs().max()) < 2e-6
    pc = prob.clone()
    pc[0, 0, 0], pc[1, 0, 0] = 0.0, 1.0
    u = dcrf.unary_from_softmax(pc.numpy())
    assert abs(float(u[0, 0, 0]) + np.log(1e-5)) < 1e-5 and float(u[1, 0, 0]) == 0.0
    ul = dcrf.unary_from_labels(labels.numpy(), C, 0.7)
    assert np.array_equal(ul, R.unary_from_labels(labels, C, 0.7).numpy())
    # crf_inference_label (utils/dcrf.py:26-40: Gaussian (3, 3), bilateral (50, 5, 10)) against fp64
    l_np = dcrf.crf_inference_label(img.numpy(), labels.numpy(), t=10, n_labels=C, gt_prob=0.7)
    l_d = dcrf.crf_inference_label(img.to(dev), labels.to(dev), n_labels=C)
    assert l_np.shape == (H, W) and np.array_equal(l_np, l_d.cpu().numpy())
    Q64 = R.mean_field(img, R.unary_from_labels(labels, C, 0.7), 10, 3.0, 3.0, 10.0, 50.0, 5.0)
    close = R.top2_margin(Q64) < R.MARGIN
    differ = torch.from_numpy(l_np) != Q64.argmax(0)
    print(f"crf_inference_label: {int(differ.sum())} labels differ from fp64, {int(close.sum())} pixels have margin < {R.MARGIN}")
    assert not bool((differ & ~close).any()) and float(close.float().mean()) <= R.TIE_SHARE


def _voc_folder(tmp_path, dev):
    """A tiny VOC-layout folder and a reference-format checkpoint, as tests/test_eval_gpu.py builds them."""
    from PIL import Image
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.synthetic_val import synthetic_val_samples
    from oracle import dupl_oracle as O
    root, lists, run = tmp_path / "VOC2012", tmp_path / "lists", tmp_path / "run" / "checkpoints"
    for d in (root / "JPEGImages", root / "SegmentationClassAug", lists, run):
        d.mkdir(parents=True)
    names, cls = [], {}
    for i, (x, lab, c) in enumerate(synthetic_val_samples(sizes=((75, 100), (96, 64), (64, 64)))):
        nm = f"2007_{i:06d}"
        img = ((x[0].permute(1, 2, 0).numpy() * 40 + 120).clip(0, 255)).astype(np.uint8)
        Image.fromarray(img).save(root / "JPEGImages" / (nm + ".jpg"), quality=95)
        Image.fromarray(lab[0].numpy().astype(np.uint8)).save(root / "SegmentationClassAug" / (nm + ".png"))
        names.append(nm)
        cls[nm] = c[0].numpy()
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    np.save(lists / "cls_labels_onehot.npy", cls)
    pp = O.make_siamese_params(O.VIT_TINY, 21, seed=2)
    pp = {k: (v * 6.0 if ("classifier.weight" in k or k.endswith("decoder.conv8.weight")) else v) for k, v in pp.items()}
    model = siamese_network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    model.load_state_dict(pp, strict=True)
    ckpt = str(run / "checkpoint.pth")
    torch.save({"module." + k: v.detach().cpu() for k, v in model.state_dict().items()}, ckpt)
    argv = ["--dataset", "voc", "--model_path", ckpt, "--backbone", "tiny_test", "--data_folder", str(root), "--list_folder",
            str(lists), "--scales", "(1.0, 1.5, 1.25)"]
    return root, names, argv


def _run_cli(argv):
    """`python -m dupl_amd.tools.eval_seg <argv>` as its own process, the way it is used -> (stdout, the dict of its last line)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "dupl_amd.tools.eval_seg"] + argv, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout, eval(r.stdout.strip().splitlines()[-1], {"np": np, "nan": float("nan")})     # a dict of numpy scalars


def test_eval_seg_cli_with_crf(dev, tmp_path):
    """(e) `python -m dupl_amd.tools.eval_seg ... --crf 1` goes from the checkpoint to the seg_crf score: one label PNG per image
    equal to the argmax of DenseCRF(10, 1, 1, 4, 121, 5) on the saved logits of the better student, the palette PNG beside it,
    a seg_crf table, and a score equal to evaluate.scores on those PNGs; without the flag the output is what it was."""
    from PIL import Image
    from dupl_amd import ops
    from dupl_amd.utils import evaluate, imutils
    from dupl_amd.utils.dcrf import DenseCRF
    root, names, argv = _voc_folder(tmp_path, dev)
    out0, plain = _run_cli(argv)
    assert "seg_crf" not in out0 and "crf post-processing" not in out0
    assert sorted(plain) == ["Seg_1 mIoU", "Seg_2 mIoU", "next"] and plain["next"].startswith("DenseCRF over ")
    assert not (tmp_path / "run" / "segs" / "seg_preds").exists()

    out1, last = _run_cli(argv + ["--crf", "1"])
    assert "crf post-processing..." in out1 and "seg_crf" in out1
    assert sorted(last) == ["Seg_1 mIoU", "Seg_2 mIoU", "seg_crf mIoU"]
    assert last["Seg_1 mIoU"] == plain["Seg_1 mIoU"] and last["Seg_2 mIoU"] == plain["Seg_2 mIoU"]
    table = out1[out1.index("crf post-processing..."):]
    assert "seg_crf" in table and "mIoU" in table and "aeroplane" in table           # the per-class seg_crf table
    s1, s2 = {"miou": last["Seg_1 mIoU"]}, {"miou": last["Seg_2 mIoU"]}
    branch = "branch1" if s1["miou"] > s2["miou"] else "branch2"
    post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=1, bi_xy_std=121, bi_rgb_std=5, bi_w=4)
    gts, preds = [], []
    for nm in names:
        png = np.array(Image.open(tmp_path / "run" / "segs" / "seg_preds" / "val" / (nm + ".png")))
        rgb = np.array(Image.open(tmp_path / "run" / "segs" / "seg_preds_rgb" / "val" / (nm + ".png")))
        image = np.array(Image.open(root / "JPEGImages" / (nm + ".jpg")).convert("RGB"))
        z = np.load(tmp_path / "run" / "segs" / "logits" / "val" / branch / (nm + ".npy"), allow_pickle=True).item()["msc_seg"]
        H, W, _ = image.shape
        logit = ops.resize_bilinear(torch.from_numpy(z).to(dev), H, W)
        want = post.from_logits(torch.from_numpy(image).to(dev), logit[0]).argmax(0).cpu().numpy()
        assert png.shape == (H, W) and png.dtype == np.uint8 and np.array_equal(png, want)
        assert np.array_equal(rgb, imutils.encode_cmap(png))
        gts.append(np.array(Image.open(root / "SegmentationClassAug" / (nm + ".png"))))
        preds.append(png)
    ref = evaluate.scores(gts, preds)
    assert last["seg_crf mIoU"] == ref["miou"] and 0.0 <= ref["miou"] <= 1.0


def test_bad_arguments_are_refused_and_launch_nothing(dev):
    """(f) a wrong struct_size, zero dimensions, a missing pointer or a short workspace: DUPL_ERR_ARG, outputs untouched."""
    from dupl_amd import _lib, ops
    L = _lib.lib()
    C, H, W = 3, 5, 7
    Q = torch.softmax(torch.randn((C, H, W), device=dev), 0)
    img = torch.randint(0, 256, (H, W, 3), device=dev, dtype=torch.uint8)
    out = torch.full((C, H, W), -7.0, device=dev)
    ws = torch.empty(((2 + 2 * C) * H * W,), device=dev)

    def msg(**kw):
        d = _lib.CrfDesc(C=C, H=H, W=W, img=img.data_ptr(), Q=Q.data_ptr(), out=out.data_ptr(), sxy=121.0, srgb=5.0)
        for k, v in kw.items():
            setattr(d, k, v)
        return L.dupl_crf_message.raw(ctypes.byref(d), ops._stream())

    def crf(**kw):
        d = _lib.CrfDesc(C=C, H=H, W=W, T=2, img=img.data_ptr(), unary=Q.data_ptr(), out=out.data_ptr(), workspace=ws.data_ptr(),
                         workspace_bytes=ws.numel() * 4, w_g=1.0, sxy_g=1.0, w_b=4.0, sxy_b=121.0, srgb_b=5.0)
        for k, v in kw.items():
            setattr(d, k, v)
        return L.dupl_dense_crf.raw(ctypes.byref(d), ops._stream())

    bad = [dict(struct_size=ctypes.sizeof(_lib.CrfDesc) - 8), dict(struct_size=0), dict(C=0), dict(H=0), dict(W=0), dict(H=-3),
           dict(out=None)]
    for kw in bad + [dict(sxy=0.0), dict(srgb=0.0), dict(out=Q.data_ptr())]:
        assert msg(**kw) == -1, kw
    for kw in bad + [dict(sxy_g=0.0), dict(sxy_b=-1.0), dict(srgb_b=0.0), dict(T=-1), dict(img=None), dict(unary=None),
                     dict(workspace=None), dict(workspace_bytes=ws.numel() * 4 - 4)]:
        assert crf(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert msg() == 0 and crf() == 0
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())
    with pytest.raises(RuntimeError):
        L.dupl_crf_unary(Q.data_ptr(), out.data_ptr(), 0, H * W, 0, ops._stream())
    with pytest.raises(RuntimeError):
        L.dupl_crf_unary_labels(Q.data_ptr(), out.data_ptr(), 1, H * W, 0.7, ops._stream())
