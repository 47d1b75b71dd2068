"""Offline CAM inference on the device (csrc/cam_eval.hip, dupl_amd.tools.infer_cam): the fused pass against the composed
existing path (ops.resize_bilinear -> cam_helper.cam_to_label -> ConfusionMatrix.update per threshold), against an independent fp64
restatement on the CPU, the overlay against a numpy restatement, the CLI end to end, and the argument errors.

Ties: a label may differ from the comparison path only where that path itself cannot tell -- |v - thr| < MARGIN for the threshold in
question or a top-2 gap < MARGIN (the repository's tie margin) -- and on at most TIE_SHARE of the pixels of a case.  The fused tap
is pinned to the roundings of resize_bilinear_kernel, so against the composed path the count is expected to be 0; against fp64 the
fp32 source coordinate (up to 448 * 2^-23 off) times the CAM's slope (<= 1/16 per pixel for a CAM up-sampled 16x) stays below MARGIN."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
TIE_SHARE = 1e-4
SWEEP19 = [float(np.float32(0.05 + 0.05 * i)) for i in range(19)]

# name: B, C, nc, (h, w), (H, W), classes present per image, thresholds
CASES = {
    "voc_375x500_T19_K2_K0": (2, 20, 21, (448, 448), (375, 500), [[3, 14], []], SWEEP19),
    "voc_500x334_T1_K1_K5": (2, 20, 21, (448, 448), (500, 334), [[0], [1, 5, 7, 12, 19]], [0.5]),
    "voc_96x96_T19_K3_K4": (2, 20, 21, (64, 64), (96, 96), [[2, 9, 10], [0, 4, 18, 19]], SWEEP19),
    "voc_97x101_odd_T19": (2, 20, 21, (448, 448), (97, 101), [[6, 7], [11]], SWEEP19),       # H*W % 4 != 0: the scalar stores
    "all_present_T1": (2, 3, 4, (32, 48), (50, 70), [[0, 1, 2], [0, 1, 2]], [0.3]),
    # 81 x (20 + 1) rows x 20 counters do not fit the 30 720 of a workgroup: the thresholds go in two chunks (17 + 2); 81 x 7 x 20 fit
    "coco_333x500_T19_K20_K6": (2, 80, 81, (448, 448), (333, 500), [list(range(0, 80, 4)), [1, 2, 33, 34, 60, 78]], SWEEP19),
    "coco_480x640_T1_K12": (1, 80, 81, (448, 448), (480, 640), [[0, 3, 8, 15, 22, 31, 40, 47, 55, 62, 71, 79]], [0.45]),
    # 2049 x (10 + 1) rows: not even one threshold fits, the histogram goes through global atomics without being asked to (impl 0);
    # every case also runs its histogram once more with impl = 1, which forces that path
    "wide_nc2049_T2_K10": (1, 80, 2049, (448, 448), (120, 160), [list(range(0, 80, 8))], [0.5, 0.7]),
}


def make_case(name):
    """Min-max normalised CAMs as the pipeline makes them (28^2 activations up-sampled to (h,w), normalised per plane), the
    multi-hot labels, and a ground truth of random class blobs with 255 sprinkled in and a 255 border band."""
    B, C, nc, (h, w), (H, W), present, thr = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    low = torch.rand((B, C, 28, 28), generator=g) ** 2
    cam = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)
    mn, mx = cam.amin((2, 3), keepdim=True), cam.amax((2, 3), keepdim=True)
    cam = ((cam - mn) / (mx - mn + 1e-5)).contiguous()
    cls = torch.zeros((B, C))
    for b, ks in enumerate(present):
        for k in ks:
            cls[b, k] = 1.0
    gt = torch.randint(0, nc, (B, 1, 12, 16), generator=g).float()
    gt = F.interpolate(gt, size=(H, W), mode="nearest")[:, 0].long()
    gt[torch.rand((B, H, W), generator=g) < 0.05] = 255
    gt[:, :2, :] = 255
    return B, C, nc, (H, W), cam, cls, gt, [float(t) for t in thr]


def composed(ops, cam_helper, evaluate, cam, cls, gt, thr, nc, size):
    """The existing path: resize, then per threshold cam_to_label and ConfusionMatrix.update -> (labels (T,B,H,W), hists, value,
    top-2 gap of the valid CAM)."""
    rc = ops.resize_bilinear(cam, size[0], size[1])
    labels, hists = [], []
    for t in thr:
        lab = cam_helper.cam_to_label(rc, cls, bkg_thre=t)
        cm = evaluate.ConfusionMatrix(nc, cam.device)
        cm.update(gt, lab)
        labels.append(lab)
        hists.append(cm.hist)
    valid = cam_helper.get_valid_cam(rc, cls)
    top = torch.topk(valid, min(2, valid.shape[1]), dim=1)[0]
    gap = top[:, 0] - top[:, -1] if valid.shape[1] > 1 else torch.full_like(top[:, 0], float("inf"))
    return torch.stack(labels), torch.stack(hists), valid.max(dim=1)[0], gap


def fused(ops, evaluate, cam, cls, gt, thr, nc, size, impl=0):
    """ops.cam_eval: all T histograms in one call (with the value), and the label map of every threshold (one call each)."""
    hist = torch.zeros((len(thr), nc, nc), device=cam.device, dtype=torch.int64)
    _, value = ops.cam_eval(cam, cls, size, thr, gt=gt, hist=hist, want_value=True, impl=impl)
    labels = torch.stack([ops.cam_eval(cam, cls, size, thr, label_at=t)[0] for t in range(len(thr))])
    # the histogram of threshold t is the confusion matrix of the label map at t, as integers
    for t in range(len(thr)):
        cm = evaluate.ConfusionMatrix(nc, cam.device)
        cm.update(gt, labels[t].long())
        assert torch.equal(cm.hist, hist[t]), f"hist[{t}] is not the confusion matrix of the label map at thr[{t}]"
    return labels, hist, value


def check_labels(tag, got, want, value_ref, gap_ref, thr):
    """got / want (T,B,H,W): equal except at proven ties of the comparison path, on at most TIE_SHARE of the pixels."""
    T = got.shape[0]
    diff = got.long() != want.long()
    n_diff = int(diff.sum())
    thr_t = torch.tensor(thr, dtype=value_ref.dtype, device=value_ref.device).view(T, 1, 1, 1)
    tie = ((value_ref[None] - thr_t).abs() < MARGIN) | (gap_ref[None] < MARGIN)
    unexplained = int((diff & ~tie).sum())
    px = want[0].numel()
    per_t = diff.flatten(1).sum(1)
    print(f"{tag}: {n_diff} label(s) differ over {T} threshold(s) x {px} pixels (worst threshold {int(per_t.max())}), "
          f"{unexplained} of them not at a tie")
    assert unexplained == 0
    assert int(per_t.max()) <= TIE_SHARE * px
    return n_diff


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_pass_equals_the_composed_path(dev, name):
    """(a) label maps, all T histograms and the value against resize_bilinear -> cam_to_label -> ConfusionMatrix.update."""
    from dupl_amd import ops
    from dupl_amd.utils import cam_helper, evaluate
    B, C, nc, size, cam, cls, gt, thr = make_case(name)
    cam, cls, gt = cam.to(dev), cls.to(dev), gt.to(dev)
    lab_c, hist_c, val_c, gap_c = composed(ops, cam_helper, evaluate, cam, cls, gt, thr, nc, size)
    lab_c2, hist_c2, val_c2, _ = composed(ops, cam_helper, evaluate, cam, cls, gt, thr, nc, size)
    assert torch.equal(lab_c, lab_c2) and torch.equal(hist_c, hist_c2) and torch.equal(val_c, val_c2)      # no exemption
    lab_f, hist_f, val_f = fused(ops, evaluate, cam, cls, gt, thr, nc, size)
    assert lab_f.dtype == torch.uint8 and val_f.dtype == torch.float32 and tuple(val_f.shape) == (B,) + tuple(size)
    assert torch.equal(val_f, val_c), f"value_out differs from the max of the resized valid CAM: max |d| {float((val_f - val_c).abs().max()):.3e}"
    n_diff = check_labels(f"{name} vs composed", lab_f, lab_c, val_c, gap_c, thr)
    if n_diff == 0:
        assert torch.equal(hist_f, hist_c)
    # every image without a class is all background; counts: every pixel with a ground truth in [0, nc) once per threshold
    for b in range(B):
        if not bool(cls[b].any()):
            assert int(lab_f[:, b].max()) == 0 and float(val_f[b].abs().max()) == 0.0
    assert hist_f.sum(dim=(1, 2)).tolist() == [int(((gt >= 0) & (gt < nc)).sum())] * len(thr)
    assert int(lab_f.max()) <= C and set(lab_f.unique().tolist()) <= {0} | {c + 1 for c in range(C) if bool(cls[:, c].any())}
    # accumulation (+=) and the forced global-atomics histogram give the same counts
    hist_g = hist_f.clone()
    ops.cam_eval(cam, cls, size, thr, gt=gt, hist=hist_g, impl=1)
    assert torch.equal(hist_g, 2 * hist_f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_pass_equals_an_fp64_restatement(dev, name):
    """(b) F.interpolate in float64 on the CPU + the reference's cam_to_label lines (cam_helper.py:12-16)."""
    from dupl_amd import ops
    from dupl_amd.utils import evaluate
    B, C, nc, size, cam, cls, gt, thr = make_case(name)
    rc = F.interpolate(cam.double(), size=size, mode="bilinear", align_corners=False)
    valid = cls.double()[:, :, None, None] * rc
    value64, arg = valid.max(dim=1)
    want = torch.stack([torch.where(value64 <= float(np.float32(t)), torch.zeros_like(arg), arg + 1) for t in thr])
    top = torch.topk(valid, min(2, C), dim=1)[0]
    gap = top[:, 0] - top[:, -1]
    lab_f, hist_f, val_f = fused(ops, evaluate, cam.to(dev), cls.to(dev), gt.to(dev), thr, nc, size)
    lab_f, hist_f, val_f = lab_f.cpu(), hist_f.cpu(), val_f.cpu()
    err = float((val_f.double() - value64).abs().max())
    print(f"{name}: max |value - fp64| {err:.3e}")
    assert err < MARGIN
    n_diff = check_labels(f"{name} vs fp64", lab_f, want, value64, gap, thr)
    if n_diff == 0:
        for t in range(len(thr)):
            ref = evaluate._fast_hist(gt.numpy().reshape(-1), want[t].numpy().reshape(-1), nc)
            assert np.array_equal(hist_f[t].numpy(), ref)


def test_overlay_equals_a_float64_numpy_restatement(dev, golden_dir):
    """(c) color_map(v)[:, :, :3] * 255, alpha-blended with the de-normalised image in float64 and truncated
    (infer_cam_voc.py:81-87), fed with the kernel's own value_out."""
    from dupl_amd import ops
    from dupl_amd.utils import imutils
    lut = np.load(os.path.join(golden_dir, "jet_lut.npy"))
    for name in ("voc_375x500_T19_K2_K0", "voc_97x101_odd_T19"):
        B, C, nc, (H, W), cam, cls, gt, thr = make_case(name)
        _, value = ops.cam_eval(cam.to(dev), cls.to(dev), (H, W), thr, want_value=True)
        value[0, 0, :4] = torch.tensor([0.0, 1.0, 255.0 / 256.0, 0.999999], device=dev)
        g = torch.Generator().manual_seed(7)
        inputs = (torch.randn((B, 3, H, W), generator=g) * 1.2).clamp(-2.1, 2.6).to(dev)
        got = ops.cam_overlay(value, inputs, alpha=0.6).cpu().numpy()
        plain = ops.cam_overlay(value).cpu().numpy()
        assert got.shape == (B, H, W, 3) and got.dtype == np.uint8 and plain.shape == got.shape
        v = value.cpu().numpy()
        idx = np.minimum((v * np.float32(256)).astype(np.int64), 255)
        rgb = lut[idx] * 255
        img = imutils.denormalize_img(inputs).permute(0, 2, 3, 1).cpu().numpy()
        alpha = 0.6
        blend = alpha * rgb + (1 - alpha) * img
        want = blend.astype(np.uint8)
        assert np.array_equal(plain, rgb.astype(np.uint8))                       # the image-less form: exact
        d = got.astype(np.int64) - want.astype(np.int64)
        near = np.abs(blend - np.round(blend)) < 1e-3
        slack = int((d != 0).sum())
        print(f"overlay {name}: {slack} of {d.size} bytes use the +-1 allowance")
        assert np.abs(d).max() <= 1 and not bool(((d != 0) & ~near).any())


def _voc_folder(tmp_path):
    """A tiny VOC-layout folder and a reference-format checkpoint, as tests/test_crf_gpu.py builds them."""
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
    argv = ["--model_path", ckpt, "--backbone", "tiny_test", "--data_folder", str(root), "--list_folder", str(lists),
            "--infer_set", "val"]
    return root, lists, names, cls, ckpt, argv


def _run_cli(argv):
    """`python -m dupl_amd.tools.infer_cam <argv>` as its own process -> (stdout, the dict of its last line)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "dupl_amd.tools.infer_cam"] + argv, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout, eval(r.stdout.strip().splitlines()[-1], {"np": np, "nan": float("nan")})


def test_infer_cam_cli(dev, tmp_path):
    """(d) from the checkpoint to the cam / aux_cam scores, the overlays and the label PNGs; the scores equal those of
    multi_scale_cam2_siamese + the composed path over the same loader, computed in this process."""
    from PIL import Image
    from torch.utils.data import DataLoader
    from dupl_amd import ops
    from dupl_amd.datasets import voc
    from dupl_amd.datasets.device_loader import DeviceValLoader, raw_collate
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.tools.eval_seg import load_checkpoint
    from dupl_amd.utils import cam_helper, evaluate, imutils
    root, lists, names, cls, ckpt, argv = _voc_folder(tmp_path)
    out, last = _run_cli(argv + ["--save_labels", "1"])
    assert sorted(last) == ["aux_cam mIoU", "cam mIoU"]
    assert "aux_cam" in out and "aeroplane" in out and "mIoU" in out and "bkg_thre 0." not in out
    run = tmp_path / "run"
    for nm in names:
        H, W = np.array(Image.open(root / "SegmentationClassAug" / (nm + ".png"))).shape
        for d in ("cam_img", "cam_img_aux"):
            jpg = np.array(Image.open(run / d / "val" / (nm + ".jpg")))
            assert jpg.shape == (H, W, 3) and jpg.dtype == np.uint8
        png = np.array(Image.open(run / "cam_labels" / "val" / (nm + ".png")))
        assert png.shape == (H, W) and png.dtype == np.uint8
        assert set(np.unique(png).tolist()) <= {0} | {int(c) + 1 for c in np.nonzero(cls[nm])[0]}
        rgb = np.array(Image.open(run / "cam_labels_rgb" / "val" / (nm + ".png")))
        assert np.array_equal(rgb, imutils.encode_cmap(png))

    # the same numbers in this process: the composed path over the same loader
    ds = voc.VOC12SegDataset(root_dir=str(root), name_list_dir=str(lists), split="val", stage="val", aug=False, ignore_index=255,
                             num_classes=21)
    loader = DeviceValLoader(DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=raw_collate), dev)
    model = siamese_network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    load_checkpoint(model, ckpt)
    model.to(dev).eval()
    cms = [evaluate.ConfusionMatrix(21, dev) for _ in range(2)]
    pngs = {}
    with torch.no_grad():
        for name, inputs, labels, cl in loader:
            inputs, labels, cl = inputs.to(dev).float().contiguous(), labels.to(dev).long().contiguous(), cl.to(dev).float()
            x = ops.resize_bilinear(inputs, 448, 448)
            cams = cam_helper.multi_scale_cam2_siamese(model, inputs=x, scales=(1.0, 0.5, 1.5), branch=1)
            for cm, c in zip(cms, cams):
                lab = cam_helper.cam_to_label(ops.resize_bilinear(c, labels.shape[1], labels.shape[2]), cl, bkg_thre=0.5)
                cm.update(labels, lab)
                pngs.setdefault(name[0], lab[0].cpu().numpy().astype(np.uint8))
    want = [c.scores()["miou"] for c in cms]
    print(f"infer_cam CLI: cam mIoU {last['cam mIoU']:.6f} (composed {want[0]:.6f}), aux_cam mIoU {last['aux_cam mIoU']:.6f} "
          f"(composed {want[1]:.6f})")
    assert abs(last["cam mIoU"] - want[0]) <= 1e-12 and abs(last["aux_cam mIoU"] - want[1]) <= 1e-12
    assert 0.0 <= want[0] <= 1.0
    for nm in names:
        assert np.array_equal(np.array(Image.open(run / "cam_labels" / "val" / (nm + ".png"))), pngs[nm])

    out2, sw = _run_cli(argv + ["--sweep", "0.1:0.9:0.2", "--save_img", "0"])
    assert sorted(sw) == ["aux_cam best mIoU", "aux_cam best_bkg_thre", "aux_cam mIoU", "cam best mIoU", "cam best_bkg_thre", "cam mIoU"]
    assert sw["cam mIoU"] == last["cam mIoU"] and sw["aux_cam mIoU"] == last["aux_cam mIoU"]
    assert sw["cam best mIoU"] >= sw["cam mIoU"] and sw["aux_cam best mIoU"] >= sw["aux_cam mIoU"]
    lines = [ln for ln in out2.splitlines() if ln.startswith("bkg_thre ")]
    assert len(lines) == 5 and any(ln.startswith("bkg_thre 0.5000:") for ln in lines)      # 0.1 .. 0.9 step 0.2: 0.5 is a point


def test_bad_arguments_are_refused_and_launch_nothing(dev):
    """(e) descending thresholds, T = 0, a null cam or a label_at out of range: DUPL_ERR_ARG from the library, an exception from
    the wrapper, outputs untouched."""
    from dupl_amd import _lib, ops
    L = _lib.lib()
    B, C, h, w, H, W = 1, 4, 8, 8, 10, 12
    cam = torch.rand((B, C, h, w), device=dev)
    cls = torch.ones((B, C), device=dev)
    label = torch.full((B, H, W), 77, device=dev, dtype=torch.uint8)
    value = torch.full((B, H, W), -7.0, device=dev)
    gt = torch.zeros((B, H, W), device=dev, dtype=torch.int64)
    hist = torch.zeros((2, 5, 5), device=dev, dtype=torch.int64)

    def raw(thr, **kw):
        arr = np.asarray(thr, dtype=np.float32)
        base = dict(B=B, C=C, h=h, w=w, H=H, W=W, T=len(thr), num_classes=5, label_at=0, cam=cam.data_ptr(), cls_label=cls.data_ptr(),
                    thr=arr.ctypes.data if len(thr) else None, gt=gt.data_ptr(), hist=hist.data_ptr(), label_out=label.data_ptr(),
                    value_out=value.data_ptr())
        base.update(kw)
        d = _lib.CamEvalDesc(**base)
        if "struct_size" in kw:
            d.struct_size = kw["struct_size"]
        return L.dupl_cam_eval.raw(ctypes.byref(d), ops._stream())

    assert raw([0.25, 0.5]) == 0                                                   # the good call, for contrast
    torch.cuda.synchronize()
    assert int(hist.sum()) == 2 * H * W and float(value.min()) >= 0.0
    label.fill_(77), value.fill_(-7.0), hist.zero_()
    bad = [raw([0.5, 0.25]), raw([]), raw([0.5] * 65), raw([0.25, 0.5], cam=None), raw([0.25, 0.5], label_at=2),
           raw([0.25, 0.5], label_at=-1), raw([-0.1, 0.5]), raw([0.5, 1.5]), raw([0.25, float("nan")]), raw([0.25, 0.5], gt=None),
           raw([0.25, 0.5], num_classes=4), raw([0.25, 0.5], C=256), raw([0.25, 0.5], H=0), raw([0.25, 0.5], struct_size=8),
           raw([0.25, 0.5], hist=None, label_out=None, value_out=None)]
    assert bad == [-1] * len(bad), bad
    with pytest.raises(ValueError):
        ops.cam_eval(cam, cls, (H, W), [0.5, 0.25], label_at=0)
    with pytest.raises(ValueError):
        ops.cam_eval(cam, cls, (H, W), [], label_at=0)
    with pytest.raises(RuntimeError):
        ops.cam_eval(cam, cls, (H, W), [0.25, 0.5], label_at=2)
    with pytest.raises(RuntimeError):
        ops.cam_eval(cam, cls, (H, W), [0.25, 0.5])                                # no output asked for
    ov = torch.full((B, H, W, 3), 9, device=dev, dtype=torch.uint8)
    assert L.dupl_cam_overlay.raw(None, None, ov.data_ptr(), B, H, W, 0.6, None, ops._stream()) == -1
    assert L.dupl_cam_overlay.raw(value.data_ptr(), None, None, B, H, W, 0.6, None, ops._stream()) == -1
    assert L.dupl_cam_overlay.raw(value.data_ptr(), None, ov.data_ptr(), B, 0, W, 0.6, None, ops._stream()) == -1
    assert L.dupl_cam_overlay.raw(value.data_ptr(), None, ov.data_ptr(), B, H, W, 1.5, None, ops._stream()) == -1
    torch.cuda.synchronize()
    assert int(label.min()) == 77 and float(value.max()) == -7.0 and int(hist.sum()) == 0 and int(ov.min()) == 9
