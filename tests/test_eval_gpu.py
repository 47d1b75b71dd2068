"""SURVEY 8f-2 / 8f-4 on the GPU: in-loop validation (validate_siamase), device confusion matrices / mIoU, multi-scale
segmentation inference and the reference checkpoint format, against tests/golden/val_tiny.npz (made by
oracle/gen_golden_val.py from the reference's own functions) and against the oracle."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAMES = ["CAM_1", "aux_CAM_1", "Seg_1", "CAM_2", "aux_CAM_2", "Seg_2"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny_model(dev):
    from dupl_amd.model.model_dupl import siamese_network
    from oracle import dupl_oracle as O
    pp = O.make_siamese_params(O.VIT_TINY, 21, seed=2)
    pp = {k: (v * 6.0 if ("classifier.weight" in k or k.endswith("decoder.conv8.weight")) else v) for k, v in pp.items()}
    model = siamese_network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    model.load_state_dict(pp, strict=True)
    return model.to(dev), pp


def _loader():
    from dupl_amd.synthetic_val import synthetic_val_samples
    return [((f"img{i}",), x, lab, cls) for i, (x, lab, cls) in enumerate(synthetic_val_samples())]


def test_confusion_f1_argmax_kernels(dev):
    from dupl_amd import ops
    from dupl_amd.utils import evaluate
    rng = np.random.RandomState(0)
    for nc, n in ((21, 100_003), (81, 250_000), (200, 50_000)):
        gt = rng.randint(0, nc + 2, size=n).astype(np.int64)
        gt[rng.rand(n) < 0.1] = 255
        pred = rng.randint(0, nc, size=n).astype(np.int64)
        cm = evaluate.ConfusionMatrix(nc, dev)
        cm.update(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev))
        cm.update(torch.from_numpy(gt[: n // 2]).to(dev), torch.from_numpy(pred[: n // 2]).to(dev))
        ref = evaluate._fast_hist(gt, pred, nc) + evaluate._fast_hist(gt[: n // 2], pred[: n // 2], nc)
        assert np.array_equal(cm.hist.cpu().numpy(), ref)
    logits = torch.randn(3, 21, 13, 17)
    up = F.interpolate(logits, size=(75, 100), mode="bilinear", align_corners=False)
    got = ops.upsample_argmax(logits.to(dev), 75, 100).cpu()
    # a pixel may differ from the float64 argmax only where the float64 top-1 - top-2 margin is within twice what a correct fp32
    # bilinear may be off (tests/glue_ref.py), and such pixels are at most 0.1 % of the map
    import glue_ref
    arg64, margin, bound = glue_ref.upsample_argmax64(logits, 75, 100)
    excusable = margin <= 2.0 * bound
    assert not bool(((got != arg64) & ~excusable).any())
    assert int(excusable.sum()) <= 1e-3 * excusable.numel()
    assert torch.equal(ops.argmax_channels(up.to(dev)).cpu(), up.argmax(1))
    from sklearn.metrics import f1_score
    cls = torch.randn(5, 20)
    lab = (torch.rand(5, 20) < 0.2).float()
    lab[3] = 0
    cls[3] = -1.0                      # no positives anywhere: f1 = 0
    tot = torch.zeros(1, device=dev)
    ops.multilabel_f1_accum(cls.to(dev), lab.to(dev), tot)
    ref = sum(f1_score(lab[i].numpy(), (cls[i] > 0).numpy().astype(np.float32), zero_division=0) for i in range(5))
    assert abs(float(tot.item()) - ref) < 1e-5


def _cam_tie_pixels(pp, crop):
    """Pixels whose CAM label is decided by a floating-point tie: min-max normalisation maps the maximum of EVERY
    class plane to 1/(1+1e-5), so two present classes that peak at the same location differ by rounding only (the
    oracle itself flips such pixels between machines).  Returned per confusion-matrix name."""
    from oracle import dupl_oracle as O
    from dupl_amd.synthetic_val import synthetic_val_samples
    ties = {n: 0 for n in NAMES}
    with torch.no_grad():
        for x, lab, cls in synthetic_val_samples():
            xin = F.interpolate(x, size=[crop, crop], mode="bilinear", align_corners=False)
            for k in (1, 2):
                cams = O.multi_scale_cam(O.sub_params(pp, f"branch{k}."), xin, O.VIT_TINY, (1.0, 0.5, 1.5))
                for nm, c in zip((f"CAM_{k}", f"aux_CAM_{k}"), cams):
                    v = cls[:, :, None, None] * F.interpolate(c, size=lab.shape[1:], mode="bilinear", align_corners=False)
                    top = v.topk(2, dim=1).values
                    tie = ((top[:, 0] - top[:, 1]) < 1e-5) & (top[:, 0] > 0.5)
                    ties[nm] += int((tie | ((top[:, 0] - 0.5).abs() < 1e-5)).sum())
    return ties


@pytest.mark.parametrize("dual", [False, True])
def test_validate_siamase_matches_reference(dev, golden_dir, dual):
    from dupl_amd.utils import train_helper
    g = np.load(os.path.join(golden_dir, "val_tiny.npz"))
    model, pp = _tiny_model(dev)
    model.enable_dual_stream(dual)
    ties = _cam_tie_pixels(pp, int(g["crop_size"]))
    print("fp-tie pixels per map:", ties)
    args = types.SimpleNamespace(crop_size=int(g["crop_size"]), cam_scales=(1.0, 0.5, 1.5), bkg_thre=0.5, high_thre=0.7,
                                 low_thre=0.25, ignore_index=255)
    captured = {}
    from dupl_amd.utils import evaluate
    orig = evaluate.ConfusionMatrix.scores

    def spy(self):
        captured[len(captured)] = self.hist.cpu().numpy().copy()
        return orig(self)

    evaluate.ConfusionMatrix.scores = spy
    try:
        c1, c2, table, items = train_helper.validate_siamase(model=model, data_loader=_loader(), args=args, return_item=True)
    finally:
        evaluate.ConfusionMatrix.scores = orig
    print(table)
    assert model.training
    assert abs(c1 - float(g["cls_scores"][0])) < 1e-6 and abs(c2 - float(g["cls_scores"][1])) < 1e-6
    for i, n in enumerate(NAMES):
        ref = g[f"hist.{n}"]
        diff = int(np.abs(captured[i] - ref).sum())
        print(f"{n}: confusion-matrix L1 difference {diff} of {int(ref.sum())} px")
        assert captured[i].sum() == ref.sum()
        assert diff <= 2 * ties[n] + 4, n     # every differing pixel moves one count between two bins
        ref_item = float(g["validate_items"][i])         # return value of the reference's validate_siamase itself
        assert np.isclose(ref_item, float(np.mean(g[f"iou.{n}"] * 100)), equal_nan=True)
        if np.isnan(ref_item):
            assert np.isnan(items[i])
        else:
            assert abs(items[i] - ref_item) < 0.05 + 100.0 * ties[n] / max(int(ref.sum()), 1)


def test_msc_seg_inference_and_checkpoint(dev, golden_dir, tmp_path):
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    g = np.load(os.path.join(golden_dir, "val_tiny.npz"))
    src, pp = _tiny_model(dev)
    # the reference's checkpoint: state_dict of the DDP-wrapped model (keys prefixed `module.`)
    path = str(tmp_path / "checkpoint.pth")
    torch.save({"module." + k: v.detach().cpu() for k, v in src.state_dict().items()}, path)
    model = siamese_network("tiny_test", num_classes=21, pretrained=False, aux_layer=-3)
    eval_seg.load_checkpoint(model, path)
    model.to(dev)
    for k, v in pp.items():
        assert torch.equal(model.state_dict()[k].cpu(), v), k
    loader = _loader()
    scales = tuple(float(s) for s in g["scales"])
    kept = {}
    args = types.SimpleNamespace(scales=scales)
    s1, s2 = eval_seg.validate(model, loader, args, num_classes=21, keep_logits=lambda name, k, t: kept.__setitem__((name[0], k), t.cpu()))
    for i in range(len(loader)):
        for k in (1, 2):
            got = kept[(f"img{i}", k)]
            ref = torch.from_numpy(g[f"msc_logits.{k}.{i}"])
            err = float((got[:, :, ::3, ::3] - ref).abs().max() / ref.abs().max())
            assert err < 2e-4, (i, k, err)
            # predictions == the reference's except at proven ties: where they differ, the top-2 gap of the logits must be
            # within twice the measured logit deviation (the golden keeps the reference logits on a 1/3 sub-grid only)
            pred = got.argmax(1)[0]
            t2 = got.topk(2, dim=1).values
            gap = (t2[:, 0] - t2[:, 1])[0]
            bad = torch.from_numpy(pred.numpy().astype(np.uint8) != g[f"msc_pred.{k}.{i}"])
            tol = 2.0 * float((got[:, :, ::3, ::3] - ref).abs().max()) + 1e-6
            worst = float(gap[bad].max()) if bad.any() else 0.0
            print(f"img{i} branch{k}: {int(bad.sum())} prediction mismatches, largest top-2 gap among them {worst:.2e} (bar {tol:.2e})")
            assert worst <= tol and int(bad.sum()) <= 1e-3 * bad.numel(), (i, k, worst, tol)
    for k, s in ((1, s1), (2, s2)):
        ref = float(g["msc_miou"][k - 1])
        print(f"branch{k}: msc mIoU {s['miou']:.6f} (reference {ref:.6f})")
        assert abs(s["miou"] - ref) < 2e-3


def test_eval_seg_cli_on_a_voc_folder(dev, tmp_path):
    """`python -m dupl_amd.tools.eval_seg` (tools/eval_seg_voc.py's flags): a VOC-layout folder on disk (JPEGImages /
    SegmentationClassAug / val.txt / cls_labels_onehot.npy), a reference-format checkpoint; the CLI's scores equal a direct
    validate() over the same decoded files and the per-image logits are written where the reference's CRF stage reads them."""
    from PIL import Image
    from torch.utils.data import DataLoader
    from dupl_amd.datasets import voc
    from dupl_amd.datasets.device_loader import DeviceValLoader, raw_collate
    from dupl_amd.tools import eval_seg
    from dupl_amd.synthetic_val import synthetic_val_samples
    root, lists, run = tmp_path / "VOC2012", tmp_path / "lists", tmp_path / "run" / "checkpoints"
    for d in (root / "JPEGImages", root / "SegmentationClassAug", lists, run):
        d.mkdir(parents=True)
    names, cls = [], {}
    for i, (x, lab, c) in enumerate(synthetic_val_samples(sizes=((75, 100), (96, 64), (110, 90), (64, 64)))):
        nm = f"2007_{i:06d}"
        img = ((x[0].permute(1, 2, 0).numpy() * 40 + 120).clip(0, 255)).astype(np.uint8)
        Image.fromarray(img).save(root / "JPEGImages" / (nm + ".jpg"), quality=95)
        Image.fromarray(lab[0].numpy().astype(np.uint8)).save(root / "SegmentationClassAug" / (nm + ".png"))
        names.append(nm)
        cls[nm] = c[0].numpy()
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    np.save(lists / "cls_labels_onehot.npy", cls)
    src, _ = _tiny_model(dev)
    ckpt = str(run / "checkpoint.pth")
    torch.save({"module." + k: v.detach().cpu() for k, v in src.state_dict().items()}, ckpt)
    s1, s2 = eval_seg.main(["--dataset", "voc", "--model_path", ckpt, "--backbone", "tiny_test", "--data_folder", str(root),
                            "--list_folder", str(lists), "--scales", "(1.0, 1.5, 1.25)"])
    ds = voc.VOC12SegDataset(root_dir=str(root), name_list_dir=str(lists), split="val", stage="val", aug=False)
    loader = DeviceValLoader(DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=raw_collate), dev)
    with torch.no_grad():
        d1, d2 = eval_seg.validate(src, loader, types.SimpleNamespace(scales=(1.0, 1.5, 1.25)), num_classes=21)
    assert s1["miou"] == d1["miou"] and s2["miou"] == d2["miou"] and 0.0 <= s1["miou"] <= 1.0
    for b in ("branch1", "branch2"):
        for nm, (x, lab, _) in zip(names, synthetic_val_samples(sizes=((75, 100), (96, 64), (110, 90), (64, 64)))):
            z = np.load(tmp_path / "run" / "segs" / "logits" / "val" / b / (nm + ".npy"), allow_pickle=True).item()["msc_seg"]
            assert z.shape == (1, 21) + tuple(lab.shape[1:]) and np.isfinite(z).all()


def test_coco_style_msc_inference(dev, golden_dir):
    """tools/eval_seg_coco_ddp.py:76-125 (resize to a square, sum over scales at logit size, up-sample the sum) vs the
    reference composition in val_tiny.npz; 21-class tiny model, the ConfusionMatrix path of validate_coco."""
    from dupl_amd.tools import eval_seg
    g = np.load(os.path.join(golden_dir, "val_tiny.npz"))
    model, _ = _tiny_model(dev)
    loader = _loader()
    scales = tuple(float(s) for s in g["coco_scales"])
    size = int(g["coco_size"])
    for i, data in enumerate(loader):
        seg = eval_seg.msc_seg_logits_coco(model, data[1].to(dev), scales, size)
        for k in (1, 2):
            ref = torch.from_numpy(g[f"coco_logits.{k}.{i}"])
            err = float((seg[k - 1].cpu() - ref).abs().max() / ref.abs().max())
            assert err < 2e-4, (i, k, err)
    args = types.SimpleNamespace(scales=scales, crop_size=size)
    s1, s2 = eval_seg.validate_coco(model, loader, args, num_classes=21)
    for k, s in ((1, s1), (2, s2)):
        ref = float(g["coco_miou"][k - 1])
        print(f"branch{k}: coco-style mIoU {s['miou']:.6f} (reference {ref:.6f})")
        assert abs(s["miou"] - ref) < 2e-3
