"""tools/eval_seg --boundary / --trimap_widths / --crf_method on a tiny VOC-layout folder (the recipe of tests/test_crf_gpu.py's CLI
test, copied): without the flags nothing changes; with them every column's "boundary" dict is tests/boundary_ref.py applied to the
argmax of the saved logits and the label PNGs, and the CRF stage runs the chosen inference."""
import os

import numpy as np
import pytest
import torch

import boundary_ref as BR

pytestmark = pytest.mark.gpu

SIZES = ((75, 100), (96, 64), (64, 64))
WIDTHS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def voc(tmp_path_factory, dev):
    """(root, run dir, names, argv): a VOC-layout folder of three synthetic images and a reference-format tiny_test checkpoint."""
    from PIL import Image
    from dupl_amd.model.model_dupl import siamese_network
    from dupl_amd.synthetic_val import synthetic_val_samples
    from oracle import dupl_oracle as O
    tmp = tmp_path_factory.mktemp("voc")    # stdout prints paths below it: no "boundary" in the name
    root, lists, run = tmp / "VOC2012", tmp / "lists", tmp / "run" / "checkpoints"
    for d in (root / "JPEGImages", root / "SegmentationClassAug", lists, run):
        d.mkdir(parents=True)
    names, cls = [], {}
    for i, (x, lab, c) in enumerate(synthetic_val_samples(sizes=SIZES)):
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
    return root, tmp / "run", names, argv


def _main(argv, capsys):
    """eval_seg.main in this process -> (its return value, its stdout, the dict of its last line)"""
    from dupl_amd.tools import eval_seg
    capsys.readouterr()
    ret = eval_seg.main(argv)
    out = capsys.readouterr().out
    return ret, out, eval(out.strip().splitlines()[-1], {"np": np, "nan": float("nan")})


def _gt(root, nm):
    from PIL import Image
    return np.array(Image.open(root / "SegmentationClassAug" / (nm + ".png"))).astype(np.int64)


def _logits(run, nm, dev):
    return [torch.from_numpy(np.load(run / "segs" / "logits" / "val" / b / (nm + ".npy"), allow_pickle=True).item()["msc_seg"]).to(dev)
            for b in ("branch1", "branch2")]


def _pngs(run, names):
    from PIL import Image
    return [np.array(Image.open(run / "segs" / "seg_preds" / "val" / (nm + ".png"))) for nm in names]


def test_boundary_scores_of_every_column(dev, voc, capsys):
    from dupl_amd import ops
    root, run, names, argv = voc
    plain, out0, last0 = _main(argv, capsys)
    assert isinstance(plain, tuple) and len(plain) == 2 and all("boundary" not in s for s in plain)
    assert "boundary" not in out0 and "BIoU" not in out0 and sorted(last0) == ["Seg_1 mIoU", "Seg_2 mIoU", "next"]
    sc, out1, last1 = _main(argv + ["--boundary", "1", "--ensemble", "1", "--trimap_widths", ",".join(map(str, WIDTHS))], capsys)
    assert len(sc) == 3 and sc[0]["miou"] == plain[0]["miou"] and sc[1]["miou"] == plain[1]["miou"]
    pairs = [[], [], []]
    for nm in names:
        z, gt = _logits(run, nm, dev), _gt(root, nm)
        assert max(gt.shape) <= 110 and z[0].shape[-2:] == gt.shape
        preds = [z[0].argmax(1)[0], z[1].argmax(1)[0], ops.seg_ensemble(z[0], z[1], gt.shape, want_pred=True)[0]]
        for col, p in zip(pairs, preds):
            col.append((gt, p.cpu().numpy()))
    for k, col in enumerate(("Seg_1", "Seg_2", "Seg_ens")):
        want = BR.boundary_scores(pairs[k], 21, WIDTHS, R=max(WIDTHS))
        got = sc[k]["boundary"]
        assert sorted(got) == ["biou", "biou_iou", "trimap"] and list(got["trimap"]) == list(WIDTHS)
        np.testing.assert_equal(got, want)
        assert 0.0 < want["biou"] <= 1.0 and want["trimap"][1]["miou"] != want["trimap"][8]["miou"]   # the widths discriminate
        assert last1[col + " BIoU"] == want["biou"] and f"boundary {col}: BIoU {100 * want['biou']:.3f} | trimap mIoU @1 " in out1
    assert out1.index("boundary Seg_1:") > out1.index("mIoU")                   # under the existing table
    assert sorted(last1) == sorted(["Seg_1 mIoU", "Seg_2 mIoU", "Seg_ens mIoU", "agree", "Seg_1 BIoU", "Seg_2 BIoU", "Seg_ens BIoU", "next"])


def test_crf_method_and_the_crf_column(dev, voc, capsys):
    from PIL import Image
    from dupl_amd import ops
    from dupl_amd.utils.dcrf import DenseCRF
    root, run, names, argv = voc
    default, _, last_d = _main(argv + ["--crf", "1"], capsys)
    png_default = _pngs(run, names)
    assert len(default) == 3 and "boundary" not in default[2] and "seg_crf BIoU" not in last_d
    _main(argv + ["--crf", "1", "--crf_method", "exact"], capsys)
    assert all(np.array_equal(a, b) for a, b in zip(png_default, _pngs(run, names)))
    sc, out, last = _main(argv + ["--crf", "1", "--crf_method", "lattice", "--boundary", "1", "--trimap_widths", ",".join(map(str, WIDTHS))],
                          capsys)
    png_lattice = _pngs(run, names)
    branch = 0 if sc[0]["miou"] > sc[1]["miou"] else 1
    post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=1, bi_xy_std=121, bi_rgb_std=5, bi_w=4)
    post.method = "lattice"
    pairs = []
    for nm, png in zip(names, png_lattice):
        image = np.array(Image.open(root / "JPEGImages" / (nm + ".jpg")).convert("RGB"))
        H, W, _ = image.shape
        logit = ops.resize_bilinear(_logits(run, nm, dev)[branch], H, W)
        want = post.from_logits(torch.from_numpy(image).to(dev), logit[0]).argmax(0).cpu().numpy()
        assert png.shape == (H, W) and np.array_equal(png, want)
        pairs.append((_gt(root, nm), png.astype(np.int64)))
    assert not all(np.array_equal(a, b) for a, b in zip(png_default, png_lattice))            # the flag reached the CRF
    want = BR.boundary_scores(pairs, 21, WIDTHS, R=max(WIDTHS))
    np.testing.assert_equal(sc[2]["boundary"], want)
    assert last["seg_crf BIoU"] == want["biou"] and f"boundary seg_crf: BIoU {100 * want['biou']:.3f}" in out
    assert all("boundary" in s for s in sc[:2]) and "Seg_1 BIoU" in last
