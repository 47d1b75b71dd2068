"""tools/eval_seg --calibration / --calib_bins / --temp_sweep / --calib_json and tools/predict --temperature on the GPU, on the tiny
VOC-layout folder of tests/test_eval_seg_boundary_gpu.py and the seeded tiny model: every "calibration" entry is an
evaluate.CalibrationMatrix fed by hand from the saved logits; without the flags nothing is added; the confidence predict writes at
a temperature is, bit for bit, the one the calibration pass binned."""
import json
import types

import numpy as np
import pytest
import torch

import calib_ref as CR
import kernel_guard as KG
from test_eval_seg_boundary_gpu import _gt, _logits, _main, voc  # noqa: F401  (voc: the module-scoped fixture)

pytestmark = pytest.mark.gpu

SWEEP, BINS = "0.5:4:5", 10
COLS = ("Seg_1", "Seg_2", "Seg_ens")


def test_calibration_of_every_column(dev, voc, capsys, tmp_path):
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    root, run, names, argv = voc
    plain, out0, last0 = _main(argv, capsys)
    assert len(plain) == 2 and all("calibration" not in s for s in plain)
    assert "calibration" not in out0 and "ECE" not in out0 and sorted(last0) == ["Seg_1 mIoU", "Seg_2 mIoU", "next"]
    path = tmp_path / "calib.json"
    flags = ["--calibration", "1", "--calib_bins", str(BINS), "--temp_sweep", SWEEP, "--calib_json", str(path)]
    two, out2, _ = _main(argv + flags, capsys)
    # the flag adds its lines and its keys and changes nothing else
    kept = [ln for ln in out2.splitlines()[:-1] if not ln.startswith("calibration ")]
    assert kept == out0.splitlines()[:-1] and len(two) == 2 and two[0]["miou"] == plain[0]["miou"]
    assert {k: v for k, v in two[1].items() if k != "calibration"}.keys() == plain[1].keys()
    sc, out1, last1 = _main(argv + flags + ["--ensemble", "1"], capsys)
    temps = eval_seg.parse_temp_sweep(SWEEP)
    assert temps == (1.0, 0.5, 0.840896415254, 1.41421356237, 2.37841423001, 4.0)
    cms = [evaluate.CalibrationMatrix(21, dev, temperatures=temps, nbins=BINS) for _ in range(3)]
    for nm in names:
        z, gt = _logits(run, nm, dev), torch.from_numpy(_gt(root, nm)).to(dev)
        assert z[0].shape[-2:] == gt.shape                                       # VOC: the identity form
        cms[0].update(gt, z[0])
        cms[1].update(gt, z[1])
        cms[2].update(gt, z[0], z[1])
    written = json.load(open(path))
    assert sorted(written) == sorted(COLS)
    for k, col in enumerate(COLS):
        want = eval_seg.calibration_scores(cms[k])
        got = sc[k]["calibration"]
        np.testing.assert_equal(got, want)
        one = want["scores"][0]
        assert one["T"] == 1.0 and one["n"] > 0 and one["acc"] == pytest.approx(sc[k]["pAcc"], abs=1e-12)
        assert 0.0 <= one["ece"] <= one["mce"] <= 1.0 and one["nll"] > 0 and 0 < one["brier"] < 2 and 1 / 21 <= one["mean_conf"] <= 1
        assert sum(r["n"] for r in one["reliability"]) == one["n"] == sum(c["n"] for c in one["classes"].values())
        assert last1[col + " ECE"] == one["ece"] and f"calibration {col}: ECE {one['ece']:.4f} MCE " in out1
        assert written[col]["scores"][0]["n"] == one["n"] and written[col]["best"]["T_grid"] == want["best"]["T_grid"]
        assert len(want["scores"]) == 6 and want["scores"][1]["ece"] != one["ece"]                 # the temperatures discriminate
    np.testing.assert_equal(two[0]["calibration"], sc[0]["calibration"])         # a student's column does not depend on --ensemble
    assert out1.index("calibration Seg_1:") > out1.index("mIoU")                 # under the existing table
    assert sorted(last1) == sorted(["Seg_1 mIoU", "Seg_2 mIoU", "Seg_ens mIoU", "agree", "Seg_1 ECE", "Seg_2 ECE", "Seg_ens ECE", "next"])


def test_the_crf_column_is_scored_at_T_1(dev, voc, capsys):
    from PIL import Image
    from dupl_amd import ops
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    from dupl_amd.utils.dcrf import DenseCRF
    root, run, names, argv = voc
    sc, out, last = _main(argv + ["--crf", "1", "--calibration", "1", "--temp_sweep", SWEEP], capsys)
    assert len(sc) == 3 and sc[2]["calibration"]["temperatures"] == [1.0] and len(sc[0]["calibration"]["temperatures"]) == 6
    branch = 0 if sc[0]["miou"] > sc[1]["miou"] else 1
    post = DenseCRF(iter_max=10, pos_xy_std=1, pos_w=1, bi_xy_std=121, bi_rgb_std=5, bi_w=4)
    cm = evaluate.CalibrationMatrix(21, dev, temperatures=(1.0,), nbins=15)
    for nm in names:
        image = np.array(Image.open(root / "JPEGImages" / (nm + ".jpg")).convert("RGB"))
        H, W, _ = image.shape
        Q = post.from_logits(torch.from_numpy(image).to(dev), ops.resize_bilinear(_logits(run, nm, dev)[branch], H, W)[0])
        cm.update(torch.from_numpy(_gt(root, nm)).to(dev), Q, is_prob=True)
    want = eval_seg.calibration_scores(cm)
    np.testing.assert_equal(sc[2]["calibration"], want)
    assert last["seg_crf ECE"] == want["scores"][0]["ece"] and f"calibration seg_crf: ECE {want['scores'][0]['ece']:.4f}" in out
    assert " | best" not in [ln for ln in out.splitlines() if ln.startswith("calibration seg_crf")][0]


def test_validate_coco_scores_the_up_sampling_form(dev, golden_dir):
    import os
    from dupl_amd.tools import eval_seg
    from dupl_amd.utils import evaluate
    from test_eval_gpu import _loader, _tiny_model
    model, _ = _tiny_model(dev)
    loader = _loader()
    g = np.load(os.path.join(golden_dir, "val_tiny.npz"))
    args = types.SimpleNamespace(scales=tuple(float(v) for v in g["coco_scales"]), crop_size=int(g["coco_size"]))
    cal = {"temperatures": (1.0, 2.0, 0.5), "nbins": 15}
    s1, s2 = eval_seg.validate_coco(model, loader, args, num_classes=21)
    assert "calibration" not in s1 and "calibration" not in s2
    sc = eval_seg.validate_coco(model, loader, args, num_classes=21, ensemble=True, calibration=cal)
    assert len(sc) == 3 and sc[0]["miou"] == s1["miou"] and sc[1]["miou"] == s2["miou"]
    cms = [evaluate.CalibrationMatrix(21, dev, **cal) for _ in range(3)]
    for data in loader:
        seg = eval_seg.msc_seg_logits_coco(model, data[1].to(dev), args.scales, args.crop_size)
        gt = data[2].to(dev)
        assert tuple(seg[0].shape[2:]) != tuple(gt.shape[1:])                    # low-resolution logits: the up-sampling form
        cms[0].update(gt, seg[0])
        cms[1].update(gt, seg[1])
        cms[2].update(gt, seg[0], seg[1])
    for k in range(3):
        np.testing.assert_equal(sc[k]["calibration"], eval_seg.calibration_scores(cms[k]))
        assert sc[k]["calibration"]["scores"][0]["acc"] == pytest.approx(sc[k]["pAcc"], abs=1e-12)


def test_predict_image_temperature(dev):
    from dupl_amd import ops
    from dupl_amd.datasets.device_loader import DeviceTransform
    from dupl_amd.tools import predict
    from dupl_amd.utils import evaluate
    from test_eval_gpu import _tiny_model
    model, _ = _tiny_model(dev)
    model.eval()
    H, W, scales = 75, 100, (1.0, 1.25)
    image = np.random.RandomState(3).randint(0, 256, size=(5, 7, 3)).astype(np.uint8).repeat(16, 0).repeat(16, 1)[:H, :W]
    inputs = DeviceTransform(dev).val_item(torch.from_numpy(np.ascontiguousarray(image)).to(dev))[None]
    seg = predict.msc_seg_logits_windowed(model, inputs, (H, W), scales, 0, 0, 8)
    inv = ops.inv_temperature(2.0)
    gt = torch.from_numpy(CR.gt_for(21, H, W, 9)).to(dev)
    for branch, chosen in (("1", (0,)), ("2", (1,)), ("ens", (0, 1))):
        base = predict.predict_image(model, image, scales=scales, branch=branch)
        same = predict.predict_image(model, image, scales=scales, branch=branch, temperature=1.0)
        assert torch.equal(base["label"], same["label"]) and KG.same_bits(base["conf"], same["conf"]) and torch.equal(base["stats"], same["stats"])
        hot = predict.predict_image(model, image, scales=scales, branch=branch, temperature=2.0)
        label, conf = ops.seg_decide(*[ops.scale_(seg[k].clone(), inv) for k in chosen])
        assert KG.same_bits(hot["conf"], conf) and torch.equal(hot["label"], label)
        assert float(hot["conf"].mean()) < float(base["conf"].mean())            # a temperature above 1 flattens the soft-max
        if branch != "ens":
            assert torch.equal(hot["label"], base["label"])                      # a single student's argmax does not move
        # what eval_seg --calibration 1 binned at T = 2 is this confidence, bit for bit
        cm = evaluate.CalibrationMatrix(21, dev, temperatures=(1.0, 2.0), nbins=15)
        cm.update(gt, *[seg[k] for k in chosen])
        for t, r in enumerate((base, hot)):
            b, c, s = CR.host_counters(r["label"].cpu().numpy(), r["conf"].cpu().numpy(), gt.cpu().numpy(), 21, 15)
            assert np.array_equal(cm.bins[t].cpu().numpy(), b) and np.array_equal(cm.cls[t].cpu().numpy(), c)
            assert cm.sums[t, :2].tolist() == s.tolist()
    with pytest.raises(ValueError, match="not a soft-max of these logits"):
        predict.predict_image(model, image, scales=scales, branch="1", crf=True, temperature=2.0)
    with pytest.raises(ValueError):
        predict.predict_image(model, image, scales=scales, branch="1", temperature=0.0)


def test_predict_command_line_records_the_temperature_only_when_given(dev, tmp_path):
    from PIL import Image
    from dupl_amd.tools import predict
    from test_eval_gpu import _tiny_model
    model, _ = _tiny_model(dev)
    ckpt = str(tmp_path / "checkpoint.pth")
    torch.save({"module." + k: v.detach().cpu() for k, v in model.state_dict().items()}, ckpt)
    img = tmp_path / "a.jpg"
    Image.fromarray(np.random.RandomState(4).randint(0, 256, size=(3, 4, 3)).astype(np.uint8).repeat(16, 0).repeat(16, 1)).save(img, quality=95)
    common = ["--model_path", ckpt, "--backbone", "tiny_test", "--input", str(img), "--scales", "1.0", "--branch", "1", "--save_conf", "1"]
    outs = {}
    for tag, extra in (("plain", []), ("one", ["--temperature", "1.0"]), ("two", ["--temperature", "2"])):
        predict.main(common + ["--out_dir", str(tmp_path / tag)] + extra)
        outs[tag] = json.load(open(tmp_path / tag / "summary.json"))
    assert "temperature" not in outs["plain"] and outs["one"]["temperature"] == 1.0 and outs["two"]["temperature"] == 2.0
    assert {k: v for k, v in outs["one"].items() if k != "temperature"} == outs["plain"]
    read = lambda tag, sub: (tmp_path / tag / sub / "a.png").read_bytes()
    for sub in ("labels", "overlay", "conf"):
        assert read("plain", sub) == read("one", sub)                            # at exactly 1.0 every file is byte-identical
    assert read("plain", "labels") == read("two", "labels") and read("plain", "conf") != read("two", "conf")
    m = lambda tag: outs[tag]["images"][0]["classes"][0]["mean_conf"]
    assert m("two") < m("plain")
    with pytest.raises(SystemExit, match="not a soft-max of these logits"):
        predict.main(common + ["--out_dir", str(tmp_path / "no"), "--temperature", "2", "--crf", "1"])
