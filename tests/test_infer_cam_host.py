"""Offline CAM inference (dupl_amd.tools.infer_cam, csrc/cam_eval.hip), the part that needs no GPU: the C ABI surface, the CLI
flags, the jet table, the (gt, class, k) -> T confusion matrices identity and the three small cam_helper functions."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

EXPORTS = ("dupl_cam_eval", "dupl_cam_overlay")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_header_declares_and_library_exports_the_cam_eval_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from dupl_amd import _lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in EXPORTS:
        assert name in protos, f"{name} is not declared in include/dupl_hip.h"
        assert hasattr(cdll, name), f"{name} is not exported by the library"
    assert protos["dupl_cam_eval"][0] is ctypes.POINTER(_lib.CamEvalDesc)
    assert protos["dupl_cam_overlay"][6] is ctypes.c_double and len(protos["dupl_cam_overlay"]) == 9
    assert _lib.lib().dupl_abi_version() == 4                     # additive exports: the ABI version stays
    hdr = open(_lib.HEADER).read()
    body = re.search(r"typedef struct dupl_cam_eval_desc \{(.*?)\} dupl_cam_eval_desc;", hdr, re.S).group(1)
    assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[0].split() == ["uint32_t", "struct_size"]
    fields = [n for n, _ in _lib.CamEvalDesc._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dupl_hip.h"\nint main(void) { printf("%zu", sizeof(dupl_cam_eval_desc));\n'
           + "".join(f'printf(" %zu", offsetof(dupl_cam_eval_desc, {n}));\n' for n in fields)
           + 'printf(" %d %d", DUPL_CAM_EVAL_MAX_T, DUPL_CAM_EVAL_MAX_C);\nreturn 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sz.c"), os.path.join(td, "sz")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(_lib.HEADER), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:-2] == [ctypes.sizeof(_lib.CamEvalDesc)] + [getattr(_lib.CamEvalDesc, n).offset for n in fields], got
    assert _lib.CamEvalDesc().struct_size == got[0]
    assert got[-2:] == [_lib.CAM_EVAL_MAX_T, _lib.CAM_EVAL_MAX_C] == [64, 255]


def test_parser_has_the_reference_flags_and_the_new_ones():
    from dupl_amd.tools import infer_cam
    a = vars(infer_cam.build_parser().parse_args([]))
    # tools/infer_cam_voc.py:22-35 of the reference (hard-coded: the reference tree is not part of this repository)
    assert a == {"bkg_thre": 0.5, "model_path": "your_model_path/checkpoint.pth", "backbone": "vit_base_patch16_224", "pooling": "gmp",
                 "data_folder": "your_voc_dir", "num_classes": 21, "ignore_index": 255, "infer_set": "train",
                 "list_folder": "datasets/voc", "branch": 1, "scales": "1.0,0.5,1.5", "sweep": "", "save_img": 1, "save_labels": 0}
    assert isinstance(a["bkg_thre"], float)
    assert infer_cam.parse_scales(a["scales"]) == (1.0, 0.5, 1.5)
    with pytest.raises(SystemExit):
        infer_cam.build_parser().parse_args(["--branch", "3"])
    assert [p for p in inspect.signature(infer_cam.infer_cams).parameters][:3] == ["model", "loader", "args"]
    assert list(inspect.signature(infer_cam.main).parameters) == ["argv"]


def test_sweep_thresholds():
    from dupl_amd.tools.infer_cam import sweep_thresholds
    f32 = lambda v: float(np.float32(v))
    assert sweep_thresholds("", 0.5) == ([0.5], 0)
    thr, at = sweep_thresholds("0.05:0.95:0.05", 0.5)
    assert len(thr) == 19 and thr[at] == 0.5 and thr == sorted(thr) and thr[0] == f32(0.05) and thr[-1] == f32(0.05 + 18 * 0.05)
    thr, at = sweep_thresholds("0.1:0.9:0.2", 0.45)                     # --bkg_thre is inserted when it is not a point
    assert thr == [f32(0.1), f32(0.1 + 0.2), f32(0.45), f32(0.5), f32(0.1 + 3 * 0.2), f32(0.1 + 4 * 0.2)] and at == 2
    for bad in ("0.5", "0.9:0.1:0.1", "0:1:0", "0:1.5:0.1", "a:b:c", "0:1:0.01"):
        with pytest.raises(SystemExit):
            sweep_thresholds(bad, 0.5)


def test_thresholds_are_validated_on_the_host():
    from dupl_amd import ops
    assert ops.check_thresholds([0.0, 0.5, 0.5, 1.0]).dtype == np.float32
    for bad in ([], [0.6, 0.5], [-0.1, 0.5], [0.5, 1.1], [float("nan")], list(np.linspace(0, 1, 65))):
        with pytest.raises(ValueError):
            ops.check_thresholds(bad)
    sig = inspect.signature(ops.cam_eval).parameters
    assert list(sig)[:8] == ["cam", "cls_label", "out_size", "thresholds", "gt", "hist", "label_at", "want_value"]
    assert [sig[k].default for k in ("gt", "hist", "label_at", "want_value")] == [None, None, None, False]
    sig = inspect.signature(ops.cam_overlay).parameters
    assert list(sig) == ["value", "inputs", "alpha"] and sig["inputs"].default is None and sig["alpha"].default == 0.6


def test_jet_table_is_matplotlibs():
    from dupl_amd import ops
    import sys
    mods = set(sys.modules)
    lut = ops.jet_lut()
    assert "matplotlib" not in set(sys.modules) - mods               # the product computes it from the segment data
    want = np.load(os.path.join(GOLDEN, "jet_lut.npy"))              # matplotlib 3.10.8: colormaps["jet"]._lut[:256, :3]
    assert want.shape == (256, 3) and want.dtype == np.float64 and lut.shape == (256, 3) and lut.dtype == np.float64
    assert np.array_equal((lut * 255).astype(np.uint8), (want * 255).astype(np.uint8))
    assert np.abs(lut - want).max() <= 4e-16
    # the image-less overlay: blending a colour with itself (infer_cam_voc.py:86) truncates to the colour's own byte
    assert np.array_equal((0.6 * (want * 255) + (1 - 0.6) * (want * 255)).astype(np.uint8), (want * 255).astype(np.uint8))
    try:
        import matplotlib
    except ImportError:
        return
    cm = matplotlib.colormaps["jet"]
    v = np.random.default_rng(0).random(20000).astype(np.float32)
    v[:3] = (0.0, 1.0, np.float32(255 / 256))
    idx = np.minimum((v * np.float32(256)).astype(np.int64), 255)    # the kernel's index rule
    assert np.array_equal((cm(v)[:, :3] * 255).astype(np.uint8), (lut[idx] * 255).astype(np.uint8))


def test_bins_expand_to_the_confusion_matrices_of_every_threshold():
    """The identity the kernel relies on: with ascending thresholds, k = #{t : thr[t] < v}, a pixel is foreground at t exactly when
    t < k -- against a brute-force loop over the thresholds with _fast_hist, values exactly equal to a threshold included."""
    from dupl_amd import ops
    from dupl_amd.utils.evaluate import _fast_hist
    rng = np.random.default_rng(3)
    nc, S, n = 7, 4, 5000
    slot_pred = np.array([2, 3, 5, 6])                               # label of a slot when foreground (class index + 1)
    for thr in (np.array([0.5], np.float32), np.linspace(0.05, 0.95, 19).astype(np.float32),
                np.array([0.0, 0.25, 0.25, 1.0], np.float32)):
        T = len(thr)
        v = rng.random(n).astype(np.float32)
        v[: n // 4] = rng.choice(thr, n // 4)                         # exact ties: v <= thr is background
        v[n // 4: n // 4 + 50] = 0.0
        s = rng.integers(0, S, n)
        gt = rng.integers(0, nc + 2, n)
        gt[gt >= nc] = 255                                            # outside [0, nc): skipped
        k = (thr[None, :] < v[:, None]).sum(1)
        bins = np.zeros((nc, S, T + 1), np.int64)
        ok = gt < nc
        np.add.at(bins, (gt[ok], s[ok], k[ok]), 1)
        got = ops.sweep_bins_to_hists(bins, slot_pred, T)
        for t in range(T):
            pred = np.where(v <= thr[t], 0, slot_pred[s])
            assert np.array_equal(got[t], _fast_hist(gt, pred, nc)), (T, t)
        assert got.sum() == T * ok.sum()


def test_threshold_sweep_surface():
    from dupl_amd.utils import evaluate
    sw = evaluate.ThresholdSweep(5, [0.25, 0.5], torch.device("cpu"))
    assert tuple(sw.hist.shape) == (2, 5, 5) and sw.hist.dtype == torch.int64 and sw.thresholds == [0.25, 0.5]
    sw.hist[0] = torch.eye(5, dtype=torch.int64) * 3 + 1
    sw.hist[1] = torch.eye(5, dtype=torch.int64) * 5 + 1
    sc = sw.scores()
    assert len(sc) == 2 and sc[0]["miou"] == evaluate.scores_from_hist(sw.hist[0].numpy())["miou"] < sc[1]["miou"]
    t, best = sw.best()
    assert t == 0.5 and best["miou"] == sc[1]["miou"]


def test_cam_helper_has_the_three_missing_functions():
    from dupl_amd.utils import cam_helper
    g = torch.Generator().manual_seed(0)
    cam = torch.rand((2, 4, 5, 6), generator=g)
    cls = torch.tensor([[1., 0., 1., 0.], [0., 0., 0., 1.]])
    valid = cam_helper.get_valid_cam(cam, cls)
    assert valid.dtype == cam.dtype and torch.equal(valid, cls.unsqueeze(-1).unsqueeze(-1).repeat([1, 1, 5, 6]) * cam)
    label = torch.randint(0, 5, (2, 5, 6), generator=g)
    box = torch.tensor([[1, 4, 0, 3], [0, 5, 2, 6]], dtype=torch.int16)
    out = cam_helper.ignore_img_box(label, box, 255)
    want = torch.ones_like(label) * 255
    for i, c in enumerate(box):
        want[i, c[0]:c[1], c[2]:c[3]] = label[i, c[0]:c[1], c[2]:c[3]]
    assert out.dtype == label.dtype and torch.equal(out, want)
    roi = cam_helper.cam_to_roi_mask2(cam, cls, hig_thre=0.7, low_thre=0.3)
    value = valid.max(dim=1)[0]
    want = torch.ones_like(value, dtype=torch.int16)
    want[value <= 0.3] = 0
    want[value >= 0.7] = 2
    assert roi.dtype == torch.int16 and torch.equal(roi, want) and set(roi.unique().tolist()) == {0, 1, 2}
    assert list(inspect.signature(cam_helper.cam_to_roi_mask2).parameters) == ["cam", "cls_label", "hig_thre", "low_thre"]
    assert list(inspect.signature(cam_helper.ignore_img_box).parameters) == ["label", "img_box", "ignore_index"]
