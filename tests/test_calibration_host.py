"""Confidence calibration, the host side (no GPU): the header, the export and the ctypes mirror of dupl_seg_calib; descriptors that
are refused before any launch; evaluate.CalibrationMatrix's arithmetic on hand-written counters; the --temp_sweep parser and the
new flags of eval_seg and predict; and what tests/calib_ref.py alone says about the inputs of tests/test_calibration_gpu.py -- the
share of pixels its float64 reference sets aside, and the planted temperature."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import calib_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_point():
    from dupl_amd import _lib
    L = _lib.lib()
    assert L.dupl_abi_version() == 4                                           # the export is additive
    assert "dupl_seg_calib" in L.protos and hasattr(L.cdll, "dupl_seg_calib")
    assert L.protos["dupl_seg_calib"][0] is ctypes.POINTER(_lib.SegCalibDesc)
    hdr = open(_lib.HEADER).read()
    for name, val in (("DUPL_SEG_CALIB_MAX_T", _lib.SEG_CALIB_MAX_T), ("DUPL_SEG_CALIB_MAX_BINS", _lib.SEG_CALIB_MAX_BINS),
                      ("DUPL_SEG_CALIB_MAX_C", _lib.SEG_CALIB_MAX_C)):
        assert f"#define {name} {val}\n" in hdr
    assert (_lib.SEG_CALIB_MAX_T, _lib.SEG_CALIB_MAX_BINS) == (16, 64)


def test_ctypes_mirror_has_the_c_structs_layout(tmp_path):
    from dupl_amd import _lib
    D = _lib.SegCalibDesc
    fields = ["is_prob", "T", "nbins", "a", "inv_temp", "sums"]
    prog, exe = tmp_path / "sz.c", tmp_path / "sz"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dupl_hip.h"\nint main(void) { printf("%zu", sizeof(dupl_seg_calib_desc));\n'
                    + "".join(f'printf(" %zu", offsetof(dupl_seg_calib_desc, {f}));\n' for f in fields) + "return 0; }\n")
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(["which", c], capture_output=True).returncode == 0
               or os.path.exists(c)), None)
    assert cc is not None, "no C compiler"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(D)] + [getattr(D, f).offset for f in fields] and got[0] == 96
    assert D().struct_size == ctypes.sizeof(D)


def _desc(inv=(1.0,), **over):
    """a descriptor that only the checked fields can make wrong: the pointers are non-null host addresses that are never followed
    (a refused descriptor launches nothing)"""
    from dupl_amd import _lib
    host = (ctypes.c_float * 32)(*inv)
    ptr = ctypes.cast(host, ctypes.c_void_p).value
    d = _lib.SegCalibDesc(C=21, h=37, w=53, H=37, W=53, is_prob=0, T=len(inv), nbins=15, a=ptr, b=None, gt=ptr, inv_temp=ptr,
                          bins=ptr, cls=ptr, sums=ptr)
    for k, v in over.items():
        setattr(d, k, v)
    return d, host


@pytest.mark.parametrize("inv, over", [
    ((1.0,), dict(struct_size=92)), ((1.0,), dict(struct_size=0)), ((1.0,), dict(T=0)), ((1.0,) * 17, dict()),
    ((1.0,), dict(nbins=0)), ((1.0,), dict(nbins=65)), ((1.0,), dict(is_prob=1, h=36)), ((1.0,), dict(is_prob=1, w=52)),
    ((1.0, 1.0), dict(is_prob=1)), ((0.5,), dict(is_prob=1)), ((0.0,), dict()), ((-1.0,), dict()), ((1.0, math.inf), dict()),
    ((1.0, math.nan), dict()), ((1.0,), dict(bins=None, cls=None, sums=None)), ((1.0,), dict(C=0)), ((1.0,), dict(C=256)),
    ((1.0,), dict(a=None)), ((1.0,), dict(gt=None)), ((1.0,), dict(inv_temp=None)), ((1.0,), dict(H=0)), ((1.0,), dict(reserved0=1)),
], ids=lambda v: (",".join(f"{k}={x}" for k, x in v.items()) or "-") if isinstance(v, dict) else f"inv{len(v)}:{v[-1]}")
def test_bad_descriptors_are_refused_before_any_launch(inv, over):
    from dupl_amd import _lib
    d, keep = _desc(inv, **over)
    assert _lib.lib().dupl_seg_calib.raw(ctypes.byref(d), None) == -1          # no GPU is needed to ask
    assert _lib.lib().dupl_seg_calib.raw(None, None) == -1


def test_inv_temperature_is_the_fp32_inverse():
    from dupl_amd import ops
    assert ops.inv_temperature(1.0) == 1.0 and ops.inv_temperature(2.0) == 0.5
    for T in (0.5, 0.594603557501, 1.68179283051, 3.0, 4.0):
        assert ops.inv_temperature(T) == float(np.float32(1.0) / np.float32(T)) == CR.inv_temperature(T)
        assert np.float32(ops.inv_temperature(T)) == ops.inv_temperature(T)    # exactly an fp32 value
    for bad in (0.0, -2.0, math.inf, math.nan, 1e-45, 1e39):
        with pytest.raises(ValueError):
            ops.inv_temperature(bad)


def _filled(nc, temps, nbins, bins=None, cls=None, sums=None):
    from dupl_amd.utils import evaluate
    cm = evaluate.CalibrationMatrix(nc, "cpu", temperatures=temps, nbins=nbins)
    assert cm.bins.shape == (len(temps), nbins, 3) and cm.cls.shape == (len(temps), nc, 3) and cm.sums.shape == (len(temps), 4)
    assert all(t.dtype == torch.int64 for t in cm.tensors())
    for t, v in ((cm.bins, bins), (cm.cls, cls), (cm.sums, sums)):
        if v is not None:
            t.copy_(torch.as_tensor(np.asarray(v, dtype=np.int64)).reshape(t.shape))
    return cm


Q = 1 << 24


def test_a_perfectly_calibrated_table_has_ece_zero():
    # 4 bins; in every bin the accuracy equals the mean confidence: 1/8, 3/8, 5/8, 7/8
    bins = [[[8, 1, 8 * Q // 8], [8, 3, 3 * Q], [16, 10, 10 * Q], [8, 7, 7 * Q]]]
    s = _filled(2, (1.0,), 4, bins=bins, sums=[[40, 21, 0, 0]]).scores()[0]
    assert s["ece"] == 0.0 and s["mce"] == 0.0 and s["acc"] == 21 / 40 and s["mean_conf"] == pytest.approx(21 / 40) and s["n"] == 40
    assert [r["n"] for r in s["reliability"]] == [8, 8, 16, 8] and s["reliability"][2] == {"n": 16, "acc": 0.625, "conf": 0.625}


def test_two_bins_by_hand_empty_bins_and_classes():
    # bin 0 empty; bin 1: 10 pixels, 4 right, mean conf 0.6 -> gap 0.2; bin 2: 30 pixels, 27 right, mean conf 0.8 -> gap 0.1
    bins = [[[0, 0, 0], [10, 4, 6 * Q], [30, 27, 24 * Q]]]
    cls = [[[40, 31, 30 * Q], [0, 0, 0]]]
    sums = [[40, 31, 20 << 20, 10 * Q]]
    s = _filled(2, (1.0,), 3, bins, cls, sums).scores()[0]
    assert s["ece"] == pytest.approx(10 / 40 * 0.2 + 30 / 40 * 0.1) and s["mce"] == pytest.approx(0.2)
    assert s["nll"] == 0.5 and s["brier"] == 0.25 and s["acc"] == 31 / 40 and s["mean_conf"] == pytest.approx(0.75)
    assert math.isnan(s["reliability"][0]["acc"]) and math.isnan(s["reliability"][0]["conf"]) and s["reliability"][0]["n"] == 0
    rc = s["risk_coverage"]
    assert [r["min_conf"] for r in rc] == [0.0, 1 / 3, 2 / 3]
    assert [r["coverage"] for r in rc] == [1.0, 1.0, 0.75] and [r["acc"] for r in rc] == [31 / 40, 31 / 40, 27 / 30]
    assert s["classes"][0] == {"n": 40, "precision": 31 / 40, "mean_conf": 0.75}
    assert s["classes"][1]["n"] == 0 and math.isnan(s["classes"][1]["precision"]) and math.isnan(s["classes"][1]["mean_conf"])
    # nothing counted at all: nan everywhere, no division error
    e = _filled(2, (1.0, 2.0), 3).scores()
    assert len(e) == 2 and e[1]["T"] == 2.0
    assert all(math.isnan(e[0][k]) for k in ("ece", "mce", "nll", "brier", "acc", "mean_conf")) and math.isnan(e[0]["risk_coverage"][2]["acc"])
    from dupl_amd.utils import evaluate
    assert math.isnan(evaluate.CalibrationMatrix(2, "cpu", (1.0, 2.0)).best_temperature()["T_grid"])


def _with_nll(temps, nll):
    return _filled(2, temps, 2, sums=[[1 << 10, 0, int(round(v * (1 << 30))), 0] for v in nll])


def test_best_temperature_parabola_and_edges():
    # y = 3 + (x - ln 1.5)^2 sampled at ln 1, ln 2, ln 4: the vertex is T = 1.5, the grid minimum T = 2 ((ln 2 - ln 1.5)^2 is the least)
    temps = (1.0, 4.0, 2.0)
    best = _with_nll(temps, [3 + (math.log(t) - math.log(1.5)) ** 2 for t in temps]).best_temperature()
    assert best["T_grid"] == 2.0 and best["at_edge"] is False and best["index"] == 2 and best["T_fit"] == pytest.approx(1.5, rel=1e-6)
    # unevenly spaced in log T (T = 1 sits inside a geometric grid): still the vertex
    temps = (1.0, 0.5, 1.3, 3.0)
    best = _with_nll(temps, [2 + 0.7 * (math.log(t) - math.log(1.1)) ** 2 for t in temps]).best_temperature()
    assert best["T_grid"] == 1.0 and best["T_fit"] == pytest.approx(1.1, rel=1e-6) and not best["at_edge"]
    # the minimum at either end of the grid: T_fit is T_grid and the caller is told
    for nll, want in (([3.0, 2.0, 4.0], 0.5), ([3.0, 5.0, 2.5], 4.0)):
        best = _with_nll((1.0, 0.5, 4.0), nll).best_temperature()
        assert best == {"T_grid": want, "T_fit": want, "at_edge": True, "index": (1.0, 0.5, 4.0).index(want)}
    assert _with_nll((1.0,), [1.0]).best_temperature()["at_edge"] is True
    # equal NLL: the lowest temperature
    assert _with_nll((0.5, 1.0, 2.0), [3.0, 3.0, 3.0]).best_temperature()["T_grid"] == 0.5
    # the independent implementation of tests/calib_ref.py agrees
    temps = (1.0, 0.5, 0.7, 1.4, 2.0, 2.8, 4.0)
    nll = [2.6, 4.2, 3.2, 2.27, 2.19, 2.25, 2.38]
    best = _with_nll(temps, nll).best_temperature()
    Tg, Tf, edge = CR.best_temperature(temps, nll)
    assert (best["T_grid"], best["at_edge"]) == (Tg, edge) and best["T_fit"] == pytest.approx(Tf, rel=1e-6)


def test_calibration_matrix_refuses_what_one_pass_cannot_take():
    from dupl_amd.utils import evaluate
    for kw in (dict(temperatures=(1.0,) * 17), dict(temperatures=()), dict(nbins=0), dict(nbins=65), dict(temperatures=(1.0, 0.0)),
               dict(temperatures=(1.0, math.inf))):
        with pytest.raises(ValueError):
            evaluate.CalibrationMatrix(21, "cpu", **kw)


def test_temp_sweep_parser():
    import argparse
    from dupl_amd.tools import eval_seg
    sweep = eval_seg.parse_temp_sweep("0.5:4:13")
    assert sweep[0] == 1.0 and len(sweep) == 13 and sweep.count(1.0) == 1 and 2.0 in sweep and sweep[1] == 0.5 and sweep[-1] == 4.0
    grid = sorted(sweep)
    ratios = [b / a for a, b in zip(grid, grid[1:])]
    assert max(ratios) / min(ratios) == pytest.approx(1.0, abs=1e-9)           # T = 1 falls on this grid: geometric throughout
    odd = eval_seg.parse_temp_sweep("0.3:3:15")
    assert odd[0] == 1.0 and len(odd) == 16 and list(odd[1:]) == sorted(odd[1:]) and odd[1] == 0.3 and odd[-1] == 3.0
    r = [b / a for a, b in zip(odd[1:], odd[2:])]
    assert max(r) / min(r) == pytest.approx(1.0, abs=1e-9)
    for bad in ("0.5:4:16", "0.5:4:1", "4:0.5:5", "0:4:5", "-1:4:5", "0.5:4", "a:b:c", "0.5:inf:4", "1:1:3"):
        with pytest.raises(argparse.ArgumentTypeError):
            eval_seg.parse_temp_sweep(bad)


def test_eval_seg_flags_and_neutral_defaults():
    from dupl_amd.tools import eval_seg
    for ds in ("voc", "coco"):
        p = eval_seg.build_parser(ds)
        a = p.parse_args([])
        assert a.calibration == 0 and a.calib_bins == 15 and a.calib_json is None and a.temp_sweep == eval_seg.parse_temp_sweep("0.5:4:13")
        assert eval_seg.calibration_spec(a) is None
        eval_seg.check_branch_args(a)
        a = p.parse_args(["--calibration", "1", "--calib_bins", "20", "--temp_sweep", "1:3:3", "--calib_json", "c.json"])
        assert eval_seg.calibration_spec(a) == {"temperatures": (1.0, 1.73205080757, 3.0), "nbins": 20} and a.calib_json == "c.json"
        for bad in (["--calibration", "2"], ["--temp_sweep", "0.5:4:16"], ["--calib_bins", "x"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)
        for bins in ("0", "65"):
            with pytest.raises(SystemExit, match="calib_bins"):
                eval_seg.check_branch_args(p.parse_args(["--calib_bins", bins]))


def test_format_calibration_and_scores_dict():
    from dupl_amd.tools import eval_seg
    temps = (1.0, 0.5, 2.0, 4.0)
    cm = _filled(2, temps, 3, bins=[[[0, 0, 0], [10, 4, 6 * Q], [30, 27, 24 * Q]]] * 4, cls=[[[40, 31, 30 * Q], [0, 0, 0]]] * 4,
                 sums=[[40, 31, int(v * 40) << 20, 10 * Q] for v in (3, 5, 2, 4)])
    c = eval_seg.calibration_scores(cm)
    assert sorted(c) == ["best", "nbins", "scores", "temperatures"] and c["temperatures"] == list(temps) and c["nbins"] == 3
    assert len(c["scores"]) == 4 and c["best"]["T_grid"] == 2.0 and not c["best"]["at_edge"]
    line = eval_seg.format_calibration([{"calibration": c}], ["Seg_1"])
    assert line.startswith("calibration Seg_1: ECE 0.1250 MCE 0.2000 NLL 3.0000 Brier 0.2500 conf 0.7500 acc 0.7750 at T=1 | best T 2 (fit ")
    assert "NLL 2.0000" in line and "widen" not in line and "\n" not in line
    edge = eval_seg.calibration_scores(_filled(2, (1.0, 2.0), 3, sums=[[40, 31, 3 * 40 << 20, 0], [40, 31, 2 * 40 << 20, 0]]))
    assert "widen --temp_sweep" in eval_seg.format_calibration([{"calibration": edge}], ["Seg_2"])
    one = eval_seg.calibration_scores(_filled(2, (1.0,), 3, sums=[[40, 31, 3 * 40 << 20, 0]]))
    assert " | best" not in eval_seg.format_calibration([{"calibration": one}], ["seg_crf"])     # the CRF column: T = 1 only


def test_predict_flags():
    from dupl_amd.tools import predict
    base = ["--input", "x.jpg", "--out_dir", "o"]
    a = predict.parse_args(base)
    assert a.temperature == 1.0 and a.temperature_given is False
    a = predict.parse_args(base + ["--temperature", "2"])
    assert a.temperature == 2.0 and a.temperature_given is True
    assert predict.parse_args(base + ["--temperature", "1.0", "--crf", "1"]).temperature_given is True       # 1.0 changes nothing: allowed
    with pytest.raises(SystemExit, match="not a soft-max of these logits"):
        predict.parse_args(base + ["--temperature", "2", "--crf", "1"])
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--temperature"):
            predict.parse_args(base + ["--temperature", bad])


@pytest.mark.parametrize("nbins", (15, 64))
def test_the_reference_alone_sets_few_pixels_aside(nbins):
    """The committed seeds of the GPU test's float64 cases: the share of pixels that are ambiguous to the reference itself, asserted
    here so that the GPU test cannot hide behind its cap.  Measured: at most 0.31 % (81 channels, 7 x 9 -> 37 x 53, two students,
    64 bins); most cases 0 - 0.2 %."""
    worst = 0.0
    for shape, students, is_prob in CR.F64_CASES:
        *_, ref, share = CR.f64_case(shape, students, is_prob, nbins)
        assert share <= CR.AMBIGUOUS_CAP, (shape, students, is_prob, nbins, share)
        assert not ref["ambiguous"].any() or share > 0                          # the second pass runs on the cleaned gt
        worst = max(worst, share)
    print(f"nbins {nbins}: worst share set aside {100 * worst:.3f} %")
    assert worst <= 0.0035


def test_the_planted_temperature_in_float64():
    """What the GPU test asserts of the kernel, first of the reference: gt drawn from softmax(z / 2) is best explained at T = 2."""
    from dupl_amd.tools import eval_seg
    temps = eval_seg.parse_temp_sweep("0.5:4:13")
    (z,), gt = CR.planted(1)
    ref = CR.reference(z, None, CR.PLANTED[1:], gt, temps, 15)
    nll = ref["sums"][:, 2] / ref["sums"][:, 0]
    Tg, Tf, edge = CR.best_temperature(temps, nll)
    i2 = temps.index(2.0)
    assert Tg == 2.0 and not edge and 1.68 <= Tf <= 2.38
    assert nll[i2] + 0.01 < min(nll[temps.index(1.68179283051)], nll[temps.index(2.37841423001)])     # four orders above the NLL bar
    assert CR.ece(ref["bins"][0]) > 0.2 and CR.ece(ref["bins"][i2]) < 0.05
