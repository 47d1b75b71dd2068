"""The host side of the two-student ensemble (ops.seg_ensemble, evaluate.EnsembleMatrix, eval_seg --ensemble / --crf_branch): the
float64 reference the GPU suite leans on is pinned against torch, the flags and what they refuse, the C descriptor and its mirror."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_ensemble_ref as R


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_is_interpolate_softmax_mean_in_float64(shape):
    """tests/seg_ensemble_ref.py (numpy, from the definition) == F.interpolate(bilinear, align_corners=False) -> softmax -> mean in
    float64, predictions included; the pixels whose top-2 margin of e is under MARGIN are the few the GPU suite may excuse."""
    C, h, w, H, W = shape
    a, b, gt, ref = R.case(shape)
    assert a.shape == (1, C, h, w) and b.shape == (1, C, h, w) and gt.shape == (H, W) and gt.dtype == torch.int64
    share255 = float((gt == 255).double().mean())
    assert set(np.unique(gt.numpy())) <= set(range(C)) | {255} and (H * W < 100 or 0.03 < share255 < 0.2)
    ups = [F.interpolate(t.double(), size=(H, W), mode="bilinear", align_corners=False)[0] for t in (a, b)]
    if (h, w) == (H, W):
        assert torch.equal(ups[0], a[0].double())                  # the identity: nothing is interpolated
    e = 0.5 * (torch.softmax(ups[0], 0) + torch.softmax(ups[1], 0))
    assert float((torch.from_numpy(ref["e"]) - e).abs().max()) <= 1e-13
    assert np.abs(ref["e"].sum(0) - 1.0).max() <= 1e-13
    assert np.array_equal(ref["pred1"], ups[0].argmax(0).numpy()) and np.array_equal(ref["pred2"], ups[1].argmax(0).numpy())
    top = e.topk(2, dim=0).values
    assert float((torch.from_numpy(ref["margin"]) - (top[0] - top[1])).abs().max()) <= 1e-13
    clear = ref["margin"] >= R.MARGIN
    assert np.array_equal(ref["pred"][clear], e.argmax(0).numpy()[clear])
    ties = int((~clear).sum())
    print(f"{shape}: {ties} of {H * W} pixels with a top-2 margin of e under {R.MARGIN}")
    assert ties == R.REF_TIES[R.SHAPES.index(shape)] and ties <= R.TIE_SHARE * H * W
    # the ensemble is not one of the students: a kernel that returned a student's prediction would be found out
    for k in ("pred1", "pred2"):
        if H * W >= 100:
            assert 0.3 < float((ref["pred"] != ref[k]).mean()) < 0.7


def test_flags_defaults_and_refusal():
    from dupl_amd.tools import eval_seg
    for ds in ("voc", "coco"):
        p = eval_seg.build_parser(ds)
        args = p.parse_args([])
        assert args.ensemble == 0 and args.crf_branch == "auto" and args.crf == 0 and args.save_logits == 1
        eval_seg.check_branch_args(args)                           # the defaults are served
        eval_seg.check_branch_args(p.parse_args(["--ensemble", "1", "--crf_branch", "ens"]))
        eval_seg.check_branch_args(p.parse_args(["--crf_branch", "2"]))
        with pytest.raises(SystemExit):
            p.parse_args(["--crf_branch", "3"])
        with pytest.raises(SystemExit):
            p.parse_args(["--ensemble", "2"])
    # refused by main before a device, a data set or a checkpoint is touched, and the message says what is missing
    for argv in (["--crf_branch", "ens"], ["--dataset", "coco", "--crf", "1", "--crf_branch", "ens", "--ensemble", "0"]):
        with pytest.raises(SystemExit) as ei:
            eval_seg.main(argv)
        assert "requires --ensemble 1" in str(ei.value) and "--crf_branch ens" in str(ei.value)


def test_crf_branch_choice():
    """auto without the ensemble is the rule main() had (student 1 only when strictly better); with it the highest mIoU of the
    three, the earliest of branch1, branch2, ens on equal mIoU; 1 / 2 / ens are taken as given."""
    from dupl_amd.tools.eval_seg import pick_crf_branch as pick
    m = lambda v: {"miou": v}
    for a, b in ((0.5, 0.4), (0.4, 0.5), (0.5, 0.5), (float("nan"), 0.5)):
        assert pick("auto", m(a), m(b)) == ("branch1" if a > b else "branch2")
    assert pick("auto", m(0.5), m(0.4), m(0.6)) == "ens"
    assert pick("auto", m(0.5), m(0.7), m(0.6)) == "branch2"
    assert pick("auto", m(0.7), m(0.7), m(0.7)) == "branch1"
    assert pick("auto", m(0.6), m(0.7), m(0.7)) == "branch2"
    assert pick("auto", m(0.7), m(0.6), m(0.7)) == "branch1"
    assert pick("1", m(0.1), m(0.9), m(0.9)) == "branch1" and pick("2", m(0.9), m(0.1)) == "branch2"
    assert pick("ens", m(0.9), m(0.1), m(0.0)) == "ens"


def test_header_prototype_lib_entry_and_descriptor_agree():
    import __graft_entry__ as ge
    ge.build()
    from dupl_amd import _lib
    protos = _lib.parse_header()
    assert protos["dupl_seg_ensemble"] == [ctypes.POINTER(_lib.SegEnsembleDesc), ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dupl_seg_ensemble")
    L = _lib.lib()
    assert L.dupl_abi_version() == 4                               # the export is additive
    assert L.dupl_seg_ensemble.raw.argtypes == protos["dupl_seg_ensemble"]
    fields = [n for n, _ in _lib.SegEnsembleDesc._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dupl_hip.h"\nint main(void) { printf("%zu %d", sizeof(dupl_seg_ensemble_desc), '
           'DUPL_SEG_ENSEMBLE_MAX_C); ' + " ".join(f'printf(" %zu", offsetof(dupl_seg_ensemble_desc, {n}));' for n in fields) +
           ' printf("\\n"); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sz.c"), os.path.join(td, "sz")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(_lib.HEADER), c, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.SegEnsembleDesc) == _lib.SegEnsembleDesc().struct_size
    assert out[1] == _lib.SEG_ENSEMBLE_MAX_C
    assert out[2:] == [getattr(_lib.SegEnsembleDesc, n).offset for n in fields]
