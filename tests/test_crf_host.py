"""DenseCRF post-processing, the part that needs no GPU: the C ABI surface, the reference's module surface (utils/dcrf.py), the
CLI flag, and the fp64 brute-force reference of tests/crf_ref.py checked against itself -- including the proof that the
seeded inputs of the GPU tests are non-trivial and nearly tie-free."""
import ctypes
import inspect
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import crf_ref as R

EXPORTS = ("dupl_crf_message", "dupl_dense_crf", "dupl_crf_unary", "dupl_crf_unary_labels")


def test_header_declares_and_library_exports_the_crf_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from dupl_amd import _lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in EXPORTS:
        assert name in protos, f"{name} is not declared in include/dupl_hip.h"
        assert hasattr(cdll, name), f"{name} is not exported by the library"
    assert protos["dupl_crf_message"][0] is ctypes.POINTER(_lib.CrfDesc) and protos["dupl_dense_crf"][0] is ctypes.POINTER(_lib.CrfDesc)
    assert _lib.lib().dupl_abi_version() == 4                     # additive exports: the ABI version stays
    # the descriptor is plain C with struct_size first, and the ctypes mirror has the C compiler's layout
    hdr = open(_lib.HEADER).read()
    body = re.search(r"typedef struct dupl_crf_desc \{(.*?)\} dupl_crf_desc;", hdr, re.S).group(1)
    assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[0].split() == ["uint32_t", "struct_size"]
    fields = [n for n, _ in _lib.CrfDesc._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dupl_hip.h"\nint main(void) { printf("%zu", sizeof(dupl_crf_desc));\n'
           + "".join(f'printf(" %zu", offsetof(dupl_crf_desc, {n}));\n' for n in fields) + "return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sz.c"), os.path.join(td, "sz")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(_lib.HEADER), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.CrfDesc)] + [getattr(_lib.CrfDesc, n).offset for n in fields], got
    assert _lib.CrfDesc().struct_size == got[0]


def test_dcrf_module_has_the_reference_surface():
    """utils/dcrf.py:7,26,42-43,51 of the reference: names, parameter names and defaults (hard-coded: the reference tree is not
    part of this repository)."""
    from dupl_amd.utils import dcrf

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert sig(dcrf.crf_inference) == [("img", E), ("probs", E), ("t", 10), ("scale_factor", 1), ("labels", 21)]
    assert sig(dcrf.crf_inference_label) == [("img", E), ("labels", E), ("t", 10), ("n_labels", 21), ("gt_prob", 0.7)]
    assert sig(dcrf.DenseCRF.__init__) == [("self", E), ("iter_max", E), ("pos_w", E), ("pos_xy_std", E), ("bi_w", E),
                                           ("bi_xy_std", E), ("bi_rgb_std", E)]
    assert sig(dcrf.DenseCRF.__call__) == [("self", E), ("image", E), ("probmap", E)]
    p = dcrf.DenseCRF(10, 1, 1, 4, 121, 5)
    assert (p.iter_max, p.pos_w, p.pos_xy_std, p.bi_w, p.bi_xy_std, p.bi_rgb_std) == (10, 1, 1, 4, 121, 5)
    doc = dcrf.__doc__.lower()
    assert "exact" in doc and "lattice" in doc and "compared" in doc          # the module says what it is and is not


def test_ops_surface():
    from dupl_amd import ops
    assert list(inspect.signature(ops.crf_message).parameters)[:4] == ["img", "Q", "sxy", "srgb"]
    assert inspect.signature(ops.crf_message).parameters["normalize"].default is True
    assert list(inspect.signature(ops.dense_crf).parameters) == ["unary", "img_u8", "T", "w_g", "sxy_g", "w_b", "sxy_b", "srgb_b"]


def test_eval_seg_has_the_crf_flag_and_refuses_it_without_logits():
    from dupl_amd.tools import eval_seg
    for ds in ("voc", "coco"):
        a = eval_seg.build_parser(ds).parse_args([])
        assert a.crf == 0 and a.save_logits == 1
        assert eval_seg.build_parser(ds).parse_args(["--crf", "1"]).crf == 1
    with pytest.raises(SystemExit) as e:
        eval_seg.main(["--crf", "1", "--save_logits", "0"])
    assert "save_logits" in str(e.value)
    assert "stays outside this package" not in eval_seg.__doc__


def test_encode_cmap_is_the_voc_palette():
    from dupl_amd.utils import imutils
    want = {0: (0, 0, 0), 1: (128, 0, 0), 2: (0, 128, 0), 3: (128, 128, 0), 4: (0, 0, 128), 8: (64, 0, 0), 15: (192, 128, 128),
            20: (0, 64, 128), 255: (224, 224, 192)}
    lab = np.array([list(want)], dtype=np.int64)
    out = imutils.encode_cmap(lab)
    assert out.shape == (1, len(want), 3) and out.dtype == np.uint8
    assert [tuple(int(v) for v in px) for px in out[0]] == list(want.values())


def test_reference_unaries_follow_their_formulas():
    g = torch.Generator().manual_seed(0)
    p = torch.softmax(4 * torch.randn((5, 3, 4), generator=g), 0)
    p[0, 0, 0], p[1, 0, 0] = 0.0, 1.0
    U = R.unary_from_softmax(p)
    assert U.dtype == torch.float32
    for c in range(5):
        for y in range(3):
            for x in range(4):
                assert U[c, y, x].item() == np.float32(-math.log(min(max(float(p[c, y, x]), 1e-5), 1.0))) or \
                    abs(U[c, y, x].item() + math.log(min(max(float(p[c, y, x]), 1e-5), 1.0))) < 1e-6
    assert abs(U[0, 0, 0].item() + math.log(1e-5)) < 1e-5 and U[1, 0, 0].item() == 0.0
    lab = torch.randint(0, 5, (3, 4), generator=g)
    U = R.unary_from_labels(lab, 5, 0.7)
    for c in range(5):
        for y in range(3):
            for x in range(4):
                want = -math.log(0.7) if int(lab[y, x]) == c else -math.log(0.3 / 4)
                assert abs(U[c, y, x].item() - want) < 1e-6


def test_reference_is_consistent_with_itself():
    img, _, logits = R.make_case(9, 13, 5, seed=3)
    U = R.unary_from_softmax(torch.softmax(logits, 0))
    # weights 0 (or no iteration): softmax(-U)
    for Q in (R.mean_field(img, U, 3, 0.0, 1.0, 0.0, 121.0, 5.0), R.mean_field(img, U, 0, 1.0, 1.0, 4.0, 121.0, 5.0)):
        assert torch.equal(Q, torch.softmax(-U.double(), 0))
    # M_k is symmetric: sum_i a_i M(b)_i = sum_i b_i M(a)_i, for both kernels, with and without normalisation
    g = torch.Generator().manual_seed(1)
    a, b = torch.rand((1, 9 * 13), generator=g).double(), torch.rand((1, 9 * 13), generator=g).double()
    for im, sxy, srgb in ((None, 1.0, 1.0), (img, 121.0, 5.0), (img, 80.0, 13.0)):
        f = R.features(9, 13, im, sxy, srgb, torch.float64)
        K = R.kernel_rows(f)
        assert torch.equal(K.diagonal(), torch.ones(9 * 13, dtype=torch.float64))          # j = i is part of the sum
        for n in (None, R.norm_of(K)):
            lhs, rhs = float((a * R.message(K, b, n)).sum()), float((b * R.message(K, a, n)).sum())
            assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
        # the chunked row evaluation is the full one
        rows = torch.tensor([0, 5, 116, 60])
        n = R.norm_of(K)
        assert torch.allclose(R.message_rows(f, b, rows, n, chunk=3), R.message(K, b, n)[:, rows], rtol=1e-13, atol=0)
        assert torch.allclose(R.rowsum_rows(f, rows, chunk=3), K.sum(1)[rows], rtol=1e-13, atol=0)


@pytest.mark.parametrize("H,W,C", R.CASES)
@pytest.mark.parametrize("pset", sorted(R.PARAMS))
def test_seeded_inputs_are_non_trivial_and_nearly_tie_free(H, W, C, pset):
    """What tests/test_crf_gpu.py relies on, shown on the fp64 reference alone: the CRF changes the argmax of a sizeable share of
    the pixels (the inputs exercise the update), at most REF_TIE_SHARE of the pixels have an fp64 top-2 margin under MARGIN (the
    label comparison excuses only those), and a plain fp32 evaluation of the same formulas reproduces the fp64 labels
    everywhere else."""
    img, _, logits = R.make_case(H, W, C, seed=R.case_seed(H, W))
    p = torch.softmax(logits, 0)
    U = R.unary_from_softmax(p)
    Q64 = R.mean_field(img, U, 10, **R.PARAMS[pset])
    Q32 = R.mean_field(img, U, 10, dtype=torch.float32, **R.PARAMS[pset])
    changed = float((Q64.argmax(0) != p.argmax(0)).float().mean())
    close = R.top2_margin(Q64) < R.MARGIN
    err32 = float((Q32.double() - Q64).abs().max())
    print(f"({H},{W},{C}) {pset}: argmax changed at {100 * changed:.1f} % of the pixels, {100 * float(close.float().mean()):.3f} % "
          f"with margin < {R.MARGIN}, fp32-vs-fp64 max |dQ| {err32:.2e}")
    assert changed > 0.02
    assert float(close.float().mean()) <= R.REF_TIE_SHARE
    assert bool(((Q32.argmax(0) == Q64.argmax(0)) | close).all())
    assert err32 < 1e-4
