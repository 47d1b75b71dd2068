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


# ---------------------------------------------------------------------------- what tests/test_crf_edges_gpu.py relies on
def test_gauss_radius_restatement_against_hand_values():
    """sigma = 1: ln(2 pi + 1) = 1.98555, + 32 ln 2 = 22.18071 -> 24.16626, x 2 = 48.33252, sqrt = 6.95216 -> R = 7, a 15 x 15
    window (225 pixels).  sigma = 3: ln(18 pi + 1) = 4.05264 -> 26.23335, x 2 = 52.46670, sqrt = 7.24339, x 3 = 21.7302 -> R = 22,
    a 45 x 45 window (2025 pixels).  The mass outside the disc is below 2^-32 at R and not at R - 1."""
    assert R.gauss_radius(1.0) == 7 and R.gauss_radius(3.0) == 22
    assert abs(math.sqrt(2 * (1.98555 + 22.18071)) - 6.95216) < 1e-4 and abs(3 * math.sqrt(2 * (4.05264 + 22.18071)) - 21.7302) < 1e-3
    for s in (1.0, 3.0, 0.5, 10.0):
        r = R.gauss_radius(s)
        assert 2 * math.pi * s * s * math.exp(-r * r / (2 * s * s)) < 2.0 ** -32
        assert 2 * math.pi * s * s * math.exp(-(r - 2) ** 2 / (2 * s * s)) > 2.0 ** -32      # ceil and the "+ 1" cost under 2 pixels
    assert R.gauss_radius(1e6) == 1000000 and R.gauss_radius(3e38) == 1000000 and R.gauss_radius(1e-25) == 1
    # the shapes of the GPU test on either side of win^2 = N
    assert not R.gauss_takes_stencil(15, 15, 1.0)                                             # 225 < 225 is false: dense
    assert R.gauss_takes_stencil(2, 113, 1.0) and R.gauss_takes_stencil(226, 1, 1.0) and R.gauss_takes_stencil(33, 33, 1.0)
    assert not R.gauss_takes_stencil(40, 25, 3.0)
    assert 33 > 2 * 7 + 1                                                                     # 33 x 33 has unclipped windows
    assert all(not R.gauss_takes_stencil(H, W, 3.0) for H, W in R.SEAM_SHAPES)
    assert all(R.gauss_takes_stencil(9, 13, s) for s in R.EXTREME_STD[:3]) and not any(R.gauss_takes_stencil(9, 13, s) for s in R.EXTREME_STD[3:])


def test_seam_shapes_have_the_pixel_counts_they_are_named_for():
    assert tuple(H * W for H, W in R.SEAM_SHAPES) == R.SEAM_N
    assert {(3, 43), (15, 17), (16, 16), (19, 27)} <= set(R.SEAM_SHAPES)
    assert any(H == 1 for H, W in R.SEAM_SHAPES) and any(W == 1 for H, W in R.SEAM_SHAPES)


def test_wide_range_q_spans_thirty_decades():
    Q = R.wide_range_q(21, 24, 40, seed=5)
    tiny = float(np.finfo(np.float32).tiny)
    assert Q.dtype == torch.float32 and Q.shape == (21, 960) and bool((Q >= 0).all())
    print(f"wide_range_q: {R.decades(Q):.1f} decades, {int(((Q > 0) & (Q < tiny)).sum())} denormals, {int((Q == 0).sum())} zeros")
    assert R.decades(Q) >= 30.0
    assert int(((Q > 0) & (Q < tiny)).sum()) >= 10                          # denormals included
    assert bool((Q[1] == 0).all()) and bool((Q[0] > 0).any())
    assert float((Q.double().sum(0) - 1).abs().max()) < 1e-6
    # within single pixels too, not only across the image: the median pixel's own entries span 30 decades
    pos = torch.where(Q > 0, Q.double(), torch.ones((), dtype=torch.float64))
    assert float(torch.log10(Q.double().amax(0) / pos.amin(0)).median()) >= 30.0


def test_ulp_distance_and_exact_unary():
    one, nxt = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    a = torch.tensor([0.0, -0.0, one, one, -one, 1e-45, 3.0])
    b = torch.tensor([-0.0, 0.0, nxt, np.nextafter(nxt, np.float32(2.0)), -nxt, -1e-45, 3.0])
    assert R.ulp_distance(a, b).tolist() == [0, 0, 1, 2, 1, 2, 0]
    lo = np.float32(1e-5)
    p = torch.tensor([0.0, 1e-45, 1e-6, np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1)), 0.5, 1.0, 1.5])
    U = R.unary_exact(p)
    at_lo = np.float32(-math.log(float(lo)))
    assert U.dtype == torch.float32 and U[:5].tolist() == [float(at_lo)] * 5 and float(U[5]) <= float(at_lo)
    assert float(R.unary_exact(torch.tensor([1.1e-5]))) == float(np.float32(-math.log(float(np.float32(1.1e-5))))) < float(at_lo)
    assert float(U[6]) == float(np.float32(math.log(2.0))) and U[7:].tolist() == [0.0, 0.0]
    lab = torch.tensor([[-1, 0, 1, 2, 255]])
    Ul = R.unary_from_any_labels(lab, 2, 0.999)
    g, o = float(np.float32(-math.log(0.999))), float(np.float32(-math.log(0.001)))
    assert Ul.tolist() == [[o, g, o, o, o], [o, o, g, o, o]]
    assert torch.equal(R.unary_from_any_labels(torch.tensor([[0, 1, 1]]), 2, 0.5), R.unary_from_labels(torch.tensor([[0, 1, 1]]), 2, 0.5).reshape(2, -1))


@pytest.mark.parametrize("H,W,C", R.BRANCH_CASES)
def test_zero_weight_cases_are_tie_free(H, W, C):
    """The dense_crf cases with a zero weight (tests/test_crf_edges_gpu.py), on the fp64 reference alone: the share of pixels
    with a top-2 margin under MARGIN stays under REF_TIE_SHARE, a plain fp32 evaluation has the fp64 labels, and each kernel on
    its own still changes labels."""
    img, _, logits = R.make_case(H, W, C, seed=R.branch_seed(H, W, C))
    prob = torch.softmax(logits, 0)
    U = R.unary_from_softmax(prob)
    p = R.PARAMS["eval"]
    for w_g, w_b in R.BRANCH_WEIGHTS:
        Q64 = R.mean_field(img, U, R.BRANCH_T, w_g, p["sxy_g"], w_b, p["sxy_b"], p["srgb_b"])
        Q32 = R.mean_field(img, U, R.BRANCH_T, w_g, p["sxy_g"], w_b, p["sxy_b"], p["srgb_b"], dtype=torch.float32)
        close = R.top2_margin(Q64) < R.MARGIN
        changed = float((Q64.argmax(0) != prob.argmax(0)).float().mean())
        print(f"({H},{W},{C}) w_g={w_g} w_b={w_b}: {int(close.sum())} pixels with margin < {R.MARGIN} (smallest "
              f"{float(R.top2_margin(Q64).min()):.2e}), argmax changed at {100 * changed:.1f} %")
        assert float(close.float().mean()) <= R.REF_TIE_SHARE
        assert bool(((Q32.argmax(0) == Q64.argmax(0)) | close).all())
        assert (changed > 0.02) == (w_g != 0.0 or w_b != 0.0)
