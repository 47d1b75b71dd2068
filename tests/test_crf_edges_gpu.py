"""The exact DenseCRF kernels (csrc/crf.hip) at their edges: the seams of the query / key / channel tiling, the switch between the
Gaussian stencil and the dense kernel, guard bands around every buffer, a Q that spans the fp32 range, the zero-weight branches of
dupl_dense_crf, the unary kernels at their clips and at the grid cap, and standard deviations at both ends of the admitted range.

The references are the brute-force functions of tests/crf_ref.py in fp64 and the bar is that of tests/test_crf_gpu.py: the
device error may be at most FACTOR = 4 x the error of the same formulas evaluated by torch in fp32, floored at 2^-24;
row-relative for messages, relative for n.  Every case prints its device / fp32-torch ratio."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import crf_ref as R
import kernel_guard as KG

pytestmark = pytest.mark.gpu

FACTOR = 4.0
EVAL = R.PARAMS["eval"]


def _bar(err32):
    return FACTOR * max(err32, R.EPS32)


@functools.lru_cache(maxsize=None)
def _case(H, W, C):
    return R.make_case(H, W, C, seed=R.case_seed(H, W))


@functools.lru_cache(maxsize=None)
def _kernel(H, W, C, bilateral, sxy, srgb):
    """(K64, K32, n64, n32) of one kernel on the seeded image of (H, W, C): computed once, shared, never modified."""
    im = _case(H, W, C)[0] if bilateral else None
    K64 = R.kernel_rows(R.features(H, W, im, sxy, srgb, torch.float64))
    K32 = R.kernel_rows(R.features(H, W, im, sxy, srgb, torch.float32))
    return K64, K32, R.norm_of(K64), R.norm_of(K32)


def _check(tag, err, err32):
    ratio = err / max(err32, R.EPS32)
    print(f"{tag}: err {err:.2e}, fp32 torch {err32:.2e}, ratio {ratio:.2f}")
    assert err <= _bar(err32), f"{tag}: device error {err:.3e} over {FACTOR} x the fp32 evaluation's {max(err32, R.EPS32):.3e}"
    return ratio


def _check_kernel(dev, tag, H, W, C, Q, bilateral, sxy, srgb):
    """n and the message of Q (C', N) fp32, normalised and not, of one kernel against fp64 -> (worst ratio, [n, M_norm, M_plain])."""
    from dupl_amd import ops
    K64, K32, n64, n32 = _kernel(H, W, C, bilateral, sxy, srgb)
    img_d = _case(H, W, C)[0].to(dev) if bilateral else None
    n_d = ops.crf_norm(img_d, H, W, sxy, srgb, device=dev)
    outs = [n_d.cpu()]
    worst = _check(f"({H},{W}) {tag} n", R.rel_err(outs[0].reshape(-1), n64), R.rel_err(n32, n64))
    for normalize in (True, False):
        ref = R.message(K64, Q.double(), n64 if normalize else None)
        t32 = R.message(K32, Q, n32 if normalize else None)
        out = ops.crf_message(img_d, Q.reshape(-1, H, W).to(dev), sxy, srgb, normalize=normalize).cpu()
        assert out.shape == (Q.shape[0], H, W) and out.dtype == torch.float32
        outs.append(out)
        worst = max(worst, _check(f"({H},{W},{Q.shape[0]}) {tag} normalize={normalize}", R.row_rel_err(out, ref), R.row_rel_err(t32, ref)))
    return worst, outs


# ------------------------------------------------------------------------------------------------ 1. query / key tile seams
@pytest.mark.parametrize("H,W", R.SEAM_SHAPES, ids=[f"{h}x{w}" for h, w in R.SEAM_SHAPES])
def test_pixel_counts_around_the_tile_sizes(dev, H, W):
    """N = 31 ... 513, one short of, at and one past 32, 64, 128, 256 and 512 (the MFMA tile, a wave's queries, the key tile and
    the row-sum half block, the query block), as rows, columns and 2-D images: the bilateral kernel 121/5 and the Gaussian
    sigma = 3 (the dense kernel without an image at these sizes), normalised and not, and n."""
    Q = torch.softmax(_case(H, W, 3)[2], 0).reshape(3, -1)
    worst = 0.0
    for tag, bilateral, sxy, srgb in (("bilateral 121/5", True, 121.0, 5.0), ("gauss sxy=3", False, 3.0, 1.0)):
        worst = max(worst, _check_kernel(dev, tag, H, W, 3, Q, bilateral, sxy, srgb)[0])
    print(f"({H},{W}) N={H * W}: worst device / fp32-torch error ratio {worst:.2f} (bar {FACTOR})")


# ------------------------------------------------------------------------------------------------ 2. channel chunk seams
def _message_raw(img_d, Q_d, n_d, out_ptr, C, H, W, sxy, srgb):
    from dupl_amd import _lib, ops
    d = _lib.CrfDesc(C=C, H=H, W=W, img=None if img_d is None else img_d.data_ptr(), Q=None if Q_d is None else Q_d.data_ptr(),
                     norm=None if n_d is None else n_d.data_ptr(), out=out_ptr, sxy=sxy, srgb=srgb)
    return _lib.lib().dupl_crf_message.raw(ctypes.byref(d), ops._stream())


def _all_written(g):
    """no element of the guard's view still carries the sentinel (a NaN payload)"""
    torch.cuda.synchronize()
    return bool((g.view.contiguous().view(g.itype) != g.pat).all())


@pytest.mark.parametrize("H,W", [(257, 1), (1, 257)])
def test_channel_counts_around_the_chunk(dev, H, W):
    """C = 1, 31, 32, 33, 64, 65 at N = 257 (a prime: the image is a column or a row) on the dense kernel with and without an
    image and on the stencil: the fp64 bar, every channel written (the output starts as a NaN-payload sentinel), nothing written
    around it, and channel c of the C-channel call has the bits of channel c of the 65-channel call."""
    from dupl_amd import ops
    img, _, logits = _case(H, W, 65)
    N = H * W
    Q65 = torch.softmax(logits, 0).reshape(65, N)
    img_d, Q_d = img.to(dev), Q65.to(dev)
    worst = 0.0
    for tag, bilateral, sxy, srgb in (("bilateral 121/5", True, 121.0, 5.0), ("gauss sxy=3 (dense)", False, 3.0, 1.0),
                                      ("gauss sxy=1 (stencil)", False, 1.0, 1.0)):
        assert bilateral or R.gauss_takes_stencil(H, W, sxy) == (sxy == 1.0)
        K64, K32, n64, n32 = _kernel(H, W, 65, bilateral, sxy, srgb)
        im = img_d if bilateral else None
        n_d = ops.crf_norm(im, H, W, sxy, srgb, device=dev)
        for normalize in (True, False):
            ref65 = R.message(K64, Q65.double(), n64 if normalize else None)
            t65 = R.message(K32, Q65, n32 if normalize else None)
            full = None
            for C in reversed(R.CHUNK_C):
                g = KG.Guard((C, H, W), dev)
                assert _message_raw(im, Q_d[:C].contiguous(), n_d if normalize else None, g.ptr, C, H, W, sxy, srgb) == 0
                assert _all_written(g), f"{tag} C={C}: an output element was not written"
                out = g.cpu().reshape(C, N)
                worst = max(worst, _check(f"({H},{W},{C}) {tag} normalize={normalize}", R.row_rel_err(out, ref65[:C]),
                                          R.row_rel_err(t65[:C], ref65[:C])))
                full = out if C == 65 else full
                assert KG.same_bits(out, full[:C]), f"{tag} C={C}: a channel's value depends on the number of channels"
    print(f"({H},{W}): worst device / fp32-torch error ratio {worst:.2f} (bar {FACTOR})")


# ------------------------------------------------------------------------------------------------ 3. the Gaussian switch
@pytest.mark.parametrize("H,W,sxy,stencil", [(15, 15, 1.0, False), (2, 113, 1.0, True), (226, 1, 1.0, True), (33, 33, 1.0, True),
                                             (40, 25, 3.0, False)])
def test_gaussian_on_both_sides_of_the_switch(dev, H, W, sxy, stencil):
    """The truncated stencil runs only when its (2R + 1)^2 window is smaller than the image (R of crf_ref.gauss_radius: 7 for
    sigma = 1, 225 pixels).  15 x 15 is the largest image on the dense kernel, 2 x 113 and 226 x 1 the smallest on the stencil,
    33 x 33 has windows clipped at each border and corner and whole ones in the middle, 40 x 25 under sigma = 3 is a 2-D image on
    the dense kernel without colours.  Both sides meet the fp64 bar: the mass the stencil drops is not visible in fp32."""
    assert R.gauss_takes_stencil(H, W, sxy) == stencil
    Q = torch.softmax(_case(H, W, 3)[2], 0).reshape(3, -1)
    worst, _ = _check_kernel(dev, f"gauss sxy={sxy:g} ({'stencil' if stencil else 'dense'})", H, W, 3, Q, False, sxy, 1.0)
    print(f"({H},{W}) sxy={sxy:g}: worst device / fp32-torch error ratio {worst:.2f} (bar {FACTOR})")


# ------------------------------------------------------------------------------------------------ 4. guard bands
@pytest.mark.parametrize("H,W", [(1, 1), (3, 43), (17, 16)])
def test_nothing_outside_the_buffers(dev, H, W):
    """Raw ABI calls with every output and the workspace inside sentinel buffers, every float input inside NaN slack one float off
    alignment and the image inside a uint8 sentinel buffer on an odd address, C = 33: the slack is intact, the results are finite
    and have the bits of the plain call.  A workspace one float short is refused and leaves the output untouched."""
    from dupl_amd import _lib, ops
    L, C, N = _lib.lib(), 33, H * W
    img, labels, logits = _case(H, W, C)
    Q = torch.softmax(logits, 0)
    img_d, Q_d = img.to(dev), Q.to(dev)
    g_img = KG.Guard((H, W, 3), dev, torch.uint8, init=img_d, front=KG.PAD_U8 + 1)
    assert g_img.ptr % 2 == 1
    q_in = KG.nan_in(Q, dev, front=KG.PAD + 1)
    assert q_in.data_ptr() % 8 == 4
    for tag, im, gim, sxy, srgb in (("bilateral", img_d, g_img.view, 121.0, 5.0), ("gauss 3", None, None, 3.0, 1.0), ("gauss 1", None, None, 1.0, 1.0)):
        want_n = ops.crf_norm(im, H, W, sxy, srgb, device=dev)
        g_n = KG.Guard((H, W), dev, front=KG.PAD + 1)
        assert _message_raw(gim, None, None, g_n.ptr, 1, H, W, sxy, srgb) == 0
        assert KG.same_bits(g_n.cpu(), want_n.cpu()) and bool(torch.isfinite(want_n).all()), tag
        n_in = KG.nan_in(want_n.cpu(), dev, front=KG.PAD + 3)
        for nrm, nrm_in in ((want_n, n_in), (False, None)):
            want = ops.crf_message(im, Q_d, sxy, srgb, normalize=nrm)
            g_out = KG.Guard((C, H, W), dev, front=KG.PAD + 1)
            assert _message_raw(gim, q_in, nrm_in, g_out.ptr, C, H, W, sxy, srgb) == 0
            assert KG.same_bits(g_out.cpu(), want.cpu()) and bool(torch.isfinite(want).all()), tag
    # the whole inference
    U = R.unary_from_softmax(Q)
    want = ops.dense_crf(U.to(dev), img_d, 2, **EVAL)
    u_in = KG.nan_in(U, dev, front=KG.PAD + 1)
    g_out, g_ws = KG.Guard((C, H, W), dev, front=KG.PAD + 1), KG.Guard(((2 + 2 * C) * N,), dev, front=KG.PAD + 1)

    def crf(out, ws_bytes):
        d = _lib.CrfDesc(C=C, H=H, W=W, T=2, img=g_img.ptr, unary=u_in.data_ptr(), out=out.ptr, workspace=g_ws.ptr,
                         workspace_bytes=ws_bytes, **EVAL)
        return L.dupl_dense_crf.raw(ctypes.byref(d), ops._stream())

    assert crf(g_out, g_ws.n * 4) == 0
    assert KG.same_bits(g_out.cpu(), want.cpu()) and bool(torch.isfinite(want).all())
    torch.cuda.synchronize()
    assert g_ws.intact() and _all_written(g_ws)
    g_short = KG.Guard((C, H, W), dev)
    assert crf(g_short, g_ws.n * 4 - 4) == -1                       # DUPL_ERR_ARG
    torch.cuda.synchronize()
    assert g_short.untouched()
    # the unary kernels
    z_in = KG.nan_in(logits, dev, front=KG.PAD + 1)
    for mode, src, src_in in ((0, Q_d, q_in), (1, logits.to(dev), z_in)):
        want = ops.crf_unary(src, from_logits=bool(mode))
        g_u = KG.Guard((C, H, W), dev, front=KG.PAD + 1)
        assert L.dupl_crf_unary.raw(src_in.data_ptr(), g_u.ptr, C, N, mode, ops._stream()) == 0
        assert KG.same_bits(g_u.cpu(), want.cpu()) and bool(torch.isfinite(want).all())
    g_lab = KG.Guard((H, W), dev, torch.int64, init=labels.to(dev), front=KG.PAD + 1)
    want = ops.crf_unary_labels(labels.to(dev), C, 0.7)
    g_u = KG.Guard((C, H, W), dev, front=KG.PAD + 1)
    assert L.dupl_crf_unary_labels.raw(g_lab.ptr, g_u.ptr, C, N, 0.7, ops._stream()) == 0
    assert KG.same_bits(g_u.cpu(), want.cpu())
    torch.cuda.synchronize()
    assert g_img.intact() and torch.equal(g_img.view.cpu(), img) and g_lab.intact()


# ------------------------------------------------------------------------------------------------ 5. wide-range Q
def test_q_spanning_the_fp32_range(dev):
    """Q = softmax of 25 x N(0,1) logits on a 24 x 40 image, 21 channels: the entries run from 1 through the fp32 denormals to
    0 (over 40 decades, crf_ref.wide_range_q), one channel is 0 everywhere.  Under the bilateral kernel 121/5, and under
    srgb = 1, where a pixel's sum is made of the few keys of its own colour and so of whatever small entries those carry, the
    messages meet the row-relative fp64 bar, and nothing is NaN or negative.
    Measured on the MI355X: worst device / fp32-torch error ratio 0.98 (bar 4)."""
    H, W, C = 24, 40, 21
    Q = R.wide_range_q(C, H, W, seed=5)
    assert R.decades(Q) >= 30.0
    worst = 0.0
    for tag, sxy, srgb in (("bilateral 121/5", 121.0, 5.0), ("bilateral 121/1", 121.0, 1.0)):
        w, outs = _check_kernel(dev, tag + " wide Q", H, W, C, Q, True, sxy, srgb)
        worst = max(worst, w)
        for out in outs:
            assert bool(torch.isfinite(out).all()) and bool((out >= 0).all()), tag
        assert bool((outs[1][1] == 0).all()) and bool((outs[2][1] == 0).all())         # the channel of zeros stays 0
    print(f"wide-range Q: worst device / fp32-torch error ratio {worst:.2f} (bar {FACTOR})")


# ------------------------------------------------------------------------------------------------ 6. dupl_dense_crf branches
def _dense_crf_raw(dev, U, img, T, w_g, w_b):
    """dupl_dense_crf with the output and the workspace in sentinel buffers -> (Q on the host, the workspace's bits on the host)"""
    from dupl_amd import _lib, ops
    C, H, W = U.shape
    g_out, g_ws = KG.Guard((C, H, W), dev), KG.Guard(((2 + 2 * C) * H * W,), dev)
    u_d, img_d = U.to(dev), img.to(dev)
    d = _lib.CrfDesc(C=C, H=H, W=W, T=T, img=img_d.data_ptr(), unary=u_d.data_ptr(), out=g_out.ptr, workspace=g_ws.ptr,
                     workspace_bytes=g_ws.n * 4, w_g=w_g, sxy_g=EVAL["sxy_g"], w_b=w_b, sxy_b=EVAL["sxy_b"], srgb_b=EVAL["srgb_b"])
    assert _lib.lib().dupl_dense_crf.raw(ctypes.byref(d), ops._stream()) == 0
    return g_out.cpu(), KG.bits(g_ws.cpu()) != g_ws.pat


@pytest.mark.parametrize("H,W,C", R.BRANCH_CASES)
def test_dense_crf_without_iterations_is_the_softmax(dev, H, W, C):
    """T = 0: Q = softmax(-U), as far from torch's fp64 softmax as 4 x torch's fp32 softmax is; no workspace word is written."""
    img, _, logits = R.make_case(H, W, C, seed=R.branch_seed(H, W, C))
    U = R.unary_from_softmax(torch.softmax(logits, 0))
    Q, written = _dense_crf_raw(dev, U, img, 0, EVAL["w_g"], EVAL["w_b"])
    ref = torch.softmax(-U.double(), 0)
    _check(f"({H},{W},{C}) T=0", float((Q.double() - ref).abs().max()), float((torch.softmax(-U, 0).double() - ref).abs().max()))
    assert not bool(written.any())


@pytest.mark.parametrize("w_g,w_b", R.BRANCH_WEIGHTS)
@pytest.mark.parametrize("H,W,C", R.BRANCH_CASES)
def test_dense_crf_with_a_zero_weight(dev, H, W, C, w_g, w_b):
    """w_g = 0, w_b = 0 or both: ten iterations against the fp64 mean field with the same weights -- Q within the bar, labels equal
    except where the fp64 top-2 margin is under 1e-4, at most 0.2 % of the pixels so excused -- and the n and M regions of the
    workspace that belong to a kernel of weight 0 are never written, the others wholly."""
    img, _, logits = R.make_case(H, W, C, seed=R.branch_seed(H, W, C))
    U = R.unary_from_softmax(torch.softmax(logits, 0))
    N = H * W
    args = (w_g, EVAL["sxy_g"], w_b, EVAL["sxy_b"], EVAL["srgb_b"])
    Q64, Q32 = R.mean_field(img, U, R.BRANCH_T, *args), R.mean_field(img, U, R.BRANCH_T, *args, dtype=torch.float32)
    Q, written = _dense_crf_raw(dev, U, img, R.BRANCH_T, w_g, w_b)
    _check(f"({H},{W},{C}) w_g={w_g:g} w_b={w_b:g}", float((Q.double() - Q64).abs().max()), float((Q32.double() - Q64).abs().max()))
    close, differ = R.top2_margin(Q64) < R.MARGIN, Q.argmax(0) != Q64.argmax(0)
    print(f"  {int(differ.sum())} labels differ, {int(close.sum())} of {close.numel()} pixels have margin < {R.MARGIN}")
    assert not bool((differ & ~close).any())
    assert float(close.float().mean()) <= R.TIE_SHARE
    assert float((Q.sum(0) - 1).abs().max()) < 1e-5
    ng, nb, Mg, Mb = written[:N], written[N:2 * N], written[2 * N:(2 + C) * N], written[(2 + C) * N:]
    for tag, w, regions in (("Gaussian", w_g, (ng, Mg)), ("bilateral", w_b, (nb, Mb))):
        for r in regions:
            assert bool(r.all()) if w != 0.0 else not bool(r.any()), f"{tag} workspace region with weight {w}"


# ------------------------------------------------------------------------------------------------ 7. unary kernels
GRID_CAP = 16384 * 256                                   # crf_ew_grid: at most 16384 blocks of 256 threads, then a grid-stride loop
UNARY_SIZES = [(1, 2), (1, 5), (255, 2), (255, 5), (257, 2), (257, 5), (GRID_CAP + 1, 2)]


def _specials(N, C, values, seed):
    """(C, N) of seeded uniform values with `values` written over it, cycling, so that every size holds each of them, the
    first and the last pixel included"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((C, N), generator=g)
    v = torch.tensor(values, dtype=torch.float32)
    idx = torch.arange(0, C * N, 3)
    x.view(-1)[idx] = v[(idx // 3) % len(v)]
    x.view(-1)[-1] = v[(C * N) % len(v)]
    return x


@pytest.mark.parametrize("N,C", UNARY_SIZES)
def test_unary_from_probabilities(dev, N, C):
    """U = -log(clip(p, 1e-5, 1)) for p = 0, denormals, 1e-6, exactly 1e-5 (the fp32 value of the clip), its two neighbours, 1
    and 1.5: within 1 ulp of the fp64 logarithm rounded to fp32.  The clip is exact in fp32.  A logarithm accurate to 1 ulp (the
    figure the HIP documentation gives, "HIP math API", for log) lands at most one fp32 value from the correctly rounded one.
    logf as compiled for gfx950 did not: it is v_log_f32 (log2 to 1 ulp) times ln 2, and 1 ulp of log2(1e-5) = -16.6 is 1.4 ulp of
    11.5 -- measured on the MI355X, the energy at the clip was 2 fp32 values off.  The kernel now takes the logarithm in fp64
    (1 ulp of fp64) and rounds once.  At the clips the result is the constant: -log(1e-5f) rounded, and 0."""
    from dupl_amd import ops
    lo = np.float32(1e-5)
    vals = [0.0, 1e-45, 1e-39, 1e-6, float(np.nextafter(lo, np.float32(0))), float(lo), float(np.nextafter(lo, np.float32(1))), 0.3,
            float(np.nextafter(np.float32(1), np.float32(0))), 1.0, 1.5]
    p = _specials(N, C, vals, seed=N + C)
    U = ops.crf_unary(p.reshape(C, 1, N).to(dev)).cpu().reshape(C, N)
    want = R.unary_exact(p)
    d = R.ulp_distance(U, want)
    print(f"N={N} C={C}: largest distance {int(d.max())} ulp, {float((d > 0).float().mean()) * 100:.2f} % of the values not correctly rounded")
    assert int(d.max()) <= 1
    assert bool((U[p <= float(lo)] == float(np.float32(-math.log(float(lo))))).all()) and bool((U[p >= 1.0] == 0.0).all())


@pytest.mark.parametrize("N,C", UNARY_SIZES)
def test_unary_from_logits(dev, N, C):
    """U = -log(clip(softmax(z), 1e-5, 1)) for logits of +-80 (exp alone would overflow), rows of equal values (at 80, -80 and 0)
    and ordinary ones, against the fp64 softmax under the row-relative bar."""
    from dupl_amd import ops
    g = torch.Generator().manual_seed(N * 7 + C)
    z = 3.0 * torch.randn((C, N), generator=g)
    sel = torch.arange(N) % 5
    z[:, sel == 0] = torch.where(torch.rand((C, int((sel == 0).sum())), generator=g) < 0.5, 80.0, -80.0)
    z[:, sel == 1] = torch.tensor([80.0, -80.0, 0.0])[torch.arange(int((sel == 1).sum())) % 3]
    z[0, sel == 2], z[1, sel == 2] = 80.0, -80.0
    U = ops.crf_unary(z.reshape(C, 1, N).to(dev), from_logits=True).cpu().reshape(C, N)
    ref, t32 = R.unary_from_logits(z), R.unary_from_logits(z, torch.float32)
    assert bool(torch.isfinite(U).all()) and bool((U >= 0).all())
    eq = sel == 1
    assert bool((U[:, eq] == U[:1, eq]).all())                                   # equal logits: equal energies
    _check(f"N={N} C={C} unary from logits", R.row_rel_err(U, ref), R.row_rel_err(t32, ref))


@pytest.mark.parametrize("gt_prob", [0.5, 0.999])
@pytest.mark.parametrize("N,C", UNARY_SIZES)
def test_unary_from_labels(dev, N, C, gt_prob):
    """Labels in [0, C) give -log(gt_prob) in their channel; -1, C and 255 match no channel and give the "other" energy
    -log((1 - gt_prob) / (C - 1)) in every one.  Bit-equal to the fp64 values rounded to fp32."""
    from dupl_amd import ops
    lab = KG.rndint(0, C, N, seed=N + C).to(torch.int64)
    out_of_range = torch.tensor([-1, C, 255])
    idx = torch.arange(0, N, 4)
    lab[idx] = out_of_range[(idx // 4) % 3]
    lab[-1] = C if N > 1 else -1
    U = ops.crf_unary_labels(lab.reshape(1, N).to(dev), C, gt_prob).cpu().reshape(C, N)
    want = R.unary_from_any_labels(lab, C, gt_prob)
    assert KG.same_bits(U, want)
    bad = (lab < 0) | (lab >= C)
    assert bool(bad.any()) and bool((U[:, bad] == float(np.float32(-math.log((1.0 - gt_prob) / (C - 1))))).all())


# ------------------------------------------------------------------------------------------------ 8. extreme sigma
@pytest.mark.parametrize("std", R.EXTREME_STD)
def test_standard_deviations_at_the_ends_of_the_range(dev, std):
    """sxy and srgb at 1e-25, 1e-19, 1e-3, 1e6 and 3e38 (all inside the admitted 0 < sigma <= 3e38) on a 9 x 13 image with 5
    channels, against the fp64 reference at the same (fp32-rounded) sigma: towards 0 the kernel is the identity (k = delta_ij,
    n = 1, M(Q) = Q), towards infinity k = 1.  Every output is finite.  (log2(e) / 2 sigma^2 overflows fp32 below
    sigma = 4.6e-20; unsaturated, inf x the zero distance of j = i made every output NaN.)"""
    H, W, C = 9, 13, 5
    s = float(np.float32(std))
    img, _, logits = _case(H, W, C)
    Q = torch.softmax(logits, 0).reshape(C, -1)
    worst = 0.0
    for tag, bilateral, sxy, srgb in ((f"gauss sxy={std:g}", False, s, 1.0), (f"bilateral {std:g}/5", True, s, 5.0),
                                      (f"bilateral 121/{std:g}", True, 121.0, s), (f"bilateral {std:g}/{std:g}", True, s, s)):
        w, outs = _check_kernel(dev, tag, H, W, C, Q, bilateral, sxy, srgb)
        worst = max(worst, w)
        for out in outs:
            assert bool(torch.isfinite(out).all()), tag
        if std < 1e-10 and not tag.startswith("bilateral 121"):
            assert torch.equal(outs[0], torch.ones(H, W)) and torch.equal(outs[2].reshape(C, -1), Q), tag      # the identity, exactly
    print(f"sigma={std:g}: worst device / fp32-torch error ratio {worst:.2f} (bar {FACTOR})")
