"""The HBM-bound glue kernels (csrc/tokens.hip, cam.hip, conv.hip, eval.hip and the element-wise helpers of norm.hip) at
their edges: odd shapes, strided operands, the scalar / per-pixel / fall-through launcher paths, ties, thresholds, non-finite
columns and the second trip of every grid-stride loop -- each against a plain float64 (or bit-exact fp32) host reference from
tests/glue_ref.py, whose bounds tests/test_glue_ref_host.py checks first.

Technique (as tests/test_attention_gpu.py): every output lives inside a larger buffer whose slack holds a sentinel that must be
bit-unchanged afterwards; every input lives inside a buffer whose slack (and every element the kernel is told to skip: padding
columns, the cls row) is NaN, so a finite result proves nothing else was read.  Kernels are called through dupl_amd.ops /
ops.L() on the current stream; the test synchronises and compares on the host.  Tolerance tests print their worst err / bound."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G
from kernel_guard import (NAN, EPS24, PAD, SENT, _ALIVE, Guard, bits, nan_in, ratio_report, rnd, rndint, same_bits,  # noqa: F401
                          stream)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


# =========================================================================================== tokens: global max pool
GMP_SHAPES = [(2, 784, 768), (1, 1, 64), (3, 15, 70), (2, 17, 130), (1, 65, 64), (2, 196, 21)]


def _gmp_fwd(dev, tok):
    from dupl_amd import ops
    B, n1, D = tok.shape
    tin = nan_in(tok, dev)
    out, idx = Guard((B, D), dev), Guard((B, D), dev, torch.int32)
    ops.L().dupl_gmp_fwd(tin.data_ptr(), out.ptr, idx.ptr, B, n1 - 1, D, stream())
    return out.cpu(), idx.cpu()


def _gmp_bwd_check(dev, idx, B, n, D, seed):
    """dtokens += scatter(dout): accumulates onto a non-zero start and touches no other element (the cls rows included)."""
    from dupl_amd import ops
    assert int(idx.min()) >= 0 and int(idx.max()) < n          # checked on the host BEFORE the scatter is launched
    start, dout = rnd(B, n + 1, D, seed=seed), rnd(B, D, seed=seed + 1)
    dt = Guard((B, n + 1, D), dev, init=start)
    ops.gmp_bwd(nan_in(dout, dev), idx.to(dev), dt.view, B, n, D)
    want = start.clone()
    want[:, 1:].scatter_add_(1, idx.long().unsqueeze(1), dout.unsqueeze(1))     # one add per element: exact
    assert same_bits(dt.cpu(), want)


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("B,n,D", GMP_SHAPES)
def test_gmp_values_and_indices_are_torchs(dev, B, n, D, kind):
    """Value AND index equal tokens[:, 1:].max(1) exactly.  "ties": values from 5 distinct floats, so every column ties many
    times within a row group (rows i, i + 16), across groups and across the 4-way unroll and its tail; torch's first wins."""
    if kind == "random":
        tok = rnd(B, n + 1, D, seed=n + D)
    else:
        tok = torch.tensor([-1.5, 0.25, 0.5, 2.0, -0.0])[rndint(0, 5, B, n + 1, D, seed=n + D)]
    tok[:, 0] = NAN                                  # the cls row is never read
    mx, idx = _gmp_fwd(dev, tok)
    rm, ri = tok[:, 1:].max(dim=1)
    assert torch.equal(mx, rm)
    assert torch.equal(idx.long(), ri)
    _gmp_bwd_check(dev, idx, B, n, D, seed=7)


def _first_nan_else_first_max(col):
    nan = np.isnan(col)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(col))


@pytest.mark.parametrize("B,n,D", [(2, 70, 130), (1, 15, 70), (2, 784, 64), (1, 1, 5)])
def test_gmp_non_finite_columns(dev, B, n, D):
    """torch.max semantics on non-finite columns: NaN wherever a column holds one, with the index of the FIRST NaN; -inf with
    index 0 for an all -inf column; the first +inf.  Every index is a patch row.  idx is inspected on the host first and
    gmp_bwd is launched only with indices that passed (an index of INT_MAX would make its scatter a wild store)."""
    tok = rnd(B, n + 1, D, seed=3)
    tok[:, 0] = NAN
    p = tok[:, 1:]                                   # a view: patch rows
    p[:, :, 0] = NAN                                 # all NaN
    p[:, n - 1, 1] = NAN                             # a single NaN, in the last row
    late = [r for r in range(n) if r % 16 >= 1]      # NaNs in row groups >= 1 only
    if late:
        p[:, late[len(late) // 2], 2] = NAN
        p[:, late[-1], 2] = NAN
        p[0, late[0], 2] = NAN
    p[:, :, 3] = -math.inf                           # all -inf
    p[:, n // 2, 4] = math.inf                       # +inf twice
    p[:, n - 1, 4] = math.inf
    mx, idx = _gmp_fwd(dev, tok)
    rm, ri = p.max(dim=1)
    want_idx = torch.tensor([[_first_nan_else_first_max(p[b, :, d].numpy()) for d in range(D)] for b in range(B)])
    assert torch.equal(ri, want_idx), "torch.max itself: first NaN, else first maximum"
    assert int(idx.min()) >= 0 and int(idx.max()) < n, f"index outside [0, {n}): {int(idx.min())} .. {int(idx.max())}"
    assert torch.equal(idx.long(), want_idx)
    assert torch.equal(torch.isnan(mx), torch.isnan(rm)) and bool(torch.isnan(mx[:, 0]).all())
    assert torch.equal(torch.nan_to_num(mx, nan=0.0), torch.nan_to_num(rm, nan=0.0))       # -inf / +inf as torch
    assert bool((mx[:, 3] == -math.inf).all()) and bool((idx[:, 3] == 0).all()) and bool((mx[:, 4] == math.inf).all())
    _gmp_bwd_check(dev, idx, B, n, D, seed=11)


# =========================================================================================== tokens: transposes
TR_SHAPES = [(2, 784, 21), (1, 784, 81), (2, 33, 31), (3, 1, 1), (1, 32, 32), (2, 31, 768)]


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("B,n,D", TR_SHAPES)
def test_token_transposes_are_exact(dev, B, n, D, skip):
    from dupl_amd import ops
    tok = rnd(B, skip + n, D, seed=n + D + skip)
    if skip:
        tok[:, 0] = NAN
    out = Guard((B, D, n), dev)
    ops.L().dupl_tokens_to_nchw(nan_in(tok, dev).data_ptr(), out.ptr, B, n, D, skip, stream())
    want = tok[:, skip:].transpose(1, 2).contiguous()
    got = out.cpu()
    assert same_bits(got, want)
    # the add form: onto a random non-zero destination, cls row untouched when skipped
    start, src = rnd(B, skip + n, D, seed=5), rnd(B, D, n, seed=6)
    dst = Guard((B, skip + n, D), dev, init=start)
    ops.nchw_to_tokens_add(nan_in(src, dev), dst.view, B, n, D, skip_cls=bool(skip))
    ref = start.clone()
    ref[:, skip:] += src.transpose(1, 2)             # one rounding per element
    assert same_bits(dst.cpu(), ref)
    # round trip onto zeros
    back = Guard((B, skip + n, D), dev, init=torch.zeros(B, skip + n, D))
    ops.nchw_to_tokens_add(nan_in(got, dev), back.view, B, n, D, skip_cls=bool(skip))
    rt = back.cpu()
    assert same_bits(rt[:, skip:] + 0.0, tok[:, skip:] + 0.0) and bool((rt[:, :skip] == 0).all())


# =========================================================================================== tokens: patch im2row
def _im2row_ref(x, P):
    B, _, H, W = x.shape
    h, w = H // P, W // P
    return F.unfold(x[..., :h * P, :w * P], P, stride=P).transpose(1, 2).reshape(B * h * w, 3 * P * P)


@pytest.mark.parametrize("B,H,W,P,off", [(2, 64, 96, 16, 0), (1, 70, 90, 16, 0), (1, 468, 625, 16, 0), (2, 33, 50, 16, 0),
                                         (1, 16, 16, 16, 0), (3, 40, 52, 8, 0), (2, 64, 96, 16, 1)])
def test_patch_im2row_is_unfold(dev, B, H, W, P, off):
    """Bit-equal to F.unfold of the image cropped to whole patches: W % 4 in {0, 1, 2} (vector and scalar path), trailing rows
    and columns ignored; off = 1: x starts 4 bytes into its allocation (the scalar path at W % 4 == 0)."""
    from dupl_amd import ops
    x = rnd(B, 3, H, W, seed=H + W)
    xin = nan_in(x, dev, front=PAD + off)
    assert (xin.data_ptr() % 16 == 0) == (off == 0)
    rows = Guard((B * (H // P) * (W // P), 3 * P * P), dev)
    ops.L().dupl_patch_im2row(xin.data_ptr(), rows.ptr, B, H, W, P, stream())
    assert same_bits(rows.cpu(), _im2row_ref(x, P))


def test_patch_im2row_refuses_bad_patch_sizes(dev):
    from dupl_amd import ops
    x = nan_in(rnd(1, 3, 24, 24, seed=1), dev)
    rows = Guard((64, 3 * 16 * 16), dev)
    for (H, W, P) in ((24, 24, 6), (8, 24, 16), (24, 8, 16), (24, 24, 0)):
        with pytest.raises(RuntimeError, match="status -1"):
            ops.L().dupl_patch_im2row(x.data_ptr(), rows.ptr, 1, H, W, P, stream())
    torch.cuda.synchronize()
    assert rows.untouched()


# =========================================================================================== tokens: pos-embed, assembly
@pytest.mark.parametrize("g,h,w", [(14, 28, 28), (14, 4, 6), (14, 6, 4), (14, 1, 1), (14, 7, 9), (14, 30, 39), (14, 14, 14), (1, 3, 5)])
def test_pos_embed_resize_against_bicubic64(dev, g, h, w):
    """3e-6 of the output maximum (the bar test_token_plumbing holds this kernel to); the cls row is a bit-exact copy and
    h = w = g copies everything."""
    from dupl_amd import ops
    D = 40
    pe = rnd(1 + g * g, D, seed=g + h + w)
    out = Guard((1 + h * w, D), dev)
    ops.L().dupl_pos_embed_resize(nan_in(pe, dev).data_ptr(), out.ptr, g, h, w, D, stream())
    got, ref = out.cpu(), G.pos_embed64(pe, g, h, w)
    assert same_bits(got[0], pe[0])
    e = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"pos_embed {g} -> {h}x{w}: err / max {e:.2e} (bar 3e-6)")
    assert e < 3e-6
    if h == g and w == g:
        assert same_bits(got, pe)


@pytest.mark.parametrize("B,n,D", [(1, 1, 4), (5, 37, 68), (16, 784, 768)])
def test_assemble_tokens_and_backward(dev, B, n, D):
    """Forward: bit-equal to torch's fp32 cat(cls, patch) + pos.  Backward: rows 1..n copied exactly; dcls accumulates onto a
    non-zero start within (B + 1) * 2^-24 * (|start| + sum_b |row 0|) of float64 -- B - 1 roundings of the partial sums and one of
    start + sum, each of a quantity no larger than that sum.  (16, 784, 768) also drives the grid-stride loop."""
    from dupl_amd import ops
    patch, cls, pos = rnd(B * n, D, seed=1), rnd(D, seed=2), rnd(n + 1, D, seed=3)
    tok = Guard((B * (n + 1), D), dev)
    ops.L().dupl_assemble_tokens(nan_in(patch, dev).data_ptr(), nan_in(cls, dev).data_ptr(), nan_in(pos, dev).data_ptr(),
                                 tok.ptr, B, n, D, stream())
    want = torch.cat((cls.view(1, 1, D).expand(B, 1, D), patch.view(B, n, D)), 1) + pos
    assert same_bits(tok.cpu().view(B, n + 1, D), want)
    dtok, start = rnd(B, n + 1, D, seed=4), rnd(D, seed=5)
    dpatch, dcls = Guard((B * n, D), dev), Guard((D,), dev, init=start)
    ops.L().dupl_assemble_tokens_bwd(nan_in(dtok, dev).data_ptr(), dpatch.ptr, dcls.ptr, B, n, D, stream())
    assert same_bits(dpatch.cpu().view(B, n, D), dtok[:, 1:].contiguous())
    ref = start.double() + dtok[:, 0].double().sum(0)
    bound = (B + 1) * EPS24 * (start.double().abs() + dtok[:, 0].double().abs().sum(0))
    assert ratio_report(f"assemble_tokens_bwd dcls B={B}", (dcls.cpu().double() - ref).abs(), bound) <= 1.0


# =========================================================================================== CAM: bilinear resize
RESIZE_IDS = [f"{a}x{b}-{c}x{d}-{'ac' if e else 'hp'}" for a, b, c, d, e in G.RESIZE_CASES]


def _resize(dev, x, Ho, Wo, flip, align):
    from dupl_amd import ops
    B, C, Hi, Wi = x.shape
    out = Guard(((2 * B) if flip else B, C, Ho, Wo), dev)
    ops.L().dupl_resize_bilinear(nan_in(x, dev).data_ptr(), out.ptr, B, C, Hi, Wi, Ho, Wo, int(flip), int(align), stream())
    return out.cpu()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flipcat"])
@pytest.mark.parametrize("case", G.RESIZE_CASES, ids=RESIZE_IDS)
def test_resize_bilinear_within_the_fp32_bound(dev, case, flip):
    """Against bilinear64 within bilinear_bound at every pixel; the flipped half is bit-equal to the flip of the first half (odd
    widths included).  2x3 -> 1000x999 has 6 M outputs: past the 8192-block grid cap."""
    Hi, Wi, Ho, Wo, al = case
    B, C = 2, 3
    x = rnd(B, C, Hi, Wi, seed=Hi + Wo)
    got = _resize(dev, x, Ho, Wo, flip, al)
    assert bool(torch.isfinite(got).all())
    err = (got[:B].double() - G.bilinear64(x, Ho, Wo, al)).abs()
    assert ratio_report(f"resize_bilinear {RESIZE_IDS[G.RESIZE_CASES.index(case)]}", err, G.bilinear_bound(x, Ho, Wo, al)) <= 1.0
    if flip:
        assert same_bits(got[B:], got[:B].flip(-1))


def test_resize_bilinear_identity_and_constant_planes(dev):
    x = rnd(2, 3, 37, 53, seed=1)
    assert same_bits(_resize(dev, x, 37, 53, False, False), x)
    assert same_bits(_resize(dev, x, 37, 53, False, True), x)
    for c in (0.1, -3.3333333, 1e-30, 7e20):
        k = torch.full((1, 2, 5, 7), c)
        for (Ho, Wo, al) in ((13, 11, False), (3, 4, False), (13, 11, True)):
            got = _resize(dev, k, Ho, Wo, False, al)
            assert float((got.double() - float(k[0, 0, 0, 0])).abs().max()) <= 2 * EPS24 * abs(float(k[0, 0, 0, 0]))


# =========================================================================================== CAM: multi-scale fusion
def _fuse_inputs(sizes, B, C, row_off, ldc, seed, dev):
    """Token-major logits [2B][row_off + hs*ws][ldc] with NaN in the cls row and the padding columns; host and device copies."""
    host, device = [], []
    for i, (hs, ws) in enumerate(sizes):
        t = rnd(2 * B, row_off + hs * ws, ldc, seed=seed + i)
        t[:, :row_off] = NAN
        t[:, :, C:] = NAN
        host.append(t.view(-1, ldc))
        device.append(nan_in(t.view(-1, ldc), dev))
    return host, device


def _fuse(dev, lows, sizes, B, C, H, W, row_off, ldc, impl, band_blocks=0, cam_off=0):
    from dupl_amd import ops
    n = len(lows)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in lows])
    hs = (ctypes.c_int32 * max(n, 1))(*[s[0] for s in sizes])
    ws = (ctypes.c_int32 * max(n, 1))(*[s[1] for s in sizes])
    cam, mm = Guard((B, C, H, W), dev, front=PAD + cam_off), Guard((B * C, 2), dev)
    ops.L().dupl_cam_fuse(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(hs, ctypes.c_void_p), ctypes.cast(ws, ctypes.c_void_p),
                          n, row_off, ldc, cam.ptr, mm.ptr, B, C, H, W, int(impl), int(band_blocks), stream())
    return cam.cpu(), mm.cpu()


SCALES = [(28, 28), (14, 14), (42, 42), (9, 7)]


def _check_per_pixel(tag, dev, sizes, B, C, H, W, row_off, ldc, seed):
    host, device = _fuse_inputs(sizes, B, C, row_off, ldc, seed, dev)
    cam, mm = _fuse(dev, device, sizes, B, C, H, W, row_off, ldc, impl=1)
    ref, bound = G.cam_fuse64(host, sizes, B, C, H, W, row_off, ldc)
    assert bool(torch.isfinite(cam).all())
    assert ratio_report(tag, (cam.double() - ref).abs(), bound) <= 1.0
    flat = cam.view(B * C, -1)
    assert same_bits(mm, torch.stack((flat.amin(1), flat.amax(1)), 1)), "mm is the min / max of the kernel's own output"
    return device, cam, mm


@pytest.mark.parametrize("nscale", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", [(3, 4), (8, 96), (97, 500), (64, 64), (375, 450), (480, 640), (50, 1028)])
def test_cam_fuse_per_pixel_kernel_within_the_fp32_bound(dev, nscale, H, W):
    """The yardstick of the bit-identity tests (impl = 1) against cam_fuse64 within its bound; mm exact."""
    row_off, pad = (H + nscale) % 2, 3 * (W % 3 == 0)
    C = 3
    _check_per_pixel(f"cam_fuse per-pixel ns={nscale} {H}x{W}", dev, SCALES[:nscale], 1, C, H, W, row_off, C + pad, seed=H + W)


def _assert_choice_is_per_pixel(dev, device, sizes, B, C, H, W, row_off, ldc, band_blocks, cam_off=0):
    a_cam, a_mm = _fuse(dev, device, sizes, B, C, H, W, row_off, ldc, impl=0, band_blocks=band_blocks, cam_off=cam_off)
    b_cam, b_mm = _fuse(dev, device, sizes, B, C, H, W, row_off, ldc, impl=1)
    assert same_bits(a_cam, b_cam) and same_bits(a_mm, b_mm), (len(sizes), H, W, band_blocks, ldc, row_off, cam_off)
    return b_cam


FUSE_W = [4, 96, 500, 512, 516, 640, 1024, 1028, 450]
FUSE_H = [3, 8, 97, 375, 480]
FUSE_BB = [0, 1, 64, 4096, 1 << 20]


@pytest.mark.parametrize("nscale", [1, 2, 3, 4])
@pytest.mark.parametrize("W", FUSE_W)
def test_cam_fuse_library_choice_is_bit_identical(dev, nscale, W):
    """impl = 0 (the band kernel's 8 instantiations: NS 1-4 x PX 2 / 4, row phases where 256 % (W / PX) != 0; the per-pixel
    path for W = 1028 and 450) equals impl = 1 bit for bit in cam and mm, over H (< 8, not a multiple of the band), band_blocks,
    ldc (NaN padding columns) and row_off (NaN cls row).  Every H is crossed with every band_blocks."""
    B, C = 1, 2
    sizes = SCALES[:nscale]
    for ih, H in enumerate(FUSE_H):
        row_off, pad = (ih + nscale) % 2, 3 * ((ih + FUSE_W.index(W)) % 2)
        host, device = _fuse_inputs(sizes, B, C, row_off, C + pad, H + W + nscale, dev)
        ref_cam, ref_mm = _fuse(dev, device, sizes, B, C, H, W, row_off, C + pad, impl=1)
        for bb in FUSE_BB:
            cam, mm = _fuse(dev, device, sizes, B, C, H, W, row_off, C + pad, impl=0, band_blocks=bb)
            assert same_bits(cam, ref_cam) and same_bits(mm, ref_mm), (nscale, H, W, bb, pad, row_off)


@pytest.mark.parametrize("name,sizes,H,W,bb", [
    ("down-sampling hs > H", [(200, 30), (14, 14)], 97, 96, 0),
    ("halving loop, tall scale", [(300, 100)], 480, 512, 1),
    ("halving loop, ws = 2000", [(60, 2000), (14, 14)], 480, 512, 64),
    ("halving loop, ws = 2000, PX 4", [(60, 2000), (7, 9), (14, 14)], 375, 1024, 64),
    ("no fit at one row: ws = 3000", [(4, 3000), (14, 14)], 97, 512, 0),
    ("ws past 16 bits", [(1, 40000)], 8, 96, 0)])
def test_cam_fuse_launcher_paths(dev, name, sizes, H, W, bb):
    """The LDS-halving loop of the band choice, its fall-through to the per-pixel kernel and a down-sampling scale: the per-pixel
    kernel is within the float64 bound and the library's choice is bit-identical to it, with ldc = C + 3 and a NaN cls row."""
    B, C, row_off, ldc = 1, 2, 1, 5
    device, cam, _ = _check_per_pixel(f"cam_fuse {name}", dev, sizes, B, C, H, W, row_off, ldc, seed=H)
    got = _assert_choice_is_per_pixel(dev, device, sizes, B, C, H, W, row_off, ldc, bb)
    assert same_bits(got, cam)


def test_cam_fuse_unaligned_cam_takes_the_per_pixel_path(dev):
    """A cam that starts 8 bytes off 16-byte alignment cannot take the band kernel's vector stores; the result is the same bits."""
    B, C, H, W, sizes = 2, 3, 97, 512, SCALES[:3]
    host, device = _fuse_inputs(sizes, B, C, 1, C, 5, dev)
    aligned = _assert_choice_is_per_pixel(dev, device, sizes, B, C, H, W, 1, C, 0)
    off = _assert_choice_is_per_pixel(dev, device, sizes, B, C, H, W, 1, C, 0, cam_off=2)
    assert same_bits(aligned, off)


def test_cam_fuse_refuses_bad_arguments(dev):
    B, C, H, W, sizes = 1, 2, 8, 8, SCALES[:1]
    host, device = _fuse_inputs(sizes, B, C, 1, C, 5, dev)
    five = [device[0]] * 5
    for kw in (dict(lows=[], sizes=[], ldc=C, impl=0), dict(lows=five, sizes=[SCALES[0]] * 5, ldc=C, impl=0),
               dict(lows=device, sizes=sizes, ldc=C - 1, impl=0), dict(lows=device, sizes=sizes, ldc=C, impl=2)):
        with pytest.raises(RuntimeError, match="status -1"):
            _fuse(dev, kw["lows"], kw["sizes"], B, C, H, W, 1, kw["ldc"], kw["impl"])


def test_cam_fuse_nan_contract(dev):
    """The contract for non-finite logits: v_max3_f32 returns the largest non-NaN operand, so an up-sampled value that is NaN
    (any of its four taps NaN, whatever their weights) is DROPPED: the pixel gets the other image's value or 0 where torch's
    max / relu would give NaN.  Both kernels launder the same way: the output is finite, within the float64 bound of
    relu(max(.)) with NaN read as -inf, and the library's choice still equals the per-pixel kernel bit for bit."""
    B, C, H, W, sizes, row_off, ldc = 1, 3, 97, 96, SCALES[:3], 1, 4
    host, _ = _fuse_inputs(sizes, B, C, row_off, ldc, 9, dev)
    clean = [t.clone() for t in host]
    for i, (hs, ws) in enumerate(sizes):
        t = host[i].view(2 * B, row_off + hs * ws, ldc)
        t[0, row_off + (hs // 2) * ws + ws // 3, 0] = NAN                   # image only
        t[1, row_off + (hs // 3) * ws + ws // 2, 1] = NAN                   # flipped image only
        t[0, row_off + 1, 2] = NAN                                          # both, at mirrored positions
        t[1, row_off + ws - 2, 2] = NAN
    device = [nan_in(t, dev) for t in host]
    got = _assert_choice_is_per_pixel(dev, device, sizes, B, C, H, W, row_off, ldc, 0)
    assert bool(torch.isfinite(got).all())
    ref = torch.zeros(B, C, H, W, dtype=torch.float64)
    for t, (hs, ws) in zip(host, sizes):
        up = G.bilinear64(G._low_planes(t, hs, ws, 2 * B, C, row_off, ldc), H, W, False)
        up = torch.nan_to_num(up, nan=-math.inf)
        ref += torch.relu(torch.max(up[:B], up[B:].flip(-1)))
    _, bound = G.cam_fuse64(clean, sizes, B, C, H, W, row_off, ldc)
    # the bound of the clean planes, with M / L of a plane possibly set by the tap that is now NaN: take twice it
    assert ratio_report("cam_fuse NaN laundering", (got.double() - ref).abs(), 2.0 * bound) <= 1.0
    assert int((got != _fuse(dev, [nan_in(t, dev) for t in clean], sizes, B, C, H, W, row_off, ldc, 1)[0]).sum()) > 0


# =========================================================================================== CAM: normalise, labels, de-normalise
@pytest.mark.parametrize("given", [False, True], ids=["own-minmax", "given-minmax"])
@pytest.mark.parametrize("planes,H,W", [(3, 97, 131), (1, 1, 1), (5, 448, 448), (2, 7, 3)])
def test_cam_normalise_is_the_fp32_expression(dev, planes, H, W, given):
    """(cam - min) / ((max - min) + 1e-5) in fp32, bit for bit (one subtract, one add, one IEEE divide: the kernel's division
    compiles to the correctly rounded sequence); a constant plane comes out all 0; HW % 4 != 0 moves the float4 loop of the
    min / max pass off 16-byte alignment on every plane but the first."""
    from dupl_amd import ops
    cam = rnd(planes, H, W, seed=H) + 0.5              # negative values included
    cam[0] = 0.37                                      # a constant plane
    flat = cam.view(planes, -1)
    mn, mx = flat.amin(1), flat.amax(1)
    buf = Guard((planes, 1, H, W), dev, init=cam.view(planes, 1, H, W))
    mm = Guard((planes, 2), dev, init=torch.stack((mn, mx), 1) if given else None)
    ops.L().dupl_cam_minmax_normalise(buf.ptr, mm.ptr, planes, H * W, int(given), stream())
    assert same_bits(mm.cpu(), torch.stack((mn, mx), 1))
    den = (mx - mn) + torch.tensor(1e-5, dtype=torch.float32)
    want = (flat - mn[:, None]) / den[:, None]
    assert same_bits(buf.cpu().view(planes, -1), want)
    assert bool((buf.cpu()[0] == 0).all())


def _label_case(b, C, h, w, seed):
    """CAMs in [0, 1) with crafted pixels: values exactly on each threshold and one float either side of it, exact ties between
    two present classes, an all-zero pixel whose first class is absent, and one image without any class."""
    g = torch.Generator().manual_seed(seed)
    cam = torch.rand(b, C, h, w, generator=g)
    cls = (torch.rand(b, C, generator=g) < 0.3).float()
    cls[:, 1 % C] = 1.0
    cls[:, 0] = 0.0 if C > 1 else 1.0
    cls[b - 1] = 0.0                                   # no class at all in the last image
    bkg, low = float(np.float32(0.45)), float(np.float32(0.25))
    high = torch.tensor([float(np.float32(0.65 + 0.03 * i)) for i in range(b)])
    px = 0
    for i in range(b):
        present = torch.nonzero(cls[i]).flatten().tolist()
        if not present:
            continue
        for t in (bkg, float(high[i]), low):
            t32 = np.float32(t)
            for v in (t32, np.nextafter(t32, np.float32(2)), np.nextafter(t32, np.float32(-2))):
                for k in range(2):                     # as a single maximum, then tied between two present classes
                    y, x = (px // w) % h, px % w
                    cam[i, :, y, x] = 0.0
                    cam[i, present[0], y, x] = float(v)
                    if k and len(present) > 1:
                        cam[i, present[-1], y, x] = float(v)
                    px += 7
        y, x = (px // w) % h, px % w
        cam[i, :, y, x] = 0.0                          # present classes at exactly 0 tie with the absent class 0
        cam[i, 0, y, x] = 0.9
        px += 7
    return cam, cls, bkg, low, high


@pytest.mark.parametrize("b,C,h,w", [(3, 20, 28, 28), (2, 80, 97, 131), (3, 2, 840, 840)])
def test_cam_to_label_on_thresholds_and_ties(dev, b, C, h, w):
    """Labels and valid_cam equal the oracle's exactly on crafted threshold / tie pixels, with and without img_box, ignore_mid
    and want_valid; boxes empty, full and one pixel wide; 3 x 840 x 840 is past the grid cap."""
    from dupl_amd import ops
    from oracle import dupl_oracle as O
    cam, cls, bkg, low, high = _label_case(b, C, h, w, seed=h)
    boxes = torch.tensor([[0, h, 0, w], [h // 2, h // 2, 0, w], [1, h, w // 3, w // 3 + 1]][:b], dtype=torch.int32)
    cam_d, cls_d = nan_in(cam, dev), nan_in(cls, dev)
    boxes_d, high_d = boxes.to(dev), high.to(dev)
    for use_box, ignore_mid, want_valid in ((False, False, False), (True, False, True), (True, True, True), (True, True, False)):
        label = Guard((b, h, w), dev, torch.int64)
        valid = Guard((b, C, h, w), dev) if want_valid else None
        ops.L().dupl_cam_to_label(cam_d.data_ptr(), cls_d.data_ptr(), boxes_d.data_ptr() if use_box else None,
                                  high_d.data_ptr() if use_box else None, bkg, low, int(ignore_mid), 255, label.ptr,
                                  valid.ptr if valid is not None else None, b, C, h, w, stream())
        if use_box:
            rv, rl = O.cam_to_label(cam, cls, img_box=boxes.tolist(), bkg_thre=bkg, high_thre=high, low_thre=low,
                                    ignore_mid=ignore_mid, ignore_index=255)
        else:
            rv, rl = None, O.cam_to_label(cam, cls, bkg_thre=bkg)
        assert torch.equal(label.cpu(), rl), (use_box, ignore_mid)
        if valid is not None:
            assert same_bits(valid.cpu() + 0.0, rv + 0.0)


@pytest.mark.parametrize("B,HW,custom", [(2, 33 * 35, True), (2, 33 * 35, False), (3, 500 * 520, True)])
def test_denormalize_img_truncation_and_wrap(dev, B, HW, custom):
    """x * std + mean in fp32 (rounded product, then rounded sum), truncated toward zero and wrapped to 8 bits, / 255: values
    that land exactly on integers and one float below them, negative results and results above 255.  3 x 3 x 260 000 is past
    the grid cap."""
    from dupl_amd import ops
    mean, std = ([120.5, 110.25, 100.0], [60.0, 55.5, 50.25]) if custom else ([123.675, 116.28, 103.53], [58.395, 57.12, 57.375])
    x = rnd(B, 3, HW, 1, seed=HW, scale=2.5)           # |x| up to ~10: results from about -450 to 700
    m32, s32 = torch.tensor(mean), torch.tensor(std)
    for c in range(3):                                 # exact integers and just below them
        k = torch.arange(-40, 300, dtype=torch.float32)
        xi = (k - m32[c]) / s32[c]
        x[0, c, :k.numel(), 0] = xi
        x[0, c, k.numel():2 * k.numel(), 0] = torch.from_numpy(np.nextafter(xi.numpy(), np.float32(-1e9)))
    out = Guard((B, 3, HW, 1), dev)
    ms = (ctypes.c_float * 6)(*mean, *std) if custom else None
    ops.L().dupl_denormalize_img(nan_in(x, dev).data_ptr(), out.ptr, B, HW, ms, stream())
    v = x * s32.view(1, 3, 1, 1) + m32.view(1, 3, 1, 1)
    u8 = v.to(torch.int32) & 0xFF
    assert int((v < 0).sum()) > 0 and int((v > 256).sum()) > 0
    assert same_bits(out.cpu(), u8.float() / 255.0)


# =========================================================================================== decoder conv helpers
def _token_major(x, ld, lead, fill=NAN):
    """(B, Cin, h, w) -> the engine's layout [B][lead + h*w][ld] (lead cls rows, ld - Cin padding columns, both `fill`)."""
    B, Cin, h, w = x.shape
    t = torch.full((B, lead + h * w, ld), fill, dtype=torch.float32)
    t[:, lead:, :Cin] = x.permute(0, 2, 3, 1).reshape(B, h * w, Cin)
    return t


CONV_SMALL = [(2, 12, 12, 24, 5), (1, 6, 10, 7, 12), (3, 5, 9, 33, 1), (1, 1, 1, 4, 3)]
CONV_BIG = [(2, 28, 28, 768, 6), (8, 28, 28, 768, 12)]            # the second: 4.8 M elements, past the 16384-block grid cap
CONV_CONFIGS = ([s + (pad, lead, acc, relu) for s in CONV_SMALL for pad in (0, 5) for lead in (0, 1) for acc in (0, 1) for relu in (0, 1)]
                + [CONV_BIG[0] + (0, 0, 0, 0), CONV_BIG[0] + (5, 1, 1, 1), CONV_BIG[1] + (5, 1, 1, 1), CONV_BIG[1] + (0, 1, 0, 0)])


@pytest.mark.parametrize("B,h,w,Cin,dil,pad,lead,acc,relu", CONV_CONFIGS)
def test_im2col_col2im_dil3(dev, B, h, w, Cin, dil, pad, lead, acc, relu):
    """im2col_dil3 is bit-equal to F.unfold (column c*9 + tap) from a token-major operand with a row stride ld >= Cin and an
    image stride that skips a cls row -- NaN in every element it must skip.  col2im_dil3 against F.fold in float64 within
    9 * 2^-24 * fold(|dcol|) per element (8 roundings of the tap sum and one to spare); with accumulate the final add rounds
    start + s, so 2^-24 |start| joins the bound.  relu_of zeroes where !(v > 0): exact zeros, negative zeros and NaN.
    Elements outside the operand (padding columns, cls rows) keep their bits.  <im2col(x), c> = <x, col2im(c)> to the same bound."""
    from dupl_amd import ops
    ld, hw = Cin + pad, h * w
    x = rnd(B, Cin, h, w, seed=h + Cin)
    xt = nan_in(_token_major(x, ld, lead), dev)
    col = Guard((B * hw, Cin * 9), dev)
    ops.L().dupl_im2col_dil3(xt.data_ptr() + 4 * lead * ld, col.ptr, B, h, w, Cin, dil, ld, (lead + hw) * ld, stream())
    got_col = col.cpu()
    assert same_bits(got_col + 0.0, G.im2col64(x, dil) + 0.0)
    del col
    # the adjoint
    dcol = rnd(B * hw, Cin * 9, seed=dil)
    start = rnd(B, lead + hw, ld, seed=3)
    dx = Guard((B, lead + hw, ld), dev, init=start)
    mask_d = None
    keep = torch.ones(B, Cin, h, w, dtype=torch.bool)
    if relu:
        m = rnd(B, Cin, h, w, seed=4)
        sel = rndint(0, 8, B, Cin, h, w, seed=5)
        m[sel == 0], m[sel == 1], m[sel == 2] = 0.0, -0.0, NAN
        keep = m > 0
        mask_d = nan_in(_token_major(m, ld, lead), dev)
    ops.L().dupl_col2im_dil3(nan_in(dcol, dev).data_ptr(), dx.ptr + 4 * lead * ld, B, h, w, Cin, dil, ld, (lead + hw) * ld, acc,
                             mask_d.data_ptr() + 4 * lead * ld if relu else None, stream())
    got = dx.cpu()
    outside = torch.ones(B, lead + hw, ld, dtype=torch.bool)
    outside[:, lead:, :Cin] = False
    assert bool((bits(got)[outside] == bits(start)[outside]).all()), "col2im wrote outside its operand"
    got_x = got[:, lead:, :Cin].reshape(B, h, w, Cin).permute(0, 3, 1, 2).double()
    st_x = start[:, lead:, :Cin].reshape(B, h, w, Cin).permute(0, 3, 1, 2).double()
    s64 = G.col2im64(dcol.double(), B, h, w, dil) * keep
    bound = 9 * EPS24 * G.col2im64(dcol.double().abs(), B, h, w, dil)
    ref = s64 + st_x if acc else s64
    if acc:
        bound = bound + EPS24 * st_x.abs()
    assert bool(torch.isfinite(got_x).all())
    assert ratio_report(f"col2im_dil3 B={B} {h}x{w} Cin={Cin} dil={dil} ld+{pad} lead={lead} acc={acc} relu={relu}",
                        (got_x - ref).abs(), bound) <= 1.0
    if not relu:
        lhs = float((got_col.double() * dcol.double()).sum())
        rhs = float((x.double() * (got_x - st_x if acc else got_x)).sum())
        slack = float((x.double().abs() * (bound + (2 * EPS24 * st_x.abs() if acc else 0))).sum())
        assert abs(lhs - rhs) <= slack + 1e-12 * abs(lhs)


# =========================================================================================== eval
def _argmax_case(dev, tag, logits, H, W):
    from dupl_amd import ops
    B = logits.shape[0]
    out = Guard((B, H, W), dev, torch.int64)
    ops.L().dupl_upsample_argmax(nan_in(logits, dev).data_ptr(), out.ptr, B, logits.shape[1], logits.shape[2], logits.shape[3],
                                 H, W, stream())
    got = out.cpu()
    arg, margin, bound = G.upsample_argmax64(logits, H, W)
    excusable = margin <= 2.0 * bound
    n_ex, n_bad = int(excusable.sum()), int((got != arg).sum())
    print(f"upsample_argmax {tag}: {n_bad} pixels differ from float64, {n_ex} of {got.numel()} excusable "
          f"({100.0 * n_ex / got.numel():.4f} %)")
    assert not bool(((got != arg) & ~excusable).any()), "a pixel differs where the float64 margin exceeds twice the fp32 bound"
    assert n_ex <= 1e-3 * got.numel()


@pytest.mark.parametrize("B,C,h,w,H,W", [(3, 21, 13, 17, 75, 100), (2, 81, 30, 40, 480, 640), (1, 21, 47, 35, 375, 500),
                                         (2, 21, 28, 28, 448, 448), (1, 21, 40, 40, 23, 31), (1, 2, 1, 1, 5, 7),
                                         (1, 3, 50, 60, 1500, 1400)])
def test_upsample_argmax_differs_only_on_proven_ties(dev, B, C, h, w, H, W):
    """A pixel may differ from the float64 argmax only where the float64 top-1 - top-2 margin is <= twice its bilinear_bound, and
    such pixels are <= 0.1 % of the case.  1500 x 1400 is past the grid cap."""
    _argmax_case(dev, f"{B}x{C}x{h}x{w}->{H}x{W}", rnd(B, C, h, w, seed=h + W), H, W)


def test_upsample_argmax_lower_index_wins_identical_channels(dev):
    from dupl_amd import ops
    logits = rnd(2, 8, 13, 17, seed=1)
    logits[:, 2] += 100.0
    logits[:, 5] = logits[:, 2]
    out = Guard((2, 75, 100), dev, torch.int64)
    ops.L().dupl_upsample_argmax(nan_in(logits, dev).data_ptr(), out.ptr, 2, 8, 13, 17, 75, 100, stream())
    assert bool((out.cpu() == 2).all())


@pytest.mark.parametrize("B,C,H,W", [(2, 1, 5, 7), (3, 7, 33, 31), (2, 3, 1100, 1000)])
def test_argmax_channels_exact_with_ties(dev, B, C, H, W):
    from dupl_amd import ops
    x = torch.tensor([-2.0, -0.0, 0.0, 1.5])[rndint(0, 4, B, C, H, W, seed=C)]
    out = Guard((B, H, W), dev, torch.int64)
    ops.L().dupl_argmax_channels(nan_in(x, dev).data_ptr(), out.ptr, B, C, H * W, stream())
    # first maximum wins; -0.0 == 0.0 is a tie
    assert torch.equal(out.cpu(), (x + 0.0).argmax(1))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C,h,w,H,W", [(21, 24, 32, 375, 500), (81, 30, 40, 480, 640), (2, 1, 1, 3, 5)])
def test_msc_seg_accum_modes(dev, C, h, w, H, W, mode):
    """Modes 0 / 1 / 2 against msc_seg64 within its bound; mode 0 overwrites an acc full of NaN."""
    from dupl_amd import ops
    segs = rnd(2, C, h, w, seed=h + mode)
    acc0 = torch.full((1, C, H, W), NAN) if mode == 0 else rnd(1, C, H, W, seed=9)
    acc = Guard((1, C, H, W), dev, init=acc0)
    ops.msc_seg_accum_(acc.view, nan_in(segs, dev), mode)
    got = acc.cpu()
    ref, bound = G.msc_seg64(segs, acc0, mode)
    assert bool(torch.isfinite(got).all())
    assert ratio_report(f"msc_seg_accum mode {mode} C={C} {h}x{w}->{H}x{W}", (got[0].double() - ref).abs(), bound) <= 1.0


def test_msc_seg_accum_refuses_a_bad_mode(dev):
    from dupl_amd import ops
    acc = Guard((1, 2, 3, 5), dev)
    for mode in (-1, 3):
        with pytest.raises(RuntimeError, match="status -1"):
            ops.msc_seg_accum_(acc.view, nan_in(rnd(2, 2, 1, 1), dev), mode)
    torch.cuda.synchronize()
    assert acc.untouched()


@pytest.mark.parametrize("nc,n", [(1, 1), (1, 5000), (90, 1), (90, 200_003), (91, 200_003)])
def test_confusion_accum_ignores_out_of_range(dev, nc, n):
    """pred outside [0, nc) and negative gt are ignored; nc = 90 / 91 sit either side of the LDS-privatised limit."""
    from dupl_amd import ops
    gt, pred = rndint(-3, nc + 3, n, seed=nc), rndint(-3, nc + 3, n, seed=nc + 1)
    if n == 1:
        gt[0], pred[0] = nc - 1, 0
    start = rndint(0, 1000, nc, nc, seed=2)
    hist = Guard((nc, nc), dev, torch.int64, init=start)
    ops.confusion_accum(gt.to(dev), pred.to(dev), hist.view)
    ok = (gt >= 0) & (gt < nc) & (pred >= 0) & (pred < nc)
    want = start + torch.bincount(gt[ok] * nc + pred[ok], minlength=nc * nc).view(nc, nc)
    assert torch.equal(hist.cpu(), want)
    assert int(ok.sum()) >= 1 and (n == 1 or int((~ok).sum()) > 0)


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("C", [1, 20, 64, 65, 80, 200])
def test_multilabel_f1_accum(dev, B, C):
    """Rows with no positives, logits exactly 0 (not predicted), labels 0.5 (not a positive), onto a non-zero total; against
    numpy float64 within (B + 1) * 2^-24 * (B + |total0|): B atomic additions of values <= 1 and their own division."""
    from dupl_amd import ops
    logits = rnd(B, C, seed=B + C)
    label = (torch.rand(B, C, generator=torch.Generator().manual_seed(C)) < 0.3).float()
    sel = rndint(0, 6, B, C, seed=B)
    logits[sel == 0] = 0.0
    label[sel == 1] = 0.5
    label[B // 2] = 0.0
    logits[B // 2] = -1.0
    total0 = 3.25
    tot = Guard((1,), dev, init=torch.tensor([total0]))
    ops.multilabel_f1_accum(nan_in(logits, dev), nan_in(label, dev), tot.view)
    p, t = logits.numpy() > 0, label.numpy() == 1.0
    tp, fp, fn = (p & t).sum(1), (p & ~t).sum(1), (~p & t).sum(1)
    den = 2 * tp + fp + fn
    f1 = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    ref = total0 + float(f1.sum())
    bound = (B + 1) * EPS24 * (B + abs(total0))
    assert ratio_report(f"multilabel_f1 B={B} C={C}", torch.tensor([abs(float(tot.cpu()[0]) - ref)]), torch.tensor([bound])) <= 1.0


# =========================================================================================== element-wise helpers
EW_N = [1, 3, 255, 257, 2_097_153 + 5]


@pytest.mark.parametrize("n", EW_N)
def test_fill_axpy_scale_are_exact(dev, n):
    """One rounding each: fill writes the value, scale is one multiply, axpy one fused multiply-add (a * x + y rounded once:
    the product of two fp32 is exact in the 64-bit significand of the host's long double).  The last n is past the grid cap."""
    from dupl_amd import ops
    y0, x = rnd(n, seed=1), rnd(n, seed=2)
    a = 0.30000001192092896                            # a float32 value
    buf = Guard((n,), dev, init=y0)
    ops.fill_(buf.view, -2.5)
    assert bool((buf.cpu() == -2.5).all())
    buf = Guard((n,), dev, init=y0)
    ops.scale_(buf.view, a)
    assert same_bits(buf.cpu(), y0 * torch.tensor(a, dtype=torch.float32))
    buf = Guard((n,), dev, init=y0)
    ops.axpy_(buf.view, nan_in(x, dev), a)
    assert np.finfo(np.longdouble).nmant >= 63
    fma = (np.longdouble(np.float32(a)) * x.numpy().astype(np.longdouble) + y0.numpy().astype(np.longdouble)).astype(np.float32)
    assert same_bits(buf.cpu(), torch.from_numpy(fma))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("M,N", [(1, 1), (300, 70), (3137, 768), (20000, 3)])
def test_colsum_on_a_strided_operand(dev, M, N, acc):
    """ldx = N + 3 with NaN padding columns; within M * 2^-24 * (sum |x| + |start|) of float64."""
    from dupl_amd import ops
    x = rnd(M, N, seed=M)
    xs = torch.full((M, N + 3), NAN)
    xs[:, :N] = x
    start = rnd(N, seed=5)
    out = Guard((N,), dev, init=start)
    ops.colsum(nan_in(xs, dev)[:, :N], out.view, accumulate=bool(acc))
    ref = x.double().sum(0) + (start.double() if acc else 0.0)
    bound = M * EPS24 * (x.double().abs().sum(0) + (start.double().abs() if acc else 0.0))
    assert ratio_report(f"colsum {M}x{N} acc={acc}", (out.cpu().double() - ref).abs(), bound) <= 1.0
