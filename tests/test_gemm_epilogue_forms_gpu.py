"""GPU: the compile-time epilogue forms of the split GEMMs (csrc/gemm_split.hip, EPI_P / EPI_G / EPI_R on gemm_f16x3_ring16_kernel,
EPI_D / EPI_A on the 16x16x32 k-major body) against the generic epilogue walk of the same body: dupl_gemm16_desc.tile 18 / 22 / 26 take
the form the launcher matches, 28 / 30 / 32 are the same bodies with EPI_GENERIC forced.

Every case launches one descriptor both ways into kernel_guard.Guard allocations and asks for
  * the same BITS in everything written: C, both result planes, the stored pre-activation, the amax word;
  * the sentinel untouched beyond M, beyond N, in the ld padding, in rows >= c_rows and around the allocation;
  * the standing bar of tests/test_gemm_km16_bodies_gpu.py against a float64 product of the values the operand planes represent:
    error / max |ref| <= 2 x the exact-f32 kernel's + 2e-7.

Shapes: K = 32 on the forward (one k-tile), 96 on the k-major body (its 3-stage prologue).  M x N is the FULL product of
  M in {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300} (the 16-row chunk, the 64-row pass, the 64- and 128-row wave tiles, the 256-row
  block) and N in {4, 60, 64, 68, 124, 128, 132, 252, 256, 260} (the 64-column wave tile, the 128- and 256-column blocks); the k-major
  body, whose N must be a multiple of 8, takes N in {8, 56, 64, 72, 120, 128, 136, 248, 256, 264}.
What is a covering subset is everything else, rotated with the position (i, j) of the shape in that product so that each value meets
every M and, over the M cases, every N:
  * leading dimensions: N + 8 where (i + j) is odd, else N;
  * c_rows of form G: {0, 1, 17, M}[(i + j) % 4] (capped at M), with STORE_PRE; every fifth (i + 2 j) without STORE_PRE;
  * out_exp of forms P and G: 3, and 0 (format 0 planes, the forms' second plane format: what the step's qkv writes) where (i + 3 j) % 7 == 0.
One case apart runs N = 6 (not a multiple of 4: the vector path must be refused) and one offsets every output base by 8 bytes (planes
stay 8-byte aligned, fp32 outputs are no longer 16-byte aligned: `vec` is false), both over all M.
The pair split (split2_f32_u / split2_f32, common.h) is tested through dupl_split_f16x2b / dupl_split_f16x2 against the scalar formula
written out in numpy."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from kernel_guard import PAD, Guard

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
NS = (4, 60, 64, 68, 124, 128, 132, 252, 256, 260)
NS_KM = (8, 56, 64, 72, 120, 128, 136, 248, 256, 264)
FWD_TILES = ((18, 28), (22, 30))        # (takes the form, generic forced)
KM_TILES = (26, 32)
EXP_A, EXP_W = 3, 9
SENT_F32, SENT_I32 = 0x7FC5A5A5, -0x5A5A5A5B


def _rep(p16):
    return (p16.planes[0].double() + p16.planes[1].double()).cpu() * (2.0 ** -p16.exp)


def _gelu(x):
    return x * 0.5 * (1 + torch.erf(x / 2 ** 0.5))


def _gelu_grad(p):
    return 0.5 * (1 + torch.erf(p / 2 ** 0.5)) + p * torch.exp(-0.5 * p * p) / (2 * torch.pi) ** 0.5


def _err(got, want):
    return float((got.double() - want).abs().max()) / float(want.abs().max())


@functools.lru_cache(maxsize=None)
def _fwd_operands(M, N):
    """x [M, 32], W [N, 32] as format 1 planes, bias [N], residual [M, N]; the float64 values they represent; the exact-f32 kernel's
    results on those values.  Built once per shape, never modified."""
    from dupl_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100000 + 1000 * M + N)
    x, W = torch.randn(M, 32, generator=g).to(dev), (torch.randn(N, 32, generator=g) * 0.03).to(dev)
    bias, res = (torch.randn(N, generator=g) * 0.3).to(dev), torch.randn(M, N, generator=g).to(dev)
    x16, W16 = ops.split16(x, exp=EXP_A), ops.split16(W, exp=EXP_W)
    torch.cuda.synchronize()
    x_r, W_r = _rep(x16), _rep(W16)
    pre = x_r @ W_r.t() + bias.double().cpu()
    x32, W32 = x_r.float().to(dev), W_r.float().to(dev)
    pre32 = torch.empty((M, N), device=dev)
    want = {"pre": pre, "P": pre, "G": _gelu(pre), "R": pre + res.double().cpu()}
    f32 = {"P": ops.linear(x32, W32, bias).cpu(), "G": ops.linear(x32, W32, bias, gelu=True, store_pre=pre32).cpu(),
           "R": ops.linear(x32, W32, bias, res=res).cpu(), "pre": pre32.cpu()}
    e32 = {k: _err(f32[k], want[k]) for k in want}
    return dict(x16=x16, W16=W16, bias=bias, res=res, want=want, e32=e32)


def _planes(rows, ld, dev, front):
    """fp16 [rows, ld] inside an int32 Guard (two halves per word)"""
    return Guard((rows * ld // 2,), dev, dtype=torch.int32, front=front)


def _halves(g, rows, ld):
    return g.view.cpu().view(torch.float16).view(rows, ld)


def _padded(t, ld, dev):
    """t [R, C] as the first C columns of a NaN-filled [R, ld] device tensor"""
    b = torch.full((t.shape[0], ld), float("nan"), device=dev)
    b[:, :t.shape[1]] = t
    return b


def _launch(d):
    from dupl_amd import ops
    rc = ops.L().dupl_gemm_f16x3(ctypes.byref(d), ops._stream())      # (the wrapper raises on a refused descriptor)
    assert rc == 0, ("dupl_gemm_f16x3 refused the descriptor", rc, d.tile)


def _fwd(o, M, N, form, tile, *, pad, off8, out_exp=3, c_rows=0, pre=True):
    """One forward launch of `form` on `tile`; returns {name: (Guard, rows, ld, valid rows)} of everything it may write."""
    from dupl_amd import _lib
    dev = o["bias"].device
    ld = N + pad
    d = _lib.Gemm16Desc()
    d.fmt, d.post_scale, d.K, d.M, d.N, d.lda, d.ldb, d.tile = 1, 2.0 ** -(EXP_A + EXP_W), 32, M, N, 32, 32, tile
    d.A_hi, d.A_lo, d.B_hi, d.B_lo = o["x16"].hi, o["x16"].lo, o["W16"].hi, o["W16"].lo
    d.bias = o["bias"].data_ptr()
    outs, keep = {}, []
    f32_front = PAD + (2 if off8 else 0)
    if form == "R":
        C = Guard((M, ld), dev, front=f32_front)
        res = _padded(o["res"], ld, dev)
        keep.append(res)
        d.C, d.ldc, d.res, d.ldr = C.ptr, ld, res.data_ptr(), ld
        outs["C"] = (C, M, ld, M)
    else:
        hi, lo = _planes(M, ld, dev, PAD + (2 if off8 else 0)), _planes(M, ld, dev, PAD + (2 if off8 else 0))
        d.C_hi, d.C_lo, d.ldo, d.out_exp = hi.ptr, lo.ptr, ld, out_exp
        outs["hi"], outs["lo"] = (hi, M, ld, M), (lo, M, ld, M)
        if form == "G":
            d.flags = _lib.GEMM_GELU
            d.c_rows = c_rows
            if pre:
                rows = c_rows or M
                aux = Guard((rows, ld), dev, front=f32_front)
                d.flags |= _lib.GEMM_STORE_PRE
                d.aux, d.ldaux = aux.ptr, ld
                outs["aux"] = (aux, rows, ld, rows)
    _launch(d)
    torch.cuda.synchronize()
    return outs, keep


def _same_and_fenced(tag, a, b, N):
    """Both launches left the same bits in their whole allocations, and the sentinel outside the [valid rows, N] they own."""
    for name, (ga, rows, ld, valid) in a.items():
        gb = b[name][0]
        assert ga.intact() and gb.intact(), (tag, name, "wrote outside the output")
        ia, ib = ga.buf.view(ga.itype).cpu(), gb.buf.view(gb.itype).cpu()
        assert torch.equal(ia, ib), (tag, name, "form and generic walk differ", int((ia != ib).sum()))
        if name == "amax":
            continue
        if name in ("hi", "lo"):        # planes: halves
            body = ga.view.cpu().view(torch.int16).view(rows, ld)
            pat = torch.tensor([SENT_I32], dtype=torch.int32).view(torch.int16)[0]
        else:
            body = ga.view.cpu().view(torch.int32).view(rows, ld)
            pat = torch.tensor([SENT_F32], dtype=torch.int32)[0]
        assert bool((body[:, N:] == pat).all()) and bool((body[valid:] == pat).all()), (tag, name, "wrote into the padding")


def _value(outs, out_exp, M, N):
    if "C" in outs:
        return outs["C"][0].view.cpu()[:, :N]
    hi, lo = (_halves(outs[k][0], M, outs[k][2])[:, :N].double() for k in ("hi", "lo"))
    return (hi + lo) * 2.0 ** -out_exp if out_exp else hi + lo / 2048.0


def _fwd_case(M, N, i, j, *, off8=False, forms=("P", "G", "R")):
    o = _fwd_operands(M, N)
    pad = 8 if (i + j) & 1 else 0
    c_rows = min((0, 1, 17, M)[(i + j) % 4], M)
    pre = (i + 2 * j) % 5 != 0
    out_exp = 0 if (i + 3 * j) % 7 == 0 else 3
    for spec, gen in FWD_TILES:
        for form in forms:
            kw = dict(pad=pad, off8=off8)
            if form != "R":
                kw["out_exp"] = out_exp
            if form == "G":
                kw.update(c_rows=c_rows if pre else 0, pre=pre)
            tag = f"fwd {form} t{spec} {M}x{N} {kw}"
            a, keep_a = _fwd(o, M, N, form, spec, **kw)
            b, keep_b = _fwd(o, M, N, form, gen, **kw)
            _same_and_fenced(tag, a, b, N)
            e = _err(_value(a, kw.get("out_exp", 0), M, N), o["want"][form])
            assert e <= 2.0 * o["e32"][form] + 2e-7, (tag, e, o["e32"][form])
            if "aux" in a:
                rows = a["aux"][1]
                e = _err(a["aux"][0].view.cpu()[:, :N], o["want"]["pre"][:rows])
                assert e <= 2.0 * o["e32"]["pre"] + 2e-7, (tag, "pre", e)


@pytest.mark.parametrize("M", MS)
def test_forward_forms_match_the_generic_walk(dev, M):
    """Forms P, G, R on both forward tiles over every N of the product (module docstring: what rotates with the shape)."""
    i = MS.index(M)
    for j, N in enumerate(NS):
        _fwd_case(M, N, i, j)


def test_forward_forms_refuse_the_vector_path(dev):
    """N = 6 (no multiple of 4) and output bases offset by 8 bytes: `vec` is false, every element goes out singly, in every form."""
    for i, M in enumerate(MS):
        _fwd_case(M, 6, i, 0)
        _fwd_case(M, 132, i, 1, off8=True)


# ------------------------------------------------------------------------------------------ k-major data gradients (D, A)
@functools.lru_cache(maxsize=None)
def _km_operands(M, N):
    """dy [M, 96] (scaled format 1 gradient planes) and W [96, N] read k-major, pre [M, N]: test_gemm_km16_gpu's operands"""
    from test_gemm_km16_gpu import _operands
    return _operands(M, 96, N)


def _km(o, M, N, dgelu, tile, *, pad, off8):
    from dupl_amd import _lib
    dev = o["pre"].device
    ld = N + pad
    d = _lib.Gemm16Desc()
    dy, W = o["dy16"], o["W16"]
    d.fmt, d.post_scale, d.K, d.M, d.N, d.tile = 1, 2.0 ** -(dy.exp + W.exp), 96, M, N, tile
    d.A_hi, d.A_lo, d.B_hi, d.B_lo, d.lda, d.ldb = dy.hi, dy.lo, W.hi, W.lo, dy.cols, W.cols
    d.b_layout, d.kb_valid, d.alpha_dev = 1, 96, o["alpha"]
    C = Guard((M, ld), dev, front=PAD + (2 if off8 else 0))
    amax = Guard((1,), dev, dtype=torch.int32, init=torch.zeros(1, dtype=torch.int32))
    d.C, d.ldc, d.amax_out = C.ptr, ld, amax.ptr
    keep = []
    if dgelu:
        aux = _padded(o["pre"], ld, dev)
        keep.append(aux)
        d.flags, d.aux, d.ldaux = _lib.GEMM_MUL_DGELU, aux.data_ptr(), ld
    _launch(d)
    torch.cuda.synchronize()
    return {"C": (C, M, ld, M), "amax": (amax, 1, 1, 1)}, keep


@pytest.mark.parametrize("M", MS)
def test_kmajor_forms_match_the_generic_walk(dev, M):
    """Forms D (gelu') and A on the 16x16x32 body, with the amax word: max |dx| exactly, in both launches."""
    from dupl_amd import ops
    i = MS.index(M)
    for j, N in enumerate(NS_KM):
        o = _km_operands(M, N)
        want = o["dy_r"] @ o["W_r"]
        for dgelu in (False, True):
            w = want * _gelu_grad(o["pre"].double().cpu()) if dgelu else want
            e32 = _err(ops.linear_dgrad(o["dy32"], o["W32"], dgelu_of=o["pre"] if dgelu else None).cpu(), w)
            for off8 in ((False, True) if j == 6 else (False,)):
                kw = dict(pad=8 if (i + j) & 1 else 0, off8=off8)
                tag = f"km {'D' if dgelu else 'A'} {M}x{N} {kw}"
                a, ka = _km(o, M, N, dgelu, KM_TILES[0], **kw)
                b, kb = _km(o, M, N, dgelu, KM_TILES[1], **kw)
                _same_and_fenced(tag, a, b, N)
                dx = a["C"][0].view.cpu()[:, :N]
                assert float(a["amax"][0].view.cpu().view(torch.float32)) == float(dx.abs().max()) > 0, tag
                e = _err(dx, w)
                assert e <= 2.0 * e32 + 2e-7, (tag, e, e32)


# ------------------------------------------------------------------------------------------ the pair split
def _split_ref(x, scale, fmt1):
    """split_f32_u / split_f32 (common.h), the scalar form, in numpy: IEEE fp32 operations, round-to-nearest-even conversions"""
    with np.errstate(all="ignore"):
        x = (x * np.float32(scale)).astype(np.float32) if fmt1 else x
        c = np.minimum(np.maximum(x, np.float32(-65504.0)), np.float32(65504.0))        # (fmaxf / fminf return the non-NaN operand ...
        x = np.where(np.abs(x) <= np.finfo(np.float32).max, c, x).astype(np.float32)  #  ... but NaN and Inf pass through here)
        hi = x.astype(np.float16)
        r = (x - hi.astype(np.float32)).astype(np.float32)
        lo = (r if fmt1 else (r * np.float32(2048.0)).astype(np.float32)).astype(np.float16)
    return hi, lo


def test_pair_split_is_the_scalar_split(dev):
    """dupl_split_f16x2 (format 0) and dupl_split_f16x2b (format 1, 2^0 / 2^3 / 2^9) now split on pairs: the same bits as the scalar
    formula on +-65504, the values around it, the largest floats, +-0, fp16- and fp32-subnormals, Inf, NaN and 4096 random values of
    every magnitude; NaN positions agree (payloads are not compared)."""
    from dupl_amd import ops
    f = np.float32
    edge = [65504.0, 65505.0, 65519.99, 65520.0, 65536.0, 7.0e4, 3.0e38, 3.4028235e38, 8188.0, 8190.0, 127.96875, 0.0, 6.1e-5, 6.0e-8,
            2.9e-8, 1.0e-40, 1.4e-45, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 2049.0 / 2048.0]
    g = np.random.default_rng(7)
    rnd = (g.standard_normal(4096) * np.exp2(g.integers(-30, 17, 4096))).astype(f)
    x = np.concatenate([np.array(edge, f), -np.array(edge, f), np.array([np.inf, -np.inf, np.nan, -np.nan], f), rnd])
    x = np.concatenate([x, x[::-1][:-1], np.zeros((-(2 * len(x) - 1)) % 4, f)])      # every value in an even and in an odd pair slot
    xd = torch.from_numpy(x).to(dev)
    for exp in (None, 0, 3, 9):
        hi, lo = _planes(1, len(x), dev, PAD), _planes(1, len(x), dev, PAD)
        if exp is None:
            ops.L().dupl_split_f16x2(xd.data_ptr(), hi.ptr, lo.ptr, len(x), ops._stream())
        else:
            ops.L().dupl_split_f16x2b(xd.data_ptr(), hi.ptr, lo.ptr, len(x), exp, ops._stream())
        torch.cuda.synchronize()
        assert hi.intact() and lo.intact()
        want_hi, want_lo = _split_ref(x, 2.0 ** (exp or 0), exp is not None)
        for name, got, want in (("hi", hi, want_hi), ("lo", lo, want_lo)):
            got = got.view.cpu().view(torch.float16).numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (exp, name)
            bad = (got.view(np.uint16) != want.view(np.uint16)) & ~nan
            assert not bad.any(), (exp, name, x[bad][:8], got[bad][:8], want[bad][:8])
