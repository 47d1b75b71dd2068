"""-m gpu: the single-product forward GEMM (dupl_gemm16_desc.products = 1; csrc/gemm_split.hip gemm_f16x3_ring16_kernel<.., NP = 1>, tiles 18:
256 x 256 and 22: 256 x 128, four LDS stages each): C = act(alpha * post_scale * A_hi . B_hi^T + bias) (+ res), fp32 accumulation.

  1  against the fp64 product of the DECODED HI PLANES the kernel reads (+ the epilogue in fp64), inside the project's bar for an
     fp32-accumulating MFMA GEMM: err <= 2 x the exact-f32 kernel's error on the same (hi) operands + 1e-7 -- result, stored
     pre-activation, planes in both formats (2^-21 of the maximum), c_rows.  Shapes: one row / 8 columns / one k-tile, the edge tiles of
     test_gemm_mfma16_gpu.py, K = 96 (no multiple of 64), a step shape (394 x 576 x 192), and K = 32 S, 32 (S + 1) for the kernel's
     S = 4 stages (the steady loop is never entered / runs once).
  2  the kernel really is single-product: the inputs are such that the hi-plane reference lies >= 20 bars away from the
     full-precision reference (a condition on the inputs, asserted), so a three-product result cannot pass 1.
  3  bit identities: both tiles and tile 0; a row does not depend on M; products 0 and 3 are the launch without the argument.
  4  refusals before the launch, and NULL lo planes accepted.

Helpers, cases and the refusal bases are imported from tests/test_gemm_mfma16_gpu.py.  Every output is pre-filled with NaN."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gemm_mfma16_gpu as G
from test_gemm_mfma16_gpu import _nan, _planes_nan

pytestmark = pytest.mark.gpu

STAGES = 4      # G16H_STAGES of csrc/gemm_split.hip
SHAPES = [(1, 8, 32), (257, 264, 32), (300, 200, 96), (129, 128, 128), (513, 520, 160), (394, 576, 192),
          (257, 264, 32 * STAGES), (257, 264, 32 * (STAGES + 1))]
TILES = [18, 22]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """The operands of test_gemm_mfma16_gpu._case, the fp64 references on the decoded hi planes, and the exact-f32 kernel's error on
    those same operands: computed once per shape, read-only."""
    from dupl_amd import ops
    c = G._case(M, N, K)
    xh = c["xs"].planes[0].float() / 2.0 ** ops.EXP_ACT          # exact: a power-of-two scale of an fp16 value
    Wh = c["Ws"].planes[0].float() / 2.0 ** ops.EXP_W
    b, res = c["b"], c["res"]
    ref = xh.double() @ Wh.double().t() + b.double()
    want_g = F.gelu(ref)
    want = want_g + res.double()
    y32 = ops.linear(xh, Wh, b, gelu=True, res=res)
    e32 = float((y32.double() - want).abs().max()) / float(want.abs().max())
    pre32 = torch.empty(M, N, device=xh.device)
    y32g = ops.linear(xh, Wh, b, gelu=True, store_pre=pre32)
    e32_g = float((y32g.double() - want_g).abs().max()) / float(want_g.abs().max())
    e32_pre = float((pre32.double() - ref).abs().max()) / float(ref.abs().max())
    return dict(xs=c["xs"], Ws=c["Ws"], b=b, res=res, ref=ref, want=want, want_g=want_g, e32=e32, e32_g=e32_g, e32_pre=e32_pre,
                want_full=c["want"])


def _run(c, tile, M=None, products=1):
    """GELU + residual + stored pre-activation + format 1 planes, into NaN-filled outputs, on the first M rows of case c."""
    from dupl_amd import ops
    xs, res = c["xs"], c["res"]
    if M is not None:
        xs, res = ops.Split16View(xs, 0, M), res[:M]
    M, N = res.shape
    tn = dict(ops.GEMM16_TUNING, tile=tile)
    y, pre, y16 = _nan(M, N), _nan(M, N), _planes_nan(M, N, ops.EXP_ACT)
    kw = {} if products is None else {"products": products}
    ops.linear16(xs, c["Ws"], c["b"], gelu=True, res=res, store_pre=pre, out=y, out16=y16, tuning=tn, **kw)
    return y, pre, y16


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_f16_tiles_hold_the_fp32_accumulation_bar_on_the_hi_planes(dev, M, N, K, tile):
    from dupl_amd import ops
    c = _case(M, N, K)
    want, ref, e32 = c["want"], c["ref"], c["e32"]
    sc = float(want.abs().max())
    bar = 2.0 * e32 + 1e-7
    # 2: a condition on the inputs -- the full-precision reference is far outside the bar around the hi-plane reference
    dist = float((c["want_full"] - want).abs().max()) / sc
    print(f"{M}x{N}x{K}: |ref_hi - ref_full| {dist:.2e} of the maximum, bar {bar:.2e}")
    assert dist >= 20.0 * bar
    y, pre, y16 = _run(c, tile)
    e16 = float((y.double() - want).abs().max()) / sc
    epre = float((pre.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"{M}x{N}x{K} tile {tile}: f16 {e16:.2e}  f32 {e32:.2e};  pre-activation {epre:.2e}")
    assert e16 <= bar
    assert epre <= bar
    assert y16.exp == ops.EXP_ACT
    rec1 = (y16.planes[0].float() + y16.planes[1].float()) / 2.0 ** ops.EXP_ACT
    assert float((rec1 - y).abs().max()) <= 2.0 ** -21 * sc
    tn = dict(ops.GEMM16_TUNING, tile=tile)
    # planes in format 0, no fp32 output
    y16f0 = _planes_nan(M, N, 0)
    ops.linear16(c["xs"], c["Ws"], c["b"], gelu=True, res=c["res"], want_f32=False, out16=y16f0, tuning=tn, products=1)
    assert y16f0.exp == 0
    rec0 = y16f0.planes[0].float() + y16f0.planes[1].float() / 2048.0
    assert float((rec0 - y).abs().max()) <= 2.0 ** -21 * sc
    # GELU without residual on every row, then the same with the fp32 outputs limited to c_rows rows (planes for every row)
    yfull, prefull = _nan(M, N), _nan(M, N)
    ops.linear16(c["xs"], c["Ws"], c["b"], gelu=True, store_pre=prefull, out=yfull, tuning=tn, products=1)
    want_g, e32_g, e32_pre = c["want_g"], c["e32_g"], c["e32_pre"]
    eg = float((yfull.double() - want_g).abs().max()) / float(want_g.abs().max())
    ep = float((prefull.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"   GELU only: f16 {eg:.2e}  f32 {e32_g:.2e};  pre-activation: {ep:.2e}  f32 {e32_pre:.2e}")
    assert eg <= 2.0 * e32_g + 1e-7
    assert ep <= 2.0 * e32_pre + 1e-7
    crow = M // 3
    if crow:
        yc, prec, y16c = _nan(crow, N), _nan(crow, N), _planes_nan(M, N, ops.EXP_ACT)
        ops.linear16(c["xs"], c["Ws"], c["b"], gelu=True, store_pre=prec, out=yc, out16=y16c, c_rows=crow, tuning=tn, products=1)
        assert torch.equal(yc, yfull[:crow]) and torch.equal(prec, prefull[:crow])
        recc = (y16c.planes[0].float() + y16c.planes[1].float()) / 2.0 ** ops.EXP_ACT
        assert float((recc - yfull).abs().max()) <= 2.0 ** -21 * float(yfull.abs().max())


def test_f16_reads_format_0_planes_too(dev):
    """The same kernel on format 0 planes (hi = fp16(x), post_scale 1): the bar against the decoded hi planes, fp32 out + planes."""
    from dupl_amd import ops
    M, N, K = 300, 200, 96
    c = G._case(M, N, K)
    xs, Ws = ops.split16(c["x"]), ops.split16(c["W"])
    xh, Wh = xs.planes[0].float(), Ws.planes[0].float()
    want = F.gelu(xh.double() @ Wh.double().t() + c["b"].double()) + c["res"].double()
    sc = float(want.abs().max())
    e32 = float((ops.linear(xh, Wh, c["b"], gelu=True, res=c["res"]).double() - want).abs().max()) / sc
    for tile in TILES:
        y, y16 = _nan(M, N), _planes_nan(M, N, 0)
        ops.linear16(xs, Ws, c["b"], gelu=True, res=c["res"], out=y, out16=y16, tuning=dict(ops.GEMM16_TUNING, tile=tile), products=1)
        assert float((y.double() - want).abs().max()) / sc <= 2.0 * e32 + 1e-7
        assert float((y16.planes[0].float() + y16.planes[1].float() / 2048.0 - y).abs().max()) <= 2.0 ** -21 * sc


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_f16_tiles_are_bit_identical_to_each_other_and_to_tile_0(dev, M, N, K):
    outs = {t: _run(_case(M, N, K), t) for t in (18, 22, 0)}
    for t in (22, 0):
        assert torch.equal(outs[18][0], outs[t][0]) and torch.equal(outs[18][1], outs[t][1])
        assert torch.equal(outs[18][2].planes, outs[t][2].planes)
    assert not bool(torch.isnan(outs[18][0]).any())


@pytest.mark.parametrize("tile", TILES)
def test_f16_rows_do_not_depend_on_the_launch(dev, tile):
    """Rows 0 .. 128 of the M = 300 launch equal the same rows run as an M = 129 launch."""
    c = _case(300, 200, 96)
    full, part = _run(c, tile), _run(c, tile, M=129)
    assert torch.equal(full[0][:129], part[0]) and torch.equal(full[1][:129], part[1])
    assert torch.equal(full[2].planes[:, :129], part[2].planes)
    assert not bool(torch.isnan(part[0]).any())


@pytest.mark.parametrize("M,N,K", [(300, 200, 96), (513, 520, 160)])
def test_products_0_and_3_are_the_launch_without_the_argument(dev, M, N, K):
    """products = 0 and products = 3 give the bits of ops.linear16 without the argument (the f16x3 kernels), and those differ from
    the single-product result."""
    c = _case(M, N, K)
    base = _run(c, 0, products=None)
    for p in (0, 3):
        got = _run(c, 0, products=p)
        assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]) and torch.equal(base[2].planes, got[2].planes)
    assert not torch.equal(base[0], _run(c, 0)[0])


# ------------------------------------------------------------------------------------------ the launcher's argument checks
def _null_hi(d, keep):
    return None


F16_REFUSALS = {
    "products2": ("f1", G._set(products=2)),
    "products4": ("f1", G._set(products=4)),
    "products-1": ("f1", G._set(products=-1)),
    "accum": ("f1", G._set(products=1, flags=G._ACCUM, C_hi=None, C_lo=None, bias=None)),
    "kmajor-B": ("dgrad", G._set(products=1)),
    "kmajor-A-and-B": ("wgrad", G._set(products=1)),
    "A_hi-null": ("f1", G._set(products=1, A_hi=_null_hi)),
    "B_hi-null": ("f1", G._set(products=1, B_hi=_null_hi)),
    "tile9": ("f1", G._set(products=1, tile=9)),
    "out_exp3-fmt0": ("f0", G._set(products=1, out_exp=3)),
}


@pytest.mark.parametrize("case", list(F16_REFUSALS))
def test_f16_launcher_refuses_before_launching(dev, case):
    """Status -1 from a check that precedes the launch: C, aux and the result planes keep their NaN fill."""
    from dupl_amd import ops
    bases, keep = G._refusal_bases(dev)
    base, edit = F16_REFUSALS[case]
    d = bases[base]
    edit(d, keep)
    with pytest.raises(RuntimeError, match="status -1"):
        ops.L().dupl_gemm_f16x3(ctypes.byref(d), ops._stream())
    torch.cuda.synchronize()
    for name in ("C", "aux"):
        assert bool(torch.isnan(keep[name]).all()), f"{case}: {name} was written"
    for name in ("o1", "o0"):
        assert bool(torch.isnan(keep[name].planes).all()), f"{case}: planes {name} were written"


@pytest.mark.parametrize("base", ["f1", "f0"])
def test_f16_accepts_null_lo_planes(dev, base):
    """products = 1 never reads A_lo / B_lo: with both NULL the launch succeeds and gives the bits of the launch that passes them."""
    from dupl_amd import ops
    outs = []
    for null_lo in (False, True):
        bases, keep = G._refusal_bases(dev)
        d = bases[base]
        d.products = 1
        if null_lo:
            d.A_lo = d.B_lo = None
        ops.L().dupl_gemm_f16x3(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(keep["C"]).all())
        outs.append((keep["C"].clone(), keep["o0" if base == "f0" else "o1"].planes.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
