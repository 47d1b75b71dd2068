"""The format 1 forward GEMMs on v_mfma_f32_16x16x32_f16 (dupl_gemm16_desc.tile 18: 256 x 256, 22: 256 x 128; csrc/gemm_split.hip
gemm_f16x3_ring16_kernel): the fp64 bar of test_gemm_f16x3_format1_is_fp32_equivalent at the edges of the pipeline -- one k-tile (the
prologue with fewer tiles than stages, a one-row second row tile, an 8-column edge), exactly as many k-tiles as stages (the steady
loop is never entered), one steady iteration, several tiles per XCD, a step shape -- with every output pre-filled with NaN, and the
bit identities the launcher relies on: both tiles give the same bits, a row's result does not depend on the launch it rides in, and
tile 0 is the code it resolves to.
The launcher's row split (more than 256 tiles of 256 x 256: one 256 x 256 launch for the full rounds and one 256 x 128 launch for the
remaining rows, on the same two kernels) is not reached by these shapes; it is covered by the tests that run tile 0 at large row
counts, test_kernels_gpu.py::test_gemm_f16x3_format1_at_the_coco8_row_counts and the merged ms-CAM / training pass of the step
tests."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(257, 264, 32), (300, 200, 96), (129, 128, 128), (513, 520, 160), (1570, 768, 768)]
TILES = [18, 22]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Operands, their planes, the fp64 references and the exact-f32 kernel's error: computed once per shape, read-only."""
    from dupl_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(dev)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    xs, Ws = ops.split16(x, exp=ops.EXP_ACT), ops.split16(W, exp=ops.EXP_W)
    ref = x.double() @ W.double().t() + b.double()
    want = F.gelu(ref) + res.double()
    y32 = ops.linear(x, W, b, gelu=True, res=res)
    e32 = float((y32.double() - want).abs().max()) / float(want.abs().max())
    # the exact-f32 kernel's error on the epilogue of the c_rows case (GELU, no residual) and on its stored pre-activation
    want_g = F.gelu(ref)
    pre32 = torch.empty(M, N, device=dev)
    y32g = ops.linear(x, W, b, gelu=True, store_pre=pre32)
    e32_g = float((y32g.double() - want_g).abs().max()) / float(want_g.abs().max())
    e32_pre = float((pre32.double() - ref).abs().max()) / float(ref.abs().max())
    return dict(x=x, W=W, b=b, res=res, xs=xs, Ws=Ws, ref=ref, want=want, e32=e32, want_g=want_g, e32_g=e32_g, e32_pre=e32_pre)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=torch.device("cuda", 0))


def _planes_nan(M, N, exp):
    from dupl_amd import ops
    p = ops.split16_empty(M, N, torch.device("cuda", 0), exp)
    p.planes.fill_(float("nan"))
    return p


def _run(c, tile, M=None):
    """GELU + residual + stored pre-activation + format 1 planes, into NaN-filled outputs, on the first M rows of case c."""
    from dupl_amd import ops
    xs, res = c["xs"], c["res"]
    if M is not None:
        xs, res = ops.Split16View(xs, 0, M), res[:M]
    M = res.shape[0]
    N = res.shape[1]
    ops.GEMM16_TUNING["tile"] = tile
    try:
        y, pre, y16 = _nan(M, N), _nan(M, N), _planes_nan(M, N, ops.EXP_ACT)
        ops.linear16(xs, c["Ws"], c["b"], gelu=True, res=res, store_pre=pre, out=y, out16=y16)
    finally:
        ops.GEMM16_TUNING["tile"] = 0
    return y, pre, y16


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mfma16_tiles_are_fp32_equivalent(dev, M, N, K, tile):
    """Error vs fp64 <= 2x the exact-f32 MFMA kernel's + 1e-7 for the result, the stored pre-activation and the planes in both formats,
    and with the fp32 outputs limited to c_rows = M // 3 rows; a NaN left anywhere in an output fails the comparison."""
    from dupl_amd import ops
    c = _case(M, N, K)
    want, ref, e32 = c["want"], c["ref"], c["e32"]
    sc = float(want.abs().max())
    y, pre, y16 = _run(c, tile)
    e16 = float((y.double() - want).abs().max()) / sc
    print(f"{M}x{N}x{K} tile {tile}: 16x16x32 {e16:.2e}  f32 {e32:.2e}")
    assert e16 <= 2.0 * e32 + 1e-7
    assert float((pre.double() - ref).abs().max()) / float(ref.abs().max()) <= 2.0 * e32 + 1e-7
    assert y16.exp == ops.EXP_ACT
    rec1 = (y16.planes[0].float() + y16.planes[1].float()) / 2.0 ** ops.EXP_ACT
    assert float((rec1 - y).abs().max()) <= 2.0 ** -21 * sc
    ops.GEMM16_TUNING["tile"] = tile
    try:
        # planes in format 0, no fp32 output
        y16f0 = _planes_nan(M, N, 0)
        ops.linear16(c["xs"], c["Ws"], c["b"], gelu=True, res=c["res"], want_f32=False, out16=y16f0)
        # GELU without residual on every row, then the same with the fp32 outputs limited to c_rows rows (planes for every row)
        yfull, prefull = _nan(M, N), _nan(M, N)
        ops.linear16(c["xs"], c["Ws"], c["b"], gelu=True, store_pre=prefull, out=yfull)
        crow = M // 3
        yc, prec, y16c = _nan(crow, N), _nan(crow, N), _planes_nan(M, N, ops.EXP_ACT)
        ops.linear16(c["xs"], c["Ws"], c["b"], gelu=True, store_pre=prec, out=yc, out16=y16c, c_rows=crow)
    finally:
        ops.GEMM16_TUNING["tile"] = 0
    assert y16f0.exp == 0
    rec0 = y16f0.planes[0].float() + y16f0.planes[1].float() / 2048.0
    assert float((rec0 - y).abs().max()) <= 2.0 ** -21 * sc
    # the c_rows case against its own epilogue's references: the full-row run holds the bar, the limited run equals its rows
    want_g, e32_g, e32_pre = c["want_g"], c["e32_g"], c["e32_pre"]
    eg = float((yfull.double() - want_g).abs().max()) / float(want_g.abs().max())
    ep = float((prefull.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"   GELU only: 16x16x32 {eg:.2e}  f32 {e32_g:.2e};  pre-activation: {ep:.2e}  f32 {e32_pre:.2e}")
    assert eg <= 2.0 * e32_g + 1e-7
    assert ep <= 2.0 * e32_pre + 1e-7
    assert torch.equal(yc, yfull[:crow]) and torch.equal(prec, prefull[:crow])
    recc = (y16c.planes[0].float() + y16c.planes[1].float()) / 2.0 ** ops.EXP_ACT
    assert float((recc - yfull).abs().max()) <= 2.0 ** -21 * float(yfull.abs().max())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mfma16_tiles_are_bit_identical_to_each_other_and_to_tile_0(dev, M, N, K):
    outs = {t: _run(_case(M, N, K), t) for t in (18, 22, 0)}
    for t in (22, 0):
        assert torch.equal(outs[18][0], outs[t][0]) and torch.equal(outs[18][1], outs[t][1])
        assert torch.equal(outs[18][2].planes, outs[t][2].planes)
    assert not bool(torch.isnan(outs[18][0]).any())


@pytest.mark.parametrize("tile", TILES)
def test_mfma16_rows_do_not_depend_on_the_launch(dev, tile):
    """Rows 0 .. 128 of the M = 300 launch equal the same rows run as an M = 129 launch."""
    c = _case(300, 200, 96)
    full, part = _run(c, tile), _run(c, tile, M=129)
    assert torch.equal(full[0][:129], part[0]) and torch.equal(full[1][:129], part[1])
    assert torch.equal(full[2].planes[:, :129], part[2].planes)
    assert not bool(torch.isnan(part[0]).any())


@pytest.mark.parametrize("tile", TILES)
def test_mfma16_element_wise_store_path(dev, tile):
    """N = 202 is no multiple of 4: every store of the epilogue goes out element-wise (fp32 out only)."""
    from dupl_amd import ops
    M, N, K = 300, 202, 96
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(dev)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(dev)
    want = F.gelu(x.double() @ W.double().t() + b.double()) + res.double()
    sc = float(want.abs().max())
    y = _nan(M, N)
    ops.GEMM16_TUNING["tile"] = tile
    try:
        ops.linear16(ops.split16(x, exp=ops.EXP_ACT), ops.split16(W, exp=ops.EXP_W), b, gelu=True, res=res, out=y)
    finally:
        ops.GEMM16_TUNING["tile"] = 0
    y32 = ops.linear(x, W, b, gelu=True, res=res)
    e16, e32 = float((y.double() - want).abs().max()) / sc, float((y32.double() - want).abs().max()) / sc
    print(f"{M}x{N}x{K} tile {tile}: 16x16x32 {e16:.2e}  f32 {e32:.2e}")
    assert e16 <= 2.0 * e32 + 1e-7


# ------------------------------------------------------------------------------------------ the launchers' argument checks
def _refusal_bases(dev):
    """Four valid 64 x 64 x 96 descriptors, every destination NaN-filled: f1 = format 1, k-contiguous, bias + planes out (the forward);
    f0 = the same on format 0 planes; dgrad = f1 with a k-major B; wgrad = format 1, both operands k-major, C += (what the group
    entry point takes)."""
    from dupl_amd import ops, _lib
    M = N = 64
    K = 96
    g = torch.Generator().manual_seed(96)
    x, xt = torch.randn(M, K, generator=g).to(dev), torch.randn(K, M, generator=g).to(dev)
    keep = dict(x1=ops.split16(x, exp=ops.EXP_ACT), x0=ops.split16(x), xt1=ops.split16(xt, exp=ops.EXP_ACT),
                bias=torch.zeros(N, device=dev), C=_nan(M, N), aux=_nan(M, N), o1=_planes_nan(M, N, ops.EXP_ACT), o0=_planes_nan(M, N, 0))

    def desc(a, b, lda, out16):
        d = _lib.Gemm16Desc()
        d.A_hi, d.A_lo, d.B_hi, d.B_lo = a.hi, a.lo, b.hi, b.lo
        d.C = keep["C"].data_ptr()
        if out16 is not None:
            d.C_hi, d.C_lo, d.out_exp = out16.hi, out16.lo, out16.exp
        d.M, d.N, d.K = M, N, K
        d.lda = d.ldb = lda
        d.ldc = d.ldo = d.ldaux = N
        d.fmt = a.fmt
        d.post_scale = 2.0 ** -(a.exp + b.exp)
        return d

    f1, f0 = desc(keep["x1"], keep["x1"], K, keep["o1"]), desc(keep["x0"], keep["x0"], K, keep["o0"])
    dgrad, wgrad = desc(keep["x1"], keep["xt1"], K, keep["o1"]), desc(keep["xt1"], keep["xt1"], M, None)
    dgrad.ldb, dgrad.b_layout = N, 1
    wgrad.flags, wgrad.a_layout, wgrad.b_layout = _lib.GEMM_ACCUM, 1, 1
    for d in (f1, f0, dgrad):
        d.bias, d.aux = keep["bias"].data_ptr(), keep["aux"].data_ptr()
    return dict(f1=f1, f0=f0, dgrad=dgrad, wgrad=wgrad), keep


def _set(**fields):
    def edit(d, keep):
        for k, v in fields.items():
            setattr(d, k, v(d, keep) if callable(v) else v)
    return edit


def _flag(name):
    """dupl_amd._lib.<name>, looked up when the case runs."""
    def get(d, keep):
        from dupl_amd import _lib
        return getattr(_lib, name)
    return get


_ACCUM, _PRE = _flag("GEMM_ACCUM"), _flag("GEMM_STORE_PRE")
# case -> (base descriptor, the edit that breaks it).  More than one field is set only where the broken one cannot be reached otherwise:
# the accumulating cases drop what ACCUM does not take besides the field in question.
GEMM16_REFUSALS = {
    "struct_size": ("f1", _set(struct_size=lambda d, k: d.struct_size + 8)),
    "K100": ("f1", _set(K=100)),
    "lda100": ("f1", _set(lda=100)),
    "A_hi-plus-2-bytes": ("f1", _set(A_hi=lambda d, k: d.A_hi + 2)),
    "tile4": ("f1", _set(tile=4)),
    "tile9": ("f1", _set(tile=9)),
    "persist_blocks12": ("f1", _set(persist_blocks=12)),
    "concurrency9": ("f1", _set(concurrency=9)),
    "no-C-no-C_hi": ("f1", _set(C=None, C_hi=None, C_lo=None)),
    "C_hi-without-C_lo": ("f1", _set(C_lo=None)),
    "store_pre-without-aux": ("f1", _set(flags=_PRE, aux=None)),
    "unknown-flag": ("f1", _set(flags=1 << 12)),
    "accum-with-bias": ("f0", _set(flags=_ACCUM, C_hi=None, C_lo=None)),
    "fmt2": ("f1", _set(fmt=2)),
    "out_exp3-fmt0": ("f0", _set(out_exp=3)),
    "fmt1-kcontig-accum": ("f1", _set(flags=_ACCUM, C_hi=None, C_lo=None, bias=None)),
    "a_layout-fmt0": ("f0", _set(a_layout=1, lda=64)),
    "b_layout-N60": ("dgrad", _set(N=60)),
    "kmajor-K64": ("dgrad", _set(K=64)),
    "ka_valid-without-a_layout": ("dgrad", _set(ka_valid=64)),
    "group-n0": ("wgrad", _set()),
    "group-n-above-max": ("wgrad", _set()),
    "group-flags0": ("wgrad", _set(flags=0)),
    "group-fmt0": ("wgrad", _set(fmt=0)),
}


@pytest.mark.parametrize("case", list(GEMM16_REFUSALS))
def test_gemm16_launchers_refuse_bad_descriptors(dev, case):
    """dupl_gemm_f16x3 / dupl_gemm_f16x3_group answer every broken descriptor with status -1 from a check that precedes the launch:
    C, aux and the result planes keep their NaN fill."""
    import ctypes
    from dupl_amd import ops, _lib
    bases, keep = _refusal_bases(dev)
    base, edit = GEMM16_REFUSALS[case]
    d = bases[base]
    edit(d, keep)
    if case.startswith("group-"):
        n = {"group-n0": 0, "group-n-above-max": _lib.GEMM16_GROUP_MAX + 1}.get(case, 1)
        arr = (_lib.Gemm16Desc * max(n, 1))(*([d] * max(n, 1)))

        def call():
            ops.L().dupl_gemm_f16x3_group(arr, n, ops._stream())
    else:
        def call():
            ops.L().dupl_gemm_f16x3(ctypes.byref(d), ops._stream())
    with pytest.raises(RuntimeError, match="status -1"):
        call()
    torch.cuda.synchronize()
    for name in ("C", "aux"):
        assert bool(torch.isnan(keep[name]).all()), f"{case}: {name} was written"
    for name in ("o1", "o0"):
        assert bool(torch.isnan(keep[name].planes).all()), f"{case}: planes {name} were written"


def test_gemm16_refusal_bases_are_accepted(dev):
    """The descriptors the refusal cases start from are valid: each launches (status 0) and overwrites its NaN-filled C."""
    import ctypes
    from dupl_amd import ops, _lib
    for name in ("f1", "f0", "dgrad", "wgrad", "group"):
        bases, keep = _refusal_bases(dev)
        d = bases["wgrad" if name == "group" else name]
        if d.flags & _lib.GEMM_ACCUM:
            keep["C"].zero_()
        if name == "group":
            ops.L().dupl_gemm_f16x3_group((_lib.Gemm16Desc * 1)(d), 1, ops._stream())
        else:
            ops.L().dupl_gemm_f16x3(ctypes.byref(d), ops._stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(keep["C"]).all()), name
        if not d.flags & _lib.GEMM_ACCUM:
            assert bool(torch.isfinite(keep["o0" if name == "f0" else "o1"].planes.float()).all()), name
