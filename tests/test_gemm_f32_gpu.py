"""-m gpu: the exact-fp32 GEMM (csrc/gemm.hip, dupl_gemm_f32) at its edges -- the kernel every "2 x the exact-f32 kernel's error" bar of
the split kernels is measured with.  Case table, planner, float64 reference and bound: tests/gemm32_ref.py (checked on the host by
tests/test_gemm32_ref_host.py: the table reaches all 36 instantiations, the bound separates a correct fp32 chain from four mistakes).

  a  accuracy: every element within the element-wise bound gamma(K + 2) * sum_k |a| |b| of float64, every case x 4 layouts x the
     three forced tiles (the 128-row tiles run nowhere else), unit-scale and heavy-tailed operands
  b  one result, many routes: a C element is the same k-ascending chain in every instantiation, so its BITS agree across tiles,
     group sizes, storage layouts, a base pointer shifted by one float, odd and padded leading dimensions, and between batch
     element z of a batched call (zdiv 1 and H, with bias / res / aux strides) and the same matrices alone
  c  epilogues at (68, 132, 36) and (65, 129, 33): bias, alpha, RELU, ABS, res, ACCUM, RELUMASK, STORE_PRE, GELU, MUL_DGELU
  d  split-K: atomics inside gamma(K + ksplit + 1) * (S + |C_old|); deterministic runs bit-equal to the one-split route
  e  containment and isolation: every output inside a sentinel buffer with ldc > N, every input inside NaN slack; a NaN row of A
     / column of B / batch element reaches its own row / column / element of C only
  f  refusals: status -1 and C untouched

Measured on one MI355X, worst err / bound per section (every comparison must stay below 1):
  a  0.24 (3 x 5 x 2, heavy-tailed A); 0.05 - 0.22 at the tiled shapes       b  bit-equal on every route, no exception
  c  0.10 against the bounds; GELU 0.86 of its 2^-22 bar, MUL_DGELU 0.23 of its 2^-20 bar
  d  0.011 (K = 129, 2 splits), 0.004 (K = 320, 3), 0.001 (K = 513, 5 and K = 900 x 150, 7); deterministic runs bit-equal
  e, f  hold as written.  The pass found no defect in csrc/gemm.hip.
This module alone runs in 3.3 s (80 tests, the slowest 0.2 s).  The whole -m gpu suite with this module and
tests/test_attention_f32_gpu.py: 774 s (2 394 tests); the two modules are 7.2 s of it (172 tests), i.e. 767 s without them.

Mutation check (scratch builds, not committed; both change arithmetic on in-bounds data only).  With the k-range mask of the
FAST == 2 loader removed (`keep = true`), 21 tests fail at (4, 4, 4), (68, 132, 36), (68, 132, 33), (200, 132, 72) and at K = 129,
513, 900 of section d ("gemm32 68x132x36 unit tile64x64 NT: err / bound 1140462.546").  With `gin % gsz` / `gin / gsz` of the
grouped tile order turned into `% g_gm` / `/ g_gm`, 40 tests fail, at every shape of more than one tile ("the destination was not
fully written")."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gemm32_ref as R
from kernel_guard import _ALIVE, NAN, PAD, Guard, Tally, bits, nan_in, rnd, same_bits, stream

pytestmark = pytest.mark.gpu

CASE_IDS = [f"{m}x{n}x{k}" for m, n, k in R.CASES]
EDGE_IDS = [f"{m}x{n}x{k}" for m, n, k in R.EDGE_CASES]
TILE_IDS = [f"tile{r}x{c or 128}" for r, c in R.TILES]
EPI_CASES = [(68, 132, 36), (65, 129, 33)]
LAY = list(zip(R.LAYOUT_IDS, R.LAYOUTS))


@pytest.fixture
def tuning():
    """set(tile, group) writes ops.GEMM32_TUNING (dupl_gemm_desc.tile_rows / tile_cols / group of every later call); restored."""
    from dupl_amd import ops
    saved = dict(ops.GEMM32_TUNING)

    def set_(tile=(0, 0), group=0):
        ops.GEMM32_TUNING.update(tile_rows=tile[0], tile_cols=tile[1], group=group)
    yield set_
    ops.GEMM32_TUNING.update(saved)
    _ALIVE.clear()


@pytest.fixture
def deterministic():
    from dupl_amd import ops
    saved = ops.deterministic()
    yield ops.set_deterministic
    ops.set_deterministic(saved)


# ------------------------------------------------------------------------------------------ helpers
def _store(X, transposed, dev, ld_pad=0, shift=0):
    """[Z][rows][cols] (transposed first when asked) on the device with `ld_pad` NaN columns behind every row, inside NaN slack;
    shift = 1 puts the base pointer one float off its 16-byte alignment.  Returns (view, leading dimension)."""
    S = (X.transpose(1, 2) if transposed else X).contiguous()
    if ld_pad:
        P = torch.full(S.shape[:2] + (S.shape[2] + ld_pad,), NAN)
        P[:, :, :S.shape[2]] = S
        S = P
    return nan_in(S, dev, front=PAD + shift), S.shape[2]


class Out:
    """A [Z][M][N] destination with row stride N + pad inside a Guard: slack and pad columns hold the sentinel (a NaN)."""

    def __init__(self, Z, M, N, dev, pad, init=None):
        self.N, self.ld = N, N + pad
        self.g = Guard((Z, M, self.ld), dev)
        if init is not None:
            self.g.view[:, :, :N].copy_(init)

    def get(self, allow_nan=False):
        full = self.g.cpu()                                   # synchronizes; asserts the slack around the buffer is intact
        assert bool((bits(full[:, :, self.N:]) == self.g.pat).all()), "columns N .. ld-1 of a destination were written"
        out = full[:, :, :self.N].contiguous()
        assert allow_nan or not torch.isnan(out).any(), "the destination was not fully written"
        return out


def gemm(dev, A, B, amc, bnc, *, flags=0, alpha=1.0, bias=None, res=None, aux=None, store_aux=False, c_old=None, zdiv=1,
         lda_pad=0, ldb_pad=0, shift=0, allow_nan=False):
    """dupl_gemm_f32 through ops.gemm_raw on the logical A [M][K] / B [K][N] (or [Z][..][..]: a batched call, z -> (z // zdiv,
    z % zdiv)), stored as the layout asks.  C, res and aux rows are wider than N (3, 5, 2 floats).  Returns (C, aux written)."""
    from dupl_amd import ops, _lib
    single = A.dim() == 2
    if single:
        A, B = A[None], B[None]
        bias, res, aux, c_old = (None if t is None else t[None] for t in (bias, res, aux, c_old))
    Z, M, K = A.shape
    N = B.shape[2]
    a, lda = _store(A, amc, dev, lda_pad, shift)
    b, ldb = _store(B, not bnc, dev, ldb_pad, shift)
    C = Out(Z, M, N, dev, 3, init=c_old)
    kw = {}

    def strides(per):                                         # a single matrix passes no strides (they enter the loader choice)
        return (0, 0) if single else (zdiv * per, per)
    if bias is not None:
        kw.update(bias=nan_in(bias, dev).data_ptr(), sBias=strides(N))
    if res is not None:
        r, ldr = _store(res, False, dev, 5)
        kw.update(res=r.data_ptr(), ldr=ldr, sR=strides(M * ldr))
    X = None
    if store_aux:
        X = Out(Z, M, N, dev, 2)
        kw.update(aux=X.g.ptr, ldaux=X.ld, sX=strides(M * X.ld))
    elif aux is not None:
        x, ldx = _store(aux, False, dev, 2)
        kw.update(aux=x.data_ptr(), ldaux=ldx, sX=strides(M * ldx))
    fl = flags | (_lib.GEMM_A_MCONTIG if amc else 0) | (_lib.GEMM_B_NCONTIG if bnc else 0)
    ops.gemm_raw(a.data_ptr(), b.data_ptr(), C.g.ptr, M, N, K, lda, ldb, C.ld, flags=fl, alpha=alpha, batch=Z, zdiv=zdiv,
                 sA=strides(a.shape[1] * lda), sB=strides(b.shape[1] * ldb), sC=strides(M * C.ld), **kw)
    c, x = C.get(allow_nan), (X.get(allow_nan) if X is not None else None)
    return (c[0], None if x is None else x[0]) if single else (c, x)


@functools.lru_cache(maxsize=None)
def _data(M, N, K, heavy=False):
    """(A, B, float64 reference, bound) of a case: computed once, shared, never written."""
    A, B = rnd(M, K, seed=1), rnd(K, N, seed=2)
    if heavy:
        A = A ** 3
    _, ref, bound = R.ref_and_bound(A.numpy(), B.numpy())
    return A, B, torch.from_numpy(ref), torch.from_numpy(bound)


def _err(c, ref):
    return (c.double() - torch.as_tensor(ref)).abs()


# ------------------------------------------------------------------------------------------ a. accuracy
@pytest.mark.parametrize("heavy", [False, True], ids=["unit", "heavy-tailed"])
@pytest.mark.parametrize("M,N,K", R.CASES, ids=CASE_IDS)
def test_every_element_within_the_bound(dev, tuning, M, N, K, heavy):
    A, B, ref, bound = _data(M, N, K, heavy)
    t = Tally(f"gemm32 {M}x{N}x{K} {'heavy' if heavy else 'unit'}")
    for tile, tid in zip(R.TILES, TILE_IDS):
        tuning(tile)
        for lid, (amc, bnc) in LAY:
            c, _ = gemm(dev, A, B, amc, bnc)
            t.add(f"{tid} {lid}", _err(c, ref), bound)
    t.done()


# ------------------------------------------------------------------------------------------ b. one result, many routes
@pytest.mark.parametrize("M,N,K", R.CASES, ids=CASE_IDS)
def test_one_result_on_every_route(dev, tuning, M, N, K):
    A, B, ref, bound = _data(M, N, K)
    tuning((64, 64))
    base, _ = gemm(dev, A, B, False, False)
    assert bool((_err(base, ref) <= bound).all())
    for tile, tid in zip(R.TILES, TILE_IDS):
        for lid, (amc, bnc) in LAY:
            tuning(tile)
            assert same_bits(gemm(dev, A, B, amc, bnc)[0], base), f"{tid} {lid}"
            for group in (1, 3, 16, 4096):
                tuning(tile, group)
                assert same_bits(gemm(dev, A, B, amc, bnc)[0], base), f"{tid} {lid} group {group}"
    tuning((64, 128))
    for lid, (amc, bnc) in LAY:
        assert same_bits(gemm(dev, A, B, amc, bnc, shift=1)[0], base), f"{lid}: base pointers one float off alignment"
        assert same_bits(gemm(dev, A, B, amc, bnc, lda_pad=1, ldb_pad=1)[0], base), f"{lid}: odd leading dimensions"
        assert same_bits(gemm(dev, A, B, amc, bnc, lda_pad=4, ldb_pad=4)[0], base), f"{lid}: leading dimensions + 4 (NaN behind the rows)"
        assert same_bits(gemm(dev, A, B, amc, bnc, lda_pad=4, ldb_pad=1)[0], base), f"{lid}: one operand guarded"


@pytest.mark.parametrize("zdiv", [1, 3], ids=["zdiv1", "zdivH"])
@pytest.mark.parametrize("M,N,K", EPI_CASES, ids=EDGE_IDS[:2])
def test_a_batch_element_equals_the_same_matrices_alone(dev, tuning, M, N, K, zdiv):
    """batch = 6 as z or as (z // 3, z % 3), every operand and bias / res / aux with batch strides of its own; flags RELU and
    STORE_PRE so that both C and aux are outputs.  (65, 129, 33): every stride is odd, the guarded loader."""
    from dupl_amd import _lib
    Z = 6
    A, B, bias, res = rnd(Z, M, K, seed=11), rnd(Z, K, N, seed=12), rnd(Z, N, seed=13), rnd(Z, M, N, seed=14)
    fl = _lib.GEMM_RELU | _lib.GEMM_STORE_PRE
    for lid, (amc, bnc) in LAY:
        c, x = gemm(dev, A, B, amc, bnc, flags=fl, alpha=0.75, bias=bias, res=res, store_aux=True, zdiv=zdiv)
        for z in range(Z):
            c1, x1 = gemm(dev, A[z], B[z], amc, bnc, flags=fl, alpha=0.75, bias=bias[z], res=res[z], store_aux=True)
            assert same_bits(c[z], c1) and same_bits(x[z], x1), f"{lid} z {z}"
        _, ref, bound = R.ref_and_bound(A[0].numpy(), B[0].numpy(), 0.75, bias[0].numpy())
        assert bool((_err(x[0], ref) <= torch.from_numpy(bound)).all())


# ------------------------------------------------------------------------------------------ c. epilogues
@pytest.mark.parametrize("tile", R.TILES, ids=TILE_IDS)
@pytest.mark.parametrize("M,N,K", EPI_CASES, ids=EDGE_IDS[:2])
def test_epilogues(dev, tuning, deterministic, M, N, K, tile):
    from dupl_amd import _lib
    A, B = rnd(M, K, seed=1), rnd(K, N, seed=2)
    bias, res, c_old, mask, gpre = rnd(N, seed=3), rnd(M, N, seed=4), rnd(M, N, seed=5), rnd(M, N, seed=6), rnd(M, N, seed=7, scale=1.5)
    An, Bn = A.numpy(), B.numpy()
    alpha = -0.5
    pre, _, b_pre = R.ref_and_bound(An, Bn, alpha, bias.numpy())
    _, ref_res, b_res = R.ref_and_bound(An, Bn, alpha, bias.numpy(), res=res.numpy())
    _, ref_acc, b_acc = R.ref_and_bound(An, Bn, alpha, bias.numpy(), c_old=c_old.numpy())
    pre = torch.from_numpy(pre)
    clamp, coef = R.gelu_coefficients()
    tuning(tile)
    t = Tally(f"gemm32 epilogues {M}x{N}x{K} {tile}")
    worst_gelu = worst_dgelu = 0.0
    for lid, lay in LAY:
        run = functools.partial(gemm, dev, A, B, *lay, alpha=alpha, bias=bias)
        plain, _ = run()
        t.add(f"{lid} alpha bias", _err(plain, pre), b_pre)
        t.add(f"{lid} RELU", _err(run(flags=_lib.GEMM_RELU)[0], pre.clamp_min(0)), b_pre)
        t.add(f"{lid} ABS", _err(run(flags=_lib.GEMM_ABS)[0], pre.abs()), b_pre)
        t.add(f"{lid} res", _err(run(res=res)[0], ref_res), b_res)
        t.add(f"{lid} RELU res", _err(run(flags=_lib.GEMM_RELU, res=res)[0], pre.clamp_min(0) + res.double()), b_res)
        acc, _ = run(flags=_lib.GEMM_ACCUM, c_old=c_old)
        t.add(f"{lid} ACCUM", _err(acc, ref_acc), b_acc)
        assert same_bits(acc, c_old + plain), f"{lid}: ACCUM is fl32(C_old + C_plain)"
        t.add(f"{lid} RELUMASK", _err(run(flags=_lib.GEMM_MUL_RELUMASK, aux=mask)[0], torch.where(mask > 0, pre, torch.zeros_like(pre))), b_pre)
        c, x = run(flags=_lib.GEMM_RELU | _lib.GEMM_STORE_PRE, store_aux=True)
        assert same_bits(x, plain), f"{lid}: STORE_PRE writes the C of the same call without an activation"
        assert torch.equal(c, plain.clamp_min(0)), f"{lid}: RELU of the stored pre-activation"
        # GELU: y = x * Phi(x) of the kernel's own stored pre-activation, as the header's formula gives it in fp32
        y, x = run(flags=_lib.GEMM_GELU | _lib.GEMM_STORE_PRE, store_aux=True)
        assert same_bits(x, plain), f"{lid}: STORE_PRE under GELU"
        p_ = x.numpy()
        want = (p_ * R.gelu_phi32(p_, clamp, coef)).astype(np.float32)
        err, tol = np.abs(y.numpy().astype(np.float64) - want), 2.0 ** -22 * np.maximum(np.abs(want), 2.0 ** -20)
        worst_gelu = max(worst_gelu, float((err / tol).max()))
        assert (err <= tol).all(), (lid, "GELU", float((err / tol).max()))
        # MUL_DGELU: lin * gelu'(aux), lin = the flagless call; the bar is absolute in gelu' (test_gelu_epilogues_follow_the_header_formula)
        dx, _ = run(flags=_lib.GEMM_MUL_DGELU, aux=gpre)
        lin = plain.numpy()
        want = (lin * R.gelu_grad32(gpre.numpy(), clamp, coef)).astype(np.float32)
        err, tol = np.abs(dx.numpy().astype(np.float64) - want), 2.0 ** -20 * np.abs(lin) + 1e-30
        worst_dgelu = max(worst_dgelu, float((err / tol).max()))
        assert (err <= tol).all(), (lid, "MUL_DGELU", float((err / tol).max()))
        # a pure accumulate (the split-K predicate holds) with the switch on: one block owns the whole reduction
        deterministic(True)
        plain1, _ = gemm(dev, A, B, *lay)
        acc1, _ = gemm(dev, A, B, *lay, flags=_lib.GEMM_ACCUM, c_old=c_old)
        deterministic(False)
        assert same_bits(acc1, c_old + plain1), f"{lid}: deterministic ACCUM is fl32(C_old + C_plain)"
    t.done()
    print(f"gemm32 epilogues {M}x{N}x{K} {tile}: worst err / bar GELU {worst_gelu:.3f}, MUL_DGELU {worst_dgelu:.3f}")


# ------------------------------------------------------------------------------------------ d. split-K
@pytest.mark.parametrize("M,N,K,Z", R.SPLITK_CASES, ids=[f"{m}x{n}x{k}-batch{z}" for m, n, k, z in R.SPLITK_CASES])
def test_split_k(dev, tuning, deterministic, M, N, K, Z):
    """Pure accumulate on k-major operands (the weight-gradient call) into a non-zero C.  K = 513: the last split is the single
    k = 512; batch 150 x K = 900: the seventh split is empty and returns early."""
    from dupl_amd import _lib
    A, B, c_old = rnd(Z, M, K, seed=21), rnd(Z, K, N, seed=22), rnd(Z, M, N, seed=23)
    _, ksplit, _ = R.dispatch(M, N, K, True, True, batch=Z, pure_accum=True)
    assert ksplit > 1
    _, ref, bound = R.ref_and_bound(A.numpy(), B.numpy(), c_old=c_old.numpy(), ksplit=ksplit)
    t = Tally(f"gemm32 split-K {M}x{N}x{K} batch {Z} ({ksplit} splits)")
    deterministic(False)
    for tile, tid in zip([(0, 0)] + R.TILES, ["heuristic"] + TILE_IDS):
        tuning(tile)
        c, _ = gemm(dev, A, B, True, True, flags=_lib.GEMM_ACCUM, c_old=c_old)
        t.add(tid, _err(c, ref), bound)
    t.done()
    tuning()
    plain, _ = gemm(dev, A, B, False, False)                 # the one-split route of section b
    deterministic(True)
    d1, _ = gemm(dev, A, B, True, True, flags=_lib.GEMM_ACCUM, c_old=c_old)
    d2, _ = gemm(dev, A, B, True, True, flags=_lib.GEMM_ACCUM, c_old=c_old)
    assert same_bits(d1, d2), "two deterministic runs differ"
    assert same_bits(d1, c_old + plain), "the deterministic run is not fl32(C_old + the one-split result)"
    if Z == 1:                                               # and through the wrapper the engine uses (dW += dy^T x)
        from dupl_amd import ops
        dy, x = A[0].t().contiguous().to(dev), B[0].contiguous().to(dev)
        dW = c_old[0].to(dev)
        ops.linear_wgrad(dy, x, dW, accumulate=True)
        assert same_bits(dW.cpu(), d1[0])


# ------------------------------------------------------------------------------------------ e. containment and isolation
@pytest.mark.parametrize("tile", R.TILES, ids=TILE_IDS)
@pytest.mark.parametrize("M,N,K", R.EDGE_CASES, ids=EDGE_IDS)
def test_a_nan_reaches_its_own_row_and_column_only(dev, tuning, M, N, K, tile):
    """Every call of this module keeps C / aux in sentinel buffers with ldc > N and its inputs in NaN slack (gemm() above); here
    one row of A (the last -- the row the branch-free loaders clamp to -- and row 31), then one column of B, is NaN."""
    A, B, _, _ = _data(M, N, K)
    tuning(tile)
    for lid, lay in LAY:
        clean, _ = gemm(dev, A, B, *lay)
        for r in (M - 1, 31):
            A2 = A.clone()
            A2[r] = NAN
            c, _ = gemm(dev, A2, B, *lay, allow_nan=True)
            keep = torch.arange(M) != r
            assert torch.isnan(c[r]).all() and same_bits(c[keep], clean[keep]), f"{lid}: NaN in row {r} of A"
        for col in (N - 1, 64):
            B2 = B.clone()
            B2[:, col] = NAN
            c, _ = gemm(dev, A, B2, *lay, allow_nan=True)
            keep = torch.arange(N) != col
            assert torch.isnan(c[:, col]).all() and same_bits(c[:, keep], clean[:, keep]), f"{lid}: NaN in column {col} of B"


@pytest.mark.parametrize("M,N,K", R.EDGE_CASES, ids=EDGE_IDS)
def test_a_nan_batch_element_reaches_its_own_result_only(dev, tuning, M, N, K):
    from dupl_amd import _lib
    Z = 3
    A, B, bias, res, mask = rnd(Z, M, K, seed=31), rnd(Z, K, N, seed=32), rnd(Z, N, seed=33), rnd(Z, M, N, seed=34), rnd(Z, M, N, seed=35)
    for lid, lay in LAY:
        clean, _ = gemm(dev, A, B, *lay, flags=_lib.GEMM_MUL_RELUMASK, bias=bias, res=res, aux=mask)
        A2, B2, bias2, res2, mask2 = (t.clone() for t in (A, B, bias, res, mask))
        for t_ in (A2, B2, bias2, res2, mask2):
            t_[1] = NAN
        c, _ = gemm(dev, A2, B2, *lay, flags=_lib.GEMM_MUL_RELUMASK, bias=bias2, res=res2, aux=mask2, allow_nan=True)
        assert torch.isnan(c[1]).all() and same_bits(c[0], clean[0]) and same_bits(c[2], clean[2]), lid


# ------------------------------------------------------------------------------------------ f. refusals
def _set(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


_AUX_FLAGS = {"MUL_DGELU": 16, "MUL_RELUMASK": 64, "STORE_PRE": 256}
REFUSALS = {"struct_size": _set(struct_size=8), "struct_size+8": lambda d: setattr(d, "struct_size", d.struct_size + 8),
            "A-null": _set(A=None), "B-null": _set(B=None), "C-null": _set(C=None),
            **{f"{f}-{v}": _set(**{f: v}) for f in ("M", "N", "K", "batch", "zdiv") for v in (0, -1)},
            "tile_rows-32": _set(tile_rows=32), "tile_cols-32": _set(tile_cols=32), "group--1": _set(group=-1),
            "group-4097": _set(group=4097),
            **{f"{n}-without-aux": _set(flags=v) for n, v in _AUX_FLAGS.items()}}


def _base_desc(dev):
    from dupl_amd import _lib
    M, N, K = 4, 4, 4
    A, B = rnd(M, K, seed=41), rnd(N, K, seed=42)
    a, b = nan_in(A, dev), nan_in(B, dev)
    C = Guard((M, N), dev)
    d = _lib.GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), C.ptr
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, K, K, N
    d.batch, d.zdiv, d.alpha = 1, 1, 1.0
    return d, C, A, B


@pytest.mark.parametrize("case", ["null-descriptor"] + list(REFUSALS))
def test_bad_descriptors_are_refused_before_the_launch(dev, tuning, case):
    from dupl_amd import ops, _lib
    assert (_lib.GEMM_MUL_DGELU, _lib.GEMM_MUL_RELUMASK, _lib.GEMM_STORE_PRE) == tuple(_AUX_FLAGS.values())
    d, C, _, _ = _base_desc(dev)
    if case != "null-descriptor":
        REFUSALS[case](d)
    with pytest.raises(RuntimeError, match="status -1"):
        ops.L().dupl_gemm_f32(None if case == "null-descriptor" else ctypes.byref(d), stream())
    torch.cuda.synchronize()
    assert C.untouched(), f"{case}: C was written"


def test_the_unmodified_base_descriptor_is_accepted(dev, tuning):
    from dupl_amd import ops
    d, C, A, B = _base_desc(dev)
    assert ops.L().dupl_gemm_f32(ctypes.byref(d), stream()) == 0
    c = C.cpu()
    _, ref, bound = R.ref_and_bound(A.numpy(), B.t().numpy())
    assert not torch.isnan(c).any() and bool((_err(c, ref) <= torch.from_numpy(bound)).all())
