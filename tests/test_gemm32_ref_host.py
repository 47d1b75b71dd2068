"""No GPU: the case table and the error bound of tests/gemm32_ref.py are worth something.

  1  CASES x 4 layouts x the three forced tiles reaches every one of the 36 instantiations of gemm_f32_kernel, and the split-K
     cases split the way the GPU test expects (a split with a single k, an empty split)
  2  a numpy fp32 emulation of the kernel (k ascending, fused and unfused) stays inside ref_and_bound at every shape, and four
     plausible kernel mistakes leave it at the shape the table holds for them"""
import numpy as np
import pytest

import gemm32_ref as R


def _rnd(*shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_case_table_reaches_all_36_instantiations():
    reached = {}
    for (M, N, K) in R.CASES:
        for a_mc, b_nc in R.LAYOUTS:
            for tr, tc in R.TILES:
                inst, ksplit, _ = R.dispatch(M, N, K, a_mc, b_nc, tr, tc)
                assert ksplit == 1
                reached.setdefault(inst, (M, N, K))
    want = {(a, b, bm, fast, nj) for a, b in R.LAYOUTS for bm, nj in ((64, 1), (64, 2), (128, 2)) for fast in (0, 1, 2)}
    assert len(want) == 36 and set(reached) == want, sorted(want - set(reached))
    # the shapes the table holds for one loader each
    for a_mc, b_nc in R.LAYOUTS:
        assert R.dispatch(68, 132, 36, a_mc, b_nc)[0][3] == 2
        assert R.dispatch(65, 129, 33, a_mc, b_nc)[0][3] == 0
        assert R.dispatch(128, 128, 64, a_mc, b_nc)[0][3] == 1
        assert R.dispatch(68, 132, 33, a_mc, b_nc)[0][3] == (2 if a_mc and b_nc else 0)        # odd K on the branch-free loader
    # what must select the guarded loader: an unaligned base pointer, a leading dimension or a batch stride that is no multiple of 4
    assert R.dispatch(68, 132, 36, False, False, aligned=False)[0][3] == 0
    assert R.dispatch(68, 132, 36, False, False, lda=37)[0][3] == 0
    assert R.dispatch(68, 132, 36, True, True, ldb=133)[0][3] == 0
    assert R.dispatch(68, 132, 36, True, True, strides=(0, 0, 4, 2))[0][3] == 0
    assert R.dispatch(68, 132, 36, True, True, lda=72, ldb=136)[0][3] == 2


def test_split_k_cases_split_as_expected():
    got = {c: R.dispatch(c[0], c[1], c[2], True, True, batch=c[3], pure_accum=True) for c in R.SPLITK_CASES}
    assert got[(8, 8, 129, 1)][1:] == (2, [(0, 96), (96, 129)])
    assert got[(8, 8, 513, 1)][1] == 5 and got[(8, 8, 513, 1)][2][-1] == (512, 513)            # a split with a single k
    assert got[(64, 64, 320, 1)][1:] == (3, [(0, 128), (128, 256), (256, 320)])
    ks, rg = got[(8, 8, 900, 150)][1:]
    assert ks == 7 and rg[5] == (800, 900) and rg[6][0] >= 900 and rg[6][0] == rg[6][1]        # the last split is empty
    for c, (inst, ks, rg) in got.items():
        # 64 x 64 tiles; an odd K runs on the branch-free loader with the k-range mask, K = 320 without the mask
        assert inst == (True, True, 64, 1 if c[2] % R.BK == 0 else 2, 1)
        assert sum(b - a for a, b in rg) == c[2] and all(a % R.BK == 0 for a, _ in rg)
        assert R.dispatch(c[0], c[1], c[2], True, True, batch=c[3], pure_accum=True, deterministic=True)[1] == 1
    for tr, tc in R.TILES:                               # the forced tiles do not change the splits of these shapes
        assert R.dispatch(8, 8, 513, True, True, tr, tc, pure_accum=True)[1] == 5


def _inside(got, ref, bound):
    return bool((np.abs(got.astype(np.float64) - ref) <= bound).all())


@pytest.mark.parametrize("M,N,K", R.CASES, ids=[f"{m}x{n}x{k}" for m, n, k in R.CASES])
def test_emulated_kernel_stays_inside_the_bound(M, N, K):
    A, B, bias, c_old = _rnd(M, K, seed=1), _rnd(K, N, seed=2), _rnd(N, seed=3), _rnd(M, N, seed=4)
    heavy = (A.astype(np.float64) ** 3).astype(np.float32)
    worst = 0.0
    for a in (A, heavy):
        for alpha, b, c in ((1.0, None, None), (-0.5, bias, None), (1.0, bias, c_old)):
            _, ref, bound = R.ref_and_bound(a, B, alpha, b, c_old=c)
            for fused in (True, False):
                got = R.emulate(a, B, alpha, b, c_old=c, fused=fused)
                assert _inside(got, ref, bound)
                worst = max(worst, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
    print(f"{M}x{N}x{K}: worst emulated err / bound {worst:.3f}")


@pytest.mark.parametrize("M,N,K,batch", R.SPLITK_CASES, ids=[f"{m}x{n}x{k}" for m, n, k, _ in R.SPLITK_CASES])
def test_emulated_split_k_stays_inside_its_bound(M, N, K, batch):
    A, B, c_old = _rnd(M, K, seed=5), _rnd(K, N, seed=6), _rnd(M, N, seed=7)
    _, ks, rg = R.dispatch(M, N, K, True, True, batch=batch, pure_accum=True)
    _, ref, bound = R.ref_and_bound(A, B, c_old=c_old, ksplit=ks)
    for order in (rg, rg[::-1]):                         # atomics land in any order
        assert _inside(R.emulate(A, B, kranges=order, c_old=c_old), ref, bound)


@pytest.mark.parametrize("K", [33, 70])
def test_bound_catches_a_dropped_last_k(K):
    M, N = (65, 129) if K == 33 else (257, 131)
    A, B = _rnd(M, K, seed=1), _rnd(K, N, seed=2)
    _, ref, bound = R.ref_and_bound(A, B)
    assert _inside(R.emulate(A, B), ref, bound)
    assert not _inside(R.emulate(A[:, :K - 1], B[:K - 1]), ref, bound)


def test_bound_catches_a_k_tail_filled_from_the_clamped_chunk():
    """K = 36 on the branch-free loader of a k-contiguous operand: the chunks at k = 36, 40, .. 60 of the second k-tile are read
    from the clamped address k = 32; without the k-range mask the products of k = 32..35 enter seven more times."""
    M, N, K = 68, 132, 36
    A, B = _rnd(M, K, seed=1), _rnd(K, N, seed=2)
    _, ref, bound = R.ref_and_bound(A, B)
    assert _inside(R.emulate(A, B), ref, bound)
    assert not _inside(R.emulate(A, B, tail_from=(32, 36, 7)), ref, bound)


def test_bound_catches_two_swapped_rows_at_the_tile_edge():
    M, N, K = 65, 129, 33
    A, B = _rnd(M, K, seed=1), _rnd(K, N, seed=2)
    _, ref, bound = R.ref_and_bound(A, B)
    got = R.emulate(A, B)
    assert _inside(got, ref, bound)
    got[[63, 64]] = got[[64, 63]]
    assert not _inside(got, ref, bound)


def test_bound_catches_a_dropped_single_k_split():
    M, N, K = 8, 8, 513
    A, B, c_old = _rnd(M, K, seed=5), _rnd(K, N, seed=6), _rnd(M, N, seed=7)
    _, ks, rg = R.dispatch(M, N, K, True, True, pure_accum=True)
    assert rg[-1] == (512, 513)
    _, ref, bound = R.ref_and_bound(A, B, c_old=c_old, ksplit=ks)
    assert _inside(R.emulate(A, B, kranges=rg, c_old=c_old), ref, bound)
    assert not _inside(R.emulate(A, B, kranges=rg[:-1], c_old=c_old), ref, bound)


def test_gelu_restatement_matches_the_plain_formula():
    """The fp32 restatement of csrc/common.h's GELU agrees with erf-based float64 GELU / GELU' to the accuracy the header claims."""
    import math
    clamp, coef = R.gelu_coefficients()
    x = np.linspace(-8, 8, 4001).astype(np.float32)
    x64 = x.astype(np.float64)
    Phi = np.array([0.5 * (1 + math.erf(v / math.sqrt(2))) for v in x64])
    assert float(np.abs(R.gelu_phi32(x, clamp, coef) - Phi).max()) < 5e-7
    grad = Phi + x64 * np.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
    assert float(np.abs(R.gelu_grad32(x, clamp, coef) - grad).max()) < 1e-6
