"""tests/split_ref.py against exact arithmetic (CPU only): the reference that tests/test_split_kernels_gpu.py compares the
operand-split kernels with, bit for bit, is itself checked here in float64, which holds every quantity involved exactly --
a float32 input (24 significant bits), its product with a power of two, an fp16 plane (11 bits), their difference and the
difference times 2048 all fit 53 bits with room to spare.  "Nearest, ties to even" is decided by comparing distances to the
neighbours in the table of all finite fp16 values, not by a second float16 cast."""
import math

import numpy as np
import pytest

import split_ref as S

_TABLE = np.unique(np.arange(0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64))
_TABLE = np.concatenate([-_TABLE[:0:-1], _TABLE])            # every finite fp16 value once, ascending (one zero)
X = S.special_values()
FIN = np.isfinite(X)


def assert_nearest_even(v, h, what):
    """h (fp16) is the fp16 nearest to v (float64, |v| <= 65504), the one with the even significand on a tie, and carries v's sign
    when it is a zero of a non-zero v"""
    v, h64 = np.asarray(v, dtype=np.float64), np.asarray(h).astype(np.float64)
    assert np.isfinite(h64).all(), what
    i = np.clip(np.searchsorted(_TABLE, v), 1, len(_TABLE) - 1)
    below, above = _TABLE[i - 1], _TABLE[i]                  # below <= v <= above (or v on a table value)
    d, db, da = np.abs(v - h64), np.abs(v - below), np.abs(v - above)
    assert (d <= np.minimum(db, da)).all(), f"{what}: not the nearest fp16"
    tie = (db == da) & (below != above)
    assert ((np.asarray(h).view(np.uint16)[tie] & 1) == 0).all(), f"{what}: a tie did not go to the even significand"
    nz = v != 0
    assert (np.signbit(h64[nz]) == np.signbit(v[nz])).all(), f"{what}: sign lost"


def test_the_vector_holds_what_it_promises():
    assert X.dtype == np.float32 and X.size > 3 * 65536 + 2 * 0x7BFF
    for v in (65504.0, 65520.0, 1e30, float(S.FLT_MAX), float(S.BELOW_65520), 2.0 ** -149, 2.0 ** -25):
        assert (X == np.float32(v)).any() and (X == -np.float32(v)).any()
    assert float(S.BELOW_65520) < 65520.0 and float(np.nextafter(S.BELOW_65520, np.float32(np.inf))) == 65520.0
    assert np.isnan(X).any() and np.isposinf(X).any() and np.isneginf(X).any()
    assert (np.signbit(X) & (X == 0)).any() and (~np.signbit(X) & (X == 0)).any()
    t = S.f16_ties().astype(np.float64)                      # every tie is exactly half way between two neighbours of the table
    i = np.searchsorted(_TABLE, t[np.abs(t) < 65520])
    assert (_TABLE[i] - t[np.abs(t) < 65520] == t[np.abs(t) < 65520] - _TABLE[i - 1]).all()


def test_format0_is_the_definition():
    """hi = nearest-even fp16 of the clamped value, lo = nearest-even fp16 of the exact (x - hi) * 2048, and the pair
    reconstructs x to  max(2^-22 |x|, 2^-36):

    x = hi + e1 exactly, with |e1| <= half an fp16 ulp at x, i.e. <= 2^-11 |x| (x normal in fp16) or <= 2^-25 (x in fp16's
    subnormal range, spacing 2^-24).  r = 2048 e1 is exact in float32.  lo = fp16(r) errs by <= 2^-11 |r| where r is a normal
    fp16 and by <= 2^-25 where it is subnormal, so |x - (hi + lo / 2048)| = |r - lo| / 2048 <= max(2^-11 |e1|, 2^-36)
    <= max(2^-22 |x|, 2^-36).  (|r| <= 2048 * 16 = 32768: lo never overflows.)"""
    hi, lo = S.split0(X)
    x, h, l = X[FIN].astype(np.float64), hi[FIN], lo[FIN]
    c = np.clip(x, -65504.0, 65504.0)
    assert_nearest_even(c, h, "format 0 hi")
    assert_nearest_even((c - h.astype(np.float64)) * 2048.0, l, "format 0 lo")
    inr = np.abs(x) <= 65504.0
    err = np.abs(x - (h.astype(np.float64) + l.astype(np.float64) / 2048.0))[inr]
    assert (err <= np.maximum(2.0 ** -22 * np.abs(x[inr]), 2.0 ** -36)).all()
    big = np.abs(x) > 65504.0                                # finite values saturate: (+-65504, 0)
    assert (np.abs(h[big].astype(np.float64)) == 65504.0).all() and (l[big] == 0).all()


@pytest.mark.parametrize("exp", [0, 3, 9, 15])
def test_format1_is_the_definition(exp):
    """X = x * 2^exp (exact, or Inf where the float32 product overflows: then the planes are those of Inf), hi = nearest-even
    fp16 of the clamped X, lo = nearest-even fp16 of the exact X - hi, and hi + lo reconstructs X to  max(2^-22 |X|, 2^-25):

    X = hi + e1 exactly, with |e1| <= 2^-11 |X| (X normal in fp16) or <= 2^-25 (X in fp16's subnormal range).  lo = fp16(e1) errs by <= 2^-11 |e1| <= 2^-22 |X| where e1 is a normal fp16 (|e1| >= 2^-14) and by <= 2^-25 (half
    the subnormal spacing) below that -- the format's floor is absolute, 2^-25 on X's scale, which is why the planes travel
    pre-scaled.  The derivation gives the issue's constants."""
    hi, lo = S.split1(X, exp)
    Xs = X[FIN].astype(np.float64) * 2.0 ** exp
    over = np.abs(Xs) > float(S.FLT_MAX)                     # x * 2^exp has x's significand: representable, or past FLT_MAX
    h, l = hi[FIN], lo[FIN]
    assert np.isinf(h[over]).all() and (np.signbit(h[over]) == np.signbit(Xs[over])).all() and np.isnan(l[over]).all()
    Xs, h, l = Xs[~over], h[~over], l[~over]
    c = np.clip(Xs, -65504.0, 65504.0)
    assert_nearest_even(c, h, "format 1 hi")
    assert_nearest_even(c - h.astype(np.float64), l, "format 1 lo")
    inr = np.abs(Xs) <= 65504.0
    err = np.abs(Xs - (h.astype(np.float64) + l.astype(np.float64)))[inr]
    assert (err <= np.maximum(2.0 ** -22 * np.abs(Xs[inr]), 2.0 ** -25)).all()
    big = np.abs(Xs) > 65504.0
    assert (np.abs(h[big].astype(np.float64)) == 65504.0).all() and (l[big] == 0).all()


def test_finite_gives_finite_and_nonfinite_propagates():
    """every finite input gives finite planes in format 0, and in format 1 wherever x * 2^exp is a finite float32;
    Inf gives (Inf, NaN), NaN gives (NaN, NaN)"""
    hi, lo = S.split0(X)
    assert np.isfinite(hi[FIN]).all() and np.isfinite(lo[FIN]).all()
    for exp in (0, 3, 9, 15):
        h1, l1 = S.split1(X, exp)
        with np.errstate(over="ignore", invalid="ignore"):
            ok = np.isfinite(X * np.float32(2.0 ** exp))
        assert np.isfinite(h1[ok]).all() and np.isfinite(l1[ok]).all()
        for h, l in ((hi, lo), (h1, l1)):
            for inf in (np.isposinf(X), np.isneginf(X)):
                assert np.isinf(h[inf]).all() and (np.signbit(h[inf]) == np.signbit(X[inf])).all() and np.isnan(l[inf]).all()
            assert np.isnan(h[np.isnan(X)]).all() and np.isnan(l[np.isnan(X)]).all()
    assert X[FIN].size and float(np.abs(X[FIN]).max()) == float(S.FLT_MAX)


def _amax_sweep():
    """amax words over all float32 exponents (0 = subnormals .. 254), each with the smallest, two middle and the largest
    significand, and every single-bit subnormal"""
    w = [(e << 23) | m for e in range(255) for m in (0, 1, 0x400000, 0x7FFFFF) if (e, m) != (0, 0)]
    return w + [1 << j for j in range(23)]


@pytest.mark.parametrize("target", [1, 4, 15])
def test_scale_rule(target):
    """s and inv are finite, normal, non-zero powers of two with s * inv == 1 for every amax; wherever the unclamped rule is
    representable (|target - e| <= 126) it is that rule: amax * s in [2^(target-1), 2^target)"""
    seen_clamped = False
    for w in _amax_sweep():
        s, inv = S.scale_rule(w, target)
        assert s.dtype == np.float32 and inv.dtype == np.float32
        for v in (s, inv):
            b = int(np.array([v], dtype=np.float32).view(np.uint32)[0])
            assert (b & 0x7FFFFF) == 0 and 1 <= (b >> 23) <= 254, f"amax word {w:#x}: {v!r} is not a normal positive power of two"
        assert np.float32(s * inv) == np.float32(1.0) and float(s) * float(inv) == 1.0
        a = float(np.array([w], dtype=np.uint32).view(np.float32)[0])
        e = math.frexp(a)[1]
        if abs(target - e) <= 126:
            assert 2.0 ** (target - 1) <= a * float(s) < 2.0 ** target, f"amax {a!r}"
        else:
            seen_clamped = True
            assert float(s) == (2.0 ** 126 if target - e > 0 else 2.0 ** -126)
            if target - e > 0:
                assert a * float(s) < 2.0 ** target                      # a tiny tensor stays below the target: never Inf
            else:                                                        # target 1 and amax >= 2^127 only: one binade above
                assert target - e == -127 and a * float(s) < 2.0 ** (target + 1)
    assert seen_clamped
    for w in (0, 0x7F800000, 0x7FC00000, 0xFFC00000, 0x7F800001):
        assert S.scale_rule(w, target) == (np.float32(1.0), np.float32(1.0))


def test_scale_rule_examples():
    """the issue's example: amax = 1e-36 has e = -119, 15 - e = 134 > 127: ldexp(1, 134) is Inf in float32"""
    w = S.amax_bits(np.array([1e-36, -1e-37], dtype=np.float32))
    assert math.frexp(float(np.float32(1e-36)))[1] == -119
    assert math.ldexp(1.0, 134) > float(S.FLT_MAX)
    assert S.scale_rule(w, 15) == (np.float32(2.0 ** 126), np.float32(2.0 ** -126))
    assert S.scale_rule(S.amax_bits(np.array([3e-6], dtype=np.float32)), 15) == (np.float32(2.0 ** 33), np.float32(2.0 ** -33))
    assert S.scale_rule(1, 4) == (np.float32(2.0 ** 126), np.float32(2.0 ** -126))


def test_split_prepare_ref_layout():
    g = np.random.default_rng(3)
    R, C, ld, Rp, Rz = 5, 12, 16, 16, 9
    x = g.standard_normal(R * ld).astype(np.float32) * np.float32(3e-6)
    (hi, lo), (hiT, loT), (s, inv), cs = S.split_prepare_ref(x, R, C, ld, True, 15, True, Rp, Rz)
    v = x.reshape(R, ld)[:, :C]
    assert hi.shape == (Rz, C) and hiT.shape == (C, Rp) and cs.shape == (C,)
    assert not hi[R:].any() and not lo[R:].any() and not hiT[:, R:].any() and not loT[:, R:].any()
    assert (hiT[:, :R] == hi[:R].T).all() and (loT[:, :R] == lo[:R].T).all()
    assert 2.0 ** 14 <= float(np.abs(v).max()) * float(s) < 2.0 ** 15 and float(s) * float(inv) == 1.0
    back = (hi[:R].astype(np.float64) + lo[:R].astype(np.float64)) * float(inv)
    assert (np.abs(back - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25 * float(inv))).all()
    assert np.allclose(cs, v.astype(np.float64).sum(0), rtol=0, atol=0)
    # unscaled, format 0
    (hi0, lo0), _, sc, _ = S.split_prepare_ref(x, R, C, ld, False, 15, False, 8, 0)
    h, l = S.split0(v)
    assert sc == (np.float32(1.0), np.float32(1.0)) and S.same_f16(hi0, h) and S.same_f16(lo0, l)


def test_param_bounds_ref():
    t = np.array([[3.0, -4.0], [1.0, 1.0]], dtype=np.float32)
    assert S.param_bounds_ref(t) == (4.0, 5.0)
    t[1, 0] = np.nan
    assert S.param_bounds_ref(t) == (math.inf, math.inf)
    t[1, 0] = np.inf
    assert S.param_bounds_ref(t) == (math.inf, math.inf)
    assert S.param_bounds_ref(np.zeros((3, 4), dtype=np.float32)) == (0.0, 0.0)
