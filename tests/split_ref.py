"""The f16x3 operand-plane formats in numpy, written from their definition (csrc/common.h) and independent of the library:

    format 0   x = hi + lo / 2048,   hi = fp16(x),  lo = fp16((x - hi) * 2048)
    format 1   X = x * 2^s,          hi = fp16(X),  lo = fp16(X - hi)

fp16() is round-to-nearest-even (numpy's float32 -> float16 cast); finite values saturate at +-65504 before the split, NaN and
Inf propagate (hi = NaN / Inf, lo = NaN).  Every intermediate is float32, as in the kernels: the residual x - hi and the
power-of-two products are exact there (X = x * 2^s overflows to Inf only where the float32 product does).  Gradient tensors
are additionally scaled by a power of two chosen from their max-abs (scale_rule, the specification of scale_from_amax in
csrc/split_prep.hip).  tests/test_split_ref_host.py checks this file against exact arithmetic; tests/test_split_kernels_gpu.py
checks the kernels against it, bit for bit."""
import math

import numpy as np

F16_MAX = np.float32(65504.0)
LO_SCALE = np.float32(2048.0)
U24 = 2.0 ** -24             # unit roundoff of float32
K_MAX = 126                  # |exponent| of the gradient scale: 2^126 and 2^-126 are both normal float32


def _clamp(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.minimum(np.maximum(x, -F16_MAX), F16_MAX), x).astype(np.float32)


def split0(x):
    """format 0 planes (hi, lo) of a float32 array"""
    c = _clamp(x)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = c.astype(np.float16)
        lo = ((c - hi.astype(np.float32)) * LO_SCALE).astype(np.float16)
    return hi, lo


def split1(x, exp):
    """format 1 planes (hi, lo) of x * 2^exp"""
    with np.errstate(invalid="ignore", over="ignore"):
        X = np.asarray(x, dtype=np.float32) * np.float32(2.0 ** exp)
        c = _clamp(X)
        hi = c.astype(np.float16)
        lo = (c - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def scale_rule(amax_bits, target):
    """(s, inv) as float32 for the amax word `amax_bits` (the float32 bit pattern of max |x|): with amax in [2^(e-1), 2^e),
    s = 2^k and inv = 2^-k for k = target - e clamped to [-126, 126], so that both are normal float32 powers of two and
    s * inv == 1 for every amax.  Wherever target - e is within the clamp, amax * s lies in [2^(target-1), 2^target).  A tiny
    tensor (amax < 2^(target-127)) is scaled by 2^126 only: its planes are then smaller than the target, never Inf.  (The
    lower clamp is met by target 1 and amax >= 2^127 alone: amax * s is then in [2, 4).)
    amax == 0 and a non-finite amax give (1, 1)."""
    a = float(np.array([int(amax_bits) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
    if not (a > 0.0 and a < math.inf):
        return np.float32(1.0), np.float32(1.0)
    e = math.frexp(a)[1]
    k = min(max(target - e, -K_MAX), K_MAX)
    return np.float32(math.ldexp(1.0, k)), np.float32(math.ldexp(1.0, -k))


def amax_bits(x):
    """the amax word of a tensor: the bits of max |x| over its non-NaN elements (0 for none)"""
    a = np.abs(np.asarray(x, dtype=np.float32)).reshape(-1)
    a = a[~np.isnan(a)]
    m = np.float32(a.max()) if a.size else np.float32(0.0)
    return int(np.array([m], dtype=np.float32).view(np.uint32)[0])


def split_prepare_ref(x, R, C, ld, scaled, target, fmt1, Rp, rows_zero_to):
    """dupl_split_prepare of x (float32, at least R * ld elements; columns C .. ld-1 are not read).
    Returns ((hi, lo) row-major [max(R, rows_zero_to), C] with zero rows from R on, (hiT, loT) [C, Rp] with zero rows
    R .. Rp-1 of the transposed image, (s, inv), float64 column sums of the UNSCALED values)."""
    v = np.asarray(x, dtype=np.float32).reshape(-1)[:R * ld].reshape(R, ld)[:, :C]
    s, inv = scale_rule(amax_bits(v), target) if scaled else (np.float32(1.0), np.float32(1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        y = v * s
    hi, lo = split1(y, 0) if fmt1 else split0(y)
    Rz = max(R, rows_zero_to)
    rm = np.zeros((2, Rz, C), dtype=np.float16)
    rm[0, :R], rm[1, :R] = hi, lo
    T = np.zeros((2, C, Rp), dtype=np.float16)
    if Rp >= R:                                              # (no transposed planes are asked for otherwise)
        T[0, :, :R], T[1, :, :R] = hi.T, lo.T
    with np.errstate(invalid="ignore"):
        colsum = v.astype(np.float64).sum(axis=0)
    return (rm[0], rm[1]), (T[0], T[1]), (s, inv), colsum


def param_bounds_ref(t):
    """(max |t|, largest row L2 norm) of a 2-d array in float64; a NaN anywhere gives (+inf, +inf)"""
    t = np.asarray(t, dtype=np.float64)
    if np.isnan(t).any():
        return math.inf, math.inf
    with np.errstate(over="ignore"):
        return float(np.abs(t).max()), float(np.sqrt((t * t).sum(axis=1)).max())


def row_norm_bound(rows, cols, off):
    """Two-sided relative bound on the row norm that csrc/range.hip computes for a [rows, cols] tensor that starts `off` floats
    from a 16-byte aligned base (u = 2^-24).  A lane sums m products -- m = ceil(cols / 256) * 4
    on the float4 path (cols % 4 == 0 and the row 16-byte aligned), ceil(cols / 64) on the scalar path -- so a term passes through
    its product's rounding and at most m additions (fewer where the compiler contracts to an FMA), then the six shuffle additions
    of wave_sum: at most m + 7 roundings.  All terms are >= 0, so the computed sum of squares is exact * (1 + t) with
    |t| <= (1 + u)^(m + 7) - 1.  The square root halves that, and sqrtf adds at most one ulp (2 u; HIP documents 1 ulp, the
    IEEE operation would be u):  |got / exact - 1| <= sqrt((1 + u)^(m + 7)) * (1 + 2 u) - 1.  The largest m over the tensor's
    rows is used: the maximum of values each within the bound of its exact value is within the bound of the exact maximum."""
    m = 0
    for r in range(rows):
        vec = cols % 4 == 0 and (off + r * cols) % 4 == 0
        m = max(m, (cols + 255) // 256 * 4 if vec else (cols + 63) // 64)
    return math.sqrt((1.0 + U24) ** (m + 7)) * (1.0 + 2.0 * U24) - 1.0


# ------------------------------------------------------------------------------------------------------- the test vectors
def f16_patterns():
    """every one of the 65536 fp16 bit patterns, widened to float32 (exact)"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)


def f16_ties():
    """the float32 midpoint of every pair of adjacent finite fp16 values (both signs), and +-65520 (the midpoint of 65504 and
    the 2^16 that fp16 does not have)"""
    p = np.arange(0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)     # 0 .. 65504, ascending
    mid = np.concatenate([(p[:-1] + p[1:]) * np.float32(0.5), np.array([65520.0], dtype=np.float32)])
    return np.concatenate([mid, -mid])


FLT_MAX = np.float32(3.4028234663852886e38)
BELOW_65520 = np.nextafter(np.float32(65520.0), np.float32(0.0))


def special_values():
    """the vector the host test and the GPU test of dupl_split_f16x2 / f16x2b share: every fp16 pattern, each one's float32
    neighbours, every tie, +-0, the fp16 subnormal range and |x| < 2^-25 (float32 subnormals included), the top of the range
    (65504, the largest float32 below 65520, 65520, 1e30, values around the old 3.0e38 guard, FLT_MAX), +-Inf and NaN"""
    p = f16_patterns()
    with np.errstate(invalid="ignore", over="ignore"):
        up, dn = np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(-np.inf))
    g = np.random.default_rng(7)
    sub = (g.uniform(-1.0, 1.0, 2048) * 2.0 ** -14).astype(np.float32)                         # fp16 subnormal range
    tiny = (g.uniform(-1.0, 1.0, 2048) * 2.0 ** g.integers(-149, -25, 2048).astype(np.float64)).astype(np.float32)
    tiny_edges = np.array([2.0 ** -25, 2.0 ** -24, 2.0 ** -126, 2.0 ** -127, 2.0 ** -149, 1.5 * 2.0 ** -25], dtype=np.float32)
    top = np.array([65504.0, BELOW_65520, 65520.0, 65536.0, 1e30, 2.9999999e38, 3.0e38, 3.0000001e38, 3.2e38, FLT_MAX], dtype=np.float32)
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    return np.concatenate([p, up, dn, f16_ties(), sub, tiny, tiny_edges, -tiny_edges, top, -top, odd]).astype(np.float32)


def same_f16(got, ref):
    """bit equality of fp16 arrays; where the reference is NaN, any NaN (payload and sign ignored)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float16 and ref.dtype == np.float16 and got.shape == ref.shape
    n = np.isnan(ref)
    return bool((np.isnan(got) == n).all()) and bool((got.view(np.uint16)[~n] == ref.view(np.uint16)[~n]).all())


def first_diff(got, ref, x=None):
    """a short description of the first element where same_f16 fails (for assertion messages)"""
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    n = np.isnan(ref)
    bad = np.where(n, ~np.isnan(got), np.isnan(got) | (got.view(np.uint16) != ref.view(np.uint16)))
    idx = np.flatnonzero(bad)
    if not idx.size:
        return "equal"
    i = int(idx[0])
    src = "" if x is None else f" x = {float(np.asarray(x).reshape(-1)[i])!r}"
    return f"{idx.size} of {got.size} differ; first at {i}:{src} got {float(got[i])!r} (0x{int(got.view(np.uint16)[i]):04x}), " \
           f"reference {float(ref[i])!r} (0x{int(ref.view(np.uint16)[i]):04x})"
