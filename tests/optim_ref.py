"""fp32 emulation of csrc/optim.hip's adamw_one, operation by operation, on the host: every rounding of the kernel is ONE numpy
float32 operation here (numpy's float32 *, -, +, /, sqrt are IEEE correctly rounded), and the two fused multiply-adds round once
(fma32 below).  tests/test_par_ref_host.py proves fma32 on operands where rounding twice gives the other answer;
tests/test_adamw_gmm_kernels_gpu.py holds the four instantiations of the kernel to this bit for bit.

Out of scope: flush-versus-gradual underflow.  adamw_ref refuses inputs for which any input or intermediate is subnormal."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)          # 2^-126, the smallest normal


def fma32_twice_rounded(a, b, c):
    """The WRONG route, kept for the host test: a * b + c in float64 (product exact, sum rounded to 53 bits), then cast (rounded
    again to 24 bits)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
                + np.asarray(c, F32).astype(np.float64)).astype(F32)


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, vectorised.  The product of two float32 is exact in float64 (48 bits).  The float64 sum
    s = fl64(p + c) is rounded to 53 bits; TwoSum gives its exact error e.  Where e != 0 and the last bit of s is even, s is moved
    one float64 step towards the exact value: that is rounding to ODD (of the two float64 neighbours of the exact sum the odd one
    is kept), and a round-to-odd result with 53 >= 2 * 24 + 2 bits rounds to float32 exactly as the unrounded sum would
    (Boldo & Melquiond 2008), ties of the second rounding included."""
    a, b, c = (np.asarray(t, F32).astype(np.float64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                                   # TwoSum (Knuth): p + c == s + e exactly
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def fma32_exact(a, b, c) -> np.float32:
    """Scalar fl32(a * b + c) by exact rational arithmetic: the float32 nearest to the exact value, ties to the even mantissa.
    Finite operands whose result is a normal float32 only (the host test's yardstick for fma32)."""
    x = Fraction(float(F32(a))) * Fraction(float(F32(b))) + Fraction(float(F32(c)))
    g = F32(float(x))                                                   # a float32 within one step of x
    cands = sorted({g, np.nextafter(g, F32(np.inf)), np.nextafter(g, F32(-np.inf))}, key=float)
    best = min(abs(Fraction(float(t)) - x) for t in cands)
    near = [t for t in cands if abs(Fraction(float(t)) - x) == best]
    if len(near) == 2:
        near = [t for t in near if (t.view(np.int32) & 1) == 0]
    return near[0]


def _refuse_subnormal(name, t):
    t = np.asarray(t)
    a = np.abs(t[np.isfinite(t)])
    if a.size and bool(((a > 0) & (a < TINY)).any()):
        raise ValueError(f"adamw_ref: {name} holds a subnormal float32: flush-versus-gradual underflow is out of scope")
    return t


def host_scalars(lr, beta1, beta2, eps, wd, step):
    """What dupl_adamw's launcher derives in float32 from its float arguments (utils/optimizer.adamw_segment passes bc1 and
    sqrt(bc2) computed in double and rounded once): (decay, step_size, bc2_sqrt) with b1, b2, eps."""
    lr, b1, b2, eps, wd = F32(lr), F32(beta1), F32(beta2), F32(eps), F32(wd)
    bc1 = F32(1.0 - float(beta1) ** step)
    bc2_sqrt = F32(np.sqrt(1.0 - float(beta2) ** step))
    return dict(decay=F32(1) - lr * wd, step_size=lr / bc1, bc2_sqrt=bc2_sqrt, b1=b1, b2=b2, eps=eps)


def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, grad_scale=1.0):
    """One update of float32 arrays -> (p, g, m, v) afterwards, as adamw_kernel leaves them: g is g * grad_scale (one rounding)
    when grad_scale != 1 and untouched otherwise."""
    p, g, m, v = (_refuse_subnormal(n_, np.asarray(t, F32)) for n_, t in (("p", p), ("g", g), ("m", m), ("v", v)))
    k = host_scalars(lr, beta1, beta2, eps, wd, step)
    chk = _refuse_subnormal
    with np.errstate(all="ignore"):
        gs = F32(grad_scale)
        if gs != F32(1):
            g = chk("g * grad_scale", g * gs)
        p1 = chk("p * decay", p * k["decay"])
        m1 = chk("m", fma32(k["b1"], m, chk("(1 - b1) g", (F32(1) - k["b1"]) * g)))
        v1 = chk("v", fma32(k["b2"], v, chk("(1 - b2) g g", chk("(1 - b2) g", (F32(1) - k["b2"]) * g) * g)))
        denom = chk("denom", chk("sqrt(v) / bc2_sqrt", chk("sqrt(v)", np.sqrt(v1)) / k["bc2_sqrt"]) + k["eps"])
        p2 = chk("p", p1 - chk("step_size * (m / denom)", k["step_size"] * chk("m / denom", m1 / denom)))
    return p2.astype(F32), g.astype(F32), m1.astype(F32), v1.astype(F32)


def same_bits_or_both_nan(a, b) -> bool:
    """bit equality of float32 arrays, except that any NaN matches any NaN (the payload and sign of a generated NaN are the
    processor's choice: inf / inf is 0x7FC00000 on the device and 0xFFC00000 on x86)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------- the cases of both suites
ADAMW_N = [1, 3, 4, 5, 255 * 4 + 2, 1024 + 7]
ADAMW_SCALES = [1.0, 0.125, 1.0 / 3.0]
ADAMW_STRIDE_N = 8192 * 1024 + 1024 + 3            # one element past the first trip of the capped grid, float4 body and scalar tail
HYPER = dict(lr=6e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
# |g| from 1e-6 to 1e3, zero, one inf, one NaN (they must stay inside their own element of a float4)
G_SPECIALS = [0.0, 1e-6, -1e-6, 1e-3, 1.0, -1e3, 1e3, float("inf"), 3e-5, float("nan"), -0.25, 17.0]


def adamw_case(n: int, first_step: bool, shift: int = 0, seed: int = 0):
    """(p, g, m, v, step): first_step -> m = v = 0 at step 1; otherwise step 3 with a running state.  g cycles through G_SPECIALS
    (starting at `shift`) with log-uniform magnitudes in between; where g == 0 the state is zero too (0 / eps)."""
    r = np.random.RandomState(1000 + 7 * n + seed)
    p = (r.standard_normal(n) * 0.05).astype(F32)
    g = (np.exp(r.uniform(np.log(1e-6), np.log(1e3), n)) * r.choice([-1.0, 1.0], n)).astype(F32)
    sp = np.asarray(G_SPECIALS, F32)
    idx = np.arange(0, n, 2 if n <= 64 else 5)       # every 5th element: each lane of a float4 meets each special in turn
    g[idx] = sp[(np.arange(idx.size) + shift) % len(sp)]
    if first_step:
        m, v, step = np.zeros(n, F32), np.zeros(n, F32), 1
    else:
        m, v, step = (r.standard_normal(n) * 1e-4).astype(F32), (r.uniform(size=n) * 1e-6).astype(F32), 3
        m[g == 0], v[g == 0] = 0, 0
    return p, g, m, v, step
