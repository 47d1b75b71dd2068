"""Host-side reference of the exact-fp32 GEMM (csrc/gemm.hip, dupl_gemm_f32): the case table of tests/test_gemm_f32_gpu.py, a planner
that says which of the 36 kernel instantiations a call reaches, the float64 result with an element-wise error bound, a numpy fp32
emulation of the kernel's arithmetic (tests/test_gemm32_ref_host.py shows the bound separates it from four plausible mistakes), and
the fp32 restatement of the GELU / GELU' formulas of csrc/common.h.  Needs numpy only."""
import os
import re

import numpy as np

BK = 32
U = 2.0 ** -24
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]          # (A m-contiguous, B n-contiguous)
LAYOUT_IDS = ["NT", "NN", "TT", "TN"]                                           # BLAS-style names of the same four
TILES = [(64, 64), (64, 128), (128, 0)]                                         # (tile_rows, tile_cols) forced through the descriptor

# (M, N, K): the smallest shapes at which each path of the kernel can still go wrong
CASES = [(1, 1, 1), (3, 5, 2), (4, 4, 4),        # below every tile; (4, 4, 4) is the smallest shape the branch-free loaders accept
         (64, 64, 32), (128, 128, 64),           # exact tiles, FAST 1
         (68, 132, 36),                          # FAST 2 in every layout, edge tiles in m and n for every tile size
         (65, 129, 33),                          # guarded everywhere
         (68, 132, 33),                          # FAST 2 with odd K when both operands are m- / n-contiguous, guarded otherwise
         (200, 132, 72),                         # 4 x 3 tiles: the group order and the XCD remap with 12 blocks (not a multiple of 8)
         (257, 131, 70)]                         # from test_gemm_layouts
EDGE_CASES = [(68, 132, 36), (65, 129, 33), (68, 132, 33)]
# pure accumulate (TN: both operands k-major) -> split-K: (M, N, K, batch)
SPLITK_CASES = [(8, 8, 129, 1), (8, 8, 513, 1), (64, 64, 320, 1), (8, 8, 900, 150)]


def k_ranges(K, ksplit):
    """[kbeg, kend) of every blockIdx.z, as gemm_f32_kernel computes them; an empty range (kbeg >= kend) is (kbeg, kbeg)."""
    if ksplit <= 1:
        return [(0, K)]
    kchunk = ((K + ksplit - 1) // ksplit + BK - 1) // BK * BK
    out = []
    for z in range(ksplit):
        kbeg = z * kchunk
        out.append((kbeg, max(kbeg, min(K, kbeg + kchunk))))
    return out


def dispatch(M, N, K, a_mc, b_nc, tile_rows=0, tile_cols=0, *, batch=1, pure_accum=False, deterministic=False, lda=None, ldb=None,
             aligned=True, strides=(0, 0, 0, 0)):
    """A Python restatement of the launcher dupl_gemm_f32: ((a_mc, b_nc, BM, FAST, NJ), ksplit, k-ranges) of a call.  This is a
    PLANNER for the case table -- it tells the tests which instantiation a shape is meant to reach -- not a check of the launcher:
    nothing compares it with what the library launches.
    pure_accum: flags are DUPL_GEMM_ACCUM (+ layout bits) only, no bias / res, alpha 1 (the split-K predicate); aligned: both base
    pointers 16-byte aligned; strides: (sA0, sA1, sB0, sB1) in elements."""
    lda = (M if a_mc else K) if lda is None else lda
    ldb = (N if b_nc else K) if ldb is None else ldb
    small = tile_rows == 64 if tile_rows else True
    bm = 64 if small else 128
    nbm = (M + bm - 1) // bm
    ncols = 128
    if small and (pure_accum or nbm * ((N + 127) // 128) * batch < 640):
        ncols = 64
    if tile_cols and small:
        ncols = tile_cols
    nbn = (N + ncols - 1) // ncols
    ksplit = 1
    if pure_accum:
        blocks = nbm * nbn * batch
        if blocks < 1024:
            ksplit = max(1, min((1024 + blocks - 1) // blocks, (K + 127) // 128))
    if deterministic:
        ksplit = 1
    fast = aligned and lda % 4 == 0 and ldb % 4 == 0 and K >= 4 and all(s % 4 == 0 for s in strides)
    fast = fast and ((M % 4 == 0 and M >= 4) if a_mc else K % 4 == 0)
    fast = fast and ((N % 4 == 0 and N >= 4) if b_nc else K % 4 == 0)
    FAST = (1 if K % BK == 0 else 2) if fast else 0
    return (bool(a_mc), bool(b_nc), bm, FAST, ncols // 64), ksplit, k_ranges(K, ksplit)


def gamma(n):
    return n * U / (1.0 - n * U)


def ref_and_bound(A, B, alpha=1.0, bias=None, res=None, c_old=None, ksplit=1):
    """float64 value of  alpha * A @ B + bias  (+ res) (+ c_old)  from the fp32 operands (A: [M][K], B: [K][N], logical), and an
    element-wise bound on what ANY fp32 evaluation of it may be off by -- any accumulation order, products fused or not:
        pre-activation alpha * acc + bias            gamma(K + 2) * (|alpha| S + |bias|)        S = sum_k |a| |b| in float64
        with res                                     gamma(K + 3) * (... + |res|)
        with ACCUM (c_old)                           gamma(K + 4) * (... + |c_old|)
        split-K with atomics (ksplit > 1)            gamma(K + ksplit + 1) * (S + |c_old|)
    u = 2^-24, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  RELU, ABS and
    the RELU mask are 1-Lipschitz or exact masks: apply them to the reference, the bound of their input holds for their output.
    Returns (pre, ref, bound): pre is the pre-activation alone (what an activation applies to), ref includes res / c_old."""
    A64, B64 = np.asarray(A, np.float64), np.asarray(B, np.float64)
    K = A64.shape[-1]
    pre = float(alpha) * (A64 @ B64)
    S = abs(float(alpha)) * (np.abs(A64) @ np.abs(B64))
    n = K + 2
    if bias is not None:
        b = np.asarray(bias, np.float64)
        pre, S = pre + b, S + np.abs(b)
    ref = pre
    if res is not None:
        r = np.asarray(res, np.float64)
        ref, S, n = ref + r, S + np.abs(r), n + 1
    if c_old is not None:
        c = np.asarray(c_old, np.float64)
        ref, S, n = ref + c, S + np.abs(c), K + 4
    if ksplit > 1:
        assert bias is None and res is None and alpha == 1.0 and c_old is not None
        n = K + ksplit + 1
    return pre, ref, gamma(n) * S


def emulate(A, B, alpha=1.0, bias=None, kranges=None, c_old=None, fused=True, tail_from=None):
    """The kernel's arithmetic in numpy fp32: per element one chain over k ascending (fused: one rounding per multiply-add, as the
    MFMA; not fused: two), then alpha * acc + bias; with kranges every range is a chain of its own that is added to c_old.
    tail_from = (k0, k1, times): the MISTAKE of a k-tail filled from the clamped last chunk -- the products of k in [k0, k1) enter
    the chain `times` more often (what the FAST 2 loader computes without its k-range mask)."""
    f32 = np.float32
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    M, K = A.shape
    N = B.shape[1]

    def chain(k0, k1):
        acc = np.zeros((M, N), f32)
        ks = list(range(k0, k1))
        if tail_from is not None and k1 == K:
            ks += list(range(tail_from[0], tail_from[1])) * tail_from[2]
        for k in ks:
            a, b = A[:, k:k + 1], B[k:k + 1, :]
            acc = (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(f32) if fused else acc + a * b
        return acc
    if kranges is None:
        v = f32(alpha) * chain(0, K)
        if bias is not None:
            v = v + np.asarray(bias, f32)
        return v if c_old is None else v + np.asarray(c_old, f32)
    C = np.array(c_old, f32)
    for k0, k1 in kranges:
        if k0 < k1:
            C = C + chain(k0, k1)
    return C


# ------------------------------------------------------------------------------------------ GELU as csrc/common.h computes it
def gelu_coefficients(root=None):
    """(clamp, [9 Horner coefficients]) parsed from csrc/common.h (GELU_CLAMP, GELU_Q)."""
    root = root or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "dupl_amd", "csrc", "common.h")).read()
    body = src[src.index("constexpr float GELU_CLAMP"):src.index("float gelu_f(float x)")]
    nums = [float(v) for v in re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f", body)]
    return nums[0], nums[1:10]


def gelu_phi32(x, clamp, coef):
    """Phi(x) as gelu_phi gives it in fp32: the Horner chain with one rounding per fused multiply-add, exp2 in double then rounded
    (v_exp_f32 is within 1 ulp of that)."""
    f32 = np.float32
    u = np.minimum(np.abs(x), f32(clamp)).astype(f32)
    q = np.full_like(u, f32(coef[0]))
    for c in coef[1:]:
        q = (q.astype(np.float64) * u + f32(c)).astype(f32)
    he = (f32(0.5) * np.exp2(-(q * u).astype(f32).astype(np.float64)).astype(f32)).astype(f32)
    return np.where(x >= 0, (f32(1.0) - he).astype(f32), he)


def gelu_grad32(x, clamp, coef):
    """gelu'(x) = fmaf(x, pdf, Phi(x)) as gelu_grad_f gives it in fp32."""
    f32 = np.float32
    e = ((f32(-0.72134752044448170368) * x).astype(f32) * x).astype(f32)
    pdf = (f32(0.39894228040143267794) * np.exp2(e.astype(np.float64)).astype(f32)).astype(f32)
    return (x.astype(np.float64) * pdf + gelu_phi32(x, clamp, coef)).astype(f32)
