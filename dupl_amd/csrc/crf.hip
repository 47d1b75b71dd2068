// Dense-CRF mean-field post-processing (reference: utils/dcrf.py -> pydensecrf.DenseCRF2D; tools/eval_seg_voc.py:94-153 crf_proc).
// This is the EXACT mean-field update of Kraehenbuehl & Koltun with Potts compatibility and symmetric normalisation: every
// message is the full sum over all pixel pairs,
//     M_k(Q)[c,i] = n_i * sum_j k(f_i, f_j) * n_j * Q[c,j],   n_i = 1 / sqrt(sum_j k(f_i, f_j) + 1e-20),
// where pydensecrf approximates the same sum on a permutohedral lattice.  crf_lattice.hip is that approximation; its labels have been
// compared with this code's on seeded cases (tests/test_crf_lattice_host.py), pydensecrf's own output has not.
//
// crf_dense_mfma_kernel -- the hot path (bilateral kernel; also the Gaussian one when its window covers the image): one launch
//   per kernel application.  A block streams 128-key tiles through LDS -- per key the raw features (x, y, r, g, b as exact small
//   integers) and 32 channel values n_j * Q[c,j] -- and each of its 4 waves owns 64 query pixels x 32 channels (blockIdx.y =
//   channel chunk) as two accumulator tiles of the exact-fp32 MFMA.  fp32 throughout:
//     - the feature differences and their squared sums are exact in fp32 (integers < 2^24), so the exponent carries 3 roundings;
//     - the k * Q products are the MFMA's fp32 fmaf chain; the sum over the keys is two-level: that chain inside a 128-key
//       tile, Kahan-compensated across the tiles (a plain sequential sum over 3e5 keys would lose ~sqrt(N) ulp);
//     - each wave owns its output rows: no atomics, bit-reproducible run to run.
//   Measured alternatives are in DESIGN.md (section 3, DenseCRF): the same product as VALU FMAs (v_pk_fma_f32, 2 queries x 24
//   channels per thread) was 1.6x slower; the f16x3 split on v_mfma_f32_32x32x16_f16 was not built (Q spans > 30 decades across
//   one image and the bilateral kernel can make a row's sum consist of its smallest entries: the planes would need a per-row scale).
// crf_rowsum_kernel -- n = 1 / sqrt(row sums), VALU only, once per image and kernel.
// crf_gauss_kernel -- the Gaussian (position-only) kernel as a truncated square stencil of radius R(sxy) (crf_gauss_radius): the
//   mass outside is < 2^-32 of the smallest possible row sum (>= 1, the j = i term).
// crf_softmax_kernel (crf_softmax.h, shared with crf_lattice.hip) -- energy assembly + channel softmax, one launch per iteration;
//   crf_unary_kernel -- unary from probabilities or logits (softmax, clip, -log); crf_unary_labels_kernel --
//   pydensecrf.utils.unary_from_labels.
#include "common.h"
#include "../../include/dupl_hip.h"
#include "crf_softmax.h"
#include <float.h>
#include <math.h>

namespace {

constexpr float CRF_HALF_LOG2E = 0.72134752044448170368f;    // k = exp(-d^2 / 2) = exp2(-d^2 * log2(e) / 2)

// The kernel value of one pixel pair from the raw features: the differences and the sums of their squares are exact in fp32
// (integers < 2^24), so the exponent carries three roundings.
__device__ __forceinline__ float crf_kval(float qx, float qy, float qr, float qg, float qb, const float4 f0, float fb, float ax,
                                          float ac) {
    const float dx = qx - f0.x, dy = qy - f0.y, dr = qr - f0.z, dg = qg - f0.w, db = qb - fb;
    const float ds = fmaf(dy, dy, dx * dx);
    const float dc = fmaf(db, db, fmaf(dg, dg, dr * dr));
    return __builtin_amdgcn_exp2f(-fmaf(ac, dc, ax * ds));
}

// out[i] = n_i = 1 / sqrt(sum_j k(i,j) + 1e-20): the row sums of the dense kernel (M applied to ones), once per image and kernel.
// VALU only: a thread owns 2 query pixels, the keys' features are broadcast from LDS.
constexpr int RS_KT = 128, RS_QPT = 2;
__global__ __launch_bounds__(RS_KT) void crf_rowsum_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int H, int W,
                                                           float ax, float ac) {
    __shared__ float4 kf0[RS_KT];
    __shared__ float kfb[RS_KT];
    const long N = (long)H * W;
    const int tid = threadIdx.x;
    long qi[RS_QPT];
    float qx[RS_QPT], qy[RS_QPT], qr[RS_QPT], qg[RS_QPT], qb[RS_QPT], tot[RS_QPT], cmp[RS_QPT];
#pragma unroll
    for (int q = 0; q < RS_QPT; ++q) {
        qi[q] = (long)blockIdx.x * (RS_KT * RS_QPT) + q * RS_KT + tid;
        const long ic = qi[q] < N ? qi[q] : N - 1;
        qx[q] = (float)(ic % W);
        qy[q] = (float)(ic / W);
        qr[q] = img ? (float)img[ic * 3 + 0] : 0.f;
        qg[q] = img ? (float)img[ic * 3 + 1] : 0.f;
        qb[q] = img ? (float)img[ic * 3 + 2] : 0.f;
        tot[q] = cmp[q] = 0.f;
    }
    for (long j0 = 0; j0 < N; j0 += RS_KT) {
        __syncthreads();
        const long j = j0 + tid;
        if (j < N) {
            kf0[tid] = make_float4((float)(j % W), (float)(j / W), img ? (float)img[j * 3 + 0] : 0.f, img ? (float)img[j * 3 + 1] : 0.f);
            kfb[tid] = img ? (float)img[j * 3 + 2] : 0.f;
        }
        __syncthreads();
        const int kn = (int)((N - j0) < RS_KT ? (N - j0) : RS_KT);
        float acc[RS_QPT] = {0.f, 0.f};
        for (int jj = 0; jj < kn; ++jj) {
            const float4 f0 = kf0[jj];
            const float fb = kfb[jj];
#pragma unroll
            for (int q = 0; q < RS_QPT; ++q) acc[q] += crf_kval(qx[q], qy[q], qr[q], qg[q], qb[q], f0, fb, ax, ac);
        }
#pragma unroll
        for (int q = 0; q < RS_QPT; ++q) {          // Kahan step per tile
            const float y = acc[q] - cmp[q];
            const float t = tot[q] + y;
            cmp[q] = (t - tot[q]) - y;
            tot[q] = t;
        }
    }
#pragma unroll
    for (int q = 0; q < RS_QPT; ++q)
        if (qi[q] < N) out[qi[q]] = 1.f / sqrtf(tot[q] + 1e-20f);
}

// The dense message on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): D[c][i] += sum over 2 keys of Q'[c][j] * k(j, i).
// A wave owns 64 query pixels (two 32-wide accumulator tiles) and 32 channels; per step of 2 keys a lane evaluates ONE kernel
// value per tile -- lane l: query l & 31, key l >> 5, exactly the B-operand layout -- and reads ONE A value Q'[c = l & 31][key]
// from LDS, so nothing is evaluated twice and the 2 * 32 * 32 products per MFMA cost no VALU issue slot.
constexpr int MK_KT = 128;         // keys per LDS tile
constexpr int MK_ROW = 33;         // LDS row pitch of a key's 32 channel values (33: the staging writes spread over the banks)
#define CRF_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__global__ __launch_bounds__(256, 3) void crf_dense_mfma_kernel(const uint8_t* __restrict__ img, const float* __restrict__ Q,
                                                             const float* __restrict__ nrm, float* __restrict__ out, int C, int H,
                                                             int W, float ax, float ac) {
    __shared__ float4 kf0[MK_KT];             // {x, y, r, g}
    __shared__ float kfb[MK_KT];              // b
    __shared__ float qs[MK_KT * MK_ROW];      // n_j * Q[c0 + c][j]
    const long N = (long)H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.y * 32;
    const long qbase = (long)blockIdx.x * 256 + wave * 64;
    float qx[2], qy[2], qr[2], qg[2], qb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long i = qbase + t * 32 + l31;
        const long ic = i < N ? i : N - 1;
        qx[t] = (float)(ic % W);
        qy[t] = (float)(ic / W);
        qr[t] = img ? (float)img[ic * 3 + 0] : 0.f;
        qg[t] = img ? (float)img[ic * 3 + 1] : 0.f;
        qb[t] = img ? (float)img[ic * 3 + 2] : 0.f;
    }
    f32x16 tot[2], cmp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[t][r] = cmp[t][r] = 0.f;

    for (long j0 = 0; j0 < N; j0 += MK_KT) {
        __syncthreads();
        {
            // keys past the end are staged as zeros: their (finite) kernel values meet an A operand of 0
            const int kk = tid & (MK_KT - 1), part = tid >> 7;
            const long j = j0 + kk;
            const bool ok = j < N;
            if (part == 0) {
                const bool im = ok && img;
                kf0[kk] = ok ? make_float4((float)(j % W), (float)(j / W), im ? (float)img[j * 3 + 0] : 0.f, im ? (float)img[j * 3 + 1] : 0.f)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
                kfb[kk] = im ? (float)img[j * 3 + 2] : 0.f;
            }
            const float nj = ok ? (nrm ? nrm[j] : 1.f) : 0.f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int cc = c0 + part * 16 + c;
                qs[kk * MK_ROW + part * 16 + c] = (ok && cc < C) ? Q[(long)cc * N + j] * nj : 0.f;
            }
        }
        __syncthreads();
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll 2
        for (int jj = 0; jj < MK_KT; jj += 2) {
            const int kk = jj + h;
            const float4 f0 = kf0[kk];
            const float fb = kfb[kk];
            const float a = qs[kk * MK_ROW + l31];
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc[t] = CRF_MFMA32(a, crf_kval(qx[t], qy[t], qr[t], qg[t], qb[t], f0, fb, ax, ac), acc[t]);
        }
        // Kahan step per tile: tot += acc with the rounding error carried in cmp
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float y = acc[t][r] - cmp[t][r];
                const float s = tot[t][r] + y;
                cmp[t][r] = (s - tot[t][r]) - y;
                tot[t][r] = s;
            }
    }
    // D layout: column (query) = lane & 31, row (channel) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long i = qbase + t * 32 + l31;
        if (i >= N) continue;
        const float ni = nrm ? nrm[i] : 1.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (c < C) out[(long)c * N + i] = tot[t][r] * ni;
        }
    }
}

// Truncated Gaussian stencil, one thread per (channel, pixel); Q == nullptr: out[i] = n_i.  The sum is two-level (per window
// row, then over the rows).
__global__ __launch_bounds__(256) void crf_gauss_kernel(const float* __restrict__ Q, const float* __restrict__ nrm,
                                                        float* __restrict__ out, int C, int H, int W, int R, float ax) {
    const long N = (long)H * W, total = (Q ? (long)C : 1L) * N;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long c = idx / N, i = idx - c * N;
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        const int y0 = y - R < 0 ? 0 : y - R, y1 = y + R > H - 1 ? H - 1 : y + R;
        const int x0 = x - R < 0 ? 0 : x - R, x1 = x + R > W - 1 ? W - 1 : x + R;
        float tot = 0.f;
        for (int yy = y0; yy <= y1; ++yy) {
            const float dy = (float)(yy - y);
            const float* q = Q ? Q + c * N + (long)yy * W : nullptr;
            const float* nr = nrm ? nrm + (long)yy * W : nullptr;
            float row = 0.f;
            for (int xx = x0; xx <= x1; ++xx) {
                const float dx = (float)(xx - x);
                const float k = __builtin_amdgcn_exp2f(-(ax * fmaf(dy, dy, dx * dx)));
                const float v = q ? q[xx] * (nr ? nr[xx] : 1.f) : 1.f;
                row = fmaf(k, v, row);
            }
            tot += row;
        }
        out[idx] = Q ? tot * (nrm ? nrm[i] : 1.f) : 1.f / sqrtf(tot + 1e-20f);
    }
}

// mode 0: U = -log(clip(p, 1e-5, 1)) (pydensecrf.utils.unary_from_softmax); mode 1: p = softmax_c(in) first
__global__ __launch_bounds__(256) void crf_unary_kernel(const float* __restrict__ in, float* __restrict__ U, int C, long N, int mode) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
        float mx = 0.f, s = 1.f;
        if (mode == 1) {
            mx = -INFINITY;
            for (int c = 0; c < C; ++c) mx = fmaxf(mx, in[(long)c * N + i]);
            s = 0.f;
            for (int c = 0; c < C; ++c) s += expf(in[(long)c * N + i] - mx);
        }
        for (int c = 0; c < C; ++c) {
            const long o = (long)c * N + i;
            const float p = mode == 1 ? expf(in[o] - mx) / s : in[o];
            // the logarithm in fp64, rounded once: logf is v_log_f32 (log2, 1 ulp) times ln 2, and an ulp of log2(1e-5) = -16.6 is
            // 1.4 ulp of the result 11.5 -- measured 2 fp32 values off the correctly rounded energy at the clip
            U[o] = (float)-log((double)fminf(fmaxf(p, 1e-5f), 1.f));
        }
    }
}

__global__ __launch_bounds__(256) void crf_unary_labels_kernel(const long long* __restrict__ labels, float* __restrict__ U, int C,
                                                               long N, float e_gt, float e_other) {
    const long total = (long)C * N;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long c = idx / N, i = idx - c * N;
        U[idx] = labels[i] == c ? e_gt : e_other;
    }
}

// Radius of the truncated Gaussian window: the mass outside a disc of radius R, 2 pi s^2 exp(-R^2 / 2 s^2), stays below 2^-32 of
// the smallest possible row sum (1, the j = i term) -- under fp32 round-off of that sum by 2^-8.  The square window contains the disc.
inline int crf_gauss_radius(float sxy) {
    const double s = sxy;
    const double r = s * sqrt(2.0 * (log(2.0 * M_PI * s * s + 1.0) + 32.0 * M_LN2));
    return r > 1.0e6 ? 1000000 : (int)ceil(r);
}

// log2(e) / (2 s^2), the factor of the squared distance in the exponent, saturated at FLT_MAX: for s below ~4.6e-20 the fp32
// quotient is +inf, and inf * 0 (the distance of j = i) would make k(i,i), n and every output NaN.  At FLT_MAX a distance of 0
// still gives k = 1 and every other one (>= 1: pixel and colour coordinates are integers) under-flows k to 0 -- the limit
// k = delta_ij of s -> 0.  Every finite quotient is left as it is.
inline float crf_exp_scale(float s) { return fminf(CRF_HALF_LOG2E / (s * s), FLT_MAX); }

// one application of one kernel.  Q == nullptr: out (N) = n.  img == nullptr: Gaussian kernel (srgb unused).
void crf_message_launch(const uint8_t* img, const float* Q, const float* nrm, float* out, int C, int H, int W, float sxy, float srgb,
                        hipStream_t s) {
    const long N = (long)H * W;
    const float ax = crf_exp_scale(sxy), ac = img ? crf_exp_scale(srgb) : 0.f;
    if (!img) {
        const long R = crf_gauss_radius(sxy), win = 2 * R + 1;
        if (win * win < N) {
            DUPL_LAUNCH(crf_gauss_kernel, dim3(crf_ew_grid((Q ? (long)C : 1L) * N)), dim3(256), 0, s, Q, nrm, out, C, H, W, (int)R, ax);
            return;
        }
    }
    if (!Q) {
        DUPL_LAUNCH(crf_rowsum_kernel, dim3((int)((N + RS_KT * RS_QPT - 1) / (RS_KT * RS_QPT))), dim3(RS_KT), 0, s, img, out, H, W, ax, ac);
        return;
    }
    DUPL_LAUNCH(crf_dense_mfma_kernel, dim3((int)((N + 255) / 256), (C + 31) / 32), dim3(256), 0, s, img, Q, nrm, out, C, H, W, ax, ac);
}

bool crf_dims_ok(const dupl_crf_desc* d) {
    return d && d->struct_size == sizeof(dupl_crf_desc) && d->C >= 1 && d->H >= 1 && d->W >= 1 && d->C <= 65535 &&
           (int64_t)d->H * d->W * d->C <= (int64_t)1 << 40 && (int64_t)d->H * d->W <= 0x7fffffffLL / 4;
}
bool crf_std_ok(float v) { return v > 0.f && v <= 3.0e38f; }

}  // namespace

extern "C" int dupl_crf_message(const dupl_crf_desc* d, dupl_stream_t s) {
    if (!crf_dims_ok(d) || !d->out || !crf_std_ok(d->sxy) || (d->img && !crf_std_ok(d->srgb))) return DUPL_ERR_ARG;
    if (d->Q == d->out || (d->norm && d->norm == d->out)) return DUPL_ERR_ARG;
    crf_message_launch(d->img, d->Q, d->norm, d->out, d->C, d->H, d->W, d->sxy, d->srgb, (hipStream_t)s);
    return dupl_launch_status();
}

extern "C" int dupl_dense_crf(const dupl_crf_desc* d, dupl_stream_t s) {
    if (!crf_dims_ok(d) || !d->unary || !d->out || !d->img || !d->workspace || d->T < 0) return DUPL_ERR_ARG;
    if (!crf_std_ok(d->sxy_g) || !crf_std_ok(d->sxy_b) || !crf_std_ok(d->srgb_b)) return DUPL_ERR_ARG;
    const long N = (long)d->H * d->W;
    const int C = d->C;
    if (d->workspace_bytes < (int64_t)sizeof(float) * (2 * N + 2 * (long)C * N)) return DUPL_ERR_ARG;
    hipStream_t st = (hipStream_t)s;
    float* ng = d->workspace;
    float* nb = ng + N;
    float* Mg = nb + N;
    float* Mb = Mg + (long)C * N;
    const bool use_g = d->w_g != 0.f, use_b = d->w_b != 0.f;
    const int grid = crf_ew_grid(N);
    if (d->T > 0 && use_g) crf_message_launch(nullptr, nullptr, nullptr, ng, 1, d->H, d->W, d->sxy_g, 0.f, st);
    if (d->T > 0 && use_b) crf_message_launch(d->img, nullptr, nullptr, nb, 1, d->H, d->W, d->sxy_b, d->srgb_b, st);
    DUPL_LAUNCH(crf_softmax_kernel, dim3(grid), dim3(256), 0, st, d->unary, (const float*)nullptr, (const float*)nullptr, 0.f, 0.f,
                d->out, C, N);
    for (int t = 0; t < d->T; ++t) {
        if (use_g) crf_message_launch(nullptr, d->out, ng, Mg, C, d->H, d->W, d->sxy_g, 0.f, st);
        if (use_b) crf_message_launch(d->img, d->out, nb, Mb, C, d->H, d->W, d->sxy_b, d->srgb_b, st);
        DUPL_LAUNCH(crf_softmax_kernel, dim3(grid), dim3(256), 0, st, d->unary, use_g ? (const float*)Mg : (const float*)nullptr,
                    use_b ? (const float*)Mb : (const float*)nullptr, d->w_g, d->w_b, d->out, C, N);
    }
    return dupl_launch_status();
}

extern "C" int dupl_crf_unary(const float* in, float* U, int32_t C, int64_t N, int32_t mode, dupl_stream_t s) {
    if (!in || !U || C <= 0 || N <= 0 || mode < 0 || mode > 1) return DUPL_ERR_ARG;
    DUPL_LAUNCH(crf_unary_kernel, dim3(crf_ew_grid(N)), dim3(256), 0, (hipStream_t)s, in, U, C, (long)N, mode);
    return dupl_launch_status();
}

extern "C" int dupl_crf_unary_labels(const int64_t* labels, float* U, int32_t C, int64_t N, double gt_prob, dupl_stream_t s) {
    if (!labels || !U || C < 2 || N <= 0 || !(gt_prob > 0.0 && gt_prob < 1.0)) return DUPL_ERR_ARG;
    const float e_gt = (float)-log(gt_prob), e_other = (float)-log((1.0 - gt_prob) / (C - 1));
    DUPL_LAUNCH(crf_unary_labels_kernel, dim3(crf_ew_grid((long)C * N)), dim3(256), 0, (hipStream_t)s, (const long long*)labels, U, C,
                (long)N, e_gt, e_other);
    return dupl_launch_status();
}
