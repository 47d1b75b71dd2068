// Ensemble of the two students at evaluation time (tools/eval_seg --ensemble 1; beyond the reference, which scores each student alone):
// per output pixel the bilinear up-sampling of both students' accumulated logits, their softmax over the channels, the mean of the two
// probability vectors, and the argmax of each student and of the mean -- ONE pass over the (H,W) label grid that also accumulates the
// three confusion matrices and the two agreement counters.  The up-sampled logits and the per-student probabilities live in registers
// only; composed from resize_bilinear, softmax, argmax_channels and confusion_accum the same result moves two (C,H,W) fp32 maps through
// HBM four times.  Floor: one read of both students' logits + 8 B/px of gt + what is asked for (8 B/px pred, 4 C B/px prob).
//   identity (VOC: the logits are already at label size): a thread reads its pixel's 2 C values straight from HBM -- once, kept in
//     registers, when C <= 24; channel by channel in three sweeps (maximum, partition sum, mean) beyond;
//   up-sampling (COCO: 28 x 28 logits, 254 KB per student, L2-resident): a workgroup owns a 64 x 4 output tile and stages the few
//     source pixels under it (x C x 2 students) in LDS, channel-fastest, so a tap is one 16-byte LDS read per 4 channels; the channel
//     loop runs twice (maximum + partition sum, then the mean).  Where the footprint does not fit (down-sampling) the taps are read
//     through L1, channel by channel.
// Histograms: 3 C^2 counters of 16 bits privatised per workgroup in LDS where they fit 40 KB (C <= 82) and flushed with 64-bit atomics,
// otherwise 64-bit atomics straight to hist.  Integer atomics only: the result is bit-reproducible in either mode.
// seg_decide_kernel (below) is the same pass without a ground truth, for tools/predict: winner, confidence, rejection, label bytes and
// per-label statistics on the same tiles, for one student, two, or probabilities (DenseCRF's marginals).
#include "seg_pixel.h"                   // the tile, the tap, the exp and the staging: shared with seg_calib.hip
#include "../../include/dupl_hip.h"

namespace {

constexpr int SE_BINS = 20480;           // 16-bit counters, two to a word (40 KB): 3 * 82^2 = 20172
constexpr int SE_BLOCK_TILES = 255;      // tiles per workgroup at most: 255 * 256 pixels cannot overflow a 16-bit counter

struct SegEnsArgs {
    const float* a;
    const float* b;
    const long long* gt;
    unsigned long long* hist;
    unsigned long long* counts;
    long long* pred;
    float* prob;
    int C, h, w, H, W;
    int priv;            // histograms privatised in LDS
    int bin_words;       // words of LDS in front of the stage
    int stage_cap;       // floats of stage (0: every tap through L1)
    int tiles_x, ntiles;
};

// Identity, C <= SE_SMALL (the VOC form).  r1 / r2: channel 0 of the wave's row segment (the same for all lanes: the loads take a
// scalar base and the lane as offset, so SE_SMALL of them per student are in flight without an address register each).  Both
// students' values are read ONCE and stay in registers through maximum, partition sum and mean: one exp per value.
__device__ __forceinline__ void se_pixel_regs(const float* __restrict__ r1, const float* __restrict__ r2, int lane, int C,
                                              float* __restrict__ prow, long HW, int& b1, int& b2, int& be, float& me) {
    float u1[SE_SMALL], u2[SE_SMALL];
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {       // channels past C read as -inf: exp gives 0 and no argmax takes them
        u1[j] = j < C ? r1[(long)j * HW + lane] : -INFINITY;
        u2[j] = j < C ? r2[(long)j * HW + lane] : -INFINITY;
    }
    float m1 = -INFINITY, m2 = -INFINITY;
    b1 = 0; b2 = 0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        if (u1[j] > m1) { m1 = u1[j]; b1 = j; }
        if (u2[j] > m2) { m2 = u2[j]; b2 = j; }
    }
    double s1 = 0.0, s2 = 0.0;                 // the partition sums in float64: the channel sums of e stay within rounding of 1
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        u1[j] = se_exp(u1[j] - m1);
        u2[j] = se_exp(u2[j] - m2);
        s1 += (double)u1[j];
        s2 += (double)u2[j];
    }
    const float h1 = 0.5f / (float)s1, h2 = 0.5f / (float)s2;          // e = (p1 + p2) / 2 = ex1 * (0.5 / s1) + ex2 * (0.5 / s2)
    me = -INFINITY;
    be = 0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        const float e = fmaf(u1[j], h1, u2[j] * h2);
        if (e > me) { me = e; be = j; }
        if (prow && j < C) prow[(long)j * HW + lane] = e;
    }
}

// Up-sampling from the staged footprint.  The stage holds, per source pixel, student 1's Cp channels and then student 2's (Cp = C
// rounded up to 4, the pad is 0): a tap is one 16-byte LDS read per 4 channels, and the four taps of a pixel need one address each.
// t00 .. t11: float index of the four source pixels.  The channel loop runs twice, 4 channels at a time: first the maximum and the
// partition sum together (the running sum is rescaled when a chunk raises the maximum), then the mean of the two probability
// vectors and its argmax.
__device__ __forceinline__ void se_chunk(const float* st, int t00, int t01, int t10, int t11, int c0, int C, float ly, float lx,
                                         float (&u)[4]) {
    const f32x4 A = *reinterpret_cast<const f32x4*>(st + t00 + c0), B = *reinterpret_cast<const f32x4*>(st + t01 + c0);
    const f32x4 Cc = *reinterpret_cast<const f32x4*>(st + t10 + c0), D = *reinterpret_cast<const f32x4*>(st + t11 + c0);
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = c0 + k < C ? se_tap(A[k], B[k], Cc[k], D[k], ly, lx) : -INFINITY;
}
__device__ __forceinline__ void se_pixel_lds(const float* st, int Cp, int t00, int t01, int t10, int t11, float ly, float lx, int C,
                                             float* prob, long HW, int& b1, int& b2, int& be, float& me) {
    float m1 = -INFINITY, m2 = -INFINITY;
    double s1 = 0.0, s2 = 0.0;
    b1 = 0; b2 = 0;
#pragma unroll 2
    for (int c0 = 0; c0 < C; c0 += 4) {
        float u1[4], u2[4];
        se_chunk(st, t00, t01, t10, t11, c0, C, ly, lx, u1);
        se_chunk(st + Cp, t00, t01, t10, t11, c0, C, ly, lx, u2);
        const float o1 = m1, o2 = m2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (u1[k] > m1) { m1 = u1[k]; b1 = c0 + k; }
            if (u2[k] > m2) { m2 = u2[k]; b2 = c0 + k; }
        }
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a1 += se_exp(u1[k] - m1);
            a2 += se_exp(u2[k] - m2);
        }
        s1 = s1 * (double)se_exp(o1 - m1) + (double)a1;                 // first chunk: o = -inf, the factor is 0
        s2 = s2 * (double)se_exp(o2 - m2) + (double)a2;
    }
    const float h1 = 0.5f / (float)s1, h2 = 0.5f / (float)s2;
    me = -INFINITY;
    be = 0;
#pragma unroll 2
    for (int c0 = 0; c0 < C; c0 += 4) {
        float u1[4], u2[4];
        se_chunk(st, t00, t01, t10, t11, c0, C, ly, lx, u1);
        se_chunk(st + Cp, t00, t01, t10, t11, c0, C, ly, lx, u2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = fmaf(se_exp(u1[k] - m1), h1, se_exp(u2[k] - m2) * h2);
            if (e > me) { me = e; be = c0 + k; }
            if (prob && c0 + k < C) prob[(long)(c0 + k) * HW] = e;
        }
    }
}

// Everything else (identity with more channels, a footprint too large to stage: down-sampling), channel by channel through L1 / L2:
// maximum, partition sum, mean.  IDENT: q points at the pixel itself, channel stride ps; otherwise at channel 0 of the source, ps the
// plane stride and o00 .. o11 the four taps inside a plane.
template <bool IDENT>
__device__ __forceinline__ void se_pixel_any(const float* q1, const float* q2, long ps, int o00, int o01, int o10, int o11, float ly,
                                             float lx, int C, float* prob, long HW, int& b1, int& b2, int& be, float& me) {
    auto val = [&](const float* q, int c) -> float {
        const float* p = q + (long)c * ps;
        if (IDENT) return p[0];
        return se_tap(p[o00], p[o01], p[o10], p[o11], ly, lx);
    };
    float m1 = -INFINITY, m2 = -INFINITY;
    b1 = 0; b2 = 0;
    for (int c = 0; c < C; ++c) {
        const float u1 = val(q1, c), u2 = val(q2, c);
        if (u1 > m1) { m1 = u1; b1 = c; }
        if (u2 > m2) { m2 = u2; b2 = c; }
    }
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < C; ++c) {
        s1 += (double)se_exp(val(q1, c) - m1);
        s2 += (double)se_exp(val(q2, c) - m2);
    }
    const float h1 = 0.5f / (float)s1, h2 = 0.5f / (float)s2;
    me = -INFINITY;
    be = 0;
    for (int c = 0; c < C; ++c) {
        const float e = fmaf(se_exp(val(q1, c) - m1), h1, se_exp(val(q2, c) - m2) * h2);
        if (e > me) { me = e; be = c; }
        if (prob) prob[(long)c * HW] = e;
    }
}

__global__ __launch_bounds__(SE_THREADS) void seg_ens_kernel(const SegEnsArgs a) {
    extern __shared__ __align__(16) unsigned int se_lds[];
    unsigned int* bins32 = se_lds;
    float* st = reinterpret_cast<float*>(se_lds + a.bin_words);          // bin_words is a multiple of 4: 16-byte aligned
    const int tid = threadIdx.x, C = a.C, H = a.H, W = a.W, h = a.h, w = a.w;
    const int lane = tid & 63, wrow = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = 3 * C * C, Cp = (C + 3) & ~3;
    const bool want_hist = a.hist != nullptr, want_cnt = a.counts != nullptr;
    const bool priv = want_hist && a.priv;
    if (priv) {
        for (int i = tid; i < (nb + 1) / 2; i += SE_THREADS) bins32[i] = 0u;
        __syncthreads();
    }
    const bool ident = h == H && w == W;       // as torch: the same size is a copy, nothing is interpolated
    const float sy = bil_scale(h, H, false), sx = bil_scale(w, W, false);
    const long HW = (long)H * W, hw = (long)h * w;
    int n_valid = 0, n_agree = 0;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int ty0 = (t / a.tiles_x) * SE_TH, tx0 = (t % a.tiles_x) * SE_TW;
        const int x = tx0 + lane, y = ty0 + wrow;
        const bool live = x < W && y < H;
        int fy0 = 0, fx0 = 0, fw = 0;
        bool staged = false;
        if (!ident) staged = se_stage_tile(a.a, a.b, st, tid, ty0, tx0, C, h, w, H, W, sy, sx, a.stage_cap, fy0, fx0, fw);
        if (!live) continue;                   // no barrier below this line
        const long px = (long)y * W + x;
        float* prob = a.prob ? a.prob + px : nullptr;
        int b1, b2, be;
        float me;
        if (ident && C <= SE_SMALL) {
            const long row = (long)y * W + tx0;                      // the same for all lanes of the wave
            se_pixel_regs(a.a + row, a.b + row, lane, C, a.prob ? a.prob + row : nullptr, HW, b1, b2, be, me);
        } else if (ident) {
            se_pixel_any<true>(a.a + px, a.b + px, HW, 0, 0, 0, 0, 0.f, 0.f, C, prob, HW, b1, b2, be, me);
        } else {
            int y0, y1, x0, x1;
            float ly, lx;
            se_src(y, sy, h, y0, y1, ly);
            se_src(x, sx, w, x0, x1, lx);
            if (staged) {
                const int r0 = (y0 - fy0) * fw - fx0, r1 = (y1 - fy0) * fw - fx0, ps = 2 * Cp;
                se_pixel_lds(st, Cp, (r0 + x0) * ps, (r0 + x1) * ps, (r1 + x0) * ps, (r1 + x1) * ps, ly, lx, C, prob, HW, b1, b2, be, me);
            } else {
                se_pixel_any<false>(a.a, a.b, hw, y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1, ly, lx, C, prob, HW, b1, b2, be, me);
            }
        }
        if (a.pred) a.pred[px] = be;
        if (!want_hist && !want_cnt) continue;
        const long long g = a.gt[px];
        if (g < 0 || g >= C) continue;         // evaluate._fast_hist: pixels with gt outside [0, C) are skipped
        ++n_valid;
        n_agree += b1 == b2 ? 1 : 0;
        if (!want_hist) continue;
        const int row = (int)g * C, cc = C * C;
        const int i1 = row + b1, i2 = cc + row + b2, i3 = 2 * cc + row + be;
        if (priv) {
            atomicAdd(&bins32[i1 >> 1], 1u << ((i1 & 1) * 16));
            atomicAdd(&bins32[i2 >> 1], 1u << ((i2 & 1) * 16));
            atomicAdd(&bins32[i3 >> 1], 1u << ((i3 & 1) * 16));
        } else {
            atomicAdd(&a.hist[i1], 1ull);
            atomicAdd(&a.hist[i2], 1ull);
            atomicAdd(&a.hist[i3], 1ull);
        }
    }
    if (priv) {
        __syncthreads();
        for (int i = tid; i < nb; i += SE_THREADS) {
            const unsigned int v = (bins32[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
            if (v) atomicAdd(&a.hist[i], (unsigned long long)v);
        }
    }
    if (want_cnt) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_valid += __shfl_xor(n_valid, o, 64);
            n_agree += __shfl_xor(n_agree, o, 64);
        }
        if ((tid & 63) == 0 && n_valid) {
            atomicAdd(&a.counts[0], (unsigned long long)n_valid);
            if (n_agree) atomicAdd(&a.counts[1], (unsigned long long)n_agree);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- dupl_seg_decide
// The tail of a label-less run (tools/predict) on the same tiles: winner, its confidence, rejection under min_conf, the label map as
// bytes and the per-label pixel counts and confidence sums.  Two students take the ensemble's own pixel functions above (the label
// and conf are the bits of seg_ens_kernel's pred and prob); one student needs two sweeps only -- maximum, partition sum -- since
// conf = softmax(u)[argmax u] = 1 / sum exp(u - max); probabilities (what DenseCRF returns) need one.
enum { SD_ONE = 0, SD_TWO = 1, SD_PROB = 2 };
constexpr int SD_SLOTS = 256;            // DUPL_SEG_DECIDE_MAX_C labels + the rejected pixels

struct SegDecArgs {
    const float* a;
    const float* b;
    float* conf;
    unsigned char* label;
    unsigned long long* stats;
    int C, h, w, H, W;
    int mode, ignore;
    float min_conf;
    int stage_cap, tiles_x, ntiles;
};

// IDENT: q points at the pixel itself, channel stride ps; otherwise at channel 0 of the source, ps the plane stride, o00 .. o11 the taps
template <bool IDENT>
__device__ __forceinline__ void sd_pixel_one(const float* q, long ps, int o00, int o01, int o10, int o11, float ly, float lx, int C,
                                             int& best, float& conf) {
    auto val = [&](int c) -> float {
        const float* p = q + (long)c * ps;
        if (IDENT) return p[0];
        return se_tap(p[o00], p[o01], p[o10], p[o11], ly, lx);
    };
    float m = -INFINITY;
    best = 0;
    for (int c = 0; c < C; ++c) {
        const float u = val(c);
        if (u > m) { m = u; best = c; }
    }
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)se_exp(val(c) - m);
    conf = 1.f / (float)s;                     // the winner's exp is exactly 1
}

// Identity, C <= SE_SMALL, one student (the VOC form): as se_pixel_regs, the wave's row segment is read once and stays in registers
// through both sweeps.  The same sums in the same order as sd_pixel_one: the same bits.
__device__ __forceinline__ void sd_pixel_one_regs(const float* __restrict__ r, int lane, int C, long HW, int& best, float& conf) {
    float u[SE_SMALL];
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) u[j] = j < C ? r[(long)j * HW + lane] : -INFINITY;
    float m = -INFINITY;
    best = 0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j)
        if (u[j] > m) { m = u[j]; best = j; }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) s += (double)se_exp(u[j] - m);      // the pad's exp is 0
    conf = 1.f / (float)s;
}

// probabilities at the output size: v = a, or the mean of a and b; the winner and its value
__device__ __forceinline__ void sd_pixel_prob(const float* q1, const float* q2, long ps, int C, int& best, float& conf) {
    float m = -INFINITY;
    best = 0;
    for (int c = 0; c < C; ++c) {
        const float v = q2 ? 0.5f * (q1[(long)c * ps] + q2[(long)c * ps]) : q1[(long)c * ps];
        if (v > m) { m = v; best = c; }
    }
    conf = m;
}

__global__ __launch_bounds__(SE_THREADS) void seg_decide_kernel(const SegDecArgs a) {
    extern __shared__ __align__(16) unsigned int se_lds[];
    __shared__ unsigned int s_cnt[SD_SLOTS];
    __shared__ unsigned long long s_sum[SD_SLOTS];
    float* st = reinterpret_cast<float*>(se_lds);
    const int tid = threadIdx.x, C = a.C, H = a.H, W = a.W, h = a.h, w = a.w;
    const int lane = tid & 63, wrow = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cp = (C + 3) & ~3;
    const bool want_stats = a.stats != nullptr;
    if (want_stats) {
        for (int i = tid; i <= C; i += SE_THREADS) { s_cnt[i] = 0u; s_sum[i] = 0ull; }
        __syncthreads();
    }
    const bool ident = h == H && w == W;
    const float sy = bil_scale(h, H, false), sx = bil_scale(w, W, false);
    const long HW = (long)H * W, hw = (long)h * w;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int ty0 = (t / a.tiles_x) * SE_TH, tx0 = (t % a.tiles_x) * SE_TW;
        const int x = tx0 + lane, y = ty0 + wrow;
        const bool live = x < W && y < H;
        int fy0 = 0, fx0 = 0, fw = 0;
        bool staged = false;
        if (a.mode == SD_TWO && !ident) staged = se_stage_tile(a.a, a.b, st, tid, ty0, tx0, C, h, w, H, W, sy, sx, a.stage_cap, fy0, fx0, fw);
        const long px = (long)y * W + x;
        int win = 0;
        float cf = 0.f;
        if (live) {                            // the lanes off the grid stay in step: the epilogue shuffles across the wave
            int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
            float ly = 0.f, lx = 0.f;
            if (!ident) {
                se_src(y, sy, h, y0, y1, ly);
                se_src(x, sx, w, x0, x1, lx);
            }
            int b1, b2;
            if (a.mode == SD_PROB) {
                sd_pixel_prob(a.a + px, a.b ? a.b + px : nullptr, HW, C, win, cf);
            } else if (a.mode == SD_ONE) {
                if (ident && C <= SE_SMALL) sd_pixel_one_regs(a.a + ((long)y * W + tx0), lane, C, HW, win, cf);
                else if (ident) sd_pixel_one<true>(a.a + px, HW, 0, 0, 0, 0, 0.f, 0.f, C, win, cf);
                else sd_pixel_one<false>(a.a, hw, y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1, ly, lx, C, win, cf);
            } else if (ident && C <= SE_SMALL) {
                const long row = (long)y * W + tx0;
                se_pixel_regs(a.a + row, a.b + row, lane, C, nullptr, HW, b1, b2, win, cf);
            } else if (ident) {
                se_pixel_any<true>(a.a + px, a.b + px, HW, 0, 0, 0, 0, 0.f, 0.f, C, nullptr, HW, b1, b2, win, cf);
            } else if (staged) {
                const int r0 = (y0 - fy0) * fw - fx0, r1 = (y1 - fy0) * fw - fx0, ps = 2 * Cp;
                se_pixel_lds(st, Cp, (r0 + x0) * ps, (r0 + x1) * ps, (r1 + x0) * ps, (r1 + x1) * ps, ly, lx, C, nullptr, HW, b1, b2, win, cf);
            } else {
                se_pixel_any<false>(a.a, a.b, hw, y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1, ly, lx, C, nullptr, HW, b1, b2, win, cf);
            }
            if (a.conf) a.conf[px] = cf;
        }
        const bool rej = cf < a.min_conf;
        if (a.label) {
            // four labels to a word where the word lies inside this wave's row segment; the row ends (W is arbitrary) byte by byte
            const unsigned int lab = live ? (unsigned int)(rej ? a.ignore : win) : 0u;
            const unsigned int l1 = __shfl_down(lab, 1, 64), l2 = __shfl_down(lab, 2, 64), l3 = __shfl_down(lab, 3, 64);
            if (live) {
                unsigned char* p = a.label + px;
                const int k = (int)(reinterpret_cast<unsigned long long>(p) & 3ull);
                const bool full = lane >= k && lane - k + 3 < 64 && x - k + 3 < W;
                if (!full) *p = (unsigned char)lab;
                else if (k == 0) *reinterpret_cast<unsigned int*>(p) = lab | (l1 << 8) | (l2 << 16) | (l3 << 24);
            }
        }
        if (want_stats) {
            // neighbouring pixels mostly share a label: a wave whose 64 pixels agree adds once; otherwise a pixel at a time
            const int slot = live ? (rej ? C : win) : -1;
            long long q = live ? (long long)rintf(cf * 16777216.f) : 0ll;
            const int first = __builtin_amdgcn_readfirstlane(slot);
            if (__ballot(slot != first) == 0ull) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
                if (lane == 0 && first >= 0) {
                    atomicAdd(&s_cnt[first], 64u);
                    atomicAdd(&s_sum[first], (unsigned long long)q);
                }
            } else if (live) {
                atomicAdd(&s_cnt[slot], 1u);
                atomicAdd(&s_sum[slot], (unsigned long long)q);
            }
        }
    }
    if (want_stats) {
        __syncthreads();
        for (int i = tid; i <= C; i += SE_THREADS) {
            if (s_cnt[i]) {
                atomicAdd(&a.stats[i], (unsigned long long)s_cnt[i]);
                atomicAdd(&a.stats[C + 1 + i], s_sum[i]);
            }
        }
    }
}

}  // namespace

extern "C" int dupl_seg_decide(const dupl_seg_decide_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_seg_decide_desc)) return DUPL_ERR_ARG;
    if (!d->a) return DUPL_ERR_ARG;
    if (d->C < 1 || d->C > DUPL_SEG_DECIDE_MAX_C || d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0) return DUPL_ERR_ARG;
    if ((long)d->H * d->W > 0x7ffffff0L || (long)d->h * d->w > 0x7ffffff0L) return DUPL_ERR_ARG;
    if (d->is_prob && (d->h != d->H || d->w != d->W)) return DUPL_ERR_ARG;
    if (d->ignore_index < 0 || d->ignore_index > 255 || d->reserved0 != 0) return DUPL_ERR_ARG;
    if (!d->conf && !d->label && !d->stats) return DUPL_ERR_ARG;
    SegDecArgs a;
    a.a = d->a; a.b = d->b; a.conf = d->conf; a.label = d->label; a.stats = (unsigned long long*)d->stats;
    a.C = d->C; a.h = d->h; a.w = d->w; a.H = d->H; a.W = d->W;
    a.mode = d->is_prob ? SD_PROB : (d->b ? SD_TWO : SD_ONE);
    a.ignore = d->ignore_index;
    a.min_conf = d->min_conf;
    a.stage_cap = a.mode == SD_TWO ? se_stage_floats(d->C, d->h, d->w, d->H, d->W) : 0;
    a.tiles_x = (d->W + SE_TW - 1) / SE_TW;
    const long ntiles = (long)a.tiles_x * ((d->H + SE_TH - 1) / SE_TH);
    if (ntiles > 0x7fffffffL) return DUPL_ERR_ARG;
    a.ntiles = (int)ntiles;
    const long grid = ntiles < 2048 ? ntiles : 2048;
    DUPL_LAUNCH(seg_decide_kernel, dim3((unsigned)grid), dim3(SE_THREADS), sizeof(float) * (size_t)a.stage_cap, (hipStream_t)stream, a);
    return dupl_launch_status();
}

extern "C" int dupl_seg_ensemble(const dupl_seg_ensemble_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_seg_ensemble_desc)) return DUPL_ERR_ARG;
    if (!d->a || !d->b) return DUPL_ERR_ARG;
    if (d->C < 1 || d->C > DUPL_SEG_ENSEMBLE_MAX_C || d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0) return DUPL_ERR_ARG;
    if ((long)d->H * d->W > 0x7ffffff0L || (long)d->h * d->w > 0x7ffffff0L) return DUPL_ERR_ARG;
    if (!d->hist && !d->counts && !d->pred && !d->prob) return DUPL_ERR_ARG;
    if ((d->hist || d->counts) && !d->gt) return DUPL_ERR_ARG;
    SegEnsArgs a;
    a.a = d->a; a.b = d->b; a.gt = (const long long*)d->gt;
    a.hist = (unsigned long long*)d->hist; a.counts = (unsigned long long*)d->counts;
    a.pred = (long long*)d->pred; a.prob = d->prob;
    a.C = d->C; a.h = d->h; a.w = d->w; a.H = d->H; a.W = d->W;
    const int nb = 3 * d->C * d->C;
    a.priv = d->hist && nb <= SE_BINS;
    a.bin_words = a.priv ? (((nb + 1) / 2 + 3) & ~3) : 0;               // the stage behind it stays 16-byte aligned
    a.stage_cap = se_stage_floats(d->C, d->h, d->w, d->H, d->W);
    a.tiles_x = (d->W + SE_TW - 1) / SE_TW;
    const long ntiles = (long)a.tiles_x * ((d->H + SE_TH - 1) / SE_TH);
    if (ntiles > 0x7fffffffL) return DUPL_ERR_ARG;
    a.ntiles = (int)ntiles;
    long grid = ntiles < 2048 ? ntiles : 2048;
    if (a.priv && grid * SE_BLOCK_TILES < ntiles) grid = (ntiles + SE_BLOCK_TILES - 1) / SE_BLOCK_TILES;
    const size_t lds = sizeof(unsigned int) * (size_t)a.bin_words + sizeof(float) * (size_t)a.stage_cap;
    DUPL_LAUNCH(seg_ens_kernel, dim3((unsigned)grid), dim3(SE_THREADS), lds, (hipStream_t)stream, a);
    return dupl_launch_status();
}
