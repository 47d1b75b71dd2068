// Confidence calibration of the segmentation heads (tools/eval_seg --calibration 1; beyond the reference): per image and score column
// ONE pass over the (H,W) label grid that scales the SOURCE logits by up to 16 inverse temperatures, up-samples them, takes the
// soft-max (or the mean of the two students' soft-maxes) and bins winner, confidence, negative log-likelihood and Brier score against
// the ground truth -- the counters of a reliability diagram, an ECE and a temperature fit.  No (C,H,W) probability map is written and
// nothing goes to the host; composed from dupl_scale, dupl_seg_decide, a read-back and a host bincount the same counters cost that
// chain once per temperature.
// The winner and the confidence are, per temperature, THE BITS dupl_seg_decide returns on logits that dupl_scale multiplied by
// inv_temp[t] (tools/predict --temperature does exactly that): the multiply is one pinned fp32 rounding of each source value
// (sc_mul), and everything behind it is seg_ens.hip's arithmetic, form by form:
//   one student:   maximum, then the partition sum in float64 in channel order, conf = 1 / (float)s -- whatever feeds the channels
//                  (registers, the stage, taps through L1), the sums and their order are sd_pixel_one's;
//   two students:  identity: se_pixel_regs / se_pixel_any's three sweeps (the same sums, C <= 24 from registers);
//                  up-sampling from the stage: se_pixel_lds's 4-channel chunks with the rescaled running sum -- other bits than the
//                  three sweeps, so a tile is staged exactly where dupl_seg_decide stages it (se_stage_tile, se_stage_floats);
//                  a footprint that does not fit (down-sampling): se_pixel_any's sweeps over taps read through L1;
//   probabilities: sd_pixel_prob.
// The taps are re-evaluated per temperature (the definition scales the source): VALU work under a loop that the exp unit bounds.
// Counters: bins, sums and -- up to SC_CLS_CELLS = T C cells -- cls are privatised per workgroup in LDS as 64-bit cells (pixels in
// the low word and correct pixels in the high word of one cell, the fixed-point sum in the next), pre-aggregated within a wave
// (the sums always, a bin or a class where the wave's 64 pixels agree on it), flushed with 64-bit integer atomics.  No workgroup
// waits for another, no float atomics: bit-reproducible.  The packed 32-bit halves cannot wrap: a launch has at most 2^31 pixels.
#include "seg_pixel.h"
#include "../../include/dupl_hip.h"

#include <float.h>
#include <math.h>

namespace {

enum { SC_ONE = 0, SC_TWO = 1, SC_PROB = 2 };
constexpr int SC_CLS_CELLS = 1472;       // T * C up to which cls is privatised: 23 KB beside 16 KB of bins and 24 KB of stage

struct SegCalArgs {
    const float* a;
    const float* b;
    const long long* gt;
    unsigned long long* bins;
    unsigned long long* cls;
    unsigned long long* sums;
    int C, h, w, H, W;
    int mode, T, nbins;
    int cls_priv;        // cls privatised in LDS
    int stage_cap;       // floats of stage (0: every tap through L1)
    int ns;              // students in the stage
    int tiles_x, ntiles;
    float inv[DUPL_SEG_CALIB_MAX_T];
};

struct ScPix {
    int win;
    float conf, nll, brier;
};

// v = x * inv_temp as ONE fp32 rounding, never contracted into the subtraction or the tap behind it: what dupl_scale leaves
__device__ __forceinline__ float sc_mul(float x, float k) {
#pragma clang fp contract(off)
    const float v = x * k;
    return v;
}

// One student from any source of channel values, sd_pixel_one's sums.  nll in the logit domain: finite whatever the logits.
__device__ __forceinline__ void sc_finish_one(float m, double s, double q, float vg, int best, ScPix& o) {
    const float sf = (float)s;
    o.win = best;
    o.conf = 1.f / sf;                          // the winner's exp is exactly 1
    o.nll = logf(sf) - (vg - m);
    const float pg = se_exp(vg - m) * o.conf;
    o.brier = (float)q * (o.conf * o.conf) - 2.f * pg + 1.f;
}
template <typename Val>
__device__ __forceinline__ void sc_pixel_one(Val val, int C, int g, ScPix& o) {
    float m = -INFINITY, vg = 0.f;
    int best = 0;
    for (int c = 0; c < C; ++c) {
        const float u = val(c);
        if (u > m) { m = u; best = c; }
        if (c == g) vg = u;
    }
    double s = 0.0, q = 0.0;
    for (int c = 0; c < C; ++c) {
        const float e = se_exp(val(c) - m);
        s += (double)e;
        q += (double)e * (double)e;
    }
    sc_finish_one(m, s, q, vg, best, o);
}
// identity, C <= SE_SMALL: the raw values stay in registers across the temperatures (sd_pixel_one_regs's sums)
__device__ __forceinline__ void sc_pixel_one_regs(const float (&raw)[SE_SMALL], float k, int C, int g, ScPix& o) {
    float u[SE_SMALL];
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) u[j] = j < C ? sc_mul(raw[j], k) : -INFINITY;
    float m = -INFINITY, vg = 0.f;
    int best = 0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        if (u[j] > m) { m = u[j]; best = j; }
        if (j == g) vg = u[j];
    }
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        const float e = se_exp(u[j] - m);      // the pad's exp is 0
        s += (double)e;
        q += (double)e * (double)e;
    }
    sc_finish_one(m, s, q, vg, best, o);
}

// Two students: e = (softmax(v_1) + softmax(v_2)) / 2 is seg_ens.hip's, nll and brier are taken from e itself.
__device__ __forceinline__ void sc_finish_two(float me, int be, float pg, double q, ScPix& o) {
    o.win = be;
    o.conf = me;
    o.nll = -logf(fmaxf(pg, FLT_MIN));
    o.brier = (float)q - 2.f * pg + 1.f;
}
template <typename Val>
__device__ __forceinline__ void sc_pixel_two(Val val, int C, int g, ScPix& o) {         // se_pixel_any's three sweeps
    float m1 = -INFINITY, m2 = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const float u1 = val(0, c), u2 = val(1, c);
        if (u1 > m1) m1 = u1;
        if (u2 > m2) m2 = u2;
    }
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < C; ++c) {
        s1 += (double)se_exp(val(0, c) - m1);
        s2 += (double)se_exp(val(1, c) - m2);
    }
    const float h1 = 0.5f / (float)s1, h2 = 0.5f / (float)s2;
    float me = -INFINITY, pg = 0.f;
    int be = 0;
    double q = 0.0;
    for (int c = 0; c < C; ++c) {
        const float e = fmaf(se_exp(val(0, c) - m1), h1, se_exp(val(1, c) - m2) * h2);
        if (e > me) { me = e; be = c; }
        if (c == g) pg = e;
        q += (double)e * (double)e;
    }
    sc_finish_two(me, be, pg, q, o);
}
__device__ __forceinline__ void sc_pixel_two_regs(const float (&raw1)[SE_SMALL], const float (&raw2)[SE_SMALL], float k, int C, int g,
                                                  ScPix& o) {                             // se_pixel_regs
    float u1[SE_SMALL], u2[SE_SMALL];
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        u1[j] = j < C ? sc_mul(raw1[j], k) : -INFINITY;
        u2[j] = j < C ? sc_mul(raw2[j], k) : -INFINITY;
    }
    float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        if (u1[j] > m1) m1 = u1[j];
        if (u2[j] > m2) m2 = u2[j];
    }
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        u1[j] = se_exp(u1[j] - m1);
        u2[j] = se_exp(u2[j] - m2);
        s1 += (double)u1[j];
        s2 += (double)u2[j];
    }
    const float h1 = 0.5f / (float)s1, h2 = 0.5f / (float)s2;
    float me = -INFINITY, pg = 0.f;
    int be = 0;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < SE_SMALL; ++j) {
        const float e = fmaf(u1[j], h1, u2[j] * h2);
        if (e > me) { me = e; be = j; }
        if (j == g) pg = e;
        q += (double)e * (double)e;            // the pad's e is 0
    }
    sc_finish_two(me, be, pg, q, o);
}
// the staged footprint, 4 channels at a time (se_chunk / se_pixel_lds with the source scaled as it is read)
__device__ __forceinline__ void sc_chunk(const float* st, int t00, int t01, int t10, int t11, int c0, int C, float ly, float lx, float kk,
                                         float (&u)[4]) {
    const f32x4 A = *reinterpret_cast<const f32x4*>(st + t00 + c0), B = *reinterpret_cast<const f32x4*>(st + t01 + c0);
    const f32x4 Cc = *reinterpret_cast<const f32x4*>(st + t10 + c0), D = *reinterpret_cast<const f32x4*>(st + t11 + c0);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        u[k] = c0 + k < C ? se_tap(sc_mul(A[k], kk), sc_mul(B[k], kk), sc_mul(Cc[k], kk), sc_mul(D[k], kk), ly, lx) : -INFINITY;
}
__device__ __forceinline__ void sc_pixel_two_lds(const float* st, int Cp, int t00, int t01, int t10, int t11, float ly, float lx, float kk,
                                                 int C, int g, ScPix& o) {
    float m1 = -INFINITY, m2 = -INFINITY;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 2
    for (int c0 = 0; c0 < C; c0 += 4) {
        float u1[4], u2[4];
        sc_chunk(st, t00, t01, t10, t11, c0, C, ly, lx, kk, u1);
        sc_chunk(st + Cp, t00, t01, t10, t11, c0, C, ly, lx, kk, u2);
        const float o1 = m1, o2 = m2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (u1[k] > m1) m1 = u1[k];
            if (u2[k] > m2) m2 = u2[k];
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
    float me = -INFINITY, pg = 0.f;
    int be = 0;
    double q = 0.0;
#pragma unroll 2
    for (int c0 = 0; c0 < C; c0 += 4) {
        float u1[4], u2[4];
        sc_chunk(st, t00, t01, t10, t11, c0, C, ly, lx, kk, u1);
        sc_chunk(st + Cp, t00, t01, t10, t11, c0, C, ly, lx, kk, u2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = fmaf(se_exp(u1[k] - m1), h1, se_exp(u2[k] - m2) * h2);
            if (e > me) { me = e; be = c0 + k; }
            if (c0 + k == g) pg = e;
            q += (double)e * (double)e;        // the pad's e is 0
        }
    }
    sc_finish_two(me, be, pg, q, o);
}

// probabilities at the output size (sd_pixel_prob): v = a, or the mean of a and b
__device__ __forceinline__ void sc_pixel_prob(const float* q1, const float* q2, long ps, int C, int g, ScPix& o) {
    float m = -INFINITY, pg = 0.f;
    int best = 0;
    double q = 0.0;
    for (int c = 0; c < C; ++c) {
        const float v = q2 ? 0.5f * (q1[(long)c * ps] + q2[(long)c * ps]) : q1[(long)c * ps];
        if (v > m) { m = v; best = c; }
        if (c == g) pg = v;
        q += (double)v * (double)v;
    }
    sc_finish_two(m, best, pg, q, o);
}

__device__ __forceinline__ long long sc_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one pixel into a pair of cells: [pixels | correct << 32], [sum of the fixed-point confidence]; a wave whose 64 pixels share the slot
// adds once (uni: the slot is the same on every lane, -1 included; qs: the wave's sum of q)
__device__ __forceinline__ void sc_add(unsigned long long* cell, bool uni, int slot, bool ok, unsigned long long okmask, long long q,
                                       long long qs, int lane) {
    if (uni) {
        if (lane == 0 && slot >= 0) {
            atomicAdd(&cell[0], 64ull | ((unsigned long long)__popcll(okmask) << 32));
            atomicAdd(&cell[1], (unsigned long long)qs);
        }
    } else if (slot >= 0) {
        atomicAdd(&cell[0], 1ull | ((unsigned long long)(ok ? 1 : 0) << 32));
        atomicAdd(&cell[1], (unsigned long long)q);
    }
}

__global__ __launch_bounds__(SE_THREADS) void seg_calib_kernel(const SegCalArgs a) {
    extern __shared__ __align__(16) unsigned long long sc_lds[];
    const int tid = threadIdx.x, C = a.C, H = a.H, W = a.W, h = a.h, w = a.w, T = a.T, nbins = a.nbins;
    const int lane = tid & 63, wrow = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cp = (C + 3) & ~3, ns = a.ns;
    // LDS: bins (T, nbins, 2), sums (T, 3) rounded up to an even count, cls (T, C, 2) where privatised, then the stage (16-byte aligned)
    const int n_bins = T * nbins * 2, n_sums = (T * 3 + 1) & ~1, n_cls = a.cls_priv ? T * C * 2 : 0;
    unsigned long long* s_bins = sc_lds;
    unsigned long long* s_sums = s_bins + n_bins;
    unsigned long long* s_cls = s_sums + n_sums;
    float* st = reinterpret_cast<float*>(s_cls + n_cls);
    for (int i = tid; i < n_bins + n_sums + n_cls; i += SE_THREADS) sc_lds[i] = 0ull;
    __syncthreads();
    const bool ident = h == H && w == W;
    const bool regs = ident && C <= SE_SMALL && a.mode != SC_PROB;
    const float sy = bil_scale(h, H, false), sx = bil_scale(w, W, false);
    const long HW = (long)H * W, hw = (long)h * w;
    const float* pa = a.a;
    const float* pb = a.b;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int ty0 = (t / a.tiles_x) * SE_TH, tx0 = (t % a.tiles_x) * SE_TW;
        const int x = tx0 + lane, y = ty0 + wrow;
        const bool live = x < W && y < H;
        int fy0 = 0, fx0 = 0, fw = 0;
        bool staged = false;
        if (!ident) staged = se_stage_tile(pa, pb, st, tid, ty0, tx0, C, h, w, H, W, sy, sx, a.stage_cap, fy0, fx0, fw, ns);
        const long px = (long)y * W + x;
        const long long gl = live ? a.gt[px] : -1ll;
        const bool valid = gl >= 0 && gl < C;   // evaluate._fast_hist: pixels with gt outside [0, C) are skipped
        if (__ballot(valid) == 0ull) continue;  // no barrier below this line; the lanes of a wave stay in step for the shuffles
        const int g = valid ? (int)gl : -1;
        int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
        float ly = 0.f, lx = 0.f;
        if (valid && !ident) {
            se_src(y, sy, h, y0, y1, ly);
            se_src(x, sx, w, x0, x1, lx);
        }
        float raw1[SE_SMALL], raw2[SE_SMALL];
        if (regs) {
            const long row = (long)y * W + tx0;                          // the same for all lanes of the wave
#pragma unroll
            for (int j = 0; j < SE_SMALL; ++j) {
                raw1[j] = valid && j < C ? pa[row + (long)j * HW + lane] : 0.f;
                raw2[j] = valid && j < C && a.mode == SC_TWO ? pb[row + (long)j * HW + lane] : 0.f;
            }
        }
        // the taps inside the stage (float index of the four source pixels) or inside a source plane
        const int r0 = (y0 - fy0) * fw - fx0, r1 = (y1 - fy0) * fw - fx0, ps = ns * Cp;
        const int t00 = (r0 + x0) * ps, t01 = (r0 + x1) * ps, t10 = (r1 + x0) * ps, t11 = (r1 + x1) * ps;
        const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
        for (int ti = 0; ti < T; ++ti) {
            const float k = a.inv[ti];
            ScPix o;
            o.win = 0; o.conf = 0.f; o.nll = 0.f; o.brier = 0.f;
            if (valid) {
                if (a.mode == SC_PROB) {
                    sc_pixel_prob(pa + px, pb ? pb + px : nullptr, HW, C, g, o);
                } else if (a.mode == SC_ONE) {
                    if (regs) sc_pixel_one_regs(raw1, k, C, g, o);
                    else if (ident) sc_pixel_one([&](int c) { return sc_mul(pa[px + (long)c * HW], k); }, C, g, o);
                    else if (staged)
                        sc_pixel_one([&](int c) { return se_tap(sc_mul(st[t00 + c], k), sc_mul(st[t01 + c], k), sc_mul(st[t10 + c], k),
                                                                sc_mul(st[t11 + c], k), ly, lx); }, C, g, o);
                    else
                        sc_pixel_one([&](int c) { const float* p = pa + (long)c * hw;
                                                  return se_tap(sc_mul(p[o00], k), sc_mul(p[o01], k), sc_mul(p[o10], k), sc_mul(p[o11], k),
                                                                ly, lx); }, C, g, o);
                } else if (regs) {
                    sc_pixel_two_regs(raw1, raw2, k, C, g, o);
                } else if (ident) {
                    sc_pixel_two([&](int s, int c) { return sc_mul((s ? pb : pa)[px + (long)c * HW], k); }, C, g, o);
                } else if (staged) {
                    sc_pixel_two_lds(st, Cp, t00, t01, t10, t11, ly, lx, k, C, g, o);
                } else {
                    sc_pixel_two([&](int s, int c) { const float* p = (s ? pb : pa) + (long)c * hw;
                                                     return se_tap(sc_mul(p[o00], k), sc_mul(p[o01], k), sc_mul(p[o10], k),
                                                                   sc_mul(p[o11], k), ly, lx); }, C, g, o);
                }
            }
            // ---- counters (every lane of the wave is here)
            int bin = (int)(o.conf * (float)nbins);
            bin = bin < nbins - 1 ? bin : nbins - 1;
            bin = bin > 0 ? bin : 0;            // a negative "probability" (is_prob on something else) stays inside the table
            const int slot_b = valid ? bin : -1, slot_c = valid ? o.win : -1;
            const bool ok = valid && o.win == g;
            const long long q = valid ? (long long)rintf(o.conf * 16777216.f) : 0ll;
            const long long nl = valid ? (long long)rintf(fminf(o.nll, DUPL_SEG_CALIB_NLL_MAX) * 1048576.f) : 0ll;
            const long long br = valid ? (long long)rintf(o.brier * 16777216.f) : 0ll;
            const unsigned long long vmask = __ballot(valid), okmask = __ballot(ok);
            const long long nls = sc_wave_sum(nl), brs = sc_wave_sum(br);
            if (lane == 0) {
                atomicAdd(&s_sums[ti * 3], (unsigned long long)__popcll(vmask) | ((unsigned long long)__popcll(okmask) << 32));
                atomicAdd(&s_sums[ti * 3 + 1], (unsigned long long)nls);
                atomicAdd(&s_sums[ti * 3 + 2], (unsigned long long)brs);
            }
            const bool uni_b = __ballot(slot_b != __builtin_amdgcn_readfirstlane(slot_b)) == 0ull;
            const bool uni_c = __ballot(slot_c != __builtin_amdgcn_readfirstlane(slot_c)) == 0ull;
            long long qs = 0ll;
            if (uni_b || uni_c) qs = sc_wave_sum(q);
            if (a.bins) sc_add(s_bins + (ti * nbins + (slot_b < 0 ? 0 : slot_b)) * 2, uni_b, slot_b, ok, okmask, q, qs, lane);
            if (a.cls) {
                if (a.cls_priv) {
                    sc_add(s_cls + (ti * C + (slot_c < 0 ? 0 : slot_c)) * 2, uni_c, slot_c, ok, okmask, q, qs, lane);
                } else if (uni_c ? (lane == 0 && slot_c >= 0) : slot_c >= 0) {
                    unsigned long long* cell = a.cls + ((long)ti * C + slot_c) * 3;
                    atomicAdd(&cell[0], uni_c ? 64ull : 1ull);
                    const unsigned long long nok = uni_c ? (unsigned long long)__popcll(okmask) : (ok ? 1ull : 0ull);
                    if (nok) atomicAdd(&cell[1], nok);
                    atomicAdd(&cell[2], (unsigned long long)(uni_c ? qs : q));
                }
            }
        }
    }
    __syncthreads();
    // flush: (pixels, correct, sum) per cell
    if (a.bins) {
        for (int i = tid; i < T * nbins; i += SE_THREADS) {
            const unsigned long long nc = s_bins[2 * i];
            if (nc) {
                atomicAdd(&a.bins[3 * i], nc & 0xffffffffull);
                if (nc >> 32) atomicAdd(&a.bins[3 * i + 1], nc >> 32);
                atomicAdd(&a.bins[3 * i + 2], s_bins[2 * i + 1]);
            }
        }
    }
    if (a.cls && a.cls_priv) {
        for (int i = tid; i < T * C; i += SE_THREADS) {
            const unsigned long long nc = s_cls[2 * i];
            if (nc) {
                atomicAdd(&a.cls[3 * i], nc & 0xffffffffull);
                if (nc >> 32) atomicAdd(&a.cls[3 * i + 1], nc >> 32);
                atomicAdd(&a.cls[3 * i + 2], s_cls[2 * i + 1]);
            }
        }
    }
    if (a.sums) {
        for (int i = tid; i < T; i += SE_THREADS) {
            const unsigned long long nc = s_sums[3 * i];
            if (nc) {
                atomicAdd(&a.sums[4 * i], nc & 0xffffffffull);
                if (nc >> 32) atomicAdd(&a.sums[4 * i + 1], nc >> 32);
                atomicAdd(&a.sums[4 * i + 2], s_sums[3 * i + 1]);
                atomicAdd(&a.sums[4 * i + 3], s_sums[3 * i + 2]);
            }
        }
    }
}

}  // namespace

extern "C" int dupl_seg_calib(const dupl_seg_calib_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_seg_calib_desc)) return DUPL_ERR_ARG;
    if (!d->a || !d->gt || !d->inv_temp || d->reserved0 != 0) return DUPL_ERR_ARG;
    if (d->C < 1 || d->C > DUPL_SEG_CALIB_MAX_C || d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0) return DUPL_ERR_ARG;
    if ((long)d->H * d->W > 0x7ffffff0L || (long)d->h * d->w > 0x7ffffff0L) return DUPL_ERR_ARG;
    if (d->T < 1 || d->T > DUPL_SEG_CALIB_MAX_T || d->nbins < 1 || d->nbins > DUPL_SEG_CALIB_MAX_BINS) return DUPL_ERR_ARG;
    for (int t = 0; t < d->T; ++t)
        if (!isfinite(d->inv_temp[t]) || !(d->inv_temp[t] > 0.f)) return DUPL_ERR_ARG;
    if (d->is_prob && (d->h != d->H || d->w != d->W || d->T != 1 || d->inv_temp[0] != 1.0f)) return DUPL_ERR_ARG;
    if (!d->bins && !d->cls && !d->sums) return DUPL_ERR_ARG;
    SegCalArgs a;
    a.a = d->a; a.b = d->b; a.gt = (const long long*)d->gt;
    a.bins = (unsigned long long*)d->bins; a.cls = (unsigned long long*)d->cls; a.sums = (unsigned long long*)d->sums;
    a.C = d->C; a.h = d->h; a.w = d->w; a.H = d->H; a.W = d->W;
    a.mode = d->is_prob ? SC_PROB : (d->b ? SC_TWO : SC_ONE);
    a.T = d->T; a.nbins = d->nbins;
    for (int t = 0; t < DUPL_SEG_CALIB_MAX_T; ++t) a.inv[t] = t < d->T ? d->inv_temp[t] : 1.f;
    a.cls_priv = d->cls && d->T * d->C <= SC_CLS_CELLS;
    // two students stage exactly where dupl_seg_decide does (the staged sums are other bits); one student's bits do not depend on it
    a.ns = a.mode == SC_TWO ? 2 : 1;
    a.stage_cap = a.mode == SC_PROB ? 0 : se_stage_floats(d->C, d->h, d->w, d->H, d->W, a.ns);
    a.tiles_x = (d->W + SE_TW - 1) / SE_TW;
    const long ntiles = (long)a.tiles_x * ((d->H + SE_TH - 1) / SE_TH);
    if (ntiles > 0x7fffffffL) return DUPL_ERR_ARG;
    a.ntiles = (int)ntiles;
    const long grid = ntiles < 2048 ? ntiles : 2048;
    const size_t cells = (size_t)d->T * d->nbins * 2 + (size_t)((d->T * 3 + 1) & ~1) + (a.cls_priv ? (size_t)d->T * d->C * 2 : 0);
    const size_t lds = sizeof(unsigned long long) * cells + sizeof(float) * (size_t)a.stage_cap;
    DUPL_LAUNCH(seg_calib_kernel, dim3((unsigned)grid), dim3(SE_THREADS), lds, (hipStream_t)stream, a);
    return dupl_launch_status();
}
