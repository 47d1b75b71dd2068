// Offline CAM inference (tools/infer_cam_voc.py:69-92 of the reference) after the 448^2 multi-scale CAMs: the reference resizes two
// (1,C,H,W) CAM stacks per image, builds a label map per background threshold and moves every map to the host for evaluate.scores.
// Here the whole tail is ONE pass over the (H,W) label grid that samples only the classes present in the image: max / argmax, the
// label map at one threshold, the max value for the overlay, and the confusion matrices of T thresholds at once.  Per pixel the
// maximum v and its channel a do not depend on the threshold; with thr ascending the pixel is foreground at threshold t exactly
// when t < k, k = #{t : thr[t] < v}.  A histogram over (gt, class slot, k) therefore holds all T matrices (a suffix sum over k).
// The counters are privatised per workgroup in LDS (16 bits each) and flushed with 64-bit atomics; where (T + 1) counters per
// (gt, slot) row do not fit, the thresholds are taken in chunks, and where not even one fits the counts go to hist directly.
// HBM-bound streaming kernels: 8 B (gt) in, 5 B (value + label) out per pixel; the low-resolution CAMs (448^2 floats per class
// present) are read through L1 / L2.
#include "common.h"
#include "../../include/dupl_hip.h"

namespace {

// The tap of resize_bilinear_kernel (cam.hip), hy * (hx a + lx b) + ly * (hx c + lx d), with every rounding pinned to what hipcc makes
// of that kernel: top = fma(lx, b, hx a), bot = fma(lx, d, hx c), v = fma(hy, top, ly bot).  Written as the plain expression the four
// pixels of a thread are vectorised into packed operations here and the contraction comes out differently (fma(hx, a, lx b), a plain
// final add): label maps and values of the fused pass must equal resize -> cam_to_label bit for bit, so nothing is left to the compiler.
__device__ __forceinline__ float ce_tap(const float* __restrict__ p, int Wi, int y0, int y1, int x0, int x1, float ly, float lx) {
#pragma clang fp contract(off)
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float top = __builtin_fmaf(lx, p[(long)y0 * Wi + x1], hx * p[(long)y0 * Wi + x0]);
    const float bot = __builtin_fmaf(lx, p[(long)y1 * Wi + x1], hx * p[(long)y1 * Wi + x0]);
    return __builtin_fmaf(hy, top, ly * bot);
}

constexpr int CE_THREADS = 256;
// 60 KB of 16-bit counters, two to a word (a workgroup never takes more than CE_BLOCK_PX pixels, so none can overflow into its
// neighbour): VOC at T = 19 needs 21 x 3 x 20, COCO with 17 classes present 81 x 18 x 20 = 29 160
constexpr int CE_BINS = 30720;
constexpr int CE_BLOCK_PX = 64512;   // 63 groups of 4 pixels per thread at most (dupl_cam_eval sizes the grid accordingly)
constexpr int CE_SLOTS = 256;        // DUPL_CAM_EVAL_MAX_C present classes + the zero of the absent ones

struct CamEvalArgs {
    const float* cam;
    const float* cls;
    const long long* gt;
    unsigned long long* hist;
    unsigned char* label;
    float* value;
    int B, C, h, w, H, W, T, nc, label_at, impl, vec;
    float thr[DUPL_CAM_EVAL_MAX_T];
};

// grid (blocks over the pixel groups of one image, B); a thread takes 4 consecutive pixels of the flattened (H,W) grid.
__global__ __launch_bounds__(CE_THREADS) void cam_eval_kernel(const CamEvalArgs a) {
    __shared__ unsigned int bins32[CE_BINS / 2];
    unsigned short* bins = reinterpret_cast<unsigned short*>(bins32);          // little endian: counter i = half (i & 1) of word i / 2
    __shared__ float slot_w[CE_SLOTS];
    __shared__ int slot_c[CE_SLOTS];
    __shared__ int s_n;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int C = a.C, T = a.T, nc = a.nc, W = a.W;
    // The slots of this image, in channel order: every class present (weight = its cls_label entry) and, at the index of the FIRST
    // absent channel, one slot of weight 0 -- cls_label * cam is exactly 0 on every absent channel, and max(dim=1) returns the first
    // of equal maxima, so the later zeros can never win.  An image without classes has that slot alone: all background.
    if (tid < 64) {
        const float* cl = a.cls + (long)b * C;
        int first_absent = C;
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + tid;
            const unsigned long long m = __ballot(c < C && cl[c] == 0.f);
            if (m && first_absent == C) first_absent = c0 + __ffsll((long long)m) - 1;
        }
        int n = 0;
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + tid;
            const float wv = c < C ? cl[c] : 0.f;
            const bool is = c < C && (wv != 0.f || c == first_absent);
            const unsigned long long m = __ballot(is);
            if (is) {
                const int pos = n + __popcll(m & ((1ull << tid) - 1ull));
                slot_c[pos] = c;
                slot_w[pos] = wv;
            }
            n += __popcll(m);
        }
        if (tid == 0) s_n = n;
    }
    __syncthreads();
    const int S = s_n;
    const int rows = nc * S;                          // nc <= 4096, S <= 256
    const bool want_hist = a.hist != nullptr;
    // Thresholds per pass over the workgroup's pixels: as many as the counters hold, (Tc + 1) per row.  All T in one pass for VOC and
    // for COCO with up to 17 classes present at T = 19; otherwise the pixels are sampled once per chunk of thresholds (for the chunk
    // [t0, t0 + Tn) the bin index is k - t0 clamped to [0, Tn]).  Where not even one threshold fits: global atomics.
    int Tc = 0;
    if (want_hist && a.impl == 0 && rows <= CE_BINS / 2) Tc = CE_BINS / rows - 1 < T ? CE_BINS / rows - 1 : T;
    const bool priv = Tc >= 1;
    const int nchunks = priv ? (T + Tc - 1) / Tc : 1;
    const int HW = a.H * W, hw = a.h * a.w;
    const float sy = bil_scale(a.h, a.H, false), sx = bil_scale(a.w, W, false);
    const float* camb = a.cam + (long)b * C * hw;
    const long base = (long)b * HW;
    const float thr_l = a.label ? a.thr[a.label_at] : 0.f;
    const int ngroups = (HW + 3) >> 2;
    const int lane = tid & 63;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int t0 = chunk * Tc;
        const int Tn = priv ? (T - t0 < Tc ? T - t0 : Tc) : T;
        const int T1 = Tn + 1;
        const bool first = chunk == 0;                // value_out and label_out are written by the first pass
        if (priv) {
            for (int i = tid; i < (rows * T1 + 1) / 2; i += CE_THREADS) bins32[i] = 0u;
            __syncthreads();
        }
        // the trip count is the same for every lane of a wave (the global-atomics histogram below votes across the wave): a thread
        // past the last group computes group 0 again and stores nothing
        for (int jb = blockIdx.x * CE_THREADS; jb < ngroups; jb += gridDim.x * CE_THREADS) {
            const bool live = jb + tid < ngroups;
            const int p0 = live ? (jb + tid) * 4 : 0;
            const int np = !live ? 0 : (HW - p0 < 4 ? HW - p0 : 4);
            float val[4];
            int sl[4], kk[4], ch[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = p0 + q < HW ? p0 + q : HW - 1;      // the tail recomputes the last pixel and stores nothing for it
                const int y = p / W, x = p - y * W;
                int y0, y1, x0, x1;
                float ly, lx;
                bil_src(y, sy, a.h, false, y0, y1, ly);
                bil_src(x, sx, a.w, false, x0, x1, lx);
                float best = -INFINITY;
                int bs = 0;
                for (int s = 0; s < S; ++s) {
                    const float wv = slot_w[s];
                    float v = 0.f;
                    if (wv != 0.f) v = wv * ce_tap(camb + (long)slot_c[s] * hw, a.w, y0, y1, x0, x1, ly, lx);
                    if (v > best) { best = v; bs = s; }
                }
                int k = 0;
                for (int t = 0; t < T; ++t) k += a.thr[t] < best ? 1 : 0;
                val[q] = best; sl[q] = bs; kk[q] = k; ch[q] = slot_c[bs];
            }
            if (a.value && first) {
                if (a.vec && live) *reinterpret_cast<float4*>(a.value + base + p0) = make_float4(val[0], val[1], val[2], val[3]);
                else if (!a.vec)
                    for (int q = 0; q < np; ++q) a.value[base + p0 + q] = val[q];
            }
            if (a.label && first) {
                unsigned int lab[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) lab[q] = val[q] <= thr_l ? 0u : (unsigned int)(ch[q] + 1);
                if (a.vec && live)
                    *reinterpret_cast<unsigned int*>(a.label + base + p0) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
                else if (!a.vec)
                    for (int q = 0; q < np; ++q) a.label[base + p0 + q] = (unsigned char)lab[q];
            }
            if (!want_hist) continue;
            long long g[4] = {-1, -1, -1, -1};
            if (a.vec && live) {
                const longlong2 g01 = *reinterpret_cast<const longlong2*>(a.gt + base + p0);
                const longlong2 g23 = *reinterpret_cast<const longlong2*>(a.gt + base + p0 + 2);
                g[0] = g01.x; g[1] = g01.y; g[2] = g23.x; g[3] = g23.y;
            } else if (!a.vec) {
                for (int q = 0; q < np; ++q) g[q] = a.gt[base + p0 + q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in = g[q] >= 0 && g[q] < nc;
                if (priv) {
                    if (in) {
                        const int kc = kk[q] - t0 < 0 ? 0 : (kk[q] - t0 > Tn ? Tn : kk[q] - t0);
                        const int i = ((int)g[q] * S + sl[q]) * T1 + kc;
                        atomicAdd(&bins32[i >> 1], 1u << ((i & 1) * 16));
                    }
                    continue;
                }
                // Straight to hist, but not T atomics per pixel.  Neighbouring pixels mostly share (gt, class, k): the wave votes on
                // one key at a time, and lane t adds the key's pixel count to the matrix of threshold t (T <= 64 lanes, T addresses).
                const unsigned int key = in ? ((unsigned int)g[q] << 15) | ((unsigned int)ch[q] << 7) | (unsigned int)kk[q] : 0u;
                unsigned long long todo = __ballot(in);
                while (todo) {
                    const unsigned int lk = __shfl(key, __ffsll((long long)todo) - 1, 64);
                    const unsigned long long same = __ballot(in && key == lk);
                    todo &= ~same;
                    if (lane < T) {
                        const int gl = (int)(lk >> 15), cl = (int)((lk >> 7) & 255u), kl = (int)(lk & 127u);
                        atomicAdd(&a.hist[((long)lane * nc + gl) * nc + (lane < kl ? cl + 1 : 0)], (unsigned long long)__popcll(same));
                    }
                }
            }
        }
        if (!priv) break;
        // bins[row][k] -> suffix sums over k (a thread per row, 16-bit accesses): afterwards bins[row][t + 1] = pixels of the row
        // that are foreground at threshold t0 + t, bins[row][0] = all pixels of the row; the others are background (prediction 0)
        __syncthreads();
        for (int r = tid; r < rows; r += CE_THREADS) {
            unsigned int run = 0u;
            for (int k = Tn; k >= 0; --k) {
                run += bins[r * T1 + k];
                bins[r * T1 + k] = (unsigned short)run;
            }
        }
        __syncthreads();
        // a thread per (gt, t): one atomic per class with foreground pixels, one for the background of all slots together
        for (int i = tid; i < nc * Tn; i += CE_THREADS) {
            const int g = i / Tn, t = i - g * Tn;
            unsigned long long* row = a.hist + ((long)(t0 + t) * nc + g) * nc;
            unsigned int bg = 0u;
            for (int s = 0; s < S; ++s) {
                const int r = g * S + s;
                const unsigned int tot = bins[r * T1];
                if (!tot) continue;
                const unsigned int fg = bins[r * T1 + t + 1];
                if (fg) atomicAdd(&row[slot_c[s] + 1], (unsigned long long)fg);
                bg += tot - fg;
            }
            if (bg) atomicAdd(&row[0], (unsigned long long)bg);
        }
        __syncthreads();
    }
}

// matplotlib's `jet` (matplotlib/_cm.py _jet_data: (x, y) nodes, no jumps) through the arithmetic of
// matplotlib.colors._create_lookup_table for N = 256, gamma = 1, operation by operation in float64.
__device__ const int JET_N[3] = {5, 6, 5};
__device__ const double JET_X[3][6] = {{0., .35, .66, .89, 1., 1.}, {0., .125, .375, .64, .91, 1.}, {0., .11, .34, .65, 1., 1.}};
__device__ const double JET_Y[3][6] = {{0., 0., 1., 1., .5, .5}, {0., 0., 1., 1., 0., 0.}, {.5, 1., 1., 0., 0., 0.}};

__device__ double jet_entry(int c, int i) {
#pragma clang fp contract(off)
    const int n = JET_N[c];
    if (i == 0) return JET_Y[c][0];
    if (i == 255) return JET_Y[c][n - 1];
    const double xi = 255.0 * ((double)i * (1.0 / 255.0));            // (N - 1) * linspace(0, 1, N)[i]
    int j = 1;
    while (j < n - 1 && JET_X[c][j] * 255.0 < xi) ++j;                // searchsorted(x * (N - 1), xi), side "left"
    const double xa = JET_X[c][j - 1] * 255.0, xb = JET_X[c][j] * 255.0;
    const double dist = (xi - xa) / (xb - xa);
    const double v = dist * (JET_Y[c][j] - JET_Y[c][j - 1]) + JET_Y[c][j - 1];
    return fmin(fmax(v, 0.0), 1.0);
}

struct OvMeanStd { float mean[3], stdv[3]; };

// a thread takes 4 consecutive pixels of the flattened (B,H,W) grid: one 16-byte load of value, 12 bytes of interleaved RGB out
__global__ __launch_bounds__(256) void cam_overlay_kernel(const float* __restrict__ value, const float* __restrict__ img,
                                                          unsigned char* __restrict__ out, long n, int HW, double alpha,
                                                          const OvMeanStd ms, int vec) {
    __shared__ double lut[256 * 3];                                   // 255 * jet, as `color_map(v)[:, :, :3] * 255`
    for (int i = threadIdx.x; i < 256 * 3; i += blockDim.x) {
#pragma clang fp contract(off)
        lut[i] = jet_entry(i % 3, i / 3) * 255.0;
    }
    __syncthreads();
    const double beta = 1.0 - alpha;
    const long ngroups = (n + 3) >> 2;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < ngroups; j += (long)gridDim.x * blockDim.x) {
        const long i0 = j * 4;
        const int np = n - i0 < 4 ? (int)(n - i0) : 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (np == 4 && vec) {
            const float4 t = *reinterpret_cast<const float4*>(value + i0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            for (int q = 0; q < np; ++q) v[q] = value[i0 + q];
        }
        unsigned int byte[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int idx = (int)(v[q] * 256.f);                            // exact in fp32; int(v * 256) of the 256-entry colormap call
            idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);
            const long i = i0 + (q < np ? q : 0);
            const long bi = i / HW, p = i - bi * HW;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma clang fp contract(off)
                double r = lut[idx * 3 + c];
                if (img) {
                    const float prod = img[(bi * 3 + c) * HW + p] * ms.stdv[c];      // the rule of denormalize_kernel (cam.hip)
                    const float d = prod + ms.mean[c];
                    const unsigned char u = (unsigned char)((int)d & 0xff);
                    const double fa = alpha * r, fb = beta * (double)u;
                    r = fa + fb;
                }
                byte[q * 3 + c] = (unsigned int)(unsigned char)(int)r;
            }
        }
        unsigned char* o = out + i0 * 3;
        if (np == 4 && vec) {
            unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
            o4[0] = byte[0] | (byte[1] << 8) | (byte[2] << 16) | (byte[3] << 24);
            o4[1] = byte[4] | (byte[5] << 8) | (byte[6] << 16) | (byte[7] << 24);
            o4[2] = byte[8] | (byte[9] << 8) | (byte[10] << 16) | (byte[11] << 24);
        } else {
            for (int q = 0; q < np * 3; ++q) o[q] = (unsigned char)byte[q];
        }
    }
}

}  // namespace

extern "C" int dupl_cam_eval(const dupl_cam_eval_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_cam_eval_desc)) return DUPL_ERR_ARG;
    if (!d->cam || !d->cls_label || !d->thr) return DUPL_ERR_ARG;
    if (d->B <= 0 || d->B > 65535 || d->C <= 0 || d->C > DUPL_CAM_EVAL_MAX_C || d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0)
        return DUPL_ERR_ARG;
    if ((long)d->H * d->W > 0x7ffffff0L || (long)d->h * d->w > 0x7ffffff0L) return DUPL_ERR_ARG;
    if (d->T < 1 || d->T > DUPL_CAM_EVAL_MAX_T || d->impl < 0 || d->impl > 1) return DUPL_ERR_ARG;
    for (int t = 0; t < d->T; ++t) {
        if (!(d->thr[t] >= 0.f && d->thr[t] <= 1.f)) return DUPL_ERR_ARG;            // NaN fails too
        if (t && d->thr[t] < d->thr[t - 1]) return DUPL_ERR_ARG;
    }
    if (!d->hist && !d->label_out && !d->value_out) return DUPL_ERR_ARG;
    if (d->hist && (!d->gt || d->num_classes < d->C + 1 || d->num_classes > 4096)) return DUPL_ERR_ARG;
    if (d->label_out && (d->label_at < 0 || d->label_at >= d->T)) return DUPL_ERR_ARG;
    CamEvalArgs a;
    a.cam = d->cam; a.cls = d->cls_label; a.gt = (const long long*)d->gt; a.hist = (unsigned long long*)d->hist;
    a.label = d->label_out; a.value = d->value_out;
    a.B = d->B; a.C = d->C; a.h = d->h; a.w = d->w; a.H = d->H; a.W = d->W; a.T = d->T;
    a.nc = d->hist ? d->num_classes : 1;
    a.label_at = d->label_out ? d->label_at : 0;
    a.impl = d->impl;
    const long HW = (long)d->H * d->W;
    a.vec = !(HW & 3) && !(reinterpret_cast<uintptr_t>(d->value_out) & 15) && !(reinterpret_cast<uintptr_t>(d->label_out) & 3) &&
            !(reinterpret_cast<uintptr_t>(d->gt) & 15);
    for (int t = 0; t < DUPL_CAM_EVAL_MAX_T; ++t) a.thr[t] = t < d->T ? d->thr[t] : 0.f;
    const long groups = (HW + 3) / 4;                           // pixel groups of one image
    long gx = (groups + CE_THREADS - 1) / CE_THREADS;
    if (gx > 256) gx = 256;                                    // one workgroup per CU; more only to keep a workgroup's share of the
    const long group_cap = CE_BLOCK_PX / 4;                    // pixels within what its 16-bit counters can hold
    if (gx * group_cap < groups) gx = (groups + group_cap - 1) / group_cap;
    DUPL_LAUNCH(cam_eval_kernel, dim3((unsigned)gx, (unsigned)d->B), dim3(CE_THREADS), 0, (hipStream_t)stream, a);
    return dupl_launch_status();
}

extern "C" int dupl_cam_overlay(const float* value, const float* img, uint8_t* out, int32_t B, int32_t H, int32_t W, double alpha,
                                const float* mean_std, dupl_stream_t s) {
    if (!value || !out || B <= 0 || H <= 0 || W <= 0 || !(alpha >= 0.0 && alpha <= 1.0)) return DUPL_ERR_ARG;
    if ((long)H * W > 0x7ffffff0L) return DUPL_ERR_ARG;
    OvMeanStd ms = {{123.675f, 116.28f, 103.53f}, {58.395f, 57.12f, 57.375f}};       // imutils.py:17 defaults, as dupl_denormalize_img
    if (mean_std)
        for (int c = 0; c < 3; ++c) { ms.mean[c] = mean_std[c]; ms.stdv[c] = mean_std[3 + c]; }
    const long n = (long)B * H * W;
    const int vec = !(reinterpret_cast<uintptr_t>(value) & 15) && !(reinterpret_cast<uintptr_t>(out) & 3);
    long g = ((n + 3) / 4 + 255) / 256;
    if (g > 2048) g = 2048;
    DUPL_LAUNCH(cam_overlay_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)s, value, img, out, n, (int)(H * W), alpha, ms,
                vec);
    return dupl_launch_status();
}
