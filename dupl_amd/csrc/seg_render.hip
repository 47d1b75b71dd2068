// Label-less inference around the encoder (tools/predict; beyond the reference, which needs a data set around every image):
//   seg_paint      label map (+ image) -> palette image / overlay with optional contours, integer arithmetic only.  A thread owns one
//                  aligned 4-byte word of the (H,W,3) byte stream (parts of two pixels) and stores it whole; the bytes in front of
//                  the first and behind the last full word go one by one.  3 B/px out, 1 (+3) B/px in: HBM / launch-bound.
//   window_gather  the sliding windows of the resized image and of its horizontal flip, cut straight from the source: the bits of
//                  resize_bilinear(flip_cat) (cam.hip) sliced, without the resized image ever reaching memory.
//   window_merge   the windows' logits back onto the (2,C,hs,ws) canvas msc_seg_accum consumes: a thread per canvas element adds the
//                  covering windows in ascending index and divides once -- no atomics, bit-reproducible.
// The window origins travel in the kernel arguments (at most DUPL_WINDOW_MAX): the calls check them on the host first.
// (dupl_seg_decide, the fourth entry point of the tool, sits with the ensemble's pixel functions in seg_ens.hip.)
#include "common.h"
#include "../../include/dupl_hip.h"

namespace {

constexpr int SR_THREADS = 256;

inline int sr_grid(long n) {
    const long g = (n + SR_THREADS - 1) / SR_THREADS;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ------------------------------------------------------------------------------------------------------------------- seg_paint
struct PaintArgs {
    const unsigned char* label;
    const unsigned char* image;
    const unsigned char* palette;
    unsigned char* out;
    int H, W, alpha, tint, contour;
    unsigned int crgb;                   // r | g << 8 | b << 16
};

// the colour of pixel p as r | g << 8 | b << 16
__device__ __forceinline__ unsigned int sr_colour(const PaintArgs& a, long p) {
    const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
    const unsigned int l = a.label[p];
    if (a.contour && ((x + 1 < a.W && a.label[p + 1] != l) || (y + 1 < a.H && a.label[p + a.W] != l))) return a.crgb;
    const unsigned char* pal = a.palette + 3 * l;
    unsigned int c[3] = {pal[0], pal[1], pal[2]};
    if (a.image) {
        const unsigned char* im = a.image + 3 * p;
        const bool keep = l == 0 && !a.tint;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = keep ? im[k] : (im[k] * (256u - a.alpha) + c[k] * a.alpha + 128u) >> 8;
    }
    return c[0] | (c[1] << 8) | (c[2] << 16);
}

__global__ __launch_bounds__(SR_THREADS) void seg_paint_kernel(const PaintArgs a) {
    const long N = 3L * a.H * a.W;                                        // bytes of out
    const int off = (int)(reinterpret_cast<unsigned long long>(a.out) & 3ull);
    const long words = (N + off + 3) / 4;
    for (long t = (long)blockIdx.x * SR_THREADS + threadIdx.x; t < words; t += (long)gridDim.x * SR_THREADS) {
        const long j0 = 4 * t - off, jlo = j0 < 0 ? 0 : j0;               // bytes j0 .. j0 + 3 of out, those inside [0, N)
        const long pA = jlo / 3;                                          // they belong to pixels pA and pA + 1
        const unsigned int cA = sr_colour(a, pA);
        const unsigned int cB = 3 * (pA + 1) < N && 3 * (pA + 1) <= j0 + 3 ? sr_colour(a, pA + 1) : 0u;
        unsigned int word = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long j = j0 + k;
            if (j < 0 || j >= N) continue;
            const long p = j / 3;
            const int ch = (int)(j - 3 * p);
            word |= (((p == pA ? cA : cB) >> (8 * ch)) & 0xffu) << (8 * k);
        }
        if (j0 >= 0 && j0 + 3 < N) {
            *reinterpret_cast<unsigned int*>(a.out + j0) = word;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k >= 0 && j0 + k < N) a.out[j0 + k] = (unsigned char)(word >> (8 * k));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- sliding windows
struct WindowArgs {
    const float* in;
    float* out;
    int C, h, w, Hs, Ws, nW, wh, ww;
    int org[2 * DUPL_WINDOW_MAX];
};

// The tap of resize_bilinear_kernel (cam.hip) with every rounding pinned to what hipcc makes of that kernel (as cam_eval.hip does):
// top = fma(lx, b, hx a), bot = fma(lx, d, hx c), v = fma(hy, top, ly bot).
__device__ __forceinline__ float sr_tap(const float* __restrict__ p, int Wi, int y0, int y1, int x0, int x1, float ly, float lx) {
#pragma clang fp contract(off)
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float top = __builtin_fmaf(lx, p[(long)y0 * Wi + x1], hx * p[(long)y0 * Wi + x0]);
    const float bot = __builtin_fmaf(lx, p[(long)y1 * Wi + x1], hx * p[(long)y1 * Wi + x0]);
    return __builtin_fmaf(hy, top, ly * bot);
}

// out[f nW + k][c][y][x] = R[c][r0 + y][X], X = c0 + x for f = 0 and Ws - 1 - (c0 + x) for the flipped half; R = resize(in, Hs, Ws)
__global__ __launch_bounds__(SR_THREADS) void window_gather_kernel(const WindowArgs a) {
    const long per = (long)a.wh * a.ww, total = 2L * a.nW * a.C * per;
    const float sy = bil_scale(a.h, a.Hs, false), sx = bil_scale(a.w, a.Ws, false);
    for (long i = (long)blockIdx.x * SR_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SR_THREADS) {
        const int x = (int)(i % a.ww), y = (int)((i / a.ww) % a.wh);
        const long kc = i / per;                                          // (f nW + k) C + c
        const int c = (int)(kc % a.C), fk = (int)(kc / a.C), f = fk >= a.nW ? 1 : 0, k = fk - f * a.nW;
        const int Y = a.org[2 * k] + y, X0 = a.org[2 * k + 1] + x, X = f ? a.Ws - 1 - X0 : X0;
        int y0, y1, x0, x1;
        float ly, lx;
        bil_src(Y, sy, a.h, false, y0, y1, ly);
        bil_src(X, sx, a.w, false, x0, x1, lx);
        a.out[i] = sr_tap(a.in + (long)c * a.h * a.w, a.w, y0, y1, x0, x1, ly, lx);
    }
}

// canvas[f][c][y][x] = (sum over the windows k covering (y,x), ascending, of in[f nW + k][c][y - r0][x - c0]) / their number
__global__ __launch_bounds__(SR_THREADS) void window_merge_kernel(const WindowArgs a) {
    const long plane = (long)a.Hs * a.Ws, total = 2L * a.C * plane, per = (long)a.wh * a.ww;
    for (long i = (long)blockIdx.x * SR_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * SR_THREADS) {
        const int x = (int)(i % a.Ws), y = (int)((i / a.Ws) % a.Hs);
        const long fc = i / plane;
        const int c = (int)(fc % a.C), f = (int)(fc / a.C);
        float sum = 0.f;
        int n = 0;
        for (int k = 0; k < a.nW; ++k) {
            const int dy = y - a.org[2 * k], dx = x - a.org[2 * k + 1];
            if (dy < 0 || dy >= a.wh || dx < 0 || dx >= a.ww) continue;
            sum += a.in[(((long)f * a.nW + k) * a.C + c) * per + (long)dy * a.ww + dx];
            ++n;
        }
        a.out[i] = n ? sum / (float)n : 0.f;
    }
}

// every window inside the (Hs,Ws) grid; copies the origins into the kernel arguments
bool sr_windows(WindowArgs& a, const int32_t* origins) {
    if (!origins || a.nW < 1 || a.nW > DUPL_WINDOW_MAX || a.wh <= 0 || a.ww <= 0 || a.Hs <= 0 || a.Ws <= 0) return false;
    for (int k = 0; k < a.nW; ++k) {
        const int r0 = origins[2 * k], c0 = origins[2 * k + 1];
        if (r0 < 0 || c0 < 0 || (long)r0 + a.wh > a.Hs || (long)c0 + a.ww > a.Ws) return false;
        a.org[2 * k] = r0;
        a.org[2 * k + 1] = c0;
    }
    return true;
}

}  // namespace

extern "C" int dupl_seg_paint(const dupl_seg_paint_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_seg_paint_desc)) return DUPL_ERR_ARG;
    if (!d->label || !d->palette || !d->out || d->H <= 0 || d->W <= 0 || (long)d->H * d->W > 0x7ffffff0L / 3) return DUPL_ERR_ARG;
    if (d->alpha256 < 0 || d->alpha256 > 256 || (d->tint_background & ~1) || (d->contour & ~1) || d->reserved0 != 0) return DUPL_ERR_ARG;
    PaintArgs a;
    a.label = d->label; a.image = d->image; a.palette = d->palette; a.out = d->out;
    a.H = d->H; a.W = d->W; a.alpha = d->alpha256; a.tint = d->tint_background; a.contour = d->contour;
    a.crgb = (unsigned int)d->contour_rgb[0] | ((unsigned int)d->contour_rgb[1] << 8) | ((unsigned int)d->contour_rgb[2] << 16);
    DUPL_LAUNCH(seg_paint_kernel, dim3(sr_grid((3L * d->H * d->W + 6) / 4)), dim3(SR_THREADS), 0, (hipStream_t)stream, a);
    return dupl_launch_status();
}

extern "C" int dupl_window_gather(const dupl_window_gather_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_window_gather_desc)) return DUPL_ERR_ARG;
    if (!d->x || !d->out || d->h <= 0 || d->w <= 0) return DUPL_ERR_ARG;
    if ((long)d->h * d->w > 0x7ffffff0L / 3 || (long)d->Hs * d->Ws > 0x7ffffff0L) return DUPL_ERR_ARG;
    WindowArgs a;
    a.in = d->x; a.out = d->out; a.C = 3; a.h = d->h; a.w = d->w; a.Hs = d->Hs; a.Ws = d->Ws; a.nW = d->nW; a.wh = d->wh; a.ww = d->ww;
    if (!sr_windows(a, d->origins)) return DUPL_ERR_ARG;
    DUPL_LAUNCH(window_gather_kernel, dim3(sr_grid(6L * a.nW * a.wh * a.ww)), dim3(SR_THREADS), 0, (hipStream_t)stream, a);
    return dupl_launch_status();
}

extern "C" int dupl_window_merge(const dupl_window_merge_desc* d, dupl_stream_t stream) {
    if (!d || d->struct_size != sizeof(dupl_window_merge_desc)) return DUPL_ERR_ARG;
    if (!d->logits || !d->canvas || d->C < 1 || (long)d->hs * d->ws > 0x7ffffff0L) return DUPL_ERR_ARG;
    WindowArgs a;
    a.in = d->logits; a.out = d->canvas; a.C = d->C; a.h = 0; a.w = 0; a.Hs = d->hs; a.Ws = d->ws; a.nW = d->nW; a.wh = d->wth; a.ww = d->wtw;
    if (!sr_windows(a, d->origins)) return DUPL_ERR_ARG;
    DUPL_LAUNCH(window_merge_kernel, dim3(sr_grid(2L * a.C * a.Hs * a.Ws)), dim3(SR_THREADS), 0, (hipStream_t)stream, a);
    return dupl_launch_status();
}
