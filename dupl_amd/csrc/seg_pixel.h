// What the passes over the (H,W) label grid share (seg_ens.hip: seg_ens_kernel, seg_decide_kernel; seg_calib.hip): the 64 x 4 output
// tile, the source index and the bilinear tap with every rounding pinned, the one-instruction exp, and the staging of the source
// pixels under a tile in LDS.
#pragma once
#include "common.h"

namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_TW = 64, SE_TH = 4;     // output tile: a wave per row segment, 256 contiguous bytes per channel of prob
constexpr int SE_STAGE = 6144;           // floats of staged source pixels (24 KB): COCO 84 x 2 x (3 x 5) = 2520
constexpr int SE_SMALL = 24;             // identity: channels a thread keeps in registers -- one read of the logits (VOC: 21)

// The students' predictions must be the bits of upsample_argmax_kernel (eval.hip), so the source index and the tap are that kernel's
// arithmetic with every rounding pinned to what hipcc makes of it there: r = fma(scale, o + 0.5, -0.5);
// v = hy * (hx a + lx b) + ly * (hx c + lx d) with top = fma(hx, a, lx b), bot = fma(hx, c, lx d) and a plain hy top + ly bot.
__device__ __forceinline__ void se_src(int o, float scale, int in, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
    const float r = fmaxf(__builtin_fmaf(scale, (float)o + 0.5f, -0.5f), 0.f);
    i0 = (int)r;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = r - (float)i0;
}
__device__ __forceinline__ float se_tap(float a, float b, float c, float d, float ly, float lx) {
#pragma clang fp contract(off)
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float top = __builtin_fmaf(hx, a, lx * b);
    const float bot = __builtin_fmaf(hx, c, lx * d);
    const float t = hy * top, u = ly * bot;
    return t + u;
}

// exp(x) for x <= 0 as one v_exp_f32: the relative error grows with |x| ((|x| + 1) * 6e-8), the value shrinks as exp(x): no
// probability is off by more than 1e-7 (tests: prob against float64, beside the composed fp32 path)
__device__ __forceinline__ float se_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// Stage the source pixels under the output tile at (ty0, tx0), ns students (2: pa then pb; 1: pa alone), where they fit stage_cap
// floats (every thread of the workgroup calls this: two barriers).  The source index is monotone in the output coordinate, so the
// first row's y0 and the last row's y1 bound every tap of the tile (the same for the columns).  Per source pixel the stage holds
// student 1's Cp channels and then student 2's (Cp = C rounded up to 4, the pad is 0).  Returns whether the tile is staged; fy0, fx0,
// fw: the footprint.
__device__ __forceinline__ bool se_stage_tile(const float* __restrict__ pa, const float* __restrict__ pb, float* st, int tid, int ty0,
                                              int tx0, int C, int h, int w, int H, int W, float sy, float sx, int stage_cap, int& fy0,
                                              int& fx0, int& fw, int ns = 2) {
    const int Cp = (C + 3) & ~3;
    const long hw = (long)h * w;
    int i1, j0;
    float l;
    const int ty1 = ty0 + SE_TH - 1 < H ? ty0 + SE_TH - 1 : H - 1, tx1 = tx0 + SE_TW - 1 < W ? tx0 + SE_TW - 1 : W - 1;
    se_src(ty0, sy, h, fy0, i1, l);
    se_src(ty1, sy, h, j0, i1, l);
    const int fh = i1 - fy0 + 1;
    se_src(tx0, sx, w, fx0, i1, l);
    se_src(tx1, sx, w, j0, i1, l);
    fw = i1 - fx0 + 1;
    const bool staged = (long)fh * fw * ns * Cp <= (long)stage_cap;
    __syncthreads();                           // the previous tile's taps are read
    if (staged) {
        // read in source order (consecutive threads on consecutive columns), written channel-fastest
        const int plane = fh * fw, n = ns * Cp * plane;
        for (int i = tid; i < n; i += SE_THREADS) {
            const int pc = i / plane, rq = i - pc * plane, r = rq / fw, q = rq - r * fw;
            const int sidx = pc >= Cp ? 1 : 0, c = pc - sidx * Cp;
            const float* src = (sidx ? pb : pa) + (long)c * hw;
            st[(rq * ns + sidx) * Cp + c] = c < C ? src[(long)(fy0 + r) * w + fx0 + q] : 0.f;
        }
    }
    __syncthreads();
    return staged;
}

// the floats of stage a launch asks for: an upper bound of a tile's footprint (the kernels check every tile's own footprint against
// it), 0 where that does not fit SE_STAGE or nothing is interpolated
inline int se_stage_floats(int C, int h, int w, int H, int W, int ns = 2) {
    if (h == H && w == W) return 0;
    const double sy = (double)h / H, sx = (double)w / W;
    long fh = (long)((SE_TH - 1) * sy) + 4, fw = (long)((SE_TW - 1) * sx) + 4;
    if (fh > h) fh = h;
    if (fw > w) fw = w;
    const long need = fh * fw * ns * ((C + 3) & ~3);
    return need <= SE_STAGE ? (int)need : 0;
}

}  // namespace
