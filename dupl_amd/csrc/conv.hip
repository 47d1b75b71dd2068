// LargeFOV helpers (conv_head.py:11-41): the 3x3 dilated convolutions run as im2col + the MFMA GEMM.
// Activations stay token-major ([pixel][channel]); the column order is (c, tap) so that the conv weight
// (Cout, Cin, 3, 3) is used in place as the GEMM's k-contiguous B operand.
#include "common.h"
#include "../../include/dupl_hip.h"

namespace {

// x: image b at x + b*img_stride, pixel p at + p*ld, channel c.  col [B*h*w][Cin*9], column = c*9 + tap.
__global__ void im2col_dil3_kernel(const float* __restrict__ x, float* __restrict__ col, int B, int h, int w, int Cin, int dil,
                                   long ld, long img_stride) {
    const long total = (long)B * h * w * Cin;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cin);
        const long r = i / Cin;
        const int px = (int)(r % w), py = (int)((r / w) % h), b = (int)(r / ((long)w * h));
        const float* xb = x + b * img_stride + c;
        float* o = col + r * (long)(Cin * 9) + (long)c * 9;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py + (t / 3 - 1) * dil, xx = px + (t % 3 - 1) * dil;
            o[t] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? xb[(long)(yy * w + xx) * ld] : 0.f;
        }
    }
}

// adjoint: dx[b][p][c] (+)= sum_tap dcol[b][p - off(tap)][c*9 + tap]
__global__ void col2im_dil3_kernel(const float* __restrict__ dcol, float* __restrict__ dx, int B, int h, int w, int Cin, int dil,
                                   long ld, long img_stride, int accumulate, const float* __restrict__ relu_of) {
    const long total = (long)B * h * w * Cin;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cin);
        const long r = i / Cin;
        const int px = (int)(r % w), py = (int)((r / w) % h), b = (int)(r / ((long)w * h));
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            // output pixel q reads input q + off(t); so input p feeds output q = p - off(t)
            const int yy = py - (t / 3 - 1) * dil, xx = px - (t % 3 - 1) * dil;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w)
                s += dcol[((long)b * h * w + (long)yy * w + xx) * (long)(Cin * 9) + (long)c * 9 + t];
        }
        const long off = b * img_stride + (long)(py * w + px) * ld + c;
        if (relu_of && !(relu_of[off] > 0.f)) s = 0.f;   // ReLU backward of the layer that produced x
        float* o = dx + off;
        *o = accumulate ? *o + s : s;
    }
}

// im2col straight into the f16x3 operand planes (format 0) of the split GEMM: no fp32 col exists.  One block = 64 pixel rows x
// 16 channels x 9 taps = a 64 x 144 tile of col, split element-wise as split16 / split_prepare do (split_f32) and parked in LDS
// as (hi | lo << 16), so that the row-major planes [M][9 Cin] and the transposed planes [9 Cin][Mp] (rows M .. Mp-1 zeros)
// both leave in whole 16-byte runs.  Cin % 8 == 0 (a channel tile is then 72 or 144 columns), Mp % 8 == 0.
// 8 elements parked in LDS as (hi | lo << 16) -> one 16-byte run of each plane
__device__ __forceinline__ void unpack8(const unsigned int (&u)[8], uint4& oh, uint4& ol) {
    oh.x = (u[0] & 0xffffu) | (u[1] << 16); oh.y = (u[2] & 0xffffu) | (u[3] << 16);
    oh.z = (u[4] & 0xffffu) | (u[5] << 16); oh.w = (u[6] & 0xffffu) | (u[7] << 16);
    ol.x = (u[0] >> 16) | (u[1] & 0xffff0000u); ol.y = (u[2] >> 16) | (u[3] & 0xffff0000u);
    ol.z = (u[4] >> 16) | (u[5] & 0xffff0000u); ol.w = (u[6] >> 16) | (u[7] & 0xffff0000u);
}

constexpr int I2P_ROWS = 64, I2P_CH = 16, I2P_COLS = I2P_CH * 9, I2P_LD = I2P_COLS + 1;
__global__ __launch_bounds__(256) void im2col_dil3_planes_kernel(const float* __restrict__ x, __half* __restrict__ hi,
                                                                 __half* __restrict__ lo, __half* __restrict__ hiT,
                                                                 __half* __restrict__ loT, int B, int h, int w, int Cin, int dil,
                                                                 long ld, long img_stride, int Mp) {
    __shared__ unsigned int tile[I2P_ROWS][I2P_LD];            // odd stride
    const int tid = threadIdx.x;
    const int M = B * h * w, K9 = Cin * 9;
    const int r0 = blockIdx.y * I2P_ROWS, c0 = blockIdx.x * I2P_CH;
    {
        // thread = (row tid / 4, channels 4 * (tid % 4) .. + 3), all 9 taps: 4 lanes read 64 contiguous bytes of one pixel
        const int r = tid >> 2, cc = (tid & 3) << 2;
        const int row = r0 + r;
        const bool live = row < M && c0 + cc < Cin;             // Cin % 4 == 0
        const int p = live ? row % (h * w) : 0, b = live ? row / (h * w) : 0;
        const int py = p / w, px = p % w;
        const float* xb = x + b * img_stride + c0 + cc;
        float4 v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py + (t / 3 - 1) * dil, xx = px + (t % 3 - 1) * dil;
            v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && yy >= 0 && yy < h && xx >= 0 && xx < w) v[t] = *reinterpret_cast<const float4*>(xb + (long)(yy * w + xx) * ld);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float e[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                __half a, c;
                split_f32(e[j], a, c);
                tile[r][(cc + j) * 9 + t] = (unsigned int)__half_as_ushort(a) | ((unsigned int)__half_as_ushort(c) << 16);
            }
        }
    }
    __syncthreads();
    const int ncol = (Cin - c0 < I2P_CH ? Cin - c0 : I2P_CH) * 9;       // 72 or 144 live columns
    if (hi) {
        // 18 runs of 8 columns per row: consecutive lanes on consecutive runs of one row
        for (int i = tid; i < I2P_ROWS * (I2P_COLS / 8); i += 256) {
            const int r = i / (I2P_COLS / 8), q = (i % (I2P_COLS / 8)) << 3;
            if (r0 + r >= M || q >= ncol) continue;
            unsigned int u[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) u[j] = tile[r][q + j];
            uint4 oh, ol;
            unpack8(u, oh, ol);
            const size_t o = (size_t)(r0 + r) * K9 + (size_t)c0 * 9 + q;
            *reinterpret_cast<uint4*>(hi + o) = oh;
            *reinterpret_cast<uint4*>(lo + o) = ol;
        }
    }
    if (hiT) {
        // 8 runs of 8 rows per column: 8 lanes = one 128-byte run of a transposed row (as split_rt_tile)
        for (int i = tid; i < I2P_COLS * (I2P_ROWS / 8); i += 256) {
            const int col = i >> 3, rr = (i & 7) << 3;
            if (col >= ncol || r0 + rr >= Mp) continue;          // Mp % 8 == 0
            unsigned int u[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) u[j] = tile[rr + j][col];           // rows >= M hold zeros
            uint4 oh, ol;
            unpack8(u, oh, ol);
            const size_t o = (size_t)(c0 * 9 + col) * Mp + r0 + rr;
            *reinterpret_cast<uint4*>(hiT + o) = oh;
            *reinterpret_cast<uint4*>(loT + o) = ol;
        }
    }
}

// Transposed format 0 planes [9 Cin][Rp] of a conv weight w [Cout][ld] (column k = c*9 + tap) with their rows in (tap, c) order:
// row tap*Cin + c holds what split_prep.hip's transposing split writes at row k (same split_f32, zeros in rows Cout .. Rp-1 of
// the transposed image).  64 x 64 tiles through LDS as there; a kernel of its own so that split_rt_tile stays as it is.
__global__ __launch_bounds__(256) void split_wT_tc_kernel(const float* __restrict__ wgt, int ld, int Cout, int Cin,
                                                          __half* __restrict__ hiT, __half* __restrict__ loT, int Rp) {
    __shared__ unsigned int tile[64][65];
    const int tid = threadIdx.x, K9 = Cin * 9;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i;            // 1024 float4 chunks: row c / 16, cols (c % 16) * 4
        const int r = c >> 4, cc = (c & 15) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + r < Cout && c0 + cc < K9) v = *reinterpret_cast<const float4*>(wgt + (size_t)(r0 + r) * ld + c0 + cc);   // K9 % 4 == 0
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __half a, b;
            split_f32(e[j], a, b);
            tile[r][cc + j] = (unsigned int)__half_as_ushort(a) | ((unsigned int)__half_as_ushort(b) << 16);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i;            // 512 runs of 8 rows: column c / 8, rows (c % 8) * 8 .. + 7
        const int col = c >> 3, rr = (c & 7) << 3;
        const int k = c0 + col;
        if (k >= K9 || r0 + rr >= Rp) continue;              // Rp % 8 == 0
        unsigned int u[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = tile[rr + j][col];
        uint4 oh, ol;
        unpack8(u, oh, ol);
        const size_t o = (size_t)((k % 9) * Cin + k / 9) * Rp + r0 + rr;
        *reinterpret_cast<uint4*>(hiT + o) = oh;
        *reinterpret_cast<uint4*>(loT + o) = ol;
    }
}

// col2im on tap-major columns: dcol [B*h*w][9 Cin] with column = tap * Cin + c (the data gradient against W^T planes whose rows
// are in (tap, c) order, dupl_split_wT_tc).  One thread = one pixel x 4 channels: every tap is one float4, consecutive lanes on
// consecutive channels, so each 128-byte line is used whole (col2im_dil3_kernel uses a ninth).  Taps are added in the order
// t = 0 .. 8 with the same out-of-image skips: the sums are bit-equal to col2im_dil3_kernel's.
__global__ void col2im_dil3_tc_kernel(const float* __restrict__ dcol, float* __restrict__ dx, int B, int h, int w, int Cin, int dil,
                                      long ld, long img_stride, int accumulate, const float* __restrict__ relu_of) {
    const int C4 = Cin >> 2;
    const long total = (long)B * h * w * C4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) << 2;
        const long r = i / C4;
        const int px = (int)(r % w), py = (int)((r / w) % h), b = (int)(r / ((long)w * h));
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = py - (t / 3 - 1) * dil, xx = px - (t % 3 - 1) * dil;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                const float4 v = *reinterpret_cast<const float4*>(
                    dcol + ((long)b * h * w + (long)yy * w + xx) * (long)(Cin * 9) + (long)t * Cin + c);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
        const long off = b * img_stride + (long)(py * w + px) * ld + c;
        if (relu_of) {
            const float4 m = *reinterpret_cast<const float4*>(relu_of + off);
            if (!(m.x > 0.f)) s.x = 0.f;
            if (!(m.y > 0.f)) s.y = 0.f;
            if (!(m.z > 0.f)) s.z = 0.f;
            if (!(m.w > 0.f)) s.w = 0.f;
        }
        float4* o = reinterpret_cast<float4*>(dx + off);
        if (accumulate) {
            const float4 a = *o;
            s.x = a.x + s.x; s.y = a.y + s.y; s.z = a.z + s.z; s.w = a.w + s.w;
        }
        *o = s;
    }
}

inline int ew_grid(long n) {
    long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace

extern "C" int dupl_im2col_dil3(const float* x, float* col, int32_t B, int32_t h, int32_t w, int32_t Cin, int32_t dil, int64_t ld,
                                int64_t img_stride, dupl_stream_t s) {
    if (!x || !col || B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || dil <= 0) return DUPL_ERR_ARG;
    DUPL_LAUNCH(im2col_dil3_kernel, dim3(ew_grid((long)B * h * w * Cin)), dim3(256), 0, (hipStream_t)s, x, col, B, h, w,
                       Cin, dil, (long)ld, (long)img_stride);
    return dupl_launch_status();
}

extern "C" int dupl_im2col_dil3_planes(const float* x, void* hi, void* lo, void* hiT, void* loT, int32_t B, int32_t h, int32_t w,
                                       int32_t Cin, int32_t dil, int64_t ld, int64_t img_stride, int32_t Mp, dupl_stream_t s) {
    if (!x || B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || dil <= 0 || (Cin & 7) || ld < Cin || (ld & 3) || (img_stride & 3) ||
        (!hi && !hiT) || ((hi == nullptr) != (lo == nullptr)) || ((hiT == nullptr) != (loT == nullptr)))
        return DUPL_ERR_ARG;
    const long M = (long)B * h * w;
    if (M * Cin * 9 > 0x7fffffffL || (hiT && (Mp < M || (Mp & 7)))) return DUPL_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo) |
         reinterpret_cast<uintptr_t>(hiT) | reinterpret_cast<uintptr_t>(loT)) & 15)
        return DUPL_ERR_ARG;
    const long rows = hiT ? Mp : M;
    const dim3 grid((unsigned)((Cin + I2P_CH - 1) / I2P_CH), (unsigned)((rows + I2P_ROWS - 1) / I2P_ROWS));
    DUPL_LAUNCH(im2col_dil3_planes_kernel, grid, dim3(256), 0, (hipStream_t)s, x, (__half*)hi, (__half*)lo, (__half*)hiT,
                (__half*)loT, B, h, w, Cin, dil, (long)ld, (long)img_stride, Mp);
    return dupl_launch_status();
}

extern "C" int dupl_col2im_dil3_tc(const float* dcol, float* dx, int32_t B, int32_t h, int32_t w, int32_t Cin, int32_t dil,
                                   int64_t ld, int64_t img_stride, int32_t accumulate, const float* relu_of, dupl_stream_t s) {
    if (!dcol || !dx || B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || dil <= 0 || (Cin & 3) || ld < Cin || (ld & 3) || (img_stride & 3))
        return DUPL_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(dcol) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(relu_of)) & 15)
        return DUPL_ERR_ARG;
    DUPL_LAUNCH(col2im_dil3_tc_kernel, dim3(ew_grid((long)B * h * w * (Cin / 4))), dim3(256), 0, (hipStream_t)s, dcol, dx, B, h, w,
                Cin, dil, (long)ld, (long)img_stride, accumulate, relu_of);
    return dupl_launch_status();
}

extern "C" int dupl_split_wT_tc(const float* w, int32_t ld, int32_t Cout, int32_t Cin, void* hiT, void* loT, int32_t Rp,
                                dupl_stream_t stream) {
    if (!w || !hiT || !loT || Cout <= 0 || Cin <= 0 || (Cin & 3) || Cin > 0x7fffffff / 9 || (ld & 3) || ld < Cin * 9 || Rp < Cout ||
        (Rp & 7) || ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(hiT) | reinterpret_cast<uintptr_t>(loT)) & 15))
        return DUPL_ERR_ARG;
    DUPL_LAUNCH(split_wT_tc_kernel, dim3((Cin * 9 + 63) / 64, (Rp + 63) / 64), dim3(256), 0, (hipStream_t)stream, w, ld, Cout, Cin,
                (__half*)hiT, (__half*)loT, Rp);
    return dupl_launch_status();
}

extern "C" int dupl_col2im_dil3(const float* dcol, float* dx, int32_t B, int32_t h, int32_t w, int32_t Cin, int32_t dil, int64_t ld,
                                int64_t img_stride, int32_t accumulate, const float* relu_of, dupl_stream_t s) {
    if (!dcol || !dx || B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || dil <= 0) return DUPL_ERR_ARG;
    DUPL_LAUNCH(col2im_dil3_kernel, dim3(ew_grid((long)B * h * w * Cin)), dim3(256), 0, (hipStream_t)s, dcol, dx, B, h, w,
                       Cin, dil, (long)ld, (long)img_stride, accumulate, relu_of);
    return dupl_launch_status();
}
