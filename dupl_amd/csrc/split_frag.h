// Fragment, DMA and block-order helpers shared by the f16x3 ("split") kernels: attn_split.hip, attn_split_bwd.hip, gemm_split.hip,
// and the band remap / fast_exp of attn.hip.  Each layout rule lives here once, with its one explanation.
#pragma once
#include "common.h"
#include <type_traits>

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr float LO_INV = 1.f / DUPL_LO_SCALE;

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
#define MFMA_16x16x32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// exp for the softmax: one v_exp_f32 on x*log2(e) instead of libm expf's ~18-instruction sequence.  Arguments are
// (score - running max) in [-inf, 0]; the result's relative error is ~1e-6 (|x| * 2^-24 from the scaled argument +
// 1 ulp of v_exp_f32), the same class as the fp32 round-off of the surrounding sums (tests: 5e-6 vs fp64).
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// ---- XCD band remap.  Workgroups are dealt round-robin to the 8 XCDs in linear order, so the ceil(N/128) blocks that share one
// head's K / V would each pull them into a different XCD's L2.  Same bijective band remap as the GEMM: XCD x owns a contiguous run
// of (query-block, head, image) work items, i.e. whole heads.  xcd_band: linear block index L of a grid of G blocks -> work item.
__device__ __forceinline__ int xcd_band(const int L, const int G) {
    const int q = G >> 3, r = G & 7;
    const int xcd = L & 7, idx = L >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// the same on a 3-D grid: (bx, by, bz) = the work item of this block
__device__ __forceinline__ void xcd_remap3(int remap, int& bx, int& by, int& bz) {
    bx = blockIdx.x; by = blockIdx.y; bz = blockIdx.z;
    if (!remap) return;
    const int gx = gridDim.x, gy = gridDim.y;
    const int total = gx * gy * gridDim.z;
    const int L = bx + gx * (by + gy * bz);
    const int w = xcd_band(L, total);
    bx = w % gx;
    by = (w / gx) % gy;
    bz = w / (gx * gy);
}

// 16 bytes per lane, global -> LDS by direct-to-LDS DMA: the LDS side is lane-linear (dst = the wave's piece, uniform), so every
// layout rule below is applied on the source side
__device__ __forceinline__ void dma16(const char* src, char* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// ---- row-major tile planes [rows][64 halfs = 128 B].  DMA piece w (1 KB) = rows 8 w .. 8 w + 7: lane -> row = 8 w + (lane >> 3),
// physical 16-byte chunk lane & 7, which holds source chunk (lane & 7) ^ ((row >> 1) & 7) (bank swizzle; a fragment read is one
// ds_read_b128).  The row stays written out at its three call sites: as a helper it changes the code of both attention kernels.
__device__ __forceinline__ int rm_piece_col_bytes(int lane, int row) { return ((lane & 7) ^ ((row >> 1) & 7)) * 16; }

// The same planes for the A operand of v_mfma_f32_16x16x32_f16 fed in the order pi16 (below): the 16 lanes of one k group read
// rows 8 (c >> 2) + 4 j + (c & 3) (c = lane & 15) at source chunk 4 kstep + (lane >> 4).  Rows 16 apart share (row >> 1) & 7, so
// the swizzle above is 2-way there; this one takes row bits 1, 3 and 4 -- the three bits of c besides row & 1 that vary in a read
// -- and is conflict-free in the four 16-lane groups of ds_read_b128 ({0-3, 12-15, 20-27}, ...: a group mixes two k groups g,
// g ^ 1 by (c >> 2) in {1, 2}, which XORs bit 0 of the chunk with c2 ^ c3 -- still one-to-one in (c1, c2, c3)).
__device__ __forceinline__ int rm16_swizzle(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }
__device__ __forceinline__ int rm16_piece_col_bytes(int lane, int row) { return ((lane & 7) ^ rm16_swizzle(row)) * 16; }

// MFMA row i <- tile row pi(i): 4-row groups 1 and 2 of every 16 swapped, so that the accumulator registers 8 s .. 8 s + 7 of a lane
// are tile rows 16 s + 8 hf + 0..7 -- the B fragment of the next product, without any permute (attn_split.hip's formulation)
__device__ __forceinline__ int pi_row(int r) {
    const int g = (r >> 2) & 3;
    return (r & ~12) | ((g == 1 ? 2 : (g == 2 ? 1 : g)) << 2);
}

// The same idea for a chain of two 16x16x32 products (attn_fwd16_m16_kernel).  Lane (c = lane & 15, g = lane >> 4) holds rows
// 4 g .. 4 g + 3 of column c of a 16 x 16 result and needs k = 8 g .. 8 g + 7 of column c as the next B operand.  A 32-row group is
// computed as two 16-row tiles T0, T1, and MFMA row r of tile Tj is fed with row pi16(r, j) = 8 (r >> 2) + 4 j + (r & 3) of the
// group: the lane then holds rows 8 g .. 8 g + 3 in T0 and 8 g + 4 .. 8 g + 7 in T1 -- the fragment, without any permute.
__device__ __forceinline__ int pi16_row(int r, int j) { return 8 * (r >> 2) + 4 * j + (r & 3); }

// B-operand fragment s (of 4) of a row held in registers: lane half hf holds halfs 16 s + 8 hf .. + 7; p points at the row's half
// 8 hf.  (One step at a time: a helper that loads the 4 steps of a plane reorders the callers' interleaved global loads.)
__device__ __forceinline__ h8 load_bfrag(const __half* p, int s) { return *reinterpret_cast<const h8*>(p + 16 * s); }

// ---- k-major operands (the contraction index is the slow one in memory; the A operand is read transposed).  The image of a [32
// rows][64 d] tile plane is 512-byte subtiles: subtile (2 sg + jj) * 2 + dblk = [8 rows][32 d] halfs, holding rows 16 sg + 4 jj +
// {0..3, 8..11} -- what one ds_read_b64_tr_b16 of row step sg, half jj gathers, so every instruction reads one contiguous subtile
// (conflict-free).  DMA piece w (1 KB, wave w) = row group w, both d blocks: lane -> subtile row (lane >> 2) & 7, 16-byte chunk
// lane & 3 of d block lane >> 5.
__device__ __forceinline__ int km_piece_row(int wave, int lane) {
    const int srow = (lane >> 2) & 7;
    return (wave >> 1) * 16 + (srow >> 2) * 8 + (wave & 1) * 4 + (srow & 3);
}
__device__ __forceinline__ int km_piece_col_bytes(int lane) { return ((lane >> 5) * 32 + (lane & 3) * 8) * 2; }
// per-lane byte offset of the transposing reads inside a plane image (lane (g = lane >> 4, q = lane & 15): subtile row
// (g >> 1) * 4 + (q >> 2), d 16 (g & 1) + 4 (q & 3) .. + 3); the subtile is an immediate offset of the read
__device__ __forceinline__ int km_read_lane_off(int lane) {
    const int g = lane >> 4, q = lane & 15;
    return ((g >> 1) * 4 + (q >> 2)) * 64 + (16 * (g & 1) + 4 * (q & 3)) * 2;
}
// ---- the same for the 16x16x32 MFMA (A = [16 d][32 rows]: lane (d, g) needs rows 8 g .. 8 g + 7).  The image of a [64 rows][64 d]
// tile plane is 16 subtiles of 512 bytes: subtile ((S * 2 + jj) * 4 + dt) = [16 rows][16 d] halfs, subtile row 4 g + i holding row
// 32 S + 8 g + 4 jj + i, d 16 dt .. + 15 -- what one ds_read_b64_tr_b16 of row step S, half jj, d tile dt gathers, at lane * 8 bytes
// (contiguous: conflict-free).  DMA piece p (1 KB, 8 per plane) = subtiles 2 p, 2 p + 1: lane -> subtile lane >> 5, subtile row
// (lane >> 1) & 15, 16-byte half lane & 1 of the row's 32 bytes.
__device__ __forceinline__ int km16_piece_row(int p, int lane) {
    const int sr = (lane >> 1) & 15;
    return (p >> 2) * 32 + (sr >> 2) * 8 + ((p >> 1) & 1) * 4 + (sr & 3);
}
__device__ __forceinline__ int km16_piece_col_bytes(int p, int lane) { return (16 * (2 * (p & 1) + (lane >> 5)) + 8 * (lane & 1)) * 2; }
__device__ __forceinline__ int km16_read_lane_off(int lane) { return lane * 8; }
// The transposing reads are INLINE ASM: behind a direct-to-LDS DMA hipcc puts `s_waitcnt vmcnt(0)` in front of every
// ds_read_b64_tr_b16 it issues itself (the builtin carries no alias information, so every LDS-DMA in flight "may" feed it) -- that
// drains the prefetch of the next tiles once per read (gemm_split.hip's ring: 87 instead of 165 TF/s-eq).  The kernels' own
// protocols (vmcnt + barrier before a stage is read) already order them; what the compiler no longer does for these reads is wait
// for their RESULTS, so every consumer waits lgkmcnt itself (LDS operations return in order).  Such a wait must carry the
// fragments as in / out operands where nothing else pins the consumers: an MFMA is no memory operation, a "memory" clobber alone
// does not hold it back (attn_split_bwd.hip's km_wait).
template <int OFF>
__device__ __forceinline__ h4 km_tr_read(const unsigned addr) {
    h4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}

// hi / lo planes of a pair of fp32 values into elements i, i + 1 of a fragment pair: one packed convert (v_cvt_pk_f16_f32, round to
// nearest even), one packed multiply, one mixed-precision FMA per element -- lo = f16(fma(f32(hi), -2048, 2048 x)) is the same value
// as f16((x - hi) * 2048) (every step before the final rounding is exact), and hi is read back from the register that becomes the
// operand, so the two planes cannot disagree (cf. split_f32)
__device__ __forceinline__ void split_pair(const f32x2 x2, h8& hi, h8& lo, const int i) {
    const h2v hh = __builtin_convertvector(x2, h2v);
    const f32x2 q2 = x2 * f32x2{DUPL_LO_SCALE, DUPL_LO_SCALE};
    hi[i] = hh[0];
    hi[i + 1] = hh[1];
    lo[i] = (_Float16)__builtin_fmaf((float)hh[0], -DUPL_LO_SCALE, q2[0]);
    lo[i + 1] = (_Float16)__builtin_fmaf((float)hh[1], -DUPL_LO_SCALE, q2[1]);
}

}  // namespace
