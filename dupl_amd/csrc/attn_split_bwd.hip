// Attention backward as fp32-equivalent f16x3 split products (see gemm_split.hip / attn_split.hip), head dim 64.
//
//   S = scale q k^T,  P = exp(S - lse),  dP = dO v^T,  dS = P (dP - delta),  delta_q = sum_d dO O
//   dq = scale dS k,   dk = scale dS^T q,   dv = P^T dO
//
// Operands: q, k, v as the fp16 hi / lo planes the qkv GEMM wrote (saved by the forward); dO as planes scaled by a power of
// two from its own max-abs (split_prep.hip; gradients sit far below fp16's range) -- dP, delta, dS then carry the same
// factor, which the epilogues divide out; P and dS are split in registers.  Two roles in one launch, both in the transposed
// ("lane owns one column") formulation of attn_split.hip, so that the in-register P / dS ARE the B operand of the
// following product (rows of the first products are fed in a permuted order: pi, pi16_row):
//   dq role      (lane = query, 32-key tiles,   v_mfma_f32_32x32x16_f16): S^T = K Q^T, dP^T = V dO^T, dS^T, dq^T += K^T dS^T
//   dk + dv role (lane = key,   32-query tiles, v_mfma_f32_16x16x32_f16): S = Q K^T, dP = dO V^T, P, dS, dv^T += dO^T P, dk^T += Q^T dS
// (Until the 16x16x32 shape dk and dv were two roles of 32 keys per wave, each recomputing S: together their accumulators, the K
// and V fragments and the S / dP tiles exceed the 256 registers of two waves per SIMD.  A wave of the merged role owns 16 keys.)
// The last product of each role contracts over the tile's ROWS (K^T dS^T, dO^T P, Q^T dS): its A operand is the same K / dO / Q rows
// read k-major -- the DMA lays the tile out as 512-byte subtiles and ds_read_b64_tr_b16 gathers the fragments (gemm_split.hip's
// k-major operands; round 4: the three planes_transpose launches per call and their scratch are gone).  The dq role keeps a
// row-major image ([32 rows][128 B], bank swizzle on the source side) next to the k-major one; the merged role reads both kinds of
// fragment from ONE image.  Two stages, one barrier per tile (explicit vmcnt(0) before it on every path).
#include "split_frag.h"
#include "../../include/dupl_hip.h"

namespace {

constexpr int HD = 64, TT = 32;             // rows (keys or queries) per tile
constexpr int PL = 4096;                    // bytes of one tile plane (row-major 32 x 128 B, or k-major: 8 subtiles of 512 B)
constexpr int MAXN = 2048;                  // lse / delta of one (b, h) are kept in LDS by the key-owner kernels

// Row permutation pi, row-major and k-major piece plans, transposing reads, DMA and the packed hi / lo split: split_frag.h
// all 16 fragments halves of one tile: [(sg * 2 + d) * 2 + plane][half]
__device__ __forceinline__ void km_read_tile(const unsigned base_hi, h4 (&f)[8][2]) {
#define KM_RD(SG, DD, PLN, JJ) f[((SG) * 2 + (DD)) * 2 + (PLN)][JJ] = km_tr_read<(PLN) * PL + (((SG) * 2 + (JJ)) * 2 + (DD)) * 512>(base_hi)
    KM_RD(0, 0, 0, 0); KM_RD(0, 0, 0, 1); KM_RD(0, 0, 1, 0); KM_RD(0, 0, 1, 1);
    KM_RD(0, 1, 0, 0); KM_RD(0, 1, 0, 1); KM_RD(0, 1, 1, 0); KM_RD(0, 1, 1, 1);
    KM_RD(1, 0, 0, 0); KM_RD(1, 0, 0, 1); KM_RD(1, 0, 1, 0); KM_RD(1, 0, 1, 1);
    KM_RD(1, 1, 0, 0); KM_RD(1, 1, 0, 1); KM_RD(1, 1, 1, 0); KM_RD(1, 1, 1, 1);
#undef KM_RD
}
// the wait of the consumer: lgkmcnt(0), with every fragment as an in / out operand (split_frag.h, km_tr_read)
__device__ __forceinline__ void km_wait(h4 (&f)[8][2]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f[0][0]), "+v"(f[0][1]), "+v"(f[1][0]), "+v"(f[1][1]), "+v"(f[2][0]), "+v"(f[2][1]), "+v"(f[3][0]), "+v"(f[3][1]),
                   "+v"(f[4][0]), "+v"(f[4][1]), "+v"(f[5][0]), "+v"(f[5][1]), "+v"(f[6][0]), "+v"(f[6][1]), "+v"(f[7][0]), "+v"(f[7][1])
                 :
                 : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ h8 h8of(const h4 lo, const h4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

// hi / lo planes of 16 accumulator values, two at a time
__device__ __forceinline__ void split_regs(const f32x16& v, h8 (&hi)[2], h8 (&lo)[2]) {
#pragma unroll
    for (int e = 0; e < 16; e += 2) split_pair(f32x2{v[e], v[e + 1]}, hi[e >> 3], lo[e >> 3], e & 7);
}

// the last product of a tile, over its k-major fragments f: g^T += X^T w (X = K, dO or Q; w = dS^T, P or dS as planes wh / wl)
__device__ __forceinline__ void last_product(const h4 (&f)[8][2], const h8 (&wh)[2], const h8 (&wl)[2], f32x16 (&gM)[2], f32x16 (&gX)[2]) {
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const h8 th = h8of(f[(sg * 2 + d) * 2][0], f[(sg * 2 + d) * 2][1]);
            const h8 tl = h8of(f[(sg * 2 + d) * 2 + 1][0], f[(sg * 2 + d) * 2 + 1][1]);
            gM[d] = MFMA16(th, wh[sg], gM[d]);
            gX[d] = MFMA16(th, wl[sg], gX[d]);
            gX[d] = MFMA16(tl, wh[sg], gX[d]);
        }
    }
}

// gradient epilogue: (main + cross / 2048) * f -> the 64 floats of this lane's row at op (lane half hf owns 4 of every 8), and
// their running |max|
__device__ __forceinline__ void store_grad(float* op, const f32x16 (&gM)[2], const f32x16 (&gX)[2], const float f, const int hf, float& amx) {
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 v;
            v.x = (gM[d][4 * g + 0] + gX[d][4 * g + 0] * LO_INV) * f;
            v.y = (gM[d][4 * g + 1] + gX[d][4 * g + 1] * LO_INV) * f;
            v.z = (gM[d][4 * g + 2] + gX[d][4 * g + 2] * LO_INV) * f;
            v.w = (gM[d][4 * g + 3] + gX[d][4 * g + 3] * LO_INV) * f;
            amx = fmaxf(fmaxf(amx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            *reinterpret_cast<float4*>(op + d * 32 + 8 * g + 4 * hf) = v;
        }
}

// delta[b][h][q] = sum_d dO[q][d] * O[q][d]   (fp32 operands)
// max |dq| / |dk| / |dv| of a wave -> the amax word of the scale slot the split of dqkv will use (dupl_split_prepare, amax_mode 1):
// one atomic per wave (non-negative floats order like their bits); the waves of the ~340 blocks retire spread over the launch
__device__ __forceinline__ void attn_bwd_amax_flush(unsigned int* amax_out, float amx) {
    if (!amax_out) return;
    amx = wave_max(amx);
    if ((threadIdx.x & 63) == 0 && amx > 0.f) atomicMax(amax_out, __float_as_uint(amx));
}

__global__ __launch_bounds__(256) void delta_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                    float* __restrict__ delta, int B, int N, int H) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)B * N * H;
    if (idx >= total) return;
    const int h = (int)(idx % H);
    const long bn = idx / H;
    const int n = (int)(bn % N), b = (int)(bn / N);
    const float4* o = reinterpret_cast<const float4*>(out + bn * (long)(H * HD) + h * HD);
    const float4* d = reinterpret_cast<const float4*>(dout + bn * (long)(H * HD) + h * HD);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
        const float4 a = o[i], c = d[i];
        s += (a.x * c.x + a.y * c.y) + (a.z * c.z + a.w * c.w);
    }
    delta[((long)b * H + h) * N + n] = s;
}

// ---------------------------------------------------------------------------------------------------- dq
// Stage (24 KB): K_hi | K_lo | V_hi | V_lo (row-major [32 keys][128 B]) | K_hi | K_lo again, k-major
__device__ __forceinline__ void attn_bwd16_dq_body(char* __restrict__ smem, const int bx, const int h, const int b,
                                                   const __half* __restrict__ qkv_hi, const __half* __restrict__ qkv_lo,
                                                   const __half* __restrict__ do_hi, const __half* __restrict__ do_lo,
                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                   const float* __restrict__ slot, float* __restrict__ dqkv, unsigned int* __restrict__ amax_out, int N, int H,
                                                   float scale) {
    constexpr int STAGE = 6 * PL;                              // 2 stages = 48 KB of the block's 64 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hf = lane >> 5;
    const int q0 = bx * 128 + wave * 32;
    const int D = H * HD, ld = 3 * D;
    const int qrow = q0 + l31;
    const bool wave_active = q0 < N, qv = qrow < N;
    const float s_do = slot[0], inv_s = slot[1];

    // B operands held in registers: Q[q][16 s + 8 hf ..] and dO[q][...], both planes
    h8 qh[4], ql[4], oh[4], ol[4];
    {
        const int rr = min(qrow, N - 1);
        const size_t qo = ((size_t)b * N + rr) * ld + h * HD + 8 * hf;
        const size_t oo = ((size_t)b * N + rr) * D + h * HD + 8 * hf;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[s] = load_bfrag(qkv_hi + qo, s);
            ql[s] = load_bfrag(qkv_lo + qo, s);
            oh[s] = load_bfrag(do_hi + oo, s);
            ol[s] = load_bfrag(do_lo + oo, s);
        }
    }
    const float my_lse = qv ? lse[((size_t)b * H + h) * N + qrow] : 0.f;
    const float my_delta = qv ? delta[((size_t)b * H + h) * N + qrow] * s_do : 0.f;

    // DMA plan: wave w fetches piece w of every plane
    const int rrow = 8 * wave + (lane >> 3), rch = rm_piece_col_bytes(lane, rrow);       // row-major pieces (split_frag.h)
    const int trow = km_piece_row(wave, lane), tcb = km_piece_col_bytes(lane);                    // k-major pieces
    const char* k_hi = reinterpret_cast<const char*>(qkv_hi + (size_t)b * N * ld + D + h * HD);
    const char* k_lo = reinterpret_cast<const char*>(qkv_lo + (size_t)b * N * ld + D + h * HD);
    auto issue = [&](int t, int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
        const size_t ro = (size_t)min(t * TT + rrow, N - 1) * (ld * 2) + rch;
        dma16(k_hi + ro, dst);
        dma16(k_lo + ro, dst + PL);
        dma16(k_hi + ro + D * 2, dst + 2 * PL);          // V = K columns + D
        dma16(k_lo + ro + D * 2, dst + 3 * PL);
        const size_t to = (size_t)min(t * TT + trow, N - 1) * (ld * 2) + tcb;      // keys past N meet dS = 0
        dma16(k_hi + to, dst + 4 * PL);
        dma16(k_lo + to, dst + 5 * PL);
    };
    const int prow = pi_row(l31);
    const int a_off = prow * 128, a_sw = (prow >> 1) & 7;             // K / V rows as A operand
    const unsigned km_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + 4 * PL + km_read_lane_off(lane);

    f32x16 dqM[2], dqX[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dqM[d][e] = 0.f; dqX[d][e] = 0.f; }

    const int nkt = (N + TT - 1) / TT;
    issue(0, 0);
    for (int t = 0; t < nkt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nkt) issue(t + 1, (t + 1) & 1);
        if (!wave_active) continue;
        const char* st = smem + (t & 1) * STAGE;
        f32x16 sM, sX, pM, pX;
#pragma unroll
        for (int e = 0; e < 16; ++e) { sM[e] = 0.f; sX[e] = 0.f; pM[e] = 0.f; pX[e] = 0.f; }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ch = ((2 * s + hf) ^ a_sw) * 16;
            const h8 kh = *reinterpret_cast<const h8*>(st + a_off + ch);
            const h8 kl = *reinterpret_cast<const h8*>(st + PL + a_off + ch);
            const h8 vh = *reinterpret_cast<const h8*>(st + 2 * PL + a_off + ch);
            const h8 vl = *reinterpret_cast<const h8*>(st + 3 * PL + a_off + ch);
            sM = MFMA16(kh, qh[s], sM);
            sX = MFMA16(kh, ql[s], sX);
            sX = MFMA16(kl, qh[s], sX);
            pM = MFMA16(vh, oh[s], pM);
            pX = MFMA16(vh, ol[s], pX);
            pX = MFMA16(vl, oh[s], pX);
        }
        // register e <-> key t*32 + 16 (e >> 3) + 8 hf + (e & 7)
        const int kb = t * TT + 8 * hf;
        f32x16 ds;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const bool kvld = kb + 16 * (e >> 3) + (e & 7) < N;
            const float sv = (sM[e] + sX[e] * LO_INV) * scale;
            const float p = kvld ? fast_exp(sv - my_lse) : 0.f;
            ds[e] = __fmul_rn(p, __fsub_rn(pM[e] + pX[e] * LO_INV, my_delta));   // s_do * dS^T[key][q]; un-contracted, see dkv
        }
        // the k-major K fragments of the last product: in flight under the hi / lo split of dS (~100 VALU instructions)
        h4 kf[8][2];
        km_read_tile(km_lds + (t & 1) * STAGE, kf);
        h8 dh[2], dl[2];
        split_regs(ds, dh, dl);
        km_wait(kf);
        last_product(kf, dh, dl, dqM, dqX);
    }
    float amx = 0.f;
    if (wave_active && qv) {
        const float f = scale * inv_s;
        float* op = dqkv + ((size_t)b * N + qrow) * ld + h * HD;
        store_grad(op, dqM, dqX, f, hf, amx);
    }
    attn_bwd_amax_flush(amax_out, amx);
}

// ---------------------------------------------------------------------------------------------------- dk and dv in one pass
// On the 32x32x16 shape (32 keys per lane column) there is no room for dk's and dv's accumulators in one wave: dk and dv were two
// roles, and the dv role recomputed S for nothing.  On v_mfma_f32_16x16x32_f16 a wave owns 16 keys: dk^T and dv^T
// (main + cross, four 16-d tiles each) are 64 registers together, the K and V fragments 32.  Lane (c = lane & 15, g = lane >> 4)
// owns key k0 + c.  Per 32-query tile:
//   S = Q K^T, dP = dO V^T   two 16-query tiles Tj fed in the order pi16_row (split_frag.h): register i of tile j is query
//                            8 g + 4 j + i, so {T0, T1} ARE the B fragment (32 queries) of the products that follow
//   P, dS = P (dP - delta)   as in the dq role
//   dv^T += dO^T P, dk^T += Q^T dS   A = the 16-d tiles of dO^T / Q^T, read transposed
// 12 products for the 15 of the former dk and dv roles, one Q / dO stream instead of two (profiles/attn_bwd_forms.txt: -16 % per
// call at 4 x 785 in one stream, -20 % next to a second stream; the step -0.74 ms).
// ONE image per plane serves both kinds of read.  The k-major image of split_frag.h (km16_*: 512-byte subtiles [16 rows][16 d],
// subtile jj * 4 + dt, subtile row 4 g' + i = tile row 8 g' + 4 jj + i) holds tile row pi16_row(c, j) in subtile row c of the
// subtiles jj = j: the A fragment of S (row c, d = 32 ks + 8 g .. + 7) is the 16 bytes at subtile j * 4 + 2 ks + (g >> 1), row c,
// half g & 1 -- one ds_read_b128 whose four 16-lane groups ({0-3, 12-15, 20-27}, ...) each cover all 64 banks once: rows c and
// c + 8 of one subtile share banks, and every group takes its c < 8 and its c >= 8 lanes from different halves (g & 1).
// Stage (16 KB) = Q_hi | Q_lo | dO_hi | dO_lo, 4 DMA pieces per wave and tile; 2 stages + 16 KB of lse / delta = 48 KB.
constexpr int KVK = 64;                       // keys per block of the merged role (4 waves x 16)

__device__ __forceinline__ void km16_wait8(h4 (&f)[8], const bool last) {
    // lgkmcnt(8): LDS returns in order, so the 8 reads issued before the 8 newest have landed; the fragments are in / out operands
    // (km_wait above)
    if (last)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]) : : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void attn_bwd16_kv_body(char* __restrict__ smem, const int bx, const int h, const int b,
                                                   const __half* __restrict__ qkv_hi, const __half* __restrict__ qkv_lo,
                                                   const __half* __restrict__ do_hi, const __half* __restrict__ do_lo,
                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                   const float* __restrict__ slot, float* __restrict__ dqkv, unsigned int* __restrict__ amax_out, int N, int H,
                                                   float scale) {
    constexpr int STAGE = 4 * PL;                             // 2 stages = 32 KB, then the lse / delta table
    float* Ls = reinterpret_cast<float*>(smem + 2 * STAGE);
    float* Ds = Ls + MAXN;
    const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k0 = bx * KVK + wave * 16;
    const int D = H * HD, ld = 3 * D;
    const int krow = k0 + c16;
    const bool wave_active = k0 < N, kv = krow < N;
    const float s_do = slot[0], inv_s = slot[1];
    const int nqt = (N + TT - 1) / TT;

    // lse and s_do * delta of this (b, h) into LDS; the entries of the last tile's queries past N are zeros (they meet P = 0)
    for (int i = tid; i < nqt * TT; i += 256) {
        Ls[i] = i < N ? lse[((size_t)b * H + h) * N + i] : 0.f;
        Ds[i] = i < N ? delta[((size_t)b * H + h) * N + i] * s_do : 0.f;
    }

    // B operands held in registers: K[key][32 ks + 8 g ..] and V[key][...], both planes
    h8 kh[2], kl[2], vh[2], vl[2];
    {
        const size_t ko = ((size_t)b * N + min(krow, N - 1)) * ld + D + h * HD + 8 * g4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kh[ks] = load_bfrag(qkv_hi + ko, 2 * ks);
            kl[ks] = load_bfrag(qkv_lo + ko, 2 * ks);
            vh[ks] = load_bfrag(qkv_hi + ko + D, 2 * ks);
            vl[ks] = load_bfrag(qkv_lo + ko + D, 2 * ks);
        }
    }

    // DMA plan: wave w fetches piece w (subtiles 2 w, 2 w + 1) of every plane
    const int trow = km16_piece_row(wave, lane), tcb = km16_piece_col_bytes(wave, lane);
    const char* q_hi = reinterpret_cast<const char*>(qkv_hi + (size_t)b * N * ld + h * HD);
    const char* q_lo = reinterpret_cast<const char*>(qkv_lo + (size_t)b * N * ld + h * HD);
    const char* o_hi = reinterpret_cast<const char*>(do_hi + (size_t)b * N * D + h * HD);
    const char* o_lo = reinterpret_cast<const char*>(do_lo + (size_t)b * N * D + h * HD);
    auto issue = [&](int t, int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
        const int tr = min(t * TT + trow, N - 1);            // queries past N meet P = dS = 0
        dma16(q_hi + (size_t)tr * (ld * 2) + tcb, dst);
        dma16(q_lo + (size_t)tr * (ld * 2) + tcb, dst + PL);
        dma16(o_hi + (size_t)tr * (D * 2) + tcb, dst + 2 * PL);
        dma16(o_lo + (size_t)tr * (D * 2) + tcb, dst + 3 * PL);
    };
    const int a_off = (g4 >> 1) * 512 + c16 * 32 + (g4 & 1) * 16;          // row reads: + plane, + j * 2048 + ks * 1024
    const unsigned km_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + km16_read_lane_off(lane);

    f32x4 dkM[4], dkX[4], dvM[4], dvX[4];                   // [d tile]: d = 16 dt + 4 g .. + 3 of key k0 + c
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d) { dkM[d] = zero4; dkX[d] = zero4; dvM[d] = zero4; dvX[d] = zero4; }

    issue(0, 0);
    for (int t = 0; t < nqt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                     // also publishes Ls / Ds on the first pass
        if (t + 1 < nqt) issue(t + 1, (t + 1) & 1);
        if (!wave_active) continue;
        const char* st = smem + (t & 1) * STAGE + a_off;
        // lse / delta of the lane's 8 queries t * 32 + 8 g + 0..7 (element 4 j + i)
        const f32x4 l0 = *reinterpret_cast<const f32x4*>(Ls + t * TT + 8 * g4), l1 = *reinterpret_cast<const f32x4*>(Ls + t * TT + 8 * g4 + 4);
        const f32x4 e0 = *reinterpret_cast<const f32x4*>(Ds + t * TT + 8 * g4), e1 = *reinterpret_cast<const f32x4*>(Ds + t * TT + 8 * g4 + 4);

        // ---- S = Q K^T and dP = dO V^T in two k steps; the fragment reads of step 1 are issued before the MFMAs of step 0
        f32x4 sM[2], sX[2], pM[2], pX[2];                   // [j]
        h8 af[2][4][2];                                      // [set][plane: Q_hi, Q_lo, dO_hi, dO_lo][j]
        auto a_read = [&](const int ks, h8(&f)[4][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int pn = 0; pn < 4; ++pn)
#pragma unroll
                for (int j = 0; j < 2; ++j) f[pn][j] = *reinterpret_cast<const h8*>(st + pn * PL + j * 2048 + ks * 1024);
        };
        a_read(0, af[0]);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (ks == 0) a_read(1, af[1]);
            __builtin_amdgcn_sched_barrier(0);
            const h8(&f)[4][2] = af[ks];
#pragma unroll
            for (int j = 0; j < 2; ++j) sM[j] = MFMA_16x16x32(f[0][j], kh[ks], ks == 0 ? zero4 : sM[j]);
#pragma unroll
            for (int j = 0; j < 2; ++j) pM[j] = MFMA_16x16x32(f[2][j], vh[ks], ks == 0 ? zero4 : pM[j]);
#pragma unroll
            for (int j = 0; j < 2; ++j) sX[j] = MFMA_16x16x32(f[0][j], kl[ks], ks == 0 ? zero4 : sX[j]);
#pragma unroll
            for (int j = 0; j < 2; ++j) pX[j] = MFMA_16x16x32(f[2][j], vl[ks], ks == 0 ? zero4 : pX[j]);
#pragma unroll
            for (int j = 0; j < 2; ++j) sX[j] = MFMA_16x16x32(f[1][j], kh[ks], sX[j]);
#pragma unroll
            for (int j = 0; j < 2; ++j) pX[j] = MFMA_16x16x32(f[3][j], vh[ks], pX[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the transposed fragments of d tile 0: in flight under the P / dS arithmetic
        const unsigned km_st = km_lds + (t & 1) * STAGE;
        h4 xf[2][8];                                         // [set][(plane * 2 + half jj)]
        auto x_read = [&](auto dc, h4(&f)[8]) __attribute__((always_inline)) {
            constexpr int DT = decltype(dc)::value;
            static_for<8>([&](auto ic) __attribute__((always_inline)) {
                constexpr int i = decltype(ic)::value, pl = i >> 1, jj = i & 1;
                f[i] = km_tr_read<pl * PL + (jj * 4 + DT) * 512>(km_st);
            });
        };
        x_read(std::integral_constant<int, 0>{}, xf[0]);
        // ---- P and dS of the lane's 8 queries
        h8 ph, pl, dh, dl;
        const int qb = t * TT + 8 * g4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 lj = j ? l1 : l0, ej = j ? e1 : e0;
            float pv[4], dv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = qb + 4 * j + i < N && kv;
                const float sv = (sM[j][i] + sX[j][i] * LO_INV) * scale;
                pv[i] = ok ? fast_exp(sv - lj[i]) : 0.f;
                // dS = P (dP - delta): the difference first, then the product (never fma(p, dP, -(p * delta)))
                dv[i] = __fmul_rn(pv[i], __fsub_rn(pM[j][i] + pX[j][i] * LO_INV, ej[i]));
            }
#pragma unroll
            for (int i = 0; i < 4; i += 2) {
                split_pair(f32x2{pv[i], pv[i + 1]}, ph, pl, 4 * j + i);
                split_pair(f32x2{dv[i], dv[i + 1]}, dh, dl, 4 * j + i);
            }
        }
        // ---- dv^T += dO^T P, dk^T += Q^T dS, one d tile per step, the reads one step ahead
        static_for<4>([&](auto dc) __attribute__((always_inline)) {
            constexpr int dt = decltype(dc)::value, cur = dt & 1;
            if constexpr (dt + 1 < 4) x_read(std::integral_constant<int, dt + 1>{}, xf[cur ^ 1]);
            km16_wait8(xf[cur], dt == 3);
            const h4(&f)[8] = xf[cur];
            const h8 qh = h8of(f[0], f[1]), ql = h8of(f[2], f[3]), oh = h8of(f[4], f[5]), ol = h8of(f[6], f[7]);
            dvX[dt] = MFMA_16x16x32(oh, pl, dvX[dt]);
            dkX[dt] = MFMA_16x16x32(qh, dl, dkX[dt]);
            dvM[dt] = MFMA_16x16x32(oh, ph, dvM[dt]);
            dkM[dt] = MFMA_16x16x32(qh, dh, dkM[dt]);
            dvX[dt] = MFMA_16x16x32(ol, ph, dvX[dt]);
            dkX[dt] = MFMA_16x16x32(ql, dh, dkX[dt]);
            __builtin_amdgcn_sched_barrier(0);
        });
    }
    float amx = 0.f;
    if (wave_active && kv) {
        // gradient epilogue of store_grad, (main + cross / 2048) * f: the lane's 4 floats of every d tile
        float* gp = dqkv + ((size_t)b * N + krow) * ld + D + h * HD + 4 * g4;
        const float fk = scale * inv_s, fv = inv_s;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            float4 a, c;
            a.x = (dkM[dt][0] + dkX[dt][0] * LO_INV) * fk; a.y = (dkM[dt][1] + dkX[dt][1] * LO_INV) * fk;
            a.z = (dkM[dt][2] + dkX[dt][2] * LO_INV) * fk; a.w = (dkM[dt][3] + dkX[dt][3] * LO_INV) * fk;
            c.x = (dvM[dt][0] + dvX[dt][0] * LO_INV) * fv; c.y = (dvM[dt][1] + dvX[dt][1] * LO_INV) * fv;
            c.z = (dvM[dt][2] + dvX[dt][2] * LO_INV) * fv; c.w = (dvM[dt][3] + dvX[dt][3] * LO_INV) * fv;
            amx = fmaxf(fmaxf(amx, fmaxf(fabsf(a.x), fabsf(a.y))), fmaxf(fabsf(a.z), fabsf(a.w)));
            amx = fmaxf(fmaxf(amx, fmaxf(fabsf(c.x), fabsf(c.y))), fmaxf(fabsf(c.z), fabsf(c.w)));
            *reinterpret_cast<float4*>(gp + 16 * dt) = a;
            *reinterpret_cast<float4*>(gp + D + 16 * dt) = c;
        }
    }
    attn_bwd_amax_flush(amax_out, amx);
}

// ---------------------------------------------------------------------------------------------------- one launch for both roles
// The roles are independent given the dO planes, and each alone leaves the chip's 512 block slots (two 256-thread blocks per CU)
// partly empty with a tail of its own (round 5).  As ONE launch -- the role is the leading index, the merged role first: its blocks
// run longest -- the blocks of the dq role fill the tail.  ceil(N / 64) + ceil(N / 128) blocks per (image, head): 960 at 4 x 785
// tokens, 12 heads (13 + 7 per head).  Same code per block as a launch per role, same results bit for bit.
constexpr int ATTNB2_LDS = 2 * 6 * PL;                      // the dq role's 48 KB = the merged role's 32 KB + 16 KB table
static_assert(2 * 4 * PL + 2 * MAXN * 4 <= ATTNB2_LDS, "the merged role's stages and table");
__global__ __launch_bounds__(256, 2) void attn_bwd16_kvq_kernel(const __half* __restrict__ qkv_hi, const __half* __restrict__ qkv_lo,
                                                                const __half* __restrict__ do_hi, const __half* __restrict__ do_lo,
                                                                const float* __restrict__ lse, const float* __restrict__ delta,
                                                                const float* __restrict__ slot, float* __restrict__ dqkv,
                                                                unsigned int* __restrict__ amax_out, int N, int H, int B, float scale,
                                                                int remap) {
    __shared__ __attribute__((aligned(1024))) char smem[ATTNB2_LDS];
    const int gk = (N + KVK - 1) / KVK, gx = (N + 127) / 128;
    const int Gk = gk * H * B;
    const int role = __builtin_amdgcn_readfirstlane((int)blockIdx.x >= Gk ? 1 : 0);     // 0: dk + dv, 1: dq
    const int g = role ? gx : gk, G = g * H * B;
    const int L = (int)blockIdx.x - role * Gk;
    const int w = remap ? xcd_band(L, G) : L;      // whole heads per XCD inside each role
    const int bx = w % g, h = (w / g) % H, b = w / (g * H);
    if (role == 0) attn_bwd16_kv_body(smem, bx, h, b, qkv_hi, qkv_lo, do_hi, do_lo, lse, delta, slot, dqkv, amax_out, N, H, scale);
    else attn_bwd16_dq_body(smem, bx, h, b, qkv_hi, qkv_lo, do_hi, do_lo, lse, delta, slot, dqkv, amax_out, N, H, scale);
}

}  // namespace

constexpr int g_attnb16_remap = 1;     // XCD-aware workgroup order

extern "C" int dupl_attention_bwd16(const void* qkv_hi, const void* qkv_lo, const float* out, const float* dout, const void* do_hi,
                                    const void* do_lo, const float* do_slot, const float* lse, float* delta, float* dqkv, int32_t B,
                                    int32_t N, int32_t H, int32_t hd, float scale, void* amax_out, dupl_stream_t stream) {
    unsigned int* ax = static_cast<unsigned int*>(amax_out);
    if (!qkv_hi || !qkv_lo || !out || !dout || !do_hi || !do_lo || !do_slot || !lse || !delta || !dqkv || B <= 0 || N <= 0 ||
        N > MAXN || H <= 0 || hd != HD)
        return DUPL_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const long total = (long)B * N * H;
    DUPL_LAUNCH(delta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out, dout, delta, B, N, H);
    const unsigned blocks = (unsigned)((((N + KVK - 1) / KVK) + ((N + 127) / 128)) * H * B);
    DUPL_LAUNCH(attn_bwd16_kvq_kernel, dim3(blocks), dim3(256), 0, s, (const __half*)qkv_hi, (const __half*)qkv_lo,
                       (const __half*)do_hi, (const __half*)do_lo, lse, delta, do_slot, dqkv, ax, N, H, B, scale, g_attnb16_remap);
    return dupl_launch_status();
}
