// Fused multi-head attention forward as fp32-equivalent split products on the f16 matrix cores ("f16x3", see
// gemm_split.hip): q, k, v arrive as fp16 hi / lo planes (the qkv GEMM writes them), S = q k^T and O = P v are each
//     hi hi + (hi lo + lo hi) / 2048       (3 v_mfma_f32_32x32x16_f16 per 32x32x16 block, fp32 accumulate)
// with the softmax in fp32 and the probabilities split in registers.  Head dim 64.
//
// Transposed formulation (as attn.hip): S^T[key][q] = K Q^T puts one query per lane column, so the row softmax is
// lane-local (+ one lane^32 exchange) and the probability registers ARE the B operand of O^T[d][q] += V^T[d][key] P^T[key][q].
// For the f16 MFMA a lane's B fragment is 8 consecutive reduction slots; the accumulator gives lane half hf the MFMA rows
// {0-3, 8-11} / {4-7, 12-15} of each 16-row group, so the K rows are fed in the permuted order pi (4-row groups 1 and 2
// swapped): then registers e = 8s .. 8s+7 of a lane ARE keys 16s + 8 hf + 0..7 -- the fragment, without any permute.
// K tiles are [64 keys][64 halfs = 128 bytes] images filled by direct-to-LDS DMA (8 rows per wave instruction) with the bank
// swizzle chunk ^ ((row >> 1) & 7) applied on the source side; a fragment read is one ds_read_b128.  V is the k-major operand
// of the second product (A = V^T [d][key], memory holds [key][d]): its DMA lays the tile out as 512-byte subtiles
// [8 keys][32 d] (the layout of gemm_split.hip's k-major operands) and ds_read_b64_tr_b16 gathers the fragments, so no
// transposed copy of V is ever written (rounds 2-3 ran a vt_planes kernel per call: 0.7 ms / step).
// Block = 4 waves x 32 queries, 64 keys per iteration, two LDS stages (64 KB, 2 blocks / CU), one barrier per key tile.
//
// Two bodies compute this, selected per launch (dupl_attention_fwd16_mfma; the rule is at the launcher):
//   attn_fwd16_kernel      v_mfma_f32_32x32x16_f16, as described above: 48 MFMAs of 32 cycles per key tile and wave.
//   attn_fwd16_m16_kernel  v_mfma_f32_16x16x32_f16: 96 MFMAs of 16 cycles, the same accumulator registers (S 2 x 32, O 2 x 32).  Lane
//       (c = lane & 15, g = lane >> 4) holds rows 4 g .. 4 g + 3 of a 16 x 16 result and k = 8 g .. 8 g + 7 of an operand, so a wave's
//       32 queries are two 16-query column tiles, a 32-key group is two 16-key S^T tiles fed in the order pi16_row (split_frag.h)
//       -- together the P^T fragment of that key step -- the K image carries the swizzle rm16_swizzle (this read's four 16-lane
//       groups), and V lies in [16 keys][16 d] subtiles (km16_*: one ds_read_b64_tr_b16 per subtile, lane * 8 bytes).  A query's keys
//       sit in four lanes: the lazy maximum is decided on per-lane partial maxima and the lanes are combined only when it moves
//       and, for the row sum, once in the epilogue -- the common path of a key tile has no cross-lane operation (the 32x32x16 body
//       has one permlane32_swap).  Same DMA protocol, segments, remap, outputs and f16x3 arithmetic; the sums differ from the
//       32x32x16 body's in the last bits (accumulation order).  Why: under this loop the chip holds its clock down, and at equal
//       MFMA cycles the 16x16x32 shape draws less (profiles/mfma16_attn.txt: -10 % per launch at 8 x 1765).
//       A template on the product count: <3> is the above, <1> the single-product form (products = 1; described at the kernel).
#include "split_frag.h"
#include "../../include/dupl_hip.h"

#ifndef ATT_PRIO
#define ATT_PRIO 0   // s_setprio around the MFMA clusters: measured null (316.3 vs 316.7 us at 8 x 1765), kept as a build knob
#endif
#ifndef ATT_ABL
#define ATT_ABL 0   // ablation builds only (tools/attn16_bench): 16 = per-phase s_memtime sums of wave 0 into the lse buffer
#endif

namespace {

constexpr int HD = 64, KT = 64;
constexpr int PLANE = KT * 128;          // one [64][128 B] image
constexpr int STAGE = 4 * PLANE;         // K_hi | K_lo | V_hi | V_lo

// Several batches of one token buffer in ONE launch (round 5).  The ms-CAM pass of a step holds three batches of different length
// (8 x 785, 8 x 197, 8 x 1 765 tokens at 448^2, 4 images); a launch per batch is 672 / 192 / 1 344 blocks for the chip's 512 block
// slots -- 1.3, 0.4 and 2.6 rounds, each with its own tail.  As one grid, longest batch first, the 2 208 blocks run back to back and
// the short ones fill the tails.  Segment = the batch's first token row in the planes, image count, tokens per image, its fp32
// output / lse (NULL: planes only) and the block index its blocks start at.
struct AttnSegs {
    int n;
    int row0[DUPL_ATTN_SEGS_MAX], B[DUPL_ATTN_SEGS_MAX], N[DUPL_ATTN_SEGS_MAX], B_f32[DUPL_ATTN_SEGS_MAX], first[DUPL_ATTN_SEGS_MAX + 1];
    float* out[DUPL_ATTN_SEGS_MAX];
    float* lse[DUPL_ATTN_SEGS_MAX];
};

// ---- shared by the forward kernels
// The planes of a launch, moved to the segment's first token row r0 (a plane the kernel never reads may be passed as NULL).
template <class In, class Out>      // (the kernels' __restrict__ pointers)
__device__ __forceinline__ void attn_seg_planes(const size_t r0, const int H, In& qkv_hi, In& qkv_lo, Out& out_hi, Out& out_lo) {
    qkv_hi += r0 * (size_t)(3 * H * HD);
    qkv_lo += r0 * (size_t)(3 * H * HD);
    if (out_hi) { out_hi += r0 * (size_t)(H * HD); out_lo += r0 * (size_t)(H * HD); }
}

__global__ __launch_bounds__(256, 2) void attn_fwd16_kernel(const __half* __restrict__ qkv_hi, const __half* __restrict__ qkv_lo,
                                                            __half* __restrict__ out_hi, __half* __restrict__ out_lo,
                                                            const AttnSegs segs, int H, float scale, int remap, float out_scale) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);            // scalar: the LDS destination of a DMA piece goes through M0
    int sg = 0;
#pragma unroll 1
    while (sg + 1 < segs.n && (int)blockIdx.x >= segs.first[sg + 1]) ++sg;
    sg = __builtin_amdgcn_readfirstlane(sg);
    const int N = segs.N[sg], B_f32 = segs.B_f32[sg];
    float* __restrict__ out = segs.out[sg];
    float* __restrict__ lse = segs.lse[sg];
    int bx, h, b;
    {
        const int gx = (N + 127) / 128;
        const int G = gx * H * segs.B[sg];
        const int L = (int)blockIdx.x - segs.first[sg];
        const int w = remap ? xcd_band(L, G) : L;      // whole heads per XCD inside the segment
        bx = w % gx; h = (w / gx) % H; b = w / (gx * H);
    }
    attn_seg_planes((size_t)segs.row0[sg], H, qkv_hi, qkv_lo, out_hi, out_lo);
    const int q0 = bx * 128 + wave * 32;
    const int D = H * HD, ld = 3 * D;
    const int qrow = q0 + l31;
    const bool wave_active = q0 < N;

    // ---- Q fragments (B operand of S^T = K Q^T): lane (q, hf) holds Q[q][16 s + 8 hf .. + 7], both planes
    h8 qh[4], ql[4];
    {
        const size_t off = ((size_t)b * N + min(qrow, N - 1)) * ld + h * HD + 8 * hf;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[s] = load_bfrag(qkv_hi + off, s);
            ql[s] = load_bfrag(qkv_lo + off, s);
        }
    }

    // ---- DMA plan: piece g = wave + 4 i covers rows 8 q .. 8 q + 7 (q = wave + 4 (i & 1)) of plane i / 2
    const int prow = lane >> 3;
    const char* kbase[2];      // K planes at this (b, h): row 0, column chunk 0
    kbase[0] = reinterpret_cast<const char*>(qkv_hi + (size_t)b * N * ld + D + h * HD);
    kbase[1] = reinterpret_cast<const char*>(qkv_lo + (size_t)b * N * ld + D + h * HD);
    const char* vbase[2];      // V planes at this (b, h)
    vbase[0] = kbase[0] + D * 2;
    vbase[1] = kbase[1] + D * 2;
    int krow[2], kch[2], vrow[2];
    const int vch = km_piece_col_bytes(lane);                   // V piece q = wave + 4 j, k-major (subtile layout: split_frag.h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = 8 * (wave + 4 * j) + prow;                 // row of this lane in row-major piece wave + 4 j (split_frag.h)
        krow[j] = r;
        kch[j] = rm_piece_col_bytes(lane, r);
        const int q = wave + 4 * j, srow = (lane >> 2) & 7;
        vrow[j] = (q >> 1) * 16 + (srow >> 2) * 8 + (q & 1) * 4 + (srow & 3);      // mirrors km_piece_row(wave + 4 * j, lane)
    }
    // a piece's source = (uniform) plane base of tile t + a 32-bit per-lane offset (the planes of one call are far below 4 GB): the
    // DMA takes the base in scalar registers, 4 vector registers hold the offsets.  A whole tile (all 64 keys < N) uses the
    // precomputed offsets, the partial last tile clamps its rows to N - 1 (K rows past N are masked to -inf scores, V rows past N
    // meet P = 0).
    const size_t tstride = (size_t)KT * ld * 2;
    unsigned koff[2], voff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        koff[j] = (unsigned)krow[j] * (unsigned)(ld * 2) + kch[j];
        voff[j] = (unsigned)vrow[j] * (unsigned)(ld * 2) + vch;
    }
    auto dma16o = [](const char* ubase, const unsigned off, char* dst) __attribute__((always_inline)) { dma16(ubase + off, dst); };
    auto issue = [&](int t, int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
        const size_t o = t * tstride;
        if (t * KT + KT <= N) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dma16o(kbase[i >> 1] + o, koff[i & 1], dst + i * 4096);
#pragma unroll
            for (int i = 0; i < 4; ++i) dma16o(vbase[i >> 1] + o, voff[i & 1], dst + (4 + i) * 4096);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dma16o(kbase[i >> 1] + o, (unsigned)(min(t * KT + krow[i & 1], N - 1) - t * KT) * (unsigned)(ld * 2) + kch[i & 1], dst + i * 4096);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dma16o(vbase[i >> 1] + o, (unsigned)(min(t * KT + vrow[i & 1], N - 1) - t * KT) * (unsigned)(ld * 2) + vch, dst + (4 + i) * 4096);
        }
    };

    // ---- fragment addresses
    // K (A operand of S^T): MFMA row l31 <- key pi(l31) of the 32-key sub-tile; chunk (2 s + hf) ^ ((row >> 1) & 7)
    const int krow_a = pi_row(l31);
    const int k_off = krow_a * 128, k_sw = (krow_a >> 1) & 7;
    // V (k-major A operand of O^T): the read (key step sg, half jj, d block dd) takes subtile (sg * 2 + jj) * 2 + dd by km_tr_read,
    // with explicit lgkmcnt waits at the consumers (split_frag.h); the lane offset mirrors km_read_lane_off(lane)
    const int vg = lane >> 4, vq = lane & 15;
    const unsigned v_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + 2 * PLANE +
                           ((vg >> 1) * 4 + (vq >> 2)) * 64 + (16 * (vg & 1) + 4 * (vq & 3)) * 2;

    f32x16 oM[2], oX[2];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) { oM[d][e] = 0.f; oX[d][e] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    const int nkt = (N + KT - 1) / KT;
    long long tph[4] = {0, 0, 0, 0}, tlast = 0;      // ATT_ABL & 16: wait + barrier, QK, softmax, PV
    constexpr bool ABL16 = ATT_ABL & 16;
    if (ABL16) tlast = clock64();
#define ATT_STAMP(i)                                  \
    if (ABL16) {                                      \
        const long long now_ = clock64();             \
        tph[i] += now_ - tlast;                       \
        tlast = now_;                                 \
    }
    issue(0, 0);
    for (int t = 0; t < nkt; ++t) {
        // EVERY wave must have its own DMA pieces of tile t landed before it arrives at the barrier -- including waves
        // that do not compute (query rows past N): hipcc places the vmcnt wait of a direct-to-LDS load before the wave's
        // own first LDS read, i.e. nowhere on the `continue` path, so it is written out (found as a cross-wave race:
        // partial query blocks read K / V^T pieces that an idle wave had issued but not yet seen land).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nkt) issue(t + 1, (t + 1) & 1);
        if (!wave_active) continue;
        const char* st = smem + (t & 1) * STAGE;
        ATT_STAMP(0)

        // ---- S^T = K Q^T, two 32-key sub-tiles.  Fragment reads run ONE k-step ahead of the MFMAs that consume them (two
        // register sets), and the six MFMAs of a step are ordered so that no accumulator is touched twice in a row:
        // main 0, main 1, cross 0, cross 1 (hi x lo), cross 0, cross 1 (lo x hi).
        f32x16 sM[2], sX[2];                 // no zero fill: the first MFMA of each chain takes the inline constant 0 as C
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        h8 kh[2][2], kl[2][2];               // [set][sub-tile]
        auto k_read = [&](const int sstep, h8(&fh)[2], h8(&fl)[2]) __attribute__((always_inline)) {
            const int ch = ((2 * sstep + hf) ^ k_sw) * 16;
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2) {
                fh[kt2] = *reinterpret_cast<const h8*>(st + kt2 * 4096 + k_off + ch);
                fl[kt2] = *reinterpret_cast<const h8*>(st + PLANE + kt2 * 4096 + k_off + ch);
            }
        };
        k_read(0, kh[0], kl[0]);
        __builtin_amdgcn_s_setprio(ATT_PRIO);   // MFMA clusters outrank the co-resident wave's softmax arithmetic at the issue port
#pragma unroll
        for (int sstep = 0; sstep < 4; ++sstep) {
            const int cur = sstep & 1;
            if (sstep + 1 < 4) k_read(sstep + 1, kh[cur ^ 1], kl[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);       // the reads of step s+1 are ISSUED before the MFMAs of step s (hipcc would
                                                     // otherwise sink each read to just before its use and wait for it there)
            sM[0] = MFMA16(kh[cur][0], qh[sstep], sstep == 0 ? zero16 : sM[0]);
            sM[1] = MFMA16(kh[cur][1], qh[sstep], sstep == 0 ? zero16 : sM[1]);
            sX[0] = MFMA16(kh[cur][0], ql[sstep], sstep == 0 ? zero16 : sX[0]);
            sX[1] = MFMA16(kh[cur][1], ql[sstep], sstep == 0 ? zero16 : sX[1]);
            sX[0] = MFMA16(kl[cur][0], qh[sstep], sX[0]);
            sX[1] = MFMA16(kl[cur][1], qh[sstep], sX[1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        if (ATT_ABL & 16) { asm volatile("" ::"v"(sM[0]), "v"(sM[1]), "v"(sX[0]), "v"(sX[1])); }
        ATT_STAMP(1)
        // the first V^T fragments are fetched now: their LDS latency hides under the softmax arithmetic
        h4 vf[2][8];                         // [set][(plane * 2 + d block) * 2 + half]
        const unsigned v_st = v_lds + (t & 1) * STAGE;
        auto v_read = [&](auto sgc, h4(&f)[8]) __attribute__((always_inline)) {
            constexpr int SG = decltype(sgc)::value;
            static_for<8>([&](auto ic) __attribute__((always_inline)) {
                constexpr int i = decltype(ic)::value, pl = i >> 2, dd = (i >> 1) & 1, jj = i & 1;
                f[i] = km_tr_read<pl * PLANE + ((SG * 2 + jj) * 2 + dd) * 512>(v_st);
            });
        };
        v_read(std::integral_constant<int, 0>{}, vf[0]);
        // ---- online softmax (fp32, base-2 exponent domain: c1 = scale log2(e) folded into the score).  Register e of
        // sub-tile kt2 is key  t*64 + 32 kt2 + 16 (e >> 3) + 8 hf + (e & 7); keys >= N exist in the last tile only
        const float c1 = scale * 1.4426950408889634f, c2 = c1 * LO_INV;
        // Round 4: the VALU block between the two MFMA phases was the long pole of a key tile (2 640 of 6 230 cycles: ~12
        // instructions per score).  Now ~5: (i) the running maximum is taken over the MAIN products only (v_max3 on raw accumulators;
        // the cross terms move a score by <= 2^-11 of its size, and softmax does not care which constant near the maximum is
        // subtracted as long as numerator, denominator and lse use the same one); (ii) score scaling, cross-term fold and the
        // subtraction of the maximum are two packed FMAs on accumulator pairs feeding exp2 directly; (iii) the hi / lo split of
        // P is split_pair (split_frag.h): one packed convert, one packed multiply and one mixed-precision FMA per element.
        if (t == nkt - 1) {            // block-uniform: keys >= N exist in the last tile only
            const int kbase_t = t * KT + 8 * hf;
#pragma unroll
            for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (kbase_t + 32 * kt2 + 16 * (e >> 3) + (e & 7) >= N) sM[kt2][e] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
            for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sM[kt2][e]);
        {
            typedef unsigned u2v __attribute__((ext_vector_type(2)));
            const u2v sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
            mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * c1;          // c1 > 0; both lane halves of a query
        }
        // Lazy running maximum: it follows the tile maximum only when some query of the wave would otherwise see a probability above
        // 2^8 (wave-uniform decision).  exp2(s - m) with a stale m is the same softmax -- numerator, denominator and lse use the one
        // constant -- and P <= 256 keeps the fp16 hi / lo split as accurate as P <= 1; what it saves is the rescaling of the 64
        // accumulators, which otherwise runs whenever any of 32 maxima moves at all (most tiles).
        // (mx is the maximum of the MAIN products: the cross terms add <= 2^-10 |s| to a score in the exponent domain, so the bound is
        // P <= 2^(8 + 2^-10 max|s c1|) -- 2^8.1 for a score of 100 in that domain, far inside fp16's range either way.)
        const float m_cand = fmaxf(m_run, mx);
        const bool move = __builtin_amdgcn_ballot_w64(m_cand - m_run > 8.f) != 0;       // -inf start: inf > 8
        const float m_run2 = move ? m_cand : m_run;
        // a query that has seen only masked keys so far (m_run2 = -inf: cannot happen while every tile holds a key < N, which N >= 1
        // guarantees today -- ADVICE r4: a future masked / variable-length caller must not meet inf - inf) subtracts 0: its scores
        // are -inf, its probabilities exp2(-inf) = 0, alpha = exp2(-inf - 0) = 0 on accumulators that are still 0
        const float m_new = m_run2 == -INFINITY ? 0.f : m_run2;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);                     // exactly 1 when the maximum stays
        f32x2 psum2 = {0.f, 0.f};
        h8 ph[4], pl[4];
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                const f32x2 m2 = {sM[kt2][e], sM[kt2][e + 1]}, x2 = {sX[kt2][e], sX[kt2][e + 1]};
                const f32x2 v2 = __builtin_elementwise_fma(x2, f32x2{c2, c2}, __builtin_elementwise_fma(m2, f32x2{c1, c1}, f32x2{-m_new, -m_new}));
                const f32x2 p2 = {__builtin_amdgcn_exp2f(v2[0]), __builtin_amdgcn_exp2f(v2[1])};
                psum2 += p2;
                split_pair(p2, ph[2 * kt2 + (e >> 3)], pl[2 * kt2 + (e >> 3)], e & 7);
            }
        const float psum = psum2[0] + psum2[1];
        l_run = l_run * alpha + psum;
        if (move) {
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int e = 0; e < 16; ++e) { oM[d][e] *= alpha; oX[d][e] *= alpha; }
        }
        m_run = m_run2;
        if (ATT_ABL & 16) { asm volatile("" ::"v"(ph[0]), "v"(ph[3]), "v"(pl[0]), "v"(pl[3]), "v"(oM[0]), "v"(oX[1])); }
        ATT_STAMP(2)
        // ---- O^T += V^T P^T, same read-ahead and accumulator rotation
        __builtin_amdgcn_s_setprio(ATT_PRIO);
        static_for<4>([&](auto sgc) __attribute__((always_inline)) {
            constexpr int sg = decltype(sgc)::value, cur = sg & 1;
            if constexpr (sg + 1 < 4) {
                v_read(std::integral_constant<int, sg + 1>{}, vf[cur ^ 1]);
                asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");       // LDS returns in order: the 8 reads of step sg have landed
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
            const h4(&f)[8] = vf[cur];
            const h8 vh0 = __builtin_shufflevector(f[0], f[1], 0, 1, 2, 3, 4, 5, 6, 7), vh1 = __builtin_shufflevector(f[2], f[3], 0, 1, 2, 3, 4, 5, 6, 7);
            const h8 vl0 = __builtin_shufflevector(f[4], f[5], 0, 1, 2, 3, 4, 5, 6, 7), vl1 = __builtin_shufflevector(f[6], f[7], 0, 1, 2, 3, 4, 5, 6, 7);
            oM[0] = MFMA16(vh0, ph[sg], oM[0]);
            oM[1] = MFMA16(vh1, ph[sg], oM[1]);
            oX[0] = MFMA16(vh0, pl[sg], oX[0]);
            oX[1] = MFMA16(vh1, pl[sg], oX[1]);
            oX[0] = MFMA16(vl0, ph[sg], oX[0]);
            oX[1] = MFMA16(vl1, ph[sg], oX[1]);
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_s_setprio(0);
        if (ATT_ABL & 16) { asm volatile("" ::"v"(oM[0]), "v"(oM[1]), "v"(oX[0]), "v"(oX[1])); }
        ATT_STAMP(3)
    }
    if ((ATT_ABL & 16) && lse && tid == 0) {
        // behind the segment's real lse data ([B][H][N] floats, rounded up to 8 bytes), one record per block of the segment
        long long* q = reinterpret_cast<long long*>(lse + (((size_t)segs.B[sg] * H * N + 1) & ~(size_t)1)) +
                       (size_t)((int)blockIdx.x - segs.first[sg]) * 4;
        q[0] = tph[0]; q[1] = tph[1]; q[2] = tph[2]; q[3] = tph[3];
    }
    if (!wave_active) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_tot;
    if (b >= B_f32) { out = nullptr; lse = nullptr; }     // fp32 copies only for the images that are back-propagated
    if (qrow < N) {
        const size_t ro = ((size_t)b * N + qrow) * D + h * HD;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (oM[d][4 * g + j] + oX[d][4 * g + j] * LO_INV) * inv;
                const int col = d * 32 + 8 * g + 4 * hf;
                if (out) *reinterpret_cast<float4*>(out + ro + col) = make_float4(v[0], v[1], v[2], v[3]);
                if (out_hi) {
                    __half hh[4], ll[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (out_scale > 0.f) split_f32_u(v[j] * out_scale, hh[j], ll[j]);     // format 1 planes for the projection GEMM
                        else split_f32(v[j], hh[j], ll[j]);
                    }
                    *reinterpret_cast<uint2*>(out_hi + ro + col) = *reinterpret_cast<const uint2*>(hh);
                    *reinterpret_cast<uint2*>(out_lo + ro + col) = *reinterpret_cast<const uint2*>(ll);
                }
            }
        if (lse && hf == 0) lse[((size_t)b * H + h) * N + qrow] = m_run * 0.6931471805599453f + logf(l_tot);   // m_run is in base-2 units
    }
}

// The same forward on v_mfma_f32_16x16x32_f16 (see the file header): same block, stages, DMA protocol, segments, remap, arithmetic
// and outputs as attn_fwd16_kernel; 96 MFMAs of 16 cycles per key tile and wave instead of 48 of 32.
//   * a wave's 32 queries are two 16-query column tiles ct; lane (c = lane & 15, g = lane >> 4) owns query 16 ct + c.
//   * S^T: the 64 keys of a tile are two 32-key groups G, each two 16-key tiles Tj fed in the order pi16_row (split_frag.h), so
//     register i of sM[G][j][ct] is key 32 G + 8 g + 4 j + i and {T0, T1} of a group ARE the P^T fragment of key step G.
//   * O^T: oM / oX[dt][ct] hold d = 16 dt + 4 g .. + 3 of query 16 ct + c.
//   * softmax: a query's keys sit in its four lanes g.  The common path works on per-lane partial maxima and partial row sums only
//     (no cross-lane operation); the four lanes are combined inside `move` (maximum) and once in the epilogue (row sum).
// NP = 3 is the f16x3 arithmetic above.  NP = 1 is its single-product form (dupl_attention_fwd16_prod, products = 1: the opt-in "f16"
// mode of the no-grad encoder passes): S = q_hi k_hi^T, the same fp32 softmax with the same lazy running maximum, the probabilities
// rounded to ONE fp16 plane (p <= 2^8 under the lazy maximum: far inside fp16's range; the row sum is taken before the rounding),
// O = P_hi v_hi -- 32 MFMAs per key tile and wave instead of 96.  Only the hi plane of qkv is fetched (qkv_lo is never read): a stage
// is K_hi | V_hi (16 KB), laid out, swizzled and read exactly as the hi images of the NP = 3 stage.  No lse (no-grad only), and the
// ATT_ABL / ATT_PRIO build knobs act on NP = 3 alone.  Everything marked X below (the lo plane, the cross terms) exists for NP = 3 only.
template <int NP>
__global__ __launch_bounds__(256, 2) void attn_fwd16_m16_kernel(const __half* __restrict__ qkv_hi, const __half* __restrict__ qkv_lo,
                                                                __half* __restrict__ out_hi, __half* __restrict__ out_lo,
                                                                const AttnSegs segs, int H, float scale, int remap, float out_scale) {
    static_assert(NP == 1 || NP == 3, "one product or the three of f16x3");
    constexpr bool X = NP == 3;              // lo planes and cross terms
    constexpr int PL = X ? 2 : 1;            // planes per operand
    constexpr int STAGE = 2 * PL * PLANE;    // K planes | V planes
    constexpr bool ABL16 = X && (ATT_ABL & 16);
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (segment search and block decode as in attn_fwd16_kernel, written out: as helpers they reorder both kernels' set-up)
    int sg = 0;
#pragma unroll 1
    while (sg + 1 < segs.n && (int)blockIdx.x >= segs.first[sg + 1]) ++sg;
    sg = __builtin_amdgcn_readfirstlane(sg);
    const int N = segs.N[sg], B_f32 = segs.B_f32[sg];
    float* __restrict__ out = segs.out[sg];
    float* __restrict__ lse = X ? segs.lse[sg] : nullptr;
    int bx, h, b;
    {
        const int gx = (N + 127) / 128;
        const int G = gx * H * segs.B[sg];
        const int L = (int)blockIdx.x - segs.first[sg];
        const int w = remap ? xcd_band(L, G) : L;
        bx = w % gx; h = (w / gx) % H; b = w / (gx * H);
    }
    attn_seg_planes((size_t)segs.row0[sg], H, qkv_hi, qkv_lo, out_hi, out_lo);
    const int q0 = bx * 128 + wave * 32;
    const int D = H * HD, ld = 3 * D;
    const bool wave_active = q0 < N;

    // ---- Q fragments (B operand): lane (c, g) holds Q[q0 + 16 ct + c][32 ks + 8 g .. + 7], every plane
    h8 qh[2][2], ql[2][2];                   // [ct][ks]; ql: X
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const size_t off = ((size_t)b * N + min(q0 + 16 * ct + c16, N - 1)) * ld + h * HD + 8 * g4;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qh[ct][ks] = load_bfrag(qkv_hi + off, 2 * ks);
            if constexpr (X) ql[ct][ks] = load_bfrag(qkv_lo + off, 2 * ks);
        }
    }

    // ---- DMA plan: as attn_fwd16_kernel (piece wave + 4 i of plane i / 2), with this kernel's K swizzle and V subtiles
    const int prow = lane >> 3;
    const char* kbase[2];
    kbase[0] = reinterpret_cast<const char*>(qkv_hi + (size_t)b * N * ld + D + h * HD);
    kbase[1] = reinterpret_cast<const char*>(qkv_lo + (size_t)b * N * ld + D + h * HD);
    const char* vbase[2];
    vbase[0] = kbase[0] + D * 2;
    vbase[1] = kbase[1] + D * 2;
    int krow[2], kch[2], vrow[2];
    const int vch = km16_piece_col_bytes(wave, lane);            // the same for pieces wave and wave + 4
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        krow[j] = 8 * (wave + 4 * j) + prow;
        kch[j] = rm16_piece_col_bytes(lane, krow[j]);
        vrow[j] = km16_piece_row(wave + 4 * j, lane);
    }
    const size_t tstride = (size_t)KT * ld * 2;
    unsigned koff[2], voff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        koff[j] = (unsigned)krow[j] * (unsigned)(ld * 2) + kch[j];
        voff[j] = (unsigned)vrow[j] * (unsigned)(ld * 2) + vch;
    }
    auto dma16o = [](const char* ubase, const unsigned off, char* dst) __attribute__((always_inline)) { dma16(ubase + off, dst); };
    auto issue = [&](int t, int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
        const size_t o = t * tstride;
        if (t * KT + KT <= N) {
#pragma unroll
            for (int i = 0; i < 2 * PL; ++i) dma16o(kbase[i >> 1] + o, koff[i & 1], dst + i * 4096);
#pragma unroll
            for (int i = 0; i < 2 * PL; ++i) dma16o(vbase[i >> 1] + o, voff[i & 1], dst + (2 * PL + i) * 4096);
        } else {
#pragma unroll
            for (int i = 0; i < 2 * PL; ++i)
                dma16o(kbase[i >> 1] + o, (unsigned)(min(t * KT + krow[i & 1], N - 1) - t * KT) * (unsigned)(ld * 2) + kch[i & 1], dst + i * 4096);
#pragma unroll
            for (int i = 0; i < 2 * PL; ++i)
                dma16o(vbase[i >> 1] + o, (unsigned)(min(t * KT + vrow[i & 1], N - 1) - t * KT) * (unsigned)(ld * 2) + vch, dst + (2 * PL + i) * 4096);
        }
    };

    // ---- fragment addresses
    // K: MFMA row c of tile (G, j) <- key 32 G + pi16_row(c, j); source chunk 4 ks + g sits at chunk (4 ks + g) ^ rm16_swizzle(row),
    // and the swizzle of these rows depends on c alone: one lane offset, (G, j) immediates, ks one XOR
    const int k_off = pi16_row(c16, 0) * 128 + ((g4 ^ rm16_swizzle(pi16_row(c16, 0))) * 16);
    // V: read (key step S, half jj, d tile dt) takes subtile (S * 2 + jj) * 4 + dt by km_tr_read
    const unsigned v_lds = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + PL * PLANE + km16_read_lane_off(lane);

    f32x4 oM[4][2], oX[4][2];                // [dt][ct]; oX: X
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) { oM[d][ct] = f32x4{0.f, 0.f, 0.f, 0.f}; oX[d][ct] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};      // l_run: this lane's share of the row sum

    const int nkt = (N + KT - 1) / KT;
    long long tph[4] = {0, 0, 0, 0}, tlast = 0;
    if (ABL16) tlast = clock64();
    issue(0, 0);
    for (int t = 0; t < nkt; ++t) {
        // the wait is written out on every path, idle waves included: see attn_fwd16_kernel
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nkt) issue(t + 1, (t + 1) & 1);
        if (!wave_active) continue;
        const char* st = smem + (t & 1) * STAGE;
        ATT_STAMP(0)

        // ---- S^T = K Q^T in four steps (G, ks) = (0, 0), (0, 1), (1, 0), (1, 1); fragment reads one step ahead; the twelve MFMAs
        // of a step walk the four accumulators of the group three times (main, hi x lo, lo x hi): none is touched twice in a row
        // (NP = 1: the four main MFMAs)
        f32x4 sM[2][2][2], sX[2][2][2];      // [G][j][ct]; sX: X
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        h8 kh[2][2], kl[2][2];               // [set][j]; kl: X
        auto k_read = [&](const int step, h8(&fh)[2], h8(&fl)[2]) __attribute__((always_inline)) {
            const int a = (k_off ^ ((step & 1) * 64)) + (step >> 1) * 4096;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                fh[j] = *reinterpret_cast<const h8*>(st + a + j * 512);
                if constexpr (X) fl[j] = *reinterpret_cast<const h8*>(st + PLANE + a + j * 512);
            }
        };
        k_read(0, kh[0], kl[0]);
        if constexpr (X) __builtin_amdgcn_s_setprio(ATT_PRIO);
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const int cur = step & 1, G = step >> 1, ks = step & 1;
            if (step + 1 < 4) k_read(step + 1, kh[cur ^ 1], kl[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) sM[G][j][ct] = MFMA_16x16x32(kh[cur][j], qh[ct][ks], ks == 0 ? zero4 : sM[G][j][ct]);
            if constexpr (X) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) sX[G][j][ct] = MFMA_16x16x32(kh[cur][j], ql[ct][ks], ks == 0 ? zero4 : sX[G][j][ct]);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) sX[G][j][ct] = MFMA_16x16x32(kl[cur][j], qh[ct][ks], sX[G][j][ct]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (X) __builtin_amdgcn_s_setprio(0);
        if (ABL16) {
#pragma unroll
            for (int G = 0; G < 2; ++G)
#pragma unroll
                for (int j = 0; j < 2; ++j) asm volatile("" ::"v"(sM[G][j][0]), "v"(sM[G][j][1]), "v"(sX[G][j][0]), "v"(sX[G][j][1]));
        }
        ATT_STAMP(1)
        // the first V^T fragments are fetched now: their LDS latency hides under the softmax arithmetic.  A PV step is (key step S,
        // d tile pair dh): 4 PL reads = plane x d tile x half, 4 NP MFMAs
        h4 vf[2][4 * PL];                         // [set][(plane * 2 + d tile of the pair) * 2 + half]
        const unsigned v_st = v_lds + (t & 1) * STAGE;
        auto v_read = [&](auto hc, h4(&f)[4 * PL]) __attribute__((always_inline)) {
            constexpr int HS = decltype(hc)::value, S = HS >> 1, DH = HS & 1;
            static_for<4 * PL>([&](auto ic) __attribute__((always_inline)) {
                constexpr int i = decltype(ic)::value, pl = i >> 2, dd = (i >> 1) & 1, jj = i & 1;
                f[i] = km_tr_read<pl * PLANE + ((S * 2 + jj) * 4 + 2 * DH + dd) * 512>(v_st);
            });
        };
        v_read(std::integral_constant<int, 0>{}, vf[0]);
        // ---- online softmax: the arithmetic of attn_fwd16_kernel (see there), per column tile
        const float c1 = scale * 1.4426950408889634f, c2 = c1 * LO_INV;
        if (t == nkt - 1) {            // block-uniform: keys >= N exist in the last tile only
            const int kbase_t = t * KT + 8 * g4;
#pragma unroll
            for (int G = 0; G < 2; ++G)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (kbase_t + 32 * G + 4 * j + i >= N) { sM[G][j][0][i] = -INFINITY; sM[G][j][1][i] = -INFINITY; }
        }
        // Lazy running maximum, decided on the lanes' PARTIAL maxima: some lane's partial c1 - m_run > 8 <=> some query's maximum
        // exceeds its running one by more than 8 (m_run is the same in a query's four lanes) -- the wave-uniform decision of
        // attn_fwd16_kernel without its cross-lane exchange.  Only a move combines the four lanes.
        float mxp[2];
        bool want = false;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            float mx = -INFINITY;
#pragma unroll
            for (int G = 0; G < 2; ++G)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) mx = fmaxf(mx, sM[G][j][ct][i]);
            mxp[ct] = mx * c1;                                               // c1 > 0
            want = want || (fmaxf(m_run[ct], mxp[ct]) - m_run[ct] > 8.f);    // -inf start: inf > 8; all masked so far: NaN > 8 is false
        }
        const bool move = __builtin_amdgcn_ballot_w64(want) != 0;
        if (move) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                float mx = mxp[ct];
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float m2 = fmaxf(m_run[ct], mx);
                const float alpha = __builtin_amdgcn_exp2f(m_run[ct] - (m2 == -INFINITY ? 0.f : m2));
                m_run[ct] = m2;
                l_run[ct] *= alpha;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    oM[d][ct] *= alpha;
                    if constexpr (X) oX[d][ct] *= alpha;
                }
            }
        }
        h8 ph[2][2], pl[2][2];               // [key step G][ct]; pl: X
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float m_new = m_run[ct] == -INFINITY ? 0.f : m_run[ct];      // the guard of attn_fwd16_kernel
            f32x2 psum2 = {0.f, 0.f};
#pragma unroll
            for (int G = 0; G < 2; ++G)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 4; i += 2) {
                        const f32x2 m2 = {sM[G][j][ct][i], sM[G][j][ct][i + 1]};
                        f32x2 v2;
                        if constexpr (X) {
                            const f32x2 x2 = {sX[G][j][ct][i], sX[G][j][ct][i + 1]};
                            v2 = __builtin_elementwise_fma(x2, f32x2{c2, c2}, __builtin_elementwise_fma(m2, f32x2{c1, c1}, f32x2{-m_new, -m_new}));
                        } else v2 = __builtin_elementwise_fma(m2, f32x2{c1, c1}, f32x2{-m_new, -m_new});
                        const f32x2 p2 = {__builtin_amdgcn_exp2f(v2[0]), __builtin_amdgcn_exp2f(v2[1])};
                        psum2 += p2;
                        if constexpr (X) split_pair(p2, ph[G][ct], pl[G][ct], 4 * j + i);
                        else {
                            const h2v hh = __builtin_convertvector(p2, h2v);       // one packed convert, round to nearest even
                            ph[G][ct][4 * j + i] = hh[0];
                            ph[G][ct][4 * j + i + 1] = hh[1];
                        }
                    }
            l_run[ct] += psum2[0] + psum2[1];
        }
        if (ABL16) {
            asm volatile("" ::"v"(ph[0][0]), "v"(ph[1][1]), "v"(pl[0][0]), "v"(pl[1][1]), "v"(oM[0][0]), "v"(oX[3][1]));
        }
        ATT_STAMP(2)
        // ---- O^T += V^T P^T, same read-ahead and accumulator rotation
        if constexpr (X) __builtin_amdgcn_s_setprio(ATT_PRIO);
        static_for<4>([&](auto hc) __attribute__((always_inline)) {
            constexpr int hs = decltype(hc)::value, cur = hs & 1, S = hs >> 1, d0 = 2 * (hs & 1);
            if constexpr (hs + 1 < 4) {
                v_read(std::integral_constant<int, hs + 1>{}, vf[cur ^ 1]);
                if constexpr (X) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");       // LDS returns in order: the 8 reads of step hs have landed
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_sched_barrier(0);
            const h4(&f)[4 * PL] = vf[cur];
            const h8 vh0 = __builtin_shufflevector(f[0], f[1], 0, 1, 2, 3, 4, 5, 6, 7), vh1 = __builtin_shufflevector(f[2], f[3], 0, 1, 2, 3, 4, 5, 6, 7);
            oM[d0][0] = MFMA_16x16x32(vh0, ph[S][0], oM[d0][0]);
            oM[d0][1] = MFMA_16x16x32(vh0, ph[S][1], oM[d0][1]);
            oM[d0 + 1][0] = MFMA_16x16x32(vh1, ph[S][0], oM[d0 + 1][0]);
            oM[d0 + 1][1] = MFMA_16x16x32(vh1, ph[S][1], oM[d0 + 1][1]);
            if constexpr (X) {
                const h8 vl0 = __builtin_shufflevector(f[4], f[5], 0, 1, 2, 3, 4, 5, 6, 7), vl1 = __builtin_shufflevector(f[6], f[7], 0, 1, 2, 3, 4, 5, 6, 7);
            oX[d0][0] = MFMA_16x16x32(vh0, pl[S][0], oX[d0][0]);
            oX[d0][1] = MFMA_16x16x32(vh0, pl[S][1], oX[d0][1]);
            oX[d0 + 1][0] = MFMA_16x16x32(vh1, pl[S][0], oX[d0 + 1][0]);
            oX[d0 + 1][1] = MFMA_16x16x32(vh1, pl[S][1], oX[d0 + 1][1]);
            oX[d0][0] = MFMA_16x16x32(vl0, ph[S][0], oX[d0][0]);
            oX[d0][1] = MFMA_16x16x32(vl0, ph[S][1], oX[d0][1]);
            oX[d0 + 1][0] = MFMA_16x16x32(vl1, ph[S][0], oX[d0 + 1][0]);
            oX[d0 + 1][1] = MFMA_16x16x32(vl1, ph[S][1], oX[d0 + 1][1]);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (X) __builtin_amdgcn_s_setprio(0);
        if (ABL16) {
#pragma unroll
            for (int d = 0; d < 4; ++d) asm volatile("" ::"v"(oM[d][0]), "v"(oM[d][1]), "v"(oX[d][0]), "v"(oX[d][1]));
        }
        ATT_STAMP(3)
    }
    if ((ABL16) && lse && tid == 0) {
        long long* q = reinterpret_cast<long long*>(lse + (((size_t)segs.B[sg] * H * N + 1) & ~(size_t)1)) +
                       (size_t)((int)blockIdx.x - segs.first[sg]) * 4;
        q[0] = tph[0]; q[1] = tph[1]; q[2] = tph[2]; q[3] = tph[3];
    }
    if (!wave_active) return;
    if (b >= B_f32) { out = nullptr; lse = nullptr; }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        float l_tot = l_run[ct];                      // the row sum over the query's four lanes, once
        l_tot += __shfl_xor(l_tot, 16, 64);
        l_tot += __shfl_xor(l_tot, 32, 64);
        const float inv = 1.f / l_tot;
        const int qrow = q0 + 16 * ct + c16;
        if (qrow < N) {
            const size_t ro = ((size_t)b * N + qrow) * D + h * HD;
#pragma unroll
            for (int d = 0; d < 4; ++d) {             // a query's four lanes write 64 contiguous bytes (fp32) per instruction
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (X ? oM[d][ct][j] + oX[d][ct][j] * LO_INV : oM[d][ct][j]) * inv;
                const int col = 16 * d + 4 * g4;
                if (out) *reinterpret_cast<float4*>(out + ro + col) = make_float4(v[0], v[1], v[2], v[3]);
                if (out_hi) {
                    __half hh[4], ll[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (out_scale > 0.f) split_f32_u(v[j] * out_scale, hh[j], ll[j]);
                        else split_f32(v[j], hh[j], ll[j]);
                    }
                    *reinterpret_cast<uint2*>(out_hi + ro + col) = *reinterpret_cast<const uint2*>(hh);
                    *reinterpret_cast<uint2*>(out_lo + ro + col) = *reinterpret_cast<const uint2*>(ll);
                }
            }
            if (lse && g4 == 0) lse[((size_t)b * H + h) * N + qrow] = m_run[ct] * 0.6931471805599453f + logf(l_tot);
        }
    }
}


}  // namespace

constexpr int g_attn16_remap = 1;      // XCD-aware workgroup order (whole heads per XCD)

static int attn_fwd16_launch(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, const dupl_attn_seg* sv, int32_t n,
                             int32_t H, int32_t hd, float scale, int32_t out_exp, int32_t mfma, int32_t products, dupl_stream_t s) {
    if (mfma != 0 && mfma != 16 && mfma != 32) return DUPL_ERR_ARG;
    if (products != 1 && products != 3) return DUPL_ERR_ARG;
    const bool single = products == 1;       // attn_fwd16_m16_kernel<1>: the hi plane only, the 16x16x32 shape only, no lse
    if (single && mfma == 32) return DUPL_ERR_ARG;
    if (single && !qkv_lo) qkv_lo = qkv_hi;  // (not read; stands in for the checks below)
    if (out_exp < 0 || out_exp > 15 || !sv || n < 1 || n > DUPL_ATTN_SEGS_MAX) return DUPL_ERR_ARG;
    if (!qkv_hi || !qkv_lo || ((out_hi == nullptr) != (out_lo == nullptr)) || H <= 0 || hd != HD) return DUPL_ERR_ARG;
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(qkv_hi) || !al16(qkv_lo)) return DUPL_ERR_ARG;
    // longest batch first (its blocks run longest); ties keep the caller's order
    int order[DUPL_ATTN_SEGS_MAX];
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && sv[order[j]].N > sv[order[j - 1]].N; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    AttnSegs g;
    g.n = n;
    int total = 0;
    for (int k = 0; k < n; ++k) {
        const dupl_attn_seg& q = sv[order[k]];
        int bf = q.B_f32 == 0 ? q.B : q.B_f32;          // 0 = the fp32 output / lse for every image
        if (q.B <= 0 || q.N <= 0 || q.row0 < 0 || bf < 0 || bf > q.B || (!q.out && !out_hi) || (bf < q.B && q.out && !out_hi)) return DUPL_ERR_ARG;
        if (single && q.lse) return DUPL_ERR_ARG;
        g.row0[k] = (int)q.row0; g.B[k] = q.B; g.N[k] = q.N; g.B_f32[k] = bf; g.out[k] = q.out; g.lse[k] = q.lse;
        g.first[k] = total;
        total += ((q.N + 127) / 128) * H * q.B;
    }
    g.first[n] = total;
    // The library's choice (mfma = 0) is the 16x16x32 kernel for every launch.  Stand-alone, old and new interleaved in one process
    // (profiles/mfma16_attn.txt): 8 x 1765 -10.6 %, 8 x 785 -7.4 %, 4 x 785 -4.1 %, the step's segmented launch -10.3 % in one stream
    // and -10.8 % next to a second stream, 8 x 197 a tie (12.8 us both).  No rule on the segment lengths: the two kernels differ in
    // the last bits, and an image's rows must not depend on the launch it rides in (a segmented launch against one launch per batch,
    // 8 images against the same images two at a time) -- so one kernel serves all lengths.
    const bool m16 = mfma != 32;
    const float out_scale = out_exp ? ldexpf(1.f, out_exp) : 0.f;
    if (!m16)
        DUPL_LAUNCH(attn_fwd16_kernel, dim3((unsigned)total), dim3(256), 0, (hipStream_t)s, (const __half*)qkv_hi, (const __half*)qkv_lo,
                    (__half*)out_hi, (__half*)out_lo, g, H, scale, g_attn16_remap, out_scale);
    else if (!single)
        DUPL_LAUNCH(attn_fwd16_m16_kernel<3>, dim3((unsigned)total), dim3(256), 0, (hipStream_t)s, (const __half*)qkv_hi, (const __half*)qkv_lo,
                    (__half*)out_hi, (__half*)out_lo, g, H, scale, g_attn16_remap, out_scale);
    else
        DUPL_LAUNCH(attn_fwd16_m16_kernel<1>, dim3((unsigned)total), dim3(256), 0, (hipStream_t)s, (const __half*)qkv_hi, (const __half*)qkv_lo,
                    (__half*)out_hi, (__half*)out_lo, g, H, scale, g_attn16_remap, out_scale);
    return dupl_launch_status();
}

extern "C" int dupl_attention_fwd16_prod(const void* qkv_hi, const void* qkv_lo, float* out, void* out_hi, void* out_lo, float* lse,
                                         int32_t B, int32_t N, int32_t H, int32_t hd, float scale, int32_t B_f32, int32_t out_exp,
                                         int32_t mfma, int32_t products, dupl_stream_t s) {
    if (B_f32 < 0 || B_f32 > B || (B_f32 != 0 && B_f32 < B && !out_hi) || (!out && !out_hi)) return DUPL_ERR_ARG;
    dupl_attn_seg q;
    q.row0 = 0; q.B = B; q.N = N; q.B_f32 = B_f32; q.out = out; q.lse = lse;
    return attn_fwd16_launch(qkv_hi, qkv_lo, out_hi, out_lo, &q, 1, H, hd, scale, out_exp, mfma, products, s);
}

extern "C" int dupl_attention_fwd16_segs_prod(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, const dupl_attn_seg* segs,
                                              int32_t n, int32_t H, int32_t hd, float scale, int32_t out_exp, int32_t mfma,
                                              int32_t products, dupl_stream_t s) {
    return attn_fwd16_launch(qkv_hi, qkv_lo, out_hi, out_lo, segs, n, H, hd, scale, out_exp, mfma, products, s);
}

// the entry points without the products argument: the f16x3 attention
extern "C" int dupl_attention_fwd16_mfma(const void* qkv_hi, const void* qkv_lo, float* out, void* out_hi, void* out_lo, float* lse,
                                         int32_t B, int32_t N, int32_t H, int32_t hd, float scale, int32_t B_f32, int32_t out_exp,
                                         int32_t mfma, dupl_stream_t s) {
    return dupl_attention_fwd16_prod(qkv_hi, qkv_lo, out, out_hi, out_lo, lse, B, N, H, hd, scale, B_f32, out_exp, mfma, 3, s);
}

extern "C" int dupl_attention_fwd16_segs_mfma(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, const dupl_attn_seg* segs,
                                              int32_t n, int32_t H, int32_t hd, float scale, int32_t out_exp, int32_t mfma,
                                              dupl_stream_t s) {
    return attn_fwd16_launch(qkv_hi, qkv_lo, out_hi, out_lo, segs, n, H, hd, scale, out_exp, mfma, 3, s);
}

// the entry points without the argument: the library's choice
extern "C" int dupl_attention_fwd16(const void* qkv_hi, const void* qkv_lo, float* out, void* out_hi, void* out_lo, float* lse,
                                    int32_t B, int32_t N, int32_t H, int32_t hd, float scale, int32_t B_f32, int32_t out_exp,
                                    dupl_stream_t s) {
    return dupl_attention_fwd16_mfma(qkv_hi, qkv_lo, out, out_hi, out_lo, lse, B, N, H, hd, scale, B_f32, out_exp, 0, s);
}

extern "C" int dupl_attention_fwd16_segs(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, const dupl_attn_seg* segs,
                                         int32_t n, int32_t H, int32_t hd, float scale, int32_t out_exp, dupl_stream_t s) {
    return attn_fwd16_launch(qkv_hi, qkv_lo, out_hi, out_lo, segs, n, H, hd, scale, out_exp, 0, 3, s);
}
