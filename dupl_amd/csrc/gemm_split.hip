// fp32-equivalent GEMM on the f16 matrix cores by operand splitting ("f16x3"):
//     x = hi + lo / 2048,   hi = fp16(x),   lo = fp16((x - hi) * 2048)            (x - hi is exact in fp32)
//     a * b  ~=  hi_a hi_b + (hi_a lo_b + lo_a hi_b) / 2048                         (lo_a lo_b / 2^22 dropped: <= 2^-22 |ab|)
// Every f16 x f16 product is exact in the MFMA's fp32 accumulation; hi + lo / 2048 carries 22+ significant bits of x
// (rms error ~2^-23.6 |x|), so the result sits within fp32 round-off of the exact-fp32 kernel (gemm.hip) -- measured on
// the ViT-B forward: closer to an fp64-accumulated reference than the fp32 fmaf chain is.  Cost: 3
// v_mfma_f32_32x32x16_f16 (32 cycles each) per 32x32x16 block instead of 8 v_mfma_f32_32x32x2_f32 (64 cycles each):
// 5.3x the f32-MFMA rate at the same operand bytes (two f16 planes = one fp32).  The cross terms accumulate in their
// own register set (the 2048 scaling keeps `lo` in fp16's normal range: no subnormal loss, no per-tensor scale search).
//
// k-contiguous x k-contiguous layout only (A [M][K], B [N][K]: every Linear forward directly; the backward GEMMs through
// transposed operand planes, split_prep.hip), K % 32 == 0.
// Block tile 128 x 128 x 32 on 8 waves (2 x 4, wave tile 64 x 32 = 2 x 1 MFMA tiles, two accumulator sets, 103 VGPRs ->
// 4 waves / SIMD with 2 blocks / CU) or 128 x 64 on 4 waves when the grid would leave most block slots empty.
// Global -> LDS by direct-to-LDS DMA (global_load_lds_dwordx4): a k-tile is 1 KB pieces of 16 rows x 64 bytes in the order
// A_hi | A_lo | B_hi | B_lo, piece g is fetched by wave g % NW; the LDS image is lane-linear, so the bank swizzle is applied
// on the SOURCE side: 16-byte chunk j of row r is stored at chunk j ^ ((r >> 2) & 3), which makes every ds_read_b128
// lane group hit 64 distinct banks (SQ_LDS_BANK_CONFLICT = 0).  Two LDS stages (64 KB, 2 blocks / CU), one barrier per
// k-tile: the DMA of tile t+1 runs under the MFMAs of tile t.  Accumulating GEMMs (weight gradients) split K over
// gridDim.y and add with fp32 atomics.
#include "split_frag.h"
#include "../../include/dupl_hip.h"

#ifndef G16_ABL
#define G16_ABL 0   // ablation builds only (tools/gemm16_abl.sh): 1 no DMA, 2 no MFMA, 4 no epilogue global traffic, 8 no epilogue
#endif

namespace {

constexpr int TBK = 32;

template <bool F1>
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ x, __half* __restrict__ hi, __half* __restrict__ lo,
                                                    long n4, float scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        split_h2 h[2], l[2];      // the pair form (common.h): the scalar form's bits
        if constexpr (F1) {
            split2_f32_u(gelu_f32x2{v.x, v.y}, scale, h[0], l[0]);
            split2_f32_u(gelu_f32x2{v.z, v.w}, scale, h[1], l[1]);
        } else {
            split2_f32(gelu_f32x2{v.x, v.y}, h[0], l[0]);
            split2_f32(gelu_f32x2{v.z, v.w}, h[1], l[1]);
        }
        reinterpret_cast<uint2*>(hi)[i] = *reinterpret_cast<uint2*>(h);
        reinterpret_cast<uint2*>(lo)[i] = *reinterpret_cast<uint2*>(l);
    }
}


// dupl_gemm16_desc.amax_out: block max of the per-lane max |C| values -> ONE atomic per block (non-negative floats order like
// their bits; same-address atomics cost ~12 ns each, a per-wave flush would add ~25 us to the tail of a 2048-wave launch).
// scratch: LDS that no wave reads any more once the first barrier is passed.
__device__ __forceinline__ void gemm16_amax_flush(unsigned int* out, float amx, float* scratch, const int wave, const int lane,
                                                  const int nwaves) {
    amx = wave_max(amx);
    __syncthreads();
    if (lane == 0) scratch[wave] = amx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = scratch[0];
        for (int w = 1; w < nwaves; ++w) m = fmaxf(m, scratch[w]);
        if (m > 0.f) atomicMax(out, __float_as_uint(m));
    }
}

// Epilogue shared by the split GEMM kernels.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) +
// 4 * (lane >> 5).  (mw, nw): first row / column of this wave's tile; interior: block-uniform, no per-element edge tests.
template <int WM, int WN>
__device__ __forceinline__ void gemm16_epilogue(const dupl_gemm16_desc& p, f32x16 (&accM)[WM][WN], f32x16 (&accX)[WM][WN],
                                                const int mw, const int nw, const bool interior, const int l31, const int hf,
                                                const int ksplit, float& amx) {
    const int fl = p.flags;
    const bool f_pre = fl & DUPL_GEMM_STORE_PRE, f_gelu = fl & DUPL_GEMM_GELU, f_relu = fl & DUPL_GEMM_RELU;
    const bool f_acc = fl & DUPL_GEMM_ACCUM, f_dgelu = fl & DUPL_GEMM_MUL_DGELU, f_rmask = fl & DUPL_GEMM_MUL_RELUMASK;
    const float alpha = p.alpha_dev ? *p.alpha_dev : 1.f;      // inverse operand scale(s) of scaled gradient planes
    __half* Ch = static_cast<__half*>(p.C_hi);
    __half* Cl = static_cast<__half*>(p.C_lo);
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int col = nw + j * 32 + l31;
        if (!interior && col >= p.N) continue;
        const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            const int rbase = mw + i * 32 + 4 * hf;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                int row = rbase + (e & 3) + 8 * (e >> 2);
                asm volatile("" : "+v"(row));        // keep the address arithmetic of element e AT element e: hoisted and
                                                     // CSE'd across the 16 x WM x WN elements it spills (144 VGPRs at 2 x 2 tiles)
                if (!interior && row >= p.M) continue;
                float v = (accM[i][j][e] + accX[i][j][e] * LO_INV) * alpha + bv;
                const bool w32 = p.c_rows <= 0 || row < p.c_rows;      // fp32 copies for the first c_rows rows only
                if (f_pre && w32) p.aux[(size_t)row * p.ldaux + col] = v;
                if (f_gelu) v = gelu_f(v);
                if (f_relu) v = fmaxf(v, 0.f);
                if (f_dgelu) v *= gelu_grad_f(p.aux[(size_t)row * p.ldaux + col]);
                if (f_rmask) v = p.aux[(size_t)row * p.ldaux + col] > 0.f ? v : 0.f;
                if (p.res) v += p.res[(size_t)row * p.ldr + col];
                if (f_acc) {
                    float* cp = p.C + (size_t)row * p.ldc + col;
                    if (ksplit > 1) unsafeAtomicAdd(cp, v);
                    else *cp += v;
                    continue;
                }
                amx = fmaxf(amx, fabsf(v));
                if (p.C && w32) p.C[(size_t)row * p.ldc + col] = v;
                if (Ch) {
                    __half h, l;
                    split_f32(v, h, l);
                    Ch[(size_t)row * p.ldo + col] = h;
                    Cl[(size_t)row * p.ldo + col] = l;
                }
            }
        }
    }
}


// Epilogue FORMS.  The walk above tests every descriptor flag again per row and per float4 (a runtime loop of ~1 850 instructions per
// 16 float4, a quarter of them scalar tests and branches, and -- on the residual path -- a full vmcnt(0) drain in front of every load).
// The step launches five flag combinations only; each is compiled as a form of its own, chosen by the host launcher from the
// descriptor (g16_epi_form / g16_epi_form_km), with the walk above as EPI_GENERIC for everything else:
//     EPI_P   bias -> result planes (format 1 of out_exp, or format 0), no fp32 C                         (qkv)
//     EPI_G   bias, STORE_PRE for rows < c_rows if asked, GELU -> planes (either format)                  (fc1)
//     EPI_R   bias + residual -> fp32 C                                                                   (proj, fc2)
//     EPI_D   alpha . tile . gelu'(aux) -> fp32 C, amax                                                   (k-major data gradient of fc2)
//     EPI_A   alpha . tile -> fp32 C, amax                                                                (k-major data gradient of proj)
// A form is the same arithmetic on the same values in the same order: the same bits (tests/test_gemm_epilogue_forms_gpu.py).
enum : int { EPI_GENERIC = 0, EPI_P = 1, EPI_G = 2, EPI_R = 3, EPI_D = 4, EPI_A = 5 };
// The epilogues hand a tile from lane to lane through LDS: a lane reads what OTHER lanes of its wave parked.  The hardware runs a wave's
// LDS instructions in order, but the compiler orders a thread's accesses only where it cannot prove them disjoint -- and in the
// straight-line code of a form it can (a lane never reads its own floats), and then moves the reads over the writes.  So the forms put
// this compiler-only fence between the parking and the walk, both ways.  It takes the LDS pointer as an operand: a memory clobber alone
// does not cover an object whose address the asm cannot know (the kernel's own __shared__ array), and the reads of one pass were
// found folded into the previous pass's.
__device__ __forceinline__ void epi_lds_fence(const float* lds) { asm volatile("" ::"v"(lds) : "memory"); }
// `vec` of the walk, for the forms
__device__ __forceinline__ bool g16_epi_vec(const dupl_gemm16_desc& p) {
    auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    return !(p.N & 3) && !(p.ldc & 3) && !(p.ldo & 3) && !(p.ldr & 3) && !(p.ldaux & 3) && a16(p.C) && a16(p.res) && a16(p.aux) &&
           a16(p.bias) && !(reinterpret_cast<uintptr_t>(p.C_hi) & 7) && !(reinterpret_cast<uintptr_t>(p.C_lo) & 7);
}


// Epilogue through LDS (ring kernels): the wave parks its (alpha-scaled) tile in its own LDS region [TH][TW] floats and walks it back
// row-wise, one float4 (4 consecutive columns) per lane -- 64 lanes = 4 rows x 256 contiguous bytes at TW = 64 -- so that every
// global access of the epilogue (C, planes, aux, res) is a full-width vector access on whole 128-byte lines instead of 2 x 128-byte
// dword rows (fp32) / 2 x 64 bytes (planes) per instruction, and the epilogue is a short runtime loop instead of unrolled element bodies.
// This is the row walk, shared by both MFMA shapes: park(ps) writes pass ps of the wave's tile into `tile` (the NPS passes reuse the
// region, same wave, in order), the walk reads it back.  ROT (the 16x16 MFMA's 4-register blocks): the floats of row r sit rotated by 16
// columns when r & 4, see gemm16_epilogue_lds16.
// Vector path needs N, ldc, ldo, ldr, ldaux multiples of 4 and 16-byte (8 for planes) aligned bases: `vec`, block-uniform;
// otherwise, and in edge columns, the same values go out element-wise.
// FORM: EPI_GENERIC reads every flag and pointer from the descriptor; a form (EPI_P / EPI_G / EPI_R, matched by the launcher) is the same
// code with what the form fixes folded at compile time -- the element-safe walk of a form's edge tiles and non-vector launches.
template <int TW, int TH, int NPS, bool ROT, int FORM = EPI_GENERIC, class Park>
__device__ __forceinline__ void gemm16_epilogue_rows(const dupl_gemm16_desc& p, Park&& park, float* __restrict__ tile, const int mw0,
                                                     const int nw, const int lane, const int ksplit, float& amx) {
    constexpr int LPR = TW / 4, RPI = 64 / LPR;
    constexpr bool GEN = FORM == EPI_GENERIC;
    auto at = [](const int r, const int c) { return r * TW + (ROT ? ((c + ((r >> 2) & 1) * 16) & (TW - 1)) : c); };
    const int fl = p.flags;
    const bool f_pre = (GEN || FORM == EPI_G) && (fl & DUPL_GEMM_STORE_PRE), f_gelu = GEN ? fl & DUPL_GEMM_GELU : FORM == EPI_G;
    const bool f_relu = GEN && (fl & DUPL_GEMM_RELU);
    const bool f_acc = GEN && (fl & DUPL_GEMM_ACCUM), f_dgelu = GEN && (fl & DUPL_GEMM_MUL_DGELU), f_rmask = GEN && (fl & DUPL_GEMM_MUL_RELUMASK);
    const float out_scale = p.out_exp > 0 ? ldexpf(1.f, p.out_exp) : 0.f;      // > 0: the planes go out in format 1
    // (read at every use, as the generic walk always did: its code stays what it was)
    auto res_p = [&]() -> const float* { if constexpr (GEN || FORM == EPI_R) return p.res; else return nullptr; };
    auto C_p = [&]() -> float* { if constexpr (GEN || FORM == EPI_R) return p.C; else return nullptr; };
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
    const int mw = mw0 + ps * TH;
    if constexpr (!GEN) epi_lds_fence(tile);
    park(ps);
    if constexpr (!GEN) epi_lds_fence(tile);
    __half* Ch = GEN || FORM != EPI_R ? static_cast<__half*>(p.C_hi) : nullptr;
    __half* Cl = GEN || FORM != EPI_R ? static_cast<__half*>(p.C_lo) : nullptr;
    auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const bool vec = !(p.N & 3) && !(p.ldc & 3) && !(p.ldo & 3) && !(p.ldr & 3) && !(p.ldaux & 3) && a16(p.C) && a16(p.res) &&
                     a16(p.aux) && a16(p.bias) && !(reinterpret_cast<uintptr_t>(Ch) & 7) && !(reinterpret_cast<uintptr_t>(Cl) & 7);
    if (f_acc) {
        // C += tile (weight gradients; split-K partials meet in fp32 atomics): lane = column, so that one instruction adds
        // to 32 WN consecutive floats of a row -- whole lines per atomic request instead of 16-byte-strided lanes
        constexpr int RPA = 64 / TW;        // rows per instruction
        const int ca = lane % TW, ra = lane / TW;
        if (nw + ca >= p.N) continue;
        for (int r = ra; r < TH; r += RPA) {
            const int row = mw + r;
            if (row >= p.M) break;
            float* cp = p.C + (size_t)row * p.ldc + nw + ca;
            const float v = tile[at(r, ca)];
            if (ksplit > 1) unsafeAtomicAdd(cp, v);
            else *cp += v;
        }
        continue;
    }
    const int cl = (lane % LPR) * 4, rl = lane / LPR;
    const int col = nw + cl;
    const int nv = min(4, p.N - col);          // valid columns of this lane's float4 (<= 0: none)
    if (nv <= 0) continue;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nv) bv[c] = p.bias[col + c];
    }
    const bool fast = vec && nv == 4;
    // Rows are handled EPU at a time: the global LOADS of a chunk (residual, aux of the gelu' / relu-mask epilogues) are issued
    // before anything of it is computed or stored -- one load per row with its use right behind it made the whole epilogue a chain
    // of EPU-times as many exposed memory latencies (2 waves per SIMD hide none of it): the residual epilogue cost 19 % of a
    // 15 696 x 768 x 3 072 launch.  res / aux never alias an output of the same launch (host API: distinct tensors).
    constexpr int EPU = 4;
    const bool need_aux = f_dgelu | f_rmask;
    for (int r0 = rl; r0 < TH; r0 += EPU * RPI) {
        f32x4 rq[EPU], aq[EPU];
        if (fast) {
#pragma unroll
            for (int u = 0; u < EPU; ++u) {
                const int r = r0 + u * RPI, row = mw + r;
                if (r < TH && row < p.M) {
                    if (res_p()) rq[u] = *reinterpret_cast<const f32x4*>(res_p() + (size_t)row * p.ldr + col);
                    if (need_aux) aq[u] = *reinterpret_cast<const f32x4*>(p.aux + (size_t)row * p.ldaux + col);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < EPU; ++u) {
        const int r = r0 + u * RPI;
        if (r >= TH) break;
        const int row = mw + r;
        if (row >= p.M) break;
        const f32x4 t = *reinterpret_cast<const f32x4*>(tile + at(r, cl));
        if (G16_ABL & 4) {
            if (t[0] + t[1] + t[2] + t[3] == 123.456f) p.C[0] = 1.f;
            continue;
        }
        float v[4] = {t[0] + bv[0], t[1] + bv[1], t[2] + bv[2], t[3] + bv[3]};
        float* auxp = p.aux + (size_t)row * p.ldaux + col;
        const bool w32 = p.c_rows <= 0 || row < p.c_rows;
        if (f_pre && w32) {
            if (fast) *reinterpret_cast<f32x4*>(auxp) = f32x4{v[0], v[1], v[2], v[3]};
            else
                {
_Pragma("unroll") for (int c = 0; c < 4; ++c) if (c < nv) auxp[c] = v[c]; }
        }
        if (f_gelu) gelu4(v);
        if (f_relu) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c], 0.f);
        }
        if (need_aux) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (fast) {
                a[0] = aq[u][0]; a[1] = aq[u][1]; a[2] = aq[u][2]; a[3] = aq[u][3];
            } else
                {
_Pragma("unroll") for (int c = 0; c < 4; ++c) if (c < nv) a[c] = auxp[c]; }
            if (f_dgelu) gelu_grad_mul4(v, a);
            else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = a[c] > 0.f ? v[c] : 0.f;
            }
        }
        if (res_p()) {
            const float* rp = res_p() + (size_t)row * p.ldr + col;
            if (fast) {
                v[0] += rq[u][0]; v[1] += rq[u][1]; v[2] += rq[u][2]; v[3] += rq[u][3];
            } else
                {
_Pragma("unroll") for (int c = 0; c < 4; ++c) if (c < nv) v[c] += rp[c]; }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nv) amx = fmaxf(amx, fabsf(v[c]));
        if (C_p() && w32) {
            float* cp = C_p() + (size_t)row * p.ldc + col;
            if (fast) *reinterpret_cast<f32x4*>(cp) = f32x4{v[0], v[1], v[2], v[3]};
            else
                {
_Pragma("unroll") for (int c = 0; c < 4; ++c) if (c < nv) cp[c] = v[c]; }
        }
        if (Ch) {
            __half h[4], l[4];
            if (out_scale > 0.f) {
#pragma unroll
                for (int c = 0; c < 4; ++c) split_f32_u(v[c] * out_scale, h[c], l[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) split_f32(v[c], h[c], l[c]);
            }
            __half* hp = Ch + (size_t)row * p.ldo + col;
            __half* lp = Cl + (size_t)row * p.ldo + col;
            if (fast) {
                *reinterpret_cast<uint2*>(hp) = *reinterpret_cast<const uint2*>(h);
                *reinterpret_cast<uint2*>(lp) = *reinterpret_cast<const uint2*>(l);
            } else
                {
_Pragma("unroll") for (int c = 0; c < 4; ++c)
                    if (c < nv) {
                        hp[c] = h[c];
                        lp[c] = l[c];
                    }
                }
        }
        }   // rows of the chunk
    }
    }   // passes
}

// The forms P, G, R of the row walk on a wave tile that lies wholly inside M x N of a `vec` launch (the caller's test; every other wave
// takes the walk above): straight-line code per 16-row chunk -- no row or column predicates, the bias in registers, the planes split on
// pairs, and (R) the residual quads of chunk q + 1 requested before the stores of chunk q go out, across the passes, so that every wait
// is a counted one.  (The loads stand in front of the stores in the source, and may alias them for the compiler: it keeps the order.)
template <int FORM, int TW, int TH, int NPS, bool ROT, class Park>
__device__ __forceinline__ void gemm16_epilogue_rows_form(const dupl_gemm16_desc& p, Park&& park, float* tile, const int mw0,
                                                          const int nw, const int lane) {
    static_assert(FORM == EPI_P || FORM == EPI_G || FORM == EPI_R, "forms of the row walk");
    constexpr int LPR = TW / 4, RPI = 64 / LPR, EPU = 4, CH = EPU * RPI, CPP = TH / CH, NCH = NPS * CPP;
    static_assert(TH % CH == 0, "whole chunks");
    auto at = [](const int r, const int c) { return r * TW + (ROT ? ((c + ((r >> 2) & 1) * 16) & (TW - 1)) : c); };
    const int cl = (lane % LPR) * 4, rl = lane / LPR;
    const int col = nw + cl;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + col);
    auto row_of = [&](const int q, const int u) { return (q / CPP) * TH + (q % CPP) * CH + u * RPI + rl; };      // in the wave tile
    if constexpr (FORM == EPI_R) {
        const float* rp = p.res + (size_t)(mw0 + rl) * p.ldr + col;
        float* cp = p.C + (size_t)(mw0 + rl) * p.ldc + col;
        f32x4 rq[2][EPU];
        auto load = [&](auto qc) __attribute__((always_inline)) {
            constexpr int Q = decltype(qc)::value;
#pragma unroll
            for (int u = 0; u < EPU; ++u)
                rq[Q & 1][u] = *reinterpret_cast<const f32x4*>(rp + (size_t)((Q / CPP) * TH + (Q % CPP) * CH + u * RPI) * p.ldr);
        };
        load(std::integral_constant<int, 0>{});
        static_for<NCH>([&](auto qc) __attribute__((always_inline)) {
            constexpr int Q = decltype(qc)::value;
            if constexpr (Q % CPP == 0) {
                epi_lds_fence(tile);
                park(Q / CPP);
                epi_lds_fence(tile);
            }
            if constexpr (Q + 1 < NCH) load(std::integral_constant<int, Q + 1>{});
#pragma unroll
            for (int u = 0; u < EPU; ++u) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(tile + at((Q % CPP) * CH + u * RPI + rl, cl));
                f32x4 v = t + bv;
                v += rq[Q & 1][u];
                *reinterpret_cast<f32x4*>(cp + (size_t)((Q / CPP) * TH + (Q % CPP) * CH + u * RPI) * p.ldc) = v;
            }
        });
    } else {
        const float out_scale = ldexpf(1.f, p.out_exp);
        __half* hp = static_cast<__half*>(p.C_hi) + (size_t)(mw0 + rl) * p.ldo + col;
        __half* lp = static_cast<__half*>(p.C_lo) + (size_t)(mw0 + rl) * p.ldo + col;
        // STORE_PRE: rows of the wave tile below npre keep their pre-activation (c_rows <= 0: all of them)
        const bool f_pre = FORM == EPI_G && (p.flags & DUPL_GEMM_STORE_PRE);
        const int npre = !f_pre ? 0 : (p.c_rows <= 0 ? NPS * TH : p.c_rows - mw0);
        float* ap = f_pre ? p.aux + (size_t)(mw0 + rl) * p.ldaux + col : nullptr;
        // F1: the planes go out in format 1 (out_exp > 0: fc1 -> fc2) or in format 0 (qkv -> the split attention); one wave-uniform
        // choice in front of the walk
        auto walk = [&](auto f1c) __attribute__((always_inline)) {
            constexpr bool F1 = decltype(f1c)::value;
            static_for<NCH>([&](auto qc) __attribute__((always_inline)) {
                constexpr int Q = decltype(qc)::value;
                if constexpr (Q % CPP == 0) {
                    epi_lds_fence(tile);
                    park(Q / CPP);
                    epi_lds_fence(tile);
                }
#pragma unroll
                for (int u = 0; u < EPU; ++u) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(tile + at((Q % CPP) * CH + u * RPI + rl, cl));
                    const f32x4 v4 = t + bv;
                    float v[4] = {v4[0], v4[1], v4[2], v4[3]};
                    if constexpr (FORM == EPI_G) {
                        if (row_of(Q, u) < npre) *reinterpret_cast<f32x4*>(ap + (size_t)((Q / CPP) * TH + (Q % CPP) * CH + u * RPI) * p.ldaux) = v4;
                        gelu4(v);
                    }
                    split_h2 h[2], l[2];
                    if constexpr (F1) {
                        split2_f32_u(gelu_f32x2{v[0], v[1]}, out_scale, h[0], l[0]);
                        split2_f32_u(gelu_f32x2{v[2], v[3]}, out_scale, h[1], l[1]);
                    } else {
                        split2_f32(gelu_f32x2{v[0], v[1]}, h[0], l[0]);
                        split2_f32(gelu_f32x2{v[2], v[3]}, h[1], l[1]);
                    }
                    const size_t o = (size_t)((Q / CPP) * TH + (Q % CPP) * CH + u * RPI) * p.ldo;
                    *reinterpret_cast<uint2*>(hp + o) = *reinterpret_cast<const uint2*>(h);
                    *reinterpret_cast<uint2*>(lp + o) = *reinterpret_cast<const uint2*>(l);
                }
            });
        };
        if (p.out_exp > 0) walk(std::true_type{});
        else walk(std::false_type{});
    }
}

// The row walk for accumulators of the 32x32 MFMA: the tile is main + cross / 2048, [32 WMP][32 WN] floats per pass.
// LDS banking: the b32 writes of one MFMA register cover 32 consecutive floats per half-wave; the b128 reads of a 16-lane
// group cover two row segments that tile all 64 banks (unpadded rows of 32 / 64 floats) -- both conflict-free.
// WMP: MFMA row tiles per pass (the region holds 32 WMP rows; WM / WMP passes).  SINGLE: the cross terms were accumulated into
// accM (unscaled lo planes), accX is unused.
template <int WM, int WN, int WMP, bool SINGLE>
__device__ __forceinline__ void gemm16_epilogue_lds(const dupl_gemm16_desc& p, f32x16 (&accM)[WM][WN], f32x16 (&accX)[SINGLE ? 1 : WM][SINGLE ? 1 : WN],
                                                    float* __restrict__ tile, const int mw0, const int nw, const int lane,
                                                    const int ksplit, float& amx) {
    constexpr int TW = 32 * WN, TH = 32 * WMP;
    static_assert(WM % WMP == 0, "passes");
    const int l31 = lane & 31, hf = lane >> 5;
    const float alpha = (p.alpha_dev ? *p.alpha_dev : 1.f) * (p.post_scale != 0.f ? p.post_scale : 1.f);
    auto park = [&](const int ps) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < WMP; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float v;
                    if constexpr (SINGLE) v = accM[ps * WMP + i][j][e] * alpha;
                    else v = (accM[ps * WMP + i][j][e] + accX[ps * WMP + i][j][e] * LO_INV) * alpha;
                    tile[(i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hf) * TW + j * 32 + l31] = v;
                }
    };
    gemm16_epilogue_rows<TW, TH, WM / WMP, false>(p, park, tile, mw0, nw, lane, ksplit, amx);
}

// The same for accumulators of the 16x16x32 MFMA (format 1, one set): RB x CB blocks of 4 registers, col = lane & 15, row =
// 4 (lane >> 4) + reg; RBP row blocks per pass.  The b32 writes of one register put lanes l and l + 16 four rows apart, which is a
// multiple of 32 banks at 64-float rows: rows with bit 2 set are stored rotated by 16 floats, so that a half-wave covers 32 banks;
// the four rows of one b128 read instruction share that bit, their banks are permuted as a whole -- both stay conflict-free.
// EPI: the epilogue form the launcher matched the descriptor to (interior wave tiles of vector launches; the rest walk generically).
template <int RB, int CB, int RBP, int EPI = EPI_GENERIC>
__device__ __forceinline__ void gemm16_epilogue_lds16(const dupl_gemm16_desc& p, f32x4 (&acc)[RB][CB], float* __restrict__ tile,
                                                      const int mw0, const int nw, const int lane, const int ksplit, float& amx) {
    constexpr int TW = 16 * CB, TH = 16 * RBP;
    static_assert(RB % RBP == 0 && TW == 64, "passes; the rotation is laid out for 64-float rows");
    const int l15 = lane & 15, q = lane >> 4;
    const float alpha = (p.alpha_dev ? *p.alpha_dev : 1.f) * (p.post_scale != 0.f ? p.post_scale : 1.f);
    auto park = [&](const int ps) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < RBP; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    tile[(i * 16 + 4 * q + e) * TW + ((j * 16 + l15 + (q & 1) * 16) & (TW - 1))] = acc[ps * RBP + i][j][e] * alpha;
    };
    if constexpr (EPI != EPI_GENERIC) {
        // one wave-uniform test: the wave tile wholly inside M x N, and the vector path's conditions
        if (mw0 + 16 * RB <= p.M && nw + TW <= p.N && g16_epi_vec(p)) {
            gemm16_epilogue_rows_form<EPI, TW, TH, RB / RBP, true>(p, park, tile, mw0, nw, lane);
            return;
        }
    }
    gemm16_epilogue_rows<TW, TH, RB / RBP, true, EPI>(p, park, tile, mw0, nw, lane, ksplit, amx);
}


// One float4 of the epilogue: v = 4 consecutive columns of output row `row` starting at `col` (alpha already applied), nv of
// them inside N.  Bias, activation, aux / res traffic and the stores exactly as gemm16_epilogue_lds does them (ACCUM excluded).
struct Epi16 {
    bool f_pre, f_gelu, f_relu, f_dgelu, f_rmask, vec;
    float out_scale;        // > 0: the result planes go out in format 1 (C * out_scale, unscaled lo)
    __half *Ch, *Cl;
};
// FORM: EPI_D / EPI_A fix the flags and pointers at compile time (the launcher matched the descriptor), as in gemm16_epilogue_rows
template <int FORM = EPI_GENERIC>
__device__ __forceinline__ Epi16 epi16_setup(const dupl_gemm16_desc& p) {
    Epi16 e;
    constexpr bool GEN = FORM == EPI_GENERIC;
    const int fl = p.flags;
    e.f_pre = GEN && (fl & DUPL_GEMM_STORE_PRE); e.f_gelu = GEN && (fl & DUPL_GEMM_GELU); e.f_relu = GEN && (fl & DUPL_GEMM_RELU);
    e.f_dgelu = GEN ? fl & DUPL_GEMM_MUL_DGELU : FORM == EPI_D; e.f_rmask = GEN && (fl & DUPL_GEMM_MUL_RELUMASK);
    e.Ch = GEN ? static_cast<__half*>(p.C_hi) : nullptr;
    e.Cl = GEN ? static_cast<__half*>(p.C_lo) : nullptr;
    e.out_scale = GEN && p.out_exp > 0 ? ldexpf(1.f, p.out_exp) : 0.f;
    auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    e.vec = !(p.N & 3) && !(p.ldc & 3) && !(p.ldo & 3) && !(p.ldr & 3) && !(p.ldaux & 3) && a16(p.C) && a16(p.res) && a16(p.aux) &&
            a16(p.bias) && !(reinterpret_cast<uintptr_t>(e.Ch) & 7) && !(reinterpret_cast<uintptr_t>(e.Cl) & 7);
    return e;
}
// pre / pre_kind: the residual (1) / aux (2) quad of this row when the caller has loaded it already (fast lanes only), else kind 0
template <int FORM = EPI_GENERIC>
__device__ __forceinline__ void epi16_quad(const dupl_gemm16_desc& p, const Epi16& E, const int row, const int col, const int nv,
                                           const f32x4 t, const float (&bv)[4], float& amx, const f32x4 pre = f32x4{0.f, 0.f, 0.f, 0.f},
                                           const int pre_kind = 0) {
    auto res_p = [&]() -> const float* { if constexpr (FORM == EPI_GENERIC) return p.res; else return nullptr; };
    const bool fast = E.vec && nv == 4;
    float v[4] = {t[0] + bv[0], t[1] + bv[1], t[2] + bv[2], t[3] + bv[3]};
    float* auxp = p.aux + (size_t)row * p.ldaux + col;
    const bool w32 = p.c_rows <= 0 || row < p.c_rows;          // fp32 copies for the first c_rows rows only
    if (E.f_pre && w32) {
        if (fast) *reinterpret_cast<f32x4*>(auxp) = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (c < nv) auxp[c] = v[c];
        }
    }
    if (E.f_gelu) gelu4(v);
    if (E.f_relu) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c], 0.f);
    }
    if (E.f_dgelu | E.f_rmask) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (fast) {
            const f32x4 q = pre_kind == 2 ? pre : *reinterpret_cast<const f32x4*>(auxp);
            a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; a[3] = q[3];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (c < nv) a[c] = auxp[c];
        }
        if (E.f_dgelu) gelu_grad_mul4(v, a);
        else {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = a[c] > 0.f ? v[c] : 0.f;
        }
    }
    if (res_p()) {
        const float* rp = res_p() + (size_t)row * p.ldr + col;
        if (fast) {
            const f32x4 q = pre_kind == 1 ? pre : *reinterpret_cast<const f32x4*>(rp);
            v[0] += q[0]; v[1] += q[1]; v[2] += q[2]; v[3] += q[3];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (c < nv) v[c] += rp[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < nv) amx = fmaxf(amx, fabsf(v[c]));
    if (p.C && w32) {
        float* cp = p.C + (size_t)row * p.ldc + col;
        if (fast) *reinterpret_cast<f32x4*>(cp) = f32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int c = 0; c < 4; ++c) if (c < nv) cp[c] = v[c];
        }
    }
    if (E.Ch) {
        __half h[4], l[4];
        if (E.out_scale > 0.f) {
#pragma unroll
            for (int c = 0; c < 4; ++c) split_f32_u(v[c] * E.out_scale, h[c], l[c]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) split_f32(v[c], h[c], l[c]);
        }
        __half* hp = E.Ch + (size_t)row * p.ldo + col;
        __half* lp = E.Cl + (size_t)row * p.ldo + col;
        if (fast) {
            *reinterpret_cast<uint2*>(hp) = *reinterpret_cast<const uint2*>(h);
            *reinterpret_cast<uint2*>(lp) = *reinterpret_cast<const uint2*>(l);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < nv) {
                    hp[c] = h[c];
                    lp[c] = l[c];
                }
        }
    }
}

// Epilogue of the persistent kernel: the stages already receive the next tile, so the tile leaves through a 2 KB per wave
// side buffer, 8 rows x 64 columns at a time (4 WM passes: MFMA tile i, register group g = rows 8 g .. 8 g + 7 of it).
// Same access pattern as gemm16_epilogue_lds (b32 writes of 32 consecutive floats, b128 reads of whole 256-byte rows ->
// float4 global accesses); in-order LDS execution within the wave orders the passes.
// OVERW: the caller may ask for C = v in place of C += v (DUPL_GEMM_C_FRESH; the grouped whole-tile launch only)
template <int WM, int WN, bool ACC = false, bool SINGLE = false, bool ATOM = true, bool OVERW = false>
__device__ __forceinline__ void gemm16_epilogue_side(const dupl_gemm16_desc& p, f32x16 (&accM)[WM][WN],
                                                     f32x16 (&accX)[SINGLE ? 1 : WM][SINGLE ? 1 : WN],
                                                     float* __restrict__ side, const int mw, const int nw, const int lane,
                                                     float& amx) {
    static_assert(WN == 2, "side buffer rows are 64 floats");
    const int l31 = lane & 31, hf = lane >> 5;
    const float alpha = (p.alpha_dev ? *p.alpha_dev : 1.f) * (p.post_scale != 0.f ? p.post_scale : 1.f);
    const Epi16 E = epi16_setup(p);
    const int cl = (lane & 15) * 4, rl = lane >> 4;
    const int col = nw + cl;
    const int nv = min(4, p.N - col);
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (!ACC && p.bias && nv > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nv) bv[c] = p.bias[col + c];
    }
    // (one of the two at most: the persistent kernels keep their accumulators in registers through the epilogue, 16 more would spill)
    const bool want_aux = E.f_dgelu || E.f_rmask;
    const bool pre_ld = !ACC && E.vec && nv == 4 && ((p.res != nullptr) != want_aux);
    const float* pre_src = want_aux ? p.aux : p.res;
    const int pre_ldm = want_aux ? p.ldaux : p.ldr;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // the residual / aux quads of this pass's two rows go out BEFORE the LDS round trip of the accumulators, so that their
            // latency overlaps it instead of standing in front of every row's arithmetic
            f32x4 pq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            if (pre_ld) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int row = mw + i * 32 + 8 * g + rl + 4 * k;
                    if (row < p.M) pq[k] = *reinterpret_cast<const f32x4*>(pre_src + (size_t)row * pre_ldm + col);
                }
            }
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
                    float v;
                    if constexpr (SINGLE) v = accM[i][j][4 * g + q] * alpha;
                    else v = (accM[i][j][4 * g + q] + accX[SINGLE ? 0 : i][SINGLE ? 0 : j][4 * g + q] * LO_INV) * alpha;
                    side[(q + 4 * hf) * 64 + j * 32 + l31] = v;
                }
            if constexpr (ACC) {
                // C += partial (stream-K pieces of a weight gradient meet in fp32 atomics): lane = column, one instruction adds
                // to 64 consecutive floats of a row
                if (OVERW && (p.flags & DUPL_GEMM_C_FRESH)) {
                    // the owner of a whole tile over all of K, and C holds no value yet (a lazily zeroed gradient range): C = 0 + v,
                    // the bits `C += v` leaves in a zero-filled C (the add keeps an underflowed -0 the +0 it would have become)
                    if (nw + lane < p.N) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) {
                            const int row = mw + i * 32 + 8 * g + r;
                            if (row < p.M) p.C[(size_t)row * p.ldc + nw + lane] = 0.f + side[r * 64 + lane];
                        }
                    }
                } else if (nw + lane < p.N) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int row = mw + i * 32 + 8 * g + r;
                        if (row < p.M) {
                            float* cp = p.C + (size_t)row * p.ldc + nw + lane;
                            if constexpr (ATOM) unsafeAtomicAdd(cp, side[r * 64 + lane]);
                            else *cp += side[r * 64 + lane];      // one block owns the whole tile and all of K: fixed order
                        }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int r = rl + 4 * k;
                    const f32x4 t = *reinterpret_cast<const f32x4*>(side + r * 64 + cl);
                    const int row = mw + i * 32 + 8 * g + r;
                    if (nv > 0 && row < p.M)
                        epi16_quad(p, E, row, col, nv, t, bv, amx, pq[k], pre_ld ? (want_aux ? 2 : 1) : 0);
                }
            }
        }
}

// The same side-buffer epilogue for the 4 x 4 blocks of 16x16x32 accumulators of a 64 x 64 wave tile (gemm_f16x3_km16_body; one set:
// format 1).  Register e of block (i, j) is row 16 i + 4 (lane >> 4) + e, column 16 j + (lane & 15), so a pass of 8 rows takes a register
// PAIR of every lane: pass (i, ep) = rows 16 i + 4 g + 2 ep + de (g = lane >> 4, de = 0, 1), parked in side row 2 g + de.  The b32 writes of
// one register put the four lane groups two side rows apart at the same 16 columns: side rows 2 g, 2 g + 1 are stored rotated by 16 g
// floats, so that one write instruction covers the 64 banks once; a row read back (b128, 16 lanes per row; b32, lane = column) is one
// whole rotated row -- both stay conflict-free.  Everything a row then meets is epi16_quad / the ACC forms of gemm16_epilogue_side.
// EPI: EPI_D / EPI_A (the full-epilogue data gradients) run wave tiles wholly inside M x N of a vector launch as straight-line code: no
// flag, row or column tests, the aux quads of pass q + 1 requested before the stores of pass q go out (a counted wait, no drain).
template <bool ACC, bool ATOM, bool OVERW, int EPI = EPI_GENERIC>
__device__ __forceinline__ void gemm16_epilogue_side16(const dupl_gemm16_desc& p, f32x4 (&acc)[4][4], float* __restrict__ side, const int mw,
                                                       const int nw, const int lane, float& amx) {
    const int l15 = lane & 15, g = lane >> 4;
    const float alpha = (p.alpha_dev ? *p.alpha_dev : 1.f) * (p.post_scale != 0.f ? p.post_scale : 1.f);
    const Epi16 E = epi16_setup<EPI>(p);
    auto res_p = [&]() -> const float* { if constexpr (EPI == EPI_GENERIC) return p.res; else return nullptr; };
    auto bias_p = [&]() -> const float* { if constexpr (EPI == EPI_GENERIC) return p.bias; else return nullptr; };
    const int cl = l15 * 4, rl = g;
    const int col = nw + cl;
    const int nv = min(4, p.N - col);
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (!ACC && bias_p() && nv > 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < nv) bv[c] = bias_p()[col + c];
    }
    const bool want_aux = E.f_dgelu || E.f_rmask;
    const bool pre_ld = !ACC && E.vec && nv == 4 && ((res_p() != nullptr) != want_aux);
    const float* pre_src = want_aux ? p.aux : res_p();
    const int pre_ldm = want_aux ? p.ldaux : p.ldr;
    auto tile_row = [](const int i, const int ep, const int s) { return 16 * i + 4 * (s >> 1) + 2 * ep + (s & 1); };   // of side row s
    if constexpr (!ACC && (EPI == EPI_D || EPI == EPI_A)) {
        if (mw + 64 <= p.M && nw + 64 <= p.N && E.vec) {
            // row of (pass q = (i, ep), k) in the wave tile: tile_row(i, ep, rl + 4 k) = tile_row(0, 0, rl) + 16 i + 2 ep + 8 k -- a lane's own
            // row plus a constant, which is pinned at its pass (16 + 16 row addresses computed up front spill)
            const float* xp = p.aux + (size_t)(mw + tile_row(0, 0, rl)) * p.ldaux + col;
            float* cp = p.C + (size_t)(mw + tile_row(0, 0, rl)) * p.ldc + col;
            auto pass_row = [](const int q) __attribute__((always_inline)) {
                int r = 16 * (q >> 1) + 2 * (q & 1);
                asm volatile("" : "+s"(r));
                return r;
            };
            // (one set of aux quads: the next pass's are requested once this pass's are consumed, still in front of its stores -- a
            // second set spills)
            f32x4 aq[2];
            auto load = [&](auto qc) __attribute__((always_inline)) {
                constexpr int Q = decltype(qc)::value;
                const int r0 = pass_row(Q);
#pragma unroll
                for (int k = 0; k < 2; ++k) aq[k] = *reinterpret_cast<const f32x4*>(xp + (size_t)(r0 + 8 * k) * p.ldaux);
            };
            if constexpr (EPI == EPI_D) load(std::integral_constant<int, 0>{});
            static_for<8>([&](auto qc) __attribute__((always_inline)) {
                constexpr int Q = decltype(qc)::value, i = Q >> 1, ep = Q & 1;
                epi_lds_fence(side);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int de = 0; de < 2; ++de) side[(2 * g + de) * 64 + ((j * 16 + l15 + 16 * g) & 63)] = acc[i][j][2 * ep + de] * alpha;
                epi_lds_fence(side);
                f32x4 vv[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int s = rl + 4 * k;
                    const f32x4 t = *reinterpret_cast<const f32x4*>(side + s * 64 + ((cl + 16 * (s >> 1)) & 63));
                    float v[4] = {t[0] + 0.f, t[1] + 0.f, t[2] + 0.f, t[3] + 0.f};      // (the walk's `+ bias` without one: -0 -> +0)
                    if constexpr (EPI == EPI_D) {
                        const float a[4] = {aq[k][0], aq[k][1], aq[k][2], aq[k][3]};
                        gelu_grad_mul4(v, a);
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) amx = fmaxf(amx, fabsf(v[c]));
                    vv[k] = f32x4{v[0], v[1], v[2], v[3]};
                }
                if constexpr (EPI == EPI_D && Q + 1 < 8) load(std::integral_constant<int, Q + 1>{});
                const int r0 = pass_row(Q);
#pragma unroll
                for (int k = 0; k < 2; ++k) *reinterpret_cast<f32x4*>(cp + (size_t)(r0 + 8 * k) * p.ldc) = vv[k];
            });
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int ep = 0; ep < 2; ++ep) {
            f32x4 pq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            if (pre_ld) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int row = mw + tile_row(i, ep, rl + 4 * k);
                    if (row < p.M) pq[k] = *reinterpret_cast<const f32x4*>(pre_src + (size_t)row * pre_ldm + col);
                }
            }
            if constexpr (EPI != EPI_GENERIC) epi_lds_fence(side);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int de = 0; de < 2; ++de) side[(2 * g + de) * 64 + ((j * 16 + l15 + 16 * g) & 63)] = acc[i][j][2 * ep + de] * alpha;
            if constexpr (EPI != EPI_GENERIC) epi_lds_fence(side);
            if constexpr (ACC) {
                if (nw + lane < p.N) {
                    const bool fresh = OVERW && (p.flags & DUPL_GEMM_C_FRESH);      // C = 0 + v: see gemm16_epilogue_side
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int row = mw + tile_row(i, ep, r);
                        if (row < p.M) {
                            float* cp = p.C + (size_t)row * p.ldc + nw + lane;
                            const float v = side[r * 64 + ((lane + 16 * (r >> 1)) & 63)];
                            if (fresh) *cp = 0.f + v;
                            else if constexpr (ATOM) unsafeAtomicAdd(cp, v);
                            else *cp += v;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int s = rl + 4 * k;
                    const f32x4 t = *reinterpret_cast<const f32x4*>(side + s * 64 + ((cl + 16 * (s >> 1)) & 63));
                    const int row = mw + tile_row(i, ep, s);
                    if (nv > 0 && row < p.M) epi16_quad<EPI>(p, E, row, col, nv, t, bv, amx, pq[k], pre_ld ? (want_aux ? 2 : 1) : 0);
                }
            }
        }
}

// ---- shared by the kernels below: the block tile's geometry, the block -> tile order, the piece DMA and the 32x32x16 fragment set
// WM x WN: 32x32 MFMA tiles per wave; NWM x NWN: waves per block.  Block tile (32 WM NWM) x (32 WN NWN) x 32.
template <int WM, int WN, int NWM, int NWN>
struct RingGeom {
    static constexpr int BM = 32 * WM * NWM, BN = 32 * WN * NWN, NW = NWM * NWN;
    static constexpr int PA = BM / 16, PB = BN / 16;          // 16-row x 64-byte DMA pieces per operand plane and k-tile
    static constexpr int NP = 2 * PA + 2 * PB;                // pieces per k-tile; LDS image: piece g at g * 1024 bytes
    static constexpr int STAGE = NP * 1024;
    static constexpr int PPW = NP / NW;                       // pieces per wave
    static constexpr int NMF = 3 * WM * WN, NR = 2 * (WM + WN);   // MFMAs / fragment reads of a k-step (32x32x16)
    static_assert(NP % NW == 0, "pieces must divide over the waves");
};

// Block -> tile: XCD-aware bijective remap + grouped row-tile order (same scheme as gemm.hip).  Blocks are dealt to the 8 XCDs
// round-robin; XCD x takes the x-th run of q8 (+ 1 for x < r8) positions of the tile list `lid`, and the list walks groups of g_gm row
// tiles, all column tiles of a group, row tile fastest.
template <int BM, int BN>
struct TileOrder {
    int nbm, g_gm, nblk, q8, r8, gspan;
    __device__ __forceinline__ TileOrder(const int nbm_, const int nbn, const int g_gm_)
        : nbm(nbm_), g_gm(g_gm_), nblk(nbm_ * nbn), q8(nblk >> 3), r8(nblk & 7), gspan(g_gm_ * nbn) {}
    __device__ __forceinline__ void lid_origin(const int lid, int& m0, int& n0) const {
        const int gid = lid / gspan, gin = lid - gid * gspan;
        const int gfirst = gid * g_gm;
        const int gsz = min(nbm - gfirst, g_gm);
        m0 = (gfirst + gin % gsz) * BM;
        n0 = (gin / gsz) * BN;
    }
    __device__ __forceinline__ void tile_origin(const int bid, int& m0, int& n0) const {
        const int xcd = bid & 7, idx = bid >> 3;
        lid_origin((xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx, m0, n0);
    }
    // a block whose first index is past the last tile of its XCD's share has nothing to do (idx >= q8 + (xcd < r8))
    __device__ __forceinline__ bool has_tile(const int bid) const { return (bid >> 3) < q8 + ((bid & 7) < r8 ? 1 : 0); }
};

// k-steps every piece of work of the persistent kernels must have: their prologue fills the three LDS stages before it looks at the
// piece's length.  The stream-K cuts and slices of the kernels keep to it, and so does the host where it checks K and chooses a
// slice count.
constexpr int G16_PROLOGUE = 3;

// One 1 KB piece of a k-contiguous operand plane -> LDS by direct-to-LDS DMA; the source steps to the next k-tile.
__device__ __forceinline__ void g16_dma_piece(const char*& gp, char* dst) {
    if (!(G16_ABL & 1))
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp, (__attribute__((address_space(3))) void*)dst,
                                         16, 0, 0);
    gp += TBK * 2;
}

// The fragment set of the 32x32x16 MFMA, shared by the ring kernel and its persistent form.  A set is h8 fa[2 WM], fb[2 WN]: [0, W) hi
// planes, [W, 2 W) lo planes.  a_row / b_row: this lane's row offsets inside a stage (bytes); cs: the 16-byte chunk of the k-step.
template <int WM, int WN, int PA, int PB>
struct Frag32 {
    int a_row, b_row;
    __device__ __forceinline__ void read_frags(const char* st, const int cs, h8 (&fa)[2 * WM], h8 (&fb)[2 * WN]) const {
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            fa[i] = *reinterpret_cast<const h8*>(st + a_row + i * 2048 + cs);
            fa[WM + i] = *reinterpret_cast<const h8*>(st + PA * 1024 + a_row + i * 2048 + cs);
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            fb[j] = *reinterpret_cast<const h8*>(st + b_row + j * 2048 + cs);
            fb[WN + j] = *reinterpret_cast<const h8*>(st + PB * 1024 + b_row + j * 2048 + cs);
        }
    }
    // the R-th of those reads alone.  Phase B: fragment reads of the next tile and DMA pieces alternate IN SOURCE ORDER (an LDS read
    // and an LDS-DMA write are ordered for the compiler, so the issue-order hints can only follow the source)
    template <int R>
    __device__ __forceinline__ void read_item(const char* st, const int cs, h8 (&fa)[2 * WM], h8 (&fb)[2 * WN]) const {
        if constexpr (R < WM) fa[R] = *reinterpret_cast<const h8*>(st + a_row + R * 2048 + cs);
        else if constexpr (R < 2 * WM) fa[R] = *reinterpret_cast<const h8*>(st + PA * 1024 + a_row + (R - WM) * 2048 + cs);
        else if constexpr (R < 2 * WM + WN) fb[R - 2 * WM] = *reinterpret_cast<const h8*>(st + b_row + (R - 2 * WM) * 2048 + cs);
        else fb[R - 2 * WM] = *reinterpret_cast<const h8*>(st + PB * 1024 + b_row + (R - 2 * WM - WN) * 2048 + cs);
    }
    // three passes (main, cross hi x lo, cross lo x hi), kept apart for the MFMA pipe: an accumulator is touched once per
    // pass, WM WN MFMAs apart (sched_barrier: nothing but MFMAs is pinned, reads and DMA may cross).  SINGLE (format 1 operands):
    // the cross terms go into accM, accX is unused.
    template <bool SINGLE>
    static __device__ __forceinline__ void mfmas(const h8 (&fa)[2 * WM], const h8 (&fb)[2 * WN], f32x16 (&accM)[WM][WN],
                                                 f32x16 (&accX)[SINGLE ? 1 : WM][SINGLE ? 1 : WN]) {
        constexpr int XMFMA = 0x7ff & ~0x8;
        if (G16_ABL & 2) {
#pragma unroll
            for (int i = 0; i < 2 * WM; ++i) asm volatile("" ::"v"(fa[i]));
#pragma unroll
            for (int j = 0; j < 2 * WN; ++j) asm volatile("" ::"v"(fb[j]));
            return;
        }
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) accM[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], accM[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(XMFMA);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                if constexpr (SINGLE) accM[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[WN + j], accM[i][j], 0, 0, 0);
                else accX[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[WN + j], accX[i][j], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(XMFMA);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                if constexpr (SINGLE) accM[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[WM + i], fb[j], accM[i][j], 0, 0, 0);
                else accX[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[WM + i], fb[j], accX[i][j], 0, 0, 0);
            }
    }
};

template <int WM, int WN, int NWM, int NWN, int MINB>
__global__ __launch_bounds__(64 * NWM * NWN, MINB) void gemm_f16x3_kernel(const dupl_gemm16_desc p, const int g_gm) {
    using G = RingGeom<WM, WN, NWM, NWN>;
    constexpr int BM = G::BM, BN = G::BN, NW = G::NW, PA = G::PA, PB = G::PB, STAGE = G::STAGE, PPW = G::PPW;
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const int l31 = lane & 31, hf = lane >> 5;

    // ---- tile id: TileOrder::tile_origin written out (through the struct one scalar add of this kernel comes out commuted)
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    const int nblk = nbm * nbn;
    const int bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int gspan = g_gm * nbn;
    const int gid = lid / gspan, gin = lid - gid * gspan;
    const int gfirst = gid * g_gm;
    const int gsz = min(nbm - gfirst, g_gm);
    const int tm = gfirst + gin % gsz, tn = gin / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- DMA plan: piece g = wave + NW * i; lane -> (row lane/4 of the 16-row piece, physical 16-byte chunk lane%4)
    const int prow = lane >> 2;
    const int jsrc = (lane & 3) ^ ((prow >> 2) & 3);           // logical chunk this lane fetches (source-side swizzle)
    const char* gp[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int g = wave + NW * i;
        const __half* plane;
        int ld, r0, R, q;
        if (g < PA) { plane = static_cast<const __half*>(p.A_hi); ld = p.lda; r0 = m0; R = p.M; q = g; }
        else if (g < 2 * PA) { plane = static_cast<const __half*>(p.A_lo); ld = p.lda; r0 = m0; R = p.M; q = g - PA; }
        else if (g < 2 * PA + PB) { plane = static_cast<const __half*>(p.B_hi); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA; }
        else { plane = static_cast<const __half*>(p.B_lo); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA - PB; }
        const int row = min(r0 + q * 16 + prow, R - 1);       // clamp: rows past the edge re-read the last row (discarded)
        gp[i] = reinterpret_cast<const char*>(plane + (size_t)row * ld) + jsrc * 16;
    }
    auto issue = [&](int t, int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp[i] + (size_t)t * (TBK * 2)),
                                             (__attribute__((address_space(3))) void*)(dst + i * (NW * 1024)), 16, 0, 0);
        }
    };

    // ---- fragment addresses (bytes inside a stage): plane base + row * 64 + ((s*2 + hf) ^ ((row >> 2) & 3)) * 16
    const int sw = (l31 >> 2) & 3;
    const int a_row = (wm * (32 * WM) + l31) * 64, b_row = 2 * PA * 1024 + (wn * (32 * WN) + l31) * 64;
    const int c0 = ((0 | hf) ^ sw) * 16, c1 = ((2 | hf) ^ sw) * 16;
    const Frag32<WM, WN, PA, PB> frag{a_row, b_row};

    f32x16 accM[WM][WN], accX[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                accM[i][j][e] = 0.f;
                accX[i][j][e] = 0.f;
            }

    // split-K (gridDim.y > 1, accumulating GEMMs only): this block reduces k-tiles [tb, te) and adds its partial tile
    // atomically
    const int ntk = p.K / TBK;
    const int ksplit = gridDim.y;
    const int per = (ntk + ksplit - 1) / ksplit;
    const int tb = blockIdx.y * per, te = min(ntk, tb + per);
    if (tb >= te) return;
    const int nt = te - tb;
    issue(tb, 0);
    for (int t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // my DMA pieces of tile t have landed (written out: hipcc only
                                                           // guarantees this wait before the wave's OWN first LDS read)
        __syncthreads();                       // everyone's pieces landed, and everyone is done reading the other stage
        if (t + 1 < nt) issue(tb + t + 1, (t + 1) & 1);
        const char* st = smem + (t & 1) * STAGE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            h8 fa[2 * WM], fb[2 * WN];
            frag.read_frags(st, s == 0 ? c0 : c1, fa, fb);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    accM[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], accM[i][j], 0, 0, 0);
                    accX[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[WN + j], accX[i][j], 0, 0, 0);
                    accX[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[WM + i], fb[j], accX[i][j], 0, 0, 0);
                }
        }
    }
    float amx = 0.f;
    gemm16_epilogue<WM, WN>(p, accM, accX, m0 + wm * (32 * WM), n0 + wn * (32 * WN), m0 + BM <= p.M && n0 + BN <= p.N, l31, hf,
                            ksplit, amx);
    if (p.amax_out)
        gemm16_amax_flush(static_cast<unsigned int*>(p.amax_out), amx, reinterpret_cast<float*>(smem), threadIdx.x >> 6,
                          threadIdx.x & 63, NWM * NWN);
}


// ---------------------------------------------------------------------------------------------------------------------------
// Ring-pipelined variant (round 3).  Same operand format, fragment layout and epilogue as gemm_f16x3_kernel; what changes
// is the staging pipeline and the tile:
//   * block tile 256 x 128 x 32 (48 KB per k-tile: A 2 x 16 KB, B 2 x 8 KB) -> 32 B/clk/CU of L2->LDS stream at MFMA peak
//     instead of 42.7 for 128 x 128, and 8 (wave 64 x 64) or 12 (wave 128 x 64) fragment reads per 12 / 24 MFMAs instead
//     of 6 per 6;
//   * STAGES = 3 LDS stages (144 KB, one block per CU) filled by direct-to-LDS DMA TWO k-tiles ahead; the only wait in the
//     loop is a COUNTED `s_waitcnt vmcnt(PPW)` (this wave's pieces of tile t have landed, those of tile t+1 stay in flight)
//     followed by a raw s_barrier -- never vmcnt(0), never __syncthreads() (whose fence would drain the DMA queue).
//     Hazards: RAW -- tile t is read only after every wave waited for its own pieces of t and passed the barrier of
//     iteration t; WAR -- the DMA of tile t+2 into stage (t+2) % 3 = (t-1) % 3 is issued after that same barrier, which
//     every wave reaches only after its last fragment read of tile t-1 returned (the MFMAs that consumed it precede it).
// s_waitcnt immediate (gfx9 encoding): lgkmcnt(0), expcnt untouched, vmcnt(n)
#define WAIT_LGKM0_VM(n) ((((n) & 15) | (((n) >> 4) << 14)) | (7 << 4))

// issue-order hints (hipcc keeps ds_read / MFMA / DMA clusters apart otherwise): NMF MFMAs spread over NR fragment reads
// (phase A) or over NR reads + ND DMA pieces (phase B: reads and DMA alternate while both remain)
template <int NMF, int NR, int R = 0>
__device__ __forceinline__ void sched_mfma_ds() {
    if constexpr (R < NR) {
        constexpr int nm = (R + 1) * NMF / NR - R * NMF / NR;
        if constexpr (nm > 0) __builtin_amdgcn_sched_group_barrier(0x008, nm, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        sched_mfma_ds<NMF, NR, R + 1>();
    }
}
template <int NMF, int NR, int ND, int S = 0, int RD = 0, int DD = 0>
__device__ __forceinline__ void sched_mfma_ds_dma() {
    constexpr int NS = NR + ND;
    if constexpr (S < NS) {
        constexpr int nm = (S + 1) * NMF / NS - S * NMF / NS;
        if constexpr (nm > 0) __builtin_amdgcn_sched_group_barrier(0x008, nm, 0);
        // next slot: a read if reads are behind their share, else a DMA piece
        constexpr bool rd = RD < NR && (DD >= ND || RD * ND <= DD * NR);
        if constexpr (rd) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            sched_mfma_ds_dma<NMF, NR, ND, S + 1, RD + 1, DD>();
        } else {
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
            sched_mfma_ds_dma<NMF, NR, ND, S + 1, RD, DD + 1>();
        }
    }
}

// the loads of phase B in the order sched_mfma_ds_dma asks for
template <int NR, int ND, int RD = 0, int DD = 0, class FR, class FD, class A, class B>
__device__ __forceinline__ void loads_b(FR& read_item, FD& dma_item, const char* st, const int cs, A& fa, B& fb, char* dst) {
    if constexpr (RD + DD < NR + ND) {
        constexpr bool rd = RD < NR && (DD >= ND || RD * ND <= DD * NR);
        if constexpr (rd) {
            read_item(std::integral_constant<int, RD>{}, st, cs, fa, fb);
            loads_b<NR, ND, RD + 1, DD>(read_item, dma_item, st, cs, fa, fb, dst);
        } else {
            dma_item(std::integral_constant<int, DD>{}, dst);
            loads_b<NR, ND, RD, DD + 1>(read_item, dma_item, st, cs, fa, fb, dst);
        }
    }
}

template <int WM, int WN, int NWM, int NWN, int WPS, int STAGES = 3, bool SINGLE = false>
__global__ __launch_bounds__(64 * NWM * NWN, WPS) void gemm_f16x3_ring_kernel(const dupl_gemm16_desc p, const int g_gm) {
    using G = RingGeom<WM, WN, NWM, NWN>;
    constexpr int BM = G::BM, BN = G::BN, NW = G::NW, PA = G::PA, PB = G::PB, STAGE = G::STAGE, PPW = G::PPW;
    constexpr int NMF = G::NMF, NR = G::NR;
    static_assert(STAGES * STAGE <= 160 * 1024, "LDS");
    static_assert((STAGES - 1) * PPW <= 63, "vmcnt range");
    __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int l31 = lane & 31, hf = lane >> 5;

    // tile id: TileOrder::tile_origin written out, as in gemm_f16x3_kernel
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    const int nblk = nbm * nbn;
    const int bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int gspan = g_gm * nbn;
    const int gid = lid / gspan, gin = lid - gid * gspan;
    const int gfirst = gid * g_gm;
    const int gsz = min(nbm - gfirst, g_gm);
    const int tm = gfirst + gin % gsz, tn = gin / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const int ntk = p.K / TBK;
    const int ksplit = gridDim.y;
    const int per = (ntk + ksplit - 1) / ksplit;
    const int tb = blockIdx.y * per, te = min(ntk, tb + per);
    if (tb >= te) return;
    const int nt = te - tb;
    if (G16_ABL & 16)
        if (tid == 0 && p.aux) {
            long long* q = reinterpret_cast<long long*>(p.aux) + (size_t)(blockIdx.x + gridDim.x * blockIdx.y) * 8;
            q[0] = clock64();
            q[4] = wall_clock64();
        }

    // ---- DMA plan (as gemm_f16x3_kernel): piece g = wave + NW * i
    const int prow = lane >> 2;
    const int jsrc = (lane & 3) ^ ((prow >> 2) & 3);
    const char* gp[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int g = wave + NW * i;
        const __half* plane;
        int ld, r0, R, q;
        if (g < PA) { plane = static_cast<const __half*>(p.A_hi); ld = p.lda; r0 = m0; R = p.M; q = g; }
        else if (g < 2 * PA) { plane = static_cast<const __half*>(p.A_lo); ld = p.lda; r0 = m0; R = p.M; q = g - PA; }
        else if (g < 2 * PA + PB) { plane = static_cast<const __half*>(p.B_hi); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA; }
        else { plane = static_cast<const __half*>(p.B_lo); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA - PB; }
        const int row = min(r0 + q * 16 + prow, R - 1);
        gp[i] = reinterpret_cast<const char*>(plane + (size_t)row * ld) + jsrc * 16 + (size_t)tb * (TBK * 2);
    }
    auto issue = [&](int buf) __attribute__((always_inline)) {   // next k-tile of this block -> stage buf
        char* dst = smem + buf * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            g16_dma_piece(gp[i], dst + i * (NW * 1024));
        }
    };

    // ---- fragment addresses (bytes inside a stage): plane base + row * 64 + ((s*2 + hf) ^ ((row >> 2) & 3)) * 16
    const int sw = (l31 >> 2) & 3;
    const int a_row = (wm * (32 * WM) + l31) * 64, b_row = 2 * PA * 1024 + (wn * (32 * WN) + l31) * 64;
    const int c0 = ((0 | hf) ^ sw) * 16, c1 = ((2 | hf) ^ sw) * 16;

    f32x16 accM[WM][WN], accX[SINGLE ? 1 : WM][SINGLE ? 1 : WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                accM[i][j][e] = 0.f;
                if constexpr (!SINGLE) accX[i][j][e] = 0.f;
            }
    // two fragment sets: F0 = k-step 0 of a tile, F1 = k-step 1; [0, W) hi planes, [W, 2 W) lo planes
    h8 f0a[2 * WM], f0b[2 * WN], f1a[2 * WM], f1b[2 * WN];
    const Frag32<WM, WN, PA, PB> frag{a_row, b_row};
    auto read_frags = [&](const char* st, const int cs, h8(&fa)[2 * WM], h8(&fb)[2 * WN]) __attribute__((always_inline)) { frag.read_frags(st, cs, fa, fb); };
    auto mfmas = [&](const h8(&fa)[2 * WM], const h8(&fb)[2 * WN]) __attribute__((always_inline)) { frag.template mfmas<SINGLE>(fa, fb, accM, accX); };
    auto read_item = [&](auto rc, const char* st, const int cs, h8(&fa)[2 * WM], h8(&fb)[2 * WN]) __attribute__((always_inline)) {
        frag.template read_item<decltype(rc)::value>(st, cs, fa, fb);
    };
    auto dma_item = [&](auto dc, char* dst) __attribute__((always_inline)) {
        constexpr int I = decltype(dc)::value;
        g16_dma_piece(gp[I], dst + I * (NW * 1024));
    };
    // ---- pipeline.  Tile t lives in stage t % 3.  Iteration t:
    //   phase A:  read F1(t)                      | MFMAs on F0(t)
    //   lgkmcnt(0); vmcnt(PPW): my pieces of tile t+1 landed (tile t+2 may still fly); s_barrier
    //   phase B:  read F0(t+1), DMA tile t+3 -> stage t % 3 (whose last reads, F1(t), every wave retired before the barrier)
    //                                             | MFMAs on F1(t)
    // never vmcnt(0) and never __syncthreads() in the steady state; the last three iterations run without DMA.
#pragma unroll
    for (int s = 0; s < STAGES; ++s)
        if (s < nt) issue(s);
    if (nt >= STAGES) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 1) * PPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    read_frags(smem, c0, f0a, f0b);
    if (G16_ABL & 16)
        if (tid == 0 && p.aux) reinterpret_cast<long long*>(p.aux)[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * 8 + 1] = clock64();
    int rb = 0;
    int t = 0;
    for (; t + STAGES < nt; ++t) {
        const char* st = smem + rb * STAGE;
        const int nb = rb + 1 == STAGES ? 0 : rb + 1;
        read_frags(st, c1, f1a, f1b);
        mfmas(f0a, f0b);
        sched_mfma_ds<NMF, NR>();
        __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM((STAGES - 2) * PPW));   // the builtin, so that hipcc knows F1 has landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        loads_b<NR, PPW>(read_item, dma_item, smem + nb * STAGE, c0, f0a, f0b, smem + rb * STAGE + wave * 1024);
        mfmas(f1a, f1b);
        sched_mfma_ds_dma<NMF, NR, PPW>();
        rb = nb;
    }
    for (; t < nt; ++t) {
        const char* st = smem + rb * STAGE;
        const int nb = rb + 1 == STAGES ? 0 : rb + 1;
        read_frags(st, c1, f1a, f1b);
        mfmas(f0a, f0b);
        sched_mfma_ds<NMF, NR>();
        if (t + 1 < nt) {
            __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM(0));
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            read_frags(smem + nb * STAGE, c0, f0a, f0b);
        }
        mfmas(f1a, f1b);
        rb = nb;
    }

    // every wave is done reading the stages and no DMA is in flight -> reuse the LDS for the epilogue tiles
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    constexpr int WMP = (NW * (32 * WM) * (32 * WN) * 4 <= STAGES * STAGE) ? WM : WM / 2;   // epilogue passes
    static_assert(NW * (32 * WMP) * (32 * WN) * 4 <= STAGES * STAGE, "epilogue tiles must fit the stages");
    if (G16_ABL & 16)
        if (tid == 0 && p.aux) reinterpret_cast<long long*>(p.aux)[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * 8 + 2] = clock64();
    if (G16_ABL & 8) {
        float sum = 0.f;   // keep every accumulator live
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) sum += accM[i][j][e] + (SINGLE ? 0.f : accX[SINGLE ? 0 : i][SINGLE ? 0 : j][e]);
        if (sum == 123.456f) p.C[0] = 1.f;
        return;
    }
    float amx = 0.f;
    gemm16_epilogue_lds<WM, WN, WMP, SINGLE>(p, accM, accX, reinterpret_cast<float*>(smem) + wave * ((32 * WMP) * (32 * WN)),
                                             m0 + wm * (32 * WM), n0 + wn * (32 * WN), lane, ksplit, amx);
    if (p.amax_out) gemm16_amax_flush(static_cast<unsigned int*>(p.amax_out), amx, reinterpret_cast<float*>(smem), wave, lane, NWM * NWN);
    if (G16_ABL & 16) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0 && p.aux) {
            long long* q = reinterpret_cast<long long*>(p.aux) + (size_t)(blockIdx.x + gridDim.x * blockIdx.y) * 8;
            q[3] = clock64();
            q[5] = wall_clock64();
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// The single-accumulator (format 1) ring kernel on v_mfma_f32_16x16x32_f16.  Same block and wave tiles (WM x WN still count 32 x 32
// units), LDS stages, DMA ring and tile order as gemm_f16x3_ring_kernel<.., SINGLE = true>; the same MFMA cycles (3 x 16 per 16 x 16
// block and k-tile instead of 2 x 3 x 32 per 32 x 32 block), accumulator registers and fragment reads.  What it is for: under this
// loop the chip holds its clock down, and the clock it holds depends on the MFMA shape.
//   * lane l holds row (l & 15), k = 8 (l >> 4) .. + 7 of an operand block: a k-tile (32) is ONE MFMA k-step, and a fragment is one
//     whole 1 KB DMA piece (16 rows x 64 bytes) read by one ds_read_b128.  Source-side swizzle: chunk j of row r sits at chunk
//     j ^ ((4 - (r >> 2)) & 3) -- conflict-free in all four lane groups of that read (the 32 x 32 kernels' (r >> 2) & 3 is 2-way here).
//   * per accumulator and k-tile: hi.hi, hi.lo, lo.hi, in k order -- the same code in both block tiles, so a row's result does not
//     depend on the tile it rides in.  The sums differ from the 32 x 32 x 16 kernels' in the last bits (32 products per MFMA, not 16).
//   * pipeline: the B fragments of a k-tile (2 CB) are held through the tile, the A fragments go in WM phases of two row blocks
//     (32 rows: 4 fragments), double-buffered: 64 fragment registers.  A phase walks its column blocks in order, so that the last
//     phase can refill the B fragments in place, block by block.  Phase i < WM - 1 reads A(i + 1) under the MFMAs of A(i); then ONE
//     counted s_waitcnt vmcnt + raw s_barrier (tile t + 1 landed, every wave done reading tile t); the last phase reads A(0) and B of
//     tile t + 1 and issues the DMA of tile t + STAGES into tile t's stage.
//
// NP = 1 is the single-product forward (dupl_gemm16_desc.products = 1, the opt-in "f16" mode of the no-grad encoder passes):
//     C = act(alpha * post_scale * A_hi . B_hi^T + bias) (+ res),   fp32 accumulation
// ONE MFMA per 16 x 16 block and k-tile instead of three, and only the hi planes are fetched (the lo pointers are never read and may
// be NULL); the planes are the ones the f16x3 forward takes, in either format -- the format only decides post_scale.  The result
// differs from the exact product by the rounding of the operands to fp16 (relative 2^-11 per element).  What NP changes, all of it
// behind PL (planes per operand) below:
//   * a k-tile is PL (PA + PB) pieces.  With one plane that is half a stage's bytes (32 KB at 256 x 256, 24 KB at 256 x 128), and the
//     LDS goes to a deeper ring instead (the launcher's G16H_STAGES): the loop has a third of the MFMA cycles per barrier to hide a
//     DMA round trip under.  The k-tile stays ONE MFMA k-step (32), so K % 32 == 0 is all a shape needs.
//   * a phase is 2 NP CB MFMAs with 2 PL fragment reads under its first PL column blocks.
//   * NP = 1 alone flushes the epilogue's amax (p.amax_out).
//   * EPI: the epilogue form (EPI_P / EPI_G / EPI_R, NP = 3; see gemm16_epilogue_rows_form), EPI_GENERIC for every other descriptor.
template <int WM, int WN, int NWM, int NWN, int WPS, int STAGES, int NP = 3, int EPI = EPI_GENERIC>
__global__ __launch_bounds__(64 * NWM * NWN, WPS) void gemm_f16x3_ring16_kernel(const dupl_gemm16_desc p, const int g_gm) {
    using G = RingGeom<WM, WN, NWM, NWN>;
    static_assert(NP == 1 || NP == 3, "one product or the three of f16x3");
    constexpr int PL = NP == 3 ? 2 : 1;              // planes per operand: hi, lo
    constexpr int BM = G::BM, BN = G::BN, NW = G::NW, PA = G::PA, PB = G::PB;
    constexpr int STAGE = PL * (PA + PB) * 1024, PPW = PL * (PA + PB) / NW;      // A planes | B planes, piece g at g * 1024 bytes
    constexpr int RB = 2 * WM, CB = 2 * WN;          // 16 x 16 blocks of the wave tile
    constexpr int NPH = WM;                          // phases of a k-tile: two row blocks each
    static_assert(PL * (PA + PB) % NW == 0, "pieces must divide over the waves");
    static_assert(STAGES >= 2 && STAGES * STAGE <= 160 * 1024, "LDS");
    static_assert((STAGES - 1) * PPW <= 63, "vmcnt range");
    static_assert(NPH % 2 == 0, "the A fragment sets alternate by phase");
    __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;

    // tile id: TileOrder::tile_origin written out, as in gemm_f16x3_kernel
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    const int nblk = nbm * nbn;
    const int bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int gspan = g_gm * nbn;
    const int gid = lid / gspan, gin = lid - gid * gspan;
    const int gfirst = gid * g_gm;
    const int gsz = min(nbm - gfirst, g_gm);
    const int tm = gfirst + gin % gsz, tn = gin / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nt = p.K / TBK;

    // ---- DMA plan (as gemm_f16x3_ring_kernel, with this kernel's swizzle): piece g = wave + NW * i; rows past the operand's end are
    // read as its last row (their results are never stored)
    const int prow = lane >> 2;
    const int jsrc = (lane & 3) ^ ((4 - (prow >> 2)) & 3);
    const char* gp[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int g = wave + NW * i;
        const __half* plane;
        int ld, r0, R, q;
        if (g < PA) { plane = static_cast<const __half*>(p.A_hi); ld = p.lda; r0 = m0; R = p.M; q = g; }
        else if (PL == 2 && g < 2 * PA) { plane = static_cast<const __half*>(p.A_lo); ld = p.lda; r0 = m0; R = p.M; q = g - PA; }
        else if (PL == 1 || g < 2 * PA + PB) { plane = static_cast<const __half*>(p.B_hi); ld = p.ldb; r0 = n0; R = p.N; q = g - PL * PA; }
        else { plane = static_cast<const __half*>(p.B_lo); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA - PB; }
        const int row = min(r0 + q * 16 + prow, R - 1);
        gp[i] = reinterpret_cast<const char*>(plane + (size_t)row * ld) + jsrc * 16;
    }
    auto dma_item = [&](auto dc, char* dst) __attribute__((always_inline)) {
        constexpr int I = decltype(dc)::value;
        g16_dma_piece(gp[I], dst + I * (NW * 1024));
    };
    auto issue = [&](int buf) __attribute__((always_inline)) {   // next k-tile of this block -> stage buf
        static_for<PPW>([&](auto i) __attribute__((always_inline)) { dma_item(i, smem + buf * STAGE + wave * 1024); });
    };

    // ---- fragment addresses (bytes inside a stage): plane base + row * 64 + ((lane >> 4) ^ swizzle(row)) * 16
    const int l15 = lane & 15;
    const int ch = ((lane >> 4) ^ ((4 - (l15 >> 2)) & 3)) * 16;
    const int a_off = (wm * (32 * WM) + l15) * 64 + ch, b_off = PL * PA * 1024 + (wn * (32 * WN) + l15) * 64 + ch;

    f32x4 acc[RB][CB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A: two sets of {hi rb 0, hi rb 1, lo rb 0, lo rb 1}, alternating by phase; B: {hi cb .., lo cb ..} of the k-tile (PL = 1: no lo)
    h8 fa0[2 * PL], fa1[2 * PL], fb[PL * CB];
    auto read_a = [&](auto rc, const char* st, const int ph, h8(&fa)[2 * PL]) __attribute__((always_inline)) {
        constexpr int R = decltype(rc)::value;
        fa[R] = *reinterpret_cast<const h8*>(st + (R >> 1) * (PA * 1024) + a_off + (2 * ph + (R & 1)) * 1024);
    };
    auto read_b = [&](auto jc, const char* st) __attribute__((always_inline)) {
        constexpr int J = decltype(jc)::value;
        fb[J] = *reinterpret_cast<const h8*>(st + b_off + J * 1024);
        if constexpr (PL == 2) fb[CB + J] = *reinterpret_cast<const h8*>(st + PB * 1024 + b_off + J * 1024);
    };
    // column block J of a phase: hi.hi (NP = 3: then hi.lo, lo.hi) on each of its two accumulators
    constexpr int NMB = 2 * NP;                      // MFMAs of a column block
    auto mfma_block = [&](auto phc, auto jc, const h8(&fa)[2 * PL]) __attribute__((always_inline)) {
        constexpr int PH = decltype(phc)::value, J = decltype(jc)::value;
#pragma unroll
        for (int k = 0; k < 2; ++k) acc[2 * PH + k][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[k], fb[J], acc[2 * PH + k][J], 0, 0, 0);
        if constexpr (NP == 3) {
#pragma unroll
            for (int k = 0; k < 2; ++k) acc[2 * PH + k][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[k], fb[CB + J], acc[2 * PH + k][J], 0, 0, 0);
#pragma unroll
            for (int k = 0; k < 2; ++k) acc[2 * PH + k][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[2 + k], fb[J], acc[2 * PH + k][J], 0, 0, 0);
        }
    };
    constexpr int S_MFMA = 0x008, S_DSR = 0x100, S_VMEM = 0x010;
    // issue-order hint for one column block (NMB MFMAs) with NRD fragment reads under it: one read behind each of the first MFMAs,
    // whatever is left of them behind the last one
    auto hint = [](auto nrd) __attribute__((always_inline)) {
        constexpr int NRD = decltype(nrd)::value, PAIRS = NRD < NMB ? NRD : NMB - 1;
        static_for<PAIRS>([](auto) __attribute__((always_inline)) {
            __builtin_amdgcn_sched_group_barrier(S_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(S_DSR, 1, 0);
        });
        __builtin_amdgcn_sched_group_barrier(S_MFMA, NMB - PAIRS, 0);
        if constexpr (NRD > PAIRS) __builtin_amdgcn_sched_group_barrier(S_DSR, NRD - PAIRS, 0);
    };
    // phases 0 .. NPH - 2 of the tile in stage st: the first PL column blocks of phase i run over the reads of A(i + 1); the very
    // first one also over the tile's own last B fragments (their registers are busy to the end of the previous tile's last phase)
    auto inner_phases = [&](const char* st) __attribute__((always_inline)) {
        static_for<NPH - 1>([&](auto ph) __attribute__((always_inline)) {
            constexpr int PH = decltype(ph)::value;
            static_for<CB>([&](auto j) __attribute__((always_inline)) {
                constexpr int J = decltype(j)::value;
                constexpr int NRD = (J < PL ? 2 : 0) + (PH == 0 && J == 0 ? PL : 0);
                if constexpr (PH == 0 && J == 0) read_b(std::integral_constant<int, CB - 1>{}, st);
                if constexpr (J < PL) {
                    read_a(std::integral_constant<int, 2 * J>{}, st, PH + 1, PH & 1 ? fa0 : fa1);
                    read_a(std::integral_constant<int, 2 * J + 1>{}, st, PH + 1, PH & 1 ? fa0 : fa1);
                }
                mfma_block(ph, j, PH & 1 ? fa1 : fa0);
                hint(std::integral_constant<int, NRD>{});
            });
        });
    };
    // the last phase.  LOAD: the fragments of the next tile (stage nx) are read under it -- A(0) under column block 0, the B fragments
    // of column block j IN PLACE under block j + 1, once the MFMAs of block j are out (the last ones: inner_phases); DMA: the PPW pieces
    // of tile t + STAGES go out between the blocks.  The loads stand in the source in the order the hints pin them (an LDS read and an
    // LDS-DMA write are ordered for the compiler).
    auto last_phase = [&](auto loadc, auto dmac, const char* nx, char* dst) __attribute__((always_inline)) {
        constexpr bool LOAD = decltype(loadc)::value, DMA = decltype(dmac)::value;
        constexpr auto ph = std::integral_constant<int, NPH - 1>{};
        static_for<CB>([&](auto j) __attribute__((always_inline)) {
            constexpr int J = decltype(j)::value;
            constexpr int D0 = J * PPW / CB, D1 = (J + 1) * PPW / CB;      // this block's DMA pieces
            if constexpr (LOAD) {
                if constexpr (J == 0) static_for<2 * PL>([&](auto r) __attribute__((always_inline)) { read_a(r, nx, 0, fa0); });
                else read_b(std::integral_constant<int, J - 1>{}, nx);
            }
            if constexpr (DMA) static_for<D1 - D0>([&](auto i) __attribute__((always_inline)) {
                dma_item(std::integral_constant<int, D0 + decltype(i)::value>{}, dst);
            });
            mfma_block(ph, j, fa1);
            hint(std::integral_constant<int, LOAD ? (J == 0 ? 2 * PL : PL) : 0>{});
            if constexpr (DMA && D1 > D0) __builtin_amdgcn_sched_group_barrier(S_VMEM, D1 - D0, 0);
        });
    };
    // ---- pipeline.  Tile t lives in stage t % STAGES.  Iteration t: the inner phases; lgkmcnt(0), vmcnt((STAGES - 2) PPW): my
    // pieces of tile t + 1 landed (later tiles may still fly); s_barrier: every wave is done reading tile t; the last phase.  Never
    // vmcnt(0) below the pieces in flight and never __syncthreads() in the steady state; the last STAGES iterations run without DMA.
#pragma unroll
    for (int s = 0; s < STAGES; ++s)
        if (s < nt) issue(s);
    if (nt >= STAGES) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 1) * PPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    static_for<2 * PL>([&](auto r) __attribute__((always_inline)) { read_a(r, smem, 0, fa0); });
    static_for<CB - 1>([&](auto j) __attribute__((always_inline)) { read_b(j, smem); });
    int rb = 0;
    int t = 0;
    for (; t + STAGES < nt; ++t) {
        const int nb = rb + 1 == STAGES ? 0 : rb + 1;
        inner_phases(smem + rb * STAGE);
        __builtin_amdgcn_sched_barrier(0);      // the MFMAs of the inner phases stay in front of the wait (they are no memory operations)
        __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM((STAGES - 2) * PPW));   // the builtin, so that hipcc knows the fragments have landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        last_phase(std::true_type{}, std::true_type{}, smem + nb * STAGE, smem + rb * STAGE + wave * 1024);
        rb = nb;
    }
    for (; t + 1 < nt; ++t) {
        const int nb = rb + 1 == STAGES ? 0 : rb + 1;
        inner_phases(smem + rb * STAGE);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM(0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        last_phase(std::true_type{}, std::false_type{}, smem + nb * STAGE, nullptr);
        rb = nb;
    }
    inner_phases(smem + rb * STAGE);
    last_phase(std::false_type{}, std::false_type{}, nullptr, nullptr);

    // every wave is done reading the stages and no DMA is in flight -> reuse the LDS for the epilogue tiles
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    constexpr int WTILE = NW * 16 * (16 * CB) * 4;          // bytes of one row block of every wave's tile
    constexpr int RBP = RB * WTILE <= STAGES * STAGE ? RB : ((RB / 2) * WTILE <= STAGES * STAGE ? RB / 2 : RB / 4);   // row blocks per pass
    static_assert(RBP >= 1 && RBP * WTILE <= STAGES * STAGE, "epilogue tiles must fit the stages");
    float amx = 0.f;
    gemm16_epilogue_lds16<RB, CB, RBP, EPI>(p, acc, reinterpret_cast<float*>(smem) + wave * ((16 * RBP) * (16 * CB)), m0 + wm * (32 * WM),
                                       n0 + wn * (32 * WN), lane, 1, amx);
    if constexpr (NP == 1)
        if (p.amax_out) gemm16_amax_flush(static_cast<unsigned int*>(p.amax_out), amx, reinterpret_cast<float*>(smem), wave, lane, NW);
}


// ---------------------------------------------------------------------------------------------------------------------------
// Persistent form of the ring kernel (round 3): one block per CU walks over the output tiles (tile = blockIdx.x + k gridDim.x,
// gridDim.x a multiple of 8 so that a block keeps its XCD and the XCD-aware tile order holds).  What it buys over one block per
// tile: the three-stage prologue DMA of the NEXT tile is issued before the epilogue of the current one (the stages are free
// once every wave has left the k-loop; the tile leaves through the side buffer, gemm16_epilogue_side), so a block pays its
// ~5 k-cycle pipeline fill once per launch instead of once per tile, and blocks drift apart, which spreads the HBM write
// bursts of the epilogues that otherwise come from all 256 CUs at once.  No split-K (the weight gradients stay on tile 5).
// SK (stream-K, the weight gradients C += A . B^T with few output tiles and K = all tokens): the linear space of
// (tile, k-step) pairs is cut into gridDim.x equal runs, one per block, XCD x taking the x-th eighth; a block walks its run
// piece by piece (a piece = the part of the run inside one tile) and adds every piece to C with fp32 atomics.  No block waits
// for another one, every CU gets the same number of k-steps whatever the tile count -- a split-K grid of 288 or 540 blocks
// on 256 CUs leaves the chip half empty for its second round.  Cuts are moved off the first / last two k-steps of a tile, so
// that every piece has the >= 3 k-steps the three-stage prologue needs.
template <int WM, int WN, int NWM, int NWN, int WPS, bool SK = false, bool SINGLE = false, int STAGES = 3>
__global__ __launch_bounds__(64 * NWM * NWN, WPS) void gemm_f16x3_pring_kernel(const dupl_gemm16_desc p, const int g_gm) {
    using G = RingGeom<WM, WN, NWM, NWN>;
    constexpr int BM = G::BM, BN = G::BN, NW = G::NW, PA = G::PA, PB = G::PB, STAGE = G::STAGE, PPW = G::PPW;
    constexpr int NMF = G::NMF, NR = G::NR;
    constexpr int SIDE = NW * 2048;
    static_assert(STAGES * STAGE + SIDE <= 160 * 1024, "LDS");
    static_assert(STAGES <= G16_PROLOGUE, "the prologue fills every stage before it looks at the piece's length");
    __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE + SIDE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int l31 = lane & 31, hf = lane >> 5;
    const TileOrder<BM, BN> order((p.M + BM - 1) / BM, (p.N + BN - 1) / BN, g_gm);
    const int ntf = p.K / TBK;                    // k-steps of a whole tile, >= STAGES (host)
    int nt = ntf;                                 // k-steps of the current piece (SK: a part of the tile's)

    const int prow = lane >> 2;
    const int jsrc = (lane & 3) ^ ((prow >> 2) & 3);
    const char* gp[PPW];
    auto plan = [&](const int m0, const int n0, const int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int g = wave + NW * i;
            const __half* plane;
            int ld, r0, R, q;
            if (g < PA) { plane = static_cast<const __half*>(p.A_hi); ld = p.lda; r0 = m0; R = p.M; q = g; }
            else if (g < 2 * PA) { plane = static_cast<const __half*>(p.A_lo); ld = p.lda; r0 = m0; R = p.M; q = g - PA; }
            else if (g < 2 * PA + PB) { plane = static_cast<const __half*>(p.B_hi); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA; }
            else { plane = static_cast<const __half*>(p.B_lo); ld = p.ldb; r0 = n0; R = p.N; q = g - 2 * PA - PB; }
            const int row = min(r0 + q * 16 + prow, R - 1);
            gp[i] = reinterpret_cast<const char*>(plane + (size_t)row * ld + (size_t)k0 * TBK) + jsrc * 16;
        }
    };
    auto issue = [&](int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            g16_dma_piece(gp[i], dst + i * (NW * 1024));
        }
    };
    const int sw = (l31 >> 2) & 3;
    const int a_row = (wm * (32 * WM) + l31) * 64, b_row = 2 * PA * 1024 + (wn * (32 * WN) + l31) * 64;
    const int c0 = ((0 | hf) ^ sw) * 16, c1 = ((2 | hf) ^ sw) * 16;
    f32x16 accM[WM][WN], accX[SINGLE ? 1 : WM][SINGLE ? 1 : WN];      // SINGLE (format 1 operands): the cross terms go into accM
    h8 f0a[2 * WM], f0b[2 * WN], f1a[2 * WM], f1b[2 * WN];
    const Frag32<WM, WN, PA, PB> frag{a_row, b_row};
    auto read_frags = [&](const char* st, const int cs, h8(&fa)[2 * WM], h8(&fb)[2 * WN]) __attribute__((always_inline)) { frag.read_frags(st, cs, fa, fb); };
    auto mfmas = [&](const h8(&fa)[2 * WM], const h8(&fb)[2 * WN]) __attribute__((always_inline)) { frag.template mfmas<SINGLE>(fa, fb, accM, accX); };
    auto read_item = [&](auto rc, const char* st, const int cs, h8(&fa)[2 * WM], h8(&fb)[2 * WN]) __attribute__((always_inline)) {
        frag.template read_item<decltype(rc)::value>(st, cs, fa, fb);
    };
    auto dma_item = [&](auto dc, char* dst) __attribute__((always_inline)) {
        constexpr int I = decltype(dc)::value;
        g16_dma_piece(gp[I], dst + I * (NW * 1024));
    };

    int bid = blockIdx.x;
    int pos = 0, pend = 0;           // SK: this block's run of the linear (tile, k-step) space
    int m0, n0;
    if constexpr (SK) {
        const int T = order.nblk * ntf, G = gridDim.x;
        const int L = (bid & 7) * (G >> 3) + (bid >> 3);
        auto cut = [&](const int l) {
            int x = (int)((long)T * l / G);
            const int r = x % ntf;
            if (r && r < G16_PROLOGUE) x -= r;
            else if (r > ntf - G16_PROLOGUE) x += ntf - r;
            return x;
        };
        pos = cut(L);
        pend = cut(L + 1);
        if (pos >= pend) return;
        const int lid = pos / ntf, k0 = pos - lid * ntf;
        nt = min(pend - pos, ntf - k0);
        order.lid_origin(lid, m0, n0);
        plan(m0, n0, k0);
    } else {
        if (!order.has_tile(bid)) return;
        order.tile_origin(bid, m0, n0);
        plan(m0, n0, 0);
    }
#pragma unroll
    for (int s = 0; s < STAGES; ++s) issue(s);
    bool first = true;
    float amx = 0.f;                 // max |C| over this block's tiles (dupl_gemm16_desc.amax_out)
    for (;;) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    accM[i][j][e] = 0.f;
                    if constexpr (!SINGLE) accX[i][j][e] = 0.f;
                }
        // tile 0 of this k-loop has landed.  First tile of the block: the two younger stages may still fly; later tiles: the
        // prologue was issued before the previous epilogue, whose stores are younger in the same counter -> drain everything
        if (first) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 1) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        first = false;
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        read_frags(smem, c0, f0a, f0b);
        int rb = 0;
        int t = 0;
        for (; t + STAGES < nt; ++t) {
            const char* st = smem + rb * STAGE;
            const int nb = rb + 1 == STAGES ? 0 : rb + 1;
            read_frags(st, c1, f1a, f1b);
            mfmas(f0a, f0b);
            sched_mfma_ds<NMF, NR>();
            __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM((STAGES - 2) * PPW));
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            loads_b<NR, PPW>(read_item, dma_item, smem + nb * STAGE, c0, f0a, f0b, smem + rb * STAGE + wave * 1024);
            mfmas(f1a, f1b);
            sched_mfma_ds_dma<NMF, NR, PPW>();
            rb = nb;
        }
        for (; t < nt; ++t) {
            const char* st = smem + rb * STAGE;
            const int nb = rb + 1 == STAGES ? 0 : rb + 1;
            read_frags(st, c1, f1a, f1b);
            mfmas(f0a, f0b);
            sched_mfma_ds<NMF, NR>();
            if (t + 1 < nt) {
                __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM(0));
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                read_frags(smem + nb * STAGE, c0, f0a, f0b);
            }
            mfmas(f1a, f1b);
            rb = nb;
        }
        // every wave has left the k-loop -> the stages are free: start the next tile's pipeline, then write this tile out
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int mw = m0 + wm * (32 * WM), nw = n0 + wn * (32 * WN);
        bool more;
        if constexpr (SK) {
            pos += nt;
            more = pos < pend;
            if (more) {              // the piece ended at its tile's last k-step: the next one starts a tile
                nt = min(pend - pos, ntf);
                order.lid_origin(pos / ntf, m0, n0);
                plan(m0, n0, 0);
            }
        } else {
            bid += gridDim.x;
            more = order.has_tile(bid);
            if (more) {
                order.tile_origin(bid, m0, n0);
                plan(m0, n0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int s = 0; s < STAGES; ++s) issue(s);
        }
        gemm16_epilogue_side<WM, WN, SK, SINGLE>(p, accM, accX, reinterpret_cast<float*>(smem + STAGES * STAGE) + wave * 512, mw, nw, lane,
                                         amx);
        if (!more) break;
    }
    if (p.amax_out)
        gemm16_amax_flush(static_cast<unsigned int*>(p.amax_out), amx, reinterpret_cast<float*>(smem + STAGES * STAGE), wave, lane,
                          NWM * NWN);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Layout-general single-accumulator kernel (round 4): the persistent 3-stage ring kernel for format 1 operands whose A and / or
// B operand may be stored K-MAJOR -- [K][rows] with the rows contiguous, i.e. the contraction index is the slow one.  That is
// how the backward's operands lie in memory anyway:
//   dgrad  dx[M][Kin] = dy[M][Nout] . W[Nout][Kin]        A = dy planes (k-contiguous), B = the forward's W planes, k-major
//   wgrad  dW[Nout][Kin] += dy[M][Nout]^T . x[M][Kin]     A = dy planes, k-major;       B = the forward's x planes, k-major
// so no transposed operand planes are built any more (split_rt's transposing outputs, the per-step W^T planes, the fp32 copies
// of ln1 / ln2 / h1 that existed only to be transposed).
// The MFMA fragment (lane = row l & 31, 8 consecutive k at 8 (l >> 5)) of a k-major operand is gathered by ds_read_b64_tr_b16: a
// 16-lane group reads a [4 k][16 rows] block -- lane p supplies the address of k-row (p >> 2), rows 4 (p & 3) .. + 3 -- and
// receives it transposed, lane p = row p, 4 consecutive k; two such reads (k + 0..3, k + 4..7) make the 8-half fragment.  The LDS
// image of a k-major k-tile is built for that gather (on the SOURCE side of the DMA, whose LDS side is lane-linear): 512-byte
// subtiles [8 keys][32 rows], the 8 keys being the two groups of 4 that one instruction reads, so that every instruction reads
// one contiguous subtile.
// Rows of a k-major operand beyond its k_valid are clamped to the last valid row (finite garbage): the OTHER operand must hold
// zeros there (the scaled gradient planes are written zero-padded to K, dupl_split_prepare rows_zero_to).
// SK: stream-K over (tile, k-step) as in gemm_f16x3_pring_kernel, pieces meet in fp32 atomics (ACC 1); ACC 2: C += tile by the one
// block that owns the tile (deterministic mode); ACC 0: the full epilogue (bias / activation / aux / planes / amax).
typedef short s4v __attribute__((ext_vector_type(4)));
// phase B of the k-major kernel: NR read instructions and ND DMA pieces alternate, the rarer kind spread over the other
constexpr bool slot_is_read(int S, int NR, int ND) {
    int rd = 0, dd = 0;
    for (int s = 0;; ++s) {
        const bool r = rd < NR && (dd >= ND || rd * ND <= dd * NR);
        if (s == S) return r;
        if (r) ++rd; else ++dd;
    }
}
constexpr int slot_index(int S, int NR, int ND) {
    int rd = 0, dd = 0;
    for (int s = 0;; ++s) {
        const bool r = rd < NR && (dd >= ND || rd * ND <= dd * NR);
        if (s == S) return r ? rd : dd;
        if (r) ++rd; else ++dd;
    }
}

template <int WM, int WN, int NWM, int NWN, int WPS, bool SK, int ACC, bool AKM, bool BKM, int STAGES = 3, bool ONESHOT = false>
__device__ __forceinline__ void gemm_f16x3_km_body(const dupl_gemm16_desc& p, const int g_gm, const int bid0, const int grid) {
    using G = RingGeom<WM, WN, NWM, NWN>;
    constexpr int BM = G::BM, BN = G::BN, NW = G::NW, PA = G::PA, PB = G::PB, STAGE = G::STAGE, PPW = G::PPW;
    constexpr int APW = 2 * PA / NW;                       // this wave's first APW pieces belong to A, the rest to B
    constexpr int RBA = 2 * BM, RBB = 2 * BN;              // bytes per k-row of a k-major plane image
    constexpr int NDA = AKM ? 2 : 1, NDB = BKM ? 2 : 1;    // LDS read instructions per fragment
    constexpr int NIA = 2 * WM * NDA, NIB = 2 * WN * NDB;  // ... per k-step and operand
    constexpr int NRI = NIA + NIB;
    constexpr int NMF = G::NMF;
    constexpr int SIDE = NW * 2048;
    static_assert((2 * PA) % NW == 0, "pieces must divide over the waves, operand by operand");
    static_assert(STAGES * STAGE + SIDE <= 160 * 1024, "LDS");
    static_assert(STAGES <= G16_PROLOGUE, "the prologue fills every stage before it looks at the piece's length");
    static_assert(1024 % RBA == 0 && 1024 % RBB == 0, "whole k-rows per DMA piece");
    static_assert(!SK || ACC == 1, "stream-K pieces meet in atomics");
    __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE + SIDE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int l31 = lane & 31, hf = lane >> 5;
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    const int ntf = p.K / TBK;                    // k-steps of a whole tile, >= STAGES (host)
    int nt = ntf;
    const TileOrder<BM, BN> order(nbm, nbn, g_gm);

    // ---- DMA plan.  k-contiguous operand: as in the ring kernel (16-row x 64-byte pieces, chunk ^ ((row >> 2) & 3)), gp walks
    // along k.  k-major operand: piece q = k-rows q RPP .. of the tile; lane -> (k-row, physical 16-byte chunk); gp holds the
    // column address in k-row 0 of the operand, the k-row is added (clamped to k_valid - 1) at issue time.
    const int ka_valid = p.ka_valid > 0 ? p.ka_valid : p.K, kb_valid = p.kb_valid > 0 ? p.kb_valid : p.K;
    const char* gp[PPW];
    int prow[PPW];
    int kt = 0;                                   // next k-tile to fetch
    auto plan = [&](const int m0, const int n0, const int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int g = wave + NW * i;
            const bool isA = i < APW;
            const int gg = isA ? g : g - 2 * PA;
            const int PO = isA ? PA : PB;
            const bool lo = gg >= PO;
            const int q = lo ? gg - PO : gg;
            const __half* plane = static_cast<const __half*>(isA ? (lo ? p.A_lo : p.A_hi) : (lo ? p.B_lo : p.B_hi));
            const int ld = isA ? p.lda : p.ldb, r0 = isA ? m0 : n0, R = isA ? p.M : p.N;
            const bool km = isA ? AKM : BKM;
            if (!km) {
                const int pr = lane >> 2;
                const int jsrc = (lane & 3) ^ ((pr >> 2) & 3);
                const int row = min(r0 + q * 16 + pr, R - 1);
                gp[i] = reinterpret_cast<const char*>(plane + (size_t)row * ld + (size_t)k0 * TBK) + jsrc * 16;
                prow[i] = 0;
            } else {
                // LDS image of a k-major plane: [4 key groups kk][BM / 32 row blocks][8 keys][32 rows] halfs = 512-byte subtiles;
                // key group kk = (k >> 4) * 2 + ((k >> 2) & 1) holds keys {16 ks + 4 jj + 0..3} and {16 ks + 8 + 4 jj + 0..3} -- exactly
                // what ONE ds_read_b64_tr_b16 of k-step ks, half jj gathers -- in subtile rows ((k >> 3) & 1) * 4 + (k & 3), so that
                // the 64 lanes of an instruction read one contiguous 512-byte subtile (conflict-free; a [k][rows] image with
                // a row pitch of 512 / 256 bytes is not, whatever XOR is applied to it)
                const int NBLK = (isA ? BM : BN) / 32;
                const int off = q * 1024 + lane * 16;                  // byte offset inside the plane image
                const int sub = off >> 9, srow = (off >> 6) & 7, c = (off >> 4) & 3;
                const int kk = sub / NBLK, mblk = sub - kk * NBLK;
                const int r = (kk >> 1) * 16 + (srow >> 2) * 8 + (kk & 1) * 4 + (srow & 3);      // k-row inside the k-tile, 0 .. 31
                const int col = min(r0 + mblk * 32 + c * 8, R - 8);      // R % 8 == 0 (host): the last whole chunk
                gp[i] = reinterpret_cast<const char*>(plane + col);
                prow[i] = r;
            }
        }
        kt = k0;
    };
    auto dma_piece = [&](const int i, char* dst) __attribute__((always_inline)) {
        const bool km = (i < APW) ? AKM : BKM;
        if (!km) g16_dma_piece(gp[i], dst + i * (NW * 1024));
        else {
            const int kv = (i < APW) ? ka_valid : kb_valid;
            const int ld = (i < APW) ? p.lda : p.ldb;
            const int krow = min(kt * TBK + prow[i], kv - 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp[i] + (size_t)krow * ld * 2),
                                             (__attribute__((address_space(3))) void*)(dst + i * (NW * 1024)), 16, 0, 0);
        }
    };
    auto issue = [&](int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) dma_piece(i, dst);
        ++kt;
    };

    // ---- fragment addresses (bytes inside a stage)
    const int sw = (l31 >> 2) & 3;
    const int a_row = (wm * (32 * WM) + l31) * 64, b_row = 2 * PA * 1024 + (wn * (32 * WN) + l31) * 64;
    const int c0 = ((0 | hf) ^ sw) * 16, c1 = ((2 | hf) ^ sw) * 16;
    // k-major: the read (k-step ks, half jj) of the 32-row block wm WM + i takes subtile (ks * 2 + jj) * (BM / 32) + block at the lane
    // offset of split_frag.h: one base per lane, everything else is an immediate offset
    const int kml = km_read_lane_off(lane);
    const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem);      // LDS byte address of stage 0
    const unsigned akm0 = lds0 + kml + wm * WM * 512, bkm0 = lds0 + 2 * PA * 1024 + kml + wn * WN * 512;

    f32x16 acc[WM][WN];
    f32x16 accX_unused[1][1];
    // fragments as 4-half halves: [2 t], [2 t + 1] = k 0..3 / 4..7 of fragment t; t < W: hi plane, t >= W: lo plane
    h4 f0a[4 * WM], f0b[4 * WN], f1a[4 * WM], f1b[4 * WN];
    // The transposing reads are km_tr_read (inline asm, split_frag.h): every consumer phase starts with an explicit lgkmcnt(0).
    // They go through this adapter (offset as a value): called directly, two register moves of one instantiation change places.
    auto tr_off = [](const unsigned addr, auto offc) __attribute__((always_inline)) { return km_tr_read<decltype(offc)::value>(addr); };
    // one LDS read instruction: RI-th of the A / B operand (KS = k-step inside the tile); st = stage pointer, so = its byte offset
    auto read_a = [&](auto ric, auto ksc, const char* st, const unsigned so, h4(&fa)[4 * WM]) __attribute__((always_inline)) {
        constexpr int RI = decltype(ric)::value, KS = decltype(ksc)::value;
        if constexpr (!AKM) {
            constexpr int t = RI;
            const h8 v = *reinterpret_cast<const h8*>(st + (t < WM ? 0 : PA * 1024) + a_row + (t % WM) * 2048 + (KS ? c1 : c0));
            fa[2 * t] = __builtin_shufflevector(v, v, 0, 1, 2, 3);
            fa[2 * t + 1] = __builtin_shufflevector(v, v, 4, 5, 6, 7);
        } else {
            constexpr int t = RI / 2, half = RI % 2;
            fa[2 * t + half] = tr_off(akm0 + so, std::integral_constant<int, (t < WM ? 0 : PA * 1024) + ((KS * 2 + half) * (BM / 32) + (t % WM)) * 512>{});
        }
    };
    auto read_b = [&](auto ric, auto ksc, const char* st, const unsigned so, h4(&fb)[4 * WN]) __attribute__((always_inline)) {
        constexpr int RI = decltype(ric)::value, KS = decltype(ksc)::value;
        if constexpr (!BKM) {
            constexpr int t = RI;
            const h8 v = *reinterpret_cast<const h8*>(st + (t < WN ? 0 : PB * 1024) + b_row + (t % WN) * 2048 + (KS ? c1 : c0));
            fb[2 * t] = __builtin_shufflevector(v, v, 0, 1, 2, 3);
            fb[2 * t + 1] = __builtin_shufflevector(v, v, 4, 5, 6, 7);
        } else {
            constexpr int t = RI / 2, half = RI % 2;
            fb[2 * t + half] = tr_off(bkm0 + so, std::integral_constant<int, (t < WN ? 0 : PB * 1024) + ((KS * 2 + half) * (BN / 32) + (t % WN)) * 512>{});
        }
    };
    // R-th read instruction of a k-step (A's first, then B's)
    auto read_r = [&](auto rc, auto ksc, const char* st, const unsigned so, h4(&fa)[4 * WM], h4(&fb)[4 * WN]) __attribute__((always_inline)) {
        constexpr int R = decltype(rc)::value;
        if constexpr (R < NIA) read_a(std::integral_constant<int, R>{}, ksc, st, so, fa);
        else read_b(std::integral_constant<int, R - NIA>{}, ksc, st, so, fb);
    };
    auto read_frags = [&](auto ksc, const int rbuf, h4(&fa)[4 * WM], h4(&fb)[4 * WN]) __attribute__((always_inline)) {
        static_for<NRI>([&](auto rc) __attribute__((always_inline)) { read_r(rc, ksc, smem + rbuf * STAGE, (unsigned)(rbuf * STAGE), fa, fb); });
    };
    auto frag = [](const h4 lo, const h4 hi) __attribute__((always_inline)) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); };
    // n-th MFMA of a k-step: three passes (main, hi x lo, lo x hi) over the WM x WN tiles, an accumulator is touched once per pass
    auto mfma_n = [&](auto nc, const h8(&A)[2 * WM], const h8(&B)[2 * WN]) __attribute__((always_inline)) {
        constexpr int n = decltype(nc)::value, pass = n / (WM * WN), idx = n % (WM * WN), i = idx / WN, j = idx % WN;
        if constexpr (pass == 0) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[i], B[j], acc[i][j], 0, 0, 0);
        else if constexpr (pass == 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[i], B[WN + j], acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[WM + i], B[j], acc[i][j], 0, 0, 0);
    };
    // A phase = the NMF MFMAs of one k-step on fragments (fa, fb), with NS load slots spread evenly between them IN THIS ORDER:
    // the instruction stream is written out slot by slot and pinned (sched_barrier(0)), since issue-order hints cannot see the
    // inline-asm reads
    auto phase = [&](auto nsc, const h4(&fa)[4 * WM], const h4(&fb)[4 * WN], auto&& slot) __attribute__((always_inline)) {
        constexpr int NS = decltype(nsc)::value;
        h8 A[2 * WM], B[2 * WN];
#pragma unroll
        for (int t = 0; t < 2 * WM; ++t) A[t] = frag(fa[2 * t], fa[2 * t + 1]);
#pragma unroll
        for (int t = 0; t < 2 * WN; ++t) B[t] = frag(fb[2 * t], fb[2 * t + 1]);
        if constexpr (NS == 0) {
            static_for<NMF>([&](auto nc) __attribute__((always_inline)) { mfma_n(nc, A, B); });
        } else {
            static_for<NS>([&](auto sc) __attribute__((always_inline)) {
                constexpr int S = decltype(sc)::value, n0 = S * NMF / NS, n1 = (S + 1) * NMF / NS;
                static_for<n1 - n0>([&](auto kc) __attribute__((always_inline)) { mfma_n(std::integral_constant<int, n0 + decltype(kc)::value>{}, A, B); });
                slot(sc);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
    };
    constexpr std::integral_constant<int, 0> KS0{};
    constexpr std::integral_constant<int, 1> KS1{};
    constexpr int LGKM0 = 0xC07F;        // s_waitcnt lgkmcnt(0), vmcnt / expcnt untouched

    int bid = bid0;
    int pos = 0, pend = 0;
    int m0, n0;
    if constexpr (SK) {
        const int T = order.nblk * ntf, G = grid;
        if (p.sk_slices > 0) {
            // ALIGNED k-slices (round 5): the k axis of every tile is cut into S = sk_slices equal slices and a block takes ONE (tile,
            // slice) unit; units are numbered slice-major and dealt to the XCDs in contiguous runs, so the ~G / 8 blocks of an XCD
            // work on neighbouring tiles OVER THE SAME k-RANGE at the same time: the A rows of a row band and the B columns of the
            // slice are fetched into that XCD's L2 once and shared.  The equal-run cut below gives every block its own k-range
            // (run l starts at k = 29.25 l mod 96 for fc1's data gradient): nothing is shared, 256 blocks x 1.4 MB = 365 MB come over
            // the fabric for 58 MB of operands (profiles/r04_final_pmc_hbm.txt: 380 MB per launch, 4.9 TB/s -- the kernel was bound by
            // that, not by its MFMAs).
            const int S = p.sk_slices, nblk = order.nblk, U = nblk * S;
            const int xcd = bid & 7, idx = bid >> 3;
            const int ulo = (int)((long)U * xcd / 8), uhi = (int)((long)U * (xcd + 1) / 8);
            if (idx >= uhi - ulo) return;
            const int u = ulo + idx;
            const int slice = u / nblk, lid = u - slice * nblk;
            const int per = (ntf + S - 1) / S;
            const int k0 = slice * per;
            nt = min(per, ntf - k0);            // >= G16_PROLOGUE for every slice (host)
            pos = lid * ntf + k0;
            pend = pos + nt;
            order.lid_origin(lid, m0, n0);
            plan(m0, n0, k0);
        } else {
        const int L = (bid & 7) * (G >> 3) + (bid >> 3);
        auto cut = [&](const int l) {
            int x = (int)((long)T * l / G);
            const int r = x % ntf;
            if (r && r < G16_PROLOGUE) x -= r;
            else if (r > ntf - G16_PROLOGUE) x += ntf - r;
            return x;
        };
        pos = cut(L);
        pend = cut(L + 1);
        if (pos >= pend) return;
        const int lid = pos / ntf, k0 = pos - lid * ntf;
        nt = min(pend - pos, ntf - k0);
        order.lid_origin(lid, m0, n0);
        plan(m0, n0, k0);
        }
    } else if constexpr (ONESHOT) {
        if (bid >= order.nblk) return;       // grouped launch: bid0 IS the tile's position in this problem's grouped order
        order.lid_origin(bid, m0, n0);
        plan(m0, n0, 0);
    } else {
        if (!order.has_tile(bid)) return;
        order.tile_origin(bid, m0, n0);
        plan(m0, n0, 0);
    }
#pragma unroll
    for (int s = 0; s < STAGES; ++s) issue(s);
    bool first = true;
    float amx = 0.f;
    for (;;) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        if (first) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 1) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        first = false;
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        read_frags(KS0, 0, f0a, f0b);
        int rb = 0;
        int t = 0;
        for (; t + STAGES < nt; ++t) {
            const int nb = rb + 1 == STAGES ? 0 : rb + 1;
            const char* st = smem + rb * STAGE;
            const unsigned so = (unsigned)(rb * STAGE), son = (unsigned)(nb * STAGE);
            __builtin_amdgcn_s_waitcnt(LGKM0);                       // F0(t) has landed
            // phase A: read F1(t) | MFMAs on F0(t)
            phase(std::integral_constant<int, NRI>{}, f0a, f0b, [&](auto sc) __attribute__((always_inline)) { read_r(sc, KS1, st, so, f1a, f1b); });
            __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM((STAGES - 2) * PPW));   // F1(t) landed; my pieces of tile t+1 landed
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // phase B: read F0(t+1), DMA tile t+3 -> stage rb (alternating) | MFMAs on F1(t)
            char* dst = smem + rb * STAGE + wave * 1024;
            phase(std::integral_constant<int, NRI + PPW>{}, f1a, f1b, [&](auto sc) __attribute__((always_inline)) {
                constexpr int S = decltype(sc)::value;
                if constexpr (slot_is_read(S, NRI, PPW)) read_r(std::integral_constant<int, slot_index(S, NRI, PPW)>{}, KS0, smem + nb * STAGE, son, f0a, f0b);
                else {
                    constexpr int I = slot_index(S, NRI, PPW);
                    dma_piece(I, dst);
                    if constexpr (I == PPW - 1) ++kt;
                }
            });
            rb = nb;
        }
        for (; t < nt; ++t) {
            const int nb = rb + 1 == STAGES ? 0 : rb + 1;
            const char* st = smem + rb * STAGE;
            const unsigned so = (unsigned)(rb * STAGE), son = (unsigned)(nb * STAGE);
            __builtin_amdgcn_s_waitcnt(LGKM0);
            phase(std::integral_constant<int, NRI>{}, f0a, f0b, [&](auto sc) __attribute__((always_inline)) { read_r(sc, KS1, st, so, f1a, f1b); });
            if (t + 1 < nt) {
                __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM(0));
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                phase(std::integral_constant<int, NRI>{}, f1a, f1b, [&](auto sc) __attribute__((always_inline)) { read_r(sc, KS0, smem + nb * STAGE, son, f0a, f0b); });
            } else {
                __builtin_amdgcn_s_waitcnt(LGKM0);
                phase(std::integral_constant<int, 0>{}, f1a, f1b, [](auto) {});
            }
            rb = nb;
        }
        // every wave has left the k-loop -> the stages are free: start the next tile's pipeline, then write this tile out
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int mw = m0 + wm * (32 * WM), nw = n0 + wn * (32 * WN);
        bool more;
        if constexpr (SK) {
            pos += nt;
            more = pos < pend;
            if (more) {
                nt = min(pend - pos, ntf);
                order.lid_origin(pos / ntf, m0, n0);
                plan(m0, n0, 0);
            }
        } else if constexpr (ONESHOT) {
            more = false;                 // one tile per block (grouped launch): no next-tile state to carry through the epilogue
        } else {
            bid += grid;
            more = order.has_tile(bid);
            if (more) {
                order.tile_origin(bid, m0, n0);
                plan(m0, n0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int s = 0; s < STAGES; ++s) issue(s);
        }
        gemm16_epilogue_side<WM, WN, ACC != 0, true, ACC == 1, ONESHOT>(p, acc, accX_unused, reinterpret_cast<float*>(smem + STAGES * STAGE) + wave * 512,
                                                               mw, nw, lane, amx);
        if (!more) break;
    }
    if (p.amax_out)
        gemm16_amax_flush(static_cast<unsigned int*>(p.amax_out), amx, reinterpret_cast<float*>(smem + STAGES * STAGE), wave, lane,
                          NWM * NWN);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same kernel body on v_mfma_f32_16x16x32_f16 (dupl_gemm16_desc.tile 26; gemm_f16x3_km_body is tile 24).  Unchanged: the template
// switches, the 256 x 128 block tile on 8 waves of 64 x 64, the stage size and the ring (DMA STAGES k-tiles ahead, one counted vmcnt +
// s_barrier per k-tile, vmcnt(0) in front of every other barrier), TileOrder, the stream-K slice rules, the k_valid clamp and every
// descriptor field.  What changes, for the reason given at gemm_f16x3_ring16_kernel (the clock the chip holds under this loop):
//   * 4 x 4 accumulators of f32x4 (the same 64 registers); a k-tile (32) is ONE MFMA k-step of 48 instructions, per accumulator hi.hi,
//     hi.lo, lo.hi.  Only the order of the sums inside a k-tile differs from the 32x32x16 body (32 products per MFMA, not 2 x 16).
//   * a k-contiguous operand lies as in gemm_f16x3_ring16_kernel: 16-row x 64-byte pieces, chunk j of row r at j ^ ((4 - (r >> 2)) & 3),
//     a fragment = one ds_read_b128 of a whole piece.
//   * a k-major operand lies in the [16 k][16 rows] 512-byte subtiles of split_frag.h (km16_*): plane image = subtile jj * (rows / 16) +
//     dt, subtile row 4 g + i = k 8 g + 4 jj + i, rows 16 dt .. + 15; DMA piece q = subtiles 2 q, 2 q + 1 (64 contiguous bytes of 16
//     k-rows).  A fragment = two ds_read_b64_tr_b16 (jj = 0, 1) at lane * 8: one contiguous subtile each, conflict-free.
//   * schedule (gemm_f16x3_ring16_kernel's): the B fragments of a k-tile are held through it, the A fragments go in two phases of two
//     row blocks, double-buffered -- 64 fragment registers.  Phase 0 runs over the reads of the tile's last B column block and of
//     A(phase 1); then the counted wait and the barrier (tile t + 1 landed, every wave done reading tile t); phase 1 walks its column
//     blocks in order and under block j reads A(phase 0) (j = 0) / B column block j - 1 (in place) of tile t + 1, and issues the DMA of
//     tile t + STAGES into tile t's stage.  The stream is written out and pinned slot by slot as in gemm_f16x3_km_body; every wait for
//     an inline-asm read carries the fragments it releases (split_frag.h).
template <int WM, int WN, int NWM, int NWN, int WPS, bool SK, int ACC, bool AKM, bool BKM, int STAGES = 3, bool ONESHOT = false, int EPI = EPI_GENERIC>
__device__ __forceinline__ void gemm_f16x3_km16_body(const dupl_gemm16_desc& p, const int g_gm, const int bid0, const int grid) {
    using G = RingGeom<WM, WN, NWM, NWN>;
    constexpr int BM = G::BM, BN = G::BN, NW = G::NW, PA = G::PA, PB = G::PB, STAGE = G::STAGE, PPW = G::PPW;
    constexpr int APW = 2 * PA / NW;                       // this wave's first APW pieces belong to A, the rest to B
    constexpr int RB = 2 * WM, CB = 2 * WN;                // 16 x 16 blocks of the wave tile
    constexpr int NDA = AKM ? 2 : 1, NDB = BKM ? 2 : 1;    // LDS read instructions per fragment
    constexpr int NLA = 4 * NDA, NLB = 2 * NDB;            // ... per A phase set (hi / lo of two row blocks) and per B column block (hi, lo)
    constexpr int SIDE = NW * 2048;
    static_assert(RB == 4 && CB == 4, "wave tile 64 x 64: two phases of two row blocks, the 4 x 4 side-buffer epilogue");
    static_assert((2 * PA) % NW == 0, "pieces must divide over the waves, operand by operand");
    static_assert(STAGES * STAGE + SIDE <= 160 * 1024, "LDS");
    static_assert(STAGES <= G16_PROLOGUE, "the prologue fills every stage before it looks at the piece's length");
    static_assert(!SK || ACC == 1, "stream-K pieces meet in atomics");
    __shared__ __attribute__((aligned(1024))) char smem[STAGES * STAGE + SIDE];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
    const int ntf = p.K / TBK;                    // k-steps of a whole tile, >= STAGES (host)
    int nt = ntf;
    const TileOrder<BM, BN> order(nbm, nbn, g_gm);

    // ---- DMA plan: as gemm_f16x3_km_body, with the images described above
    const int ka_valid = p.ka_valid > 0 ? p.ka_valid : p.K, kb_valid = p.kb_valid > 0 ? p.kb_valid : p.K;
    // (bytes per k-row, read once: in the grouped kernel the descriptor is an indexed element of the argument block, and a scalar
    // load inside the k-loop waits, with lgkmcnt, for every LDS read in flight)
    const unsigned lda2 = __builtin_amdgcn_readfirstlane(p.lda * 2), ldb2 = __builtin_amdgcn_readfirstlane(p.ldb * 2);
    const char* gp[PPW];
    int prow[PPW];
    int kt = 0;                                   // next k-tile to fetch
    auto plan = [&](const int m0, const int n0, const int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int g = wave + NW * i;
            const bool isA = i < APW;
            const int gg = isA ? g : g - 2 * PA;
            const int PO = isA ? PA : PB;
            const bool lo = gg >= PO;
            const int q = lo ? gg - PO : gg;
            const __half* plane = static_cast<const __half*>(isA ? (lo ? p.A_lo : p.A_hi) : (lo ? p.B_lo : p.B_hi));
            const int ld = isA ? p.lda : p.ldb, r0 = isA ? m0 : n0, R = isA ? p.M : p.N;
            const bool km = isA ? AKM : BKM;
            if (!km) {
                const int pr = lane >> 2;
                const int jsrc = (lane & 3) ^ ((4 - (pr >> 2)) & 3);
                const int row = min(r0 + q * 16 + pr, R - 1);
                gp[i] = reinterpret_cast<const char*>(plane + (size_t)row * ld + (size_t)k0 * TBK) + jsrc * 16;
                prow[i] = 0;
            } else {
                const int NPH = (isA ? BM : BN) / 32;                    // pieces per half jj of the plane image
                const int jj = q / NPH, dp = q - jj * NPH;               // piece q = subtiles (jj, dt = 2 dp), (jj, 2 dp + 1)
                const int col = min(r0 + dp * 32 + km16_piece_col_bytes(0, lane) / 2, R - 8);      // R % 8 == 0 (host): the last whole chunk
                gp[i] = reinterpret_cast<const char*>(plane + col);
                prow[i] = km16_piece_row(jj << 1, lane);                 // k-row inside the k-tile, 0 .. 31
            }
        }
        kt = k0;
    };
    auto dma_piece = [&](const int i, char* dst) __attribute__((always_inline)) {
        const bool km = (i < APW) ? AKM : BKM;
        if (!km) g16_dma_piece(gp[i], dst + i * (NW * 1024));
        else {
            const int kv = (i < APW) ? ka_valid : kb_valid;
            const int krow = min(kt * TBK + prow[i], kv - 1);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp[i] + (size_t)krow * ((i < APW) ? lda2 : ldb2)),
                                             (__attribute__((address_space(3))) void*)(dst + i * (NW * 1024)), 16, 0, 0);
        }
    };
    auto issue = [&](int buf) __attribute__((always_inline)) {
        char* dst = smem + buf * STAGE + wave * 1024;
#pragma unroll
        for (int i = 0; i < PPW; ++i) dma_piece(i, dst);
        ++kt;
    };

    // ---- fragment addresses (bytes inside a stage)
    const int l15 = lane & 15;
    const int ch = ((lane >> 4) ^ ((4 - (l15 >> 2)) & 3)) * 16;
    const int a_off = (wm * (32 * WM) + l15) * 64 + ch, b_off = 2 * PA * 1024 + (wn * (32 * WN) + l15) * 64 + ch;
    const unsigned lds0 = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)smem);      // LDS byte address of stage 0
    const unsigned akm0 = lds0 + km16_read_lane_off(lane) + wm * RB * 512, bkm0 = lds0 + 2 * PA * 1024 + km16_read_lane_off(lane) + wn * CB * 512;

    f32x4 acc[RB][CB];
    // fragments as 4-half halves, [2 f], [2 f + 1] = k 0..3 / 4..7 of the lane's 8.  A sets (one per phase): f = {hi rb 0, hi rb 1, lo rb 0,
    // lo rb 1} of the phase's two row blocks; B: f = column block (hi), CB + column block (lo)
    h4 fa0[8], fa1[8], fb[4 * CB];
    auto tr_off = [](const unsigned addr, auto offc) __attribute__((always_inline)) { return km_tr_read<decltype(offc)::value>(addr); };
    // RI-th LDS read instruction of the A set of phase PH / of column block J; st = stage pointer, so = its byte offset
    auto read_a = [&](auto ric, auto phc, const char* st, const unsigned so, h4(&fa)[8]) __attribute__((always_inline)) {
        constexpr int RI = decltype(ric)::value, PH = decltype(phc)::value;
        constexpr int f = RI / NDA, half = RI % NDA, pl = f >> 1, rbk = 2 * PH + (f & 1);
        if constexpr (!AKM) {
            const h8 v = *reinterpret_cast<const h8*>(st + pl * (PA * 1024) + a_off + rbk * 1024);
            fa[2 * f] = __builtin_shufflevector(v, v, 0, 1, 2, 3);
            fa[2 * f + 1] = __builtin_shufflevector(v, v, 4, 5, 6, 7);
        } else {
            fa[2 * f + half] = tr_off(akm0 + so, std::integral_constant<int, pl * (PA * 1024) + (half * (BM / 16) + rbk) * 512>{});
        }
    };
    auto read_b = [&](auto ric, auto jc, const char* st, const unsigned so) __attribute__((always_inline)) {
        constexpr int RI = decltype(ric)::value, J = decltype(jc)::value;
        constexpr int pl = RI / NDB, half = RI % NDB, f = pl * CB + J;
        if constexpr (!BKM) {
            const h8 v = *reinterpret_cast<const h8*>(st + pl * (PB * 1024) + b_off + J * 1024);
            fb[2 * f] = __builtin_shufflevector(v, v, 0, 1, 2, 3);
            fb[2 * f + 1] = __builtin_shufflevector(v, v, 4, 5, 6, 7);
        } else {
            fb[2 * f + half] = tr_off(bkm0 + so, std::integral_constant<int, pl * (PB * 1024) + (half * (BN / 16) + J) * 512>{});
        }
    };
    auto frag = [](const h4 lo, const h4 hi) __attribute__((always_inline)) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); };
    // n-th MFMA of column block J in phase PH: its two accumulators, main, then hi x lo, then lo x hi
    auto mfma_n = [&](auto phc, auto jc, auto nc, const h4(&fa)[8]) __attribute__((always_inline)) {
        constexpr int PH = decltype(phc)::value, J = decltype(jc)::value, n = decltype(nc)::value, pass = n / 2, k = n % 2;
        constexpr int af = pass == 2 ? 2 + k : k, bf = pass == 1 ? CB + J : J;
        acc[2 * PH + k][J] = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag(fa[2 * af], fa[2 * af + 1]), frag(fb[2 * bf], fb[2 * bf + 1]),
                                                                    acc[2 * PH + k][J], 0, 0, 0);
    };
    // A column block = 6 MFMAs with NS load slots spread evenly between them IN THIS ORDER (slot s, then its share of the MFMAs): the
    // stream is written out and pinned (sched_barrier(0)), since issue-order hints cannot see the inline-asm reads
    constexpr int NMB = 6;
    auto block = [&](auto phc, auto jc, auto nsc, const h4(&fa)[8], auto&& slot) __attribute__((always_inline)) {
        constexpr int NS = decltype(nsc)::value;
        if constexpr (NS == 0) {
            static_for<NMB>([&](auto nc) __attribute__((always_inline)) { mfma_n(phc, jc, nc, fa); });
        } else {
            static_for<NS>([&](auto sc) __attribute__((always_inline)) {
                constexpr int S = decltype(sc)::value, n0 = S * NMB / NS, n1 = (S + 1) * NMB / NS;
                slot(sc);
                static_for<n1 - n0>([&](auto kc) __attribute__((always_inline)) { mfma_n(phc, jc, std::integral_constant<int, n0 + decltype(kc)::value>{}, fa); });
                __builtin_amdgcn_sched_barrier(0);
            });
        }
    };
    // waits for inline-asm reads: lgkmcnt(0) with the released fragments as in / out operands (an MFMA is no memory operation)
    auto wait_a = [](h4(&f)[8]) __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]) : : "memory");
    };
    auto pin4 = [](h4& a, h4& b, h4& c, h4& d) __attribute__((always_inline)) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : : "memory"); };
    auto pin_b = [&](auto jc) __attribute__((always_inline)) {      // (behind a wait: carries column block J's four halves)
        constexpr int J = decltype(jc)::value;
        pin4(fb[2 * J], fb[2 * J + 1], fb[2 * (CB + J)], fb[2 * (CB + J) + 1]);
    };
    constexpr std::integral_constant<int, 0> P0{};
    constexpr std::integral_constant<int, 1> P1{};
    constexpr std::integral_constant<int, CB - 1> JL{};
    // One k-tile in stage rb.  On entry the reads of A(phase 0) and of B column blocks 0 .. CB - 2 are in flight.  LOAD: tile t + 1 (stage
    // nb) follows; DMA: tile t + STAGES is fetched into stage rb; VM: the vmcnt of the mid-tile wait.
    auto k_tile = [&](auto loadc, auto dmac, auto vmc, const int rb, const int nb) __attribute__((always_inline)) {
        constexpr bool LOAD = decltype(loadc)::value, DMA = decltype(dmac)::value;
        const char* st = smem + rb * STAGE;
        const char* nx = smem + nb * STAGE;
        const unsigned so = (unsigned)(rb * STAGE), son = (unsigned)(nb * STAGE);
        wait_a(fa0);
        static_for<CB - 1>([&](auto jc) __attribute__((always_inline)) { pin_b(jc); });
        __builtin_amdgcn_sched_barrier(0);
        // phase 0: the last B column block, then A(phase 1), under the first CB - 1 column blocks
        constexpr int NL0 = NLB + NLA;
        static_for<CB - 1>([&](auto jc) __attribute__((always_inline)) {
            constexpr int J = decltype(jc)::value, L0 = J * NL0 / (CB - 1), L1 = (J + 1) * NL0 / (CB - 1);
            block(P0, jc, std::integral_constant<int, L1 - L0>{}, fa0, [&](auto sc) __attribute__((always_inline)) {
                constexpr int L = L0 + decltype(sc)::value;
                if constexpr (L < NLB) read_b(std::integral_constant<int, L>{}, JL, st, so);
                else read_a(std::integral_constant<int, L - NLB>{}, P1, st, so, fa1);
            });
        });
        wait_a(fa1);
        pin_b(JL);
        __builtin_amdgcn_sched_barrier(0);
        block(P0, JL, std::integral_constant<int, 0>{}, fa0, [](auto) {});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (LOAD) {
            // every read of stage rb has returned (above); my pieces of tile t + 1 landed; everyone's, and everyone done with stage rb
            __builtin_amdgcn_s_waitcnt(WAIT_LGKM0_VM(decltype(vmc)::value));
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        // phase 1
        char* dst = smem + rb * STAGE + wave * 1024;
        static_for<CB>([&](auto jc) __attribute__((always_inline)) {
            constexpr int J = decltype(jc)::value;
            constexpr int D0 = DMA ? J * PPW / CB : 0, D1 = DMA ? (J + 1) * PPW / CB : 0;      // this block's DMA pieces
            constexpr int NRD = LOAD ? (J == 0 ? NLA : NLB) : 0;
            block(P1, jc, std::integral_constant<int, NRD + (D1 - D0)>{}, fa1, [&](auto sc) __attribute__((always_inline)) {
                constexpr int S = decltype(sc)::value;
                if constexpr (S < NRD) {
                    if constexpr (J == 0) read_a(sc, P0, nx, son, fa0);
                    else read_b(sc, std::integral_constant<int, J - 1>{}, nx, son);
                } else {
                    constexpr int I = D0 + S - NRD;
                    dma_piece(I, dst);
                    if constexpr (I == PPW - 1) ++kt;
                }
            });
        });
        __builtin_amdgcn_sched_barrier(0);
    };

    int bid = bid0;
    int pos = 0, pend = 0;
    int m0, n0;
    if constexpr (SK) {
        const int T = order.nblk * ntf, G = grid;
        if (p.sk_slices > 0) {
            // aligned k-slices: see gemm_f16x3_km_body
            const int S = p.sk_slices, nblk = order.nblk, U = nblk * S;
            const int xcd = bid & 7, idx = bid >> 3;
            const int ulo = (int)((long)U * xcd / 8), uhi = (int)((long)U * (xcd + 1) / 8);
            if (idx >= uhi - ulo) return;
            const int u = ulo + idx;
            const int slice = u / nblk, lid = u - slice * nblk;
            const int per = (ntf + S - 1) / S;
            const int k0 = slice * per;
            nt = min(per, ntf - k0);            // >= G16_PROLOGUE for every slice (host)
            pos = lid * ntf + k0;
            pend = pos + nt;
            order.lid_origin(lid, m0, n0);
            plan(m0, n0, k0);
        } else {
            const int L = (bid & 7) * (G >> 3) + (bid >> 3);
            auto cut = [&](const int l) {
                int x = (int)((long)T * l / G);
                const int r = x % ntf;
                if (r && r < G16_PROLOGUE) x -= r;
                else if (r > ntf - G16_PROLOGUE) x += ntf - r;
                return x;
            };
            pos = cut(L);
            pend = cut(L + 1);
            if (pos >= pend) return;
            const int lid = pos / ntf, k0 = pos - lid * ntf;
            nt = min(pend - pos, ntf - k0);
            order.lid_origin(lid, m0, n0);
            plan(m0, n0, k0);
        }
    } else if constexpr (ONESHOT) {
        if (bid >= order.nblk) return;       // grouped launch: bid0 IS the tile's position in this problem's grouped order
        order.lid_origin(bid, m0, n0);
        plan(m0, n0, 0);
    } else {
        if (!order.has_tile(bid)) return;
        order.tile_origin(bid, m0, n0);
        plan(m0, n0, 0);
    }
#pragma unroll
    for (int s = 0; s < STAGES; ++s) issue(s);
    bool first = true;
    float amx = 0.f;
    for (;;) {
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (first) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 1) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        first = false;
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        static_for<NLA>([&](auto rc) __attribute__((always_inline)) { read_a(rc, P0, smem, 0u, fa0); });
        static_for<CB - 1>([&](auto jc) __attribute__((always_inline)) {
            static_for<NLB>([&](auto rc) __attribute__((always_inline)) { read_b(rc, jc, smem, 0u); });
        });
        __builtin_amdgcn_sched_barrier(0);
        int rb = 0;
        int t = 0;
        for (; t + STAGES < nt; ++t) {
            const int nb = rb + 1 == STAGES ? 0 : rb + 1;
            k_tile(std::true_type{}, std::true_type{}, std::integral_constant<int, (STAGES - 2) * PPW>{}, rb, nb);
            rb = nb;
        }
        for (; t + 1 < nt; ++t) {
            const int nb = rb + 1 == STAGES ? 0 : rb + 1;
            k_tile(std::true_type{}, std::false_type{}, std::integral_constant<int, 0>{}, rb, nb);
            rb = nb;
        }
        k_tile(std::false_type{}, std::false_type{}, std::integral_constant<int, 0>{}, rb, rb);
        // every wave has left the k-loop -> the stages are free: start the next tile's pipeline, then write this tile out
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int mw = m0 + wm * (32 * WM), nw = n0 + wn * (32 * WN);
        bool more;
        if constexpr (SK) {
            pos += nt;
            more = pos < pend;
            if (more) {
                nt = min(pend - pos, ntf);
                order.lid_origin(pos / ntf, m0, n0);
                plan(m0, n0, 0);
            }
        } else if constexpr (ONESHOT) {
            more = false;                 // one tile per block (grouped launch)
        } else {
            bid += grid;
            more = order.has_tile(bid);
            if (more) {
                order.tile_origin(bid, m0, n0);
                plan(m0, n0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int s = 0; s < STAGES; ++s) issue(s);
        }
        gemm16_epilogue_side16<ACC != 0, ACC == 1, ONESHOT, EPI>(p, acc, reinterpret_cast<float*>(smem + STAGES * STAGE) + wave * 512, mw, nw, lane, amx);
        if (!more) break;
    }
    if (p.amax_out)
        gemm16_amax_flush(static_cast<unsigned int*>(p.amax_out), amx, reinterpret_cast<float*>(smem + STAGES * STAGE), wave, lane,
                          NWM * NWN);
}

// MF: the MFMA shape of the body, 32 (32x32x16, gemm_f16x3_km_body) or 16 (16x16x32, gemm_f16x3_km16_body)
// EPI: the epilogue form of the 16x16x32 body's full-epilogue launches (EPI_D / EPI_A: gemm16_epilogue_side16)
template <int WM, int WN, int NWM, int NWN, int WPS, bool SK, int ACC, bool AKM, bool BKM, int STAGES = 3, int MF = 32, int EPI = EPI_GENERIC>
__global__ __launch_bounds__(64 * NWM * NWN, WPS) void gemm_f16x3_km_kernel(const dupl_gemm16_desc p, const int g_gm) {
    static_assert(MF == 16 || MF == 32, "MFMA shape");
    static_assert(EPI == EPI_GENERIC || (MF == 16 && ACC == 0), "forms: the 16x16x32 body's C = ... launches");
    if constexpr (MF == 16) gemm_f16x3_km16_body<WM, WN, NWM, NWN, WPS, SK, ACC, AKM, BKM, STAGES, false, EPI>(p, g_gm, blockIdx.x, gridDim.x);
    else gemm_f16x3_km_body<WM, WN, NWM, NWN, WPS, SK, ACC, AKM, BKM, STAGES>(p, g_gm, blockIdx.x, gridDim.x);
}

// Grouped weight gradients (round 4): the four dW of one transformer block -- 2304 x 768, 768 x 768, 3072 x 768, 768 x 3072, each
// only 18 .. 72 tiles of 256 x 128 -- as ONE launch of 216 tiles: every block owns a whole tile and walks all of K (the token
// axis: 99 k-steps at 4 images), so nothing is split, nothing meets in atomics (C += tile by the one owner: the same bits in
// deterministic mode and out of it), the 3-stage prologue and the epilogue are paid once per 99 k-steps instead of once per
// ~14 (stream-K pieces), and the tile count does not depend on the batch.  Problem i owns the tiles [first[i], first[i + 1]) of
// one list, which the kernel deals to the XCDs in contiguous eighths (round 5).
struct g16_group_args {
    dupl_gemm16_desc d[DUPL_GEMM16_GROUP_MAX];
    int first[DUPL_GEMM16_GROUP_MAX + 1];
    int n;
};
template <int WM, int WN, int NWM, int NWN, int WPS, int MF = 32>
__global__ __launch_bounds__(64 * NWM * NWN, WPS) void gemm_f16x3_km_group_kernel(const g16_group_args g, const int g_gm) {
    // tile list = problem after problem, each in its grouped order (g_gm row tiles x all column tiles per group); XCD x (= blockIdx % 8)
    // takes the x-th eighth of the LIST: ~27 consecutive tiles of (mostly) one problem = 4-5 row tiles x all its column tiles, whose dy
    // columns and x columns meet in that XCD's L2 -- round 4 dealt every problem over all 8 XCDs (9 / 9 / 7 / 2 tiles each): every XCD
    // fetched nearly all of every x and a band of every dy, 487 MB of fabric traffic per launch for 183 MB of operands
    const int T = g.first[g.n];
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int lo = (int)((long)T * xcd / 8), hi = (int)((long)T * (xcd + 1) / 8);
    if (idx >= hi - lo) return;
    const int t = lo + idx;
    int i = 0;
#pragma unroll 1
    while (i + 1 < g.n && t >= g.first[i + 1]) ++i;
    i = __builtin_amdgcn_readfirstlane(i);
    // one tile per block: a step of the whole grid ends the persistent walk after the first tile
    if constexpr (MF == 16) gemm_f16x3_km16_body<WM, WN, NWM, NWN, WPS, false, 2, true, true, 3, true>(g.d[i], g_gm, t - g.first[i], 1 << 28);
    else gemm_f16x3_km_body<WM, WN, NWM, NWN, WPS, false, 2, true, true, 3, true>(g.d[i], g_gm, t - g.first[i], 1 << 28);
}

}  // namespace

// Launch tuning travels in the descriptor (dupl_gemm16_desc.tile / concurrency / persist_blocks / group; 0 = these defaults):
// nothing about kernel selection is process-global, the library is re-entrant per call.
constexpr int G16_GROUP_M = 8;      // 128-row tile kernels
constexpr int G16_GROUP_RING = 2;   // row tiles (256 rows) per group of the ring kernels' block order: 512-row A bands stay in an
                                    // XCD's L2 while it sweeps the columns (2 / 3: 320, 4: 312, 8: 304, 16: 285 TF/s-eq on 15696 x 3072 x 768)
constexpr int G16_F1_BIG_FROM = 96; // format 1: 256 x 256 tiles from this many of them

// dupl_gemm16_desc.tile: the codes dupl_gemm_f16x3 accepts
constexpr int G16_TILES[] = {
    0,    // the launcher's choice
    3,    // gemm_f16x3_kernel, 128 x 64 on 4 waves; format 0, split-K
    5,    // gemm_f16x3_kernel, 128 x 128 on 8 waves; format 0, split-K
    6,    // gemm_f16x3_ring_kernel, 256 x 128 on 8 waves; format 0, one block per tile
    7,    // gemm_f16x3_ring_kernel, 256 x 128 on 4 waves; format 0, one block per tile
    8,    // gemm_f16x3_ring_kernel SINGLE, 256 x 256 on 8 waves; format 1, one block per tile
    10,   // gemm_f16x3_pring_kernel, 256 x 128; format 0, persistent
    11,   // gemm_f16x3_pring_kernel SK, 256 x 128; format 0, stream-K for DUPL_GEMM_ACCUM
    12,   // gemm_f16x3_ring_kernel SINGLE, 256 x 128; format 1, one block per tile
    14,   // gemm_f16x3_pring_kernel SINGLE, 256 x 128; format 1, persistent
    18,   // gemm_f16x3_ring16_kernel, 256 x 256; format 1 on the 16x16x32 MFMA, one block per tile
    22,   // gemm_f16x3_ring16_kernel, 256 x 128; format 1 on the 16x16x32 MFMA, one block per tile
    24,   // k-major launches (single and grouped): gemm_f16x3_km_body, the 32x32x16 MFMA; any other launch: as 0
    26,   // k-major launches (single and grouped): gemm_f16x3_km16_body, the 16x16x32 MFMA; any other launch: as 0
    28,   // as 18 with the generic epilogue walk forced (EPI_GENERIC): the A/B partner of the epilogue forms
    30,   // as 22 with the generic epilogue walk forced
    32,   // as 26 with the generic epilogue walk forced
};
// A code resolved, once, into what it asks for
struct g16_tile_t {
    int family;     // the kernel of a k-contiguous launch (3 .. 22 above); 0 = the launcher's choice.  k-major launches do not look at it
    bool forms;     // false: the generic epilogue walk forced
    int km_body;    // the MFMA body of a k-major launch, 16 or 32; 0 = the launcher's choice per instantiation (KM16_* below)
};
static g16_tile_t g16_resolve_tile(const int code) {
    switch (code) {
        case 24: return {0, true, 32};
        case 26: return {0, true, 16};
        case 28: return {18, false, 0};
        case 30: return {22, false, 0};
        case 32: return {0, false, 16};
        default: return {code, true, 0};
    }
}
// all kernels of dupl_gemm_f16x3 share one signature: a choice of kernel is a pointer
using g16_kernel_t = void (*)(dupl_gemm16_desc, int);

// The k-major launches' automatic choice of the body (dupl_gemm16_desc.tile 0): per instantiation, the 16x16x32 body only where the
// stand-alone A/B on the step's own shapes shows it faster (profiles/kmajor16_bodies.txt).  The whole-tile weight gradients (single
// launch in deterministic mode, grouped launch) switch together: they carry the same bits.
// (us per launch, median of 5 interleaved rounds, one stream / next to the same launch on a second stream; 32x32x16 -> 16x16x32)
constexpr bool KM16_DGRAD_EPI = true;       // data gradient, full epilogue: 3140 x 3072 x 768 dgelu + amax 74.8 -> 72.4 / 117.2 -> 106.6; 3140 x 768 x 768 amax 31.8 -> 31.3 / 32.9 -> 32.9
constexpr bool KM16_DGRAD_SK = true;        // stream-K data gradient: 3140 x 768 x 3072 60.2 -> 56.6 / 102.4 -> 93.1; 3140 x 768 x 2304 51.2 -> 48.5 / 82.4 -> 76.4
constexpr bool KM16_WGRAD_SK = false;       // stream-K weight gradient: not in the step, not measured -- stays on the 32x32x16 body
constexpr bool KM16_WGRAD_TILE = true;      // whole-tile weight gradients: a block's four at K = 3168, grouped, 121.7 -> 112.5 / 239.8 -> 224.9
static bool g16_km16(const g16_tile_t& t, const bool automatic) { return t.km_body ? t.km_body == 16 : automatic; }
// The k-major kernels (256 x 128, persistent, 3 stages) by body and epilogue form; the forms exist for the full-epilogue data gradient on
// the 16x16x32 body only
template <bool SK, int ACC, bool AKM, bool BKM>
static g16_kernel_t g16_km_kernel(const bool km16, const int epi = EPI_GENERIC) {
    if (!km16) return gemm_f16x3_km_kernel<2, 2, 4, 2, 2, SK, ACC, AKM, BKM, 3, 32>;
    if constexpr (!SK && ACC == 0) {
        if (epi == EPI_D) return gemm_f16x3_km_kernel<2, 2, 4, 2, 2, SK, ACC, AKM, BKM, 3, 16, EPI_D>;
        if (epi == EPI_A) return gemm_f16x3_km_kernel<2, 2, 4, 2, 2, SK, ACC, AKM, BKM, 3, 16, EPI_A>;
    }
    return gemm_f16x3_km_kernel<2, 2, 4, 2, 2, SK, ACC, AKM, BKM, 3, 16>;
}

// The epilogue forms (EPI_*): the launcher matches flags, pointers and c_rows of a descriptor against the forms the step launches and takes
// the specialised instantiation where the stand-alone A/B on the step's own shapes shows it faster or equal (tools/gemm16_bench with
// tile 18 / 22 / 26 against 28 / 30 / 32, the same bodies with EPI_GENERIC forced; profiles/epilogue_forms.txt).  Everything else, the
// ablation builds and the forced codes run the generic walk.
// (us per launch, median of 5 interleaved rounds, one stream / next to the same launch on a second stream; GENERIC -> form)
constexpr bool EPI_USE_P = true;        // bias -> planes: 15696 x 2304 x 768 189.1 -> 164.9 / 311.9 -> 289.4; 6280 x 2304 x 768 66.0 -> 60.6 / 124.8 -> 114.0
constexpr bool EPI_USE_G = true;        // bias, pre, GELU -> planes: 15696 x 3072 x 768 241.3 -> 234.7 / 492.7 -> 461.3; 6280 x 3072 x 768 136.2 -> 122.4 / 191.5 -> 179.9
constexpr bool EPI_USE_R = true;        // bias + residual -> fp32: 15696 x 768 x 3072 211.0 -> 203.1 / 384.0 -> 370.3; 15696 x 768 x 768 65.4 -> 57.2 / 127.6 -> 110.6;
                                        // on the 256 x 128 tile 6280 x 768 x 3072 92.4 -> 90.8 / 159.3 -> 155.3; 6280 x 768 x 768 31.6 -> 29.1 / 51.3 -> 48.2
constexpr bool EPI_USE_D = true;        // gelu' + amax: 3140 x 3072 x 768 73.6 -> 61.5 / 110.4 -> 100.3
constexpr bool EPI_USE_A = true;        // amax: 3140 x 768 x 768 31.4 -> 26.8 / 33.0 -> 29.2
static int g16_epi_form(const dupl_gemm16_desc& d) {       // the k-contiguous format 1 forward (gemm_f16x3_ring16_kernel, NP = 3)
    if (G16_ABL) return EPI_GENERIC;
    if (d.C_hi && !d.C && !d.res) {
        if (d.flags == 0) return EPI_USE_P ? EPI_P : EPI_GENERIC;
        if ((d.flags & ~DUPL_GEMM_STORE_PRE) == DUPL_GEMM_GELU) return EPI_USE_G ? EPI_G : EPI_GENERIC;
    }
    if (d.C && !d.C_hi && d.res && d.flags == 0 && d.c_rows == 0) return EPI_USE_R ? EPI_R : EPI_GENERIC;
    return EPI_GENERIC;
}
static int g16_epi_form_km(const dupl_gemm16_desc& d) {    // the full-epilogue data gradient on the 16x16x32 body
    if (G16_ABL || !d.C || d.C_hi || d.res || d.bias || d.c_rows) return EPI_GENERIC;
    if (d.flags == DUPL_GEMM_MUL_DGELU) return EPI_USE_D ? EPI_D : EPI_GENERIC;
    if (d.flags == 0) return EPI_USE_A ? EPI_A : EPI_GENERIC;
    return EPI_GENERIC;
}

extern "C" int dupl_split_f16x2(const float* x, void* hi, void* lo, int64_t n, dupl_stream_t stream) {
    if (!x || !hi || !lo || n <= 0 || (n & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(hi) & 7) ||
        (reinterpret_cast<uintptr_t>(lo) & 7))
        return DUPL_ERR_ARG;
    const long n4 = n / 4;
    long g = (n4 + 255) / 256;
    if (g > 8192) g = 8192;
    DUPL_LAUNCH(split_kernel<false>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, (__half*)hi, (__half*)lo, n4, 1.f);
    return dupl_launch_status();
}

extern "C" int dupl_split_f16x2b(const float* x, void* hi, void* lo, int64_t n, int32_t scale_exp, dupl_stream_t stream) {
    if (!x || !hi || !lo || n <= 0 || (n & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(hi) & 7) ||
        (reinterpret_cast<uintptr_t>(lo) & 7) || scale_exp < 0 || scale_exp > 15)
        return DUPL_ERR_ARG;
    const long n4 = n / 4;
    long g = (n4 + 255) / 256;
    if (g > 8192) g = 8192;
    DUPL_LAUNCH(split_kernel<true>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, (__half*)hi, (__half*)lo, n4,
                       ldexpf(1.f, scale_exp));
    return dupl_launch_status();
}

// What dupl_gemm_f16x3 and dupl_gemm_f16x3_group require of a descriptor alike: the operands and their layout.  (Each entry point adds
// its own conditions on the outputs, the epilogue and the launch tuning.)
static bool g16_operands_ok(const dupl_gemm16_desc& d) {
    if (d.struct_size != sizeof(dupl_gemm16_desc)) return false;      // a caller built against another header
    if (!d.A_hi || !d.A_lo || !d.B_hi || !d.B_lo || d.M <= 0 || d.N <= 0 || d.K <= 0) return false;
    if ((d.K % TBK) || (d.lda % 8) || (d.ldb % 8)) return false;       // whole 16-byte chunks, whole k-tiles
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!al16(d.A_hi) || !al16(d.A_lo) || !al16(d.B_hi) || !al16(d.B_lo)) return false;
    if (d.group < 0 || d.group > 4096) return false;
    if (d.a_layout < 0 || d.a_layout > 1 || d.b_layout < 0 || d.b_layout > 1 || d.ka_valid < 0 || d.kb_valid < 0) return false;
    if (d.a_layout || d.b_layout) {
        // k-major operand(s): format 1 planes, the 3-stage prologue, whole 16-byte chunks of rows, k_valid of a k-major operand only
        if (d.fmt != 1 || d.K / TBK < G16_PROLOGUE) return false;
        if ((d.a_layout && (d.M & 7)) || (d.b_layout && (d.N & 7))) return false;
        if (d.ka_valid > d.K || d.kb_valid > d.K) return false;
        if ((!d.a_layout && d.ka_valid) || (!d.b_layout && d.kb_valid)) return false;
    }
    return true;
}

extern "C" int dupl_gemm_f16x3_group(const dupl_gemm16_desc* descs, int32_t n, dupl_stream_t stream) {
    if (!descs || n < 1 || n > DUPL_GEMM16_GROUP_MAX) return DUPL_ERR_ARG;
    g16_group_args g;
    g.n = n;
    int total = 0, group = 0, tile = 0;
    for (int i = 0; i < n; ++i) {
        const dupl_gemm16_desc& d = descs[i];
        if (!g16_operands_ok(d)) return DUPL_ERR_ARG;
        // a weight gradient on the forward's planes: C += alpha A^T . B, both operands k-major, nothing else (per problem with
        // DUPL_GEMM_C_FRESH: C = that, the owner block does not read C)
        if ((d.flags & ~DUPL_GEMM_C_FRESH) != DUPL_GEMM_ACCUM || d.a_layout != 1 || d.b_layout != 1) return DUPL_ERR_ARG;
        if (!d.C || d.C_hi || d.C_lo || d.bias || d.res || d.c_rows || d.amax_out) return DUPL_ERR_ARG;
        g.d[i] = d;
        g.first[i] = total;
        const int nblk = ((d.M + 255) / 256) * ((d.N + 127) / 128);
        total += nblk;                          // first[] counts TILES: the kernel deals the list to the XCDs in eighths
        if (d.group) group = d.group;
        if (d.tile) tile = d.tile;              // (24 / 26 choose the body; every other code is the library's choice)
    }
    g.first[n] = total;
    const dim3 grid((unsigned)(8 * ((total + 7) / 8)));
    void (*const kernel)(g16_group_args, int) = g16_km16(g16_resolve_tile(tile), KM16_WGRAD_TILE) ? gemm_f16x3_km_group_kernel<2, 2, 4, 2, 2, 16>
                                                                                                  : gemm_f16x3_km_group_kernel<2, 2, 4, 2, 2, 32>;
    DUPL_LAUNCH(kernel, grid, dim3(512), 0, (hipStream_t)stream, g, group ? group : G16_GROUP_RING);
    return dupl_launch_status();
}

// Rows [0, M1) and [M1, M) of a forward launch as two descriptors (rows are independent: each on its own row range of every
// operand).  False when the second part would have nothing to write.
static bool g16_split_rows(const dupl_gemm16_desc& d, const int M1, dupl_gemm16_desc& d1, dupl_gemm16_desc& d2) {
    d1 = d; d2 = d;
    d1.M = M1;
    d2.M = d.M - M1;
    auto adv = [&](const void* q, size_t elems, size_t bytes) { return q ? static_cast<const void*>(static_cast<const char*>(q) + elems * bytes) : nullptr; };
    d2.A_hi = adv(d.A_hi, (size_t)M1 * d.lda, 2); d2.A_lo = adv(d.A_lo, (size_t)M1 * d.lda, 2);
    d2.C = (float*)adv(d.C, (size_t)M1 * d.ldc, 4);
    d2.C_hi = (void*)adv(d.C_hi, (size_t)M1 * d.ldo, 2); d2.C_lo = (void*)adv(d.C_lo, (size_t)M1 * d.ldo, 2);
    d2.res = (const float*)adv(d.res, (size_t)M1 * d.ldr, 4);
    d2.aux = (float*)adv(d.aux, (size_t)M1 * d.ldaux, 4);
    if (d.c_rows > 0) {             // fp32 outputs for the first c_rows rows only
        if (d.c_rows <= M1) {       // ... all of them in part 1: part 2 writes planes only
            d2.c_rows = 0; d2.C = nullptr; d2.aux = nullptr; d2.flags &= ~DUPL_GEMM_STORE_PRE;
        } else { d1.c_rows = 0; d2.c_rows = d.c_rows - M1; }
    }
    return d2.C || d2.C_hi;
}

// ---- dupl_gemm_f16x3 in three steps: g16_check (every refusal), g16_choose (what to launch, as values), and one place that launches.

// 1. Every condition under which dupl_gemm_f16x3 returns DUPL_ERR_ARG.  d: with the stand-in lo planes of products = 1 (`single`).
static bool g16_check(const dupl_gemm16_desc& d, const bool single) {
    if (!g16_operands_ok(d)) return false;
    if (d.products != 0 && d.products != 1 && d.products != 3) return false;      // 0 = 3: the f16x3 kernels
    if (d.concurrency < 0 || d.concurrency > 8 || d.persist_blocks < 0 || d.persist_blocks > 1024 || (d.persist_blocks & 7)) return false;
    bool known_tile = false;
    for (const int t : G16_TILES) known_tile |= d.tile == t;
    if (!known_tile) return false;
    if (!d.C && !d.C_hi) return false;
    if ((d.C_hi == nullptr) != (d.C_lo == nullptr)) return false;
    if ((d.flags & (DUPL_GEMM_STORE_PRE | DUPL_GEMM_MUL_DGELU | DUPL_GEMM_MUL_RELUMASK)) && !d.aux) return false;
    if (d.flags & ~(DUPL_GEMM_GELU | DUPL_GEMM_RELU | DUPL_GEMM_STORE_PRE | DUPL_GEMM_ACCUM | DUPL_GEMM_MUL_DGELU | DUPL_GEMM_MUL_RELUMASK))
        return false;
    const bool kmajor = d.a_layout || d.b_layout, accum = d.flags & DUPL_GEMM_ACCUM;
    if (accum && (!d.C || d.C_hi || d.bias || d.res || d.c_rows)) return false;   // C += alpha * A B^T, nothing else
    if (d.c_rows < 0 || (d.c_rows && (d.flags & (DUPL_GEMM_MUL_DGELU | DUPL_GEMM_MUL_RELUMASK)))) return false;
    if (d.amax_out && (accum || d.c_rows || (reinterpret_cast<uintptr_t>(d.amax_out) & 3))) return false;
    if (d.fmt < 0 || d.fmt > 1 || d.out_exp < 0 || d.out_exp > 15 || (d.out_exp && d.fmt != 1) || (d.fmt == 1 && !kmajor && (accum || d.amax_out)))
        return false;
    if (single && (accum || kmajor)) return false;      // products = 1 is the forward only: k-contiguous operands, C = ...
    if (kmajor) {
        // the three k-major forms: the data gradient with the full epilogue (dy k-contiguous, W k-major); the data gradient with a LINEAR
        // epilogue into a zero-filled dx, stream-K (in deterministic mode the caller takes the one-block-per-tile form instead); the
        // weight gradient (both operands token-major)
        if (!accum && (d.a_layout || !d.b_layout)) return false;
        if (accum && !d.a_layout && (!d.b_layout || d.deterministic)) return false;
        if (accum && d.a_layout && !d.b_layout) return false;
    }
    return true;
}

// 2. What to launch: at most two launches on the stream (the row split of the forward).  A launch passes the caller's descriptor or one of
// the plan's own (`own`: the stream-K descriptor with its slice count resolved, the two parts of a row split).
struct g16_launch_t {
    g16_kernel_t kernel;
    dim3 grid, block;
    int group;                            // the kernels' second argument: row tiles per group of the block -> tile order
    const dupl_gemm16_desc* d;
};
struct g16_plan {
    int n = 0;
    g16_launch_t l[2];
    dupl_gemm16_desc own[2];
    void add(const g16_kernel_t kernel, const dim3 grid, const dim3 block, const int group, const dupl_gemm16_desc* d) {
        l[n++] = g16_launch_t{kernel, grid, block, group, d};
    }
    g16_plan() = default;
    g16_plan(const g16_plan&) = delete;   // (l[].d may point into own)
};

// The two forward tiles on the 16x16x32 MFMA (gemm_f16x3_ring16_kernel), for the format 1 f16x3 forward and the single-product forward
// alike: 18 = 256 x 256 (`big`) where the grid fills the chip, 22 = 256 x 128 (`small`) below.  Both tiles carry the same bits.
static int g16_tile16(const dupl_gemm16_desc& d) {
    return ((d.M + 255) / 256) * ((d.N + 255) / 256) >= G16_F1_BIG_FROM ? 18 : 22;
}
// big / small: the instantiations of the two tiles by epilogue form ([EPI_GENERIC] .. [EPI_R]; NULL = that form has none); forms: take
// them (the form is matched per launch: the two parts of a row split may differ)
constexpr int EPI_FWD_COUNT = 4;        // forms of the forward kernel, generic included: what g16_epi_form may return
static_assert(EPI_GENERIC == 0 && EPI_P < EPI_FWD_COUNT && EPI_G < EPI_FWD_COUNT && EPI_R < EPI_FWD_COUNT, "the forward form tables are indexed by EPI_*");
static void g16_choose16(g16_plan& pl, const dupl_gemm16_desc& d, const int t, const bool automatic, const int group,
                         const g16_kernel_t (&big)[EPI_FWD_COUNT], const g16_kernel_t (&small)[EPI_FWD_COUNT], const bool forms) {
    auto add = [&](const g16_kernel_t (&ks)[EPI_FWD_COUNT], const dupl_gemm16_desc& q, const int bn) {
        const int f = forms ? g16_epi_form(q) : EPI_GENERIC;
        pl.add(ks[f] ? ks[f] : ks[EPI_GENERIC], dim3((unsigned)(((q.M + 255) / 256) * ((q.N + bn - 1) / bn))), dim3(512), group, &q);
    };
    if (t == 22) return add(small, d, 128);
    // One block per CU and launch: nb22 tiles take ceil(nb22 / 256) rounds, and a last round that holds a few tiles costs as
    // much as a full one.  The merged ms-CAM / training pass of a step is exactly that case -- 21 976 rows = 86 row tiles, x
    // {12, 9, 3} column tiles = 1 032 / 774 / 258 tiles = 4, 3, 1 full rounds + 8 / 6 / 2 tiles (rocprofv3, one stream: 340 us
    // per launch where 6 280 + 15 696 rows took 290).  So: when the last round would be less than 30 % full, the rows of
    // the full rounds go to this kernel and the remaining row tiles to the 256 x 128 kernel (rows are independent: two
    // launches on the stream, each on its own row range of every operand).  Next to a second stream the tail is filled by
    // the other student's blocks anyway; alone this is worth 9-22 % per launch.  The automatic choice only.
    const int cn = (d.N + 255) / 256, rm = (d.M + 255) / 256, cus = 256;
    const int nb22 = rm * cn, full = nb22 / cus, tail = nb22 - full * cus;
    const int r_big = full > 0 ? (full * cus) / cn : 0;
    if (automatic && full > 0 && tail > 0 && tail * 10 < cus * 3 && r_big > 0 && r_big < rm && !d.amax_out &&
        g16_split_rows(d, r_big * 256, pl.own[0], pl.own[1])) {
        add(big, pl.own[0], 256);
        add(small, pl.own[1], 128);
    } else add(big, d, 256);
}

// products = 1: the single-product forward, gemm_f16x3_ring16_kernel<.., NP = 1> on the tiles and with the row split of the format 1
// forward (g16_choose16).
#ifndef G16H_STAGES
#define G16H_STAGES 4   // ring depth of both tiles (4 x 32 KB / 4 x 24 KB)
#endif
static void g16_choose_hi(g16_plan& pl, const dupl_gemm16_desc& d, const g16_tile_t& t, const int group);      // (below: its kernels are emitted last)

// The k-major launches: the backward GEMMs on the forward's own planes (gemm_f16x3_km_kernel; 256 x 128, persistent).  whole: the grid
// of the forms in which a block owns whole tiles; sk: the weight gradient may split K.
static void g16_choose_km(g16_plan& pl, const dupl_gemm16_desc& d, const g16_tile_t& t, const bool sk, const int persist_blocks, const dim3 whole,
                          const int group) {
    const bool accum = d.flags & DUPL_GEMM_ACCUM;
    const int nb21 = ((d.M + 255) / 256) * ((d.N + 127) / 128);
    const dim3 block(512), all((unsigned)persist_blocks);
    if (!accum) {      // the data gradient with the full epilogue
        const bool km16 = g16_km16(t, KM16_DGRAD_EPI);
        return pl.add(g16_km_kernel<false, 0, false, true>(km16, t.forms ? g16_epi_form_km(d) : EPI_GENERIC), whole, block, group, &d);
    }
    // stream-K forms: aligned k-slices (dupl_gemm16_desc.sk_slices: 0 = as many slices per tile as the grid has blocks for, every
    // slice >= G16_PROLOGUE k-steps; < 0 = the equal-run cut of round 4)
    dupl_gemm16_desc& dsk = pl.own[0];
    dsk = d;
    const int ntf = d.K / TBK;
    auto per = [&](int s_) { return (ntf + s_ - 1) / s_; };
    auto fits = [&](int s_) {
        return s_ > 0 && (long)nb21 * s_ <= persist_blocks && per(s_) >= G16_PROLOGUE && ntf - (s_ - 1) * per(s_) >= G16_PROLOGUE;
    };
    // an explicit slice count that does not fit THIS shape (more units than blocks, a slice shorter than the prologue) falls back
    // to the library's choice instead of failing the launch: the value is a per-model tuning default that meets every shape of
    // the step, including the launches that never look at it (deterministic mode, one block per tile) -- ADVICE r5
    if (dsk.sk_slices > 0 && !fits(dsk.sk_slices)) dsk.sk_slices = 0;
    if (dsk.sk_slices == 0) {
        // more tiles than blocks: the equal-run cut (a block's run then spans several tiles); otherwise as many slices as
        // there are blocks for.  Measured (profiles/r05_sk_slices.txt): stand-alone 3140 x 768 x 3072 244 vs 211 TF/s-eq, 1570 x
        // 768 x 3072 171-187 vs 149; with a second stream's launch in flight the 4-image shape is slower stand-alone (2 slices
        // = 156 of 192 blocks: 287 vs 312) but the STEP is faster with it at 4 images too (52.0 vs 52.35 ms, 30.5 vs 30.9 at 2):
        // the blocks it leaves free and the fabric bandwidth it no longer takes go to the other student's kernels
        int S = nb21 > persist_blocks ? -1 : persist_blocks / nb21;
        while (S > 1 && (per(S) < G16_PROLOGUE || ntf - (S - 1) * per(S) < G16_PROLOGUE)) --S;
        dsk.sk_slices = S;
    }
    if (dsk.sk_slices > 0 && !fits(dsk.sk_slices)) dsk.sk_slices = -1;      // (cannot happen for the choice above: kept as a guard -> equal runs)
    if (!d.a_layout)
        // a data gradient with a LINEAR epilogue (dx = alpha dy . W, nothing else) into a zero-filled dx: stream-K pieces meet in
        // fp32 atomics, so that the N = 768 outputs (78 tiles of 256 x 128 at 4 images, 42 at 2) run on every CU
        pl.add(g16_km_kernel<true, 1, false, true>(g16_km16(t, KM16_DGRAD_SK)), all, block, group, &dsk);
    else if (sk) pl.add(g16_km_kernel<true, 1, true, true>(g16_km16(t, KM16_WGRAD_SK)), all, block, group, &dsk);
    else pl.add(g16_km_kernel<false, 2, true, true>(g16_km16(t, KM16_WGRAD_TILE)), whole, block, group, &d);
}

static void g16_choose(g16_plan& pl, const dupl_gemm16_desc& d, const bool single) {
    const g16_tile_t t = g16_resolve_tile(d.tile);
    const bool kmajor = d.a_layout || d.b_layout, accum = d.flags & DUPL_GEMM_ACCUM;
    const int concurrency = d.concurrency > 0 ? d.concurrency : 1;
    const int persist_blocks = d.persist_blocks ? d.persist_blocks : (concurrency >= 2 ? 192 : 256);
    const int group_m = d.group ? d.group : G16_GROUP_M, group_ring = d.group ? d.group : G16_GROUP_RING;
    const int ntf = d.K / TBK, nb21 = ((d.M + 255) / 256) * ((d.N + 127) / 128);
    if (single) return g16_choose_hi(pl, d, t, group_ring);
    // split-K for accumulating GEMMs (weight gradients: few output tiles, K = all tokens): >= ~2 blocks per CU,
    // >= 8 k-tiles per split
    int ksplit = 1;
    if (accum) {
        const long tiles = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
        ksplit = (int)((512 + tiles - 1) / tiles);
        const int maxs = (ntf + 7) / 8;
        if (ksplit > maxs) ksplit = maxs;
        if (ksplit < 1) ksplit = 1;
        if (d.deterministic) ksplit = 1;      // no fp32 atomics
    }
    auto blocks = [&](int bm, int bn) { return dim3((unsigned)(((d.M + bm - 1) / bm) * ((d.N + bn - 1) / bn)), (unsigned)ksplit); };
    // grid of a persistent kernel, every block walks the same number of tiles: with tx tiles per XCD and at most maxb / 8 blocks per
    // XCD the walk takes rounds = ceil(tx / (maxb / 8)) tiles, and ceil(tx / rounds) blocks per XCD are enough for that -- 600 tiles
    // run as 3 x 200 instead of 2.3 x 256 (the kernel is power-bound: a few CUs less cost nothing, an idle last round does)
    auto persist_grid = [&](const int nblk) {
        const int tx = (nblk + 7) / 8, bmax = persist_blocks / 8;
        const int rounds = (tx + bmax - 1) / bmax;
        return dim3((unsigned)(8 * ((tx + rounds - 1) / rounds)));
    };
    if (kmajor) return g16_choose_km(pl, d, t, accum && !d.deterministic && ksplit > 1, persist_blocks, persist_grid(nb21), group_ring);
    if (d.fmt == 1) {
        // format 1 operands: one accumulator set.  256 x 256 on 8 waves (wave tile 128 x 64, two LDS stages of 64 KB; tile 8) where
        // the grid fills the chip, 256 x 128 (the ring kernel's tile with half the accumulators; 12) below.  One block per tile: the
        // persistent form of 256 x 128 (14) measures the same or 1-3 % less, that of 256 x 256 spills (228 vs 353 TF/s-eq)
        // (round 6, measured and dropped: the same 256 x 256 tile on FOUR waves of 128 x 128 -- one wave per SIMD in the 512-register
        // file, 252 VGPRs + 256 accumulation registers, no spill, 16 instead of 24 fragment reads per 48 MFMAs -- is 8-20 % SLOWER on
        // every forward shape, alone and next to a second stream (15 696 x 3 072 x 768 bias + GELU -> planes: 247 vs 300 TF/s-eq,
        // 15 696 x 768 x 3 072 bias + residual: 295 vs 328; profiles/r06_tile16.txt): with one wave per SIMD nothing covers a wave's
        // own waits, the result tile 7 gave in round 3)
        // (18 / 22: the same two tiles on the 16x16x32 MFMA, gemm_f16x3_ring16_kernel; the launcher's own choice, since the clock the
        // chip holds under this loop is higher on that shape.  Both tiles switch together: they are bit-identical to each other)
        int f = (t.family == 8 || t.family == 12 || t.family == 14 || t.family == 18 || t.family == 22) ? t.family : g16_tile16(d);
        if (ntf < G16_PROLOGUE && f == 14) f = 12;
        if (f == 18 || f == 22) {
            static const g16_kernel_t big[EPI_FWD_COUNT] = {gemm_f16x3_ring16_kernel<4, 2, 2, 4, 2, 2>, gemm_f16x3_ring16_kernel<4, 2, 2, 4, 2, 2, 3, EPI_P>,
                                                gemm_f16x3_ring16_kernel<4, 2, 2, 4, 2, 2, 3, EPI_G>, gemm_f16x3_ring16_kernel<4, 2, 2, 4, 2, 2, 3, EPI_R>};
            static const g16_kernel_t small[EPI_FWD_COUNT] = {gemm_f16x3_ring16_kernel<2, 2, 4, 2, 2, 3>, gemm_f16x3_ring16_kernel<2, 2, 4, 2, 2, 3, 3, EPI_P>,
                                                  gemm_f16x3_ring16_kernel<2, 2, 4, 2, 2, 3, 3, EPI_G>, gemm_f16x3_ring16_kernel<2, 2, 4, 2, 2, 3, 3, EPI_R>};
            return g16_choose16(pl, d, f, t.family == 0, group_ring, big, small, t.forms);
        }
        if (f == 8) return pl.add(gemm_f16x3_ring_kernel<4, 2, 2, 4, 2, 2, true>, blocks(256, 256), dim3(512), group_ring, &d);
        if (f == 12) return pl.add(gemm_f16x3_ring_kernel<2, 2, 4, 2, 2, 3, true>, blocks(256, 128), dim3(512), group_ring, &d);
        return pl.add(gemm_f16x3_pring_kernel<2, 2, 4, 2, 2, false, true, 3>, persist_grid(nb21), dim3(512), group_ring, &d);
    }
    // format 0 operands
    int f = t.family;
    if (f == 0) {
        // Measured on the shapes of the step (tools/gemm16_bench -w 200 with and without -2, profiles/r03_gemm16_tiles.txt),
        // sustained clocks.  The persistent 256 x 128 ring kernel (tile 10; 6 = the same, one block per tile) is one block
        // per CU: it wins wherever its grid covers a good part of the chip -- >= 64 tiles when a second stream feeds the chip
        // as well (the two students: dupl_gemm16_desc.concurrency 2), >= 128 tiles alone.  The weight gradients go to its
        // stream-K form (tile 11) when every block gets >= 10 k-steps (K = 1600, one stream: 3072 x 768 143 vs 117, 2304 x 768 116 vs 100): 3072 x 768 x 3168 alone 155 -> 205 TF/s-eq, with a
        // second stream 219 -> 238 (there only from 64 tiles on: 2304 x 768 loses 6 % to two co-resident 128 x 128 blocks of
        // both streams); the rest stay on split-K grids of 128 x 128 (tile 5, two blocks per CU) / 128 x 64 (tile 3).
        const long b256 = nb21;
        const long b128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128) * ksplit;
        const bool ring = b256 >= (concurrency >= 2 ? 64 : 128);
        if (!accum && ring) f = 10;
        else if (accum && ksplit > 1 && ntf >= 8 && b256 * ntf >= 10L * persist_blocks && (concurrency < 2 || b256 >= 64)) f = 11;
        else f = b128 < 200 ? 3 : 5;
    }
    if (f == 10 && (accum || ntf < G16_PROLOGUE)) f = 6;      // the persistent kernel has no split-K and a 3-stage prologue
    if (f == 11 && (!accum || d.deterministic || ntf < 8)) f = accum ? 5 : 6;   // stream-K: atomics, pieces >= G16_PROLOGUE k-steps
    // (11: the caller's descriptor as it is -- this kernel takes the equal-run cut whatever sk_slices says)
    if (f == 11) return pl.add(gemm_f16x3_pring_kernel<2, 2, 4, 2, 2, true>, dim3((unsigned)persist_blocks), dim3(512), group_ring, &d);
    if (f == 10) return pl.add(gemm_f16x3_pring_kernel<2, 2, 4, 2, 2>, persist_grid(nb21), dim3(512), group_ring, &d);
    if (f == 8 || f == 12 || f == 14 || f == 18 || f == 22) f = 5;      // single-accumulator tiles: format 1 operands only (above)
    if (f == 6) return pl.add(gemm_f16x3_ring_kernel<2, 2, 4, 2, 2>, blocks(256, 128), dim3(512), group_ring, &d);
    if (f == 7) return pl.add(gemm_f16x3_ring_kernel<4, 2, 2, 2, 1>, blocks(256, 128), dim3(256), group_ring, &d);
    if (f == 3) return pl.add(gemm_f16x3_kernel<2, 1, 2, 2, 2>, blocks(128, 64), dim3(256), group_m, &d);
    pl.add(gemm_f16x3_kernel<2, 1, 2, 4, 4>, blocks(128, 128), dim3(512), group_m, &d);
}

// 3. Launch.
extern "C" int dupl_gemm_f16x3(const dupl_gemm16_desc* d, dupl_stream_t stream) {
    if (!d) return DUPL_ERR_ARG;
    // products = 1 reads no lo plane: NULL lo pointers are accepted, and stand in as the hi planes for the checks both forms share
    dupl_gemm16_desc hi1;
    const bool single = d->struct_size == sizeof(dupl_gemm16_desc) && d->products == 1;
    if (single) {
        hi1 = *d;
        if (!hi1.A_lo) hi1.A_lo = hi1.A_hi;
        if (!hi1.B_lo) hi1.B_lo = hi1.B_hi;
        d = &hi1;
    }
    if (!g16_check(*d, single)) return DUPL_ERR_ARG;
    g16_plan pl;
    g16_choose(pl, *d, single);
    for (int i = 0; i < pl.n; ++i) DUPL_LAUNCH(pl.l[i].kernel, pl.l[i].grid, pl.l[i].block, 0, (hipStream_t)stream, *pl.l[i].d, pl.l[i].group);
    return dupl_launch_status();
}

static void g16_choose_hi(g16_plan& pl, const dupl_gemm16_desc& d, const g16_tile_t& t, const int group) {
    // (the generic epilogue only: NP = 1 has no forms)
    static const g16_kernel_t small[EPI_FWD_COUNT] = {gemm_f16x3_ring16_kernel<2, 2, 4, 2, 2, G16H_STAGES, 1>, nullptr, nullptr, nullptr};
    static const g16_kernel_t big[EPI_FWD_COUNT] = {gemm_f16x3_ring16_kernel<4, 2, 2, 4, 2, G16H_STAGES, 1>, nullptr, nullptr, nullptr};
    g16_choose16(pl, d, (t.family == 18 || t.family == 22) ? t.family : g16_tile16(d), t.family == 0, group, big, small, false);
}

