// Stand-alone timing of the split attention forward (csrc/attn_split.hip) and backward (csrc/attn_split_bwd.hip) through the C ABI.
//   default        the four single-batch cases with the kernel chosen by -m (0 = the library's choice, 32, 16); with an ATT_ABL=16
//                  build of the library (LD_LIBRARY_PATH) -d prints the per-phase cycle sums of wave 0: wait + barrier / QK^T /
//                  softmax / PV
//   -c [-r R]      both kernels (mfma 32 and 16) INTERLEAVED in one process, R rounds (default 5) of one -w window each: the four
//                  cases, then the step's segmented launch ((8, 1765), (8, 197)) in one stream and next to a second stream that
//                  runs the same launch.  Per case: median / min / max of each kernel's rounds, its spread (max - min) / median, and
//                  the ratio of the medians.
//   -b [-r R]      the BACKWARD (dupl_attention_bwd16: delta + the two-role launch) at H = 12, B x N = 4 x 785 (the step), 2 x 785,
//                  8 x 785, 4 x 197: random planes, out / lse from the forward, the dO planes and scale record from the real split; each
//                  case in one stream and next to a second stream, median / min / max of R rounds
//   -s             the segmented launch alone, one stream, kernel -m, one -w window (what a counter pass is taken on)
// build: hipcc -O2 --offload-arch=gfx950 -Iinclude tools/attn16_bench.cpp -Ldupl_amd -ldupl_hip -Wl,-rpath,'$ORIGIN/../dupl_amd' -o tools/attn16_bench
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include "dupl_hip.h"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)
__device__ __forceinline__ uint32_t hash32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
__global__ void fill_kernel(float* x, long n, uint32_t seed, float sigma) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        uint32_t h = hash32((uint32_t)i * 2654435761U + seed);
        float s = 0.f;
        for (int k = 0; k < 4; ++k) { h = hash32(h + 0x9e3779b9U); s += (float)(h >> 8) * (1.f / 16777216.f) - 0.5f; }
        x[i] = s * sigma * 1.7320508f;
    }
}

static const int H = 12, hd = 64, D = H * hd;

// wall time per call of `launch` (asynchronous; everything it started is awaited), over about window_ms
static double time_us(const std::function<int()>& launch, int window_ms) {
    auto wall = [&](int n) {
        CK(hipDeviceSynchronize());
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; ++i) if (launch()) { fprintf(stderr, "launch failed\n"); exit(2); }
        CK(hipDeviceSynchronize());
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    };
    const double probe = wall(3) / 3;
    const int iters = (int)(window_ms * 1e3 / probe) + 1;
    wall(iters / 3 + 1);
    return wall(iters) / iters;
}

struct Planes {          // q / k / v planes of `rows` tokens and one set of output planes
    float* qkv; __half *q16, *o16; long nq, rows;
    explicit Planes(long rows_, uint32_t seed) : rows(rows_) {
        nq = rows * 3 * D;
        CK(hipMalloc(&qkv, nq * 4)); CK(hipMalloc(&q16, nq * 4)); CK(hipMalloc(&o16, rows * D * 4));
        fill_kernel<<<1024, 256>>>(qkv, nq, seed, 1.5f);
        dupl_split_f16x2(qkv, q16, q16 + nq, nq, nullptr);
        CK(hipDeviceSynchronize());
    }
    ~Planes() { hipFree(qkv); hipFree(q16); hipFree(o16); }
};

static void report(const char* tag, std::vector<double> t32, std::vector<double> t16) {
    auto stat = [](std::vector<double>& v, double& med, double& lo, double& hi) {
        std::sort(v.begin(), v.end());
        med = v[v.size() / 2]; lo = v.front(); hi = v.back();
    };
    double m32, l32, h32, m16, l16, h16;
    stat(t32, m32, l32, h32); stat(t16, m16, l16, h16);
    printf("%-34s | %7.1f %7.1f %7.1f  %5.2f%% | %7.1f %7.1f %7.1f  %5.2f%% | %6.3f  %+5.1f%%\n", tag, m32, l32, h32, (h32 - l32) / m32 * 100,
           m16, l16, h16, (h16 - l16) / m16 * 100, m16 / m32, (m16 / m32 - 1) * 100);
}

static int compare(int rounds, int window_ms) {
    hipStream_t st, st2; CK(hipStreamCreate(&st)); CK(hipStreamCreate(&st2));
    printf("time per launch, us: median / min / max of %d interleaved rounds, spread = (max - min) / median\n", rounds);
    printf("%-34s | 32x32x16: med     min     max  spread | 16x16x32: med     min     max  spread |  ratio   gain\n", "case");
    const int cases[][2] = {{8, 1765}, {8, 785}, {8, 197}, {4, 785}};
    for (auto& c : cases) {
        const int B = c[0], N = c[1];
        Planes p((long)B * N, 7);
        std::vector<double> t32, t16;
        for (int r = 0; r < rounds; ++r)
            for (int m : {32, 16}) {
                auto run = [&]() { return dupl_attention_fwd16_mfma(p.q16, p.q16 + p.nq, nullptr, p.o16, p.o16 + p.rows * D, nullptr, B, N, H, hd, 0.125f, 0, 0, m, st); };
                (m == 32 ? t32 : t16).push_back(time_us(run, window_ms));
            }
        char tag[64]; snprintf(tag, sizeof tag, "B=%d N=%d", B, N);
        report(tag, t32, t16);
    }
    // the step's segmented ms-CAM launch, alone and next to a second stream running the same launch on its own buffers
    const long rows = 8L * 1765 + 8L * 197;
    Planes a(rows, 11), b(rows, 13);
    dupl_attn_seg segs[2];
    segs[0].row0 = 0; segs[0].B = 8; segs[0].N = 1765; segs[1].row0 = 8L * 1765; segs[1].B = 8; segs[1].N = 197;
    for (auto& s : segs) { s.B_f32 = 0; s.reserved0 = 0; s.out = nullptr; s.lse = nullptr; }
    for (int two = 0; two < 2; ++two) {
        std::vector<double> t32, t16;
        for (int r = 0; r < rounds; ++r)
            for (int m : {32, 16}) {
                auto run = [&]() {
                    int e = dupl_attention_fwd16_segs_mfma(a.q16, a.q16 + a.nq, a.o16, a.o16 + rows * D, segs, 2, H, hd, 0.125f, 0, m, st);
                    if (two && !e) e = dupl_attention_fwd16_segs_mfma(b.q16, b.q16 + b.nq, b.o16, b.o16 + rows * D, segs, 2, H, hd, 0.125f, 0, m, st2);
                    return e;
                };
                (m == 32 ? t32 : t16).push_back(time_us(run, window_ms));
            }
        report(two ? "segs 8x1765 + 8x197, two streams" : "segs 8x1765 + 8x197, one stream", t32, t16);
    }
    return 0;
}

// Everything one backward call needs, made the way a step makes it: q / k / v planes of random data, out and lse from the forward,
// a random dout of a step's magnitude, its planes and scale record from the real split (dupl_split_prepare, target_exp 4).
struct Bwd {
    Planes p; int B, N; float *out, *dout, *lse, *delta, *dqkv, *slot; __half* do16; long no;
    Bwd(int B_, int N_, uint32_t seed, hipStream_t st) : p((long)B_ * N_, seed), B(B_), N(N_) {
        no = (long)B * N * D;
        CK(hipMalloc(&out, no * 4)); CK(hipMalloc(&dout, no * 4)); CK(hipMalloc(&do16, no * 4)); CK(hipMalloc(&dqkv, p.nq * 4));
        CK(hipMalloc(&lse, (long)B * H * N * 4)); CK(hipMalloc(&delta, (long)B * H * N * 4)); CK(hipMalloc(&slot, 32));
        CK(hipMemset(slot, 0, 32));
        fill_kernel<<<1024, 256>>>(dout, no, seed + 1, 2e-5f);
        if (dupl_attention_fwd16_mfma(p.q16, p.q16 + p.nq, out, nullptr, nullptr, lse, B, N, H, hd, 0.125f, 0, 0, 0, st)) { fprintf(stderr, "forward failed\n"); exit(2); }
        dupl_split_desc d; memset(&d, 0, sizeof d);
        d.struct_size = sizeof d; d.x = dout; d.ld = D; d.R = B * N; d.C = D; d.slot = slot; d.next_bits = slot + 6;
        d.hi = do16; d.lo = do16 + no; d.Rp = (B * N + 31) / 32 * 32; d.target_exp = 4;
        if (dupl_split_prepare(&d, st)) { fprintf(stderr, "split failed\n"); exit(2); }
        CK(hipDeviceSynchronize());
    }
    int run(hipStream_t st) const {
        return dupl_attention_bwd16(p.q16, p.q16 + p.nq, out, dout, do16, do16 + no, slot, lse, delta, dqkv, B, N, H, hd, 0.125f, nullptr, st);
    }
    ~Bwd() { hipFree(out); hipFree(dout); hipFree(do16); hipFree(dqkv); hipFree(lse); hipFree(delta); hipFree(slot); }
};

// -b: dupl_attention_bwd16 (the delta launch + the dq / dk + dv launch), each case in one stream and next to a second stream that runs
// the same call on its own buffers.  Two builds of the library are compared by alternating two runs of this mode (LD_LIBRARY_PATH).
static int time_bwd(int rounds, int window_ms) {
    hipStream_t st, st2; CK(hipStreamCreate(&st)); CK(hipStreamCreate(&st2));
    printf("backward, time per call, us: median / min / max of %d rounds, spread = (max - min) / median\n", rounds);
    const int cases[][2] = {{4, 785}, {2, 785}, {8, 785}, {4, 197}};
    for (auto& c : cases) {
        Bwd a(c[0], c[1], 7, st), b(c[0], c[1], 17, st);
        for (int two = 0; two < 2; ++two) {
            std::vector<double> t;
            for (int r = 0; r < rounds; ++r) {
                auto run = [&]() { int e = a.run(st); if (two && !e) e = b.run(st2); return e; };
                t.push_back(time_us(run, window_ms));
            }
            std::sort(t.begin(), t.end());
            printf("B=%d N=%4d, %-11s | %7.1f %7.1f %7.1f  %5.2f%%\n", c[0], c[1], two ? "two streams" : "one stream", t[t.size() / 2], t.front(),
                   t.back(), (t.back() - t.front()) / t[t.size() / 2] * 100);
        }
    }
    return 0;
}

static int segs_only(int mfma, int window_ms) {
    hipStream_t st; CK(hipStreamCreate(&st));
    const long rows = 8L * 1765 + 8L * 197;
    Planes a(rows, 11);
    dupl_attn_seg segs[2];
    segs[0].row0 = 0; segs[0].B = 8; segs[0].N = 1765; segs[1].row0 = 8L * 1765; segs[1].B = 8; segs[1].N = 197;
    for (auto& s : segs) { s.B_f32 = 0; s.reserved0 = 0; s.out = nullptr; s.lse = nullptr; }
    auto run = [&]() { return dupl_attention_fwd16_segs_mfma(a.q16, a.q16 + a.nq, a.o16, a.o16 + rows * D, segs, 2, H, hd, 0.125f, 0, mfma, st); };
    printf("mfma %2d segs 8x1765 + 8x197: %7.1f us\n", mfma, time_us(run, window_ms));
    return 0;
}

int main(int argc, char** argv) {
    bool dbg = false, cmp = false, sgo = false, bwd = false;
    int window_ms = 200, mfma = 0, rounds = 5;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-d")) dbg = true;
        else if (!strcmp(argv[i], "-c")) cmp = true;
        else if (!strcmp(argv[i], "-s")) sgo = true;
        else if (!strcmp(argv[i], "-b")) bwd = true;
        else if (!strcmp(argv[i], "-w") && i + 1 < argc) window_ms = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-m") && i + 1 < argc) mfma = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) rounds = std::max(1, atoi(argv[++i]));
    }
    if (bwd) return time_bwd(rounds, window_ms);
    if (cmp) return compare(rounds, window_ms);
    if (sgo) return segs_only(mfma, window_ms);
    const int cases[][2] = {{8, 1765}, {8, 785}, {8, 197}, {4, 785}};
    hipStream_t st; CK(hipStreamCreate(&st));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (auto& c : cases) {
        const int B = c[0], N = c[1];
        const long nq = (long)B * N * 3 * D;
        float* qkv; __half *q16, *o16; float *out, *lse;
        CK(hipMalloc(&qkv, nq * 4)); CK(hipMalloc(&q16, nq * 4));
        CK(hipMalloc(&o16, (long)B * N * D * 4)); CK(hipMalloc(&out, (long)B * N * D * 4)); CK(hipMalloc(&lse, (long)B * H * N * 4 + (1 << 20)));
        fill_kernel<<<1024, 256>>>(qkv, nq, 7, 1.5f);
        dupl_split_f16x2(qkv, q16, q16 + nq, nq, nullptr);
        CK(hipDeviceSynchronize());
        auto run = [&]() { return dupl_attention_fwd16_mfma(q16, q16 + nq, nullptr, o16, o16 + (long)B * N * D, lse, B, N, H, hd, 0.125f, 0, 0, mfma, st); };
        if (run()) { fprintf(stderr, "launch failed\n"); return 2; }
        CK(hipEventRecord(e0, st)); for (int i = 0; i < 3; ++i) run(); CK(hipEventRecord(e1, st)); CK(hipDeviceSynchronize());
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        int iters = (int)(window_ms / (ms / 3)) + 1;
        for (int i = 0; i < iters / 3; ++i) run();
        CK(hipEventRecord(e0, st)); for (int i = 0; i < iters; ++i) run(); CK(hipEventRecord(e1, st)); CK(hipDeviceSynchronize());
        CK(hipEventElapsedTime(&ms, e0, e1));
        const double us = ms * 1e3 / iters, fl = 4.0 * B * H * (double)N * N * hd;
        printf("mfma %2d B=%d N=%4d: %7.1f us  %5.0f TF/s-eq", mfma, B, N, us, fl / us / 1e6);
        if (dbg) {
            // one record of four sums per block, behind the lse data (both kernels: blocks in launch order, one segment)
            const int nblk = ((N + 127) / 128) * H * B;
            std::vector<long long> h((size_t)nblk * 4);
            CK(hipMemcpy(h.data(), lse + ((((size_t)B * H * N) + 1) & ~(size_t)1), h.size() * 8, hipMemcpyDeviceToHost));
            double p[4] = {0, 0, 0, 0};
            for (int b = 0; b < nblk; ++b) for (int k = 0; k < 4; ++k) p[k] += (double)h[4 * b + k];
            const double nt = (double)((N + 63) / 64) * nblk;
            printf("  [cycles per key tile, wave 0: wait+barrier %.0f, QK %.0f, softmax %.0f, PV %.0f]", p[0] / nt, p[1] / nt, p[2] / nt, p[3] / nt);
        }
        printf("\n");
        hipFree(qkv); hipFree(q16); hipFree(o16); hipFree(out); hipFree(lse);
    }
    return 0;
}
