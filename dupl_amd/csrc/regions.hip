// Connected regions of a (H,W) uint8 label map (tools/predict --min_region / --regions; beyond the reference, which never looks at
// objects).  Two pixels are connected when they carry the same label and are 4- or 8-neighbours; pixels equal to ignore_index (or
// >= C) belong to no region.  The representative of a region is its first pixel in raster order, regions are numbered in raster
// order of that pixel.  dupl_seg_regions, six launches:
//   local    a 64 x 16 tile per workgroup: union-find in LDS, union by smaller index (atomicMin), the tile's roots written as global
//            linear indices into parent (N int32);
//   seam     a thread per pixel on a tile seam: the pairs that cross it (the diagonal ones under 8-connectivity) united with the
//            same atomicMin rule on the global parent array -- the final root is the component's smallest index in any arrival order;
//   flatten  parent[i] = root, and the roots of every 1024 pixels counted (the block sums of the scan);
//   scan     the block sums, by one workgroup; the total is n_regions;
//   number   the add: root pixels get their id, and their table row starts as the root pixel alone;
//   stats    region[i] = id of parent[i]; area, box, conf sum and the per-label counts combined per distinct key in an LDS hash table
//            (512 pixels per pass, 1024 slots; a wave whose 128 pixels agree inserts once), then one global atomic per workgroup
//            pass, key and column -- box columns only where they still move the stored value.
// No workgroup waits for another: every loop is a retry of atomicMin / atomicCAS that ends on its own (the indices fall strictly;
// the hash table has more slots than a pass has keys).  Integer atomics only: every output is bit-reproducible.
// dupl_seg_regions_clean: count (areas of the regions beyond the table, only where there are any), vote, decide, apply.
#include "common.h"
#include "../../include/dupl_hip.h"
#include <climits>

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_TW = 64, RG_TH = 16, RG_TILE = RG_TW * RG_TH;
constexpr int RG_CHUNK = 1024;               // pixels per workgroup of flatten / number: four consecutive ones per thread
constexpr int RG_PASS = 512;                 // pixels per hash-table pass of stats / count: two consecutive ones per thread
constexpr int RG_SLOTS = 1024;               // twice the keys a pass can hold
constexpr int RG_EMPTY = -1, RG_IGN = -2;    // hash keys: free slot, the ignored pixels
constexpr int RG_MAX_GRID = 2048;            // grid-stride kernels

struct RegArgs {
    const unsigned char* label;
    const float* conf;
    int* parent;                             // N
    int* rid;                                // N: the id at root pixels after `number`; `region` itself where that is given
    int* region;
    int* bsum;                               // nb block sums, scanned in place
    int* n_ws;
    int* n_out;
    long long* table;
    unsigned long long* stats;
    int H, W, C, conn8, ignore, max_regions, tiles_x, tiles_y, nb;
    long N;
};

__device__ __forceinline__ bool rg_valid(const RegArgs& a, int l) { return l != a.ignore && l < a.C; }

// ------------------------------------------------------------------------------------------------------------------ union-find
// parent[i] <= i throughout, and only ever falls.  A retry continues with strictly smaller indices, so every loop ends.
__device__ __forceinline__ int rg_find_lds(volatile int* par, int x) {
    int p;
    while ((p = par[x]) != x) x = p;
    return x;
}
__device__ __forceinline__ void rg_union_lds(int* par, int a, int b) {
    for (;;) {
        a = rg_find_lds(par, a);
        b = rg_find_lds(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;                // a was a root and now hangs below b
        a = old;                             // a had been hung below `old` meanwhile: unite that with b
    }
}
__device__ __forceinline__ int rg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int rg_find_g(const int* par, int x) {
    int p;
    while ((p = rg_load(par + x)) != x) x = p;
    return x;
}
__device__ __forceinline__ void rg_union_g(int* par, int a, int b) {
    const int a0 = a, b0 = b;
    a = rg_find_g(par, a);
    b = rg_find_g(par, b);
    if (a != a0) atomicMin(&par[a0], a);     // shorten the two chains just walked: an ancestor stays an ancestor
    if (b != b0) atomicMin(&par[b0], b);
    for (;;) {
        a = rg_find_g(par, a);
        b = rg_find_g(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

// ----------------------------------------------------------------------------------------------------------------------- local
__global__ __launch_bounds__(RG_THREADS) void rg_local_kernel(const RegArgs a) {
    __shared__ int s_par[RG_TILE];
    __shared__ short s_lab[RG_TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ty0 = (int)(blockIdx.x / a.tiles_x) * RG_TH, tx0 = (int)(blockIdx.x % a.tiles_x) * RG_TW;
    // a wave holds one tile row per step (RG_TW = 64 lanes): the row's runs of equal labels come from one ballot, and every pixel
    // starts below the first pixel of its run -- no union along the rows at all
#pragma unroll
    for (int k = 0; k < RG_TILE / RG_THREADS; ++k) {
        const int i = tid + k * RG_THREADS, y = ty0 + (i >> 6), x = tx0 + lane;
        int l = -1;
        if (y < a.H && x < a.W) {
            const int v = a.label[(long)y * a.W + x];
            if (rg_valid(a, v)) l = v;
        }
        const int lw = __shfl_up(l, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || lw != l);
        s_lab[i] = (short)l;
        s_par[i] = (i & ~63) + 63 - __clzll(heads & (~0ull >> (63 - lane)));
    }
    __syncthreads();
    // A pair of equal labels is united only where no neighbouring pair already implies it: the pixel above when the pair to the
    // left is not the same two labels, a diagonal pixel only when neither pixel between the two carries the label.
#pragma unroll
    for (int k = 0; k < RG_TILE / RG_THREADS; ++k) {
        const int i = tid + k * RG_THREADS, ly = i >> 6, lx = i & 63;
        const short l = s_lab[i];
        if (l < 0 || ly == 0) continue;
        const bool west = lx > 0 && s_lab[i - 1] == l;
        if (s_lab[i - RG_TW] == l) {
            if (!west || s_lab[i - RG_TW - 1] != l) rg_union_lds(s_par, i, i - RG_TW);
        } else if (a.conn8) {
            if (lx > 0 && !west && s_lab[i - RG_TW - 1] == l) rg_union_lds(s_par, i, i - RG_TW - 1);
            if (lx < RG_TW - 1 && s_lab[i - RG_TW + 1] == l && s_lab[i + 1] != l) rg_union_lds(s_par, i, i - RG_TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RG_TILE / RG_THREADS; ++k) {
        const int i = tid + k * RG_THREADS, y = ty0 + (i >> 6), x = tx0 + (i & 63);
        if (y >= a.H || x >= a.W) continue;
        int out = -1;
        if (s_lab[i] >= 0) {
            const int r = rg_find_lds(s_par, i);
            out = (ty0 + (r >> 6)) * a.W + tx0 + (r & 63);
        }
        a.parent[(long)y * a.W + x] = out;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ seam
// the label at (y, x), -1 off the image and on pixels that belong to no region
__device__ __forceinline__ int rg_lab(const RegArgs& a, int y, int x) {
    if (y < 0 || x < 0 || x >= a.W) return -1;
    const int l = a.label[y * a.W + x];
    return rg_valid(a, l) ? l : -1;
}

// threads [0, rows W): pixel (k RG_TH, x) of horizontal seam k against the row above; the rest: the pixel pair on either side of
// vertical seam k in row y against each other and against the row above
__global__ __launch_bounds__(RG_THREADS) void rg_seam_kernel(const RegArgs a) {
    const long nrow = (long)(a.tiles_y - 1) * a.W, total = nrow + (long)(a.tiles_x - 1) * a.H;
    for (long t = (long)blockIdx.x * RG_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * RG_THREADS) {
        // as in the tile: a pair is united only where the neighbouring pair along the seam is not the same two labels (that one is
        // united, or implied in turn), a diagonal pair only when neither pixel between the two carries the label.  Where the two
        // seams cross nothing is left out: there each of the two pairs would otherwise count on the other.
        if (t < nrow) {
            const int y = (int)(t / a.W + 1) * RG_TH, x = (int)(t % a.W);
            const int l = rg_lab(a, y, x);
            if (l < 0) continue;
            const int p = y * a.W + x;
            if (rg_lab(a, y - 1, x) == l) {
                if (x % RG_TW == 0 || rg_lab(a, y, x - 1) != l || rg_lab(a, y - 1, x - 1) != l) rg_union_g(a.parent, p, p - a.W);
            } else if (a.conn8) {
                if (rg_lab(a, y - 1, x - 1) == l && rg_lab(a, y, x - 1) != l) rg_union_g(a.parent, p, p - a.W - 1);
                if (rg_lab(a, y - 1, x + 1) == l && rg_lab(a, y, x + 1) != l) rg_union_g(a.parent, p, p - a.W + 1);
            }
        } else {
            const long u = t - nrow;
            const int x = (int)(u / a.H + 1) * RG_TW, y = (int)(u % a.H);
            const int l = rg_lab(a, y, x), lw = rg_lab(a, y, x - 1);
            const int p = y * a.W + x;
            if (l >= 0 && l == lw) {
                if (y % RG_TH == 0 || rg_lab(a, y - 1, x) != l || rg_lab(a, y - 1, x - 1) != l) rg_union_g(a.parent, p, p - 1);
            } else if (a.conn8) {
                if (l >= 0 && rg_lab(a, y - 1, x - 1) == l && rg_lab(a, y - 1, x) != l) rg_union_g(a.parent, p, p - a.W - 1);
                if (lw >= 0 && rg_lab(a, y - 1, x) == lw && rg_lab(a, y - 1, x - 1) != lw) rg_union_g(a.parent, p - 1, p - a.W);
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------- flatten
// The roots do not move in this launch; an entry another thread flattens meanwhile reads as its old parent or as its root: both
// lead to the root.
__global__ __launch_bounds__(RG_THREADS) void rg_flatten_kernel(const RegArgs a) {
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * RG_CHUNK + threadIdx.x * 4;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = base + k;
        if (i >= a.N) break;
        const int p = a.parent[i];
        if (p < 0) continue;
        const int r = rg_find_g(a.parent, p);
        if (r != p) a.parent[i] = r;
        cnt += r == (int)i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = s_cnt;
}

// exclusive scan of the nb block sums in place, by one workgroup: a contiguous stretch per thread
__global__ __launch_bounds__(RG_THREADS) void rg_scan_kernel(const RegArgs a) {
    __shared__ int s[RG_THREADS];
    const int per = (a.nb + RG_THREADS - 1) / RG_THREADS;
    const long lo = (long)threadIdx.x * per, hi = lo + per < a.nb ? lo + per : a.nb;
    int sum = 0;
    for (long j = lo; j < hi; ++j) sum += a.bsum[j];
    s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < RG_THREADS; ++t) {
            const int v = s[t];
            s[t] = run;
            run += v;
        }
        *a.n_ws = run;
        if (a.n_out) *a.n_out = run;
    }
    __syncthreads();
    int run = s[threadIdx.x];
    for (long j = lo; j < hi; ++j) {
        const int v = a.bsum[j];
        a.bsum[j] = run;
        run += v;
    }
}

__global__ __launch_bounds__(RG_THREADS) void rg_number_kernel(const RegArgs a) {
    __shared__ int s_wave[RG_THREADS / 64];
    const long base = (long)blockIdx.x * RG_CHUNK + threadIdx.x * 4;
    bool f[4];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = base + k;
        f[k] = i < a.N && a.parent[i] == (int)i;
        cnt += f[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int id = a.bsum[blockIdx.x] + inc - cnt;
    for (int w = 0; w < wave; ++w) id += s_wave[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!f[k]) continue;
        const long i = base + k;
        a.rid[i] = id;
        if (a.table && id < a.max_regions) {
            long long* row = a.table + 8L * id;
            const int y = (int)(i / a.W), x = (int)(i - (long)y * a.W);
            row[0] = a.label[i]; row[1] = 0; row[2] = y; row[3] = x; row[4] = y; row[5] = x; row[6] = 0; row[7] = i;
        }
        ++id;
    }
}

// ----------------------------------------------------------------------------------------------------------------------- stats
struct RgHash {
    int key[RG_SLOTS];
    unsigned int area[RG_SLOTS];
    int x0[RG_SLOTS], x1[RG_SLOTS], y1[RG_SLOTS], cls[RG_SLOTS];
    unsigned long long sum[RG_SLOTS];
};

// the slot of `key`: linear probing; a pass holds at most RG_PASS + 1 keys in RG_SLOTS slots, so a free slot always turns up
__device__ __forceinline__ int rg_slot(int* keys, int key) {
    unsigned int s = ((unsigned int)key * 2654435761u) >> 22;
    for (;;) {
        const int k = atomicCAS(&keys[s], RG_EMPTY, key);
        if (k == RG_EMPTY || k == key) return (int)s;
        s = (s + 1) & (RG_SLOTS - 1);
    }
}
__device__ __forceinline__ void rg_put(RgHash& h, int key, int cls, unsigned int cnt, int x0, int x1, int y1, unsigned long long sum) {
    const int s = rg_slot(h.key, key);
    atomicAdd(&h.area[s], cnt);
    atomicMin(&h.x0[s], x0);
    atomicMax(&h.x1[s], x1);
    atomicMax(&h.y1[s], y1);
    if (sum) atomicAdd(&h.sum[s], sum);
    h.cls[s] = cls;
}

__global__ __launch_bounds__(RG_THREADS) void rg_stats_kernel(const RegArgs a, const int npass) {
    __shared__ RgHash h;
    __shared__ unsigned int s_cnt[257];
    __shared__ unsigned long long s_sum[257];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool hashing = a.table != nullptr || a.stats != nullptr;
    if (a.stats) {
        for (int i = tid; i <= a.C; i += RG_THREADS) { s_cnt[i] = 0u; s_sum[i] = 0ull; }
    }
    for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        if (hashing) {
            for (int s = tid; s < RG_SLOTS; s += RG_THREADS) {
                h.key[s] = RG_EMPTY; h.area[s] = 0u; h.x0[s] = INT_MAX; h.x1[s] = -1; h.y1[s] = -1; h.sum[s] = 0ull;
            }
            __syncthreads();
        }
        const long i0 = (long)pass * RG_PASS + 2 * tid;
        int key[2], cls[2], y[2], x[2];
        unsigned long long q[2];
        bool use[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long i = i0 + k;
            key[k] = RG_EMPTY; cls[k] = 0; y[k] = 0; x[k] = 0; q[k] = 0ull; use[k] = false;
            if (i >= a.N) continue;
            const int p = a.parent[i];
            const int id = p < 0 ? -1 : a.rid[p];
            if (a.region) a.region[i] = id;
            if (!hashing) continue;
            key[k] = p < 0 ? RG_IGN : id;
            cls[k] = p < 0 ? a.C : (int)a.label[i];
            y[k] = (int)(i / a.W);
            x[k] = (int)(i - (long)y[k] * a.W);
            if (a.conf) q[k] = (unsigned long long)(long long)rintf(a.conf[i] * 16777216.f);
            use[k] = a.stats != nullptr || (id >= 0 && id < a.max_regions);
        }
        if (hashing) {
            const int first = __builtin_amdgcn_readfirstlane(key[0]);
            if (first != RG_EMPTY && __ballot(key[0] != first || key[1] != first) == 0ull) {
                // the wave's 128 pixels are one key: reduce across the lanes, one insert
                int mx0 = x[0] < x[1] ? x[0] : x[1], mx1 = x[0] > x[1] ? x[0] : x[1], my1 = y[1];
                unsigned long long sum = q[0] + q[1];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const int t0 = __shfl_xor(mx0, o, 64), t1 = __shfl_xor(mx1, o, 64), t2 = __shfl_xor(my1, o, 64);
                    mx0 = t0 < mx0 ? t0 : mx0; mx1 = t1 > mx1 ? t1 : mx1; my1 = t2 > my1 ? t2 : my1;
                    sum += __shfl_xor(sum, o, 64);
                }
                if (lane == 0 && use[0]) rg_put(h, first, cls[0], 128u, mx0, mx1, my1, sum);
            } else if (key[0] != RG_EMPTY && key[0] == key[1]) {
                if (use[0]) rg_put(h, key[0], cls[0], 2u, x[0] < x[1] ? x[0] : x[1], x[0] > x[1] ? x[0] : x[1], y[1], q[0] + q[1]);
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (key[k] != RG_EMPTY && use[k]) rg_put(h, key[k], cls[k], 1u, x[k], x[k], y[k], q[k]);
            }
            __syncthreads();
            for (int s = tid; s < RG_SLOTS; s += RG_THREADS) {
                const int k = h.key[s];
                if (k == RG_EMPTY) continue;
                if (a.stats) {
                    atomicAdd(&s_cnt[h.cls[s]], h.area[s]);
                    if (h.sum[s]) atomicAdd(&s_sum[h.cls[s]], h.sum[s]);
                }
                if (a.table && k >= 0 && k < a.max_regions) {
                    long long* row = a.table + 8L * k;
                    atomicAdd(reinterpret_cast<unsigned long long*>(row + 1), (unsigned long long)h.area[s]);
                    // the box columns only fall / rise: a value that would not move what is stored (even a stale read of it) is skipped
                    if (h.x0[s] < __hip_atomic_load(row + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                        __hip_atomic_fetch_min(row + 3, (long long)h.x0[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h.y1[s] > __hip_atomic_load(row + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                        __hip_atomic_fetch_max(row + 4, (long long)h.y1[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h.x1[s] > __hip_atomic_load(row + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                        __hip_atomic_fetch_max(row + 5, (long long)h.x1[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h.sum[s]) atomicAdd(reinterpret_cast<unsigned long long*>(row + 6), h.sum[s]);
                }
            }
            __syncthreads();
        }
    }
    if (a.stats) {
        __syncthreads();
        for (int i = tid; i <= a.C; i += RG_THREADS) {
            if (s_cnt[i]) {
                atomicAdd(&a.stats[i], (unsigned long long)s_cnt[i]);
                atomicAdd(&a.stats[a.C + 1 + i], s_sum[i]);
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------------- clean
struct CleanArgs {
    const unsigned char* label;
    const int* region;
    const int* n;
    const long long* table;
    unsigned char* out;
    unsigned long long* changed;
    int* votes;                              // rows x C
    int* area_x;                             // N - rows: the areas of regions rows, rows + 1, ...
    int* newcls;                             // rows
    long long min_area;
    int H, W, C, rows;
    long N;
};

__device__ __forceinline__ bool rc_kept(const CleanArgs& c, int r) {
    const long long area = r < c.rows ? c.table[8L * r + 1] : (long long)c.area_x[r - c.rows];
    return area >= c.min_area;
}

// the areas of the regions the table has no row for; nothing to do when every region has one
__global__ __launch_bounds__(RG_THREADS) void rc_count_kernel(const CleanArgs c, const int npass) {
    __shared__ int s_key[RG_SLOTS];
    __shared__ unsigned int s_area[RG_SLOTS];
    if (*c.n <= c.rows) return;
    const int tid = threadIdx.x;
    for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) {
        for (int s = tid; s < RG_SLOTS; s += RG_THREADS) { s_key[s] = RG_EMPTY; s_area[s] = 0u; }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const long i = (long)pass * RG_PASS + 2 * tid + k;
            if (i >= c.N) continue;
            const int r = c.region[i];
            if (r >= c.rows) atomicAdd(&s_area[rg_slot(s_key, r)], 1u);
        }
        __syncthreads();
        for (int s = tid; s < RG_SLOTS; s += RG_THREADS)
            if (s_key[s] != RG_EMPTY) atomicAdd(&c.area_x[s_key[s] - c.rows], (int)s_area[s]);
        __syncthreads();
    }
}

// votes[r][class of q] += 1 for every pixel p of a small region r with a row and every 4-neighbour q of p in a kept region; a small
// region has fewer than min_area pixels, so a row collects at most 4 min_area increments
__global__ __launch_bounds__(RG_THREADS) void rc_vote_kernel(const CleanArgs c) {
    for (long i = (long)blockIdx.x * RG_THREADS + threadIdx.x; i < c.N; i += (long)gridDim.x * RG_THREADS) {
        const int r = c.region[i];
        if (r < 0 || r >= c.rows || rc_kept(c, r)) continue;
        const int y = (int)(i / c.W), x = (int)(i - (long)y * c.W);
        const long nb[4] = {y > 0 ? i - c.W : -1, x > 0 ? i - 1 : -1, x + 1 < c.W ? i + 1 : -1, y + 1 < c.H ? i + c.W : -1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (nb[k] < 0) continue;
            const int rq = c.region[nb[k]];
            if (rq < 0 || rq == r || !rc_kept(c, rq)) continue;
            const int lq = c.label[nb[k]];
            if (lq < c.C) atomicAdd(&c.votes[(long)r * c.C + lq], 1);
        }
    }
}

__global__ __launch_bounds__(RG_THREADS) void rc_decide_kernel(const CleanArgs c) {
    __shared__ unsigned long long s_ch[2];
    if (threadIdx.x < 2) s_ch[threadIdx.x] = 0ull;
    __syncthreads();
    const int n = *c.n < c.rows ? *c.n : c.rows;
    for (long r = (long)blockIdx.x * RG_THREADS + threadIdx.x; r < n; r += (long)gridDim.x * RG_THREADS) {
        int win = -1;
        const long long area = c.table[8L * r + 1];
        if (area < c.min_area) {
            int best = 0;
            for (int k = 0; k < c.C; ++k) {
                const int v = c.votes[r * c.C + k];
                if (v > best) { best = v; win = k; }
            }
        }
        c.newcls[r] = win;
        if (win >= 0) {
            atomicAdd(&s_ch[0], 1ull);
            atomicAdd(&s_ch[1], (unsigned long long)area);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_ch[threadIdx.x]) atomicAdd(&c.changed[threadIdx.x], s_ch[threadIdx.x]);
}

// label_out may be label itself: a thread reads and writes its own pixel only
__global__ __launch_bounds__(RG_THREADS) void rc_apply_kernel(const CleanArgs c) {
    for (long i = (long)blockIdx.x * RG_THREADS + threadIdx.x; i < c.N; i += (long)gridDim.x * RG_THREADS) {
        const int r = c.region[i];
        int l = c.label[i];
        if (r >= 0 && r < c.rows) {
            const int w = c.newcls[r];
            if (w >= 0) l = w;
        }
        c.out[i] = (unsigned char)l;
    }
}

inline long rg_up(long v) { return (v + 255) & ~255L; }
inline int rg_grid(long n, int per) {
    const long g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g > RG_MAX_GRID ? RG_MAX_GRID : g));
}

bool rg_desc_ok(const dupl_seg_regions_desc* d) {
    if (!d || d->struct_size != sizeof(dupl_seg_regions_desc)) return false;
    if (d->H <= 0 || d->W <= 0 || (long)d->H * d->W > 0x7ffffff0L) return false;
    if (d->C < 1 || d->C > DUPL_SEG_REGIONS_MAX_C || (d->connectivity != 4 && d->connectivity != 8)) return false;
    if (d->ignore_index < 0 || d->ignore_index > 255 || d->max_regions < 0 || d->reserved0 != 0) return false;
    return true;
}
bool rc_desc_ok(const dupl_seg_regions_clean_desc* d) {
    if (!d || d->struct_size != sizeof(dupl_seg_regions_clean_desc)) return false;
    if (d->H <= 0 || d->W <= 0 || (long)d->H * d->W > 0x7ffffff0L) return false;
    if (d->C < 1 || d->C > DUPL_SEG_REGIONS_MAX_C || d->max_regions < 1 || d->min_area < 0 || d->reserved0 != 0) return false;
    return true;
}
inline long rc_rows(const dupl_seg_regions_clean_desc* d) {
    const long N = (long)d->H * d->W;
    return d->max_regions < N ? d->max_regions : N;
}

}  // namespace

extern "C" int64_t dupl_seg_regions_workspace(const dupl_seg_regions_desc* d) {
    if (!rg_desc_ok(d)) return -1;
    const long N = (long)d->H * d->W, nb = (N + RG_CHUNK - 1) / RG_CHUNK;
    return 2 * rg_up(4 * N) + rg_up(4 * (nb + 1));
}

extern "C" int dupl_seg_regions(const dupl_seg_regions_desc* d, dupl_stream_t stream) {
    if (!rg_desc_ok(d) || !d->label) return DUPL_ERR_ARG;
    if (!d->region && !d->n_regions && !d->table && !d->stats) return DUPL_ERR_ARG;
    if (d->table && d->max_regions < 1) return DUPL_ERR_ARG;
    if (!d->workspace || (reinterpret_cast<unsigned long long>(d->workspace) & 7ull) || d->workspace_bytes < dupl_seg_regions_workspace(d))
        return DUPL_ERR_ARG;
    const long N = (long)d->H * d->W, nb = (N + RG_CHUNK - 1) / RG_CHUNK;
    char* ws = static_cast<char*>(d->workspace);
    RegArgs a;
    a.label = d->label; a.conf = d->conf; a.region = d->region; a.n_out = d->n_regions; a.table = (long long*)d->table;
    a.stats = (unsigned long long*)d->stats;
    a.parent = reinterpret_cast<int*>(ws);
    a.rid = d->region ? d->region : reinterpret_cast<int*>(ws + rg_up(4 * N));
    a.bsum = reinterpret_cast<int*>(ws + 2 * rg_up(4 * N));
    a.n_ws = a.bsum + nb;
    a.H = d->H; a.W = d->W; a.C = d->C; a.conn8 = d->connectivity == 8; a.ignore = d->ignore_index; a.max_regions = d->max_regions;
    a.tiles_x = (d->W + RG_TW - 1) / RG_TW; a.tiles_y = (d->H + RG_TH - 1) / RG_TH; a.nb = (int)nb; a.N = N;
    hipStream_t s = (hipStream_t)stream;
    DUPL_LAUNCH(rg_local_kernel, dim3((unsigned)((long)a.tiles_x * a.tiles_y)), dim3(RG_THREADS), 0, s, a);
    const long seam = (long)(a.tiles_y - 1) * a.W + (long)(a.tiles_x - 1) * a.H;
    if (seam > 0) DUPL_LAUNCH(rg_seam_kernel, dim3(rg_grid(seam, RG_THREADS)), dim3(RG_THREADS), 0, s, a);
    DUPL_LAUNCH(rg_flatten_kernel, dim3((unsigned)nb), dim3(RG_THREADS), 0, s, a);
    DUPL_LAUNCH(rg_scan_kernel, dim3(1), dim3(RG_THREADS), 0, s, a);
    if (d->region || d->table || d->stats) {
        DUPL_LAUNCH(rg_number_kernel, dim3((unsigned)nb), dim3(RG_THREADS), 0, s, a);
        const long npass = (N + RG_PASS - 1) / RG_PASS;
        DUPL_LAUNCH(rg_stats_kernel, dim3(rg_grid(npass, 1)), dim3(RG_THREADS), 0, s, a, (int)npass);
    }
    return dupl_launch_status();
}

extern "C" int64_t dupl_seg_regions_clean_workspace(const dupl_seg_regions_clean_desc* d) {
    if (!rc_desc_ok(d)) return -1;
    const long N = (long)d->H * d->W, rows = rc_rows(d);
    return rg_up(4 * rows * d->C + 4 * (N - rows)) + rg_up(4 * rows);
}

extern "C" int dupl_seg_regions_clean(const dupl_seg_regions_clean_desc* d, dupl_stream_t stream) {
    if (!rc_desc_ok(d)) return DUPL_ERR_ARG;
    if (!d->label || !d->region || !d->n_regions || !d->table || !d->label_out || !d->changed) return DUPL_ERR_ARG;
    if (!d->workspace || (reinterpret_cast<unsigned long long>(d->workspace) & 7ull) || d->workspace_bytes < dupl_seg_regions_clean_workspace(d))
        return DUPL_ERR_ARG;
    const long N = (long)d->H * d->W, rows = rc_rows(d);
    char* ws = static_cast<char*>(d->workspace);
    CleanArgs c;
    c.label = d->label; c.region = d->region; c.n = d->n_regions; c.table = (const long long*)d->table; c.out = d->label_out;
    c.changed = (unsigned long long*)d->changed;
    c.votes = reinterpret_cast<int*>(ws);
    c.area_x = c.votes + rows * d->C;
    c.newcls = reinterpret_cast<int*>(ws + rg_up(4 * rows * d->C + 4 * (N - rows)));
    c.min_area = d->min_area; c.H = d->H; c.W = d->W; c.C = d->C; c.rows = (int)rows; c.N = N;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)(4 * rows * d->C + 4 * (N - rows)), s) != hipSuccess) return DUPL_ERR_LAUNCH;
    if (hipMemsetAsync(d->changed, 0, 2 * sizeof(int64_t), s) != hipSuccess) return DUPL_ERR_LAUNCH;
    const long npass = (N + RG_PASS - 1) / RG_PASS;
    if (N > rows) DUPL_LAUNCH(rc_count_kernel, dim3(rg_grid(npass, 1)), dim3(RG_THREADS), 0, s, c, (int)npass);
    DUPL_LAUNCH(rc_vote_kernel, dim3(rg_grid(N, RG_THREADS)), dim3(RG_THREADS), 0, s, c);
    DUPL_LAUNCH(rc_decide_kernel, dim3(rg_grid(rows, RG_THREADS)), dim3(RG_THREADS), 0, s, c);
    DUPL_LAUNCH(rc_apply_kernel, dim3(rg_grid(N, RG_THREADS)), dim3(RG_THREADS), 0, s, c);
    return dupl_launch_status();
}
