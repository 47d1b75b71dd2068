// Boundary scores of one (gt, pred) pair of (H,W) int64 label maps (tools/eval_seg --boundary 1; beyond the reference, which scores
// the confusion matrix only): the trimap band histogram band_hist[min(dist(gt), R+1) - 1][gt][pred] and the Boundary IoU counters
// I / G / P per class at distance d (Cheng et al., CVPR 2021), where dist(L)[p] is the Chebyshev distance from p to the nearest pixel
// inside the image whose label differs from L[p].  dupl_seg_boundary, three launches, no host synchronisation:
//   pack     the two int64 maps are read from HBM ONCE and compacted to bytes (anything outside [0, nc) becomes BD_INVALID);
//   row      hx[p] = the distance along the row to the nearest differently-labelled pixel, capped at M + 1, M = max(R, d): a wave
//            per 64 pixels of a row; three ballots of "differs from its left neighbour" cover the pixels and 64 on either side, and
//            the nearest change on each side is a bit scan.  Written as label | hx << 8, 2 B per pixel and map;
//   column   dist[p] = min(hx[p], min over 1 <= |dy| <= M of (L[y+dy,x] != L[y,x] ? |dy| : max(|dy|, hx[y+dy,x]))), stopped as soon as
//            |dy| reaches the running minimum: a 64 x 16 tile of label | hx of both maps plus a halo of M rows in LDS.  The same
//            kernel counts: (bin, gt, pred) keys are combined per wave (the lanes that share the first live lane's key insert once),
//            then per workgroup in an LDS hash table (2048 slots for at most 1024 keys), the 3 nc Boundary IoU counters in a small LDS
//            array; one global 64-bit atomic per distinct key and workgroup.
// Positions outside the image are never read from memory: every load and every scan step tests its coordinate against the image first.  Labels index
// the counters only after the pack kernel has mapped them into [0, nc) or to BD_INVALID, and BD_INVALID pixels are skipped.  Integer
// atomics only, no workgroup waits for another (the hash probe ends because the table has more slots than a tile has pixels):
// every output is bit-reproducible.
#include "common.h"
#include "../../include/dupl_hip.h"

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_INVALID = 255;              // the byte of every gt / pred value outside [0, nc); nc <= 255 keeps it free
constexpr int BD_STAGE = 5;                  // rows a wave of the column kernel loads before it stores them to LDS
constexpr int BD_TW = 64, BD_TH = 16;        // column kernel: tile
constexpr int BD_MAXD = DUPL_SEG_BOUNDARY_MAX_DIST;
constexpr int BD_SLOTS = 2048;               // twice the keys a tile can hold
constexpr int BD_EMPTY = -1;
constexpr int BD_MAX_GRID = 2048;

struct BdArgs {
    const long long* gt;
    const long long* pred;
    unsigned char* lab[2];                   // N bytes each: gt, pred
    unsigned short* lh[2];                   // N each: label | hx << 8, hx = the distance along the row capped at M + 1
    unsigned char* dist[2];                  // optional outputs, capped at R + 1
    unsigned long long* band;                // (R+1, nc, nc)
    unsigned long long* biou;                // (3, nc); or null
    int H, W, nc, R, d, M;
    long N;
};

__device__ __forceinline__ unsigned int bd_byte(long long v, int nc) { return (v >= 0 && v < nc) ? (unsigned int)v : (unsigned int)BD_INVALID; }

// ------------------------------------------------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(BD_THREADS) void bd_pack_kernel(const BdArgs a) {
    const long nq = (a.N + 3) / 4;
    for (long q = (long)blockIdx.x * BD_THREADS + threadIdx.x; q < nq; q += (long)gridDim.x * BD_THREADS) {
        const long i0 = 4 * q;
        unsigned int wg = 0u, wp = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= a.N) continue;
            wg |= bd_byte(a.gt[i0 + k], a.nc) << (8 * k);
            wp |= bd_byte(a.pred[i0 + k], a.nc) << (8 * k);
        }
        if (i0 + 3 < a.N) {                  // the byte maps start 256-byte aligned and i0 is a multiple of 4
            *reinterpret_cast<unsigned int*>(a.lab[0] + i0) = wg;
            *reinterpret_cast<unsigned int*>(a.lab[1] + i0) = wp;
        } else {
            for (int k = 0; i0 + k < a.N; ++k) {
                a.lab[0][i0 + k] = (unsigned char)(wg >> (8 * k));
                a.lab[1][i0 + k] = (unsigned char)(wp >> (8 * k));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------- row
// A wave owns 64 consecutive pixels of one row of one map.  Bit i of a ballot says that the pixel at position i of a 64-pixel chunk
// differs from its left neighbour (both inside the row); three ballots cover the chunk and the 64 pixels on either side, which is the
// whole search range (M <= 64).  The nearest label change to the left of a lane is the highest set bit at or below it, to the right the
// lowest set bit above it: two bit scans per side, no loop and no LDS.  Writes label | hx << 8.
__device__ __forceinline__ bool bd_differs(const unsigned char* __restrict__ row, int p, int W) {
    return p >= 1 && p < W && row[p] != row[p - 1];
}

__global__ __launch_bounds__(BD_THREADS) void bd_row_kernel(const BdArgs a) {
    const int lane = threadIdx.x & 63, chunks = (a.W + 63) / 64;
    const long per_map = (long)a.H * chunks;
    for (long it = (long)blockIdx.x * (BD_THREADS / 64) + (threadIdx.x >> 6); it < 2 * per_map; it += (long)gridDim.x * (BD_THREADS / 64)) {
        const int m = it >= per_map;
        const long rem = it - m * per_map;
        const int y = (int)(rem / chunks), p = (int)(rem % chunks) * 64 + lane;
        const unsigned char* row = a.lab[m] + (long)y * a.W;
        const unsigned long long dl = __ballot(bd_differs(row, p - 64, a.W)), dc = __ballot(bd_differs(row, p, a.W)),
                                 dr = __ballot(bd_differs(row, p + 64, a.W));
        int h = a.M + 1;
        const unsigned long long lc = dc & (~0ull >> (63 - lane));                 // changes at or left of this lane
        if (lc) h = lane - (63 - __clzll((long long)lc)) + 1;
        else if (dl) h = lane + 64 - (63 - __clzll((long long)dl)) + 1;
        const unsigned long long rc = lane < 63 ? dc & (~0ull << (lane + 1)) : 0ull; // changes right of this lane
        int right = a.M + 1;
        if (rc) right = __ffsll((long long)rc) - 1 - lane;
        else if (dr) right = 64 + __ffsll((long long)dr) - 1 - lane;
        h = right < h ? right : h;
        h = h < a.M + 1 ? h : a.M + 1;
        if (p < a.W) a.lh[m][(long)y * a.W + p] = (unsigned short)(row[p] | (h << 8));
    }
}

// ---------------------------------------------------------------------------------------------------------------------- column
// the slot of `key`: linear probing; a tile holds at most BD_TW BD_TH keys in BD_SLOTS slots, so a free slot always turns up
__device__ __forceinline__ int bd_slot(int* keys, int key) {
    unsigned int s = ((unsigned int)key * 2654435761u) >> 21;
    for (;;) {
        const int k = atomicCAS(&keys[s], BD_EMPTY, key);
        if (k == BD_EMPTY || k == key) return (int)s;
        s = (s + 1) & (BD_SLOTS - 1);
    }
}

// s: label | hx << 8 of one map, LDS rows of BD_TW; `at` the pixel in it, y its image row.  Four steps of the search are read together:
// a step k >= the running minimum cannot lower it (its value is >= k), so reading ahead changes nothing; k is held at M, the staged halo.
__device__ __forceinline__ int bd_col_dist(const unsigned short* s, int at, int y, int H, int M) {
    const unsigned int l = s[at] & 255u;
    int dist = s[at] >> 8;                   // <= M + 1
    for (int k0 = 1; k0 < dist; k0 += 4) {
        unsigned int up[4], dn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j < M ? k0 + j : M;
            up[j] = s[at - k * BD_TW];
            dn[j] = s[at + k * BD_TW];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j < M ? k0 + j : M;
            if (y - k >= 0) {                // rows outside the image were staged as zeros and are not looked at
                const int h = (int)(up[j] >> 8), v = (up[j] & 255u) != l ? k : (h > k ? h : k);
                dist = v < dist ? v : dist;
            }
            if (y + k < H) {
                const int h = (int)(dn[j] >> 8), v = (dn[j] & 255u) != l ? k : (h > k ? h : k);
                dist = v < dist ? v : dist;
            }
        }
    }
    return dist;
}

__global__ __launch_bounds__(BD_THREADS) void bd_col_kernel(const BdArgs a) {
    __shared__ unsigned short s_lh[2][(BD_TH + 2 * BD_MAXD) * BD_TW];
    __shared__ int s_key[BD_SLOTS];
    __shared__ unsigned int s_cnt[BD_SLOTS];
    __shared__ unsigned int s_biou[3 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, M = a.M;
    const int tiles_x = (a.W + BD_TW - 1) / BD_TW;
    const int tx0 = (int)(blockIdx.x % tiles_x) * BD_TW, ty0 = (int)(blockIdx.x / tiles_x) * BD_TH;
    for (int s = tid; s < BD_SLOTS; s += BD_THREADS) { s_key[s] = BD_EMPTY; s_cnt[s] = 0u; }
    for (int i = tid; i < 3 * 256; i += BD_THREADS) s_biou[i] = 0u;
    // a wave stages BD_STAGE rows per step, their loads in flight together; what lies outside the image is staged as zero
    const int rows = BD_TH + 2 * M, x = tx0 + lane;
    for (int r0 = wave; r0 < rows; r0 += BD_STAGE * (BD_THREADS / 64)) {
        unsigned short v[BD_STAGE][2];
#pragma unroll
        for (int u = 0; u < BD_STAGE; ++u) {
            const int y = ty0 - M + r0 + u * (BD_THREADS / 64);
            const bool in = y >= 0 && y < a.H && x < a.W;
            v[u][0] = in ? a.lh[0][(long)y * a.W + x] : (unsigned short)0;
            v[u][1] = in ? a.lh[1][(long)y * a.W + x] : (unsigned short)0;
        }
#pragma unroll
        for (int u = 0; u < BD_STAGE; ++u) {
            const int r = r0 + u * (BD_THREADS / 64);
            if (r < rows) { s_lh[0][r * BD_TW + lane] = v[u][0]; s_lh[1][r * BD_TW + lane] = v[u][1]; }
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < BD_TH / (BD_THREADS / 64); ++k) {
        const int ty = wave + k * (BD_THREADS / 64), y = ty0 + ty, ly = ty + M;
        int key = BD_EMPTY;
        if (y < a.H && x < a.W) {
            const int dg = bd_col_dist(s_lh[0], ly * BD_TW + lane, y, a.H, M);
            const int dp = bd_col_dist(s_lh[1], ly * BD_TW + lane, y, a.H, M);
            const long g = (long)y * a.W + x;
            if (a.dist[0]) a.dist[0][g] = (unsigned char)(dg < a.R + 1 ? dg : a.R + 1);
            if (a.dist[1]) a.dist[1][g] = (unsigned char)(dp < a.R + 1 ? dp : a.R + 1);
            const int lg = s_lh[0][ly * BD_TW + lane] & 255, lp = s_lh[1][ly * BD_TW + lane] & 255;
            if (lg != BD_INVALID && lp != BD_INVALID) {          // both below nc from here on
                const int bin = (dg < a.R + 1 ? dg : a.R + 1) - 1;
                key = (bin * a.nc + lg) * a.nc + lp;
                if (a.biou) {
                    int edge = x < y ? x : y;
                    edge = a.W - 1 - x < edge ? a.W - 1 - x : edge;
                    edge = a.H - 1 - y < edge ? a.H - 1 - y : edge;
                    const bool gb = (dg < edge + 1 ? dg : edge + 1) <= a.d, pb = (dp < edge + 1 ? dp : edge + 1) <= a.d;
                    if (gb && pb && lg == lp) atomicAdd(&s_biou[lg], 1u);
                    if (gb) atomicAdd(&s_biou[256 + lg], 1u);
                    if (pb) atomicAdd(&s_biou[512 + lp], 1u);
                }
            }
        }
        // per-wave combine: the lanes that carry the first live lane's key leave together, with one insert
        unsigned long long live = __ballot(key != BD_EMPTY);
        while (live) {
            const int lead = __ffsll((long long)live) - 1;
            const int kk = __shfl(key, lead, 64);
            const unsigned long long same = __ballot(key == kk);
            if (lane == lead) atomicAdd(&s_cnt[bd_slot(s_key, kk)], (unsigned int)__popcll(same));
            live &= ~same;
        }
    }
    __syncthreads();
    for (int s = tid; s < BD_SLOTS; s += BD_THREADS)
        if (s_key[s] != BD_EMPTY) atomicAdd(&a.band[s_key[s]], (unsigned long long)s_cnt[s]);
    if (a.biou) {
        for (int i = tid; i < 3 * 256; i += BD_THREADS) {
            const int row = i >> 8, c = i & 255;
            if (c < a.nc && s_biou[i]) atomicAdd(&a.biou[row * a.nc + c], (unsigned long long)s_biou[i]);
        }
    }
}

inline long bd_up(long n) { return (n + 255) & ~255L; }

bool bd_desc_ok(const dupl_seg_boundary_desc* d) {
    if (!d || d->struct_size != sizeof(dupl_seg_boundary_desc)) return false;
    if (d->H < 1 || d->W < 1 || (long)d->H * d->W > 0x7ffffff0L) return false;
    if (d->num_classes < 1 || d->num_classes > DUPL_SEG_BOUNDARY_MAX_C) return false;
    if (d->max_dist < 1 || d->max_dist > BD_MAXD || d->biou_dist < 0 || d->biou_dist > BD_MAXD) return false;
    return true;
}

}  // namespace

extern "C" int64_t dupl_seg_boundary_workspace(const dupl_seg_boundary_desc* d) {
    if (!bd_desc_ok(d)) return -1;
    return 6 * bd_up((long)d->H * d->W);
}

extern "C" int dupl_seg_boundary(const dupl_seg_boundary_desc* d, dupl_stream_t stream) {
    if (!bd_desc_ok(d) || !d->gt || !d->pred || !d->band_hist) return DUPL_ERR_ARG;
    if (d->biou_dist > 0 && !d->biou) return DUPL_ERR_ARG;
    if (!d->workspace || (reinterpret_cast<unsigned long long>(d->workspace) & 3ull) || d->workspace_bytes < dupl_seg_boundary_workspace(d))
        return DUPL_ERR_ARG;
    BdArgs a;
    a.N = (long)d->H * d->W;
    unsigned char* ws = static_cast<unsigned char*>(d->workspace);
    const long part = bd_up(a.N);           // lab[0], lab[1]: one part each; lh[0], lh[1]: two parts each
    unsigned short* lh = reinterpret_cast<unsigned short*>(ws + 2 * part);
    a.gt = (const long long*)d->gt; a.pred = (const long long*)d->pred;
    a.lab[0] = ws; a.lab[1] = ws + part; a.lh[0] = lh; a.lh[1] = lh + part;
    a.dist[0] = d->dist_gt; a.dist[1] = d->dist_pred;
    a.band = (unsigned long long*)d->band_hist;
    a.biou = d->biou_dist > 0 ? (unsigned long long*)d->biou : nullptr;
    a.H = d->H; a.W = d->W; a.nc = d->num_classes; a.R = d->max_dist; a.d = d->biou_dist;
    a.M = a.R > a.d ? a.R : a.d;
    hipStream_t s = (hipStream_t)stream;
    long pg = ((a.N + 3) / 4 + BD_THREADS - 1) / BD_THREADS;
    if (pg > BD_MAX_GRID) pg = BD_MAX_GRID;
    DUPL_LAUNCH(bd_pack_kernel, dim3((unsigned)pg), dim3(BD_THREADS), 0, s, a);
    // the column kernel: one workgroup per tile, numbered row-major in x
    long row_grid = (2L * a.H * ((a.W + 63) / 64) + BD_THREADS / 64 - 1) / (BD_THREADS / 64);
    if (row_grid > BD_MAX_GRID) row_grid = BD_MAX_GRID;
    const long col_tiles = (long)((a.W + BD_TW - 1) / BD_TW) * ((a.H + BD_TH - 1) / BD_TH);
    DUPL_LAUNCH(bd_row_kernel, dim3((unsigned)row_grid), dim3(BD_THREADS), 0, s, a);
    DUPL_LAUNCH(bd_col_kernel, dim3((unsigned)col_tiles), dim3(BD_THREADS), 0, s, a);
    return dupl_launch_status();
}
