// Lesion tables: the connected components of `planes` mask planes as measured rows (count, voxels, extent, centroid sums, largest 3-D and in-slice
// diameters with the pairs that attain them, the perpendicular in-slice extent), an optional label volume, and the joint histogram of two label volumes.
// Launches of rsuper_lesion_table, plane = blockIdx.y (blockIdx.z in lt_pair3), launches being the only synchronisation between them:
//   lt_label    ccl.hpp tile pass; zeroes the size words of the tile and, in block 0, the plane's counters
//   lt_merge    ccl.hpp border pass
//   lt_size     path compression; size[root] += run length (one atomic per run of equal roots in a wave); foreground count
//   lt_roots    every root of >= min_voxels voxels appends the key (size << 32) | (0xFFFFFFFF - root) to the plane's list, the others are counted
//   lt_select   one block per plane: the K largest keys by an 8 x 8-bit radix select, ranked; rows initialised, size[root] = marker | row
//   lt_stats    labels; bounding box and coordinate sums per row (LDS, then one global atomic per block and field); candidate counts
//   lt_scan     exclusive scans of the candidate counts: per (row, slice) for the in-slice search, per row for the 3-D search
//   lt_scatter  candidates compacted into their segments
//   lt_pair2    per slice and row: the in-slice pair search in LDS tiles
//   lt_pair3    per row: the 3-D pair search in LDS tiles, tile pairs dealt to LT_G3 blocks
//   lt_final    per row: the partial results reduced, b measured in the slice of (pa, qa), rows finished
// Candidates.  The squared distance to a fixed point is strictly convex along a line, so a voxel whose two neighbours along an axis both belong to its
// component is never an endpoint of a pair of maximal distance: the pair with the farther neighbour is strictly longer.  The 3-D search keeps the
// voxels for which this holds along no axis, the in-slice search those for which it holds along neither y nor x (the z neighbours are not in the
// slice).  Every attaining pair survives, so the maximum and the lexicographically smallest attaining pair are those of the full component.
// Squared distances are (q0 dz^2 + q1 dy^2) + q2 dx^2 with every product and sum rounded on its own, never an FMA: two pairs with the same
// |dz|, |dy|, |dx| tie exactly, and the tie set is the one a float64 numpy expression of the same form has.  hipcc contracts a * b + c by default,
// also when the product comes out of __dmul_rn (a plain multiply in the HIP headers), so the Makefile builds this file with -ffp-contract=off and
// the pragma below says the same for the code of this file.
// Every cross-workgroup result is an integer atomic or a per-block slot reduced in a fixed order: the outputs do not depend on the schedule.
#include "common.hpp"
#include "ccl.hpp"
#include "../../include/rsuper_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = CCL_NT;
constexpr int GRID_CAP = 2048;                           // blocks of a grid-stride pass
constexpr int LT_MAX_PLANES = RSUPER_LESION_MAX_PLANES;
constexpr int LT_MAX_ROWS = RSUPER_LESION_TABLE_MAX_ROWS;
constexpr int LT_G3 = 64;                                // blocks that share the tile pairs of one row's 3-D search
constexpr uint32_t LT_MARK = 0xFFFFFF00u;                // size[root] of a component with a row: LT_MARK | row (sizes are <= 2^31)
constexpr uint32_t LT_C3 = 0x80000000u;                  // bit 31 of an in-slice candidate word: also a 3-D candidate (indices are < 2^31)
constexpr unsigned long long LT_BIG = 1ull << 40;        // above every coordinate
constexpr unsigned long long NO_PAIR = ~0ull;

struct LtState {                                         // 64 bytes per plane
    unsigned long long fg;                               // foreground voxels
    uint32_t n_list, dropped, nrows, pad[11];
};
static_assert(sizeof(LtState) == 64, "state layout");

// the plane's part of the workspace
struct LtPlane {
    uint32_t* parent;                                    // [ps]
    uint32_t* size;                                      // [ps] voxels per root; after lt_stats: the 3-D candidates
    unsigned long long* list;                            // [ps / 2] keys of the roots; after lt_select: the in-slice candidates, ps words
    uint8_t* lab;                                        // [ps] labels when the caller passes none
    LtState* st;
    uint32_t *cnt3, *off3, *cur3;                        // [256]
    uint32_t *off2, *cur2;                               // [rows * D]
    double* key2; unsigned long long* pair2;             // [rows * D]
    double* key3; unsigned long long* pair3;             // [rows * LT_G3]
};

struct LtLayout {
    long ps, kd, small_bytes, plane_bytes;
    LtLayout(long n, int D, int rows) {
        ps = (n + 63) & ~63L;
        kd = ((long)rows * D + 1) & ~1L;
        small_bytes = 64 + 3 * 256 * 4 + 2 * kd * 4 + 2 * kd * 8 + 2 * (long)rows * LT_G3 * 8;
        plane_bytes = 13 * ps + small_bytes;
    }
    __host__ __device__ LtPlane plane(void* ws, int p, int rows) const {
        char* b = (char*)ws + (long)p * plane_bytes;
        LtPlane q;
        q.parent = (uint32_t*)b;
        q.size = (uint32_t*)(b + 4 * ps);
        q.list = (unsigned long long*)(b + 8 * ps);
        q.lab = (uint8_t*)(b + 12 * ps);
        char* s = b + 13 * ps;
        q.st = (LtState*)s;                 s += 64;
        q.cnt3 = (uint32_t*)s;              s += 1024;
        q.off3 = (uint32_t*)s;              s += 1024;
        q.cur3 = (uint32_t*)s;              s += 1024;
        q.off2 = (uint32_t*)s;              s += kd * 4;
        q.cur2 = (uint32_t*)s;              s += kd * 4;
        q.key2 = (double*)s;                s += kd * 8;
        q.pair2 = (unsigned long long*)s;   s += kd * 8;
        q.key3 = (double*)s;                s += (long)rows * LT_G3 * 8;
        q.pair3 = (unsigned long long*)s;
        return q;
    }
};

struct LtArgs {
    void* ws;
    LtLayout lay;
    const uint8_t* masks;
    uint8_t* labels;                                     // null: the workspace copy
    long long* rows_i; double* rows_f; long long* totals;
    long n;
    int D, H, W, tiles_x, tiles_y, rows, min_voxels, max_candidates;
    double q0, q1, q2, s0, s1, s2;
    __device__ LtPlane plane(int p) const { return lay.plane(ws, p, rows); }
    __device__ uint8_t* lab(int p) const { return labels ? labels + (long)p * n : plane(p).lab; }
};

__device__ __forceinline__ double sqdist(int dz, int dy, int dx, double q0, double q1, double q2) {
    const double z = dz, y = dy, x = dx;
    return __dadd_rn(__dadd_rn(__dmul_rn(q0, __dmul_rn(z, z)), __dmul_rn(q1, __dmul_rn(y, y))), __dmul_rn(q2, __dmul_rn(x, x)));
}

// sqrt(x) rounded to nearest for x >= 0.  The compiler expands the f64 square root into a reciprocal square root refined twice; d3 and a are compared
// bit for bit with a correctly rounded host square root, so the result does not rest on that expansion being exact.  With r within an ulp of the root the
// residual e = x - r * r is exact in one FMA (x and r * r are multiples of ulp(r)^2 and differ by a few ulp(r) * r), and the root lies past the
// midpoint to the next double above, r + u / 2, exactly when e > r * u (e - r * u is a multiple of u^2, so the u^2 / 4 of the squared midpoint never
// decides); likewise below.  Two rounds cover a start two steps off.
__device__ __forceinline__ double sqrt_nearest(double x) {
    if (!(x > 0.0)) return x;
    double r = __dsqrt_rn(x);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = __fma_rn(-r, r, x);
        const double up = __longlong_as_double(__double_as_longlong(r) + 1), dn = __longlong_as_double(__double_as_longlong(r) - 1);
        if (e > __dmul_rn(r, up - r)) r = up;
        else if (e <= -__dmul_rn(r, r - dn)) r = dn;
    }
    return r;
}

// the better of two (squared distance, pair) results: the larger distance, then the smaller (p << 32) | q
__device__ __forceinline__ void take_better(double& k, unsigned long long& pr, double k2, unsigned long long pr2) {
    if (k2 > k || (k2 == k && pr2 < pr)) { k = k2; pr = pr2; }
}
__device__ __forceinline__ unsigned long long pair_of(uint32_t a, uint32_t b) {
    return a < b ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
}

// the block's best result, in every thread
__device__ __forceinline__ void block_best(double& k, unsigned long long& pr) {
    __shared__ double bk[NT / 64];
    __shared__ unsigned long long bp[NT / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take_better(k, pr, __shfl_xor(k, o, 64), __shfl_xor(pr, o, 64));
    __syncthreads();                                     // the arrays may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) { bk[threadIdx.x >> 6] = k; bp[threadIdx.x >> 6] = pr; }
    __syncthreads();
    k = bk[0]; pr = bp[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) take_better(k, pr, bk[w], bp[w]);
}

// length of the run of equal values that starts at this lane (0 for a lane that starts none); every lane of the wave calls it
__device__ __forceinline__ int run_length(uint32_t v) {
    const int lane = threadIdx.x & 63;
    const uint32_t prev = __shfl_up(v, 1, 64);
    const bool head = lane == 0 || prev != v;
    const unsigned long long heads = __ballot(head);
    if (!head) return 0;
    const unsigned long long higher = lane == 63 ? 0ull : heads >> (lane + 1);
    return higher ? __ffsll((long long)higher) : 64 - lane;
}

template <int CONN>
__global__ __launch_bounds__(NT) void lt_label_kernel(LtArgs a) {
    const LtPlane pl = a.plane(blockIdx.y);
    const uint8_t* m = a.masks + (long)blockIdx.y * a.n;
    ccl_label_tile<CONN>(pl.parent, blockIdx.x, a.tiles_x, a.tiles_y, a.D, a.H, a.W, [&](long gi) { return m[gi] != 0; });
    int oz, oy, ox;
    ccl_tile_origin(blockIdx.x, a.tiles_x, a.tiles_y, oz, oy, ox);
    for (int i = threadIdx.x; i < CCL_N; i += NT) {
        const int lx = i % CCL_X, t = i / CCL_X, ly = t % CCL_Y, lz = t / CCL_Y;
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        if (gz < a.D && gy < a.H && gx < a.W) pl.size[((long)gz * a.H + gy) * a.W + gx] = 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        LtState s = {};
        *pl.st = s;
    }
}

template <int CONN>
__global__ __launch_bounds__(NT) void lt_merge_kernel(LtArgs a) {
    ccl_link_borders<CONN>(a.plane(blockIdx.y).parent, blockIdx.x, a.tiles_x, a.tiles_y, a.D, a.H, a.W);
}

__global__ __launch_bounds__(NT) void lt_size_kernel(LtArgs a) {
    const LtPlane pl = a.plane(blockIdx.y);
    unsigned long long fg = 0;
    for (long base = (long)blockIdx.x * NT; base < a.n; base += (long)gridDim.x * NT) {      // whole waves stay in the loop: run_length shuffles
        const long i = base + threadIdx.x;
        const uint32_t r = i < a.n ? ccl_compress(pl.parent, i) : CCL_BG;
        const int len = run_length(r);
        if (len && r != CCL_BG) { atomicAdd(&pl.size[r], (uint32_t)len); fg += len; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fg += __shfl_xor(fg, o, 64);
    if ((threadIdx.x & 63) == 0 && fg) atomicAdd(&pl.st->fg, fg);
}

__global__ __launch_bounds__(NT) void lt_roots_kernel(LtArgs a) {
    const LtPlane pl = a.plane(blockIdx.y);
    const uint32_t cap = (uint32_t)(a.lay.ps / 2);       // >= ceil(n / 2) >= the number of components (no two 6-adjacent voxels are both roots)
    uint32_t dropped = 0;
    for (long base = (long)blockIdx.x * NT; base < a.n; base += (long)gridDim.x * NT) {
        const long i = base + threadIdx.x;
        if (i >= a.n || pl.parent[i] != (uint32_t)i) continue;
        const uint32_t s = pl.size[i];
        if (s < (uint32_t)a.min_voxels) { ++dropped; continue; }
        const uint32_t pos = atomicAdd(&pl.st->n_list, 1u);
        if (pos < cap) pl.list[pos] = ((unsigned long long)s << 32) | (0xFFFFFFFFull - (unsigned long long)i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dropped += __shfl_xor(dropped, o, 64);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&pl.st->dropped, dropped);
}

// One block per plane.  The K-th largest key by radix select (keys are distinct: they hold the root), the keys at or above it gathered and ranked.
__global__ __launch_bounds__(NT) void lt_select_kernel(LtArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long sel[LT_MAX_ROWS + 2], prefix_s;
    __shared__ uint32_t need_s, nsel;
    const int p = blockIdx.y;
    const LtPlane pl = a.plane(p);
    const uint32_t cap = (uint32_t)(a.lay.ps / 2);
    const uint32_t M = pl.st->n_list < cap ? pl.st->n_list : cap;
    const int K = M < (uint32_t)a.rows ? (int)M : a.rows;
    if (threadIdx.x == 0) { prefix_s = 0ull; need_s = (uint32_t)K; nsel = 0u; }
    __syncthreads();
    if (K > 0) {
        for (int b = 7; b >= 0; --b) {
            hist[threadIdx.x] = 0u;
            __syncthreads();
            const unsigned long long prefix = prefix_s;
            for (uint32_t i = threadIdx.x; i < M; i += NT) {
                const unsigned long long key = pl.list[i];
                if (b == 7 || (key >> (8 * (b + 1))) == prefix) atomicAdd(&hist[(key >> (8 * b)) & 255u], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t need = need_s;
                int d = 255;
                while (d > 0 && hist[d] < need) { need -= hist[d]; --d; }
                need_s = need;
                prefix_s = (prefix << 8) | (unsigned long long)d;
            }
            __syncthreads();
        }
        const unsigned long long kth = prefix_s;
        for (uint32_t i = threadIdx.x; i < M; i += NT) {
            const unsigned long long key = pl.list[i];
            if (key >= kth) {
                const uint32_t pos = atomicAdd(&nsel, 1u);
                if (pos < (uint32_t)LT_MAX_ROWS) sel[pos] = key;
            }
        }
        __syncthreads();
    }
    long long* ri = a.rows_i + (long)p * a.rows * 16;
    double* rf = a.rows_f + (long)p * a.rows * 4;
    for (int t = threadIdx.x; t < a.rows; t += NT) {
        if (t >= K) {
            for (int j = 0; j < 16; ++j) ri[t * 16 + j] = 0;
            for (int j = 0; j < 4; ++j) rf[t * 4 + j] = 0.0;
        }
    }
    if ((int)threadIdx.x < K) {
        const unsigned long long key = sel[threadIdx.x];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += sel[j] > key ? 1 : 0;
        const uint32_t root = (uint32_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
        long long* r = ri + rank * 16;
        r[0] = (long long)root; r[1] = (long long)(key >> 32);
        r[2] = r[3] = r[4] = (long long)LT_BIG;
        for (int j = 5; j < 16; ++j) r[j] = 0;
        pl.size[root] = LT_MARK | (uint32_t)rank;
    }
    for (long i = threadIdx.x; i < (long)K * a.D; i += NT) pl.cur2[i] = 0u;
    pl.cnt3[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        pl.st->nrows = (uint32_t)K;
        long long* t = a.totals + (long)p * 4;
        t[0] = (long long)pl.st->n_list; t[1] = (long long)pl.st->dropped; t[2] = (long long)pl.st->fg; t[3] = K;
    }
}

// bit 0: an in-slice candidate, bit 1: a 3-D candidate (see the head of the file); r is the root of voxel (z, y, x) = index i
__device__ __forceinline__ int candidate_bits(const uint32_t* par, uint32_t r, long i, int z, int y, int x, int D, int H, int W) {
    const long hw = (long)H * W;
    const bool bx = x > 0 && x < W - 1 && par[i - 1] == r && par[i + 1] == r;
    const bool by = y > 0 && y < H - 1 && par[i - W] == r && par[i + W] == r;
    if (bx || by) return 0;
    const bool bz = z > 0 && z < D - 1 && par[i - hw] == r && par[i + hw] == r;
    return bz ? 1 : 3;
}

__global__ __launch_bounds__(NT) void lt_stats_kernel(LtArgs a) {
    __shared__ int smin[3][256], smax[3][256];
    __shared__ unsigned long long ssum[3][256];
    const int p = blockIdx.y;
    const LtPlane pl = a.plane(p);
    uint8_t* lab = a.lab(p);
    for (int j = 0; j < 3; ++j) { smin[j][threadIdx.x] = 0x7FFFFFFF; smax[j][threadIdx.x] = -1; ssum[j][threadIdx.x] = 0ull; }
    __syncthreads();
    const long hw = (long)a.H * a.W;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < a.n; i += (long)gridDim.x * NT) {
        const uint32_t r = pl.parent[i];
        uint8_t l = 0;
        if (r != CCL_BG) {
            const uint32_t m = pl.size[r];
            l = 255;
            if ((m & LT_MARK) == LT_MARK) {
                const int k = (int)(m & 255u);
                l = (uint8_t)(k + 1);
                const int z = (int)(i / hw), y = (int)((i - z * hw) / a.W), x = (int)(i - z * hw - (long)y * a.W);
                atomicMin(&smin[0][k], z); atomicMin(&smin[1][k], y); atomicMin(&smin[2][k], x);
                atomicMax(&smax[0][k], z); atomicMax(&smax[1][k], y); atomicMax(&smax[2][k], x);
                atomicAdd(&ssum[0][k], (unsigned long long)z); atomicAdd(&ssum[1][k], (unsigned long long)y); atomicAdd(&ssum[2][k], (unsigned long long)x);
                const int cb = candidate_bits(pl.parent, r, i, z, y, x, a.D, a.H, a.W);
                if (cb & 1) atomicAdd(&pl.cur2[(long)k * a.D + z], 1u);
                if (cb & 2) atomicAdd(&pl.cnt3[k], 1u);
            }
        }
        lab[i] = l;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (smax[0][k] >= 0) {
        unsigned long long* r = (unsigned long long*)(a.rows_i + ((long)p * a.rows + k) * 16);
        for (int j = 0; j < 3; ++j) {
            atomicMin(&r[2 + j], (unsigned long long)smin[j][k]);
            atomicMax(&r[5 + j], (unsigned long long)smax[j][k]);
            atomicAdd(&r[8 + j], ssum[j][k]);
        }
    }
}

// One block per plane: off2 = exclusive scan of the in-slice counts over (row, slice), the counters zeroed for the scatter; off3 = exclusive scan of
// the 3-D counts of the rows that are searched (a row above max_candidates keeps no 3-D candidates).
__global__ __launch_bounds__(NT) void lt_scan_kernel(LtArgs a) {
    __shared__ uint32_t part[NT];
    const LtPlane pl = a.plane(blockIdx.y);
    const int K = (int)pl.st->nrows;
    const long N = (long)K * a.D, per = (N + NT - 1) / NT;
    const long lo = per * threadIdx.x < N ? per * threadIdx.x : N, hi = lo + per < N ? lo + per : N;
    uint32_t s = 0;
    for (long i = lo; i < hi; ++i) s += pl.cur2[i];
    part[threadIdx.x] = s;
    __syncthreads();
    uint32_t run = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) run += part[t];
    for (long i = lo; i < hi; ++i) { const uint32_t c = pl.cur2[i]; pl.off2[i] = run; pl.cur2[i] = 0u; run += c; }
    if (threadIdx.x == 0) {
        uint32_t o = 0;
        for (int k = 0; k < K; ++k) {
            pl.off3[k] = o;
            pl.cur3[k] = 0u;
            if (pl.cnt3[k] <= (uint32_t)a.max_candidates) o += pl.cnt3[k];
        }
    }
}

__global__ __launch_bounds__(NT) void lt_scatter_kernel(LtArgs a) {
    const int p = blockIdx.y;
    const LtPlane pl = a.plane(p);
    const uint8_t* lab = a.lab(p);
    uint32_t* cand2 = (uint32_t*)pl.list;
    uint32_t* cand3 = pl.size;
    const long hw = (long)a.H * a.W;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < a.n; i += (long)gridDim.x * NT) {
        const int l = lab[i];
        if (l == 0 || l == 255) continue;
        const int k = l - 1;
        const int z = (int)(i / hw), y = (int)((i - z * hw) / a.W), x = (int)(i - z * hw - (long)y * a.W);
        const int cb = candidate_bits(pl.parent, pl.parent[i], i, z, y, x, a.D, a.H, a.W);
        if (!(cb & 1)) continue;
        const long seg = (long)k * a.D + z;
        const bool c3 = (cb & 2) && pl.cnt3[k] <= (uint32_t)a.max_candidates;
        cand2[pl.off2[seg] + atomicAdd(&pl.cur2[seg], 1u)] = (uint32_t)i | (c3 ? LT_C3 : 0u);
        if (c3) cand3[pl.off3[k] + atomicAdd(&pl.cur3[k], 1u)] = (uint32_t)i;
    }
}

// The best pair among m candidates (linear indices, bit 31 ignored) in tiles of NT: tile pair tp = ta * ntile + tb is searched when ta <= tb and
// tp = first, first + step, ...  Called by every thread of the block; the result is per thread (block_best folds it).
__device__ __forceinline__ void pair_search(const uint32_t* cand, uint32_t m, long first, long step, const LtArgs& a, double& best,
                                            unsigned long long& bpair) {
    __shared__ int tz[NT], ty[NT], tx[NT];
    __shared__ uint32_t ti[NT];
    const long hw = (long)a.H * a.W;
    const long ntile = ((long)m + NT - 1) / NT;
    for (long tp = first; tp < ntile * ntile; tp += step) {
        const long ta = tp / ntile, tb = tp - ta * ntile;
        if (tb < ta) continue;
        const long ia = ta * NT + threadIdx.x, ib = tb * NT + threadIdx.x;
        __syncthreads();                                 // the tile of the round before has been read
        if (ib < (long)m) {
            const uint32_t v = cand[ib] & ~LT_C3;
            const int z = (int)(v / hw), y = (int)((v - z * hw) / a.W);
            ti[threadIdx.x] = v; tz[threadIdx.x] = z; ty[threadIdx.x] = y; tx[threadIdx.x] = (int)(v - z * hw - (long)y * a.W);
        }
        __syncthreads();
        if (ia >= (long)m) continue;
        const uint32_t v = cand[ia] & ~LT_C3;
        const int z = (int)(v / hw), y = (int)((v - z * hw) / a.W), x = (int)(v - z * hw - (long)y * a.W);
        const int nb = (long)m - tb * NT < NT ? (int)((long)m - tb * NT) : NT;
        for (int j = 0; j < nb; ++j)
            take_better(best, bpair, sqdist(z - tz[j], y - ty[j], x - tx[j], a.q0, a.q1, a.q2), pair_of(v, ti[j]));
    }
}

// grid (D, planes): slice z of every row whose extent holds it
__global__ __launch_bounds__(NT) void lt_pair2_kernel(LtArgs a) {
    const int p = blockIdx.y, z = blockIdx.x;
    const LtPlane pl = a.plane(p);
    const int K = (int)pl.st->nrows;
    const uint32_t* cand2 = (const uint32_t*)pl.list;
    for (int k = 0; k < K; ++k) {
        const long long* r = a.rows_i + ((long)p * a.rows + k) * 16;
        if (z < r[2] || z > r[5]) continue;              // the same for every thread
        const long seg = (long)k * a.D + z;
        double best = -1.0;
        unsigned long long bpair = NO_PAIR;
        pair_search(cand2 + pl.off2[seg], pl.cur2[seg], 0, 1, a, best, bpair);
        block_best(best, bpair);
        if (threadIdx.x == 0) { pl.key2[seg] = best; pl.pair2[seg] = bpair; }
    }
}

// grid (LT_G3, rows, planes)
__global__ __launch_bounds__(NT) void lt_pair3_kernel(LtArgs a) {
    const int p = blockIdx.z, k = blockIdx.y;
    const LtPlane pl = a.plane(p);
    if (k >= (int)pl.st->nrows) return;
    double best = -1.0;
    unsigned long long bpair = NO_PAIR;
    const uint32_t m = pl.cnt3[k];
    if (m <= (uint32_t)a.max_candidates) pair_search(pl.size + pl.off3[k], m, blockIdx.x, LT_G3, a, best, bpair);
    block_best(best, bpair);
    if (threadIdx.x == 0) { pl.key3[k * LT_G3 + blockIdx.x] = best; pl.pair3[k * LT_G3 + blockIdx.x] = bpair; }
}

// grid (rows, planes)
__global__ __launch_bounds__(NT) void lt_final_kernel(LtArgs a) {
    const int p = blockIdx.y, k = blockIdx.x;
    const LtPlane pl = a.plane(p);
    if (k >= (int)pl.st->nrows) return;
    long long* r = a.rows_i + ((long)p * a.rows + k) * 16;
    double* f = a.rows_f + ((long)p * a.rows + k) * 4;
    const int zmin = (int)r[2], ymin = (int)r[3], xmin = (int)r[4], zmax = (int)r[5], ymax = (int)r[6], xmax = (int)r[7];
    const bool capped = pl.cnt3[k] > (uint32_t)a.max_candidates;
    double k3 = -1.0, k2 = -1.0;
    unsigned long long p3 = NO_PAIR, p2 = NO_PAIR;
    if (threadIdx.x < LT_G3) { k3 = pl.key3[k * LT_G3 + threadIdx.x]; p3 = pl.pair3[k * LT_G3 + threadIdx.x]; }
    block_best(k3, p3);
    for (int z = zmin + threadIdx.x; z <= zmax; z += NT) take_better(k2, p2, pl.key2[(long)k * a.D + z], pl.pair2[(long)k * a.D + z]);
    block_best(k2, p2);
    // b: the extent of the component's voxels in the slice of (pa, qa) along the in-plane normal of pa -> qa
    const long hw = (long)a.H * a.W;
    const uint32_t pa = (uint32_t)(p2 >> 32), qa = (uint32_t)(p2 & 0xFFFFFFFFull);
    const int za = (int)(pa / hw);
    const int ya = (int)((pa - za * hw) / a.W), xa = (int)(pa - za * hw - (long)ya * a.W);
    const int yb = (int)((qa - za * hw) / a.W), xb = (int)(qa - za * hw - (long)yb * a.W);
    const double ey = (double)(yb - ya) * a.s1, ex = (double)(xb - xa) * a.s2;
    const double av = sqrt_nearest(k2);
    double tmin = 1e300, tmax = -1e300;
    if (k2 > 0.0) {
        const uint8_t* lab = a.lab(p) + za * hw;
        const int nx = xmax - xmin + 1;
        const long cells = (long)(ymax - ymin + 1) * nx;
        for (long c = threadIdx.x; c < cells; c += NT) {
            const int y = ymin + (int)(c / nx), x = xmin + (int)(c % nx);
            if (lab[(long)y * a.W + x] != k + 1) continue;
            const double t = ey * ((double)x * a.s2) - ex * ((double)y * a.s1);
            tmin = t < tmin ? t : tmin;
            tmax = t > tmax ? t : tmax;
        }
    }
    __shared__ double rmin[NT / 64], rmax[NT / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(tmin, o, 64), v = __shfl_xor(tmax, o, 64);
        tmin = u < tmin ? u : tmin;
        tmax = v > tmax ? v : tmax;
    }
    if ((threadIdx.x & 63) == 0) { rmin[threadIdx.x >> 6] = tmin; rmax[threadIdx.x >> 6] = tmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) { tmin = rmin[w] < tmin ? rmin[w] : tmin; tmax = rmax[w] > tmax ? rmax[w] : tmax; }
        if (capped) {
            r[11] = -1; r[12] = -1; r[15] = 1;
            f[0] = __longlong_as_double(0x7FF8000000000000ll);
        } else {
            r[11] = (long long)(p3 >> 32); r[12] = (long long)(p3 & 0xFFFFFFFFull); r[15] = 0;
            f[0] = sqrt_nearest(k3);
        }
        r[13] = (long long)pa; r[14] = (long long)qa;
        f[1] = av;
        f[2] = k2 > 0.0 ? (tmax - tmin) / av : 0.0;
        f[3] = (double)(zmax - zmin) * a.s0;
    }
}

__global__ __launch_bounds__(NT) void lo_zero_kernel(long long* counts, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) counts[i] = 0;
}

// joint histogram: one atomic per run of equal (a, b) in a wave; background on both sides and values above Ka / Kb (255 among them) count nowhere
__global__ __launch_bounds__(NT) void lo_count_kernel(const uint8_t* __restrict__ la, const uint8_t* __restrict__ lb, long voxels, int Ka, int Kb,
                                                      long long* counts) {
    const uint8_t* pa = la + (long)blockIdx.y * voxels;
    const uint8_t* pb = lb + (long)blockIdx.y * voxels;
    unsigned long long* c = (unsigned long long*)counts + (long)blockIdx.y * (Ka + 1) * (Kb + 1);
    for (long base = (long)blockIdx.x * NT; base < voxels; base += (long)gridDim.x * NT) {
        const long i = base + threadIdx.x;
        uint32_t v = 0xFFFFFFFFu;                        // counts nowhere
        if (i < voxels) {
            const int x = pa[i], y = pb[i];
            if ((x | y) != 0 && x <= Ka && y <= Kb) v = (uint32_t)(x * (Kb + 1) + y);
        }
        if (__ballot(v != 0xFFFFFFFFu) == 0ull) continue;                // the same for the whole wave
        const int len = run_length(v);
        if (len && v != 0xFFFFFFFFu) atomicAdd(&c[v], (unsigned long long)len);
    }
}

bool shape_ok(int planes, int D, int H, int W, int rows) {
    return planes >= 1 && planes <= LT_MAX_PLANES && D > 0 && H > 0 && W > 0 && (long)D * H * W <= (1L << 31) && rows >= 1 && rows <= LT_MAX_ROWS;
}
bool spacing_ok(double s) { return s > 0.0 && s < __builtin_inf(); }     // false for a NaN

template <int CONN>
int run_table(const LtArgs& a, int planes, hipStream_t st) {
    const int tz = (a.D + CCL_Z - 1) / CCL_Z;
    const dim3 tiles(a.tiles_x * a.tiles_y * tz, planes), flat(grid_for(a.n, GRID_CAP), planes), one(1, planes);
    hipLaunchKernelGGL(lt_label_kernel<CONN>, tiles, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_merge_kernel<CONN>, tiles, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_size_kernel, flat, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_roots_kernel, flat, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_select_kernel, one, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_stats_kernel, flat, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_scan_kernel, one, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_scatter_kernel, flat, dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_pair2_kernel, dim3(a.D, planes), dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_pair3_kernel, dim3(LT_G3, a.rows, planes), dim3(NT), 0, st, a);
    hipLaunchKernelGGL(lt_final_kernel, dim3(a.rows, planes), dim3(NT), 0, st, a);
    return rs_check_launch();
}

}  // namespace

extern "C" {

long rsuper_lesion_table_workspace_bytes(int planes, int D, int H, int W, int max_lesions) {
    if (!shape_ok(planes, D, H, W, max_lesions)) return 0;
    return (long)planes * LtLayout((long)D * H * W, D, max_lesions).plane_bytes;
}

int rsuper_lesion_table_launches(void) { return 11; }

int rsuper_lesion_table(const uint8_t* masks, int planes, int D, int H, int W, int conn, int min_voxels, int max_lesions, int max_candidates, double s0,
                        double s1, double s2, long long* rows_i, double* rows_f, long long* totals, uint8_t* labels, void* workspace,
                        long workspace_bytes, void* stream) {
    if (!masks || !rows_i || !rows_f || !totals || !workspace || !shape_ok(planes, D, H, W, max_lesions)) return RS_ERR_ARG;
    if ((conn != 6 && conn != 26) || min_voxels < 1 || max_candidates < 2 || !spacing_ok(s0) || !spacing_ok(s1) || !spacing_ok(s2)) return RS_ERR_ARG;
    if (((uintptr_t)rows_i | (uintptr_t)rows_f | (uintptr_t)totals | (uintptr_t)workspace) & 7) return RS_ERR_ARG;
    const long n = (long)D * H * W;
    const LtLayout lay(n, D, max_lesions);
    if (workspace_bytes < (long)planes * lay.plane_bytes) return RS_ERR_ARG;
    LtArgs a = {workspace, lay, masks, labels, rows_i, rows_f, totals, n, D, H, W, (W + CCL_X - 1) / CCL_X, (H + CCL_Y - 1) / CCL_Y, max_lesions,
                min_voxels, max_candidates, s0 * s0, s1 * s1, s2 * s2, s0, s1, s2};
    return conn == 6 ? run_table<6>(a, planes, (hipStream_t)stream) : run_table<26>(a, planes, (hipStream_t)stream);
}

int rsuper_label_overlap(const uint8_t* labels_a, const uint8_t* labels_b, int planes, long voxels, int Ka, int Kb, long long* counts, void* stream) {
    if (!labels_a || !labels_b || !counts || planes < 1 || planes > 65535 || voxels < 1 || Ka < 0 || Ka > LT_MAX_ROWS || Kb < 0 || Kb > LT_MAX_ROWS)
        return RS_ERR_ARG;
    if ((uintptr_t)counts & 7) return RS_ERR_ARG;
    const long total = (long)planes * (Ka + 1) * (Kb + 1);
    hipLaunchKernelGGL(lo_zero_kernel, dim3(grid_for(total, GRID_CAP)), dim3(NT), 0, (hipStream_t)stream, counts, total);
    hipLaunchKernelGGL(lo_count_kernel, dim3(grid_for(voxels, GRID_CAP), planes), dim3(NT), 0, (hipStream_t)stream, labels_a, labels_b, voxels, Ka, Kb,
                       counts);
    return rs_check_launch();
}

}  // extern "C"
