// The union-find connected-component labeller of the device data path (largest component in postproc.hip, lesion candidates in pseudo_label.hip).
//   tile pass     ccl_label_tile: one block labels one 8 x 8 x 32 tile in LDS and writes parent = global index of the tile-local root (background: CCL_BG)
//   border pass   ccl_link_borders: every voxel with a backward neighbour outside its tile links to it in the global parent words
//   compression   ccl_compress: a voxel's word is pointed straight at its root
// Connectivity is a template parameter: 6 (3 backward neighbours) or 26 (13).  Linking is by atomicMin, so the root of a set is its smallest linear index
// whatever the order the links land in; callers depend on the result only through roots and sizes.  Launches are the only synchronisation between the
// passes; inside the border pass and the compression only the agent-scope atomics below cross workgroups.
#pragma once
#include "common.hpp"

constexpr int CCL_NT = 256;                              // threads per block of the tile and border passes (4 waves)
constexpr int CCL_Z = 8, CCL_Y = 8, CCL_X = 32;          // block-local labelling tile
constexpr int CCL_N = CCL_Z * CCL_Y * CCL_X;
constexpr uint32_t CCL_BG = 0xFFFFFFFFu;                 // parent word of a background voxel

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// order-preserving u32 / u64 image of an f32 / f64 (larger key <=> larger value; 0 is below every value)
__device__ __forceinline__ uint32_t f32_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ unsigned long long f64_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_f64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

__device__ __forceinline__ int lds_find(int* p, int a) {
    int q;
    while ((q = __hip_atomic_load(&p[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != a) a = q;
    return a;
}

// union by atomicMin linking: the larger root is linked below the smaller one, so every parent <= its child and the root of a set is its
// smallest index whatever the order the links land in
__device__ __forceinline__ void lds_union(int* p, int a, int b) {
    bool done = false;
    while (!done) {
        a = lds_find(p, a);
        b = lds_find(p, b);
        if (a < b) { const int old = atomicMin(&p[b], a); done = old == b; b = old; }
        else if (b < a) { const int old = atomicMin(&p[a], b); done = old == a; a = old; }
        else done = true;
    }
}

// Parent words another workgroup may write: agent-scope atomic loads (a plain load can return a stale copy from another XCD's L2).
__device__ __forceinline__ uint32_t g_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t g_find(const uint32_t* p, uint32_t a) {
    uint32_t q;
    while ((q = g_load(&p[a])) != a) a = q;
    return a;
}

__device__ __forceinline__ void g_union(uint32_t* p, uint32_t a, uint32_t b) {
    bool done = false;
    while (!done) {
        a = g_find(p, a);
        b = g_find(p, b);
        if (a < b) { const uint32_t old = atomicMin(&p[b], a); done = old == b; b = old; }
        else if (b < a) { const uint32_t old = atomicMin(&p[a], b); done = old == a; a = old; }
        else done = true;
    }
}

// The neighbours that precede a voxel in C order, and the items of the border pass: item j of the tile at (oz, oy, ox) -> the voxel (lz, ly, lx) and the
// first of its BORDER_K backward neighbours to try; on = false when the item has nothing to link.
struct CclBorderItem { int lz, ly, lx, k0; bool on; };
template <int CONN> struct CclNeighbours;

// 6-connected: k = 0 / 1 / 2 -> dx / dy / dz = -1.  The border pass enumerates the three low faces only, one neighbour each (a voxel on an edge is
// an item of two faces): 576 items per tile against 2048 voxels.
template <> struct CclNeighbours<6> {
    static constexpr int K = 3;
    static constexpr int FX = CCL_Z * CCL_Y, FY = CCL_Z * CCL_X, FZ = CCL_Y * CCL_X;
    static constexpr int ITEMS = FX + FY + FZ, BORDER_K = 1;
    __device__ static __forceinline__ void backward(int k, int& dz, int& dy, int& dx) { dz = -(int)(k == 2); dy = -(int)(k == 1); dx = -(int)(k == 0); }
    __device__ static __forceinline__ CclBorderItem border_item(int j, int oz, int oy, int ox) {    // a face on the volume's border has no items
        if (j < FX) return {j / CCL_Y, j % CCL_Y, 0, 0, ox != 0};
        if (j < FX + FY) return {(j - FX) / CCL_X, 0, (j - FX) % CCL_X, 1, oy != 0};
        return {0, (j - FX - FY) / CCL_X, (j - FX - FY) % CCL_X, 2, oz != 0};
    }
};

// 26-connected: k 0..8 -> dz = -1, (dy, dx) in [-1, 1]^2; 9..11 -> dz = 0, dy = -1; 12 -> dx = -1.  A backward neighbour lies outside the tile across
// the low z / y / x faces and, for (dz, dy, dx) such as (-1, +1, +1) or (0, -1, +1), across the high y and x faces too -- face-, edge- and
// corner-adjacent tiles alike: the border pass walks all voxels and keeps those on one of these five faces.
template <> struct CclNeighbours<26> {
    static constexpr int K = 13;
    static constexpr int ITEMS = CCL_N, BORDER_K = K;
    __device__ static __forceinline__ void backward(int k, int& dz, int& dy, int& dx) {
        if (k < 9) { dz = -1; dy = k / 3 - 1; dx = k % 3 - 1; }
        else if (k < 12) { dz = 0; dy = -1; dx = k - 10; }
        else { dz = 0; dy = 0; dx = -1; }
    }
    __device__ static __forceinline__ CclBorderItem border_item(int j, int, int, int) {
        const int lx = j % CCL_X, t = j / CCL_X, ly = t % CCL_Y, lz = t / CCL_Y;
        return {lz, ly, lx, 0, lz == 0 || ly == 0 || ly == CCL_Y - 1 || lx == 0 || lx == CCL_X - 1};
    }
};

// origin of tile `tile` of a (tiles_z, tiles_y, tiles_x) grid, x fastest
__device__ __forceinline__ void ccl_tile_origin(int tile, int tiles_x, int tiles_y, int& oz, int& oy, int& ox) {
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / tiles_x / tiles_y;
    oz = tz * CCL_Z; oy = ty * CCL_Y; ox = tx * CCL_X;
}

// Tile pass, called by every thread of a CCL_NT block: labels tile `tile` of the (D, H, W) volume in LDS and writes parent = global index of the
// tile-local root for foreground voxels, CCL_BG for the others.  fg(global index) -> bool is called exactly once for every voxel of the tile that lies
// inside the volume.
template <int CONN, typename Pred>
__device__ __forceinline__ void ccl_label_tile(uint32_t* __restrict__ parent, int tile, int tiles_x, int tiles_y, int D, int H, int W, Pred fg) {
    typedef CclNeighbours<CONN> NB;
    __shared__ int lp[CCL_N];
    int oz, oy, ox;
    ccl_tile_origin(tile, tiles_x, tiles_y, oz, oy, ox);
    for (int i = threadIdx.x; i < CCL_N; i += CCL_NT) {
        const int lx = i % CCL_X, t = i / CCL_X, ly = t % CCL_Y, lz = t / CCL_Y;
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        bool f = false;
        if (gz < D && gy < H && gx < W) f = fg(((long)gz * H + gy) * W + gx);
        lp[i] = f ? i : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CCL_N; i += CCL_NT) {
        if (lp[i] < 0) continue;                         // foreground words stay >= 0 under the unions, background stays -1
        const int lx = i % CCL_X, t = i / CCL_X, ly = t % CCL_Y, lz = t / CCL_Y;
        for (int k = 0; k < NB::K; ++k) {
            int dz, dy, dx;
            NB::backward(k, dz, dy, dx);
            const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
            if (nz < 0 || ny < 0 || ny >= CCL_Y || nx < 0 || nx >= CCL_X) continue;
            const int j = (nz * CCL_Y + ny) * CCL_X + nx;
            if (lp[j] >= 0) lds_union(lp, i, j);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CCL_N; i += CCL_NT) {
        const int lx = i % CCL_X, t = i / CCL_X, ly = t % CCL_Y, lz = t / CCL_Y;
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        if (gz >= D || gy >= H || gx >= W) continue;
        uint32_t v = CCL_BG;
        if (lp[i] >= 0) {
            const int r = lds_find(lp, i);
            const int rx = r % CCL_X, rt = r / CCL_X, ry = rt % CCL_Y, rz = rt / CCL_Y;
            v = (uint32_t)((((long)(oz + rz)) * H + oy + ry) * W + ox + rx);
        }
        parent[((long)gz * H + gy) * W + gx] = v;
    }
}

// Border pass, called by every thread of a CCL_NT block after the tile pass of the whole volume: links the foreground voxels of tile `tile` to their
// backward neighbours outside the tile.  Two voxels are 6- / 26-adjacent exactly when one is a backward neighbour of the other, so each pair is linked
// once: by the tile pass when both lie in one tile, here otherwise.
template <int CONN>
__device__ __forceinline__ void ccl_link_borders(uint32_t* parent, int tile, int tiles_x, int tiles_y, int D, int H, int W) {
    typedef CclNeighbours<CONN> NB;
    int oz, oy, ox;
    ccl_tile_origin(tile, tiles_x, tiles_y, oz, oy, ox);
    for (int j = threadIdx.x; j < NB::ITEMS; j += CCL_NT) {
        const CclBorderItem it = NB::border_item(j, oz, oy, ox);
        if (!it.on) continue;
        const int lz = it.lz, ly = it.ly, lx = it.lx;
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        if (gz >= D || gy >= H || gx >= W) continue;
        const long a = ((long)gz * H + gy) * W + gx;
        const uint32_t pa = g_load(&parent[a]);
        if (pa == CCL_BG) continue;
        uint32_t last = CCL_BG;                          // the neighbour word this voxel linked to last
        for (int k = it.k0; k < it.k0 + NB::BORDER_K; ++k) {
            int dz, dy, dx;
            NB::backward(k, dz, dy, dx);
            const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
            if (nz >= 0 && ny >= 0 && ny < CCL_Y && nx >= 0 && nx < CCL_X) continue;            // inside the tile: linked by the tile pass
            const int hz = gz + dz, hy = gy + dy, hx = gx + dx;
            if (hz < 0 || hy < 0 || hy >= H || hx < 0 || hx >= W) continue;                      // outside the volume (hz < D: dz <= 0)
            const long b = ((long)hz * H + hy) * W + hx;
            // parent words never leave their set, so two neighbours with the same word are in one set already: on a smooth mask the up to nine
            // outside neighbours of a face voxel mostly share one tile root, and one request does for all of them
            const uint32_t pb = g_load(&parent[b]);
            if (pb == CCL_BG || pb == last) continue;
            g_union(parent, pa, pb);
            last = pb;
        }
    }
}

// Compression, after the border pass: the root of voxel i's set (CCL_BG for a background voxel); the voxel's word is pointed straight at it.  Root words
// do not change in the launch that calls this.
__device__ __forceinline__ uint32_t ccl_compress(uint32_t* parent, long i) {
    const uint32_t q = g_load(&parent[i]);
    if (q == CCL_BG) return CCL_BG;
    const uint32_t r = g_find(parent, q);
    if (r != q) __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return r;
}

// blocks of CCL_NT threads for a grid-stride pass over n items, at most `cap` (a tuned value per call site)
static inline int grid_for(long n, int cap) {
    const long b = (n + CCL_NT - 1) / CCL_NT;
    return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}
