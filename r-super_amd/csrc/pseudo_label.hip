// Report-guided pseudo-label refinement (baselines/pseudo_labels: extract_lesion_candidates of the reference's pseudo_label_report_refinement.py).
// Per lesion plane, repeated until the report's lesion count is reached or the volume runs dry:
//   peak       the maximum of `work` and the first C-order voxel holding it: a u64 atomicMax on (orderable f32 bits << 32) | (0xFFFFFFFF - index)
//   threshold  thr = float32(peak_cut) * peak, one IEEE f32 multiply; mask = work >= thr
//   label      union-find over the mask, 26-connected (13 backward neighbours): tile labelling in LDS, then links across every tile border
//   apply      the seed's component: size >= min_voxels -> out = 1, kept += 1; always work = 0, iterations += 1
// P planes advance in the same launches (plane = blockIdx.y), each with its own state.  Loop control stays on the device by predication: every kernel
// reads its plane's `done` word first and returns when it is set, so the host enqueues K iterations back to back and reads the state block once.  Launches
// are the only synchronisation between phases; inside a launch only the agent-scope atomics of the union-find cross workgroups.  Every cross-workgroup
// result is an integer atomic (u64 max key, atomicMin links, a size counter): deterministic by construction.
//
// Who writes which state word, and when (no word is written in a launch in which another block reads it):
//   key         pl_peak (atomicMax, all blocks); zeroed by pl_apply block 0 (pl_apply reads `root`, never the key)
//   done, size  pl_local block 0 (every block of pl_local derives the stop condition itself from key / kept / n, it does not read `done` for it);
//               `done` also by pl_apply block 0 when the seed has no component, which every block of pl_apply sees in `root` and returns on
//   root        pl_count block 0
//   kept, iterations   pl_apply block 0
#include "common.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int NT = 256;                                  // threads per block (4 waves)
constexpr int PL_Z = 8, PL_Y = 8, PL_X = 32;             // block-local labelling tile
constexpr int PL_N = PL_Z * PL_Y * PL_X;
constexpr uint32_t PL_BG = 0xFFFFFFFFu;                  // parent word of a voxel outside the mask
constexpr int PL_MAX_PLANES = RSUPER_LESION_MAX_PLANES;

struct PlaneState {                                      // RSUPER_LESION_STATE_WORDS 32-bit words per plane
    int kept, iterations, done, n_lesions;
    unsigned long long key;                              // (orderable peak bits << 32) | (0xFFFFFFFF - seed index); 0 = not computed
    uint32_t root, size;                                 // the seed component's root and voxel count
};
static_assert(sizeof(PlaneState) == RSUPER_LESION_STATE_WORDS * 4, "state layout");

struct Counts { int n[PL_MAX_PLANES]; };

// order-preserving u32 image of an f32 (larger key <=> larger value)
__device__ __forceinline__ uint32_t f32_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ int lds_find(int* p, int a) {
    int q;
    while ((q = __hip_atomic_load(&p[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != a) a = q;
    return a;
}

// union by atomicMin linking: every parent <= its child, the root of a set is its smallest index whatever the order the links land in
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

// the k-th of the 13 neighbours that precede a voxel in C order: k 0..8 -> dz = -1, (dy, dx) in [-1, 1]^2; 9..11 -> dz = 0, dy = -1; 12 -> dx = -1
__device__ __forceinline__ void backward(int k, int& dz, int& dy, int& dx) {
    if (k < 9) { dz = -1; dy = k / 3 - 1; dx = k % 3 - 1; }
    else if (k < 12) { dz = 0; dy = -1; dx = k - 10; }
    else { dz = 0; dy = 0; dx = -1; }
}

// out = 0 and the state of every plane: one launch, no memset (a captured hipMemsetAsync is what README round 3 warns about)
__global__ __launch_bounds__(NT) void pl_begin_kernel(uint8_t* __restrict__ out, long total, PlaneState* st, Counts c, int planes) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) out[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < planes) {
        PlaneState s;
        s.kept = 0; s.iterations = 0; s.done = c.n[threadIdx.x] <= 0 ? 1 : 0; s.n_lesions = c.n[threadIdx.x];
        s.key = 0ull; s.root = 0u; s.size = 0u;
        st[threadIdx.x] = s;
    }
}

// (1) peak of the plane and its first index
__global__ __launch_bounds__(NT) void pl_peak_kernel(const float* __restrict__ work, long n, PlaneState* st) {
    PlaneState* s = st + blockIdx.y;
    if (s->done || s->kept >= s->n_lesions) return;      // the count is reached: pl_local sets `done`, the key stays 0
    const float* w = work + (long)blockIdx.y * n;
    unsigned long long best = 0ull;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const unsigned long long k = ((unsigned long long)f32_key(w[i]) << 32) | (0xFFFFFFFFull - (unsigned long long)i);
        best = k > best ? k : best;
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&s->key, best);
}

// (2) stop or go; label one tile of work >= thr in LDS, parent = global index of the tile-local root (outside the mask: PL_BG)
__global__ __launch_bounds__(NT) void pl_local_kernel(const float* __restrict__ work, uint32_t* __restrict__ parent, long n, long pstride, PlaneState* st,
                                                      float peak_cut, float min_peak, int D, int H, int W, int tiles_x, int tiles_y) {
    __shared__ int lp[PL_N];
    PlaneState* s = st + blockIdx.y;
    if (s->done) return;
    const unsigned long long key = s->key;
    const float peak = key_f32((uint32_t)(key >> 32));
    // the same for every block of the plane.  !(peak >= min_peak), not peak < min_peak: a NaN peak (a NaN in the caller's volume orders above every
    // finite value) stops the plane here -- its threshold would be NaN, the mask empty and the seed outside it
    const bool stop = s->kept >= s->n_lesions || key == 0ull || !(peak >= min_peak);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (stop) s->done = 1; else s->size = 0u;
    }
    if (stop) return;
    const float thr = __fmul_rn(peak_cut, peak);
    const float* w = work + (long)blockIdx.y * n;
    uint32_t* par = parent + (long)blockIdx.y * pstride;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / tiles_x / tiles_y;
    const int oz = tz * PL_Z, oy = ty * PL_Y, ox = tx * PL_X;
    for (int i = threadIdx.x; i < PL_N; i += NT) {
        const int lx = i % PL_X, t = i / PL_X, ly = t % PL_Y, lz = t / PL_Y;
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        bool f = false;
        if (gz < D && gy < H && gx < W) f = w[((long)gz * H + gy) * W + gx] >= thr;
        lp[i] = f ? i : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PL_N; i += NT) {
        if (lp[i] < 0) continue;                         // mask words stay >= 0 under the unions, the others stay -1
        const int lx = i % PL_X, t = i / PL_X, ly = t % PL_Y, lz = t / PL_Y;
        for (int k = 0; k < 13; ++k) {
            int dz, dy, dx;
            backward(k, dz, dy, dx);
            const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
            if (nz < 0 || ny < 0 || ny >= PL_Y || nx < 0 || nx >= PL_X) continue;
            const int j = (nz * PL_Y + ny) * PL_X + nx;
            if (lp[j] >= 0) lds_union(lp, i, j);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PL_N; i += NT) {
        const int lx = i % PL_X, t = i / PL_X, ly = t % PL_Y, lz = t / PL_Y;
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        if (gz >= D || gy >= H || gx >= W) continue;
        uint32_t v = PL_BG;
        if (lp[i] >= 0) {
            const int r = lds_find(lp, i);
            const int rx = r % PL_X, rt = r / PL_X, ry = rt % PL_Y, rz = rt / PL_Y;
            v = (uint32_t)((((long)(oz + rz)) * H + oy + ry) * W + ox + rx);
        }
        par[((long)gz * H + gy) * W + gx] = v;
    }
}

// (3) every voxel with a backward neighbour outside its tile links to it: the low z / y / x faces and, for (dz, dy, dx) such as (-1, +1, +1) or
// (0, -1, +1), the high y and x faces too -- face-, edge- and corner-adjacent tiles alike
__global__ __launch_bounds__(NT) void pl_merge_kernel(uint32_t* parent, long pstride, const PlaneState* st, int D, int H, int W, int tiles_x, int tiles_y) {
    if (st[blockIdx.y].done) return;
    uint32_t* par = parent + (long)blockIdx.y * pstride;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / tiles_x / tiles_y;
    const int oz = tz * PL_Z, oy = ty * PL_Y, ox = tx * PL_X;
    for (int i = threadIdx.x; i < PL_N; i += NT) {
        const int lx = i % PL_X, t = i / PL_X, ly = t % PL_Y, lz = t / PL_Y;
        if (lz != 0 && ly != 0 && ly != PL_Y - 1 && lx != 0 && lx != PL_X - 1) continue;       // every backward neighbour lies inside the tile
        const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
        if (gz >= D || gy >= H || gx >= W) continue;
        const long a = ((long)gz * H + gy) * W + gx;
        const uint32_t pa = g_load(&par[a]);
        if (pa == PL_BG) continue;
        uint32_t last = PL_BG;                           // the neighbour word this voxel linked to last
        for (int k = 0; k < 13; ++k) {
            int dz, dy, dx;
            backward(k, dz, dy, dx);
            const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
            if (nz >= 0 && ny >= 0 && ny < PL_Y && nx >= 0 && nx < PL_X) continue;              // inside the tile: linked by pl_local
            const int hz = gz + dz, hy = gy + dy, hx = gx + dx;
            if (hz < 0 || hy < 0 || hy >= H || hx < 0 || hx >= W) continue;                      // outside the volume (hz < D: dz <= 0)
            const long b = ((long)hz * H + hy) * W + hx;
            // parent words never leave their set, so two neighbours with the same word are in one set already: on a smooth mask the up to nine
            // outside neighbours of a face voxel mostly share one tile root, and one request does for all of them
            const uint32_t pb = g_load(&par[b]);
            if (pb == PL_BG || pb == last) continue;
            g_union(par, pa, pb);
            last = pb;
        }
    }
}

// (4) path compression and the size of the seed's component: one counter add per wave
__global__ __launch_bounds__(NT) void pl_count_kernel(uint32_t* parent, long n, long pstride, PlaneState* st) {
    __shared__ uint32_t seed_root;
    PlaneState* s = st + blockIdx.y;
    if (s->done) return;
    uint32_t* par = parent + (long)blockIdx.y * pstride;
    if (threadIdx.x == 0) {
        const uint32_t seed = (uint32_t)(0xFFFFFFFFull - (s->key & 0xFFFFFFFFull));
        // root words do not change in this launch: every block finds the same one.  A finite peak lies inside its own mask (thr <= peak for
        // 0 < peak_cut <= 1); were the seed ever outside it, its word is PL_BG, which is no index: nothing is followed and pl_apply ends the plane
        seed_root = g_load(&par[seed]) == PL_BG ? PL_BG : g_find(par, seed);
        if (blockIdx.x == 0) s->root = seed_root;
    }
    __syncthreads();
    const uint32_t root = seed_root;
    uint32_t mine = 0u;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const uint32_t q = g_load(&par[i]);
        if (q == PL_BG) continue;
        const uint32_t r = g_find(par, q);
        if (r != q) __hip_atomic_store(&par[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine += r == root ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s->size, mine);
}

// (5) the seed's component: kept when large enough, zeroed in `work` either way; then the plane's counters
__global__ __launch_bounds__(NT) void pl_apply_kernel(float* __restrict__ work, uint8_t* __restrict__ out, const uint32_t* __restrict__ parent, long n,
                                                      long pstride, PlaneState* st, int min_voxels) {
    PlaneState* s = st + blockIdx.y;
    if (s->done) return;
    const uint32_t root = s->root;
    if (root == PL_BG) {                                 // no seed component (see pl_count): nothing to zero, so the plane could not advance -- end it
        if (blockIdx.x == 0 && threadIdx.x == 0) s->done = 1;
        return;
    }
    const bool keep = s->size >= (uint32_t)min_voxels;
    const uint32_t* par = parent + (long)blockIdx.y * pstride;
    float* w = work + (long)blockIdx.y * n;
    uint8_t* o = out + (long)blockIdx.y * n;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        if (par[i] != root) continue;
        if (keep) o[i] = 1;
        w[i] = 0.f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        s->kept += keep ? 1 : 0;
        s->iterations += 1;
        s->key = 0ull;
    }
}

int grid_for(long n) {
    const long b = (n + NT - 1) / NT;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

bool launched() { return hipGetLastError() == hipSuccess; }

bool shape_ok(int planes, int D, int H, int W) {
    return planes >= 1 && planes <= PL_MAX_PLANES && D > 0 && H > 0 && W > 0 && (long)D * H * W <= (1L << 31);
}

long parent_stride(long n) { return (n + 63) & ~63L; }

}  // namespace

extern "C" {

long rsuper_lesion_candidates_workspace_bytes(int planes, int D, int H, int W) {
    if (!shape_ok(planes, D, H, W)) return 0;
    return (long)planes * parent_stride((long)D * H * W) * 4;
}

int rsuper_lesion_candidates_begin(uint8_t* out, int planes, int D, int H, int W, const int* n_lesions, void* state, void* stream) {
    if (!out || !n_lesions || !state || !shape_ok(planes, D, H, W)) return RS_ERR_ARG;
    Counts c;
    for (int p = 0; p < PL_MAX_PLANES; ++p) c.n[p] = p < planes ? n_lesions[p] : 0;
    const long total = (long)planes * D * H * W;
    hipLaunchKernelGGL(pl_begin_kernel, dim3(grid_for(total)), dim3(NT), 0, (hipStream_t)stream, out, total, (PlaneState*)state, c, planes);
    return launched() ? RS_OK : RS_ERR_LAUNCH;
}

int rsuper_lesion_candidates_run(float* work, uint8_t* out, int planes, int D, int H, int W, float peak_cut, int min_voxels, float min_peak, void* state,
                                 void* workspace, int iterations, void* stream) {
    if (!work || !out || !state || !workspace || !shape_ok(planes, D, H, W)) return RS_ERR_ARG;
    if (!(peak_cut > 0.f && peak_cut <= 1.f) || !(min_peak > 0.f) || min_voxels < 1 || iterations < 1) return RS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    PlaneState* s = (PlaneState*)state;
    uint32_t* parent = (uint32_t*)workspace;
    const long n = (long)D * H * W, ps = parent_stride(n);
    const int tx = (W + PL_X - 1) / PL_X, ty = (H + PL_Y - 1) / PL_Y, tz = (D + PL_Z - 1) / PL_Z;
    const dim3 tiles(tx * ty * tz, planes), flat(grid_for(n), planes);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(pl_peak_kernel, flat, dim3(NT), 0, st, (const float*)work, n, s);
        hipLaunchKernelGGL(pl_local_kernel, tiles, dim3(NT), 0, st, (const float*)work, parent, n, ps, s, peak_cut, min_peak, D, H, W, tx, ty);
        hipLaunchKernelGGL(pl_merge_kernel, tiles, dim3(NT), 0, st, parent, ps, (const PlaneState*)s, D, H, W, tx, ty);
        hipLaunchKernelGGL(pl_count_kernel, flat, dim3(NT), 0, st, parent, n, ps, s);
        hipLaunchKernelGGL(pl_apply_kernel, flat, dim3(NT), 0, st, work, out, (const uint32_t*)parent, n, ps, s, min_voxels);
        if (!launched()) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

}  // extern "C"
