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
#include "ccl.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int NT = CCL_NT;                               // threads per block (4 waves)
constexpr int GRID_CAP = 2048;                           // blocks of a grid-stride pass (tuned)
constexpr int PL_MAX_PLANES = RSUPER_LESION_MAX_PLANES;

struct PlaneState {                                      // RSUPER_LESION_STATE_WORDS 32-bit words per plane
    int kept, iterations, done, n_lesions;
    unsigned long long key;                              // (orderable peak bits << 32) | (0xFFFFFFFF - seed index); 0 = not computed
    uint32_t root, size;                                 // the seed component's root and voxel count
};
static_assert(sizeof(PlaneState) == RSUPER_LESION_STATE_WORDS * 4, "state layout");

struct Counts { int n[PL_MAX_PLANES]; };

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

// (2) stop or go; label one tile of work >= thr in LDS, parent = global index of the tile-local root (outside the mask: CCL_BG)
__global__ __launch_bounds__(NT) void pl_local_kernel(const float* __restrict__ work, uint32_t* __restrict__ parent, long n, long pstride, PlaneState* st,
                                                      float peak_cut, float min_peak, int D, int H, int W, int tiles_x, int tiles_y) {
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
    ccl_label_tile<26>(parent + (long)blockIdx.y * pstride, blockIdx.x, tiles_x, tiles_y, D, H, W, [&](long gi) { return w[gi] >= thr; });
}

// (3) every mask voxel with a backward neighbour outside its tile links to it (ccl.hpp: the low z / y / x faces and the high y and x faces)
__global__ __launch_bounds__(NT) void pl_merge_kernel(uint32_t* parent, long pstride, const PlaneState* st, int D, int H, int W, int tiles_x, int tiles_y) {
    if (st[blockIdx.y].done) return;
    ccl_link_borders<26>(parent + (long)blockIdx.y * pstride, blockIdx.x, tiles_x, tiles_y, D, H, W);
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
        // 0 < peak_cut <= 1); were the seed ever outside it, its word is CCL_BG, which is no index: nothing is followed and pl_apply ends the plane
        seed_root = g_load(&par[seed]) == CCL_BG ? CCL_BG : g_find(par, seed);
        if (blockIdx.x == 0) s->root = seed_root;
    }
    __syncthreads();
    const uint32_t root = seed_root;
    uint32_t mine = 0u;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const uint32_t r = ccl_compress(par, i);
        mine += r != CCL_BG && r == root ? 1u : 0u;      // root itself is CCL_BG when the seed has no component
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
    if (root == CCL_BG) {                                 // no seed component (see pl_count): nothing to zero, so the plane could not advance -- end it
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
    hipLaunchKernelGGL(pl_begin_kernel, dim3(grid_for(total, GRID_CAP)), dim3(NT), 0, (hipStream_t)stream, out, total, (PlaneState*)state, c, planes);
    return rs_check_launch();
}

int rsuper_lesion_candidates_run(float* work, uint8_t* out, int planes, int D, int H, int W, float peak_cut, int min_voxels, float min_peak, void* state,
                                 void* workspace, int iterations, void* stream) {
    if (!work || !out || !state || !workspace || !shape_ok(planes, D, H, W)) return RS_ERR_ARG;
    if (!(peak_cut > 0.f && peak_cut <= 1.f) || !(min_peak > 0.f) || min_voxels < 1 || iterations < 1) return RS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    PlaneState* s = (PlaneState*)state;
    uint32_t* parent = (uint32_t*)workspace;
    const long n = (long)D * H * W, ps = parent_stride(n);
    const int tx = (W + CCL_X - 1) / CCL_X, ty = (H + CCL_Y - 1) / CCL_Y, tz = (D + CCL_Z - 1) / CCL_Z;
    const dim3 tiles(tx * ty * tz, planes), flat(grid_for(n, GRID_CAP), planes);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(pl_peak_kernel, flat, dim3(NT), 0, st, (const float*)work, n, s);
        hipLaunchKernelGGL(pl_local_kernel, tiles, dim3(NT), 0, st, (const float*)work, parent, n, ps, s, peak_cut, min_peak, D, H, W, tx, ty);
        hipLaunchKernelGGL(pl_merge_kernel, tiles, dim3(NT), 0, st, parent, ps, (const PlaneState*)s, D, H, W, tx, ty);
        hipLaunchKernelGGL(pl_count_kernel, flat, dim3(NT), 0, st, parent, n, ps, s);
        hipLaunchKernelGGL(pl_apply_kernel, flat, dim3(NT), 0, st, work, out, (const uint32_t*)parent, n, ps, s, min_voxels);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

}  // extern "C"
