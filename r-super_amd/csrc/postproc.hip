// Post-processing of the predicted volumes (predict_abdomenatlas.py / eval_AUC.py; integer and byte kernels, no MFMA):
//   detection      eval_AUC.detection :56-112: f64 align-corners trilinear zoom + 9-threshold erode / dilate / AND chain, collapsed to one
//                  integer pass over the output grid: L = #thresholds exceeded, F = min(max5(min3(L)), L), volume(t) = #(F > t)
//   binary det.    test_with_reports.detection :56-94: `value > th`, order-0 zoom, erode / dilate x 2 / AND, count: the one-threshold case of the
//                  tile pass above with a nearest sample; uint8 planes read as bytes
//   organ mask     postprocess_npz :655-688: lesion * box3_dilate(organ_a (+ organ_b) > 0.5)
//   largest cc     keep_largest_component :692-716: 6-connected union-find, root = smallest linear index, largest size / first root
// Every cross-workgroup result is an integer atomic (histogram bins, u64 max keys, union-find links): deterministic by construction.
#include "common.hpp"
#include "ccl.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int NT = CCL_NT;                               // threads per block of every kernel below (4 waves)
constexpr int GRID_CAP = 8192;                           // blocks of a grid-stride pass (tuned)

// ------------------------------------------------------------------------------------------------ shared helpers
// One separable box pass over a byte tile in LDS: d[z][y][x] = op(s[(z, y, x) + k * axis], k < K); d has the source extents minus K - 1 along AX.
template <bool MAX, int K, int AX>
__device__ __forceinline__ void box_pass(const uint8_t* s, uint8_t* d, int sz, int sy, int sx) {
    const int dz = AX == 2 ? sz - K + 1 : sz, dy = AX == 1 ? sy - K + 1 : sy, dx = AX == 0 ? sx - K + 1 : sx;
    const int step = AX == 0 ? 1 : AX == 1 ? sx : sx * sy;
    const int n = dz * dy * dx;
    for (int i = threadIdx.x; i < n; i += NT) {
        const int x = i % dx, t = i / dx, y = t % dy, z = t / dy;
        const uint8_t* p = s + (z * sy + y) * sx + x;
        uint8_t v = p[0];
#pragma unroll
        for (int k = 1; k < K; ++k) v = MAX ? (p[k * step] > v ? p[k * step] : v) : (p[k * step] < v ? p[k * step] : v);
        d[i] = v;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ detection
constexpr int DT_Z = 8, DT_Y = 16, DT_X = 32;            // output tile; the erode form adds a halo of 3 (min3 needs 1, max5 needs 2)
constexpr int DT_BINS = 256;                             // levels 0..255; workspace row = 256 bins + the max key

struct Thresholds { double t[255]; };                    // sorted ascending, by value in the kernel arguments (graph-capturable)

struct ZoomGrid {
    int Di, Hi, Wi, Do, Ho, Wo;
    double sz, sy, sx;                                   // input coordinate = output index * s (ndimage.zoom, grid_mode=False)
    int identity;                                        // all three axes unscaled: the sample is the input value itself
};

// false when the coordinate lies beyond the last input sample: ndimage's 'constant' mode maps it to cval (0) instead of interpolating, which
// happens to the last output plane of an axis whenever (n_out - 1) * s rounds above n_in - 1 in f64
__device__ __forceinline__ bool zoom_axis(int o, double s, int n, int& i0, int& i1, double& w1) {
    const double c = (double)o * s;
    if (c > (double)(n - 1)) return false;
    const int i = (int)c;                                // 0 <= c <= n - 1: truncation == floor
    i0 = i;
    i1 = i + 1 < n ? i + 1 : n - 1;                      // weight 0 at c == n - 1
    w1 = c - (double)i;
    return true;
}

// order-1 spline of ndimage.zoom in f64: sum over the 8 corners of ((value * wz) * wy) * wx, last axis fastest, no contraction into FMAs --
// the same operations in the same order as scipy's zoom_shift
__device__ __forceinline__ double zoom_sample(const float* __restrict__ x, const ZoomGrid& g, int z, int y, int xo) {
#pragma clang fp contract(off)
    if (g.identity) return (double)x[((long)z * g.Hi + y) * g.Wi + xo];
    int z0, z1, y0, y1, x0, x1;
    double fz, fy, fx;
    if (!zoom_axis(z, g.sz, g.Di, z0, z1, fz) || !zoom_axis(y, g.sy, g.Hi, y0, y1, fy) || !zoom_axis(xo, g.sx, g.Wi, x0, x1, fx)) return 0.0;
    const int zi[2] = {z0, z1}, yi[2] = {y0, y1}, xi[2] = {x0, x1};
    const double wz[2] = {1.0 - fz, fz}, wy[2] = {1.0 - fy, fy}, wx[2] = {1.0 - fx, fx};
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                t += (double)x[((long)zi[a] * g.Hi + yi[b]) * g.Wi + xi[c]] * wz[a] * wy[b] * wx[c];
    return t;
}

// number of thresholds v exceeds (thresholds sorted ascending): first index k with !(v > th[k])
__device__ __forceinline__ int level_of(double v, const double* th, int n) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v > th[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NT) void detect_zero_kernel(unsigned long long* ws, long n) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) ws[i] = 0ull;
}

// One block = one output tile of one plane.  The levels of the tile plus halo are computed from the input (the halo is recomputed by the
// neighbouring tiles; the input stays in L2), min3 / max5 run as separable byte passes in LDS, the final levels go into an LDS histogram and
// each non-empty bin is added to the plane's global bins once per block.
template <bool ERODE>
__global__ __launch_bounds__(NT) void detect_kernel(const float* __restrict__ x, long in_plane, ZoomGrid g, Thresholds th, int nth, int tiles_x,
                                                    int tiles_y, unsigned long long* __restrict__ ws) {
    constexpr int HL = ERODE ? 3 : 0;
    constexpr int RZ = DT_Z + 2 * HL, RY = DT_Y + 2 * HL, RX = DT_X + 2 * HL;
    constexpr int NA = ERODE ? RZ * RY * (RX - 2) : 1, NB = ERODE ? RZ * (RY - 2) * (RX - 2) : 1;
    __shared__ uint8_t r0[RZ * RY * RX];
    __shared__ uint8_t ba[NA], bb[NB];
    __shared__ double ths[255];
    __shared__ unsigned int lh[DT_BINS];
    __shared__ unsigned long long wmax[NT / 64];
    const int p = blockIdx.y;
    const float* xp = x + (long)p * in_plane;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / tiles_x / tiles_y;
    const int oz = tz * DT_Z - HL, oy = ty * DT_Y - HL, ox = tx * DT_X - HL;
    for (int i = threadIdx.x; i < nth; i += NT) ths[i] = th.t[i];
    for (int i = threadIdx.x; i < DT_BINS; i += NT) lh[i] = 0u;
    __syncthreads();
    unsigned long long mkey = 0ull;
    for (int i = threadIdx.x; i < RZ * RY * RX; i += NT) {
        const int rx = i % RX, t = i / RX, ry = t % RY, rz = t / RY;
        const int gz = oz + rz, gy = oy + ry, gx = ox + rx;
        uint8_t l = 0;                                   // outside the volume: level 0 (erosion's border_value = 0)
        if (gz >= 0 && gz < g.Do && gy >= 0 && gy < g.Ho && gx >= 0 && gx < g.Wo) {
            const double v = zoom_sample(xp, g, gz, gy, gx);
            l = (uint8_t)level_of(v, ths, nth);
            if (rz >= HL && rz < HL + DT_Z && ry >= HL && ry < HL + DT_Y && rx >= HL && rx < HL + DT_X) {
                const unsigned long long k = f64_key(v);
                mkey = k > mkey ? k : mkey;
            }
        }
        r0[i] = l;
    }
    __syncthreads();
    const uint8_t* fin = r0;
    if constexpr (ERODE) {
        // min3 over the tile + 2 (outside voxels are level 0, so their min3 is 0 and they add nothing to the max5 below)
        box_pass<false, 3, 0>(r0, ba, RZ, RY, RX);
        box_pass<false, 3, 1>(ba, bb, RZ, RY, RX - 2);
        box_pass<false, 3, 2>(bb, ba, RZ, RY - 2, RX - 2);
        // max5 over the tile (two box-3 dilations of a box domain)
        box_pass<true, 5, 0>(ba, bb, RZ - 2, RY - 2, RX - 2);
        box_pass<true, 5, 1>(bb, ba, RZ - 2, RY - 2, DT_X);
        box_pass<true, 5, 2>(ba, bb, RZ - 2, DT_Y, DT_X);
        fin = bb;
    }
    for (int i = threadIdx.x; i < DT_Z * DT_Y * DT_X; i += NT) {
        const int lx = i % DT_X, t = i / DT_X, ly = t % DT_Y, lz = t / DT_Y;
        if (oz + HL + lz >= g.Do || oy + HL + ly >= g.Ho || ox + HL + lx >= g.Wo) continue;
        const uint8_t l0 = r0[((lz + HL) * RY + ly + HL) * RX + lx + HL];
        uint8_t f = l0;
        if constexpr (ERODE) f = fin[i] < l0 ? fin[i] : l0;
        if (f) atomicAdd(&lh[f], 1u);                    // level 0 counts towards no threshold: not binned
    }
    mkey = wave_max_u64(mkey);
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mkey;
    __syncthreads();
    unsigned long long* row = ws + (long)p * (DT_BINS + 1);
    for (int b = threadIdx.x; b < DT_BINS; b += NT)
        if (lh[b]) atomicAdd(&row[b], (unsigned long long)lh[b]);
    if (threadIdx.x == 0) {
        unsigned long long m = wmax[0];
        for (int w = 1; w < NT / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
        if (m) atomicMax(&row[DT_BINS], m);
    }
}

// volumes[p][t] = #(final level > t) = sum of the bins above t; max_prob[p] from its key.  One block per plane.
__global__ __launch_bounds__(NT) void detect_finalize_kernel(const unsigned long long* __restrict__ ws, int nth, long long* volumes, double* max_prob) {
    const int p = blockIdx.x;
    const unsigned long long* row = ws + (long)p * (DT_BINS + 1);
    for (int t = threadIdx.x; t < nth; t += NT) {
        unsigned long long s = 0ull;
        for (int l = t + 1; l <= nth; ++l) s += row[l];
        volumes[(long)p * nth + t] = (long long)s;
    }
    if (threadIdx.x == 0) max_prob[p] = key_f64(row[DT_BINS]);
}

// ------------------------------------------------------------------------------------------------ binary detection
// test_with_reports.detection :56-94: the one-threshold case of detect_kernel on a mask binarised BEFORE the zoom, sampled with ndimage.zoom's
// order 0.  Source index of output o along an axis: floor(c + 0.5) with c = o * s; -1 (the constant 0) beyond the last input sample, as in zoom_axis.
__device__ __forceinline__ int nearest_axis(int o, double s, int n) {
    const double c = (double)o * s;
    if (c > (double)(n - 1)) return -1;
    return (int)(c + 0.5);                               // 0 <= c <= n - 1: truncation == floor, and the index stays <= n - 1
}

// Same tile, halo and LDS box_pass chain as detect_kernel with levels in {0, 1}; T = uint8_t (labels, bool) or float, `value > th` in f64 like
// get_fdata().  The set voxels of the tile go to bin 1 of the plane's workspace row, one integer atomic per block.
template <typename T, bool ERODE>
__global__ __launch_bounds__(NT) void detect_binary_kernel(const T* __restrict__ x, long in_plane, ZoomGrid g, double th, int tiles_x, int tiles_y,
                                                           unsigned long long* __restrict__ ws) {
    constexpr int HL = ERODE ? 3 : 0;
    constexpr int RZ = DT_Z + 2 * HL, RY = DT_Y + 2 * HL, RX = DT_X + 2 * HL;
    constexpr int NA = ERODE ? RZ * RY * (RX - 2) : 1, NB = ERODE ? RZ * (RY - 2) * (RX - 2) : 1;
    __shared__ uint8_t r0[RZ * RY * RX];
    __shared__ uint8_t ba[NA], bb[NB];
    __shared__ unsigned int cnt;
    const int p = blockIdx.y;
    const T* xp = x + (long)p * in_plane;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / tiles_x / tiles_y;
    const int oz = tz * DT_Z - HL, oy = ty * DT_Y - HL, ox = tx * DT_X - HL;
    if (threadIdx.x == 0) cnt = 0u;
    for (int i = threadIdx.x; i < RZ * RY * RX; i += NT) {
        const int rx = i % RX, t = i / RX, ry = t % RY, rz = t / RY;
        const int gz = oz + rz, gy = oy + ry, gx = ox + rx;
        uint8_t l = 0;                                   // outside the volume: 0 (erosion's border_value = 0)
        if (gz >= 0 && gz < g.Do && gy >= 0 && gy < g.Ho && gx >= 0 && gx < g.Wo) {
            const int iz = nearest_axis(gz, g.sz, g.Di), iy = nearest_axis(gy, g.sy, g.Hi), ix = nearest_axis(gx, g.sx, g.Wi);
            if (iz >= 0 && iy >= 0 && ix >= 0) l = (double)xp[((long)iz * g.Hi + iy) * g.Wi + ix] > th ? 1 : 0;
        }
        r0[i] = l;
    }
    __syncthreads();
    const uint8_t* fin = r0;
    if constexpr (ERODE) {
        box_pass<false, 3, 0>(r0, ba, RZ, RY, RX);
        box_pass<false, 3, 1>(ba, bb, RZ, RY, RX - 2);
        box_pass<false, 3, 2>(bb, ba, RZ, RY - 2, RX - 2);
        box_pass<true, 5, 0>(ba, bb, RZ - 2, RY - 2, RX - 2);
        box_pass<true, 5, 1>(bb, ba, RZ - 2, RY - 2, DT_X);
        box_pass<true, 5, 2>(ba, bb, RZ - 2, DT_Y, DT_X);
        fin = bb;
    }
    unsigned int n = 0u;
    for (int i = threadIdx.x; i < DT_Z * DT_Y * DT_X; i += NT) {
        const int lx = i % DT_X, t = i / DT_X, ly = t % DT_Y, lz = t / DT_Y;
        if (oz + HL + lz >= g.Do || oy + HL + ly >= g.Ho || ox + HL + lx >= g.Wo) continue;
        uint8_t f = r0[((lz + HL) * RY + ly + HL) * RX + lx + HL];
        if constexpr (ERODE) f = fin[i] < f ? fin[i] : f;
        n += f;
    }
    if (n) atomicAdd(&cnt, n);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(&ws[(long)p * (DT_BINS + 1) + 1], (unsigned long long)cnt);
}

__global__ __launch_bounds__(NT) void detect_binary_finalize_kernel(const unsigned long long* __restrict__ ws, int planes, long long* counts) {
    for (int p = blockIdx.x * NT + threadIdx.x; p < planes; p += gridDim.x * NT) counts[p] = (long long)ws[(long)p * (DT_BINS + 1) + 1];
}

// ------------------------------------------------------------------------------------------------ organ mask
constexpr int OM_Z = 8, OM_Y = 16, OM_X = 32;            // output tile; halo 1 for the box-3 dilation
constexpr int OM_MAX = 128;                              // lesion planes per launch

struct OrganPlanes { int les[OM_MAX], oa[OM_MAX], ob[OM_MAX]; };

// `organ > 0.5` of postprocess_npz: labels add as uint8 (wrapping), probabilities as f32
__device__ __forceinline__ bool organ_on(const uint8_t* a, const uint8_t* b, long i) { return (uint8_t)(b ? a[i] + b[i] : a[i]) > 0; }
__device__ __forceinline__ bool organ_on(const float* a, const float* b, long i) { return (b ? a[i] + b[i] : a[i]) > 0.5f; }
// organ.astype(lesion dtype) * lesion
__device__ __forceinline__ uint8_t masked(bool m, uint8_t l) { return (uint8_t)((m ? 1 : 0) * l); }
__device__ __forceinline__ float masked(bool m, float l) { return (m ? 1.0f : 0.0f) * l; }

template <typename T>
__global__ __launch_bounds__(NT) void organ_mask_kernel(const T* __restrict__ pred, T* __restrict__ out, OrganPlanes pl, int D, int H, int W,
                                                        int tiles_x, int tiles_y) {
    constexpr int RZ = OM_Z + 2, RY = OM_Y + 2, RX = OM_X + 2;
    __shared__ uint8_t r0[RZ * RY * RX], ba[RZ * RY * OM_X], bb[RZ * OM_Y * OM_X];
    const int k = blockIdx.y;
    const long V = (long)D * H * W;
    const T* oa = pred + (long)pl.oa[k] * V;
    const T* ob = pl.ob[k] >= 0 ? pred + (long)pl.ob[k] * V : nullptr;
    const T* les = pred + (long)pl.les[k] * V;
    T* o = out + (long)k * V;
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / tiles_x / tiles_y;
    const int oz = tz * OM_Z - 1, oy = ty * OM_Y - 1, ox = tx * OM_X - 1;
    for (int i = threadIdx.x; i < RZ * RY * RX; i += NT) {
        const int rx = i % RX, t = i / RX, ry = t % RY, rz = t / RY;
        const int gz = oz + rz, gy = oy + ry, gx = ox + rx;
        bool m = false;                                  // binary_dilation's border_value = 0
        if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) m = organ_on(oa, ob, ((long)gz * H + gy) * W + gx);
        r0[i] = m;
    }
    __syncthreads();
    box_pass<true, 3, 0>(r0, ba, RZ, RY, RX);
    box_pass<true, 3, 1>(ba, bb, RZ, RY, OM_X);
    box_pass<true, 3, 2>(bb, r0, RZ, OM_Y, OM_X);
    for (int i = threadIdx.x; i < OM_Z * OM_Y * OM_X; i += NT) {
        const int lx = i % OM_X, t = i / OM_X, ly = t % OM_Y, lz = t / OM_Y;
        const int gz = oz + 1 + lz, gy = oy + 1 + ly, gx = ox + 1 + lx;
        if (gz >= D || gy >= H || gx >= W) continue;
        const long gi = ((long)gz * H + gy) * W + gx;
        o[gi] = masked(r0[i] != 0, les[gi]);
    }
}

// ------------------------------------------------------------------------------------------------ largest connected component
// The labeller itself (tile pass, border pass, compression, the union-find and why its loads are agent-scope atomics) is ccl.hpp, 6-connected here.
__device__ __forceinline__ bool fg(const uint8_t* m, long i) { return m[i] > 0; }
__device__ __forceinline__ bool fg(const float* m, long i) { return m[i] > 0.f; }

// (a) label one tile, zero the size counters and the key
template <typename T>
__global__ __launch_bounds__(NT) void cc_local_kernel(const T* __restrict__ m, uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                      unsigned long long* key, int D, int H, int W, int tiles_x, int tiles_y) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *key = 0ull;
    ccl_label_tile<6>(parent, blockIdx.x, tiles_x, tiles_y, D, H, W, [&](long gi) {
        count[gi] = 0u;
        return fg(m, gi);
    });
}

// (b) link across the three low faces of every tile
__global__ __launch_bounds__(NT) void cc_merge_kernel(uint32_t* parent, int D, int H, int W, int tiles_x, int tiles_y) {
    ccl_link_borders<6>(parent, blockIdx.x, tiles_x, tiles_y, D, H, W);
}

// (c) path compression + component sizes: one counter add per distinct root in a wave
__global__ __launch_bounds__(NT) void cc_compress_kernel(uint32_t* parent, uint32_t* __restrict__ count, long n) {
    const int lane = threadIdx.x & 63;
    for (long base = (long)blockIdx.x * NT; base < n; base += (long)gridDim.x * NT) {
        const long i = base + threadIdx.x;
        bool act = false;
        uint32_t r = 0;
        if (i < n) {
            r = ccl_compress(parent, i);
            act = r != CCL_BG;
        }
        unsigned long long pend = __ballot(act);
        while (pend) {
            const int leader = __ffsll((long long)pend) - 1;
            const uint32_t lr = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(act && r == lr);
            if (lane == leader) atomicAdd(&count[lr], (uint32_t)__popcll(same));
            if (act && r == lr) act = false;
            pend &= ~same;
        }
    }
}

// (d) key = (size << 32) | (0xFFFFFFFF - root): the largest size, ties to the smallest root (= first in raster order)
__global__ __launch_bounds__(NT) void cc_pick_kernel(const uint32_t* __restrict__ count, long n, unsigned long long* key) {
    unsigned long long best = 0ull;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const uint32_t c = count[i];                     // non-zero only at roots
        if (c) {
            const unsigned long long k = ((unsigned long long)c << 32) | (0xFFFFFFFFull - (unsigned long long)i);
            best = k > best ? k : best;
        }
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0 && best) atomicMax(key, best);
}

// (e) out = (root == chosen root); no component at all -> all ones (sitk.Equal(cc, 0) of the reference on an empty mask)
__global__ __launch_bounds__(NT) void cc_write_kernel(const uint32_t* __restrict__ parent, const unsigned long long* __restrict__ key, long n,
                                                      uint8_t* __restrict__ out) {
    const unsigned long long k = *key;
    const uint32_t sel = (uint32_t)(0xFFFFFFFFull - (k & 0xFFFFFFFFull));
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT)
        out[i] = k == 0ull ? 1 : (parent[i] == sel ? 1 : 0);
}

template <typename T>
int organ_mask_launch(const T* pred, int D, int H, int W, int n, const int* lesion, const int* organ_a, const int* organ_b, T* out, hipStream_t st) {
    const int tx = (W + OM_X - 1) / OM_X, ty = (H + OM_Y - 1) / OM_Y, tz = (D + OM_Z - 1) / OM_Z;
    for (int k0 = 0; k0 < n; k0 += OM_MAX) {
        const int nk = n - k0 < OM_MAX ? n - k0 : OM_MAX;
        OrganPlanes pl;
        for (int k = 0; k < nk; ++k) { pl.les[k] = lesion[k0 + k]; pl.oa[k] = organ_a[k0 + k]; pl.ob[k] = organ_b[k0 + k]; }
        hipLaunchKernelGGL(organ_mask_kernel<T>, dim3(tx * ty * tz, nk), dim3(NT), 0, st, pred, out + (long)k0 * D * H * W, pl, D, H, W, tx, ty);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

template <typename T>
int largest_component_launch(const T* m, int D, int H, int W, uint8_t* out, void* ws, hipStream_t st) {
    const long n = (long)D * H * W;
    unsigned long long* key = (unsigned long long*)ws;
    uint32_t* parent = (uint32_t*)((char*)ws + 256);
    uint32_t* count = parent + ((n + 63) & ~63L);
    const int tx = (W + CCL_X - 1) / CCL_X, ty = (H + CCL_Y - 1) / CCL_Y, tz = (D + CCL_Z - 1) / CCL_Z;
    hipLaunchKernelGGL(cc_local_kernel<T>, dim3(tx * ty * tz), dim3(NT), 0, st, m, parent, count, key, D, H, W, tx, ty);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(tx * ty * tz), dim3(NT), 0, st, parent, D, H, W, tx, ty);
    hipLaunchKernelGGL(cc_compress_kernel, dim3(grid_for(n, GRID_CAP)), dim3(NT), 0, st, parent, count, n);
    hipLaunchKernelGGL(cc_pick_kernel, dim3(grid_for(n, GRID_CAP)), dim3(NT), 0, st, (const uint32_t*)count, n, key);
    hipLaunchKernelGGL(cc_write_kernel, dim3(grid_for(n, GRID_CAP)), dim3(NT), 0, st, (const uint32_t*)parent, (const unsigned long long*)key, n, out);
    return rs_check_launch();
}

bool dims_ok(int D, int H, int W) { return D > 0 && H > 0 && W > 0 && (long)D * H * W <= (1L << 31); }

}  // namespace

extern "C" {

long rsuper_detection_workspace_bytes(int planes) { return planes > 0 ? (long)planes * (DT_BINS + 1) * 8 : 0; }

int rsuper_detection(const float* x, int planes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, const double* thresholds, int nthr, int erode,
                     long long* volumes, double* max_prob, void* workspace, void* stream) {
    if (!x || !thresholds || !volumes || !max_prob || !workspace || planes < 1 || planes > 65535 || nthr < 1 || nthr > 255) return RS_ERR_ARG;
    if (!dims_ok(Di, Hi, Wi) || !dims_ok(Do, Ho, Wo)) return RS_ERR_ARG;
    Thresholds th;
    for (int i = 0; i < nthr; ++i) {
        if (i > 0 && !(thresholds[i] >= thresholds[i - 1])) return RS_ERR_ARG;     // sorted ascending, no NaN
        th.t[i] = thresholds[i];
    }
    for (int i = nthr; i < 255; ++i) th.t[i] = 0.0;
    ZoomGrid g;
    g.Di = Di; g.Hi = Hi; g.Wi = Wi; g.Do = Do; g.Ho = Ho; g.Wo = Wo;
    g.sz = Do > 1 ? (double)(Di - 1) / (double)(Do - 1) : 0.0;
    g.sy = Ho > 1 ? (double)(Hi - 1) / (double)(Ho - 1) : 0.0;
    g.sx = Wo > 1 ? (double)(Wi - 1) / (double)(Wo - 1) : 0.0;
    g.identity = Di == Do && Hi == Ho && Wi == Wo;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* ws = (unsigned long long*)workspace;
    const long nws = (long)planes * (DT_BINS + 1);
    hipLaunchKernelGGL(detect_zero_kernel, dim3(grid_for(nws, GRID_CAP)), dim3(NT), 0, st, ws, nws);
    const int tx = (Wo + DT_X - 1) / DT_X, ty = (Ho + DT_Y - 1) / DT_Y, tz = (Do + DT_Z - 1) / DT_Z;
    const dim3 grid(tx * ty * tz, planes);
    const long in_plane = (long)Di * Hi * Wi;
    if (erode) hipLaunchKernelGGL(detect_kernel<true>, grid, dim3(NT), 0, st, x, in_plane, g, th, nthr, tx, ty, ws);
    else hipLaunchKernelGGL(detect_kernel<false>, grid, dim3(NT), 0, st, x, in_plane, g, th, nthr, tx, ty, ws);
    hipLaunchKernelGGL(detect_finalize_kernel, dim3(planes), dim3(NT), 0, st, (const unsigned long long*)ws, nthr, volumes, max_prob);
    return rs_check_launch();
}

int rsuper_detection_binary(const void* x, int is_u8, int planes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, double th, int erode,
                            long long* counts, void* workspace, void* stream) {
    if (!x || !counts || !workspace || planes < 1 || planes > 65535 || !(th == th)) return RS_ERR_ARG;
    if (!dims_ok(Di, Hi, Wi) || !dims_ok(Do, Ho, Wo)) return RS_ERR_ARG;
    ZoomGrid g;
    g.Di = Di; g.Hi = Hi; g.Wi = Wi; g.Do = Do; g.Ho = Ho; g.Wo = Wo;
    g.sz = Do > 1 ? (double)(Di - 1) / (double)(Do - 1) : 0.0;
    g.sy = Ho > 1 ? (double)(Hi - 1) / (double)(Ho - 1) : 0.0;
    g.sx = Wo > 1 ? (double)(Wi - 1) / (double)(Wo - 1) : 0.0;
    g.identity = 0;                                      // unused: an unscaled axis has s == 1.0 and samples its own index
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* ws = (unsigned long long*)workspace;
    const long nws = (long)planes * (DT_BINS + 1);
    hipLaunchKernelGGL(detect_zero_kernel, dim3(grid_for(nws, GRID_CAP)), dim3(NT), 0, st, ws, nws);
    const int tx = (Wo + DT_X - 1) / DT_X, ty = (Ho + DT_Y - 1) / DT_Y, tz = (Do + DT_Z - 1) / DT_Z;
    const dim3 grid(tx * ty * tz, planes);
    const long in_plane = (long)Di * Hi * Wi;
    if (is_u8) {
        const uint8_t* xb = (const uint8_t*)x;
        if (erode) hipLaunchKernelGGL((detect_binary_kernel<uint8_t, true>), grid, dim3(NT), 0, st, xb, in_plane, g, th, tx, ty, ws);
        else hipLaunchKernelGGL((detect_binary_kernel<uint8_t, false>), grid, dim3(NT), 0, st, xb, in_plane, g, th, tx, ty, ws);
    } else {
        const float* xf = (const float*)x;
        if (erode) hipLaunchKernelGGL((detect_binary_kernel<float, true>), grid, dim3(NT), 0, st, xf, in_plane, g, th, tx, ty, ws);
        else hipLaunchKernelGGL((detect_binary_kernel<float, false>), grid, dim3(NT), 0, st, xf, in_plane, g, th, tx, ty, ws);
    }
    hipLaunchKernelGGL(detect_binary_finalize_kernel, dim3(grid_for(planes, GRID_CAP)), dim3(NT), 0, st, (const unsigned long long*)ws, planes, counts);
    return rs_check_launch();
}

int rsuper_organ_mask_u8(const uint8_t* pred, int C, int D, int H, int W, int n, const int* lesion, const int* organ_a, const int* organ_b,
                         uint8_t* out, void* stream) {
    if (!pred || !out || !lesion || !organ_a || !organ_b || n < 1 || n > 65535 * OM_MAX || !dims_ok(D, H, W)) return RS_ERR_ARG;
    for (int k = 0; k < n; ++k)
        if (lesion[k] < 0 || lesion[k] >= C || organ_a[k] < 0 || organ_a[k] >= C || organ_b[k] < -1 || organ_b[k] >= C) return RS_ERR_ARG;
    return organ_mask_launch(pred, D, H, W, n, lesion, organ_a, organ_b, out, (hipStream_t)stream);
}

int rsuper_organ_mask_f32(const float* pred, int C, int D, int H, int W, int n, const int* lesion, const int* organ_a, const int* organ_b,
                          float* out, void* stream) {
    if (!pred || !out || !lesion || !organ_a || !organ_b || n < 1 || n > 65535 * OM_MAX || !dims_ok(D, H, W)) return RS_ERR_ARG;
    for (int k = 0; k < n; ++k)
        if (lesion[k] < 0 || lesion[k] >= C || organ_a[k] < 0 || organ_a[k] >= C || organ_b[k] < -1 || organ_b[k] >= C) return RS_ERR_ARG;
    return organ_mask_launch(pred, D, H, W, n, lesion, organ_a, organ_b, out, (hipStream_t)stream);
}

long rsuper_largest_component_workspace_bytes(int D, int H, int W) {
    if (!dims_ok(D, H, W)) return 0;
    const long n = (long)D * H * W;
    return 256 + 2 * ((n + 63) & ~63L) * 4;
}

int rsuper_largest_component(const void* mask, int is_u8, int D, int H, int W, uint8_t* out, void* workspace, void* stream) {
    if (!mask || !out || !workspace || !dims_ok(D, H, W)) return RS_ERR_ARG;
    if (is_u8) return largest_component_launch((const uint8_t*)mask, D, H, W, out, workspace, (hipStream_t)stream);
    return largest_component_launch((const float*)mask, D, H, W, out, workspace, (hipStream_t)stream);
}

}  // extern "C"
