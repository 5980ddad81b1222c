// Surface-distance metrics of the validation loop (metric/metrics.py compute_surface_distances :265-573; byte, integer and f64 kernels, no MFMA):
//   surface codes  the 2x2x2 neighbour code of both masks on the corner grid (D+1, H+1, W+1), the box of the border corners (code neither 0 nor
//                  255) of either mask, the voxel counts |gt|, |pred|, |gt & pred| and the border-corner counts, from one read of the masks
//   edt3           exact squared Euclidean distance transform (anisotropic spacing, f64) of a corner sub-box to the border corners of one code
//                  volume, separable in three passes: a wave-level nearest-set-bit scan along W, then a Felzenszwalb-Huttenlocher lower envelope
//                  per line along H and along D with adjacent lanes on adjacent w; the envelope stacks live in a caller workspace that mirrors
//                  the layout of the map, so the lanes of a wave interleave
//   surfel gather  (sqrt of the other mask's map, table[code]) of every border corner, compacted
// Every cross-workgroup result is an integer atomic (counts, box bounds, the compaction cursor): the values never depend on the order.  The
// compacted pairs are sorted by the caller, so the order the cursor hands out does not reach any result either.
#include "common.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int NT = 256;                                  // threads per block of every kernel below (4 waves)
constexpr int SC_ITEMS = 8;                              // corner chunks of NT per block of the code kernel: one set of atomics per 2048 corners
constexpr int EDT_MAX_SIDE = 4096;                       // corners per line (the W pass keeps one int per 64 corners of its line in LDS)
constexpr int NO_FEATURE = 1 << 28;                      // |index distance| of a line without a border corner

__device__ __forceinline__ bool is_border(uint8_t c) { return c != 0 && c != 255; }

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

// ------------------------------------------------------------------------------------------------ surface codes
// bbox[p] = {min z, min y, min x, max z, max y, max x} of the border corners (min > max: none); counts[p] = {|gt|, |pred|, |gt & pred|,
// border corners of gt, border corners of pred}
__global__ __launch_bounds__(NT) void sc_init_kernel(int* bbox, unsigned long long* counts, int P) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < P * 6) bbox[i] = (i % 6) < 3 ? 0x7FFFFFFF : -1;
    if (i < P * 5) counts[i] = 0ull;
}

// correlate(mask, [[[128, 64], [32, 16]], [[8, 4], [2, 1]]], mode='constant'): corner (i, j, k) sees voxels i-1..i, j-1..j, k-1..k, zero outside
__device__ __forceinline__ uint8_t corner_code(const uint8_t* __restrict__ m, int i, int j, int k, int D, int H, int W) {
    unsigned c = 0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int z = i - 1 + a, y = j - 1 + b, x = k - 1 + e;
                bool on = false;
                if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) on = m[((long)z * H + y) * W + x] != 0;
                c |= (on ? 1u : 0u) << (7 - (a * 4 + b * 2 + e));
            }
    return (uint8_t)c;
}

__global__ __launch_bounds__(NT) void surface_codes_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred, int D, int H, int W,
                                                           uint8_t* __restrict__ cg, uint8_t* __restrict__ cp, int* bbox,
                                                           unsigned long long* counts) {
    __shared__ int sbox[NT / 64][6];
    __shared__ unsigned int scnt[NT / 64][5];
    const int p = blockIdx.y;
    const long V = (long)D * H * W, NC = (long)(D + 1) * (H + 1) * (W + 1);
    const uint8_t* g = gt + (long)p * V;
    const uint8_t* q = pred + (long)p * V;
    uint8_t* og = cg + (long)p * NC;
    uint8_t* op = cp + (long)p * NC;
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
    unsigned int n[5] = {0u, 0u, 0u, 0u, 0u};
    for (int it = 0; it < SC_ITEMS; ++it) {
        const long c = ((long)blockIdx.x * SC_ITEMS + it) * NT + threadIdx.x;
        if (c >= NC) break;
        const int k = (int)(c % (W + 1));
        const long t = c / (W + 1);
        const int j = (int)(t % (H + 1)), i = (int)(t / (H + 1));
        const uint8_t a = corner_code(g, i, j, k, D, H, W), b = corner_code(q, i, j, k, D, H, W);
        og[c] = a;
        op[c] = b;
        n[0] += a & 1u;                                  // weight 1 is voxel (i, j, k) itself: every voxel is counted at its own corner
        n[1] += b & 1u;
        n[2] += a & b & 1u;
        const bool ba = is_border(a), bb = is_border(b);
        n[3] += ba;
        n[4] += bb;
        if (ba || bb) {
            lo[0] = i < lo[0] ? i : lo[0]; lo[1] = j < lo[1] ? j : lo[1]; lo[2] = k < lo[2] ? k : lo[2];
            hi[0] = i > hi[0] ? i : hi[0]; hi[1] = j > hi[1] ? j : hi[1]; hi[2] = k > hi[2] ? k : hi[2];
        }
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int l = wave_min_i(lo[a]), h = wave_max_i(hi[a]);
        if (lane == 0) { sbox[w][a] = l; sbox[w][3 + a] = h; }
    }
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        int v = (int)n[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) scnt[w][a] = (unsigned int)v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        int v = sbox[0][a];
        for (int k = 1; k < NT / 64; ++k) v = a < 3 ? (sbox[k][a] < v ? sbox[k][a] : v) : (sbox[k][a] > v ? sbox[k][a] : v);
        if (a < 3) { if (v != 0x7FFFFFFF) atomicMin(&bbox[p * 6 + a], v); }
        else if (v >= 0) atomicMax(&bbox[p * 6 + a], v);
    } else if (threadIdx.x >= 64 && threadIdx.x < 69) {
        const int a = threadIdx.x - 64;
        unsigned int v = 0u;
        for (int k = 0; k < NT / 64; ++k) v += scnt[k][a];
        if (v) atomicAdd(&counts[p * 5 + a], (unsigned long long)v);
    }
}

// ------------------------------------------------------------------------------------------------ exact distance transform
struct Box { int z0, y0, x0, nz, ny, nx; };

// Pass along W: one wave per (z, y) line of the box.  The border bits of 64 corners are one ballot word; the nearest border to the left of a lane
// is the highest set bit at or below it (or the carry from the chunks before), the nearest to the right the lowest set bit at or above it (or the
// carry from the chunks after, kept per chunk in LDS by a first right-to-left sweep).  out = (s2 * |x - nearest|)^2, +inf on a line without one.
__global__ __launch_bounds__(NT) void edt_w_kernel(const uint8_t* __restrict__ codes, int Hc, int Wc, Box bx, double s2, double* __restrict__ out) {
    __shared__ int next_r[NT / 64][EDT_MAX_SIDE / 64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long line = (long)blockIdx.x * (NT / 64) + w;
    if (line >= (long)bx.nz * bx.ny) return;             // wave-uniform; the kernel has no block barrier
    const int z = (int)(line / bx.ny), y = (int)(line % bx.ny);
    const uint8_t* src = codes + ((long)(bx.z0 + z) * Hc + bx.y0 + y) * Wc + bx.x0;
    double* dst = out + line * bx.nx;
    const int nch = (bx.nx + 63) >> 6;
    int carry = NO_FEATURE;                              // index of the first border corner in the chunks after this one
    for (int c = nch - 1; c >= 0; --c) {
        const int x = c * 64 + lane;
        const unsigned long long bal = __ballot(x < bx.nx && is_border(src[x]));
        next_r[w][c] = carry;                            // every lane stores the same word and reads back its own store
        if (bal) carry = c * 64 + __ffsll((long long)bal) - 1;
    }
    int last = -NO_FEATURE;                              // index of the last border corner in the chunks before this one
    for (int c = 0; c < nch; ++c) {
        const int x = c * 64 + lane;
        const unsigned long long bal = __ballot(x < bx.nx && is_border(src[x]));
        const unsigned long long below = bal & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)), above = bal & (~0ull << lane);
        const int l = below ? c * 64 + 63 - __clzll((long long)below) : last;
        const int r = above ? c * 64 + __ffsll((long long)above) - 1 : next_r[w][c];
        const int dl = x - l, dr = r - x;
        const int g = dl < dr ? dl : dr;
        if (x < bx.nx) {
            const double d = s2 * (double)g;
            dst[x] = g >= NO_FEATURE / 2 ? INFINITY : d * d;
        }
        if (bal) last = c * 64 + 63 - __clzll((long long)bal);
    }
}

// Pass along H or D, in place: one thread per line, adjacent threads on adjacent x.  Element q of the line is map[base + q * st]; the envelope
// stack of the line (parabola index v, its value f, the start z of its interval) sits at the same addresses of the workspace arrays, so the k-th
// stack entries of adjacent lines are adjacent words.  Lower envelope of f(p) + sp2 * (q - p)^2 over the finite f(p) (Felzenszwalb & Huttenlocher
// 2012): intersections in f64, in units of the index.  A line with no finite value stays +inf.
__global__ __launch_bounds__(NT) void edt_line_kernel(double* __restrict__ map, double* __restrict__ wz, double* __restrict__ wf, int* __restrict__ wv,
                                                      long lines, int nx, long outer_stride, long st, int n, double sp2) {
    const long t = (long)blockIdx.x * NT + threadIdx.x;
    if (t >= lines) return;
    const long base = (t / nx) * outer_stride + (t % nx);
    const double inv = 0.5 / sp2;
    int k = -1, tv = 0;                                  // top of the stack in registers: (tv, tf, tz)
    double tf = 0.0, tz = -INFINITY;
    for (int q = 0; q < n; ++q) {
        const double f = map[base + (long)q * st];
        if (!(f < INFINITY)) continue;
        double s = -INFINITY;
        while (k >= 0) {
            s = (f - tf) * inv / (double)(q - tv) + 0.5 * (double)(q + tv);
            if (k > 0 && s <= tz) {                      // the top parabola is nowhere the lowest any more
                --k;
                tv = wv[base + (long)k * st]; tf = wf[base + (long)k * st]; tz = wz[base + (long)k * st];
            } else break;
        }
        ++k;
        tv = q; tf = f; tz = k == 0 ? -INFINITY : s;
        wv[base + (long)k * st] = tv; wf[base + (long)k * st] = tf; wz[base + (long)k * st] = tz;
    }
    if (k < 0) return;
    const int K = k;
    int j = 0, v = wv[base];
    double f = wf[base], nz = K >= 1 ? wz[base + st] : INFINITY;
    for (int q = 0; q < n; ++q) {
        while (nz < (double)q) {
            ++j;
            v = wv[base + (long)j * st]; f = wf[base + (long)j * st];
            nz = j < K ? wz[base + (long)(j + 1) * st] : INFINITY;
        }
        const double d = (double)(q - v);
        map[base + (long)q * st] = sp2 * d * d + f;
    }
}

// ------------------------------------------------------------------------------------------------ surfel gather
__global__ void sg_init_kernel(unsigned long long* count) { *count = 0ull; }

__global__ __launch_bounds__(NT) void surfel_gather_kernel(const uint8_t* __restrict__ codes, int Hc, int Wc, Box bx, const double* __restrict__ sq,
                                                           const double* __restrict__ table, double* __restrict__ dist, double* __restrict__ area,
                                                           unsigned long long* count, long capacity) {
    const long nb = (long)bx.nz * bx.ny * bx.nx;
    const int lane = threadIdx.x & 63;
    for (long b0 = (long)blockIdx.x * NT; b0 < nb; b0 += (long)gridDim.x * NT) {
        const long i = b0 + threadIdx.x;
        uint8_t c = 0;
        if (i < nb) {
            const int x = (int)(i % bx.nx);
            const long t = i / bx.nx;
            const int y = (int)(t % bx.ny), z = (int)(t / bx.ny);
            c = codes[((long)(bx.z0 + z) * Hc + bx.y0 + y) * Wc + bx.x0 + x];
        }
        const bool on = is_border(c);
        const unsigned long long bal = __ballot(on);
        if (!bal) continue;
        unsigned long long pos = 0ull;
        if (lane == __ffsll((long long)bal) - 1) pos = atomicAdd(count, (unsigned long long)__popcll(bal));
        pos = __shfl(pos, __ffsll((long long)bal) - 1, 64) + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
        if (on && (long)pos < capacity) {
            dist[pos] = sq ? sqrt(sq[i]) : INFINITY;
            area[pos] = table[c];
        }
    }
}

int grid_for(long n) {
    const long b = (n + NT - 1) / NT;
    return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

bool launched() { return hipGetLastError() == hipSuccess; }

bool dims_ok(int D, int H, int W) { return D > 0 && H > 0 && W > 0 && (long)(D + 1) * (H + 1) * (W + 1) <= (1L << 31); }

bool box_ok(int Dc, int Hc, int Wc, const Box& b) {
    return Dc > 0 && Hc > 0 && Wc > 0 && (long)Dc * Hc * Wc <= (1L << 31) && b.z0 >= 0 && b.y0 >= 0 && b.x0 >= 0 && b.nz > 0 && b.ny > 0 && b.nx > 0 &&
           b.z0 + (long)b.nz <= Dc && b.y0 + (long)b.ny <= Hc && b.x0 + (long)b.nx <= Wc;
}

long aligned_elems(long n) { return (n + 31) & ~31L; }   // every workspace array starts on a 256-byte boundary

}  // namespace

extern "C" {

int rsuper_surface_codes(const uint8_t* gt, const uint8_t* pred, int planes, int D, int H, int W, uint8_t* codes_gt, uint8_t* codes_pred,
                         int* bbox, long long* counts, void* stream) {
    if (!gt || !pred || !codes_gt || !codes_pred || !bbox || !counts || planes < 1 || planes > 65535 || !dims_ok(D, H, W)) return RS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sc_init_kernel, dim3((planes * 6 + NT - 1) / NT), dim3(NT), 0, st, bbox, (unsigned long long*)counts, planes);
    const long nc = (long)(D + 1) * (H + 1) * (W + 1), per = (long)NT * SC_ITEMS;
    hipLaunchKernelGGL(surface_codes_kernel, dim3((unsigned)((nc + per - 1) / per), planes), dim3(NT), 0, st, gt, pred, D, H, W, codes_gt, codes_pred,
                       bbox, (unsigned long long*)counts);
    return launched() ? RS_OK : RS_ERR_LAUNCH;
}

long rsuper_edt3_workspace_bytes(int nz, int ny, int nx) {
    if (nz < 1 || ny < 1 || nx < 1 || nz > EDT_MAX_SIDE || ny > EDT_MAX_SIDE || nx > EDT_MAX_SIDE || (long)nz * ny * nx > (1L << 31)) return 0;
    const long n = aligned_elems((long)nz * ny * nx);
    return n * (8 + 8 + 4);
}

int rsuper_edt3(const uint8_t* codes, int Dc, int Hc, int Wc, int z0, int y0, int x0, int nz, int ny, int nx, double s0, double s1, double s2,
                double* out, void* workspace, long workspace_bytes, void* stream) {
    const Box bx{z0, y0, x0, nz, ny, nx};
    if (!codes || !out || !workspace || !box_ok(Dc, Hc, Wc, bx) || !(s0 > 0.0) || !(s1 > 0.0) || !(s2 > 0.0) || !(s0 < 1e6) || !(s1 < 1e6) || !(s2 < 1e6))
        return RS_ERR_ARG;
    const long need = rsuper_edt3_workspace_bytes(nz, ny, nx);
    if (need == 0) return RS_ERR_UNSUPPORTED;
    if (workspace_bytes < need) return RS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long n = aligned_elems((long)nz * ny * nx);
    double* wz = (double*)workspace;
    double* wf = wz + n;
    int* wv = (int*)(wf + n);
    const long wl = (long)nz * ny;
    hipLaunchKernelGGL(edt_w_kernel, dim3((unsigned)((wl + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, st, codes, Hc, Wc, bx, s2, out);
    if (ny > 1) {
        const long lines = (long)nz * nx;
        hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)((lines + NT - 1) / NT)), dim3(NT), 0, st, out, wz, wf, wv, lines, nx, (long)ny * nx, (long)nx,
                           ny, s1 * s1);
    }
    if (nz > 1) {
        const long lines = (long)ny * nx;
        hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)((lines + NT - 1) / NT)), dim3(NT), 0, st, out, wz, wf, wv, lines, nx, (long)nx, (long)ny * nx,
                           nz, s0 * s0);
    }
    return launched() ? RS_OK : RS_ERR_LAUNCH;
}

int rsuper_surfel_gather(const uint8_t* codes, int Dc, int Hc, int Wc, int z0, int y0, int x0, int nz, int ny, int nx, const double* sqdist,
                         const double* table, double* dist, double* area, long long* count, long capacity, void* stream) {
    const Box bx{z0, y0, x0, nz, ny, nx};
    if (!codes || !table || !dist || !area || !count || capacity < 1 || !box_ok(Dc, Hc, Wc, bx)) return RS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sg_init_kernel, dim3(1), dim3(1), 0, st, (unsigned long long*)count);
    hipLaunchKernelGGL(surfel_gather_kernel, dim3(grid_for((long)nz * ny * nx)), dim3(NT), 0, st, codes, Hc, Wc, bx, sqdist, table, dist, area,
                       (unsigned long long*)count, capacity);
    return launched() ? RS_OK : RS_ERR_LAUNCH;
}

}  // extern "C"
