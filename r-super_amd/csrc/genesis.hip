// Models Genesis pretext pairs (baselines/model_genesis/utils.py generate_one_pair :206-266 with data_augmentation :50, local_pixel_shuffling :76,
// nonlinear_transformation :61, image_in_painting :106, image_out_painting :125) on a batch of (B, D, H, W) f32 crops, and the voxel-wise MSE of the
// pre-training loss (losses_foundation.py model_genesis_loss :667).  The host draws a plan per sample (which transforms fired, the shuffled blocks, the
// Bezier curve as interpolation knots, the painted boxes); the device applies it.  The reference's (rows, cols, deps) are (D, H, W).
//
// Per sample, in the output frame (the frame after the flips):
//   v    = (img - min) / max(max - min, 1e-7f)                         f32, IEEE division
//   y    = flip(v)
//   orig = flip(v);  blocks k = 0 .. nb-1 in order: box_k.flat[i] = orig_box_k.flat[perm_k[i]]  (every block reads orig, never the partly shuffled image,
//          so a voxel carries what the LAST block covering it wrote and an uncovered voxel keeps orig)
//   x    = interp(x; xp, fp) in f64, rounded to f32 once               (np.interp's expression, multiply and add unfused)
//   x    = noise inside the boxes (in-painting) / outside their union (out-painting)
//   x, y = x * span + min, y * span + min                              f32, multiply and add unfused
//
// Launches per group of up to 8 samples (grid.y = sample; blocks of a sample that does not take part return at once):
//   (a) minmax     one (min, max) partial per block; fills the sample's owner map with -1 when it shuffles
//   (b) owner      one workgroup per shuffled block: atomicMax of the block index into the map -- an integer maximum does not depend on arrival order
//   (c) shuffle    one workgroup per shuffled block k: where map[voxel] == k it replaces k by -2 - (source voxel).  The source voxels are distinct from every
//                  block index and from -1, so another workgroup that reads the entry meanwhile sees "not mine" before and after.  Without explicit
//                  permutations the workgroup draws one Philox key per box voxel into LDS and ranks them: perm_k = stable argsort of the keys.
//   (d) pair       pointwise: normalise, flip, follow the map, curve, paint, map back; writes x and y
// = 4 launches when a sample of the group shuffles, 2 otherwise.  No atomics on floats, no memset: the same bits on every run.
//
// Philox4x32-10 keyed by the sample's 64-bit seed as in augment_intensity.hip; the third counter word names the stream: 0 is the Gaussian field there,
// 1 the painting noise (counter (i >> 2 low, i >> 2 high, 1, 0), voxel i of the output frame takes word i & 3, u = ((r >> 8) + 0.5) * 2^-24 rounded once
// to f32), 2 the shuffling keys (counter (i, k, 2, 0), word 0, for flat position i of block k).
//
// Float contraction is off in this file: numpy rounds a * b + c twice.  The arithmetic is written with plain operators, not with __fmul_rn / __fadd_rn /
// __dmul_rn / __dadd_rn: those are inline functions of the HIP headers, compiled in the headers' contraction mode, and after inlining the compiler fuses
// their product and sum into one fma.  Division is IEEE by default (v_div_scale / v_div_fmas / v_div_fixup).
#include "common.hpp"
#include "../../include/rsuper_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, MAXB = 8;
constexpr int PARTS_MAX = 128;                           // (min, max) partials per sample
constexpr long PART_VOX = (long)NT * 4 * 8;              // voxels a minmax block takes at least
constexpr int MAXBOX = RSUPER_GENESIS_MAX_BOXES, MAXSIDE = RSUPER_GENESIS_MAX_BLOCK_SIDE, MAXAXIS = RSUPER_GENESIS_MAX_AXIS;
constexpr int MAXN = MAXSIDE * MAXSIDE * MAXSIDE;        // voxels of a shuffled block
constexpr int VPT = 4;                                   // voxels per thread of the pair kernel
constexpr uint32_t STREAM_PAINT = 1, STREAM_PERM = 2;
constexpr int MSE_PARTS_MAX = 1024;
constexpr long MSE_PART_ELEMS = (long)NT * 4 * 4;
static_assert(MAXN * 8 <= 65536, "static LDS of the shuffle kernel");
static_assert((long)MAXAXIS * MAXAXIS * MAXAXIS < (1l << 31) - 2, "a source voxel fits the map's encoding");

enum { F_FLIP_D = 1, F_FLIP_H = 2, F_FLIP_W = 4, F_SHUFFLE = 8, F_CURVE = 16, F_INPAINT = 32, F_OUTPAINT = 64, F_ALL = 127 };

struct Sample {
    int flags, nbox;
    uint32_t k0, k1;
    int box[MAXBOX][6];                                  // z0, y0, x0, nz, ny, nx
};

struct Args {
    const float* img;
    float* x;
    float* y;
    const float* noise;                                  // optional explicit U[0, 1) field, output frame
    float* part;                                         // [MAXB][PARTS_MAX][2]
    int* map;                                            // [B][V]: -1 = nobody, k >= 0 = owner block (between (b) and (c)), <= -2: -2 - source voxel
    const int* blocks;                                   // [B][nb][6]: z0, y0, x0, nz, ny, nx
    const int* perm;                                     // optional: source position per box position, concatenated
    const long long* perm_off;                           // [B][nb]
    long long perm_len;
    const double* curve;                                 // [B][2][n]: xp, fp
    int n, nb;
    int D, H, W, parts;
    long V, per;                                         // voxels per sample, per minmax block (multiple of 4)
    Sample s[MAXB];
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
__device__ __forceinline__ float unit(uint32_t r) { return fmaf((float)(r >> 8), 0x1p-24f, 0x1p-25f); }

// ---- (a) one (min, max) partial per block; the owner map of a shuffling sample starts at -1
__global__ __launch_bounds__(NT) void genesis_minmax_kernel(Args a) {
    __shared__ float shw[NT / 64][2];
    const int b = blockIdx.y;
    const float* __restrict__ x = a.img + (long)b * a.V;
    const long n0 = (long)blockIdx.x * a.per, n1 = n0 + a.per < a.V ? n0 + a.per : a.V;
    float lo = INFINITY, hi = -INFINITY;
    for (long i = n0 + threadIdx.x; i < n1; i += NT) {
        const float v = x[i];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
    }
    if (a.s[b].flags & F_SHUFFLE) {
        int* __restrict__ m = a.map + (long)b * a.V;
        for (long i = n0 + threadIdx.x; i < n1; i += NT) m[i] = -1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { shw[threadIdx.x >> 6][0] = lo; shw[threadIdx.x >> 6][1] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) { lo = fminf(lo, shw[w][0]); hi = fmaxf(hi, shw[w][1]); }
        float* p = a.part + ((long)b * PARTS_MAX + blockIdx.x) * 2;
        p[0] = lo; p[1] = hi;
    }
}

struct Block {
    int z0, y0, x0, nz, ny, nx, n;
};
// the record of block k of sample b; false (for the whole workgroup) when it does not lie inside the volume or a side is outside 1 .. MAXSIDE
__device__ __forceinline__ bool load_block(const Args& a, int b, int k, Block& q) {
    const int* r = a.blocks + ((long)b * a.nb + k) * 6;
    q.z0 = r[0]; q.y0 = r[1]; q.x0 = r[2]; q.nz = r[3]; q.ny = r[4]; q.nx = r[5];
    if (q.nz < 1 || q.ny < 1 || q.nx < 1 || q.nz > MAXSIDE || q.ny > MAXSIDE || q.nx > MAXSIDE) return false;
    if (q.z0 < 0 || q.y0 < 0 || q.x0 < 0 || q.z0 > a.D - q.nz || q.y0 > a.H - q.ny || q.x0 > a.W - q.nx) return false;
    q.n = q.nz * q.ny * q.nx;
    return true;
}
// flat (row-major) position i of the box -> voxel of the sample
__device__ __forceinline__ int box_voxel(const Args& a, const Block& q, int i) {
    const int ix = i % q.nx, t = i / q.nx, iy = t % q.ny, iz = t / q.ny;
    return ((q.z0 + iz) * a.H + q.y0 + iy) * a.W + q.x0 + ix;
}

// ---- (b) the highest block index that covers each voxel
__global__ __launch_bounds__(NT) void genesis_owner_kernel(Args a) {
    const int b = blockIdx.y, k = blockIdx.x;
    if (!(a.s[b].flags & F_SHUFFLE)) return;
    Block q;
    if (!load_block(a, b, k, q)) return;
    int* m = a.map + (long)b * a.V;
    for (int i = threadIdx.x; i < q.n; i += NT) atomicMax(m + box_voxel(a, q, i), k);
}

// ---- (c) block k writes the source voxel of every voxel it owns
__global__ __launch_bounds__(NT) void genesis_shuffle_kernel(Args a) {
    __shared__ unsigned long long keys[MAXN];
    const int b = blockIdx.y, k = blockIdx.x;
    const Sample& s = a.s[b];
    if (!(s.flags & F_SHUFFLE)) return;
    Block q;
    if (!load_block(a, b, k, q)) return;
    int* m = a.map + (long)b * a.V;
    int mine = 0;
    for (int i = threadIdx.x; i < q.n; i += NT) mine |= m[box_voxel(a, q, i)] == k;
    if (!__syncthreads_or(mine)) return;                 // every voxel of the box belongs to a later block
    if (a.perm) {
        const long long off = a.perm_off[(long)b * a.nb + k];
        if (off < 0 || off + q.n > a.perm_len) return;
        for (int i = threadIdx.x; i < q.n; i += NT) {
            const int dst = box_voxel(a, q, i);
            if (m[dst] != k) continue;
            int p = a.perm[off + i];
            if ((unsigned)p >= (unsigned)q.n) p = i;     // not a position of the box: the voxel stays
            m[dst] = -2 - box_voxel(a, q, p);
        }
        return;
    }
    for (int i = threadIdx.x; i < q.n; i += NT) {
        uint32_t r[4];
        philox4x32_10((uint32_t)i, (uint32_t)k, STREAM_PERM, 0u, s.k0, s.k1, r);
        keys[i] = ((unsigned long long)r[0] << 32) | (unsigned)i;      // ties fall to the lower position: a stable sort
    }
    __syncthreads();
    for (int i = threadIdx.x; i < q.n; i += NT) {
        const unsigned long long ki = keys[i];
        int rank = 0;
        for (int j = 0; j < q.n; ++j) rank += keys[j] < ki;            // every lane reads the same word: an LDS broadcast
        const int dst = box_voxel(a, q, rank);                         // perm[rank] = i
        if (m[dst] == k) m[dst] = -2 - box_voxel(a, q, i);
    }
}

// np.interp(x, xp, fp) for one x: j = the last knot with xp[j] <= x
__device__ __forceinline__ double interp(const double* __restrict__ xp, const double* __restrict__ fp, int n, double x) {
    if (x <= xp[0]) return fp[0];
    int lo = 0, hi = n;                                  // xp[lo] <= x; hi = n or xp[hi] > x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    if (lo == n - 1) return fp[n - 1];
    const double x0 = xp[lo], f0 = fp[lo];
    if (x == x0) return f0;
    const double slope = (fp[lo + 1] - f0) / (xp[lo + 1] - x0);
    const double rise = slope * (x - x0);
    return rise + f0;
}

// ---- (d) the pair
__global__ __launch_bounds__(NT) void genesis_pair_kernel(Args a) {
    __shared__ float sh[2];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Sample& s = a.s[b];
    if (tid < 64) {
        const float* p = a.part + (long)b * PARTS_MAX * 2;
        float lo = INFINITY, hi = -INFINITY;
        for (int i = tid; i < a.parts; i += 64) { lo = fminf(lo, p[2 * i]); hi = fmaxf(hi, p[2 * i + 1]); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if (tid == 0) { sh[0] = lo; sh[1] = hi; }
    }
    __syncthreads();
    const float minv = sh[0], span = fmaxf(sh[1] - sh[0], 1e-7f);
    const int D = a.D, H = a.H, W = a.W, flags = s.flags;
    const float* __restrict__ src = a.img + (long)b * a.V;
    const int* __restrict__ m = a.map + (long)b * a.V;
    const double* __restrict__ xp = a.curve + (long)b * 2 * a.n;
    const double* __restrict__ fp = xp + a.n;
    auto value = [&](int z, int y, int x) {              // the normalised voxel of the flipped image
        if (flags & F_FLIP_D) z = D - 1 - z;
        if (flags & F_FLIP_H) y = H - 1 - y;
        if (flags & F_FLIP_W) x = W - 1 - x;
        return (src[((long)z * H + y) * W + x] - minv) / span;
    };
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const long i = ((long)blockIdx.x * VPT + u) * NT + tid;
        if (i >= a.V) break;
        const int x = (int)(i % W), t = (int)(i / W), y = t % H, z = t / H;
        const float yv = value(z, y, x);
        float xv = yv;
        if (flags & F_SHUFFLE) {
            const int e = m[i];
            if (e <= -2) {
                const int j = -2 - e;
                if (j != (int)i && j < a.V) {
                    const int t2 = j / W;
                    xv = value(t2 / H, t2 % H, j % W);
                }
            }
        }
        if (flags & F_CURVE) xv = (float)interp(xp, fp, a.n, (double)xv);
        if (flags & (F_INPAINT | F_OUTPAINT)) {
            bool inside = false;
            for (int q = 0; q < s.nbox; ++q) {
                const int* bx = s.box[q];
                inside |= (unsigned)(z - bx[0]) < (unsigned)bx[3] && (unsigned)(y - bx[1]) < (unsigned)bx[4] && (unsigned)(x - bx[2]) < (unsigned)bx[5];
            }
            if (inside == ((flags & F_INPAINT) != 0)) {
                if (a.noise) xv = a.noise[(long)b * a.V + i];
                else {
                    uint32_t r[4];
                    const unsigned long q4 = (unsigned long)i >> 2;
                    philox4x32_10((uint32_t)q4, (uint32_t)(q4 >> 32), STREAM_PAINT, 0u, s.k0, s.k1, r);
                    xv = unit(r[i & 3]);
                }
            }
        }
        const float xs = xv * span, ys = yv * span;
        a.x[(long)b * a.V + i] = xs + minv;
        a.y[(long)b * a.V + i] = ys + minv;
    }
}

int minmax_parts(long V) {
    const long p = (V + PART_VOX - 1) / PART_VOX;
    return (int)(p < 1 ? 1 : p > PARTS_MAX ? PARTS_MAX : p);
}

// ---- MSE
int mse_parts(long n) {
    const long p = (n + MSE_PART_ELEMS - 1) / MSE_PART_ELEMS;
    return (int)(p < 1 ? 1 : p > MSE_PARTS_MAX ? MSE_PARTS_MAX : p);
}

// the sum of a block's per-thread doubles in a fixed order -> thread 0
__device__ __forceinline__ double block_sum(double v, double* shw) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < NT / 64; ++w) v += shw[w];
    return v;
}

// one f32 partial per block: the f64 sum of the exact squared differences of its run, rounded once
__global__ __launch_bounds__(NT) void mse_partial_kernel(const float* __restrict__ r, const float* __restrict__ y, long n, long per, int vec, float* __restrict__ part) {
    __shared__ double shw[NT / 64];
    const long n0 = (long)blockIdx.x * per, n1 = n0 + per < n ? n0 + per : n;
    double acc = 0.0;
    for (long i = n0 + 4 * (long)threadIdx.x; i < n1; i += 4 * NT) {
        if (vec && i + 4 <= n1) {
            const float4 p = *reinterpret_cast<const float4*>(r + i), q = *reinterpret_cast<const float4*>(y + i);
            const double d0 = (double)p.x - (double)q.x, d1 = (double)p.y - (double)q.y, d2 = (double)p.z - (double)q.z, d3 = (double)p.w - (double)q.w;
            acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
        } else {
            for (int j = 0; j < 4 && i + j < n1; ++j) {
                const double d = (double)r[i + j] - (double)y[i + j];
                acc += d * d;
            }
        }
    }
    acc = block_sum(acc, shw);
    if (threadIdx.x == 0) part[blockIdx.x] = (float)acc;
}

__global__ __launch_bounds__(NT) void mse_final_kernel(const float* __restrict__ part, int parts, long n, float* __restrict__ out) {
    __shared__ double shw[NT / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < parts; i += NT) acc += (double)part[i];
    acc = block_sum(acc, shw);
    if (threadIdx.x == 0) out[0] = (float)(acc / (double)n);
}

__global__ __launch_bounds__(NT) void mse_bwd_kernel(const float* __restrict__ r, const float* __restrict__ y, const float* __restrict__ g, long n, float* __restrict__ dr) {
    const double c = (double)g[0] * 2.0 / (double)n;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) dr[i] = (float)(c * ((double)r[i] - (double)y[i]));
}

}  // namespace

extern "C" {

long rsuper_genesis_workspace_bytes(int B, int D, int H, int W, int nb) {
    if (B < 1 || D < 1 || H < 1 || W < 1 || nb < 0) return 0;
    return (long)MAXB * PARTS_MAX * 2 * (long)sizeof(float) + (nb > 0 ? (long)B * D * H * W * (long)sizeof(int) : 0l);
}

int rsuper_genesis_launches(int B, const int* flags) {
    if (B < 1 || !flags) return 0;
    int n = 0;
    for (int b0 = 0; b0 < B; b0 += MAXB) {
        int any = 0;
        for (int b = b0; b < B && b < b0 + MAXB; ++b) any |= flags[b];
        n += (any & F_SHUFFLE) ? 4 : 2;
    }
    return n;
}

int rsuper_genesis_pair(const float* img, float* x, float* y, int B, int D, int H, int W, const int* flags, int nb, const int* blocks, const int* perm,
                        const long long* perm_off, long long perm_len, const double* curve, int n, const int* nbox, const int* boxes,
                        const unsigned long long* seeds, const float* noise, void* workspace, long workspace_bytes, void* stream) {
    if (!img || !x || !y || img == x || img == y || x == y || !flags || !seeds || B < 1 || D < 1 || H < 1 || W < 1 || nb < 0) return RS_ERR_ARG;
    if (D > MAXAXIS || H > MAXAXIS || W > MAXAXIS) return RS_ERR_ARG;
    int any = 0;
    for (int b = 0; b < B; ++b) {
        const int f = flags[b];
        if (f < 0 || f > F_ALL || ((f & F_INPAINT) && (f & F_OUTPAINT))) return RS_ERR_ARG;
        if (f & (F_INPAINT | F_OUTPAINT)) {
            if (!nbox || !boxes || nbox[b] < 0 || nbox[b] > MAXBOX) return RS_ERR_ARG;
            for (int q = 0; q < nbox[b]; ++q) {
                const int* bx = boxes + ((long)b * MAXBOX + q) * 6;
                if (bx[3] < 1 || bx[4] < 1 || bx[5] < 1 || bx[0] < 0 || bx[1] < 0 || bx[2] < 0 || bx[0] > D - bx[3] || bx[1] > H - bx[4] || bx[2] > W - bx[5])
                    return RS_ERR_ARG;
            }
        }
        any |= f;
    }
    if ((any & F_SHUFFLE) && (nb < 1 || !blocks || (perm && (!perm_off || perm_len < 0)))) return RS_ERR_ARG;
    if ((any & F_CURVE) && (!curve || n < 2 || (uintptr_t)curve % 8)) return RS_ERR_ARG;
    const long V = (long)D * H * W;
    const bool shuffles = (any & F_SHUFFLE) != 0;
    if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < rsuper_genesis_workspace_bytes(B, D, H, W, shuffles ? nb : 0)) return RS_ERR_ARG;

    Args a{};
    a.D = D; a.H = H; a.W = W; a.V = V;
    a.n = n; a.nb = nb;
    a.part = (float*)workspace;
    a.parts = minmax_parts(V);
    a.per = ((V + a.parts - 1) / a.parts + 3) & ~3l;
    a.perm = shuffles ? perm : nullptr;
    a.perm_len = perm_len;
    for (int b0 = 0; b0 < B; b0 += MAXB) {               // the per-sample records travel in the kernel arguments, MAXB samples per launch
        const int g = B - b0 < MAXB ? B - b0 : MAXB;
        int grp = 0;
        for (int b = 0; b < g; ++b) {
            Sample& s = a.s[b];
            s = Sample{};
            s.flags = flags[b0 + b];
            s.k0 = (uint32_t)seeds[b0 + b]; s.k1 = (uint32_t)(seeds[b0 + b] >> 32);
            if (s.flags & (F_INPAINT | F_OUTPAINT)) {
                s.nbox = nbox[b0 + b];
                for (int q = 0; q < s.nbox; ++q)
                    for (int j = 0; j < 6; ++j) s.box[q][j] = boxes[((long)(b0 + b) * MAXBOX + q) * 6 + j];
            }
            grp |= s.flags;
        }
        a.img = img + (long)b0 * V;
        a.x = x + (long)b0 * V;
        a.y = y + (long)b0 * V;
        a.noise = noise ? noise + (long)b0 * V : nullptr;
        a.map = shuffles ? (int*)((char*)workspace + (long)MAXB * PARTS_MAX * 2 * sizeof(float)) + (long)b0 * V : nullptr;
        a.blocks = blocks ? blocks + (long)b0 * nb * 6 : nullptr;
        a.perm_off = perm_off ? perm_off + (long)b0 * nb : nullptr;
        a.curve = curve ? curve + (long)b0 * 2 * n : nullptr;
        hipLaunchKernelGGL(genesis_minmax_kernel, dim3(a.parts, g), dim3(NT), 0, (hipStream_t)stream, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
        if (grp & F_SHUFFLE) {
            hipLaunchKernelGGL(genesis_owner_kernel, dim3(nb, g), dim3(NT), 0, (hipStream_t)stream, a);
            if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
            hipLaunchKernelGGL(genesis_shuffle_kernel, dim3(nb, g), dim3(NT), 0, (hipStream_t)stream, a);
            if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(genesis_pair_kernel, dim3((unsigned)((V + (long)NT * VPT - 1) / ((long)NT * VPT)), g), dim3(NT), 0, (hipStream_t)stream, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

long rsuper_mse_workspace_bytes(long n) { return n < 1 ? 0 : (long)MSE_PARTS_MAX * (long)sizeof(float); }

int rsuper_mse_fwd(const float* r, const float* y, long n, float* out, void* workspace, long workspace_bytes, void* stream) {
    if (!r || !y || !out || n < 1 || !workspace || (uintptr_t)workspace % 4 || workspace_bytes < rsuper_mse_workspace_bytes(n)) return RS_ERR_ARG;
    const int parts = mse_parts(n);
    const long per = ((n + parts - 1) / parts + 3) & ~3l;
    const int vec = (uintptr_t)r % 16 == 0 && (uintptr_t)y % 16 == 0;
    hipLaunchKernelGGL(mse_partial_kernel, dim3(parts), dim3(NT), 0, (hipStream_t)stream, r, y, n, per, vec, (float*)workspace);
    if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float*)workspace, parts, n, out);
    return rs_check_launch();
}

int rsuper_mse_bwd(const float* r, const float* y, const float* g, long n, float* dr, void* stream) {
    if (!r || !y || !g || !dr || n < 1) return RS_ERR_ARG;
    const long blocks = (n + NT - 1) / NT;
    hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(NT), 0, (hipStream_t)stream, r, y, g, n, dr);
    return rs_check_launch();
}

}  // extern "C"
