// Whole-CT preprocessing and spacing resampling of predictions (predict_abdomenatlas.py preprocess :325-356 from the clip onward, pad_to_training_size
// :249-306, unpad_img :311-322, resample_image_with_gpu :718-742).
//
// ct_stats / ct_normalize: z-score of clip(x, lo, hi) with the whole-volume mean and unbiased standard deviation, written into a zero-padded output.
//   launch 1  PARTS blocks; block b reduces its run of the volume in f64 and writes ONE partial (count, sum, sum of squares) into the caller's
//             workspace.  Every block writes, an empty run writes zeros: the workspace needs no memset.
//   launch 2  every block re-reduces the PARTS partials in the same fixed order, forms mean = S / N and std = sqrt((Q - N mean^2) / (N - 1)) in f64
//             (rsuper_ct_normalize_pop: / N, the np.std of dataset_conversion/nii2npz.py :72),
//             rounds each to f32 and writes (clip(x) - mean) / std (true division) inside the source box, 0 outside.
//   No atomics, no host synchronisation between the two, the same bits on every run.  Squares of f32 values are exact in f64; with |clip(x)| <= 991 and
//   N <= 3e8 the sum of squares stays below 2^49, and Q - N mean^2 loses fewer than 20 of the 53 bits.  Nothing is special-cased: a
//   constant volume gives 0 / 0 = NaN inside the box (the padding stays 0), N = 1 gives NaN.
//   The volume is read flat in 16-byte vectors (8 int16 / 4 f32) from the first 16-byte boundary on; the output is written flat in 16-byte vectors of
//   4 f32 from ITS first 16-byte boundary on; block 0 takes the scalar heads and tails.  A vector whose 4 voxels sit in one source row takes them in
//   one load (an unaligned one where the padding shifts the row), otherwise voxel by voxel.
//
// resample3d: one launch for a (C, Dp, Hp, Wp) stack; the source is the sub-box (z0, y0, x0) + (D, H, W) of every plane (the fused unpad_img).
//   nearest    scale = (float)n_in / (float)n_out;  src = min((int)floorf((float)dst * scale), n_in - 1)                    (upsample_nearest3d)
//   trilinear  scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0;  s = scale * (float)dst;  i0 = min((int)s, n_in - 1);
//              i1 = i0 + (i0 < n_in - 1);  l1 = s - (float)i0;  l0 = 1 - l1                                                  (align_corners = True)
//   all in f32.  A lane produces 4 consecutive x outputs (one 16-byte f32 or 4-byte u8 store when the row pitch allows) and keeps their x indices and
//   weights in registers while it walks the rows of the block's 4 (z) x 8 (y) tile of output rows; the y and z index and weight are computed once
//   per row.  The three lerps run x, y, z as l0 * a + l1 * b with float contraction off.  trilinear: the block first lerps every source row its tile
//   touches along x into LDS (one pass of two gathered loads per staged value; the rows of a tile share their source planes and rows), then each
//   lane reads its four x-lerped neighbours back as 16-byte LDS vectors.  A tile whose source rows exceed the 48 KiB LDS tile (strong
//   downsampling) and nearest read global memory directly; the tile's rows then share their source rows through L2.
#include "common.hpp"
#include "../../include/rsuper_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int PARTS = 512;                               // partials of a volume: fixed, so launch 2 needs no count from launch 1
constexpr int SNT = 512;                                 // threads of a stats block
constexpr int NT = 256;
constexpr int NITER = 16;                                // 16-byte output vectors a lane of the normalise kernel writes
constexpr int TY = 8, TZ = 4;                            // output rows of a resample block
constexpr int LDS_FLOATS = 12288;                        // x-lerped source rows of a trilinear tile: 48 rows of 256 (a 2 : 1 upsampling needs 5 x 9)

template <typename T> struct Src;
template <> struct Src<short> { static constexpr int VEC = 8; };
template <> struct Src<float> { static constexpr int VEC = 4; };

__device__ __forceinline__ float clipf(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }   // the clip keeps a NaN

__device__ __forceinline__ void unpack(const uint4& q, const short*, float* f) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[2 * j] = (float)(short)(w[j] & 0xffffu); f[2 * j + 1] = (float)(short)(w[j] >> 16); }
}
__device__ __forceinline__ void unpack(const uint4& q, const float*, float* f) {
    f[0] = __uint_as_float(q.x); f[1] = __uint_as_float(q.y); f[2] = __uint_as_float(q.z); f[3] = __uint_as_float(q.w);
}

struct StatArgs {
    const void* x;
    double* ws;                                          // [3][PARTS]: count, sum, sum of squares
    unsigned N, head, nvec, vper;                        // voxels; scalar voxels before the first 16-byte boundary; vectors; vectors per block
    float lo, hi;
};

template <typename T>
__global__ __launch_bounds__(SNT) void ct_stats_kernel(StatArgs a) {
    constexpr int VEC = Src<T>::VEC;
    __shared__ double shw[SNT / 64][3];
    const T* __restrict__ x = (const T*)a.x;
    const int tid = threadIdx.x;
    double cnt = 0.0, sum = 0.0, sq = 0.0;
    auto take = [&](float v) {
        v = clipf(v, a.lo, a.hi);
        cnt += 1.0; sum += (double)v; sq += (double)v * (double)v;
    };
    const unsigned v0 = blockIdx.x * a.vper, v1 = v0 + a.vper < a.nvec ? v0 + a.vper : a.nvec;
    const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x + a.head);
#pragma unroll 4
    for (unsigned i = v0 + tid; i < v1; i += SNT) {
        float f[VEC];
        unpack(xv[i], (const T*)nullptr, f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) take(f[j]);
    }
    if (blockIdx.x == 0) {                               // head and tail: fewer than 2 * VEC voxels
        const unsigned tail0 = a.head + a.nvec * VEC;
        if ((unsigned)tid < a.head) take((float)x[tid]);
        if (tail0 + tid < a.N) take((float)x[tail0 + tid]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); sum += __shfl_xor(sum, o, 64); sq += __shfl_xor(sq, o, 64); }
    if ((tid & 63) == 0) { shw[tid >> 6][0] = cnt; shw[tid >> 6][1] = sum; shw[tid >> 6][2] = sq; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SNT / 64; ++w) { cnt += shw[w][0]; sum += shw[w][1]; sq += shw[w][2]; }
        a.ws[blockIdx.x] = cnt; a.ws[PARTS + blockIdx.x] = sum; a.ws[2 * PARTS + blockIdx.x] = sq;
    }
}

struct NormArgs {
    const void* x;
    float* out;
    const double* ws;
    float* ms;                                           // (mean, std) for the caller
    int D, H, W, Do, Ho, Wo, z_lo, y_lo, x_lo;
    unsigned No, head, ngrp;                             // output voxels; scalar voxels before the first 16-byte boundary; 16-byte vectors
    float lo, hi;
    int pop;                                             // divide the squared deviations by N (np.std, ddof = 0) instead of N - 1
};

// NORM: z-score with the statistics of the workspace; otherwise the box is copied as it is (pad_to_training_size on its own)
template <typename T, bool NORM>
__global__ __launch_bounds__(NT) void ct_normalize_kernel(NormArgs a) {
    __shared__ double shw[NT / 64][3];
    const int tid = threadIdx.x;
    const T* __restrict__ x = (const T*)a.x;
    float mean = 0.f, sd = 1.f;
    if (NORM) {
        double cnt = 0.0, sum = 0.0, sq = 0.0;
        for (int i = tid; i < PARTS; i += NT) { cnt += a.ws[i]; sum += a.ws[PARTS + i]; sq += a.ws[2 * PARTS + i]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); sum += __shfl_xor(sum, o, 64); sq += __shfl_xor(sq, o, 64); }
        if ((tid & 63) == 0) { shw[tid >> 6][0] = cnt; shw[tid >> 6][1] = sum; shw[tid >> 6][2] = sq; }
        __syncthreads();
        cnt = shw[0][0]; sum = shw[0][1]; sq = shw[0][2];
        for (int w = 1; w < NT / 64; ++w) { cnt += shw[w][0]; sum += shw[w][1]; sq += shw[w][2]; }
        const double m = sum / cnt;
        const double var = (sq - cnt * m * m) / (a.pop ? cnt : cnt - 1.0);   // unbiased unless pop; 0 / 0 and a negative rounding residue stay what they are
        mean = (float)m; sd = (float)sqrt(var);
        if (blockIdx.x == 0 && tid == 0) { a.ms[0] = mean; a.ms[1] = sd; }
    }
    auto score = [&](float v) { return NORM ? (clipf(v, a.lo, a.hi) - mean) / sd : v; };
    auto voxel = [&](int z, int y, int xx) {             // output voxel (z, y, xx)
        const int sz = z - a.z_lo, sy = y - a.y_lo, sx = xx - a.x_lo;
        if ((unsigned)sz >= (unsigned)a.D || (unsigned)sy >= (unsigned)a.H || (unsigned)sx >= (unsigned)a.W) return 0.f;
        return score((float)x[((unsigned)sz * a.H + sy) * a.W + sx]);
    };
    auto flat = [&](unsigned i) {
        const unsigned r = i / a.Wo;
        return voxel((int)(r / a.Ho), (int)(r % a.Ho), (int)(i % a.Wo));
    };
    const unsigned g0 = blockIdx.x * (unsigned)(NT * NITER);
#pragma unroll 2
    for (int it = 0; it < NITER; ++it) {
        const unsigned g = g0 + it * NT + tid;
        if (g >= a.ngrp) break;
        const unsigned i = a.head + 4 * g, r = i / a.Wo;
        int xx = (int)(i % a.Wo), y = (int)(r % a.Ho), z = (int)(r / a.Ho);
        const int sz = z - a.z_lo, sy = y - a.y_lo, sx = xx - a.x_lo;
        float v[4];
        if (xx + 3 < a.Wo && (unsigned)sz < (unsigned)a.D && (unsigned)sy < (unsigned)a.H && sx >= 0 && sx + 3 < a.W) {
            T raw[4];
            __builtin_memcpy(raw, x + ((unsigned)sz * a.H + sy) * a.W + sx, sizeof(raw));   // one load; the padding may leave it unaligned
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = score((float)raw[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = voxel(z, y, xx);
                if (++xx == a.Wo) { xx = 0; if (++y == a.Ho) { y = 0; ++z; } }
            }
        }
        *reinterpret_cast<float4*>(a.out + i) = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (blockIdx.x == 0) {                               // head and tail: fewer than 4 voxels each
        const unsigned tail0 = a.head + 4 * a.ngrp;
        if ((unsigned)tid < a.head) a.out[tid] = flat(tid);
        if (tail0 + tid < a.No) a.out[tail0 + tid] = flat(tail0 + tid);
    }
}

struct RsArgs {
    const void* src;
    void* out;
    int Dp, Hp, Wp, z0, y0, x0, D, H, W, Do, Ho, Wo;
    int nbx, nby, lx, vec, use_thr;                      // lx: lanes per output row of the tile (a power of two <= 64)
    float thr, sz, sy, sx;                               // the per-axis scales, formed on the host in f32
};

template <int MODE> struct Axis { int i0, i1; float l0, l1; };

template <int MODE>
__device__ __forceinline__ Axis<MODE> axis(int dst, int n_in, float scale) {
    Axis<MODE> r;
    if (MODE == RSUPER_RESAMPLE_NEAREST) {
        const int i = (int)floorf((float)dst * scale);
        r.i0 = r.i1 = i < n_in - 1 ? i : n_in - 1;
        r.l0 = 1.f; r.l1 = 0.f;
    } else {
        const float s = scale * (float)dst;
        const int i = (int)s;
        r.i0 = i < n_in - 1 ? i : n_in - 1;
        r.i1 = r.i0 + (r.i0 < n_in - 1);
        r.l1 = s - (float)r.i0;
        r.l0 = 1.f - r.l1;
    }
    return r;
}

template <typename TO>
__device__ __forceinline__ void store4(const RsArgs& a, TO* __restrict__ q, int ox, const float* v) {
    TO o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = a.use_thr ? (TO)(v[j] > a.thr) : (TO)v[j];
    if (a.vec) {
        if (sizeof(TO) == 4) *reinterpret_cast<float4*>(q) = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
        else *reinterpret_cast<uint32_t*>(q) = (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16 | (uint32_t)o[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ox + j < a.Wo) q[j] = o[j];
    }
}

template <typename TI, typename TO, int MODE>
__global__ __launch_bounds__(NT) void resample3d_kernel(RsArgs a) {
    const int tid = threadIdx.x, xg = tid & (a.lx - 1), rs = tid / a.lx, rp = NT / a.lx;
    const int bx = blockIdx.x % a.nbx, t0 = blockIdx.x / a.nbx, by = t0 % a.nby, bz = t0 / a.nby;
    const int ox = (bx * a.lx + xg) * 4;
    const TI* __restrict__ src = (const TI*)a.src + (size_t)blockIdx.y * a.Dp * a.Hp * a.Wp;
    TO* __restrict__ out = (TO*)a.out + (size_t)blockIdx.y * a.Do * a.Ho * a.Wo;

    if (MODE == RSUPER_RESAMPLE_TRILINEAR) {
        // The source rows the tile touches, lerped along x once into LDS: T[row][tile x].  A row serves every output row of the tile that lies next to
        // it in y or z, so an output voxel costs (rows / output rows) * 2 global loads instead of 8, and its four x-lerped neighbours are read back as
        // 16-byte LDS vectors.  The same three lerps in the same order as the direct path below: the same bits.
        __shared__ __attribute__((aligned(16))) float T[LDS_FLOATS];
        const int XT = a.lx * 4;
        const int oz_b = (bz * TZ + TZ < a.Do ? bz * TZ + TZ : a.Do) - 1, oy_b = (by * TY + TY < a.Ho ? by * TY + TY : a.Ho) - 1;
        const int zlo = axis<MODE>(bz * TZ, a.D, a.sz).i0, ylo = axis<MODE>(by * TY, a.H, a.sy).i0;
        const int nz = axis<MODE>(oz_b, a.D, a.sz).i1 - zlo + 1, ny = axis<MODE>(oy_b, a.H, a.sy).i1 - ylo + 1;
        if ((long)nz * ny * XT <= LDS_FLOATS) {          // the same answer in every lane of the block
            const int xq = tid & (XT - 1), sxo = bx * XT + xq;
            const Axis<MODE> aq = axis<MODE>(sxo < a.Wo ? sxo : a.Wo - 1, a.W, a.sx);
            for (int row = tid / XT; row < nz * ny; row += NT / XT) {
                const TI* __restrict__ p = src + ((a.z0 + zlo + row / ny) * a.Hp + (a.y0 + ylo + row % ny)) * a.Wp + a.x0;
                T[row * XT + xq] = aq.l0 * (float)p[aq.i0] + aq.l1 * (float)p[aq.i1];
            }
            __syncthreads();
            if (ox >= a.Wo) return;
            for (int r = rs; r < TY * TZ; r += rp) {
                const int oy = by * TY + r % TY, oz = bz * TZ + r / TY;
                if (oy >= a.Ho || oz >= a.Do) continue;
                const Axis<MODE> ay = axis<MODE>(oy, a.H, a.sy), az = axis<MODE>(oz, a.D, a.sz);
                const float* t = T + 4 * xg;
                const float4 a00 = *reinterpret_cast<const float4*>(t + ((az.i0 - zlo) * ny + (ay.i0 - ylo)) * XT);
                const float4 a01 = *reinterpret_cast<const float4*>(t + ((az.i0 - zlo) * ny + (ay.i1 - ylo)) * XT);
                const float4 a10 = *reinterpret_cast<const float4*>(t + ((az.i1 - zlo) * ny + (ay.i0 - ylo)) * XT);
                const float4 a11 = *reinterpret_cast<const float4*>(t + ((az.i1 - zlo) * ny + (ay.i1 - ylo)) * XT);
                const float c00[4] = {a00.x, a00.y, a00.z, a00.w}, c01[4] = {a01.x, a01.y, a01.z, a01.w};
                const float c10[4] = {a10.x, a10.y, a10.z, a10.w}, c11[4] = {a11.x, a11.y, a11.z, a11.w};
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float b0 = ay.l0 * c00[j] + ay.l1 * c01[j], b1 = ay.l0 * c10[j] + ay.l1 * c11[j];
                    v[j] = az.l0 * b0 + az.l1 * b1;
                }
                store4<TO>(a, out + ((unsigned)oz * a.Ho + oy) * a.Wo + ox, ox, v);
            }
            return;
        }
    }

    // direct path: nearest, and a trilinear tile whose source rows do not fit the LDS tile (strong downsampling)
    if (ox >= a.Wo) return;
    Axis<MODE> ax[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ax[j] = axis<MODE>(ox + j < a.Wo ? ox + j : a.Wo - 1, a.W, a.sx);        // a lane past the row's end repeats the last voxel and stores nothing
        ax[j].i0 += a.x0; ax[j].i1 += a.x0;
    }
    for (int r = rs; r < TY * TZ; r += rp) {
        const int oy = by * TY + r % TY, oz = bz * TZ + r / TY;
        if (oy >= a.Ho || oz >= a.Do) continue;
        const Axis<MODE> ay = axis<MODE>(oy, a.H, a.sy), az = axis<MODE>(oz, a.D, a.sz);
        float v[4];
        if (MODE == RSUPER_RESAMPLE_NEAREST) {
            const TI* __restrict__ p = src + ((a.z0 + az.i0) * a.Hp + (a.y0 + ay.i0)) * a.Wp;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (float)p[ax[j].i0];
        } else {
            const TI* __restrict__ p00 = src + ((a.z0 + az.i0) * a.Hp + (a.y0 + ay.i0)) * a.Wp;
            const TI* __restrict__ p01 = src + ((a.z0 + az.i0) * a.Hp + (a.y0 + ay.i1)) * a.Wp;
            const TI* __restrict__ p10 = src + ((a.z0 + az.i1) * a.Hp + (a.y0 + ay.i0)) * a.Wp;
            const TI* __restrict__ p11 = src + ((a.z0 + az.i1) * a.Hp + (a.y0 + ay.i1)) * a.Wp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a00 = ax[j].l0 * (float)p00[ax[j].i0] + ax[j].l1 * (float)p00[ax[j].i1];
                const float a01 = ax[j].l0 * (float)p01[ax[j].i0] + ax[j].l1 * (float)p01[ax[j].i1];
                const float a10 = ax[j].l0 * (float)p10[ax[j].i0] + ax[j].l1 * (float)p10[ax[j].i1];
                const float a11 = ax[j].l0 * (float)p11[ax[j].i0] + ax[j].l1 * (float)p11[ax[j].i1];
                const float b0 = ay.l0 * a00 + ay.l1 * a01, b1 = ay.l0 * a10 + ay.l1 * a11;
                v[j] = az.l0 * b0 + az.l1 * b1;
            }
        }
        store4<TO>(a, out + ((unsigned)oz * a.Ho + oy) * a.Wo + ox, ox, v);
    }
}

bool fits31(int a, int b, int c) { return (long)a * b * c < (1l << 31); }

// launch 2 of the z-score, or the plain padded copy
int pad_launch(bool norm, const void* x, int dtype, int D, int H, int W, float lo, float hi, const void* ws, float* out, int Do, int Ho, int Wo,
               int z_lo, int y_lo, int x_lo, float* ms, void* stream, bool pop = false) {
    NormArgs a{};
    a.pop = pop ? 1 : 0;
    a.x = x; a.out = out; a.ws = (const double*)ws; a.ms = ms;
    a.D = D; a.H = H; a.W = W; a.Do = Do; a.Ho = Ho; a.Wo = Wo; a.z_lo = z_lo; a.y_lo = y_lo; a.x_lo = x_lo;
    a.lo = lo; a.hi = hi;
    a.No = (unsigned)((long)Do * Ho * Wo);
    const unsigned mis = (unsigned)((16 - (uintptr_t)out % 16) % 16 / 4);
    a.head = mis < a.No ? mis : a.No;
    a.ngrp = (a.No - a.head) / 4;
    const unsigned per = NT * NITER, nb = a.ngrp ? (a.ngrp + per - 1) / per : 1;
    const dim3 grid(nb), block(NT);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == RSUPER_VOX_I16) {
        if (norm) hipLaunchKernelGGL((ct_normalize_kernel<short, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ct_normalize_kernel<short, false>), grid, block, 0, s, a);
    } else {
        if (norm) hipLaunchKernelGGL((ct_normalize_kernel<float, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ct_normalize_kernel<float, false>), grid, block, 0, s, a);
    }
    return rs_check_launch();
}

bool pad_args_ok(const void* x, int dtype, int D, int H, int W, const float* out, int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo) {
    if (!x || !out || (const void*)out == x || (dtype != RSUPER_VOX_I16 && dtype != RSUPER_VOX_F32)) return false;
    if (D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1 || !fits31(D, H, W) || !fits31(Do, Ho, Wo)) return false;
    if (z_lo < 0 || y_lo < 0 || x_lo < 0 || z_lo > Do - D || y_lo > Ho - H || x_lo > Wo - W) return false;
    return (uintptr_t)x % (dtype == RSUPER_VOX_I16 ? 2 : 4) == 0 && (uintptr_t)out % 4 == 0;
}

}  // namespace

extern "C" {

long rsuper_ct_stats_workspace_bytes(void) { return 3l * PARTS * (long)sizeof(double); }

int rsuper_ct_stats(const void* x, int dtype, int D, int H, int W, float lo, float hi, void* workspace, long workspace_bytes, void* stream) {
    if (!x || !workspace || (dtype != RSUPER_VOX_I16 && dtype != RSUPER_VOX_F32) || D < 1 || H < 1 || W < 1 || !fits31(D, H, W)) return RS_ERR_ARG;
    if (workspace_bytes < rsuper_ct_stats_workspace_bytes() || (uintptr_t)workspace % 8) return RS_ERR_ARG;
    const unsigned esz = dtype == RSUPER_VOX_I16 ? 2 : 4, vec = 16 / esz;
    if ((uintptr_t)x % esz) return RS_ERR_ARG;
    StatArgs a{};
    a.x = x; a.ws = (double*)workspace; a.lo = lo; a.hi = hi;
    a.N = (unsigned)((long)D * H * W);
    const unsigned mis = (unsigned)((16 - (uintptr_t)x % 16) % 16 / esz);
    a.head = mis < a.N ? mis : a.N;
    a.nvec = (a.N - a.head) / vec;
    a.vper = (a.nvec + PARTS - 1) / PARTS;
    if (dtype == RSUPER_VOX_I16) hipLaunchKernelGGL(ct_stats_kernel<short>, dim3(PARTS), dim3(SNT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ct_stats_kernel<float>, dim3(PARTS), dim3(SNT), 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

int rsuper_ct_normalize(const void* x, int dtype, int D, int H, int W, float lo, float hi, const void* workspace, long workspace_bytes, float* out,
                        int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo, float* mean_std, void* stream) {
    if (!pad_args_ok(x, dtype, D, H, W, out, Do, Ho, Wo, z_lo, y_lo, x_lo) || !workspace || !mean_std) return RS_ERR_ARG;
    if (workspace_bytes < rsuper_ct_stats_workspace_bytes() || (uintptr_t)workspace % 8 || (uintptr_t)mean_std % 4) return RS_ERR_ARG;
    return pad_launch(true, x, dtype, D, H, W, lo, hi, workspace, out, Do, Ho, Wo, z_lo, y_lo, x_lo, mean_std, stream);
}

int rsuper_ct_normalize_pop(const void* x, int dtype, int D, int H, int W, float lo, float hi, const void* workspace, long workspace_bytes, float* out,
                            int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo, float* mean_std, void* stream) {
    if (!pad_args_ok(x, dtype, D, H, W, out, Do, Ho, Wo, z_lo, y_lo, x_lo) || !workspace || !mean_std) return RS_ERR_ARG;
    if (workspace_bytes < rsuper_ct_stats_workspace_bytes() || (uintptr_t)workspace % 8 || (uintptr_t)mean_std % 4) return RS_ERR_ARG;
    return pad_launch(true, x, dtype, D, H, W, lo, hi, workspace, out, Do, Ho, Wo, z_lo, y_lo, x_lo, mean_std, stream, true);
}

int rsuper_pad_box(const void* x, int dtype, int D, int H, int W, float* out, int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo, void* stream) {
    if (!pad_args_ok(x, dtype, D, H, W, out, Do, Ho, Wo, z_lo, y_lo, x_lo)) return RS_ERR_ARG;
    return pad_launch(false, x, dtype, D, H, W, 0.f, 0.f, nullptr, out, Do, Ho, Wo, z_lo, y_lo, x_lo, nullptr, stream);
}

int rsuper_resample3d(const void* src, int in_dtype, int C, int Dp, int Hp, int Wp, int z0, int y0, int x0, int D, int H, int W, void* out,
                      int out_dtype, int Do, int Ho, int Wo, int mode, int use_threshold, float threshold, void* stream) {
    if (!src || !out || src == out || C < 1 || C > 65535 || Dp < 1 || Hp < 1 || Wp < 1 || D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1)
        return RS_ERR_ARG;
    if ((in_dtype != RSUPER_VOX_U8 && in_dtype != RSUPER_VOX_F32) || (out_dtype != RSUPER_VOX_U8 && out_dtype != RSUPER_VOX_F32)) return RS_ERR_ARG;
    if (mode != RSUPER_RESAMPLE_NEAREST && mode != RSUPER_RESAMPLE_TRILINEAR) return RS_ERR_ARG;
    if (z0 < 0 || y0 < 0 || x0 < 0 || z0 > Dp - D || y0 > Hp - H || x0 > Wp - W || !fits31(Dp, Hp, Wp) || !fits31(Do, Ho, Wo)) return RS_ERR_ARG;
    if ((in_dtype == RSUPER_VOX_F32 && (uintptr_t)src % 4) || (out_dtype == RSUPER_VOX_F32 && (uintptr_t)out % 4)) return RS_ERR_ARG;
    if (use_threshold && out_dtype != RSUPER_VOX_U8) return RS_ERR_ARG;
    // a u8 output without a threshold is a copy of u8 voxels: an interpolated or f32 value has no defined byte
    if (!use_threshold && out_dtype == RSUPER_VOX_U8 && (in_dtype != RSUPER_VOX_U8 || mode != RSUPER_RESAMPLE_NEAREST)) return RS_ERR_UNSUPPORTED;
    RsArgs a{};
    a.src = src; a.out = out;
    a.Dp = Dp; a.Hp = Hp; a.Wp = Wp; a.z0 = z0; a.y0 = y0; a.x0 = x0; a.D = D; a.H = H; a.W = W; a.Do = Do; a.Ho = Ho; a.Wo = Wo;
    a.use_thr = use_threshold ? 1 : 0; a.thr = threshold;
    if (mode == RSUPER_RESAMPLE_NEAREST) {
        a.sz = (float)D / (float)Do; a.sy = (float)H / (float)Ho; a.sx = (float)W / (float)Wo;
    } else {
        a.sz = Do > 1 ? (float)(D - 1) / (float)(Do - 1) : 0.f;
        a.sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
        a.sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    }
    const int groups = (Wo + 3) / 4;
    a.lx = 1;
    while (a.lx < 64 && a.lx < groups) a.lx *= 2;
    a.nbx = (groups + a.lx - 1) / a.lx;
    a.nby = (Ho + TY - 1) / TY;
    const long nblk = (long)a.nbx * a.nby * ((Do + TZ - 1) / TZ);
    if (nblk >= (1l << 31)) return RS_ERR_ARG;
    a.vec = Wo % 4 == 0 && (uintptr_t)out % (out_dtype == RSUPER_VOX_F32 ? 16 : 4) == 0;
    const dim3 grid((unsigned)nblk, C), block(NT);
    hipStream_t s = (hipStream_t)stream;
    const int key = (in_dtype == RSUPER_VOX_F32 ? 4 : 0) | (out_dtype == RSUPER_VOX_F32 ? 2 : 0) | (mode == RSUPER_RESAMPLE_TRILINEAR ? 1 : 0);
    switch (key) {
    case 0: hipLaunchKernelGGL((resample3d_kernel<uint8_t, uint8_t, 0>), grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL((resample3d_kernel<uint8_t, uint8_t, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((resample3d_kernel<uint8_t, float, 0>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((resample3d_kernel<uint8_t, float, 1>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((resample3d_kernel<float, uint8_t, 0>), grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL((resample3d_kernel<float, uint8_t, 1>), grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL((resample3d_kernel<float, float, 0>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((resample3d_kernel<float, float, 1>), grid, block, 0, s, a); break;
    }
    return rs_check_launch();
}

}  // extern "C"
