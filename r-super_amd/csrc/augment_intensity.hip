// Intensity augmentation of the loader (training/augmentation.py brightness_multiply / brightness_additive / gamma / contrast / gaussian_blur /
// gaussian_noise :27-103, gated per sample as dataset/augmented.py online_intensity_augmentation :142-158 gates them) on a batch of (B, 1, D, H, W) f32
// volumes.  Per sample a host record says which of the six fired and with which parameter; they apply in the loader's fixed order.
//
// Passes (every launch covers up to 8 samples, grid.y = sample; blocks of a sample that does not need a pass return at once):
//   stats 0   min / max / sum / sum of squares of x2 = x * f + a                      (samples with gamma or contrast)
//   stats 1   the same four of y = pow((x2 - lo) / (hi - lo), g) * (hi - lo) + lo     (samples with gamma)
//   apply     chain -> blur -> noise -> store                                          (always)
// so a batch costs 1 launch without gamma / contrast, 2 with contrast only, 3 with gamma.  A stats block reduces its run of the sample in f64
// (squares of f32 values are exact in f64) and writes ONE partial (4 doubles) into the caller's workspace; the consumer (stats 1, apply) combines the
// partials of its sample in a fixed order -- no atomics, no memset, the same bits on every run.  Contrast after gamma takes no third reduction: the map
// y -> z = (y - mean y) / std y * std + mean is increasing, so min z / max z are that same f32 expression applied to min y / max y, and mean z is
// the mean gamma restores.
//
// apply, sample with blur: one block = one 8 x 8 x 32 output brick.  The brick plus a halo of r (z, y) and of the 16-byte groups that cover r (x) is
// read once with the pointwise chain applied on the way into LDS -- zeros outside the volume: the padding is of the post-contrast image -- then the
// three 1-D passes W, H, D run in place in that one 18 x 18 x 48 f32 tile (62 208 bytes: two blocks per CU) and the D pass adds the noise and stores.
// The taps arrive centred in an 11-tap record (tap[5 - r .. 5 + r]), so the tile layout does not depend on r while the loops only touch what r needs.
// apply, sample without blur: the same brick, pointwise.  x is the fast axis: 16-byte loads and stores when W % 4 == 0 and the bases are aligned,
// scalar otherwise.
//
// Noise: Philox4x32-10, key = the sample's 64-bit seed (low, high word), counter = (i >> 2 low, i >> 2 high, 0, 0) for voxel i of the sample; the four
// outputs r0..r3 give u = ((r >> 8) + 0.5) * 2^-24 (rounded once to f32) and two Box-Muller pairs: normals 0, 1 = sqrt(-2 ln u(r0)) * (cos, sin)(2 pi u(r1)),
// normals 2, 3 the same from (r2, r3); voxel i takes normal i & 3.  A function of (seed, i) alone.
//
// Float contraction is off in this file: a * b + c is two roundings as in the ATen expressions it restates; the blur uses explicit fmaf.
#include "common.hpp"
#include "../../include/rsuper_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, MAXB = 8;
constexpr int RMAX = RSUPER_BLUR_MAX_RADIUS, NTAP = 2 * RMAX + 1;
constexpr int BZ = 8, BY = 8, BX = 32;                   // output brick
constexpr int XPAD = (RMAX + 3) / 4 * 4;                 // x halo of the tile: whole 16-byte groups
constexpr int LZ = BZ + 2 * RMAX, LY = BY + 2 * RMAX, LX = BX + 2 * XPAD;
constexpr int XG = BX / 4;                               // 16-byte groups per brick row
constexpr int WIN = (XPAD - RMAX + 3 + NTAP + 3) / 4 * 4; // floats a W-pass item reads: output c = 0..3 uses window[c + XPAD - RMAX + j]
constexpr int PARTS_MAX = 128;                           // partials per sample and pass
constexpr long PART_VOX = (long)NT * 4 * 8;              // voxels a stats block takes at least
static_assert(BZ * BY * XG == 2 * NT && NT % (XG * BY) == 0, "the D pass and the pointwise brick give every lane two 16-byte groups");
static_assert(NT % XG == 0, "the groups of one tile row stay in one wave (the W pass runs in place)");
static_assert(XPAD >= RMAX && XPAD - RMAX + 3 + NTAP <= WIN && BX - 4 + WIN <= LX, "W-pass window");
static_assert(LZ * LY * LX * 4 + 256 <= 65536, "static LDS");

enum { F_MUL = 1, F_ADD = 2, F_GAMMA = 4, F_CONTRAST = 8, F_BLUR = 16, F_NOISE = 32 };

struct Sample {
    int flags, r;
    float f, a, g, c, nstd;
    uint32_t k0, k1;
    float tap[NTAP];                                     // centred: tap[RMAX - r .. RMAX + r]
};

struct Args {
    const float* img;
    float* out;
    const float* noise;                                  // optional explicit N(0, 1) field
    double* ws;                                          // [2][MAXB][PARTS_MAX][4]
    int D, H, W, parts, vec, nbx, nby;
    long V, per;                                         // voxels per sample, per stats block (multiple of 4)
    Sample s[MAXB];
};

struct Chain {                                           // the pointwise part of one sample, f32 as the host code holds it
    int flags;
    float f, a;
    float lo, span, g, my, sy, s, m;                     // gamma
    float clo, chi, cmean, c;                            // contrast
};

__device__ __forceinline__ float pre(const Chain& k, float x) {
    if (k.flags & F_MUL) x = x * k.f;
    if (k.flags & F_ADD) x = x + k.a;
    return x;
}
__device__ __forceinline__ float gamma_y(const Chain& k, float x2) { return powf((x2 - k.lo) / k.span, k.g) * k.span + k.lo; }
__device__ __forceinline__ float gamma_z(const Chain& k, float y) { return (y - k.my) / k.sy * k.s + k.m; }
__device__ __forceinline__ float contrast(const Chain& k, float v) {
    const float t = (v - k.cmean) * k.c + k.cmean;
    return t != t ? t : fminf(fmaxf(t, k.clo), k.chi);   // clamp keeps a NaN
}
__device__ __forceinline__ float chain(const Chain& k, float x) {
    x = pre(k, x);
    if (k.flags & F_GAMMA) x = gamma_z(k, gamma_y(k, x));
    if (k.flags & F_CONTRAST) x = contrast(k, x);
    return x;
}

__device__ __forceinline__ double* partials(const Args& a, int pass, int b) { return a.ws + ((long)(pass * MAXB + b) * PARTS_MAX) * 4; }

// sum, sum of squares, min, max of the sample's partials -> sh[0..3]; wave 0 in a fixed order, then a barrier
__device__ __forceinline__ void combine(const double* p, int parts, double* sh) {
    if (threadIdx.x < 64) {
        double s = 0.0, q = 0.0, lo = INFINITY, hi = -INFINITY;
        for (int i = threadIdx.x; i < parts; i += 64) {
            s += p[4 * i]; q += p[4 * i + 1];
            lo = fmin(lo, p[4 * i + 2]); hi = fmax(hi, p[4 * i + 3]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64);
            lo = fmin(lo, __shfl_xor(lo, o, 64)); hi = fmax(hi, __shfl_xor(hi, o, 64));
        }
        if (threadIdx.x == 0) { sh[0] = s; sh[1] = q; sh[2] = lo; sh[3] = hi; }
    }
    __syncthreads();
}

__device__ __forceinline__ void moments(const double* st, long N, float& mean, float& sd, float& lo, float& hi) {
    const double n = (double)N, m = st[0] / n;
    double var = (st[1] - st[0] * m) / (n - 1.0);        // unbiased
    var = var < 0.0 ? 0.0 : var;
    mean = (float)m; sd = (float)sqrt(var);
    lo = (float)st[2]; hi = (float)st[3];
    if (st[0] != st[0]) lo = hi = NAN;                   // min / max of a volume that holds a NaN
}

__device__ __forceinline__ void derive0(Chain& k, const Sample& s, const double* st, long N) {
    float mean, sd, lo, hi;
    moments(st, N, mean, sd, lo, hi);
    k.lo = lo; k.span = hi - lo; k.g = s.g; k.s = sd; k.m = mean;      // gamma
    k.clo = lo; k.chi = hi; k.cmean = mean; k.c = s.c;                 // contrast without gamma (derive1 replaces them after gamma)
}
__device__ __forceinline__ void derive1(Chain& k, const double* st, long N) {
    float lo, hi;
    moments(st, N, k.my, k.sy, lo, hi);
    k.clo = gamma_z(k, lo); k.chi = gamma_z(k, hi); k.cmean = k.m;
}

// ---- stats pass: one partial per block
__global__ __launch_bounds__(NT) void intensity_stats_kernel(Args a, int pass) {
    const int b = blockIdx.y;
    const Sample& s = a.s[b];
    if (!(s.flags & (pass ? F_GAMMA : (F_GAMMA | F_CONTRAST)))) return;
    __shared__ double sh[4], shw[NT / 64][4];
    Chain k{};
    k.flags = s.flags; k.f = s.f; k.a = s.a;
    if (pass) {
        combine(partials(a, 0, b), a.parts, sh);
        derive0(k, s, sh, a.V);
    }
    const float* __restrict__ x = a.img + (long)b * a.V;
    const long n0 = (long)blockIdx.x * a.per, n1 = n0 + a.per < a.V ? n0 + a.per : a.V;
    double sum = 0.0, sq = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    auto take = [&](float v) {
        v = pre(k, v);
        if (pass) v = gamma_y(k, v);
        sum += (double)v; sq += (double)v * (double)v;
        lo = fminf(lo, v); hi = fmaxf(hi, v);
    };
    if (a.vec) {                                         // V, per and n0 are multiples of 4
        for (long i = n0 + 4 * (long)threadIdx.x; i < n1; i += 4 * NT) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            take(v.x); take(v.y); take(v.z); take(v.w);
        }
    } else {
        for (long i = n0 + threadIdx.x; i < n1; i += NT) take(x[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64); sq += __shfl_xor(sq, o, 64);
        lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shw[wave][0] = sum; shw[wave][1] = sq; shw[wave][2] = lo; shw[wave][3] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) {
            sum += shw[w][0]; sq += shw[w][1];
            lo = fminf(lo, (float)shw[w][2]); hi = fmaxf(hi, (float)shw[w][3]);
        }
        double* p = partials(a, pass, b) + 4 * blockIdx.x;
        p[0] = sum; p[1] = sq; p[2] = lo; p[3] = hi;
    }
}

// ---- noise
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t r[4]) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
__device__ __forceinline__ float unit(uint32_t r) { return fmaf((float)(r >> 8), 0x1p-24f, 0x1p-25f); }
// the four normals of voxels 4 q .. 4 q + 3
__device__ __forceinline__ void normals4(long q, const Sample& s, float n[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)((unsigned long)q >> 32), s.k0, s.k1, r);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float R = sqrtf(-2.f * logf(unit(r[2 * p])));
        float sn, cs;
        sincospif(2.f * unit(r[2 * p + 1]), &sn, &cs);
        n[2 * p] = R * cs; n[2 * p + 1] = R * sn;
    }
}

// noise and store of 4 voxels along x starting at linear index i of the sample (gx = their x; the row ends at W)
__device__ __forceinline__ void finish4(const Args& a, const Sample& s, int b, long i, int gx, float v[4]) {
    float* __restrict__ out = a.out + (long)b * a.V + i;
    if (a.vec) {
        if (s.flags & F_NOISE) {
            float n[4];
            if (a.noise) {
                const float4 t = *reinterpret_cast<const float4*>(a.noise + (long)b * a.V + i);
                n[0] = t.x; n[1] = t.y; n[2] = t.z; n[3] = t.w;
            } else normals4(i >> 2, s, n);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] + n[j] * s.nstd;
        }
        *reinterpret_cast<float4*>(out) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (gx + j >= a.W) break;
            float r = v[j];
            if (s.flags & F_NOISE) {
                float n;
                if (a.noise) n = a.noise[(long)b * a.V + i + j];
                else {
                    float t[4];
                    normals4((i + j) >> 2, s, t);
                    n = t[(i + j) & 3];
                }
                r = r + n * s.nstd;
            }
            out[j] = r;
        }
    }
}

// ---- apply pass
__global__ __launch_bounds__(NT) void intensity_apply_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) float T[LZ * LY * LX];
    __shared__ double sh[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Sample& s = a.s[b];
    const int D = a.D, H = a.H, W = a.W;
    const int bx = blockIdx.x % a.nbx, t0 = blockIdx.x / a.nbx, by = t0 % a.nby, bz = t0 / a.nby;
    const int x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;
    const float* __restrict__ src = a.img + (long)b * a.V;

    Chain k{};
    k.flags = s.flags; k.f = s.f; k.a = s.a;
    if (s.flags & (F_GAMMA | F_CONTRAST)) {
        combine(partials(a, 0, b), a.parts, sh);
        derive0(k, s, sh, a.V);
        if (s.flags & F_GAMMA) {
            __syncthreads();                             // sh is reused
            combine(partials(a, 1, b), a.parts, sh);
            derive1(k, sh, a.V);
        }
    }

    if (!(s.flags & F_BLUR)) {                           // pointwise brick: two 16-byte groups per lane
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int it = tid + n * NT;
            const int gx = x0 + 4 * (it % XG), gy = y0 + (it / XG) % BY, gz = z0 + it / (XG * BY);
            if (gx >= W || gy >= H || gz >= D) continue;
            const long i = ((long)gz * H + gy) * W + gx;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.vec) {
                const float4 q = *reinterpret_cast<const float4*>(src + i);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gx + j < W) v[j] = src[i + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = chain(k, v[j]);
            finish4(a, s, b, i, gx, v);
        }
        return;
    }

    const int r = s.r, lo = RMAX - r;                    // first tile row / plane in use
    const int nz = BZ + 2 * r, ny = BY + 2 * r;
    const int q0 = (XPAD - r) >> 2, nq = ((XPAD + BX + r + 3) >> 2) - q0;
    // stage: chain(x) inside the volume, 0 outside.  Tile index (lz, ly, lx) <-> voxel (z0 + lz - RMAX, y0 + ly - RMAX, x0 + lx - XPAD)
    for (int it = tid; it < nz * ny * nq; it += NT) {
        const int q = q0 + it % nq, t = it / nq, ly = lo + t % ny, lz = lo + t / ny;
        const int gz = z0 + lz - RMAX, gy = y0 + ly - RMAX, gx = x0 + 4 * q - XPAD;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)gz < (unsigned)D && (unsigned)gy < (unsigned)H) {
            const long i = ((long)gz * H + gy) * W + gx;
            if (a.vec) {
                if ((unsigned)gx < (unsigned)W) {
                    const float4 u = *reinterpret_cast<const float4*>(src + i);
                    v[0] = chain(k, u.x); v[1] = chain(k, u.y); v[2] = chain(k, u.z); v[3] = chain(k, u.w);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((unsigned)(gx + j) < (unsigned)W) v[j] = chain(k, src[i + j]);
            }
        }
        *reinterpret_cast<float4*>(T + (lz * LY + ly) * LX + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();

    // W pass, in place: the XG items of a tile row sit in consecutive lanes of one wave, which reads all their windows before it writes
    for (int it0 = 0; it0 < nz * ny * XG; it0 += NT) {   // the same trip count for every lane: the wave barrier sits in uniform control flow
        const int it = it0 + tid;
        const bool act = it < nz * ny * XG;
        const int g = it % XG, t = it / XG, ly = lo + t % ny, lz = lo + t / ny;
        float* row = T + (lz * LY + ly) * LX + 4 * g;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (act) {
            float w[WIN];
#pragma unroll
            for (int m = 0; m < WIN / 4; ++m) {
                const float4 u = *reinterpret_cast<const float4*>(row + 4 * m);
                w[4 * m] = u.x; w[4 * m + 1] = u.y; w[4 * m + 2] = u.z; w[4 * m + 3] = u.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < NTAP; ++j)
                    if (j >= lo && j <= RMAX + r) acc = fmaf(s.tap[j], w[c + XPAD - RMAX + j], acc);
                o[c] = acc;
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (act) *reinterpret_cast<float4*>(row + XPAD) = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();

    // H pass, in place: one lane walks one (plane, group) column downwards; output row oy goes to tile row lo + oy, which no later output reads
    for (int it = tid; it < nz * XG; it += NT) {
        const int g = it % XG, lz = lo + it / XG;
        float* col = T + (lz * LY) * LX + XPAD + 4 * g;
        for (int oy = 0; oy < BY; ++oy) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = lo; j <= RMAX + r; ++j) {
                const float4 u = *reinterpret_cast<const float4*>(col + (oy + j) * LX);
                const float tp = s.tap[j];
                acc.x = fmaf(tp, u.x, acc.x); acc.y = fmaf(tp, u.y, acc.y); acc.z = fmaf(tp, u.z, acc.z); acc.w = fmaf(tp, u.w, acc.w);
            }
            *reinterpret_cast<float4*>(col + (lo + oy) * LX) = acc;
        }
    }
    __syncthreads();

    // D pass: lane = (pair of output planes, row, group); noise and store
    {
        const int g = tid % XG, y = (tid / XG) % BY, zp = tid / (XG * BY);
        const int gx = x0 + 4 * g, gy = y0 + y;
        const float* col = T + (lo + y) * LX + XPAD + 4 * g;
#pragma unroll
        for (int n = 0; n < BZ / (NT / (XG * BY)); ++n) {
            const int oz = zp * (BZ / (NT / (XG * BY))) + n, gz = z0 + oz;
            if (gx >= W || gy >= H || gz >= D) continue;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = lo; j <= RMAX + r; ++j) {
                const float4 u = *reinterpret_cast<const float4*>(col + (oz + j) * (LY * LX));
                const float tp = s.tap[j];
                acc.x = fmaf(tp, u.x, acc.x); acc.y = fmaf(tp, u.y, acc.y); acc.z = fmaf(tp, u.z, acc.z); acc.w = fmaf(tp, u.w, acc.w);
            }
            float v[4] = {acc.x, acc.y, acc.z, acc.w};
            finish4(a, s, b, ((long)gz * H + gy) * W + gx, gx, v);
        }
    }
}

int stat_parts(long V) {
    const long p = (V + PART_VOX - 1) / PART_VOX;
    return (int)(p < 1 ? 1 : p > PARTS_MAX ? PARTS_MAX : p);
}

}  // namespace

extern "C" {

long rsuper_intensity_augment_workspace_bytes(int B, int D, int H, int W) {
    if (B < 1 || D < 1 || H < 1 || W < 1) return 0;
    return 2l * MAXB * PARTS_MAX * 4 * (long)sizeof(double);
}

int rsuper_intensity_augment_launches(int B, const int* flags) {
    if (B < 1 || !flags) return 0;
    int n = 0;
    for (int b0 = 0; b0 < B; b0 += MAXB) {
        int any = 0;
        for (int b = b0; b < B && b < b0 + MAXB; ++b) any |= flags[b];
        n += 1 + ((any & (F_GAMMA | F_CONTRAST)) ? 1 : 0) + ((any & F_GAMMA) ? 1 : 0);
    }
    return n;
}

int rsuper_intensity_augment(const float* img, float* out, int B, int D, int H, int W, const int* flags, const float* scalars, const int* radius,
                             const float* taps, const unsigned long long* seeds, const float* noise, void* workspace, long workspace_bytes,
                             void* stream) {
    if (!img || !out || img == out || !flags || !scalars || !radius || !taps || !seeds || B < 1 || D < 1 || H < 1 || W < 1) return RS_ERR_ARG;
    const long V = (long)D * H * W;
    if (V >= (1l << 31)) return RS_ERR_ARG;
    int any = 0;
    for (int b = 0; b < B; ++b) {
        if (flags[b] < 0 || flags[b] > 63) return RS_ERR_ARG;
        if ((flags[b] & F_BLUR) && (radius[b] < 0 || radius[b] > RMAX)) return RS_ERR_ARG;   // never clamped
        any |= flags[b];
    }
    if ((any & (F_GAMMA | F_CONTRAST)) && (!workspace || workspace_bytes < rsuper_intensity_augment_workspace_bytes(B, D, H, W) || (uintptr_t)workspace % 8))
        return RS_ERR_ARG;

    Args a{};
    a.D = D; a.H = H; a.W = W; a.V = V;
    a.ws = (double*)workspace;
    a.parts = stat_parts(V);
    a.per = ((V + a.parts - 1) / a.parts + 3) & ~3l;
    a.vec = (W % 4 == 0) && ((uintptr_t)img % 16 == 0) && ((uintptr_t)out % 16 == 0) && (!noise || (uintptr_t)noise % 16 == 0);
    a.nbx = (W + BX - 1) / BX;
    a.nby = (H + BY - 1) / BY;
    const int nbricks = a.nbx * a.nby * ((D + BZ - 1) / BZ);
    for (int b0 = 0; b0 < B; b0 += MAXB) {               // the per-sample records travel in the kernel arguments, MAXB samples per launch
        const int nb = B - b0 < MAXB ? B - b0 : MAXB;
        int grp = 0;
        for (int b = 0; b < nb; ++b) {
            Sample& s = a.s[b];
            const float* sc = scalars + 5 * (b0 + b);
            s = Sample{};
            s.flags = flags[b0 + b];
            s.f = sc[0]; s.a = sc[1]; s.g = sc[2]; s.c = sc[3]; s.nstd = sc[4];
            s.k0 = (uint32_t)seeds[b0 + b]; s.k1 = (uint32_t)(seeds[b0 + b] >> 32);
            if (s.flags & F_BLUR) {
                s.r = radius[b0 + b];
                for (int j = 0; j <= 2 * s.r; ++j) s.tap[RMAX - s.r + j] = taps[(long)NTAP * (b0 + b) + j];
            }
            grp |= s.flags;
        }
        a.img = img + (long)b0 * V;
        a.out = out + (long)b0 * V;
        a.noise = noise ? noise + (long)b0 * V : nullptr;
        if (grp & (F_GAMMA | F_CONTRAST)) {
            hipLaunchKernelGGL(intensity_stats_kernel, dim3(a.parts, nb), dim3(NT), 0, (hipStream_t)stream, a, 0);
            if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
        }
        if (grp & F_GAMMA) {
            hipLaunchKernelGGL(intensity_stats_kernel, dim3(a.parts, nb), dim3(NT), 0, (hipStream_t)stream, a, 1);
            if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(intensity_apply_kernel, dim3(nbricks, nb), dim3(NT), 0, (hipStream_t)stream, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

}  // extern "C"
