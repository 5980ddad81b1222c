// NIfTI front and back end of a case on the device (predict_abdomenatlas.py preprocess :333-343, dataset_conversion/utils.py ResampleXYZAxis /
// reorient_image): reorientation as strided reads, the cubic B-spline prefilter in x and y, the "B-spline in-plane, nearest along z" resample,
// and the way back from canonical uint8 masks to the file's voxel order.  DESIGN.md 6p has the layout, the tables and the bytes per pass.
//
// nifti_lines_kernel   one kernel for both prefilter passes and for the plain reoriented copy.  A block stages NR whole lines of N samples in LDS
//   (pitch = 1 mod 32 floats, so the lanes of a 32-lane group, which hold 32 different lines, sit on 32 different banks), filters them there and
//   writes them out.  Source and destination are addressed by three element strides each (line, row, outer), so a flip is a negative stride and a
//   permutation costs nothing; the side whose unit stride lies along the rows is walked with the lanes along the rows ("fast rows"), the other
//   with the lanes along the line: either way a lane group touches consecutive addresses.
//     pass 1  file buffer (any dtype, scaled) -> canonical [Z][Y][X] f32, lines along x
//     pass 2  in place on that volume, lines along y, rows along x (32 columns = one 128-byte line per y), only with prefilter
//   The recursion c+[k] = g s[k] + z1 c+[k-1], c[k] = z1 (c[k+1] - c+[k]) (z1 = sqrt(3) - 2, g = (1 - z1)(1 - 1/z1) = 6) forgets its start at the
//   rate |z1|^k, below 2^-30 from k = 16 on.  A line is therefore cut into segments of L samples with one lane each: a lane starts its causal run
//   with the 16-term sum  sum_k z1^k g s[mirror(a - k)]  (at a = 0 this is the whole-sample mirror start with the terms below 2^-30 dropped) and
//   its anticausal run 16 samples past its segment, or at the line's end with c[N-1] = z1 / (z1^2 - 1) (c+[N-1] + z1 c+[N-2]).
//   Starts are computed from values no lane is writing (a barrier separates them from the in-place runs).  N = 1: the sample itself.
//
// bspline_resample_kernel   a block makes a 64 (x) x 16 (y) tile of one output slice.  The coefficient rows the tile's y taps touch are first
//   interpolated along x into LDS (4 gathered loads per staged value; the 64 lanes read one or two cache lines per load), then every output is
//   4 LDS reads.  Output slices that the nearest-z table maps to the same source slice are written by one block.  A tile whose rows do not fit
//   the 64-row LDS tile (in-plane downsampling beyond about 3.5 : 1) reads global memory directly.
//
// reorient_store_kernel   canonical [C][Z][Y][X] uint8 -> file order at a byte offset of a caller's buffer; the lanes run along the file's i.
#include "common.hpp"
#include "../../include/rsuper_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_SIDE = 4096;
constexpr int LT = 256;                                  // threads of a line block at most
constexpr int SEG = 64;                                  // samples per lane before the bank rule rounds it up
constexpr int WARM = 16;                                 // |z1|^16 < 2^-30
constexpr int LDS_BUDGET = 72 * 1024;                    // two blocks per CU
constexpr float Z1 = -0.26794919243112270647f;
constexpr float GAIN = 6.0f;
constexpr float CEND = Z1 / (Z1 * Z1 - 1.f);
constexpr float CMID = -Z1 / (1.f - Z1);                 // c of a constant c+ to the right: the start of an interior warm-up

struct LineArgs {
    const void* src;
    float* dst;
    long s_off, s_line, s_row, s_outer, d_line, d_row, d_outer;
    int N, nrow, NR, logNR, TPR, L, pitch;
    int src_fast_rows, dst_fast_rows, prefilter, scale;
    float slope, inter;
};

__device__ __forceinline__ int mirror(int i, int N) {    // whole-sample mirror about 0 and N - 1; N >= 2
    const int P = 2 * N - 2;
    int m = i % P;
    if (m < 0) m += P;
    return m < N ? m : P - m;
}

template <typename TI>
__global__ __launch_bounds__(LT) void nifti_lines_kernel(LineArgs a) {
    extern __shared__ float nl_tile[];
    const int t = threadIdx.x, T = a.NR * a.TPR, N = a.N;
    const int row0 = blockIdx.x * a.NR;
    const int nr = a.nrow - row0 < a.NR ? a.nrow - row0 : a.NR;
    const int r = t & (a.NR - 1), g = t >> a.logNR;
    const TI* src = (const TI*)a.src;                       // pass 2 runs in place: no __restrict__
    const long sbase = a.s_off + (long)blockIdx.y * a.s_outer + (long)row0 * a.s_row;
    auto conv = [&](TI raw) {
        float v = (float)raw;
        if (a.scale) v = v * a.slope + a.inter;
        return v;
    };
    if (a.src_fast_rows) {
        if (r < nr)
            for (int x = g; x < N; x += a.TPR) nl_tile[r * a.pitch + x] = conv(src[sbase + (long)r * a.s_row + (long)x * a.s_line]);
    } else {
        for (int rr = 0; rr < nr; ++rr)
            for (int x = t; x < N; x += T) nl_tile[rr * a.pitch + x] = conv(src[sbase + (long)rr * a.s_row + (long)x * a.s_line]);
    }
    __syncthreads();
    if (a.prefilter && N > 1) {
        const int a0 = g * a.L, b0 = a0 + a.L < N ? a0 + a.L : N;
        const bool active = r < nr && a0 < N;
        float* row = nl_tile + r * a.pitch;
        float acc = 0.f;
        if (active) {
            if (a0 >= WARM - 1) {
#pragma unroll
                for (int k = WARM - 1; k >= 0; --k) acc = GAIN * row[a0 - k] + Z1 * acc;
            } else {
                for (int k = WARM - 1; k >= 0; --k) acc = GAIN * row[mirror(a0 - k, N)] + Z1 * acc;
            }
        }
        __syncthreads();
        if (active) {
            row[a0] = acc;
            for (int k = a0 + 1; k < b0; ++k) { acc = GAIN * row[k] + Z1 * acc; row[k] = acc; }
        }
        __syncthreads();
        float c = 0.f;
        if (active) {
            const int e = b0 - 1 + WARM < N - 1 ? b0 - 1 + WARM : N - 1;
            c = e == N - 1 ? CEND * (row[N - 1] + Z1 * row[N - 2]) : CMID * row[e];
            for (int k = e - 1; k >= b0 - 1; --k) c = Z1 * (c - row[k]);
        }
        __syncthreads();
        if (active) {
            row[b0 - 1] = c;
            for (int k = b0 - 2; k >= a0; --k) { c = Z1 * (c - row[k]); row[k] = c; }
        }
        __syncthreads();
    }
    float* dst = a.dst + (long)blockIdx.y * a.d_outer + (long)row0 * a.d_row;
    if (a.dst_fast_rows) {
        if (r < nr)
            for (int x = g; x < N; x += a.TPR) dst[(long)r * a.d_row + (long)x * a.d_line] = nl_tile[r * a.pitch + x];
    } else {
        for (int rr = 0; rr < nr; ++rr)
            for (int x = t; x < N; x += T) dst[(long)rr * a.d_row + (long)x * a.d_line] = nl_tile[rr * a.pitch + x];
    }
}

// lanes per line, lines per block, samples per lane and the LDS pitch of lines of N samples
void line_config(LineArgs& a) {
    const int N = a.N;
    int tpr = 1;
    while (tpr * SEG < N) tpr *= 2;                      // <= 64 for N <= 4096
    a.pitch = (N + 31) / 32 * 32 + 1;
    int nr = LT / tpr;
    while (nr > 1 && (long)nr * a.pitch * 4 > LDS_BUDGET) nr /= 2;
    int L = (N + tpr - 1) / tpr;
    if (nr < 32)                                         // a 32-lane group holds 32 / nr segments of nr lines: bank = line + segment * L mod 32
        while (L % 32 != nr % 32) ++L;
    a.TPR = tpr; a.NR = nr; a.L = L;
    a.logNR = 0;
    while ((1 << a.logNR) < nr) ++a.logNR;
}

template <typename TI>
int launch_lines(LineArgs& a, int nouter, hipStream_t s) {
    line_config(a);
    const size_t smem = (size_t)a.NR * a.pitch * sizeof(float);
    if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)nifti_lines_kernel<TI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    const dim3 grid((a.nrow + a.NR - 1) / a.NR, nouter), block(a.NR * a.TPR);
    hipLaunchKernelGGL(nifti_lines_kernel<TI>, grid, block, smem, s, a);
    return rs_check_launch();
}

constexpr int BT = 256, TOX = 64, TOY = 16, BROWS = 64;

struct BsArgs {
    const float* coef;
    const int *ix, *iy, *iz;
    const float *wx, *wy;
    float* out;
    int Z, Y, X, Zo, Yo, Xo;
    float outside;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(BT) void bspline_resample_kernel(BsArgs a) {
    __shared__ float T[BROWS][TOX];
    __shared__ int yr[2];
    const int t = threadIdx.x, tx = t & (TOX - 1), ty = t / TOX;
    const int ox = blockIdx.x * TOX + tx, oy0 = blockIdx.y * TOY, zo = blockIdx.z;
    int zs = a.iz[zo];
    if (zs >= 0 && zo > 0 && a.iz[zo - 1] == zs) return;                 // the block of the first slice of a run writes the whole run
    int nrep = 1;
    if (zs >= 0)
        while (zo + nrep < a.Zo && a.iz[zo + nrep] == zs) ++nrep;
    if (zs < 0) {
        for (int oyl = ty; oyl < TOY; oyl += BT / TOX) {
            const int oy = oy0 + oyl;
            if (oy < a.Yo && ox < a.Xo) a.out[((long)zo * a.Yo + oy) * a.Xo + ox] = a.outside;
        }
        return;
    }
    zs = zs < a.Z ? zs : a.Z - 1;
    const bool xin = ox < a.Xo && a.ix[4 * ox] >= 0;
    int xi[4] = {0, 0, 0, 0};
    float xw[4] = {0.f, 0.f, 0.f, 0.f};
    if (xin) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { xi[i] = clampi(a.ix[4 * ox + i], a.X - 1); xw[i] = a.wx[4 * ox + i]; }
    }
    if (t == 0) { yr[0] = 0x7fffffff; yr[1] = -1; }
    __syncthreads();
    if (t < TOY * 4) {
        const int oy = oy0 + t / 4;
        if (oy < a.Yo && a.iy[4 * oy] >= 0) {
            const int v = clampi(a.iy[4 * oy + (t & 3)], a.Y - 1);
            atomicMin(&yr[0], v);
            atomicMax(&yr[1], v);
        }
    }
    __syncthreads();
    const int ymin = yr[0], nrows = yr[1] < 0 ? 0 : yr[1] - ymin + 1;
    const bool lds = nrows <= BROWS;
    const float* __restrict__ plane = a.coef + (long)zs * a.Y * a.X;
    if (lds) {
        for (int row = ty; row < nrows; row += BT / TOX) {
            const float* __restrict__ p = plane + (long)(ymin + row) * a.X;
            T[row][tx] = xin ? xw[0] * p[xi[0]] + xw[1] * p[xi[1]] + xw[2] * p[xi[2]] + xw[3] * p[xi[3]] : 0.f;
        }
        __syncthreads();
    }
    for (int oyl = ty; oyl < TOY; oyl += BT / TOX) {
        const int oy = oy0 + oyl;
        if (oy >= a.Yo || ox >= a.Xo) continue;
        float v = a.outside;
        if (xin && a.iy[4 * oy] >= 0) {
            v = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = clampi(a.iy[4 * oy + j], a.Y - 1);
                float h;
                if (lds) h = T[yy - ymin][tx];
                else {
                    const float* __restrict__ p = plane + (long)yy * a.X;
                    h = xw[0] * p[xi[0]] + xw[1] * p[xi[1]] + xw[2] * p[xi[2]] + xw[3] * p[xi[3]];
                }
                v += a.wy[4 * oy + j] * h;
            }
        }
        for (int rep = 0; rep < nrep; ++rep) a.out[((long)(zo + rep) * a.Yo + oy) * a.Xo + ox] = v;
    }
}

struct RoArgs {
    const uint8_t* src;
    uint8_t* dst;
    long plane_stride, ci, cj, ck, coff, nvox;
    int ni, nj, nk, vec;
};

__global__ __launch_bounds__(256) void reorient_store_kernel(RoArgs a) {
    const uint8_t* __restrict__ src = a.src + (long)blockIdx.y * a.nvox;
    uint8_t* __restrict__ dst = a.dst + (long)blockIdx.y * a.plane_stride;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long f = a.vec ? 4 * g : g;
    if (f >= a.nvox) return;
    const int i = (int)(f % a.ni);
    const long q = f / a.ni;
    const int j = (int)(q % a.nj), k = (int)(q / a.nj);
    const long s = a.coff + i * a.ci + j * a.cj + k * a.ck;
    if (a.vec) {
        const uint32_t w = (uint32_t)src[s] | (uint32_t)src[s + a.ci] << 8 | (uint32_t)src[s + 2 * a.ci] << 16 | (uint32_t)src[s + 3 * a.ci] << 24;
        *reinterpret_cast<uint32_t*>(dst + f) = w;
    } else {
        dst[f] = src[s];
    }
}

// [lo, hi] of off + a * sa + b * sb + c * sc over 0 <= a < na, ...
void index_range(long off, long sa, int na, long sb, int nb, long sc, int nc, long& lo, long& hi) {
    lo = hi = off;
    const long s[3] = {sa, sb, sc};
    const int n[3] = {na, nb, nc};
    for (int d = 0; d < 3; ++d) {
        const long span = s[d] * (n[d] - 1);
        if (span < 0) lo += span; else hi += span;
    }
}

long labs_(long v) { return v < 0 ? -v : v; }

}  // namespace

extern "C" {

int rsuper_nifti_load_prefilter(const void* src, int dtype, long n_src, int Z, int Y, int X, long sz, long sy, long sx, long offset, float slope,
                                float inter, int prefilter, float* out, void* stream) {
    static const int esz[6] = {1, 1, 2, 2, 4, 4};
    if (!src || !out || (const void*)out == src || dtype < 0 || dtype > RSUPER_NII_F32 || Z < 1 || Y < 1 || X < 1 || n_src < 1) return RS_ERR_ARG;
    if (Z > MAX_SIDE || Y > MAX_SIDE || X > MAX_SIDE) return RS_ERR_UNSUPPORTED;
    if ((uintptr_t)src % esz[dtype] || (uintptr_t)out % 4 || (long)Z * Y * X > n_src) return RS_ERR_ARG;
    long lo, hi;
    index_range(offset, sz, Z, sy, Y, sx, X, lo, hi);
    if (lo < 0 || hi >= n_src) return RS_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    LineArgs a{};
    a.src = src; a.dst = out; a.s_off = offset; a.s_line = sx;
    a.N = X; a.prefilter = prefilter ? 1 : 0;
    a.scale = (slope != 1.f || inter != 0.f) ? 1 : 0; a.slope = slope; a.inter = inter;
    a.d_line = 1; a.dst_fast_rows = 0;
    int nouter;
    if (labs_(sz) == 1 && labs_(sx) != 1 && labs_(sy) != 1) {      // the file's fastest axis is canonical z: the rows of a block run along z
        a.s_row = sz; a.s_outer = sy; a.nrow = Z; nouter = Y; a.d_row = (long)Y * X; a.d_outer = X; a.src_fast_rows = 1;
    } else {
        a.s_row = sy; a.s_outer = sz; a.nrow = Y; nouter = Z; a.d_row = X; a.d_outer = (long)Y * X; a.src_fast_rows = labs_(sx) != 1 && labs_(sy) == 1;
    }
    int rc;
    switch (dtype) {
    case RSUPER_NII_U8: rc = launch_lines<uint8_t>(a, nouter, s); break;
    case RSUPER_NII_I8: rc = launch_lines<int8_t>(a, nouter, s); break;
    case RSUPER_NII_I16: rc = launch_lines<int16_t>(a, nouter, s); break;
    case RSUPER_NII_U16: rc = launch_lines<uint16_t>(a, nouter, s); break;
    case RSUPER_NII_I32: rc = launch_lines<int32_t>(a, nouter, s); break;
    default: rc = launch_lines<float>(a, nouter, s); break;
    }
    if (rc != RS_OK || !prefilter || Y == 1) return rc;
    LineArgs b{};                                        // pass 2: lines along y, in place
    b.src = out; b.dst = out; b.s_off = 0; b.s_line = X; b.s_row = 1; b.s_outer = (long)Y * X;
    b.d_line = X; b.d_row = 1; b.d_outer = (long)Y * X;
    b.N = Y; b.nrow = X; b.prefilter = 1; b.scale = 0; b.slope = 1.f; b.inter = 0.f;
    b.src_fast_rows = b.dst_fast_rows = 1;
    return launch_lines<float>(b, Z, s);
}

int rsuper_bspline_resample(const float* coef, int Z, int Y, int X, const int* ix, const float* wx, const int* iy, const float* wy, const int* iz,
                            float* out, int Zo, int Yo, int Xo, float outside_value, void* stream) {
    if (!coef || !ix || !wx || !iy || !wy || !iz || !out || out == coef || Z < 1 || Y < 1 || X < 1 || Zo < 1 || Yo < 1 || Xo < 1) return RS_ERR_ARG;
    if ((uintptr_t)coef % 4 || (uintptr_t)out % 4 || (uintptr_t)ix % 4 || (uintptr_t)iy % 4 || (uintptr_t)iz % 4 || (uintptr_t)wx % 4 || (uintptr_t)wy % 4)
        return RS_ERR_ARG;
    if (Z > MAX_SIDE || Y > MAX_SIDE || X > MAX_SIDE || Zo > 65535 || (Yo + TOY - 1) / TOY > 65535) return RS_ERR_UNSUPPORTED;
    BsArgs a{};
    a.coef = coef; a.ix = ix; a.iy = iy; a.iz = iz; a.wx = wx; a.wy = wy; a.out = out;
    a.Z = Z; a.Y = Y; a.X = X; a.Zo = Zo; a.Yo = Yo; a.Xo = Xo; a.outside = outside_value;
    const dim3 grid((Xo + TOX - 1) / TOX, (Yo + TOY - 1) / TOY, Zo), block(BT);
    hipLaunchKernelGGL(bspline_resample_kernel, grid, block, 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

int rsuper_reorient_store(const uint8_t* src, int C, int Z, int Y, int X, uint8_t* dst, long dst_bytes, long dst_offset, long plane_stride, int ni,
                          int nj, int nk, long ci, long cj, long ck, long coff, void* stream) {
    if (!src || !dst || C < 1 || C > 65535 || Z < 1 || Y < 1 || X < 1 || ni < 1 || nj < 1 || nk < 1 || dst_offset < 0) return RS_ERR_ARG;
    const long nvox = (long)Z * Y * X;
    if ((long)ni * nj * nk != nvox || nvox >= (1l << 31) || plane_stride < nvox) return RS_ERR_ARG;
    if (dst_offset + (C - 1) * plane_stride + nvox > dst_bytes) return RS_ERR_ARG;
    if (src + C * nvox > dst && dst + dst_bytes > src) return RS_ERR_ARG;             // overlapping buffers
    long lo, hi;
    index_range(coff, ci, ni, cj, nj, ck, nk, lo, hi);
    if (lo < 0 || hi >= nvox) return RS_ERR_ARG;
    RoArgs a{};
    a.src = src; a.dst = dst + dst_offset; a.plane_stride = plane_stride; a.ci = ci; a.cj = cj; a.ck = ck; a.coff = coff; a.nvox = nvox;
    a.ni = ni; a.nj = nj; a.nk = nk;
    a.vec = ni % 4 == 0 && (uintptr_t)a.dst % 4 == 0 && plane_stride % 4 == 0;
    const long items = a.vec ? nvox / 4 : nvox;
    const dim3 grid((unsigned)((items + 255) / 256), C), block(256);
    hipLaunchKernelGGL(reorient_store_kernel, grid, block, 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

}  // extern "C"
