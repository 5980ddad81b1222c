// Spatial augmentation of the loader (training/augmentation.py random_scale_rotate_translate_3d :228-319 followed by crop_3d 'center' :446-469):
// one affine resampling of an f32 image (trilinear, zero padding) and of up to three byte volumes (nearest, zero padding) that writes ONLY the
// output crop.  The byte volumes are the bit-packed label / unknown / segment volumes (np.packbits along the class axis: nearest resampling of 0/1
// planes is a gather of the packed bytes, 4 bytes per voxel for 26 classes) or plain u8 planes.
//
// Coordinates: the reference builds F.affine_grid(theta, (B, C, D, H, W), align_corners=True), g = theta . (x, y, z, 1) with x = -1 + 2 i / (W - 1)
// (likewise y over H, z over D), and grid_sample un-normalises src = ((g + 1) / 2) (N - 1).  With c = i - (N - 1) / 2 (exact in f64) that is
//     src_r = sum_c theta[r][c] * ((N_r - 1) / (N_c - 1)) * c_c  +  (theta[r][3] + 1) * (N_r - 1) / 2
// which is evaluated here in f64 -- the same value up to f64 rounding, and for an identity theta exactly the integer index, so an identity launch
// is a plain copy bit for bit.  i is the index on the FULL D x H x W grid: the crop offset shifts the output indices, it does not re-centre.
// Nearest = rint (half to even, as nearbyint); trilinear weights are the f64 fractions rounded to f32, the 8 corners tested for bounds one by one.
//
// One block = one 4 x 8 x 32 output brick of one sample, one lane = 4 consecutive voxels along w: the image goes out as one 16-byte store per lane
// and channel (128 contiguous bytes per brick row), every byte plane as one dword.  The coordinate is computed once per voxel and shared by the
// image and all byte planes.  Bricks are numbered so that the blocks one XCD receives (block index mod 8) form a contiguous run of bricks: the
// source footprint of a run is a slab of the volume that stays in that XCD's L2.  No atomics, no workspace, no memset.
#include "common.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int NT = 256;
constexpr int BZ = 4, BY = 8, BX = 32, VX = 4;          // brick extents; voxels per lane along w.  (BX / VX) * BY * BZ == NT
constexpr int MAXV = RSUPER_AFFINE_MAX_VOLUMES, MAXP = RSUPER_AFFINE_MAX_PLANES, MAXB = 8;
constexpr int XCDS = 8;
static_assert((BX / VX) * BY * BZ == NT, "one lane per 4-voxel group of the brick");

struct AffineArgs {
    const float* theta;                                  // [B][3][4]
    const float* img;                                    // [B][Ci][D][H][W]
    float* img_out;                                      // [B][Ci][d][h][w]
    const uint8_t* vol[MAXV];                            // [B][P][D][H][W]
    uint8_t* vol_out[MAXV];                              // [B][P][d][h][w]
    int planes[MAXV];
    int nvol, Ci, D, H, W, d, h, w;
    int off[MAXB][3];                                    // per sample of this launch: z, y, x of the crop on the full grid
    int nbx, nby, nbricks, chunk;
    int vec;                                             // w % 4 == 0 and every output base is 16-byte aligned: vector stores
};

struct Coord {                                           // one output voxel's source position
    int n;                                               // nearest voxel's linear index, -1 when out of bounds
    int x0, y0, z0;                                      // floor corner (clamped to [-2, N]: anything outside has no corner in bounds)
    float fx, fy, fz;                                    // fractions
};

__device__ __forceinline__ void axis(double s, int N, int& i0, float& f, int& nn) {
    const double fl = fmin(fmax(floor(s), -2.0), (double)N);          // NaN -> -2: no corner in bounds
    i0 = (int)fl;
    f = (float)(s - fl);
    const double r = rint(s);
    nn = (r >= 0.0 && r <= (double)(N - 1)) ? (int)r : -1;
}

__global__ __launch_bounds__(NT) void affine_crop_kernel(AffineArgs a) {
    // brick of this block: XCD x (= blockIdx.x % 8, the dispatcher's round-robin) works through bricks [x * chunk, (x + 1) * chunk)
    const int brick = (blockIdx.x % XCDS) * a.chunk + blockIdx.x / XCDS;
    if (brick >= a.nbricks) return;
    const int b = blockIdx.y;
    const int bx = brick % a.nbx, t = brick / a.nbx, by = t % a.nby, bz = t / a.nby;
    const int lane = threadIdx.x;
    const int ox = bx * BX + (lane & (BX / VX - 1)) * VX, oy = by * BY + ((lane / (BX / VX)) & (BY - 1)), oz = bz * BZ + lane / (BX / VX * BY);
    if (ox >= a.w || oy >= a.h || oz >= a.d) return;

    const int D = a.D, H = a.H, W = a.W;
    const int n[3] = {W, H, D};
    const float* th = a.theta + (long)b * 12;
    double A[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = (double)th[r * 4 + c] * ((double)(n[r] - 1) / (double)(n[c] - 1));
        A[r][3] = ((double)th[r * 4 + 3] + 1.0) * (0.5 * (double)(n[r] - 1));
    }
    const double cy = (double)(oy + a.off[b][1]) - 0.5 * (double)(H - 1), cz = (double)(oz + a.off[b][0]) - 0.5 * (double)(D - 1);
    double row[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) row[r] = fma(A[r][1], cy, fma(A[r][2], cz, A[r][3]));

    Coord c[VX];
#pragma unroll
    for (int j = 0; j < VX; ++j) {
        const double cx = (double)(ox + j + a.off[b][2]) - 0.5 * (double)(W - 1);
        int nx, ny, nz;
        axis(fma(A[0][0], cx, row[0]), W, c[j].x0, c[j].fx, nx);
        axis(fma(A[1][0], cx, row[1]), H, c[j].y0, c[j].fy, ny);
        axis(fma(A[2][0], cx, row[2]), D, c[j].z0, c[j].fz, nz);
        c[j].n = (nx >= 0 && ny >= 0 && nz >= 0) ? (nz * H + ny) * W + nx : -1;
    }
    const long V = (long)D * H * W, v = (long)a.d * a.h * a.w;
    const long o = ((long)oz * a.h + oy) * a.w + ox;     // first of the lane's voxels inside an output plane
    const int nv = a.w - ox < VX ? a.w - ox : VX;        // voxels of this lane inside the crop (ragged last group)

    // ---- image: trilinear, zero padding
    for (int ch = 0; ch < a.Ci; ++ch) {
        const float* __restrict__ s = a.img + ((long)b * a.Ci + ch) * V;
        float r[VX];
#pragma unroll
        for (int j = 0; j < VX; ++j) {
            const int x0 = c[j].x0, y0 = c[j].y0, z0 = c[j].z0;
            const float wx[2] = {1.f - c[j].fx, c[j].fx}, wy[2] = {1.f - c[j].fy, c[j].fy}, wz[2] = {1.f - c[j].fz, c[j].fz};
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
                const int x = x0 + dx, y = y0 + dy, z = z0 + dz;
                const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && (unsigned)z < (unsigned)D;
                const float val = in ? s[((long)z * H + y) * W + x] : 0.f;
                acc = in ? fmaf(val, wz[dz] * wy[dy] * wx[dx], acc) : acc;   // a corner out of bounds adds nothing, whatever its weight
            }
            r[j] = acc;
        }
        float* __restrict__ q = a.img_out + ((long)b * a.Ci + ch) * v + o;
        if (a.vec) *reinterpret_cast<float4*>(q) = make_float4(r[0], r[1], r[2], r[3]);
        else
#pragma unroll
            for (int j = 0; j < VX; ++j)
                if (j < nv) q[j] = r[j];
    }

    // ---- byte volumes: nearest, zero padding
    for (int k = 0; k < a.nvol; ++k) {
        const int P = a.planes[k];
        const uint8_t* __restrict__ s = a.vol[k] + (long)b * P * V;
        uint8_t* __restrict__ q = a.vol_out[k] + (long)b * P * v + o;
        for (int p = 0; p < P; ++p, s += V, q += v) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < VX; ++j) word |= (uint32_t)(c[j].n >= 0 ? s[c[j].n] : (uint8_t)0) << (8 * j);
            if (a.vec) *reinterpret_cast<uint32_t*>(q) = word;
            else
#pragma unroll
                for (int j = 0; j < VX; ++j)
                    if (j < nv) q[j] = (uint8_t)(word >> (8 * j));
        }
    }
}

}  // namespace

extern "C" {

int rsuper_affine_crop(const float* theta, const float* img, float* img_out, int B, int Ci, int D, int H, int W, int nvol,
                       const uint8_t* const* vols, uint8_t* const* vols_out, const int* planes, int d, int h, int w, const int* offsets,
                       void* stream) {
    if (!theta || !img || !img_out || !offsets || B < 1 || B > 65535 || Ci < 1 || nvol < 0 || nvol > MAXV) return RS_ERR_ARG;
    if (nvol > 0 && (!vols || !vols_out || !planes)) return RS_ERR_ARG;
    if (D < 2 || H < 2 || W < 2 || (long)D * H * W >= (1l << 31)) return RS_ERR_ARG;   // N == 1 has no align-corners coordinate (division by N - 1)
    if (d < 1 || h < 1 || w < 1 || d > D || h > H || w > W) return RS_ERR_ARG;
    for (int b = 0; b < B; ++b) {
        const int* f = offsets + 3 * b;
        if (f[0] < 0 || f[1] < 0 || f[2] < 0 || f[0] > D - d || f[1] > H - h || f[2] > W - w) return RS_ERR_ARG;
    }
    AffineArgs a{};
    a.vec = (w % 4 == 0) && ((uintptr_t)img_out % 16 == 0);
    for (int k = 0; k < nvol; ++k) {
        if (!vols[k] || !vols_out[k] || planes[k] < 1 || planes[k] > MAXP) return RS_ERR_ARG;
        a.vol[k] = vols[k];
        a.vol_out[k] = vols_out[k];
        a.planes[k] = planes[k];
        a.vec = a.vec && ((uintptr_t)vols_out[k] % 4 == 0);
    }
    a.nvol = nvol; a.Ci = Ci; a.D = D; a.H = H; a.W = W; a.d = d; a.h = h; a.w = w;
    a.nbx = (w + BX - 1) / BX;
    a.nby = (h + BY - 1) / BY;
    a.nbricks = a.nbx * a.nby * ((d + BZ - 1) / BZ);
    a.chunk = (a.nbricks + XCDS - 1) / XCDS;
    const long V = (long)D * H * W, v = (long)d * h * w;
    for (int b0 = 0; b0 < B; b0 += MAXB) {               // the per-sample offsets travel in the kernel arguments, MAXB samples per launch
        const int nb = B - b0 < MAXB ? B - b0 : MAXB;
        a.theta = theta + (long)b0 * 12;
        a.img = img + (long)b0 * Ci * V;
        a.img_out = img_out + (long)b0 * Ci * v;
        for (int k = 0; k < nvol; ++k) {
            a.vol[k] = vols[k] + (long)b0 * planes[k] * V;
            a.vol_out[k] = vols_out[k] + (long)b0 * planes[k] * v;
        }
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < 3; ++i) a.off[b][i] = offsets[3 * (b0 + b) + i];
        hipLaunchKernelGGL(affine_crop_kernel, dim3(a.chunk * XCDS, nb), dim3(NT), 0, (hipStream_t)stream, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

}  // extern "C"
