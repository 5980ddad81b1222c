// Crop-on-tumour from a whole CT whose label is still bit-packed (training/augmentation.py random_crop_on_tumor :600, negative_crop :662, organ_crop :675,
// tumor_crop :716, crop_around_coordinate_3d :498, pad_volume_pair :1023).  The reference inflates the label, sums class planes and calls torch.nonzero
// on a whole-CT plane to pick one voxel; here presence and counts are popcounts over the packed bytes, the chosen voxel is "the k-th set bit of column
// c in row-major order", and the crop is a box copy of the image and of the packed byte planes.
//
// class_counts   packed [B][P][V] u8, read chunk by chunk (layout, chunks, head and tail: label_bits.hpp).  Block (chunk, b) writes ONE row of the chunk
//                table [B][chunks][C + 1] int32: the set voxels of every class and, in column C, the voxels whose P bytes are all zero
//                (label.sum(0) == 0: packbits zero-fills the padding bits).  Counting: __popc of the dword under the class's bit replicated into its
//                4 bytes; the OR of the planes stays in registers for the background column.  A second launch sums the rows into [B][C + 1] int64.
//                Every entry is written, nothing is accumulated in memory: no memset, no atomics, the same bits on every run.  plain: the label is
//                [B][C][V] bytes, class c = plane c, a voxel is set where its byte is not zero (the u8 / int64 labels of the reference's own
//                functions); same table.
// select_voxel   one block.  Prefix sums of column c over the table find the chunk that holds rank k; inside it every lane builds the 64-bit mask of
//                its 64 consecutive voxels, the popcounts are prefix-summed over the lanes, and the lane that holds the rank clears that many low bits.
//                Lanes own consecutive voxels, so the order is row-major: (z, y, x) = torch.nonzero(mask)[k].  Reads stay inside the chunk whatever
//                the table holds; a rank the table does not reach writes (-1, -1, -1) (the host has already refused k >= count).
// crop_box       one launch: f32 or int16 image -> f32 crop, up to three byte volumes -> byte crops, all of (d, h, w).  The source counts as zero-padded
//                symmetrically to (max(D, pd), max(H, ph), max(W, pw)) with pad // 2 on the low side (pad_volume_pair); the padded copy is never made:
//                a voxel whose source coordinate falls outside the real volume is written as 0.  The origin is a kernel argument per sample or, with a
//                device centre, clip(centre - crop // 2 + offset, 0, padded size - crop) (crop_around_coordinate_3d 'small_rnd_shift' :523-542); the one
//                used is written to origin_out.  One lane = 4 consecutive voxels along w: one 16-byte store per image channel and one dword per byte
//                plane when w % 4 == 0, voxel by voxel otherwise; 4 source voxels inside one row are one (possibly unaligned) load.
#include "common.hpp"
#include "label_bits.hpp"

namespace {

constexpr int NT = LB_NT;
constexpr int CHUNK = LB_CHUNK;
constexpr int LPV = CHUNK / NT;                          // voxels per lane of the selection: 64
constexpr int CP = RSUPER_CROP_MAX_CLASSES / 8;          // bit-packed byte planes the counting kernel takes
constexpr int MAXV = RSUPER_AFFINE_MAX_VOLUMES, MAXPL = RSUPER_AFFINE_MAX_PLANES, MAXB = 8;
static_assert(LPV == 64, "a lane of the selection owns one 64-bit mask");
static_assert(RSUPER_CROP_MAX_CLASSES + 1 <= NT, "one lane per column of a table row");

struct CountArgs {
    const uint8_t* packed;                               // [B][P][V]
    int* table;                                          // [B][nchunks][C + 1]
    long V;
    int P, C, nchunks, plain;                            // plain: P == C planes of 0 / non-zero bytes instead of bit planes
};

__global__ __launch_bounds__(NT) void class_counts_kernel(CountArgs a) {
    __shared__ int sh[RSUPER_CROP_MAX_CLASSES][NT / 64];
    __shared__ int shnz[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LabelChunk ck(a.packed + (long)blockIdx.y * a.P * a.V, a.V, blockIdx.x, tid);

    uint4 any[LB_VPL];
    uint32_t anys = 0;
#pragma unroll
    for (int v = 0; v < LB_VPL; ++v) any[v] = make_uint4(0, 0, 0, 0);

    for (int p = 0; p < a.P; ++p) {
        int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto take = [&](uint32_t w) {
            if (a.plain) acc[0] += __popc(nonzero_bytes(w));
            else
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += __popc(w & (0x01010101u << class_bit(j)));
        };
        ck.for_each(p,
            [&](int v, const uint4 q) {
                any[v].x |= q.x; any[v].y |= q.y; any[v].z |= q.z; any[v].w |= q.w;
                take(q.x); take(q.y); take(q.z); take(q.w);
            },
            [&](uint32_t w) { anys |= w; take(w); });
        // a lane holds at most 16 * LB_VPL + 1 voxels and a wave 64 times that: two counts share a dword through the wave reduction
        uint32_t pk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pk[i] = (uint32_t)acc[2 * i] | (uint32_t)acc[2 * i + 1] << 16;
        wave_reduce_all<RedSum, RedSum, RedSum, RedSum>(pk[0], pk[1], pk[2], pk[3]);
        if (lane == 0) {
            if (a.plain) sh[p][wave] = (int)(pk[0] & 0xffffu);
            else
#pragma unroll
                for (int i = 0; i < 4; ++i) { sh[p * 8 + 2 * i][wave] = (int)(pk[i] & 0xffffu); sh[p * 8 + 2 * i + 1][wave] = (int)(pk[i] >> 16); }
        }
    }
    int nz = __popc(nonzero_bytes(anys));
#pragma unroll
    for (int v = 0; v < LB_VPL; ++v)
        nz += __popc(nonzero_bytes(any[v].x)) + __popc(nonzero_bytes(any[v].y)) + __popc(nonzero_bytes(any[v].z)) + __popc(nonzero_bytes(any[v].w));
    block_stage<RedSum>(nz, shnz);
    __syncthreads();
    int* __restrict__ row = a.table + ((long)blockIdx.y * a.nchunks + blockIdx.x) * (a.C + 1);
    if (tid < a.C) row[tid] = block_finish<RedSum>(sh[tid]);
    else if (tid == a.C) row[tid] = ck.len - block_finish<RedSum>(shnz);
}

// block (column, b): the column's sum over the chunk rows
__global__ __launch_bounds__(NT) void class_totals_kernel(const int* __restrict__ table, long long* __restrict__ totals, int nchunks, int cols) {
    __shared__ long long shw[NT / 64];
    const int tid = threadIdx.x, col = blockIdx.x, b = blockIdx.y;
    const int* __restrict__ t = table + (long)b * nchunks * cols + col;
    long long s = 0;
    for (int j = tid; j < nchunks; j += NT) s += t[(long)j * cols];
    block_stage<RedSum>(s, shw);
    __syncthreads();
    if (tid == 0) totals[(long)b * cols + col] = block_finish<RedSum>(shw);
}

struct SelArgs {
    const uint8_t* packed;                               // [P][V] of the sample
    const int* table;                                    // [nchunks][C + 1] of the sample
    int* out;                                            // (z, y, x)
    long V, k;
    int P, C, nchunks, col, H, W, plain, add[3];
};

__global__ __launch_bounds__(NT) void select_voxel_kernel(SelArgs a) {
    __shared__ long long run[NT];
    __shared__ int cnt[NT];
    __shared__ int found[3];                             // chunk, rank inside the chunk; then lane, rank inside the lane's mask
    const int tid = threadIdx.x, cols = a.C + 1;
    const int* __restrict__ t = a.table + a.col;
    const int per = (a.nchunks + NT - 1) / NT;
    const int j0 = tid * per < a.nchunks ? tid * per : a.nchunks, j1 = j0 + per < a.nchunks ? j0 + per : a.nchunks;
    long long s = 0;
    for (int j = j0; j < j1; ++j) s += t[(long)j * cols];
    run[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long rem = a.k;
        int T = 0;
        while (T < NT && rem >= run[T]) rem -= run[T++];
        int j = -1;
        if (T < NT && rem >= 0) {
            const int e = (T + 1) * per < a.nchunks ? (T + 1) * per : a.nchunks;
            j = T * per;
            while (j < e && rem >= t[(long)j * cols]) rem -= t[(long)j * cols], ++j;
            if (j >= e) j = -1;
        }
        found[0] = j; found[1] = (int)rem;
    }
    __syncthreads();
    const int chunk = found[0];
    if (chunk < 0) {                                     // the same answer in every lane
        if (tid < 3) a.out[tid] = -1;
        return;
    }
    const long start = (long)chunk * CHUNK;
    const int len = a.V - start < CHUNK ? (int)(a.V - start) : CHUNK;
    const int off = tid * LPV, nvalid = len - off < 0 ? 0 : len - off > LPV ? LPV : len - off;
    unsigned long long mask = 0;
    const bool background = a.col == a.C;
    const int p0 = background ? 0 : a.plain ? a.col : a.col >> 3, p1 = background ? a.P : p0 + 1;
    const int shift = class_bit(a.col);
    for (int q = 0; q < LPV / 16; ++q) {
        if (q * 16 >= nvalid) break;
        uint32_t f[4] = {0, 0, 0, 0};                    // bit 0 of byte i = voxel 4 * word + i has a bit in the column's planes
        for (int p = p0; p < p1; ++p) {
            const uint8_t* __restrict__ sp = a.packed + (long)p * a.V + start + off + q * 16;
            uint32_t w[4] = {0, 0, 0, 0};
            if (q * 16 + 16 <= nvalid) {
                const uint4 v = ld16(sp, false);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
                for (int i = 0; i < nvalid - q * 16; ++i) w[i >> 2] |= (uint32_t)sp[i] << (8 * (i & 3));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) f[i] |= background || a.plain ? nonzero_bytes(w[i]) : (w[i] >> shift) & 0x01010101u;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t sel = background ? f[i] ^ 0x01010101u : f[i];
            mask |= (unsigned long long)fold_nibble(sel) << (q * 16 + i * 4);
        }
    }
    if (nvalid < LPV) mask &= (1ull << nvalid) - 1ull;   // voxels past the volume's end are nobody's
    cnt[tid] = __popcll(mask);
    __syncthreads();
    if (tid == 0) {
        int rem = found[1], T = 0;
        while (T < NT && rem >= cnt[T]) rem -= cnt[T++];
        found[0] = T < NT ? T : -1; found[2] = rem;
    }
    __syncthreads();
    if (found[0] < 0) {
        if (tid < 3) a.out[tid] = -1;
        return;
    }
    if (tid == found[0]) {
        for (int i = found[2]; i > 0; --i) mask &= mask - 1ull;
        const long vox = start + off + __ffsll((long long)mask) - 1;
        const long hw = (long)a.H * a.W;
        a.out[0] = (int)(vox / hw) + a.add[0];
        a.out[1] = (int)(vox % hw / a.W) + a.add[1];
        a.out[2] = (int)(vox % a.W) + a.add[2];
    }
}

struct BoxArgs {
    const void* img;                                     // [B][Ci][D][H][W]
    float* img_out;                                      // [B][Ci][d][h][w]
    const uint8_t* vol[MAXV];
    uint8_t* vol_out[MAXV];
    int planes[MAXV];
    const int* center;                                   // device [B][3] in padded coordinates, or null
    int* origin_out;                                     // device [B][3], or null
    int nvol, Ci, D, H, W, d, h, w;
    int size[3], lo[3];                                  // the padded extents and the padding on the low side
    int org[MAXB][3];                                    // per sample of this launch: the origin, or the offset added to the centred corner
    int groups, vec;
    long items;                                          // d * h * groups
};

template <typename T>
__global__ __launch_bounds__(NT) void crop_box_kernel(BoxArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int crop[3] = {a.d, a.h, a.w};
    int o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        long c = a.org[b][i];
        if (a.center) {
            c += (long)a.center[b * 3 + i] - crop[i] / 2;
            const long hi = a.size[i] - crop[i];
            c = c < 0 ? 0 : c > hi ? hi : c;
        }
        o[i] = (int)c;
    }
    if (a.origin_out && blockIdx.x == 0 && tid < 3) a.origin_out[b * 3 + tid] = tid == 0 ? o[0] : tid == 1 ? o[1] : o[2];
    const long item = (long)blockIdx.x * NT + tid;
    if (item >= a.items) return;
    const int g = (int)(item % a.groups), r = (int)(item / a.groups);
    const int ox = g * 4, oy = r % a.h, oz = r / a.h;
    const int sz = oz + o[0] - a.lo[0], sy = oy + o[1] - a.lo[1], sx = ox + o[2] - a.lo[2];
    const bool rowok = (unsigned)sz < (unsigned)a.D && (unsigned)sy < (unsigned)a.H;
    const bool whole = rowok && sx >= 0 && sx + 3 < a.W;                 // 4 source voxels inside one row
    const int nv = a.w - ox < 4 ? a.w - ox : 4;
    const long V = (long)a.D * a.H * a.W, v = (long)a.d * a.h * a.w;
    const long so = rowok ? ((long)sz * a.H + sy) * a.W + sx : 0, oo = ((long)oz * a.h + oy) * a.w + ox;

    for (int ch = 0; ch < a.Ci; ++ch) {
        const T* __restrict__ s = (const T*)a.img + ((long)b * a.Ci + ch) * V + so;
        float val[4];
        if (whole) {
            T raw[4];
            __builtin_memcpy(raw, s, sizeof(raw));
#pragma unroll
            for (int j = 0; j < 4; ++j) val[j] = (float)raw[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) val[j] = rowok && (unsigned)(sx + j) < (unsigned)a.W ? (float)s[j] : 0.f;
        }
        float* __restrict__ q = a.img_out + ((long)b * a.Ci + ch) * v + oo;
        if (a.vec) *reinterpret_cast<float4*>(q) = make_float4(val[0], val[1], val[2], val[3]);
        else
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) q[j] = val[j];
    }
    for (int k = 0; k < a.nvol; ++k) {
        const int P = a.planes[k];
        const uint8_t* __restrict__ s = a.vol[k] + (long)b * P * V + so;
        uint8_t* __restrict__ q = a.vol_out[k] + (long)b * P * v + oo;
        for (int p = 0; p < P; ++p, s += V, q += v) {
            uint32_t word = 0;
            if (whole) __builtin_memcpy(&word, s, 4);
            else
#pragma unroll
                for (int j = 0; j < 4; ++j) word |= (uint32_t)(rowok && (unsigned)(sx + j) < (unsigned)a.W ? s[j] : (uint8_t)0) << (8 * j);
            if (a.vec) *reinterpret_cast<uint32_t*>(q) = word;
            else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nv) q[j] = (uint8_t)(word >> (8 * j));
        }
    }
}

long chunks_of(long V) { return (V + CHUNK - 1) / CHUNK; }

bool counts_shape_ok(int B, int P, int C, int plain, int D, int H, int W) {
    if (B < 1 || B > 65535 || C < 1 || C > RSUPER_CROP_MAX_CLASSES || D < 1 || H < 1 || W < 1) return false;
    if (plain ? P != C : (P < (C + 7) / 8 || P > CP)) return false;
    return (long)D * H * W < (1l << 31);
}

}  // namespace

extern "C" {

long rsuper_class_counts_workspace_bytes(int B, int C, int D, int H, int W) {
    if (B < 1 || C < 1 || D < 1 || H < 1 || W < 1) return 0;
    return (long)B * chunks_of((long)D * H * W) * (C + 1) * (long)sizeof(int);
}

int rsuper_class_counts(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, void* workspace, long workspace_bytes, long long* totals,
                        void* stream) {
    if (!packed || !workspace || !totals || !counts_shape_ok(B, P, C, plain, D, H, W)) return RS_ERR_ARG;
    if (workspace_bytes < rsuper_class_counts_workspace_bytes(B, C, D, H, W) || (uintptr_t)workspace % 4 || (uintptr_t)totals % 8) return RS_ERR_ARG;
    CountArgs a{};
    a.packed = packed; a.table = (int*)workspace; a.V = (long)D * H * W; a.P = P; a.C = C; a.plain = plain ? 1 : 0; a.nchunks = (int)chunks_of(a.V);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(class_counts_kernel, dim3(a.nchunks, B), dim3(NT), 0, s, a);
    if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    hipLaunchKernelGGL(class_totals_kernel, dim3(C + 1, B), dim3(NT), 0, s, (const int*)workspace, totals, a.nchunks, C + 1);
    return rs_check_launch();
}

int rsuper_select_voxel(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, const void* workspace, long workspace_bytes, int b, int column,
                        long k, long count, int add_z, int add_y, int add_x, int* zyx, void* stream) {
    if (!packed || !workspace || !zyx || !counts_shape_ok(B, P, C, plain, D, H, W) || (uintptr_t)zyx % 4 || (uintptr_t)workspace % 4) return RS_ERR_ARG;
    if (workspace_bytes < rsuper_class_counts_workspace_bytes(B, C, D, H, W)) return RS_ERR_ARG;
    if (b < 0 || b >= B || column < 0 || column > C) return RS_ERR_ARG;
    const long V = (long)D * H * W;
    if (count < 0 || count > V || k < 0 || k >= count) return RS_ERR_ARG;        // the rank is checked against the totals the caller read
    SelArgs a{};
    a.nchunks = (int)chunks_of(V);
    a.packed = packed + (long)b * P * V;
    a.table = (const int*)workspace + (long)b * a.nchunks * (C + 1);
    a.out = zyx; a.V = V; a.k = k; a.P = P; a.C = C; a.plain = plain ? 1 : 0; a.col = column; a.H = H; a.W = W;
    a.add[0] = add_z; a.add[1] = add_y; a.add[2] = add_x;
    hipLaunchKernelGGL(select_voxel_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

int rsuper_crop_box(const void* img, int img_dtype, float* img_out, int B, int Ci, int D, int H, int W, int nvol, const uint8_t* const* vols,
                    uint8_t* const* vols_out, const int* planes, int d, int h, int w, int pad_d, int pad_h, int pad_w, const int* center,
                    const int* origin, int* origin_out, void* stream) {
    if (!origin || B < 1 || B > 65535 || Ci < 0 || nvol < 0 || nvol > MAXV || (Ci == 0 && nvol == 0)) return RS_ERR_ARG;
    if (Ci > 0 && (!img || !img_out || (img_dtype != RSUPER_VOX_F32 && img_dtype != RSUPER_VOX_I16))) return RS_ERR_ARG;
    if (Ci > 0 && ((uintptr_t)img % (img_dtype == RSUPER_VOX_I16 ? 2 : 4) || (uintptr_t)img_out % 4)) return RS_ERR_ARG;
    if (nvol > 0 && (!vols || !vols_out || !planes)) return RS_ERR_ARG;
    if (D < 1 || H < 1 || W < 1 || (long)D * H * W >= (1l << 31) || d < 1 || h < 1 || w < 1 || (long)d * h * w >= (1l << 31)) return RS_ERR_ARG;
    if (pad_d < 0 || pad_h < 0 || pad_w < 0 || (center && (uintptr_t)center % 4) || (origin_out && (uintptr_t)origin_out % 4)) return RS_ERR_ARG;
    BoxArgs a{};
    const int src[3] = {D, H, W}, pad[3] = {pad_d, pad_h, pad_w}, crop[3] = {d, h, w};
    for (int i = 0; i < 3; ++i) {
        a.size[i] = src[i] > pad[i] ? src[i] : pad[i];
        a.lo[i] = (a.size[i] - src[i]) / 2;
        if (crop[i] > a.size[i]) return RS_ERR_ARG;
    }
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < 3; ++i) {
            const int f = origin[3 * b + i];
            if (center ? (f < -(1 << 24) || f > (1 << 24)) : (f < 0 || f > a.size[i] - crop[i])) return RS_ERR_ARG;
        }
    a.vec = w % 4 == 0 && (Ci == 0 || (uintptr_t)img_out % 16 == 0);
    for (int k = 0; k < nvol; ++k) {
        if (!vols[k] || !vols_out[k] || planes[k] < 1 || planes[k] > MAXPL) return RS_ERR_ARG;
        a.planes[k] = planes[k];
        a.vec = a.vec && (uintptr_t)vols_out[k] % 4 == 0;
    }
    a.nvol = nvol; a.Ci = Ci; a.D = D; a.H = H; a.W = W; a.d = d; a.h = h; a.w = w;
    a.groups = (w + 3) / 4;
    a.items = (long)d * h * a.groups;
    const long nblk = (a.items + NT - 1) / NT;
    if (nblk >= (1l << 31)) return RS_ERR_ARG;
    const long V = (long)D * H * W, v = (long)d * h * w, esz = img_dtype == RSUPER_VOX_I16 ? 2 : 4;
    for (int b0 = 0; b0 < B; b0 += MAXB) {               // the per-sample origins travel in the kernel arguments, MAXB samples per launch
        const int nb = B - b0 < MAXB ? B - b0 : MAXB;
        a.img = Ci ? (const char*)img + (long)b0 * Ci * V * esz : nullptr;
        a.img_out = Ci ? img_out + (long)b0 * Ci * v : nullptr;
        a.center = center ? center + 3 * b0 : nullptr;
        a.origin_out = origin_out ? origin_out + 3 * b0 : nullptr;
        for (int k = 0; k < nvol; ++k) {
            a.vol[k] = vols[k] + (long)b0 * planes[k] * V;
            a.vol_out[k] = vols_out[k] + (long)b0 * planes[k] * v;
        }
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < 3; ++i) a.org[b][i] = origin[3 * (b0 + b) + i];
        const dim3 grid((unsigned)nblk, nb), block(NT);
        if (img_dtype == RSUPER_VOX_I16 && Ci) hipLaunchKernelGGL(crop_box_kernel<short>, grid, block, 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(crop_box_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

}  // extern "C"
