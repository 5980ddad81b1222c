// The report-annotated branch of the whole-CT crop (dataset_abdomenatlas_UFO.py get_random_tumor_seg_mask :855, assign_labels :1154,
// get_chosen_segment_mask :808; training/augmentation.py crop_foreground_3d :790, denoise_mask :746) on a label that stays bit-packed.  The reference
// inflates the label, sums the chosen segment planes, calls torch.nonzero for six minima / maxima, runs scipy's erosions / dilations over the whole CT
// and stacks three more inflated volumes plane by plane.  Here:
//
// union_bbox     packed [B][P][V] u8 (layout and chunks: label_bits.hpp; plain: [B][C][V] bytes) and one HOST 64-bit class set per sample.  A voxel
//                is on where any class of the set is.  Block (chunk, b) reads its chunk of the planes the set touches and writes ONE row (count,
//                min z y x, max z y x) of the partial table; one div / mod pair per non-empty vector.  A second launch folds the rows in a fixed order into count [B] int64 and bbox [B][6]
//                int32.  No voxel -> min = (D, H, W), max = (-1, -1, -1).
// union_bits     the same union inside the sub-box (z0, y0, x0) + (nz, ny, nx) of sample b as bits [nz][ny][ceil(nx / 64)] u64: one wave per word, one
//                voxel per lane, one __ballot.  Bits past nx are zero.
// bits_open      binary_dilation(binary_erosion(m, iterations = r), iterations = r) & m, scipy's cross structure, border_value = 0: 2r passes over two
//                ping-pong bit volumes, one lane per word: AND (OR) of the word, its four row / plane neighbours and its two one-bit shifts, which
//                carry the neighbour word's edge bit; everything outside the box, the bits past nx of a row's last word included, reads as zero.  The last pass ANDs with m and writes the bits, the
//                [nz][ny][nx] u8 mask rsuper_largest_component takes and its block's partial row; one more launch folds the rows as above.
// label_remap    in [B][P_in][v] packed -> nvol <= 3 packed volumes out[k] [B][P_out][v]; output class j of volume k at a voxel =
//                (in_bits & masks[b][k][j]) != 0 || bit j of ones[b][k].  The HOST tables travel in the kernel arguments: one launch per 8 samples, or
//                per as many as fit RSUPER_REMAP_TABLE_WORDS.  One lane = 4 consecutive voxels, one dword per plane when v % 4 == 0.
//
// No hipMemsetAsync, no atomics; every output and workspace entry a later launch reads is written by an earlier launch of the same call.
#include "common.hpp"
#include "label_bits.hpp"

namespace {

constexpr int NT = LB_NT;
constexpr int CHUNK = LB_CHUNK;
constexpr int CP = RSUPER_CROP_MAX_CLASSES / 8;
constexpr int MAXB = 8, MAXV = 3, ROW = 8;               // samples per launch, remapped volumes, ints of a partial row
constexpr int TW = RSUPER_REMAP_TABLE_WORDS;
constexpr int BIG = 0x7fffffff;
typedef unsigned long long u64;

struct Box {
    int cnt, mn[3], mx[3];
    __device__ void init() { cnt = 0; mn[0] = mn[1] = mn[2] = BIG; mx[0] = mx[1] = mx[2] = -1; }
    __device__ void add(int z, int y, int x0, int x1) {
        mn[0] = min(mn[0], z); mx[0] = max(mx[0], z);
        mn[1] = min(mn[1], y); mx[1] = max(mx[1], y);
        mn[2] = min(mn[2], x0); mx[2] = max(mx[2], x1);
    }
};

// the block's box -> row[0..6] (count, min z y x, max z y x); every thread of the block calls it
__device__ void block_box(Box v, int* __restrict__ row) {
    __shared__ int sh[7][NT / 64];
    const int tid = threadIdx.x;
    int f[7] = {v.cnt, v.mn[0], v.mn[1], v.mn[2], v.mx[0], v.mx[1], v.mx[2]};
    wave_reduce_all<RedSum, RedMin, RedMin, RedMin, RedMax, RedMax, RedMax>(f[0], f[1], f[2], f[3], f[4], f[5], f[6]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int i = 0; i < 7; ++i) sh[i][tid >> 6] = f[i];
    __syncthreads();
    if (tid < 7) row[tid] = tid == 0 ? block_finish<RedSum>(sh[0]) : tid < 4 ? block_finish<RedMin>(sh[tid]) : block_finish<RedMax>(sh[tid]);
}

struct UnionArgs {
    const uint8_t* packed;                               // [nb][P][V]
    int* part;                                           // [nb][nchunks][ROW]
    long V;
    int P, plain, nchunks, H, W;
    u64 set[MAXB];
};

__global__ __launch_bounds__(NT) void union_bbox_kernel(UnionArgs a) {
    const int tid = threadIdx.x, b = blockIdx.y;
    const LabelChunk ck(a.packed + (long)b * a.P * a.V, a.V, blockIdx.x, tid);
    const u64 set = a.set[b];

    uint4 any[LB_VPL];
    uint32_t anys = 0;
#pragma unroll
    for (int v = 0; v < LB_VPL; ++v) any[v] = make_uint4(0, 0, 0, 0);
    for (int p = 0; p < a.P; ++p) {
        const uint32_t bm = plane_mask(set, p, a.plain);
        if (!bm) continue;                               // the same in every lane: a plane the set does not touch is not read
        const uint32_t rep = bm * 0x01010101u;
        ck.for_each(p,
            [&](int v, const uint4 q) { any[v].x |= q.x & rep; any[v].y |= q.y & rep; any[v].z |= q.z & rep; any[v].w |= q.w & rep; },
            [&](uint32_t w) { anys |= w & bm; });
    }

    Box box;
    box.init();
    const uint32_t HW = (uint32_t)a.H * (uint32_t)a.W, W = (uint32_t)a.W;
#pragma unroll
    for (int v = 0; v < LB_VPL; ++v) {
        const uint32_t m = fold_nibble(nonzero_bytes(any[v].x)) | fold_nibble(nonzero_bytes(any[v].y)) << 4 | fold_nibble(nonzero_bytes(any[v].z)) << 8 |
                           fold_nibble(nonzero_bytes(any[v].w)) << 12;
        if (!m) continue;
        const uint32_t lin = (uint32_t)(ck.start + ck.vec_off(v));             // V < 2^31
        const uint32_t z = lin / HW, r = lin - z * HW, y = r / W, x = r - y * W;
        const int lo = __ffs((int)m) - 1, hi = 31 - __clz((int)m);
        box.cnt += __popc(m);
        if (x + hi < W) box.add((int)z, (int)y, (int)x + lo, (int)x + hi);
        else
            for (int i = lo; i <= hi; ++i)
                if (m >> i & 1u) {
                    const uint32_t l = lin + i, zz = l / HW, rr = l - zz * HW, yy = rr / W, xx = rr - yy * W;
                    box.add((int)zz, (int)yy, (int)xx, (int)xx);
                }
    }
    if (ck.soff >= 0 && anys) {
        const uint32_t l = (uint32_t)(ck.start + ck.soff), zz = l / HW, rr = l - zz * HW, yy = rr / W, xx = rr - yy * W;
        box.cnt += 1;
        box.add((int)zz, (int)yy, (int)xx, (int)xx);
    }
    block_box(box, a.part + ((long)b * a.nchunks + blockIdx.x) * ROW);
}

// block b: the partial rows of sample b in a fixed order -> count[b], bbox[b][6]; no voxel: min = empty_min + add, max = add - 1
__global__ __launch_bounds__(NT) void fold_box_kernel(const int* __restrict__ part, int nrows, long long* __restrict__ count, int* __restrict__ bbox,
                                                      int ez, int ey, int ex, int az, int ay, int ax) {
    __shared__ long long shc[NT / 64];
    __shared__ int shb[6][NT / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int* __restrict__ t = part + (long)b * nrows * ROW;
    long long c = 0;
    int f[6] = {BIG, BIG, BIG, -1, -1, -1};
    for (int j = tid; j < nrows; j += NT) {
        const int* __restrict__ row = t + (long)j * ROW;
        if (row[0] == 0) continue;
        c += row[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) { f[i] = min(f[i], row[1 + i]); f[3 + i] = max(f[3 + i], row[4 + i]); }
    }
    wave_reduce_all<RedSum, RedMin, RedMin, RedMin, RedMax, RedMax, RedMax>(c, f[0], f[1], f[2], f[3], f[4], f[5]);
    if ((tid & 63) == 0) {
        shc[tid >> 6] = c;
#pragma unroll
        for (int i = 0; i < 6; ++i) shb[i][tid >> 6] = f[i];
    }
    __syncthreads();
    if (tid == 0) {
        c = block_finish<RedSum>(shc);
        const int e[3] = {ez, ey, ex}, ad[3] = {az, ay, ax};
        count[b] = c;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            bbox[b * 6 + i] = (c ? block_finish<RedMin>(shb[i]) : e[i]) + ad[i];
            bbox[b * 6 + 3 + i] = (c ? block_finish<RedMax>(shb[3 + i]) : -1) + ad[i];
        }
    }
}

struct BitsArgs {
    const uint8_t* packed;                               // [P][V] of the sample
    u64* bits;                                           // [nz][ny][nw]
    long V, nwords;
    int P, plain, H, W, z0, y0, x0, ny, nx, nw;
    u64 set;
};

__global__ __launch_bounds__(NT) void union_bits_kernel(BitsArgs a) {
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (wid >= a.nwords) return;                         // whole waves leave
    const int k = (int)(wid % a.nw);
    const long r = wid / a.nw;
    const int y = (int)(r % a.ny), z = (int)(r / a.ny), x = 64 * k + lane;
    bool on = false;
    if (x < a.nx) {
        const uint8_t* __restrict__ s = a.packed + ((long)(a.z0 + z) * a.H + (a.y0 + y)) * a.W + (a.x0 + x);
        for (int p = 0; p < a.P; ++p) {
            const uint32_t bm = plane_mask(a.set, p, a.plain);
            if (bm) on = on || (s[(long)p * a.V] & bm) != 0;
        }
    }
    const u64 word = __ballot(on);
    if (lane == 0) a.bits[wid] = word;
}

struct OpenArgs {
    const u64* src;                                      // the pass's input
    u64* dst;
    const u64* orig;                                     // last pass: m
    uint8_t* mask;                                       // last pass: [nz][ny][nx]
    int* part;                                           // last pass: [blocks][ROW]
    long nwords;
    int nz, ny, nx, nw;
};

// one cross step of the word at (z, y, k): ERODE ? AND : OR over the 7 neighbours, zero outside the box
template <bool ERODE>
__device__ __forceinline__ u64 cross_step(const OpenArgs& a, long idx, int z, int y, int k) {
    const u64* __restrict__ s = a.src;
    const long pl = (long)a.ny * a.nw;
    // bits past nx in a row's last word count as zero whatever the caller left there, and nothing grows past the box
    const u64 last = (a.nx & 63) ? (1ull << (a.nx & 63)) - 1ull : ~0ull;
    const u64 own = k == a.nw - 1 ? last : ~0ull;
    const u64 c = s[idx] & own;
    const u64 up = z > 0 ? s[idx - pl] & own : 0ull, dn = z < a.nz - 1 ? s[idx + pl] & own : 0ull;
    const u64 fr = y > 0 ? s[idx - a.nw] & own : 0ull, bk = y < a.ny - 1 ? s[idx + a.nw] & own : 0ull;
    const u64 lf = k > 0 ? s[idx - 1] : 0ull, rt = k < a.nw - 1 ? s[idx + 1] & (k == a.nw - 2 ? last : ~0ull) : 0ull;
    const u64 sl = c << 1 | lf >> 63, sr = c >> 1 | rt << 63;
    if (ERODE) return c & up & dn & fr & bk & sl & sr;
    return (c | up | dn | fr | bk | sl | sr) & own;
}

template <bool ERODE>
__global__ __launch_bounds__(NT) void open_step_kernel(OpenArgs a) {
    const long idx = (long)blockIdx.x * NT + threadIdx.x;
    if (idx >= a.nwords) return;
    const int k = (int)(idx % a.nw);
    const long r = idx / a.nw;
    a.dst[idx] = cross_step<ERODE>(a, idx, (int)(r / a.ny), (int)(r % a.ny), k);
}

// the last dilation, & m, and the three forms of the result
__global__ __launch_bounds__(NT) void open_last_kernel(OpenArgs a) {
    __shared__ u64 shw[NT];
    const int tid = threadIdx.x;
    const long idx = (long)blockIdx.x * NT + tid;
    Box box;
    box.init();
    u64 res = 0;
    if (idx < a.nwords) {
        const int k = (int)(idx % a.nw);
        const long r = idx / a.nw;
        const int y = (int)(r % a.ny), z = (int)(r / a.ny);
        res = cross_step<false>(a, idx, z, y, k) & a.orig[idx];
        a.dst[idx] = res;
        if (res) {
            box.cnt = __popcll(res);
            box.add(z, y, 64 * k + __ffsll((long long)res) - 1, 64 * k + 63 - __clzll((long long)res));
        }
    }
    shw[tid] = res;
    __syncthreads();
    // bytes: a wave writes the 64 voxels of one word, consecutive lanes consecutive bytes
    const int lane = tid & 63, wave = tid >> 6;
    for (int i = 0; i < 64; ++i) {
        const int wl = i * (NT / 64) + wave;
        const long widx = (long)blockIdx.x * NT + wl;
        if (widx >= a.nwords) break;
        const int k = (int)(widx % a.nw), x = 64 * k + lane;
        if (x < a.nx) a.mask[(widx / a.nw) * a.nx + x] = (uint8_t)(shw[wl] >> lane & 1ull);
    }
    block_box(box, a.part + (long)blockIdx.x * ROW);
}

struct RemapArgs {
    const uint8_t* in;                                   // [nb][P_in][v]
    uint8_t* out[MAXV];                                  // [nb][P_out][v]
    long v, items;
    int P_in, P_out, C_out, nvol, vec;
    u64 in_valid;
    u64 ones[MAXB][MAXV];
    u64 masks[TW];                                       // [nb][nvol][C_out]
};
static_assert(sizeof(RemapArgs) <= 4096, "the tables travel in the 4 KB kernel-argument block");

__global__ __launch_bounds__(NT) void label_remap_kernel(RemapArgs a) {
    __shared__ u64 shm[MAXV * RSUPER_CROP_MAX_CLASSES];
    const int tid = threadIdx.x, b = blockIdx.y, n = a.nvol * a.C_out;
    for (int t = tid; t < n; t += NT) shm[t] = a.masks[b * n + t];
    __syncthreads();
    const long item = (long)blockIdx.x * NT + tid;
    if (item >= a.items) return;
    const long v0 = item * 4;
    const int nv = a.v - v0 < 4 ? (int)(a.v - v0) : 4;
    u64 bits[4] = {0, 0, 0, 0};
    for (int p = 0; p < a.P_in; ++p) {
        const uint8_t* __restrict__ s = a.in + ((long)b * a.P_in + p) * a.v + v0;
        uint32_t w = 0;
        if (a.vec) w = *reinterpret_cast<const uint32_t*>(s);
        else
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < nv) w |= (uint32_t)s[i] << (8 * i);
        const uint32_t r = __brev(w);                    // byte 3 - i = voxel i's byte with class 8p + j at bit j
#pragma unroll
        for (int i = 0; i < 4; ++i) bits[i] |= (u64)(r >> (8 * (3 - i)) & 0xffu) << (8 * p);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) bits[i] &= a.in_valid;
    for (int k = 0; k < a.nvol; ++k) {
        const u64 ones = a.ones[b][k];
        for (int p = 0; p < a.P_out; ++p) {
            uint32_t w = 0;
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * p + j;
                if (c >= a.C_out) break;                 // the padding bits of the last plane stay zero
                const u64 mk = shm[k * a.C_out + c];
                const uint32_t one = (uint32_t)(ones >> c & 1ull);
#pragma unroll
                for (int i = 0; i < 4; ++i) w |= (((bits[i] & mk) != 0ull ? 1u : 0u) | one) << (8 * i + 7 - j);   // class_bit(c): j = c & 7
            }
            uint8_t* __restrict__ q = a.out[k] + ((long)b * a.P_out + p) * a.v + v0;
            if (a.vec) *reinterpret_cast<uint32_t*>(q) = w;
            else
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < nv) q[i] = (uint8_t)(w >> (8 * i));
        }
    }
}

long chunks_of(long V) { return (V + CHUNK - 1) / CHUNK; }

bool label_shape_ok(int B, int P, int C, int plain, int D, int H, int W) {
    if (B < 1 || B > 65535 || C < 1 || C > RSUPER_CROP_MAX_CLASSES || D < 1 || H < 1 || W < 1) return false;
    if (plain ? P != C : (P < (C + 7) / 8 || P > CP)) return false;
    return (long)D * H * W < (1l << 31);
}

bool set_ok(u64 set, int C) { return C == 64 || (set >> C) == 0ull; }

long words_of(int nz, int ny, int nx) { return (long)nz * ny * ((nx + 63) / 64); }

long open_blocks(int nz, int ny, int nx) { return (words_of(nz, ny, nx) + NT - 1) / NT; }

bool box_ok(int nz, int ny, int nx) { return nz >= 1 && ny >= 1 && nx >= 1 && (long)nz * ny * nx < (1l << 31); }

}  // namespace

extern "C" {

long rsuper_union_bbox_workspace_bytes(int B, int D, int H, int W) {
    if (B < 1 || D < 1 || H < 1 || W < 1) return 0;
    return (long)B * chunks_of((long)D * H * W) * ROW * (long)sizeof(int);
}

int rsuper_union_bbox(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, const unsigned long long* sets, void* workspace,
                      long workspace_bytes, long long* count, int* bbox, void* stream) {
    if (!packed || !sets || !workspace || !count || !bbox || !label_shape_ok(B, P, C, plain, D, H, W)) return RS_ERR_ARG;
    if (workspace_bytes < rsuper_union_bbox_workspace_bytes(B, D, H, W) || (uintptr_t)workspace % 4 || (uintptr_t)count % 8 || (uintptr_t)bbox % 4)
        return RS_ERR_ARG;
    for (int b = 0; b < B; ++b)
        if (!set_ok(sets[b], C)) return RS_ERR_ARG;
    UnionArgs a{};
    a.V = (long)D * H * W; a.P = P; a.plain = plain ? 1 : 0; a.nchunks = (int)chunks_of(a.V); a.H = H; a.W = W;
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += MAXB) {               // the sets travel in the kernel arguments, MAXB samples per launch
        const int nb = B - b0 < MAXB ? B - b0 : MAXB;
        a.packed = packed + (long)b0 * P * a.V;
        a.part = (int*)workspace + (long)b0 * a.nchunks * ROW;
        for (int b = 0; b < nb; ++b) a.set[b] = sets[b0 + b];
        hipLaunchKernelGGL(union_bbox_kernel, dim3(a.nchunks, nb), dim3(NT), 0, s, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(fold_box_kernel, dim3(B), dim3(NT), 0, s, (const int*)workspace, a.nchunks, count, bbox, D, H, W, 0, 0, 0);
    return rs_check_launch();
}

int rsuper_union_bits(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, int b, unsigned long long set, int z0, int y0, int x0,
                      int nz, int ny, int nx, unsigned long long* bits, void* stream) {
    if (!packed || !bits || (uintptr_t)bits % 8 || !label_shape_ok(B, P, C, plain, D, H, W) || b < 0 || b >= B || !set_ok(set, C)) return RS_ERR_ARG;
    if (!box_ok(nz, ny, nx) || z0 < 0 || y0 < 0 || x0 < 0 || nz > D - z0 || ny > H - y0 || nx > W - x0) return RS_ERR_ARG;
    BitsArgs a{};
    a.V = (long)D * H * W;
    a.packed = packed + (long)b * P * a.V;
    a.bits = bits; a.P = P; a.plain = plain ? 1 : 0; a.H = H; a.W = W; a.z0 = z0; a.y0 = y0; a.x0 = x0; a.ny = ny; a.nx = nx; a.nw = (nx + 63) / 64;
    a.set = set; a.nwords = words_of(nz, ny, nx);
    const long nblk = (a.nwords + NT / 64 - 1) / (NT / 64);
    if (nblk >= (1l << 31)) return RS_ERR_ARG;
    hipLaunchKernelGGL(union_bits_kernel, dim3((unsigned)nblk), dim3(NT), 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

long rsuper_bits_open_workspace_bytes(int nz, int ny, int nx) {
    if (!box_ok(nz, ny, nx)) return 0;
    return 2 * words_of(nz, ny, nx) * 8 + open_blocks(nz, ny, nx) * ROW * (long)sizeof(int);
}

int rsuper_bits_open(const unsigned long long* bits, int nz, int ny, int nx, int r, int add_z, int add_y, int add_x, void* workspace, long workspace_bytes,
                     unsigned long long* out_bits, uint8_t* out_mask, long long* count, int* bbox, void* stream) {
    if (!bits || !workspace || !out_bits || !out_mask || !count || !bbox || !box_ok(nz, ny, nx) || r < 1 || r > RSUPER_OPEN_MAX_RADIUS) return RS_ERR_ARG;
    if (out_bits == bits || (uintptr_t)bits % 8 || (uintptr_t)out_bits % 8 || (uintptr_t)workspace % 8 || (uintptr_t)count % 8 || (uintptr_t)bbox % 4)
        return RS_ERR_ARG;
    if (workspace_bytes < rsuper_bits_open_workspace_bytes(nz, ny, nx)) return RS_ERR_ARG;
    {                                                    // neither the input nor the output may lie in the ping-pong copies
        const uintptr_t w0 = (uintptr_t)workspace, w1 = w0 + (uintptr_t)rsuper_bits_open_workspace_bytes(nz, ny, nx);
        const uintptr_t nb = (uintptr_t)words_of(nz, ny, nx) * 8, i0 = (uintptr_t)bits, o0 = (uintptr_t)out_bits;
        if ((i0 < w1 && i0 + nb > w0) || (o0 < w1 && o0 + nb > w0) || (i0 < o0 + nb && o0 < i0 + nb)) return RS_ERR_ARG;
    }
    const long nwords = words_of(nz, ny, nx), nblk = open_blocks(nz, ny, nx);
    u64* buf[2] = {(u64*)workspace, (u64*)workspace + nwords};
    int* part = (int*)((u64*)workspace + 2 * nwords);
    OpenArgs a{};
    a.nwords = nwords; a.nz = nz; a.ny = ny; a.nx = nx; a.nw = (nx + 63) / 64;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk), block(NT);
    const u64* src = bits;
    for (int i = 0; i < 2 * r - 1; ++i) {                // r erosions, then r - 1 of the r dilations
        a.src = src; a.dst = buf[i & 1];
        if (i < r) hipLaunchKernelGGL(open_step_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(open_step_kernel<false>, grid, block, 0, s, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
        src = a.dst;
    }
    a.src = src; a.dst = out_bits; a.orig = bits; a.mask = out_mask; a.part = part;
    hipLaunchKernelGGL(open_last_kernel, grid, block, 0, s, a);
    if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    hipLaunchKernelGGL(fold_box_kernel, dim3(1), dim3(NT), 0, s, (const int*)part, (int)nblk, count, bbox, nz, ny, nx, add_z, add_y, add_x);
    return rs_check_launch();
}

int rsuper_label_remap(const uint8_t* in, int B, int P_in, int C_in, long v, int nvol, uint8_t* const* outs, int P_out, int C_out,
                       const unsigned long long* masks, const unsigned long long* ones, void* stream) {
    if (!in || !outs || !masks || !ones || B < 1 || B > 65535 || nvol < 1 || nvol > MAXV || v < 1 || v >= (1l << 31)) return RS_ERR_ARG;
    if (C_in < 1 || C_in > RSUPER_CROP_MAX_CLASSES || P_in < (C_in + 7) / 8 || P_in > CP) return RS_ERR_ARG;
    if (C_out < 1 || C_out > RSUPER_CROP_MAX_CLASSES || P_out != (C_out + 7) / 8) return RS_ERR_ARG;
    RemapArgs a{};
    a.vec = v % 4 == 0 && (uintptr_t)in % 4 == 0;
    for (int k = 0; k < nvol; ++k) {
        if (!outs[k] || outs[k] == in) return RS_ERR_ARG;
        a.vec = a.vec && (uintptr_t)outs[k] % 4 == 0;
    }
    for (long i = 0; i < (long)B * nvol; ++i)
        if (!set_ok(ones[i], C_out)) return RS_ERR_ARG;
    for (long i = 0; i < (long)B * nvol * C_out; ++i)
        if (!set_ok(masks[i], C_in)) return RS_ERR_ARG;
    a.v = v; a.items = (v + 3) / 4; a.P_in = P_in; a.P_out = P_out; a.C_out = C_out; a.nvol = nvol;
    a.in_valid = C_in == 64 ? ~0ull : (1ull << C_in) - 1ull;
    const long nblk = (a.items + NT - 1) / NT;
    const int per = nvol * C_out;
    const int group = TW / per < MAXB ? TW / per : MAXB;  // >= 2: 3 * 64 words per sample at the most
    for (int b0 = 0; b0 < B; b0 += group) {
        const int nb = B - b0 < group ? B - b0 : group;
        a.in = in + (long)b0 * P_in * v;
        for (int k = 0; k < nvol; ++k) a.out[k] = outs[k] + (long)b0 * P_out * v;
        for (int b = 0; b < nb; ++b)
            for (int k = 0; k < nvol; ++k) a.ones[b][k] = ones[(long)(b0 + b) * nvol + k];
        for (int i = 0; i < nb * per; ++i) a.masks[i] = masks[(long)b0 * per + i];
        hipLaunchKernelGGL(label_remap_kernel, dim3((unsigned)nblk, nb), dim3(NT), 0, (hipStream_t)stream, a);
        if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    }
    return RS_OK;
}

}  // extern "C"
