// Bit-packed label volumes on the device: packing, inflation and per-plane "any voxel" flags (layout: label_bits.hpp).
//   unpack_bits[_sel]  np.unpackbits(packed, axis = class)[:C], all class planes or the wanted ones only
//   pack_bits          np.packbits(volume != 0, axis = class)
//   plane_any[_bits]   flags[plane] = the plane holds a voxel, on byte planes or straight from the packed bytes
#include "common.hpp"
#include "label_bits.hpp"
#include "morph.hpp"

// Bit-packed label ingestion.  The reference stores label / unk / chosen-segment volumes as
// np.packbits(bool (C, D, H, W), axis=0) (dataset_abdomenatlas_UFO.py:955,970,975) and inflates them on the host with
// np.unpackbits(...)[:C] (:1031-1034) before a 16x larger H2D copy.  Here the packed bytes travel and are inflated on the
// device: out[b][c][v] = (packed[b][c >> 3][v] >> class_bit(c)) & 1.
// Thread = 16 voxels of one byte plane: one 16-byte load, up to eight 16-byte stores.
// Plane (b, c) is written iff flags[b * C + c] != 0 or force[c] != 0 (either table may be null; both null = every plane).  A byte plane none of whose
// eight classes is wanted is not read.  What the report losses need of a bit-packed volume: the lesion channels (force) and, of the unknown map, the
// planes that hold a voxel at all (flags from plane_any_bits_kernel) -- the other planes of `out` are never written and never read.
__global__ __launch_bounds__(256) void unpack_bits_sel_kernel(const uint8_t* __restrict__ packed, uint8_t* __restrict__ out, int P, int C, long V,
                                                              const uint8_t* __restrict__ flags, const uint8_t* __restrict__ force) {
    const long nvec = (V + 15) / 16;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int pl = blockIdx.y % P, b = blockIdx.y / P;
    unsigned want = 0;                                           // wave-uniform (depends on the block's plane only)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = pl * 8 + k;
        if (c < C && ((flags && flags[(size_t)b * C + c]) || (force && force[c]) || (!flags && !force))) want |= 1u << k;
    }
    if (!want || t >= nvec) return;
    const uint8_t* src = packed + ((size_t)b * P + pl) * V;
    const long v0 = t * 16;
    const bool full = v0 + 16 <= V && (V & 15) == 0;
    uint8_t in[16];
    if (full) *(uint4*)in = *(const uint4*)(src + v0);
    else {
#pragma unroll
        for (int j = 0; j < 16; ++j) in[j] = v0 + j < V ? src[v0 + j] : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (!((want >> k) & 1u)) continue;
        const int c = pl * 8 + k;
        uint8_t o[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = (in[j] >> class_bit(k)) & 1;
        uint8_t* dst = out + ((size_t)b * C + c) * V + v0;
        if (full) *(uint4*)dst = *(const uint4*)o;
        else {
#pragma unroll
            for (int j = 0; j < 16; ++j) if (v0 + j < V) dst[j] = o[j];
        }
    }
}
int rs_launch_unpack_bits_sel(const uint8_t* packed, uint8_t* out, int B, int P, int C, long V, const uint8_t* flags, const uint8_t* force, hipStream_t st) {
    const long nvec = (V + 15) / 16;
    hipLaunchKernelGGL(unpack_bits_sel_kernel, dim3((unsigned)((nvec + 255) / 256), (unsigned)(B * P)), dim3(256), 0, st, packed, out, P, C, V, flags, force);
    return rs_check_launch();
}
int rs_launch_unpack_bits(const uint8_t* packed, uint8_t* out, int B, int P, int C, long V, hipStream_t st) {
    return rs_launch_unpack_bits_sel(packed, out, B, P, C, V, nullptr, nullptr, st);
}

// The inverse, np.packbits((src != 0), axis = class) on the device: dst[b][p][v] = OR_k (src[b][8 p + k][v] != 0) << class_bit(k), classes >= C contribute 0.
// What the dataset converter writes is the unpacked int8 (C, D, H, W) volume (dataset_conversion/nii2npz.py:80-82); the croppers read the packed form.
// The two plane strides (bytes, >= V) let a z-slab held in a staging buffer be packed straight into its place of the whole packed volume.
// VEC: every plane of src and dst starts 16-byte aligned (bases and strides are multiples of 16).  Thread = 16 voxels of one byte plane: up to eight 16-byte
// loads, one 16-byte store; the V % 16 tail of a plane goes byte by byte and nothing is read or written at or past V.
// !VEC (an unaligned base or stride): thread = 1 voxel, up to eight byte loads (lanes read consecutive bytes), one byte store.
template <bool VEC>
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int P, int C, long V, long sstride, long dstride) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int pl = blockIdx.y % P, b = blockIdx.y / P;
    const int nk = min(8, C - pl * 8);                             // wave-uniform
    const uint8_t* s = src + ((size_t)b * C + (size_t)pl * 8) * (size_t)sstride;
    uint8_t* d = dst + ((size_t)b * P + pl) * (size_t)dstride;
    if (VEC) {
        const long v0 = t * 16;
        if (v0 >= V) return;
        if (v0 + 16 <= V) {
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < nk) {
                    const uint4 x = *(const uint4*)(s + (size_t)k * (size_t)sstride + v0);
                    const int sh = class_bit(k);
                    o.x |= nonzero_bytes(x.x) << sh; o.y |= nonzero_bytes(x.y) << sh; o.z |= nonzero_bytes(x.z) << sh; o.w |= nonzero_bytes(x.w) << sh;
                }
            }
            *(uint4*)(d + v0) = o;
        } else {
            for (long v = v0; v < V; ++v) {
                unsigned o = 0;
                for (int k = 0; k < nk; ++k) o |= (unsigned)(s[(size_t)k * (size_t)sstride + v] != 0) << class_bit(k);
                d[v] = (uint8_t)o;
            }
        }
    } else {
        if (t >= V) return;
        unsigned o = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nk) o |= (unsigned)(s[(size_t)k * (size_t)sstride + t] != 0) << class_bit(k);
        d[t] = (uint8_t)o;
    }
}

int rs_launch_pack_bits(const uint8_t* src, uint8_t* dst, int B, int C, long V, long sstride, long dstride, hipStream_t st) {
    const int P = (C + 7) / 8;
    const bool vec = !(((uintptr_t)src | (uintptr_t)dst | (uintptr_t)sstride | (uintptr_t)dstride) & 15);
    const long nthr = vec ? (V + 15) / 16 : V;
    const dim3 grid((unsigned)((nthr + 255) / 256), (unsigned)(B * P));
    if (vec) hipLaunchKernelGGL(pack_bits_kernel<true>, grid, dim3(256), 0, st, src, dst, P, C, V, sstride, dstride);
    else hipLaunchKernelGGL(pack_bits_kernel<false>, grid, dim3(256), 0, st, src, dst, P, C, V, sstride, dstride);
    return rs_check_launch();
}

// OR of the V bytes at src over the blocks of grid row blockIdx.y, this thread's share: the four byte lanes of the result are not folded.
// Four independent 16-byte loads in flight per thread (one at a time ran at 1.4 TB/s); block 0 takes the V % 16 tail byte by byte.
__device__ __forceinline__ unsigned int plane_or(const uint8_t* __restrict__ src, long V) {
    const long nvec = V / 16;
    unsigned int any = 0;
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const uint4 a = ((const uint4*)src)[i], b = ((const uint4*)src)[i + stride], c = ((const uint4*)src)[i + 2 * stride], d = ((const uint4*)src)[i + 3 * stride];
        any |= (a.x | a.y | a.z | a.w) | (b.x | b.y | b.z | b.w) | (c.x | c.y | c.z | c.w) | (d.x | d.y | d.z | d.w);
    }
    for (; i < nvec; i += stride) {
        const uint4 q = ((const uint4*)src)[i];
        any |= q.x | q.y | q.z | q.w;
    }
    if (blockIdx.x == 0) for (long j = nvec * 16 + threadIdx.x; j < V; j += 256) any |= src[j];
    return any;
}

// blocks along x of the two plane_any grids
static int plane_any_blocks(long V) {
    const long nb = (V / 16 + 255) / 256;
    return (int)(nb > 32 ? 32 : nb < 1 ? 1 : nb);
}

__global__ void plane_flags_zero_kernel(uint8_t* flags, long planes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < planes) flags[i] = 0;
}

// flags[b * C + c] = any voxel of class c of sample b set, straight from the packed bytes: the OR over byte plane (b, p) holds the eight class flags of that plane
// (bit class_bit(k) = class 8 p + k).  1/8 of the bytes rsuper_plane_any reads on the inflated volume.  flags must be zeroed first (plane_flags_zero_kernel).
__global__ __launch_bounds__(256) void plane_any_bits_kernel(const uint8_t* __restrict__ packed, int P, int C, long V, uint8_t* __restrict__ flags) {
    const int pl = blockIdx.y % P, b = blockIdx.y / P;
    unsigned int any = plane_or(packed + (size_t)blockIdx.y * V, V);
    any |= any >> 16; any |= any >> 8; any &= 0xFFu;             // fold the four byte lanes of the word
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o, 64);
    if (any && (threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (((any >> class_bit(k)) & 1u) && pl * 8 + k < C) flags[(size_t)b * C + pl * 8 + k] = 1;
    }
}
int rs_launch_plane_any_bits(const uint8_t* packed, int B, int P, int C, long V, uint8_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(plane_flags_zero_kernel, dim3((unsigned)(((long)B * C + 255) / 256)), dim3(256), 0, st, flags, (long)B * C);
    hipLaunchKernelGGL(plane_any_bits_kernel, dim3((unsigned)plane_any_blocks(V), (unsigned)(B * P)), dim3(256), 0, st, packed, P, C, V, flags);
    return rs_check_launch();
}

// any(plane) for `planes` byte volumes of V voxels each: flags[p] = 1 if the plane has a non-zero byte.  Replaces the ATen
// `.flatten(1).any(1)` reductions of the loss' host control flow (150 us each on a 46 MB uint8 tensor) at HBM rate.
__global__ __launch_bounds__(256) void plane_any_kernel(const uint8_t* __restrict__ m, long V, uint8_t* __restrict__ flags) {
    const unsigned int any = plane_or(m + (size_t)blockIdx.y * V, V);
    if (__any(any != 0) && (threadIdx.x & 63) == 0) flags[blockIdx.y] = 1;
}
int rs_launch_plane_any(const uint8_t* m, long planes, long V, uint8_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(plane_flags_zero_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, st, flags, planes);   // a kernel, not a memset node (optim.hip)
    hipLaunchKernelGGL(plane_any_kernel, dim3((unsigned)plane_any_blocks(V), (unsigned)planes), dim3(256), 0, st, m, V, flags);
    return rs_check_launch();
}
