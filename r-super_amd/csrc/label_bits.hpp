// Reading a bit-packed whole-CT label on the device (class_counts / select_voxel in crop.hip, union_bbox / union_bits in crop_report.hip, the packing
// kernels in label_bits.hip).
//
// Layout: packed [B][P][V] u8 = np.packbits(label, axis = class), MSB first: class c is bit class_bit(c) = 7 - (c & 7) of byte plane c >> 3; packbits
// zero-fills the padding bits of the last plane.
//
// Chunks: the V voxels of a sample are cut into chunks of RSUPER_CROP_CHUNK = 16384 voxels, one block of LB_NT = 256 threads each.  A lane reads 16
// voxels of a plane as one 16-byte vector, LB_VPL = 4 of them, from the first 16-byte boundary of the chunk in plane 0 on; the fewer than 16 voxels
// before it (head) and after the last whole vector (tail) go to lanes 0..15 and 16..31 of the same block as single bytes: a chunk's result must hold
// exactly its own voxels, so every block owns its head and tail.  A plane whose base is shifted against plane 0 (V % 16 != 0) is read with unaligned
// 16-byte loads.
#pragma once
#include "common.hpp"
#include "../../include/rsuper_hip.h"

constexpr int LB_NT = 256;
constexpr int LB_CHUNK = RSUPER_CROP_CHUNK;
constexpr int LB_VPL = LB_CHUNK / 16 / LB_NT;            // 16-byte vectors of a plane per lane: 4
static_assert(LB_VPL * 16 * LB_NT == LB_CHUNK, "a block's vectors cover one chunk");

__device__ __forceinline__ uint4 ld16(const uint8_t* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint4*>(p);
    uint4 q;
    __builtin_memcpy(&q, p, 16);
    return q;
}

// the bit of its byte plane (c >> 3) that holds class c
__device__ __forceinline__ int class_bit(int c) { return 7 - (c & 7); }

// bit 0 of every byte = that byte of x is not zero (bit 7 of ((x & 0x7f..) + 0x7f..) | x is set exactly then; no carry leaves a byte)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) { return ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u; }

// bit 0 of byte i of f -> bit i
__device__ __forceinline__ uint32_t fold_nibble(uint32_t f) { return (f * 0x01020408u) >> 24 & 0xfu; }

// the byte of plane p under which the classes of the 64-bit class set sit (plain: [B][C][V] bytes, class c = plane c: all of it or nothing)
__device__ __forceinline__ uint32_t plane_mask(unsigned long long set, int p, int plain) {
    if (plain) return (set >> p) & 1ull ? 0xffu : 0u;
    return __brev((uint32_t)(set >> (8 * p)) & 0xffu) >> 24;
}

// The chunk of block `chunk` of a sample ([P][V] bytes at `sample`) as thread `tid` of the block reads it.
struct LabelChunk {
    const uint8_t* base;                                 // plane 0 at the chunk's first voxel
    long V, start;
    int len, h, nvec, tail0;                             // voxels; head bytes; whole vectors; first tail byte
    int tid, soff;                                       // the lane's single byte (head: lanes 0..15, tail: lanes 16..31) or -1

    __device__ __forceinline__ LabelChunk(const uint8_t* sample, long V_, int chunk, int tid_) : V(V_), tid(tid_) {
        start = (long)chunk * LB_CHUNK;
        len = V - start < LB_CHUNK ? (int)(V - start) : LB_CHUNK;
        base = sample + start;
        h = (int)((16 - (uintptr_t)base % 16) % 16);
        if (h > len) h = len;
        nvec = (len - h) / 16;
        tail0 = h + nvec * 16;
        soff = tid < h ? tid : (tid >= 16 && tid < 32 && tail0 + tid - 16 < len) ? tail0 + tid - 16 : -1;
    }
    __device__ __forceinline__ const uint8_t* plane(int p) const { return base + (long)p * V; }
    __device__ __forceinline__ bool aligned(int p) const { return (uintptr_t)(plane(p) + h) % 16 == 0; }
    // offset inside the chunk of the first voxel of the lane's v-th vector
    __device__ __forceinline__ int vec_off(int v) const { return h + 16 * (v * LB_NT + tid); }
    // plane p of the chunk: on_vec(v, q) for each of the lane's vectors v < LB_VPL that exists, on_byte(w) for the lane's single byte if it has one
    template <typename FV, typename FB>
    __device__ __forceinline__ void for_each(int p, FV on_vec, FB on_byte) const {
        const uint8_t* __restrict__ s = plane(p);
        const bool al = aligned(p);
#pragma unroll
        for (int v = 0; v < LB_VPL; ++v)
            if (v * LB_NT + tid < nvec) on_vec(v, ld16(s + vec_off(v), al));
        if (soff >= 0) on_byte((uint32_t)s[soff]);
    }
};

// Block reduction of a partial row over LB_NT threads: block_stage leaves the four waves' results in sh[0..3] (wave shuffle, lane 0 writes); after a
// __syncthreads block_finish folds them in any one thread.
struct RedSum { template <typename T> __device__ static __forceinline__ T op(T a, T b) { return a + b; } };
struct RedMin { template <typename T> __device__ static __forceinline__ T op(T a, T b) { return a < b ? a : b; } };
struct RedMax { template <typename T> __device__ static __forceinline__ T op(T a, T b) { return a > b ? a : b; } };

// several values at once, value i under Ops i: step by step, so the independent shuffles of a step are in flight together
template <typename... Ops, typename... Ts>
__device__ __forceinline__ void wave_reduce_all(Ts&... v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ((v = Ops::op(v, (Ts)__shfl_xor(v, o, 64))), ...);
}
template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce(T v) {
    wave_reduce_all<Op>(v);
    return v;
}
template <typename Op, typename T>
__device__ __forceinline__ void block_stage(T v, T* sh) {
    v = wave_reduce<Op>(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}
template <typename Op, typename T>
__device__ __forceinline__ T block_finish(const T* sh) {
    T s = sh[0];
#pragma unroll
    for (int w = 1; w < LB_NT / 64; ++w) s = Op::op(s, sh[w]);
    return s;
}
