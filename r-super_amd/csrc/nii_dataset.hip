// NIfTI CT + mask files -> a packed training case on the device (dataset_conversion/abdomenatlas_3d.py ResampleImage :59-103 and process_case_* :106-217,
// dataset_conversion/nii2npz.py process_file :32-86).  DESIGN.md 6q has the layout and the bytes per pass.
//
// label_gather_pack_kernel   one launch per output byte plane = a group of up to eight classes.  Every class of the group is a mask FILE as it lies on
//   disk: its voxel buffer sits somewhere in one device buffer and a descriptor says where (element offset), what (RSUPER_NII_* integer dtype) and how
//   the canonical voxel (z, y, x) is found in it: element base + z * sz + y * sy + x * sx, the "reorientation is a strided read, a flip is a negative
//   stride" convention of nifti_lines_kernel -- per class, because a mask may be stored in another voxel order than the CT.  The three per-axis
//   nearest tables (inference/nifti.py resample_axis_table 'nearest') map an output voxel of the resampled box to its source voxel, so
//       dst[zo + oz][yo + oy][xo + ox] = OR_k (src_k[iz[oz]][iy[oy]][ix[ox]] != 0) << class_bit(k)
//   in the layout of label_bits.hpp.  A table entry outside the source (OUTSIDE = -1), an absent class (the reference substitutes a zero label for a
//   missing file) and everything outside the box give 0 bits: the kernel writes the WHOLE padded plane, box and zero padding, in one pass, so no memset
//   precedes it.  No unpacked (C, D, H, W) volume ever exists.
//   This single gather is the composite of the reference's two label passes.  ResampleLabelToRef puts a label first onto the xy-resampled image
//   (x, y at the target spacing, z maps to itself) and then onto the xyz-resampled image (x and y map to themselves, z at the target spacing); both are
//   nearest neighbour with the identity transform, and a nearest pass whose axis maps to itself is the identity on that axis, so the two passes are
//   exactly out[oz][oy][ox] = in[iz[oz]][iy[oy]][ix[ox]] with the three per-axis tables, an outside voxel of either pass being ITK's default pixel 0.
//   Label-map mode (LUT, process_case_nnunet_format): ONE integer source volume and a table lut [n_values][P] u8; the bytes of plane p are
//   lut[value][p], a value below 0 or at or above n_values gives 0, and one launch writes all P planes.
//   Lanes run along the output's flat order, x fastest: a lane makes 16 consecutive output bytes (one 16-byte store per plane) from the first 16-byte
//   boundary of plane 0 on, class by class: the 16 loads of a class carry no branch between them and are in flight together (with one load at a time
//   the launch was bound by load latency: DESIGN 6q); block 0 takes the fewer than 16 bytes in front of it and behind the last whole vector byte by byte, and nothing is written
//   at or past the plane's end.  When the file's unit stride is canonical x a lane's 16 reads of a class are near-consecutive source bytes; a
//   permuted file is read with a stride (not tiled through LDS: DESIGN 6q).
//   Nothing the tables or the descriptors say is trusted with memory: every source index is compared with its axis, every element index with the
//   class's element count, and a class whose buffer does not lie inside the raw buffer reads as absent.
//
// label_background_kernel   nii2npz.py :58-60 makes a missing `background` as 1 - sum over the other classes and the dataset packs astype(bool): the
//   bit is set where the number of other classes at the voxel is not 1 -- on an overlap as well as where there is none.  Over the resampled box only
//   (the reference pads afterwards); a lane owns its voxel's byte of the background's plane.
#include "common.hpp"
#include "label_bits.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int GNT = 256;
constexpr int DW = RSUPER_LABEL_DESC_WORDS;

struct GpArgs {
    const uint8_t* raw;
    const long long* desc;
    const uint8_t* lut;
    const int *ix, *iy, *iz;
    uint8_t* dst;
    long raw_bytes, V;
    int nclass, n_values, P;
    int Z, Y, X, Zb, Yb, Xb, Do, Ho, Wo, zo, yo, xo;
    unsigned head, ngrp;
};

struct ClassDesc {
    long off_bytes, sz, sy, sx, base, n;
    int dtype, ok;
};

__device__ __forceinline__ int load_value(const uint8_t* __restrict__ raw, const ClassDesc& c, long e) {
    const uint8_t* p = raw + c.off_bytes;
    switch (c.dtype) {
    case RSUPER_NII_U8: return (int)p[e];
    case RSUPER_NII_I8: return (int)(int8_t)p[e];
    case RSUPER_NII_I16: return (int)reinterpret_cast<const int16_t*>(p)[e];
    case RSUPER_NII_U16: return (int)reinterpret_cast<const uint16_t*>(p)[e];
    default: return reinterpret_cast<const int32_t*>(p)[e];
    }
}

// The values of one source volume at the lane's 16 voxels: element (second row ? rb1 : rb0) + sxc[j] * sx, `inval` where the voxel is not valid or
// the element lies outside the buffer.  The loads are unconditional -- an invalid voxel reads element 0, which exists -- so all 16 are in flight.
template <typename T>
__device__ __forceinline__ void load16(const uint8_t* __restrict__ raw, const ClassDesc& c, long rb0, long rb1, unsigned sec, unsigned valid, const int* sxc,
                                       int inval, int* v) {
    const T* __restrict__ p = reinterpret_cast<const T*>(raw + c.off_bytes);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        long e = ((sec >> j) & 1u ? rb1 : rb0) + (long)sxc[j] * c.sx;
        const bool ok = ((valid >> j) & 1u) && (unsigned long)e < (unsigned long)c.n;
        e = ok ? e : 0;
        const int t = (int)p[e];
        v[j] = ok ? t : inval;
    }
}

__device__ __forceinline__ void gather16(const uint8_t* __restrict__ raw, const ClassDesc& c, long rb0, long rb1, unsigned sec, unsigned valid, const int* sxc,
                                         int inval, int* v) {
    switch (c.dtype) {                                   // wave-uniform
    case RSUPER_NII_U8: load16<uint8_t>(raw, c, rb0, rb1, sec, valid, sxc, inval, v); break;
    case RSUPER_NII_I8: load16<int8_t>(raw, c, rb0, rb1, sec, valid, sxc, inval, v); break;
    case RSUPER_NII_I16: load16<int16_t>(raw, c, rb0, rb1, sec, valid, sxc, inval, v); break;
    case RSUPER_NII_U16: load16<uint16_t>(raw, c, rb0, rb1, sec, valid, sxc, inval, v); break;
    default: load16<int32_t>(raw, c, rb0, rb1, sec, valid, sxc, inval, v); break;
    }
}

template <bool LUT>
__global__ __launch_bounds__(GNT) void label_gather_pack_kernel(GpArgs a) {
    constexpr int NK = LUT ? 1 : 8;                      // source volumes of a launch
    constexpr int NP = LUT ? 8 : 1;                      // byte planes a lane writes
    __shared__ ClassDesc cd[NK];
    const int tid = threadIdx.x;
    if (tid < NK) {
        ClassDesc c{};
        if (tid < a.nclass) {
            const long long* d = a.desc + (long)tid * DW;
            const long eoff = d[0], n = d[6];
            const int dt = (int)d[1];
            if (dt >= RSUPER_NII_U8 && dt <= RSUPER_NII_I32 && !d[7]) {
                const long esz = dt <= RSUPER_NII_I8 ? 1 : dt <= RSUPER_NII_U16 ? 2 : 4;
                if (eoff >= 0 && n >= 1 && eoff <= a.raw_bytes && n <= a.raw_bytes && (eoff + n) * esz <= a.raw_bytes) {
                    c.off_bytes = eoff * esz; c.dtype = dt; c.sz = d[2]; c.sy = d[3]; c.sx = d[4]; c.base = d[5]; c.n = n; c.ok = 1;
                }
            }
        }
        cd[tid] = c;
    }
    __syncthreads();
    const uint8_t* __restrict__ raw = a.raw;
    const int P = LUT ? a.P : 1;

    struct Row { bool ok; long rb[NK]; };
    auto row_of = [&](int z, int y) {                    // output row (z, y): its source row per class, or not ok (padding, outside the scan)
        Row r;
        r.ok = false;
#pragma unroll
        for (int k = 0; k < NK; ++k) r.rb[k] = 0;
        const int bz = z - a.zo, by = y - a.yo;
        if ((unsigned)bz < (unsigned)a.Zb && (unsigned)by < (unsigned)a.Yb) {
            const int szv = a.iz[bz], syv = a.iy[by];
            if ((unsigned)szv < (unsigned)a.Z && (unsigned)syv < (unsigned)a.Y) {
                r.ok = true;
#pragma unroll
                for (int k = 0; k < NK; ++k) r.rb[k] = cd[k].base + szv * cd[k].sz + syv * cd[k].sy;
            }
        }
        return r;
    };
    auto voxel = [&](const Row& r, int x, uint32_t* out) {   // the NP output bytes of voxel x of the row
#pragma unroll
        for (int p = 0; p < NP; ++p) out[p] = 0;
        if (!r.ok) return;
        const int bx = x - a.xo;
        if ((unsigned)bx >= (unsigned)a.Xb) return;
        const int sxv = a.ix[bx];
        if ((unsigned)sxv >= (unsigned)a.X) return;
        if (LUT) {
            if (!cd[0].ok) return;
            const long e = r.rb[0] + sxv * cd[0].sx;
            if ((unsigned long)e >= (unsigned long)cd[0].n) return;
            const int v = load_value(raw, cd[0], e);
            if ((unsigned)v >= (unsigned)a.n_values) return;
            const uint8_t* __restrict__ row = a.lut + (long)v * P;
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < P) out[p] = row[p];
        } else {
            uint32_t o = 0;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                if (k < a.nclass && cd[k].ok) {
                    const long e = r.rb[k] + sxv * cd[k].sx;
                    if ((unsigned long)e < (unsigned long)cd[k].n) o |= (uint32_t)(load_value(raw, cd[k], e) != 0) << class_bit(k);
                }
            }
            out[0] = o;
        }
    };

    const unsigned g = blockIdx.x * (unsigned)GNT + tid;
    if (g < a.ngrp) {
        const unsigned i = a.head + 16u * g, rr = i / (unsigned)a.Wo;
        int x = (int)(i % (unsigned)a.Wo), y = (int)(rr % (unsigned)a.Ho), z = (int)(rr / (unsigned)a.Ho);
        uint32_t acc[NP][4];
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p][0] = acc[p][1] = acc[p][2] = acc[p][3] = 0;
        if (a.Wo >= 16) {
            // The lane's 16 voxels lie in this output row and, past its end, in the next one.  Everything per voxel is a select, not a branch, and a
            // class is read by 16 unconditional loads (an invalid voxel reads element 0 and is masked), so the loads of a class are in flight together.
            const Row r0 = row_of(z, y);
            int y1 = y + 1, z1 = z;
            if (y1 == a.Ho) { y1 = 0; ++z1; }
            const Row r1 = row_of(z1, y1);               // past the last row of the plane: z1 == Do is outside the box, nothing is read
            unsigned sec = 0, valid = 0;
            int sxc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int xj = x + j;
                const bool s = xj >= a.Wo;
                const int bx = (s ? xj - a.Wo : xj) - a.xo;
                bool ok = (s ? r1.ok : r0.ok) && (unsigned)bx < (unsigned)a.Xb;
                const int sxv = a.ix[ok ? bx : 0];
                ok = ok && (unsigned)sxv < (unsigned)a.X;
                sxc[j] = ok ? sxv : 0;
                sec |= (unsigned)s << j;
                valid |= (unsigned)ok << j;
            }
            if (LUT) {
                if (cd[0].ok) {
                    int v[16];
                    gather16(raw, cd[0], r0.rb[0], r1.rb[0], sec, valid, sxc, -1, v);
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        if (p < P) {
#pragma unroll
                            for (int j = 0; j < 16; ++j) {
                                const bool in = (unsigned)v[j] < (unsigned)a.n_values;
                                const uint32_t b = a.lut[(long)(in ? v[j] : 0) * P + p];
                                acc[p][j >> 2] |= (in ? b : 0u) << (8 * (j & 3));
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    if (k < a.nclass && cd[k].ok) {
                        int v[16];
                        gather16(raw, cd[k], r0.rb[k], r1.rb[k], sec, valid, sxc, 0, v);
#pragma unroll
                        for (int j = 0; j < 16; ++j) acc[0][j >> 2] |= (uint32_t)(v[j] != 0) << (8 * (j & 3) + class_bit(k));
                    }
                }
            }
        } else {                                         // rows shorter than a vector: voxel by voxel
            Row row = row_of(z, y);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                uint32_t b[NP];
                voxel(row, x, b);
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[p][j >> 2] |= b[p] << (8 * (j & 3));
                if (++x == a.Wo) {
                    x = 0;
                    if (++y == a.Ho) { y = 0; ++z; }
                    row = row_of(z, y);                  // past the last row of the plane: z == Do is outside the box, nothing is read
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (p < P) {
                uint8_t* d = a.dst + (long)p * a.V + i;
                const uint4 q = make_uint4(acc[p][0], acc[p][1], acc[p][2], acc[p][3]);
                if ((uintptr_t)d % 16 == 0) *reinterpret_cast<uint4*>(d) = q;
                else __builtin_memcpy(d, &q, 16);        // a later plane of a volume with V % 16 != 0
            }
        }
    }
    if (blockIdx.x == 0) {                               // head and tail: fewer than 16 bytes each
        const unsigned tail0 = a.head + 16u * a.ngrp;
        auto one = [&](unsigned i) {
            const unsigned rr = i / (unsigned)a.Wo;
            const Row row = row_of((int)(rr / (unsigned)a.Ho), (int)(rr % (unsigned)a.Ho));
            uint32_t b[NP];
            voxel(row, (int)(i % (unsigned)a.Wo), b);
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (p < P) a.dst[(long)p * a.V + i] = (uint8_t)b[p];
        };
        if ((unsigned)tid < a.head) one((unsigned)tid);
        if (tid < 16 && (long)tail0 + tid < a.V) one(tail0 + (unsigned)tid);
    }
}

struct BgArgs {
    uint8_t* packed;
    long V, nbox;
    int P, bgp, Ho, Wo, zo, yo, xo, Yb, Xb;
    uint32_t bgmask;
};

__global__ __launch_bounds__(GNT) void label_background_kernel(BgArgs a) {
    const long t = (long)blockIdx.x * GNT + threadIdx.x;
    if (t >= a.nbox) return;
    const int bx = (int)(t % a.Xb);
    const long q = t / a.Xb;
    const int by = (int)(q % a.Yb), bz = (int)(q / a.Yb);
    const long i = ((long)(a.zo + bz) * a.Ho + (a.yo + by)) * a.Wo + (a.xo + bx);
    int others = 0;
    uint32_t own = 0;
    for (int p = 0; p < a.P; ++p) {
        const uint32_t b = a.packed[(long)p * a.V + i];
        if (p == a.bgp) { own = b; others += __popc(b & ~a.bgmask); }
        else others += __popc(b);
    }
    a.packed[(long)a.bgp * a.V + i] = (uint8_t)((own & ~a.bgmask) | (others != 1 ? a.bgmask : 0u));
}

}  // namespace

extern "C" {

int rsuper_label_gather_pack(const void* raw, long raw_bytes, const long long* desc, int nclass, const uint8_t* lut, int n_values, int P, const int* ix,
                             const int* iy, const int* iz, int Z, int Y, int X, int Zb, int Yb, int Xb, uint8_t* dst, int Do, int Ho, int Wo, int zo, int yo,
                             int xo, void* stream) {
    if (!raw || !desc || !ix || !iy || !iz || !dst || raw_bytes < 1) return RS_ERR_ARG;
    if ((uintptr_t)raw % 4 || (uintptr_t)desc % 8 || (uintptr_t)ix % 4 || (uintptr_t)iy % 4 || (uintptr_t)iz % 4) return RS_ERR_ARG;
    if (Z < 1 || Y < 1 || X < 1 || Zb < 1 || Yb < 1 || Xb < 1 || Do < 1 || Ho < 1 || Wo < 1) return RS_ERR_ARG;
    if (zo < 0 || yo < 0 || xo < 0 || zo > Do - Zb || yo > Ho - Yb || xo > Wo - Xb) return RS_ERR_ARG;
    const long V = (long)Do * Ho * Wo;
    if (V >= (1l << 31)) return RS_ERR_ARG;
    if (lut ? (nclass != 1 || n_values < 1 || P < 1 || P > 8) : (nclass < 1 || nclass > 8 || P != 1)) return RS_ERR_ARG;
    const uint8_t* rb = (const uint8_t*)raw;
    if (rb < dst + (long)P * V && dst < rb + raw_bytes) return RS_ERR_ARG;                 // overlapping buffers
    GpArgs a{};
    a.raw = rb; a.raw_bytes = raw_bytes; a.desc = desc; a.lut = lut; a.ix = ix; a.iy = iy; a.iz = iz; a.dst = dst; a.V = V;
    a.nclass = nclass; a.n_values = n_values; a.P = P;
    a.Z = Z; a.Y = Y; a.X = X; a.Zb = Zb; a.Yb = Yb; a.Xb = Xb; a.Do = Do; a.Ho = Ho; a.Wo = Wo; a.zo = zo; a.yo = yo; a.xo = xo;
    const long mis = (long)((16 - (uintptr_t)dst % 16) % 16);
    a.head = (unsigned)(mis < V ? mis : V);
    a.ngrp = (unsigned)((V - a.head) / 16);
    const unsigned nb = a.ngrp ? (a.ngrp + GNT - 1) / GNT : 1;
    if (lut) hipLaunchKernelGGL(label_gather_pack_kernel<true>, dim3(nb), dim3(GNT), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(label_gather_pack_kernel<false>, dim3(nb), dim3(GNT), 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

int rsuper_label_background(uint8_t* packed, int P, int bg_class, int Do, int Ho, int Wo, int zo, int yo, int xo, int Zb, int Yb, int Xb, void* stream) {
    if (!packed || P < 1 || P > 8 || bg_class < 0 || bg_class >= 8 * P || Do < 1 || Ho < 1 || Wo < 1 || Zb < 1 || Yb < 1 || Xb < 1) return RS_ERR_ARG;
    if (zo < 0 || yo < 0 || xo < 0 || zo > Do - Zb || yo > Ho - Yb || xo > Wo - Xb) return RS_ERR_ARG;
    const long V = (long)Do * Ho * Wo;
    if (V >= (1l << 31)) return RS_ERR_ARG;
    BgArgs a{};
    a.packed = packed; a.V = V; a.nbox = (long)Zb * Yb * Xb; a.P = P; a.bgp = bg_class >> 3; a.bgmask = 1u << (7 - (bg_class & 7));
    a.Ho = Ho; a.Wo = Wo; a.zo = zo; a.yo = yo; a.xo = xo; a.Yb = Yb; a.Xb = Xb;
    hipLaunchKernelGGL(label_background_kernel, dim3((unsigned)((a.nbox + GNT - 1) / GNT)), dim3(GNT), 0, (hipStream_t)stream, a);
    return rs_check_launch();
}

}  // extern "C"
