// The dispatch of the kernels MedFormer's attention stages run on -- pointwise.hip (1x1x1 convolution GEMM, its weight gradient), depthwise.hip and
// instnorm.hip (channel norm, squeeze-excite, cl_planar) -- host only: WHICH kernel a launch runs, with which template selector, grid, workgroup and
// rows of `part` / workspace.  One mf_*_plan per launch; nothing here launches anything and nothing elsewhere decides: api.hip asks the plans of an
// entry point and hands each GluePlan (misc.hpp; `kernel` is an MfKernel) to a launcher that only switches over it; rsuper_mf_plan and the row /
// split / byte queries give the same answers to tests and to the modules that allocate.  A new kernel or grid of the family is taught to this file
// and to the launcher's switch.  Included by api.hip only (after glue_plan.hpp); tests/test_mf_plan_cpu.py pins every answer against the launches
// recorded in tests/golden/mf_launches.json.
#pragma once
#include <stdlib.h>
#include "common.hpp"
#include "misc.hpp"
#include "mf_tiles.hpp"

// The switches of the family, read from the environment once:
//   RSUPER_PW_WG_TARGET=n      blocks per pointwise weight-gradient launch that the slab count aims at (256; measured: 128 / 256 / 512 / 1024 ->
//                              MedFormer step 28.6 / 28.5 / 28.9 / 29.4 ms)
//   RSUPER_PW_WG_DIRECT=rows   rows up to which ONE slab is forced (a single slab writes dW itself, no reduce launch).  0: 768 measured no faster than
//                              7 slabs + reduce at 432 rows (MedFormer 27.2 vs 27.0 ms); a naturally single slab (<= 64 rows) always writes directly
//   RSUPER_DW_NO_LDS           (set to anything) the register-run depthwise kernel for every shape
//   RSUPER_CNORM_SMALL_VOX=n   voxels up to which a channel norm is ONE launch (512)
struct MfSwitches { int pw_wg_target, pw_wg_direct; bool dw_no_lds; long cnorm_small_vox; };
static const MfSwitches& mf_switches() {
    static const MfSwitches s = [] {
        auto env = [](const char* name, const char* unset) { const char* e = getenv(name); return e ? e : unset; };
        return MfSwitches{atoi(env("RSUPER_PW_WG_TARGET", "256")), atoi(env("RSUPER_PW_WG_DIRECT", "0")), env("RSUPER_DW_NO_LDS", nullptr) != nullptr,
                          atol(env("RSUPER_CNORM_SMALL_VOX", "512"))};
    }();
    return s;
}

static const GluePlan MF_NO_PLAN = {MF_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static GluePlan mf_plan_of(int kernel, long bx, long by, long bz, int threads) { return {kernel, 0, (int)bx, (int)by, (int)bz, threads, 0, 0, RS_F32, 0}; }
static inline long mf_cdiv(long a, long b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------------------------------------ pointwise.hip
// weight fragments of one layer: a thread per 16-byte fragment slot
static size_t mf_pw_packed_bytes(int dtype, int K, int N) { return (size_t)pw_ksteps(K, dtype == RS_F32) * pw_ntiles(N) * 64 * 16; }
static GluePlan mf_pw_pack_plan(int dtype, int K, int N) {
    GluePlan pl = mf_plan_of(MF_PW_PACK, mf_cdiv((long)pw_ksteps(K, dtype == RS_F32) * pw_ntiles(N) * 64, 256), 1, 1, 256);
    pl.dtype = dtype;
    return pl;
}
static GluePlan mf_pw_pack_batch_plan(int dtype, long total_items) {
    GluePlan pl = mf_plan_of(MF_PW_PACK_BATCH, mf_cdiv(total_items, 256), 1, 1, 256);
    pl.dtype = dtype;
    return pl;
}
// y (R x N) = x (R x K) op(W), mode 0 and mode 1 alike.  NF 32-channel tiles per wave; the reduction split over the four waves of a block (32 rows
// per block instead of 128) when whole-K blocks of 128 rows would cover less than half of the CUs -- measured: 216 whole-K blocks beat 864 split
// ones (26 vs 37 us), 54 lose (37 vs 17 us)
static GluePlan mf_pw_plan(int dtype, int R, int K, int N) {
    const int ntiles = pw_ntiles(N), nf = ntiles >= 4 ? 4 : ntiles >= 2 ? 2 : 1;
    const long gy = mf_cdiv(ntiles, nf);
    const bool ksplit = pw_ksteps(K, dtype == RS_F32) >= 8 && mf_cdiv(R, 128) * gy < 128;
    GluePlan pl = mf_plan_of(MF_PW_GEMM, mf_cdiv(R, ksplit ? 32 : 128), gy, 1, 256);
    pl.dtype = dtype; pl.sel = nf; pl.arg = ksplit;
    return pl;
}
// dW (N x K) = dy^T x over R rows: WNW x (4 / WNW) wave tiles of 64 x 64 per block, S slabs of the rows in z.  S <= 0: the plan's own count -- about
// one resident block per CU (more slabs = more partial traffic for the reduce), at least 64 rows per slab; a caller's S is taken as it is (a slab
// past the last row writes its -- zero -- partial).  Slabs are whole MFMA steps (16 rows), so the count is re-cut: no slab without rows.
// rows = S slabs of N*K + N floats in the workspace; one slab writes dW / db itself.
static GluePlan mf_pw_wgrad_plan(int dtype, int R, int N, int K, int S) {
    const int wnw = N <= 64 ? 1 : K <= 64 ? 4 : 2;
    GluePlan pl = mf_plan_of(MF_PW_WGRAD, mf_cdiv(N, wnw * 64), mf_cdiv(K, (4 / wnw) * 64), 1, 256);
    auto rows_per = [R](int s) { return (int)(mf_cdiv(mf_cdiv(R, s), 16) * 16); };
    if (S <= 0) {
        const int tiles = pl.bx * pl.by;
        S = mf_switches().pw_wg_target / tiles;
        if (S > mf_cdiv(R, 64)) S = (int)mf_cdiv(R, 64);
        if (S < 1 || R <= mf_switches().pw_wg_direct) S = 1;
        S = (int)mf_cdiv(R, rows_per(S));
    }
    pl.dtype = dtype; pl.sel = wnw; pl.bz = pl.rows = S; pl.arg = rows_per(S);
    return pl;
}
// the sum over the slabs, a float4 of the (N*K + N)-element result per thread; MF_NONE: one slab, no launch
static GluePlan mf_pw_wgrad_reduce_plan(int N, int K, int S) {
    return S > 1 ? mf_plan_of(MF_PW_WGRAD_REDUCE, mf_cdiv(((long)N * K + N) / 4, 256), 1, 1, 256) : MF_NO_PLAN;
}

// ------------------------------------------------------------------------------------------------ depthwise.hip
static inline bool mf_dw_ok(int N, int D, int H, int W, int C) { return (long)N * D * H * W * C < (1L << 30); }      // 32-bit byte offsets of the buffer loads (< 4 GiB)
// Forward and data gradient.  Measured (B = 2): 48^3 x 256 ch 209 -> 149 us; 24^3 x 512 41 -> 40, 24^3 x 384 33 -> 37, 24^3 x 128 14 -> 20 us (the
// halo planes of the short D segments and 6 waves per CU cost more than the L2 re-reads there): the LDS kernel takes the 32^2-and-larger planes only.
static GluePlan mf_dw_plan(int N, int D, int H, int W, int C) {
    if (!mf_dw_ok(N, D, H, W, C)) return MF_NO_PLAN;
    if (!mf_switches().dw_no_lds && H >= 32 && W >= 32 && D >= 6 && (C % 4) == 0 && (size_t)H * W * C * 4 < 0x40000000ull) {
        const long tiles = mf_cdiv(H, DL_T) * mf_cdiv(W, DL_T), groups = mf_cdiv(C, DL_C);
        // split D so that >= ~1500 blocks are in flight (3 per CU), but keep >= 6 planes per segment (2 halo planes are re-read per segment)
        int dsegs = 1;
        while (tiles * groups * N * dsegs < 1536 && D / (dsegs + 1) >= 6) ++dsegs;
        GluePlan pl = mf_plan_of(MF_DW_LDS, tiles * dsegs, groups, N, 128);
        pl.arg = dsegs;
        return pl;
    }
    // the LDS weight staging is per block: aim at >= 8 passes per block, but never below ~1024 blocks in flight (small volumes)
    const long runs = (long)N * D * H * mf_cdiv(W, DW_R), groups = mf_cdiv(C, DW_CG), all = mf_cdiv(runs, DW_VPB);
    long bx = mf_cdiv(runs, DW_VPB * 8);
    if (bx * groups < 1024) bx = mf_cdiv(1024, groups);
    if (bx > all) bx = all;
    if (bx > 2048) bx = 2048;
    return mf_plan_of(MF_DW_FWD, bx, groups, 1, 256);
}
// weight gradient: rows of `part` (rows, 27, C) = blocks in x, >= 8 passes per block; then the fixed-order sum of the rows
static int mf_dw_rows(long vox) {
    const long b = mf_cdiv(vox, DW_VPB * 8);
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}
static GluePlan mf_dw_wgrad_plan(int N, int D, int H, int W, int C) {
    if (!mf_dw_ok(N, D, H, W, C)) return MF_NO_PLAN;
    GluePlan pl = mf_plan_of(MF_DW_WGRAD, mf_dw_rows((long)N * D * H * W), mf_cdiv(C, DW_CG), 1, 256);
    pl.rows = pl.bx;
    return pl;
}
static GluePlan mf_dw_wgrad_reduce_plan(int N, int D, int H, int W, int C) {
    return mf_dw_ok(N, D, H, W, C) ? mf_plan_of(MF_DW_WGRAD_REDUCE, mf_cdiv(27 * C, 32), 1, 1, 256) : MF_NO_PLAN;
}

// ------------------------------------------------------------------------------------------------ instnorm.hip
// statistics: rows of `part` (N, rows, C, 2) = blocks in x, >= 8 passes per block; mode 0: sums of x, 1: of the backward pass
static int mf_cnorm_rows(long vox) {
    const long b = mf_cdiv(vox, CN_VPB * 8);
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}
static GluePlan mf_cnorm_stats_plan(int N, long vox, int C, int mode) {
    GluePlan pl = mf_plan_of(MF_CNORM_STATS, mf_cnorm_rows(vox), mf_cdiv(C, CN_CG), N, 256);
    pl.sel = mode; pl.rows = pl.bx;
    return pl;
}
static GluePlan mf_cnorm_apply_plan(int N, long vox, int C, int mode) {      // mode 0: norm, 1: its backward, 2: per-(sample, channel) affine map
    const long bx = mf_cdiv(vox, CN_VPB);
    GluePlan pl = mf_plan_of(MF_CNORM_APPLY, bx > 2048 ? 2048 : bx, mf_cdiv(C, CN_CG), N, 256);
    pl.sel = mode;
    return pl;
}
static GluePlan mf_cnorm_small_plan(int N, int C, int mode) {      // statistics, finalize and apply of a small volume in ONE launch: no `part`
    GluePlan pl = mf_plan_of(MF_CNORM_SMALL, mf_cdiv(C, CS_CG), N, 1, 256);
    pl.sel = mode;
    return pl;
}
// the first launch of a whole norm (rsuper_cnorm_forward: mode 0, _backward: 1): the low-resolution stages and the semantic maps take one launch,
// the rest statistics -> finalize -> apply (mf_cnorm_apply_plan)
static GluePlan mf_cnorm_plan(int N, long vox, int C, int mode) {
    return vox <= mf_switches().cnorm_small_vox ? mf_cnorm_small_plan(N, C, mode) : mf_cnorm_stats_plan(N, vox, C, mode);
}
// squeeze-excite: the launches between the channel statistics and the affine apply.  C and r are LDS extents and loop bounds of one block.
static GluePlan mf_se_plan(int kernel, int N, int C, int r) {
    if (C > 8192 || r > 8192 || r < 1) return MF_NO_PLAN;
    GluePlan pl = MF_NO_PLAN;
    switch (kernel) {
        case MF_SE_HIDDEN_FWD: pl = mf_plan_of(kernel, N, mf_cdiv(r, 16), 1, 1024); break;
        case MF_SE_GATE_FWD:   pl = mf_plan_of(kernel, N, mf_cdiv(C, 64), 1, 1024); break;
        case MF_SE_BWD_HIDDEN: pl = mf_plan_of(kernel, N, mf_cdiv(r, 32), 1, 1024); pl.lds = (int)((C + 32 * 33) * sizeof(float)); break;
        case MF_SE_WGRAD:      pl = mf_plan_of(kernel, mf_cdiv((long)C * r, 256), 1, 1, 256); break;
        case MF_SE_DM:         pl = mf_plan_of(kernel, N, mf_cdiv(C, 32), 1, 1024); break;
    }
    return pl;
}
// channels-last (vox, C) <-> planar (K, vox) of the first K channels, a 64-channel tile in LDS
static GluePlan mf_cl_planar_plan(int N, long vox, int C, int K) {
    const long bx = mf_cdiv(vox, 128);
    if (C > 64 || (C & 3) || K > C || K < 1 || bx > 0x7FFFFFFFL) return MF_NO_PLAN;
    return mf_plan_of(MF_CL_PLANAR, bx, N, 1, 256);
}

// rsuper_mf_plan: the plan of one launch from the shape alone (MfOp names the shape's entries).  *ws: what the caller allocates for it -- bytes of the
// packed fragments (MF_OP_PW_PACK), floats of the weight-gradient workspace (MF_OP_PW_WGRAD), else 0.
static int mf_plan_query(int op, int dtype, const int* s, GluePlan* out, long* ws) {
    static const int ndims[MF_OP_COUNT] = {2, 1, 3, 3, 3, 5, 5, 5, 4, 4, 4, 3, 3, 3, 3, 3, 4};
    if (op < 0 || op >= MF_OP_COUNT || !dt_ok(dtype) || !s) return RS_ERR_ARG;
    const bool norm = op == MF_OP_CNORM || op == MF_OP_CNORM_STATS || op == MF_OP_CNORM_APPLY;
    for (int i = 0; i < ndims[op] - (norm ? 1 : 0); ++i) if (s[i] <= 0) return RS_ERR_ARG;
    *ws = 0;
    switch (op) {
        case MF_OP_PW_PACK: *out = mf_pw_pack_plan(dtype, s[0], s[1]); *ws = (long)mf_pw_packed_bytes(dtype, s[0], s[1]); break;
        case MF_OP_PW_PACK_BATCH: *out = mf_pw_pack_batch_plan(dtype, s[0]); break;
        case MF_OP_PW:
            if (s[2] % 4) return RS_ERR_ARG;
            *out = mf_pw_plan(dtype, s[0], s[1], s[2]);
            break;
        case MF_OP_PW_WGRAD: case MF_OP_PW_WGRAD_REDUCE: {
            if ((s[1] % 4) || (s[2] % 4)) return RS_ERR_ARG;
            const GluePlan wg = mf_pw_wgrad_plan(dtype, s[0], s[1], s[2], 0);
            *out = op == MF_OP_PW_WGRAD ? wg : mf_pw_wgrad_reduce_plan(s[1], s[2], wg.rows);
            *ws = op == MF_OP_PW_WGRAD ? (long)wg.rows * ((long)s[1] * s[2] + s[1]) : 0;
            return RS_OK;                                    // no reduce launch is an answer, not a refusal
        }
        case MF_OP_DW: case MF_OP_DW_WGRAD: case MF_OP_DW_WGRAD_REDUCE:
            if (s[4] & 3) return RS_ERR_ARG;
            *out = op == MF_OP_DW ? mf_dw_plan(s[0], s[1], s[2], s[3], s[4]) : op == MF_OP_DW_WGRAD ? mf_dw_wgrad_plan(s[0], s[1], s[2], s[3], s[4])
                                                                                                  : mf_dw_wgrad_reduce_plan(s[0], s[1], s[2], s[3], s[4]);
            break;
        case MF_OP_CNORM: case MF_OP_CNORM_STATS: case MF_OP_CNORM_APPLY:
            if ((s[2] & 3) || s[3] < 0 || s[3] > (op == MF_OP_CNORM_APPLY ? 2 : 1)) return RS_ERR_ARG;
            *out = op == MF_OP_CNORM ? mf_cnorm_plan(s[0], s[1], s[2], s[3]) : op == MF_OP_CNORM_STATS ? mf_cnorm_stats_plan(s[0], s[1], s[2], s[3])
                                                                                                      : mf_cnorm_apply_plan(s[0], s[1], s[2], s[3]);
            break;
        case MF_OP_SE_HIDDEN: case MF_OP_SE_GATE: case MF_OP_SE_BWD_HIDDEN: case MF_OP_SE_WGRAD: case MF_OP_SE_DM:
            if (s[1] & 3) return RS_ERR_ARG;
            *out = mf_se_plan(MF_SE_HIDDEN_FWD + (op - MF_OP_SE_HIDDEN), s[0], s[1], s[2]);
            break;
        case MF_OP_CL_PLANAR: *out = mf_cl_planar_plan(s[0], s[1], s[2], s[3]); break;
    }
    return out->kernel == MF_NONE ? RS_ERR_UNSUPPORTED : RS_OK;
}
