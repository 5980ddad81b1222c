// The dispatch of the bandwidth-bound "glue" kernels of unet_misc.hip (InstanceNorm backward tail, max pool, stride-2 subsample, trilinear up-sampling),
// host only: WHICH kernel a launch runs, with which template selector, grid, workgroup, LDS and statistics rows.  Nothing here launches anything and
// nothing elsewhere decides: api.hip asks one glue_*_plan per entry point and hands the GluePlan (misc.hpp) to a launcher that only switches over it;
// rsuper_glue_plan / rsuper_stat_rows give the same answers to tests and to the modules that allocate `part`.  A new kernel or grid of the family is
// taught to this file and to the launcher's switch.  Included by api.hip only (before lazy_tail_plan.hpp, whose trilinear answer reads glue_up_bwd_plan);
// tests/test_glue_plan_cpu.py pins every answer against the launches recorded in tests/golden/glue_launches.json.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "common.hpp"
#include "misc.hpp"
#include "up_coord.hpp"

// The switches of the family, read from the environment once:
//   RSUPER_GLUE_KERNELS=0    the kernels and grids that in_bwd_finalize2, maxpool_fwd2, upsample_fwd3 and the channel-split grids replaced
//                            (rs_glue_variant; also settable through the C ABI, and read by loss.hip)
//   RSUPER_UPSAMPLE_BWD4=0   the trilinear backward on the gather kernel instead of the row-sharing one (tools/bench_up.py)
struct GlueSwitches { int variant; bool bwd4; };
static GlueSwitches& glue_switches() {
    static GlueSwitches s = [] {
        auto off = [](const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; };
        return GlueSwitches{!off("RSUPER_GLUE_KERNELS"), !off("RSUPER_UPSAMPLE_BWD4")};
    }();
    return s;
}
// 1 (default): the tuned kernels of this family and of loss.hip (pipelined plane_partials_fwd); 0: the ones they replaced (A/B runs and
// tests/test_gpu_glue_kernels.py: results are bit-identical).  Other values query.
int rs_glue_variant(int v) {
    if (v == 0 || v == 1) glue_switches().variant = v;
    return glue_switches().variant;
}

static const GluePlan GLUE_NO_PLAN = {GLUE_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static GluePlan glue_plan_of(int kernel, int dtype, int bx, int N, int threads, size_t lds) { return {kernel, 0, bx, N, 1, threads, (int)lds, 0, dtype, 0}; }
static inline int glue_kp(int dtype) { return dtype == RS_F32 ? 4 : 8; }      // elements of a 16-byte vector

// Rows of `part` of the forwards that write statistics rows -- the caller allocates them, and they are gridDim.x of the kernel.
int rs_stat_rows(int op, long vox) {
    if (vox < 0) return 0;
    if (op == GLUE_OP_POOL_FWD || op == GLUE_OP_SUB_FWD || op == GLUE_OP_UP_FWD) return (int)(vox / 64 > 2048 ? 2048 : vox / 64 < 1 ? 1 : vox / 64);
    if (op == GLUE_OP_STEM_FWD) return (int)((vox + 255) / 256);              // one row per 256-voxel block of the stem kernels
    return 0;
}

// Channel split of the kernels that write statistics rows (max pool, subsample, trilinear forward): `rows` is the row count of `part` and their
// gridDim.x.  Where rows * N leaves most of the chip idle, z blocks of CV / z channel vectors (at least 128 bytes of a voxel, at least one wave)
// share a row.
static int stat_csplit(int rows, int N, int CV) {
    if (!rs_glue_variant(-1)) return 1;
    const int VL = 256 / CV;
    int z = 1;
    while ((size_t)rows * N * z < 1024 && CV % (2 * z) == 0 && CV / (2 * z) >= 8 && (CV / (2 * z)) * VL >= 64) z *= 2;
    return z;
}
// A statistics-row kernel on the channel-split grid: 256 / CV voxel lanes x CV / z channel vectors per block, the scratch of its channels
static GluePlan stat_rows_plan(int kernel, int dtype, int rows, int N, int CV, int z, size_t smem, size_t tab) {
    GluePlan pl = glue_plan_of(kernel, dtype, rows, N, z == 1 ? 256 : (CV / z) * (256 / CV), smem / z + tab);
    pl.bz = z; pl.rows = rows;
    return pl;
}
static inline size_t stat_smem(int CV, int C) { return (size_t)(256 / CV) * C * 2 * sizeof(float); }      // block_channel_sums' scratch

// InstanceNorm backward tail over N x vox x C.  One or two vectors per thread on the looping grid's 256 ... 8192 blocks (up to 48^3 x 128 channels at
// bf16): in_bwd_finalize2 gives a thread several vectors, all loads up front.  Larger tensors loop on 4096 blocks and run at the HBM rate already.
static GluePlan glue_in_bwd_plan(int dtype, int N, int vox, int C) {
    const uint32_t CV = (uint32_t)(C / glue_kp(dtype));
    const size_t vecs = (size_t)vox * (C / glue_kp(dtype));
    if (vecs >= 0xFFFFFFFFull) return GLUE_NO_PLAN;
    const size_t nb1 = (vecs + 255) / 256;
    if (rs_glue_variant(-1) && CV > 0 && (CV & (CV - 1)) == 0 && CV <= 256 && nb1 >= 256 && nb1 <= 8192) {
        const int U = nb1 >= 1024 ? 4 : 2;
        GluePlan pl = glue_plan_of(GLUE_IN_BWD2, dtype, (int)((nb1 + U - 1) / U), N, 256, 0);
        pl.sel = U; pl.arg = __builtin_ctz(CV);
        return pl;
    }
    return glue_plan_of(GLUE_IN_BWD, dtype, rs_elem_blocks(vecs), N, 256, 0);
}

// MaxPool3d(2) forward; rows: the rows of `part` the caller allocated (the voxel walk follows from them, not from the shape)
static GluePlan glue_pool_fwd_plan(int dtype, int N, int C, int rows) {
    const int CV = C / glue_kp(dtype);
    if (CV > 256) return GLUE_NO_PLAN;
    if (rs_glue_variant(-1) && (size_t)rows * N < 1024)         // small volumes: channel-split grid, four voxels of loads in flight
        return stat_rows_plan(GLUE_POOL_FWD2, dtype, rows, N, CV, stat_csplit(rows, N, CV), stat_smem(CV, C), 0);
    return stat_rows_plan(GLUE_POOL_FWD, dtype, rows, N, CV, 1, stat_smem(CV, C), 0);
}
static GluePlan glue_pool_bwd_plan(int dtype, int N, int D, int H, int W, int C) {
    const int CV = C / glue_kp(dtype);
    if (CV > 256) return GLUE_NO_PLAN;
    const size_t items = (size_t)(D / 2) * (H / 2) * (W / 2) * CV;
    const int b = rs_elem_blocks(items);
    if (rs_glue_variant(-1) && (size_t)b * N < 512) return glue_plan_of(GLUE_POOL_BWD, dtype, (int)((items + 63) / 64), N, 64, 0);   // small volumes: one wave per block, four times the CUs
    return glue_plan_of(GLUE_POOL_BWD, dtype, b, N, 256, 0);
}

// Stride-2 subsample forward (rows as above) and its scatter backward into an (N, D, H, W, C) gradient
static GluePlan glue_sub_fwd_plan(int dtype, int N, int C, int rows) {
    const int CV = C / glue_kp(dtype);
    if (CV > 256) return GLUE_NO_PLAN;
    return stat_rows_plan(GLUE_SUB_FWD, dtype, rows, N, CV, stat_csplit(rows, N, CV), stat_smem(CV, C), 0);
}
static GluePlan glue_sub_bwd_plan(int dtype, int N, int D, int H, int W, int C) {
    const int CV = C / glue_kp(dtype);
    if (CV > 256) return GLUE_NO_PLAN;
    return glue_plan_of(GLUE_SUB_BWD, dtype, rs_elem_blocks((size_t)D * H * W * CV), N, 256, 0);
}

// Trilinear forward I -> O; ldx: row stride of the input (the kernels after the first generation address it with 32-bit offsets).  The table-driven
// kernel where its per-axis tables fit 64 KB next to the statistics scratch, on the channel-split grid.
static GluePlan glue_up_fwd_plan(int dtype, int N, int ID, int IH, int IW, int OD, int OH, int OW, int C, int ldx, int rows) {
    const int CV = C / glue_kp(dtype);
    if (CV > 256) return GLUE_NO_PLAN;
    const size_t smem = stat_smem(CV, C), tab3 = (size_t)(OD + OH + OW) * sizeof(UpTab);
    const bool small = (size_t)N * ID * IH * IW * ldx < 0x7FFFFFFFull;
    if (!small) return stat_rows_plan(GLUE_UP_FWD, dtype, rows, N, CV, 1, smem, 0);
    if (rs_glue_variant(-1) && (size_t)ID * IH * IW * ldx * (dtype == RS_F32 ? 4 : 2) < 0xFFFFFFFFull && smem + tab3 <= 64 * 1024)
        return stat_rows_plan(GLUE_UP_FWD3, dtype, rows, N, CV, stat_csplit(rows, N, CV), smem, tab3);
    return stat_rows_plan(GLUE_UP_FWD2, dtype, rows, N, CV, 1, smem, 0);
}

// largest number of contributing outputs of any input index of one axis (the arithmetic of the kernel: lin_coord is not contracted on either side)
static int up_max_count(int I, int O) {
    const float sc = O > 1 ? (float)(I - 1) / (float)(O - 1) : 0.f;
    int m = 1;
    for (int i = 0; i < I; ++i) {
        int lo, hi;
        up_range(i, sc, O, lo, hi);
        int first = -1, last = -2;
        for (int o = lo; o <= hi; ++o)
            if (up_weight(o, i, sc, I) != 0.f) { if (first < 0) first = o; last = o; }
        if (last - first + 1 > m) m = last - first + 1;
    }
    return m;
}
static int up_pair_window(int I, int O) {                        // widest candidate window (up_range) of an aligned pair of input indices
    const float sc = O > 1 ? (float)(I - 1) / (float)(O - 1) : 0.f;
    int m = 1;
    for (int i = 0; i < I; i += 2) {
        int lo, hi, lo2, hi2;
        up_range(i, sc, O, lo, hi);
        if (i + 1 < I) { up_range(i + 1, sc, O, lo2, hi2); if (hi2 > hi) hi = hi2; }
        if (hi - lo + 1 > m) m = hi - lo + 1;
    }
    return m;
}
// NT of upsample_bwd4_kernel for a scale its tile tables hold (4 or 6), else 0.  The table sizes depend on the shape only: remembered per
// (ID, IH, IW, OD, OH, OW) (the host loops cost a few microseconds per call otherwise)
static int up_bwd4_nt(int ID, int IH, int IW, int OD, int OH, int OW) {
    struct Memo { int k[6]; int ok, nmax; };
    static thread_local Memo memo[8] = {};
    static thread_local int memo_next = 0;
    const int key[6] = {ID, IH, IW, OD, OH, OW};
    const Memo* hit = nullptr;
    for (int i = 0; i < 8 && !hit; ++i) if (memo[i].k[0] && !memcmp(memo[i].k, key, sizeof(key))) hit = &memo[i];
    if (!hit) {
        Memo& m = memo[memo_next++ & 7];
        memcpy(m.k, key, sizeof(key));
        m.ok = up_pair_window(ID, OD) <= UP4_ROWS && up_pair_window(IH, OH) <= UP4_ROWS;
        m.nmax = up_max_count(IW, OW);
        hit = &m;
    }
    return !hit->ok || hit->nmax > 6 ? 0 : hit->nmax <= 4 ? 4 : 6;
}

// Trilinear backward O -> I; ld: the widest row stride of what the kernel reads on the output grid (the gradient; with a lazy gradient also the
// up-sampled tensor).  bf16: the row-sharing kernel (upsample_bwd4) where its tile tables hold the scale; else the gather kernel on per-axis tables,
// or the first-generation one beyond 32-bit offsets.  Contributing outputs per input index < 2 * (O-1)/(I-1) + 2: the table kernel holds
// UP_MAXW = 12 (up to 4x: the aux head); larger scales have no kernel.
static GluePlan glue_up_bwd_plan(int dtype, int N, int ID, int IH, int IW, int OD, int OH, int OW, int C, int ld) {
    const int CV = C / glue_kp(dtype);
    if (CV > 256) return GLUE_NO_PLAN;
    auto ratio = [](int O, int I) { return I > 1 ? (double)(O - 1) / (double)(I - 1) : (double)O; };
    const double rmax = fmax(ratio(OD, ID), fmax(ratio(OH, IH), ratio(OW, IW)));
    if (2.0 * rmax + 2.0 > (double)UP_MAXW + 1e-9) return GLUE_NO_PLAN;
    const size_t obytes = (size_t)OD * OH * OW * (size_t)ld * (dtype == RS_F32 ? 4 : 2);
    if (dtype == RS_BF16 && glue_switches().bwd4 && (C % 8) == 0 && N <= 65535 && obytes < 0xFFFFFFFFull) {      // 32-bit byte offsets
        if (const int nt = up_bwd4_nt(ID, IH, IW, OD, OH, OW)) {
            const int nbx = (IW * (C / 8) + 255) / 256;
            GluePlan pl = glue_plan_of(GLUE_UP_BWD4, dtype, ((ID + 1) / 2) * ((IH + 1) / 2) * nbx, N, 256, 0);
            pl.sel = nt; pl.arg = nbx;
            return pl;
        }
    }
    const int b = rs_elem_blocks((size_t)ID * IH * IW * CV);
    const size_t tab = (size_t)(ID + IH + IW) * sizeof(UpEnt);
    const bool small = obytes < 0xFFFFFFFFull && (size_t)ID * IH * IW * CV < 0xFFFFFFFFull && tab <= 48 * 1024;
    return small ? glue_plan_of(GLUE_UP_BWD2, dtype, b, N, 256, tab) : glue_plan_of(GLUE_UP_BWD, dtype, b, N, 256, 0);
}

// rsuper_glue_plan: the plan of one launch from the shape alone (the rows of the forwards are rs_stat_rows').  shape: N, then D, H, W of the input
// (pool, subsample), ID, IH, IW, OD, OH, OW (trilinear) or vox (tail); ld: the row stride glue_up_fwd_plan / glue_up_bwd_plan look at.
static int glue_plan_query(int op, int dtype, const int* s, int C, int ld, GluePlan* out) {
    if (!dt_ok(dtype) || !s || C <= 0 || (C % 8) || (ld % 8) || ld < C || s[0] <= 0) return RS_ERR_ARG;
    const int ndims = op == GLUE_OP_IN_BWD ? 1 : (op == GLUE_OP_UP_FWD || op == GLUE_OP_UP_BWD) ? 6 : 3;
    for (int i = 1; i <= ndims; ++i) if (s[i] <= 0) return RS_ERR_ARG;
    if (s[0] > 65535) return RS_ERR_UNSUPPORTED;                 // N is gridDim.y: the launch itself fails
    const int N = s[0];
    switch (op) {
        case GLUE_OP_IN_BWD: *out = glue_in_bwd_plan(dtype, N, s[1], C); break;
        case GLUE_OP_POOL_FWD:
            if (s[1] < 2 || s[2] < 2 || s[3] < 2) return RS_ERR_ARG;
            *out = glue_pool_fwd_plan(dtype, N, C, rs_stat_rows(op, (long)(s[1] / 2) * (s[2] / 2) * (s[3] / 2)));
            break;
        case GLUE_OP_POOL_BWD: *out = glue_pool_bwd_plan(dtype, N, s[1], s[2], s[3], C); break;
        case GLUE_OP_SUB_FWD:
            *out = glue_sub_fwd_plan(dtype, N, C, rs_stat_rows(op, (long)((s[1] + 1) / 2) * ((s[2] + 1) / 2) * ((s[3] + 1) / 2)));
            break;
        case GLUE_OP_SUB_BWD: *out = glue_sub_bwd_plan(dtype, N, s[1], s[2], s[3], C); break;
        case GLUE_OP_UP_FWD:
            *out = glue_up_fwd_plan(dtype, N, s[1], s[2], s[3], s[4], s[5], s[6], C, ld, rs_stat_rows(op, (long)s[4] * s[5] * s[6]));
            break;
        case GLUE_OP_UP_BWD: *out = glue_up_bwd_plan(dtype, N, s[1], s[2], s[3], s[4], s[5], s[6], C, ld); break;
        default: return RS_ERR_ARG;
    }
    return out->kernel == GLUE_NONE ? RS_ERR_UNSUPPORTED : RS_OK;
}
