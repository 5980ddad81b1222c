// The dispatch of the 3x3x3 implicit GEMMs, host only: WHICH kernel a launch runs, with which block width, writing how many statistics rows.
// Nothing here launches anything and nothing elsewhere decides: api.hip's queries (rsuper_conv3_plan / _part_rows / _kd_bn / _box_bn / _s2_part_rows) and
// its launches (rsuper_conv3_igemm / _igemm_s2) read igemm_plan / s2_kernel.  A new kernel of the family is taught to this file and to the switch in
// rs_launch_igemm.  Included by api.hip only (after its dt_ok / bn_ok helpers); tests/test_dispatch_cpu.py pins every answer.
#pragma once
#include <stdlib.h>
#include "common.hpp"
#include "kernels.hpp"
#include "../../include/rsuper_hip.h"

static int g_variant = 3;            // rsuper_conv3_variant

// variant 2 (auto, default): producer/consumer kernel where it measured faster on MI355X -- data-gradient launches with
// bn <= 64 (its epilogue operand prefetch), all 32-column launches, and small grids (persistent blocks fill the chip);
// classic kernel elsewhere.
// variant 3 (default): as variant 2, and 32-column launches over a single 32-channel K chunk (the 32 -> 32 layers at full
// resolution) run the weight-stationary kernel (conv3d_igemm_ws.hip), which writes the same partial rows as the
// producer/consumer kernel.  variant 4: weight-stationary kernel for every bf16 32-column launch (multi-chunk too; tests).
static bool use_pc(int dtype, int epi, int bn, int tiles_total) {
    if (dtype != RS_BF16) return false;
    if (g_variant == 4) return bn == 32 || (bn <= 64 && (epi == 1 || tiles_total <= 1024));
    if (g_variant == 2 || g_variant == 3) return bn <= 64 && (epi == 1 || bn == 32 || tiles_total <= 1024);
    return g_variant == 1;
}

// Volume-fitted K-split kernel (conv3d_igemm_box.hip) for launches that cannot fill the chip with 4x4x16-voxel tiles: bf16, more than
// 32 columns, and fewer than 512 classic work items (the 24^3 / 12^3 / 6^3 levels at batch 2).  Shapes 1 / 2 (4x4x8 / 4x4x4 boxes) take
// 64-column blocks; shape 3 (volumes of at most 6x6x6: one box per sample, the reduction split over blocks through the registered
// workspace, second pass box_splitk_epilogue_kernel) takes 32-column blocks.  Variants 6 / 7 force the kernel for every bf16 launch
// (6: shape chosen per volume, 7: the 4x4x4 box) -- test paths.
// one registered workspace PER DEVICE (indexed by the current HIP device of the calling thread: a host that drives several GPUs from one process
// registers one on each); launches on two streams of the same device share it and must not overlap 6^3-level convolutions
static const int RS_MAX_DEVICES = 64;
static void* g_ws_dev[RS_MAX_DEVICES] = {nullptr};
static size_t g_ws_bytes_dev[RS_MAX_DEVICES] = {0};
static int ws_dev() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= RS_MAX_DEVICES) return 0;
    return d;
}
#define g_ws (g_ws_dev[ws_dev()])
#define g_ws_bytes (g_ws_bytes_dev[ws_dev()])
static const size_t BOXC_WS_BYTES = (size_t)256 * 216 * 32 * 4;    // nsplit x N x 216 x n_cols floats while N x ceil(n_cols / 32) <= 256 (rs_box_nsplit)
// Bytes the split shape writes into the workspace: nsplit x N x voxels x n_cols floats.  rs_box_nsplit deals at most 256 / (N x groups) splits (at least
// one), so beyond N x groups = 256 the requirement grows with N x n_cols without bound -- the shape is only taken while it fits what the caller registered.
static size_t boxc_ws_need(int nsplit, int N, int D, int H, int W, int n_cols) {
    return (size_t)nsplit * (size_t)N * (size_t)(D * H * W) * (size_t)n_cols * sizeof(float);
}
static bool boxc_fits(int N, int D, int H, int W, int n_cols) {
    const int groups = (n_cols + 31) / 32;
    const long ng = (long)N * groups;
    const int smax = ng >= 256 ? 1 : (int)(256 / ng);
    return g_ws && boxc_ws_need(smax, N, D, H, W, n_cols) <= g_ws_bytes;
}
static int box_shape(int dtype, int N, int D, int H, int W, int n_cols) {
    if (dtype != RS_BF16) return 0;
    const bool forced = g_variant == 6 || g_variant == 7;
    static const int off = getenv("RSUPER_NO_BOX") ? atoi(getenv("RSUPER_NO_BOX")) : 0;      // 1: no box kernel, 2: no split shape
    if (!forced && (g_variant != 3 || off == 1 || n_cols <= 32)) return 0;
    if (g_variant != 7 && off != 2 && D <= 6 && H <= 6 && W <= 6 && boxc_fits(N, D, H, W, n_cols)) return 3;
    if (g_variant == 7) return 2;
    if (!forced && (long)N * rsuper_conv3_tiles(D, H, W) * ((n_cols + 127) / 128) >= 512) return 0;
    return rs_box_config(N, D, H, W, n_cols);
}
// Depth-reuse kernel (conv3d_igemm_kd.hip, round 5): bf16 launches with more than 32 columns whose volume gives the persistent blocks enough 4 x 8 x 16-voxel
// tiles (the full-resolution level at batch 2: 3456 tiles; KD_MIN_TILES).  Forward launches (normalised sources, staging with arithmetic in registers)
// take 64-column blocks; data-gradient launches (raw dY) 64 / 96 / 128.  Variant 8 forces it wherever its limits allow (tests).
static const int KD_MIN_TILES = 400;
static int kd_bn_for(int dtype, int epi, int N, int D, int H, int W, int n_cols, int src_flags) {
    if (dtype != RS_BF16 || n_cols <= 32) return 0;
    if (src_flags & 1) return 0;        // one normalised and one raw source: the depth-reuse kernel stages both sources the same way (rs_igemm_kd_supported)
    static const int off = getenv("RSUPER_KD") ? atoi(getenv("RSUPER_KD")) == 0 : 0;
    static const int dgrad = getenv("RSUPER_KD_DGRAD") ? atoi(getenv("RSUPER_KD_DGRAD")) : 0;
    static const int wide = getenv("RSUPER_KD_WIDE") ? atoi(getenv("RSUPER_KD_WIDE")) : 0;
    if (g_variant != 8 && (g_variant != 3 || off)) return 0;
    if ((long)N * D * H * W >= (1l << 24) || D > 1023 || H > 1023 || W > 1023) return 0;
    if (g_variant != 8) {
        // measured (profiles/r05_conv_layers.txt, same box): forward launches of exactly 33 .. 64 columns at 96^3 / 48^3 gain 10-11 % (up4.0 648 -> 576 us,
        // 64 -> 64 @48^3 60 -> 54 us); 128-column forwards (two column blocks) and the data gradients do not beat the 128-column classic / producer-consumer
        // kernels yet -- they stay selectable (RSUPER_KD_DGRAD=1) and run every parity case under variant 8
        const long tiles = (long)N * ((D + 3) / 4) * ((H + 7) / 8) * ((W + 15) / 16);
        if (tiles < KD_MIN_TILES) return 0;
        if (epi == 0 && n_cols > 64) return 0;
        if (epi == 1 && !dgrad) return 0;
    }
    // one column fragment per wave (64-column blocks): two fragments per wave (96 / 128-column blocks, raw sources by LDS-DMA) do not fit the register file
    // without spills yet and measured slower (up4.0 data gradient: 96-column blocks 733 us against 705 us for 2 x 64); RSUPER_KD_WIDE=1 selects them
    if (epi == 0 || !wide) return 64;
    const int r = n_cols % 128;
    return (n_cols > 128 || r == 0) ? 128 : r > 96 ? 128 : r > 64 ? 96 : 64;
}
// Block width of a launch whose kernel does not prescribe one: 32 / 64 / 128 columns (f32 parity mode: at most 64).  tiles_total = 4x4x16-voxel tiles x batch
// (0: no volume given): on small volumes the largest width that still yields >= BN_FILL workgroups (24^3 and below would otherwise leave most of the 256 CUs
// idle; the narrower widths also run on the persistent kernels), else the width with the least padding, the wider one on a tie.
static const int BN_FILL = 512;      // two resident blocks per CU (measured 128 / 256 / 512: 13.89 / - / 13.80 ms per step)
static int free_bn(int dtype, int n_cols, long tiles_total) {
    const bool bf = dtype == RS_BF16;
    const int widest = bf ? 128 : 64;
    if (n_cols <= 32) return 32;
    if (bf && g_variant == 4) return 32;                           // forced weight-stationary kernel (tests / experiments): n_cols / 32 blocks in grid.y
    if (tiles_total > 0 && tiles_total * ((n_cols + 127) / 128) < BN_FILL) {
        for (int bn = widest; bn > 32; bn >>= 1)
            if (tiles_total * ((n_cols + bn - 1) / bn) >= BN_FILL) return bn;
        return 32;
    }
    // e.g. 96 columns (up4.0 data gradient): three exact 32-column tiles on the producer/consumer kernel (671 us) beat one 25 %-padded 128 tile on the
    // classic kernel (739 us)
    if (bf && n_cols > 64 && n_cols % 64) return 32;
    int best = 32;
    for (int bn = 64; bn <= widest; bn <<= 1)
        if ((n_cols + bn - 1) / bn * bn <= (n_cols + best - 1) / best * best) best = bn;
    return best;
}

// THE dispatch of the stride-1 3x3x3 implicit GEMM: which kernel, which block width, how many statistics rows.  Every query below and the launch read this one
// function, so `bn` (the weights are packed for it), the rows of `part` (the caller allocates them) and the kernel that runs cannot disagree.
//   bn = 0: choose the width -- the depth-reuse kernel's where it takes the launch, else the volume-fitted kernel's, else free_bn.
//   bn != 0: plan for that width (weights already packed): a kernel with a width of its own runs only where bn is that width.
//   N = 0 (with bn = 0): a width query without a volume; only .bn is meaningful.  Arguments that describe no launch: NO_PLAN.
//   Ca, Cb: source channels (0, 0: unknown).  They decide between the producer/consumer and the weight-stationary kernel only, which write the same rows.
//   src_flags bit 0: one normalised and one raw source -- neither the depth-reuse nor the weight-stationary kernel stages those.
struct IgemmPlan { int kernel, bn, box_cfg, nsplit, part_rows; };
static const IgemmPlan NO_PLAN = {-1, 0, 0, 0, 0};
static IgemmPlan igemm_plan(int dtype, int epi, int N, int D, int H, int W, int Ca, int Cb, int n_cols, int src_flags, int bn) {
    if (!dt_ok(dtype) || n_cols <= 0 || Ca < 0 || Cb < 0 || (bn && !bn_ok(bn))) return NO_PLAN;
    if (N ? (epi != 0 && epi != 1) || N < 0 || D <= 0 || H <= 0 || W <= 0 : bn != 0) return NO_PLAN;
    IgemmPlan pl = {RS_IGEMM_CLASSIC, bn, 0, 0, 0};
    if (N == 0) {
        pl.bn = (dtype == RS_BF16 && (g_variant == 6 || g_variant == 7)) ? 64 : free_bn(dtype, n_cols, 0);   // forced volume-fitted kernel: its 64-column blocks
        return pl;
    }
    const int tiles = rsuper_conv3_tiles(D, H, W), nch = (Ca + 31) / 32 + (Cb + 31) / 32;
    const int kd_bn = kd_bn_for(dtype, epi, N, D, H, W, n_cols, src_flags);
    const int cfg = box_shape(dtype, N, D, H, W, n_cols), box_bn = cfg == 3 ? 32 : cfg ? 64 : 0;
    if (!bn) pl.bn = bn = kd_bn ? kd_bn : box_bn ? box_bn : free_bn(dtype, n_cols, (long)N * tiles);
    if (bn == kd_bn) {
        pl.kernel = RS_IGEMM_KD;
        pl.part_rows = rs_igemm_kd_part_rows(bn, N, D, H, W, n_cols);
    } else if (bn == box_bn) {
        pl.kernel = RS_IGEMM_BOX; pl.box_cfg = cfg;
        if (cfg == 3 && nch > 0) pl.nsplit = rs_box_nsplit(N, n_cols, nch);              // the reduction is split over the K chunks: needs Ca / Cb
        pl.part_rows = rs_box_part_rows(cfg, D, H, W);
    } else {
        const bool pc = use_pc(dtype, epi, bn, N * tiles);
        // variant 3: 32-column launches over a single 32-channel K chunk; variant 4: every 32-column launch
        const bool ws = pc && bn == 32 && !(src_flags & 1) && (g_variant == 4 || (g_variant == 3 && nch == 1));
        pl.kernel = ws ? RS_IGEMM_WS : pc ? RS_IGEMM_PC : RS_IGEMM_CLASSIC;
        pl.part_rows = rs_igemm_part_rows(bn, pc, tiles, n_cols, N);
    }
    return pl;
}

// the persistent strided forward (conv3d_igemm_s2k.hip) takes bf16 forward GEMMs with a 16-channel-aligned source; RSUPER_S2K=0: the parity-class kernel everywhere
static bool s2k_on() {                                                       // read per call (tests switch it inside one process)
    const char* e = getenv("RSUPER_S2K");
    return !(e && atoi(e) == 0);
}
static bool s2d_on() {                                                       // RSUPER_S2D=0: the parity-class data gradient
    const char* e = getenv("RSUPER_S2D");
    return !(e && atoi(e) == 0);
}
// The kernel of a stride-2 launch -- the one place it is chosen, read by the row count and by the launch.  mode 1: forward, mode 2: data gradient.
enum S2Kernel { S2_PARITY, S2_S2K, S2_S2D };
static S2Kernel s2_kernel(int dtype, int mode, int Ca, int Cb, int n_cols, int N, int FD, int FH, int FW) {
    if (mode == 1 && s2k_on() && rs_igemm_s2k_shape_ok(dtype, Ca, Cb, n_cols, N, FD, FH, FW)) return S2_S2K;
    if (mode == 2 && s2d_on() && rs_igemm_s2d_shape_ok(dtype, Ca, Cb, n_cols, N, FD, FH, FW)) return S2_S2D;
    return S2_PARITY;
}
