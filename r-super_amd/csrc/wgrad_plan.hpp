// The dispatch of the stride-1 3x3x3 weight gradient, host only: WHICH kernel a launch runs, in which configuration, over how many slabs.
// Nothing here launches anything and nothing elsewhere decides: api.hip's queries (rsuper_conv3_wgrad_plan / _wgrad_splits) and its launches
// (rsuper_conv3_wgrad / _wgrad_partial) read wgrad_plan, and rs_launch_wgrad switches over the plan it is handed.  A new kernel of the family is taught
// to this file and to that switch.  Included by api.hip only (after its dt_ok helper); tests/test_dispatch_cpu.py pins every answer.
// Every environment switch of the choice is read here, once per process.
#pragma once
#include <stdlib.h>
#include "common.hpp"
#include "kernels.hpp"
#include "../../include/rsuper_hip.h"

// Configuration of the tile-streaming kernel per launch (measured on MI355X, tools/bench_conv.py):
//   0: M <= 32           -> 32 rows x 27 taps, 8 waves (four taps per wave), one block per CU
//   1: M > 32, few tiles -> 64 rows x 9 taps (kd split over blocks), 4 waves, two blocks per CU
//   2: M > 32, >= 128 tiles (bf16) -> 64 rows x 27 taps, 8 waves, one block per CU: the x halo and the dY tile are staged
//      once for all 27 taps (2.4x less operand traffic than config 1), seven taps per A fragment
static int wgrad_config(int dtype, int Mtot, int tiles_total) {
    if (Mtot <= 32) return 0;
    return (dtype == RS_BF16 && tiles_total >= 128) ? 2 : 1;
}

// 64-row weight gradients with too few tiles for 64-row blocks of the second-generation kernel (the 64 -> 64 layers at 48^3: 864 tiles / 128 splits) run it
// as two 32-row blocks per chunk: half the splits, 13.5 tiles per block -- 64 -> 64 @48^3 72.5 -> 67.7 us (tools/bench_conv.py, same box).  RSUPER_WG2_MT1=0: off (A/B).
static bool wgrad2_mt1(int dtype, int Mtot, int tiles_total) {
    static const int on = getenv("RSUPER_WG2_MT1") ? atoi(getenv("RSUPER_WG2_MT1")) : 1;
    static const int maxm = getenv("RSUPER_WG2_MT1_MAXM") ? atoi(getenv("RSUPER_WG2_MT1_MAXM")) : 64;                // experiment knobs (tools/wg_mt1_exp.sh)
    static const int mint = getenv("RSUPER_WG2_MT1_MIN_TILES") ? atoi(getenv("RSUPER_WG2_MT1_MIN_TILES")) : 512;
    return on && dtype == RS_BF16 && Mtot >= 64 && Mtot <= maxm && (Mtot % 32) == 0 && tiles_total >= mint && tiles_total < 2048;
}

// slabs of the tile-streaming kernels (the first and the second generation share the count)
static int wgrad_tile_splits(int dtype, int Mtot, int nch, int tiles_total) {
    const int cfg = wgrad_config(dtype, Mtot, tiles_total);
    int gy = cfg == 0 ? 1 : (cfg == 1 ? 3 : 1) * ((Mtot + 63) / 64);
    if (wgrad2_mt1(dtype, Mtot, tiles_total)) gy = Mtot / 32;     // 32-row blocks on the second-generation kernel (twice the tiles per block, half the slab bytes)
    const int target = cfg == 1 ? 512 : 256;                     // resident blocks on 256 CUs
    int s = target / (nch * gy > 0 ? nch * gy : 1);
    if (s > tiles_total) s = tiles_total;
    return s < 1 ? 1 : s;
}

// tiles per block from which bf16 launches take the second-generation kernel (t < 0: query); rsuper_conv3_wgrad2_min_tiles
static int wgrad2_min_tiles(int t) {
    static int v = getenv("RSUPER_WGRAD2_MIN_TILES") ? atoi(getenv("RSUPER_WGRAD2_MIN_TILES")) : 12;
    if (t >= 0) v = t;
    return v;
}

// splits (= N x parts per sample) of the small-volume kernel, 0 when it does not apply: bf16, a slab of at least one plane fits LDS, at most 64 tiles of
// 4x4x16 voxels in the batch (the levels where the tile-streaming kernels sweep < 4 tiles per block), 32-row groups of dY inside one source each
static int wgrad_sv_splits(int dtype, int Mtot, int Ya, int nch, int N, int D, int H, int W) {
    static const int off = getenv("RSUPER_WGRAD_SV") ? atoi(getenv("RSUPER_WGRAD_SV")) == 0 : 0;
    const int w2 = wgrad2_min_tiles(-1);
    if (off || dtype != RS_BF16 || w2 == 0 || w2 >= (1 << 20)) return 0;      // 0 / "never": the tests force the tile-streaming kernels
    const long tiles = (long)N * ((D + 3) / 4) * ((H + 3) / 4) * ((W + 15) / 16);
    if (tiles > 64 || (Ya < Mtot && (Ya % 32))) return 0;
    // above 6^3 the kernel pays only while the whole launch is small: the wide fused [conv1 | shortcut] of up1.0 (512 rows x 18 input chunks at 12^3 = 288 output
    // tiles x N x depth parts blocks, each re-staging its slab) measured 180 us here against 120 us on the tile-streaming kernel; 256 -> 256 / 128 -> 2 x 256 at
    // 12^3 are equal on both, the 6^3 level is 20-25 % faster here (tools/r06_wgsv_exp.sh, profiles/r06_wgsv_exp.txt)
    static const long max_tiles12 = getenv("RSUPER_WGRAD_SV_MAX") ? atol(getenv("RSUPER_WGRAD_SV_MAX")) : 4096;
    if ((long)D * H * W > 216 && (long)Mtot * nch > max_tiles12) return 0;
    return N * rs_wgrad_sv_parts(N, D, H, W, nch, Mtot);
}

// what the second-generation kernel requires of a launch: bf16; 32-row groups of dY inside one source each (buffer resources are wave-uniform)
static bool wgrad2_supported(int dtype, int Ya, int Yb, int N, int src_flags) {
    static const int off = getenv("RSUPER_WGRAD2") ? atoi(getenv("RSUPER_WGRAD2")) == 0 : 0;
    if (off || dtype != RS_BF16 || N > 32) return false;        // per-sample constants table: 256 B of LDS per sample
    if (Yb > 0 && (Ya % 32)) return false;
    return !(src_flags & 1);                                    // both sources normalised or both raw, as everywhere
}

// THE dispatch of the stride-1 3x3x3 weight gradient.  The split query and the launch read this one function, so the slabs of the workspace (the caller
// allocates them) and the kernel that writes them cannot disagree.
//   splits = 0: choose the count -- the small-volume kernel's where it applies, else the tile-streaming kernels'.  It never depends on use_tr or src_flags.
//   splits != 0: plan for that count (workspace already sized): the small-volume kernel runs only where the count is its own.
//   use_tr = 0 (RSUPER_WGRAD_TR=0) and f32: the tile-streaming kernel without the transposed staging, whatever else holds.
//   src_flags bit 0: one normalised and one raw x source -- the second-generation kernel does not stage those.
//   .cfg: wgrad_config of the launch; .mt: 32-row groups of dY per block (the row form of the kernel).  Arguments that describe no launch: NO_WGRAD_PLAN.
static const WgradPlan NO_WGRAD_PLAN = {-1, 0, 0, 0};
static WgradPlan wgrad_plan(int dtype, int use_tr, int Ca, int Cb, int Ya, int Yb, int N, int D, int H, int W, int src_flags, int splits) {
    if (!dt_ok(dtype) || Ca <= 0 || Cb < 0 || Ya <= 0 || Yb < 0 || N <= 0 || D <= 0 || H <= 0 || W <= 0 || splits < 0) return NO_WGRAD_PLAN;
    const int nch = (Ca + 31) / 32 + (Cb + 31) / 32, Mtot = Ya + Yb;
    const int tiles_total = N * rsuper_conv3_tiles(D, H, W);
    const int cfg = wgrad_config(dtype, Mtot, tiles_total);
    // small volumes (12^3 / 6^3 levels): one depth slab of a sample whole in LDS (conv3d_wgrad_sv.hip), N x (depth parts per sample) slabs.  A fused
    // [conv1 | shortcut] whose first source is not a multiple of 32 rows does not take it, so its split count is not sized for it
    const int sv = wgrad_sv_splits(dtype, Mtot, Ya, nch, N, D, H, W);
    if (!splits) splits = sv ? sv : wgrad_tile_splits(dtype, Mtot, nch, tiles_total);
    WgradPlan pl = {RS_WGRAD_TILE, splits, cfg, cfg == 0 ? 1 : 2};
    if (dtype != RS_BF16 || !use_tr) return pl;
    if (sv > 0 && sv == splits) {
        pl.kernel = RS_WGRAD_SV; pl.mt = 1;
        return pl;
    }
    // Second-generation kernel (conv3d_wgrad2.hip: operand re-use across taps, double-buffered tiles) where a block sweeps enough tiles to amortise its
    // heavier prologue (descriptor / constants tables, two tiles staged before the first MFMA): measured same-box against the tile kernel, >= 12 tiles
    // per block 0.81-0.93x (32 -> 32 @96^3, up4.0, up3.0, up2.0), 6.75 tiles per block 1.02-1.08x (64 -> 64 @48^3, 128 -> 128 @24^3, down1.0).
    // What it does not take stays on the tile kernel: few tiles per block, the 9-tap configuration.
    if (cfg != 1 && (long)tiles_total >= (long)wgrad2_min_tiles(-1) * splits && wgrad2_supported(dtype, Ya, Yb, N, src_flags)) {
        pl.kernel = RS_WGRAD_2;
        pl.mt = (Mtot <= 32 || wgrad2_mt1(dtype, Mtot, tiles_total)) ? 1 : 2;
    }
    return pl;
}
