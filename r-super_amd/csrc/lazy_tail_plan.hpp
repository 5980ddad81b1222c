// Where an InstanceNorm backward tail runs inside the kernel that consumes its result, host only.  The tail dx = rstd (g - mean(g) - x_n mean(g x_n))
// of a convolution input whose only reader is the next backward kernel need not be a launch and a tensor of its own: that kernel can take the raw data
// gradient g with the statistics and apply the tail as it reads ("lazy" gradient).  Nothing here launches anything and nothing elsewhere decides:
// api.hip's queries (rsuper_maxpool2_bwd_lazy_plan / rsuper_upsample_bwd_lazy_plan, which the modules ask before they hand out a differentiable
// statistics tensor) and its launches (rsuper_maxpool2_bwd_lazy / rsuper_upsample_bwd_lazy) read lazy_pool_plan / lazy_up_plan.  Included by api.hip
// only (after its dt_ok helper and glue_plan.hpp); tests/test_lazy_tail_plan_cpu.py pins the answers.
#pragma once
#include <stdlib.h>
#include "common.hpp"

// 1 (default): lazy gradients where the plans below admit them; 0: every tail is its own launch (A/B runs and tests/test_gpu_lazy_tails.py: results are
// bit-identical); 2: wherever a fused kernel can take the launch, measured faster or not (tools/bench_lazy_tails.py measures both forms with it).
// RSUPER_LAZY_TAILS in the environment selects the value at start-up.  Other values query.
static int lazy_tails_variant(int v) {
    static int g = getenv("RSUPER_LAZY_TAILS") ? atoi(getenv("RSUPER_LAZY_TAILS")) : 1;
    if (v >= 0 && v <= 2) g = v;
    if (g < 0 || g > 2) g = 1;
    return g;
}

// Max-pool backward of an (N, D, H, W, C) input with one or both gradients lazy: 1 = the fused kernel, 0 = in_bwd_finalize first.
// The tail needs the norm's forward input, which the kernel holds already (x of the 2x2x2 cell for the skip gradient, the cell's maximum for the pooled
// gradient), and g is read in place of the finished gradient: no byte more than the launch it was.
// Odd sizes stay on two launches (the never-pooled trailing planes take the skip gradient alone: rsuper_maxpool2_bwd_add refuses them too).
static int lazy_pool_plan(int dtype, int N, int D, int H, int W, int C) {
    if (!dt_ok(dtype) || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return -1;
    if (!lazy_tails_variant(-1)) return 0;
    const int KP = dtype == RS_F32 ? 4 : 8;
    if ((D & 1) || (H & 1) || (W & 1) || (C % 8) || C / KP > 256 || N > 65535) return 0;      // channel counts as every entry of the library takes them (ch_ok)
    return 1;
}

// Trilinear backward (I -> O, C channels) of a lazy gradient: 1 = upsample_bwd4_kernel's lazy instantiation, 0 = in_bwd_finalize first.
// bf16 only: the f32 mode and the first-generation kernels finalise first.  The row-sharing kernel reads every output-gradient vector from several
// (d, h, w) positions, so the tail is computed several times over where in_bwd_finalize computes it once at the HBM rate, and the second operand
// buffers and 32 constants per thread halve its occupancy (184 VGPRs against 98).  Measured on MI355X inside the UNet step (kernel trace of bench.py,
// B = 2, 9 steps, profiles/lazy_in_bwd_tails.md), in_bwd_finalize + upsample_bwd4 against the fused launch:
//     48^3 -> 96^3 x  64    ~122 + 88.8 us   211.1 us      (alone, back to back: 123.9 + 70.9 against 193.0 us)
//     24^3 -> 48^3 x 128    28.5 + 27.4 us    71.9 us      (26.1 + 23.5 against 60.3 us)
//     12^3 -> 24^3 x 256     9.9 + 17.0 us    29.5 us      ( 8.7 + 12.6 against 26.2 us)
//      6^3 -> 12^3 x 320    ~5.2 + 16.1 us    27.8 us      ( 8.4 + 11.8 against 22.3 us)
// No gain at 96^3 and a loss at the three smaller shapes, and nothing suggests a shape in between where it would win: the default keeps two launches
// everywhere.  The fused kernel stays selectable (rsuper_lazy_tails(2)) for tests and for measuring a changed kernel, and only where the trilinear
// backward's own plan (glue_plan.hpp) names the row-sharing kernel: a scale its tile tables do not hold, or RSUPER_UPSAMPLE_BWD4=0, answers 0 here, so
// no module hands out a differentiable statistics tensor for a launch that will not happen.  Asked for dense tensors (row stride C); the launch
// asks again with the strides it got.
static int lazy_up_plan(int dtype, int N, int ID, int IH, int IW, int OD, int OH, int OW, int C) {
    if (!dt_ok(dtype) || N <= 0 || ID <= 0 || IH <= 0 || IW <= 0 || OD <= 0 || OH <= 0 || OW <= 0 || C <= 0) return -1;
    if (dtype != RS_BF16 || (C % 8) || N > 65535 || lazy_tails_variant(-1) != 2) return 0;
    return glue_up_bwd_plan(dtype, N, ID, IH, IW, OD, OH, OW, C, C).kernel == GLUE_UP_BWD4;
}
