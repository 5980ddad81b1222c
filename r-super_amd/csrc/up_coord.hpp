// Trilinear (align_corners) coordinate arithmetic that the kernels of unet_misc.hip and the host-only dispatch of glue_plan.hpp share: the plan sizes the
// backward kernels' tap tables and the forward kernel's LDS with the same functions, constants and table entries the device uses, so neither side
// can see a zero / non-zero weight or a table size the other does not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ __forceinline__ void lin_coord(int o, float scale, int I, int& i0, int& i1, float& l1) {
    // ATen area_pixel_compute_source_index(align_corners=True): src = scale * dst (float32).  No contraction of `scale * o - i0` into one fma: the
    // host sizes the backward kernel's tap tables with this same function and must see the same zero / non-zero weights as the device
#pragma clang fp contract(off)
    const float src = scale * (float)o;
    i0 = (int)src;
    if (i0 > I - 1) i0 = I - 1;
    i1 = i0 + (i0 < I - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

// contribution range of input index i along one axis: outputs o whose i0(o)==i or i1(o)==i
__host__ __device__ __forceinline__ void up_range(int i, float scale, int O, int& lo, int& hi) {
    if (scale <= 0.f) { lo = 0; hi = O - 1; return; }
    lo = (int)floorf((float)(i - 1) / scale) - 1;
    hi = (int)ceilf((float)(i + 1) / scale) + 1;
    if (lo < 0) lo = 0;
    if (hi > O - 1) hi = O - 1;
}
__host__ __device__ __forceinline__ float up_weight(int o, int i, float scale, int I) {
    int i0, i1; float l1;
    lin_coord(o, scale, I, i0, i1, l1);
    float w = 0.f;
    if (i0 == i) w += 1.f - l1;
    if (i1 == i) w += l1;
    return w;
}

struct UpTab { uint32_t o0, o1; float l0, l1; };      // upsample_fwd3: one output coordinate of one axis (byte offsets of the two sources, their weights)
constexpr int UP_MAXW = 12;      // contributing outputs per input index: <= 2 / scale + 2, i.e. up to 4x up-sampling (the aux head)
struct UpEnt { int lo, n; float w[UP_MAXW]; };        // upsample_bwd2: one input index of one axis (first contributing output, count, weights)
constexpr int UP4_ROWS = 16;       // candidate output rows of a pair of input indices (up_range of the first .. of the second): <= 2 * 2 / scale + 6
