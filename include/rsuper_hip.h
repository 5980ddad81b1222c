/* rsuper_hip.h -- C ABI of the MI355X-native (gfx950) kernels behind R-Super's training hot path.
 *
 * The reference (MrGiovanni/R-Super) contains no native code and no FFI: every device op of
 * rsuper_train/train_ddp.py's step is an ATen/cuDNN call made from Python.
 * Each entry point below therefore cites the reference Python call site whose ATen op it replaces
 * (paths relative to rsuper_train/).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless named host_*;
 *   - activations are channels-last: element (n,d,h,w,c) of a view lives at x[(((n*D+d)*H+h)*W+w)*ld + c];
 *     C and ld are multiples of 8, base pointers 16-byte aligned;
 *   - dtype: RSUPER_F32 (parity mode, exact-f32 MFMA) or RSUPER_BF16 (bf16 storage, f32 accumulate);
 *   - logits, masks' companions and all parameter/gradient tensors are f32; masks are uint8 0/1;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous, never own their inputs;
 *   - return value: 0 = RSUPER_OK, otherwise an RSUPER_ERR_* code (nothing was launched on error).
 */
#ifndef RSUPER_HIP_H
#define RSUPER_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RSUPER_F32 0
#define RSUPER_BF16 1
#define RSUPER_OK 0
#define RSUPER_ERR_ARG 1
#define RSUPER_ERR_LAUNCH 2
#define RSUPER_ERR_UNSUPPORTED 3
#define RSUPER_ERR_NO_DEVICE 4

const char* rsuper_version(void);
/* 0 when device 0 is a gfx950 GPU; RSUPER_ERR_NO_DEVICE otherwise.  The host layer refuses to run without it. */
int rsuper_device_check(void);

/* ------------------------------------------------------------------------------------------------
 * 3x3x3 convolution (stride 1, pad 1, no bias) -- nn.Conv3d inside ConvNormAct,
 * model/dim3/conv_layers.py:29-38,46-51; BasicBlock model/dim3/conv_layers.py:86-94.
 * ------------------------------------------------------------------------------------------------ */

/* Elements (of `dtype`) of the fragment-ordered weight buffer for GEMM-K sources (ka, kb) and n_cols columns. */
size_t rsuper_conv3_packed_elems(int dtype, int ka, int kb, int n_cols, int bn);

/* Re-order state_dict weights (Cout, Cin, 3,3,3) f32 into MFMA B-fragment order.
 * mode 0 (forward):  K = forward input channels split as ka|kb (concat sources, model/dim3/unet_utils.py:71),
 *                    columns [0,na) from wa and [na,na+nb) from wb (conv1 + shortcut fused, conv_layers.py:79,84).
 * mode 1 (data grad): K = forward output channels (ka rows of wa, kb rows of wb), columns = forward Cin = na;
 *                    taps flipped.  nb = 0: all na columns; nb = (first column << 16) | columns (first column a multiple of 32):
 *                    only that column range, as a buffer of its own (rsuper_conv3_packed_elems with n_cols = columns) -- the data gradient of a
 *                    two-source block as one launch per source (round 5: 96 columns = 32 + 64 run 11 % faster as two launches). */
int rsuper_conv3_pack_weights(int dtype, int mode, const float* wa, const float* wb, int ka, int kb, int na, int nb,
                              int bn, void* packed, void* stream);

/* Same for n layers in one launch (all convolutions of a UNet forward, or of its backward).  host_desc: n x 6 ints
 * (mode, ka, kb, na, nb, bn); host_wa/host_wb: n device pointers each (wb may be NULL); host_out_elems: element offset
 * of every layer's fragment buffer inside `packed`, laid out back to back (each rsuper_conv3_packed_elems long). */
int rsuper_conv3_pack_weights_batch(int dtype, int n, const int* host_desc, const float* const* host_wa, const float* const* host_wb,
                                    const size_t* host_out_elems, void* packed, void* stream);

/* Number of 4x4x16 output tiles per sample == rows of the per-block partial-sum buffer. */
int rsuper_conv3_tiles(int D, int H, int W);

/* Kernel variant of rsuper_conv3_igemm: 0 = classic one-tile-per-block kernel (always used for f32), 1 = wave-specialised
 * producer/consumer persistent kernel (bf16), 2 = per-launch choice between the two (round-1 default), 3 (default) = as 2,
 * with the weight-stationary 8-wave kernel (weights in registers, activation fragments re-used across taps, epilogue
 * straight from the accumulators) for 32-column launches over a single 32-channel K chunk, 4 = weight-stationary kernel
 * for every bf16 32-column launch, 6 / 7 = the volume-fitted
 * K-split kernel (rsuper_conv3_box_bn) forced for every bf16 64-column launch (6: box shape per volume, 7: the 4x4x4 box).
 * v < 0 queries.  Returns the variant in effect. */
int rsuper_conv3_variant(int v);
/* bf16 weight gradients (rsuper_conv3_wgrad) run the second-generation kernel (operand re-use across taps, double-buffered tiles) when a block
 * sweeps at least `t` spatial tiles -- default 12, the measured break-even against the round-3 kernel; 0 = every supported launch (tests),
 * >= 2^20 = never.  Both extremes also switch the small-volume kernel off (batches of at most 64 tiles whose depth slabs fit LDS otherwise run
 * conv3d_wgrad_sv.hip), so that the tests can pin each tile-streaming kernel on small volumes.  t < 0 queries.  Returns the threshold in effect. */
int rsuper_conv3_wgrad2_min_tiles(int t);

/* THE dispatch query of rsuper_conv3_igemm: which kernel a launch runs, with which block width, writing how many statistics rows.  The library makes
 * that choice in one function; this query, the three single-answer queries below and the launch itself all read it, so they cannot disagree.
 *   bn = 0:  the library chooses the width (the depth-reuse kernel's where it takes the launch, else the volume-fitted kernel's, else the width that
 *            fills the chip / pads least).  Pack the weights with plan[1] and pass it to rsuper_conv3_igemm.
 *   bn != 0: the plan of a launch with that width.
 *   N = 0 (D, H, W, epi ignored; bn = 0): a width query without a volume -- only plan[1] is meaningful.
 *   Ca, Cb:  channels of the two sources (0, 0: unknown).  They only decide between kernels 1 and 2, which write the same rows.
 *   src_flags bit 0: the launch has two sources of which exactly ONE carries (mean, rstd) (mra == NULL xor mrb == NULL); rsuper_conv3_igemm derives the
 *            bit from its own arguments.  Kernels 2 and 3 stage both sources the same way and never take such a launch.
 * plan[0] kernel: 0 classic, 1 producer/consumer, 2 weight-stationary, 3 depth-reuse, 4 volume-fitted K-split;  plan[1] bn;  plan[2] the volume-fitted
 * kernel's box shape (else 0);  plan[3] its reduction splits (shape 3, needs Ca / Cb; else 0);  plan[4] rows per sample of `part`.
 * The answer depends on rsuper_conv3_variant and on the workspace registered at the time (rsuper_conv3_set_workspace). */
int rsuper_conv3_plan(int dtype, int epi, int N, int D, int H, int W, int Ca, int Cb, int n_cols, int src_flags, int bn, int* plan);

/* Launches whose volume cannot fill the chip with 4x4x16-voxel tiles (the 24^3 / 12^3 levels of the UNet at batch 2:
 * model/dim3/unet.py:49-58 after three / four poolings) run a volume-fitted kernel under the default variant: boxes of
 * 4x4x8 or 4x4x4 voxels that divide the volume, GEMM rows = flat voxel index of the box, the block's four waves split the
 * reduction (taps x k-steps) and reduce-scatter their partial tiles through LDS before the same fused epilogue.  It works
 * on 64-column blocks: returns 64 when rsuper_conv3_igemm(dtype, ..., n_cols, bn = 64, N, D, H, W) would take that kernel
 * (pack the weights with bn = 64 then), else 0. */
int rsuper_conv3_box_bn(int dtype, int N, int D, int H, int W, int n_cols);

/* The wide full-resolution layers (more than 32 columns, enough 4x8x16-voxel tiles for one persistent block per CU: up4.0 / the 96^3 level at
 * batch 2) run the depth-reuse kernel (conv3d_igemm_kd.hip: an activation fragment feeds the three kd taps, 0.5 / NF LDS fragment reads per MFMA):
 * returns the block width (64 forward; 64 / 96 / 128 data gradient) rsuper_conv3_igemm(dtype, epi, ..., n_cols, bn, N, D, H, W) takes that kernel
 * with, else 0 (rsuper_conv3_plan(..., bn = 0): kernel 3 and its width).  src_flags as for rsuper_conv3_plan: with bit 0 set the query returns 0 and
 * rsuper_conv3_igemm keeps the kernel that bn gets elsewhere. */
int rsuper_conv3_kd_bn(int dtype, int epi, int N, int D, int H, int W, int n_cols, int src_flags);

/* Volumes of at most 6x6x6 voxels (the 6^3 bottleneck level: model/dim3/unet.py:53, four poolings of a 96^3 patch) run one box
 * per sample with the REDUCTION (32-channel chunks) split over blocks: each block writes its raw f32 tile to a workspace and a
 * second kernel adds the splits and applies the epilogue (deterministic: fixed split order).  The caller registers one device
 * buffer of at least rsuper_conv3_workspace_bytes() PER DEVICE (the registration and every launch refer to the calling thread's
 * current HIP device); launches on one stream share it, launches on two streams of one device must not overlap such
 * convolutions.  Without a registered workspace those volumes take the 4x4x4-box shape.  rsuper_conv3_box_bn returns 32 for them. */
int rsuper_conv3_set_workspace(void* ptr, size_t bytes);
size_t rsuper_conv3_workspace_bytes(void);

/* Rows per sample of the `part` buffer rsuper_conv3_igemm(dtype, epi, ..., n_cols, bn, N, D, H, W) writes under the
 * current variant (classic: one row per tile; producer/consumer: one row per (persistent block, consumer wave row)): plan[4] of
 * rsuper_conv3_plan(..., bn).  src_flags as there (bit 0: one normalised + one raw source). */
int rsuper_conv3_part_rows(int dtype, int epi, int N, int D, int H, int W, int n_cols, int bn, int src_flags);

/* Implicit-GEMM convolution.  epi 0: forward  y = conv(prologue(x)) [+ res]; part <- per-tile (sum, sumsq) of y.
 *                             epi 1: data gradient g = conv(dy, flipped w) * [x_hat > 0]; part <- (sum g, sum g*x_n),
 *                                    where x_hat/x_n come from the forward inputs (ex*, with their mean/rstd emr*).
 * mra/mrb: [N][C][2] (mean, rstd) -> fused InstanceNorm(eps=1e-4)+ReLU prologue (conv_layers.py:40-43); NULL = raw.
 * part:    [N][rsuper_conv3_part_rows][n_cols][2] f32 or NULL.
 * Every activation tensor must be smaller than 4 GiB (N*D*H*W*ld*sizeof < 2^32: buffer-addressed staging); larger
 * volumes are refused with RS_ERR_UNSUPPORTED, also by rsuper_conv3_wgrad. */
int rsuper_conv3_igemm(int dtype, int epi,
                       const void* xa, int lda, int Ca, const float* mra,
                       const void* xb, int ldb, int Cb, const float* mrb,
                       const void* packed, int n_cols, int bn, int N, int D, int H, int W,
                       void* out, int ldo, const void* res, int ldr, float* part,
                       const void* exa, int elda, int eCa, const float* emra,
                       const void* exb, int eldb, int eCb, const float* emrb, void* stream);
/* The same launch with TWO output tensors: columns [0, out_split) go to `out`, columns [out_split, n_cols) to a tensor `out_part` ELEMENTS behind it (allocate
 * both from one buffer), each with row stride ldo.  For the fused [conv1 | shortcut] GEMM of a BasicBlock whose halves are narrower than a 128-byte line (32 bf16
 * channels: up4.0): every consumer of one half -- conv2's staging, its weight gradient, the ReLU mask of its data gradient, the InstanceNorm-backward tail -- then
 * reads whole lines instead of half-used ones.  out_split a multiple of 32; only launches the depth-reuse kernel takes (rsuper_conv3_plan: kernel 3),
 * RS_ERR_UNSUPPORTED otherwise: the caller falls back to the interleaved output. */
int rsuper_conv3_igemm_split_out(int dtype, int epi,
                                 const void* xa, int lda, int Ca, const float* mra,
                                 const void* xb, int ldb, int Cb, const float* mrb,
                                 const void* packed, int n_cols, int bn, int N, int D, int H, int W,
                                 void* out, int ldo, const void* res, int ldr, float* part,
                                 const void* exa, int elda, int eCa, const float* emra,
                                 const void* exb, int eldb, int eCb, const float* emrb, int out_split, long long out_part, void* stream);
/* The STRIDED member: Conv3d(k=3, stride=2, pad=1, bias=False) of down_block(pool=False) (unet_utils.py:38-39; BasicBlock conv1 + shortcut,
 * conv_layers.py:29-38,82-84) and its data gradient, with the minimal MFMA work (the 27 taps split over the 8 parity classes of the input /
 * of the gradient's output; conv3d_igemm_s2.hip).  FD x FH x FW = the full-resolution grid; the half-resolution one is ceil(F / 2).
 *   mode 1 (forward): xa = x (N, FD, FH, FW, lda) with statistics mra; out (N, OD, OH, OW, ldo) = conv(relu(norm(x))); part: N x
 *                     rsuper_conv3_s2_part_rows(dtype, 1, ...) rows of column sums / sums of squares for the next InstanceNorm; xb unused.
 *   mode 2 (dgrad)  : xa | xb = dy sources on the half grid (no statistics); out (N, FD, FH, FW, ldo) = the gradient w.r.t. relu(norm(x)),
 *                     masked by [x_n > 0] of the forward input exa (N, FD, FH, FW, elda) with statistics emra; part: N x
 *                     rsuper_conv3_s2_part_rows(dtype, 2, ...) rows of the InstanceNorm-backward sums.  packed = rsuper_conv3_pack_weights(mode - 1, ..., bn = 64). */
int rsuper_conv3_s2_part_rows(int dtype, int mode, int Ca, int Cb, int n_cols, int N, int FD, int FH, int FW);
int rsuper_conv3_igemm_s2(int dtype, int mode, const void* xa, int lda, int Ca, const float* mra,
                          const void* xb, int ldb, int Cb, const void* packed, int n_cols, int N, int FD, int FH, int FW,
                          void* out, int ldo, float* part, const void* exa, int elda, const float* emra, void* stream);

/* Weight gradient dW[co][ci][tap] += sum_v dy[v][co] * x_hat[v+tap][ci]   (autograd of the same nn.Conv3d under
 * loss.backward(), train_ddp.py:349).  dy rows [0,Ya) accumulate into dwa (Ya, Ca+Cb, 27), rows [Ya,Ya+Yb) into dwb.
 * dwa/dwb are overwritten.  workspace: splits * 27 * (Ya+Yb) * (Ca+Cb) floats (per-split partial slabs, summed by a
 * reduce kernel -- deterministic, no atomics).  use_tr selects ds_read_b64_tr_b16 operand fetch (bf16). */
/* THE dispatch query of rsuper_conv3_wgrad / _wgrad_partial: which kernel a launch runs, in which configuration, over how many slabs.  The library makes
 * that choice in one function; this query, rsuper_conv3_wgrad_splits and the launches read it, so the workspace and the kernel cannot disagree.
 *   splits = 0: choose the count;  splits != 0: plan for a workspace of that many slabs (the small-volume kernel runs only on its own count).
 *   src_flags bit 0: one normalised and one raw x source.  Arguments that describe no launch: RSUPER_ERR_ARG.
 * plan[0] kernel: 0 tile-streaming, 1 second-generation, 2 small-volume;  plan[1] splits;  plan[2] configuration of the tile-streaming kernel (0: 32 rows x
 * 27 taps, 1: 64 rows x 9 taps, 2: 64 rows x 27 taps);  plan[3] 32-row groups of dY per block (1 / 2).
 * The count never depends on use_tr or src_flags.  The answer depends on rsuper_conv3_wgrad2_min_tiles at the time. */
int rsuper_conv3_wgrad_plan(int dtype, int use_tr, int Ca, int Cb, int Ya, int Yb, int N, int D, int H, int W, int src_flags, int splits, int* plan);
/* Number of voxel-tile splits (= partial slabs in `workspace`) rsuper_conv3_wgrad should be called with for this shape: plan[1] of
 * rsuper_conv3_wgrad_plan(..., splits = 0).  Returns <= 0 on bad arguments. */
int rsuper_conv3_wgrad_splits(int dtype, int Ca, int Cb, int Ya, int Yb, int N, int D, int H, int W);

int rsuper_conv3_wgrad(int dtype, int use_tr,
                       const void* xa, int lda, int Ca, const float* mra,
                       const void* xb, int ldb, int Cb, const float* mrb,
                       const void* ya, int ldya, int Ya, const void* yb, int ldyb, int Yb,
                       float* dwa, float* dwb, float* workspace, int N, int D, int H, int W, int splits, void* stream);

/* The same in two steps, so that the slab reduction (a small bandwidth-bound kernel nothing on the data-gradient chain waits for)
 * can run on another stream: _partial writes the per-split slabs only, _reduce sums them into dwa / dwb (Cin = Ca + Cb). */
int rsuper_conv3_wgrad_partial(int dtype, int use_tr, const void* xa, int lda, int Ca, const float* mra,
                               const void* xb, int ldb, int Cb, const float* mrb,
                               const void* ya, int ldya, int Ya, const void* yb, int ldyb, int Yb,
                               float* workspace, int N, int D, int H, int W, int splits, void* stream);
int rsuper_conv3_wgrad_reduce(const float* workspace, int splits, int Cin, int Ya, int Yb, float* dwa, float* dwb, void* stream);
/* _reduce for n weight gradients in ONE launch (arrays of length n: the workspaces written by _partial, their splits, Cin = Ca + Cb, Ya, Yb and the
 * destinations): the per-layer reduction is a ~10 us launch at the dependent-launch floor and the hot loop has 34 of them per step
 * (loss.backward(), train_ddp.py:349 -- every nn.Conv3d weight gradient); nothing but the optimiser / the gradient exchange reads dW. */
int rsuper_conv3_wgrad_reduce_batch(int n, const void* const* workspaces, const int* splits, const int* Cin, const int* Ya, const int* Yb,
                                    void* const* dwa, void* const* dwb, void* stream);
/* The same launch also finalises up to two statistics buffers (rsuper_stats_finalize's arithmetic, bit-identical): in a BasicBlock's backward the data gradient of
 * conv1 leaves its InstanceNorm-backward partial rows and the block's two weight gradients their slabs -- one launch turns both into what the InstanceNorm-backward
 * tail and the optimiser read (autograd of conv_layers.py:86-94; a dependent ~5 us launch less per block and input source).  n in [1, 48], nstats in [0, 2];
 * arrays of length nstats: parts[i] = [sN][snblk][sC][2] f32, souts[i] = [sN][sC][2] f32 (two tables when ssplit > 0), scnt = voxels per sample, smode 0 / 1. */
int rsuper_conv3_wgrad_reduce_batch_stats(int n, const void* const* workspaces, const int* splits, const int* Cin, const int* Ya, const int* Yb,
                                           void* const* dwa, void* const* dwb, int nstats, const void* const* parts, const int* sN, const int* snblk,
                                           const int* sC, const double* scnt, const int* smode, const int* ssplit, void* const* souts, float eps, void* stream);

/* Weight gradient of the STRIDED member (Conv3d(k=3, stride=2, pad=1): BasicBlock(stride=2) conv1 + shortcut of down_block(pool=False),
 * unet_utils.py:18-33, conv_layers.py:60-94):  dW[co][ci][t] = sum_o dy[o][co] * x_hat[2o + t - 1][ci].
 * x (with its mean/rstd) lives on the full-resolution grid (N, FD, FH, FW); dy rows [0,Ya) -> dwa, [Ya,Ya+Yb) -> dwb live on the
 * ((FD+1)/2, (FH+1)/2, (FW+1)/2) grid -- no zero-stuffed operand.  workspace: splits * 27 * (Ya+Yb) * Ca floats, splits from
 * rsuper_conv3_wgrad_s2_splits.  dwa / dwb are overwritten (deterministic slab reduction). */
int rsuper_conv3_wgrad_s2_splits(int dtype, int Ca, int Mtot, int N, int FD, int FH, int FW);
int rsuper_conv3_wgrad_s2(int dtype, const void* xa, int lda, int Ca, const float* mra,
                          const void* ya, int ldya, int Ya, const void* yb, int ldyb, int Yb,
                          float* dwa, float* dwb, float* workspace, int N, int FD, int FH, int FW, int splits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * InstanceNorm3d(eps, affine=False) statistics and backward tail -- conv_layers.py:40-42
 * ------------------------------------------------------------------------------------------------ */
/* 1x1x1 convolution / linear layer over the channel axis of f32 channels-last rows, as an MFMA GEMM (bf16 or exact-f32 compute, f32
 * storage): the pointwise members of MedFormer's attention stages -- DepthwiseSeparableConv.pointwise (conv_layers.py:126-157), MBConv
 * expand / project (:197-239), BidirectionAttention's feat_qv / map_qv / out projections (medformer_utils.py:13-99).
 *   mode 0: y[r][n] = sum_k x[r][k] w[n][k] (+ bias[n]),  w = (N, K) as in the state_dict   (F.conv3d(k=1) / F.linear forward)
 *   mode 1: y[r][n] = sum_k x[r][k] w[k][n],              w = (K, N)                        (their data gradient, x := dy)
 * res (nullable, [R][ldr] f32): added after the bias -- the identity shortcut of MBConv (`... + x`, conv_layers.py:239) and of the attention
 * blocks, in the GEMM's epilogue instead of a separate element-wise launch (same fp32 additions in the same order: bit-identical).
 * N, ldx, ldy multiples of 4; R * ldx * 4 < 2^32; packed: device workspace of rsuper_pointwise_packed_bytes(dtype, K, N) bytes. */
size_t rsuper_pointwise_packed_bytes(int dtype, int K, int N);
int rsuper_pointwise(int dtype, int mode, const float* x, int ldx, const float* w, const float* bias, const float* res, int ldr,
                     float* y, int ldy, long R, int K, int N, void* packed, void* stream);
/* The fragments of MANY weights in one launch.  table (device): n + 1 rows of 8 x int64 {weight pointer (f32, row-major rows x cols), byte offset
 * of its fragments in `arena`, rows, cols, mode, ceil(N / 32), k-steps = ceil(K / (dtype == f32 ? 8 : 16)), first item}; an item is one 16-byte
 * fragment slot (64 per (k-step, 32-row tile)), numbered through all entries; row n holds {.., first item = total_items}.  rsuper_pointwise with
 * w == nullptr then takes `packed` = arena + offset as is. */
int rsuper_pointwise_pack_batch(int dtype, const long long* table, int n, long total_items, void* arena, void* stream);
/* Weight and bias gradient of the same layer (autograd of F.linear / Conv3d(k=1) under loss.backward(), train_ddp.py:349):
 *   dw[n][k] = sum_r dy[r][n] x[r][k]  (N, K) f32, overwritten;   db[n] = sum_r dy[r][n] (nullptr: not wanted)
 * The rows are cut into `splits` = rsuper_pointwise_wgrad_splits(R, N, K) slabs whose partial results go through `workspace`
 * (splits * (N*K + N) floats) and are added in slab order (deterministic).  N, K multiples of 4; (R + 1) * ld * 4 < 2^32. */
int rsuper_pointwise_wgrad_splits(long R, int N, int K);
int rsuper_pointwise_wgrad(int dtype, const float* dy, int ldy, const float* x, int ldx, long R, int N, int K, float* workspace, int splits,
                           float* dw, float* db, void* stream);

/* part [N][nblk][C][2] -> out [N][C][2]: mode 0 (mean, rstd = 1/sqrt(var+eps)), mode 1 (sum0/cnt, sum1/cnt).
 * split > 0 writes two contiguous tables instead, [N][split][2] followed by [N][C-split][2] (the column groups of a fused
 * conv1 + shortcut GEMM, or the two sources of a concatenated input), so each can be handed to a kernel as-is. */
int rsuper_stats_finalize(const float* part, int N, int nblk, int C, double cnt, float eps, int mode, int split, float* out, void* stream);
/* The bandwidth-bound kernels around the convolutions (InstanceNorm backward tail, max pool, subsample, trilinear forward, plane partial sums):
 * 1 (default) = the tuned kernels and grids, 0 = the ones they replaced -- results are bit-identical, the switch serves A/B runs and tests
 * (RSUPER_GLUE_KERNELS=0 in the environment selects 0 at start-up).  Any other v queries.  Returns the value in effect.  Which kernel and grid a
 * launch of the family gets under either value is decided in one place (csrc/glue_plan.hpp) and can be asked with rsuper_glue_plan. */
int rsuper_glue_variant(int v);
/* Operations of that family, for the two queries below. */
enum { RSUPER_GLUE_IN_BWD = 0, RSUPER_GLUE_POOL_FWD, RSUPER_GLUE_POOL_BWD, RSUPER_GLUE_SUB_FWD, RSUPER_GLUE_SUB_BWD, RSUPER_GLUE_UP_FWD,
       RSUPER_GLUE_UP_BWD, RSUPER_GLUE_STEM_FWD };
/* Rows of the partial statistics `part` ([N][rows][C][2]) that a forward writes for `vox` output voxels per sample -- the `blocks` argument of
 * rsuper_maxpool2_fwd / rsuper_subsample2_fwd / rsuper_upsample_fwd, and the rows rsuper_stem_fwd writes.  0: the operation writes none. */
int rsuper_stat_rows(int op, long vox);
/* The launch the library makes for one operation, from the shape alone (pure host code; csrc/glue_plan.hpp is the one place that decides, and
 * the entry points below read the same functions).  shape[7]: N, then vox (IN_BWD), the input's D, H, W (POOL_*, SUB_*) or ID, IH, IW, OD, OH, OW
 * (UP_*); ld: the row stride that the kernels' 32-bit offsets see (the widest operand's; C for dense tensors).
 * out[8]: kernel (0 in_bwd_finalize, 1 in_bwd_finalize2, 2 maxpool_fwd, 3 maxpool_fwd2, 4 maxpool_bwd, 5 subsample_fwd, 6 subsample_bwd,
 * 7 upsample_fwd, 8 upsample_fwd2, 9 upsample_fwd3, 10 upsample_bwd, 11 upsample_bwd2, 12 upsample_bwd4), template selector (U of in_bwd_finalize2,
 * NT of upsample_bwd4, else 0), blocks in x, y, z, threads per block, dynamic LDS bytes, rows of `part` (rsuper_stat_rows; 0: none).
 * RSUPER_ERR_UNSUPPORTED where the launch would answer it, RSUPER_ERR_ARG for arguments that describe no launch. */
int rsuper_glue_plan(int op, int dtype, const int* shape, int C, int ld, int* out);
/* The same for the kernels MedFormer's attention stages run on (1x1x1 convolution GEMM and its weight gradient, depthwise 3x3x3, channel norm,
 * squeeze-excite, rsuper_cl_planar): csrc/mf_plan.hpp is the one place that decides, one `op` per launch.  shape: K, N (PW_PACK); fragment slots
 * (PW_PACK_BATCH); R, K, N (PW, either mode); R, N, K (PW_WGRAD*); N, D, H, W, C (DW*); N, vox, C, mode (CNORM*; CNORM is the first launch of
 * rsuper_cnorm_forward (mode 0) / _backward (mode 1)); N, C, r (SE_*); N, vox, C, K (CL_PLANAR).
 * out[10]: kernel (0 pw_pack, 1 pw_pack_batch, 2 pw_gemm, 3 pw_wgrad, 4 pw_wgrad_reduce, 5 depthwise_fwd, 6 depthwise_lds, 7 depthwise_wgrad,
 * 8 depthwise_wgrad_reduce, 9 cnorm_stats, 10 cnorm_apply, 11 cnorm_small, 12 se_hidden_fwd, 13 se_gate_fwd, 14 se_excite_bwd_hidden, 15 se_excite_wgrad,
 * 16 se_dm, 17 cl_planar; -1 with RSUPER_OK: PW_WGRAD_REDUCE of a single slab, no launch), template selector (NF of pw_gemm, WNW of pw_wgrad, MODE of
 * cnorm_*), blocks in x, y, z, threads per block, dynamic LDS bytes, rows (of `part`: cnorm statistics, depthwise weight gradient; slabs of the
 * pw_wgrad workspace; 0: none), the kernel argument that goes with the grid (KSPLIT of pw_gemm, rows per slab of pw_wgrad, D segments of
 * depthwise_lds), and what the caller allocates (bytes of PW_PACK's fragments, floats of PW_WGRAD's workspace, else 0).  dtype: the compute type of
 * the pointwise kernels; storage is f32 throughout.  Errors as rsuper_glue_plan; an error leaves `out` untouched. */
enum { RSUPER_MF_PW_PACK = 0, RSUPER_MF_PW_PACK_BATCH, RSUPER_MF_PW, RSUPER_MF_PW_WGRAD, RSUPER_MF_PW_WGRAD_REDUCE, RSUPER_MF_DW, RSUPER_MF_DW_WGRAD,
       RSUPER_MF_DW_WGRAD_REDUCE, RSUPER_MF_CNORM, RSUPER_MF_CNORM_STATS, RSUPER_MF_CNORM_APPLY, RSUPER_MF_SE_HIDDEN, RSUPER_MF_SE_GATE,
       RSUPER_MF_SE_BWD_HIDDEN, RSUPER_MF_SE_WGRAD, RSUPER_MF_SE_DM, RSUPER_MF_CL_PLANAR };
int rsuper_mf_plan(int op, int dtype, const int* shape, int* out);
/* dx = rstd * (g - gm0 - x_n * gm1) [+ add1] [+ add2] */
int rsuper_in_bwd_finalize(int dtype, const void* g, int ldg, const void* x, int ldx, const float* mr, const float* gm,
                           const void* add1, int lda1, const void* add2, int lda2, void* out, int ldo,
                           int N, int vox, int C, void* stream);

/* nn.MaxPool3d(2) -- model/dim3/unet_utils.py:35-37.  part: [N][blocks][C][2] partial stats of y (or NULL). */
int rsuper_maxpool2_fwd(int dtype, const void* x, int ldx, void* y, int ldy, float* part, int blocks,
                        int N, int D, int H, int W, int C, void* stream);
int rsuper_maxpool2_bwd(int dtype, const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx,
                        int N, int D, int H, int W, int C, void* stream);
/* dx = maxpool backward(dy) + add in one pass: x of a down_block is also the skip connection of the matching up_block (model/dim3/unet.py:57-66),
 * `add` is the gradient that arrived through the skip; autograd would store their sum with one more read-read-write launch.  Even D, H, W only
 * (RS_ERR_UNSUPPORTED otherwise).  Bit-identical to the two steps (both round the f32 sum of two bf16 values once). */
int rsuper_maxpool2_bwd_add(int dtype, const void* x, int ldx, const void* dy, int lddy, const void* add, int lda, void* dx, int lddx,
                            int N, int D, int H, int W, int C, void* stream);
/* rsuper_maxpool2_bwd_add with lazy gradients: where gm_y (gm_x) is given, dy (add) is not a finished gradient but the raw data gradient g of the
 * convolution that read the pooled tensor (x) through InstanceNorm + ReLU, mr_* are that tensor's (mean, rstd) and gm_* the backward means
 * (mean(g), mean(g x_n)), all [N][C][2]; the kernel applies the tail of rsuper_in_bwd_finalize to each vector as it reads it and rounds it to the
 * storage type, so dx is bit for bit what rsuper_in_bwd_finalize followed by rsuper_maxpool2_bwd_add gives, without the launch and the tensor between
 * them.  NULL gm_*: that gradient is final, as in rsuper_maxpool2_bwd_add.  RS_ERR_UNSUPPORTED where rsuper_maxpool2_bwd_lazy_plan does not answer 1
 * (the caller then finalises the gradients itself). */
int rsuper_maxpool2_bwd_lazy(int dtype, const void* x, int ldx, const void* dy, int lddy, const float* mr_y, const float* gm_y,
                             const void* add, int lda, const float* mr_x, const float* gm_x, void* dx, int lddx,
                             int N, int D, int H, int W, int C, void* stream);
/* The one decision (csrc/lazy_tail_plan.hpp): 1 = the max-pool backward of an (N, D, H, W, C) input takes lazy gradients, 0 = the InstanceNorm backward
 * tails run as launches of their own (odd sizes, rsuper_lazy_tails(0)), < 0 = bad arguments.  Pure host code. */
int rsuper_maxpool2_bwd_lazy_plan(int dtype, int N, int D, int H, int W, int C);
/* 1 (default): lazy gradients wherever the plans admit them; 0: none (A/B runs and tests: results are bit-identical); 2: wherever a fused kernel can take
 * the launch, measured faster or not (tools/bench_lazy_tails.py).  RSUPER_LAZY_TAILS in the environment selects the value at start-up.  Any other v
 * queries.  Returns the value in effect. */
int rsuper_lazy_tails(int v);

/* Stride-(2,2,2) down-sampling of down_block(pool=False) -- model/dim3/unet_utils.py:38-39 (`block(in_ch, out_ch,
 * stride=down_scale)`; conv_layers.py:29-38 with stride 2, padding 1).  The strided convolution is the stride-1 convolution
 * (rsuper_conv3_igemm) evaluated at the even voxels: fwd picks y[od,oh,ow] = x[2od,2oh,2ow] (output ceil(D/2) x ceil(H/2) x
 * ceil(W/2)) and writes the partial stats of y; bwd scatters dy back to the even voxels of a zero-filled dx (D, H, W = the
 * full-resolution dims in both calls). */
int rsuper_subsample2_fwd(int dtype, const void* x, int ldx, void* y, int ldy, float* part, int blocks,
                          int N, int D, int H, int W, int C, void* stream);
int rsuper_subsample2_bwd(int dtype, const void* dy, int lddy, void* dx, int lddx, int N, int D, int H, int W, int C, void* stream);

/* F.interpolate(mode='trilinear', align_corners=True) -- model/dim3/unet_utils.py:69 */
int rsuper_upsample_fwd(int dtype, const void* x, int ldx, void* y, int ldy, float* part, int blocks,
                        int N, int ID, int IH, int IW, int OD, int OH, int OW, int C, void* stream);
int rsuper_upsample_bwd(int dtype, const void* dy, int lddy, void* dx, int lddx,
                        int N, int ID, int IH, int IW, int OD, int OH, int OW, int C, void* stream);
/* rsuper_upsample_bwd of a lazy gradient: g is the raw data gradient of the convolution that read the up-sampled tensor u through InstanceNorm + ReLU,
 * mr the statistics of u and gm the backward means ([N][C][2]); the load stage of the row-sharing kernel applies the tail of rsuper_in_bwd_finalize and
 * its rounding, so dx is bit for bit what rsuper_in_bwd_finalize followed by rsuper_upsample_bwd gives.  bf16 only.  RS_ERR_UNSUPPORTED where
 * rsuper_upsample_bwd_lazy_plan does not answer 1 or the kernel's tile tables do not hold the scale (the caller then finalises g itself). */
int rsuper_upsample_bwd_lazy(int dtype, const void* g, int ldg, const void* u, int ldu, const float* mr, const float* gm, void* dx, int lddx,
                             int N, int ID, int IH, int IW, int OD, int OH, int OW, int C, void* stream);
/* The one decision (csrc/lazy_tail_plan.hpp): 1 = lazy gradient, 0 = the tail runs as a launch of its own, < 0 = bad arguments.  Pure host code. */
int rsuper_upsample_bwd_lazy_plan(int dtype, int N, int ID, int IH, int IW, int OD, int OH, int OW, int C);

/* inconv.conv1 = nn.Conv3d(1, C, 3, padding=1, bias=False) -- model/dim3/unet_utils.py:14.  x: [N][D][H][W] f32. */
int rsuper_stem_fwd(int dtype, const float* x, const float* w, void* y, int ldy, float* part,
                    int N, int D, int H, int W, int C, void* stream);
/* dw (C,1,3,3,3) f32 is overwritten (per-block partial rows + fixed-order reduce: deterministic, no atomics). */
int rsuper_stem_wgrad(int dtype, const float* x, const void* dy, int lddy, float* dw, int N, int D, int H, int W, int C, void* stream);

/* outc = nn.Conv3d(C, K, kernel_size=1) with bias -- model/dim3/unet.py:47.  logits: [N][K][vox] f32 (NCDHW). */
int rsuper_head_fwd(int dtype, const void* x, int ldx, const float* w, const float* b, float* logits, int N, int vox, int C, int K, void* stream);
int rsuper_head_bwd_data(int dtype, const float* dlogits, const float* w, void* dx, int lddx, int N, int vox, int C, int K, void* stream);
/* dw (K,C) and db (K) f32 are overwritten (same reduction scheme as rsuper_stem_wgrad). */
int rsuper_head_bwd_weight(int dtype, const void* x, int ldx, const float* dlogits, float* dw, float* db, int N, int vox, int C, int K, void* stream);
/* Both gradients of the head in one call: dx (bf16 / f32 channels-last) = dlogits^T W, dw / db overwritten.  With bf16 activations, K <= 32 classes and
 * C <= 32 channels this is ONE pass over dlogits (the weight-gradient kernel also multiplies its staged dlogits tile with W on the matrix cores);
 * otherwise the two calls above.  Autograd of outc = nn.Conv3d(C, K, 1) (model/dim3/unet.py:47) under loss.backward() (train_ddp.py:349). */
int rsuper_head_bwd(int dtype, const void* x, int ldx, const float* dlogits, const float* w, void* dx, int lddx, float* dw, float* db,
                    int N, int vox, int C, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loss reductions -- training/losses_foundation.py:945-956 (masked BCE), :541-607 (DiceLossMultiClass),
 * :329/:367 (soft volume), :1743-1811 (ball loss BCE with GWRP / background weights).
 * sums[planes][6] f64 (pre-zeroed): S=sum bce*k, A=sum sig*k, B=sum sig*t*k, Cn=sum t*k, F1=sum bce*k*w1, F2=sum bce*k*(1-w2)
 * flags: bit 0 (backward only) dx += instead of dx =; bit 1: `k` holds the dilated UNKNOWN mask and the voxel weight is
 * 1 - k (get_known_voxels, :150-165) -- saves materialising `1 - dilate(unk)`.
 * ------------------------------------------------------------------------------------------------ */
int rsuper_plane_partials_fwd(const float* x, size_t xstride, const uint8_t* t, const uint8_t* k, const float* w1, const uint8_t* w2,
                              double* sums, int flags, int planes, size_t V, void* stream);
int rsuper_plane_partials_bwd(const float* x, size_t xstride, const uint8_t* t, const uint8_t* k, const float* w1, const uint8_t* w2,
                              const float* g, float* dx, int flags, int planes, size_t V, void* stream);
/* The same two passes reading the target planes in the dataset's bit-packed form (`np.packbits(label, axis=0)`,
 * dataset_abdomenatlas_UFO.py:955,970,975 -- class c of sample b is bit 7 - (c & 7) of byte plane b * tP + (c >> 3); tpk = [planes / tC][tP][V], replaces t)
 * and skipping the planes of the dilated unknown map that cannot hold a 1 (kflags[planes] = rsuper_plane_any of the UNdilated map; only with flags bit 1):
 * 1/8 of the label bytes and, for the usual batch, none of the unknown-map bytes cross HBM. */
int rsuper_plane_partials_fwd2(const float* x, size_t xstride, const uint8_t* t, const uint8_t* tpk, int tP, int tC, const uint8_t* k, const uint8_t* kflags,
                               const float* w1, const uint8_t* w2, double* sums, int flags, int planes, size_t V, void* stream);
int rsuper_plane_partials_bwd2(const float* x, size_t xstride, const uint8_t* t, const uint8_t* tpk, int tP, int tC, const uint8_t* k, const uint8_t* kflags,
                               const float* w1, const uint8_t* w2, const float* g, float* dx, int flags, int planes, size_t V, void* stream);
/* The forward sums without a float atomic (round 6): every block of the launch stores its six partial sums to pblk[plane][block][6]
 * (blocks = rsuper_plane_partials_blocks(V) per plane; no pre-zeroing) and rsuper_plane_sums_reduce adds them in block order and converts to f32:
 * out[row][6] for `rows` consecutive planes of one or several _fwd3 launches.  Bit-reproducible by construction; one launch less than the atomic form
 * (zero fill + sums + f64 -> f32 conversion). */
int rsuper_plane_partials_blocks(size_t V);
int rsuper_plane_partials_fwd3(const float* x, size_t xstride, const uint8_t* t, const uint8_t* tpk, int tP, int tC, const uint8_t* k, const uint8_t* kflags,
                               const float* w1, const uint8_t* w2, double* pblk, int flags, int planes, size_t V, void* stream);
int rsuper_plane_sums_reduce(const double* pblk, int rows, int nb, float* out, void* stream);
/* Segmentation term from the sums of the (B*C) label planes: loss[0] = scale * ( sum(S*cw)/(B*C*V) + DiceLossMultiClass ),
 * :945-956 with the adaptive-Tversky Dice of :541-607 (alpha_c = clamp(sum_b FP / (sum_b FP + sum_b FN + 1e-5), 0.2, 0.8),
 * dice = TP / (TP + alpha FP + (1-alpha) FN + 1e-5), mean over (b, c) of (1 - dice) * cw).  sums f32 [B*C][6] as produced
 * by rsuper_plane_partials_fwd (cast to f32); cw [B*C] or NULL; dsums [B*C][6] receives d loss / d sums. */
int rsuper_seg_from_sums(const float* sums, const float* cw, int B, int C, size_t V, double scale, float* loss, float* dsums, void* stream);
/* The report terms of calculate_loss from the (R, 6) sums rsuper_plane_partials_fwd produced for them, with their Jacobians, without leaving the
 * device: dice_volume_loss (volume_loss_basic :250-349 with dice_based_volume_loss :352-395) from the first L*B rows (row li*B + b; flags[b][2L] =
 * annotated-tumour flag | segment gate, rvol[b] = reported volume) when use_vol, ball_loss_bce / ball_loss_dice (:1625-1661 for a sample without
 * tumour = L rows, :1793-1811 + DiceLossMultiClass :541-607 for a tumour sample = 1 row) as the mean over the `nplans` plans given as
 * plan[nplans][2] = (kind 0 / 1, first row).  roww[R] = class weight per row.  loss[3] = (ball_loss_bce, ball_loss_dice, dice_volume_loss),
 * jac[3][R][6] = d loss_k / d sums. */
int rsuper_report_from_sums(const float* sums, const float* roww, int R, int B, int L, size_t V, int use_vol, const float* flags, const float* rvol,
                            double tol, double E, int nplans, const int* plan, int apply_dice, int standard_ce, float* loss, float* jac, void* stream);
int rsuper_sigmoid_mask(const float* x, const uint8_t* m, float* out, size_t V, void* stream);

/* Sliding-window inference -- inference/inference3d.py:28-107 (inference_sliding_window) and :8-25
 * (inference_whole_image, assign = 1 with the window covering the volume).  The reference accumulates window
 * probabilities on the host; here acc[BK][D][H][W] (f32, device) receives sigmoid(logits[BK][wd][wh][ww]) at offset
 * (d0, h0, w0): added (assign = 0) or stored (assign = 1).  rsuper_window_normalize divides by the separable window count
 * cd[d] * ch[h] * cw[w] (f32 device vectors of D, H, W entries), the `pred_output /= counter` of :101. */
int rsuper_window_accumulate(const float* logits, float* acc, int BK, int wd, int wh, int ww, int D, int H, int W, int d0, int h0, int w0,
                             int assign, void* stream);
int rsuper_window_normalize(float* acc, const float* cd, const float* ch, const float* cw, long BK, int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone InstanceNorm3d(affine=False) [+ ReLU], channels-last f32 [N][vox][C], C % 4 == 0 -- the bare norm layers of
 * MedFormer's attention stages (model/dim3/medformer_utils.py:117-118, :160; conv_layers.py:46-51 for 1x1x1 / depthwise members).
 * stats: part [N][rsuper_cnorm_rows(vox)][C][2]; mode 0 (sum x, sum x^2) -> rsuper_stats_finalize(mode 0) gives mr = (mean, rstd);
 *        mode 1 (sum g, sum g * x_hat) with g = dy * [x_hat > 0 when relu] -> rsuper_stats_finalize(mode 1) gives gm.
 * apply: mode 0 out = x_hat (max(x_hat, 0) when relu); mode 1 out = rstd * (g - gm0 - x_hat * gm1).
 *        mode 2 out = x * mr[1] + mr[0]: a per-(sample, channel) affine map (SEBlock scaling x * s and its gradient, conv_layers.py:159-174).
 * ------------------------------------------------------------------------------------------------ */
int rsuper_cnorm_rows(long vox);
/* one-launch kernel (statistics + finalize + apply in a block per (sample, 16 channels)), at any size:
 * mode 0: out = norm(x) [+ relu], mr_out = (mean, rstd);  mode 1: out = dx from (x, dy, mr). */
int rsuper_cnorm_small(const float* x, const float* dy, const float* mr, float* out, float* mr_out, int N, long vox, int C, int relu, float eps,
                       int mode, void* stream);
int rsuper_cnorm_stats(const float* x, const float* dy, const float* mr, float* part, int N, long vox, int C, int relu, int mode, void* stream);
/* A whole norm in one host call: forward writes mr and y = norm(x) [+ relu]; backward writes dx.  Small volumes (up to RSUPER_CNORM_SMALL_VOX = 512
 * voxels) take the one-launch kernel, the others stats -> rsuper_stats_finalize -> apply (part / mr / gm as above; backward writes gm).
 * rsuper_cnorm_part_rows: the rows of `part` these two want, 0 where the one launch runs: part (and gm) are then not read and may be NULL. */
int rsuper_cnorm_part_rows(long vox);
int rsuper_cnorm_forward(const float* x, float* part, float* mr, float* y, int N, long vox, int C, int relu, float eps, void* stream);
int rsuper_cnorm_backward(const float* x, const float* dy, const float* mr, float* part, float* gm, float* dx, int N, long vox, int C, int relu,
                          void* stream);
int rsuper_cnorm_apply(const float* x, const float* dy, const float* mr, const float* gm, float* out, int N, long vox, int C, int relu, int mode,
                       void* stream);

/* SEBlock (model/dim3/conv_layers.py:159-174) on a channels-last f32 tensor [N][vox][C]: y = x * sigmoid(W2 relu(W1 mean(x) + b1) + b2), w1 (r, C),
 * w2 (C, r) as in the state_dict of the two 1x1x1 convolutions.  One host call per direction (channel statistics + finalize, the excitation on the
 * (N, C) vector in one block per sample, the per-(sample, channel) affine apply).  Scratch kept by the caller from forward to backward: ms [N][C][2]
 * (channel means), tab [N][C][2] = (0, s), hbuf [N][r] (hidden activations).  part: rsuper_cnorm_rows(vox) * N * C * 2 floats of workspace.
 * backward: ident = [N][C][2] table of (0, 1); gm, dz1 [N][r], tab2 [N][C][2] are workspaces; dw1 / db1 / dw2 / db2 are overwritten. */
int rsuper_se_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* part, float* ms, float* tab,
                      float* hbuf, float* y, int N, long vox, int C, int r, void* stream);
int rsuper_se_backward(const float* x, const float* dy, const float* ident, const float* w1, const float* w2, const float* ms, const float* tab,
                       const float* hbuf, float* part, float* gm, float* dz1, float* tab2, float* dx, float* dw1, float* db1, float* dw2, float* db2,
                       int N, long vox, int C, int r, void* stream);

/* Re-layout of a logits-like f32 tensor between channels-last [N][vox][C] (C % 4 == 0, C <= 64, the first K channels real) and
 * planar [N][K][vox] -- the `permute(0, 4, 1, 2, 3)` between MedFormer's channels-last deep-supervision head and the (N, K, D, H, W)
 * planes the loss reads (model/dim3/medformer.py:190-194).  to_channels_last = 0: dst planar <- src channels-last;
 * 1: dst channels-last <- src planar, padding channels K..C-1 written as zero (the gradient direction). */
int rsuper_cl_planar(const float* src, float* dst, int N, long vox, int C, int K, int to_channels_last, void* stream);

/* Self-attention core of the SemanticMapFusion transformer (Attention.forward, trans_layers.py:52-84 under medformer_utils.py:239-273):
 *   o = softmax(q k^T * scale) v per (sample, head).  qkv (B, L, 3*heads*dim_head) f32 = q | k | v thirds with head h at columns
 *   [h*dim_head, (h+1)*dim_head) of its third (to_qkv(x).chunk(3, -1) + 'b l (h d) -> b h l d'); o (B, L, heads*dim_head) in the
 *   'b h l d -> b l (h d)' layout; p (B, heads, L, L) = the soft-max rows, written forward and read backward (with o, the forward's
 *   output).  _bwd overwrites d_qkv (same layout as qkv).  One launch per direction, deterministic.  L <= 128, dim_head <= 64
 *   (rsuper_token_attn_supported); other shapes -> RS_ERR_UNSUPPORTED. */
int rsuper_token_attn_supported(int L, int dim_head);
int rsuper_token_attn_fwd(const float* qkv, float* o, float* p, int B, int L, int heads, int dim_head, float scale, void* stream);
int rsuper_token_attn_bwd(const float* qkv, const float* o, const float* p, const float* d_o, float* d_qkv, int B, int L, int heads, int dim_head, float scale,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bidirectional attention between the L voxels of a stage and its T semantic-map tokens, f32 channels-last -- the score / soft-max /
 * mixing core of BidirectionAttention (model/dim3/medformer_utils.py:13-99: the two einsums 'bhid,bhjd->bhij', the soft-max
 * over either axis, 'bhij,bhjd->bhid' / 'bhji,bhjd->bhid' and the head rearranges around them):
 *   S[t,l] = scale * <mq[t], fq[l]>;  f_out[l] = sum_t softmax_t(S[:,l])[t] mv[t];  m_out[t] = sum_l softmax_l(S[t,:])[l] fv[l]
 * fqv [B][L][2*inner], mqv [B][T][2*inner]: q in channels [0, inner), v in [inner, 2*inner), inner = heads * dim_head, channel =
 * dim_head_index * heads + head ('b (dim_head heads) ...'); f_out [B][L][inner], m_out [B][T][inner] in the same channel order.
 * lse [B][heads][T][2] = (max, sum) of the voxel-axis soft-max (saved for backward).
 * Workspaces (n = rsuper_battn_chunks(L, heads)): fwd part B*n*T*inner floats, pms B*n*heads*T*2 floats; bwd part B*n*T*2*inner.
 * Built for (T, dim_head) in {(27, 32), (8, 16)}, heads <= 10 (rsuper_battn_supported); anything else -> RS_ERR_UNSUPPORTED.
 * Deterministic (fixed-order merges, no atomics).
 * ------------------------------------------------------------------------------------------------ */
int rsuper_battn_supported(int T, int dim_head, int heads);
int rsuper_battn_chunks(int L, int heads);
int rsuper_battn_fwd(const float* fqv, const float* mqv, float* f_out, float* m_out, float* lse, float* part, float* pms, int B, int L, int T,
                     int heads, int dim_head, float scale, void* stream);
int rsuper_battn_bwd(const float* fqv, const float* mqv, const float* m_out, const float* lse, const float* d_f_out, const float* d_m_out,
                     float* d_fqv, float* d_mqv, float* part, int B, int L, int T, int heads, int dim_head, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depthwise 3x3x3 convolution (groups = C, stride 1, padding 1, no bias), channels-last f32 [N][D][H][W][C], C % 4 == 0 --
 * DepthwiseSeparableConv.depthwise / MBConv.depthwise of MedFormer (model/dim3/conv_layers.py:126-157, :198-240).
 * w: (C, 1, 3, 3, 3) as in the state_dict.  flip = 1 evaluates the data gradient (x := dy, taps mirrored).
 * wgrad: part = workspace of rsuper_depthwise3_rows(N*D*H*W) * 27 * C floats; dw (C, 1, 3, 3, 3) is overwritten (fixed-order
 * reduction, deterministic).
 * ------------------------------------------------------------------------------------------------ */
int rsuper_depthwise3_rows(long vox);
int rsuper_depthwise3_fwd(const float* x, const float* w, float* y, int N, int D, int H, int W, int C, int flip, void* stream);
int rsuper_depthwise3_wgrad(const float* x, const float* dy, float* part, float* dw, int N, int D, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Binary morphology and selection -- training/losses_foundation.py
 * ------------------------------------------------------------------------------------------------ */
/* dilate_volume :22-46 (iterated ball dilation).  in/out/tmp: nvol volumes of D*H*W bytes; tmp may be NULL when
 * kernel_size <= 7. */
int rsuper_dilate_volume(const uint8_t* in, uint8_t* out, uint8_t* tmp, long nvol, int D, int H, int W, int kernel_size, void* stream);
/* Same, with flags[nvol] (0 = the volume is all zero, e.g. from rsuper_plane_any): flagged-empty volumes are written as zeros without
 * being read -- most label planes carry no unknown / segment voxels.  flags may be NULL (= dense). */
int rsuper_dilate_volume_sparse(const uint8_t* in, uint8_t* out, uint8_t* tmp, const uint8_t* flags, long nvol, int D, int H, int W,
                                int kernel_size, void* stream);
/* isolate_tumor :1423-1445: Gaussian-ball correlation (odd diameter d_odd, std) and first-maximum argmax.
 * best: device u64, pre-zeroed; key = (f32 bits << 32) | (0xFFFFFFFF - linear index). conv_out optional (debug).
 * workspace: rsuper_ball_workspace_floats(D, H, W, d_odd) floats ((d_odd/2 + 1) * D*H*W row sums + one occupancy bit per (z, y)
 * row) -> separable two-stage form (row sums per half width, then a k^2 gather per voxel instead of k^3 taps, over the rows of x
 * that hold a non-zero only: x is zero outside the report's organ segment); NULL -> direct form.  Both are f32; they differ
 * only in summation order. */
long rsuper_ball_workspace_floats(int D, int H, int W, int d_odd);
int rsuper_ball_conv_argmax(const float* x, int D, int H, int W, int d_odd, float std, unsigned long long* best, float* conv_out, float* workspace,
                            void* stream);
/* insert_ball :1336-1385; count (device u32, pre-zeroed) += voxels set. */
int rsuper_insert_ball(uint8_t* out, int D, int H, int W, int cz, int cy, int cx, int d_odd, int half, unsigned int* count, void* stream);
/* The same with the centre decoded on the device from `best` (the argmax key rsuper_ball_conv_argmax wrote): isolate_tumor's argmax -> insert_ball
 * hand-over (losses_foundation.py:1445-1448) without a device->host read.  count: device u32, pre-zeroed, receives the ball's voxel count. */
int rsuper_insert_ball_at(uint8_t* out, int D, int H, int W, const unsigned long long* best, int d_odd, int half, unsigned int* count, void* stream);
/* exact top-k as radix select over non-negative f32 (torch.topk use at :1483-1492); ties -> lower index first. */
int rsuper_radix_hist(const float* x, const uint8_t* m, long V, uint32_t prefix, int shift, unsigned int* hist256, void* stream);
/* need_eq = 0xFFFFFFFF: every element equal to the threshold is selected (parallel); otherwise the first need_eq in index order. */
int rsuper_topk_mark(const float* x, const uint8_t* m, long V, uint32_t thr_bits, unsigned int need_eq, uint8_t* out, void* stream);
/* The same top-k with the radix-select state kept on the device: ONE call, no host round trips (the histogram passes above
 * need four device->host reads per mask).  workspace: 260 u32 on the device.  out[i] = 1 for the k largest of x*m
 * (x >= 0), ties -> lower index first.  1 <= k <= V. */
int rsuper_topk_select(const float* x, const uint8_t* m, long V, unsigned int k, uint8_t* out, unsigned int* workspace, void* stream);
/* nk <= 4 selections over the same (x, m) in one pass sequence (isolate_tumor's t / t_small / t_big masks, :1483-1507): k is a HOST
 * array of nk counts, out holds nk volumes, workspace nk * 260 u32.  clip_to_mask != 0 ANDs every selection with m (voxels outside m
 * rank with value 0 as in the dense top-k but are never marked: the "no tumor_mask value outside the ball" step). */
int rsuper_topk_select_multi(const float* x, const uint8_t* m, long V, const unsigned int* k, int nk, uint8_t* out, unsigned int* workspace,
                             int clip_to_mask, void* stream);
/* GlobalWeightedRankPooling(return_weights, hard_cutoff) :442-535 restricted to the pseudo mask. */
int rsuper_compact(const float* x, const uint8_t* pm, long V, float* vals, uint32_t* idx, unsigned int* n, void* stream);
int rsuper_rank_weights(const float* vals, const uint32_t* idx, unsigned int n, float log2_d, float scale, float* w, void* stream);
/* The same weights from a rank order: w[ids[r]] = 2^(r * log2_d) * scale for r < n (ids = voxel indices sorted by value descending, ties by index
 * ascending -- what rsuper_rank_weights derives by pairwise counting in O(n^2)); identical arithmetic, O(n): the large-tumour path of GWRP. */
int rsuper_rank_assign(const long long* ids, unsigned int n, float log2_d, float scale, float* w, void* stream);
/* flags[p] = any(m[p][:]) for `planes` contiguous byte volumes of V voxels (V % 16 == 0 when planes > 1): the
 * `.sum() > 0` / `.any()` tests of calculate_loss / ball_loss (:1625, :313, :335) at HBM rate. */
int rsuper_plane_any(const uint8_t* m, long planes, long V, uint8_t* flags, void* stream);

/* The per-step input guards of train_epoch (train_ddp.py:311-313: `assert not isnan(img).any()`, `max(img) <= 100`, `min(img) >= -100` -- three
 * device->host synchronisations per step in the reference) as one pass over the f32 tensor x[n] (16-byte aligned) that only ORs device flags:
 * flags[0] any NaN, flags[1] any x > hi, flags[2] any x < lo.  The host mirror (train_ddp.StepGuard) reads the flags asynchronously and raises the
 * reference's assertion no later than one step after the fact. */
int rsuper_guard_range(const float* x, size_t n, float lo, float hi, int* flags, void* stream);
/* The batch consistency checks of calculate_loss (losses_foundation.py:864-869) on device flags: per sample b with m_any[b] != 0 (chosen segment mask not all
 * zero; bytes from rsuper_plane_any), flags[0] |= (u_any[b] == 0) ("unk_voxels should not be all zeros ..."), flags[1] |= (sum_t volumes[b][t] == 0)
 * ("tumor_volumes_report should not be all zeros ...").  volumes: [B][T] f32. */
int rsuper_guard_consistency(const uint8_t* m_any, const uint8_t* u_any, const float* volumes, int B, int T, int* flags, void* stream);
int rsuper_mask_op(uint8_t* a, const uint8_t* b, long V, int op /*0 and, 1 or, 2 andnot*/, void* stream);

/* Bit-packed label ingestion: device-side np.unpackbits(packed, axis=0)[:C] of the label / unk / chosen-
 * segment volumes the dataset stores with np.packbits(axis=0) -- training/dataset/dim3/dataset_abdomenatlas_UFO.py:955,
 * 970,975 (pack), :1031-1034 (unpack).  packed: [B][P = ceil(C/8)][V] bytes (MSB = lowest class), out: [B][C][V] 0/1. */
int rsuper_unpack_bits(const uint8_t* packed, uint8_t* out, int B, int P, int C, long V, void* stream);
/* The inverse: device-side np.packbits(src != 0, axis = class) of the unpacked int8 / uint8 / bool (C, D, H, W) label the dataset converter writes
 * (dataset_conversion/nii2npz.py:80-82; the dataset accepts both forms, dataset_abdomenatlas_UFO.py:465-470).  src: B * C one-byte planes of V voxels, plane
 * (b, c) at src + (b * C + c) * src_plane_stride; any non-zero byte counts as 1.  dst: B * P byte planes, P = ceil(C / 8), plane (b, p) at
 * dst + (b * P + p) * dst_plane_stride; class c is bit 7 - (c & 7) of plane c >> 3, the unused low bits of the last plane are 0.  Both strides are in bytes and
 * >= V: a z-slab in a staging buffer is packed straight into its place of the whole packed volume.  Nothing at or past V of a plane is read or written.
 * 16-byte vectors when both pointers and both strides are multiples of 16, bytes otherwise.  B * P <= 65535. */
int rsuper_pack_bits(const uint8_t* src, uint8_t* dst, int B, int C, long V, long src_plane_stride, long dst_plane_stride, void* stream);
/* Timing events for SURVEY 8(d)'s per-launch measurement (bench.py's roofline pass: HIP events around every conv MFMA launch, on the launch stream): events
 * created with hipEventDisableSystemFence -- a default event performs a system-scope release (cache write-back + invalidate) when recorded, which is charged to the
 * bracket and leaves the next kernel a cold L2; the HIP header recommends the flag for events that only measure time.  elapsed_ms waits for `b`. */
int rsuper_timer_event_create(void** ev);
int rsuper_timer_event_record(void* ev, void* stream);
int rsuper_timer_event_elapsed_ms(void* a, void* b, float* ms);
int rsuper_timer_event_destroy(void* ev);

/* The report losses read only a few planes of a bit-packed volume ("loss kernels should read the packed u8 directly"; losses_foundation.py:286-297,
 * 1571-1605 index the lesion channels of label / unknown / segment mask): plane (b, c) of out[B][C][V] is written iff flags[b * C + c] != 0 or force[c] != 0
 * (flags: [B * C] device bytes or NULL, force: [C] device bytes or NULL; both NULL = rsuper_unpack_bits); the other planes are left untouched, byte planes
 * without a wanted class are not read. */
int rsuper_unpack_bits_sel(const uint8_t* packed, uint8_t* out, int B, int P, int C, long V, const uint8_t* flags, const uint8_t* force, void* stream);
/* flags[b * C + c] = any(class c of sample b) from the packed bytes (OR over byte plane (b, c >> 3), bit 7 - (c & 7)): rsuper_plane_any on the inflated volume
 * at 1/8 of the bytes.  packed 16-byte aligned, V % 16 == 0.  Use: the kflags of rsuper_plane_partials_*2 / the flags of rsuper_dilate_volume_sparse for the
 * unknown-voxel map (get_known_voxels, losses_foundation.py:150-165), the mask / unknown consistency guard (:864-869). */
int rsuper_plane_any_bits(const uint8_t* packed, int B, int P, int C, long V, uint8_t* flags, void* stream);
int rsuper_zero_where(float* x, const uint8_t* m, long V, void* stream);
int rsuper_count(const uint8_t* m, long V, unsigned int* count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prediction post-processing and detection volumes -- predict_abdomenatlas.py, eval_AUC.py.  Volumes up to 2^31 voxels.
 * No call issues a memset: every workspace is initialised by the call's own kernels, so stale contents do not matter.
 * ------------------------------------------------------------------------------------------------ */
/* eval_AUC.detection :56-112 for `planes` f32 volumes x[planes][Di][Hi][Wi]: ndimage.zoom(order=1) onto [Do][Ho][Wo] (f64 align-corners trilinear,
 * input coordinate = o * (n_in - 1) / (n_out - 1); identity when the shapes agree), then for each of the nthr <= 255 thresholds (HOST array, sorted
 * ascending, compared in f64 as `value > t`) the voxel count of binary_dilation(binary_erosion(B_t, box3), box3, iterations=2) & B_t -- computed as
 * one integer pass: level L = #thresholds exceeded, final = min(max5(min3(L)), L) with min3 reading level 0 outside the volume, volume(t) =
 * #(final > t).  erode == 0: #(L > t).  volumes: device [planes][nthr] i64; max_prob: device [planes] f64 = max of the resampled values.
 * workspace: rsuper_detection_workspace_bytes(planes) bytes on the device. */
long rsuper_detection_workspace_bytes(int planes);
int rsuper_detection(const float* x, int planes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, const double* thresholds, int nthr, int erode,
                     long long* volumes, double* max_prob, void* workspace, void* stream);
/* test_with_reports.detection :56-94 for `planes` volumes x[planes][Di][Hi][Wi] (u8 bytes when is_u8, else f32): m = value > th (in f64, like
 * get_fdata(); a value equal to th is not set), ndimage.zoom(m, order=0) onto [Do][Ho][Wo] -- source index floor(c + 0.5) per axis with
 * c = o * (n_in - 1) / (n_out - 1) in f64 (0 for n_out == 1), and the constant 0 where c > n_in - 1 (scipy's 'constant' mode, as for order 1 above)
 * -- then, with erode, binary_dilation(binary_erosion(z, box3), box3, iterations=2) & z, else z; counts: device [planes] i64 = the set voxels.
 * Same tile, LDS passes and integer bins as rsuper_detection; workspace: rsuper_detection_workspace_bytes(planes) bytes on the device.
 * Null pointers, planes outside 1..65535, a NaN th or an empty / over-large grid -> RSUPER_ERR_ARG, checked before anything is launched. */
int rsuper_detection_binary(const void* x, int is_u8, int planes, int Di, int Hi, int Wi, int Do, int Ho, int Wo, double th, int erode,
                            long long* counts, void* workspace, void* stream);
/* postprocess_npz :655-688 (--organ_mask_on_lesion) on pred[C][D][H][W]: out[k] = pred[lesion[k]] * binary_dilation(organ > 0.5, box3), organ =
 * pred[organ_a[k]] (+ pred[organ_b[k]] when organ_b[k] >= 0).  u8: labels, the sum wraps as uint8; f32: probabilities, the sum is an f32 add.
 * lesion / organ_a / organ_b: HOST arrays of n plane indices; out: device [n][D][H][W]. */
int rsuper_organ_mask_u8(const uint8_t* pred, int C, int D, int H, int W, int n, const int* lesion, const int* organ_a, const int* organ_b,
                         uint8_t* out, void* stream);
int rsuper_organ_mask_f32(const float* pred, int C, int D, int H, int W, int n, const int* lesion, const int* organ_a, const int* organ_b,
                          float* out, void* stream);
/* keep_largest_component :692-716: out[D][H][W] (u8) = the largest face-connected component of mask > 0 (mask: u8 when is_u8, else f32); ties go to
 * the component whose first voxel comes first in C order (SimpleITK's label order); an empty mask gives all ones (the reference's
 * Equal(cc, 0)).  Union-find with the smallest linear index as root: tile labelling in LDS, atomicMin links across tiles, path compression,
 * sizes, an atomicMax on (size << 32) | (0xFFFFFFFF - root).  workspace: rsuper_largest_component_workspace_bytes(D, H, W) bytes on the device. */
long rsuper_largest_component_workspace_bytes(int D, int H, int W);
int rsuper_largest_component(const void* mask, int is_u8, int D, int H, int W, uint8_t* out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Report-guided pseudo-label refinement -- baselines/pseudo_labels/pseudo_label_report_refinement.py extract_lesion_candidates :48-70, for `planes`
 * lesion planes [planes][D][H][W] at once, each with its own lesion count.  One iteration of a plane: peak = max(work) at its first C-order voxel;
 * stop when peak < min_peak or kept == n_lesions; thr = peak_cut * peak (one f32 multiply); the 26-connected component of work >= thr that holds the
 * peak voxel is zeroed in work and, when it has at least min_voxels voxels, set to 1 in out and counted in kept.
 * state: planes * RSUPER_LESION_STATE_WORDS 32-bit words on the device (8-byte aligned), per plane
 *   { int kept, iterations, done, n_lesions; u64 peak key; u32 seed root, seed component size }.
 * _begin zeroes out and the state (no memset) and stores the counts (host array; n <= 0: done at once).  _run enqueues `iterations` iterations; every
 * kernel returns at once for a plane whose `done` word is set, so iterations past the end leave work, out and the state as they are: enqueue a batch,
 * read the state, repeat while a plane has neither `done` nor kept == n_lesions.  A plane that is not done zeroes at least one positive voxel per
 * iteration, so the loop ends after at most D*H*W iterations.  work is consumed in place.  workspace: _workspace_bytes on the device, any content.
 * RS_ERR_ARG: null pointers, planes outside 1..RSUPER_LESION_MAX_PLANES, D*H*W > 2^31, !(0 < peak_cut <= 1), !(min_peak > 0), min_voxels < 1,
 * iterations < 1.  Non-finite values in work are the caller's error and the result is then unspecified, but nothing is read out of bounds and every
 * plane ends: the stop test is !(peak >= min_peak), so a plane whose peak is NaN gets `done` at once; a NaN with the sign bit set orders below every
 * value and never enters a mask; +inf is a peak like any other. */
#define RSUPER_LESION_MAX_PLANES 64
#define RSUPER_LESION_STATE_WORDS 8
long rsuper_lesion_candidates_workspace_bytes(int planes, int D, int H, int W);
int rsuper_lesion_candidates_begin(uint8_t* out, int planes, int D, int H, int W, const int* n_lesions, void* state, void* stream);
int rsuper_lesion_candidates_run(float* work, uint8_t* out, int planes, int D, int H, int W, float peak_cut, int min_voxels, float min_peak, void* state,
                                 void* workspace, int iterations, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lesion tables -- no counterpart in the reference: the connected components of masks[planes][D][H][W] (u8, non-zero = foreground; conn 6 or 26)
 * as measured rows.  Components of fewer than min_voxels voxels are dropped; the others are ordered by voxel count descending, ties to the smaller
 * root (the first voxel in C order), and the first max_lesions of a plane are its rows, row k with label k + 1.
 *   totals[planes][4] i64   = { components kept after min_voxels, components dropped by it, foreground voxels, rows written }
 *   rows_i[planes][max_lesions][16] i64 = { root, voxels, zmin, ymin, xmin, zmax, ymax, xmax, sum z, sum y, sum x, p3, q3, pa, qa, flags }
 *   rows_f[planes][max_lesions][4] f64  = { d3, a, b, c } in mm between voxel centres (spacing s0, s1, s2 along D, H, W)
 *   labels[planes][D][H][W] u8 (may be NULL) = 0 background, k + 1 a voxel of row k, 255 a voxel of a component without a row
 * Rows past the last written one are zeroed.  d3: the largest distance between two voxels of the component, (p3, q3) the linear indices of the pair
 * that attains it, p3 <= q3, the lexicographically smallest such pair (one voxel: d3 = 0, p3 = q3 = root).  a, (pa, qa): the same among pairs in one
 * axis-0 slice, over all slices.  b: in the slice of (pa, qa), over the component's voxels v there, (max t_v - min t_v) / a with
 * t_v = (dy s1)(x_v s2) - (dx s2)(y_v s1), (dy, dx) = qa - pa; 0 when a = 0.  c = (zmax - zmin) s0.  Squared distances are compared as
 * (s0^2 dz^2 + s1^2 dy^2) + s2^2 dx^2 in f64, every product and sum rounded on its own.  The searches run over the voxels that have, along no axis
 * (3-D) / along neither H nor W (in-slice), both neighbours in their own component: no other voxel can end an attaining pair.  A component with more
 * than max_candidates such voxels for the 3-D search gets d3 = NaN, p3 = q3 = -1 and bit 0 of flags; its other fields stay exact.
 * workspace: rsuper_lesion_table_workspace_bytes bytes on the device, 8-byte aligned like rows_i, rows_f and totals; it and the outputs may hold
 * anything on entry.  rsuper_lesion_table_launches() kernels on `stream`, no memset, no device-to-host read.
 * RSUPER_ERR_ARG, before anything is launched: null pointers (labels excepted), planes outside 1..RSUPER_LESION_MAX_PLANES, D*H*W > 2^31, conn other
 * than 6 or 26, min_voxels < 1, max_lesions outside 1..RSUPER_LESION_TABLE_MAX_ROWS, max_candidates < 2, a spacing that is not finite and > 0,
 * misaligned outputs, workspace_bytes below the requirement.  _workspace_bytes answers 0 for a shape it refuses. */
#define RSUPER_LESION_TABLE_MAX_ROWS 254
long rsuper_lesion_table_workspace_bytes(int planes, int D, int H, int W, int max_lesions);
int rsuper_lesion_table_launches(void);
int rsuper_lesion_table(const uint8_t* masks, int planes, int D, int H, int W, int conn, int min_voxels, int max_lesions, int max_candidates, double s0,
                        double s1, double s2, long long* rows_i, double* rows_f, long long* totals, uint8_t* labels, void* workspace,
                        long workspace_bytes, void* stream);
/* Joint histogram of two label volumes [planes][voxels] u8 with values 0..Ka and 0..Kb (each at most RSUPER_LESION_TABLE_MAX_ROWS):
 * counts[planes][Ka + 1][Kb + 1] i64 (8-byte aligned, any content on entry).  A voxel whose value is above Ka / Kb on either side (255 among them)
 * counts nowhere; counts[.][0][0] stays 0 -- voxels that are background on both sides are skipped.  Two launches, integer atomics. */
int rsuper_label_overlap(const uint8_t* labels_a, const uint8_t* labels_b, int planes, long voxels, int Ka, int Kb, long long* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validation metrics -- metric/metrics.py compute_surface_distances :265-573.  Masks of up to 2^31 corners ((D+1) * (H+1) * (W+1)).
 * No call issues a memset: counters and bounds are initialised by the call's own kernels.
 * ------------------------------------------------------------------------------------------------ */
/* Neighbour codes of two mask stacks gt, pred [planes][D][H][W] (u8, non-zero = foreground) on the corner grid: codes_*[planes][D+1][H+1][W+1] =
 * correlate(mask, [[[128, 64], [32, 16]], [[8, 4], [2, 1]]], mode='constant'), corner (i, j, k) seeing voxels i-1..i, j-1..j, k-1..k and zero outside.
 * bbox: device [planes][6] i32 = min z, y, x and max z, y, x of the corners whose code is a border code (neither 0 nor 255) in either mask
 * (min > max when there is none).  counts: device [planes][5] i64 = |gt|, |pred|, |gt & pred|, border corners of gt, border corners of pred. */
int rsuper_surface_codes(const uint8_t* gt, const uint8_t* pred, int planes, int D, int H, int W, uint8_t* codes_gt, uint8_t* codes_pred,
                         int* bbox, long long* counts, void* stream);
/* Exact squared Euclidean distance transform, distance_transform_edt(~borders, sampling=(s0, s1, s2)) ** 2 in f64, of the sub-box
 * [z0, z0 + nz) x [y0, y0 + ny) x [x0, x0 + nx) of one code volume codes[Dc][Hc][Wc] to the border corners inside the box: out[nz][ny][nx].
 * Separable: a wave-level scan along W, then a lower envelope per line along H and D (Felzenszwalb-Huttenlocher) whose stacks live in the
 * workspace (rsuper_edt3_workspace_bytes(nz, ny, nx) bytes on the device; 0 = unsupported box: a side above 4096 corners or more than 2^31
 * corners).  A box without a border corner gives +inf everywhere.  workspace_bytes below the requirement is refused with RSUPER_ERR_ARG. */
long rsuper_edt3_workspace_bytes(int nz, int ny, int nx);
int rsuper_edt3(const uint8_t* codes, int Dc, int Hc, int Wc, int z0, int y0, int x0, int nz, int ny, int nx, double s0, double s1, double s2,
                double* out, void* workspace, long workspace_bytes, void* stream);
/* For every border corner of codes[Dc][Hc][Wc] inside the box: dist = sqrt(sqdist[box index]) (sqdist NULL: +inf, the other mask has no surface),
 * area = table[code] (table: device [256] f64), compacted into dist / area [capacity] in an order that is not fixed (the caller sorts the pairs);
 * *count (device i64) = number of border corners in the box.  Pairs beyond capacity are counted, not written. */
int rsuper_surfel_gather(const uint8_t* codes, int Dc, int Hc, int Wc, int z0, int y0, int x0, int nz, int ny, int nx, const double* sqdist,
                         const double* table, double* dist, double* area, long long* count, long capacity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spatial augmentation -- training/augmentation.py random_scale_rotate_translate_3d :228-319 + crop_3d :446-469.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_AFFINE_MAX_VOLUMES 3
#define RSUPER_AFFINE_MAX_PLANES 64
/* F.affine_grid(theta, (B, C, D, H, W), align_corners=True) + F.grid_sample(align_corners=True, padding_mode='zeros') evaluated only on the crop
 * [oz, oz + d) x [oy, oy + h) x [ox, ox + w) of the full D x H x W output grid (the offset shifts output indices; the transform stays centred on the
 * full grid).  theta: device [B][3][4] f32, rows x, y, z as affine_grid takes them.  img [B][Ci][D][H][W] f32 -> img_out [B][Ci][d][h][w], trilinear,
 * every corner tested for bounds.  nvol <= RSUPER_AFFINE_MAX_VOLUMES byte volumes vols[k] [B][planes[k]][D][H][W] u8 -> vols_out[k]
 * [B][planes[k]][d][h][w], the byte of the nearest voxel (half to even), 0 out of bounds, with the image's coordinates; 1 <= planes[k] <=
 * RSUPER_AFFINE_MAX_PLANES (bit-packed class planes or plain u8 planes alike).  vols, vols_out, planes: HOST arrays (of device pointers);
 * offsets: HOST [B][3] ints (z, y, x per sample).  Coordinates are computed in f64.  D, H, W >= 2 (N == 1 has no align-corners coordinate) and
 * D * H * W < 2^31; the crop must lie inside the grid.  One launch per 8 samples, no workspace. */
int rsuper_affine_crop(const float* theta, const float* img, float* img_out, int B, int Ci, int D, int H, int W, int nvol,
                       const uint8_t* const* vols, uint8_t* const* vols_out, const int* planes, int d, int h, int w, const int* offsets,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Intensity augmentation -- training/augmentation.py brightness_multiply / brightness_additive / gamma / contrast / gaussian_blur /
 * gaussian_noise :27-103, gated per sample as dataset/augmented.py online_intensity_augmentation :142-158.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_BLUR_MAX_RADIUS 5
/* img [B][1][D][H][W] f32 -> out (another buffer of the same shape; img is not modified).  Per sample b, HOST arrays: flags[b] = bit 0 multiply, 1 additive,
 * 2 gamma, 3 contrast, 4 blur, 5 noise (the transforms that fired; they apply in this order); scalars[b][5] = multiply factor, additive offset, gamma
 * exponent, contrast factor, noise std; radius[b] and taps[b][2 * RSUPER_BLUR_MAX_RADIUS + 1] (the first 2 * radius + 1 are read) for the zero-padded
 * separable blur W -> H -> D of the post-contrast image; seeds[b] = the Philox4x32-10 key of the in-kernel N(0, 1) field (counter (i >> 2, 0, 0) for voxel
 * i of the sample, two Box-Muller pairs, voxel i takes normal i & 3).  noise: optional device [B][1][D][H][W] f32 that replaces the generator.
 * gamma: lo, hi, mean, unbiased std of x2 = x * f + a; y = pow((x2 - lo) / (hi - lo), g) * (hi - lo) + lo; z = (y - mean y) / std y * std + mean (a
 * constant volume gives NaN, as the host code does).  contrast: clamp((v - mean) * c + mean, lo, hi) with lo, hi, mean of its input -- after gamma
 * they are z(min y), z(max y) and gamma's restored mean.  The reductions go through per-block partials in `workspace` (device,
 * rsuper_intensity_augment_workspace_bytes(B, D, H, W) bytes; needed when gamma or contrast fires anywhere; 0 = an empty shape) combined in a fixed
 * order: no atomics, no memset, bit-reproducible.  rsuper_intensity_augment_launches: kernel launches the call makes for these flags (per group of 8
 * samples: 1, +1 with contrast or gamma, +1 with gamma).  A blur radius above RSUPER_BLUR_MAX_RADIUS, flags outside 0..63, D * H * W >= 2^31 or a missing /
 * short workspace -> RSUPER_ERR_ARG. */
long rsuper_intensity_augment_workspace_bytes(int B, int D, int H, int W);
int rsuper_intensity_augment_launches(int B, const int* flags);
int rsuper_intensity_augment(const float* img, float* out, int B, int D, int H, int W, const int* flags, const float* scalars, const int* radius,
                             const float* taps, const unsigned long long* seeds, const float* noise, void* workspace, long workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Models Genesis pre-training -- baselines/model_genesis/utils.py generate_one_pair :206-266 (flips :50, local_pixel_shuffling :76,
 * nonlinear_transformation :61, image_in_painting :106, image_out_painting :125) and losses_foundation.py model_genesis_loss :667.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_GENESIS_MAX_BOXES 5
#define RSUPER_GENESIS_MAX_BLOCK_SIDE 16
#define RSUPER_GENESIS_MAX_AXIS 169
/* img [B][D][H][W] f32 -> the pair x, y (two more buffers of that shape; none may alias another).  The reference's (rows, cols, deps) are (D, H, W).
 * Per sample b, HOST arrays: flags[b] = bit 0 / 1 / 2 the net flip of D / H / W (x and y alike), 3 local pixel shuffling, 4 the non-linear intensity
 * curve, 5 in-painting, 6 out-painting (5 and 6 exclude each other); nbox[b] <= RSUPER_GENESIS_MAX_BOXES and boxes[b][RSUPER_GENESIS_MAX_BOXES][6] =
 * (z0, y0, x0, nz, ny, nx) of the painted boxes, inside the volume; seeds[b] = the Philox4x32-10 key of the sample.  DEVICE arrays:
 * blocks [B][nb][6] (z0, y0, x0, nz, ny, nx), the nb shuffled blocks of every sample in the order they apply, a side at most
 * RSUPER_GENESIS_MAX_BLOCK_SIDE; perm (optional) the source position of every box position, flattened row-major and concatenated, block k of sample b at
 * perm_off[b][k] (perm_len entries in all): box.flat[i] = orig_box.flat[perm[i]], where orig is the flipped normalised image, never the partly shuffled
 * one -- a voxel carries what the last block covering it wrote.  Without perm the device draws perm_k = the stable argsort of the keys
 * philox(counter (i, k, 2, 0), seed)[0], i = 0 .. n_k - 1 (uniform up to the probability of a tie, about n_k^2 / 2^33).  A block that does not lie inside
 * the volume, a side outside 1 .. 16, offsets past perm_len and perm entries outside 0 .. n_k - 1 are skipped on the device (the voxels keep orig).
 * curve [B][2][n] f64: the knots xp (ascending) and fp of np.interp, evaluated in f64 with np.interp's expression (multiply and add unfused) and rounded
 * to f32 once.  noise: optional [B][D][H][W] f32 field of the painted values in the output frame; without it voxel i takes u = ((r >> 8) + 0.5) * 2^-24
 * of word i & 3 of philox(counter (i >> 2 low, i >> 2 high, 1, 0), seed).
 * v = (img - min) / max(max - min, 1e-7f) per sample; y = flip(v); x = flip(v) -> shuffle -> curve -> paint; both leave as v * span + min, in f32 with
 * IEEE division and unfused multiply-add: bit for bit the reference's values for the same plan.  workspace: device, 8-byte aligned,
 * rsuper_genesis_workspace_bytes(B, D, H, W, nb) bytes (nb = 0 when no sample shuffles).  rsuper_genesis_launches: kernel launches of the call, per group
 * of 8 samples 4 when one of them shuffles, else 2.  No float atomics, no memset: bit-reproducible.  An axis above RSUPER_GENESIS_MAX_AXIS, flags outside
 * 0..127 or with bits 5 and 6, a painted box outside the volume, a missing array or a short workspace -> RSUPER_ERR_ARG. */
long rsuper_genesis_workspace_bytes(int B, int D, int H, int W, int nb);
int rsuper_genesis_launches(int B, const int* flags);
int rsuper_genesis_pair(const float* img, float* x, float* y, int B, int D, int H, int W, const int* flags, int nb, const int* blocks, const int* perm,
                        const long long* perm_off, long long perm_len, const double* curve, int n, const int* nbox, const int* boxes,
                        const unsigned long long* seeds, const float* noise, void* workspace, long workspace_bytes, void* stream);
/* out[0] = mean((r - y)^2) over n f32 elements: per block the f64 sum of the exact squared differences rounded to one f32 partial in `workspace`
 * (device, rsuper_mse_workspace_bytes(n) bytes), then one block sums the partials in a fixed order -- two launches, no atomics.
 * rsuper_mse_bwd: dr = g[0] * 2 * (r - y) / n, evaluated in f64 and rounded once (g: the device scalar gradient of out). */
long rsuper_mse_workspace_bytes(long n);
int rsuper_mse_fwd(const float* r, const float* y, long n, float* out, void* workspace, long workspace_bytes, void* stream);
int rsuper_mse_bwd(const float* r, const float* y, const float* g, long n, float* dr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-task and CLIP baselines -- model/dim3/medformer.py ClassificationBranch :12-78, training/losses_foundation.py classification_loss
 * :614-664, training/info_nce.py :63-126.
 * ------------------------------------------------------------------------------------------------ */
/* The tail of ClassificationBranch after its extra_layer, one workgroup per sample: reducer Conv3d(160, 64, 1) -> TransformerBlock(dim 64, depth 1,
 * 4 heads x 16, mlp 320; pre-LayerNorm eps 1e-5, exact erf GELU, residuals) -> mean over the L tokens -> Linear(64, Nc).  All f32.
 * x [B][L][160] channels-last tokens; weights: HOST array of 15 device pointers, 16-byte aligned, contiguous f32 in torch's [out][in] layout:
 *   reducer.weight [64][160], reducer.bias, norm1.weight, norm1.bias, to_qkv.weight [192][64], to_out.weight [64][64], to_out.bias, norm2.weight,
 *   norm2.bias, fc1.weight [320][64], fc1.bias, fc2.weight [64][320], fc2.bias, head.weight [Nc][64], head.bias.
 * _fwd: one launch, grid B; writes out [B][Nc] and the activations the backward reads into save (device, 16-byte aligned,
 *   B * rsuper_cls_tail_save_floats(L) floats, any content).
 * _bwd: two launches.  The first (grid B) reads dout [B][Nc] and save (which it also uses as scratch), writes dx [B][L][160] and the per-sample
 *   gradient of every parameter into partials (device, 16-byte aligned, rsuper_cls_tail_partial_floats(B, Nc) floats); the second adds the partials
 *   in sample order into grads: rsuper_cls_tail_param_floats(Nc) floats, the parameters in the order of `weights`, each in its own layout.
 * No atomics, no memset, every sum in a fixed order: bit-reproducible.  1 <= L <= 64 and 1 <= Nc <= 768 (rsuper_cls_tail_supported, answered on the
 * host); other sizes -> RSUPER_ERR_UNSUPPORTED; null / misaligned pointers -> RSUPER_ERR_ARG, checked before anything is launched. */
int rsuper_cls_tail_supported(int L, int Nc);
long rsuper_cls_tail_save_floats(int L);
long rsuper_cls_tail_param_floats(int Nc);
long rsuper_cls_tail_partial_floats(int B, int Nc);
int rsuper_cls_tail_fwd(const float* x, const void* const* weights, float* out, float* save, int B, int L, int Nc, void* stream);
int rsuper_cls_tail_bwd(const float* x, const void* const* weights, const float* dout, float* save, float* dx, float* partials, float* grads, int B, int L,
                        int Nc, void* stream);
/* classification_loss from presence flags, one launch.  logits [B][Nc] f32; flags_* [B][C] u8 "class c of sample b has a voxel" of the label, the
 * chosen segment mask and the unknown voxels (mask / unknown may be NULL = none); class_set: bit c = class c is one of the Nc classes of the head, in
 * class order (C <= 64, popcount == Nc); weights: NULL or [B][Nc] f32.  target = label | mask; an entry with an unknown flag and a zero target counts 0;
 * loss[0] = sum(weight * BCE-with-logits) / (B * Nc) and dlogits [B][Nc] = its derivative, both evaluated in f64 in a fixed order and rounded once. */
int rsuper_cls_loss(const float* logits, const uint8_t* flags_label, const uint8_t* flags_mask, const uint8_t* flags_unk, const float* weights, int B, int C,
                    int Nc, unsigned long long class_set, float* loss, float* dlogits, void* stream);
/* info_nce with implicit negatives, reduction 'mean', one launch: rows L2-normalised (eps 1e-12), logits = q k^T / temperature, cross-entropy against the
 * diagonal.  query, key [N][D] f32; loss[0] and dquery, dkey [N][D] = the derivatives, f64 sums in a fixed order, rounded once.  N <= 64
 * (rsuper_info_nce_supported), else RSUPER_ERR_UNSUPPORTED. */
int rsuper_info_nce_supported(int N, int D);
int rsuper_info_nce(const float* query, const float* key, int N, int D, double temperature, float* loss, float* dquery, float* dkey, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-CT preprocessing and spacing resampling -- predict_abdomenatlas.py preprocess :325-356 (from the clip onward), pad_to_training_size
 * :249-306, unpad_img :311-322, resample_image_with_gpu :718-742.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_VOX_U8 0
#define RSUPER_VOX_F32 1
#define RSUPER_VOX_I16 2
#define RSUPER_RESAMPLE_NEAREST 0
#define RSUPER_RESAMPLE_TRILINEAR 1
/* z-score of clip(x, lo, hi) in two launches.  x: device [D][H][W], dtype RSUPER_VOX_I16 (HU as a CT stores them) or RSUPER_VOX_F32, D * H * W < 2^31.
 * rsuper_ct_stats writes a fixed number of per-block f64 partials (count, sum, sum of squares) into `workspace` (device, 8-byte aligned, at least
 * rsuper_ct_stats_workspace_bytes() bytes; every partial is written: no memset).  rsuper_ct_normalize re-reduces them in a fixed order in every block,
 * forms mean and the unbiased std in f64, rounds each to f32, stores them to mean_std[0..1] (device) and writes (clip(x) - mean) / std (IEEE
 * division) into out [Do][Ho][Wo] f32 at the box (z_lo, y_lo, x_lo) + (D, H, W); every voxel outside the box is 0 (the reference pads after
 * normalising).  No atomics, no host synchronisation between the two launches, bit-reproducible.  Nothing degenerate is special-cased: a constant
 * volume gives 0 / 0 = NaN inside the box, D * H * W == 1 gives NaN.  rsuper_pad_box: the same padded write of x itself (no clip, no statistics).
 * Null pointers, non-positive sizes, a box outside the output, out == x or a short workspace -> RSUPER_ERR_ARG, checked before anything is launched. */
long rsuper_ct_stats_workspace_bytes(void);
int rsuper_ct_stats(const void* x, int dtype, int D, int H, int W, float lo, float hi, void* workspace, long workspace_bytes, void* stream);
int rsuper_ct_normalize(const void* x, int dtype, int D, int H, int W, float lo, float hi, const void* workspace, long workspace_bytes, float* out,
                        int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo, float* mean_std, void* stream);
/* rsuper_ct_normalize with the population standard deviation: sqrt((Q - N mean^2) / N), numpy's np.std (ddof = 0), which dataset_conversion/nii2npz.py
 * :71-74 uses.  The same kernel, arguments and checks; N == 1 gives 0 / 0 = NaN. */
int rsuper_ct_normalize_pop(const void* x, int dtype, int D, int H, int W, float lo, float hi, const void* workspace, long workspace_bytes, float* out,
                            int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo, float* mean_std, void* stream);
int rsuper_pad_box(const void* x, int dtype, int D, int H, int W, float* out, int Do, int Ho, int Wo, int z_lo, int y_lo, int x_lo, void* stream);
/* One launch: src [C][Dp][Hp][Wp] (RSUPER_VOX_U8 / RSUPER_VOX_F32), of every plane the sub-box (z0, y0, x0) + (D, H, W) -> out [C][Do][Ho][Wo].
 * mode RSUPER_RESAMPLE_NEAREST: scale = (float)n_in / (float)n_out, src = min((int)floorf((float)dst * scale), n_in - 1) (F.interpolate 'nearest');
 * RSUPER_RESAMPLE_TRILINEAR: scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0, s = scale * (float)dst, i0 = min((int)s, n_in - 1),
 * i1 = i0 + (i0 < n_in - 1), l1 = s - (float)i0, l0 = 1 - l1 (align_corners = True), lerps in x, y, z order, all f32.  out_dtype RSUPER_VOX_F32: the
 * value; RSUPER_VOX_U8 with use_threshold: value > threshold as 0 / 1; RSUPER_VOX_U8 without: u8 input and nearest only (a copy of bytes), anything
 * else -> RSUPER_ERR_UNSUPPORTED.  Dp * Hp * Wp and Do * Ho * Wo < 2^31, C <= 65535.  Null pointers, non-positive sizes, a sub-box outside the
 * tensor, an unknown dtype or mode -> RSUPER_ERR_ARG, checked before anything is launched. */
int rsuper_resample3d(const void* src, int in_dtype, int C, int Dp, int Hp, int Wp, int z0, int y0, int x0, int D, int H, int W, void* out,
                      int out_dtype, int Do, int Ho, int Wo, int mode, int use_threshold, float threshold, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Crop-on-tumour from a whole CT with a bit-packed label -- training/augmentation.py random_crop_on_tumor :600, negative_crop :662, organ_crop :675,
 * tumor_crop :716, crop_around_coordinate_3d :498, pad_volume_pair :1023.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_CROP_CHUNK 16384
#define RSUPER_CROP_MAX_CLASSES 64
/* packed: device [B][P][D][H][W] u8 as np.packbits(axis = class) wrote it (class c = bit 7 - (c & 7) of byte plane c >> 3), ceil(C / 8) <= P <= 8,
 * C <= RSUPER_CROP_MAX_CLASSES, D * H * W < 2^31.  Launch 1 writes the chunk table [B][chunks][C + 1] int32 into `workspace` (device, 4-byte aligned,
 * rsuper_class_counts_workspace_bytes bytes; chunks = ceil(D * H * W / RSUPER_CROP_CHUNK), a chunk = RSUPER_CROP_CHUNK consecutive voxels in row-major
 * order): per chunk the set voxels of every class and, in column C, the voxels whose P bytes are all zero (the background).  Launch 2 sums the rows
 * into totals [B][C + 1] int64 (device).  Every entry is written: no memset, no atomics, bit-reproducible.  Any base alignment and any voxel count.
 * plain != 0: the label is [B][C][D][H][W] bytes instead (P == C, class c = plane c, set = byte not zero), the table is the same. */
long rsuper_class_counts_workspace_bytes(int B, int C, int D, int H, int W);
int rsuper_class_counts(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, void* workspace, long workspace_bytes, long long* totals,
                        void* stream);
/* zyx (device, 3 int32) = (z + add_z, y + add_y, x + add_x) of the k-th voxel, in row-major order, of sample b whose bit of class `column` is set
 * (column == C: whose P bytes are all zero): torch.nonzero(mask)[k].  workspace: the chunk table rsuper_class_counts wrote for this tensor.  count:
 * the column's total as the caller read it; k < 0 or k >= count -> RSUPER_ERR_ARG, nothing is launched.  One block; it reads the table and one chunk. */
int rsuper_select_voxel(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, const void* workspace, long workspace_bytes, int b, int column,
                        long k, long count, int add_z, int add_y, int add_x, int* zyx, void* stream);
/* One launch per 8 samples: img [B][Ci][D][H][W] (RSUPER_VOX_F32 or RSUPER_VOX_I16; Ci == 0: no image) -> img_out [B][Ci][d][h][w] f32, and nvol <=
 * RSUPER_AFFINE_MAX_VOLUMES byte volumes vols[k] [B][planes[k]][D][H][W] -> vols_out[k] [B][planes[k]][d][h][w] (vols, vols_out, planes: HOST arrays).
 * The source counts as zero-padded to (max(D, pad_d), max(H, pad_h), max(W, pad_w)) with (padded - real) / 2 voxels on the low side (pad_volume_pair);
 * all coordinates are padded coordinates and no padded copy is made.  origin: HOST [B][3] ints.  center == NULL: the crop's corner itself, inside
 * [0, padded size - crop].  center: device [B][3] int32 (rsuper_select_voxel's output): corner = clip(center - crop / 2 + origin, 0, padded size -
 * crop), origin being the host-drawn shift (crop_around_coordinate_3d 'small_rnd_shift').  origin_out: optional device [B][3] int32 that receives the
 * corner used.  A crop larger than the padded source, a corner outside it or null pointers -> RSUPER_ERR_ARG, checked before anything is launched. */
int rsuper_crop_box(const void* img, int img_dtype, float* img_out, int B, int Ci, int D, int H, int W, int nvol, const uint8_t* const* vols,
                    uint8_t* const* vols_out, const int* planes, int d, int h, int w, int pad_d, int pad_h, int pad_w, const int* center,
                    const int* origin, int* origin_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The report-annotated branch of the whole-CT crop -- dataset_abdomenatlas_UFO.py get_random_tumor_seg_mask :855, assign_labels :1154,
 * get_chosen_segment_mask :808; training/augmentation.py crop_foreground_3d :790, denoise_mask :746.  No memset, no atomics, bit-reproducible; every
 * argument is checked before anything is launched (RSUPER_ERR_ARG); any base alignment of the label and any voxel count.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_OPEN_MAX_RADIUS 4
#define RSUPER_REMAP_TABLE_WORDS 448
/* packed, B, P, C, plain, D, H, W: the label of rsuper_class_counts.  sets: HOST [B] 64-bit class sets (bit c = class c; a bit at or above C ->
 * RSUPER_ERR_ARG); a voxel is on where any class of its sample's set is.  count [B] int64 and bbox [B][6] int32 (device): the on voxels and their
 * min z, y, x, max z, y, x; none: min = (D, H, W), max = (-1, -1, -1).  Only the planes a set touches are read.  Launch 1 writes one row of 8 int32
 * per RSUPER_CROP_CHUNK voxels into `workspace` (device, 4-byte aligned, rsuper_union_bbox_workspace_bytes bytes), launch 2 folds them in a fixed
 * order; one launch 1 per 8 samples. */
long rsuper_union_bbox_workspace_bytes(int B, int D, int H, int W);
int rsuper_union_bbox(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, const unsigned long long* sets, void* workspace,
                      long workspace_bytes, long long* count, int* bbox, void* stream);
/* The same union of sample b inside the sub-box (z0, y0, x0) + (nz, ny, nx) as bits [nz][ny][ceil(nx / 64)] u64 (device, 8-byte aligned): bit i of
 * word k of a row is voxel x0 + 64 k + i, bits past nx are zero.  One launch, one wave per word.  A sub-box outside the volume -> RSUPER_ERR_ARG. */
int rsuper_union_bits(const uint8_t* packed, int B, int P, int C, int plain, int D, int H, int W, int b, unsigned long long set, int z0, int y0, int x0,
                      int nz, int ny, int nx, unsigned long long* bits, void* stream);
/* binary_dilation(binary_erosion(m, iterations = r), iterations = r) & m of the bit volume `bits` [nz][ny][ceil(nx / 64)] (scipy's default cross,
 * border_value = 0: zero is read outside the box), 1 <= r <= RSUPER_OPEN_MAX_RADIUS, in 2 r + 1 launches over two ping-pong copies in `workspace`
 * (device, 8-byte aligned, rsuper_bits_open_workspace_bytes bytes).  Bits past nx in a row's last word are ignored on input.  out_bits: the result in
 * the same layout; `bits`, out_bits and the workspace must not overlap (RSUPER_ERR_ARG); out_mask: the result as
 * [nz][ny][nx] u8 0 / 1; count (1 int64) and bbox (6 int32), device: as rsuper_union_bbox writes them, in box coordinates + (add_z, add_y, add_x). */
long rsuper_bits_open_workspace_bytes(int nz, int ny, int nx);
int rsuper_bits_open(const unsigned long long* bits, int nz, int ny, int nx, int r, int add_z, int add_y, int add_x, void* workspace, long workspace_bytes,
                     unsigned long long* out_bits, uint8_t* out_mask, long long* count, int* bbox, void* stream);
/* in: device [B][P_in][v] u8 bit-packed as above (C_in classes, ceil(C_in / 8) <= P_in <= 8) -> nvol <= 3 volumes outs[k] [B][P_out][v] (outs: HOST
 * array of device pointers, none of them `in`) of C_out classes, P_out = ceil(C_out / 8).  masks: HOST [B][nvol][C_out], ones: HOST [B][nvol], 64-bit:
 * class j of volume k of sample b at a voxel = (the voxel's input classes & masks[b][k][j]) != 0 || bit j of ones[b][k]; the padding bits of the last
 * plane are zero.  The tables travel in the kernel arguments: one launch per min(8, RSUPER_REMAP_TABLE_WORDS / (nvol * C_out)) samples.  A table bit
 * at or above C_in (masks) or C_out (ones) -> RSUPER_ERR_ARG.  Dword loads and stores when v % 4 == 0 and the bases are 4-byte aligned. */
int rsuper_label_remap(const uint8_t* in, int B, int P_in, int C_in, long v, int nvol, uint8_t* const* outs, int P_out, int C_out,
                       const unsigned long long* masks, const unsigned long long* ones, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser -- train_ddp.py:352-357, training/utils.py:46-51,154-161.  host_* are HOST arrays of device pointers.
 * ------------------------------------------------------------------------------------------------ */
/* *total_sq = sum of squared elements of the n gradient tensors (f64, deterministic order).  The accumulator need not be zeroed: the first launch
 * assigns it -- and no hipMemsetAsync is issued, so the call is safe to capture in a hipGraph (a captured memset node writes 0xC0 bytes after eager
 * interludes on ROCm 7.2: DESIGN.md 3.4c).  The same holds for rsuper_plane_any's flags and rsuper_maxpool2_bwd's zero fill. */
int rsuper_grad_sqnorm(int n, void* const* host_g, const size_t* host_numel, double* total_sq, void* stream);
int rsuper_clip_scale(int n, void* const* host_g, const size_t* host_numel, float max_norm, const double* total_sq, void* stream);
/* One fused pass: clip (coef from *total_sq, NULL = no clipping) + AdamW + EMA (host_ema NULL = no EMA). */
int rsuper_adamw_ema_step(int n, void* const* host_p, void* const* host_g, void* const* host_m, void* const* host_v,
                          void* const* host_ema, const size_t* host_numel, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int step, float ema_alpha, float max_norm, const double* total_sq, void* stream);
/* Same update with the step-dependent scalars read on the device: dyn = [lr, lr / (1 - beta1^t), sqrt(1 - beta2^t), ema_alpha] (f32).
 * A training step captured in a hipGraph replays this launch unchanged while the host refreshes the four floats before each replay. */
int rsuper_adamw_ema_step_dyn(int n, void* const* host_p, void* const* host_g, void* const* host_m, void* const* host_v,
                              void* const* host_ema, const size_t* host_numel, float beta1, float beta2, float eps, float weight_decay,
                              float max_norm, const double* total_sq, const float* dyn, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DEFLATE on the device -- the np.savez_compressed of uint8 masks (baselines/pseudo_labels/pseudo_label_report_refinement.py:153,
 * to_npz.py:63, and the .npz files this package's predict_abdomenatlas writes), a zlib pass on one host thread.  csrc/deflate.hip.
 * ------------------------------------------------------------------------------------------------ */
/* Every plane becomes one raw DEFLATE stream (RFC 1951) that zlib inflates with wbits = -15: one byte-aligned fragment per chunk of
 * rsuper_deflate_chunk_bytes() input bytes -- a Huffman block with the caller's code table closed by an empty stored block, or a stored block when that is
 * shorter -- and the closing block 01 00 00 FF FF.  Tokens are literals and matches of 3..258 bytes at distance 1 (a run) or `pitch` (the row above);
 * the greedy rule is written down at the top of csrc/deflate.hip and restated in tests/deflate_ref.py.  Integer arithmetic only: the bytes are a function
 * of the input.
 * Host functions: the largest stream of an n-byte plane (<= n + n / 1024 + 64), the workspace of a call, the chunk and the segment (the bytes one lane
 * parses; a match never crosses a segment boundary). */
size_t rsuper_deflate_bound(size_t n);
size_t rsuper_deflate_workspace_bytes(int planes, size_t n);
int rsuper_deflate_chunk_bytes(void);
int rsuper_deflate_segment_bytes(void);
/* src: planes byte planes of n bytes (0 <= n < 2^32), plane p at src + p * plane_stride (any alignment, stride >= n), 1 <= planes <= 65535.
 * pitch: 0 (runs only) or the row length 1..32768; a larger one -> RSUPER_ERR_ARG.
 * table: device, 316 words, (bits << 24) | bit-reversed code for the 286 literal/length symbols and then the 30 distance symbols; header: device words
 * holding the header_bits (3..4096) bits that open a block, least significant bit first: BFINAL = 0, BTYPE and, for BTYPE 10, the code lengths.
 * out: device, planes * rsuper_deflate_bound(n) bytes; the streams lie back to back in plane order, stream p at out + offsets[p], sizes[p] bytes long;
 * crcs[p] = CRC-32 of plane p.  offsets, sizes, crcs: device arrays of `planes` entries.  Three launches, no memset. */
int rsuper_deflate_planes(const uint8_t* src, long plane_stride, size_t n, int planes, int pitch, const uint32_t* table, const uint32_t* header,
                          int header_bits, uint8_t* out, unsigned long long* offsets, unsigned long long* sizes, uint32_t* crcs, void* workspace,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * NIfTI front and back end of a case -- reorientation, the cubic B-spline prefilter and the "B-spline in-plane, nearest along z" resample that
 * precede the clip in predict_abdomenatlas.py preprocess (:333-343, dataset_conversion/utils.py:10-47), and masks back in the file's voxel order.
 * csrc/nifti.hip; the tables and headers are made on the host (inference/nifti.py).
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_NII_U8 0
#define RSUPER_NII_I8 1
#define RSUPER_NII_I16 2
#define RSUPER_NII_U16 3
#define RSUPER_NII_I32 4
#define RSUPER_NII_F32 5
/* src: device, the file's voxel buffer of n_src elements of `dtype`.  Canonical voxel (z, y, x) is element offset + z * sz + y * sy + x * sx of it
 * (a flipped axis has a negative stride) and is scaled as (float)v * slope + inter in f32 unless slope == 1 and inter == 0.
 * out: device [Z][Y][X] f32.  prefilter == 0: the scaled samples.  Otherwise the cubic B-spline coefficients of every slice: the causal and
 * anticausal recursion with pole sqrt(3) - 2 along x, then along y (in place), whole-sample mirror boundaries, the start sums cut where |z1|^k
 * falls below 2^-30 (16 terms); a line of one sample is the sample.  One launch, two with prefilter (and Y > 1).
 * A side above 4096 -> RSUPER_ERR_UNSUPPORTED.  Null or misaligned pointers, out == src, an unknown dtype, non-positive sizes or strides that
 * leave the buffer -> RSUPER_ERR_ARG, checked before anything is launched. */
int rsuper_nifti_load_prefilter(const void* src, int dtype, long n_src, int Z, int Y, int X, long sz, long sy, long sx, long offset, float slope,
                                float inter, int prefilter, float* out, void* stream);
/* coef: device [Z][Y][X] f32 coefficients.  ix, wx [Xo][4] and iy, wy [Yo][4] (device int32 / f32): the four source indices (mirror applied) and
 * weights of an output index, ix[o][0] < 0 = outside; iz [Zo] int32: the source slice, < 0 = outside.
 * out [Zo][Yo][Xo] f32 = sum_j wy[j] sum_i wx[i] coef[iz][iy[j]][ix[i]], or outside_value where any axis is outside.  Indices are clamped into the
 * volume before they are used.  One launch.  Input sides above 4096 or Zo above 65535 -> RSUPER_ERR_UNSUPPORTED; null or misaligned pointers,
 * out == coef, non-positive sizes -> RSUPER_ERR_ARG. */
int rsuper_bspline_resample(const float* coef, int Z, int Y, int X, const int* ix, const float* wx, const int* iy, const float* wy, const int* iz,
                            float* out, int Zo, int Yo, int Xo, float outside_value, void* stream);
/* src: device [C][Z][Y][X] uint8 (canonical).  Plane c is written in the file's voxel order (i fastest, ni * nj * nk == Z * Y * X < 2^31) at
 * dst + dst_offset + c * plane_stride: file voxel (i, j, k) = src plane element coff + i * ci + j * cj + k * ck.  dst holds dst_bytes bytes; the
 * bytes in front of and between the planes (file headers) are left as they are.  One launch.  A plane that leaves dst, strides that leave the
 * source plane, overlapping buffers, C outside 1..65535 -> RSUPER_ERR_ARG. */
int rsuper_reorient_store(const uint8_t* src, int C, int Z, int Y, int X, uint8_t* dst, long dst_bytes, long dst_offset, long plane_stride, int ni,
                          int nj, int nk, long ci, long cj, long ck, long coff, void* stream);

/* ------------------------------------------------------------------------------------------------
 * NIfTI CT + mask files -> a packed training case -- dataset_conversion/abdomenatlas_3d.py ResampleImage :59-103, process_case_bdmap_format :106,
 * process_case_nnunet_format :150; dataset_conversion/nii2npz.py process_file :32-86.  csrc/nii_dataset.hip; the image goes through
 * rsuper_nifti_load_prefilter / rsuper_bspline_resample / rsuper_ct_stats / rsuper_ct_normalize_pop.
 * ------------------------------------------------------------------------------------------------ */
#define RSUPER_LABEL_DESC_WORDS 8
/* One output byte plane (up to eight classes) of a bit-packed label, gathered from the mask files' own voxel buffers.
 * raw: device, raw_bytes bytes, 4-byte aligned: the voxel buffers of the group's files.  desc: device [nclass][RSUPER_LABEL_DESC_WORDS] int64, per class
 * {element offset of its buffer in raw (in elements of its dtype), RSUPER_NII_* integer dtype (U8 .. I32), sz, sy, sx, base, elements of the buffer,
 * absent}: canonical voxel (z, y, x) of the class is element base + z * sz + y * sy + x * sx of its buffer (nifti.canonical_layout; a flipped axis has
 * a negative stride); absent != 0, an unknown or float dtype, a buffer that leaves raw or an element index outside the buffer read as 0.
 * ix [Xb], iy [Yb], iz [Zb]: device int32, the nearest source index of every voxel of the resampled box on each axis (canonical source size Z, Y, X);
 * an entry below 0 or at or above the axis is outside the scan.
 * lut == NULL: 1 <= nclass <= 8, P == 1; dst [Do][Ho][Wo] u8 (any alignment) = OR_k (voxel of class k != 0) << (7 - k) inside the box
 * (zo, yo, xo) + (Zb, Yb, Xb) and 0 in the padding around it: every byte of the plane is written, none beyond it, no memset is needed.
 * lut != NULL (label-map mode): nclass == 1, lut device [n_values][P] u8, 1 <= P <= 8; dst [P][Do][Ho][Wo], byte of plane p = lut[value][p], a value
 * below 0 or at or above n_values gives 0.  One launch.  Do * Ho * Wo < 2^31.  Null or misaligned pointers, non-positive sizes, a box outside the
 * output, dst overlapping raw, nclass / P out of range -> RSUPER_ERR_ARG, checked before anything is launched. */
int rsuper_label_gather_pack(const void* raw, long raw_bytes, const long long* desc, int nclass, const uint8_t* lut, int n_values, int P, const int* ix,
                             const int* iy, const int* iz, int Z, int Y, int X, int Zb, int Yb, int Xb, uint8_t* dst, int Do, int Ho, int Wo, int zo, int yo,
                             int xo, void* stream);
/* packed: device [P][Do][Ho][Wo] u8 bit-packed (class c = bit 7 - (c & 7) of plane c >> 3), 1 <= P <= 8.  Inside the box (zo, yo, xo) + (Zb, Yb, Xb) the
 * bit of class bg_class becomes (number of OTHER classes set at the voxel) != 1 -- nii2npz.py :58-60 (1 - sum) followed by the dataset's astype(bool):
 * set where no class is and where two or more overlap.  Outside the box nothing is touched.  One launch. */
int rsuper_label_background(uint8_t* packed, int P, int bg_class, int Do, int Ho, int Wo, int zo, int yo, int xo, int Zb, int Yb, int Xb, void* stream);

#ifdef __cplusplus
}
#endif
#endif
