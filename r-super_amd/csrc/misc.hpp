// Launch interfaces of the HBM-bound UNet kernels (unet_misc.hip), the loss kernels (loss.hip),
// the morphology kernels (morph.hip) and the optimiser kernels (optim.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct InBwdParams {
    const void* g; int ldg;        // masked upstream gradient g = dX_hat * [x_hat > 0]
    const void* x; int ldx;        // forward input of the norm
    const float* mr;               // [N][C][2] mean, rstd
    const float* gm;               // [N][C][2] mean(g), mean(g * x_n)
    const void* add1; int lda1;    // optional extra gradient terms (residual / skip paths)
    const void* add2; int lda2;
    void* out; int ldo;
    int N, vox, C;
};

struct PoolParams {
    const void* x; int ldx;        // forward input
    void* y; int ldy;              // forward: pooled output; backward: pooled gradient (read)
    void* dx; int lddx;            // backward output
    float* part;                   // forward: partial stats [N][blocks][C][2] or nullptr
    int N, D, H, W, C;             // input dims
    const void* add; int lda;      // max-pool backward: optional second gradient of x (the skip connection's) added to every voxel
    // max-pool backward with lazy gradients: a gradient that arrives with its backward means gm is the raw data gradient g of an InstanceNorm'd
    // convolution input, and the kernel applies the InstanceNorm backward tail while reading it (both [N][C][2]; nullptr: the gradient is final)
    const float* mr_y; const float* gm_y;   // y lazy: (mean, rstd) of the pooled tensor, (mean(g), mean(g x_n))
    const float* mr_x; const float* gm_x;   // add lazy: the same of x
};

struct UpParams {
    const void* x; int ldx;        // forward input (low resolution)
    void* y; int ldy;              // forward: output; backward: output gradient (read)
    void* dx; int lddx;
    float* part;
    int N, ID, IH, IW, OD, OH, OW, C;
};

struct StemParams {
    const float* x;                // [N][D][H][W] f32 (single input channel)
    const float* w;                // (C,1,3,3,3)
    void* y; int ldy;              // forward: output; wgrad: dY (read)
    float* part;                   // forward partial stats [N][blocks][C][2]
    float* dw;                     // wgrad output (C,27) f32, pre-zeroed
    int N, D, H, W, C;
};

struct HeadParams {
    const void* x; int ldx;        // features, channels-last
    const float* w; const float* b;   // (K,C), (K)
    float* logits;                 // forward: out [N][K][vox] f32; backward: d logits (read)
    void* dx; int lddx;
    float* dw; float* db;          // pre-zeroed
    int N, vox, C, K;
};

int rs_battn_supported(int T, int dh, int heads);
int rs_battn_chunks(int L, int heads);
int rs_launch_battn(const float* fqv, const float* mqv, float* fout, float* mout, float* lse, const float* dfo, const float* dmo,
                    float* dfqv, float* dmqv, float* part, float* pms, int B, int L, int T, int heads, int dh, float scale, int bwd,
                    hipStream_t st);
int rs_launch_stats_finalize(const float* part, int N, int nblk, int C, double cnt, float eps, int mode, int split, float* out, hipStream_t st);
int rs_elem_blocks(size_t items);
int rs_glue_variant(int v);      // 1: tuned bandwidth-bound kernels (default), 0: the ones they replaced; other values query (defined in glue_plan.hpp)

// One launch of the bandwidth-bound "glue" family of unet_misc.hip, as glue_plan.hpp decides it and the launchers below carry it out: the launchers
// switch over `kernel` and look at no shape, limit or environment variable themselves.  rsuper_glue_plan hands the same fields to tests.
enum GlueOp { GLUE_OP_IN_BWD, GLUE_OP_POOL_FWD, GLUE_OP_POOL_BWD, GLUE_OP_SUB_FWD, GLUE_OP_SUB_BWD, GLUE_OP_UP_FWD, GLUE_OP_UP_BWD, GLUE_OP_STEM_FWD };
enum GlueKernel {                // one value per __global__ of the family; GLUE_NONE: the launch answers RS_ERR_UNSUPPORTED
    GLUE_NONE = -1, GLUE_IN_BWD, GLUE_IN_BWD2, GLUE_POOL_FWD, GLUE_POOL_FWD2, GLUE_POOL_BWD, GLUE_SUB_FWD, GLUE_SUB_BWD,
    GLUE_UP_FWD, GLUE_UP_FWD2, GLUE_UP_FWD3, GLUE_UP_BWD, GLUE_UP_BWD2, GLUE_UP_BWD4
};
struct GluePlan {
    int kernel;                  // GlueKernel
    int sel;                     // template selector: U of in_bwd_finalize2 (2, 4), NT of upsample_bwd4 (4, 6); 0 elsewhere
    int bx, by, bz, threads;     // grid and workgroup
    int lds;                     // dynamic LDS bytes
    int rows;                    // rows of `part` the kernel writes per sample (= bx), 0: none
    int dtype;
    int arg;                     // the kernel argument that goes with the grid: cv_shift of in_bwd_finalize2, nbx of upsample_bwd4
};
int rs_stat_rows(int op, long vox);      // rows of `part` of a statistics-row forward (GlueOp; vox: output voxels per sample), 0: the op writes none
int rs_launch_in_bwd(const InBwdParams& p, const GluePlan& pl, hipStream_t st);
int rs_launch_pool(const PoolParams& p, const GluePlan& pl, hipStream_t st);
int rs_launch_subsample(const PoolParams& p, const GluePlan& pl, hipStream_t st);
// forward and the gather backward kernels; GLUE_UP_BWD4 with u, mr, gm (or nullptr): the lazy operands -- p.y is then a raw data gradient and the
// kernel applies its InstanceNorm backward tail (u the up-sampled tensor, row stride ldu; mr, gm [N][C][2])
int rs_launch_upsample(const UpParams& p, const GluePlan& pl, hipStream_t st, const void* u = nullptr, int ldu = 0, const float* mr = nullptr,
                       const float* gm = nullptr);
int rs_launch_stem(const StemParams& p, int dtype, int wgrad, hipStream_t st);
int rs_launch_head(const HeadParams& p, int dtype, int which, hipStream_t st);

// One launch of the MedFormer-stage family (pointwise.hip, depthwise.hip, instnorm.hip), as mf_plan.hpp decides it: a GluePlan whose `kernel` is an
// MfKernel.  The launchers switch over `kernel` / `sel` and look at no shape, limit or environment variable themselves; rsuper_mf_plan hands the same
// fields to tests.  sel: NF of pw_gemm (1, 2, 4), WNW of pw_wgrad (1, 2, 4), MODE of the cnorm kernels.  arg: KSPLIT of pw_gemm, rows_per of
// pw_wgrad, dsegs of depthwise_lds.  rows: rows of `part` (cnorm statistics, depthwise weight gradient), slabs of the pw_wgrad workspace.
enum MfOp {                      // one per launch; shape of rsuper_mf_plan in brackets
    MF_OP_PW_PACK, MF_OP_PW_PACK_BATCH, MF_OP_PW,                      // [K, N], [items], [R, K, N]
    MF_OP_PW_WGRAD, MF_OP_PW_WGRAD_REDUCE,                             // [R, N, K]
    MF_OP_DW, MF_OP_DW_WGRAD, MF_OP_DW_WGRAD_REDUCE,                   // [N, D, H, W, C]
    MF_OP_CNORM, MF_OP_CNORM_STATS, MF_OP_CNORM_APPLY,                 // [N, vox, C, mode]; MF_OP_CNORM: the first launch of rsuper_cnorm_forward (mode 0) / _backward (1)
    MF_OP_SE_HIDDEN, MF_OP_SE_GATE, MF_OP_SE_BWD_HIDDEN, MF_OP_SE_WGRAD, MF_OP_SE_DM,      // [N, C, r]
    MF_OP_CL_PLANAR,                                                   // [N, vox, C, K]
    MF_OP_COUNT
};
enum MfKernel {                  // one value per __global__ of the family; MF_NONE: no launch (a refused shape answers RS_ERR_UNSUPPORTED)
    MF_NONE = -1, MF_PW_PACK, MF_PW_PACK_BATCH, MF_PW_GEMM, MF_PW_WGRAD, MF_PW_WGRAD_REDUCE, MF_DW_FWD, MF_DW_LDS, MF_DW_WGRAD, MF_DW_WGRAD_REDUCE,
    MF_CNORM_STATS, MF_CNORM_APPLY, MF_CNORM_SMALL, MF_SE_HIDDEN_FWD, MF_SE_GATE_FWD, MF_SE_BWD_HIDDEN, MF_SE_WGRAD, MF_SE_DM, MF_CL_PLANAR
};
int rs_launch_cnorm_small(const float* x, const float* dy, const float* mr, float* out, float* mr_out, int N, long vox, int C, int relu, float eps, const GluePlan& pl,
                          hipStream_t st);
int rs_launch_cnorm_stats(const float* x, const float* dy, const float* mr, float* part, int N, long vox, int C, int relu, const GluePlan& pl, hipStream_t st);
int rs_launch_cnorm_apply(const float* x, const float* dy, const float* mr, const float* gm, float* out, int N, long vox, int C, int relu, const GluePlan& pl,
                          hipStream_t st);
// the excitation between the channel statistics and the affine apply of SEBlock (api.hip strings the five launches of a direction together)
int rs_launch_se_excite(const float* ms, const float* w1, const float* b1, const float* w2, const float* b2, float* hbuf, float* tab, int C, int r,
                        const GluePlan& hidden, const GluePlan& gate, hipStream_t st);
int rs_launch_se_excite_bwd(const float* gm, const float* tab, const float* hbuf, const float* ms, const float* w1, const float* w2, float* dz1buf, float* tab2,
                            float* dw1, float* db1, float* dw2, float* db2, int N, long vox, int C, int r, const GluePlan& hidden, const GluePlan& wgrad,
                            const GluePlan& dm, hipStream_t st);
int rs_launch_cl_planar(const float* src, float* dst, int N, long vox, int C, int K, int dir, const GluePlan& pl, hipStream_t st);
int rs_launch_depthwise(const float* x, const float* w, float* y, int N, int D, int H, int W, int C, int flip, const GluePlan& pl, hipStream_t st);
int rs_launch_depthwise_wgrad(const float* x, const float* dy, float* part, float* dw, int N, int D, int H, int W, int C, const GluePlan& pl,
                              const GluePlan& reduce, hipStream_t st);
