// Tile constants of the MedFormer-stage kernels (pointwise.hip, depthwise.hip, instnorm.hip) that their launch plans need too (mf_plan.hpp): what
// a block or a pass covers.  Shared so that the grids the plan computes and the walks of the kernels cannot drift apart.
#pragma once

// pointwise.hip: a packed weight set is ksteps x ntiles fragments of 64 lanes x 16 bytes (32 output channels x 16 (bf16) / 8 (f32) reduction steps)
static inline int pw_ntiles(int N) { return (N + 31) / 32; }
static inline int pw_ksteps(int K, bool f32) { const int KS = f32 ? 8 : 16; return (K + KS - 1) / KS; }

// depthwise.hip, register-run kernel and weight gradient
constexpr int DW_CG = 64;              // channels per block
constexpr int DW_VPB = 16;             // voxels per pass: 256 threads = 16 voxels x 16 channel vectors
constexpr int DW_R = 4;                // consecutive outputs along W per thread
// depthwise.hip, LDS-tiled kernel
constexpr int DL_T = 8;                                  // tile edge in H and W
constexpr int DL_C = 32;                                 // channels per block

// instnorm.hip: channels per block and voxels per pass of the statistics / apply kernels, and of the one-launch kernel
constexpr int CN_CG = 64, CN_VPB = 16;
constexpr int CS_CG = 16, CS_VPB = 64;
