// Multi-task / CLIP baselines: the tail of MedFormer's ClassificationBranch in one workgroup per sample, and the two losses that consume it.
//
// Tail (rsuper_train/model/dim3/medformer.py:65-75 with trans_layers.py:79-118): on the L = (d/2)(h/2)(w/2) tokens of one sample,
//   x0 = reducer(x)            (L,160) -> (L,64)      Conv3d(160, 64, 1) with bias
//   x1 = x0 + to_out(attention(to_qkv(LN1(x0))))      4 heads x 16, soft-max over the L tokens, scale 16^-0.5
//   x2 = x1 + fc2(gelu(fc1(LN2(x1))))                 64 -> 320 -> 64, exact erf GELU, LayerNorm eps 1e-5
//   out = head(mean over tokens of x2)                64 -> Nc, Nc looped (1..768)
// The unfused path runs this as about twenty launches on operands of at most 64 x 320 floats.  Here: forward = 1 launch (grid B), backward = 1
// launch (grid B) that writes d x and the per-sample partial gradient of every parameter + 1 launch that adds the partials in sample order.
// No float atomics, every sum in a fixed order: two runs give the same bits.  All arithmetic f32 (the attention stages of MedFormer are f32).
//
// Saved, not recomputed: the forward writes every activation the backward reads (x0's LayerNorm'ed values and rstd, qkv, the soft-max rows,
// the attention output, x1, fc1's output before and after GELU, the token mean) into a per-sample workspace of rsuper_cls_tail_save_floats(L)
// floats -- 410 KB at L = 64, L2 resident -- because the backward's LDS is taken by the operands of the GEMM it is in (map below).
// The weights (116 k floats at Nc = 3) are streamed from L2: a lane owns one output column and walks its weight row in 16-byte loads while the
// activation rows come from LDS as broadcasts (forward, mode `gemm`); the data gradients walk the weight rows across the lanes (coalesced).
//
// LDS map (floats; L <= 64, dynamic, above 64 KiB it is requested with hipFuncSetAttribute):
//   forward   A [L][320]  x (stride 160) -> LN1 out (64) -> attention out (64) -> gelu(fc1) (320)
//             B [L][193]  qkv, padded rows (lane = token reads of k and v: stride 193 = 1 mod 32 banks) -> LN2 out (stride 64)
//             C [L][64]   x0 -> x1 -> x2 (residual stream, updated in place)
//   backward  A [L][320]  gelu(fc1) -> d fc1 (320) | d scores [4][L][L] | d LN1 out (64) | x (stride 160)
//             B [L][65]   LN2 out -> attention out -> v (padded) ...  (stride 64 except v)
//             C [L][64]   d LN2 out -> d attention out -> LN1 out
//             G [L][64]   gradient of the residual stream: d x2 -> d x1 -> d x0
#include <stdio.h>
#include "common.hpp"
#include "../../include/rsuper_hip.h"

namespace {

constexpr int CT_NT = 512, CT_NW = CT_NT / 64;
constexpr int CIN = 160, DM = 64, NH = 4, DH = 16, QKV = 3 * DM, HID = 320, MAXL = 64, MAXNC = 768;
constexpr int QS = QKV + 1;          // padded qkv row (forward)
constexpr int VS = DM + 1;           // padded v row (backward)
constexpr float LN_EPS = 1e-5f;

struct ClsW { const float *Wr, *br, *g1, *be1, *Wqkv, *Wo, *bo, *g2, *be2, *W1, *b1, *W2, *b2, *Wh, *bh; };
constexpr int CLS_NW = 15;
static_assert(sizeof(ClsW) == CLS_NW * sizeof(const float*), "ClsW is the 15 weight pointers in the order of include/rsuper_hip.h, nothing else");

// offsets of the parameters in the flat gradient vector (same order as ClsW)
constexpr int O_WR = 0, O_BR = O_WR + DM * CIN, O_G1 = O_BR + DM, O_BE1 = O_G1 + DM, O_WQKV = O_BE1 + DM, O_WO = O_WQKV + QKV * DM,
              O_BO = O_WO + DM * DM, O_G2 = O_BO + DM, O_BE2 = O_G2 + DM, O_W1 = O_BE2 + DM, O_B1 = O_W1 + HID * DM, O_W2 = O_B1 + HID,
              O_B2 = O_W2 + DM * HID, O_WH = O_B2 + DM;
__host__ __device__ inline long param_floats(int Nc) { return (long)O_WH + (long)Nc * DM + Nc; }
__host__ __device__ inline long part_stride(int Nc) { return (param_floats(Nc) + 3) & ~3L; }      // per-sample partials start 16-byte aligned

// per-sample workspace (floats)
struct SaveOff { long xh1, rs1, qkv, p, o, x1, xh2, rs2, h1, a, m, dqkv, total; };
__host__ __device__ inline SaveOff save_off(int L) {
    SaveOff s;
    long o = 0;
    s.xh1 = o; o += (long)L * DM;
    s.rs1 = o; o += (L + 3) & ~3;
    s.qkv = o; o += (long)L * QKV;
    s.p = o; o += ((long)NH * L * L + 3) & ~3L;
    s.o = o; o += (long)L * DM;
    s.x1 = o; o += (long)L * DM;
    s.xh2 = o; o += (long)L * DM;
    s.rs2 = o; o += (L + 3) & ~3;
    s.h1 = o; o += (long)L * HID;
    s.a = o; o += (long)L * HID;
    s.m = o; o += DM;
    s.dqkv = o; o += (long)L * QKV;
    s.total = o;
    return s;
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_d(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

constexpr int LT = 4;      // token rows per work item of the GEMM helpers
constexpr int KC = 32;     // weights of one work item are fetched KC at a time (eight 16-byte loads in flight per lane: the streams come from L2)

// y[l][n] = bias[n] + sum_k in[l * si + k] * W[n * K + k] for l < L, n < N; K % KC == 0, in 16-byte aligned rows.  A lane owns column n of LT rows;
// `st(l, n, v)` stores.  in: LDS (all lanes of a column group read the same address: broadcast).
template <class St>
__device__ __forceinline__ void gemm(const float* in, int si, const float* __restrict__ W, const float* __restrict__ bias, int L, int K, int N, St st) {
    const int groups = (L + LT - 1) / LT;
    for (int it = threadIdx.x; it < N * groups; it += CT_NT) {
        const int n = it % N, l0 = (it / N) * LT;
        float acc[LT];
        const float b = bias ? bias[n] : 0.f;
#pragma unroll
        for (int t = 0; t < LT; ++t) acc[t] = b;
        const float* w = W + (size_t)n * K;
#pragma unroll 1
        for (int k0 = 0; k0 < K; k0 += KC) {
            float4 wv[KC / 4];
#pragma unroll
            for (int c = 0; c < KC / 4; ++c) wv[c] = *(const float4*)(w + k0 + 4 * c);
#pragma unroll
            for (int c = 0; c < KC / 4; ++c) {
#pragma unroll
                for (int t = 0; t < LT; ++t) {
                    const int l = l0 + t < L ? l0 + t : L - 1;
                    const float4 xv = *(const float4*)(in + l * si + k0 + 4 * c);
                    acc[t] = fmaf(xv.x, wv[c].x, acc[t]); acc[t] = fmaf(xv.y, wv[c].y, acc[t]);
                    acc[t] = fmaf(xv.z, wv[c].z, acc[t]); acc[t] = fmaf(xv.w, wv[c].w, acc[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < LT; ++t)
            if (l0 + t < L) st(l0 + t, n, acc[t]);
    }
}

// data gradient: dx[l][k] = sum_n g[l * sg + n] * W[n * K + k] for l < L, k < K; a lane owns column k (W rows read across the lanes), n ascending.
template <class St>
__device__ __forceinline__ void dgrad(const float* g, int sg, const float* __restrict__ W, int L, int K, int N, St st) {
    const int groups = (L + LT - 1) / LT;
    for (int it = threadIdx.x; it < K * groups; it += CT_NT) {
        const int k = it % K, l0 = (it / K) * LT;
        float acc[LT];
#pragma unroll
        for (int t = 0; t < LT; ++t) acc[t] = 0.f;
#pragma unroll 1
        for (int n0 = 0; n0 < N; n0 += 8) {          // N % 8 == 0; eight weight rows in flight per lane
            float wv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) wv[c] = W[(size_t)(n0 + c) * K + k];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
#pragma unroll
                for (int t = 0; t < LT; ++t) {
                    const int l = l0 + t < L ? l0 + t : L - 1;
                    acc[t] = fmaf(g[l * sg + n0 + c], wv[c], acc[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < LT; ++t)
            if (l0 + t < L) st(l0 + t, k, acc[t]);
    }
}

// weight gradient of one sample: dW[n * K + k] = sum_l g[l * sg + n] * a[l * sa + k], l ascending; a lane owns 4 consecutive k of one n (K % 4 == 0).
__device__ __forceinline__ void wgrad(const float* g, int sg, const float* a, int sa, int L, int K, int N, float* __restrict__ dW) {
    const int k4 = K / 4;
    for (int it = threadIdx.x; it < N * k4; it += CT_NT) {
        const int n = it / k4, k = (it % k4) * 4;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int l = 0; l < L; ++l) {
            const float gv = g[l * sg + n];
            const float4 av = *(const float4*)(a + l * sa + k);
            acc.x = fmaf(gv, av.x, acc.x); acc.y = fmaf(gv, av.y, acc.y); acc.z = fmaf(gv, av.z, acc.z); acc.w = fmaf(gv, av.w, acc.w);
        }
        *(float4*)(dW + (size_t)n * K + k) = acc;
    }
}

// column sums: db[n] = sum_l g[l * sg + n], l ascending
__device__ __forceinline__ void colsum(const float* g, int sg, int L, int N, float* __restrict__ db) {
    for (int n = threadIdx.x; n < N; n += CT_NT) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) s += g[l * sg + n];
        db[n] = s;
    }
}

// LayerNorm over the 64 channels of every row of src (stride 64): a wave per row, lane = channel.  xh, rs: saved; dst = xh * gamma + beta.
__device__ __forceinline__ void layernorm(const float* src, const float* __restrict__ gamma, const float* __restrict__ beta, int L, float* __restrict__ xh,
                                          float* __restrict__ rs, float* dst, int sd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float gm = gamma[lane], bt = beta[lane];
    for (int l = wave; l < L; l += CT_NW) {
        const float v = src[l * DM + lane];
        const float mean = wsum(v) * (1.f / DM);
        const float d = v - mean;
        const float r = rsqrtf(wsum(d * d) * (1.f / DM) + LN_EPS);
        const float h = d * r;
        xh[l * DM + lane] = h;
        if (lane == 0) rs[l] = r;
        dst[l * sd + lane] = fmaf(h, gm, bt);
    }
}

// LayerNorm backward: G[l][c] += rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)), dxh = dy * gamma
__device__ __forceinline__ void layernorm_bwd(const float* dy, const float* __restrict__ xh, const float* __restrict__ rs, const float* __restrict__ gamma, int L,
                                              float* G) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float gm = gamma[lane];
    for (int l = wave; l < L; l += CT_NW) {
        const float h = xh[l * DM + lane];
        const float dh = dy[l * DM + lane] * gm;
        const float m1 = wsum(dh) * (1.f / DM), m2 = wsum(dh * h) * (1.f / DM);
        G[l * DM + lane] += rs[l] * (dh - m1 - h * m2);
    }
}

// d gamma[c] = sum_l dy[l][c] * xh[l][c], d beta[c] = sum_l dy[l][c]
__device__ __forceinline__ void layernorm_wgrad(const float* dy, const float* __restrict__ xh, int L, float* __restrict__ dg, float* __restrict__ db) {
    for (int c = threadIdx.x; c < DM; c += CT_NT) {
        float sg = 0.f, sb = 0.f;
        for (int l = 0; l < L; ++l) {
            const float d = dy[l * DM + c];
            sg = fmaf(d, xh[l * DM + c], sg);
            sb += d;
        }
        dg[c] = sg; db[c] = sb;
    }
}

__global__ __launch_bounds__(CT_NT) void cls_tail_fwd_kernel(const float* __restrict__ x, ClsW w, float* __restrict__ out, float* __restrict__ save, int L, int Nc) {
    extern __shared__ float sm[];
    float* A = sm;                       // [L][320]
    float* Bq = A + L * HID;             // [L][193]
    float* C = Bq + ((L * QS + 3) & ~3);  // [L][64]
    float* M = C + L * DM;               // [64]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SaveOff so = save_off(L);
    float* sv = save + (size_t)b * so.total;
    const float* xb = x + (size_t)b * L * CIN;
    for (int e = tid * 4; e < L * CIN; e += CT_NT * 4) *(float4*)(A + e) = *(const float4*)(xb + e);
    __syncthreads();
    gemm(A, CIN, w.Wr, w.br, L, CIN, DM, [&](int l, int n, float v) { C[l * DM + n] = v; });
    __syncthreads();
    layernorm(C, w.g1, w.be1, L, sv + so.xh1, sv + so.rs1, A, DM);
    __syncthreads();
    gemm(A, DM, w.Wqkv, nullptr, L, DM, QKV, [&](int l, int n, float v) { Bq[l * QS + n] = v; sv[so.qkv + l * QKV + n] = v; });
    __syncthreads();
    // attention: a wave per (head, query row); lane = key token for the scores, lane = (part, d) for the mix
    for (int r = wave; r < NH * L; r += CT_NW) {
        const int h = r / L, i = r % L;
        const int j = lane < L ? lane : L - 1;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) s = fmaf(Bq[i * QS + h * DH + d], Bq[j * QS + DM + h * DH + d], s);
        s = lane < L ? s * 0.25f : -INFINITY;
        const float mx = wmax(s);
        const float e = lane < L ? expf(s - mx) : 0.f;
        const float p = e / wsum(e);
        if (lane < L) sv[so.p + ((size_t)h * L + i) * L + lane] = p;
        const int d = lane & 15, part = lane >> 4;
        float o = 0.f;
        for (int jj = part * 16; jj < part * 16 + 16; ++jj) {
            const float pj = __shfl(p, jj);
            if (jj < L) o = fmaf(pj, Bq[jj * QS + 2 * DM + h * DH + d], o);
        }
        o += __shfl_xor(o, 16);
        o += __shfl_xor(o, 32);
        if (lane < DH) { A[i * DM + h * DH + lane] = o; sv[so.o + i * DM + h * DH + lane] = o; }
    }
    __syncthreads();
    gemm(A, DM, w.Wo, w.bo, L, DM, DM, [&](int l, int n, float v) { const float y = v + C[l * DM + n]; C[l * DM + n] = y; sv[so.x1 + l * DM + n] = y; });
    __syncthreads();
    layernorm(C, w.g2, w.be2, L, sv + so.xh2, sv + so.rs2, Bq, DM);
    __syncthreads();
    gemm(Bq, DM, w.W1, w.b1, L, DM, HID, [&](int l, int n, float v) { sv[so.h1 + l * HID + n] = v; const float a = gelu_f(v); A[l * HID + n] = a; sv[so.a + l * HID + n] = a; });
    __syncthreads();
    gemm(A, HID, w.W2, w.b2, L, HID, DM, [&](int l, int n, float v) { C[l * DM + n] += v; });
    __syncthreads();
    if (tid < DM) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) s += C[l * DM + tid];
        s /= (float)L;
        M[tid] = s; sv[so.m + tid] = s;
    }
    __syncthreads();
    for (int n = tid; n < Nc; n += CT_NT) {
        float acc = w.bh[n];
        const float* wr = w.Wh + (size_t)n * DM;
        for (int c = 0; c < DM; c += 4) {
            const float4 wv = *(const float4*)(wr + c);
            acc = fmaf(M[c], wv.x, acc); acc = fmaf(M[c + 1], wv.y, acc); acc = fmaf(M[c + 2], wv.z, acc); acc = fmaf(M[c + 3], wv.w, acc);
        }
        out[(size_t)b * Nc + n] = acc;
    }
}

__global__ __launch_bounds__(CT_NT) void cls_tail_bwd_kernel(const float* __restrict__ x, ClsW w, const float* __restrict__ dout, float* __restrict__ save,
                                                             float* __restrict__ dx, float* __restrict__ part, int L, int Nc) {
    extern __shared__ float sm[];
    float* A = sm;                       // [L][320]
    float* Bv = A + L * HID;             // [L][65]
    float* C = Bv + ((L * VS + 3) & ~3);  // [L][64]
    float* G = C + L * DM;               // [L][64]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SaveOff so = save_off(L);
    float* sv = save + (size_t)b * so.total;
    float* pg = part + (size_t)b * part_stride(Nc);
    const float* dob = dout + (size_t)b * Nc;
    // head: dWh = dout (x) m, dbh = dout; d m = Wh^T dout; d x2[l] = d m / L
    for (int e = tid; e < Nc * DM; e += CT_NT) pg[O_WH + e] = dob[e / DM] * sv[so.m + (e % DM)];
    for (int n = tid; n < Nc; n += CT_NT) pg[O_WH + (size_t)Nc * DM + n] = dob[n];
    if (tid < DM) {
        float s = 0.f;
        for (int n = 0; n < Nc; ++n) s = fmaf(dob[n], w.Wh[(size_t)n * DM + tid], s);
        s /= (float)L;
        for (int l = 0; l < L; ++l) G[l * DM + tid] = s;
    }
    for (int e = tid * 4; e < L * HID; e += CT_NT * 4) *(float4*)(A + e) = *(const float4*)(sv + so.a + e);
    __syncthreads();
    // fc2: dW2 = G^T a, db2 = colsum G, then A = (G W2) * gelu'(h1)
    wgrad(G, DM, A, HID, L, HID, DM, pg + O_W2);
    colsum(G, DM, L, DM, pg + O_B2);
    __syncthreads();
    dgrad(G, DM, w.W2, L, HID, DM, [&](int l, int k, float v) { A[l * HID + k] = v * gelu_d(sv[so.h1 + l * HID + k]); });
    // LN2 output again: Bv (stride 64) = xh2 * g2 + be2
    for (int e = tid; e < L * DM; e += CT_NT) Bv[e] = fmaf(sv[so.xh2 + e], w.g2[e % DM], w.be2[e % DM]);
    __syncthreads();
    // fc1: dW1 = A^T n2, db1 = colsum A, C = A W1
    wgrad(A, HID, Bv, DM, L, DM, HID, pg + O_W1);
    colsum(A, HID, L, HID, pg + O_B1);
    dgrad(A, HID, w.W1, L, DM, HID, [&](int l, int k, float v) { C[l * DM + k] = v; });
    __syncthreads();
    layernorm_wgrad(C, sv + so.xh2, L, pg + O_G2, pg + O_BE2);
    layernorm_bwd(C, sv + so.xh2, sv + so.rs2, w.g2, L, G);          // G = d x1
    for (int e = tid; e < L * DM; e += CT_NT) Bv[e] = sv[so.o + e];   // attention output (Bv's LN2 values are no longer read: wgrad above is behind the barrier)
    __syncthreads();
    // to_out: dWo = G^T o, dbo = colsum G, C = G Wo (d attention output)
    wgrad(G, DM, Bv, DM, L, DM, DM, pg + O_WO);
    colsum(G, DM, L, DM, pg + O_BO);
    dgrad(G, DM, w.Wo, L, DM, DM, [&](int l, int k, float v) { C[l * DM + k] = v; });
    __syncthreads();
    for (int e = tid; e < L * DM; e += CT_NT) Bv[(e / DM) * VS + (e % DM)] = sv[so.qkv + (e / DM) * QKV + 2 * DM + (e % DM)];     // v, padded rows
    __syncthreads();
    // d scores: a wave per (head, query row), lane = key token; A = dS [4][L][L]
    for (int r = wave; r < NH * L; r += CT_NW) {
        const int h = r / L, i = r % L;
        const int j = lane < L ? lane : L - 1;
        float dp = 0.f;
#pragma unroll
        for (int d = 0; d < DH; ++d) dp = fmaf(C[i * DM + h * DH + d], Bv[j * VS + h * DH + d], dp);
        const float p = lane < L ? sv[so.p + ((size_t)h * L + i) * L + j] : 0.f;
        const float t = wsum(p * dp);
        if (lane < L) A[(h * L + i) * L + lane] = p * (dp - t) * 0.25f;
    }
    __syncthreads();
    // dq[l][c] = sum_j dS[h][l][j] k[j][c];  dk[l][c] = sum_i dS[h][i][l] q[i][c];  dv[l][c] = sum_i P[h][i][l] dO[i][c]
    for (int it = tid; it < L * DM; it += CT_NT) {
        const int l = it / DM, c = it % DM, h = c / DH;
        float dq = 0.f, dk = 0.f, dv = 0.f;
#pragma unroll 4
        for (int j = 0; j < L; ++j) {
            dq = fmaf(A[(h * L + l) * L + j], sv[so.qkv + j * QKV + DM + c], dq);
            dk = fmaf(A[(h * L + j) * L + l], sv[so.qkv + j * QKV + c], dk);
            dv = fmaf(sv[so.p + ((size_t)h * L + j) * L + l], C[j * DM + c], dv);
        }
        sv[so.dqkv + l * QKV + c] = dq; sv[so.dqkv + l * QKV + DM + c] = dk; sv[so.dqkv + l * QKV + 2 * DM + c] = dv;
    }
    __syncthreads();
    // LN1 output again: C = xh1 * g1 + be1 (d attention output is consumed)
    for (int e = tid; e < L * DM; e += CT_NT) C[e] = fmaf(sv[so.xh1 + e], w.g1[e % DM], w.be1[e % DM]);
    __syncthreads();
    // to_qkv: dWqkv = dqkv^T n1, A[0 : L*64] = dqkv Wqkv (d LN1 output); dqkv is read from the workspace (uniform addresses per wave)
    wgrad(sv + so.dqkv, QKV, C, DM, L, DM, QKV, pg + O_WQKV);
    dgrad(sv + so.dqkv, QKV, w.Wqkv, L, DM, QKV, [&](int l, int k, float v) { A[l * DM + k] = v; });
    __syncthreads();
    layernorm_wgrad(A, sv + so.xh1, L, pg + O_G1, pg + O_BE1);
    layernorm_bwd(A, sv + so.xh1, sv + so.rs1, w.g1, L, G);          // G = d x0
    __syncthreads();
    // reducer: dWr = G^T x, dbr = colsum G, dx = G Wr
    const float* xb = x + (size_t)b * L * CIN;
    for (int e = tid * 4; e < L * CIN; e += CT_NT * 4) *(float4*)(A + e) = *(const float4*)(xb + e);
    __syncthreads();
    wgrad(G, DM, A, CIN, L, CIN, DM, pg + O_WR);
    colsum(G, DM, L, DM, pg + O_BR);
    float* dxb = dx + (size_t)b * L * CIN;
    dgrad(G, DM, w.Wr, L, CIN, DM, [&](int l, int k, float v) { dxb[l * CIN + k] = v; });
}

// grads[e] = sum_b part[b][e], b ascending
__global__ __launch_bounds__(256) void cls_tail_reduce_kernel(const float* __restrict__ part, float* __restrict__ grads, long n, long stride, int B) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        float s = part[e];
        for (int b = 1; b < B; ++b) s += part[(size_t)b * stride + e];
        grads[e] = s;
    }
}

size_t fwd_smem(int L) { return sizeof(float) * ((size_t)L * HID + (((size_t)L * QS + 3) & ~(size_t)3) + (size_t)L * DM + DM); }
size_t bwd_smem(int L) { return sizeof(float) * ((size_t)L * HID + (((size_t)L * VS + 3) & ~(size_t)3) + 2 * (size_t)L * DM); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int load_weights(const void* const* weights, ClsW& w) {
    for (int i = 0; i < CLS_NW; ++i)
        if (!weights[i] || !aligned16(weights[i])) return RS_ERR_ARG;
    auto f = [&](int i) { return (const float*)weights[i]; };
    w.Wr = f(0); w.br = f(1); w.g1 = f(2); w.be1 = f(3); w.Wqkv = f(4); w.Wo = f(5); w.bo = f(6); w.g2 = f(7); w.be2 = f(8);
    w.W1 = f(9); w.b1 = f(10); w.W2 = f(11); w.b2 = f(12); w.Wh = f(13); w.bh = f(14);
    return RS_OK;
}

// More than 64 KiB of dynamic LDS has to be requested per kernel and device: once, with the largest size the kernel takes (L = MAXL), remembered per
// device; a refusal is reported (RS_ERR_LAUNCH) instead of surfacing later as a failed launch.
int request_lds(const void* kernel, size_t bytes, size_t max_bytes, bool* done) {
    if (bytes <= 64 * 1024) return RS_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RS_ERR_LAUNCH;
    if (done[dev]) return RS_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes);
    if (e != hipSuccess) {
        fprintf(stderr, "rsuper cls_tail: %zu bytes of dynamic LDS refused (%s)\n", max_bytes, hipGetErrorString(e));
        return RS_ERR_LAUNCH;
    }
    done[dev] = true;
    return RS_OK;
}
bool g_fwd_lds[64], g_bwd_lds[64];

// ------------------------------------------------------------------------------------------------ classification loss
// One block.  Entry e = (b, j), j-th class of the set: target = label flag | mask flag; known = !(unknown flag) | target; value =
// mean over ALL B * Nc entries of weight * known * BCE-with-logits; dlogits = weight * known * (sigmoid(x) - target) / (B * Nc).  f64, fixed order.
__global__ __launch_bounds__(256) void cls_loss_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ fl, const uint8_t* __restrict__ fm,
                                                       const uint8_t* __restrict__ fu, const float* __restrict__ weights, int B, int C, int Nc,
                                                       unsigned long long set, float* __restrict__ loss, float* __restrict__ dlogits) {
    __shared__ double red[256];
    __shared__ int cls[64];
    const int tid = threadIdx.x;
    if (tid == 0) {
        int j = 0;
        for (int c = 0; c < C; ++c)
            if ((set >> c) & 1ull) cls[j++] = c;
    }
    __syncthreads();
    const int n = B * Nc;
    double s = 0.0;
    for (int e = tid; e < n; e += 256) {
        const int b = e / Nc, c = cls[e % Nc];
        const int t = ((fl && fl[b * C + c]) || (fm && fm[b * C + c])) ? 1 : 0;
        const int known = (fu && fu[b * C + c] && !t) ? 0 : 1;
        const double x = (double)logits[e], wt = weights ? (double)weights[e] : 1.0;
        const double v = fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
        const double sg = x >= 0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x));
        s += known ? wt * v : 0.0;
        dlogits[e] = known ? (float)(wt * (sg - t) / n) : 0.f;
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) loss[0] = (float)(red[0] / n);
}

// ------------------------------------------------------------------------------------------------ InfoNCE, implicit negatives
// One block, N <= 64: L2-normalise (eps 1e-12), S = qh kh^T / T, loss = mean_i (logsumexp_j S[i][j] - S[i][i]); dq, dk through the normalisation.
// f64 sums in a fixed order, every output rounded once.
constexpr int NCE_MAXN = 64, NCE_NT = 512, NCE_NW = NCE_NT / 64, NCE_KEEP = 16;
__device__ __forceinline__ double wsumd(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__global__ __launch_bounds__(NCE_NT) void info_nce_kernel(const float* __restrict__ q, const float* __restrict__ k, int N, int D, double inv_t,
                                                          float* __restrict__ loss, float* __restrict__ dq, float* __restrict__ dk) {
    __shared__ double S[NCE_MAXN * NCE_MAXN];      // logits, then dL/dS
    __shared__ double nq[NCE_MAXN], nk[NCE_MAXN], rowl[NCE_MAXN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double eps = 1e-12;
    for (int r = wave; r < 2 * N; r += NCE_NW) {
        const float* v = (r < N ? q : k) + (size_t)(r % N) * D;
        double s = 0.0;
        for (int d = lane; d < D; d += 64) s += (double)v[d] * (double)v[d];
        s = sqrt(wsumd(s));
        if (lane == 0) (r < N ? nq : nk)[r % N] = 1.0 / (s > eps ? s : eps);      // reciprocal of the clamped norm
    }
    __syncthreads();
    for (int r = wave; r < N * N; r += NCE_NW) {
        const int i = r / N, j = r % N;
        double s = 0.0;
        for (int d = lane; d < D; d += 64) s += (double)q[(size_t)i * D + d] * (double)k[(size_t)j * D + d];
        s = wsumd(s);
        if (lane == 0) S[i * NCE_MAXN + j] = s * nq[i] * nk[j] * inv_t;
    }
    __syncthreads();
    if (tid < N) {
        const int i = tid;
        double mx = S[i * NCE_MAXN];
        for (int j = 1; j < N; ++j) mx = fmax(mx, S[i * NCE_MAXN + j]);
        double se = 0.0;
        for (int j = 0; j < N; ++j) se += exp(S[i * NCE_MAXN + j] - mx);
        rowl[i] = (mx + log(se)) - S[i * NCE_MAXN + i];
        for (int j = 0; j < N; ++j) S[i * NCE_MAXN + j] = (exp(S[i * NCE_MAXN + j] - mx) / se - (i == j ? 1.0 : 0.0)) / N;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += rowl[i];
        loss[0] = (float)(s / N);
    }
    // a wave per output row: dh = sum_j G * other_hat * inv_t, then d = (dh - hat * (hat . dh)) / norm.  A lane keeps the dh of its first NCE_KEEP
    // columns (D <= 1024: all of them) in registers between the two passes; columns beyond are computed again.  A norm clamped to eps: d = dh / eps
    // (F.normalize's derivative there).
    for (int r = wave; r < 2 * N; r += NCE_NW) {
        const bool isq = r < N;
        const int i = r % N;
        const float* self = (isq ? q : k) + (size_t)i * D;
        const float* other = isq ? k : q;
        const double* ro = isq ? nk : nq;
        const double rs = (isq ? nq : nk)[i];
        float* dst = (isq ? dq : dk) + (size_t)i * D;
        auto dh_at = [&](int d) {
            double dh = 0.0;
            for (int j = 0; j < N; ++j) dh += (isq ? S[i * NCE_MAXN + j] : S[j * NCE_MAXN + i]) * ro[j] * (double)other[(size_t)j * D + d];
            return dh * inv_t;
        };
        double keep[NCE_KEEP];
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < NCE_KEEP; ++c) {
            const int d = lane + 64 * c;
            keep[c] = d < D ? dh_at(d) : 0.0;
            if (d < D) dot += keep[c] * ((double)self[d] * rs);
        }
        for (int d = lane + 64 * NCE_KEEP; d < D; d += 64) dot += dh_at(d) * ((double)self[d] * rs);
        dot = rs < 1.0 / eps ? wsumd(dot) : 0.0;
#pragma unroll
        for (int c = 0; c < NCE_KEEP; ++c) {
            const int d = lane + 64 * c;
            if (d < D) dst[d] = (float)((keep[c] - ((double)self[d] * rs) * dot) * rs);
        }
        for (int d = lane + 64 * NCE_KEEP; d < D; d += 64) dst[d] = (float)((dh_at(d) - ((double)self[d] * rs) * dot) * rs);
    }
}

}  // namespace

extern "C" {

int rsuper_cls_tail_supported(int L, int Nc) { return L >= 1 && L <= MAXL && Nc >= 1 && Nc <= MAXNC; }
long rsuper_cls_tail_save_floats(int L) { return L >= 1 && L <= MAXL ? save_off(L).total : 0; }
long rsuper_cls_tail_param_floats(int Nc) { return Nc >= 1 && Nc <= MAXNC ? param_floats(Nc) : 0; }
long rsuper_cls_tail_partial_floats(int B, int Nc) { return Nc >= 1 && Nc <= MAXNC && B >= 1 ? (long)B * part_stride(Nc) : 0; }

int rsuper_cls_tail_fwd(const float* x, const void* const* weights, float* out, float* save, int B, int L, int Nc, void* stream) {
    if (!x || !weights || !out || !save || B < 1 || !aligned16(x) || !aligned16(save)) return RS_ERR_ARG;
    if (!rsuper_cls_tail_supported(L, Nc)) return RS_ERR_UNSUPPORTED;
    ClsW w;
    if (const int rc = load_weights(weights, w)) return rc;
    const size_t smem = fwd_smem(L);
    if (const int rc = request_lds((const void*)cls_tail_fwd_kernel, smem, fwd_smem(MAXL), g_fwd_lds)) return rc;
    hipLaunchKernelGGL(cls_tail_fwd_kernel, dim3(B), dim3(CT_NT), smem, (hipStream_t)stream, x, w, out, save, L, Nc);
    return rs_check_launch();
}

int rsuper_cls_tail_bwd(const float* x, const void* const* weights, const float* dout, float* save, float* dx, float* partials, float* grads, int B, int L,
                        int Nc, void* stream) {
    if (!x || !weights || !dout || !save || !dx || !partials || !grads || B < 1 || !aligned16(x) || !aligned16(save) || !aligned16(partials))
        return RS_ERR_ARG;
    if (!rsuper_cls_tail_supported(L, Nc)) return RS_ERR_UNSUPPORTED;
    ClsW w;
    if (const int rc = load_weights(weights, w)) return rc;
    const size_t smem = bwd_smem(L);
    if (const int rc = request_lds((const void*)cls_tail_bwd_kernel, smem, bwd_smem(MAXL), g_bwd_lds)) return rc;
    hipLaunchKernelGGL(cls_tail_bwd_kernel, dim3(B), dim3(CT_NT), smem, (hipStream_t)stream, x, w, dout, save, dx, partials, L, Nc);
    if (rs_check_launch() != RS_OK) return RS_ERR_LAUNCH;
    const long n = param_floats(Nc);
    hipLaunchKernelGGL(cls_tail_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)partials, grads, n, part_stride(Nc), B);
    return rs_check_launch();
}

int rsuper_cls_loss(const float* logits, const uint8_t* flags_label, const uint8_t* flags_mask, const uint8_t* flags_unk, const float* weights, int B, int C,
                    int Nc, unsigned long long class_set, float* loss, float* dlogits, void* stream) {
    if (!logits || !loss || !dlogits || B < 1 || C < 1 || C > 64 || Nc < 1 || (long)B * Nc > (1 << 24)) return RS_ERR_ARG;
    if (C < 64 && (class_set >> C)) return RS_ERR_ARG;
    if (__builtin_popcountll(class_set) != Nc) return RS_ERR_ARG;
    hipLaunchKernelGGL(cls_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, flags_label, flags_mask, flags_unk, weights, B, C, Nc, class_set,
                       loss, dlogits);
    return rs_check_launch();
}

int rsuper_info_nce_supported(int N, int D) { return N >= 1 && N <= NCE_MAXN && D >= 1; }

int rsuper_info_nce(const float* query, const float* key, int N, int D, double temperature, float* loss, float* dquery, float* dkey, void* stream) {
    if (!query || !key || !loss || !dquery || !dkey || !(temperature > 0.0)) return RS_ERR_ARG;
    if (!rsuper_info_nce_supported(N, D)) return RS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(info_nce_kernel, dim3(1), dim3(NCE_NT), 0, (hipStream_t)stream, query, key, N, D, 1.0 / temperature, loss, dquery, dkey);
    return rs_check_launch();
}

}  // extern "C"
