// The one place that fills the launch descriptors of common.h (GemmArgs, GemmArgs::GnIn, AttnArgs). They reach the kernels by value and gemm_kernel.h reads GemmArgs at
// fixed kernarg offsets, so the structs stay plain aggregates and every descriptor starts here: zeroed, then the fields of its kind. What a site adds on top -- K split,
// statistics outputs, prefetch, epilogue scales -- it writes itself. Needs common.h only (qxattn.hip builds its context tiles with it); `zero`: the caller's zero_page().
#pragma once

#include <cstring>

#include "common.h"

// C [M, ldc] = epilogue(A [M, lda] . W [N, ldw]^T): bias, residual [M, ldr], GEGLU, activation; rpb / bstride / roff: the linear row map (rpb == 0: identity).
// Tile order: consecutive workgroups walk M when M <= N (the fused QKV tile's descriptor keeps 0: qkv_desc).
inline GemmArgs gemm_desc(const half_t* zero, const half_t* A, int lda, const half_t* W, int ldw, const half_t* bias, const half_t* residual, int ldr, half_t* C, int ldc,
                          int M, int N, int K, int geglu = 0, int rpb = 0, int bstride = 0, int roff = 0, int act = 0) {
  GemmArgs a;
  memset(&a, 0, sizeof a);
  a.pad = 1;
  a.A = A; a.W = W; a.C = C; a.zero = zero; a.M = M; a.N = N; a.K = K; a.ldw = ldw; a.lda = lda; a.ldc = ldc;
  a.rpb = rpb; a.bstride = bstride; a.roff = roff; a.bias = bias; a.residual = residual; a.ldr = ldr; a.geglu = geglu; a.act = act;
  a.rows_per_batch = 1;
  a.m_fastest = M <= N ? 1 : 0;
  a.acc_scale = a.bias_scale = 1.f;
  return a;
}
// the stacked Q | K | V projection [M, C3] of the fused QKV + self-attention launch (qxattn.hip): O is the only output
inline GemmArgs qkv_desc(const half_t* zero, const half_t* A, int lda, const half_t* W, const half_t* bias, int M, int C3, int K) {
  GemmArgs a = gemm_desc(zero, A, lda, W, K, bias, nullptr, 0, nullptr, C3, M, C3, K);
  a.m_fastest = 0;
  return a;
}
// 3x3 convolution as an implicit GEMM, channels-last: X [B, Hs, Ws, Cin] (up = 1: its nearest-x2 upsampled view) -> Y [B, Ho, Wo, Co]; pad_lo zero rows / columns before
// the image, one after it in every mode; X2 / X3: appended 1x1 blocks of Cin2 / Cin3 channels (K = 9 Cin + Cin2 + Cin3); rowvec: a per-image vector; residual [M, Co]
inline GemmArgs conv3_desc(const half_t* zero, const half_t* X, int B, int Hs, int Ws, int Cin, const half_t* W, const half_t* bias, int Co, int stride, int up, int pad_lo,
                           const half_t* rowvec, int rowvec_ld, const half_t* residual, half_t* Y, const half_t* X2 = nullptr, int Cin2 = 0, const half_t* X3 = nullptr, int Cin3 = 0) {
  GemmArgs a;
  memset(&a, 0, sizeof a);
  a.pad = pad_lo;
  const int Hv = Hs << up, Wv = Ws << up;
  a.Ho = (Hv + pad_lo + 1 - 3) / stride + 1; a.Wo = (Wv + pad_lo + 1 - 3) / stride + 1;
  a.A = X; a.W = W; a.C = Y; a.zero = zero; a.M = B * a.Ho * a.Wo; a.N = Co; a.K = 9 * Cin + Cin2 + Cin3; a.ldw = a.K; a.lda = Cin; a.ldc = Co;
  a.A2 = X2; a.lda2 = Cin2; a.Cin2 = Cin2;
  a.A3 = X3; a.lda3 = Cin3; a.Cin3 = Cin3;
  a.Hs = Hs; a.Ws = Ws; a.stride = stride; a.up = up; a.Cin = Cin;
  a.bias = bias; a.rowvec = rowvec; a.rowvec_ld = rowvec_ld; a.rows_per_batch = a.Ho * a.Wo; a.residual = residual; a.ldr = Co;
  a.acc_scale = a.bias_scale = 1.f;
  return a;
}
// GroupNorm operand of a fused convolution / of gn_apply_stats_kernel: C channels in `groups` groups, the first C0 of them with the column sums st0 (rows0 rows per slot),
// the rest with st1 (nullptr: one source)
inline GemmArgs::GnIn gn_in_desc(const double* st0, int rows0, const double* st1, int rows1, int C0, int C, const half_t* gamma, const half_t* beta, int groups, float eps, int silu) {
  GemmArgs::GnIn g;
  memset(&g, 0, sizeof g);
  g.st0 = st0; g.rows0 = rows0; g.st1 = st1; g.rows1 = rows1; g.C0 = C0; g.gamma = gamma; g.beta = beta;
  g.groups = groups; g.gs = C / groups; g.eps = eps; g.silu = silu;
  return g;
}
// attention over heads of 64 channels: softmax(Q K^T / sqrt(64)) V per key segment, O += weight * that
inline AttnArgs attn_desc(const half_t* Q, int ldq, half_t* O, int ldo, int B, int heads, int Nq, int nseg, const AttnSeg& s0, const AttnSeg& s1 = AttnSeg{}) {
  AttnArgs a;
  memset(&a, 0, sizeof a);
  a.Q = Q; a.ldq = ldq; a.O = O; a.ldo = ldo; a.B = B; a.heads = heads; a.Nq = Nq; a.nseg = nseg;
  a.scale_log2e = 0.125f * 1.4426950408889634f;
  a.seg[0] = s0; a.seg[1] = s1;
  return a;
}
// the attention half of the fused QKV + self-attention launch: Q, K, V stay on chip, Nq keys of weight 1
inline AttnArgs sattn_desc(half_t* O, int ldo, int B, int heads, int Nq) { return attn_desc(nullptr, 0, O, ldo, B, heads, Nq, 1, AttnSeg{nullptr, nullptr, Nq, 0, 0, 1.f}); }
