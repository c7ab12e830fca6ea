// Kernels of the ViT executor (vit_engine.hip; ImageBind's vision and audio towers) on gfx950: non-causal attention over a whole short sequence at head
// dim 64 / 80, the im2col gather of a strided patch grid, the class-token / position / LayerNorm embedding row pass, and the class-row projection.
#include "common.h"

// ---- O = softmax(Q K^T / sqrt(D)) V over ALL keys of an image, from the fused QKV buffer -----------------------------------------------------------
// qkv [B*T, 3H] rows = [q | k | v], H = heads * D; out [B*T, H]. Optional bias_k / bias_v [H]: one more key / value row appended after the T token rows
// (torch nn.MultiheadAttention(add_bias_kv=True), ImageBind's audio trunk). One workgroup per (64-query tile, image x head); 4 waves of 16 queries.
// The whole K of the head (<= 272 keys) sits in LDS, then the whole V (transposed) in the same bytes: no online-softmax rescale. Scores stay in registers:
// S^T[key][query] = K Q^T per 16-key tile (v_mfma_f32_16x16x16_f16: a lane holds 4 keys of ONE query column), so a row's max / sum are a lane-local fold over
// the tiles in tile order plus two fixed shuffles (deterministic, no atomics), and the fp16 probabilities are already the B operand of O^T = V^T P^T.
// Padding keys (>= nkeys) are masked to -inf before the maximum; their K / V rows are zero-filled so that 0 x garbage never meets the accumulators.
constexpr int FA_TMAX = 272, FA_QTILE = 64;
template <int D>
__global__ __launch_bounds__(256) void full_attention_kernel(const half_t* qkv, half_t* out, const half_t* bias_k, const half_t* bias_v, int T, int heads, float scale_log2e) {
  constexpr int NT = FA_TMAX / 16, DS = D / 16, LDK = D + 4, LDV = FA_TMAX + 4;
  constexpr int SMEM = FA_TMAX * LDK > D * LDV ? FA_TMAX * LDK : D * LDV;
  __shared__ __attribute__((aligned(16))) half_t sm[SMEM];
  const int b = blockIdx.y / heads, hd = blockIdx.y % heads, H = heads * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const int nkeys = T + (bias_k ? 1 : 0), nt = (nkeys + 15) >> 4, rows = nt * 16;
  const half_t* base = qkv + (size_t)b * T * 3 * H + hd * D;
  const h4 zero4 = {0, 0, 0, 0};
  // K rows -> LDS [key][D] (8-byte pieces)
  for (int i = threadIdx.x; i < rows * (D / 4); i += 256) {
    const int r = i / (D / 4), c4 = (i % (D / 4)) * 4;
    h4 v = zero4;
    if (r < T) v = *(const h4*)(base + (size_t)r * 3 * H + H + c4);
    else if (r < nkeys) v = *(const h4*)(bias_k + hd * D + c4);
    *(h4*)(sm + r * LDK + c4) = v;
  }
  // this lane's query (one column of every S^T tile): D / 16 B-operand fragments straight from HBM
  const int q = blockIdx.x * FA_QTILE + wave * 16 + col;
  h4 qf[DS];
#pragma unroll
  for (int s = 0; s < DS; ++s) qf[s] = q < T ? *(const h4*)(base + (size_t)q * 3 * H + 16 * s + 4 * grp) : zero4;
  __syncthreads();
  f4 sc[NT];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j < nt) {
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < DS; ++s) {
        const h4 kf = *(const h4*)(sm + (16 * j + col) * LDK + 16 * s + 4 * grp);
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[s], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i] = 16 * j + 4 * grp + i < nkeys ? acc[i] * scale_log2e : -INFINITY;
        m = fmaxf(m, acc[i]);
      }
      sc[j] = acc;
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
  h4 pf[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j < nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = exp2f(sc[j][i] - m);      // (masked keys: exp2(-inf) = 0)
        sum += p;
        pf[j][i] = (half_t)p;
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  __syncthreads();                                 // every wave is done with K
  // V rows -> LDS transposed [d][key]
  for (int i = threadIdx.x; i < rows * (D / 8); i += 256) {
    const int r = i / (D / 8), c8 = (i % (D / 8)) * 8;
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < T) v = *(const h8*)(base + (size_t)r * 3 * H + 2 * H + c8);
    else if (r < nkeys) v = *(const h8*)(bias_v + hd * D + c8);
#pragma unroll
    for (int u = 0; u < 8; ++u) sm[(c8 + u) * LDV + r] = v[u];
  }
  __syncthreads();
  const float inv = 1.f / sum;
#pragma unroll
  for (int db = 0; db < DS; ++db) {
    f4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (j < nt) {
        const h4 vf = *(const h4*)(sm + (16 * db + col) * LDV + 16 * j + 4 * grp);
        o = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[j], o, 0, 0, 0);
      }
    }
    if (q < T) {
      h4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = (half_t)(o[i] * inv);
      *(h4*)(out + ((size_t)b * T + q) * H + hd * D + 16 * db + 4 * grp) = r;
    }
  }
}

// ---- im2col rows of a strided patch grid: cols[(b * gh * gw + py * gw + px)][k], k = (c, ky, kx) as torch's conv weight flattens, zero for k >= C * ps * ps -------
// px [B, C, Hi, Wi] fp16. Non-overlapping (stride == ps) and overlapping (stride < ps) grids alike; one workgroup per patch row.
__global__ __launch_bounds__(256) void patch_gather_kernel(const half_t* px, half_t* cols, int C, int Hi, int Wi, int ps, int stride, int gh, int gw, int Kpad) {
  const int row = blockIdx.x, P = gh * gw;
  const int b = row / P, p = row % P, y0 = (p / gw) * stride, x0 = (p % gw) * stride;
  const int Kraw = C * ps * ps;
  for (int k = threadIdx.x; k < Kpad; k += 256) {
    half_t v = (half_t)0.f;
    if (k < Kraw) {
      const int c = k / (ps * ps), r = k % (ps * ps), ky = r / ps, kx = r % ps;
      v = px[(((size_t)b * C + c) * Hi + y0 + ky) * Wi + x0 + kx];
    }
    cols[(size_t)row * Kpad + k] = v;
  }
}

// ---- x[b, 0] = cls + pos[0];  x[b, 1 + p] = LN_stem?(patch[b, p]) + pos[1 + p];  then x = LN_pre?(x); stats[row] = {sum, sum^2} of the fp16 row -----------
// One wave per token row, the row in registers (H <= 2048, H % 64 == 0). LayerNorms in fp32, two-pass. The statistics are what the first block's folded
// LayerNorm GEMM reads (slot 0), as clip_embed_kernel writes them.
__global__ __launch_bounds__(256) void vit_embed_kernel(const half_t* patches, const half_t* cls, const half_t* pos, const half_t* sg, const half_t* sb,
                                                        const half_t* pg, const half_t* pb, half_t* x, float* stats, int rows, int T, int H, float eps) {
  constexpr int NJ = 32;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = row / T, t = row % T, nj = H >> 6;
  const half_t* src = t == 0 ? cls : patches + ((size_t)b * (T - 1) + t - 1) * H;
  float v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) v[j] = j < nj ? (float)src[lane + 64 * j] : 0.f;
  auto layer_norm = [&](const half_t* g, const half_t* be) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s += v[j];
    const float mean = wave_sum(s) / (float)H;
    float var = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) if (j < nj) { const float d = v[j] - mean; var += d * d; }
    const float rstd = rsqrtf(wave_sum(var) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) if (j < nj) v[j] = (v[j] - mean) * rstd * (float)g[lane + 64 * j] + (float)be[lane + 64 * j];
  };
  if (sg && t > 0) layer_norm(sg, sb);
#pragma unroll
  for (int j = 0; j < NJ; ++j) if (j < nj) v[j] += (float)pos[(size_t)t * H + lane + 64 * j];
  if (pg) layer_norm(pg, pb);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (j < nj) {
      const half_t o = (half_t)v[j];
      const float f = (float)o;
      s1 += f; s2 += f * f;
      x[(size_t)row * H + lane + 64 * j] = o;
    }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (lane == 0) ((float2*)stats)[row] = make_float2(s1, s2);
}

// ---- out[b, n] = X[b, :] . W[n, :] in fp32 (the bias-free head projection of the class rows; K % 8 == 0). One wave per output element. ----------------------
__global__ __launch_bounds__(256) void vit_project_kernel(const half_t* X, const half_t* W, float* out, int N, int K) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (n >= N) return;
  float acc = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const h8 x = *(const h8*)(X + (size_t)b * K + k), w = *(const h8*)(W + (size_t)n * K + k);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (float)x[u] * (float)w[u];
  }
  acc = wave_sum(acc);
  if (lane == 0) out[(size_t)b * N + n] = acc;
}

// ---- launchers (arguments are checked here: nothing is launched on hipErrorInvalidValue) -----------------------------------------------------------------
int ia2p_full_attention_max_keys() { return FA_TMAX; }
hipError_t ia2p_launch_full_attention(const half_t* qkv, half_t* out, const half_t* bias_k, const half_t* bias_v, int B, int T, int heads, int D, hipStream_t s) {
  const int nkeys = T + (bias_k ? 1 : 0);
  if (B < 1 || T < 1 || heads < 1 || nkeys > FA_TMAX || (D != 64 && D != 80) || (!bias_k) != (!bias_v) || (size_t)B * heads > 65535) return hipErrorInvalidValue;
  const dim3 grid((T + FA_QTILE - 1) / FA_QTILE, B * heads);
  const float sl2 = 1.4426950408889634f / sqrtf((float)D);
  if (D == 64) hipLaunchKernelGGL(full_attention_kernel<64>, grid, dim3(256), 0, s, qkv, out, bias_k, bias_v, T, heads, sl2);
  else hipLaunchKernelGGL(full_attention_kernel<80>, grid, dim3(256), 0, s, qkv, out, bias_k, bias_v, T, heads, sl2);
  return hipGetLastError();
}
hipError_t ia2p_launch_patch_gather(const half_t* px, half_t* cols, int B, int C, int Hi, int Wi, int ps, int stride, int gh, int gw, int Kpad, hipStream_t s) {
  if (B < 1 || C < 1 || ps < 1 || stride < 1 || gh < 1 || gw < 1 || (gh - 1) * stride + ps > Hi || (gw - 1) * stride + ps > Wi || Kpad < C * ps * ps) return hipErrorInvalidValue;
  hipLaunchKernelGGL(patch_gather_kernel, dim3(B * gh * gw), dim3(256), 0, s, px, cols, C, Hi, Wi, ps, stride, gh, gw, Kpad);
  return hipGetLastError();
}
hipError_t ia2p_launch_vit_embed(const half_t* patches, const half_t* cls, const half_t* pos, const half_t* stem_g, const half_t* stem_b, const half_t* pre_g, const half_t* pre_b,
                                 half_t* x, float* stats, int B, int T, int H, float eps, hipStream_t s) {
  if (B < 1 || T < 2 || H < 64 || H % 64 || H > 2048) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vit_embed_kernel, dim3((B * T + 3) / 4), dim3(256), 0, s, patches, cls, pos, stem_g, stem_b, pre_g, pre_b, x, stats, B * T, T, H, eps);
  return hipGetLastError();
}
hipError_t ia2p_launch_vit_project(const half_t* X, const half_t* W, float* out, int B, int N, int K, hipStream_t s) {
  if (B < 1 || B > 65535 || N < 1 || K < 8 || K % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vit_project_kernel, dim3((N + 3) / 4, B), dim3(256), 0, s, X, W, out, N, K);
  return hipGetLastError();
}
