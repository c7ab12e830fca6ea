// Kernels of the LLaMA decoder executor on fp16 weights, and their launchers: the decode GEMVs (one input row; 2 to 8 input rows), attention against the
// KV cache, the row kernels of the prefill path. Included by llm_engine.hip only (after engine_rt.h); the 4-bit kernels are in llm_q4.h. DESIGN.md §10.
#pragma once
#include <type_traits>

enum { EPI_PLAIN = 0, EPI_RESID = 1, EPI_QKV = 2, EPI_SWIGLU = 3 };
struct LlmGemv {
  const half_t* W;        // [N, K] row-major
  const float* X;         // [K] fp32
  const half_t* gamma;    // RMSNorm weight applied to X on the way in (with eps), or null
  float eps;
  int N, K;
  float* out;             // EPI_PLAIN: out[n] = r;  EPI_RESID: out[n] += r;  EPI_SWIGLU: out[i] = silu(r[i]) * r[I + i] (N = 2 I)
  float* hid;             // EPI_PLAIN with gamma: the normed input row (workgroup 0 writes it), or null
  // EPI_QKV (N = 3 H): q row (fp32, rotated), k / v rows of the cache at `pos`
  const float* inv_freq;  // [64]
  int pos, H;
  float* q;
  half_t* kc;
  half_t* vc;
};

// ---- what the four GEMV kernels (fp16 and 4-bit, one input row and several) share: which weight rows an output needs, and what becomes of their sums ----
// EPI_QKV / EPI_SWIGLU: output `unit` needs two weight rows, r = 0, 1 (the rows (d, d + 64) of a rotary pair / a gate row and its up row); else `unit` is a
// group of `rw` consecutive rows, r its member. Units past the end read the last one (and store nothing).
template <int EPI>
__device__ __forceinline__ int llm_weight_row(int N, int unit, int r, int rw) {
  if (EPI == EPI_QKV) { const int pidx = min(unit, N / 2 - 1); return (pidx >> 6) * 128 + (pidx & 63) + 64 * r; }
  if (EPI == EPI_SWIGLU) return min(unit, N / 2 - 1) + r * (N / 2);
  return min(unit * rw + r, N - 1);
}
// EPI_QKV: rows (d, d + 64) of rotary pair `pidx` -> q row (rotated), k row (rotated) or v row of the cache at `pos`
__device__ __forceinline__ void llm_store_qkv_pair(const LlmGemv& a, int pidx, float x1, float x2) {
  const int lo = (pidx >> 6) * 128 + (pidx & 63), sec = lo / a.H, c = lo - sec * a.H;
  if (sec < 2) {               // q, k: x cos + rotate_half(x) sin
    const float ang = (float)a.pos * a.inv_freq[pidx & 63];
    const float cs = cosf(ang), sn = sinf(ang);
    const float y1 = x1 * cs - x2 * sn, y2 = x2 * cs + x1 * sn;
    x1 = y1; x2 = y2;
  }
  if (sec == 0) { a.q[c] = x1; a.q[c + 64] = x2; }
  else {
    half_t* dst = (sec == 1 ? a.kc : a.vc) + (size_t)a.pos * a.H + c;
    dst[0] = (half_t)x1; dst[64] = (half_t)x2;
  }
}
// the store of one output: i = weight row (EPI_PLAIN, EPI_RESID: s0 its sum) or unit (EPI_SWIGLU, EPI_QKV: s0, s1 the sums of its two rows). `out` is the row's
// output (a.out in a single-row launch); EPI_QKV stores through the q row, cache rows and position of the view `a` instead
template <int EPI>
__device__ __forceinline__ void llm_store(const LlmGemv& a, float* out, int i, float s0, float s1, float rstd) {
  if (EPI == EPI_PLAIN) out[i] = s0 * rstd;
  else if (EPI == EPI_RESID) out[i] = fmaf(rstd, s0, out[i]);
  else if (EPI == EPI_SWIGLU) { const float g = s0 * rstd, u = s1 * rstd; out[i] = g / (1.0f + expf(-g)) * u; }
  else llm_store_qkv_pair(a, i, s0 * rstd, s1 * rstd);
}

// out = epilogue(W . f(x)): a workgroup of 4 waves owns R weight rows; its threads walk K in 16-byte pieces (thread t: pieces t, t + 256, ...), so each
// step of the workgroup reads 4 KiB of every row, once, with non-temporal loads; fp32 accumulation; the 4 waves' partial sums meet in LDS in wave order
// (a K split inside the workgroup: deterministic, no atomics). The RMSNorm in front is folded in: sum x^2 over the pieces the threads hold anyway,
// out = rstd * sum (x gamma) w.
// The R rows: one group of R (EPI_PLAIN, EPI_RESID), or R / 2 units of two, the second rows in the upper half of rows[] (thread t < R / 2 stores unit t).
template <int R, int EPI>
__device__ __forceinline__ void llm_gemv_rows_of(int N, int* rows) {
  constexpr int HR = R / 2;
#pragma unroll
  for (int i = 0; i < R; ++i)
    rows[i] = EPI == EPI_QKV || EPI == EPI_SWIGLU ? llm_weight_row<EPI>(N, (int)blockIdx.x * HR + i % HR, i / HR, 2) : llm_weight_row<EPI>(N, (int)blockIdx.x, i, R);
}
template <int R, int EPI>
__global__ __launch_bounds__(256) void llm_gemv_kernel(LlmGemv a) {
  __shared__ float red[4][R + 1];
  constexpr int HR = R / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  int rows[R];
  llm_gemv_rows_of<R, EPI>(a.N, rows);
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.f;
  float ss = 0.f;
  const int nvec = K >> 3;
#pragma unroll 2
  for (int v = tid; v < nvec; v += 256) {
    h8 w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = __builtin_nontemporal_load((const h8*)(a.W + (size_t)rows[r] * K) + v);
    const f4 x0 = ((const f4*)a.X)[2 * v], x1 = ((const f4*)a.X)[2 * v + 1];
    float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    if (a.gamma) {
      const h8 g = ((const h8*)a.gamma)[v];
#pragma unroll
      for (int e = 0; e < 8; ++e) { ss = fmaf(x[e], x[e], ss); x[e] *= (float)g[e]; }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[r] = fmaf(x[e], (float)w[r][e], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = wave_sum(acc[r]);
  ss = wave_sum(ss);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) red[wave][r] = acc[r];
    red[wave][R] = ss;
  }
  __syncthreads();
  float rstd = 1.f;
  if (a.gamma) rstd = 1.0f / sqrtf(((red[0][R] + red[1][R]) + (red[2][R] + red[3][R])) / (float)K + a.eps);
  auto sum4 = [&](int r) { return (red[0][r] + red[1][r]) + (red[2][r] + red[3][r]); };
  if (EPI == EPI_PLAIN || EPI == EPI_RESID) {
    const int n = (int)blockIdx.x * R + tid;
    if (tid < R && n < a.N) llm_store<EPI>(a, a.out, n, sum4(tid), 0.f, rstd);
    if (EPI == EPI_PLAIN && a.hid && a.gamma && blockIdx.x == 0)
      for (int i = tid; i < K; i += 256) a.hid[i] = a.X[i] * rstd * (float)a.gamma[i];
  } else {
    const int i = (int)blockIdx.x * HR + tid;
    if (tid < HR && i < a.N / 2) llm_store<EPI>(a, a.out, i, sum4(tid), sum4(tid + HR), rstd);
  }
}

// One query row per workgroup (head = blockIdx.x, q / out row = blockIdx.y) against the cached keys 0 .. nk - 1, head dim 128:
// 16 lanes per key (16 bytes of it each), 16 keys per pass; scores in LDS, softmax in fp32, P.V summed per key group and combined in group order.
template <typename OT>
__device__ __forceinline__ void llm_attn_row(const float* q, const half_t* kc, const half_t* vc, OT* out, int H, int nk, float scale) {
  extern __shared__ float llm_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, l = tid & 15;
  const int head = blockIdx.x, t = blockIdx.y;
  float* sc = llm_sm;                 // [nk]
  float* part = llm_sm + ((nk + 3) & ~3);   // [16][128]
  float* red = part + 16 * 128;       // [8]
  float qv[8];
  {
    const float* qp = q + (size_t)t * H + head * 128 + l * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = qp[e] * scale;
  }
  for (int j0 = 0; j0 < nk; j0 += 16) {      // (uniform trip count: the shuffles below need every lane)
    const int j = j0 + g;
    float s = 0.f;
    if (j < nk) {
      const h8 k = *(const h8*)(kc + (size_t)j * H + head * 128 + l * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(qv[e], (float)k[e], s);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (l == 0 && j < nk) sc[j] = s;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int j = tid; j < nk; j += 256) m = fmaxf(m, sc[j]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int j = tid; j < nk; j += 256) { const float e = expf(sc[j] - m); sc[j] = e; sum += e; }
  sum = wave_sum(sum);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  sum = (red[4] + red[5]) + (red[6] + red[7]);
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  for (int j = g; j < nk; j += 16) {
    const float p = sc[j];
    const h8 v = *(const h8*)(vc + (size_t)j * H + head * 128 + l * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(p, (float)v[e], o[e]);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[g * 128 + l * 8 + e] = o[e];
  __syncthreads();
  if (tid < 128) {
    float r = 0.f;
#pragma unroll
    for (int gg = 0; gg < 16; ++gg) r += part[gg * 128 + tid];
    out[(size_t)t * H + head * 128 + tid] = (OT)(r / sum);
  }
}
// prefill: grid (heads, T), row t at position p0 + t of one cache
template <typename OT>
__global__ __launch_bounds__(256) void llm_attn_kernel(const float* q, const half_t* kc, const half_t* vc, OT* out, int H, int p0, float scale) {
  llm_attn_row<OT>(q, kc, vc, out, H, p0 + (int)blockIdx.y + 1, scale);
}

// ---- row kernels of the prefill path -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void llm_rmsnorm_rows_kernel(const half_t* x, half_t* y, const half_t* gamma, int H, float eps) {
  __shared__ float red[4];
  const half_t* xr = x + (size_t)blockIdx.x * H;
  half_t* yr = y + (size_t)blockIdx.x * H;
  float ss = 0.f;
  for (int i = threadIdx.x; i < H; i += 256) { const float v = (float)xr[i]; ss = fmaf(v, v, ss); }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float rstd = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + eps);
  for (int i = threadIdx.x; i < H; i += 256) yr[i] = (half_t)((float)xr[i] * rstd * (float)gamma[i]);
}
// qkv [T, 3 H] fp16 -> q [T, H] fp32 (rotated), cache rows p0 + t (k rotated, v as is)
__global__ __launch_bounds__(256) void llm_rope_cache_rows_kernel(const half_t* qkv, float* q, half_t* kc, half_t* vc, const float* inv_freq, int H, int p0) {
  const int t = blockIdx.x, pos = p0 + t;
  const half_t* r = qkv + (size_t)t * 3 * H;
  for (int i = threadIdx.x; i < H / 2; i += 256) {
    const int c = (i >> 6) * 128 + (i & 63);
    const float ang = (float)pos * inv_freq[i & 63];
    const float cs = cosf(ang), sn = sinf(ang);
    const float q1 = (float)r[c], q2 = (float)r[c + 64], k1 = (float)r[H + c], k2 = (float)r[H + c + 64];
    q[(size_t)t * H + c] = q1 * cs - q2 * sn;
    q[(size_t)t * H + c + 64] = q2 * cs + q1 * sn;
    kc[(size_t)pos * H + c] = (half_t)(k1 * cs - k2 * sn);
    kc[(size_t)pos * H + c + 64] = (half_t)(k2 * cs + k1 * sn);
    vc[(size_t)pos * H + c] = r[2 * H + c];
    vc[(size_t)pos * H + c + 64] = r[2 * H + c + 64];
  }
}
__global__ __launch_bounds__(256) void llm_silu_mul_rows_kernel(const half_t* gu, half_t* act, int I) {
  const half_t* r = gu + (size_t)blockIdx.x * 2 * I;
  for (int i = threadIdx.x; i < I; i += 256) {
    const float g = (float)r[i], u = (float)r[I + i];
    act[(size_t)blockIdx.x * I + i] = (half_t)(g / (1.0f + expf(-g)) * u);
  }
}
__global__ __launch_bounds__(256) void llm_row_f32_kernel(const half_t* src, float* dst, int H) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H; i += gridDim.x * 256) dst[i] = (float)src[i];
}
__global__ __launch_bounds__(256) void llm_gather_rows_kernel(const int* ids, const half_t* tok, half_t* out, int H, int vocab) {
  const int id = min(max(ids[blockIdx.x], 0), vocab - 1);
  for (int i = threadIdx.x; i < H / 8; i += 256) ((h8*)(out + (size_t)blockIdx.x * H))[i] = ((const h8*)(tok + (size_t)id * H))[i];
}
// exact (erf) GELU in place: the activation between the two linears of an `mlpNx_gelu` projector head
__global__ __launch_bounds__(256) void llm_gelu_kernel(half_t* x, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { const float v = (float)x[i]; x[i] = (half_t)(0.5f * v * (1.0f + erff(v * 0.70710678118654752440f))); }
}

// =====================================================================================================================
// Up to IA2P_LLM_MAX_ROWS sequences per weight pass (ia2p_llm_decode_batch). llm_gemv_kernel and llm_gemv_q4_kernel serve one input row; the rows kernels
// read (in 4 bits: decode) every weight once and apply it to M input rows, each row at its own position and in its own cache slot. A row's arithmetic never
// involves another row and keeps the single-row kernel's order of operations, so row m of a launch equals the single-row launch on that row bit for bit:
//   llm_gemv_rows_kernel     thread t walks pieces t, t + 256, ... of K; per piece the same fmaf chain; the four waves' partials meet in LDS in wave order
//   llm_gemv_q4_rows_kernel  lane l takes pieces l, l + 64, ... (32 weights, one absmax); the same s0 / s1 packed-FMA order, fmaf(sum, absmax, acc) per
//                            block, wave_sum, rstd afterwards
//   llm_attn_rows_kernel     llm_attn_row on grid (heads, rows); row r reads the cache of its slot up to its own position
// The weight rows of an output and its store are the single-row kernels' (llm_weight_row; llm_store on the row's `out`, EPI_QKV on llm_row_view). All on VALU in fp32
// (the residual stream of a decoded row is fp32). The per-row pointers and positions travel by value in the kernel arguments: a decode step copies nothing
// to the device.
// MT = rows a launch computes (2, 4 or 8: M rounded up; the host repeats row M - 1 in the unused entries and the kernel stores rows m < M only). One row
// is the single-row kernels' (llm_launch_gemv_rows and llm_launch_gemv_q4_rows hand M = 1 to llm_launch_gemv and llm_launch_gemv_q4).
// =====================================================================================================================
constexpr int LLM_MAX_ROWS = IA2P_LLM_MAX_ROWS;
struct LlmRows {
  const float* X[LLM_MAX_ROWS];   // input rows [K] fp32
  float* out[LLM_MAX_ROWS];       // as LlmGemv::out, per row
  float* hid[LLM_MAX_ROWS];       // as LlmGemv::hid
  float* q[LLM_MAX_ROWS];         // EPI_QKV: q row, cache rows of the row's slot (this layer), position
  half_t* kc[LLM_MAX_ROWS];
  half_t* vc[LLM_MAX_ROWS];
  int pos[LLM_MAX_ROWS];
  int M;
};
// `a` carries what the rows share (W, gamma, eps, N, K, inv_freq, H); EPI_QKV stores row m through this view of it
__device__ __forceinline__ LlmGemv llm_row_view(const LlmGemv& a, const LlmRows& b, int m) {
  LlmGemv v = a;
  v.pos = b.pos[m]; v.q = b.q[m]; v.kc = b.kc[m]; v.vc = b.vc[m];
  return v;
}

// R weight rows per workgroup as in llm_gemv_kernel (R does not enter a row's arithmetic)
template <int R, int EPI, int MT>
__global__ __launch_bounds__(256) void llm_gemv_rows_kernel(LlmGemv a, LlmRows b) {
  __shared__ float red[4][MT][R + 1];
  constexpr int HR = R / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  int rows[R];
  llm_gemv_rows_of<R, EPI>(a.N, rows);
  float acc[MT][R], ss[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    ss[m] = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
  }
  const int nvec = K >> 3;
  constexpr int UNROLL = MT <= 2 ? 2 : 1;
#pragma unroll UNROLL
  for (int v = tid; v < nvec; v += 256) {
    h8 w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = __builtin_nontemporal_load((const h8*)(a.W + (size_t)rows[r] * K) + v);
    h8 g;
    if (a.gamma) g = ((const h8*)a.gamma)[v];
#pragma unroll
    for (int m = 0; m < MT; ++m) {      // the piece is in registers: every input row uses it before the next one is loaded
      const f4 x0 = ((const f4*)b.X[m])[2 * v], x1 = ((const f4*)b.X[m])[2 * v + 1];
      float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      if (a.gamma) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { ss[m] = fmaf(x[e], x[e], ss[m]); x[e] *= (float)g[e]; }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[m][r] = fmaf(x[e], (float)w[r][e], acc[m][r]);
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = wave_sum(acc[m][r]);
    ss[m] = wave_sum(ss[m]);
  }
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int r = 0; r < R; ++r) red[wave][m][r] = acc[m][r];
      red[wave][m][R] = ss[m];
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (m >= b.M) break;
    float rstd = 1.f;
    if (a.gamma) rstd = 1.0f / sqrtf(((red[0][m][R] + red[1][m][R]) + (red[2][m][R] + red[3][m][R])) / (float)K + a.eps);
    auto sum4 = [&](int r) { return (red[0][m][r] + red[1][m][r]) + (red[2][m][r] + red[3][m][r]); };
    if (EPI == EPI_PLAIN || EPI == EPI_RESID) {
      const int n = (int)blockIdx.x * R + tid;
      if (tid < R && n < a.N) llm_store<EPI>(a, b.out[m], n, sum4(tid), 0.f, rstd);
      if (EPI == EPI_PLAIN && b.hid[m] && a.gamma && blockIdx.x == 0)
        for (int i = tid; i < K; i += 256) b.hid[m][i] = b.X[m][i] * rstd * (float)a.gamma[i];
    } else {
      const int i = (int)blockIdx.x * HR + tid;
      if (tid < HR && i < a.N / 2) {
        if (EPI == EPI_QKV) llm_store<EPI>(llm_row_view(a, b, m), nullptr, i, sum4(tid), sum4(tid + HR), rstd);
        else llm_store<EPI>(a, b.out[m], i, sum4(tid), sum4(tid + HR), rstd);
      }
    }
  }
}

// llm_attn_row for one decoded row per sequence: row r = blockIdx.y against the keys 0 .. pos[r] of its own cache slot
struct LlmAttnRows {
  const half_t* kc[LLM_MAX_ROWS];
  const half_t* vc[LLM_MAX_ROWS];
  int pos[LLM_MAX_ROWS];
};
__global__ __launch_bounds__(256) void llm_attn_rows_kernel(const float* q, LlmAttnRows rows, float* out, int H, float scale) {
  llm_attn_row<float>(q, rows.kc[blockIdx.y], rows.vc[blockIdx.y], out, H, rows.pos[blockIdx.y] + 1, scale);
}
// token rows of the embedding table as fp32: row r = blockIdx.y, the ids by value
struct LlmTokRows { int id[LLM_MAX_ROWS]; };
__global__ __launch_bounds__(256) void llm_rows_f32_kernel(const half_t* tok, LlmTokRows ids, float* dst, int H) {
  const half_t* src = tok + (size_t)ids.id[blockIdx.y] * H;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H; i += gridDim.x * 256) dst[(size_t)blockIdx.y * H + i] = (float)src[i];
}
// the same with the ids in device memory (ia2p_llm_decode_batch_dev: the sampler's output is never read by the host in between): row r takes
// dev_ids[idx.id[r]], the indices by value. The id is data another kernel wrote, so it is clamped into the table here and never indexes it unchecked.
__global__ __launch_bounds__(256) void llm_rows_dev_f32_kernel(const half_t* tok, const int* dev_ids, LlmTokRows idx, float* dst, int H, int vocab) {
  const int id = min(max(dev_ids[idx.id[blockIdx.y]], 0), vocab - 1);
  const half_t* src = tok + (size_t)id * H;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H; i += gridDim.x * 256) dst[(size_t)blockIdx.y * H + i] = (float)src[i];
}

// ---- launchers ------------------------------------------------------------------------------------------------------
// the run-time epilogue as a compile-time constant: f(std::integral_constant<int, EPI>) picks the kernel instantiation (the one switch over the four)
template <typename F>
static hipError_t llm_with_epi(int epi, F&& f) {
  switch (epi) {
    case EPI_PLAIN: return f(std::integral_constant<int, EPI_PLAIN>{});
    case EPI_RESID: return f(std::integral_constant<int, EPI_RESID>{});
    case EPI_QKV: return f(std::integral_constant<int, EPI_QKV>{});
    case EPI_SWIGLU: return f(std::integral_constant<int, EPI_SWIGLU>{});
    default: return hipErrorInvalidValue;
  }
}
static bool llm_epi_shape_ok(int epi, int N, int H) { return !((epi == EPI_QKV && (N != 3 * H || H % 128)) || (epi == EPI_SWIGLU && N % 2)); }
// the argument check of the fp16 GEMVs, shared by the launchers and the ABI entry points (`x` = the first input row): 0, or what is wrong -- a null pointer
// (IA2P_ERR_INVALID) before a shape (IA2P_ERR_SHAPE). No side effect; llm_refuse words the refusal for an entry point
static ia2p_status llm_gemv_check(const void* W, const void* x, int N, int K, int H, int M, int epi) {
  if (!W || !x) return IA2P_ERR_INVALID;
  return N < 1 || K < 8 || K % 8 || M < 1 || M > LLM_MAX_ROWS || !llm_epi_shape_ok(epi, N, H) ? IA2P_ERR_SHAPE : IA2P_OK;
}
static ia2p_status llm_refuse(const char* what, ia2p_status st, int N, int K, int kmul, int kmax, int M) {
  if (st != IA2P_ERR_SHAPE) return fail(nullptr, st, "%s: null argument", what);
  if (N < 1 || K < kmul || K % kmul || (kmax && (int64_t)N * K > ((int64_t)1 << 34))) return fail(nullptr, st, "%s: N=%d K=%d (K a multiple of %d)", what, N, K, kmul);
  if (kmax && K > kmax) return fail(nullptr, st, "%s: K=%d (at most %d)", what, K, kmax);
  return fail(nullptr, st, "%s: M=%d (1..%d)", what, M, LLM_MAX_ROWS);
}
// workgroups of a launch whose workgroups own R weight rows: R / 2 outputs of two rows each (EPI_QKV, EPI_SWIGLU: N / 2 outputs) or R rows
static unsigned llm_gemv_grid(int epi, int N, int R) { return epi == EPI_QKV || epi == EPI_SWIGLU ? (N / 2 + R / 2 - 1) / (R / 2) : (N + R - 1) / R; }
template <int R>
static hipError_t gemv_launch_r(const LlmGemv& a, int epi, hipStream_t s) {
  return llm_with_epi(epi, [&](auto E) {
    hipLaunchKernelGGL((llm_gemv_kernel<R, decltype(E)::value>), dim3(llm_gemv_grid(epi, a.N, R)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
// 8 rows per workgroup where that still leaves every CU several workgroups (N >= 8192: 1024+ of them), 4 below (N = 4096: 1024 workgroups)
static hipError_t llm_launch_gemv(const LlmGemv& a, int epi, hipStream_t s) {
  if (llm_gemv_check(a.W, a.X, a.N, a.K, a.H, 1, epi) != IA2P_OK) return hipErrorInvalidValue;
  return a.N >= 8192 ? gemv_launch_r<8>(a, epi, s) : gemv_launch_r<4>(a, epi, s);
}

static LlmGemv llm_first_row(const LlmGemv& a, const LlmRows& b) {      // M = 1: what the single-row launch on row 0 takes
  LlmGemv v = a;
  v.X = b.X[0]; v.out = b.out[0]; v.hid = b.hid[0]; v.pos = b.pos[0]; v.q = b.q[0]; v.kc = b.kc[0]; v.vc = b.vc[0];
  return v;
}
static int rows_mt(int M) { return M <= 2 ? 2 : M <= 4 ? 4 : 8; }
static void rows_pad(LlmRows& b) {      // entries M .. 7 repeat row M - 1: loaded and computed where MT > M, never stored
  for (int m = b.M; m < LLM_MAX_ROWS; ++m) {
    b.X[m] = b.X[b.M - 1]; b.out[m] = b.out[b.M - 1]; b.hid[m] = b.hid[b.M - 1]; b.q[m] = b.q[b.M - 1];
    b.kc[m] = b.kc[b.M - 1]; b.vc[m] = b.vc[b.M - 1]; b.pos[m] = b.pos[b.M - 1];
  }
}
template <int R, int MT>
static hipError_t gemv_rows_launch_r(const LlmGemv& a, const LlmRows& b, int epi, hipStream_t s) {
  return llm_with_epi(epi, [&](auto E) {
    hipLaunchKernelGGL((llm_gemv_rows_kernel<R, decltype(E)::value, MT>), dim3(llm_gemv_grid(epi, a.N, R)), dim3(256), 0, s, a, b);
    return hipGetLastError();
  });
}
// weight rows per workgroup: llm_launch_gemv's rule for two input rows; from three input rows on always 8, because every workgroup reads all the
// input rows (4 M K bytes from L2 against 2 R K bytes of weights) and more weight rows per workgroup halve that share
static hipError_t llm_launch_gemv_rows(const LlmGemv& a, LlmRows b, int epi, hipStream_t s) {
  if (b.M == 1) return llm_launch_gemv(llm_first_row(a, b), epi, s);
  if (llm_gemv_check(a.W, b.X[0], a.N, a.K, a.H, b.M, epi) != IA2P_OK) return hipErrorInvalidValue;
  rows_pad(b);
  switch (rows_mt(b.M)) {
    case 2: return a.N >= 8192 ? gemv_rows_launch_r<8, 2>(a, b, epi, s) : gemv_rows_launch_r<4, 2>(a, b, epi, s);
    case 4: return gemv_rows_launch_r<8, 4>(a, b, epi, s);
    default: return gemv_rows_launch_r<8, 8>(a, b, epi, s);
  }
}
static size_t attn_lds(int nk) { return ((size_t)((nk + 3) & ~3) + 16 * 128 + 8) * sizeof(float); }
constexpr int LLM_MAX_POSITIONS = 8192;       // scores of one query row live in LDS (32 KiB of the 64)
