// LLaMA decoder executor (the instruction LLM) and its C ABI (ia2p_llm_*): see include/ia2p.h and DESIGN.md §10. Runtime and operator wrappers: engine_rt.h / engine_rt.hip.
#include "engine_rt.h"

// =====================================================================================================================
// transformers LlamaModel + lm_head (reference instructany2pix/pipeline.py:201-211 `any2pix_lm.generate`, a Vicuna-7B shaped model):
// pre-RMSNorm blocks, rotary embeddings in the rotate_half convention, multi-head attention at head dim 128, SwiGLU MLP, final norm, untied head.
// Two paths over one fp16 KV cache [layer][k|v][max_positions][hidden]:
//   prefill (T rows): op_gemm projections + row kernels (RMSNorm, RoPE + cache write, SiLU-multiply) + causal attention against the cache
//   decode (one row): five weight-streaming launches per layer -- QKV GEMV (RMSNorm in, RoPE + cache write out), attention, o_proj GEMV (+ residual),
//                     gate/up GEMV (RMSNorm in, silu(gate) * up out), down_proj GEMV (+ residual); the residual stream of the row stays fp32
// The projections of the layers are fp16, or 4-bit codes (ia2p_llm_set_weight_format): decode then runs the same five launches on llm_gemv_q4_kernel and
// prefill dequantises one projection at a time in front of its op_gemm.
// =====================================================================================================================

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

// out = epilogue(W . f(x)): a workgroup of 4 waves owns R weight rows; its threads walk K in 16-byte pieces (thread t: pieces t, t + 256, ...), so each
// step of the workgroup reads 4 KiB of every row, once, with non-temporal loads; fp32 accumulation; the 4 waves' partial sums meet in LDS in wave order
// (a K split inside the workgroup: deterministic, no atomics). The RMSNorm in front is folded in: sum x^2 over the pieces the threads hold anyway,
// out = rstd * sum (x gamma) w.
template <int R, int EPI>
__global__ __launch_bounds__(256) void llm_gemv_kernel(LlmGemv a) {
  __shared__ float red[4][R + 1];
  constexpr int HR = R / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  int rows[R];
  if (EPI == EPI_QKV) {            // R / 2 rotary pairs (d, d + 64) of one head block
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const int pidx = min((int)blockIdx.x * HR + i, a.N / 2 - 1);
      rows[i] = (pidx >> 6) * 128 + (pidx & 63);
      rows[i + HR] = rows[i] + 64;
    }
  } else if (EPI == EPI_SWIGLU) {  // R / 2 gate rows and their up rows
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      rows[i] = min((int)blockIdx.x * HR + i, a.N / 2 - 1);
      rows[i + HR] = a.N / 2 + rows[i];
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = min((int)blockIdx.x * R + r, a.N - 1);
  }
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
  auto total = [&](int r) { return ((red[0][r] + red[1][r]) + (red[2][r] + red[3][r])) * rstd; };
  if (EPI == EPI_PLAIN || EPI == EPI_RESID) {
    const int n = (int)blockIdx.x * R + tid;
    if (tid < R && n < a.N) {
      const float r = total(tid);
      a.out[n] = EPI == EPI_RESID ? a.out[n] + r : r;
    }
    if (EPI == EPI_PLAIN && a.hid && a.gamma && blockIdx.x == 0)
      for (int i = tid; i < K; i += 256) a.hid[i] = a.X[i] * rstd * (float)a.gamma[i];
  } else if (EPI == EPI_SWIGLU) {
    const int i = (int)blockIdx.x * HR + tid;
    if (tid < HR && i < a.N / 2) {
      const float g = total(tid), u = total(tid + HR);
      a.out[i] = g / (1.0f + expf(-g)) * u;
    }
  } else {
    const int pidx = (int)blockIdx.x * HR + tid;
    if (tid < HR && pidx < a.N / 2) llm_store_qkv_pair(a, pidx, total(tid), total(tid + HR));
  }
}

// One query row per workgroup (head = blockIdx.x, row t = blockIdx.y at position p0 + t) against the cached keys 0 .. p0 + t, head dim 128:
// 16 lanes per key (16 bytes of it each), 16 keys per pass; scores in LDS, softmax in fp32, P.V summed per key group and combined in group order.
template <typename OT>
__global__ __launch_bounds__(256) void llm_attn_kernel(const float* q, const half_t* kc, const half_t* vc, OT* out, int H, int p0, float scale) {
  extern __shared__ float llm_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, l = tid & 15;
  const int head = blockIdx.x, t = blockIdx.y, nk = p0 + t + 1;
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

template <int R>
static hipError_t gemv_launch_r(const LlmGemv& a, int epi, hipStream_t s) {
  const int units = epi == EPI_QKV || epi == EPI_SWIGLU ? (a.N / 2 + R / 2 - 1) / (R / 2) : (a.N + R - 1) / R;
  switch (epi) {
    case EPI_PLAIN: hipLaunchKernelGGL((llm_gemv_kernel<R, EPI_PLAIN>), dim3(units), dim3(256), 0, s, a); break;
    case EPI_RESID: hipLaunchKernelGGL((llm_gemv_kernel<R, EPI_RESID>), dim3(units), dim3(256), 0, s, a); break;
    case EPI_QKV: hipLaunchKernelGGL((llm_gemv_kernel<R, EPI_QKV>), dim3(units), dim3(256), 0, s, a); break;
    case EPI_SWIGLU: hipLaunchKernelGGL((llm_gemv_kernel<R, EPI_SWIGLU>), dim3(units), dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
// 8 rows per workgroup where that still leaves every CU several workgroups (N >= 8192: 1024+ of them), 4 below (N = 4096: 1024 workgroups)
static hipError_t llm_launch_gemv(const LlmGemv& a, int epi, hipStream_t s) {
  if (!a.W || !a.X || a.N < 1 || a.K < 8 || a.K % 8) return hipErrorInvalidValue;
  if ((epi == EPI_QKV && (a.N != 3 * a.H || a.H % 128)) || (epi == EPI_SWIGLU && a.N % 2)) return hipErrorInvalidValue;
  return a.N >= 8192 ? gemv_launch_r<8>(a, epi, s) : gemv_launch_r<4>(a, epi, s);
}
// =====================================================================================================================
// 4-bit weights (bitsandbytes `load_in_4bit`: block-wise absmax quantisation at load, block 64, fp32 absmax, a 16-entry codebook passed in as data).
// Arena layout of a quantised [N, K] matrix: codes in row-major weight order, two per byte (weight 2 b in the low nibble of byte b, 2 b + 1 in the high
// one), so a row is K / 2 bytes and a 16-byte piece is half a block; one fp32 absmax per block in a second array, [N * K / 64] in the same order.
// =====================================================================================================================
typedef float f2 __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
struct Q4Codebook { float v[16]; };                       // index = 4-bit code
struct Q4Thresholds { float thr[15]; unsigned long long code_at; };   // fp32 midpoints of the sorted codebook; code_at: the code at sorted position i in bits 4 i .. 4 i + 3
struct LlmQ4 { const u4v* Wq; const float* absmax; Q4Codebook cb; };
constexpr int Q4_RW = 2, Q4_U = 2;                         // rows per unit of a wave, units per wave (llm_gemv_q4_kernel)
constexpr int Q4_MAX_K = 14336;                           // the staged input row: 7 chunks of 2048 floats + the byte table fit the 64 KiB of LDS a launch gets

// 8 weights per thread, 8 threads per block: absmax = max |w| (exact in fp32), x = w / absmax (correctly rounded), code = the sorted codebook's entry at
// position #{thresholds strictly below x}; an all-zero block stores absmax 0 and the code of x = 0
__global__ __launch_bounds__(256) void llm_quantize_q4_kernel(const half_t* W, long n8, Q4Thresholds t, unsigned* packed, float* absmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const h8 w = ((const h8*)W)[i < n8 ? i : n8 - 1];       // (n8 is a multiple of 8: the 8 lanes of a block are all inside or all outside)
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)w[e]));
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 8));
  unsigned out = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = m > 0.f ? __fdiv_rn((float)w[e], m) : 0.f;
    int pos = 0;
#pragma unroll
    for (int j = 0; j < 15; ++j) pos += t.thr[j] < x ? 1 : 0;
    out |= (unsigned)((t.code_at >> (4 * pos)) & 15) << (4 * e);
  }
  if (i < n8) {
    packed[i] = out;
    if ((i & 7) == 0) absmax[i >> 3] = m;
  }
}
// packed -> fp16 [N, K]: codebook[code] * absmax, the fp32 product rounded to fp16 (what bitsandbytes hands its matmul)
// (the empty asm keeps the fp32 product a value of its own: selected together with the conversion into one v_fma_mix*_f16 it is rounded once, straight to
//  fp16, and a -0 product comes out +0)
__global__ __launch_bounds__(256) void llm_dequantize_q4_kernel(const unsigned* packed, const float* absmax, long n8, Q4Codebook cb, half_t* W) {
  __shared__ float tab[16];
  if (threadIdx.x < 16) tab[threadIdx.x] = cb.v[threadIdx.x];
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const unsigned c = packed[i];
  const float m = absmax[i >> 3];
  h8 w;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float p = tab[(c >> (4 * e)) & 15] * m;
    asm volatile("" : "+v"(p));
    w[e] = (half_t)p;
  }
  ((h8*)W)[i] = w;
}

// The decode GEMV on 4-bit weights; contract of llm_gemv_kernel (fp32 input row, RMSNorm folded in, the four epilogues, fp32 accumulation, fixed summation order,
// no atomics). A packed K = 4096 row is 128 pieces of 16 bytes, so a wave owns whole rows -- a unit of RW = 2 (EPI_QKV / EPI_SWIGLU: the two rows of one output) -- and
// no sum crosses waves: lane l takes pieces l, l + 64, ... of each row (32 weights of one block: one absmax), sums their products unscaled and scales once.
// A wave works through U such units one after the other, the next pieces loading under the current step's arithmetic, so the staging is paid once per
// 4 U RW rows (RW = U = 2: the fastest of the mappings measured on the four Vicuna-7B shapes, docs/LOG.md §15.2).
// The input row is staged once per workgroup in LDS, gamma applied, transposed so that the eight 16-byte reads of a lane's 32 inputs are contiguous across
// the wave (chunk of 2048 floats: [8][64 lanes][4]). Codes are decoded two at a time through a 256-entry LDS table of float pairs indexed by the byte.
template <int EPI>
__global__ __launch_bounds__(256) void llm_gemv_q4_kernel(LlmGemv a, LlmQ4 q) {
  constexpr int RW = Q4_RW, U = Q4_U;
  extern __shared__ float q4_sm[];
  f2* tab = (f2*)q4_sm;               // [256]
  float* red = q4_sm + 512;           // [4]
  float* xs = q4_sm + 512 + 4;        // [chunks][8][64][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, pieces = K >> 5, nit = (pieces + 63) >> 6;
  const int unit0 = ((int)blockIdx.x * 4 + wave) * U;
  auto row_of = [&](int unit, int r) {
    if (EPI == EPI_QKV) { const int pidx = min(unit, a.N / 2 - 1); return (pidx >> 6) * 128 + (pidx & 63) + 64 * r; }
    if (EPI == EPI_SWIGLU) return min(unit, a.N / 2 - 1) + r * (a.N / 2);
    return min(unit * RW + r, a.N - 1);
  };
  auto fetch = [&](int unit, int it, u4v* w, float* am) {
    const int p = min(it * 64 + lane, pieces - 1);
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const size_t row = (size_t)row_of(unit, r);
      w[r] = __builtin_nontemporal_load(q.Wq + row * pieces + p);
      am[r] = q.absmax[row * (K >> 6) + (p >> 1)];
    }
  };
  // the first pieces are on their way while the input row is staged
  u4v w[RW], wn[RW];
  float am[RW], amn[RW];
  fetch(unit0, 0, w, am);
  tab[tid] = f2{q.cb.v[tid & 15], q.cb.v[tid >> 4]};
  float ss = 0.f;
  for (int i = tid; i < (K >> 2); i += 256) {
    f4 x = ((const f4*)a.X)[i];
    if (a.gamma) {
      const h4 g = ((const h4*)a.gamma)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) { ss = fmaf(x[e], x[e], ss); x[e] *= (float)g[e]; }
    }
    const int p = i >> 3, j = i & 7;
    *(f4*)(xs + ((((p >> 6) << 3) + j) << 8) + ((p & 63) << 2)) = x;
  }
  ss = wave_sum(ss);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  float rstd = 1.f;
  if (a.gamma) rstd = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)K + a.eps);
#pragma unroll 1
  for (int u = 0; u < U; ++u) {
    const int unit = unit0 + u;
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.f;
    for (int it = 0; it < nit; ++it) {
      const bool more = it + 1 < nit || u + 1 < U;     // the next pieces (of this unit or the wave's next one) load under this step's arithmetic
      if (more) fetch(it + 1 < nit ? unit : unit + 1, it + 1 < nit ? it + 1 : 0, wn, amn);
      if (it * 64 + lane < pieces) {
        f4 x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = *(const f4*)(xs + (((it << 3) + j) << 8) + (lane << 2));
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          f2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
#pragma unroll
          for (int h = 0; h < 2; ++h) {         // half a piece at a time: its 8 table reads are issued together, then consumed
            f2 t[8];
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
              for (int b = 0; b < 4; ++b) t[4 * k + b] = tab[(w[r][2 * h + k] >> (8 * b)) & 255];
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
              for (int b = 0; b < 4; b += 2) {
                const f4 xv = x[4 * h + 2 * k + (b >> 1)];
                s0 = __builtin_elementwise_fma(t[4 * k + b], f2{xv[0], xv[1]}, s0);
                s1 = __builtin_elementwise_fma(t[4 * k + b + 1], f2{xv[2], xv[3]}, s1);
              }
          }
          const f2 s = s0 + s1;
          acc[r] = fmaf(s[0] + s[1], am[r], acc[r]);
        }
      }
      if (more) {
#pragma unroll
        for (int r = 0; r < RW; ++r) { w[r] = wn[r]; am[r] = amn[r]; }
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = wave_sum(acc[r]) * rstd;
    if (EPI == EPI_PLAIN || EPI == EPI_RESID) {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int n = unit * RW + r;
        if (lane == r && n < a.N) a.out[n] = EPI == EPI_RESID ? a.out[n] + acc[r] : acc[r];
      }
    } else if (lane == 0 && unit < a.N / 2) {
      if (EPI == EPI_SWIGLU) a.out[unit] = acc[0] / (1.0f + expf(-acc[0])) * acc[RW - 1];
      else llm_store_qkv_pair(a, unit, acc[0], acc[RW - 1]);
    }
  }
  if (EPI == EPI_PLAIN && a.hid && a.gamma && blockIdx.x == 0)
    for (int i = tid; i < K; i += 256) a.hid[i] = a.X[i] * rstd * (float)a.gamma[i];
}

static size_t q4_gemv_lds(int K) { return (size_t)(512 + 4 + (((K >> 5) + 63) >> 6) * 2048) * sizeof(float); }
static hipError_t llm_launch_gemv_q4(const LlmGemv& a, const LlmQ4& q, int epi, hipStream_t s) {
  if (!q.Wq || !q.absmax || !a.X || a.N < 1 || a.K < 64 || a.K % 64 || a.K > Q4_MAX_K) return hipErrorInvalidValue;
  if ((epi == EPI_QKV && (a.N != 3 * a.H || a.H % 128)) || (epi == EPI_SWIGLU && a.N % 2)) return hipErrorInvalidValue;
  const int units = epi == EPI_QKV || epi == EPI_SWIGLU ? a.N / 2 : (a.N + Q4_RW - 1) / Q4_RW;
  const dim3 grid((units + 4 * Q4_U - 1) / (4 * Q4_U)), block(256);
  const size_t lds = q4_gemv_lds(a.K);
  switch (epi) {
    case EPI_PLAIN: hipLaunchKernelGGL((llm_gemv_q4_kernel<EPI_PLAIN>), grid, block, lds, s, a, q); break;
    case EPI_RESID: hipLaunchKernelGGL((llm_gemv_q4_kernel<EPI_RESID>), grid, block, lds, s, a, q); break;
    case EPI_QKV: hipLaunchKernelGGL((llm_gemv_q4_kernel<EPI_QKV>), grid, block, lds, s, a, q); break;
    case EPI_SWIGLU: hipLaunchKernelGGL((llm_gemv_q4_kernel<EPI_SWIGLU>), grid, block, lds, s, a, q); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
// sorted codebook -> thresholds and the code at each sorted position (equal values keep their code order)
static Q4Thresholds q4_thresholds(const float* cb) {
  int idx[16];
  for (int i = 0; i < 16; ++i) idx[i] = i;
  std::stable_sort(idx, idx + 16, [&](int x, int y) { return cb[x] < cb[y]; });
  Q4Thresholds t{};
  for (int i = 0; i < 15; ++i) t.thr[i] = (cb[idx[i]] + cb[idx[i + 1]]) / 2.0f;
  for (int i = 0; i < 16; ++i) t.code_at |= (unsigned long long)idx[i] << (4 * i);
  return t;
}
static hipError_t llm_launch_quantize_q4(const half_t* W, size_t elems, const float* cb, void* packed, float* absmax, hipStream_t s) {
  const long n8 = (long)(elems / 8);
  hipLaunchKernelGGL(llm_quantize_q4_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, W, n8, q4_thresholds(cb), (unsigned*)packed, absmax);
  return hipGetLastError();
}
static hipError_t llm_launch_dequantize_q4(const void* packed, const float* absmax, size_t elems, const float* cb, half_t* W, hipStream_t s) {
  const long n8 = (long)(elems / 8);
  Q4Codebook c;
  memcpy(c.v, cb, sizeof c.v);
  hipLaunchKernelGGL(llm_dequantize_q4_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, (const unsigned*)packed, absmax, n8, c, W);
  return hipGetLastError();
}
static size_t attn_lds(int nk) { return ((size_t)((nk + 3) & ~3) + 16 * 128 + 8) * sizeof(float); }
constexpr int LLM_MAX_POSITIONS = 8192;       // scores of one query row live in LDS (32 KiB of the 64)

// =====================================================================================================================
// Up to IA2P_LLM_MAX_ROWS sequences per weight pass (ia2p_llm_decode_batch). The kernels above serve one input row; the three below read (in 4 bits:
// decode) every weight once and apply it to M input rows, each row at its own position and in its own cache slot. A row's arithmetic never involves
// another row and keeps the single-row kernel's order of operations, so row m of a launch equals the single-row launch on that row bit for bit:
//   llm_gemv_rows_kernel     thread t walks pieces t, t + 256, ... of K; per piece the same fmaf chain; the four waves' partials meet in LDS in wave order
//   llm_gemv_q4_rows_kernel  lane l takes pieces l, l + 64, ... (32 weights, one absmax); the same s0 / s1 packed-FMA order, fmaf(sum, absmax, acc) per
//                            block, wave_sum, rstd afterwards
//   llm_attn_rows_kernel     llm_attn_kernel's algorithm on grid (heads, rows); row r reads the cache of its slot up to its own position
// The tails the compiler contracts in the single-row kernels (out[n] + sum * rstd -> one fma) are written as fmaf here, so they do not depend on what
// the compiler decides per kernel. Everything stays on VALU in fp32 (the residual stream of a decoded row is fp32).
// The per-row pointers and positions travel by value in the kernel arguments: a decode step copies nothing to the device.
// MT = rows a launch computes (1, 2, 4 or 8: M rounded up; the host repeats row M - 1 in the unused entries and the kernel stores rows m < M only).
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
__device__ __forceinline__ LlmGemv llm_row_view(const LlmGemv& a, const LlmRows& b, int m) {
  LlmGemv v = a;
  v.pos = b.pos[m]; v.q = b.q[m]; v.kc = b.kc[m]; v.vc = b.vc[m];
  return v;
}

// `a` carries what the rows share (W, gamma, eps, N, K, inv_freq, H); R weight rows per workgroup as in llm_gemv_kernel (R does not enter a row's arithmetic)
template <int R, int EPI, int MT>
__global__ __launch_bounds__(256) void llm_gemv_rows_kernel(LlmGemv a, LlmRows b) {
  __shared__ float red[4][MT][R + 1];
  constexpr int HR = R / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  int rows[R];
  if (EPI == EPI_QKV) {
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      const int pidx = min((int)blockIdx.x * HR + i, a.N / 2 - 1);
      rows[i] = (pidx >> 6) * 128 + (pidx & 63);
      rows[i + HR] = rows[i] + 64;
    }
  } else if (EPI == EPI_SWIGLU) {
#pragma unroll
    for (int i = 0; i < HR; ++i) {
      rows[i] = min((int)blockIdx.x * HR + i, a.N / 2 - 1);
      rows[i + HR] = a.N / 2 + rows[i];
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) rows[r] = min((int)blockIdx.x * R + r, a.N - 1);
  }
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
      if (tid < R && n < a.N) b.out[m][n] = EPI == EPI_RESID ? fmaf(rstd, sum4(tid), b.out[m][n]) : sum4(tid) * rstd;
      if (EPI == EPI_PLAIN && b.hid[m] && a.gamma && blockIdx.x == 0)
        for (int i = tid; i < K; i += 256) b.hid[m][i] = b.X[m][i] * rstd * (float)a.gamma[i];
    } else if (EPI == EPI_SWIGLU) {
      const int i = (int)blockIdx.x * HR + tid;
      if (tid < HR && i < a.N / 2) {
        const float g = sum4(tid) * rstd, u = sum4(tid + HR) * rstd;
        b.out[m][i] = g / (1.0f + expf(-g)) * u;
      }
    } else {
      const int pidx = (int)blockIdx.x * HR + tid;
      if (tid < HR && pidx < a.N / 2) llm_store_qkv_pair(llm_row_view(a, b, m), pidx, sum4(tid) * rstd, sum4(tid + HR) * rstd);
    }
  }
}

// The 4-bit GEMV for M rows. Units, pieces and the per-piece arithmetic are llm_gemv_q4_kernel's: a wave owns U units of RW = 2 weight rows, lane l takes
// pieces l, l + 64, ... of each. M input rows do not fit LDS whole (a row is 16 KiB at K = 4096, 43 KiB at K = 11008), so K is staged a chunk at a time: chunk
// `it` = the 2048 inputs of every row that step `it` of the lanes consumes ([MT][8][64 lanes][4] floats, gamma applied), 64 KiB at MT = 8. Per chunk a wave
// decodes the two pieces of a unit once into registers (the same byte table) and applies them to each of the MT rows in turn, so the table reads, the
// shifts and the absmax fetch are paid once per code instead of once per code and row; the U RW MT sums stay in registers across the chunks, each
// receiving its fmaf(sum, absmax, acc) in step order as in the single-row kernel. The next chunk's pieces load under the current chunk's arithmetic.
// sum x^2 of a row: thread t adds float4s t, t + 256, ... of the row in that order, across the chunks -- the single-row kernel's order.
constexpr int Q4R_U = 2;
template <int EPI, int MT>
__global__ __launch_bounds__(256, 2) void llm_gemv_q4_rows_kernel(LlmGemv a, LlmQ4 q, LlmRows b) {
  constexpr int RW = Q4_RW, U = Q4R_U;
  extern __shared__ float q4r_sm[];
  f2* tab = (f2*)q4r_sm;                 // [256]
  float* red = q4r_sm + 512;             // [4][MT]
  float* xs = q4r_sm + 512 + 4 * MT;     // [MT][8][64][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, pieces = K >> 5, nit = (pieces + 63) >> 6;
  const int unit0 = ((int)blockIdx.x * 4 + wave) * U;
  auto row_of = [&](int unit, int r) {
    if (EPI == EPI_QKV) { const int pidx = min(unit, a.N / 2 - 1); return (pidx >> 6) * 128 + (pidx & 63) + 64 * r; }
    if (EPI == EPI_SWIGLU) return min(unit, a.N / 2 - 1) + r * (a.N / 2);
    return min(unit * RW + r, a.N - 1);
  };
  auto fetch = [&](int it, u4v (*w)[RW], float (*am)[RW]) {
    const int p = min(it * 64 + lane, pieces - 1);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const size_t row = (size_t)row_of(unit0 + u, r);
        w[u][r] = __builtin_nontemporal_load(q.Wq + row * pieces + p);
        am[u][r] = q.absmax[row * (K >> 6) + (p >> 1)];
      }
  };
  u4v w[U][RW], wn[U][RW];
  float am[U][RW], amn[U][RW];
  fetch(0, w, am);
  tab[tid] = f2{q.cb.v[tid & 15], q.cb.v[tid >> 4]};
  float ss[MT], acc[U][RW][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    ss[m] = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < RW; ++r) acc[u][r][m] = 0.f;
  }
#pragma unroll 1
  for (int it = 0; it < nit; ++it) {
    if (it) __syncthreads();              // every wave is done with the previous chunk
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int i = it * 512 + ii * 256 + tid;      // float4 index in the row
      if (i < (K >> 2)) {
        h4 g;
        if (a.gamma) g = ((const h4*)a.gamma)[i];
        const int p = i >> 3, j = i & 7;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          f4 x = ((const f4*)b.X[m])[i];
          if (a.gamma) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { ss[m] = fmaf(x[e], x[e], ss[m]); x[e] *= (float)g[e]; }
          }
          *(f4*)(xs + (m << 11) + (j << 8) + ((p & 63) << 2)) = x;
        }
      }
    }
    __syncthreads();
    const bool more = it + 1 < nit;
    if (more) fetch(it + 1, wn, amn);
    if (it * 64 + lane < pieces) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        f2 t[RW][16];                     // the unit's two pieces, decoded once
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) t[r][4 * k + c] = tab[(w[u][r][k] >> (8 * c)) & 255];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          f4 x[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = *(const f4*)(xs + (m << 11) + (j << 8) + (lane << 2));
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            f2 s0 = {0.f, 0.f}, s1 = {0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k)         // word k of the piece: bytes 0..3 against inputs 8 k .. 8 k + 7 (the single-row kernel's order)
#pragma unroll
              for (int c = 0; c < 4; c += 2) {
                const f4 xv = x[2 * k + (c >> 1)];
                s0 = __builtin_elementwise_fma(t[r][4 * k + c], f2{xv[0], xv[1]}, s0);
                s1 = __builtin_elementwise_fma(t[r][4 * k + c + 1], f2{xv[2], xv[3]}, s1);
              }
            const f2 s = s0 + s1;
            acc[u][r][m] = fmaf(s[0] + s[1], am[u][r], acc[u][r][m]);
          }
          __builtin_amdgcn_sched_barrier(0);      // one row's 32 inputs live at a time: hoisting the next rows' LDS reads costs more registers than two workgroups per CU leave
        }
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < RW; ++r) { w[u][r] = wn[u][r]; am[u][r] = amn[u][r]; }
    }
  }
  float rstd[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    ss[m] = wave_sum(ss[m]);
    if (lane == 0) red[wave * MT + m] = ss[m];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    rstd[m] = 1.f;
    if (a.gamma) rstd[m] = 1.0f / sqrtf(((red[m] + red[MT + m]) + (red[2 * MT + m] + red[3 * MT + m])) / (float)K + a.eps);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int unit = unit0 + u;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float v[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) v[r] = wave_sum(acc[u][r][m]);
      if (m >= b.M) continue;
      if (EPI == EPI_PLAIN || EPI == EPI_RESID) {
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          const int n = unit * RW + r;
          if (lane == r && n < a.N) b.out[m][n] = EPI == EPI_RESID ? fmaf(v[r], rstd[m], b.out[m][n]) : v[r] * rstd[m];
        }
      } else if (lane == 0 && unit < a.N / 2) {
        const float y0 = v[0] * rstd[m], y1 = v[RW - 1] * rstd[m];
        if (EPI == EPI_SWIGLU) b.out[m][unit] = y0 / (1.0f + expf(-y0)) * y1;
        else llm_store_qkv_pair(llm_row_view(a, b, m), unit, y0, y1);
      }
    }
  }
  if (EPI == EPI_PLAIN && a.gamma && blockIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < b.M && b.hid[m])
        for (int i = tid; i < K; i += 256) b.hid[m][i] = b.X[m][i] * rstd[m] * (float)a.gamma[i];
  }
}

// llm_attn_kernel for one decoded row per sequence: row r = blockIdx.y against the keys 0 .. pos[r] of its own cache slot
struct LlmAttnRows {
  const half_t* kc[LLM_MAX_ROWS];
  const half_t* vc[LLM_MAX_ROWS];
  int pos[LLM_MAX_ROWS];
};
__global__ __launch_bounds__(256) void llm_attn_rows_kernel(const float* q, LlmAttnRows rows, float* out, int H, float scale) {
  extern __shared__ float llm_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 4, l = tid & 15;
  const int head = blockIdx.x, t = blockIdx.y, nk = rows.pos[t] + 1;
  const half_t* kc = rows.kc[t];
  const half_t* vc = rows.vc[t];
  float* sc = llm_sm;                 // [nk]
  float* part = llm_sm + ((nk + 3) & ~3);   // [16][128]
  float* red = part + 16 * 128;       // [8]
  float qv[8];
  {
    const float* qp = q + (size_t)t * H + head * 128 + l * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = qp[e] * scale;
  }
  for (int j0 = 0; j0 < nk; j0 += 16) {
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
    out[(size_t)t * H + head * 128 + tid] = r / sum;
  }
}
// token rows of the embedding table as fp32: row r = blockIdx.y, the ids by value
struct LlmTokRows { int id[LLM_MAX_ROWS]; };
__global__ __launch_bounds__(256) void llm_rows_f32_kernel(const half_t* tok, LlmTokRows ids, float* dst, int H) {
  const half_t* src = tok + (size_t)ids.id[blockIdx.y] * H;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H; i += gridDim.x * 256) dst[(size_t)blockIdx.y * H + i] = (float)src[i];
}

static int rows_mt(int M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8; }
static void rows_pad(LlmRows& b) {      // entries M .. 7 repeat row M - 1: loaded and computed where MT > M, never stored
  for (int m = b.M; m < LLM_MAX_ROWS; ++m) {
    b.X[m] = b.X[b.M - 1]; b.out[m] = b.out[b.M - 1]; b.hid[m] = b.hid[b.M - 1]; b.q[m] = b.q[b.M - 1];
    b.kc[m] = b.kc[b.M - 1]; b.vc[m] = b.vc[b.M - 1]; b.pos[m] = b.pos[b.M - 1];
  }
}
template <int R, int MT>
static hipError_t gemv_rows_launch_r(const LlmGemv& a, const LlmRows& b, int epi, hipStream_t s) {
  const int units = epi == EPI_QKV || epi == EPI_SWIGLU ? (a.N / 2 + R / 2 - 1) / (R / 2) : (a.N + R - 1) / R;
  switch (epi) {
    case EPI_PLAIN: hipLaunchKernelGGL((llm_gemv_rows_kernel<R, EPI_PLAIN, MT>), dim3(units), dim3(256), 0, s, a, b); break;
    case EPI_RESID: hipLaunchKernelGGL((llm_gemv_rows_kernel<R, EPI_RESID, MT>), dim3(units), dim3(256), 0, s, a, b); break;
    case EPI_QKV: hipLaunchKernelGGL((llm_gemv_rows_kernel<R, EPI_QKV, MT>), dim3(units), dim3(256), 0, s, a, b); break;
    case EPI_SWIGLU: hipLaunchKernelGGL((llm_gemv_rows_kernel<R, EPI_SWIGLU, MT>), dim3(units), dim3(256), 0, s, a, b); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
// weight rows per workgroup: llm_launch_gemv's rule for one or two input rows; from four input rows on always 8, because every workgroup reads all the
// input rows (4 M K bytes from L2 against 2 R K bytes of weights) and more weight rows per workgroup halve that share
static hipError_t llm_launch_gemv_rows(const LlmGemv& a, LlmRows b, int epi, hipStream_t s) {
  if (!a.W || b.M < 1 || b.M > LLM_MAX_ROWS || a.N < 1 || a.K < 8 || a.K % 8) return hipErrorInvalidValue;
  if ((epi == EPI_QKV && (a.N != 3 * a.H || a.H % 128)) || (epi == EPI_SWIGLU && a.N % 2)) return hipErrorInvalidValue;
  rows_pad(b);
  const bool r8 = a.N >= 8192;
  switch (rows_mt(b.M)) {
    case 1: return r8 ? gemv_rows_launch_r<8, 1>(a, b, epi, s) : gemv_rows_launch_r<4, 1>(a, b, epi, s);
    case 2: return r8 ? gemv_rows_launch_r<8, 2>(a, b, epi, s) : gemv_rows_launch_r<4, 2>(a, b, epi, s);
    case 4: return gemv_rows_launch_r<8, 4>(a, b, epi, s);
    default: return gemv_rows_launch_r<8, 8>(a, b, epi, s);
  }
}
static size_t q4_rows_lds(int mt) { return (size_t)(512 + 4 * mt + mt * 2048) * sizeof(float); }
template <int MT>
static hipError_t gemv_q4_rows_launch(const LlmGemv& a, const LlmQ4& q, const LlmRows& b, int epi, hipStream_t s) {
  const int units = epi == EPI_QKV || epi == EPI_SWIGLU ? a.N / 2 : (a.N + Q4_RW - 1) / Q4_RW;
  const dim3 grid((units + 4 * Q4R_U - 1) / (4 * Q4R_U)), block(256);
  const size_t lds = q4_rows_lds(MT);
  if (lds > 64 * 1024) {          // MT = 8: 66 KiB of the CU's 160
    static bool done = false;
    if (!done) {
      hipError_t e = hipFuncSetAttribute((const void*)llm_gemv_q4_rows_kernel<EPI_PLAIN, MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)llm_gemv_q4_rows_kernel<EPI_RESID, MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)llm_gemv_q4_rows_kernel<EPI_QKV, MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void*)llm_gemv_q4_rows_kernel<EPI_SWIGLU, MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      done = true;
    }
  }
  switch (epi) {
    case EPI_PLAIN: hipLaunchKernelGGL((llm_gemv_q4_rows_kernel<EPI_PLAIN, MT>), grid, block, lds, s, a, q, b); break;
    case EPI_RESID: hipLaunchKernelGGL((llm_gemv_q4_rows_kernel<EPI_RESID, MT>), grid, block, lds, s, a, q, b); break;
    case EPI_QKV: hipLaunchKernelGGL((llm_gemv_q4_rows_kernel<EPI_QKV, MT>), grid, block, lds, s, a, q, b); break;
    case EPI_SWIGLU: hipLaunchKernelGGL((llm_gemv_q4_rows_kernel<EPI_SWIGLU, MT>), grid, block, lds, s, a, q, b); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
static hipError_t llm_launch_gemv_q4_rows(const LlmGemv& a, const LlmQ4& q, LlmRows b, int epi, hipStream_t s) {
  if (!q.Wq || !q.absmax || b.M < 1 || b.M > LLM_MAX_ROWS || a.N < 1 || a.K < 64 || a.K % 64 || a.K > Q4_MAX_K) return hipErrorInvalidValue;
  if ((epi == EPI_QKV && (a.N != 3 * a.H || a.H % 128)) || (epi == EPI_SWIGLU && a.N % 2)) return hipErrorInvalidValue;
  rows_pad(b);
  switch (rows_mt(b.M)) {
    case 1: return gemv_q4_rows_launch<1>(a, q, b, epi, s);
    case 2: return gemv_q4_rows_launch<2>(a, q, b, epi, s);
    case 4: return gemv_q4_rows_launch<4>(a, q, b, epi, s);
    default: return gemv_q4_rows_launch<8>(a, q, b, epi, s);
  }
}

struct LLayer { size_t ln1, ln2, wqkv, wo, wgu, wd; size_t aqkv, ao, agu, ad; };      // a*: the absmax arrays of the 4-bit format (w*: the packed codes then)
struct ia2p_llm : RunCtx {
  ia2p_llm_config cfg;
  size_t tok, normf, head, invf;
  std::vector<LLayer> layers;
  half_t* kv = nullptr;                                // [slot][layer][k|v][max_pos][hidden]
  int max_pos = 0, n_slots = 0, cur = 0;               // cur: the slot the single-sequence paths (prefill, decode) act on
  std::vector<int> spos{0};                            // position of every slot
  int wbits = 16;                                      // 16: fp16 projections; 4: codes of `codebook`, block 64, fp32 absmax (ia2p_llm_set_weight_format)
  float codebook[16] = {};
  std::unordered_map<std::string, size_t> q4_absmax;   // projection key -> offset of its absmax rows (arena elements)
};
// arena elements (2 bytes each) of a quantised [N, K]: packed codes, absmax
static size_t q4_code_elems(size_t nk) { return nk / 4; }
static size_t q4_absmax_elems(size_t nk) { return nk / 64 * 2; }

static ia2p_status llm_plan(ia2p_llm* c) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size;
  if (g.num_layers < 1 || g.num_heads < 1 || g.vocab_size < 1 || H < 128 || I < 64)
    return fail(c, IA2P_ERR_INVALID, "llm: layers %d, heads %d, vocabulary %d, hidden %d, intermediate %d", g.num_layers, g.num_heads, g.vocab_size, H, I);
  if (H % 64 || g.num_heads * 128 != H) return fail(c, IA2P_ERR_SHAPE, "llm: hidden %d must be a multiple of 64 and heads (%d) * 128 (head dim 128 only)", H, g.num_heads);
  if (g.num_kv_heads != g.num_heads) return fail(c, IA2P_ERR_SHAPE, "llm: %d key/value heads for %d heads (grouped-query attention is not built)", g.num_kv_heads, g.num_heads);
  if (I % 64) return fail(c, IA2P_ERR_SHAPE, "llm: intermediate %d must be a multiple of 64", I);
  const bool q4 = c->wbits == 4;
  if (q4 && (H > Q4_MAX_K || I > Q4_MAX_K)) return fail(c, IA2P_ERR_SHAPE, "llm: 4-bit weights serve rows of up to %d (hidden %d, intermediate %d)", Q4_MAX_K, H, I);
  c->params.clear(); c->layers.clear(); c->q4_absmax.clear();
  size_t cur = 0;
  auto take = [&](size_t e) { size_t o = cur; cur += (e + 127) & ~(size_t)127; return o; };
  auto reg = [&](const std::string& k, size_t off, size_t n) { c->params[k] = Param{off, n, PK_COPY, 0, 0, false, false}; };
  auto par = [&](const std::string& k, size_t n) { size_t o = take(n); reg(k, o, n); return o; };
  c->tok = par("model.embed_tokens.weight", (size_t)g.vocab_size * H);
  for (int i = 0; i < g.num_layers; ++i) {
    const std::string p = "model.layers." + std::to_string(i) + ".";
    LLayer l;
    l.ln1 = par(p + "input_layernorm.weight", H);
    // a projection of `parts` equal [rows, K] tensors stacked as rows (blocks never cross a row, so in 4 bits the codes and the absmax rows stack the same way)
    auto proj = [&](size_t* w, size_t* am, const std::vector<std::string>& keys, size_t rows, size_t K) {
      const size_t nk = rows * K, parts = keys.size();
      *w = take(q4 ? q4_code_elems(parts * nk) : parts * nk);
      *am = q4 ? take(q4_absmax_elems(parts * nk)) : 0;
      for (size_t j = 0; j < parts; ++j) {
        if (!q4) { reg(p + keys[j], *w + j * nk, nk); continue; }
        c->params[p + keys[j]] = Param{*w + j * q4_code_elems(nk), nk, PK_Q4, (int)rows, (int)K, false, false};
        c->q4_absmax[p + keys[j]] = *am + j * q4_absmax_elems(nk);
      }
    };
    proj(&l.wqkv, &l.aqkv, {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"}, H, H);     // q | k | v rows stacked: one projection
    proj(&l.wo, &l.ao, {"self_attn.o_proj.weight"}, H, H);
    l.ln2 = par(p + "post_attention_layernorm.weight", H);
    proj(&l.wgu, &l.agu, {"mlp.gate_proj.weight", "mlp.up_proj.weight"}, I, H);                                              // gate | up rows stacked
    proj(&l.wd, &l.ad, {"mlp.down_proj.weight"}, H, I);
    c->layers.push_back(l);
  }
  c->normf = par("model.norm.weight", H);
  c->head = par("lm_head.weight", (size_t)g.vocab_size * H);
  c->invf = take(128);                                      // 64 fp32 rotary frequencies (derived at finalize)
  c->arena_elems = cur;
  return IA2P_OK;
}

static half_t* KCS(ia2p_llm* c, int slot, int layer) { return c->kv + ((size_t)slot * c->cfg.num_layers + layer) * 2 * c->max_pos * c->cfg.hidden_size; }
static half_t* VCS(ia2p_llm* c, int slot, int layer) { return KCS(c, slot, layer) + (size_t)c->max_pos * c->cfg.hidden_size; }
static half_t* KC(ia2p_llm* c, int layer) { return KCS(c, c->cur, layer); }
static half_t* VC(ia2p_llm* c, int layer) { return VCS(c, c->cur, layer); }
static int& POS(ia2p_llm* c) { return c->spos[c->cur]; }

// final norm + lm_head of the fp32 row xf: hidden_out [H] fp32, logits_out [vocab] fp32
static void llm_head(ia2p_llm* c, const float* xf, float* hidden_out, float* logits_out) {
  LlmGemv a{};
  a.W = W_(c, c->head); a.X = xf; a.gamma = W_(c, c->normf); a.eps = c->cfg.rms_norm_eps; a.N = c->cfg.vocab_size; a.K = c->cfg.hidden_size;
  a.out = logits_out; a.hid = hidden_out;
  CHECK_LAUNCH(c, llm_launch_gemv(a, EPI_PLAIN, c->stream), "llm lm_head");
}

// one decode projection on the context's weight format
static hipError_t llm_proj_gemv(ia2p_llm* c, LlmGemv& a, size_t w, size_t am, int epi) {
  if (c->wbits != 4) { a.W = W_(c, w); return llm_launch_gemv(a, epi, c->stream); }
  LlmQ4 q;
  q.Wq = (const u4v*)W_(c, w); q.absmax = (const float*)W_(c, am);
  memcpy(q.cb.v, c->codebook, sizeof q.cb.v);
  return llm_launch_gemv_q4(a, q, epi, c->stream);
}
// a prefill projection's fp16 weights: the arena's, or (4 bits) dequantised into `scratch` in front of the GEMM that reads them
static const half_t* llm_proj_f16(ia2p_llm* c, size_t w, size_t am, size_t elems, T2 scratch, const char* what) {
  if (c->wbits != 4) return W_(c, w);
  CHECK_LAUNCH(c, llm_launch_dequantize_q4(W_(c, w), (const float*)W_(c, am), elems, c->codebook, scratch.p, c->stream), what);
  return scratch.p;
}

static ia2p_status llm_run_decode(ia2p_llm* c, int token, float* hidden_out, float* logits_out) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size, pos = POS(c);
  T2 xt = wsalloc(c, (size_t)2 * H), qt = wsalloc(c, (size_t)2 * H), at = wsalloc(c, (size_t)2 * H), ft = wsalloc(c, (size_t)2 * I);
  float *xf = (float*)xt.p, *qf = (float*)qt.p, *af = (float*)at.p, *ff = (float*)ft.p;
  if (!c->dry && !c->failed) {
    const half_t* src = W_(c, c->tok) + (size_t)token * H;
    hipLaunchKernelGGL(llm_row_f32_kernel, dim3((H + 255) / 256), dim3(256), 0, c->stream, src, xf, H);
    CHECK_LAUNCH(c, hipGetLastError(), "llm embedding row");
  }
  for (int i = 0; i < g.num_layers; ++i) {
    const LLayer& l = c->layers[i];
    if (c->dry || c->failed) break;
    LlmGemv a{};
    a.X = xf; a.gamma = W_(c, l.ln1); a.eps = g.rms_norm_eps; a.N = 3 * H; a.K = H; a.H = H; a.pos = pos;
    a.inv_freq = (const float*)W_(c, c->invf); a.q = qf; a.kc = KC(c, i); a.vc = VC(c, i);
    CHECK_LAUNCH(c, llm_proj_gemv(c, a, l.wqkv, l.aqkv, EPI_QKV), "llm qkv");
    hipLaunchKernelGGL(llm_attn_kernel<float>, dim3(g.num_heads, 1), dim3(256), attn_lds(pos + 1), c->stream, (const float*)qf, (const half_t*)KC(c, i), (const half_t*)VC(c, i), af, H, pos,
                       0.08838834764831845f);
    CHECK_LAUNCH(c, hipGetLastError(), "llm attention");
    LlmGemv o{};
    o.X = af; o.N = H; o.K = H; o.out = xf;
    CHECK_LAUNCH(c, llm_proj_gemv(c, o, l.wo, l.ao, EPI_RESID), "llm o_proj");
    LlmGemv u{};
    u.X = xf; u.gamma = W_(c, l.ln2); u.eps = g.rms_norm_eps; u.N = 2 * I; u.K = H; u.out = ff;
    CHECK_LAUNCH(c, llm_proj_gemv(c, u, l.wgu, l.agu, EPI_SWIGLU), "llm gate/up");
    LlmGemv d{};
    d.X = ff; d.N = H; d.K = I; d.out = xf;
    CHECK_LAUNCH(c, llm_proj_gemv(c, d, l.wd, l.ad, EPI_RESID), "llm down_proj");
  }
  if (!c->dry) llm_head(c, xf, hidden_out, logits_out);
  wsfree(c, ft); wsfree(c, at); wsfree(c, qt); wsfree(c, xt);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

// one decode projection for the rows of `b`
static hipError_t llm_proj_gemv_rows(ia2p_llm* c, LlmGemv& a, const LlmRows& b, size_t w, size_t am, int epi) {
  if (c->wbits != 4) { a.W = W_(c, w); return llm_launch_gemv_rows(a, b, epi, c->stream); }
  LlmQ4 q;
  q.Wq = (const u4v*)W_(c, w); q.absmax = (const float*)W_(c, am);
  memcpy(q.cb.v, c->codebook, sizeof q.cb.v);
  return llm_launch_gemv_q4_rows(a, q, b, epi, c->stream);
}

// n rows, row r = token tokens[r] at the position of slot slots[r]: the launches of llm_run_decode, each once for all rows
static ia2p_status llm_run_decode_rows(ia2p_llm* c, const int32_t* slots, const int32_t* tokens, int n, float* hidden_out, float* logits_out) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size;
  T2 xt = wsalloc(c, (size_t)2 * n * H), qt = wsalloc(c, (size_t)2 * n * H), at = wsalloc(c, (size_t)2 * n * H), ft = wsalloc(c, (size_t)2 * n * I);
  float *xf = (float*)xt.p, *qf = (float*)qt.p, *af = (float*)at.p, *ff = (float*)ft.p;
  if (!c->dry && !c->failed) {
    LlmTokRows ids{};
    int longest = 0;
    for (int r = 0; r < n; ++r) { ids.id[r] = tokens[r]; longest = std::max(longest, c->spos[slots[r]] + 1); }
    hipLaunchKernelGGL(llm_rows_f32_kernel, dim3((H + 255) / 256, n), dim3(256), 0, c->stream, W_(c, c->tok), ids, xf, H);
    CHECK_LAUNCH(c, hipGetLastError(), "llm embedding rows");
    auto rows = [&](const float* x, size_t xs, float* out, size_t os) {
      LlmRows b{};
      b.M = n;
      for (int r = 0; r < n; ++r) { b.X[r] = x + r * xs; b.out[r] = out ? out + r * os : nullptr; }
      return b;
    };
    for (int i = 0; i < g.num_layers && !c->failed; ++i) {
      const LLayer& l = c->layers[i];
      LlmGemv a{};
      a.gamma = W_(c, l.ln1); a.eps = g.rms_norm_eps; a.N = 3 * H; a.K = H; a.H = H; a.inv_freq = (const float*)W_(c, c->invf);
      LlmRows b = rows(xf, H, nullptr, 0);
      LlmAttnRows ar{};
      for (int r = 0; r < n; ++r) {
        b.q[r] = qf + (size_t)r * H; b.kc[r] = KCS(c, slots[r], i); b.vc[r] = VCS(c, slots[r], i); b.pos[r] = c->spos[slots[r]];
        ar.kc[r] = b.kc[r]; ar.vc[r] = b.vc[r]; ar.pos[r] = b.pos[r];
      }
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, a, b, l.wqkv, l.aqkv, EPI_QKV), "llm qkv rows");
      hipLaunchKernelGGL(llm_attn_rows_kernel, dim3(g.num_heads, n), dim3(256), attn_lds(longest), c->stream, (const float*)qf, ar, af, H, 0.08838834764831845f);
      CHECK_LAUNCH(c, hipGetLastError(), "llm attention rows");
      LlmGemv o{};
      o.N = H; o.K = H;
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, o, rows(af, H, xf, H), l.wo, l.ao, EPI_RESID), "llm o_proj rows");
      LlmGemv u{};
      u.gamma = W_(c, l.ln2); u.eps = g.rms_norm_eps; u.N = 2 * I; u.K = H;
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, u, rows(xf, H, ff, I), l.wgu, l.agu, EPI_SWIGLU), "llm gate/up rows");
      LlmGemv d{};
      d.N = H; d.K = I;
      CHECK_LAUNCH(c, llm_proj_gemv_rows(c, d, rows(ff, I, xf, H), l.wd, l.ad, EPI_RESID), "llm down_proj rows");
    }
    LlmGemv h{};          // final norm + lm_head of every row
    h.W = W_(c, c->head); h.gamma = W_(c, c->normf); h.eps = g.rms_norm_eps; h.N = g.vocab_size; h.K = H;
    LlmRows hb = rows(xf, H, logits_out, g.vocab_size);
    for (int r = 0; r < n; ++r) hb.hid[r] = hidden_out + (size_t)r * H;
    CHECK_LAUNCH(c, llm_launch_gemv_rows(h, hb, EPI_PLAIN, c->stream), "llm lm_head rows");
  }
  wsfree(c, ft); wsfree(c, at); wsfree(c, qt); wsfree(c, xt);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

static ia2p_status llm_run_prefill(ia2p_llm* c, const half_t* embeds, int T, float* hidden_out, float* logits_out) {
  const ia2p_llm_config& g = c->cfg;
  const int H = g.hidden_size, I = g.intermediate_size, p0 = POS(c);
  T2 x = wsalloc(c, (size_t)T * H), xn = wsalloc(c, (size_t)T * H), qkv = wsalloc(c, (size_t)T * 3 * H), qt = wsalloc(c, (size_t)T * H * 2);
  T2 att = wsalloc(c, (size_t)T * H), gu = wsalloc(c, (size_t)T * 2 * I), act = wsalloc(c, (size_t)T * I), xt = wsalloc(c, (size_t)2 * H);
  T2 wq{(size_t)-1, nullptr};           // 4 bits: one projection at a time as fp16 (the largest: gate | up)
  if (c->wbits == 4) wq = wsalloc(c, std::max((size_t)3 * H * H, (size_t)2 * I * H));
  float *qf = (float*)qt.p, *xf = (float*)xt.p;
  if (!c->dry && !c->failed) {
    hipError_t e = hipMemcpyAsync(x.p, embeds, (size_t)T * H * sizeof(half_t), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) fail_hip(c, e, "llm prefill");
  }
  for (int i = 0; i < g.num_layers; ++i) {
    const LLayer& l = c->layers[i];
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_rmsnorm_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)x.p, xn.p, W_(c, l.ln1), H, g.rms_norm_eps);
      CHECK_LAUNCH(c, hipGetLastError(), "llm input_layernorm");
    }
    op_gemm(c, xn.p, H, llm_proj_f16(c, l.wqkv, l.aqkv, (size_t)3 * H * H, wq, "llm dequantize qkv"), nullptr, nullptr, 0, qkv.p, 3 * H, T, 3 * H, H);
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_rope_cache_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)qkv.p, qf, KC(c, i), VC(c, i), (const float*)W_(c, c->invf), H, p0);
      CHECK_LAUNCH(c, hipGetLastError(), "llm rope");
      hipLaunchKernelGGL(llm_attn_kernel<half_t>, dim3(g.num_heads, T), dim3(256), attn_lds(p0 + T), c->stream, (const float*)qf, (const half_t*)KC(c, i), (const half_t*)VC(c, i), att.p, H, p0,
                         0.08838834764831845f);
      CHECK_LAUNCH(c, hipGetLastError(), "llm attention");
    }
    op_gemm(c, att.p, H, llm_proj_f16(c, l.wo, l.ao, (size_t)H * H, wq, "llm dequantize o_proj"), nullptr, x.p, H, x.p, H, T, H, H);
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_rmsnorm_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)x.p, xn.p, W_(c, l.ln2), H, g.rms_norm_eps);
      CHECK_LAUNCH(c, hipGetLastError(), "llm post_attention_layernorm");
    }
    op_gemm(c, xn.p, H, llm_proj_f16(c, l.wgu, l.agu, (size_t)2 * I * H, wq, "llm dequantize gate/up"), nullptr, nullptr, 0, gu.p, 2 * I, T, 2 * I, H);
    if (!c->dry && !c->failed) {
      hipLaunchKernelGGL(llm_silu_mul_rows_kernel, dim3(T), dim3(256), 0, c->stream, (const half_t*)gu.p, act.p, I);
      CHECK_LAUNCH(c, hipGetLastError(), "llm silu-multiply");
    }
    op_gemm(c, act.p, I, llm_proj_f16(c, l.wd, l.ad, (size_t)H * I, wq, "llm dequantize down_proj"), nullptr, x.p, H, x.p, H, T, H, I);
  }
  if (!c->dry && !c->failed) {          // only the last row goes through model.norm and lm_head
    hipLaunchKernelGGL(llm_row_f32_kernel, dim3((H + 255) / 256), dim3(256), 0, c->stream, (const half_t*)(x.p + (size_t)(T - 1) * H), xf, H);
    CHECK_LAUNCH(c, hipGetLastError(), "llm last row");
    llm_head(c, xf, hidden_out, logits_out);
  }
  if (c->wbits == 4) wsfree(c, wq);
  wsfree(c, xt); wsfree(c, act); wsfree(c, gu); wsfree(c, att); wsfree(c, qt); wsfree(c, qkv); wsfree(c, xn); wsfree(c, x);
  return c->failed ? IA2P_ERR_HIP : IA2P_OK;
}

static size_t llm_dry(ia2p_llm* c, int T) {
  c->dry = true; c->failed = false; c->record = false;
  c->ws.reset((size_t)1 << 46); c->ws_base = nullptr;
  if (T > 0) (void)llm_run_prefill(c, nullptr, T, nullptr, nullptr);
  else (void)llm_run_decode(c, 0, nullptr, nullptr);
  c->dry = false;
  return c->failed ? 0 : c->ws.high + 256;
}
static size_t llm_dry_rows(ia2p_llm* c, int n) {
  c->dry = true; c->failed = false; c->record = false;
  c->ws.reset((size_t)1 << 46); c->ws_base = nullptr;
  (void)llm_run_decode_rows(c, nullptr, nullptr, n, nullptr, nullptr);
  c->dry = false;
  return c->failed ? 0 : c->ws.high + 256;
}
static ia2p_status llm_ready(ia2p_llm* c, const char* what) {
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "%s before weights were finalized", what);
  if (!c->kv) return fail(c, IA2P_ERR_STATE, "%s before ia2p_llm_bind_kv", what);
  return IA2P_OK;
}
// exact: the batched decode takes `need` as the least size of an aligned workspace (the earlier entry points allow the alignment slack to be missing)
static ia2p_status llm_enter(ia2p_llm* c, void* stream, void* ws, size_t ws_bytes, size_t need, bool exact = false) {
  const uintptr_t base = ((uintptr_t)ws + 255) & ~(uintptr_t)255;
  const size_t lost = base - (uintptr_t)ws;
  if (need == 0 || ws_bytes < lost || ws_bytes - lost + (exact ? 0 : 256) < need) return fail(c, IA2P_ERR_NOMEM, "llm: workspace of %zu bytes, %zu needed", ws_bytes, need);
  c->wseq.clear(); c->widx = 0; c->dry = false; c->failed = false; c->stream = (hipStream_t)stream;
  c->ws.reset(ws_bytes - lost); c->ws_base = (char*)base;
  return IA2P_OK;
}
static ia2p_status llm_leave(ia2p_llm* c, ia2p_status st) {
  if (c->failed && st == IA2P_OK) st = IA2P_ERR_HIP;
  if (c->failed && c->err == "workspace too small") st = IA2P_ERR_NOMEM;
  return st;
}

extern "C" {

ia2p_status ia2p_llm_create(const ia2p_llm_config* cfg, ia2p_llm** out) {
  if (!cfg || !out) return fail(nullptr, IA2P_ERR_INVALID, "ia2p_llm_create: null argument");
  ia2p_llm* c = new ia2p_llm();
  c->cfg = *cfg;
  if (c->cfg.rms_norm_eps <= 0.f) c->cfg.rms_norm_eps = 1e-5f;
  if (c->cfg.rope_theta <= 0.f) c->cfg.rope_theta = 10000.f;
  ia2p_status st = llm_plan(c);
  if (st != IA2P_OK) { g_err = c->err; delete c; *out = nullptr; return st; }
  c->failed = false;
  *out = c;
  return IA2P_OK;
}
void ia2p_llm_destroy(ia2p_llm* c) { delete c; }
const char* ia2p_llm_last_error(ia2p_llm* c) { return c ? c->err.c_str() : g_err.c_str(); }
size_t ia2p_llm_arena_bytes(ia2p_llm* c) { return c ? c->arena_elems * sizeof(half_t) : 0; }
ia2p_status ia2p_llm_bind_arena(ia2p_llm* c, void* dev, size_t bytes) { return rc_bind_arena(c, dev, bytes); }
ia2p_status ia2p_llm_load_tensor(ia2p_llm* c, const char* key, const void* src, const int64_t* shape, int ndim, void* stream) {
  if (!c || !key || !src || !shape || !c->arena) return rc_load_tensor(c, key, src, shape, ndim, stream);      // (its refusals)
  auto it = c->params.find(key);
  if (it == c->params.end() || it->second.kind != PK_Q4) return rc_load_tensor(c, key, src, shape, ndim, stream);
  Param& p = it->second;              // a 4-bit projection: quantised from the fp16 tensor into the arena
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  if (n != p.elems) return fail(c, IA2P_ERR_SHAPE, "parameter '%s': expected %zu elements, got %zu", key, p.elems, n);
  hipError_t e = llm_launch_quantize_q4((const half_t*)src, n, c->codebook, c->arena + p.off, (float*)(c->arena + c->q4_absmax[key]), (hipStream_t)stream);
  if (e != hipSuccess) return fail_hip(c, e, (std::string("quantize '") + key + "'").c_str());
  p.loaded = true;
  return IA2P_OK;
}
ia2p_status ia2p_llm_set_weight_format(ia2p_llm* c, int bits, const float* codebook) {
  if (!c) return fail(nullptr, IA2P_ERR_INVALID, "llm_set_weight_format: null argument");
  if (bits != 16 && bits != 4) return fail(c, IA2P_ERR_INVALID, "llm_set_weight_format: %d bits (16 or 4)", bits);
  if (bits == 4 && !codebook) return fail(c, IA2P_ERR_INVALID, "llm_set_weight_format: 4 bits need a codebook of 16 values");
  if (c->arena) return fail(c, IA2P_ERR_STATE, "llm_set_weight_format after ia2p_llm_bind_arena");
  const int old = c->wbits;
  c->wbits = bits;
  if (bits == 4) memcpy(c->codebook, codebook, sizeof c->codebook);
  const ia2p_status st = llm_plan(c);
  if (st != IA2P_OK) { c->wbits = old; (void)llm_plan(c); c->failed = false; }
  return st;
}
int ia2p_llm_weight_bits(ia2p_llm* c) { return c ? c->wbits : 0; }
size_t ia2p_llm_q4_packed_bytes(int64_t N, int64_t K) { return N < 1 || K < 64 || K % 64 ? 0 : (size_t)N * (size_t)K / 2; }
static ia2p_status q4_op_args(const char* what, const void* a, const void* b, const void* d, const void* cb, int64_t N, int64_t K) {
  if (!a || !b || !d || !cb) return fail(nullptr, IA2P_ERR_INVALID, "%s: null argument", what);
  if (N < 1 || K < 64 || K % 64 || N * K > ((int64_t)1 << 34)) return fail(nullptr, IA2P_ERR_SHAPE, "%s: N=%lld K=%lld (K a multiple of 64)", what, (long long)N, (long long)K);
  return IA2P_OK;
}
ia2p_status ia2p_llm_quantize_q4(void* stream, const void* W, int64_t N, int64_t K, const float* codebook, void* packed, float* absmax) {
  const ia2p_status st = q4_op_args("llm_quantize_q4", W, packed, absmax, codebook, N, K);
  if (st != IA2P_OK) return st;
  hipError_t e = llm_launch_quantize_q4((const half_t*)W, (size_t)(N * K), codebook, packed, absmax, (hipStream_t)stream);
  RET_HIP(e, "llm_quantize_q4");
}
ia2p_status ia2p_llm_dequantize_q4(void* stream, const void* packed, const float* absmax, int64_t N, int64_t K, const float* codebook, void* W) {
  const ia2p_status st = q4_op_args("llm_dequantize_q4", packed, absmax, W, codebook, N, K);
  if (st != IA2P_OK) return st;
  hipError_t e = llm_launch_dequantize_q4(packed, absmax, (size_t)(N * K), codebook, (half_t*)W, (hipStream_t)stream);
  RET_HIP(e, "llm_dequantize_q4");
}
ia2p_status ia2p_llm_gemv_q4(void* stream, const void* packed, const float* absmax, const float* codebook, const float* x, float* out, int N, int K) {
  if (!x || !out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_q4: null argument");
  const ia2p_status st = q4_op_args("llm_gemv_q4", packed, absmax, out, codebook, N, K);
  if (st != IA2P_OK) return st;
  if (K > Q4_MAX_K) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_q4: K=%d (at most %d)", K, Q4_MAX_K);
  LlmGemv a{};
  a.X = x; a.N = N; a.K = K; a.out = out;
  LlmQ4 q;
  q.Wq = (const u4v*)packed; q.absmax = absmax;
  memcpy(q.cb.v, codebook, sizeof q.cb.v);
  hipError_t e = llm_launch_gemv_q4(a, q, EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_q4");
}
ia2p_status ia2p_llm_finalize_weights(ia2p_llm* c) {
  const ia2p_status st = rc_finalize(c, "LLM");
  if (st != IA2P_OK) return st;
  float f[64];      // transformers LlamaRotaryEmbedding: inv_freq = 1 / theta^(2 i / 128), fp32
  for (int i = 0; i < 64; ++i) f[i] = 1.0f / powf(c->cfg.rope_theta, (float)(2 * i) / 128.0f);
  hipError_t e = hipMemcpy(c->arena + c->invf, f, sizeof f, hipMemcpyHostToDevice);
  if (e != hipSuccess) { c->finalized = false; return fail_hip(c, e, "llm rotary table"); }
  return IA2P_OK;
}
size_t ia2p_llm_kv_slots_bytes(ia2p_llm* c, int max_positions, int n_slots) {
  if (!c || n_slots < 1 || max_positions < 1 || max_positions > LLM_MAX_POSITIONS) return 0;
  return (size_t)n_slots * c->cfg.num_layers * 2 * (size_t)max_positions * c->cfg.hidden_size * sizeof(half_t);
}
size_t ia2p_llm_kv_bytes(ia2p_llm* c, int max_positions) { return ia2p_llm_kv_slots_bytes(c, max_positions, 1); }
static ia2p_status llm_bind_slots(ia2p_llm* c, const char* what, void* dev, size_t bytes, int max_positions, int n_slots) {
  if (!c || !dev) return fail(c, IA2P_ERR_INVALID, "%s: null argument", what);
  if (n_slots < 1) return fail(c, IA2P_ERR_INVALID, "%s: %d slots", what, n_slots);
  if (max_positions < 1 || max_positions > LLM_MAX_POSITIONS) return fail(c, IA2P_ERR_SHAPE, "%s: %d positions (1..%d)", what, max_positions, LLM_MAX_POSITIONS);
  if (((uintptr_t)dev) & 15) return fail(c, IA2P_ERR_INVALID, "%s: the cache must be 16-byte aligned", what);
  const size_t need = ia2p_llm_kv_slots_bytes(c, max_positions, n_slots);
  if (bytes < need) return fail(c, IA2P_ERR_NOMEM, "%s: %zu bytes, %zu needed", what, bytes, need);
  c->kv = (half_t*)dev; c->max_pos = max_positions; c->n_slots = n_slots; c->cur = 0;
  c->spos.assign((size_t)n_slots, 0);
  return IA2P_OK;
}
ia2p_status ia2p_llm_bind_kv(ia2p_llm* c, void* dev, size_t bytes, int max_positions) { return llm_bind_slots(c, "llm_bind_kv", dev, bytes, max_positions, 1); }
ia2p_status ia2p_llm_bind_kv_slots(ia2p_llm* c, void* dev, size_t bytes, int max_positions, int n_slots) {
  return llm_bind_slots(c, "llm_bind_kv_slots", dev, bytes, max_positions, n_slots);
}
int ia2p_llm_slots(ia2p_llm* c) { return c ? c->n_slots : 0; }
size_t ia2p_llm_workspace_bytes(ia2p_llm* c, int max_T) {
  if (!c || max_T < 1) return 0;
  const size_t a = llm_dry(c, max_T), b = llm_dry(c, 0);
  return a && b ? std::max(a, b) : 0;
}
size_t ia2p_llm_batch_workspace_bytes(ia2p_llm* c, int max_T, int max_rows) {
  if (!c || max_T < 0 || max_rows < 1 || max_rows > LLM_MAX_ROWS) return 0;
  size_t a = 1;       // every T up to max_T: a prefill's need is not monotone in T (the K-split of its GEMMs changes with the row count)
  for (int T = 1; T <= max_T && a; ++T) { const size_t t = llm_dry(c, T); a = t ? std::max(a, t) : 0; }
  const size_t b = llm_dry_rows(c, max_rows);
  return a && b ? std::max(a, b) : 0;
}
ia2p_status ia2p_llm_reset(ia2p_llm* c) {
  if (!c) return fail(nullptr, IA2P_ERR_INVALID, "llm_reset: null argument");
  c->spos[0] = 0;
  return IA2P_OK;
}
int ia2p_llm_position(ia2p_llm* c) { return c ? c->spos[0] : -1; }
ia2p_status ia2p_llm_reset_slot(ia2p_llm* c, int slot) {
  if (!c) return fail(nullptr, IA2P_ERR_INVALID, "llm_reset_slot: null argument");
  if (slot < 0 || slot >= c->n_slots) return fail(c, IA2P_ERR_INVALID, "llm_reset_slot: slot %d of %d", slot, c->n_slots);
  c->spos[slot] = 0;
  return IA2P_OK;
}
int ia2p_llm_slot_position(ia2p_llm* c, int slot) { return c && slot >= 0 && slot < c->n_slots ? c->spos[slot] : -1; }
ia2p_status ia2p_llm_embed(ia2p_llm* c, void* stream, const int32_t* ids, int T, void* out) {
  if (!c || !ids || !out) return fail(c, IA2P_ERR_INVALID, "llm_embed: null argument");
  if (T < 1) return fail(c, IA2P_ERR_SHAPE, "llm_embed: T=%d", T);
  if (!c->finalized) return fail(c, IA2P_ERR_STATE, "llm_embed before weights were finalized");
  hipLaunchKernelGGL(llm_gather_rows_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, (const int*)ids, W_(c, c->tok), (half_t*)out, c->cfg.hidden_size, c->cfg.vocab_size);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? IA2P_OK : fail_hip(c, e, "llm_embed");
}
static ia2p_status llm_prefill_at(ia2p_llm* c, const char* what, int slot, void* stream, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* ws,
                                  size_t ws_bytes) {
  if (!c || !inputs_embeds || !hidden_out || !logits_out || !ws) return fail(c, IA2P_ERR_INVALID, "%s: null argument", what);
  ia2p_status st = llm_ready(c, what);
  if (st != IA2P_OK) return st;
  if (slot < 0 || slot >= c->n_slots) return fail(c, IA2P_ERR_INVALID, "%s: slot %d of %d", what, slot, c->n_slots);
  const int pos = c->spos[slot];
  if (T < 1 || pos + T > c->max_pos) return fail(c, IA2P_ERR_SHAPE, "%s: %d rows at position %d, the cache holds %d", what, T, pos, c->max_pos);
  if (!zero_page()) return fail(c, IA2P_ERR_HIP, "cannot allocate zero page");
  c->cur = slot;
  st = llm_enter(c, stream, ws, ws_bytes, llm_dry(c, T));
  if (st == IA2P_OK) st = llm_leave(c, llm_run_prefill(c, (const half_t*)inputs_embeds, T, hidden_out, logits_out));
  c->cur = 0;
  if (st == IA2P_OK) c->spos[slot] += T;
  return st;
}
ia2p_status ia2p_llm_prefill(ia2p_llm* c, void* stream, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  return llm_prefill_at(c, "llm_prefill", 0, stream, inputs_embeds, T, hidden_out, logits_out, ws, ws_bytes);
}
ia2p_status ia2p_llm_prefill_slot(ia2p_llm* c, void* stream, int slot, const void* inputs_embeds, int T, float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  return llm_prefill_at(c, "llm_prefill_slot", slot, stream, inputs_embeds, T, hidden_out, logits_out, ws, ws_bytes);
}
ia2p_status ia2p_llm_decode(ia2p_llm* c, void* stream, int token_id, float* hidden_out, float* logits_out, void* ws, size_t ws_bytes) {
  if (!c || !hidden_out || !logits_out || !ws) return fail(c, IA2P_ERR_INVALID, "llm_decode: null argument");
  ia2p_status st = llm_ready(c, "llm_decode");
  if (st != IA2P_OK) return st;
  const int pos = c->spos[0];
  if (pos < 1) return fail(c, IA2P_ERR_STATE, "llm_decode before a prefill (position 0)");
  if (pos >= c->max_pos) return fail(c, IA2P_ERR_SHAPE, "llm_decode: position %d is past the cache (%d positions)", pos, c->max_pos);
  if (token_id < 0 || token_id >= c->cfg.vocab_size) return fail(c, IA2P_ERR_SHAPE, "llm_decode: token %d outside the vocabulary (%d)", token_id, c->cfg.vocab_size);
  c->cur = 0;
  st = llm_enter(c, stream, ws, ws_bytes, llm_dry(c, 0));
  if (st != IA2P_OK) return st;
  st = llm_leave(c, llm_run_decode(c, token_id, hidden_out, logits_out));
  if (st == IA2P_OK) c->spos[0] += 1;
  return st;
}
ia2p_status ia2p_llm_decode_batch(ia2p_llm* c, void* stream, const int32_t* slots, const int32_t* token_ids, int n, float* hidden_out, float* logits_out, void* ws,
                                  size_t ws_bytes) {
  if (!c || !slots || !token_ids || !hidden_out || !logits_out || !ws) return fail(c, IA2P_ERR_INVALID, "llm_decode_batch: null argument");
  ia2p_status st = llm_ready(c, "llm_decode_batch");
  if (st != IA2P_OK) return st;
  if (n < 1 || n > LLM_MAX_ROWS) return fail(c, IA2P_ERR_INVALID, "llm_decode_batch: %d rows (1..%d)", n, LLM_MAX_ROWS);
  for (int r = 0; r < n; ++r) {
    if (slots[r] < 0 || slots[r] >= c->n_slots) return fail(c, IA2P_ERR_INVALID, "llm_decode_batch: row %d names slot %d, the cache has %d", r, slots[r], c->n_slots);
    for (int p = 0; p < r; ++p)
      if (slots[p] == slots[r]) return fail(c, IA2P_ERR_INVALID, "llm_decode_batch: slot %d is named twice (rows %d and %d)", slots[r], p, r);
  }
  for (int r = 0; r < n; ++r) {
    const int pos = c->spos[slots[r]];
    if (pos < 1) return fail(c, IA2P_ERR_STATE, "llm_decode_batch: slot %d before a prefill (position 0)", slots[r]);
    if (pos >= c->max_pos) return fail(c, IA2P_ERR_SHAPE, "llm_decode_batch: slot %d at position %d is past the cache (%d positions)", slots[r], pos, c->max_pos);
    if (token_ids[r] < 0 || token_ids[r] >= c->cfg.vocab_size)
      return fail(c, IA2P_ERR_SHAPE, "llm_decode_batch: token %d of row %d outside the vocabulary (%d)", token_ids[r], r, c->cfg.vocab_size);
  }
  st = llm_enter(c, stream, ws, ws_bytes, llm_dry_rows(c, n), true);
  if (st != IA2P_OK) return st;
  st = llm_leave(c, llm_run_decode_rows(c, slots, token_ids, n, hidden_out, logits_out));
  if (st == IA2P_OK)
    for (int r = 0; r < n; ++r) c->spos[slots[r]] += 1;
  return st;
}
static LlmRows gemv_rows_args(const float* x, float* out, int N, int K, int M) {
  LlmRows b{};
  b.M = M;
  for (int m = 0; m < M; ++m) { b.X[m] = x + (size_t)m * K; b.out[m] = out + (size_t)m * N; }
  return b;
}
ia2p_status ia2p_llm_gemv_rows(void* stream, const void* W, const float* x, float* out, int N, int K, int M) {
  if (!W || !x || !out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_rows: null argument");
  if (N < 1 || K < 8 || K % 8) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_rows: N=%d K=%d (K a multiple of 8)", N, K);
  if (M < 1 || M > LLM_MAX_ROWS) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_rows: M=%d (1..%d)", M, LLM_MAX_ROWS);
  LlmGemv a{};
  a.W = (const half_t*)W; a.N = N; a.K = K;
  hipError_t e = llm_launch_gemv_rows(a, gemv_rows_args(x, out, N, K, M), EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_rows");
}
ia2p_status ia2p_llm_gemv_q4_rows(void* stream, const void* packed, const float* absmax, const float* codebook, const float* x, float* out, int N, int K, int M) {
  if (!x || !out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv_q4_rows: null argument");
  const ia2p_status st = q4_op_args("llm_gemv_q4_rows", packed, absmax, out, codebook, N, K);
  if (st != IA2P_OK) return st;
  if (K > Q4_MAX_K) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_q4_rows: K=%d (at most %d)", K, Q4_MAX_K);
  if (M < 1 || M > LLM_MAX_ROWS) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv_q4_rows: M=%d (1..%d)", M, LLM_MAX_ROWS);
  LlmGemv a{};
  a.N = N; a.K = K;
  LlmQ4 q;
  q.Wq = (const u4v*)packed; q.absmax = absmax;
  memcpy(q.cb.v, codebook, sizeof q.cb.v);
  hipError_t e = llm_launch_gemv_q4_rows(a, q, gemv_rows_args(x, out, N, K, M), EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv_q4_rows");
}
ia2p_status ia2p_llm_gemv(void* stream, const void* W, const float* x, float* out, int N, int K) {
  if (!W || !x || !out) return fail(nullptr, IA2P_ERR_INVALID, "llm_gemv: null argument");
  if (N < 1 || K < 8 || K % 8) return fail(nullptr, IA2P_ERR_SHAPE, "llm_gemv: N=%d K=%d (K a multiple of 8)", N, K);
  LlmGemv a{};
  a.W = (const half_t*)W; a.X = x; a.N = N; a.K = K; a.out = out;
  hipError_t e = llm_launch_gemv(a, EPI_PLAIN, (hipStream_t)stream);
  RET_HIP(e, "llm_gemv");
}
ia2p_status ia2p_gelu(void* stream, void* x, int64_t n) {
  if (!x) return fail(nullptr, IA2P_ERR_INVALID, "gelu: null argument");
  if (n < 1 || n > ((int64_t)1 << 31)) return fail(nullptr, IA2P_ERR_SHAPE, "gelu: n=%lld", (long long)n);
  hipLaunchKernelGGL(llm_gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)x, (long)n);
  hipError_t e = hipGetLastError();
  RET_HIP(e, "gelu");
}

}  // extern "C"
