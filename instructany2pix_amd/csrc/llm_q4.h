// The 4-bit weight format of the LLaMA decoder executor: quantise, dequantise, the decode GEMVs on packed codes (one input row; 2 to 8 input rows) and
// their launchers. Included by llm_engine.hip only, after llm_kernels.h (LlmGemv, LlmRows, the row mapping and the epilogue store). DESIGN.md §10.
#pragma once

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
  auto fetch = [&](int unit, int it, u4v* w, float* am) {
    const int p = min(it * 64 + lane, pieces - 1);
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const size_t row = (size_t)llm_weight_row<EPI>(a.N, unit, r, RW);
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
    for (int r = 0; r < RW; ++r) acc[r] = wave_sum(acc[r]);
    if (EPI == EPI_PLAIN || EPI == EPI_RESID) {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int n = unit * RW + r;
        if (lane == r && n < a.N) llm_store<EPI>(a, a.out, n, acc[r], 0.f, rstd);
      }
    } else if (lane == 0 && unit < a.N / 2) llm_store<EPI>(a, a.out, unit, acc[0], acc[RW - 1], rstd);
  }
  if (EPI == EPI_PLAIN && a.hid && a.gamma && blockIdx.x == 0)
    for (int i = tid; i < K; i += 256) a.hid[i] = a.X[i] * rstd * (float)a.gamma[i];
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
  auto fetch = [&](int it, u4v (*w)[RW], float (*am)[RW]) {
    const int p = min(it * 64 + lane, pieces - 1);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const size_t row = (size_t)llm_weight_row<EPI>(a.N, unit0 + u, r, RW);
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
          if (lane == r && n < a.N) llm_store<EPI>(a, b.out[m], n, v[r], 0.f, rstd[m]);
        }
      } else if (lane == 0 && unit < a.N / 2) {
        if (EPI == EPI_QKV) llm_store<EPI>(llm_row_view(a, b, m), nullptr, unit, v[0], v[RW - 1], rstd[m]);
        else llm_store<EPI>(a, b.out[m], unit, v[0], v[RW - 1], rstd[m]);
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

// ---- launchers ------------------------------------------------------------------------------------------------------
static LlmQ4 llm_q4(const void* codes, const void* absmax, const float* codebook) {
  LlmQ4 q;
  q.Wq = (const u4v*)codes; q.absmax = (const float*)absmax;
  memcpy(q.cb.v, codebook, sizeof q.cb.v);
  return q;
}
static ia2p_status q4_op_args(const char* what, const void* a, const void* b, const void* d, const void* cb, int64_t N, int64_t K) {
  if (!a || !b || !d || !cb) return fail(nullptr, IA2P_ERR_INVALID, "%s: null argument", what);
  if (N < 1 || K < 64 || K % 64 || N * K > ((int64_t)1 << 34)) return fail(nullptr, IA2P_ERR_SHAPE, "%s: N=%lld K=%lld (K a multiple of 64)", what, (long long)N, (long long)K);
  return IA2P_OK;
}
// the argument check of the 4-bit GEMVs, as llm_gemv_check (the N K limit is q4_op_args')
static ia2p_status llm_gemv_q4_check(const void* codes, const void* absmax, const void* codebook, const void* x, int N, int K, int H, int M, int epi) {
  if (!codes || !absmax || !codebook || !x) return IA2P_ERR_INVALID;
  return N < 1 || K < 64 || K % 64 || (int64_t)N * K > ((int64_t)1 << 34) || K > Q4_MAX_K || M < 1 || M > LLM_MAX_ROWS || !llm_epi_shape_ok(epi, N, H) ? IA2P_ERR_SHAPE : IA2P_OK;
}
static size_t q4_gemv_lds(int K) { return (size_t)(512 + 4 + (((K >> 5) + 63) >> 6) * 2048) * sizeof(float); }
static hipError_t llm_launch_gemv_q4(const LlmGemv& a, const LlmQ4& q, int epi, hipStream_t s) {
  if (llm_gemv_q4_check(q.Wq, q.absmax, q.cb.v, a.X, a.N, a.K, a.H, 1, epi) != IA2P_OK) return hipErrorInvalidValue;
  return llm_with_epi(epi, [&](auto E) {
    hipLaunchKernelGGL((llm_gemv_q4_kernel<decltype(E)::value>), dim3(llm_gemv_grid(epi, a.N, 4 * Q4_U * Q4_RW)), dim3(256), q4_gemv_lds(a.K), s, a, q);
    return hipGetLastError();
  });
}
static size_t q4_rows_lds(int mt) { return (size_t)(512 + 4 * mt + mt * 2048) * sizeof(float); }
template <int MT>
static hipError_t gemv_q4_rows_launch(const LlmGemv& a, const LlmQ4& q, const LlmRows& b, int epi, hipStream_t s) {
  const size_t lds = q4_rows_lds(MT);
  if (lds > 64 * 1024) {          // MT = 8: 66 KiB of the CU's 160
    static bool done = false;
    for (int e = EPI_PLAIN; e <= EPI_SWIGLU && !done; ++e) {
      const hipError_t err = llm_with_epi(e, [&](auto E) {
        return hipFuncSetAttribute((const void*)llm_gemv_q4_rows_kernel<decltype(E)::value, MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      });
      if (err != hipSuccess) return err;
    }
    done = true;
  }
  return llm_with_epi(epi, [&](auto E) {
    hipLaunchKernelGGL((llm_gemv_q4_rows_kernel<decltype(E)::value, MT>), dim3(llm_gemv_grid(epi, a.N, 4 * Q4R_U * Q4_RW)), dim3(256), lds, s, a, q, b);
    return hipGetLastError();
  });
}
static hipError_t llm_launch_gemv_q4_rows(const LlmGemv& a, const LlmQ4& q, LlmRows b, int epi, hipStream_t s) {
  if (b.M == 1) return llm_launch_gemv_q4(llm_first_row(a, b), q, epi, s);
  if (llm_gemv_q4_check(q.Wq, q.absmax, q.cb.v, b.X[0], a.N, a.K, a.H, b.M, epi) != IA2P_OK) return hipErrorInvalidValue;
  rows_pad(b);
  switch (rows_mt(b.M)) {
    case 2: return gemv_q4_rows_launch<2>(a, q, b, epi, s);
    case 4: return gemv_q4_rows_launch<4>(a, q, b, epi, s);
    default: return gemv_q4_rows_launch<8>(a, q, b, epi, s);
  }
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
