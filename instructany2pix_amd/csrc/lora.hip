// LoRA adapters for the UNet family: the merge kernel behind ia2p_lora_merge (out = base + sum_a coef_a * up_a . down_a, one pass over the weight, the rank-r products on
// v_mfma_f32_16x16x32_f16) and the inverse re-layouts behind ia2p_read_tensor (engine_rt.hip: rc_read_tensor), which give a parameter back in the checkpoint's layout
// so that an adapter can be merged from -- and the weight restored to -- the bits that were loaded.
#include "engine_rt.h"

// ---- merge -------------------------------------------------------------------------------------------------------------------------------------------------------
// One workgroup (4 waves) owns a 64 x 64 tile of the weight (small tiles: the weights of a UNet are small, 640^2 .. 10240 x 1280, and a launch wants more workgroups than
// CUs). Wave w owns rows 16 w .. 16 w + 15 of the tile and all its columns, as 2 LORA_NG 16 x 16 MFMA tiles (g, t):
// `down` is the FIRST operand and `up` the second, so that D[m = 4 q + reg][n = fr] (q = lane >> 4, fr = lane & 15) puts the four registers of a lane on four consecutive
// COLUMNS of ONE row of the weight. MFMA row m of tile (g, t) is column 32 g + 8 (m >> 2) + 4 t + (m & 3) of the workgroup's tile: a lane's registers of tiles (g, 0) and
// (g, 1) are then the eight consecutive columns 32 g + 8 q .. + 7 -- one 16-byte access for the base value and one for the result.
// Operands: lane l holds A[m = l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][n = l & 15], j = 0 .. 7. A rank chunk of 32 is staged in LDS, zero-filled past the
// rank, past row N and past column K: `up` as [row][rank], `down` TRANSPOSED as [column][rank], rows of LORA_LD halves (80 bytes: 16-byte aligned fragments).
// What an element's bits depend on: its row of up, its column of down (both in rank order, chunk after chunk into one fp32 accumulator per adapter; a zero product adds
// nothing), its base value and the coefficients -- not N, K, the tile or the lane it falls on: the MFMA's internal order is a function of k alone.
constexpr int LORA_BM = 64, LORA_BC = 64, LORA_BR = 32, LORA_LD = 40;
constexpr int LORA_NG = LORA_BC / 32;          // 32-column groups of the tile: two MFMA tiles each
constexpr int LORA_CV = LORA_BC / 8;           // 8-column runs per rank row of the down chunk
static_assert(LORA_BC % 32 == 0 && 256 % LORA_CV == 0 && (LORA_BR * LORA_CV) % 256 == 0, "tile shape");
struct LoraArgs {
  const half_t* up[IA2P_LORA_MAX_ADAPTERS];
  const half_t* down[IA2P_LORA_MAX_ADAPTERS];
  int rank[IA2P_LORA_MAX_ADAPTERS];
  float coef[IA2P_LORA_MAX_ADAPTERS];
  int n;
  unsigned up_vec, down_vec;      // bit a: 16-byte loads of up[a] (rank % 8 == 0, aligned) / down[a] (K % 8 == 0, aligned)
  int base_vec;                   // 16-byte accesses of base and out
};

__global__ __launch_bounds__(256) void lora_merge_kernel(const half_t* base, half_t* out, int N, long K, LoraArgs a) {
  __shared__ __attribute__((aligned(16))) half_t s_up[LORA_BM * LORA_LD];
  __shared__ __attribute__((aligned(16))) half_t s_dn[LORA_BC * LORA_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, q = lane >> 4;
  const long c0 = (long)blockIdx.x * LORA_BC;
  const int i0 = blockIdx.y * LORA_BM;
  const int row = i0 + 16 * wave + fr;

  // the base values first (out may BE base: every element is read and written by the one lane that owns it)
  f4 sum[2 * LORA_NG];
#pragma unroll
  for (int g = 0; g < LORA_NG; ++g) {
    const long c = c0 + 32 * g + 8 * q;
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < N) {
      if (a.base_vec) { if (c < K) v = *(const h8*)(base + (long)row * K + c); }
      else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (c + e < K) v[e] = base[(long)row * K + c + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sum[2 * g][e] = (float)v[e]; sum[2 * g + 1][e] = (float)v[4 + e]; }
  }

  for (int ad = 0; ad < a.n; ++ad) {
    const half_t* up = a.up[ad];
    const half_t* dn = a.down[ad];
    const int R = a.rank[ad];
    const bool upv = (a.up_vec >> ad) & 1, dnv = (a.down_vec >> ad) & 1;
    f4 acc[2 * LORA_NG];
#pragma unroll
    for (int x = 0; x < 2 * LORA_NG; ++x) acc[x] = f4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < R; j0 += LORA_BR) {
      __syncthreads();      // the fragments of the chunk before are read
      {   // up chunk [64 rows][32 ranks]: one 8-rank run per thread
        const int r = tid >> 2, j = j0 + 8 * (tid & 3);
        h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i0 + r < N) {
          const half_t* p = up + (long)(i0 + r) * R + j;
          if (upv) { if (j < R) v = *(const h8*)p; }
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) if (j + e < R) v[e] = p[e];
          }
        }
        *(h8*)&s_up[r * LORA_LD + 8 * (tid & 3)] = v;
      }
#pragma unroll
      for (int it = 0; it < LORA_BR * LORA_CV / 256; ++it) {   // down chunk [32 ranks][LORA_BC columns] -> [column][rank]: 8-column runs
        const int jj = tid / LORA_CV + (256 / LORA_CV) * it, cv = tid % LORA_CV;
        const long c = c0 + 8 * cv;
        h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (j0 + jj < R) {
          const half_t* p = dn + (long)(j0 + jj) * K + c;
          if (dnv) { if (c < K) v = *(const h8*)p; }
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) if (c + e < K) v[e] = p[e];
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s_dn[(8 * cv + e) * LORA_LD + jj] = v[e];
      }
      __syncthreads();
      const h8 bf = *(const h8*)&s_up[(16 * wave + fr) * LORA_LD + 8 * q];
#pragma unroll
      for (int x = 0; x < 2 * LORA_NG; ++x) {
        const int col = 32 * (x >> 1) + 8 * (fr >> 2) + 4 * (x & 1) + (fr & 3);
        const h8 af = *(const h8*)&s_dn[col * LORA_LD + 8 * q];
        acc[x] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[x], 0, 0, 0);
      }
    }
    const float cf = a.coef[ad];
#pragma unroll
    for (int x = 0; x < 2 * LORA_NG; ++x)
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[x][e] = __builtin_fmaf(cf, acc[x][e], sum[x][e]);      // adapters in list order, one fused multiply-add each
  }

  if (row >= N) return;      // (no barrier follows)
#pragma unroll
  for (int g = 0; g < LORA_NG; ++g) {
    const long c = c0 + 32 * g + 8 * q;
    h8 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = (half_t)sum[2 * g][e]; v[4 + e] = (half_t)sum[2 * g + 1][e]; }      // the ONE rounding to fp16 (nearest even)
    if (a.base_vec) { if (c < K) *(h8*)(out + (long)row * K + c) = v; }
    else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (c + e < K) out[(long)row * K + c + e] = v[e];
    }
  }
}

// ---- the inverse re-layouts of misc.hip's pack kernels (permutations: pack then unpack gives the bits back) ------------------------------------------------------
__global__ void unpack_conv_kernel(const half_t* src /*[Co][tap][Ci]*/, half_t* dst /*[Co][Ci][3][3]*/, int Co, int Ci) {
  const long total = (long)Co * Ci * 9;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i / ((long)Ci * 9));
    const int k = (int)(i - (long)co * Ci * 9);
    const int ci = k / 9, tap = k - ci * 9;
    dst[i] = src[((long)co * 9 + tap) * Ci + ci];
  }
}
__global__ void unpack_conv_in_kernel(const half_t* src /*[Co][64]*/, half_t* dst /*[Co][KT]*/, int Co, int KT) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)Co * KT; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i / KT), k = (int)(i - (long)co * KT);
    dst[i] = src[(size_t)co * 64 + k];
  }
}
__global__ void unpack_geglu_kernel(const half_t* src, half_t* dst, int rows, int rowlen) {
  const long total = (long)rows * rowlen;
  const int half_ = rows / 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int p = (int)(i / rowlen), k = (int)(i - (long)p * rowlen);      // packed row p holds checkpoint row s (pack_geglu_kernel)
    const int t = p >> 5, w = p & 31;
    const int s = w < 16 ? 16 * t + w : half_ + 16 * t + (w - 16);
    dst[(long)s * rowlen + k] = src[i];
  }
}
static inline int grid_of(long n) { const long g = (n + 255) / 256; return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }
hipError_t ia2p_launch_unpack_conv(const half_t* src, half_t* dst, int Co, int Ci, hipStream_t s) {
  hipLaunchKernelGGL(unpack_conv_kernel, dim3(grid_of((long)Co * Ci * 9)), dim3(256), 0, s, src, dst, Co, Ci);
  return hipGetLastError();
}
hipError_t ia2p_launch_unpack_conv_in(const half_t* src, half_t* dst, int Co, int KT, hipStream_t s) {
  if (KT > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(unpack_conv_in_kernel, dim3(grid_of((long)Co * KT)), dim3(256), 0, s, src, dst, Co, KT);
  return hipGetLastError();
}
hipError_t ia2p_launch_unpack_geglu(const half_t* src, half_t* dst, int rows, int rowlen, hipStream_t s) {
  if (rows % 32) return hipErrorInvalidValue;      // (the pairing works on blocks of 16 value + 16 gate rows)
  hipLaunchKernelGGL(unpack_geglu_kernel, dim3(grid_of((long)rows * rowlen)), dim3(256), 0, s, src, dst, rows, rowlen);
  return hipGetLastError();
}

extern "C" {

ia2p_status ia2p_lora_merge(void* stream, const void* base, void* out, int N, int64_t K, int n, const void* const* up, const void* const* down, const int* rank, const float* coef) {
  if (!base || !out || !up || !down || !rank || !coef) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: null argument");
  if (n < 1 || n > IA2P_LORA_MAX_ADAPTERS) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: %d adapters (1 .. %d)", n, IA2P_LORA_MAX_ADAPTERS);
  if (N < 1 || K < 1) return fail(nullptr, IA2P_ERR_SHAPE, "lora_merge: N=%d K=%lld must be positive", N, (long long)K);
  if ((N + LORA_BM - 1) / LORA_BM > 65535 || (K + LORA_BC - 1) / LORA_BC > 0x7fffffffLL || K > ((int64_t)1 << 40))
    return fail(nullptr, IA2P_ERR_SHAPE, "lora_merge: N=%d K=%lld too large for one launch", N, (long long)K);
  const uintptr_t b0 = (uintptr_t)base, o0 = (uintptr_t)out;
  const size_t wbytes = (size_t)N * (size_t)K * sizeof(half_t);
  if (b0 != o0 && b0 < o0 + wbytes && o0 < b0 + wbytes) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: out overlaps base partially (in place means out == base)");
  LoraArgs a;
  memset(&a, 0, sizeof a);
  a.n = n;
  a.base_vec = K % 8 == 0 && b0 % 16 == 0 && o0 % 16 == 0;
  for (int i = 0; i < n; ++i) {
    if (!up[i] || !down[i]) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: adapter %d: null up / down", i);
    if (rank[i] < 1 || rank[i] > IA2P_LORA_MAX_RANK) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: adapter %d: rank %d (1 .. %d)", i, rank[i], IA2P_LORA_MAX_RANK);
    if (!std::isfinite(coef[i])) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: adapter %d: coefficient is not finite", i);
    const uintptr_t u0 = (uintptr_t)up[i], d0 = (uintptr_t)down[i];
    const size_t ub = (size_t)N * rank[i] * sizeof(half_t), db = (size_t)rank[i] * (size_t)K * sizeof(half_t);
    if ((u0 < o0 + wbytes && o0 < u0 + ub) || (d0 < o0 + wbytes && o0 < d0 + db)) return fail(nullptr, IA2P_ERR_INVALID, "lora_merge: adapter %d: up / down overlaps out", i);
    a.up[i] = (const half_t*)up[i]; a.down[i] = (const half_t*)down[i]; a.rank[i] = rank[i]; a.coef[i] = coef[i];
    if (rank[i] % 8 == 0 && u0 % 16 == 0) a.up_vec |= 1u << i;
    if (K % 8 == 0 && d0 % 16 == 0) a.down_vec |= 1u << i;
  }
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((K + LORA_BC - 1) / LORA_BC), (unsigned)((N + LORA_BM - 1) / LORA_BM)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)base, (half_t*)out, N, (long)K, a);
  RET_HIP(hipGetLastError(), "lora_merge");
}

}  // extern "C"
