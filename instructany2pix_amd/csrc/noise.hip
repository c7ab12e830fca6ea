// Seeded normal draws of an edit request (include/ia2p.h, "Seeded noise"): standard normals from the request's own Philox4x32-10 stream, the VAE posterior
// sample drawn from it, and the reference's polar mixing (pipeline.py:295-300) per request -- all where the latents live, so that a seeded request never
// leaves the device between inversion and sampling.
//
// The rule (the contract is in the header): element e of draw `draw` of seed `seed` comes from block j = e >> 2 = Philox(counter (j, draw, 0, 1), key (seed low,
// seed high)); pair p = (e & 3) >> 1 of its words gives u1 = ((w[2p] >> 8) + 1) 2^-24 in (0, 1] and u2 = (w[2p + 1] >> 8) 2^-24, r = sqrt(-2 ln u1), and the
// element is r cospi(2 u2) (even e) or r sinpi(2 u2) (odd e). logf, sqrtf and sincospif are the full-accuracy library functions; no native approximation.
// A block therefore yields exactly the elements 4 j .. 4 j + 3.
//
// Ownership is by INDEX: thread t of a row owns the blocks first / 4 + 2 t and + 1, i.e. the row's local elements 8 t .. 8 t + 7, wherever the row lies in
// memory. Where the row starts on a 16-byte boundary and the elements are inside the row, they leave in 16-byte stores (one for fp16, two for fp32);
// anywhere else -- a misaligned row, the last group of a row -- the same values leave in scalar stores guarded by the index. Nothing about a value depends
// on which of the two happened, on the grid, on the rows that share the launch or on the sub-range asked for.
//
// Polar mixing needs three norms per request before any output: every workgroup of a row computes all three sums of squares over the WHOLE row itself (the
// row is L2-resident: 256 KB at 4 x 128 x 128), in one fixed association that depends on `per` alone -- thread t adds the squares of the groups of 8 at
// (k * 1024 + t) * 8 in index order with __fmaf_rn, the lanes fold by xor-butterfly, the 16 wave totals are added in wave order -- and then writes its slices
// of the output. Every workgroup of a row holds the same three numbers bit for bit, so a row does not depend on B, on its place or on the slice count.
#include "engine_rt.h"
#include "normal4.h"

namespace {

constexpr int MAX_BY_VALUE = 8;                 // rows whose seeds, draws and alphas travel in the kernel arguments
constexpr int NT = 256;                         // threads per workgroup of the two draw kernels
constexpr int MIX_NT = 1024, MIX_NW = MIX_NT / 64;
constexpr long MIX_SLICE = (long)MIX_NT * 8;    // elements a workgroup writes per pass
constexpr int MIX_MAX_SLICES = 16;              // workgroups per row at most (each reads the whole row once for the norms)
constexpr long long MAX_ELEMS = 1ll << 34;      // block index j = e >> 2 is one 32-bit counter word

struct NoiseRows { uint64_t seed[MAX_BY_VALUE]; uint32_t draw[MAX_BY_VALUE]; };
struct MixRows { float alpha[MAX_BY_VALUE]; };

template <bool F16>
__global__ __launch_bounds__(NT) void randn_seeded_kernel(void* out, long per, uint32_t j0, NoiseRows rows) {
  const int b = blockIdx.y;
  const long i0 = ((long)blockIdx.x * NT + threadIdx.x) * 8;      // local index of this thread's first element
  if (i0 >= per) return;
  const uint64_t seed = rows.seed[b];
  const uint32_t draw = rows.draw[b];
  const uint32_t j = j0 + (uint32_t)(i0 >> 2);                      // first + per <= 2^34: no wrap
  float z[8];
  normal4(seed, draw, j, z);
  if (i0 + 4 < per) normal4(seed, draw, j + 1u, z + 4);
  else { z[4] = z[5] = z[6] = z[7] = 0.f; }
  if constexpr (F16) {
    half_t* row = (half_t*)out + (long)b * per;
    if ((((uintptr_t)row) & 15) == 0 && i0 + 8 <= per) {
      h8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (half_t)z[e];
      *(h8*)(row + i0) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (i0 + e < per) row[i0 + e] = (half_t)z[e];
    }
  } else {
    float* row = (float*)out + (long)b * per;
    const bool vec = (((uintptr_t)row) & 15) == 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long i = i0 + 4 * q;
      if (vec && i + 4 <= per) {
        f4 v = {z[4 * q], z[4 * q + 1], z[4 * q + 2], z[4 * q + 3]};
        *(f4*)(row + i) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (i + e < per) row[i + e] = z[4 * q + e];
      }
    }
  }
}

// x = fp16(fmaf(exp(0.5 clamp(logvar, -30, 20)), z, mean)), out = fp16(x * scaling_factor): DiagonalGaussianDistribution.sample (vae.py), then the scaling
__device__ __forceinline__ half_t posterior_one(half_t mean, half_t logvar, float z, float sf) {
  const float lv = fminf(fmaxf((float)logvar, -30.f), 20.f);
  const half_t x = (half_t)__fmaf_rn(expf(0.5f * lv), z, (float)mean);
  return (half_t)__fmul_rn((float)x, sf);
}

__global__ __launch_bounds__(NT) void posterior_seeded_kernel(const half_t* mom, half_t* out, int C, long HW, float sf, NoiseRows rows) {
  const int b = blockIdx.y;
  const long per = (long)C * HW;
  const long i0 = ((long)blockIdx.x * NT + threadIdx.x) * 8;
  if (i0 >= per) return;
  const uint64_t seed = rows.seed[b];
  const uint32_t draw = rows.draw[b];
  float z[8];
  normal4(seed, draw, (uint32_t)(i0 >> 2), z);
  if (i0 + 4 < per) normal4(seed, draw, (uint32_t)(i0 >> 2) + 1u, z + 4);
  else { z[4] = z[5] = z[6] = z[7] = 0.f; }
  const half_t* mrow = mom + (long)b * 2 * per;      // [2 C, HW]: means, then log-variances
  half_t* orow = out + (long)b * per;
  // HW % 8 == 0: the eight elements share a channel and every group of every row starts on a 16-byte boundary when the bases do
  if ((HW & 7) == 0 && ((((uintptr_t)mom) | ((uintptr_t)out)) & 15) == 0) {
    const h8 m = *(const h8*)(mrow + i0), lv = *(const h8*)(mrow + per + i0);
    h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = posterior_one(m[e], lv[e], z[e], sf);
    *(h8*)(orow + i0) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (i0 + e < per) orow[i0 + e] = posterior_one(mrow[i0 + e], mrow[per + i0 + e], z[e], sf);      // element c HW + p: mean at the same offset, logvar C HW further
  }
}

// eight values at i .. i + 7 of a row; entries at or past `per` read as 0
__device__ __forceinline__ void load8(const half_t* row, long i, long per, bool vec, float v[8]) {
  if (vec && i + 8 <= per) {
    const h8 t = *(const h8*)(row + i);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = i + e < per ? (float)row[i + e] : 0.f;
  }
}
// ll = alpha x + (1 - alpha) y in fp32, spelled once: the norm pass and the output pass must see the same bits
__device__ __forceinline__ float mix_f(float a, float b1, float x, float y) { return __fadd_rn(__fmul_rn(a, x), __fmul_rn(b1, y)); }

__device__ __forceinline__ float mix_block_sum(float v, float* red) {      // every thread gets the total; one fixed association
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  __syncthreads();                                                         // (red of the sum before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < MIX_NW; ++w) t = __fadd_rn(t, red[w]);
  return t;
}

__global__ __launch_bounds__(MIX_NT) void polar_mix_kernel(const half_t* x, const half_t* y, half_t* out, long per, MixRows rows) {
  __shared__ float red[MIX_NW];
  const int b = blockIdx.y, tid = threadIdx.x;
  const half_t* xr = x + (long)b * per;
  const half_t* yr = y + (long)b * per;
  half_t* orow = out + (long)b * per;
  const bool vx = (((uintptr_t)xr) & 15) == 0, vy = (((uintptr_t)yr) & 15) == 0, vo = (((uintptr_t)orow) & 15) == 0;
  const float a = rows.alpha[b], b1 = __fsub_rn(1.0f, a);
  float s0 = 0.f, s1 = 0.f, sl = 0.f;
  for (long i = (long)tid * 8; i < per; i += MIX_SLICE) {
    float xv[8], yv[8];
    load8(xr, i, per, vx, xv);
    load8(yr, i, per, vy, yv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {                       // (entries past the row are zeros: they add nothing, in the same place of the chain)
      const float l = mix_f(a, b1, xv[e], yv[e]);
      s0 = __fmaf_rn(xv[e], xv[e], s0);
      s1 = __fmaf_rn(yv[e], yv[e], s1);
      sl = __fmaf_rn(l, l, sl);
    }
  }
  const float n0 = sqrtf(mix_block_sum(s0, red)), n1 = sqrtf(mix_block_sum(s1, red)), nl = sqrtf(mix_block_sum(sl, red));
  const float scale = __fdiv_rn(__fadd_rn(__fmul_rn(a, n0), __fmul_rn(b1, n1)), nl);      // nl = 0: the reference's non-finite result
  for (long i = ((long)blockIdx.x * MIX_NT + tid) * 8; i < per; i += (long)gridDim.x * MIX_SLICE) {
    float xv[8], yv[8];
    load8(xr, i, per, vx, xv);
    load8(yr, i, per, vy, yv);
    if (vo && i + 8 <= per) {
      h8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (half_t)__fmul_rn(mix_f(a, b1, xv[e], yv[e]), scale);
      *(h8*)(orow + i) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (i + e < per) orow[i + e] = (half_t)__fmul_rn(mix_f(a, b1, xv[e], yv[e]), scale);
    }
  }
}

ia2p_status check_rows(const char* what, int B, long long per, long long first) {
  if (B < 1) return fail(nullptr, IA2P_ERR_SHAPE, "%s: B=%d (at least one row)", what, B);
  if (per < 1) return fail(nullptr, IA2P_ERR_SHAPE, "%s: %lld elements per row (at least one)", what, per);
  if (first < 0 || (first & 3)) return fail(nullptr, IA2P_ERR_SHAPE, "%s: first=%lld (a multiple of 4, not negative: a Philox block is four elements)", what, first);
  if (first > MAX_ELEMS || per > MAX_ELEMS - first) return fail(nullptr, IA2P_ERR_SHAPE, "%s: elements %lld .. %lld + %lld pass 2^34 (the block index is one 32-bit counter word)", what, first, first, per);
  return IA2P_OK;
}

}  // namespace

ia2p_status ia2p_randn_seeded(void* stream, void* out, int out_is_f16, int B, int64_t per, int64_t first, const uint64_t* seeds, const uint32_t* draws) {
  if (!out || !seeds || !draws) return fail(nullptr, IA2P_ERR_INVALID, "randn_seeded: null argument");
  if (out_is_f16 != 0 && out_is_f16 != 1) return fail(nullptr, IA2P_ERR_INVALID, "randn_seeded: out_is_f16=%d (0 or 1)", out_is_f16);
  if ((uintptr_t)out & (out_is_f16 ? 1 : 3)) return fail(nullptr, IA2P_ERR_INVALID, "randn_seeded: the output is not aligned to its element size");
  const ia2p_status st = check_rows("randn_seeded", B, (long long)per, (long long)first);
  if (st != IA2P_OK) return st;
  const hipStream_t s = (hipStream_t)stream;
  const size_t esize = out_is_f16 ? 2 : 4;
  const unsigned gx = (unsigned)((per + (long)NT * 8 - 1) / ((long)NT * 8));
  for (int b0 = 0; b0 < B; b0 += MAX_BY_VALUE) {                 // more rows than the arguments hold: in chunks, nothing is copied to the device
    const int nb = B - b0 < MAX_BY_VALUE ? B - b0 : MAX_BY_VALUE;
    NoiseRows rows{};
    for (int r = 0; r < nb; ++r) { rows.seed[r] = seeds[b0 + r]; rows.draw[r] = draws[b0 + r]; }
    void* o = (char*)out + (size_t)b0 * (size_t)per * esize;
    if (out_is_f16) hipLaunchKernelGGL(randn_seeded_kernel<true>, dim3(gx, nb), dim3(NT), 0, s, o, (long)per, (uint32_t)(first >> 2), rows);
    else hipLaunchKernelGGL(randn_seeded_kernel<false>, dim3(gx, nb), dim3(NT), 0, s, o, (long)per, (uint32_t)(first >> 2), rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(nullptr, e, "randn_seeded");
  }
  return IA2P_OK;
}

ia2p_status ia2p_posterior_sample_seeded(void* stream, const void* moments, void* out, int B, int C, int64_t HW, float scaling_factor, const uint64_t* seeds,
                                         const uint32_t* draws) {
  if (!moments || !out || !seeds || !draws) return fail(nullptr, IA2P_ERR_INVALID, "posterior_sample_seeded: null argument");
  if (((uintptr_t)moments | (uintptr_t)out) & 1) return fail(nullptr, IA2P_ERR_INVALID, "posterior_sample_seeded: pointers must be 2-byte aligned");
  if (C < 1 || HW < 1) return fail(nullptr, IA2P_ERR_SHAPE, "posterior_sample_seeded: C=%d HW=%lld must both be >= 1", C, (long long)HW);
  if (HW > MAX_ELEMS / C) return fail(nullptr, IA2P_ERR_SHAPE, "posterior_sample_seeded: C * HW = %d * %lld passes 2^34", C, (long long)HW);
  const long per = (long)C * (long)HW;
  const ia2p_status st = check_rows("posterior_sample_seeded", B, per, 0);
  if (st != IA2P_OK) return st;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned gx = (unsigned)((per + (long)NT * 8 - 1) / ((long)NT * 8));
  for (int b0 = 0; b0 < B; b0 += MAX_BY_VALUE) {
    const int nb = B - b0 < MAX_BY_VALUE ? B - b0 : MAX_BY_VALUE;
    NoiseRows rows{};
    for (int r = 0; r < nb; ++r) { rows.seed[r] = seeds[b0 + r]; rows.draw[r] = draws[b0 + r]; }
    hipLaunchKernelGGL(posterior_seeded_kernel, dim3(gx, nb), dim3(NT), 0, s, (const half_t*)moments + (size_t)b0 * 2 * per, (half_t*)out + (size_t)b0 * per, C,
                       (long)HW, scaling_factor, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(nullptr, e, "posterior_sample_seeded");
  }
  return IA2P_OK;
}

ia2p_status ia2p_polar_mix_v(void* stream, const void* x, const void* y, const float* alphas, void* out, int B, int64_t per) {
  if (!x || !y || !alphas || !out) return fail(nullptr, IA2P_ERR_INVALID, "polar_mix_v: null argument");
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & 1) return fail(nullptr, IA2P_ERR_INVALID, "polar_mix_v: pointers must be 2-byte aligned");
  const ia2p_status st = check_rows("polar_mix_v", B, (long long)per, 0);
  if (st != IA2P_OK) return st;
  const hipStream_t s = (hipStream_t)stream;
  const long slices = (per + MIX_SLICE - 1) / MIX_SLICE;
  const unsigned gx = (unsigned)(slices < MIX_MAX_SLICES ? slices : MIX_MAX_SLICES);
  for (int b0 = 0; b0 < B; b0 += MAX_BY_VALUE) {
    const int nb = B - b0 < MAX_BY_VALUE ? B - b0 : MAX_BY_VALUE;
    MixRows rows{};
    for (int r = 0; r < nb; ++r) rows.alpha[r] = alphas[b0 + r];
    const size_t off = (size_t)b0 * (size_t)per;
    hipLaunchKernelGGL(polar_mix_kernel, dim3(gx, nb), dim3(MIX_NT), 0, s, (const half_t*)x + off, (const half_t*)y + off, (half_t*)out + off, (long)per, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(nullptr, e, "polar_mix_v");
  }
  return IA2P_OK;
}
