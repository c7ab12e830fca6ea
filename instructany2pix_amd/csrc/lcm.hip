// The step of the consistency (LCM) sampler (include/ia2p.h, "Consistency sampler"): guidance, the boundary-condition update and the fresh noise that is
// re-injected after every step but the last, per request, in one launch -- with the noise of a seeded request made inside the kernel from the request's own
// Philox stream (normal4.h), so that a few-step request never materialises its step noise.
//
// Per element i of row b, with {g, c_x, c_e, c_n} = coef[b], fp32 arithmetic in ONE order (the _rn intrinsics: no contraction can change it), one rounding to fp16:
//   e = eps_c ? fmaf(g, eps_c - eps_u, eps_u) : eps_u;   o = fmaf(c_e, e, c_x * x);   if (c_n != 0) o = fmaf(c_n, z, o);   out = fp16(o)
// z is fp16 either way: element firsts[b] + i of stream (seeds[b], draws[b]) rounded to fp16 (a seeded row), or noise[b, i]. The rounding makes the seeded
// launch the bits of the pointer launch fed with ia2p_randn_seeded(out_is_f16 = 1, first = firsts[b]). A row with c_n == 0 forms no noise: no Philox block,
// no read of `noise`.
//
// Ownership is by INDEX, as in noise.hip: thread t of a row owns its local elements 8 t .. 8 t + 7 (two Philox blocks), wherever the row lies in memory.
// Each row pointer on a 16-byte boundary is read or written in 16-byte accesses where the eight elements are inside the row; anywhere else the same values
// move in scalar accesses guarded by the index. Nothing about a value depends on which happened, on the grid, on B or on the row's place in the launch.
#include "engine_rt.h"
#include "normal4.h"

namespace {

constexpr int MAX_BY_VALUE = 8;                 // rows whose seeds, draws and firsts travel in the kernel arguments
constexpr int NT = 256;
constexpr long long MAX_ELEMS = 1ll << 34;      // block index j = e >> 2 is one 32-bit counter word

struct LcmRows { uint64_t seed[MAX_BY_VALUE]; int64_t first[MAX_BY_VALUE]; uint32_t draw[MAX_BY_VALUE]; };      // first < 0: the row reads `noise`

// eight values at i .. i + 7 of a row; entries at or past `per` read as 0
__device__ __forceinline__ void load8(const half_t* row, long i, long per, float v[8]) {
  if ((((uintptr_t)row) & 15) == 0 && i + 8 <= per) {
    const h8 t = *(const h8*)(row + i);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = i + e < per ? (float)row[i + e] : 0.f;
  }
}
__device__ __forceinline__ void store8(half_t* row, long i, long per, const h8& v) {
  if ((((uintptr_t)row) & 15) == 0 && i + 8 <= per) *(h8*)(row + i) = v;
  else {
#pragma unroll
    for (int e = 0; e < 8; ++e) if (i + e < per) row[i + e] = v[e];
  }
}

__global__ __launch_bounds__(NT) void lcm_step_kernel(const half_t* x, const half_t* eps_u, const half_t* eps_c, const float* coef, const half_t* noise,
                                                      half_t* out, half_t* out2, long per, LcmRows rows) {
  const int b = blockIdx.y;
  const long i0 = ((long)blockIdx.x * NT + threadIdx.x) * 8;      // local index of this thread's first element
  if (i0 >= per) return;
  const long off = (long)b * per;
  const float g = coef[4 * b], c_x = coef[4 * b + 1], c_e = coef[4 * b + 2], c_n = coef[4 * b + 3];
  float xv[8], e[8], z[8];
  load8(x + off, i0, per, xv);
  load8(eps_u + off, i0, per, e);
  if (eps_c) {
    float ec[8];
    load8(eps_c + off, i0, per, ec);
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = __fmaf_rn(g, __fsub_rn(ec[k], e[k]), e[k]);
  }
  const bool noisy = c_n != 0.f;
  if (noisy) {
    const int64_t first = rows.first[b];
    if (first >= 0) {
      const uint64_t seed = rows.seed[b];
      const uint32_t draw = rows.draw[b];
      const uint32_t j = (uint32_t)((first >> 2) + (i0 >> 2));      // first + per <= 2^34: no wrap
      normal4(seed, draw, j, z);
      if (i0 + 4 < per) normal4(seed, draw, j + 1u, z + 4);
      else { z[4] = z[5] = z[6] = z[7] = 0.f; }
#pragma unroll
      for (int k = 0; k < 8; ++k) z[k] = (float)(half_t)z[k];        // the fp16 a materialised draw would hold
    } else {
      load8(noise + off, i0, per, z);
    }
  }
  h8 v;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float o = __fmaf_rn(c_e, e[k], __fmul_rn(c_x, xv[k]));
    if (noisy) o = __fmaf_rn(c_n, z[k], o);
    v[k] = (half_t)o;
  }
  store8(out + off, i0, per, v);
  if (out2) store8(out2 + off, i0, per, v);
}

}  // namespace

ia2p_status ia2p_lcm_step_v(void* stream, const void* x, const void* eps_u, const void* eps_c, const float* coef, const void* noise, const uint64_t* seeds,
                            const uint32_t* draws, const int64_t* firsts, void* out, void* out2, int B, int64_t per) {
  if (!x || !eps_u || !coef || !out) return fail(nullptr, IA2P_ERR_INVALID, "lcm_step_v: null argument");
  if (((uintptr_t)x | (uintptr_t)eps_u | (uintptr_t)eps_c | (uintptr_t)noise | (uintptr_t)out | (uintptr_t)out2) & 1)
    return fail(nullptr, IA2P_ERR_INVALID, "lcm_step_v: tensor pointers must be 2-byte aligned");
  if ((uintptr_t)coef & 3) return fail(nullptr, IA2P_ERR_INVALID, "lcm_step_v: coef must be 4-byte aligned");
  const int given = (seeds != nullptr) + (draws != nullptr) + (firsts != nullptr);
  if (given != 0 && given != 3) return fail(nullptr, IA2P_ERR_INVALID, "lcm_step_v: seeds, draws and firsts come together or not at all");
  if (B < 1) return fail(nullptr, IA2P_ERR_SHAPE, "lcm_step_v: B=%d (at least one row)", B);
  if (per < 1) return fail(nullptr, IA2P_ERR_SHAPE, "lcm_step_v: %lld elements per row (at least one)", (long long)per);
  for (int b = 0; b < B; ++b) {
    const long long first = firsts ? (long long)firsts[b] : -1;
    if (first < 0) {
      if (!noise) return fail(nullptr, IA2P_ERR_INVALID, "lcm_step_v: row %d is not seeded and there is no noise tensor", b);
      continue;
    }
    if (first & 3) return fail(nullptr, IA2P_ERR_SHAPE, "lcm_step_v: firsts[%d]=%lld (a multiple of 4: a Philox block is four elements)", b, first);
    if (first > MAX_ELEMS || (long long)per > MAX_ELEMS - first)
      return fail(nullptr, IA2P_ERR_SHAPE, "lcm_step_v: row %d: elements %lld .. %lld + %lld pass 2^34 (the block index is one 32-bit counter word)", b, first, first, (long long)per);
  }
  const hipStream_t s = (hipStream_t)stream;
  const unsigned gx = (unsigned)((per + (long)NT * 8 - 1) / ((long)NT * 8));
  for (int b0 = 0; b0 < B; b0 += MAX_BY_VALUE) {                 // more rows than the arguments hold: in chunks, nothing is copied to the device
    const int nb = B - b0 < MAX_BY_VALUE ? B - b0 : MAX_BY_VALUE;
    LcmRows rows{};
    for (int r = 0; r < nb; ++r) {
      rows.first[r] = firsts ? firsts[b0 + r] : -1;
      if (rows.first[r] >= 0) { rows.seed[r] = seeds[b0 + r]; rows.draw[r] = draws[b0 + r]; }
    }
    const size_t off = (size_t)b0 * (size_t)per;
    auto at = [off](const void* p) { return p ? (const half_t*)p + off : (const half_t*)nullptr; };
    hipLaunchKernelGGL(lcm_step_kernel, dim3(gx, nb), dim3(NT), 0, s, at(x), at(eps_u), at(eps_c), coef + 4 * (size_t)b0, at(noise), (half_t*)at(out),
                       (half_t*)at(out2), (long)per, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(nullptr, e, "lcm_step_v");
  }
  return IA2P_OK;
}
