// Automatic edit masks (include/ia2p.h, "Automatic edit mask"): the contrast of two noise predictions, thresholded against its own mean and
// dilated on the latent grid. Two launches.
//
// eps_contrast_map: map[b, p] = (sum over k, then c, of |fp32(tgt[b, k, c, p]) - fp32(src[b, k, c, p])|) * inv, inv = fp32(1 / (n C)) from the host. A pixel is one
// sequential chain, k outer, c inner, in the thread that owns it; ownership is by INDEX (thread t of a row's block owns pixels 8 t .. 8 t + 7). Where HW is a
// multiple of 8 and both bases sit on 16-byte boundaries every (k, c) plane starts on one, and the eight values arrive in one 16-byte load; anywhere else the
// same values arrive in scalar loads guarded by the index. The map leaves in 16-byte stores where its row starts on a 16-byte boundary, in scalar stores
// elsewhere. Nothing about a value depends on which happened.
//
// contrast_mask: ONE workgroup of 1024 threads per request, so the mean has one association that depends on HW alone -- thread t adds the groups of 4 at
// (j * 1024 + t) * 4, j = 0, 1, ..., in index order (entries past the row are +0: the map is not negative), the 64 lanes fold by xor-butterfly (offsets 32 .. 1),
// the 16 wave totals are added in wave order. Depth of the tree: 4 ceil(HW / 4096) + 6 + 15 additions. mean = total / fp32(HW), tau = (0.5 ratio) * mean, and
// cell (y, x) is 1 where any map value of its (2 d + 1)^2 window inside the grid is > tau (strict). The window reads the map itself: no intermediate mask, no
// workspace, no atomics. The mask leaves in 16-byte stores where its row starts on a 16-byte boundary. ratio and dilate of up to 8 requests ride in the kernel
// arguments, as the seeds of noise.hip do.
#include "engine_rt.h"

#include <cmath>

namespace {

constexpr int MAX_BY_VALUE = 8;                 // requests whose ratio and dilate travel in the kernel arguments
constexpr int MAP_NT = 256;                     // threads per workgroup of the map kernel, 8 pixels each
constexpr int MASK_NT = 1024, MASK_NW = MASK_NT / 64;
constexpr int MAX_DILATE = 16;
constexpr int MAX_GRID_Y = 65535;

struct MaskRows { float ratio[MAX_BY_VALUE]; int dilate[MAX_BY_VALUE]; };

__global__ __launch_bounds__(MAP_NT) void contrast_map_kernel(const half_t* tgt, const half_t* src, float* map, int n, int C, long HW, float inv) {
  const int b = blockIdx.y;
  const long i0 = ((long)blockIdx.x * MAP_NT + threadIdx.x) * 8;
  if (i0 >= HW) return;
  const long plane0 = (long)b * n * C;
  const bool vec = (HW & 7) == 0 && ((((uintptr_t)tgt) | ((uintptr_t)src)) & 15) == 0;      // then every plane starts on a 16-byte boundary, and i0 + 8 <= HW
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int k = 0; k < n; ++k)
    for (int c = 0; c < C; ++c) {
      const long off = (plane0 + (long)k * C + c) * HW + i0;
      if (vec) {
        const h8 t = *(const h8*)(tgt + off), s = *(const h8*)(src + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = __fadd_rn(acc[e], fabsf(__fsub_rn((float)t[e], (float)s[e])));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (i0 + e < HW) acc[e] = __fadd_rn(acc[e], fabsf(__fsub_rn((float)tgt[off + e], (float)src[off + e])));
      }
    }
  float* row = map + (long)b * HW;
  const bool vo = (((uintptr_t)row) & 15) == 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long i = i0 + 4 * q;
    if (vo && i + 4 <= HW) {
      f4 v = {__fmul_rn(acc[4 * q], inv), __fmul_rn(acc[4 * q + 1], inv), __fmul_rn(acc[4 * q + 2], inv), __fmul_rn(acc[4 * q + 3], inv)};
      *(f4*)(row + i) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (i + e < HW) row[i + e] = __fmul_rn(acc[4 * q + e], inv);
    }
  }
}

__device__ __forceinline__ float mask_block_sum(float v, float* red) {      // every thread gets the total; one fixed association
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < MASK_NW; ++w) t = __fadd_rn(t, red[w]);
  return t;
}

__global__ __launch_bounds__(MASK_NT) void contrast_mask_kernel(const float* map, half_t* mask, float* stats, int h, int w, MaskRows rows) {
  __shared__ float red[MASK_NW];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int HW = h * w;                                        // < 2^31: checked on the host
  const float* row = map + (long)b * HW;
  const bool vm = (((uintptr_t)row) & 15) == 0;
  float s = 0.f;
  for (long i = (long)tid * 4; i < HW; i += (long)MASK_NT * 4) {
    if (vm && i + 4 <= HW) {
      const f4 v = *(const f4*)(row + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __fadd_rn(s, v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __fadd_rn(s, i + e < HW ? row[i + e] : 0.f);
    }
  }
  const float mean = __fdiv_rn(mask_block_sum(s, red), (float)HW);
  const float tau = __fmul_rn(__fmul_rn(0.5f, rows.ratio[b]), mean);
  if (tid == 0) { stats[2 * (long)b] = mean; stats[2 * (long)b + 1] = tau; }
  const int d = rows.dilate[b];
  half_t* orow = mask + (long)b * HW;
  const bool vo = (((uintptr_t)orow) & 15) == 0;
  for (long i0 = (long)tid * 8; i0 < HW; i0 += (long)MASK_NT * 8) {
    half_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long p = i0 + e;
      bool on = false;
      if (p < HW) {
        const int y = (int)(p / w), x = (int)(p % w);
        const int y0 = y - d < 0 ? 0 : y - d, y1 = y + d > h - 1 ? h - 1 : y + d;
        const int x0 = x - d < 0 ? 0 : x - d, x1 = x + d > w - 1 ? w - 1 : x + d;      // clipped to the grid: outside counts 0, a row end does not wrap
        for (int yy = y0; yy <= y1 && !on; ++yy)
          for (int xx = x0; xx <= x1; ++xx)
            if (row[(long)yy * w + xx] > tau) { on = true; break; }
      }
      v[e] = on ? (half_t)1.0f : (half_t)0.0f;
    }
    if (vo && i0 + 8 <= HW) {
      h8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = v[e];
      *(h8*)(orow + i0) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) if (i0 + e < HW) orow[i0 + e] = v[e];
    }
  }
}

}  // namespace

ia2p_status ia2p_eps_contrast_map(void* stream, const void* eps_tgt, const void* eps_src, float* map_out, int B, int n, int C, int64_t HW) {
  if (!eps_tgt || !eps_src || !map_out) return fail(nullptr, IA2P_ERR_INVALID, "eps_contrast_map: null argument");
  if (((uintptr_t)eps_tgt | (uintptr_t)eps_src) & 1) return fail(nullptr, IA2P_ERR_INVALID, "eps_contrast_map: the predictions must be 2-byte aligned");
  if ((uintptr_t)map_out & 3) return fail(nullptr, IA2P_ERR_INVALID, "eps_contrast_map: the map must be 4-byte aligned");
  if (B < 1 || n < 1 || C < 1 || HW < 1) return fail(nullptr, IA2P_ERR_SHAPE, "eps_contrast_map: B=%d n=%d C=%d HW=%lld must all be >= 1", B, n, C, (long long)HW);
  if (B > MAX_GRID_Y) return fail(nullptr, IA2P_ERR_SHAPE, "eps_contrast_map: B=%d (at most %d requests per call)", B, MAX_GRID_Y);
  if ((long long)n * C > (1 << 20) || HW > (1ll << 31) - 1) return fail(nullptr, IA2P_ERR_SHAPE, "eps_contrast_map: n * C = %lld (at most 2^20), HW = %lld (below 2^31)", (long long)n * C, (long long)HW);
  const float inv = 1.0f / (float)(n * C);
  const unsigned gx = (unsigned)((HW + (long)MAP_NT * 8 - 1) / ((long)MAP_NT * 8));
  hipLaunchKernelGGL(contrast_map_kernel, dim3(gx, B), dim3(MAP_NT), 0, (hipStream_t)stream, (const half_t*)eps_tgt, (const half_t*)eps_src, map_out, n, C, (long)HW, inv);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(nullptr, e, "eps_contrast_map");
  return IA2P_OK;
}

ia2p_status ia2p_contrast_mask(void* stream, const float* map, const float* ratio, const int* dilate, void* mask_out, float* stats_out, int B, int h, int w) {
  if (!map || !ratio || !dilate || !mask_out || !stats_out) return fail(nullptr, IA2P_ERR_INVALID, "contrast_mask: null argument");
  if (((uintptr_t)map | (uintptr_t)stats_out) & 3) return fail(nullptr, IA2P_ERR_INVALID, "contrast_mask: the map and the stats must be 4-byte aligned");
  if ((uintptr_t)mask_out & 1) return fail(nullptr, IA2P_ERR_INVALID, "contrast_mask: the mask must be 2-byte aligned");
  if (B < 1 || h < 1 || w < 1) return fail(nullptr, IA2P_ERR_SHAPE, "contrast_mask: B=%d h=%d w=%d must all be >= 1", B, h, w);
  if ((long long)h * w > (1ll << 31) - 1) return fail(nullptr, IA2P_ERR_SHAPE, "contrast_mask: h * w = %lld (below 2^31)", (long long)h * w);
  for (int b = 0; b < B; ++b) {
    if (!std::isfinite(ratio[b]) || !(ratio[b] > 0.f)) return fail(nullptr, IA2P_ERR_SHAPE, "contrast_mask: ratio[%d]=%g (finite and positive)", b, (double)ratio[b]);
    if (dilate[b] < 0 || dilate[b] > MAX_DILATE) return fail(nullptr, IA2P_ERR_SHAPE, "contrast_mask: dilate[%d]=%d (0 .. %d latent cells)", b, dilate[b], MAX_DILATE);
  }
  const size_t HW = (size_t)h * (size_t)w;
  for (int b0 = 0; b0 < B; b0 += MAX_BY_VALUE) {                 // more requests than the arguments hold: in chunks, nothing is copied to the device
    const int nb = B - b0 < MAX_BY_VALUE ? B - b0 : MAX_BY_VALUE;
    MaskRows rows{};
    for (int r = 0; r < nb; ++r) { rows.ratio[r] = ratio[b0 + r]; rows.dilate[r] = dilate[b0 + r]; }
    hipLaunchKernelGGL(contrast_mask_kernel, dim3(nb), dim3(MASK_NT), 0, (hipStream_t)stream, map + (size_t)b0 * HW, (half_t*)mask_out + (size_t)b0 * HW,
                       stats_out + 2 * (size_t)b0, h, w, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(nullptr, e, "contrast_mask");
  }
  return IA2P_OK;
}
