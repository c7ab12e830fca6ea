// 8-bit image codec at the pipeline boundary: uint8 HWC images <-> the VAE's fp16 NCHW tensors (include/ia2p.h, "image codec").
// Restates diffusers 0.26.3 VaeImageProcessor arithmetic bit for bit:
//   in   pil_to_numpy (q / 255, fp32) -> numpy_to_pt -> normalize (2 v - 1, fp32) -> .to(float16)
//   out  denormalize ((x / 2 + 0.5).clamp(0, 1), fp32) -> numpy_to_pil ((v * 255).round() -> uint8, round half to even)
// Memory-bound element-wise kernels. One thread owns PX pixels of one image: on the 8-bit side that is a contiguous run of PX * C bytes
// (one 16-byte access per channel for C = 1, three for C = 3), on the fp16 side PX halfs of each channel plane (two 16-byte accesses per
// plane), so neighbouring lanes touch neighbouring 16-byte pieces on both sides and no LDS staging is needed. The vector path needs every
// such piece to be 16-byte aligned: H*W a multiple of PX and 16-byte aligned base pointers, decided once per launch on the host; other
// shapes take the scalar path of the same kernel (same arithmetic, same results).
#include "engine_rt.h"

#include <climits>

namespace {

constexpr int PX = 16;      // pixels per thread
constexpr int BLOCK = 256;

// q / 255 rounded once to fp32 (numpy's float32 division), then 2 v - 1 in fp32 (2 v is exact, so contracting it into an FMA changes nothing)
__device__ __forceinline__ half_t code_to_half(uint32_t q, int normalize) {
  const float v = __fdiv_rn((float)q, 255.0f);
  return (half_t)(normalize ? 2.0f * v - 1.0f : v);
}
// (x / 2 + 0.5).clamp(0, 1) in fp32: x / 2 is exact for every fp16 value, so an FMA gives the same bits. NaN stays NaN (torch.clamp propagates it).
__device__ __forceinline__ float half_to_unit(half_t x) {
  const float v = (float)x * 0.5f + 0.5f;
  return v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f);
}
// rint(clamp(...) * 255) with NaN -> 0 (the written-out rule; numpy's cast of NaN to uint8 is undefined)
__device__ __forceinline__ uint32_t half_to_code(half_t x) {
  float v = (float)x * 0.5f + 0.5f;
  v = v > 0.0f ? fminf(v, 1.0f) : 0.0f;
  return (uint32_t)rintf(v * 255.0f);
}

// src u8 [B, HW, C] -> dst fp16 [B, C, HW]
template <int C>
__global__ __launch_bounds__(BLOCK) void image_from_u8_kernel(const uint8_t* __restrict__ src, half_t* __restrict__ dst, int HW, int chunks, int total,
                                                             int normalize, int vec) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int b = t / chunks, p0 = (t - b * chunks) * PX;
  const uint8_t* s = src + ((size_t)b * HW + p0) * C;
  half_t* d = dst + (size_t)b * C * HW + p0;
  if (vec) {                                  // (HW % PX == 0: every chunk is whole)
    uint32_t w[4 * C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const uint4 r = ((const uint4*)s)[i];
      w[4 * i] = r.x; w[4 * i + 1] = r.y; w[4 * i + 2] = r.z; w[4 * i + 3] = r.w;
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < PX / 8; ++h) {
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = (h * 8 + e) * C + c;    // byte k of the run = pixel k / C, channel k % C
          o[e] = code_to_half((w[k >> 2] >> (8 * (k & 3))) & 0xffu, normalize);
        }
        *(h8*)(d + (size_t)c * HW + h * 8) = o;
      }
    return;
  }
  const int n = min(PX, HW - p0);
  for (int j = 0; j < n; ++j)
#pragma unroll
    for (int c = 0; c < C; ++c) d[(size_t)c * HW + j] = code_to_half(s[j * C + c], normalize);
}

// src fp16 [B, C, HW] -> dst [B, HW, C] as uint8 codes (OUT = uint8_t) or as floats in [0, 1] (OUT = float)
template <int C, typename OUT>
__global__ __launch_bounds__(BLOCK) void image_planar_to_hwc_kernel(const half_t* __restrict__ src, OUT* __restrict__ dst, int HW, int chunks, int total, int vec) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int b = t / chunks, p0 = (t - b * chunks) * PX;
  const half_t* s = src + (size_t)b * C * HW + p0;
  OUT* d = dst + ((size_t)b * HW + p0) * C;
  if (vec) {
    half_t x[C][PX];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int h = 0; h < PX / 8; ++h) {
        const h8 v = *(const h8*)(s + (size_t)c * HW + h * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[c][h * 8 + e] = v[e];
      }
    if constexpr (sizeof(OUT) == 1) {         // PX * C bytes = C x 16 bytes
#pragma unroll
      for (int i = 0; i < C; ++i) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t word = 0;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int k = 16 * i + 4 * q + m;
            word |= half_to_code(x[k % C][k / C]) << (8 * m);
          }
          w[q] = word;
        }
        ((uint4*)d)[i] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    } else {                                  // PX * C floats = 4 C x 16 bytes
#pragma unroll
      for (int i = 0; i < 4 * C; ++i) {
        const int k = 4 * i;
        ((float4*)d)[i] = make_float4(half_to_unit(x[k % C][k / C]), half_to_unit(x[(k + 1) % C][(k + 1) / C]),
                                      half_to_unit(x[(k + 2) % C][(k + 2) / C]), half_to_unit(x[(k + 3) % C][(k + 3) / C]));
      }
    }
    return;
  }
  const int n = min(PX, HW - p0);
  for (int j = 0; j < n; ++j)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const half_t v = s[(size_t)c * HW + j];
      if constexpr (sizeof(OUT) == 1) d[j * C + c] = (OUT)half_to_code(v);
      else d[j * C + c] = half_to_unit(v);
    }
}

// flat element-wise maps, 8 elements per thread: MODE 0 = denormalize to float (NCHW "pt" / "np" output of one channel),
// MODE 1 = the 8-bit round trip fp16 -> code -> fp16 in [-1, 1] (dst may alias src: each thread reads its elements before writing them)
template <int MODE, typename OUT>
__global__ __launch_bounds__(BLOCK) void image_map_kernel(const half_t* src, OUT* dst, int n, int vec) {
  const int i0 = (blockIdx.x * BLOCK + threadIdx.x) * 8;
  if (i0 >= n) return;
  auto f = [](half_t v) -> OUT {
    if constexpr (MODE == 0) return half_to_unit(v);
    else return code_to_half(half_to_code(v), 1);
  };
  if (vec && i0 + 8 <= n) {
    const h8 v = *(const h8*)(src + i0);
    if constexpr (MODE == 0) {
      ((float4*)(dst + i0))[0] = make_float4(f(v[0]), f(v[1]), f(v[2]), f(v[3]));
      ((float4*)(dst + i0))[1] = make_float4(f(v[4]), f(v[5]), f(v[6]), f(v[7]));
    } else {
      h8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f(v[e]);
      *(h8*)(dst + i0) = o;
    }
    return;
  }
  const int m = min(8, n - i0);
  for (int e = 0; e < m; ++e) dst[i0 + e] = f(src[i0 + e]);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int blocks_for(long threads) { return (int)((threads + BLOCK - 1) / BLOCK); }

// the checks every image entry point makes before any HIP call
ia2p_status check_image(const char* what, const void* src, const void* dst, int B, int H, int W, int C) {
  if (!src || !dst) return fail(nullptr, IA2P_ERR_INVALID, "%s: null pointer", what);
  if (B < 0 || H < 0 || W < 0) return fail(nullptr, IA2P_ERR_INVALID, "%s: negative size B=%d H=%d W=%d", what, B, H, W);
  if (B < 1 || H < 1 || W < 1) return fail(nullptr, IA2P_ERR_SHAPE, "%s: empty image B=%d H=%d W=%d", what, B, H, W);
  if (C != 1 && C != 3) return fail(nullptr, IA2P_ERR_SHAPE, "%s: C=%d (1 or 3 channels)", what, C);
  if ((int64_t)B * H * W * C > INT_MAX) return fail(nullptr, IA2P_ERR_SHAPE, "%s: %lld elements exceed the 32-bit count of one launch", what,
                                                    (long long)B * H * W * C);
  return IA2P_OK;
}

}  // namespace

ia2p_status ia2p_image_from_u8(void* stream, const void* src, void* dst, int B, int H, int W, int C, int normalize) {
  ia2p_status st = check_image("image_from_u8", src, dst, B, H, W, C);
  if (st != IA2P_OK) return st;
  if (normalize != 0 && normalize != 1) return fail(nullptr, IA2P_ERR_INVALID, "image_from_u8: normalize=%d (0 or 1)", normalize);
  const int HW = H * W, chunks = (HW + PX - 1) / PX, total = B * chunks;
  const int vec = HW % PX == 0 && aligned16(src) && aligned16(dst);
  const hipStream_t s = (hipStream_t)stream;
  if (C == 3) hipLaunchKernelGGL(image_from_u8_kernel<3>, dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const uint8_t*)src, (half_t*)dst, HW, chunks, total, normalize, vec);
  else hipLaunchKernelGGL(image_from_u8_kernel<1>, dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const uint8_t*)src, (half_t*)dst, HW, chunks, total, normalize, vec);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_from_u8");
}

ia2p_status ia2p_image_to_u8(void* stream, const void* src, void* dst, int B, int H, int W, int C) {
  ia2p_status st = check_image("image_to_u8", src, dst, B, H, W, C);
  if (st != IA2P_OK) return st;
  const int HW = H * W, chunks = (HW + PX - 1) / PX, total = B * chunks;
  const int vec = HW % PX == 0 && aligned16(src) && aligned16(dst);
  const hipStream_t s = (hipStream_t)stream;
  if (C == 3) hipLaunchKernelGGL((image_planar_to_hwc_kernel<3, uint8_t>), dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const half_t*)src, (uint8_t*)dst, HW, chunks, total, vec);
  else hipLaunchKernelGGL((image_planar_to_hwc_kernel<1, uint8_t>), dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const half_t*)src, (uint8_t*)dst, HW, chunks, total, vec);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_to_u8");
}

ia2p_status ia2p_image_to_f32(void* stream, const void* src, float* dst, int B, int H, int W, int C, int nhwc) {
  ia2p_status st = check_image("image_to_f32", src, dst, B, H, W, C);
  if (st != IA2P_OK) return st;
  if (nhwc != 0 && nhwc != 1) return fail(nullptr, IA2P_ERR_INVALID, "image_to_f32: nhwc=%d (0 or 1)", nhwc);
  const int HW = H * W;
  const hipStream_t s = (hipStream_t)stream;
  if (nhwc && C == 3) {
    const int chunks = (HW + PX - 1) / PX, total = B * chunks;
    const int vec = HW % PX == 0 && aligned16(src) && aligned16(dst);
    hipLaunchKernelGGL((image_planar_to_hwc_kernel<3, float>), dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const half_t*)src, dst, HW, chunks, total, vec);
  } else {                                    // NCHW, or one channel (NHWC = NCHW)
    const int n = B * C * HW;
    hipLaunchKernelGGL((image_map_kernel<0, float>), dim3(blocks_for(((long)n + 7) / 8)), dim3(BLOCK), 0, s, (const half_t*)src, dst, n,
                       (int)(aligned16(src) && aligned16(dst)));
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_to_f32");
}

ia2p_status ia2p_image_requantize(void* stream, const void* src, void* dst, int64_t n) {
  if (!src || !dst) return fail(nullptr, IA2P_ERR_INVALID, "image_requantize: null pointer");
  if (n < 0) return fail(nullptr, IA2P_ERR_INVALID, "image_requantize: negative size %lld", (long long)n);
  if (n < 1 || n > INT_MAX) return fail(nullptr, IA2P_ERR_SHAPE, "image_requantize: n=%lld (1 .. 2^31-1 elements per launch)", (long long)n);
  hipLaunchKernelGGL((image_map_kernel<1, half_t>), dim3(blocks_for((n + 7) / 8)), dim3(BLOCK), 0, (hipStream_t)stream, (const half_t*)src, (half_t*)dst,
                     (int)n, (int)(aligned16(src) && aligned16(dst)));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "image_requantize");
}
