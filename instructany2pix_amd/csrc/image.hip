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

// ---- editing inside a mask (include/ia2p.h, "edit mask"): pixel mask -> latent mask, seam feather, 8-bit composite. Integer arithmetic only. ----------------
// One thread owns PX = 16 consecutive pixels of one image row (the last chunk of a row may be shorter). `vec`: W % PX == 0 and 16-byte aligned pointers, so
// that every chunk is whole and starts on a 16-byte boundary in the u8 planes (and on a 32-byte one in the u16 workspace); other shapes run the same
// arithmetic through scalar accesses.
__device__ __forceinline__ uint32_t bin255(uint32_t q) { return q >= 128u ? 255u : 0u; }

// mask u8 [B, H, W] -> out fp16 [B, 1, H / f, W / f]: 1.0 where any pixel of the f x f block is >= 128. One thread per output cell; `pair` (f == 8, an even
// number of cells per row, 16-byte aligned mask): one thread owns two neighbouring cells, reads their 8 rows as 16-byte pieces and stores both halfs as one word.
__global__ __launch_bounds__(BLOCK) void mask_to_latent_kernel(const uint8_t* __restrict__ mask, half_t* __restrict__ out, int H, int W, int f, int total, int pair) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int h = H / f, w = W / f;
  if (pair) {
    const int wp = w >> 1, b = t / (h * wp), r = t - b * h * wp, cy = r / wp, cx = (r - cy * wp) * 2;
    const uint8_t* s = mask + ((size_t)b * H + (size_t)cy * 8) * W + cx * 8;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      const uint4 v = *(const uint4*)(s + (size_t)y * W);
      lo |= (v.x | v.y) & 0x80808080u;        // q >= 128 is bit 7
      hi |= (v.z | v.w) & 0x80808080u;
    }
    const half_t one = (half_t)1.0f, zero = (half_t)0.0f;
    const uint32_t word = (uint32_t)__builtin_bit_cast(uint16_t, lo ? one : zero) | ((uint32_t)__builtin_bit_cast(uint16_t, hi ? one : zero) << 16);
    *(uint32_t*)(out + ((size_t)b * h + cy) * w + cx) = word;
    return;
  }
  const int b = t / (h * w), r = t - b * h * w, cy = r / w, cx = r - cy * w;
  const uint8_t* s = mask + ((size_t)b * H + (size_t)cy * f) * W + (size_t)cx * f;
  uint32_t any = 0;
  for (int y = 0; y < f; ++y)
    for (int x = 0; x < f; ++x) any |= s[(size_t)y * W + x] & 0x80u;
  out[t] = any ? (half_t)1.0f : (half_t)0.0f;
}

// row pass of the box filter: ws[b, y, x] = sum over dx in [-r, r] of bin(mask[b, y, clamp(x + dx)]) (at most 129 * 255: fits 16 bits). A sliding window over
// the thread's chunk: one clamped window sum, then one byte in and one byte out per pixel.
__global__ __launch_bounds__(BLOCK) void mask_feather_rows_kernel(const uint8_t* __restrict__ mask, uint16_t* __restrict__ ws, int W, int chunks, int total, int r, int vec) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int row = t / chunks, x0 = (t - row * chunks) * PX, n = min(PX, W - x0);
  const uint8_t* s = mask + (size_t)row * W;
  auto at = [&](int x) { return bin255(s[min(max(x, 0), W - 1)]); };
  uint32_t sum = 0;
  for (int dx = -r; dx <= r; ++dx) sum += at(x0 + dx);
  uint16_t* d = ws + (size_t)row * W + x0;
  if (vec) {
    uint32_t w[PX / 2];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      w[j >> 1] = (j & 1) ? (w[j >> 1] | (sum << 16)) : sum;
      sum += at(x0 + j + 1 + r) - at(x0 + j - r);
    }
    ((uint4*)d)[0] = make_uint4(w[0], w[1], w[2], w[3]);
    ((uint4*)d)[1] = make_uint4(w[4], w[5], w[6], w[7]);
    return;
  }
  for (int j = 0; j < n; ++j) {
    d[j] = (uint16_t)sum;
    sum += at(x0 + j + 1 + r) - at(x0 + j - r);
  }
}

// column pass and the feather itself: S = sum over dy in [-r, r] of ws[b, clamp(y + dy), x] (exact, at most 129 * 129 * 255), a = (S + A / 2) / A with
// A = (2 r + 1)^2, out = min(bin, a): the ramp falls INSIDE the mask only, so out = 0 wherever the mask is 0.
__global__ __launch_bounds__(BLOCK) void mask_feather_cols_kernel(const uint8_t* __restrict__ mask, const uint16_t* __restrict__ ws, uint8_t* __restrict__ out, int H, int W,
                                                                  int chunks, int total, int r, int vec) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int row = t / chunks, x0 = (t - row * chunks) * PX, n = min(PX, W - x0);
  const int b = row / H, y = row - b * H;
  const uint32_t A = (uint32_t)(2 * r + 1) * (uint32_t)(2 * r + 1);
  uint32_t S[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) S[j] = 0;
  for (int dy = -r; dy <= r; ++dy) {
    const uint16_t* w = ws + ((size_t)b * H + min(max(y + dy, 0), H - 1)) * W + x0;
    if (vec) {
      const uint4 lo = ((const uint4*)w)[0], hi = ((const uint4*)w)[1];
      const uint32_t v[PX / 2] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int j = 0; j < PX; ++j) S[j] += (v[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    } else {
      for (int j = 0; j < n; ++j) S[j] += w[j];
    }
  }
  const uint8_t* m = mask + (size_t)row * W + x0;
  uint8_t* d = out + (size_t)row * W + x0;
  if (vec) {
    const uint4 mv = *(const uint4*)m;
    const uint32_t ms[4] = {mv.x, mv.y, mv.z, mv.w};
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t word = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) word |= min(bin255((ms[q] >> (8 * k)) & 0xffu), (S[4 * q + k] + A / 2) / A) << (8 * k);
      o[q] = word;
    }
    *(uint4*)d = make_uint4(o[0], o[1], o[2], o[3]);
    return;
  }
  for (int j = 0; j < n; ++j) d[j] = (uint8_t)min(bin255(m[j]), (S[j] + A / 2) / A);
}

// out = (a * e + (255 - a) * b + 127) / 255 per byte, a = alpha[b, y, x] shared by the C channels of the pixel: a = 255 gives e, a = 0 gives b, exactly.
// One thread owns PX pixels = PX * C bytes of edited / base / out (C 16-byte pieces each) and PX bytes of alpha. out may alias edited.
template <int C>
__global__ __launch_bounds__(BLOCK) void image_composite_kernel(const uint8_t* edited, const uint8_t* __restrict__ base, const uint8_t* __restrict__ alpha, uint8_t* out,
                                                               int npix, int total, int vec) {
  const int t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int p0 = t * PX;
  auto mix = [](uint32_t a, uint32_t e, uint32_t b) { return (a * e + (255u - a) * b + 127u) / 255u; };
  if (vec) {                                  // (npix % PX == 0: every chunk is whole)
    const uint4 av = *(const uint4*)(alpha + p0);
    const uint32_t as[4] = {av.x, av.y, av.z, av.w};
    uint32_t ew[4 * C], bw[4 * C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const uint4 ev = ((const uint4*)(edited + (size_t)p0 * C))[i], bv = ((const uint4*)(base + (size_t)p0 * C))[i];
      ew[4 * i] = ev.x; ew[4 * i + 1] = ev.y; ew[4 * i + 2] = ev.z; ew[4 * i + 3] = ev.w;
      bw[4 * i] = bv.x; bw[4 * i + 1] = bv.y; bw[4 * i + 2] = bv.z; bw[4 * i + 3] = bv.w;
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int k = 16 * i + 4 * q + m, px = k / C;      // byte k of the run = pixel k / C
          const uint32_t a = (as[px >> 2] >> (8 * (px & 3))) & 0xffu;
          word |= mix(a, (ew[k >> 2] >> (8 * (k & 3))) & 0xffu, (bw[k >> 2] >> (8 * (k & 3))) & 0xffu) << (8 * m);
        }
        o[q] = word;
      }
      ((uint4*)(out + (size_t)p0 * C))[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    return;
  }
  const int n = min(PX, npix - p0);
  for (int j = 0; j < n; ++j) {
    const uint32_t a = alpha[p0 + j];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const size_t k = (size_t)(p0 + j) * C + c;
      out[k] = (uint8_t)mix(a, edited[k], base[k]);
    }
  }
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

// ---- edit-mask launchers (arguments checked in ops_abi.hip) ------------------------------------------------------------------------------------------------
hipError_t ia2p_launch_mask_to_latent(const uint8_t* mask, half_t* out, int B, int H, int W, int f, hipStream_t s) {
  const int h = H / f, w = W / f;
  const int pair = f == 8 && w % 2 == 0 && aligned16(mask) && aligned16(out);
  const int total = B * h * (pair ? w / 2 : w);
  hipLaunchKernelGGL(mask_to_latent_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, mask, out, H, W, f, total, pair);
  return hipGetLastError();
}

hipError_t ia2p_launch_mask_feather_u8(const uint8_t* mask, uint8_t* out, uint16_t* ws, int B, int H, int W, int r, hipStream_t s) {
  const int chunks = (W + PX - 1) / PX, total = B * H * chunks;
  const int vec = W % PX == 0 && aligned16(mask) && aligned16(out) && aligned16(ws);
  hipLaunchKernelGGL(mask_feather_rows_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, mask, ws, W, chunks, total, r, vec);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mask_feather_cols_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, mask, (const uint16_t*)ws, out, H, W, chunks, total, r, vec);
  return hipGetLastError();
}

hipError_t ia2p_launch_image_composite_u8(const uint8_t* edited, const uint8_t* base, const uint8_t* alpha, uint8_t* out, int B, int H, int W, int C, hipStream_t s) {
  const int npix = B * H * W, total = (npix + PX - 1) / PX;
  const int vec = npix % PX == 0 && aligned16(edited) && aligned16(base) && aligned16(alpha) && aligned16(out);
  if (C == 3) hipLaunchKernelGGL(image_composite_kernel<3>, dim3(blocks_for(total)), dim3(BLOCK), 0, s, edited, base, alpha, out, npix, total, vec);
  else hipLaunchKernelGGL(image_composite_kernel<1>, dim3(blocks_for(total)), dim3(BLOCK), 0, s, edited, base, alpha, out, npix, total, vec);
  return hipGetLastError();
}
