// Device code of the ControlNet path (diffusers 0.26.3 ControlNetModel / StableDiffusionXLControlNetPipeline; the reference only prepares the seam:
// instructany2pix/diffusion/ip_adapter/ip_adapter.py:143-148 installs CNAttnProcessor on `pipe.controlnet`, attention_processor.py:481-568):
//   conv3x3_narrow_kernel          the 3x3 convolutions of ControlNetConditioningEmbedding whose input widths (16, 32, 96 channels) neither ia2p_conv3x3 (Cin % 64 == 0)
//                                  nor ia2p_conv_in (Cin * 9 <= 64) takes: `F.silu(conv(x))`, stride 1 or 2
//   residual_add_gnstats_kernel    `sample = sample + residual` of UNet2DConditionModel.forward (down_block_additional_residuals / mid_block_additional_residual, and the
//                                  ControlNet's own `sample = sample + controlnet_cond`), leaving the GroupNorm column sums of the sum for the consumers that fuse their norm
// The zero convolutions are the GEMM family's launch with GemmArgs::rscale (gemm_epilogue.h). The executor that strings them together lives in engine.hip.
#include "engine_rt.h"
#include "gn_fold.h"

// ---- narrow 3x3 convolution, pad 1, channels-last x [B, H, W, Cin] -> y [B, Ho, Wo, Co], w [Co][tap][Cin] (ia2p_launch_pack_conv), Cin % 16 == 0, Co % 16 == 0 ----------
// Implicit GEMM on v_mfma_f32_16x16x16_f16, K walked as [tap][Cin] in steps of 16: a wave owns 16 consecutive output pixels x up to 64 output channels (workgroup: 64 pixels,
// grid.y: blocks of 64 channels). First operand = weights (a lane: 4 input channels of output channel lane & 15), second = pixels (a lane: the same 4 channels of pixel
// lane & 15's tap neighbour, zeros outside the image), so a lane ends up with 4 consecutive output channels of ONE pixel: 8-byte stores. Both operands come straight from
// memory (the 3 x 3 neighbourhoods overlap and the weights are a few KiB: L1 / L2 serve the re-reads); the embedding runs once per request, not per step.
// out = fp16(acc + bias), then -- SILU -- fp16(silu(that)): the activation of an fp16 module output, as the reference's tensors round.
template <bool SILU>
__global__ __launch_bounds__(256) void conv3x3_narrow_kernel(const half_t* x, const half_t* w, const half_t* bias, half_t* y, int B, int H, int W, int Cin, int Co, int stride,
                                                             int Ho, int Wo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pl = lane & 15, kq = lane >> 4;
  const int npix = B * Ho * Wo;
  const int p0 = (blockIdx.x * 4 + wave) * 16;
  if (p0 >= npix) return;                                   // (wave-uniform; no barrier below)
  const int n0 = blockIdx.y * 64;
  const int nf = min(4, (Co - n0) / 16);                    // 16-channel fragments of this block (Co % 16 == 0: whole fragments only)
  const int pp = min(p0 + pl, npix - 1);
  const int b = pp / (Ho * Wo), rem = pp - b * Ho * Wo, oy = rem / Wo, ox = rem - oy * Wo;
  f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f4){0.f, 0.f, 0.f, 0.f};
  const h4 zero4 = {0, 0, 0, 0};
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int iy = oy * stride + ky - 1, ix = ox * stride + kx - 1;
    const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
    const half_t* xs = x + (((size_t)b * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1)) * Cin + kq * 4;      // (clamped, never branched around)
    const half_t* ws = w + ((size_t)(n0 + pl) * 9 + tap) * Cin + kq * 4;
#pragma unroll 2
    for (int kc = 0; kc < Cin; kc += 16) {
      const h4 xv = *(const h4*)(xs + kc);
      const h4 xf = ok ? xv : zero4;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nf) {
          const h4 wf = *(const h4*)(ws + (size_t)j * 16 * 9 * Cin + kc);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(wf, xf, acc[j], 0, 0, 0);      // D[row = channel n0 + 16 j + 4 kq + i][col = pixel pl]
        }
    }
  }
  if (p0 + pl >= npix) return;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nf) {
      const int n = n0 + j * 16 + kq * 4;
      const h4 bv = *(const h4*)(bias + n);
      h4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = (half_t)(acc[j][i] + (float)bv[i]);
        if constexpr (SILU) o[i] = (half_t)silu_f((float)o[i]);
      }
      *(h4*)(y + (size_t)(p0 + pl) * Co + n) = o;
    }
}
hipError_t ia2p_launch_conv3x3_narrow(const half_t* x, const half_t* w, const half_t* bias, half_t* y, int B, int H, int W, int Cin, int Co, int stride, int silu, hipStream_t s) {
  if (B < 1 || H < 1 || W < 1 || Cin < 16 || Cin > 256 || Cin % 16 || Co < 16 || Co % 16 || (stride != 1 && stride != 2)) return hipErrorInvalidValue;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if ((long)B * Ho * Wo > 0x7fffffffL - 64 || (long)B * H * W > 0x7fffffffL) return hipErrorInvalidValue;
  const int npix = B * Ho * Wo;
  const dim3 grid((npix + 63) / 64, (Co + 63) / 64);
  if (grid.y > 65535) return hipErrorInvalidValue;
  if (silu) hipLaunchKernelGGL(conv3x3_narrow_kernel<true>, grid, dim3(256), 0, s, x, w, bias, y, B, H, W, Cin, Co, stride, Ho, Wo);
  else hipLaunchKernelGGL(conv3x3_narrow_kernel<false>, grid, dim3(256), 0, s, x, w, bias, y, B, H, W, Cin, Co, stride, Ho, Wo);
  return hipGetLastError();
}

// ---- y = fp16(x + r) over [M, C] (y may be x), with the GroupNorm column sums of y in the producers' format ---------------------------------------------------------------
// out[(slot * C + c)] = {sum, sum of squares} (fp64) of channel c of y over the `rows` rows of slot `slot`: gn_colstats_kernel's decomposition, thread for thread -- block =
// (slot, span of 64 channels), thread (chunk tx < 8, slice ty < 32) takes the runs of 16 rows ty, ty + 32, ..., fp32 inside a run in row order (gn_seg16_add), fp64 from
// there on, the slices meet in LDS in slice order -- so the sums are, to the bit, what ia2p_gn_colstats returns for the stored tensor. Every element is read and written by
// ONE thread (the last span of a width that is no multiple of 64 leaves its surplus chunks idle instead of re-reading, unlike the read-only pass): in place is safe.
__global__ __launch_bounds__(256) void residual_add_gnstats_kernel(const half_t* x, const half_t* r, half_t* y, int M, int C, int rows, double* out) {
  __shared__ double2 red[32][64];
  const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const int slot = blockIdx.x, c0 = blockIdx.y * 64 + tx * 8;
  const bool act = c0 < C;                                  // (C % 8 == 0)
  const int r0 = slot * rows, nseg = rows / 16;
  double ds[8], dq[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { ds[e] = 0.0; dq[e] = 0.0; }
  if (act)
    for (int sg = ty; sg < nseg; sg += 32) {
      h8 a[16], d[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {                        // (rows divides M: every row of a run exists)
        const size_t o = (size_t)(r0 + sg * 16 + i) * C + c0;
        a[i] = *(const h8*)(x + o); d[i] = *(const h8*)(r + o);
      }
      float s1[8], s2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) { o[e] = (half_t)((float)a[i][e] + (float)d[i][e]); gn_seg16_add((float)o[e], s1[e], s2[e]); }
        *(h8*)(y + (size_t)(r0 + sg * 16 + i) * C + c0) = o;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) { ds[e] += (double)s1[e]; dq[e] += (double)s2[e]; }
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[ty][tx * 8 + e] = make_double2(ds[e], dq[e]);
  __syncthreads();
  if (threadIdx.x < 64 && blockIdx.y * 64 + threadIdx.x < C) {
    double a = 0.0, q = 0.0;
    const int nsl = nseg < 32 ? nseg : 32;
    for (int t = 0; t < nsl; ++t) { const double2 v = red[t][threadIdx.x]; a += v.x; q += v.y; }
    ((double2*)out)[(size_t)slot * C + blockIdx.y * 64 + threadIdx.x] = make_double2(a, q);
  }
}
// the same sum without statistics (a consumer that runs its GroupNorm as a launch of its own; images whose rows no run of 16 divides): 8 elements per thread
__global__ __launch_bounds__(256) void residual_add_kernel(const half_t* x, const half_t* r, half_t* y, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const h8 a = *(const h8*)(x + i * 8), d = *(const h8*)(r + i * 8);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)a[e] + (float)d[e]);
    *(h8*)(y + i * 8) = o;
  }
}
// out == nullptr: no statistics (rows is not read)
hipError_t ia2p_launch_residual_add_gnstats(const half_t* x, const half_t* r, half_t* y, int M, int C, int rows, double* out, hipStream_t s) {
  if (M < 1 || C < 8 || C % 8) return hipErrorInvalidValue;
  if (!out) {
    const long n8 = (long)M * C / 8;
    hipLaunchKernelGGL(residual_add_kernel, dim3((unsigned)std::min<long>((n8 + 255) / 256, 65536)), dim3(256), 0, s, x, r, y, n8);
    return hipGetLastError();
  }
  if (rows < 16 || rows % 16 || M % rows || (C + 63) / 64 > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(residual_add_gnstats_kernel, dim3(M / rows, (C + 63) / 64), dim3(256), 0, s, x, r, y, M, C, rows, out);
  return hipGetLastError();
}
