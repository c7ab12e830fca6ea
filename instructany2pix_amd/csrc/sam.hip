// Kernels of the SAM subject segmenter (sam_engine.hip) on gfx950: attention over a rectangle of the token grid with SAM's decomposed relative-position
// bias (the 14 x 14 windows of the image encoder and its global blocks are the same launch at two rectangle sizes), the mask decoder's attention at head dim 16 / 32,
// the bilinear resize + threshold of the mask logits, and the separable min / max filter of the mask post-processing.
#include "common.h"

// ---- O = softmax(Q K^T / sqrt(D) + rel_h + rel_w) V over one RECTANGLE of the [gh, gw] token grid, from the fused QKV buffer --------------------------------------
// qkv [B * gh * gw, 3H] rows = [q | k | v] in grid order, H = heads * D; out [B * gh * gw, H]. The grid is cut into nwh x nww rectangles of Sh x Sw positions
// (windows: Sh = Sw = 14; a global block: one rectangle, Sh = gh, Sw = gw); a rectangle's positions past the grid's edge are SAM's padding: the reference pads
// AFTER norm1, so such a token's k / v are the QKV bias (read from bqkv [3H], as the audio tower's bias_k row is read), it is a real key, and it is no query.
// score[q][k] = (q . k) scale + q . Rh[qh - kh + Sh - 1] + q . Rw[qw - kw + Sw - 1], the two bias terms on the UNSCALED q (Rh [2 Sh - 1, D], Rw [2 Sw - 1, D]).
// One workgroup per (64-query tile, image x rectangle x head), 4 waves of 16 queries. Per query tile the products q . Rh[r] and q . Rw[r] over ALL table rows are
// two small MFMA passes (table rows as the A operand, straight from HBM / L2); each lane scatters its results to rel[query][kh] / rel[query][Sh + kw] in LDS (fp32),
// so the key loop adds two LDS reads per score. Keys go through LDS in tiles of 64 (K as [key][D], V transposed) with an online softmax in fp32:
// S^T[key][query] = K Q^T per 16-key sub-tile (v_mfma_f32_16x16x16_f16: a lane holds 4 keys of ONE query column), so a column's max / sum are a lane-local fold
// in key order plus two fixed shuffles (deterministic, no atomics), and the fp16 probabilities are already the B operand of O^T += V^T P^T. D = 80 is five
// 16-wide blocks. Sub-tiles wholly past the last key are skipped (196 window keys cost 13 sub-tiles, not 16).
constexpr int RA_QTILE = 64, RA_KTILE = 64, RA_LDS_MAX = 64 * 1024;
template <int D>
__global__ __launch_bounds__(256) void relpos_attention_kernel(const half_t* qkv, half_t* out, const half_t* bqkv, const half_t* Rh, const half_t* Rw,
                                                               int gh, int gw, int Sh, int Sw, int nwh, int nww, int heads, float scale) {
  constexpr int DS = D / 16, LDK = D + 4, LDV = RA_KTILE + 4, NS = RA_KTILE / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  half_t* sK = (half_t*)smem;                              // [64][LDK]
  half_t* sV = sK + RA_KTILE * LDK;                        // [D][LDV]
  int* sHW = (int*)(sV + D * LDV);                         // [64] (kh << 16 | kw) of the tile's keys
  float* sRel = (float*)(sHW + RA_KTILE);                  // [64 queries][LR]
  const int LR = Sh + Sw + 1;
  const int H = heads * D, nkeys = Sh * Sw;
  int y = blockIdx.y;
  const int hd = y % heads; y /= heads;
  const int wx = y % nww; y /= nww;
  const int wy = y % nwh;
  const int b = y / nwh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, grp = lane >> 4;
  const half_t* base = qkv + (size_t)b * gh * gw * 3 * H + hd * D;
  const h4 zero4 = {0, 0, 0, 0};
  // this lane's query (one column of every S^T tile)
  const int qp = blockIdx.x * RA_QTILE + wave * 16 + col;
  const int qh = qp / Sw, qw = qp - qh * Sw;
  const int qy = wy * Sh + qh, qx = wx * Sw + qw;
  const bool qok = qp < nkeys && qy < gh && qx < gw;
  const size_t qrow = (size_t)qy * gw + qx;
  h4 qf[DS];
#pragma unroll
  for (int s = 0; s < DS; ++s) qf[s] = qok ? *(const h4*)(base + qrow * 3 * H + 16 * s + 4 * grp) : zero4;
  // rel[query][kh] = q . Rh[qh - kh + Sh - 1], rel[query][Sh + kw] = q . Rw[qw - kw + Sw - 1]: every table row r against the 16 queries, scattered to its kh = qh + Sh - 1 - r
  float* rel = sRel + (wave * 16 + col) * LR;
#pragma unroll 1
  for (int t2 = 0; t2 < 2; ++t2) {
    const half_t* R = t2 ? Rw : Rh;
    const int S = t2 ? Sw : Sh, q0 = t2 ? qw : qh, nr = 2 * S - 1;
    for (int t = 0; t * 16 < nr; ++t) {
      const int r = 16 * t + col;
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < DS; ++s) {
        const h4 rf = r < nr ? *(const h4*)(R + (size_t)r * D + 16 * s + 4 * grp) : zero4;
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(rf, qf[s], acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = q0 + S - 1 - (16 * t + 4 * grp + i);
        if (k >= 0 && k < S) rel[(t2 ? Sh : 0) + k] = acc[i];
      }
    }
  }
  float m = -INFINITY, sum = 0.f;
  f4 o[DS];
#pragma unroll
  for (int db = 0; db < DS; ++db) o[db] = f4{0.f, 0.f, 0.f, 0.f};
  const float LOG2E = 1.4426950408889634f;
  for (int k0 = 0; k0 < nkeys; k0 += RA_KTILE) {
    __syncthreads();                                 // every wave is done with the previous tile (first pass: nothing; the rel rows are per lane column, read by their own wave only)
    // K rows -> LDS [key][D] (8-byte pieces), V rows -> LDS transposed [d][key]; keys past the rectangle are zero rows, positions past the grid read the bias
    for (int i = threadIdx.x; i < RA_KTILE * (D / 4); i += 256) {
      const int r = i / (D / 4), c4 = (i % (D / 4)) * 4, kk = k0 + r;
      h4 kv = zero4, vv = zero4;
      if (kk < nkeys) {
        const int kh = kk / Sw, kw = kk - kh * Sw, ky = wy * Sh + kh, kx = wx * Sw + kw;
        if (ky < gh && kx < gw) {
          const half_t* p = base + ((size_t)ky * gw + kx) * 3 * H + c4;
          kv = *(const h4*)(p + H); vv = *(const h4*)(p + 2 * H);
        } else {
          kv = *(const h4*)(bqkv + H + hd * D + c4); vv = *(const h4*)(bqkv + 2 * H + hd * D + c4);
        }
        if (c4 == 0) sHW[r] = (kh << 16) | kw;
      } else if (c4 == 0) sHW[r] = 0;
      *(h4*)(sK + r * LDK + c4) = kv;
#pragma unroll
      for (int u = 0; u < 4; ++u) sV[(c4 + u) * LDV + r] = vv[u];
    }
    __syncthreads();
    const int ns = min(NS, (nkeys - k0 + 15) >> 4);      // sub-tiles holding a key (uniform over the workgroup)
    f4 sc[NS];
    float tm = -INFINITY;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (j < ns) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) {
          const h4 kf = *(const h4*)(sK + (16 * j + col) * LDK + 16 * s + 4 * grp);
          acc = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[s], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 16 * j + 4 * grp + i, hw = sHW[r];
          const float v = (fmaf(acc[i], scale, rel[hw >> 16]) + rel[Sh + (hw & 0xffff)]) * LOG2E;
          acc[i] = k0 + r < nkeys ? v : -INFINITY;
          tm = fmaxf(tm, acc[i]);
        }
        sc[j] = acc;
      }
    }
    tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float mn = fmaxf(m, tm);                   // finite: every tile holds at least one key
    const float alpha = exp2f(m - mn);               // (first tile: exp2(-inf) = 0)
    m = mn;
    float ts = 0.f;
    h4 pf[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      pf[j] = zero4;
      if (j < ns) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = exp2f(sc[j][i] - m);       // (masked keys: exp2(-inf) = 0)
          ts += p;
          pf[j][i] = (half_t)p;
        }
      }
    }
    ts += __shfl_xor(ts, 16, 64);
    ts += __shfl_xor(ts, 32, 64);
    sum = fmaf(sum, alpha, ts);
#pragma unroll
    for (int db = 0; db < DS; ++db) {
      f4 acc = o[db] * alpha;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        if (j < ns) {
          const h4 vf = *(const h4*)(sV + (16 * db + col) * LDV + 16 * j + 4 * grp);
          acc = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[j], acc, 0, 0, 0);
        }
      }
      o[db] = acc;
    }
  }
  if (qok) {
    const float inv = 1.f / sum;
    half_t* dst = out + ((size_t)b * gh * gw + qrow) * H + hd * D + 4 * grp;
#pragma unroll
    for (int db = 0; db < DS; ++db) {
      h4 r;
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = (half_t)(o[db][i] * inv);
      *(h4*)(dst + 16 * db) = r;
    }
  }
}

// ---- the mask decoder's attention: out[b, t, h, :] = softmax(q . k^T / sqrt(D)) v per head, D = 16 or 32, any Tq / Tk -----------------------------------------------
// q [B, Tq, heads * D], k / v [B, Tk, heads * D], out as q. One wave per (image, head, query): lane l takes keys l, l + 64, ...; three passes over the keys
// (maximum, sum, weighted values) in fp32, every wave reduction a fixed butterfly. The decoder's products are 7 x 4096, 4096 x 7 and 7 x 7 per head: no tiles to fill.
template <int D>
__global__ __launch_bounds__(256) void small_head_attention_kernel(const half_t* q, const half_t* k, const half_t* v, half_t* out, int B, int Tq, int Tk, int heads, float scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6), rows = (long)B * Tq * heads;
  if (row >= rows) return;
  const int hd = (int)(row % heads);
  const long bt = row / heads;
  const int b = (int)(bt / Tq), H = heads * D;
  const half_t* qp = q + bt * H + hd * D;
  const half_t* kb = k + (size_t)b * Tk * H + hd * D;
  const half_t* vb = v + (size_t)b * Tk * H + hd * D;
  float qv[D];
#pragma unroll
  for (int d = 0; d < D; d += 8) {
    const h8 x = *(const h8*)(qp + d);
#pragma unroll
    for (int u = 0; u < 8; ++u) qv[d + u] = (float)x[u];
  }
  auto score = [&](int t) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 8) {
      const h8 x = *(const h8*)(kb + (size_t)t * H + d);
#pragma unroll
      for (int u = 0; u < 8; ++u) s = fmaf(qv[d + u], (float)x[u], s);
    }
    return s * scale;
  };
  float m = -INFINITY;
  for (int t = lane; t < Tk; t += 64) m = fmaxf(m, score(t));
  m = wave_max(m);
  float sum = 0.f, acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.f;
  for (int t = lane; t < Tk; t += 64) {
    const float p = __expf(score(t) - m);
    sum += p;
#pragma unroll
    for (int d = 0; d < D; d += 8) {
      const h8 x = *(const h8*)(vb + (size_t)t * H + d);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[d + u] = fmaf(p, (float)x[u], acc[d + u]);
    }
  }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  float mine = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float a = wave_sum(acc[d]);
    if (lane == d) mine = a;
  }
  if (lane < D) out[bt * H + hd * D + lane] = (half_t)(mine * inv);
}

// ---- dst[n, y, x] = bilinear(src[n], align_corners = False) (torch F.interpolate), as fp32 logits and / or as the uint8 mask (logit > thr ? 255 : 0) ---------------
// src fp32 [n, sh, sw] with row stride lds and image stride sh_alloc * lds: the crop of SAM's post-processing (the un-padded corner of the padded square) is a
// smaller (sh, sw) over the same strides.
__global__ __launch_bounds__(256) void mask_upsample_kernel(const float* src, float* dstf, unsigned char* dstu, int sh, int sw, int lds, long img_stride, int H, int W, float thr) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  if (x >= W) return;
  const float fy = fmaxf(((float)y + 0.5f) * ((float)sh / (float)H) - 0.5f, 0.f), fx = fmaxf(((float)x + 0.5f) * ((float)sw / (float)W) - 0.5f, 0.f);
  const int y0 = min((int)fy, sh - 1), x0 = min((int)fx, sw - 1), y1 = min(y0 + 1, sh - 1), x1 = min(x0 + 1, sw - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float* s = src + (size_t)n * img_stride;
  const float a = s[(size_t)y0 * lds + x0], b = s[(size_t)y0 * lds + x1], c = s[(size_t)y1 * lds + x0], d = s[(size_t)y1 * lds + x1];
  const float v = (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * c + lx * d);
  const size_t o = ((size_t)n * H + y) * W + x;
  if (dstf) dstf[o] = v;
  if (dstu) dstu[o] = v > thr ? 255 : 0;
}

// ---- one axis of the k-wide min (erode) / max (dilate) filter over a uint8 image: offsets -(k / 2) .. k - k / 2 - 1, pixels outside the image ignored -------------
__global__ __launch_bounds__(256) void mask_morph_axis_kernel(const unsigned char* src, unsigned char* dst, int H, int W, int k, int vertical, int dilate) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const int c = vertical ? y : x, n = vertical ? H : W, lo = max(c - k / 2, 0), hi = min(c + k - k / 2 - 1, n - 1);
  const size_t step = vertical ? (size_t)W : 1;
  const unsigned char* p = src + (vertical ? (size_t)lo * W + x : (size_t)y * W + lo);
  int r = dilate ? 0 : 255;
  for (int i = lo; i <= hi; ++i, p += step) r = dilate ? max(r, (int)*p) : min(r, (int)*p);
  dst[(size_t)y * W + x] = (unsigned char)r;
}

// ---- small pieces of the mask decoder ------------------------------------------------------------------------------------------------------------------------------
// pixel shuffle of a ConvTranspose2d(k = 2, s = 2) computed as a GEMM to 4 Co columns ordered (ky, kx, co): y[b, 2 h + ky, 2 w + kx, co] = g[b, h, w, (ky, kx, co)]
__global__ __launch_bounds__(256) void pixel_shuffle2_kernel(const half_t* g, half_t* y, int Hs, int Ws, int Co, long total8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const int c8 = Co / 8;
  long r = i;
  const int c = (int)(r % c8) * 8; r /= c8;
  const int kx = (int)(r % 2); r /= 2;
  const int ky = (int)(r % 2); r /= 2;
  const int w = (int)(r % Ws); r /= Ws;
  const int h = (int)(r % Hs);
  const long b = r / Hs;
  const h8 v = *(const h8*)(g + i * 8);
  *(h8*)(y + (((b * 2 * Hs + 2 * h + ky) * (long)(2 * Ws)) + 2 * w + kx) * Co + c) = v;
}
// mask[n, p] = sum_c hyper[n, c] up[n, p, c] (fp32 out; C % 8 == 0, any C: a serial chain per pixel): one thread per pixel
__global__ __launch_bounds__(256) void hyper_dot_kernel(const half_t* hyper, long hyper_stride, const half_t* up, float* mask, int P, int C) {
  const int p = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (p >= P) return;
  const half_t* hp = hyper + (size_t)n * hyper_stride;
  const half_t* u = up + ((size_t)n * P + p) * C;
  float acc = 0.f;
  for (int c = 0; c < C; c += 8) {
    const h8 a = *(const h8*)(hp + c), x = *(const h8*)(u + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf((float)a[j], (float)x[j], acc);
  }
  mask[(size_t)n * P + p] = acc;
}

// x[i] = relu(x[i]) (kind 0) or exact GELU (kind 1), in place over fp16 [n]; out[i] = a[i] + b[i % period] (a row block broadcast over images); dst[i] = (float)src[i * ld]
__global__ __launch_bounds__(256) void sam_act_kernel(half_t* x, long n, int kind) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = (float)x[i];
  x[i] = (half_t)(kind ? gelu_erf_f(v) : fmaxf(v, 0.f));
}
__global__ __launch_bounds__(256) void sam_add_rows_kernel(const half_t* a, const half_t* b, half_t* out, long n8, long period8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const h8 x = *(const h8*)(a + i * 8), y = *(const h8*)(b + (i % period8) * 8);
  *(h8*)(out + i * 8) = x + y;
}
__global__ __launch_bounds__(256) void sam_take_col_kernel(const half_t* src, long ld, float* dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (float)src[(size_t)i * ld];
}

// ---- launchers (arguments are checked here: nothing is launched on hipErrorInvalidValue) -----------------------------------------------------------------
// bytes of LDS a relpos attention launch takes; the launcher refuses more than RA_LDS_MAX (a grid too large for the bias rows of 64 queries)
size_t ia2p_relpos_attention_lds(int D, int Sh, int Sw) {
  return (size_t)RA_KTILE * (D + 4) * 2 + (size_t)D * (RA_KTILE + 4) * 2 + RA_KTILE * 4 + (size_t)RA_QTILE * (Sh + Sw + 1) * 4;
}
hipError_t ia2p_launch_relpos_attention(const half_t* qkv, half_t* out, const half_t* bqkv, const half_t* Rh, const half_t* Rw, int B, int gh, int gw, int Sh, int Sw, int heads, int D,
                                        hipStream_t s) {
  if (B < 1 || gh < 1 || gw < 1 || Sh < 1 || Sw < 1 || Sh > 32767 || Sw > 32767 || heads < 1 || (D != 64 && D != 80) || !qkv || !out || !Rh || !Rw) return hipErrorInvalidValue;
  const int nwh = (gh + Sh - 1) / Sh, nww = (gw + Sw - 1) / Sw;
  if ((nwh * Sh != gh || nww * Sw != gw) && !bqkv) return hipErrorInvalidValue;      // padded positions read the bias
  const size_t lds = ia2p_relpos_attention_lds(D, Sh, Sw), gy = (size_t)B * nwh * nww * heads;
  if (lds > (size_t)RA_LDS_MAX || gy > 65535) return hipErrorInvalidValue;
  const dim3 grid((Sh * Sw + RA_QTILE - 1) / RA_QTILE, (unsigned)gy);
  const float scale = 1.f / sqrtf((float)D);
  if (D == 64) hipLaunchKernelGGL(relpos_attention_kernel<64>, grid, dim3(256), lds, s, qkv, out, bqkv, Rh, Rw, gh, gw, Sh, Sw, nwh, nww, heads, scale);
  else hipLaunchKernelGGL(relpos_attention_kernel<80>, grid, dim3(256), lds, s, qkv, out, bqkv, Rh, Rw, gh, gw, Sh, Sw, nwh, nww, heads, scale);
  return hipGetLastError();
}
hipError_t ia2p_launch_small_head_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out, int B, int Tq, int Tk, int heads, int D, hipStream_t s) {
  if (!q || !k || !v || !out || B < 1 || Tq < 1 || Tk < 1 || heads < 1 || (D != 16 && D != 32)) return hipErrorInvalidValue;
  const long rows = (long)B * Tq * heads;
  if ((rows + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
  const float scale = 1.f / sqrtf((float)D);
  if (D == 16) hipLaunchKernelGGL(small_head_attention_kernel<16>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, q, k, v, out, B, Tq, Tk, heads, scale);
  else hipLaunchKernelGGL(small_head_attention_kernel<32>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, q, k, v, out, B, Tq, Tk, heads, scale);
  return hipGetLastError();
}
hipError_t ia2p_launch_mask_upsample(const float* src, float* dstf, unsigned char* dstu, int n, int sh, int sw, int lds, long img_stride, int H, int W, float thr, hipStream_t s) {
  if (!src || (!dstf && !dstu) || n < 1 || n > 65535 || sh < 1 || sw < 1 || lds < sw || H < 1 || H > 65535 || W < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_upsample_kernel, dim3((W + 255) / 256, H, n), dim3(256), 0, s, src, dstf, dstu, sh, sw, lds, img_stride, H, W, thr);
  return hipGetLastError();
}
hipError_t ia2p_launch_mask_morph(const unsigned char* src, unsigned char* dst, unsigned char* tmp, int H, int W, int k, int dilate, hipStream_t s) {
  if (!src || !dst || !tmp || H < 1 || H > 65535 || W < 1 || k < 1 || src == tmp || dst == tmp) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_morph_axis_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, src, tmp, H, W, k, 0, dilate);
  hipLaunchKernelGGL(mask_morph_axis_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, (const unsigned char*)tmp, dst, H, W, k, 1, dilate);
  return hipGetLastError();
}
hipError_t ia2p_launch_pixel_shuffle2(const half_t* g, half_t* y, int B, int Hs, int Ws, int Co, hipStream_t s) {
  if (!g || !y || B < 1 || Hs < 1 || Ws < 1 || Co < 8 || Co % 8) return hipErrorInvalidValue;
  const long total8 = (long)B * Hs * Ws * 4 * (Co / 8);
  hipLaunchKernelGGL(pixel_shuffle2_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, s, g, y, Hs, Ws, Co, total8);
  return hipGetLastError();
}
hipError_t ia2p_launch_hyper_dot(const half_t* hyper, long hyper_stride, const half_t* up, float* mask, int n, int P, int C, hipStream_t s) {
  if (!hyper || !up || !mask || n < 1 || n > 65535 || P < 1 || C < 8 || C % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hyper_dot_kernel, dim3((P + 255) / 256, n), dim3(256), 0, s, hyper, hyper_stride, up, mask, P, C);
  return hipGetLastError();
}
hipError_t ia2p_launch_sam_act(half_t* x, long n, int kind, hipStream_t s) {
  if (!x || n < 1 || (n + 255) / 256 > 0x7fffffffL || (kind != 0 && kind != 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sam_act_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, kind);
  return hipGetLastError();
}
hipError_t ia2p_launch_sam_add_rows(const half_t* a, const half_t* b, half_t* out, long n, long period, hipStream_t s) {
  if (!a || !b || !out || n < 8 || n % 8 || period < 8 || period % 8 || n % period) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sam_add_rows_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, a, b, out, n / 8, period / 8);
  return hipGetLastError();
}
hipError_t ia2p_launch_sam_take_col(const half_t* src, long ld, float* dst, int n, hipStream_t s) {
  if (!src || !dst || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sam_take_col_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, ld, dst, n);
  return hipGetLastError();
}
