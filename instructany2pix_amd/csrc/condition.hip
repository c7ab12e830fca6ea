// Condition maps from the base image (include/ia2p.h, "condition maps"): grey, separable Gaussian blur and the Canny edge detector on 8-bit images, and the
// u8 -> fp16 [B, 3, H, W] conversion a ControlNet's condition embedding takes. Integer arithmetic from end to end: every result is exact and independent of the
// order of summation and of scheduling. No atomics anywhere.
//   grey      Y = (4899 R + 9617 G + 1868 B + 8192) >> 14                                          (OpenCV's 8-bit RGB2GRAY fixed-point rule)
//   gauss     rows: u32 sum q_|i| src[x + i] -> workspace; columns: (sum q_|j| row[y + j] + 2^23) >> 24; taps sum to 4096; replicated border
//   canny     cv::Canny (8-bit input, aperture 3) as restated in include/ia2p.h: Sobel with a replicated border, |dx| + |dy| or dx^2 + dy^2, non-maximum
//             suppression by the 22.5 / 67.5 degree fixed-point sectors, classification into off / weak / strong, hysteresis, 0 / 255 output
// Hysteresis is the only stage that is not a stencil: a weak pixel is an edge iff a chain of weak pixels connects it to a strong one, over any distance. One
// workgroup owns a 64 x 64 tile of the state map, loads it with a 1-pixel halo into LDS, promotes weak pixels next to an edge until nothing in the tile changes
// and writes the promotions back; the host repeats the launch until a round promoted nothing anywhere (a flag word the promoting threads set with plain stores,
// all of them the same value). Promotion is monotone (1 -> 2 only), so a halo byte read while a neighbour writes it back is either value of a pixel that ends
// as 2 anyway: a race costs a round at worst, and the fixed point -- the output -- is unique. No workgroup ever waits for another.
#include "engine_rt.h"

namespace {

constexpr int BLOCK = 256;
inline int blocks_for(long threads) { return (int)((threads + BLOCK - 1) / BLOCK); }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

__device__ __forceinline__ uint32_t grey_of(uint32_t r, uint32_t g, uint32_t b) { return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14; }

// rgb u8 [npix, 3] -> grey u8 [npix]; one thread owns four pixels: 12 bytes in (three words), one word out where both pointers are 4-byte aligned
__global__ __launch_bounds__(BLOCK) void grey_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ grey, int npix, int vec) {
  const int p0 = (blockIdx.x * BLOCK + threadIdx.x) * 4;
  if (p0 >= npix) return;
  if (vec && p0 + 4 <= npix) {
    const uint32_t* s = (const uint32_t*)(rgb + (size_t)p0 * 3);
    const uint32_t w[3] = {s[0], s[1], s[2]};
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int byte = 3 * j + k;
        c[k] = (w[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
      }
      out |= grey_of(c[0], c[1], c[2]) << (8 * j);
    }
    *(uint32_t*)(grey + p0) = out;
    return;
  }
  const int n = min(4, npix - p0);
  for (int j = 0; j < n; ++j) {
    const uint8_t* s = rgb + (size_t)(p0 + j) * 3;
    grey[p0 + j] = (uint8_t)grey_of(s[0], s[1], s[2]);
  }
}

// row pass: ws[row, x, c] = sum over i in [-r, r] of q_|i| * src[row, clamp(x + i), c] (at most 255 * 4096). One thread per element; the taps are kernel arguments.
__global__ __launch_bounds__(BLOCK) void gauss_rows_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ ws, int W, int C, int total, GaussTaps taps, int r) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  const int WC = W * C, row = e / WC, k = e - row * WC, x = k / C, c = k - x * C;
  const uint8_t* s = src + (size_t)row * WC + c;
  uint32_t acc = (uint32_t)taps.q[0] * s[x * C];
  for (int i = 1; i <= r; ++i) acc += (uint32_t)taps.q[i] * ((uint32_t)s[min(x + i, W - 1) * C] + (uint32_t)s[max(x - i, 0) * C]);
  ws[e] = acc;
}

// column pass: acc = sum over j of q_|j| * ws[b, clamp(y + j), x, c] (at most 255 * 2^24: fits 32 bits), dst = (acc + 2^23) >> 24
__global__ __launch_bounds__(BLOCK) void gauss_cols_kernel(const uint32_t* __restrict__ ws, uint8_t* __restrict__ dst, int H, int WC, int total, GaussTaps taps, int r) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  const int row = e / WC, k = e - row * WC, b = row / H, y = row - b * H;
  const uint32_t* s = ws + (size_t)b * H * WC + k;
  uint32_t acc = (uint32_t)taps.q[0] * s[(size_t)y * WC];
  for (int j = 1; j <= r; ++j) acc += (uint32_t)taps.q[j] * (s[(size_t)min(y + j, H - 1) * WC] + s[(size_t)max(y - j, 0) * WC]);
  dst[e] = (uint8_t)((acc + (1u << 23)) >> 24);
}

// ---- Canny, first pass: gradients, magnitude, non-maximum suppression, classification -> one state byte per pixel (0 off, 1 weak, 2 strong) -------------------
// A workgroup owns a CTW x CTH tile. The grey tile with a 2-pixel halo (coordinates clamped: the replicated border) is staged in LDS, the magnitude of the tile
// with a 1-pixel halo (0 outside the image) is computed there, so the magnitude never goes to memory.
constexpr int CTW = 64, CTH = 16;
constexpr int GW = CTW + 4, GH = CTH + 4, MW = CTW + 2, MH = CTH + 2;

__device__ __forceinline__ void sobel_at(const uint8_t (*g)[GW], int y, int x, int& dx, int& dy) {
  const int a = g[y - 1][x - 1], b = g[y - 1][x], c = g[y - 1][x + 1], d = g[y][x - 1], f = g[y][x + 1], p = g[y + 1][x - 1], q = g[y + 1][x], t = g[y + 1][x + 1];
  dx = (c + 2 * f + t) - (a + 2 * d + p);
  dy = (p + 2 * q + t) - (a + 2 * b + c);
}

__global__ __launch_bounds__(BLOCK) void canny_classify_kernel(const uint8_t* __restrict__ grey, uint8_t* __restrict__ state, int H, int W, int tx_n, int ty_n,
                                                               int lo, int hi, int l2) {
  __shared__ uint8_t g[GH][GW];
  __shared__ int m[MH][MW + 1];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tx_n, rest = blockIdx.x / tx_n, ty = rest % ty_n, b = rest / ty_n;
  const int x0 = tx * CTW, y0 = ty * CTH;
  const uint8_t* gi = grey + (size_t)b * H * W;
  for (int i = tid; i < GH * GW; i += BLOCK) {
    const int ly = i / GW, lx = i - ly * GW;
    const int gy = min(max(y0 - 2 + ly, 0), H - 1), gx = min(max(x0 - 2 + lx, 0), W - 1);
    g[ly][lx] = gi[(size_t)gy * W + gx];
  }
  __syncthreads();
  for (int i = tid; i < MH * MW; i += BLOCK) {
    const int my = i / MW, mx = i - my * MW;
    const int iy = y0 - 1 + my, ix = x0 - 1 + mx;
    int v = 0;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      int dx, dy;
      sobel_at(g, my + 1, mx + 1, dx, dy);
      v = l2 ? dx * dx + dy * dy : abs(dx) + abs(dy);
    }
    m[my][mx] = v;
  }
  __syncthreads();
  uint8_t* so = state + (size_t)b * H * W;
  for (int i = tid; i < CTH * CTW; i += BLOCK) {
    const int py = i / CTW, px = i - py * CTW;
    const int iy = y0 + py, ix = x0 + px;
    if (iy >= H || ix >= W) continue;
    const int my = py + 1, mx = px + 1, mm = m[my][mx];
    int st = 0;
    if (mm > lo) {
      int dx, dy;
      sobel_at(g, py + 2, px + 2, dx, dy);
      const int ax = abs(dx), ay = abs(dy) << 15, t22 = ax * 13573;
      bool keep;
      if (ay < t22) keep = mm > m[my][mx - 1] && mm >= m[my][mx + 1];
      else if (ay > t22 + (ax << 16)) keep = mm > m[my - 1][mx] && mm >= m[my + 1][mx];
      else {
        const int s = (dx ^ dy) < 0 ? -1 : 1;
        keep = mm > m[my - 1][mx - s] && mm > m[my + 1][mx + s];
      }
      if (keep) st = mm > hi ? 2 : 1;
    }
    so[(size_t)iy * W + ix] = (uint8_t)st;
  }
}

// ---- Canny, hysteresis: one round over every HT x HT tile of the state map ----------------------------------------------------------------------------------
// Thread t owns 16 consecutive pixels of row t / 4 of the tile and sweeps them left to right, then right to left, so that a chain along a row crosses the
// segment in one iteration; LDS is updated in place (another thread reads 1 or 2 of a pixel that ends as 2). The loop ends after an iteration in which no thread
// of the workgroup promoted anything: nothing was written in it, so every thread saw the final state and the tile is at its fixed point under this halo.
constexpr int HT = 64, HS = HT + 2, HP = HS + 2;

__global__ __launch_bounds__(BLOCK) void canny_hysteresis_kernel(uint8_t* state, uint32_t* flag, int H, int W, int tx_n, int ty_n) {
  __shared__ uint8_t s[HS][HP];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tx_n, rest = blockIdx.x / tx_n, ty = rest % ty_n, b = rest / ty_n;
  const int x0 = tx * HT, y0 = ty * HT;
  uint8_t* st = state + (size_t)b * H * W;
  for (int i = tid; i < HS * HS; i += BLOCK) {
    const int ly = i / HS, lx = i - ly * HS;
    const int iy = y0 - 1 + ly, ix = x0 - 1 + lx;
    s[ly][lx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? st[(size_t)iy * W + ix] : (uint8_t)0;
  }
  __syncthreads();
  const int y = (tid >> 2) + 1, c0 = (tid & 3) * 16 + 1;
  uint32_t mine = 0;                          // bit j: pixel j of the segment was promoted by this thread
  auto visit = [&](int j) {
    const int x = c0 + j;
    if (s[y][x] != 1) return 0;
    const int edge = (s[y - 1][x - 1] == 2) | (s[y - 1][x] == 2) | (s[y - 1][x + 1] == 2) | (s[y][x - 1] == 2) | (s[y][x + 1] == 2) | (s[y + 1][x - 1] == 2) |
                     (s[y + 1][x] == 2) | (s[y + 1][x + 1] == 2);
    if (!edge) return 0;
    s[y][x] = 2;
    mine |= 1u << j;
    return 1;
  };
  for (;;) {
    int changed = 0;
    for (int j = 0; j < 16; ++j) changed |= visit(j);
    for (int j = 14; j >= 0; --j) changed |= visit(j);
    if (!__syncthreads_or(changed)) break;
  }
  if (mine) {                                 // (a weak pixel is inside the image: what lies outside was loaded as 0)
    const int iy = y0 + y - 1;
    for (int j = 0; j < 16; ++j)
      if (mine & (1u << j)) st[(size_t)iy * W + (x0 + c0 - 1 + j)] = 2;
    *flag = 1u;
  }
}

// state u8 [n] -> edges u8 [n]: 255 where the state is 2, else 0; four pixels per thread
__global__ __launch_bounds__(BLOCK) void canny_finish_kernel(const uint8_t* __restrict__ state, uint8_t* __restrict__ edges, int n, int vec) {
  const int p0 = (blockIdx.x * BLOCK + threadIdx.x) * 4;
  if (p0 >= n) return;
  if (vec && p0 + 4 <= n) {
    const uint32_t w = *(const uint32_t*)(state + p0);
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) out |= (((w >> (8 * j)) & 0xffu) == 2u ? 255u : 0u) << (8 * j);
    *(uint32_t*)(edges + p0) = out;
    return;
  }
  const int m = min(4, n - p0);
  for (int j = 0; j < m; ++j) edges[p0 + j] = state[p0 + j] == 2 ? 255 : 0;
}

// map u8 [B, HW] -> dst fp16 [B, 3, HW]: q / 255 rounded once to fp32, once to fp16 (image.hip's code_to_half without normalisation), the same half in all three planes
__global__ __launch_bounds__(BLOCK) void condition_from_u8_c1_kernel(const uint8_t* __restrict__ map, half_t* __restrict__ dst, int HW, int total) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= total) return;
  const int b = p / HW, o = p - b * HW;
  const half_t v = (half_t)__fdiv_rn((float)map[p], 255.0f);
  half_t* d = dst + (size_t)b * 3 * HW + o;
  d[0] = v;
  d[HW] = v;
  d[2 * (size_t)HW] = v;
}

}  // namespace

// ---- launchers (arguments checked in ops_abi.hip) ---------------------------------------------------------------------------------------------------------
hipError_t ia2p_launch_grey_u8(const uint8_t* rgb, uint8_t* grey, int npix, hipStream_t s) {
  hipLaunchKernelGGL(grey_kernel, dim3(blocks_for(((long)npix + 3) / 4)), dim3(BLOCK), 0, s, rgb, grey, npix, (int)(aligned4(rgb) && aligned4(grey)));
  return hipGetLastError();
}

hipError_t ia2p_launch_gauss_u8(const uint8_t* src, uint8_t* dst, uint32_t* ws, int B, int H, int W, int C, const GaussTaps& taps, int r, hipStream_t s) {
  const int total = B * H * W * C;
  hipLaunchKernelGGL(gauss_rows_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, src, ws, W, C, total, taps, r);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gauss_cols_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, (const uint32_t*)ws, dst, H, W * C, total, taps, r);
  return hipGetLastError();
}

hipError_t ia2p_launch_canny_classify(const uint8_t* grey, uint8_t* state, int B, int H, int W, int lo, int hi, int l2, hipStream_t s) {
  const int tx_n = (W + CTW - 1) / CTW, ty_n = (H + CTH - 1) / CTH;
  hipLaunchKernelGGL(canny_classify_kernel, dim3(B * tx_n * ty_n), dim3(BLOCK), 0, s, grey, state, H, W, tx_n, ty_n, lo, hi, l2);
  return hipGetLastError();
}

// ring(H, W): the pixels of one image that lie on the outermost ring of their hysteresis tile -- the only pixels another tile ever reads
static int64_t canny_ring_pixels(int H, int W) {
  auto inner = [](int n) {                    // sum over the tiles along one axis of max(extent - 2, 0)
    int64_t v = 0;
    for (int o = 0; o < n; o += HT) v += std::max(std::min(HT, n - o) - 2, 0);
    return v;
  };
  return (int64_t)H * W - inner(H) * inner(W);
}

// The most rounds (launches over all tiles) the hysteresis can take, the last one -- which promotes nothing -- included: 2 B ring(H, W) + 2. Argument (DESIGN.md
// §22): a tile leaves every round at its fixed point under the halo it loaded, and only its own workgroup writes its interior; so a tile promotes in round
// k >= 2 only if a halo byte it loads is 2 that was not 2 at its load of round k - 1, i.e. a ring pixel of a neighbour promoted in round k - 1 or k. A ring pixel is
// promoted once, so it accounts for at most two rounds; round 1 and the final round are the + 2.
int64_t ia2p_canny_round_bound(int B, int H, int W) { return 2 * (int64_t)B * canny_ring_pixels(H, W) + 2; }

// Rounds in groups of up to four, each with its own flag word, then one 16-byte copy back and one synchronisation per group; rounds launched past the fixed
// point promote nothing. *rounds = the first round that promoted nothing (counted from 1), *converged = false when `bound` rounds were not enough.
hipError_t ia2p_run_canny_hysteresis(uint8_t* state, uint32_t* flags, int B, int H, int W, int64_t bound, int64_t* rounds, bool* converged, hipStream_t s) {
  const int tx_n = (W + HT - 1) / HT, ty_n = (H + HT - 1) / HT;
  *converged = false;
  *rounds = 0;
  for (int64_t done = 0; done < bound;) {
    const int n = (int)std::min<int64_t>(4, bound - done);
    hipError_t e = hipMemsetAsync(flags, 0, 16, s);
    if (e != hipSuccess) return e;
    for (int i = 0; i < n; ++i) {
      hipLaunchKernelGGL(canny_hysteresis_kernel, dim3(B * tx_n * ty_n), dim3(BLOCK), 0, s, state, flags + i, H, W, tx_n, ty_n);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    uint32_t host[4] = {1u, 1u, 1u, 1u};
    e = hipMemcpyAsync(host, flags, 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    for (int i = 0; i < n; ++i)
      if (host[i] == 0u) {
        *rounds = done + i + 1;
        *converged = true;
        return hipSuccess;
      }
    done += n;
    *rounds = done;
  }
  return hipSuccess;
}

hipError_t ia2p_launch_canny_finish(const uint8_t* state, uint8_t* edges, int n, hipStream_t s) {
  hipLaunchKernelGGL(canny_finish_kernel, dim3(blocks_for(((long)n + 3) / 4)), dim3(BLOCK), 0, s, state, edges, n, (int)(aligned4(state) && aligned4(edges)));
  return hipGetLastError();
}

hipError_t ia2p_launch_condition_from_u8_c1(const uint8_t* map, half_t* dst, int B, int HW, hipStream_t s) {
  const int total = B * HW;
  hipLaunchKernelGGL(condition_from_u8_c1_kernel, dim3(blocks_for(total)), dim3(BLOCK), 0, s, map, dst, HW, total);
  return hipGetLastError();
}
