// Regional IP-Adapter cross-attention for gfx950 (head_dim 64, fp16 in/out, fp32 softmax and accumulation) and the mask pyramid that feeds it.
//
//   out[b, q, h, :] = w0 softmax_j(q . k_text_j / 8) v_text_j + sum_{g < G} s[b] m[b, g, q] softmax_{j in group g}(q . k_ip_j / 8) v_ip_j
//
// (diffusers' `ip_adapter_masks`: every subject's four image tokens ride in one context, each token group has a softmax of its own and acts only where its own spatial
// mask says so). A kernel of its own beside attention_f16_kernel, whose three modes and their selection stay as they are; it shares that kernel's staging, its LDS
// images, its MFMA operand layouts and its store (attention_core.h) and keeps the structure of MODE 1 in its unfolded form: the text segment runs through one merged
// accumulator `o`, undivided, then ONE tile of 4 G <= 64 image-token keys is scaled so that the common final division by l_text leaves the sum above.
//
// Register mapping of the image-token tile. S^T = K . Q^T leaves, in accumulator register r of half kh of a lane of half hh = lane / 32, the score of key
// 32 kh + (r & 3) + 8 (r >> 2) + 4 hh against query lane % 32. The four keys of token group g are keys 4 g .. 4 g + 3: hh = g & 1, r >> 2 = (g >> 1) & 3, kh = g >> 3 --
// the FOUR registers 4 j .. 4 j + 3 of ONE lane. Maximum, exponentials, sum and the per-query coefficient of a group are therefore lane-local: no shuffle, no LDS.
// A lane holds the 8 groups of its parity (4 when 4 G <= 32: one half); its 8 mask weights m[b, g, q] are loaded ahead of the text loop.
//
// m == 0 (and a group g >= G of the padded tile) selects a coefficient of exactly +0: the probability handed to P.V is e * (+0) = +0 with 0 <= e <= 1 finite, so such a
// group's keys and values cannot move a bit of that query's output (tests/test_region_attn_gpu.py: locality, padding).
#include "attention_core.h"

// S^T[key][q] of one 64-key tile (nkh live 32-key halves) -- the qk step of attn_core
__device__ __forceinline__ void region_qk(const char* sKt, const h8 (&qf)[4], int nkh, int r31, int hh, f16v (&st)[2]) {
  h8 kf[2][4];
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    if (kh >= nkh) break;
    const int row = kh * 32 + r31;
    const char* kp = sKt + row * 128;
    const int sw = (row >> 1) & 7;
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[kh][s] = *(const h8*)(kp + (((2 * s + hh) ^ sw) << 4));
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    if (kh >= nkh) break;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[kh][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) st[kh] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kh][s], qf[s], st[kh], 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// V^T fragments of one tile (ds_read_b64_tr_b16), as attn_core reads them
__device__ __forceinline__ void region_vfrag(const char* sVt, int nkh, int lane, h8 (&vf)[2][2][2]) {
  const int hh = lane >> 5, gi = (lane >> 4) & 1, li = lane & 15;
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    if (kh >= nkh) break;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int kb0 = kh * 32 + s2 * 16 + 4 * hh + (li >> 2);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int col = d * 32 + gi * 16 + 4 * (li & 3);
        const int pos = col >> 3, sub = (col & 7) * 2;
        const int r0 = kb0, r1 = kb0 + 8;
        const fp16x4 lo = lds_tr16(sVt + r0 * 128 + ((pos ^ (((r0 >> 1) & 1) << 2)) << 4) + sub);
        const fp16x4 hi = lds_tr16(sVt + r1 * 128 + ((pos ^ (((r1 >> 1) & 1) << 2)) << 4) + sub);
        vf[kh][s2][d][0] = lo[0]; vf[kh][s2][d][1] = lo[1]; vf[kh][s2][d][2] = lo[2]; vf[kh][s2][d][3] = lo[3];
        vf[kh][s2][d][4] = hi[0]; vf[kh][s2][d][5] = hi[1]; vf[kh][s2][d][6] = hi[2]; vf[kh][s2][d][7] = hi[3];
      }
    }
  }
}

__device__ __forceinline__ void region_pv(const h8 (&vf)[2][2][2], const h8 (&pf)[2][2], int nkh, f16v (&o)[2]) {
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    if (kh >= nkh) break;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int d = 0; d < 2; ++d)
        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[kh][s2][d], pf[kh][s2], o[d], 0, 0, 0);
  }
}

__global__ __launch_bounds__(256, 2) void attention_regions_kernel(const half_t* aQ, half_t* aO, int aldq, int aldo, int aB, int aheads, int aNq, int aG, float ascale,
                                                                int axcd, const half_t* aK0, const half_t* aV0, int an0, int ald0, int arpb0, float aw0,
                                                                const half_t* aK1, const half_t* aV1, int ald1, int arpb1, float aw1, const float* aw1b,
                                                                const half_t* aRW) {
  typedef float f2v __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  char* sK = smem;
  char* sV = smem + 32768;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = aG, n0 = an0, n1 = 4 * aG, Nq = aNq;
  int b, hd, qb;
  {      // a contiguous (batch, head, query block) range per XCD, as attention_f16_kernel
    const int nq = (Nq + 127) >> 7, nwg = nq * aheads * aB;
    int bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7, i = bid >> 3;
    if (axcd & 1) bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    qb = bid % nq;
    const int bh = bid / nq;
    hd = bh % aheads; b = bh / aheads;
  }
  const int q0 = qb * 128 + wave * 32;
  const int r31 = lane & 31, hh = lane >> 5;
  const int qc = min(q0 + r31, Nq - 1);      // clamp (rows past the end are computed and discarded)
  h8 qf[4];
  {
    const half_t* qp = aQ + ((size_t)b * Nq + qc) * aldq + hd * 64 + hh * 8;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const h8*)(qp + s * 16);
  }
  // the mask weights of this lane's groups g = 8 kh + 2 j + hh (clamped into [0, G): a group past the end is switched off below), ahead of the text loop
  const int nkhi = n1 <= 32 ? 1 : 2;
  half_t mw[2][4];
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    if (kh >= nkhi) break;      // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = min(8 * kh + 2 * j + hh, G - 1);
      mw[kh][j] = aRW[((size_t)b * G + g) * Nq + qc];
    }
  }

  const half_t* K0 = aK0 + (size_t)b * arpb0 * ald0 + hd * 64;
  const half_t* V0 = aV0 + (size_t)b * arpb0 * ald0 + hd * 64;
  const half_t* K1 = aK1 + (size_t)b * arpb1 * ald1 + hd * 64;
  const half_t* V1 = aV1 + (size_t)b * arpb1 * ald1 + hd * 64;
  const int nt0 = (n0 + 63) >> 6;
  const bool resident = nt0 + 1 <= 4;      // text tiles + the image-token tile in one load phase and one barrier
  if (resident) {
    switch (nt0 + 1) {
      case 2: stage_kv2<2>(K0, V0, ald0, n0, K1, V1, ald1, n1, nt0, tid, sK, sV); break;
      case 3: stage_kv2<3>(K0, V0, ald0, n0, K1, V1, ald1, n1, nt0, tid, sK, sV); break;
      default: stage_kv2<4>(K0, V0, ald0, n0, K1, V1, ald1, n1, nt0, tid, sK, sV); break;
    }
    __syncthreads();
  }

  f16v o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float mrun = MASKED, lrun = 0.f;

  // ---- text segment: the online softmax of attn_core (MODE 1, segment 0), probabilities undivided
#pragma unroll 1
  for (int s0 = 0; s0 < n0; s0 += 256) {
    const int nsk = min(256, n0 - s0), ntile = (nsk + 63) >> 6;
    if (!resident) {
      __syncthreads();      // previous super-tile fully consumed
      switch (ntile) {
        case 1: stage_kv<1>(K0, V0, ald0, s0, nsk, tid, sK, sV); break;
        case 2: stage_kv<2>(K0, V0, ald0, s0, nsk, tid, sK, sV); break;
        case 3: stage_kv<3>(K0, V0, ald0, s0, nsk, tid, sK, sV); break;
        default: stage_kv<4>(K0, V0, ald0, s0, nsk, tid, sK, sV); break;
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int tl = 0; tl < ntile; ++tl) {
      const int k0 = s0 + tl * 64;
      const int nkh = n0 - k0 <= 32 ? 1 : 2;      // wave-uniform: a tile with <= 32 live keys is one half
      f16v st[2];
      region_qk(sK + tl * 8192, qf, nkh, r31, hh, st);
      h8 vf[2][2][2];
      region_vfrag(sV + tl * 8192, nkh, lane, vf);
      __builtin_amdgcn_sched_barrier(0);
      if (k0 + 64 > n0) {      // the last, partial tile: rows past the end were staged as zeros, their scores are masked
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
          if (kh >= nkh) break;
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (k0 + kh * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh >= n0) st[kh][r] = MASKED;
        }
      }
      float mx = st[0][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[0][r]);
      if (nkh == 2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[1][r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(mrun, mx);
      const float mc = mnew * ascale;
      const f2v sc2 = {ascale, ascale}, mc2 = {mc, mc};
      f2v psum2 = {0.f, 0.f};
      h8 pf[2][2];
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        if (kh >= nkh) break;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const f2v t = (f2v){st[kh][r], st[kh][r + 1]} * sc2 - mc2;
          const f2v e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
          psum2 += e;
          const h2 pr = __builtin_convertvector(e, h2);
          pf[kh][r >> 3][r & 7] = pr[0]; pf[kh][r >> 3][(r & 7) + 1] = pr[1];
        }
      }
      if (__any(mnew != mrun)) {
        const float alpha = __builtin_amdgcn_exp2f((mrun - mnew) * ascale);
        lrun *= alpha;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
        mrun = mnew;
      }
      lrun += psum2[0] + psum2[1];
      __builtin_amdgcn_sched_barrier(0);
      region_pv(vf, pf, nkh, o);
    }
  }
  const float lt = lrun + __shfl_xor(lrun, 32, 64);      // softmax denominator of the text segment, final

  // ---- the image-token tile: G groups of four keys, each with its own softmax in four registers of one lane
  const char* sKi = sK + nt0 * 8192;
  const char* sVi = sV + nt0 * 8192;
  if (!resident) {
    __syncthreads();
    stage_kv<1>(K1, V1, ald1, 0, n1, tid, sK, sV);
    __syncthreads();
    sKi = sK; sVi = sV;
  }
  {
    f16v st[2];
    region_qk(sKi, qf, nkhi, r31, hh, st);
    h8 vf[2][2][2];
    region_vfrag(sVi, nkhi, lane, vf);
    __builtin_amdgcn_sched_barrier(0);
    const float sw = (aw1b ? aw1b[b] : aw1) / aw0;      // s[b] / w0: the merged accumulator is multiplied by w0 / l_text at the end
    h8 pf[2][2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      if (kh >= nkhi) break;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int g = 8 * kh + 2 * j + hh;
        const float s0_ = st[kh][4 * j], s1_ = st[kh][4 * j + 1], s2_ = st[kh][4 * j + 2], s3_ = st[kh][4 * j + 3];
        const float mcg = fmaxf(fmaxf(s0_, s1_), fmaxf(s2_, s3_)) * ascale;
        const float e0 = __builtin_amdgcn_exp2f(fmaf(s0_, ascale, -mcg)), e1 = __builtin_amdgcn_exp2f(fmaf(s1_, ascale, -mcg));
        const float e2 = __builtin_amdgcn_exp2f(fmaf(s2_, ascale, -mcg)), e3 = __builtin_amdgcn_exp2f(fmaf(s3_, ascale, -mcg));
        const float lg = ((e0 + e1) + e2) + e3;      // >= 1: the group's maximum contributes exp2(0)
        const float m = (float)mw[kh][j];
        // (s[b] / w0) m l_text / l_g; m == 0 or a group of the padding: exactly +0, whatever the signs of s[b] and w0
        const float c = (g < G && m != 0.f) ? sw * m * lt / lg : 0.f;
        const h2 pa = __builtin_convertvector((f2v){e0 * c, e1 * c}, h2), pb = __builtin_convertvector((f2v){e2 * c, e3 * c}, h2);
        pf[kh][j >> 1][4 * (j & 1)] = pa[0]; pf[kh][j >> 1][4 * (j & 1) + 1] = pa[1];
        pf[kh][j >> 1][4 * (j & 1) + 2] = pb[0]; pf[kh][j >> 1][4 * (j & 1) + 3] = pb[1];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    region_pv(vf, pf, nkhi, o);
  }

  f16v otot[2];
  const float w = aw0 / lt;
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) otot[d][r] = o[d][r] * w;
  __syncthreads();                                  // every wave is through with the K / V images
  attn_store_o(otot, aO, (size_t)aB * Nq * aldo, b, q0, hd, Nq, aldo, smem + wave * 4096, lane, (axcd & 2) != 0);
}

hipError_t ia2p_launch_attention_regions(const AttnArgs& a, const half_t* region_w, int G, hipStream_t s) {
  dim3 grid(((a.Nq + 127) / 128) * a.heads * a.B);
  static bool attr_set[64] = {false};     // per device (the attribute is)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute((const void*)attention_regions_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const int xcd = 1 | (((ia2p_wt_mask() & 8) && (size_t)a.B * a.Nq * a.ldo * 2 < (size_t)0x7ffffff0) ? 2 : 0);
  hipLaunchKernelGGL(attention_regions_kernel, grid, dim3(256), 65536, s, a.Q, a.O, a.ldq, a.ldo, a.B, a.heads, a.Nq, G, a.scale_log2e, xcd,
                     a.seg[0].K, a.seg[0].V, a.seg[0].nkeys, a.seg[0].ld, a.seg[0].rows_per_batch, a.seg[0].weight,
                     a.seg[1].K, a.seg[1].V, a.seg[1].ld, a.seg[1].rows_per_batch, a.seg[1].weight, a.w1_b, region_w);
  return hipGetLastError();
}

// ---- the mask pyramid: masks [B, G, h, w] on the latent grid -> [B, G, (h / f) (w / f)], the mean of each f x f block: an fp32 sum in row-major order (one fixed
// order, one thread per output, no atomics), times 1 / f^2 (a power of two: exact), rounded once to fp16
__global__ __launch_bounds__(256) void region_levels_kernel(const half_t* __restrict__ masks, half_t* __restrict__ out, int n, int h, int w, int f) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int wo = w / f, ho = h / f;
  const int x = i % wo, y = (i / wo) % ho, bg = i / (wo * ho);
  const half_t* src = masks + ((size_t)bg * h + (size_t)y * f) * w + (size_t)x * f;
  float acc = 0.f;
  for (int dy = 0; dy < f; ++dy)
    for (int dx = 0; dx < f; ++dx) acc += (float)src[(size_t)dy * w + dx];
  out[i] = (half_t)(acc * (1.f / (float)(f * f)));
}

hipError_t ia2p_launch_region_levels(const half_t* masks, half_t* out, int B, int G, int h, int w, int f, hipStream_t s) {
  const int n = B * G * (h / f) * (w / f);
  if (n < 1) return hipSuccess;
  hipLaunchKernelGGL(region_levels_kernel, dim3((n + 255) / 256), dim3(256), 0, s, masks, out, n, h, w, f);
  return hipGetLastError();
}
