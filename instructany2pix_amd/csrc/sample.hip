// Token sampler of the instruction LLM (include/ia2p.h, "sampling on the device"): one token per logits row, drawn where the lm_head launch left the row.
// Restates the step transformers' sampling loop applies (llm.py::sample_probs): TemperatureLogitsWarper -> TopKLogitsWarper -> softmax -> one draw, with the
// draw taken from a counter-based generator (Philox4x32-10, key = the request's seed, counter = its step) by inverting the cumulative sum in index order.
//
// One workgroup of 16 waves per row; the row (128 KB at Vicuna's vocabulary, L2-resident behind lm_head) is read in up to six coalesced passes:
//   1  maximum of the scores, NaN / +inf check                      (argmax rows: + one pass for the lowest index of the maximum, done)
//   2-4  radix select of the k-th largest score, 11 / 11 / 10 bits of the order-preserving key per pass, histogram in LDS (integer LDS atomics: the counts
//        do not depend on arrival order); skipped when top_k keeps everything
//   5  sum of exp(score - max) over the kept set
//   6  cumulative sum in index order against u * sum, probabilities out
// Ownership is by INDEX, never by address: wave w owns the contiguous indices [w * seg, (w + 1) * seg), and in step j of its walk lane l owns the four
// indices w * seg + 256 j + 4 l .. + 3 (one 16-byte load where the row pointer is 16-byte aligned and the four are inside the row, four scalar loads
// otherwise -- the same values in the same registers). A lane adds its four terms in index order, the lanes' totals are scanned in lane order, the steps
// are chained in step order and the waves' totals in wave order: every sum has one fixed association, spelled with __fadd_rn, so a row gives the same
// token and the same probs_out bits in every launch, whatever its alignment and whichever rows share the launch.
// The cumulative sum of pass 6 is DEFINED as that association's value at each element; every lane tests its own elements against u * sum and the lowest
// index that passes wins (an integer minimum), so nothing relies on the rounded partial sums being monotone across lanes.
//
// Nucleus (ia2p_sample_tokens_p with top_p < 1; the rule is in include/ia2p.h): between passes 4 and 5 the threshold key rises from the k-th largest score to the
// lowest score of the nucleus. Every entry kept by top-k has the integer mass q = trunc(exp(score - max) * 2^43) (q <= 2^43 and V <= 2^20: any sum of them
// stays below 2^63), Z is the sum of all q, thr = min(trunc((1 - top_p) * Z), Z - 1) (the cap keeps the maximum in the nucleus however (1 - top_p) rounds), and
// the key sought is the lowest one whose T, the mass at or under it, exceeds thr:
//   n0     (top-k active, or V <= 256) one pass writes the (key, q) of the entries with q > 0 into LDS, in arrival order. If they are at most 256 -- top-k 50
//          leaves 50 plus ties -- thread t sums T of entry t and Z over the list, and the lowest qualifying key is an integer minimum: no further pass
//   n1-n3  (otherwise) a second radix select over the same keys with a MASS per bin instead of a count: q goes to the bin of the entry's digit with 64-bit integer
//          LDS atomics, the bins are scanned from the lowest score up, and the digit is the first bin whose inclusive cumulative mass exceeds thr
// Both ways compute the same integers, so which of them ran cannot be seen in the result.
// Integer sums have no association at all, so the nucleus of a row depends on the row, the temperature, top_k and top_p alone. Summation depth d = 1: a term
// is rounded once, when it is truncated to a multiple of 2^-43 of the row's largest term (all such truncations together move T / Z by less than V * 2^-43 <=
// 2^-23 at V = 2^20; 2^-28 at Vicuna's vocabulary), and no sum rounds. What remains between T / Z here and in exact arithmetic is the error of the fp32
// terms themselves (one subtraction, one expf), which the "+ 2" of the tests' band 2 * (d + 2) * 2^-24 stands for. An entry whose q is 0 (a term below
// 2^-43 of the largest) counts as weightless in the selection and is never in a nucleus. Passes 5 and 6 then run as they do without top-p, on the raised key.
#include "engine_rt.h"
#include "philox.h"

#include <climits>
#include <cmath>

namespace {

constexpr int NT = 1024;            // threads per workgroup
constexpr int NW = NT / 64;         // waves
constexpr int STEP = 256;           // indices a wave covers per step (64 lanes x 4)
constexpr int BINS = 2048;          // histogram bins of a radix pass (11 bits; the last pass uses 1024 of them)
constexpr int MAX_BY_VALUE = 8;     // rows whose seeds and steps travel in the kernel arguments
constexpr int CAP = 256;            // weighted survivors of top-k the nucleus is found among in LDS; more than that: passes n1-n3 over the row

struct SampleRows { uint64_t seed[MAX_BY_VALUE]; uint32_t step[MAX_BY_VALUE]; };
struct SampleArgs {
  const float* logits; long ld; int V; float temperature; int top_k; int do_sample;
  double omp;                                        // 1 - top_p, of the nucleus instantiation alone
  const uint64_t* seeds; const uint32_t* steps;      // device staging of a launch of more than MAX_BY_VALUE rows; null: SampleRows
  int* tokens; float* probs; float* u;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): word 0 of the block at counter (step, 0, 0, 0) under key (seed low, seed high)
__device__ __forceinline__ uint32_t philox_word0(uint64_t seed, uint32_t step) {
  uint32_t w[4];
  philox4x32_10(step, 0, 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  return w[0];
}

// four values at indices i .. i + 3 of the row (i a multiple of 4); entries at or past V read as 0 and are skipped by index
__device__ __forceinline__ void load4(const float* row, int i, int V, bool vec, float x[4]) {
  if (vec && i + 4 <= V) {
    const f4 v = *(const f4*)(row + i);
    x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = i + e < V ? row[i + e] : 0.f;
  }
}
// logit / temperature as torch divides (one IEEE division), -0 folded onto +0 so that the integer key orders exactly as `<` does on the floats
__device__ __forceinline__ float score_of(float x, float temperature, int do_sample) {
  const float s = do_sample ? __fdiv_rn(x, temperature) : x;
  return s == 0.f ? 0.f : s;
}
// order-preserving key: a < b as floats <=> key(a) < key(b) as unsigned (NaN never reaches it)
__device__ __forceinline__ uint32_t key_of(float s) {
  const uint32_t b = __float_as_uint(s);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
// inclusive scan over the lanes of a wave, lane order, fixed association (Hillis-Steele)
__device__ __forceinline__ float wave_scan_f(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(v, o, 64); if (lane >= o) v = __fadd_rn(v, t); }
  return v;
}
__device__ __forceinline__ int wave_scan_i(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
  return v;
}

// inclusive scan of 64-bit integers over the lanes of a wave (two 32-bit shuffles per step)
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    if (lane >= o) v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

constexpr float MASS_SCALE = 8796093022208.f;      // 2^43: a term in [0, 1] as a 64-bit integer; 2^20 of them stay below 2^63

// NUCLEUS = false is the kernel of ia2p_sample_tokens as it has always been; true adds the passes n1-n3 (and the LDS of their 64-bit bins)
template <bool NUCLEUS>
__global__ __launch_bounds__(NT) void sample_tokens_kernel(SampleArgs a, SampleRows rows) {
  __shared__ unsigned long long mass[NUCLEUS ? BINS : BINS / 2];      // the counts of passes 2-4 live in the same bytes
  __shared__ unsigned long long redl[NUCLEUS ? NW : 1];
  __shared__ unsigned long long selb[1];
  unsigned* const hist = (unsigned*)mass;
  __shared__ float redf[NW];
  __shared__ int redi[2][NW];
  __shared__ int sel[2];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
  const float* row = a.logits + (long)r * a.ld;
  const bool vec = ((uintptr_t)row & 15) == 0;
  const int seg = (V + NW * STEP - 1) / (NW * STEP) * STEP;      // indices per wave: whole steps
  const int w0 = wave * seg, steps = w0 < V ? (min(V - w0, seg) + STEP - 1) / STEP : 0;      // wave-uniform
  const float T = a.temperature;
  const int ds = a.do_sample;

  // ---- pass 1: maximum, and whether the row can be sampled at all ----
  float mx = -INFINITY;
  int bad = 0;
  for (int j = 0; j < steps; ++j) {
    const int i = w0 + j * STEP + lane * 4;
    float x[4];
    load4(row, i, V, vec, x);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < V) {
        const float s = score_of(x[e], T, ds);
        bad |= (s != s) || s == INFINITY;
        mx = fmaxf(mx, s);
      }
  }
  mx = wave_max(mx);
  if (lane == 0) redf[wave] = mx;
  bad = __syncthreads_or(bad);
#pragma unroll
  for (int w = 0; w < NW; ++w) mx = fmaxf(mx, redf[w]);
  float u = 0.f;
  if (ds) {
    const uint64_t seed = a.seeds ? a.seeds[r] : rows.seed[r];
    const uint32_t step = a.steps ? a.steps[r] : rows.step[r];
    u = (float)(philox_word0(seed, step) >> 8) * 5.9604644775390625e-8f;      // 2^-24: exact
    if (tid == 0 && a.u) a.u[r] = u;
  }
  if (bad || mx == -INFINITY) {            // (uniform) NaN, +inf or nothing finite: no token
    if (tid == 0) a.tokens[r] = -1;
    return;
  }

  if (!ds) {                               // argmax: the lowest index among the maxima
    int first = INT_MAX;
    for (int j = 0; j < steps; ++j) {
      const int i = w0 + j * STEP + lane * 4;
      float x[4];
      load4(row, i, V, vec, x);
#pragma unroll
      for (int e = 3; e >= 0; --e)
        if (i + e < V && score_of(x[e], T, ds) == mx) first = min(first, i + e);
    }
    first = wave_min_i(first);
    if (lane == 0) redi[0][wave] = first;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) first = min(first, redi[0][w]);
    if (tid == 0) a.tokens[r] = first;
    return;
  }

  // ---- passes 2-4: key of the k-th largest score; kept <=> key >= kth ----
  uint32_t kth = 0;                        // top_k <= 0 or >= V: everything is kept
  if (a.top_k > 0 && a.top_k < V) {
    int kk = a.top_k;                      // rank still sought among the keys that share the prefix found so far
#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
      const int shift = p == 0 ? 21 : p == 1 ? 10 : 0, bits = p == 2 ? 10 : 11;
      for (int b = tid; b < BINS; b += NT) hist[b] = 0;
      __syncthreads();
      for (int j = 0; j < steps; ++j) {
        const int i = w0 + j * STEP + lane * 4;
        float x[4];
        load4(row, i, V, vec, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < V) {
            const uint32_t key = key_of(score_of(x[e], T, ds));
            if (p == 0 || (key >> (shift + bits)) == kth) atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], 1u);
          }
      }
      __syncthreads();
      // bins from the top: thread t holds bins 2047 - 2t and 2046 - 2t; the thread whose range of ranks contains kk names the digit
      const int h1 = (int)hist[BINS - 1 - 2 * tid], h0 = (int)hist[BINS - 2 - 2 * tid];
      int incl = wave_scan_i(h1 + h0, lane);
      if (lane == 63) redi[0][wave] = incl;
      __syncthreads();
      for (int w = 0; w < wave; ++w) incl += redi[0][w];
      const int excl = incl - (h1 + h0);
      if (excl < kk && kk <= incl) {
        const bool upper = excl + h1 >= kk;
        sel[0] = upper ? BINS - 1 - 2 * tid : BINS - 2 - 2 * tid;
        sel[1] = upper ? kk - excl : kk - excl - h1;
      }
      __syncthreads();
      kth = (kth << bits) | (uint32_t)sel[0];
      kk = sel[1];
    }
  }

  // ---- pass n0: the weighted survivors of top-k into LDS, when they are few; the lowest key of the nucleus is then found there ----
  bool compacted = false;
  if constexpr (NUCLEUS) {
    unsigned long long* const cq = mass;                       // [CAP] masses, then [CAP] keys: the bins are not needed on this path
    uint32_t* const ckey = (uint32_t*)(mass + CAP);
    if (V <= CAP || kth != 0) {            // (uniform) without a top-k threshold a longer row cannot fit
      __syncthreads();                     // (sel was read at the end of pass 4)
      if (tid == 0) sel[1] = 0;
      __syncthreads();
      for (int j = 0; j < steps; ++j) {
        const int i = w0 + j * STEP + lane * 4;
        float x[4];
        load4(row, i, V, vec, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < V) {
            const float s = score_of(x[e], T, ds);
            const uint32_t key = key_of(s);
            if (key >= kth) {
              const unsigned long long q = (unsigned long long)(expf(__fsub_rn(s, mx)) * MASS_SCALE);
              if (q) {
                const int slot = atomicAdd(&sel[1], 1);          // the order of the slots is arbitrary; nothing below depends on it
                if (slot < CAP) { cq[slot] = q; ckey[slot] = key; }
              }
            }
          }
      }
      __syncthreads();
      const int n = sel[1];                // >= 1: the maximum's own term is 2^43
      compacted = n <= CAP;
      if (compacted) {
        uint32_t cand = 0xFFFFFFFFu;
        if (tid < n) {                     // entry tid: T = mass of the entries at or under its key, Z = mass of all
          const uint32_t mine = ckey[tid];
          unsigned long long Tm = 0, Z = 0;
          for (int j = 0; j < n; ++j) {
            const unsigned long long qj = cq[j];
            Z += qj;
            if (ckey[j] <= mine) Tm += qj;
          }
          unsigned long long thr = (unsigned long long)(a.omp * (double)Z);
          if (thr > Z - 1) thr = Z - 1;
          if (Tm > thr) cand = mine;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cand = min(cand, (uint32_t)__shfl_xor((int)cand, o, 64));
        if (lane == 0) redi[0][wave] = (int)cand;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) cand = min(cand, (uint32_t)redi[0][w]);
        kth = cand;                        // the lowest key with T > thr; the maximum always qualifies
        __syncthreads();                   // (redi)
      }
    }
  }

  // ---- passes n1-n3 (more survivors than fit): the same key by a radix select over the row ----
  if constexpr (NUCLEUS) if (!compacted) {
    uint32_t nth = 0;                      // the digits found so far
    unsigned long long below = 0, thr = 0; // mass of the kept entries under the prefix found so far; what the cumulative mass has to exceed
#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
      const int shift = p == 0 ? 21 : p == 1 ? 10 : 0, bits = p == 2 ? 10 : 11;
      __syncthreads();                     // (hist, sel and selb were read at the end of the pass before)
      for (int b = tid; b < BINS; b += NT) mass[b] = 0;
      __syncthreads();
      for (int j = 0; j < steps; ++j) {
        const int i = w0 + j * STEP + lane * 4;
        float x[4];
        load4(row, i, V, vec, x);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < V) {
            const float s = score_of(x[e], T, ds);
            const uint32_t key = key_of(s);
            if (key >= kth && (p == 0 || (key >> (shift + bits)) == nth)) {
              const unsigned long long q = (unsigned long long)(expf(__fsub_rn(s, mx)) * MASS_SCALE);
              if (q) atomicAdd(&mass[(key >> shift) & ((1u << bits) - 1u)], q);
            }
          }
      }
      __syncthreads();
      // bins from the bottom: thread t holds bins 2t and 2t + 1; the thread whose range of cumulative mass contains thr names the digit
      const unsigned long long m0 = mass[2 * tid], m1 = mass[2 * tid + 1];
      unsigned long long incl = wave_scan_u64(m0 + m1, lane);
      if (lane == 63) redl[wave] = incl;
      __syncthreads();
      unsigned long long front = 0, total = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w == wave) front = total;
        total += redl[w];
      }
      if (p == 0) {                        // total = Z >= 2^43 (the maximum's own term)
        thr = (unsigned long long)(a.omp * (double)total);
        if (thr > total - 1) thr = total - 1;
      }
      const unsigned long long excl = below + front + incl - (m0 + m1);
      if (excl <= thr && thr < excl + m0 + m1) {
        const bool lower = excl + m0 > thr;
        sel[0] = lower ? 2 * tid : 2 * tid + 1;
        selb[0] = lower ? excl : excl + m0;
      }
      __syncthreads();
      nth = (nth << bits) | (uint32_t)sel[0];
      below = selb[0];
    }
    kth = nth;                             // >= the k-th largest key: the select ran over the kept entries only
    __syncthreads();                       // (sel of the last pass)
  }

  // ---- pass 5: sum over the kept set (this wave's chain of step totals; then the waves in order) ----
  auto terms = [&](int i, float t[4]) {    // exp(score - max) of the kept entries at i .. i + 3, 0 elsewhere
    float x[4];
    load4(row, i, V, vec, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = score_of(x[e], T, ds);
      t[e] = i + e < V && key_of(s) >= kth ? expf(__fsub_rn(s, mx)) : 0.f;
    }
  };
  float carry = 0.f;
  for (int j = 0; j < steps; ++j) {
    float t[4];
    terms(w0 + j * STEP + lane * 4, t);
    const float mine = __fadd_rn(__fadd_rn(__fadd_rn(t[0], t[1]), t[2]), t[3]);
    carry = __fadd_rn(carry, __shfl(wave_scan_f(mine, lane), 63, 64));
  }
  __syncthreads();                         // (redf was read after pass 1)
  if (lane == 0) redf[wave] = carry;
  __syncthreads();
  float before = 0.f, total = 0.f;         // sum of the waves in front of this one; sum of all
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w == wave) before = total;
    total = __fadd_rn(total, redf[w]);
  }
  const float thr = __fmul_rn(u, total);

  // ---- pass 6: the first kept index whose inclusive cumulative sum exceeds u * sum; probabilities ----
  int hit = INT_MAX, last = -1;            // last: the highest index with a positive term (taken when rounding leaves no hit)
  float* prow = a.probs ? a.probs + (long)r * V : nullptr;
  carry = 0.f;
  for (int j = 0; j < steps; ++j) {
    const int i = w0 + j * STEP + lane * 4;
    float t[4];
    terms(i, t);
    const float mine = __fadd_rn(__fadd_rn(__fadd_rn(t[0], t[1]), t[2]), t[3]);
    const float incl = wave_scan_f(mine, lane);
    float up = __shfl_up(incl, 1, 64);
    if (lane == 0) up = 0.f;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      q = e == 0 ? t[0] : __fadd_rn(q, t[e]);
      if (t[e] > 0.f) {
        last = i + e;
        if (__fadd_rn(before, __fadd_rn(carry, __fadd_rn(up, q))) > thr) hit = min(hit, i + e);
      }
      if (prow && i + e < V) prow[i + e] = __fdiv_rn(t[e], total);
    }
    carry = __fadd_rn(carry, __shfl(incl, 63, 64));
  }
  hit = wave_min_i(hit);
  last = wave_max_i(last);
  if (lane == 0) { redi[0][wave] = hit; redi[1][wave] = last; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) { hit = min(hit, redi[0][w]); last = max(last, redi[1][w]); }
  if (tid == 0) a.tokens[r] = hit != INT_MAX ? hit : last;
}

}  // namespace

ia2p_status ia2p_sample_tokens_p(void* stream, const float* logits, int64_t ld, int M, int V, float temperature, int top_k, float top_p, int do_sample,
                                 const uint64_t* seeds, const uint32_t* steps, int32_t* tokens_out, float* probs_out, float* u_out) {
  if (!(top_p > 0.f && top_p <= 1.f)) return fail(nullptr, IA2P_ERR_INVALID, "sample_tokens: top_p %g (a float > 0 and <= 1)", top_p);
  if (!logits || !tokens_out) return fail(nullptr, IA2P_ERR_INVALID, "sample_tokens: null argument");
  if (do_sample != 0 && do_sample != 1) return fail(nullptr, IA2P_ERR_INVALID, "sample_tokens: do_sample=%d (0 or 1)", do_sample);
  if (do_sample && (!seeds || !steps)) return fail(nullptr, IA2P_ERR_INVALID, "sample_tokens: sampling needs seeds and steps");
  if (M < 1 || M > 4096) return fail(nullptr, IA2P_ERR_SHAPE, "sample_tokens: M=%d (1..4096 rows)", M);
  if (V < 1 || V > (1 << 20)) return fail(nullptr, IA2P_ERR_SHAPE, "sample_tokens: V=%d (1..2^20)", V);
  if (ld != 0 && ld < V) return fail(nullptr, IA2P_ERR_SHAPE, "sample_tokens: row stride %lld (0: one row for every draw, or at least V=%d)", (long long)ld, V);
  if (((uintptr_t)logits & 3) || ((uintptr_t)tokens_out & 3) || ((uintptr_t)probs_out & 3) || ((uintptr_t)u_out & 3)) return fail(nullptr, IA2P_ERR_INVALID, "sample_tokens: pointers must be 4-byte aligned");
  if (do_sample && !(temperature > 0.f && std::isfinite(temperature))) return fail(nullptr, IA2P_ERR_INVALID, "sample_tokens: temperature %g (positive and finite)", temperature);
  const hipStream_t s = (hipStream_t)stream;
  SampleArgs a{};
  a.logits = logits; a.ld = (long)ld; a.V = V; a.temperature = temperature; a.top_k = top_k; a.do_sample = do_sample;
  a.omp = 1.0 - (double)top_p;
  a.tokens = tokens_out; a.probs = do_sample ? probs_out : nullptr; a.u = do_sample ? u_out : nullptr;
  const auto kernel = do_sample && top_p < 1.f ? sample_tokens_kernel<true> : sample_tokens_kernel<false>;      // top_p = 1, argmax: the kernel without the passes n1-n3
  SampleRows rows{};
  if (!do_sample || M <= MAX_BY_VALUE) {            // nothing is copied to the device
    for (int r = 0; r < M && do_sample; ++r) { rows.seed[r] = seeds[r]; rows.step[r] = steps[r]; }
    hipLaunchKernelGGL(kernel, dim3(M), dim3(NT), 0, s, a, rows);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "sample_tokens");
  }
  // more rows than the arguments hold: seeds and steps go through device memory of this call, copied on `stream`; the call returns after the stream has drained
  void* stage = nullptr;
  const size_t sb = (size_t)M * sizeof(uint64_t), tb = (size_t)M * sizeof(uint32_t);
  hipError_t e = hipMalloc(&stage, sb + tb);
  if (e != hipSuccess) return fail_hip(nullptr, e, "sample_tokens staging");
  a.seeds = (const uint64_t*)stage;
  a.steps = (const uint32_t*)((char*)stage + sb);
  e = hipMemcpyAsync(stage, seeds, sb, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync((char*)stage + sb, steps, tb, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3(M), dim3(NT), 0, s, a, rows);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(stage);
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? IA2P_OK : fail_hip(nullptr, e, "sample_tokens");
}

ia2p_status ia2p_sample_tokens(void* stream, const float* logits, int64_t ld, int M, int V, float temperature, int top_k, int do_sample, const uint64_t* seeds,
                               const uint32_t* steps, int32_t* tokens_out, float* probs_out, float* u_out) {
  return ia2p_sample_tokens_p(stream, logits, ld, M, V, temperature, top_k, 1.f, do_sample, seeds, steps, tokens_out, probs_out, u_out);
}
