// The four normals of one Philox block under THE NOISE RULE (include/ia2p.h, "Seeded noise"): the one spelling that noise.hip (the seeded draws) and
// lcm.hip (the step noise of the consistency sampler) share, so that a value made inside either kernel is the same 32 bits.
#pragma once
#include "philox.h"

#include <cmath>

// z[0..3] = elements 4 j .. 4 j + 3 of stream (seed, draw)
__device__ __forceinline__ void normal4(uint64_t seed, uint32_t draw, uint32_t j, float z[4]) {
  uint32_t w[4];
  philox4x32_10(j, draw, 0u, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (float)((w[2 * p] >> 8) + 1u) * 5.9604644775390625e-8f;      // 2^-24: exact, (0, 1]
    const float u2 = (float)(w[2 * p + 1] >> 8) * 5.9604644775390625e-8f;         // [0, 1)
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);                                                 // the argument is exact
    z[2 * p] = __fmul_rn(r, c);
    z[2 * p + 1] = __fmul_rn(r, s);
  }
}
