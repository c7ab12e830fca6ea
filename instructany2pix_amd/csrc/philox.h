// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32 with ten rounds): the one block function behind the
// token sampler (sample.hip, counter (step, 0, 0, 0)) and the seeded normal draws (noise.hip, counter (block, draw, 0, 1)). Integer arithmetic only: the four
// words of a block depend on the counter and the key and on nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// the four output words of the block at counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
