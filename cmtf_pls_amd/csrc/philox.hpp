// The counter-based generator shared by synth.hip (noise and NaN mask of the synthetic recipe: streams 0 and 1) and
// impute.hip (hold-out masks: stream 2 + block index): Philox4x32-10 (Salmon et al., SC'11) keyed by a 64-bit seed,
// counter = global element index / 4, word (index % 4) of the block.  An element's draw depends on its global index, the
// stream and the seed only -- not on the launch shape, the vector width or the rank that holds the element.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cmtfpls {

struct Philox4 { uint32_t v[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(uint64_t counter, uint32_t stream, uint64_t key) {
  uint32_t c0 = (uint32_t)counter, c1 = (uint32_t)(counter >> 32), c2 = stream, c3 = 0u;
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ double unit_open(uint32_t x) { return ((double)x + 0.5) * 2.3283064365386963e-10; }   // (0, 1)

}  // namespace cmtfpls
