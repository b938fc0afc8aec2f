// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and what the Dropout
// draws make of it (include/nbc.h, nbc_dropout_draws).  One definition for the kernel (dropout_head.hip) and the host
// entry point nbc_dropout_mask: a counter-based generator has no state, so a word depends on (counter, key) alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nbc {

struct Philox4 {
  uint32_t v[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The four random words of quad q (elements 4q .. 4q+3) of draw `draw` of the image with identity `id` under `seed`.
__host__ __device__ __forceinline__ Philox4 dropout_words(uint32_t quad, uint32_t draw, uint64_t id, uint64_t seed) {
  return philox4x32_10(quad, draw, (uint32_t)id, (uint32_t)(id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// An element is dropped iff its word is below T = floor(p 2^32), evaluated in double; p in [0, 1) keeps T below 2^32.
inline uint32_t dropout_threshold(double p) { return (uint32_t)(uint64_t)(p * 4294967296.0); }
// What a kept element is multiplied by: float32(1) / float32(1.0 - p).
inline float dropout_scale(double p) { return 1.0f / (float)(1.0 - p); }
inline bool dropout_p_ok(double p) { return p >= 0.0 && p < 1.0; }   // false for a NaN

}  // namespace nbc
