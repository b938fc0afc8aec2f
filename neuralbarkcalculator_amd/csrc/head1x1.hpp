// The pixel fragment of classifier.4 (head1x1_body in pointwise.hip, head1x1_dropout_kernel in dropout_head.hip): a lane's
// eight input channels of one pixel, loaded in the stored form and decoded to f32.  Both kernels read their operands through
// this one pair, which is what keeps "p = 0 gives the forward's logits bit for bit" true.
#pragma once
#include <hip/hip_runtime.h>

#include "split16.hpp"

namespace nbc {

// 16-byte loads per lane and pixel: PREC 0 = f32 and 2 = f16x2 take two, 1 = bf16 one
template <int PREC>
struct Head1x1Raw {
  static constexpr int VPP = PREC == 1 ? 1 : 2;
  uint4 v[VPP];
};

// channels 8 cl .. 8 cl + 7 of pixel m of x [.][CIN] stored elements
template <int PREC, int CIN>
__device__ __forceinline__ Head1x1Raw<PREC> head1x1_load(const void* __restrict__ x, int m, int cl) {
  constexpr int VPP = Head1x1Raw<PREC>::VPP;
  Head1x1Raw<PREC> raw;
  if constexpr (PREC == 2) {      // h0 chunk cl % 4 of group cl / 4, and its h1 chunk 64 bytes on
    const uint4* xp = reinterpret_cast<const uint4*>(static_cast<const unsigned char*>(x) + (size_t)m * CIN * 4 +
                                                     (cl >> 2) * 128 + (cl & 3) * 16);
    raw.v[0] = xp[0];
    raw.v[VPP - 1] = xp[4];
  } else {
    const uint4* xp = reinterpret_cast<const uint4*>(static_cast<const unsigned char*>(x) +
                                                     ((size_t)m * CIN + cl * 8) * (PREC == 0 ? 4 : 2));
#pragma unroll
    for (int k = 0; k < VPP; ++k) raw.v[k] = xp[k];
  }
  return raw;
}

template <int PREC>
__device__ __forceinline__ void head1x1_decode(const Head1x1Raw<PREC>& raw, float (&f)[8]) {
  constexpr int VPP = Head1x1Raw<PREC>::VPP;
  if constexpr (PREC == 2) {
    join16x8(raw.v[0], raw.v[VPP - 1], f);
  } else if constexpr (PREC == 0) {
    const uint4 a = raw.v[0], b = raw.v[VPP - 1];
    f[0] = __builtin_bit_cast(float, a.x); f[1] = __builtin_bit_cast(float, a.y);
    f[2] = __builtin_bit_cast(float, a.z); f[3] = __builtin_bit_cast(float, a.w);
    f[4] = __builtin_bit_cast(float, b.x); f[5] = __builtin_bit_cast(float, b.y);
    f[6] = __builtin_bit_cast(float, b.z); f[7] = __builtin_bit_cast(float, b.w);
  } else {
    const unsigned u[4] = {raw.v[0].x, raw.v[0].y, raw.v[0].z, raw.v[0].w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = __builtin_bit_cast(float, u[k] << 16);
      f[2 * k + 1] = __builtin_bit_cast(float, u[k] & 0xffff0000u);
    }
  }
}

}  // namespace nbc
