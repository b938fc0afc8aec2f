// The three forms an activation tensor [pixels][C] is stored in, and how a lane finds and decodes its channels in each.
// PREC is the numbering of every `template <int PREC>` here: 0 = f32, 1 = bf16, 2 = f16x2 pieces (split16.hpp), whose pixel is
// C / 32 groups of 128 bytes, [h0 x 32][h1 x 32].  Read through this header: classifier.4 and its dropout form, the ASPP pooling
// branch (of every DeepLab head, the EfficientNets' f32 one included), per-image BatchNorm, keep-mode reads and the calibration
// guard.  Not: the max-pool (pointwise.hip), the ingest kernels, EfficientNet's own f32 kernels (efficientnet.hip), and the conv
// kernels' f16x2 epilogue (x2_store, f16x2_mma.hpp).  The precision numbering is also with_precision's (nbc_kernels.hpp), which
// turns the run-time precision into PREC for the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "split16.hpp"

namespace nbc {

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
  return __builtin_bit_cast(float, (unsigned)b << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {      // round to nearest even
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(unsigned short, b);
}

constexpr int stored_elem_bytes(int prec) { return prec == 1 ? 2 : 4; }   // bytes of a pixel per channel

// ---- the unit: what one lane moves with 16-byte accesses.  f32: 4 channels, bf16: 8, one uint4 each; f16x2: 8 channels, the
// 16 bytes of their h0 pieces and the 16 bytes of their h1 pieces 64 bytes on (the access pattern of x2_store).  The raw form
// and its decode are apart so that a kernel can request several pixels' loads before it decodes any.
template <int PREC>
struct Unit {
  static constexpr int CH = PREC == 0 ? 4 : 8;       // channels
  static constexpr int LOADS = PREC == 2 ? 2 : 1;    // 16-byte accesses
  uint4 v[LOADS];                                    // f16x2: h0 chunk, h1 chunk
};

// the first byte of unit j of a run of contiguous pixels that starts at p: j * 16 bytes on; in f16x2 (C is a multiple of 32, so
// the groups of consecutive pixels are contiguous) the h0 chunk j % 4 of group j / 4
template <int PREC, typename Int>
__device__ __forceinline__ const void* unit_at(const void* p, Int j) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  if constexpr (PREC == 2) return b + (j >> 2) * 128 + (j & 3) * 16;
  else return static_cast<const unsigned*>(p) + j * 4;      // four 32-bit words
}
template <int PREC, typename Int>
__device__ __forceinline__ void* unit_at(void* p, Int j) {
  return const_cast<void*>(unit_at<PREC>(static_cast<const void*>(p), j));
}

template <int PREC>
__device__ __forceinline__ Unit<PREC> unit_load(const void* at) {          // at: the unit's first byte
  const uint4* p = static_cast<const uint4*>(at);
  Unit<PREC> u;
  u.v[0] = p[0];
  if constexpr (PREC == 2) u.v[1] = p[4];
  return u;
}

template <int PREC>
__device__ __forceinline__ void unit_decode(const Unit<PREC>& u, float (&f)[Unit<PREC>::CH]) {
  if constexpr (PREC == 2) {
    join16x8(u.v[0], u.v[1], f);
  } else if constexpr (PREC == 0) {
    f[0] = __builtin_bit_cast(float, u.v[0].x); f[1] = __builtin_bit_cast(float, u.v[0].y);
    f[2] = __builtin_bit_cast(float, u.v[0].z); f[3] = __builtin_bit_cast(float, u.v[0].w);
  } else {
    const unsigned w[4] = {u.v[0].x, u.v[0].y, u.v[0].z, u.v[0].w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f[2 * k] = __builtin_bit_cast(float, w[k] << 16);
      f[2 * k + 1] = __builtin_bit_cast(float, w[k] & 0xffff0000u);
    }
  }
}

// f32: a bit copy; f16x2: split16 (no kernel writes bf16 units: the max-pool packs its own, by truncation)
template <int PREC>
__device__ __forceinline__ Unit<PREC> unit_encode(const float (&f)[Unit<PREC>::CH]) {
  static_assert(PREC != 1, "no bf16 encode");
  Unit<PREC> u;
  if constexpr (PREC == 2) {
    split16x8(f, u.v[0], u.v[1]);
  } else {
    u.v[0] = make_uint4(__builtin_bit_cast(unsigned, f[0]), __builtin_bit_cast(unsigned, f[1]), __builtin_bit_cast(unsigned, f[2]),
                        __builtin_bit_cast(unsigned, f[3]));
  }
  return u;
}

template <int PREC>
__device__ __forceinline__ void unit_store(void* at, const Unit<PREC>& u) {
  uint4* p = static_cast<uint4*>(at);
  if constexpr (PREC == 2) p[4] = u.v[1];
  p[0] = u.v[0];
}

// ---- eight channels [c8, c8 + 8) of pixel `pix` of a C-channel tensor (c8 a multiple of 8): two units in f32, one otherwise.
// classifier.4 reads its operands through this one pair in the forward (head1x1_body, pointwise.hip) and behind the live
// Dropout (head1x1_dropout_kernel, dropout_head.hip), and both run head_chain of head1x1.hpp on them (the header says which of
// its other pieces each kernel calls): the two together are what makes "p = 0 gives the forward's logits bit for bit" true.
template <int PREC>
struct Eight {
  static constexpr int UNITS = 8 / Unit<PREC>::CH;
  Unit<PREC> u[UNITS];
};

// where channels [c8, c8 + 8) lie in the pixel (or, for a lane that walks pixels, the tensor) that starts at p
template <int PREC>
__device__ __forceinline__ const unsigned char* eight_at(const void* p, int c8) {
  if constexpr (PREC == 2) return static_cast<const unsigned char*>(unit_at<PREC>(p, c8 >> 3));
  else return static_cast<const unsigned char*>(p) + (size_t)c8 * stored_elem_bytes(PREC);
}

template <int PREC>
__device__ __forceinline__ Eight<PREC> load8(const unsigned char* __restrict__ at) {
  Eight<PREC> raw;
#pragma unroll
  for (int k = 0; k < Eight<PREC>::UNITS; ++k) raw.u[k] = unit_load<PREC>(at + 16 * k);
  return raw;
}

template <int PREC>
__device__ __forceinline__ void decode8(const Eight<PREC>& raw, float (&f)[8]) {
  if constexpr (PREC == 0) {
    float lo[4], hi[4];
    unit_decode(raw.u[0], lo);
    unit_decode(raw.u[1], hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = lo[e]; f[4 + e] = hi[e]; }
  } else {
    unit_decode(raw.u[0], f);
  }
}

// Eight channels straight to f32, for a lane that has no other work to put between its loads and their use (the ASPP pooling
// sums): the pieces are joined from memory and the flat forms are addressed in their element's type, which is the machine code
// that kernel has always had; through load8's raw form it is another.
template <int PREC>
__device__ __forceinline__ void read8(const void* __restrict__ x, size_t pix, int C, int c8, float (&f)[8]) {
  if constexpr (PREC == 2) {
    const uint4* p = reinterpret_cast<const uint4*>(eight_at<PREC>(static_cast<const unsigned char*>(x) + pix * C * 4, c8));
    join16x8(p[0], p[4], f);
  } else {
    using Elem = std::conditional_t<PREC == 0, float, unsigned short>;
    decode8(load8<PREC>(reinterpret_cast<const unsigned char*>(static_cast<const Elem*>(x) + pix * C + c8)), f);
  }
}

// ---- one element as f32: channel c of pixel pix of a C-channel tensor, i = pix * C + c.  The caller gives the index and its
// parts; f32 and bf16 use the one, f16x2 the other.
template <int PREC>
__device__ __forceinline__ float load_elem(const void* x, size_t i, size_t pix, int C, int c) {
  if constexpr (PREC == 0) return static_cast<const float*>(x)[i];
  else if constexpr (PREC == 2) {
    const _Float16* hp = static_cast<const _Float16*>(x) + pix * (size_t)C * 2 + (c >> 5) * 64 + (c & 31);
    return join16(hp[0], hp[32]);
  } else return bf16_bits_to_f32(static_cast<const unsigned short*>(x)[i]);
}

template <int PREC>
__device__ __forceinline__ void store_elem(void* y, size_t i, size_t pix, int C, int c, float v) {
  if constexpr (PREC == 0) static_cast<float*>(y)[i] = v;
  else if constexpr (PREC == 2) {
    _Float16 h0, h1;
    split16(v, h0, h1);
    _Float16* yp = static_cast<_Float16*>(y) + pix * (size_t)C * 2 + (c >> 5) * 64 + (c & 31);
    yp[0] = h0;
    yp[32] = h1;
  } else static_cast<unsigned short*>(y)[i] = f32_to_bf16_bits(v);
}

}  // namespace nbc
