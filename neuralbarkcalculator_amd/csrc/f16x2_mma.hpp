// The f16x2 (NBC_PREC_F16X2) arithmetic of the two LDS-DMA convolution kernels (conv_igemm_dma.hip, conv3x3_rows.hip), defined
// once: the K-step's products and the chain's cadence, and the epilogue's pieces.  The kernels differ in how tiles reach LDS and
// how fragments are read from it; what happens to a fragment in registers and to an accumulator on its way to memory is this.
#pragma once
#include "lds_dma.hpp"
#include "split16.hpp"

namespace nbc {
namespace {

// P -> P 2^-11 (v_pk_mul_f16 by a power of two: exact for P >= 2^-3, which the row normalisation of the weights gives)
constexpr f16x8 kLow = {kH1UnscaleH, kH1UnscaleH, kH1UnscaleH, kH1UnscaleH, kH1UnscaleH, kH1UnscaleH, kH1UnscaleH, kH1UnscaleH};

// The chain joins the running sum; CLEAR: and starts again from zero.
template <bool CLEAR, int NJ, int NI>
__device__ __forceinline__ void x2_join(f32x4 (&sum)[NJ][NI], f32x4 (&chain)[NJ][NI]) {
#pragma unroll
  for (int n = 0; n < NJ * NI; ++n) {
    sum[n / NI][n % NI] += chain[n / NI][n % NI];
    if constexpr (CLEAR) {
#pragma unroll
      for (int e = 0; e < 4; ++e) chain[n / NI][n % NI][e] = 0.f;
    }
  }
}
// In front of K-step t (wave-uniform): the chain of the last eight K-steps (256 channels x 3 products) joins the sum.
template <int NJ, int NI>
__device__ __forceinline__ void x2_flush(int t, f32x4 (&sum)[NJ][NI], f32x4 (&chain)[NJ][NI]) {
  if (t > 0 && (t & 7) == 0) x2_join<true>(sum, chain);
}

// The 3 NJ NI MFMAs of a K-step: P.X0, Q.X0, (P 2^-11).X1 per 16x16 tile (xp0 / xp1: the pixels' high / low pieces, xw0 / xw1:
// the weights' P / Q).  Product-major: two MFMAs on one accumulator are NJ NI instructions apart; the scaled high pieces of a
// weight block are formed in place right in front of its third products (hoisting them cost 0-3 %,
// profiles/r04_f16x2_kloop_schedule_variants_rejected.log).  after(idx) runs behind MFMA idx (the generic kernel's refill parts).
struct NoHook { __device__ __forceinline__ void operator()(int) const {} };
template <int NJ, int NI, class After = NoHook>
__device__ __forceinline__ void x2_products(const uint4 (&xp0)[NI], const uint4 (&xp1)[NI], uint4 (&xw0)[NJ], const uint4 (&xw1)[NJ],
                                            f32x4 (&chain)[NJ][NI], After after = After{}) {
  constexpr int NTI = NJ * NI;
#pragma unroll
  for (int idx = 0; idx < 3 * NTI; ++idx) {
    const int prod = idx / NTI, n = idx % NTI, j = n / NI, i = n % NI;
    if (prod == 0)
      chain[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xw0[j]), __builtin_bit_cast(f16x8, xp0[i]), chain[j][i], 0, 0, 0);
    else if (prod == 1)
      chain[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xw1[j]), __builtin_bit_cast(f16x8, xp0[i]), chain[j][i], 0, 0, 0);
    else {
      if (i == 0) xw0[j] = __builtin_bit_cast(uint4, __builtin_bit_cast(f16x8, xw0[j]) * kLow);      // P -> P 2^-11, in place
      chain[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xw0[j]), __builtin_bit_cast(f16x8, xp1[i]), chain[j][i], 0, 0, 0);
    }
    after(idx);
  }
}

// The row-step kernel's form of the K-step (conv3x3_rows.hip): the same fragments in the same product-major order, but the third
// products take P AS STORED and go into a set of their own: chain += P.X0, Q.X0; low += P.X1.  The factor 2^-11 is a constant and
// commutes with the sum, so it is applied once per output behind the K loop (x2_join_low) where x2_products multiplies 2 NJ
// registers in every K-step; the weight fragments are not modified.  `low` runs over a tile's whole K loop: x2_flush never
// touches it.  (Its additions round at its own scale, 2^-11 of the chain's: DESIGN 1.)
template <int NJ, int NI>
__device__ __forceinline__ void x2_products_low(const uint4 (&xp0)[NI], const uint4 (&xp1)[NI], const uint4 (&xw0)[NJ], const uint4 (&xw1)[NJ],
                                                f32x4 (&chain)[NJ][NI], f32x4 (&low)[NJ][NI]) {
  constexpr int NTI = NJ * NI;
#pragma unroll
  for (int idx = 0; idx < 3 * NTI; ++idx) {
    const int prod = idx / NTI, n = idx % NTI, j = n / NI, i = n % NI;
    if (prod == 0)
      chain[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xw0[j]), __builtin_bit_cast(f16x8, xp0[i]), chain[j][i], 0, 0, 0);
    else if (prod == 1)
      chain[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xw1[j]), __builtin_bit_cast(f16x8, xp0[i]), chain[j][i], 0, 0, 0);
    else
      low[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, xw0[j]), __builtin_bit_cast(f16x8, xp1[i]), low[j][i], 0, 0, 0);
  }
}
// Behind the last x2_join<false> of a tile: sum = fma(low, 2^-11, sum), one rounding per output.
template <int NJ, int NI>
__device__ __forceinline__ void x2_join_low(f32x4 (&sum)[NJ][NI], const f32x4 (&low)[NJ][NI]) {
#pragma unroll
  for (int n = 0; n < NJ * NI; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) sum[n / NI][n % NI][e] = __builtin_fmaf(low[n / NI][n % NI][e], kH1Unscale, sum[n / NI][n % NI][e]);
}

// ---- epilogue.  Each wave takes one 32-pixel x (NT*32)-channel slab at a time through a private f32 scratch in LDS: BN on the
// way in (a); on the way out (b) lane l owns chunk l % CPR (16 output bytes) of pixel l / CPR of a pass, so identity loads and
// stores (c) are whole row segments.  Geometry of such slabs in precision PREC.  (Constants and functions of plain values: with
// the lane's run-time values in a struct the f16x2 tile <2,2,2,2,1,2> took 136 registers and lost its fourth wave per SIMD.)
template <int NT, int PREC>
struct EpiGeom {
  static constexpr int EB = PREC == 1 ? 2 : 4;
  static constexpr int SLAB_CH = NT * 32;                  // channels of the wave's slab
  static constexpr int PITCH = SLAB_CH * 4 + 16;           // f32 scratch row, padded against bank conflicts
  static constexpr int OUT_CH = PREC == 2 ? 8 : 16 / EB;   // channels per lane and pass (f16x2: an h0 chunk and an h1 chunk)
  static constexpr int CPR = SLAB_CH / OUT_CH;             // lanes per pixel row
  static constexpr int PIX_PER_PASS = 64 / CPR;
  static constexpr int PASSES = 32 / PIX_PER_PASS;
  // byte offset of the lane's chunk behind the slab's first channel (f16x2: the h0 chunk; its h1 chunk is 64 bytes on)
  static __device__ __forceinline__ unsigned lane_chunk(int o_chunk) {
    return PREC == 2 ? (unsigned)(o_chunk >> 2) * 128u + (unsigned)(o_chunk & 3) * 16u : (unsigned)o_chunk * 16u;
  }
  // the row whose identity a lane reads for `row`: tail rows read a valid row; never stored
  static __device__ __forceinline__ int id_row(int row, int rows_valid) { return row < rows_valid ? row : rows_valid - 1; }
};

// (a) BN on slab i of 16x16 accumulators (lane (r16, q16): pixel r16, channels 4*q16..+3 of each tile) into the wave's scratch.
// A channel group's scale/shift reads are all issued before its scratch writes (a wave's LDS operations complete in order).
// DUAL (the generic kernel's dual-branch form): `acc` is the chain of a convolution that never joined -- its sum is 0 + chain --
// and `id`, the identity in the same layout, is added value for value as (c) adds it row-wise.  Otherwise `id` is not read.
template <int PITCH, bool DUAL, int NJ, int NI>
__device__ __forceinline__ void bn16_to_scratch(unsigned char* scr, const unsigned char* table, const f32x4 (&acc)[NJ][NI], const f32x4 (&id)[NJ][NI],
                                                int i, int r16, int q16) {
#pragma unroll
  for (int j0 = 0; j0 < NJ; j0 += 4) {
    float4 sc[4], sh[4];
#pragma unroll
    for (int jj = 0; jj < 4 && j0 + jj < NJ; ++jj) {
      const int nl = (j0 + jj) * 16 + 4 * q16;
      sc[jj] = *reinterpret_cast<const float4*>(table + nl * 4);
      sh[jj] = *reinterpret_cast<const float4*>(table + 1024 + nl * 4);
    }
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int jj = 0; jj < 4 && j0 + jj < NJ; ++jj) {
        const int nl = (j0 + jj) * 16 + 4 * q16;
        const f32x4 kZero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 a = DUAL ? kZero + acc[j0 + jj][2 * i + i2] : acc[j0 + jj][2 * i + i2];
        float4 v;
        v.x = __builtin_fmaf(a[0], sc[jj].x, sh[jj].x);
        v.y = __builtin_fmaf(a[1], sc[jj].y, sh[jj].y);
        v.z = __builtin_fmaf(a[2], sc[jj].z, sh[jj].z);
        v.w = __builtin_fmaf(a[3], sc[jj].w, sh[jj].w);
        if constexpr (DUAL) {
          const f32x4 idv = id[j0 + jj][2 * i + i2];
          v.x += idv[0]; v.y += idv[1]; v.z += idv[2]; v.w += idv[3];
        }
        *reinterpret_cast<float4*>(scr + (i2 * 16 + r16) * PITCH + nl * 4) = v;
      }
  }
}

// (b) the slab read back row-wise, every read issued before the first use (the scratch is wave-private)
template <class G>
__device__ __forceinline__ void epi_read_rows(const unsigned char* scr, int o_pix, int o_chunk, float (&v)[G::PASSES][G::OUT_CH]) {
#pragma unroll
  for (int ps2 = 0; ps2 < G::PASSES; ++ps2) {
    const float4* sp = reinterpret_cast<const float4*>(scr + (ps2 * G::PIX_PER_PASS + o_pix) * G::PITCH + o_chunk * G::OUT_CH * 4);
#pragma unroll
    for (int q = 0; q < G::OUT_CH / 4; ++q) {
      const float4 t4 = sp[q];
      v[ps2][4 * q] = t4.x; v[ps2][4 * q + 1] = t4.y; v[ps2][4 * q + 2] = t4.z; v[ps2][4 * q + 3] = t4.w;
    }
  }
}

// (c) f16x2: [has_id: + identity, from its h0 and h1 chunks id0, id1, which are not read otherwise,] ReLU (NaN-propagating),
// split16x8, and for a row inside the image batch two 16-byte stores at dst and dst + 64.  (The identity as values and a flag:
// as a nullable pointer to the pair it went through scratch memory in the dual-branch kernels.)
__device__ __forceinline__ void x2_store(float (&v)[8], bool relu, unsigned char* dst, bool valid, bool has_id, const uint4& id0, const uint4& id1) {
  if (has_id) {
    float idv[8];
    join16x8(id0, id1, idv);
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] += idv[q];
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_elementwise_maximum(v[e], 0.f);
  }
  uint4 o, o1;
  split16x8(v, o, o1);
  if (valid) {
    *reinterpret_cast<uint4*>(dst + 64) = o1;
    *reinterpret_cast<uint4*>(dst) = o;
  }
}

// (c) without identity
__device__ __forceinline__ void x2_store(float (&v)[8], bool relu, unsigned char* dst, bool valid) { x2_store(v, relu, dst, valid, false, uint4{}, uint4{}); }

}  // namespace
}  // namespace nbc
