// The device side of csrc/softmax_census.hip (the definition and the kernel form are described there): the per-pixel step
// and the per-tile kernel, in a header so that tools/census_plain.hip can instantiate the form without register-held end
// bins beside the product's.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "reduce.hpp"

namespace nbc {
namespace census {


constexpr int kThreads = 256;                           // 4 waves
constexpr int kGroup = 4;                               // consecutive pixels per load group
constexpr int kGroups = 4;                              // groups per thread and tile
constexpr int kTile = kThreads * kGroup * kGroups;      // 4096 pixels per tile: 256 blocks at 1024 x 1024 x 1
constexpr int kBins = NBC_CENSUS_BINS;
constexpr int kCounts = NBC_CENSUS_RS;                  // H and R: the words that count pixels (u16 per tile)
constexpr int kSums = kBins * 2 + 9 + 1;                // RS, M and nonfinite: u32 per tile
constexpr int kSumRS = 0, kSumM = 2 * kBins, kSumNonfinite = kSumM + 9;
constexpr int kBrier = 3;                               // B: u64 per tile
static_assert(NBC_CENSUS_H == 0 && NBC_CENSUS_R == 9 * kBins && NBC_CENSUS_RS == NBC_CENSUS_R + 2 * kBins &&
              NBC_CENSUS_M == NBC_CENSUS_RS + 2 * kBins && NBC_CENSUS_B == NBC_CENSUS_M + 9 &&
              NBC_CENSUS_NONFINITE == NBC_CENSUS_B + 3 && NBC_CENSUS_WORDS == NBC_CENSUS_NONFINITE + 1, "the row of include/nbc.h");
static_assert(kCounts % 2 == 0 && kTile <= 65535, "two 16-bit counts per stored word");
static_assert(kGroup * kGroups <= 127, "a thread's pixels must fit the 7-bit counters");

using u32 = unsigned;
using u64 = unsigned long long;

// what a thread keeps in registers over its 16 pixels
struct Private {
  u64 end0 = 0, end255 = 0;        // H[t][c][0] and H[t][c][255]: 7 bits per (t, c) cell
  u32 r255 = 0;                    // R[hit][255]: 7 bits per hit
  u32 rs255[2] = {0, 0};           // RS[hit][255]
  u32 m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  u64 brier[3] = {0, 0, 0};
  u32 nonfinite = 0;
};

// one pixel into the LDS histograms and the thread's registers; returns its confidence byte.  kPrivateEnds: the end bins (0
// and 255 of H, 255 of R / RS) stay in registers.  The library instantiates that form alone; tools/census_plain.hip also the
// one that sends them through an LDS atomic like every other bin, to measure what the registers buy.
template <bool kPrivateEnds>
__device__ __forceinline__ u32 add_pixel(float a, float b, float c, u32 t, bool with_target, u32* __restrict__ cnt,
                                         u32* __restrict__ sum, Private& pv) {
  const bool finite = fabsf(a) <= 3.4028234663852886e38f && fabsf(b) <= 3.4028234663852886e38f && fabsf(c) <= 3.4028234663852886e38f;
  if (!finite) {                                        // NaN fails every comparison
    pv.nonfinite += 1u;
    return 0u;
  }
  const double x0 = (double)a, x1 = (double)b, x2 = (double)c;
  const double m = fmax(fmax(x0, x1), x2);
  const double e0 = exp(x0 - m), e1 = exp(x1 - m), e2 = exp(x2 - m);
  const double s = (e0 + e1) + e2;
  u32 q[3];
  q[0] = (u32)fmin(65535.0, floor(e0 / s * 65536.0));
  q[1] = (u32)fmin(65535.0, floor(e1 / s * 65536.0));
  q[2] = (u32)fmin(65535.0, floor(e2 / s * 65536.0));
  const u32 k = (u32)argmax3(a, b, c);
  const u32 hit = with_target ? (u32)(k == t) : 1u;
#pragma unroll
  for (u32 cls = 0; cls < 3u; ++cls) {
    const u32 bin = q[cls] >> 8, cell = t * 3u + cls;
    if (kPrivateEnds && bin == 0u) pv.end0 += 1ull << (7u * cell);
    else if (kPrivateEnds && bin == 255u) pv.end255 += 1ull << (7u * cell);
    else atomicAdd(&cnt[NBC_CENSUS_H + cell * kBins + bin], 1u);
    const long long d = (long long)q[cls] - (cls == t ? 65536ll : 0ll);
#pragma unroll
    for (u32 tt = 0; tt < 3u; ++tt) {
      pv.m[tt * 3u + cls] += tt == t ? q[cls] : 0u;
      pv.brier[tt] += tt == t ? (u64)(d * d) : 0ull;
    }
  }
  const u32 qk = k == 0u ? q[0] : k == 1u ? q[1] : q[2];
  const u32 bin = qk >> 8;
  if (kPrivateEnds && bin == 255u) {
    pv.r255 += 1u << (7u * hit);
    pv.rs255[0] += hit ? 0u : qk;
    pv.rs255[1] += hit ? qk : 0u;
  } else {
    atomicAdd(&cnt[NBC_CENSUS_R + hit * kBins + bin], 1u);
    atomicAdd(&sum[kSumRS + hit * kBins + bin], qk);
  }
  return bin;
}

template <bool kPrivateEnds>
__global__ __launch_bounds__(kThreads) void census_partial(const float* __restrict__ logits, const unsigned char* __restrict__ target,
                                                           unsigned char* __restrict__ confidence, long long P, int T,
                                                           u32* __restrict__ part_cnt, u32* __restrict__ part_sum,
                                                           u64* __restrict__ part_brier) {
  __shared__ u32 cnt[kCounts];
  __shared__ u32 sum[kSums];
  __shared__ u64 brier[kBrier];
  const int n = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < kCounts; i += kThreads) cnt[i] = 0u;
  for (int i = tid; i < kSums; i += kThreads) sum[i] = 0u;
  if (tid < kBrier) brier[tid] = 0ull;
  __syncthreads();

  const float* l0 = logits + (size_t)n * 3 * P;
  const float* l1 = l0 + P;
  const float* l2 = l1 + P;
  const bool with_target = target != nullptr;
  const unsigned char* tg = with_target ? target + (size_t)n * P : nullptr;
  unsigned char* cf = confidence ? confidence + (size_t)n * P : nullptr;
  // group starts are multiples of 4 pixels: they keep whatever alignment the image's planes start with
  const bool vec = ((reinterpret_cast<uintptr_t>(l0) | reinterpret_cast<uintptr_t>(l1) | reinterpret_cast<uintptr_t>(l2)) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(tg) & 3u) == 0;
  const bool vec_out = (reinterpret_cast<uintptr_t>(cf) & 3u) == 0;
  const long long start = (long long)tile * kTile;

  Private pv;
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const long long q = start + (long long)(g * kThreads + tid) * kGroup;
    if (q >= P) continue;
    if (vec && q + kGroup <= P) {
      const float4 a = *reinterpret_cast<const float4*>(l0 + q);
      const float4 b = *reinterpret_cast<const float4*>(l1 + q);
      const float4 c = *reinterpret_cast<const float4*>(l2 + q);
      const u32 t = with_target ? *reinterpret_cast<const u32*>(tg + q) : 0u;     // grey 0 is class 0
      const u32 c0 = add_pixel<kPrivateEnds>(a.x, b.x, c.x, target_class(t & 255u), with_target, cnt, sum, pv);
      const u32 c1 = add_pixel<kPrivateEnds>(a.y, b.y, c.y, target_class((t >> 8) & 255u), with_target, cnt, sum, pv);
      const u32 c2 = add_pixel<kPrivateEnds>(a.z, b.z, c.z, target_class((t >> 16) & 255u), with_target, cnt, sum, pv);
      const u32 c3 = add_pixel<kPrivateEnds>(a.w, b.w, c.w, target_class(t >> 24), with_target, cnt, sum, pv);
      if (cf) {
        if (vec_out) {
          *reinterpret_cast<u32*>(cf + q) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        } else {
          cf[q] = (unsigned char)c0; cf[q + 1] = (unsigned char)c1; cf[q + 2] = (unsigned char)c2; cf[q + 3] = (unsigned char)c3;
        }
      }
    } else {
      const int left = (int)(P - q < kGroup ? P - q : kGroup);
      for (int k = 0; k < left; ++k) {
        const u32 t = with_target ? target_class(tg[q + k]) : 0u;
        const u32 byte = add_pixel<kPrivateEnds>(l0[q + k], l1[q + k], l2[q + k], t, with_target, cnt, sum, pv);
        if (cf) cf[q + k] = (unsigned char)byte;
      }
    }
  }

  // the thread-private words: lanes by wave_sum, then one LDS add per wave and word
  if (kPrivateEnds) {
#pragma unroll
    for (int cell = 0; cell < 9; ++cell) {
      const u32 z = wave_sum((u32)(pv.end0 >> (7 * cell)) & 127u);
      const u32 f = wave_sum((u32)(pv.end255 >> (7 * cell)) & 127u);
      if (lane == 0) {
        if (z) atomicAdd(&cnt[NBC_CENSUS_H + cell * kBins], z);
        if (f) atomicAdd(&cnt[NBC_CENSUS_H + cell * kBins + 255], f);
      }
    }
#pragma unroll
    for (int hit = 0; hit < 2; ++hit) {
      const u32 r = wave_sum((pv.r255 >> (7 * hit)) & 127u);
      const u32 rs = wave_sum(pv.rs255[hit]);
      if (lane == 0 && r) {
        atomicAdd(&cnt[NBC_CENSUS_R + hit * kBins + 255], r);
        atomicAdd(&sum[kSumRS + hit * kBins + 255], rs);
      }
    }
  }
#pragma unroll
  for (int cell = 0; cell < 9; ++cell) {
    const u32 mm = wave_sum(pv.m[cell]);
    if (lane == 0 && mm) atomicAdd(&sum[kSumM + cell], mm);
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const u64 bsum = wave_sum(pv.brier[t]);
    if (lane == 0 && bsum) atomicAdd(&brier[t], bsum);
  }
  const u32 nf = wave_sum(pv.nonfinite);
  if (lane == 0 && nf) atomicAdd(&sum[kSumNonfinite], nf);
  __syncthreads();

  const size_t row = (size_t)n * T + tile;
  u32* pc = part_cnt + row * (kCounts / 2);
  for (int i = tid; i < kCounts / 2; i += kThreads) pc[i] = cnt[2 * i] | (cnt[2 * i + 1] << 16);
  u32* ps = part_sum + row * kSums;
  for (int i = tid; i < kSums; i += kThreads) ps[i] = sum[i];
  if (tid < kBrier) part_brier[row * kBrier + tid] = brier[tid];
}

}  // namespace census
}  // namespace nbc
