// The row mover of the view kernels (tta.hip: the flips; windows.hip: the crop windows).  Device helpers only.
//
// A row is a run of units (a 3-byte pixel of uint8 NHWC, a 4-byte element of a float32 NCHW plane) and is moved in granules (a
// byte, a 32-bit word): GT is the granule (unsigned char / uint32_t), UG the granules per unit (3 / 1).  A block takes a segment
// of a source row -- task = (row, segment), row_segment -- and stage_segment puts it into LDS with 16-B loads at the row's own
// alignment; then emit_run puts every copy of it together out of LDS in the destination's own 16-B vectors, unit by unit in
// reverse where the copy mirrors.  Which destination rows, and where in them, is the kernel's own geometry.  Heads and tails that
// no aligned vector covers go granule by granule, so no access leaves [row start, row end) of either buffer, at any alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nbc_kernels.hpp"

namespace nbc {

constexpr int kViewThreads = 256;
constexpr int kSegUnits = 4096;                   // units of a row per block and round: 12 KiB of pixels, 16 KiB of floats
constexpr int kViewBlocksPerCu = 8;

template <typename GT>
constexpr int kPerVec = 16 / (int)sizeof(GT);     // granules of a 16-B vector
template <typename GT, int UG>
constexpr int kSegGranules = kSegUnits * UG + kPerVec<GT>;   // the LDS of a segment, 16-B aligned: room for its misalignment

__host__ __device__ __forceinline__ int row_segments(int W) { return (W + kSegUnits - 1) / kSegUnits; }

// the grid of a views kernel over `rows` source rows of W units
inline unsigned row_view_blocks(long long rows, int W) {
  return grid_stride_blocks((size_t)(rows * row_segments(W)), 1, kViewBlocksPerCu);
}

// task -> units [u0, u0 + nu) of source row `row`
struct RowSegment {
  long long row;
  int u0, nu;
};
__device__ __forceinline__ RowSegment row_segment(long long task, int segs, int W) {
  RowSegment t;
  t.row = task / segs;
  t.u0 = (int)(task % segs) * kSegUnits;
  t.nu = (W - t.u0 < kSegUnits) ? W - t.u0 : kSegUnits;
  return t;
}

// The ng granules at src into LDS, granule i at seg[a0 + i]: a 16-B aligned global vector is a 16-B aligned LDS vector.
// Returns a0; ends with the barrier that makes the segment the block's.
template <typename GT>
__device__ __forceinline__ int stage_segment(const GT* src, int ng, GT* seg) {
  constexpr int kVec = kPerVec<GT>;
  const int tid = threadIdx.x;
  const int a0 = (int)((reinterpret_cast<uintptr_t>(src) & 15u) / sizeof(GT));
  int head = (kVec - a0) % kVec;
  if (head > ng) head = ng;
  const int vecs = (ng - head) / kVec;
  for (int i = tid; i < head; i += kViewThreads) seg[a0 + i] = src[i];
  for (int v = tid; v < vecs; v += kViewThreads)
    *reinterpret_cast<uint4*>(&seg[a0 + head + v * kVec]) = *reinterpret_cast<const uint4*>(src + head + v * kVec);
  for (int i = head + vecs * kVec + tid; i < ng; i += kViewThreads) seg[a0 + i] = src[i];
  __syncthreads();
  return a0;
}

// `units` units out of LDS, from seg[at] on, to dst, at any alignment of dst: head, 16-B vectors, tail.  Destination granule t is
// granule t of the run, or, where the run mirrors, granule (units - 1 - k) * UG + o for unit k = t / UG, o = t % UG.  (The LDS
// array and an index, not a pointer into it: measured, the uint8 flips kernel is 4 % slower with the pointer.)
template <typename GT, int UG>
__device__ __forceinline__ void emit_run(GT* dst, const GT* seg, int at, int units, bool mirror) {
  constexpr int kVec = kPerVec<GT>;
  const int tid = threadIdx.x;
  const int count = units * UG;
  auto fetch = [&](int t) -> GT {
    if (!mirror) return seg[at + t];
    const int k = t / UG, o = t - k * UG;
    return seg[at + (units - 1 - k) * UG + o];
  };
  int head = (int)(((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(GT));
  if (head > count) head = count;
  const int vecs = (count - head) / kVec;
  for (int i = tid; i < head; i += kViewThreads) dst[i] = fetch(i);
  for (int v = tid; v < vecs; v += kViewThreads) {
    const int t0 = head + v * kVec;
    uint32_t w4[4];
    if constexpr (sizeof(GT) == 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) w4[q] = (uint32_t)fetch(t0 + q);
    } else {
      int k = t0 / UG, o = t0 - k * UG;           // one division per vector, then steps
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        w4[q] = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const GT g = mirror ? seg[at + (units - 1 - k) * UG + o] : seg[at + t0 + 4 * q + e];
          w4[q] |= (uint32_t)g << (8 * e);
          if (++o == UG) { o = 0; ++k; }
        }
      }
    }
    *reinterpret_cast<uint4*>(dst + t0) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
  }
  for (int i = head + vecs * kVec + tid; i < count; i += kViewThreads) dst[i] = fetch(i);
}

}  // namespace nbc
