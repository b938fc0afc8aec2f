// What the per-image reduction passes share (confusion.hip, lovasz.hip, dataset_stats.hip, pixel_ce.hip, dropout_head.hip
// and the argmax of pointwise.hip): a batch goes in, a few numbers per image come out.
// Integer sums do not depend on their order, and the f64 sums built on wave_sum fix theirs (lane accumulation in pixel
// order, the butterfly, waves in order through LDS, tiles in tile order): either way an image's numbers are bit-identical
// alone, anywhere in a batch and on any stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/nbc.h"
#include "nbc_internal.hpp"

namespace nbc {

// target class of a grey level: round(2 * float32(v) / 255) (dataset.py:189-197) is 0 for 0..63, 1 for 64..191, 2 for
// 192..255, which is (v + 64) >> 7 on the integer
__device__ __forceinline__ unsigned target_class(unsigned grey) { return (grey + 64u) >> 7; }

// torch.argmax over three values: the first maximum wins, a NaN counts as the maximum
__device__ __forceinline__ int argmax3(float a, float b, float c) {
  int best = 0;
  float bv = a;
  if ((b > bv) || (b != b && bv == bv)) { best = 1; bv = b; }
  if ((c > bv) || (c != c && bv == bv)) { best = 2; bv = c; }
  return best;
}

// sum over the 64 lanes of a wave, in every lane: the xor butterfly, offsets 32 down to 1
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// K such sums side by side, the shuffles of one offset together
template <typename T, int K>
__device__ __forceinline__ void wave_sum(T (&v)[K]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], off, 64);
}

// Block-wide sum of kCells values per thread into the 64-bit cells out[kCells], which a memset zeroed: wave_sum, an LDS row
// per wave, then one atomic per non-zero cell.  `barrier` is the block barrier between the two levels, for a kernel that
// has a block-wide vote to take there.
template <int kThreads, int kCells, typename T, typename Barrier>
__device__ __forceinline__ void block_add(const T (&v)[kCells], unsigned long long* __restrict__ out, Barrier barrier) {
  __shared__ T part[kThreads / 64][kCells];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kCells; ++k) {
    const T x = wave_sum(v[k]);
    if ((tid & 63) == 0) part[tid >> 6][k] = x;
  }
  barrier();
  if (tid < kCells) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w][tid];
    if (s) atomicAdd(&out[tid], s);
  }
}
template <int kThreads, int kCells, typename T>
__device__ __forceinline__ void block_add(const T (&v)[kCells], unsigned long long* __restrict__ out) {
  block_add<kThreads, kCells>(v, out, [] { __syncthreads(); });
}

// A stream of `bytes` bytes from any address, read in aligned chunks of `chunk` bytes (a multiple of 16): `head` bytes up
// to the first 16-byte boundary, a body of `chunks` whole chunks that ends at `body_end`, and a tail.  Thread g of `stride`
// takes chunks g, g + stride, ... of the body and, one byte each, the same of the head and of the tail.
struct ByteStream {
  long long bytes, head, chunks, body_end;

  __device__ __forceinline__ ByteStream(const void* base, long long bytes_, int chunk) : bytes(bytes_) {
    head = (long long)((16u - ((unsigned)reinterpret_cast<uintptr_t>(base) & 15u)) & 15u);
    if (head > bytes) head = bytes;
    chunks = (bytes - head) / chunk;
    body_end = head + chunks * chunk;
  }
  // no body (a second operand is not aligned there): every byte is head
  __device__ __forceinline__ void drop_body() { head = body_end = bytes; chunks = 0; }
  // f(q) for this thread's bytes outside the body
  template <typename F>
  __device__ __forceinline__ void for_each_outside(long long g, long long stride, F f) const {
    for (long long q = g; q < head; q += stride) f(q);
    for (long long q = body_end + g; q < bytes; q += stride) f(q);
  }
};

// ---- host: what the entry points check and carve -----------------------------------------------------------------------
inline int fail(const char* who, int code, const std::string& msg) { return set_error(code, std::string(who) + ": " + msg); }
inline bool label_dtype_ok(int labels_dtype) { return labels_dtype == NBC_LABEL_U8 || labels_dtype == NBC_LABEL_I64; }

// the batch a per-image pass accepts: grid.y carries the image, a pixel index fits 31 bits
inline bool per_image_shape_ok(int N, int H, int W) {
  return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL;
}
constexpr const char* kPerImageShape = "bad shape: 1 <= N <= 65535, H, W >= 1 and H * W < 2^31";
// the same for a stack of `per_image` views or windows of each of N images, and for the frame alone; the entry points word
// their own messages
inline bool stack_entries_ok(int N, long long per_image) { return N >= 1 && per_image * N <= 65535; }
inline bool frame_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL; }

// the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// every pointer of the list is 4-byte aligned (a null one is)
template <typename... P>
inline bool aligned4(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 3u) == 0;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// carves a workspace into 256-byte aligned regions: take() returns the region's offset, `offset` ends as the total
struct Carver {
  size_t offset = 0;
  size_t take(size_t bytes) {
    const size_t at = offset;
    offset += align256(bytes);
    return at;
  }
};

// the caller's workspace holds `need` bytes and is 256-byte aligned
inline int check_workspace(const char* who, const void* ptr, size_t bytes, size_t need) {
  if (bytes < need)
    return fail(who, NBC_ERR_INVALID, "workspace of " + std::to_string(bytes) + " bytes, " + std::to_string(need) + " needed");
  if (reinterpret_cast<uintptr_t>(ptr) & 255u) return fail(who, NBC_ERR_INVALID, "workspace must be 256-byte aligned");
  return NBC_OK;
}

// slices (blocks) per image of a byte-stream pass: no more than its chunks fill, and about blocks_per_call over the batch
inline unsigned slices_for(long long bytes, int chunk, int threads, int blocks_per_call, int N) {
  const long long per_block = (long long)threads * chunk;
  long long slices = (bytes + per_block - 1) / per_block;
  const long long want = (blocks_per_call + N - 1) / N;
  if (slices > want) slices = want;
  return (unsigned)(slices < 1 ? 1 : slices);
}

}  // namespace nbc
