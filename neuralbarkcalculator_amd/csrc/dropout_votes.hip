// Per-pixel votes of the Dropout draws (include/nbc.h: nbc_dropout_votes, nbc_vote_summary; the definition: votes.hpp).
//
// Two byte streams (reduce.hpp) over data the pass loop of nbc_dropout_draws leaves on the device, nothing reused:
//   vote_accumulate_kernel  a pass's final label planes u8 [D_pass][N][P] -> the vote words u32 [N][P].  D_pass + 4 B read
//                           per pixel (D_pass in the first pass, which stores the words: no memset), 4 B written.
//   vote_summary_kernel     the vote words -> the winner's label and support bytes and ten integers per image.  4 B read
//                           and 2 B written per pixel.
// A thread owns 16 consecutive pixels of an image: one 16-B load per label plane, four 16-B loads / stores of words, one 16-B
// store per byte plane.  No atomics on the words (a pixel has one owner), no LDS in the accumulate kernel.  The grid is
// (slices of an image) x N.
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "votes.hpp"

using namespace nbc;

namespace {

constexpr int kChunk = 16;                       // pixels per thread and step

// ---- accumulate ----------------------------------------------------------------------------------------------------------
// A thread counts the pass's draws of its 16 pixels in 16 registers laid out as the word is (n1 low, n2 high): a field
// holds 16 bits, so a pass may stack up to 65535 draws -- what the pass loop's own limit (draws x N <= 65535 stacked images)
// already keeps.  The words' fields are the caller's to keep at or below 65535 in total (include/nbc.h).
constexpr int kAccThreads = 256;
constexpr int kAccBlocksPerCall = 2048;          // a plain stream, no shared cells: enough blocks to fill 256 CUs eight deep

template <bool FIRST>
__global__ __launch_bounds__(kAccThreads) void vote_accumulate_kernel(const unsigned char* __restrict__ labels, int draws,
                                                                      long long plane, long long P, uint32_t* __restrict__ votes) {
  const unsigned char* lab = labels + (long long)blockIdx.y * P;      // draw 0's plane of this image; draw d: + d * plane
  uint32_t* words = votes + (long long)blockIdx.y * P;
  const long long stride = (long long)gridDim.x * kAccThreads;
  const long long g = (long long)blockIdx.x * kAccThreads + threadIdx.x;

  // the vector body starts at the first pixel whose label byte of draw 0 is 16-B aligned; it needs the word there aligned
  // too, and every further plane: plane d starts d * N * P bytes on, aligned alike only when that is a multiple of 16
  ByteStream st(lab, P, kChunk);
  if ((reinterpret_cast<uintptr_t>(words + st.head) & 15u) || (draws > 1 && (plane & 15))) st.drop_body();

  for (long long c = g; c < st.chunks; c += stride) {
    const long long i = st.head + c * kChunk;
    uint32_t add[kChunk];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) add[j] = 0u;
    for (int d = 0; d < draws; ++d) {
      const uint4 l = *reinterpret_cast<const uint4*>(lab + (long long)d * plane + i);
      const uint32_t lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
      for (int j = 0; j < kChunk; ++j) add[j] += vote_of_label((lw[j >> 2] >> (8 * (j & 3))) & 255u);
    }
    uint4* w4 = reinterpret_cast<uint4*>(words + i);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (!FIRST) w = w4[q];
      w.x += add[4 * q]; w.y += add[4 * q + 1]; w.z += add[4 * q + 2]; w.w += add[4 * q + 3];
      w4[q] = w;
    }
  }

  // the pixels outside the body (head and tail, or every pixel of an image the body cannot reach), one per thread
  st.for_each_outside(g, stride, [&](long long q) {
    uint32_t add = 0u;
    for (int d = 0; d < draws; ++d) add += vote_of_label(lab[(long long)d * plane + q]);
    words[q] = FIRST ? add : words[q] + add;
  });
}

// ---- summary -------------------------------------------------------------------------------------------------------------
constexpr int kSumThreads = 1024;                // nbc_confusion's shape, for its reason: every block of an image adds into
constexpr int kSumBlocksPerCall = 128;           // the same cells, and atomics on one address serialise
constexpr int kCells = NBC_VOTE_STATS;
constexpr const char* kWho = "nbc_vote_summary";

// What a thread keeps of its pixels: the seven pixel counts (cells 0..5 and 7; a thread sees fewer than 2^31 pixels) and the
// three vote sums (cells 6, 8, 9), which gather in 32 bits and are folded into 64 before 2^16 pixels x 65535 can overflow.
// Compile-time indices keep all of it in registers.
struct Tally {
  unsigned won[3] = {0u, 0u, 0u}, all[3] = {0u, 0u, 0u}, invalid = 0u;
  unsigned part[3] = {0u, 0u, 0u};
  unsigned long long sum[3] = {0ull, 0ull, 0ull};

  __device__ __forceinline__ void add(const Vote& v) {   // an invalid word reaches `invalid` alone (its n_win is 0)
    const unsigned ok = v.valid ? 1u : 0u, un = v.unanimous ? 1u : 0u;
#pragma unroll
    for (unsigned k = 0; k < 3; ++k) {
      const unsigned w = (ok && v.label == k) ? 1u : 0u;
      won[k] += w;
      all[k] += w & un;
    }
    invalid += 1u - ok;
    part[0] += v.n_win;
    part[1] += ok ? v.n1 : 0u;
    part[2] += ok ? v.n2 : 0u;
  }
  __device__ __forceinline__ void fold() {
#pragma unroll
    for (int k = 0; k < 3; ++k) { sum[k] += part[k]; part[k] = 0u; }
  }
};

__global__ __launch_bounds__(kSumThreads) void vote_summary_kernel(const uint32_t* __restrict__ votes, long long P, unsigned draws,
                                                                   unsigned char* __restrict__ labels, unsigned char* __restrict__ support,
                                                                   unsigned long long* __restrict__ stats) {
  const long long base = (long long)blockIdx.y * P;
  const uint32_t* words = votes + base;
  unsigned char* lab = labels ? labels + base : nullptr;
  unsigned char* sup = support ? support + base : nullptr;
  const long long stride = (long long)gridDim.x * kSumThreads;
  const long long g = (long long)blockIdx.x * kSumThreads + threadIdx.x;
  Tally t;

  // the vector body starts at the first pixel whose byte offset in the batch is a multiple of 16: there the words and both
  // byte planes are 16-B aligned when their buffers are; a buffer that is not leaves the image to the scalar path
  ByteStream st(reinterpret_cast<const void*>((uintptr_t)(base & 15)), P, kChunk);
  if ((reinterpret_cast<uintptr_t>(words + st.head) & 15u) || (lab && (reinterpret_cast<uintptr_t>(lab + st.head) & 15u)) ||
      (sup && (reinterpret_cast<uintptr_t>(sup + st.head) & 15u)))
    st.drop_body();

  for (long long c = g; c < st.chunks; c += stride) {
    const long long i = st.head + c * kChunk;
    const uint4* w4 = reinterpret_cast<const uint4*>(words + i);
    uint32_t lb[4], sb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 w = w4[q];
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
      lb[q] = sb[q] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const Vote v = vote_decide(ww[j], draws);
        t.add(v);
        lb[q] |= v.label << (8 * j);
        sb[q] |= v.support << (8 * j);
      }
    }
    if (lab) *reinterpret_cast<uint4*>(lab + i) = make_uint4(lb[0], lb[1], lb[2], lb[3]);
    if (sup) *reinterpret_cast<uint4*>(sup + i) = make_uint4(sb[0], sb[1], sb[2], sb[3]);
    t.fold();                                    // 16 pixels x 65535 < 2^32
  }

  // the pixels outside the body, one per thread
  st.for_each_outside(g, stride, [&](long long q) {
    const Vote v = vote_decide(words[q], draws);
    t.add(v);
    if (lab) lab[q] = (unsigned char)v.label;
    if (sup) sup[q] = (unsigned char)v.support;
    t.fold();
  });

  const unsigned long long cells[kCells] = {t.won[0], t.won[1], t.won[2], t.all[0], t.all[1], t.all[2], t.sum[0], t.invalid, t.sum[1], t.sum[2]};
  block_add<kSumThreads, kCells>(cells, stats + (size_t)blockIdx.y * kCells);
}

}  // namespace

namespace nbc {

hipError_t launch_vote_accumulate(const unsigned char* labels, int draws, int N, long long P, uint32_t* votes, bool first,
                                  hipStream_t s) {
  const dim3 grid(slices_for(P, kChunk, kAccThreads, kAccBlocksPerCall, N), (unsigned)N);
  const long long plane = (long long)N * P;
  if (first)
    hipLaunchKernelGGL(vote_accumulate_kernel<true>, grid, dim3(kAccThreads), 0, s, labels, draws, plane, P, votes);
  else
    hipLaunchKernelGGL(vote_accumulate_kernel<false>, grid, dim3(kAccThreads), 0, s, labels, draws, plane, P, votes);
  return hipGetLastError();
}

}  // namespace nbc

extern "C" int nbc_vote_decode(uint32_t word, int draws, uint8_t* label, uint8_t* support) {
  if (draws < 1 || draws > kVoteMaxDraws) return fail("nbc_vote_decode", NBC_ERR_INVALID, "draws must lie in 1..65535");
  const Vote v = vote_decide(word, (uint32_t)draws);
  if (label) *label = (uint8_t)v.label;
  if (support) *support = (uint8_t)v.support;
  return NBC_OK;
}

extern "C" int nbc_vote_tally(const uint8_t* labels_dev, int N, int D, int H, int W, uint32_t* votes_dev, int accumulate, void* hip_stream) {
  constexpr const char* who = "nbc_vote_tally";
  if (!labels_dev || !votes_dev) return fail(who, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W)) return fail(who, NBC_ERR_INVALID, kPerImageShape);
  if (D < 1 || D > kVoteMaxDraws) return fail(who, NBC_ERR_INVALID, "D must lie in 1..65535");
  if (reinterpret_cast<uintptr_t>(votes_dev) & 15u) return fail(who, NBC_ERR_INVALID, "votes_dev must be 16-byte aligned");
  const hipError_t e = launch_vote_accumulate(labels_dev, D, N, (long long)H * W, votes_dev, accumulate == 0, static_cast<hipStream_t>(hip_stream));
  if (e != hipSuccess) return fail(who, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

extern "C" int nbc_vote_summary(const uint32_t* votes_dev, int N, int H, int W, int draws, uint8_t* labels_dev, uint8_t* support_dev,
                                int64_t* stats_dev, void* hip_stream) {
  if (!votes_dev || !stats_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W)) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  if (draws < 1 || draws > kVoteMaxDraws) return fail(kWho, NBC_ERR_INVALID, "draws must lie in 1..65535");
  if (reinterpret_cast<uintptr_t>(votes_dev) & 3u) return fail(kWho, NBC_ERR_INVALID, "votes_dev must be 4-byte aligned");
  const long long P = (long long)H * W;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(stats_dev);
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(unsigned long long) * kCells * (size_t)N, s);
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  const dim3 grid(slices_for(P, kChunk, kSumThreads, kSumBlocksPerCall, N), (unsigned)N);
  hipLaunchKernelGGL(vote_summary_kernel, grid, dim3(kSumThreads), 0, s, votes_dev, P, (unsigned)draws, labels_dev, support_dev, stats);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
