// The two counting passes behind the reference's dataset statistics, per image, on the device:
//   * nbc_image_moments: per channel the sum of the bytes and the sum of their squares of uint8 RGB frames, which is all that
//     compute_mean_std (bark_calculator/utils.py:23-39: ToTensor, .mean(2), .std(2) per image) needs;
//   * nbc_target_counts: the pixels per class of the grey target masks, what compute_pos_weight (utils.py:51-69) counts, and
//     the pixels whose grey level is none of 0, 127, 255.
// Only 6 + 4 integers per image leave the device; the divisions and the square root are host arithmetic
// (neuralbarkcalculator_amd/stats.py).
//
// Both are byte streams with nothing reused, walked and summed by reduce.hpp's ByteStream and block_add.  The grid is
// (slices of an image) x N, blocks of 1024 threads.
//
// Moments: interleaved RGB, so 48 bytes (three 16-byte loads) hold 16 whole pixels and byte j of a 48-byte chunk always
// belongs to "slot" j % 3.  The body starts at the image's first 16-byte boundary, `head` bytes in, so slot s is channel
// (head + s) % 3 for the whole image: the loop sums per slot and the slots are renamed once behind it.  Byte b of dword d of a
// chunk has slot (d + b) % 3 (4 = 1 mod 3): three dword classes, each with one 0/1 byte mask per slot.  A slot's sum is a
// v_dot4_u32_u8 of the dword with the mask, its sum of squares one of the masked dword with the dword.  A chunk adds at most
// 16 x 255 to a sum and 16 x 65025 to a sum of squares: they are taken per chunk in 32 bits and accumulated in 64.
//
// Counts: target_class is (v + 64) >> 7, so with a = bytes >= 64 and b = bytes >= 192
// of a dword (bit 7 | bit 6, bit 7 & bit 6: one popcount each) the classes hold 4 - a, a - b and b of its pixels; the bytes
// equal to 0, 127 or 255 are found with the exact zero-byte test ~(((x & 0x7f..) + 0x7f..) | x | 0x7f..) on v, v ^ 0x7f.. and ~v.
#include <hip/hip_runtime.h>

#include "reduce.hpp"

using namespace nbc;

namespace {

constexpr int kThreads = 1024;                  // 16 waves: few blocks, so few atomics on the cells of an image
constexpr int kBlocksPerCall = 256;             // about one block per CU over the whole batch
constexpr int kMomentChunk = 48;                // bytes per thread and step: 16 RGB pixels, three 16-byte loads
constexpr int kCountChunk = 16;                 // bytes (pixels) per thread and step
constexpr int kMomentCells = 6;                 // [channel][sum, sum of squares]
constexpr int kCountCells = 4;                  // class 0, 1, 2, off-level

typedef unsigned long long u64;

// the bytes of a dword of class k (= dword index % 3) that belong to slot s: (k + b) % 3 == s
__device__ __forceinline__ constexpr unsigned slot_mask(int k, int s, unsigned one) {
  unsigned m = 0;
  for (int b = 0; b < 4; ++b)
    if ((k + b) % 3 == s) m |= one << (8 * b);
  return m;
}

__global__ __launch_bounds__(kThreads) void image_moments_kernel(const unsigned char* __restrict__ x, long long B,
                                                                 u64* __restrict__ moments) {
  const unsigned char* img = x + (long long)blockIdx.y * B;      // B = 3 H W bytes per image
  const int tid = threadIdx.x;
  const long long g = (long long)blockIdx.x * kThreads + tid;
  const long long stride = (long long)gridDim.x * kThreads;

  const ByteStream st(img, B, kMomentChunk);

  u64 s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};     // per slot
  for (long long c = g; c < st.chunks; c += stride) {
    const uint4* p = reinterpret_cast<const uint4*>(img + st.head + c * kMomentChunk);
    const uint4 a = p[0], b = p[1], d = p[2];
    const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
    unsigned c1[3] = {0, 0, 0}, c2[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 12; ++j) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        c1[s] = __builtin_amdgcn_udot4(w[j], slot_mask(j % 3, s, 0x01u), c1[s], false);
        c2[s] = __builtin_amdgcn_udot4(w[j] & slot_mask(j % 3, s, 0xffu), w[j], c2[s], false);
      }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) { s1[s] += c1[s]; s2[s] += c2[s]; }
  }

  // slot s is channel (head + s) % 3; then the bytes outside the body (at most 15 + 47 of them), one per thread
  const int ph = (int)(st.head % 3);
  u64 acc[kMomentCells];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int s = (ch - ph + 3) % 3;
    acc[2 * ch] = s == 0 ? s1[0] : s == 1 ? s1[1] : s1[2];
    acc[2 * ch + 1] = s == 0 ? s2[0] : s == 1 ? s2[1] : s2[2];
  }
  st.for_each_outside(g, stride, [&](long long q) {
    const unsigned v = img[q];
    const int ch = (int)(q % 3);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (ch == k) { acc[2 * k] += v; acc[2 * k + 1] += v * v; }
  });

  block_add<kThreads, kMomentCells>(acc, moments + (size_t)blockIdx.y * kMomentCells);
}

// 0x80 in every byte of x that is zero, 0 elsewhere (exact: no carry crosses a byte)
__device__ __forceinline__ unsigned zero_bytes(unsigned x) {
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

__global__ __launch_bounds__(kThreads) void target_counts_kernel(const unsigned char* __restrict__ target, long long P,
                                                                 u64* __restrict__ counts) {
  const unsigned char* tgt = target + (long long)blockIdx.y * P;
  const int tid = threadIdx.x;
  const long long g = (long long)blockIdx.x * kThreads + tid;
  const long long stride = (long long)gridDim.x * kThreads;

  const ByteStream st(tgt, P, kCountChunk);

  unsigned cnt[kCountCells] = {0, 0, 0, 0};     // at most 2^31 / 1024 pixels per thread
  for (long long c = g; c < st.chunks; c += stride) {
    const uint4 t = *reinterpret_cast<const uint4*>(tgt + st.head + c * kCountChunk);
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
    unsigned ge64 = 0, ge192 = 0, on = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ge64 += __popc((w[j] | (w[j] << 1)) & 0x80808080u);
      ge192 += __popc(w[j] & (w[j] << 1) & 0x80808080u);
      on += __popc(zero_bytes(w[j]) | zero_bytes(w[j] ^ 0x7f7f7f7fu) | zero_bytes(~w[j]));
    }
    cnt[0] += 16u - ge64; cnt[1] += ge64 - ge192; cnt[2] += ge192; cnt[3] += 16u - on;
  }
  st.for_each_outside(g, stride, [&](long long q) {
    const unsigned v = tgt[q];
    const unsigned cls = target_class(v);
    cnt[0] += cls == 0u; cnt[1] += cls == 1u; cnt[2] += cls == 2u;
    cnt[3] += (v != 0u && v != 127u && v != 255u);
  });

  const u64 acc[kCountCells] = {cnt[0], cnt[1], cnt[2], cnt[3]};
  block_add<kThreads, kCountCells>(acc, counts + (size_t)blockIdx.y * kCountCells);
}

// what both entry points refuse, decided before any HIP call; then the memset of the cells and the launch
template <typename Kernel>
int run(const char* who, Kernel kernel, const uint8_t* in, int channels, int chunk, int cells, int N, int H, int W, void* out_dev,
        void* hip_stream) {
  if (!in || !out_dev) return fail(who, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W)) return fail(who, NBC_ERR_INVALID, kPerImageShape);
  const long long bytes = (long long)channels * H * W;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  u64* out = static_cast<u64*>(out_dev);
  hipError_t e = hipMemsetAsync(out, 0, sizeof(u64) * cells * (size_t)N, s);
  if (e != hipSuccess) return fail(who, NBC_ERR_HIP, hipGetErrorString(e));
  hipLaunchKernelGGL(kernel, dim3(slices_for(bytes, chunk, kThreads, kBlocksPerCall, N), (unsigned)N), dim3(kThreads), 0, s, in, bytes, out);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(who, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

}  // namespace

extern "C" int nbc_image_moments(const uint8_t* x_dev, int N, int H, int W, uint64_t* moments_dev, void* hip_stream) {
  return run("nbc_image_moments", image_moments_kernel, x_dev, 3, kMomentChunk, kMomentCells, N, H, W, moments_dev, hip_stream);
}

extern "C" int nbc_target_counts(const uint8_t* target_dev, int N, int H, int W, int64_t* counts_dev, void* hip_stream) {
  return run("nbc_target_counts", target_counts_kernel, target_dev, 1, kCountChunk, kCountCells, N, H, W, counts_dev, hip_stream);
}
