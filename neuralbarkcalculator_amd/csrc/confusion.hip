// Per-image 3x3 confusion counts of predicted labels against a grey target mask: what the evaluation loop of
// the reference's bark_calculator/__main__.py:331-332 (lovasz `iou`, `PixelWiseF1`) counts on the host, pixel by
// pixel, before it divides.  Only the 9 integers per image leave the device; the ratios are host arithmetic
// (neuralbarkcalculator_amd/metrics.py).
//
// A byte stream (reduce.hpp): 2 B per pixel with uint8 labels, 9 B with int64 labels, nothing reused.  A chunk is 16 pixels
// (one 16-B load of target bytes, one 16-B load of u8 labels or eight of int64 labels), counted into a packed 64-bit word
// (7 bits per cell: at most 16 per chunk) and unpacked into 9 register counters, which block_add sums into the image's cells.
// Blocks of 1024 threads, about 128 of them per call.  The grid is (slices of an image) x N.
#include <hip/hip_runtime.h>

#include "reduce.hpp"

using namespace nbc;

namespace {

constexpr int kThreads = 1024;                  // 16 waves: few blocks, so few atomics on the 9 cells of an image
constexpr int kChunk = 16;                      // pixels per thread and step (16 target bytes)
constexpr int kCells = 9;
constexpr int kBlocksPerCall = 128;
constexpr const char* kWho = "nbc_confusion";

// cell 3 t + p; a label outside {0,1,2} is counted nowhere
__device__ __forceinline__ unsigned long long cell_bit(unsigned grey, unsigned long long label) {
  const unsigned cell = target_class(grey) * 3u + (unsigned)label;
  return label < 3ull ? (1ull << (7u * cell)) : 0ull;
}

__device__ __forceinline__ void unpack(unsigned long long packed, unsigned (&cnt)[kCells]) {
#pragma unroll
  for (int k = 0; k < kCells; ++k) cnt[k] += (unsigned)(packed >> (7 * k)) & 127u;
}

__device__ __forceinline__ unsigned long long chunk_bits(const unsigned char* __restrict__ lab, const unsigned char* __restrict__ tgt,
                                                         long long i) {
  const uint4 l = *reinterpret_cast<const uint4*>(lab + i);
  const uint4 t = *reinterpret_cast<const uint4*>(tgt + i);
  const unsigned lw[4] = {l.x, l.y, l.z, l.w}, tw[4] = {t.x, t.y, t.z, t.w};
  unsigned long long packed = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) packed += cell_bit((tw[j >> 2] >> (8 * (j & 3))) & 255u, (lw[j >> 2] >> (8 * (j & 3))) & 255u);
  return packed;
}

__device__ __forceinline__ unsigned long long chunk_bits(const long long* __restrict__ lab, const unsigned char* __restrict__ tgt,
                                                         long long i) {
  const uint4 t = *reinterpret_cast<const uint4*>(tgt + i);
  const unsigned tw[4] = {t.x, t.y, t.z, t.w};
  const ulonglong2* l2 = reinterpret_cast<const ulonglong2*>(lab + i);
  unsigned long long packed = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const ulonglong2 l = l2[j];
    packed += cell_bit((tw[j >> 1] >> (16 * (j & 1))) & 255u, l.x);
    packed += cell_bit((tw[j >> 1] >> (16 * (j & 1) + 8)) & 255u, l.y);
  }
  return packed;
}

template <typename LabelT>
__global__ __launch_bounds__(kThreads) void confusion_kernel(const LabelT* __restrict__ labels, const unsigned char* __restrict__ target,
                                                             long long P, unsigned long long* __restrict__ conf) {
  const long long base = (long long)blockIdx.y * P;
  const LabelT* lab = labels + base;
  const unsigned char* tgt = target + base;
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * kThreads;
  unsigned cnt[kCells] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

  // the vector body starts at the first pixel whose target byte is 16-B aligned and needs the label there aligned too
  // (always so for buffers that start 16-B aligned: then the label's offset is a multiple of 16 elements as well)
  ByteStream st(tgt, P, kChunk);
  if ((reinterpret_cast<uintptr_t>(lab + st.head)) & 15u) st.drop_body();

  const long long g = (long long)blockIdx.x * kThreads + tid;
  for (long long c = g; c < st.chunks; c += stride) unpack(chunk_bits(lab, tgt, st.head + c * kChunk), cnt);

  // the pixels outside the body (head and tail, or every pixel of an image the body cannot reach), one per thread
  unsigned long long packed = 0;
  int in_packed = 0;
  st.for_each_outside(g, stride, [&](long long q) {
    packed += cell_bit(tgt[q], (unsigned long long)lab[q]);
    if (++in_packed == 127) { unpack(packed, cnt); packed = 0; in_packed = 0; }
  });
  unpack(packed, cnt);

  block_add<kThreads, kCells>(cnt, conf + (size_t)blockIdx.y * kCells);
}

}  // namespace

extern "C" int nbc_confusion(const void* labels_dev, int labels_dtype, const uint8_t* target_dev, int N, int H, int W,
                             int64_t* conf_dev, void* hip_stream) {
  if (!labels_dev || !target_dev || !conf_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W)) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  if (!label_dtype_ok(labels_dtype)) return fail(kWho, NBC_ERR_INVALID, "bad labels_dtype");
  const long long P = (long long)H * W;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  unsigned long long* conf = reinterpret_cast<unsigned long long*>(conf_dev);
  hipError_t e = hipMemsetAsync(conf, 0, sizeof(unsigned long long) * kCells * (size_t)N, s);
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  // about 128 blocks over the batch.  Every block of an image adds into the same 9 cells, and atomics on one address
  // serialise: per 1024^2 x 2 call inside the evaluation run (rocprofv3, other streams' forwards beside it) 512 blocks of
  // 256 threads took 11.4 us (median), these 128 blocks of 1024 threads 8.7 us; the 4 MB read alone would take under 1 us
  // at HBM rate.
  const dim3 grid(slices_for(P, kChunk, kThreads, kBlocksPerCall, N), (unsigned)N);
  if (labels_dtype == NBC_LABEL_I64)
    hipLaunchKernelGGL(confusion_kernel<long long>, grid, dim3(kThreads), 0, s, static_cast<const long long*>(labels_dev), target_dev,
                       P, conf);
  else
    hipLaunchKernelGGL(confusion_kernel<unsigned char>, grid, dim3(kThreads), 0, s, static_cast<const unsigned char*>(labels_dev),
                       target_dev, P, conf);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
