// The flip views the training augmented over (include/nbc.h: nbc_tta_views, nbc_tta_merge).
//
// Two kernels, both without a context:
//   tta_views_kernel  a batch -> its V mirror images, view-major.  A row is a run of units (a 3-byte pixel of uint8 NHWC, a
//                     4-byte element of a float32 NCHW plane) and is moved in granules (a byte, a 32-bit word).  A block takes a
//                     segment of a source row: 16-B loads put it into LDS at the row's own alignment, then each view's copy of
//                     the segment is put together out of LDS in the destination's own 16-B vectors -- mirrored unit by unit
//                     where the view mirrors columns, at row H-1-y where it mirrors rows.  The source is read once, every view
//                     written once: H * W * 3 * (1 + V) bytes per uint8 image.  Heads and tails that no aligned vector covers
//                     go granule by granule, so no access leaves [row start, row end) of either buffer, at any alignment.
//   tta_merge_kernel  the low-resolution logits [V][N][3][h][w] of the stacked forward -> the aligned views and their mean
//                     in the stated order: 12 V h w bytes read per image, 12 (1 + V) h w written at most.  A thread per output
//                     element; contraction off, one IEEE division.
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "views_mean.hpp"

using namespace nbc;

namespace {

constexpr int kViewThreads = 256;
constexpr int kSegUnits = 4096;                   // units of a row per block and round: 12 KiB of pixels, 16 KiB of floats
constexpr int kViewBlocksPerCu = 8;

// what bit b of the mask mirrors
__host__ __device__ __forceinline__ bool mirrors_cols(int b) { return (b & 1) != 0; }
__host__ __device__ __forceinline__ bool mirrors_rows(int b) { return (b & 2) != 0; }

__host__ __device__ __forceinline__ int count_views(int views) {
  return (views & 1) + ((views >> 1) & 1) + ((views >> 2) & 1) + ((views >> 3) & 1);
}

// GT: the granule (unsigned char / uint32_t); UG: granules per unit (3 / 1).  rows = planes * H rows of W units.
template <typename GT, int UG>
__global__ __launch_bounds__(kViewThreads) void tta_views_kernel(const GT* __restrict__ x, GT* __restrict__ out, long long planes,
                                                                int H, int W, int views) {
  constexpr int kPerVec = 16 / (int)sizeof(GT);   // granules of a 16-B vector
  __shared__ __attribute__((aligned(16))) GT seg[kSegUnits * UG + kPerVec];
  const int tid = threadIdx.x;
  const int segs = (W + kSegUnits - 1) / kSegUnits;
  const long long rows = planes * H, tasks = rows * segs;
  const long long row_g = (long long)W * UG;      // granules of a row

  for (long long task = blockIdx.x; task < tasks; task += gridDim.x) {
    const long long r = task / segs;
    const int u0 = (int)(task % segs) * kSegUnits;
    const int nu = (W - u0 < kSegUnits) ? W - u0 : kSegUnits;
    const int ng = nu * UG;                       // granules of this segment
    const long long p = r / H;
    const int y = (int)(r % H);

    // ---- the segment into LDS, granule i at seg[a0 + i]: a 16-B aligned global vector is a 16-B aligned LDS vector
    const GT* src = x + r * row_g + (long long)u0 * UG;
    const int a0 = (int)((reinterpret_cast<uintptr_t>(src) & 15u) / sizeof(GT));
    int head = (kPerVec - a0) % kPerVec;
    if (head > ng) head = ng;
    const int vecs = (ng - head) / kPerVec;
    for (int i = tid; i < head; i += kViewThreads) seg[a0 + i] = src[i];
    for (int v = tid; v < vecs; v += kViewThreads)
      *reinterpret_cast<uint4*>(&seg[a0 + head + v * kPerVec]) = *reinterpret_cast<const uint4*>(src + head + v * kPerVec);
    for (int i = head + vecs * kPerVec + tid; i < ng; i += kViewThreads) seg[a0 + i] = src[i];
    __syncthreads();

    // ---- every view's copy of the segment
    int vj = 0;
    for (int b = 0; b < 4; ++b) {
      if (!((views >> b) & 1)) continue;
      const bool mc = mirrors_cols(b);
      const int yy = mirrors_rows(b) ? H - 1 - y : y;
      const int du0 = mc ? W - u0 - nu : u0;      // where the segment's units land in the destination row
      GT* dst = out + (((long long)vj * planes + p) * H + yy) * row_g + (long long)du0 * UG;
      ++vj;
      // destination granule t of the segment is source granule t, or granule (nu-1-k) * UG + o of unit k = t / UG, o = t % UG
      auto fetch = [&](int t) -> GT {
        if (!mc) return seg[a0 + t];
        const int k = t / UG, o = t - k * UG;
        return seg[a0 + (nu - 1 - k) * UG + o];
      };
      int dhead = (int)(((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(GT));
      if (dhead > ng) dhead = ng;
      const int dvecs = (ng - dhead) / kPerVec;
      for (int i = tid; i < dhead; i += kViewThreads) dst[i] = fetch(i);
      for (int v = tid; v < dvecs; v += kViewThreads) {
        const int t0 = dhead + v * kPerVec;
        uint32_t w4[4];
        if constexpr (sizeof(GT) == 4) {
#pragma unroll
          for (int q = 0; q < 4; ++q) w4[q] = (uint32_t)fetch(t0 + q);
        } else {
          int k = t0 / UG, o = t0 - k * UG;       // one division per vector, then steps
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            w4[q] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const GT g = mc ? seg[a0 + (nu - 1 - k) * UG + o] : seg[a0 + t0 + 4 * q + e];
              w4[q] |= (uint32_t)g << (8 * e);
              if (++o == UG) { o = 0; ++k; }
            }
          }
        }
        *reinterpret_cast<uint4*>(dst + t0) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
      }
      for (int i = dhead + dvecs * kPerVec + tid; i < ng; i += kViewThreads) dst[i] = fetch(i);
    }
    __syncthreads();                              // the next round overwrites the segment
  }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 256;

#pragma clang fp contract(off)
__global__ __launch_bounds__(kMergeThreads) void tta_merge_kernel(const float* __restrict__ in, long long planes, int h, int w,
                                                                 int views, float* __restrict__ merged, float* __restrict__ aligned) {
  const long long hw = (long long)h * w, total = planes * hw;            // planes = 3 N
  const int V = count_views(views);
  const long long stride = (long long)gridDim.x * kMergeThreads;
  for (long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x; e < total; e += stride) {
    const long long pl = e / hw;
    const long long q = e - pl * hw;
    const int y = (int)(q / w), x = (int)(q - (long long)y * w);
    float sum = 0.f;
    int vj = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (!((views >> b) & 1)) continue;
      const int yy = mirrors_rows(b) ? h - 1 - y : y, xx = mirrors_cols(b) ? w - 1 - x : x;
      const float a = in[((long long)vj * planes + pl) * hw + (long long)yy * w + xx];
      if (aligned) aligned[(long long)vj * total + e] = a;
      sum = views_mean_add(sum, a, vj);            // the first view starts the sum: V = 1 keeps its bits, -0 included
      ++vj;
    }
    merged[e] = views_mean_finish(sum, V);
  }
}

bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// what both entry points refuse of (N, h, w, views); nullptr when the shape is served
const char* bad_stack_shape(int N, int H, int W, int views) {
  if (views < 1 || views > NBC_TTA_FLIPS) return "views must be a mask of NBC_TTA_* bits in 1..15";
  if (N < 1 || (long long)count_views(views) * N > 65535) return "bad shape: N >= 1 and V * N <= 65535";
  if (H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return "bad shape: H, W >= 1 and H * W < 2^31";
  return nullptr;
}

}  // namespace

namespace nbc {

hipError_t launch_tta_views(const void* x, int x_dtype, int N, int H, int W, int views, void* out, hipStream_t s) {
  if (x_dtype == NBC_IN_U8_NHWC) {
    const long long tasks = (long long)N * H * ((W + kSegUnits - 1) / kSegUnits);
    const dim3 grid(grid_stride_blocks((size_t)tasks, 1, kViewBlocksPerCu));
    hipLaunchKernelGGL((tta_views_kernel<unsigned char, 3>), grid, dim3(kViewThreads), 0, s, static_cast<const unsigned char*>(x),
                       static_cast<unsigned char*>(out), (long long)N, H, W, views);
  } else {
    const long long tasks = (long long)N * 3 * H * ((W + kSegUnits - 1) / kSegUnits);
    const dim3 grid(grid_stride_blocks((size_t)tasks, 1, kViewBlocksPerCu));
    hipLaunchKernelGGL((tta_views_kernel<uint32_t, 1>), grid, dim3(kViewThreads), 0, s, static_cast<const uint32_t*>(x),
                       static_cast<uint32_t*>(out), (long long)N * 3, H, W, views);
  }
  return hipGetLastError();
}

hipError_t launch_tta_merge(const float* lowres_views, int N, int h, int w, int views, float* merged, float* aligned, hipStream_t s) {
  const size_t total = (size_t)N * 3 * h * w;
  const dim3 grid(grid_stride_blocks(total, kMergeThreads, 8));
  hipLaunchKernelGGL(tta_merge_kernel, grid, dim3(kMergeThreads), 0, s, lowres_views, (long long)N * 3, h, w, views, merged, aligned);
  return hipGetLastError();
}

}  // namespace nbc

extern "C" int nbc_tta_views(const void* x_dev, int x_dtype, int N, int H, int W, int views, void* out_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_tta_views";
  if (!x_dev || !out_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (x_dtype != NBC_IN_F32_NCHW && x_dtype != NBC_IN_U8_NHWC) return fail(kWho, NBC_ERR_INVALID, "bad x_dtype");
  if (const char* why = bad_stack_shape(N, H, W, views)) return fail(kWho, NBC_ERR_INVALID, why);
  const bool f32 = x_dtype == NBC_IN_F32_NCHW;
  if (f32 && ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3u))
    return fail(kWho, NBC_ERR_INVALID, "float32 x_dev and out_dev must be 4-byte aligned");
  const size_t bytes = (size_t)N * H * W * 3 * (f32 ? 4 : 1);
  if (ranges_overlap(x_dev, bytes, out_dev, bytes * count_views(views))) return fail(kWho, NBC_ERR_INVALID, "out_dev must not overlap x_dev");
  const hipError_t e = launch_tta_views(x_dev, x_dtype, N, H, W, views, out_dev, static_cast<hipStream_t>(hip_stream));
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

extern "C" int nbc_tta_merge(const float* lowres_views_dev, int N, int h, int w, int views, float* merged_dev, float* aligned_dev,
                             void* hip_stream) {
  constexpr const char* kWho = "nbc_tta_merge";
  if (!lowres_views_dev || !merged_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (const char* why = bad_stack_shape(N, h, w, views)) return fail(kWho, NBC_ERR_INVALID, why);
  if ((reinterpret_cast<uintptr_t>(lowres_views_dev) | reinterpret_cast<uintptr_t>(merged_dev) | reinterpret_cast<uintptr_t>(aligned_dev)) & 3u)
    return fail(kWho, NBC_ERR_INVALID, "float32 pointers must be 4-byte aligned");
  const size_t bytes = (size_t)N * 3 * h * w * sizeof(float), stack = bytes * count_views(views);
  if (ranges_overlap(lowres_views_dev, stack, merged_dev, bytes)) return fail(kWho, NBC_ERR_INVALID, "merged_dev must not overlap the input");
  if (aligned_dev && (ranges_overlap(lowres_views_dev, stack, aligned_dev, stack) || ranges_overlap(merged_dev, bytes, aligned_dev, stack)))
    return fail(kWho, NBC_ERR_INVALID, "aligned_dev must not alias the input or merged_dev");
  const hipError_t e = launch_tta_merge(lowres_views_dev, N, h, w, views, merged_dev, aligned_dev, static_cast<hipStream_t>(hip_stream));
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
