// The flip views the training augmented over (include/nbc.h: nbc_tta_views, nbc_tta_merge).
//
// Two kernels, both without a context:
//   tta_views_kernel  a batch -> its V mirror images, view-major.  The row mover of row_views.hpp (its header states the units,
//                     the granules and the bounds it keeps at any alignment): a block stages a segment of a source row, then
//                     emits each view's copy of it -- mirrored unit by unit where the view mirrors columns, at row H-1-y where
//                     it mirrors rows.  The source is read once, every view written once: H * W * 3 * (1 + V) bytes per uint8
//                     image.
//   tta_merge_kernel  the low-resolution logits [V][N][3][h][w] of the stacked forward -> the aligned views and their mean
//                     in the stated order: 12 V h w bytes read per image, 12 (1 + V) h w written at most.  A thread per output
//                     element; contraction off, one IEEE division.
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "row_views.hpp"
#include "views_mean.hpp"

using namespace nbc;

namespace {

// what bit b of the mask mirrors
__host__ __device__ __forceinline__ bool mirrors_cols(int b) { return (b & 1) != 0; }
__host__ __device__ __forceinline__ bool mirrors_rows(int b) { return (b & 2) != 0; }

__host__ __device__ __forceinline__ int count_views(int views) {
  return (views & 1) + ((views >> 1) & 1) + ((views >> 2) & 1) + ((views >> 3) & 1);
}

// GT / UG: row_views.hpp.  rows = planes * H rows of W units.
template <typename GT, int UG>
__global__ __launch_bounds__(kViewThreads) void tta_views_kernel(const GT* __restrict__ x, GT* __restrict__ out, long long planes,
                                                                int H, int W, int views) {
  __shared__ __attribute__((aligned(16))) GT seg[kSegGranules<GT, UG>];
  const int segs = row_segments(W);
  const long long tasks = planes * H * segs;
  const long long row_g = (long long)W * UG;      // granules of a row

  for (long long task = blockIdx.x; task < tasks; task += gridDim.x) {
    const RowSegment t = row_segment(task, segs, W);
    const long long p = t.row / H;
    const int y = (int)(t.row % H);
    const int a0 = stage_segment(x + t.row * row_g + (long long)t.u0 * UG, t.nu * UG, seg);

    // ---- every view's copy of the segment
    int vj = 0;
    for (int b = 0; b < 4; ++b) {
      if (!((views >> b) & 1)) continue;
      const bool mc = mirrors_cols(b);
      const int yy = mirrors_rows(b) ? H - 1 - y : y;
      const int du0 = mc ? W - t.u0 - t.nu : t.u0;   // where the segment's units land in the destination row
      GT* dst = out + (((long long)vj * planes + p) * H + yy) * row_g + (long long)du0 * UG;
      ++vj;
      emit_run<GT, UG>(dst, seg, a0, t.nu, mc);
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

// what both entry points refuse of (N, h, w, views); nullptr when the shape is served
const char* bad_stack_shape(int N, int H, int W, int views) {
  if (views < 1 || views > NBC_TTA_FLIPS) return "views must be a mask of NBC_TTA_* bits in 1..15";
  if (!stack_entries_ok(N, count_views(views))) return "bad shape: N >= 1 and V * N <= 65535";
  if (!frame_shape_ok(H, W)) return "bad shape: H, W >= 1 and H * W < 2^31";
  return nullptr;
}

}  // namespace

extern "C" int nbc_tta_views(const void* x_dev, int x_dtype, int N, int H, int W, int views, void* out_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_tta_views";
  if (!x_dev || !out_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (x_dtype != NBC_IN_F32_NCHW && x_dtype != NBC_IN_U8_NHWC) return fail(kWho, NBC_ERR_INVALID, "bad x_dtype");
  if (const char* why = bad_stack_shape(N, H, W, views)) return fail(kWho, NBC_ERR_INVALID, why);
  const bool f32 = x_dtype == NBC_IN_F32_NCHW;
  if (f32 && !aligned4(x_dev, out_dev)) return fail(kWho, NBC_ERR_INVALID, "float32 x_dev and out_dev must be 4-byte aligned");
  const size_t bytes = (size_t)N * H * W * 3 * (f32 ? 4 : 1);
  if (ranges_overlap(x_dev, bytes, out_dev, bytes * count_views(views))) return fail(kWho, NBC_ERR_INVALID, "out_dev must not overlap x_dev");
  const hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const long long planes = (long long)N * (f32 ? 3 : 1);
  const dim3 grid(row_view_blocks(planes * H, W));
  if (f32)
    hipLaunchKernelGGL((tta_views_kernel<uint32_t, 1>), grid, dim3(kViewThreads), 0, s, static_cast<const uint32_t*>(x_dev),
                       static_cast<uint32_t*>(out_dev), planes, H, W, views);
  else
    hipLaunchKernelGGL((tta_views_kernel<unsigned char, 3>), grid, dim3(kViewThreads), 0, s, static_cast<const unsigned char*>(x_dev),
                       static_cast<unsigned char*>(out_dev), planes, H, W, views);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

extern "C" int nbc_tta_merge(const float* lowres_views_dev, int N, int h, int w, int views, float* merged_dev, float* aligned_dev,
                             void* hip_stream) {
  constexpr const char* kWho = "nbc_tta_merge";
  if (!lowres_views_dev || !merged_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (const char* why = bad_stack_shape(N, h, w, views)) return fail(kWho, NBC_ERR_INVALID, why);
  if (!aligned4(lowres_views_dev, merged_dev, aligned_dev)) return fail(kWho, NBC_ERR_INVALID, "float32 pointers must be 4-byte aligned");
  const size_t bytes = (size_t)N * 3 * h * w * sizeof(float), stack = bytes * count_views(views);
  if (ranges_overlap(lowres_views_dev, stack, merged_dev, bytes)) return fail(kWho, NBC_ERR_INVALID, "merged_dev must not overlap the input");
  if (aligned_dev && (ranges_overlap(lowres_views_dev, stack, aligned_dev, stack) || ranges_overlap(merged_dev, bytes, aligned_dev, stack)))
    return fail(kWho, NBC_ERR_INVALID, "aligned_dev must not alias the input or merged_dev");
  const dim3 grid(grid_stride_blocks(bytes / sizeof(float), kMergeThreads, 8));
  hipLaunchKernelGGL(tta_merge_kernel, grid, dim3(kMergeThreads), 0, static_cast<hipStream_t>(hip_stream), lowres_views_dev,
                     (long long)N * 3, h, w, views, merged_dev, aligned_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
