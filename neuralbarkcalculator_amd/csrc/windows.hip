// The crop windows the training augmented over (include/nbc.h: nbc_window_grid, nbc_window_views, nbc_window_merge; DESIGN.md
// 3.18).
//
// One rule for the grid (Axis, on the host and on the device) and two kernels, both without a context:
//   window_views_kernel  a batch -> the K windows of every image, window-major, the rows and columns beyond the frame filled by
//                        reflection.  The row mover of row_views.hpp (its header states the units, the granules and the bounds
//                        it keeps at any alignment): a block stages a segment of a SOURCE row, then emits its part of every
//                        window row that is made of it -- the windows that cover the row, and those that cover the row beyond
//                        the frame that reflects it.  The at most 7 reflected units of a window row go granule by granule, inside
//                        the window row.  The source is read once, every window written once: 3 H W + 3 K E_y E_x bytes per
//                        uint8 image.
//   window_merge_kernel  the low-resolution logits [K][N][3][e_y][e_x] of the stacked forward -> [N][3][h][w], the weighted
//                        mean of the windows that cover a cell in ascending window order.  A thread per output element;
//                        contraction off, one IEEE division.
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "row_views.hpp"

using namespace nbc;

namespace {

// The windows of one axis, in any unit that divides everything (pixels for the views, cells of 8 pixels for the merge):
// l the padded length L8, e the extent E, t the stride T, n windows; window k < n - 1 starts at k * t, window n - 1 at last.
struct Axis {
  int l, e, t, n, last;
};

__host__ __device__ __forceinline__ int axis_offset(const Axis& a, int k) { return k == a.n - 1 ? a.last : k * a.t; }

// the windows that cover position p (0 <= p < l): `reg` regular ones from k = first on, then window n - 1 when `tail`; ascending k
struct Cover {
  int first, reg;
  bool tail;
  __host__ __device__ __forceinline__ int count() const { return reg + (tail ? 1 : 0); }
};

__host__ __device__ __forceinline__ Cover axis_cover(const Axis& a, int p) {
  Cover c;
  c.first = p < a.e ? 0 : (p - a.e) / a.t + 1;
  int hi = p / a.t;
  if (hi > a.n - 2) hi = a.n - 2;
  c.reg = hi >= c.first ? hi - c.first + 1 : 0;
  c.tail = a.last <= p;                              // last + e = l > p
  return c;
}

__host__ __device__ __forceinline__ int cover_window(const Axis& a, const Cover& c, int i) { return i < c.reg ? c.first + i : a.n - 1; }

// the per-axis tent weight of cell j of window k (units: cells)
__device__ __forceinline__ int axis_weight(const Axis& a, int k, int j) {
  const int off = axis_offset(a, k);
  int cap = a.e / 2;
  int wgt = cap < 1 ? 1 : cap;
  if (off > 0 && j + 1 < wgt) wgt = j + 1;
  if (off + a.e < a.l && a.e - j < wgt) wgt = a.e - j;
  return wgt;
}

Axis make_axis(int L, int S, int T, int unit) {
  const int l8 = (L + 7) / 8 * 8;
  Axis a;
  a.l = l8 / unit;
  a.e = (S < l8 ? S : l8) / unit;
  a.t = T / unit;
  a.n = l8 <= S ? 1 : 1 + (l8 - S + T - 1) / T;
  a.last = l8 <= S ? 0 : (l8 - S) / unit;
  return a;
}

// ---- views ---------------------------------------------------------------------------------------------------------------
// GT / UG: row_views.hpp.  planes * H source rows of W units; ay / ax in pixels.
template <typename GT, int UG>
__global__ __launch_bounds__(kViewThreads) void window_views_kernel(const GT* __restrict__ x, GT* __restrict__ out, long long planes,
                                                                   int H, int W, Axis ay, Axis ax) {
  __shared__ __attribute__((aligned(16))) GT seg[kSegGranules<GT, UG>];
  const int tid = threadIdx.x;
  const int segs = row_segments(W);
  const long long tasks = planes * H * segs;
  const long long row_g = (long long)W * UG;      // granules of a source row
  const long long wrow_g = (long long)ax.e * UG;  // granules of a window row

  for (long long task = blockIdx.x; task < tasks; task += gridDim.x) {
    const RowSegment t = row_segment(task, segs, W);
    const int u0 = t.u0, nu = t.nu;
    const long long p = t.row / H;
    const int y = (int)(t.row % H);
    const int a0 = stage_segment(x + t.row * row_g + (long long)u0 * UG, nu * UG, seg);

    // ---- the rows of the padded frame this source row is: itself, and row 2 (H - 1) - y when that lies in [H, L8)
    for (int pass = 0; pass < 2; ++pass) {
      const int yy = pass == 0 ? y : 2 * (H - 1) - y;
      if (pass == 1 && (yy < H || yy >= ay.l)) break;
      const Cover cy = axis_cover(ay, yy);
      for (int iy = 0; iy < cy.count(); ++iy) {
        const int ky = cover_window(ay, cy, iy);
        const int wy = yy - axis_offset(ay, ky);  // the row of the window, 0 <= wy < ay.e
        for (int kx = 0; kx < ax.n; ++kx) {
          const int ox = axis_offset(ax, kx);
          GT* wrow = out + ((((long long)ky * ax.n + kx) * planes + p) * ay.e + wy) * wrow_g;
          // the units of the window row that are units of the frame row and lie in the segment: [s0, s1) of the source row
          const int s0 = ox > u0 ? ox : u0;
          int s1 = ox + ax.e < u0 + nu ? ox + ax.e : u0 + nu;   // u0 + nu <= W
          if (s1 > s0) emit_run<GT, UG>(wrow + (long long)(s0 - ox) * UG, seg, a0 + (s0 - u0) * UG, s1 - s0, false);
          // the units beyond the frame, [max(ox, W), min(ox + e, L8)): unit xx is unit 2 (W - 1) - xx of the source row
          const int x0 = ox > W ? ox : W;
          const int x1 = ox + ax.e < ax.l ? ox + ax.e : ax.l;
          for (int i = tid; i < (x1 - x0) * UG; i += kViewThreads) {
            const int xx = x0 + i / UG, o = i % UG;
            const int sx = 2 * (W - 1) - xx;
            if (sx >= u0 && sx < u0 + nu) wrow[(long long)(xx - ox) * UG + o] = seg[a0 + (sx - u0) * UG + o];
          }
        }
      }
    }
    __syncthreads();                              // the next round overwrites the segment
  }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------
constexpr int kMergeThreads = 256;

#pragma clang fp contract(off)
// ay / ax in cells; in [K][planes][e_y][e_x], merged [planes][h][w] with planes = 3 N
__global__ __launch_bounds__(kMergeThreads) void window_merge_kernel(const float* __restrict__ in, long long planes, Axis ay, Axis ax,
                                                                    int uniform, float* __restrict__ merged) {
  const int h = ay.l, w = ax.l;
  const long long hw = (long long)h * w, total = planes * hw, ehw = (long long)ay.e * ax.e;
  const long long stride = (long long)gridDim.x * kMergeThreads;
  for (long long e = (long long)blockIdx.x * kMergeThreads + threadIdx.x; e < total; e += stride) {
    const long long pl = e / hw;
    const long long q = e - pl * hw;
    const int y = (int)(q / w), x = (int)(q - (long long)y * w);
    const Cover cy = axis_cover(ay, y), cx = axis_cover(ax, x);
    const int ny = cy.count(), nx = cx.count();
    float acc = 0.f;
    int wsum = 0;
    for (int iy = 0; iy < ny; ++iy) {
      const int ky = cover_window(ay, cy, iy);
      const int jy = y - axis_offset(ay, ky);
      const int wy = uniform ? 1 : axis_weight(ay, ky, jy);
      for (int ix = 0; ix < nx; ++ix) {
        const int kx = cover_window(ax, cx, ix);
        const int jx = x - axis_offset(ax, kx);
        const int wgt = uniform ? 1 : wy * axis_weight(ax, kx, jx);
        const float v = in[(((long long)ky * ax.n + kx) * planes + pl) * ehw + (long long)jy * ax.e + jx];
        if (ny * nx == 1) {
          acc = v;                                  // one window: its own bits, -0 included
        } else {
          const float prod = (float)wgt * v;
          acc = (iy | ix) == 0 ? prod : acc + prod;
        }
        wsum += wgt;
      }
    }
    merged[e] = ny * nx == 1 ? acc : __fdiv_rn(acc, (float)wsum);
  }
}

// what every entry point refuses of (H, W, S, T); nullptr when the grid is served
const char* bad_grid(int H, int W, int S, int T) {
  if (S < 32 || S > 2048 || S % NBC_WINDOW_CELL) return "window must be a multiple of 8 in 32..2048";
  if (T < NBC_WINDOW_CELL || T % NBC_WINDOW_CELL || T > S || S > 8 * T)
    return "stride must be a multiple of 8 with 8 <= stride <= window <= 8 * stride";
  if (H < 8 || W < 8) return "bad shape: H, W >= 8";
  if (!frame_shape_ok(H, W)) return "bad shape: H * W < 2^31";
  if ((long long)make_axis(H, S, T, 1).n * make_axis(W, S, T, 1).n > NBC_WINDOW_MAX_K) return "more than 1024 windows per image";
  return nullptr;
}

const char* bad_stack(int N, int H, int W, int S, int T) {
  if (N < 1) return "bad shape: N >= 1";
  if (const char* why = bad_grid(H, W, S, T)) return why;
  if (!stack_entries_ok(N, (long long)make_axis(H, S, T, 1).n * make_axis(W, S, T, 1).n)) return "bad shape: K * N <= 65535";
  return nullptr;
}

}  // namespace

extern "C" int nbc_window_grid(int H, int W, int S, int T, int* dims, int* offsets_y, int* offsets_x) {
  constexpr const char* kWho = "nbc_window_grid";
  if (!dims) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (const char* why = bad_grid(H, W, S, T)) return fail(kWho, NBC_ERR_INVALID, why);
  const Axis ay = make_axis(H, S, T, 1), ax = make_axis(W, S, T, 1);
  dims[0] = ay.e, dims[1] = ax.e, dims[2] = ay.n, dims[3] = ax.n;
  for (int k = 0; offsets_y && k < ay.n; ++k) offsets_y[k] = axis_offset(ay, k);
  for (int k = 0; offsets_x && k < ax.n; ++k) offsets_x[k] = axis_offset(ax, k);
  return NBC_OK;
}

extern "C" int nbc_window_views(const void* x_dev, int x_dtype, int N, int H, int W, int S, int T, void* out_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_window_views";
  if (!x_dev || !out_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (x_dtype != NBC_IN_F32_NCHW && x_dtype != NBC_IN_U8_NHWC) return fail(kWho, NBC_ERR_INVALID, "bad x_dtype");
  if (const char* why = bad_stack(N, H, W, S, T)) return fail(kWho, NBC_ERR_INVALID, why);
  const bool f32 = x_dtype == NBC_IN_F32_NCHW;
  if (f32 && !aligned4(x_dev, out_dev)) return fail(kWho, NBC_ERR_INVALID, "float32 x_dev and out_dev must be 4-byte aligned");
  const Axis ay = make_axis(H, S, T, 1), ax = make_axis(W, S, T, 1);
  const size_t unit = 3 * (f32 ? 4 : 1);
  const size_t in_bytes = (size_t)N * H * W * unit, out_bytes = (size_t)ay.n * ax.n * N * ay.e * ax.e * unit;
  if (ranges_overlap(x_dev, in_bytes, out_dev, out_bytes)) return fail(kWho, NBC_ERR_INVALID, "out_dev must not overlap x_dev");
  const hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const long long planes = (long long)N * (f32 ? 3 : 1);
  const dim3 grid(row_view_blocks(planes * H, W));
  if (f32)
    hipLaunchKernelGGL((window_views_kernel<uint32_t, 1>), grid, dim3(kViewThreads), 0, s, static_cast<const uint32_t*>(x_dev),
                       static_cast<uint32_t*>(out_dev), planes, H, W, ay, ax);
  else
    hipLaunchKernelGGL((window_views_kernel<unsigned char, 3>), grid, dim3(kViewThreads), 0, s, static_cast<const unsigned char*>(x_dev),
                       static_cast<unsigned char*>(out_dev), planes, H, W, ay, ax);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

extern "C" int nbc_window_merge(const float* lowres_windows_dev, int N, int H, int W, int S, int T, int blend, float* merged_dev,
                                void* hip_stream) {
  constexpr const char* kWho = "nbc_window_merge";
  if (!lowres_windows_dev || !merged_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (blend != NBC_BLEND_TENT && blend != NBC_BLEND_UNIFORM) return fail(kWho, NBC_ERR_INVALID, "bad blend");
  if (const char* why = bad_stack(N, H, W, S, T)) return fail(kWho, NBC_ERR_INVALID, why);
  if (!aligned4(lowres_windows_dev, merged_dev)) return fail(kWho, NBC_ERR_INVALID, "float32 pointers must be 4-byte aligned");
  const Axis ay = make_axis(H, S, T, NBC_WINDOW_CELL), ax = make_axis(W, S, T, NBC_WINDOW_CELL);
  const size_t out_bytes = (size_t)N * 3 * ay.l * ax.l * sizeof(float);
  const size_t in_bytes = (size_t)ay.n * ax.n * N * 3 * ay.e * ax.e * sizeof(float);
  if (ranges_overlap(lowres_windows_dev, in_bytes, merged_dev, out_bytes))
    return fail(kWho, NBC_ERR_INVALID, "merged_dev must not overlap the input");
  const dim3 grid(grid_stride_blocks(out_bytes / sizeof(float), kMergeThreads, 8));
  hipLaunchKernelGGL(window_merge_kernel, grid, dim3(kMergeThreads), 0, static_cast<hipStream_t>(hip_stream), lowres_windows_dev,
                     (long long)N * 3, ay, ax, blend == NBC_BLEND_UNIFORM ? 1 : 0, merged_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
