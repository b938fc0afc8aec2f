// The colour-jitter views the training augmented over (include/nbc.h: nbc_jitter_views, nbc_views_mean).
//
// Three kernels, all without a context:
//   jitter_grey_sum_kernel  the contrast step's mean grey: per (brightness factor b of a view with c != 1, image) the uint64 sum
//                           of the grey of the brightness-adjusted pixels.  wave_sum, the block's waves through LDS, one 64-bit
//                           integer atomic per block into the workspace (reduce.hpp: block_add); integer sums do not depend on
//                           arrival order.  H * W * 3 bytes read per image and distinct b.
//   jitter_apply_kernel     a batch -> its V views, view-major.  A lane's unit is 16 pixels = 48 bytes = three 16-byte vectors,
//                           the least common run of whole pixels and whole vectors; units start where a pixel of the image starts
//                           on a 16-byte boundary.  The unit stays in registers across the V views: the source is read once,
//                           every view written once, H * W * 3 * (1 + V) bytes per image.  The pixels before the first unit and
//                           after the last one, and a view's copy of a unit that does not fall on a 16-byte boundary itself, go
//                           byte by byte: no access leaves [base, base + N * H * W * 3) of the source or of a view.
//   views_mean_kernel       the low-resolution logits [V][N][3][h][w] of the stacked forward -> their mean in the stated order
//                           (views_mean.hpp); a thread per output element.
// Every step of a view is blend(degenerate, image, f) = float(d) + f * float(i - d): one f32 multiply, one f32 add, contraction
// off, clamped to 0..255 and truncated.
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "views_mean.hpp"

using namespace nbc;

namespace {

constexpr int kMaxViews = NBC_JITTER_MAX_VIEWS;
constexpr int kThreads = 256;
constexpr int kUnitPixels = 16;                   // 48 bytes: three 16-byte vectors
constexpr int kUnitWords = 12;
constexpr int kBlocksPerCu = 8;

// the views as kernel arguments: the factors, and for a view with c != 1 the workspace row that holds its grey sums
struct JitterArgs {
  float b[kMaxViews], c[kMaxViews], s[kMaxViews];
  int slot[kMaxViews];
  int V;
};
// the distinct brightness factors of the views with c != 1
struct GreySumArgs {
  float b[kMaxViews];
};

#pragma clang fp contract(off)
__device__ __forceinline__ unsigned blend(int d, int i, float f) {
  const float t = (float)d + f * (float)(i - d);
  return t <= 0.f ? 0u : (t >= 255.f ? 255u : (unsigned)(int)t);
}

__device__ __forceinline__ unsigned grey_of(unsigned r, unsigned g, unsigned b) {
  return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

__device__ __forceinline__ void brighten(unsigned& r, unsigned& g, unsigned& b, float fb) {
  if (fb != 1.f) {
    r = blend(0, (int)r, fb);
    g = blend(0, (int)g, fb);
    b = blend(0, (int)b, fb);
  }
}

// saturation_s(contrast_c(brightness_b(pixel))); m: the rounded mean grey of the brightness-adjusted image (used when fc != 1)
__device__ __forceinline__ void view_pixel(unsigned& r, unsigned& g, unsigned& b, float fb, float fc, float fs, int m) {
  brighten(r, g, b, fb);
  if (fc != 1.f) {
    r = blend(m, (int)r, fc);
    g = blend(m, (int)g, fc);
    b = blend(m, (int)b, fc);
  }
  if (fs != 1.f) {
    const int l = (int)grey_of(r, g, b);
    r = blend(l, (int)r, fs);
    g = blend(l, (int)g, fs);
    b = blend(l, (int)b, fs);
  }
}

// An image's P pixels from any address: `head` pixels up to the first pixel that starts on a 16-byte boundary (3 is a unit
// modulo 16: pixel p starts at base + 3 p, and 3 * 11 = 33 = 1), `units` whole units, and the pixels from `tail` on.
struct PixelRun {
  long long head, units, tail;
  __device__ __forceinline__ PixelRun(const void* base, long long P) {
    head = (long long)(((0u - (unsigned)reinterpret_cast<uintptr_t>(base)) * 11u) & 15u);
    if (head > P) head = P;
    units = (P - head) / kUnitPixels;
    tail = head + units * kUnitPixels;
  }
  // the pixels outside the units, numbered 0 .. outside() - 1
  __device__ __forceinline__ long long outside(long long P) const { return head + (P - tail); }
  __device__ __forceinline__ long long pixel(long long t) const { return t < head ? t : tail + (t - head); }
};

__device__ __forceinline__ void load_unit(const unsigned char* at, uint32_t (&w)[kUnitWords]) {
  const uint4* v = reinterpret_cast<const uint4*>(at);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const uint4 x = v[q];
    w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
  }
}
__device__ __forceinline__ unsigned unit_byte(const uint32_t (&w)[kUnitWords], int q) { return (w[q >> 2] >> (8 * (q & 3))) & 0xffu; }

// sums[k * N + i] += the grey of every pixel of image i under brightness b[k]; grid (slices, N, K)
__global__ __launch_bounds__(kThreads) void jitter_grey_sum_kernel(const unsigned char* __restrict__ x, int N, long long P,
                                                                    GreySumArgs a, unsigned long long* __restrict__ sums) {
  const int i = blockIdx.y, k = blockIdx.z, tid = threadIdx.x;
  const float fb = a.b[k];
  const unsigned char* src = x + (long long)i * P * 3;
  const PixelRun run(src, P);
  unsigned long long acc[1] = {0ull};
  for (long long u = (long long)blockIdx.x * kThreads + tid; u < run.units; u += (long long)gridDim.x * kThreads) {
    uint32_t w[kUnitWords];
    load_unit(src + (run.head + u * kUnitPixels) * 3, w);
    unsigned part = 0;                            // 16 * 255 at most
#pragma unroll
    for (int p = 0; p < kUnitPixels; ++p) {
      unsigned r = unit_byte(w, 3 * p), g = unit_byte(w, 3 * p + 1), b = unit_byte(w, 3 * p + 2);
      brighten(r, g, b, fb);
      part += grey_of(r, g, b);
    }
    acc[0] += part;
  }
  if (blockIdx.x == 0) {
    for (long long t = tid; t < run.outside(P); t += kThreads) {
      const unsigned char* px = src + run.pixel(t) * 3;
      unsigned r = px[0], g = px[1], b = px[2];
      brighten(r, g, b, fb);
      acc[0] += grey_of(r, g, b);
    }
  }
  block_add<kThreads, 1>(acc, sums + (long long)k * N + i);
}

// out[(j * N + i)] = view j of image i; grid (slices, N).  sums: the workspace jitter_grey_sum_kernel filled (read only where a
// view has c != 1).
__global__ __launch_bounds__(kThreads) void jitter_apply_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ out,
                                                                 int N, long long P, JitterArgs a,
                                                                 const unsigned long long* __restrict__ sums) {
  __shared__ int mean_grey[kMaxViews];
  const int i = blockIdx.y, tid = threadIdx.x, V = a.V;
  if (tid < V) {                                  // m = floor((2 S + P) / (2 P)): the mean grey, an exact half rounded up
    int m = 0;
    if (a.c[tid] != 1.f) {
      const unsigned long long S = sums[(long long)a.slot[tid] * N + i];
      m = (int)((2ull * S + (unsigned long long)P) / (2ull * (unsigned long long)P));
    }
    mean_grey[tid] = m;
  }
  __syncthreads();
  const long long image = (long long)i * P * 3, entry = (long long)N * P * 3;   // bytes: where image i starts, a view's size
  const unsigned char* src = x + image;
  const PixelRun run(src, P);

  for (long long u = (long long)blockIdx.x * kThreads + tid; u < run.units; u += (long long)gridDim.x * kThreads) {
    const long long at = (run.head + u * kUnitPixels) * 3;
    uint32_t w[kUnitWords];
    load_unit(src + at, w);
    for (int j = 0; j < V; ++j) {
      const float fb = a.b[j], fc = a.c[j], fs = a.s[j];
      const int m = mean_grey[j];
      uint32_t o[kUnitWords];
#pragma unroll
      for (int q = 0; q < kUnitWords; ++q) o[q] = 0u;
#pragma unroll
      for (int p = 0; p < kUnitPixels; ++p) {
        unsigned r = unit_byte(w, 3 * p), g = unit_byte(w, 3 * p + 1), b = unit_byte(w, 3 * p + 2);
        view_pixel(r, g, b, fb, fc, fs, m);
        o[(3 * p) >> 2] |= r << (8 * ((3 * p) & 3));
        o[(3 * p + 1) >> 2] |= g << (8 * ((3 * p + 1) & 3));
        o[(3 * p + 2) >> 2] |= b << (8 * ((3 * p + 2) & 3));
      }
      unsigned char* dst = out + (long long)j * entry + image + at;
      if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        uint4* v = reinterpret_cast<uint4*>(dst);
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
      } else {                                    // this view's copy of the image lies at another alignment than the source
#pragma unroll
        for (int q = 0; q < 4 * kUnitWords; ++q) dst[q] = (unsigned char)unit_byte(o, q);
      }
    }
  }
  if (blockIdx.x == 0) {
    for (long long t = tid; t < run.outside(P); t += kThreads) {
      const long long at = run.pixel(t) * 3;
      const unsigned r0 = src[at], g0 = src[at + 1], b0 = src[at + 2];
      for (int j = 0; j < V; ++j) {
        unsigned r = r0, g = g0, b = b0;
        view_pixel(r, g, b, a.b[j], a.c[j], a.s[j], mean_grey[j]);
        unsigned char* dst = out + (long long)j * entry + image + at;
        dst[0] = (unsigned char)r;
        dst[1] = (unsigned char)g;
        dst[2] = (unsigned char)b;
      }
    }
  }
}

// mean[e] of in[j * total + e], j = 0 .. V - 1
__global__ __launch_bounds__(kThreads) void views_mean_kernel(const float* __restrict__ in, long long total, int V,
                                                               float* __restrict__ mean) {
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    float sum = 0.f;
    for (int j = 0; j < V; ++j) sum = views_mean_add(sum, in[(long long)j * total + e], j);
    mean[e] = views_mean_finish(sum, V);
  }
}

// what the entry points refuse of (N, V) and of (H, W); nullptr when the shape is served
const char* bad_stack(int N, int V) {
  if (V < 1 || V > kMaxViews) return "V must lie in 1..16";
  if (!stack_entries_ok(N, V)) return "bad shape: N >= 1 and V * N <= 65535";
  return nullptr;
}
const char* bad_frame(int H, int W) {
  if (!frame_shape_ok(H, W)) return "bad shape: H, W >= 1 and H * W < 2^31";
  return nullptr;
}

// blocks along x of a (slices, N[, K]) grid over `units` units per image: no more than the units fill, about kBlocksPerCu per CU
unsigned slices_of(long long units, long long images) {
  long long slices = (units + kThreads - 1) / kThreads;
  const long long want = ((long long)256 * kBlocksPerCu + images - 1) / images;
  if (slices > want) slices = want;
  return (unsigned)(slices < 1 ? 1 : slices);
}

}  // namespace

extern "C" int nbc_jitter_workspace_bytes(int N, int V, size_t* bytes) {
  constexpr const char* kWho = "nbc_jitter_workspace_bytes";
  if (!bytes) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (const char* why = bad_stack(N, V)) return fail(kWho, NBC_ERR_INVALID, why);
  *bytes = (size_t)V * N * sizeof(unsigned long long);
  return NBC_OK;
}

extern "C" int nbc_jitter_views(const uint8_t* x_dev, int N, int H, int W, const float* factors, int V, uint8_t* out_dev,
                                void* workspace_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_jitter_views";
  if (!x_dev || !factors || !out_dev || !workspace_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (const char* why = bad_stack(N, V)) return fail(kWho, NBC_ERR_INVALID, why);
  if (const char* why = bad_frame(H, W)) return fail(kWho, NBC_ERR_INVALID, why);
  for (int q = 0; q < 3 * V; ++q)
    if (!(factors[q] >= 0.f && factors[q] <= 4.f))
      return fail(kWho, NBC_ERR_INVALID, "factor " + std::to_string(q % 3) + " of view " + std::to_string(q / 3) +
                                             " must be finite and lie in [0, 4]");
  if (reinterpret_cast<uintptr_t>(workspace_dev) & 7u) return fail(kWho, NBC_ERR_INVALID, "workspace_dev must be 8-byte aligned");
  const long long P = (long long)H * W;
  const size_t bytes = (size_t)N * P * 3, ws_bytes = (size_t)V * N * sizeof(unsigned long long);
  if (ranges_overlap(x_dev, bytes, out_dev, bytes * V)) return fail(kWho, NBC_ERR_INVALID, "out_dev must not overlap x_dev");
  if (ranges_overlap(workspace_dev, ws_bytes, x_dev, bytes) || ranges_overlap(workspace_dev, ws_bytes, out_dev, bytes * V))
    return fail(kWho, NBC_ERR_INVALID, "workspace_dev must not overlap x_dev or out_dev");

  JitterArgs a;
  GreySumArgs g;
  int K = 0;                                      // the distinct b among the views with c != 1: views with the same b share a sum
  a.V = V;
  for (int j = 0; j < kMaxViews; ++j) {
    const bool live = j < V;
    a.b[j] = live ? factors[3 * j] : 1.f;
    a.c[j] = live ? factors[3 * j + 1] : 1.f;
    a.s[j] = live ? factors[3 * j + 2] : 1.f;
    a.slot[j] = 0;
    g.b[j] = 1.f;
  }
  for (int j = 0; j < V; ++j) {
    if (a.c[j] == 1.f) continue;
    int k = 0;
    while (k < K && g.b[k] != a.b[j]) ++k;
    if (k == K) g.b[K++] = a.b[j];
    a.slot[j] = k;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  auto* sums = static_cast<unsigned long long*>(workspace_dev);
  const long long units = P / kUnitPixels + 1;
  hipError_t e = hipSuccess;
  if (K > 0) {
    e = hipMemsetAsync(sums, 0, (size_t)K * N * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(jitter_grey_sum_kernel, dim3(slices_of(units, (long long)N * K), N, K), dim3(kThreads), 0, s, x_dev, N, P, g,
                         sums);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(jitter_apply_kernel, dim3(slices_of(units, N), N), dim3(kThreads), 0, s, x_dev, out_dev, N, P, a, sums);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

extern "C" int nbc_views_mean(const float* lowres_views_dev, int N, int V, int h, int w, float* mean_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_views_mean";
  if (!lowres_views_dev || !mean_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (const char* why = bad_stack(N, V)) return fail(kWho, NBC_ERR_INVALID, why);
  if (const char* why = bad_frame(h, w)) return fail(kWho, NBC_ERR_INVALID, why);
  if (!aligned4(lowres_views_dev, mean_dev)) return fail(kWho, NBC_ERR_INVALID, "float32 pointers must be 4-byte aligned");
  const size_t total = (size_t)N * 3 * h * w, bytes = total * sizeof(float);
  if (ranges_overlap(lowres_views_dev, bytes * V, mean_dev, bytes)) return fail(kWho, NBC_ERR_INVALID, "mean_dev must not overlap the input");
  hipLaunchKernelGGL(views_mean_kernel, dim3(grid_stride_blocks(total, kThreads, kBlocksPerCu)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(hip_stream), lowres_views_dev, (long long)total, V, mean_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
