// The two ASPP operations of DeepLabHead (models.py:46-57, torchvision 0.3) that are not convolutions on the conv kernel:
//
//   aspp_pool: the pooling branch, per image, of every DeepLab head.  AdaptiveAvgPool2d(1) of the trunk's output (cin channels,
//     a multiple of 64 up to 4096: 2048 behind ResNet-50, 1280 .. 2560 behind the EfficientNets; h x w pixels), the 1x1 conv
//     cin -> 256 in f32 with the f32 weights of the blob, BatchNorm (the folded f32 scale / shift) and ReLU, written as ONE
//     pixel of 256 channels in the storage form of the concat.  Three launches:
//       (1) partial sums: grid (kPoolSlices, N), a thread owns eight channels (and those 2048 further on) and sums its slice's
//           pixels in order (a chain of ceil(hw / kPoolSlices) values, at most 64 at 1024^2) -- the byte mover, it reads the
//           trunk's output once;
//       (2) finish: one thread per (image, channel) sums the slices' partials in order (the second level) and divides by hw;
//       (3) the 1x1 conv: one wave per output channel, lane l the products of channels l, l + 64, ... in order, a 64-lane
//           tree, then BN, ReLU and the store.
//     Slices depend on hw only, never on N, so an image of a batch gives the bits it gives alone.
//   concat: the [M][1280] projection input, channels 0-1023 from the four spatial branches and 1024-1279 the image's pooled
//     vector broadcast over its pixels.  256 channels are a whole number of 16-byte chunks in every storage form (f16x2:
//     eight 128-byte groups of [h0 x 32][h1 x 32]), so this is a pure 16-byte copy.
//
// Bounds: (1) reads N * hw * cin elements and writes N * kPoolSlices * cin floats; (2) reads those; (3) reads cout * cin * 4
// bytes of weights per image (L2-resident after the first image); concat reads 5/4 x M x 256 x 4 elements' bytes and writes the same.
#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "stored.hpp"

namespace nbc {
namespace {

constexpr int kPoolMaxCin = 4096;
constexpr int kPoolThreads = 256;               // a thread owns eight channels of every pixel, 2048 per round of the block
constexpr int kPoolSlices = 256;                // pixel slices per image (fewer when hw is smaller)

// (1) grid (slices, N), 256 threads: partial[img][slice][c] = sum over the slice's pixels, in pixel order
template <int PREC>
__global__ __launch_bounds__(kPoolThreads) void aspp_pool_partial_kernel(const void* __restrict__ x, float* __restrict__ partial,
                                                                         int hw, int cin, int slices) {
  const int slice = blockIdx.x, img = blockIdx.y;
  const int p0 = (int)(((long long)hw * slice) / slices), p1 = (int)(((long long)hw * (slice + 1)) / slices);
  const size_t base = (size_t)img * hw;
  for (int c8 = threadIdx.x * 8; c8 < cin; c8 += kPoolThreads * 8) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int p = p0;
    for (; p + 4 <= p1; p += 4) {               // four pixels' loads in flight, summed in pixel order
      float f[4][8];
#pragma unroll
      for (int q = 0; q < 4; ++q) read8<PREC>(x, base + p + q, cin, c8, f[q]);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += f[q][e];
    }
    for (; p < p1; ++p) {
      float f[8];
      read8<PREC>(x, base + p, cin, c8, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += f[e];
    }
    float4* o = reinterpret_cast<float4*>(partial + ((size_t)img * slices + slice) * cin + c8);
    o[0] = make_float4(s[0], s[1], s[2], s[3]);
    o[1] = make_float4(s[4], s[5], s[6], s[7]);
  }
}

// (2) grid (ceil(cin / 256), N): mean[img][c] = (sum over slices of partial, in slice order) / hw
__global__ __launch_bounds__(256) void aspp_pool_finish_kernel(const float* __restrict__ partial, float* __restrict__ mean, int hw,
                                                               int cin, int slices) {
  const int c = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  if (c >= cin) return;
  const float* p = partial + (size_t)img * slices * cin + c;
  float s = 0.f;
  for (int k = 0; k < slices; ++k) s += p[(size_t)k * cin];
  mean[(size_t)img * cin + c] = s / (float)hw;
}

// (3) grid (cout / 4, N), four waves, one output channel each: y = relu(fma(w . mean, scale, shift)) in the stored form.
// Dynamic LDS: the image's mean, cin floats.
template <int PREC>
__global__ __launch_bounds__(256) void aspp_pool_conv_kernel(const float* __restrict__ mean, const float* __restrict__ w,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             void* __restrict__ y, int cin, int cout) {
  extern __shared__ float m[];
  const int img = blockIdx.y;
  for (int i = threadIdx.x; i < cin; i += 256) m[i] = mean[(size_t)img * cin + i];
  __syncthreads();
  const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const float* wr = w + (size_t)o * cin;
  float acc = 0.f;
#pragma unroll 8
  for (int i = lane; i < cin; i += 64) acc = __builtin_fmaf(wr[i], m[i], acc);
  acc = wave_sum(acc);
  if (lane != 0) return;
  const float v = __builtin_fmaxf(__builtin_fmaf(acc, scale[o], shift[o]), 0.f);
  store_elem<PREC>(y, (size_t)img * cout + o, img, cout, o, v);
}

struct ConcatSrc {
  const uint4* branch[4];   // [M][256] elements each
  const uint4* pooled;      // [N][256] elements
};

// grid-stride over the 16-byte chunks of the [M][1280] output; CPB = chunks of one 256-channel branch per pixel
template <int CPB>
__global__ __launch_bounds__(256) void aspp_concat_kernel(ConcatSrc src, uint4* __restrict__ y, int M, int hw) {
  constexpr int CPR = 5 * CPB;                  // chunks per output pixel
  const size_t total = (size_t)M * CPR;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int m = (int)(i / CPR), j = (int)(i - (size_t)m * CPR);
    const int b = j / CPB, jj = j - b * CPB;
    uint4 v;
    if (b < 4) v = src.branch[b][(size_t)m * CPB + jj];
    else v = src.pooled[(size_t)(m / hw) * CPB + jj];
    y[i] = v;
  }
}

}  // namespace

int aspp_pool_slices(int hw) { return hw < kPoolSlices ? hw : kPoolSlices; }

hipError_t launch_aspp_pool(const void* x, int N, int hw, int cin, const float* w, const float* scale, const float* shift, int cout,
                            float* partial, float* mean, void* y, int precision, hipStream_t s) {
  if (cin < 64 || cin % 64 != 0 || cin > kPoolMaxCin || cout % 4 != 0 || N < 1 || N > 65535 || hw < 1) return hipErrorInvalidValue;
  const int slices = aspp_pool_slices(hw);
  const dim3 g1(slices, N), g2((cin + 255) / 256, N), g3(cout / 4, N);
  with_precision(precision, [&](auto P) {
    hipLaunchKernelGGL(aspp_pool_partial_kernel<P.value>, g1, dim3(kPoolThreads), 0, s, x, partial, hw, cin, slices);
    hipLaunchKernelGGL(aspp_pool_finish_kernel, g2, dim3(256), 0, s, partial, mean, hw, cin, slices);
    hipLaunchKernelGGL(aspp_pool_conv_kernel<P.value>, g3, dim3(256), (size_t)cin * sizeof(float), s, mean, w, scale, shift, y, cin, cout);
  });
  return hipGetLastError();
}

hipError_t launch_aspp_concat(const void* const branch[4], const void* pooled, void* y, int N, int hw, int precision,
                              hipStream_t s) {
  if (N < 1 || hw < 1) return hipErrorInvalidValue;
  ConcatSrc src;
  for (int b = 0; b < 4; ++b) src.branch[b] = static_cast<const uint4*>(branch[b]);
  src.pooled = static_cast<const uint4*>(pooled);
  const int M = N * hw;
  const int cpb = 256 * (precision == 1 ? 2 : 4) / 16;
  const dim3 blocks(grid_stride_blocks((size_t)M * 5 * cpb, 256, 16));
  if (cpb == 64) hipLaunchKernelGGL(aspp_concat_kernel<64>, blocks, dim3(256), 0, s, src, static_cast<uint4*>(y), M, hw);
  else hipLaunchKernelGGL(aspp_concat_kernel<32>, blocks, dim3(256), 0, s, src, static_cast<uint4*>(y), M, hw);
  return hipGetLastError();
}

}  // namespace nbc
