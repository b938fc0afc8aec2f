// Kernels of the EfficientNet networks (NBC_ARCH_*_EFFICIENTNET_B*, fp32 only) that are not convolutions on the conv kernel.
// Every tensor is NHWC f32 with C a multiple of 64 (zero pad channels); the 1x1 and dense convolutions run on conv_dma.
//
//   dwconv: the depthwise k x k convolution (k 3 / 5, stride 1 / 2) of an MBConv block with explicit top / left pads and
//     output size (TF "same" pads are asymmetric: a tap outside the image reads 0, checked per image), the BatchNorm's
//     (scale, shift) and swish in the epilogue, and the SE squeeze's first level: per (image, tile, channel) the sum of
//     the tile's outputs.  A block owns TH x 16 output pixels x 32 channels of one image (TH = 8 at stride 1, 4 at
//     stride 2); it stages the input window ((TH-1) s + k rows x (15 s + k) columns x 32 channels, 13.8-48 KiB) in LDS
//     once, applying the swish its producer deferred (stem / expand output), and a thread computes one channel of TH * 2
//     pixels from it.  The tiles depend on the map size only, never on N.
//   se_excite: one block per image: the SE squeeze's second level (the tiles' sums in tile order / (Ho * Wo)), _se_reduce
//     + bias, swish, _se_expand + bias, sigmoid -> gate [N][C].
//   gate_weights: the gate folded into the project conv's weights, per image: Wg[n][o][c] = W[o][c] * gate[n][c]; the
//     project conv then runs once per image on them (no pass over the gated activation).
//   swish: in place (the head conv's output).
//   head1x1: classifier.4 for any cin (a multiple of 64): FCNHead's inplanes / 4 channels, padded.  Its chain is its own
//     (lane-strided channel order); the tree, the store, the flag and the counter clearing are head1x1.hpp's.
// (DeepLabHead's pooling branch is aspp.hip's, for every trunk.)
#include "head1x1.hpp"
#include "nbc_kernels.hpp"
#include "reduce.hpp"

namespace nbc {
namespace {

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float swish_f(float x) { return x * sigmoid_f(x); }

constexpr int kDwTw = 16;        // output columns per block
constexpr int kDwCb = 32;        // channels per block: one 128-byte row segment per pixel
constexpr int kDwThreads = 256;  // 32 channels x 8 pixel groups
template <int S> constexpr int dw_th() { return S == 1 ? 8 : 4; }

template <int K, int S>
__global__ __launch_bounds__(kDwThreads) void dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            float* __restrict__ y, float* __restrict__ partial, int Hi, int Wi,
                                                            int C, int Ho, int Wo, int pad_t, int pad_l, int in_swish) {
  constexpr int TH = dw_th<S>();
  constexpr int IH = (TH - 1) * S + K, IW = (kDwTw - 1) * S + K;
  constexpr int PPT = TH * kDwTw / 8;            // pixels per thread
  __shared__ float tile[IH * IW * kDwCb];
  __shared__ float red[8][kDwCb];
  const int cblocks = C / kDwCb;
  const int img = blockIdx.z / cblocks, c0 = (blockIdx.z - img * cblocks) * kDwCb;
  const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * kDwTw;
  const int iy0 = oy0 * S - pad_t, ix0 = ox0 * S - pad_l;
  const float* xi = x + (size_t)img * Hi * Wi * C + c0;
  for (int i = threadIdx.x; i < IH * IW * kDwCb; i += kDwThreads) {
    const int c = i % kDwCb, p = i / kDwCb;
    const int iy = iy0 + p / IW, ix = ix0 + p % IW;
    float v = 0.f;                               // outside the image: the zero pad (swish(0) = 0 either way)
    if ((unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi) {
      v = xi[((size_t)iy * Wi + ix) * C + c];
      if (in_swish) v = swish_f(v);
    }
    tile[i] = v;
  }
  const int c = threadIdx.x % kDwCb, g = threadIdx.x / kDwCb;
  float wr[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) wr[t] = w[(size_t)t * C + c0 + c];
  const float sc = scale[c0 + c], sh = shift[c0 + c];
  __syncthreads();
  float* yi = y + (size_t)img * Ho * Wo * C + c0 + c;
  float sum = 0.f;
#pragma unroll 2
  for (int q = 0; q < PPT; ++q) {
    const int p = g * PPT + q;
    const int ry = p / kDwTw, rx = p % kDwTw;
    float acc = 0.f;
#pragma unroll
    for (int kh = 0; kh < K; ++kh)
#pragma unroll
      for (int kw = 0; kw < K; ++kw) acc = __builtin_fmaf(tile[((ry * S + kh) * IW + rx * S + kw) * kDwCb + c], wr[kh * K + kw], acc);
    const int oy = oy0 + ry, ox = ox0 + rx;
    if (oy < Ho && ox < Wo) {
      const float v = swish_f(__builtin_fmaf(acc, sc, sh));
      yi[((size_t)oy * Wo + ox) * C] = v;
      sum += v;
    }
  }
  red[g][c] = sum;
  __syncthreads();
  if (g == 0) {
    float s = red[0][c];
#pragma unroll
    for (int j = 1; j < 8; ++j) s += red[j][c];
    const int tiles = gridDim.x * gridDim.y, t = blockIdx.y * gridDim.x + blockIdx.x;
    partial[((size_t)img * tiles + t) * C + c0 + c] = s;
  }
}

// one block of 256 threads per image; dynamic LDS: mean [C] + reduced [cse]
__global__ __launch_bounds__(256) void se_excite_kernel(const float* __restrict__ partial, int tiles, int C, float inv_hw,
                                                        const float* __restrict__ wr, const float* __restrict__ br, int cse,
                                                        const float* __restrict__ we, const float* __restrict__ be,
                                                        float* __restrict__ gate) {
  extern __shared__ float sm[];
  float* mean = sm;
  float* red = sm + C;
  __shared__ float part[4][64];
  const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* pi = partial + (size_t)img * tiles * C;
  // second level of the squeeze: wave w sums the tiles [w T / 4, (w + 1) T / 4) in order, then the four in order
  const int t0 = wave * tiles / 4, t1 = (wave + 1) * tiles / 4;
  for (int c0 = 0; c0 < C; c0 += 64) {
    float s = 0.f;
    for (int t = t0; t < t1; ++t) s += pi[(size_t)t * C + c0 + lane];
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) mean[c0 + lane] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) * inv_hw;
    __syncthreads();
  }
  // _se_reduce + bias, swish: one wave per output, lanes over the channels, a 64-lane tree
  for (int j = wave; j < cse; j += 4) {
    const float* row = wr + (size_t)j * C;
    float acc = 0.f;
    for (int i = lane; i < C; i += 64) acc = __builtin_fmaf(row[i], mean[i], acc);
    acc = wave_sum(acc);
    if (lane == 0) red[j] = swish_f(acc + br[j]);
  }
  __syncthreads();
  // _se_expand + bias, sigmoid: one thread per channel
  for (int c = threadIdx.x; c < C; c += 256) {
    const float* row = we + (size_t)c * cse;
    float acc = 0.f;
    for (int j = 0; j < cse; ++j) acc = __builtin_fmaf(row[j], red[j], acc);
    gate[(size_t)img * C + c] = sigmoid_f(acc + be[c]);
  }
}

// Wg[n][o][c] = W[o][c] * gate[n][c], float4 at a time (Ci a multiple of 64)
__global__ __launch_bounds__(256) void gate_weights_kernel(const float4* __restrict__ w, const float* __restrict__ gate,
                                                           float4* __restrict__ wg, int Co, int Ci, int N) {
  const int ci4 = Ci / 4;
  const size_t per = (size_t)Co * ci4, total = per * N;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int n = (int)(i / per);
    const size_t r = i - (size_t)n * per;
    const int c = (int)(r % ci4) * 4;
    const float4 v = w[r];
    const float* g = gate + (size_t)n * Ci + c;
    wg[i] = make_float4(v.x * g[0], v.y * g[1], v.z * g[2], v.w * g[3]);
  }
}

__global__ __launch_bounds__(256) void swish_kernel(float4* __restrict__ y, size_t n4) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = y[i];
    y[i] = make_float4(swish_f(v.x), swish_f(v.y), swish_f(v.z), swish_f(v.w));
  }
}

// classifier.4 for cin a multiple of 64: one wave per pixel, lane l sums channels l, l + 64, ... in order, a 64-lane tree
__global__ __launch_bounds__(256) void head1x1_any_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, int M, int hw,
                                                          int C, unsigned long long* __restrict__ counts_zero, int ncounts,
                                                          unsigned* __restrict__ nonfinite) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  head_clear_counts(counts_zero, ncounts);
  if (m >= M) return;
  const float* xp = x + (size_t)m * C;
  float s[3] = {0.f, 0.f, 0.f};
  for (int i = lane; i < C; i += 64) {
    const float v = xp[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = __builtin_fmaf(v, w[c * C + i], s[c]);
  }
  head_tree<64>(s);
  if (lane != 0) return;
  const int img = m / hw, pix = m - img * hw;
  const float b[3] = {bias[0], bias[1], bias[2]};
  if (!head_store(s, b, y + (size_t)img * 3 * hw + pix, hw)) head_raise(nonfinite);
}

constexpr int kBlocksPerCu = 16;   // of this file's grid-stride kernels

template <int K, int S>
void launch_dw(const DwArgs& a, hipStream_t s) {
  const dim3 grid(dwconv_tiles_x(a.Wo), (a.Ho + dw_th<S>() - 1) / dw_th<S>(), a.N * (a.C / kDwCb));
  hipLaunchKernelGGL((dwconv_kernel<K, S>), grid, dim3(kDwThreads), 0, s, a.x, a.w, a.scale, a.shift, a.y, a.partial, a.Hi, a.Wi, a.C,
                     a.Ho, a.Wo, a.pad_t, a.pad_l, a.in_swish);
}

}  // namespace

int dwconv_tiles_x(int Wo) { return (Wo + kDwTw - 1) / kDwTw; }
int dwconv_tiles(int stride, int Ho, int Wo) {
  const int th = stride == 1 ? dw_th<1>() : dw_th<2>();
  return dwconv_tiles_x(Wo) * ((Ho + th - 1) / th);
}

hipError_t launch_dwconv(const DwArgs& a, hipStream_t s) {
  if (a.N < 1 || a.C % 64 != 0 || a.Ho < 1 || a.Wo < 1 || (size_t)a.N * (a.C / kDwCb) > 65535 || (a.Ho + 3) / 4 > 65535)
    return hipErrorInvalidValue;
  if (a.k == 3 && a.stride == 1) launch_dw<3, 1>(a, s);
  else if (a.k == 3 && a.stride == 2) launch_dw<3, 2>(a, s);
  else if (a.k == 5 && a.stride == 1) launch_dw<5, 1>(a, s);
  else if (a.k == 5 && a.stride == 2) launch_dw<5, 2>(a, s);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_se_excite(const float* partial, int N, int tiles, int C, int hw, const float* wr, const float* br, int cse,
                            const float* we, const float* be, float* gate, hipStream_t s) {
  if (N < 1 || C % 64 != 0 || tiles < 1 || cse < 1 || hw < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)(C + cse) * sizeof(float);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(se_excite_kernel, dim3(N), dim3(256), lds, s, partial, tiles, C, 1.0f / (float)hw, wr, br, cse, we, be, gate);
  return hipGetLastError();
}

hipError_t launch_gate_weights(const float* w, const float* gate, float* wg, int N, int Co, int Ci, hipStream_t s) {
  if (N < 1 || Co < 1 || Ci % 64 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gate_weights_kernel, dim3(grid_stride_blocks((size_t)N * Co * Ci / 4, 256, kBlocksPerCu)), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(w), gate, reinterpret_cast<float4*>(wg), Co, Ci, N);
  return hipGetLastError();
}

hipError_t launch_swish(float* y, size_t elems, hipStream_t s) {
  if (elems % 4 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swish_kernel, dim3(grid_stride_blocks(elems / 4, 256, kBlocksPerCu)), dim3(256), 0, s, reinterpret_cast<float4*>(y), elems / 4);
  return hipGetLastError();
}

hipError_t launch_head1x1_any(const float* x, const float* w, const float* bias, float* y, int N, int hw, int cin,
                              unsigned long long* counts_zero, unsigned* nonfinite, hipStream_t s) {
  if (cin % 64 != 0 || N < 1 || hw < 1) return hipErrorInvalidValue;
  if (!head_clears_counts(N)) counts_zero = nullptr;      // the caller then clears the counters itself
  const int M = N * hw;
  hipLaunchKernelGGL(head1x1_any_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, w, bias, y, M, hw, cin, counts_zero, 3 * N, nonfinite);
  return hipGetLastError();
}

}  // namespace nbc
