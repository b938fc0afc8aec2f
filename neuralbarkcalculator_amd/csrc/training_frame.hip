// The training run's own frame (include/nbc.h: nbc_bilinear_taps, nbc_training_frame): pad_resize of
// utils.py:242-247 on a batch of equal-shape uint8 images, without a context.
//
//   nbc_bilinear_taps       host only: PIL's coefficient table of the bilinear filter for n + 1 -> n (precompute_coeffs, then
//                           normalize_coeffs_8bpc), in doubles in PIL's order, contraction off.
//   training_frame_kernel   one launch for the batch.  The output [N][Ht][Wt][C] is one run of bytes; a lane makes four
//                           consecutive ones and stores them as the dword they are (the at most three bytes before the first
//                           aligned dword and after the last go singly, so no store leaves the output at any alignment).  An
//                           output byte is a function of its own (image, row, column, channel) alone: per axis it has up to three
//                           taps (padded index -> source index by one reflection, 22-bit coefficient); an axis that is not
//                           resampled has the one tap 2^22, which the fixed-point rounding returns unchanged.  The horizontal
//                           sums are rounded to bytes before the vertical sum reads them, as PIL's two passes do; neither the
//                           padded image nor the intermediate one exists.  Reads: at most 3 x 3 source bytes per output byte,
//                           neighbours of those of the lanes beside it; about C H W bytes in and C Ht Wt out per image.
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"

using namespace nbc;

namespace {

constexpr int kBits = 22;                         // PIL's PRECISION_BITS for 8 bits per channel: 32 - 8 - 2
constexpr int kThreads = 256;
constexpr int kBlocksPerCu = 8;

// one axis: L source pixels, Lt framed ones, the pad p on both sides; taps: int32 [Lt][4] = {first, k0, k1, k2}, null where the
// padded length is Lt itself
struct FrameAxis {
  int L, Lt, p;
  const int32_t* taps;
};

// the taps of one output index: source indices and coefficients; an unused tap has k = 0 and is never read
struct Taps {
  int idx[NBC_FRAME_TAPS], k[NBC_FRAME_TAPS];
};

// padded index i -> source index, numpy.pad(mode="reflect"); the clamps hold a table that is not nbc_bilinear_taps' inside the image
__device__ __forceinline__ int source_index(const FrameAxis& a, int i) {
  const int lp = a.L + 2 * a.p;
  i = i < 0 ? 0 : (i >= lp ? lp - 1 : i);
  int j = i - a.p;
  j = j < 0 ? -j : j;
  j = j >= a.L ? 2 * (a.L - 1) - j : j;
  return j < 0 ? 0 : j;
}

__device__ __forceinline__ Taps axis_taps(const FrameAxis& a, int o) {
  Taps t;
  if (a.taps == nullptr) {
    t.idx[0] = source_index(a, o), t.k[0] = 1 << kBits;
#pragma unroll
    for (int q = 1; q < NBC_FRAME_TAPS; ++q) t.idx[q] = 0, t.k[q] = 0;
  } else {
    const int32_t* row = a.taps + 4 * (long long)o;
    const int first = row[0];
#pragma unroll
    for (int q = 0; q < NBC_FRAME_TAPS; ++q) t.idx[q] = source_index(a, first + q), t.k[q] = row[1 + q];
  }
  return t;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <int C>
__device__ __forceinline__ int frame_byte(const unsigned char* __restrict__ img, int W, const Taps& ty, const Taps& tx, int c) {
  int col = 1 << (kBits - 1);
#pragma unroll
  for (int a = 0; a < NBC_FRAME_TAPS; ++a) {
    if (ty.k[a] == 0) continue;
    const unsigned char* row = img + (long long)ty.idx[a] * W * C + c;
    int acc = 1 << (kBits - 1);
#pragma unroll
    for (int b = 0; b < NBC_FRAME_TAPS; ++b)
      if (tx.k[b] != 0) acc += (int)row[(long long)tx.idx[b] * C] * tx.k[b];
    col += clip8(acc) * ty.k[a];                  // the horizontal pass's byte
  }
  return clip8(col);
}

// where a byte of the output lies; step() moves to the next byte
struct Cursor {
  long long n;
  int y, x, c;
};

template <int C>
__device__ __forceinline__ Cursor cursor_at(long long q, int Ht, int Wt) {
  Cursor k;
  const long long pixel = q / C;
  k.c = (int)(q - pixel * C);
  const long long area = (long long)Ht * Wt;
  k.n = pixel / area;
  const int rem = (int)(pixel - k.n * area);
  k.y = rem / Wt;
  k.x = rem - k.y * Wt;
  return k;
}

// total = N Ht Wt C bytes of out; x holds N images of H W C bytes
template <int C>
__global__ __launch_bounds__(kThreads) void training_frame_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ out,
                                                                  long long total, int H, int W, FrameAxis ay, FrameAxis ax) {
  const int Ht = ay.Lt, Wt = ax.Lt;
  const long long image = (long long)H * W * C;
  long long head = (long long)((4u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 3u)) & 3u);
  if (head > total) head = total;
  const long long words = (total - head) / 4, body_end = head + 4 * words;
  const long long stride = (long long)gridDim.x * kThreads;
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;

  for (long long i = g; i < words; i += stride) {
    const long long q = head + 4 * i;             // q + 4 <= total
    Cursor k = cursor_at<C>(q, Ht, Wt);
    Taps ty = axis_taps(ay, k.y), tx = axis_taps(ax, k.x);
    uint32_t word = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      word |= (uint32_t)frame_byte<C>(x + k.n * image, W, ty, tx, k.c) << (8 * e);
      if (e == 3) break;
      if (++k.c == C) {                           // the next byte: the next pixel, row or image
        k.c = 0;
        if (++k.x == Wt) {
          k.x = 0;
          if (++k.y == Ht) k.y = 0, ++k.n;
          ty = axis_taps(ay, k.y);
        }
        tx = axis_taps(ax, k.x);
      }
    }
    *reinterpret_cast<uint32_t*>(out + q) = word;
  }
  // the at most 3 + 3 bytes outside the aligned dwords
  const long long edge = head + (total - body_end);
  if (g < edge) {
    const long long q = g < head ? g : body_end + (g - head);
    const Cursor k = cursor_at<C>(q, Ht, Wt);
    out[q] = (unsigned char)frame_byte<C>(x + k.n * image, W, axis_taps(ay, k.y), axis_taps(ax, k.x), k.c);
  }
}

// the pad of an axis, or what the call refuses of it (why != nullptr)
int axis_pad(int L, int Lt, const char** why) {
  *why = nullptr;
  if (L < 1 || Lt < 1) {
    *why = "bad shape: H, W, Ht, Wt >= 1";
    return 0;
  }
  if (L > Lt) {
    *why = "the source exceeds the frame: H <= Ht and W <= Wt (pad_resize would shrink: left out)";
    return 0;
  }
  const int p = (Lt - L + 1) / 2;
  if (p > L - 1) *why = "the pad needs more than one reflection: ceil((Lt - L) / 2) <= L - 1 on both axes";
  return p;
}

}  // namespace

#pragma clang fp contract(off)
extern "C" int nbc_bilinear_taps(int in_size, int out_size, int32_t* first, int32_t* coeff) {
  constexpr const char* kWho = "nbc_bilinear_taps";
  if (!first || !coeff) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (out_size < 1 || out_size > 0x3fffffff || in_size != out_size + 1)
    return fail(kWho, NBC_ERR_INVALID, "in_size must be out_size + 1 with out_size >= 1: all that pad_resize can produce");
  // Resample.c, precompute_coeffs with the bilinear filter (support 1.0) and the box (0, in_size)
  const double scale = (double)in_size / (double)out_size;   // > 1, so filterscale = scale
  const double support = 1.0 * scale;
  const double ss = 1.0 / scale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > NBC_FRAME_TAPS) return fail(kWho, NBC_ERR_INVALID, "more than NBC_FRAME_TAPS taps");   // 2 * support < 3: never
    double k[NBC_FRAME_TAPS] = {0.0, 0.0, 0.0};
    for (int x = 0; x < xmax; ++x) {
      double v = (x + xmin - center + 0.5) * ss;
      if (v < 0.0) v = -v;
      const double w = v < 1.0 ? 1.0 - v : 0.0;
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    // normalize_coeffs_8bpc
    for (int x = 0; x < NBC_FRAME_TAPS; ++x)
      coeff[(size_t)xx * NBC_FRAME_TAPS + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kBits)) : (int)(0.5 + k[x] * (1 << kBits));
    first[xx] = xmin;
  }
  return NBC_OK;
}

extern "C" int nbc_training_frame(const void* x_dev, int channels, int N, int H, int W, int Ht, int Wt, const int32_t* row_taps_dev,
                                  const int32_t* col_taps_dev, void* out_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_training_frame";
  if (!x_dev || !out_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (channels != 1 && channels != 3) return fail(kWho, NBC_ERR_INVALID, "channels must be 1 or 3");
  if (N < 1 || N > 65535) return fail(kWho, NBC_ERR_INVALID, "bad shape: 1 <= N <= 65535");
  const char* why = nullptr;
  const int py = axis_pad(H, Ht, &why);
  if (why) return fail(kWho, NBC_ERR_INVALID, why);
  const int px = axis_pad(W, Wt, &why);
  if (why) return fail(kWho, NBC_ERR_INVALID, why);
  if (!frame_shape_ok(Ht, Wt)) return fail(kWho, NBC_ERR_INVALID, "bad shape: Ht * Wt < 2^31");
  const bool rows = H + 2 * py != Ht, cols = W + 2 * px != Wt;   // the padded length is one too long
  if ((rows && !row_taps_dev) || (cols && !col_taps_dev))
    return fail(kWho, NBC_ERR_INVALID, "an axis whose padded length is the frame's + 1 needs its table (nbc_bilinear_taps)");
  if (!aligned4(row_taps_dev, col_taps_dev)) return fail(kWho, NBC_ERR_INVALID, "the tables must be 4-byte aligned");
  const size_t in_bytes = (size_t)N * H * W * channels, out_bytes = (size_t)N * Ht * Wt * channels;
  if (ranges_overlap(x_dev, in_bytes, out_dev, out_bytes)) return fail(kWho, NBC_ERR_INVALID, "out_dev must not overlap x_dev");

  const FrameAxis ay{H, Ht, py, rows ? row_taps_dev : nullptr}, ax{W, Wt, px, cols ? col_taps_dev : nullptr};
  const dim3 grid(grid_stride_blocks(out_bytes / 4 + 8, kThreads, kBlocksPerCu));
  const hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const unsigned char* x = static_cast<const unsigned char*>(x_dev);
  unsigned char* out = static_cast<unsigned char*>(out_dev);
  if (channels == 3)
    hipLaunchKernelGGL((training_frame_kernel<3>), grid, dim3(kThreads), 0, s, x, out, (long long)out_bytes, H, W, ay, ax);
  else
    hipLaunchKernelGGL((training_frame_kernel<1>), grid, dim3(kThreads), 0, s, x, out, (long long)out_bytes, H, W, ay, ax);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
