// The refit of classifier.4 (models.py:121) on the device: the gradient of the pixel-wise cross-entropy family with respect to
// the 1 539 parameters of the 1x1 convolution 512 -> 3, through the bicubic upsample.  The definitions are in include/nbc.h
// (nbc_head_logits, nbc_bicubic_taps, nbc_ce_gradient, nbc_head_gradient) and DESIGN.md 3.22; the host restatement is
// neuralbarkcalculator_amd/refit.py.
//
//   head_theta_scale    the caller's theta in state_dict units -> what the forward's classifier.4 launch reads: the weights
//                       times 2^-a (the power of two the stored input carries in f16x2; exact), the bias as it is.  The trial
//                       logits are then launch_head1x1 itself (pointwise.hip) on that array: the forward's machine code.
//   ce_pixel_gradient   one thread per group of four consecutive pixels: g_c = T[t][p] (softmax_c - [c = t]) in f64 from the f32
//                       logits, written as three f64 planes per image.  A group whose logit planes are 16-byte aligned (and its
//                       target bytes 4-byte aligned) and that lies whole inside the image comes in by three 16-byte loads and
//                       one 4-byte load, as in pixel_ce.hip; the planes of g start on 16-byte boundaries (an even plane stride),
//                       so a whole group goes out by 16-byte stores either way.  How a pixel was loaded reaches nothing.
//   ce_col_adjoint      [3,H,W] -> [3,H,w]: one thread per (row Y, low-resolution column j) and image, the three classes together;
//                       it walks the outputs lo[j] .. hi[j] of its column in ascending order and, per output, the four taps
//                       in tap order, adding (double)cx * g for each tap that lands on j.
//   ce_row_adjoint      [3,H,w] -> [3,h,w]: the same down the rows.
//   head_grad_partial   one block per 64 consecutive cells and image, a wave per 16 of them: lane l owns channels 8l .. 8l+7 as
//                       the head does (load8 / decode8 of stored.hpp), adds g_c * (double)X in cell order into 24 f64
//                       accumulators (and the three plain sums of g for the bias), then the four waves in wave order through
//                       LDS: one partial [3][513] per block.
//   head_grad_finish    one thread per (image, class, column): the blocks' partials in block order, then the 2^-a.
// Every sum's order is fixed by (H, W, h, w) alone and nothing is added atomically: an image's numbers are bit-identical alone,
// anywhere in a batch and on any stream.  The tap tables come from the host (nbc_bicubic_taps below, evaluated without fused
// multiply-adds), so that the host restatement differs from the device by summation order only.
// No library besides the HIP runtime.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ce_gradient.hpp"
#include "nbc_ctx.hpp"
#include "nbc_kernels.hpp"
#include "reduce.hpp"
#include "stored.hpp"

namespace nbc {
namespace {

constexpr int kClasses = 3;
constexpr int kCin = 512;
constexpr int kRow = kCin + 1;                          // a class's row of d theta: 512 weights, then the bias
constexpr int kThreads = 256;
constexpr int kGroup = 4;                               // consecutive pixels per thread of ce_pixel_gradient
constexpr int kCellsPerWave = 16;                       // head_grad_partial: two rounds of eight loads in flight
constexpr int kCellsPerBlock = 4 * kCellsPerWave;       // a block of head_grad_partial owns 64 consecutive cells
constexpr int kHeadThetaFloats = kClasses * kRow;       // theta: f32 [3][512] in state_dict units, then the [3] of the bias
inline int head_grad_blocks(int hw) { return (hw + kCellsPerBlock - 1) / kCellsPerBlock; }

using u32 = unsigned;

__global__ __launch_bounds__(kThreads) void head_theta_scale(const float* __restrict__ theta, float* __restrict__ out, int neg_a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < kHeadThetaFloats) out[i] = i < kClasses * kCin ? ldexpf(theta[i], neg_a) : theta[i];
}

// g_c = T[t][p] (q_c - [c = t]) of one pixel (ce_gradient.hpp), q = softmax in f64 from the f32 logits
__device__ __forceinline__ void pixel_gradient(float a, float b, float c, u32 grey, const CeTable& T, double (&g)[3]) {
  double q[3];
  pixel_softmax(a, b, c, q);
  pixel_gradient(a, b, c, grey, T, q, g);
}

// grid = (ceil(P / 1024), N); gw: f64 [N][3][Pp], Pp = P rounded up to even
__global__ __launch_bounds__(kThreads) void ce_pixel_gradient(const float* __restrict__ logits, const unsigned char* __restrict__ target,
                                                              long long P, long long Pp, CeTable T, double* __restrict__ gw) {
  const int n = blockIdx.y;
  const float* l0 = logits + (size_t)n * kClasses * P;
  const float* l1 = l0 + P;
  const float* l2 = l1 + P;
  const unsigned char* tg = target + (size_t)n * P;
  double* g0 = gw + (size_t)n * kClasses * Pp;
  double* g1 = g0 + Pp;
  double* g2 = g1 + Pp;
  const bool vec = ((reinterpret_cast<uintptr_t>(l0) | reinterpret_cast<uintptr_t>(l1) | reinterpret_cast<uintptr_t>(l2)) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(tg) & 3u) == 0;
  const long long q = ((long long)blockIdx.x * kThreads + threadIdx.x) * kGroup;
  if (q >= P) return;
  if (q + kGroup <= P) {
    float4 a, b, c;
    u32 t;
    if (vec) {
      a = *reinterpret_cast<const float4*>(l0 + q);
      b = *reinterpret_cast<const float4*>(l1 + q);
      c = *reinterpret_cast<const float4*>(l2 + q);
      t = *reinterpret_cast<const u32*>(tg + q);
    } else {
      a = make_float4(l0[q], l0[q + 1], l0[q + 2], l0[q + 3]);
      b = make_float4(l1[q], l1[q + 1], l1[q + 2], l1[q + 3]);
      c = make_float4(l2[q], l2[q + 1], l2[q + 2], l2[q + 3]);
      t = (u32)tg[q] | ((u32)tg[q + 1] << 8) | ((u32)tg[q + 2] << 16) | ((u32)tg[q + 3] << 24);
    }
    double p0[3], p1[3], p2[3], p3[3];
    pixel_gradient(a.x, b.x, c.x, t & 255u, T, p0);
    pixel_gradient(a.y, b.y, c.y, (t >> 8) & 255u, T, p1);
    pixel_gradient(a.z, b.z, c.z, (t >> 16) & 255u, T, p2);
    pixel_gradient(a.w, b.w, c.w, t >> 24, T, p3);
    double* const planes[3] = {g0, g1, g2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {                       // q is a multiple of 4 and the planes start on 16 bytes
      double2* o = reinterpret_cast<double2*>(planes[k] + q);
      o[0] = make_double2(p0[k], p1[k]);
      o[1] = make_double2(p2[k], p3[k]);
    }
  } else {
    for (long long k = q; k < P; ++k) {
      double p[3];
      pixel_gradient(l0[k], l1[k], l2[k], tg[k], T, p);
      g0[k] = p[0];
      g1[k] = p[1];
      g2[k] = p[2];
    }
  }
}

// out [n][c][r][j] = sum over the outputs o = lo[j] .. hi[j] (ascending) and the taps b = 0 .. 3 (ascending) with idx[o][b] == j
// of (double)coeff[o][b] * in[n][c][r][o]: the adjoint of the filter along the last axis.  in: `rows` rows of `len` values with
// plane stride in_plane; out: rows of `cells` values, planes rows * cells apart.  grid = (ceil(rows * cells / 256), N).
__global__ __launch_bounds__(kThreads) void ce_col_adjoint(const double* __restrict__ in, long long in_plane, int rows, int len, int cells,
                                                           const int4* __restrict__ idx, const float4* __restrict__ coeff,
                                                           const int* __restrict__ lo, const int* __restrict__ hi,
                                                           double* __restrict__ out) {
  const long long at = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (at >= (long long)rows * cells) return;
  const int n = blockIdx.y;
  const int r = (int)(at / cells), j = (int)(at - (long long)r * cells);
  const double* p0 = in + (size_t)n * kClasses * in_plane + (size_t)r * len;
  const double* p1 = p0 + in_plane;
  const double* p2 = p1 + in_plane;
  const int first = max(lo[j], 0), last = min(hi[j], len - 1);   // whatever the table holds, the reads stay inside the row
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
  for (int o = first; o <= last; ++o) {          // several outputs' loads in flight; the adds stay in order
    const int4 t = idx[o];
    const float4 c = coeff[o];
    const double v0 = p0[o], v1 = p1[o], v2 = p2[o];
    const int ti[4] = {t.x, t.y, t.z, t.w};
    const float ci[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (ti[b] == j) {
        const double k = (double)ci[b];
        acc[0] += k * v0;
        acc[1] += k * v1;
        acc[2] += k * v2;
      }
  }
  const size_t plane = (size_t)rows * cells;
  double* o = out + (size_t)n * kClasses * plane + (size_t)at;
  o[0] = acc[0];
  o[plane] = acc[1];
  o[2 * plane] = acc[2];
}

// out [n][c][i][j] = sum over the rows Y = lo[i] .. hi[i] (ascending) and the taps a (ascending) with idx[Y][a] == i of
// (double)coeff[Y][a] * in[n][c][Y][j]: the adjoint down the rows of [3][H][w] planes.  grid = (ceil(h * w / 256), N).
__global__ __launch_bounds__(kThreads) void ce_row_adjoint(const double* __restrict__ in, int H, int w, int h,
                                                           const int4* __restrict__ idx, const float4* __restrict__ coeff,
                                                           const int* __restrict__ lo, const int* __restrict__ hi,
                                                           double* __restrict__ out) {
  const long long at = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (at >= (long long)h * w) return;
  const int n = blockIdx.y;
  const int i = (int)(at / w), j = (int)(at - (long long)i * w);
  const size_t in_plane = (size_t)H * w;
  const double* p0 = in + (size_t)n * kClasses * in_plane + j;
  const int first = max(lo[i], 0), last = min(hi[i], H - 1);
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
  for (int Y = first; Y <= last; ++Y) {
    const int4 t = idx[Y];
    const float4 c = coeff[Y];
    const double* p = p0 + (size_t)Y * w;
    const double v0 = p[0], v1 = p[in_plane], v2 = p[2 * in_plane];
    const int ti[4] = {t.x, t.y, t.z, t.w};
    const float ci[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (ti[a] == i) {
        const double k = (double)ci[a];
        acc[0] += k * v0;
        acc[1] += k * v1;
        acc[2] += k * v2;
      }
  }
  const size_t plane = (size_t)h * w;
  double* o = out + (size_t)n * kClasses * plane + (size_t)at;
  o[0] = acc[0];
  o[plane] = acc[1];
  o[2 * plane] = acc[2];
}

// grid = (head_grad_blocks(hw), N); part: f64 [N][blocks][3][513]
template <int PREC>
__global__ __launch_bounds__(kThreads) void head_grad_partial(const void* __restrict__ x, const double* __restrict__ g, int hw,
                                                              double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const unsigned char* xi = static_cast<const unsigned char*>(x) + (size_t)n * hw * kCin * stored_elem_bytes(PREC);
  const double* gn = g + (size_t)n * kClasses * hw;
  const int first = blockIdx.x * kCellsPerBlock + wave * kCellsPerWave;
  double acc[3][8], accb[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[c][e] = 0.0;
  for (int base = first; base < first + kCellsPerWave && base < hw; base += 8) {      // wave-uniform
    Eight<PREC> raw[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
      raw[q] = load8<PREC>(eight_at<PREC>(xi + (size_t)min(base + q, hw - 1) * kCin * stored_elem_bytes(PREC), lane * 8));
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int cell = base + q;
      if (cell < hw) {
        float f[8];
        decode8(raw[q], f);
        const double gc[3] = {gn[cell], gn[(size_t)hw + cell], gn[2 * (size_t)hw + cell]};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const double d = (double)f[e];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c][e] += gc[c] * d;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) accb[c] += gc[c];
      }
    }
  }
  // the four waves in wave order: waves 1 .. 3 park their sums, wave 0 adds them to its own
  __shared__ double red[3][3][8][64];
  __shared__ double redb[3][3];
  if (wave > 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave - 1][c][e][lane] = acc[c][e];
      if (lane == 0) redb[wave - 1][c] = accb[c];
    }
  }
  __syncthreads();
  if (wave == 0) {
    double* o = part + ((size_t)n * gridDim.x + blockIdx.x) * kClasses * kRow;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        double v = acc[c][e];
#pragma unroll
        for (int k = 0; k < 3; ++k) v += red[k][c][e][lane];
        o[c * kRow + lane * 8 + e] = v;
      }
      if (lane == 0) {
        double v = accb[c];
#pragma unroll
        for (int k = 0; k < 3; ++k) v += redb[k][c];
        o[c * kRow + kCin] = v;
      }
    }
  }
}

// grid = (ceil(1539 / 256), N)
__global__ __launch_bounds__(kThreads) void head_grad_finish(const double* __restrict__ part, int blocks, double scale,
                                                             double* __restrict__ out) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= kClasses * kRow) return;
  const int n = blockIdx.y;
  const double* p = part + (size_t)n * blocks * kClasses * kRow + k;
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < blocks; ++b) s += p[(size_t)b * kClasses * kRow];   // eight loads in flight, added in block order
  out[(size_t)n * kClasses * kRow + k] = k % kRow == kCin ? s : s * scale;
}

struct CeLayout {
  size_t g, cols, total;
  long long Pp;
};

// byte offsets of nbc_ce_gradient's workspace regions (include/nbc.h states the sum); false for a shape the call refuses
bool ce_layout(int N, int H, int W, int h, int w, CeLayout* L) {
  if (!per_image_shape_ok(N, H, W) || h < 1 || w < 1 || h > H || w > W) return false;
  const long long P = (long long)H * W;
  L->Pp = (P + 1) & ~1LL;
  Carver ws;
  L->g = ws.take((size_t)8 * kClasses * N * (size_t)L->Pp);
  L->cols = ws.take((size_t)8 * kClasses * N * (size_t)H * w);
  L->total = ws.offset;
  return true;
}

constexpr const char* kCeWho = "nbc_ce_gradient";
constexpr const char* kTapsWho = "nbc_bicubic_taps";

// the power of two the stored input of classifier.4 carries (f16x2; 0 otherwise)
int head_input_exponent(const nbc_ctx* c) {
  int a = 0;
  return stored_exponent(c, "classifier.0", &a) ? a : 0;
}

}  // namespace

hipError_t launch_bicubic_adjoint(const double* g, long long g_plane, int N, int H, int W, int h, int w, const BicubicTaps& t,
                                  double* cols, double* out, hipStream_t s) {
  if (N < 1 || N > 65535 || h < 1 || w < 1 || h > H || w > W) return hipErrorInvalidValue;
  // along the rows of the image: every full-resolution row Y is a row of W values, the planes g_plane apart
  hipLaunchKernelGGL(ce_col_adjoint, dim3((unsigned)(((long long)H * w + kThreads - 1) / kThreads), (unsigned)N), dim3(kThreads), 0, s, g,
                     g_plane, H, W, w, reinterpret_cast<const int4*>(t.col_idx), reinterpret_cast<const float4*>(t.col_coeff), t.col_lo,
                     t.col_hi, cols);
  hipLaunchKernelGGL(ce_row_adjoint, dim3((unsigned)(((long long)h * w + kThreads - 1) / kThreads), (unsigned)N), dim3(kThreads), 0, s,
                     cols, H, w, h, reinterpret_cast<const int4*>(t.row_idx), reinterpret_cast<const float4*>(t.row_coeff), t.row_lo,
                     t.row_hi, out);
  return hipGetLastError();
}

}  // namespace nbc

using namespace nbc;

// ATen's get_cubic_upsample_coefficients (f32, A = -0.75) with every product and sum rounded on its own
static void cubic_coeffs_host(float t, float c[4]) {
#pragma clang fp contract(off)
  const float A = -0.75f;
  const float x1 = t;
  c[0] = ((A * (x1 + 1.0f) - 5.0f * A) * (x1 + 1.0f) + 8.0f * A) * (x1 + 1.0f) - 4.0f * A;
  c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  const float x2 = 1.0f - t;
  c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  c[3] = ((A * (x2 + 1.0f) - 5.0f * A) * (x2 + 1.0f) + 8.0f * A) * (x2 + 1.0f) - 4.0f * A;
}

extern "C" int nbc_bicubic_taps(int in_size, int out_size, int32_t* idx, float* coeff, int32_t* lo, int32_t* hi) {
#pragma clang fp contract(off)
  if (!idx || !coeff || !lo || !hi) return fail(kTapsWho, NBC_ERR_INVALID, "null argument");
  if (in_size < 1 || out_size < 1 || in_size > (1 << 24) || out_size > (1 << 24))
    return fail(kTapsWho, NBC_ERR_INVALID, "in_size and out_size must lie in 1..2^24");
  const float scale = (float)in_size / (float)out_size;   // area_pixel_compute_scale, as launch_upsample_argmax computes it
  for (int i = 0; i < in_size; ++i) { lo[i] = 0; hi[i] = -1; }
  for (int o = 0; o < out_size; ++o) {
    const float prod = scale * ((float)o + 0.5f);
    const float s = prod - 0.5f;
    int i0 = (int)std::floor(s);
    if (i0 > in_size - 1) i0 = in_size - 1;
    float t = s - (float)i0;
    t = std::fmin(std::fmax(t, 0.f), 1.f);
    cubic_coeffs_host(t, coeff + 4 * (size_t)o);
    for (int k = 0; k < 4; ++k) {
      const int i = i0 - 1 + k;
      const int at = i < 0 ? 0 : (i > in_size - 1 ? in_size - 1 : i);
      idx[4 * (size_t)o + k] = at;
      if (hi[at] < lo[at]) lo[at] = o;                   // o ascends: the first output that touches `at`
      hi[at] = o;
    }
  }
  return NBC_OK;
}

extern "C" size_t nbc_ce_gradient_workspace_bytes(int N, int H, int W, int h, int w) {
  CeLayout L;
  return ce_layout(N, H, W, h, w, &L) ? L.total : 0;
}

extern "C" int nbc_ce_gradient(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int h, int w,
                               const int32_t* row_idx_dev, const float* row_coeff_dev, const int32_t* row_lo_dev,
                               const int32_t* row_hi_dev, const int32_t* col_idx_dev, const float* col_coeff_dev,
                               const int32_t* col_lo_dev, const int32_t* col_hi_dev, const double* table9_host, void* workspace_dev,
                               size_t workspace_bytes, double* grad_lowres_dev, void* hip_stream) {
  if (!logits_full_dev || !target_dev || !row_idx_dev || !row_coeff_dev || !row_lo_dev || !row_hi_dev || !col_idx_dev || !col_coeff_dev ||
      !col_lo_dev || !col_hi_dev || !table9_host || !workspace_dev || !grad_lowres_dev)
    return fail(kCeWho, NBC_ERR_INVALID, "null argument");
  CeLayout L;
  if (!ce_layout(N, H, W, h, w, &L))
    return fail(kCeWho, NBC_ERR_INVALID, std::string(kPerImageShape) + ", 1 <= h <= H and 1 <= w <= W");
  const BicubicTaps taps{row_idx_dev, row_coeff_dev, row_lo_dev, row_hi_dev, col_idx_dev, col_coeff_dev, col_lo_dev, col_hi_dev};
  if (int rc = check_taps(kCeWho, logits_full_dev, taps)) return rc;
  if (reinterpret_cast<uintptr_t>(grad_lowres_dev) & 7u) return fail(kCeWho, NBC_ERR_INVALID, "grad_lowres_dev must be 8-byte aligned");
  if (int rc = check_workspace(kCeWho, workspace_dev, workspace_bytes, L.total)) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  char* ws = static_cast<char*>(workspace_dev);
  double* g = reinterpret_cast<double*>(ws + L.g);
  double* cols = reinterpret_cast<double*>(ws + L.cols);
  CeTable T;
  for (int k = 0; k < 9; ++k) T.t[k] = table9_host[k];
  const long long P = (long long)H * W;
  const long long per_block = (long long)kThreads * kGroup;
  hipLaunchKernelGGL(ce_pixel_gradient, dim3((unsigned)((P + per_block - 1) / per_block), (unsigned)N), dim3(kThreads), 0, s,
                     logits_full_dev, target_dev, P, L.Pp, T, g);
  const hipError_t e = launch_bicubic_adjoint(g, L.Pp, N, H, W, h, w, taps, cols, grad_lowres_dev, s);
  if (e != hipSuccess) return fail(kCeWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

// The trial logits: the caller's theta becomes what the forward's classifier.4 launch reads (the context keeps that array), and
// launch_head1x1 on it is the forward's own machine code.
extern "C" int nbc_head_logits(nbc_ctx* c, const float* theta_dev, int N, int H, int W, float* logits_lowres_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_head_logits";
  if (!c || !theta_dev || !logits_lowres_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!aligned4(theta_dev, logits_lowres_dev)) return fail(kWho, NBC_ERR_INVALID, "theta_dev and logits_lowres_dev must be 4-byte aligned");
  if (!per_image_shape_ok(N, H, W)) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  const Op* head = nullptr;
  if (int rc = last_forward_head(kWho, c, N, H, W, &head)) return rc;
  NBC_HIP(hipSetDevice(c->device));
  NBC_HIP(c->refit_theta.reserve(kHeadThetaFloats * sizeof(float)));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  float* theta = c->refit_theta.as<float>();
  hipLaunchKernelGGL(head_theta_scale, dim3((kHeadThetaFloats + kThreads - 1) / kThreads), dim3(kThreads), 0, s, theta_dev, theta,
                     -head_input_exponent(c));
  NBC_HIP(hipGetLastError());
  NBC_HIP(launch_head1x1(c->bufs[head->in_buf].get(), 512, theta, theta + 3 * 512, logits_lowres_dev, N, c->plan.h * c->plan.w,
                         c->precision, nullptr, c->nonfinite.as<unsigned>(), s));
  return NBC_OK;
}

extern "C" size_t nbc_head_gradient_workspace_bytes(int N, int H, int W) {
  if (!per_image_shape_ok(N, H, W)) return 0;
  int h = 0, w = 0;
  if (nbc_lowres_size(H, W, &h, &w) != NBC_OK || h < 1 || w < 1) return 0;
  return align256((size_t)8 * N * head_grad_blocks(h * w) * kHeadThetaFloats);
}

// d theta [N][3][513] f64 = sum over the hw cells of g [N][3][hw] f64 times x [N][hw][512] stored elements (column 512: the
// plain sum, the bias), times 2^-a on the 512 weight columns.  One read of x; the workspace holds a partial per block.
extern "C" int nbc_head_gradient(nbc_ctx* c, const double* grad_lowres_dev, int N, int H, int W, void* workspace_dev,
                                 size_t workspace_bytes, double* grad_theta_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_head_gradient";
  if (!c || !grad_lowres_dev || !workspace_dev || !grad_theta_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if ((reinterpret_cast<uintptr_t>(grad_lowres_dev) | reinterpret_cast<uintptr_t>(grad_theta_dev)) & 7u)
    return fail(kWho, NBC_ERR_INVALID, "grad_lowres_dev and grad_theta_dev must be 8-byte aligned");
  const size_t need = nbc_head_gradient_workspace_bytes(N, H, W);
  if (need == 0) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  if (int rc = check_workspace(kWho, workspace_dev, workspace_bytes, need)) return rc;
  const Op* head = nullptr;
  if (int rc = last_forward_head(kWho, c, N, H, W, &head)) return rc;
  NBC_HIP(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int hw = c->plan.h * c->plan.w, blocks = head_grad_blocks(hw);
  double* part = static_cast<double*>(workspace_dev);
  with_precision(c->precision, [&](auto P) {
    hipLaunchKernelGGL(head_grad_partial<P.value>, dim3((unsigned)blocks, (unsigned)N), dim3(kThreads), 0, s,
                       c->bufs[head->in_buf].get(), grad_lowres_dev, hw, part);
  });
  hipLaunchKernelGGL(head_grad_finish, dim3((kClasses * kRow + kThreads - 1) / kThreads, (unsigned)N), dim3(kThreads), 0, s, part, blocks,
                     std::ldexp(1.0, -head_input_exponent(c)), grad_theta_dev);
  NBC_HIP(hipGetLastError());
  return NBC_OK;
}
