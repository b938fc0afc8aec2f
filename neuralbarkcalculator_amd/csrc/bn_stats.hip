// Per-image BatchNorm (NBC_BN_PER_IMAGE): the statistics of the image being run, as F.batch_norm(training=True) computes them
// on a batch of one -- the mode the shipped tool's forward runs in (models.py:212-250 never calls .eval() and feeds one image
// per forward).  f32 or f16x2 activations, NHWC [N][hw][C], C a power of two from 64; one set of kernels, which read and write
// their channels as units of stored.hpp: 16 bytes = four channels in f32 (the figures below), eight channels in f16x2.  The
// convolution in front has already run raw (unit scale, zero shift, no ReLU, no identity): what these kernels see is the conv
// output itself, in f16x2 times a power of two per channel that the finish kernel takes off again.
//
//   bn_stats: per (image, channel) the mean and the BIASED variance over the image's hw pixels, in two levels over fixed pixel
//     slices, then the per-image affine pair scale = gamma / sqrt(var + eps), shift = beta - mean * scale.  Two launches:
//       (1) partial sums: grid (slices, C / (4 TQ), N), 256 threads = TQ channel quads x (256 / TQ) pixel lanes; a thread reads
//           16 bytes (four channels) of every (256 / TQ)-th pixel of its slice and accumulates x and x^2 in f64; the lanes
//           are then summed in lane order through LDS and the slice writes one (sum, sum of squares) pair per channel;
//       (2) finish: grid (C / 16, N); 16 slice lanes per channel each sum every 16th slice's pair in slice order (f64), the
//           lanes are summed in lane order, then mean, variance (E[x^2] - mean^2 in f64, clamped at 0), and the f32
//           (scale, shift) table [N][C].
//     Slices depend on hw only, never on N or on timing, and there are no atomics: an image of a batch gets the bits it gets
//     alone.  f64 holds every square of an f32 exactly (48 bits) and the sums to 2^-53 relative, so the cancellation in
//     E[x^2] - mean^2 costs ~2^-53 (mean / std)^2 -- far below f32 for any channel a checkpoint produces.
//   bn_apply: in place, y = relu?(fma(y, scale[n][c], shift[n][c]) (+ identity)), 16 bytes per lane; the image's table is
//     staged in LDS once per block.
//
// Bounds: (1) reads N hw C 4 bytes, writes N slices C 16 bytes (1/64 of what it reads for C >= 256 at 256 pixels a slice);
// (2) reads those and 8 C bytes of (gamma, beta); apply reads and writes N hw C 4 bytes (+ N hw C 4 of identity).
#include "nbc_kernels.hpp"
#include "stored.hpp"

namespace nbc {
namespace {

constexpr int kThreads = 256;
constexpr int kSlicePixels = 256;     // pixels per slice ...
constexpr int kMaxSlices = 1024;      // ... up to this many slices per image (larger maps: larger slices)

// (1) grid (slices, C / (CH UNITS), N), UNITS units of CH channels x LANES pixel lanes: sums of x and x^2 over the slice's pixels,
// per channel, as f64 pairs.  LANES is a function of C alone, so both precisions sum in the same slice and lane orders.
template <int PREC, int UNITS, int LANES>
__global__ __launch_bounds__(UNITS * LANES) void bn_stats_partial_kernel(const float* __restrict__ y, double2* __restrict__ partial,
                                                                         int hw, int C, int slices) {
  static_assert(PREC != 1, "a channel takes four bytes of its pixel here");
  constexpr int CH = Unit<PREC>::CH;
  __shared__ double red[LANES][UNITS][2 * CH];
  const int slice = blockIdx.x, img = blockIdx.z;
  const int q = threadIdx.x % UNITS, lane = threadIdx.x / UNITS;
  const int unit = blockIdx.y * UNITS + q, c = unit * CH;
  const int p0 = (int)(((long long)hw * slice) / slices), p1 = (int)(((long long)hw * (slice + 1)) / slices);
  // in both forms a channel takes four bytes of its pixel: C floats on is the same unit of the next pixel
  const float* base = static_cast<const float*>(unit_at<PREC>(y + (size_t)img * hw * C, unit));
  double s[CH], ss[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) { s[e] = 0.0; ss[e] = 0.0; }
  int p = p0 + lane;
  for (; p + 3 * LANES < p1; p += 4 * LANES) {           // four pixels' loads in flight
    Unit<PREC> raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = unit_load<PREC>(base + (size_t)(p + k * LANES) * C);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v[CH];
      unit_decode(raw[k], v);
      double a[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) a[e] = (double)v[e];
#pragma unroll
      for (int e = 0; e < CH; ++e) { s[e] += a[e]; ss[e] = __builtin_fma(a[e], a[e], ss[e]); }
    }
  }
  for (; p < p1; p += LANES) {
    float v[CH];
    unit_decode(unit_load<PREC>(base + (size_t)p * C), v);
    double a[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) a[e] = (double)v[e];
#pragma unroll
    for (int e = 0; e < CH; ++e) { s[e] += a[e]; ss[e] = __builtin_fma(a[e], a[e], ss[e]); }
  }
#pragma unroll
  for (int e = 0; e < CH; ++e) { red[lane][q][e] = s[e]; red[lane][q][CH + e] = ss[e]; }
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < LANES; ++l)                        // lane order: fixed
#pragma unroll
    for (int e = 0; e < CH; ++e) { s[e] += red[l][q][e]; ss[e] += red[l][q][CH + e]; }
  double2* o = partial + ((size_t)img * slices + slice) * C + c;
#pragma unroll
  for (int e = 0; e < CH; ++e) o[e] = make_double2(s[e], ss[e]);
}

// (2) grid (C / 16, N), 256 threads = 16 channels x 16 slice lanes: lane l sums slices l, l + 16, ... in order (four loads in
// flight), the lanes are summed in lane order through LDS, then the image's f32 (scale, shift).
// f16x2: the sums are of stored values 2^r x.  inv_r[c] = 2^-r_c takes the power off the mean (and twice off the variance) in
// f64, exactly; the table carries the power 2^a_out the normalised tensor is stored with, and 2^-r_c for the stored value it
// multiplies: scale = f32(sc) 2^(a_out - r_c), shift = f32(beta - mean sc) 2^a_out.  The channel's stored rms decides the range
// bit: NBC_NONFINITE_BN_RANGE (2) into `word` when it is not finite, above 2^12, or positive and below 2^-10.
template <int PREC>
struct FinishTail {};                                    // f32: nothing more to know
template <>
struct FinishTail<2> {
  const float* inv_r;
  int a_out;
  unsigned* word;
};

template <int PREC>
__global__ __launch_bounds__(kThreads) void bn_stats_finish_kernel(const double2* __restrict__ partial, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ scale,
                                                                   float* __restrict__ shift, int hw, int C, int slices,
                                                                   FinishTail<PREC> t) {
  constexpr int CH = 16, LANES = kThreads / CH;
  __shared__ double2 red[LANES][CH];
  const int cl = threadIdx.x % CH, lane = threadIdx.x / CH;
  const int c = blockIdx.x * CH + cl, img = blockIdx.y;
  const double2* p = partial + (size_t)img * slices * C + c;
  double s = 0.0, ss = 0.0;
  int k = lane;
  for (; k + 3 * LANES < slices; k += 4 * LANES) {
    double2 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = p[(size_t)(k + q * LANES) * C];
#pragma unroll
    for (int q = 0; q < 4; ++q) { s += v[q].x; ss += v[q].y; }
  }
  for (; k < slices; k += LANES) {
    const double2 v = p[(size_t)k * C];
    s += v.x;
    ss += v.y;
  }
  red[lane][cl] = make_double2(s, ss);
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < LANES; ++l) { s += red[l][cl].x; ss += red[l][cl].y; }   // lane order: fixed
  if constexpr (PREC == 2) {
    const double ir = (double)t.inv_r[c];
    const double ms = s / (double)hw, sq = ss / (double)hw;                    // of the stored values
    const double mean = ms * ir;
    double var = sq - ms * ms;
    if (!(var > 0.0)) var = var != var ? var : 0.0;      // clamp at 0, a NaN stays a NaN
    var = var * ir * ir;
    const double sc = (double)gamma[c] / __builtin_sqrt(var + 1e-5);
    scale[(size_t)img * C + c] = (float)__builtin_scalbn((double)(float)sc * ir, t.a_out);
    shift[(size_t)img * C + c] = (float)__builtin_scalbn((double)(float)((double)beta[c] - mean * sc), t.a_out);
    const double rms = __builtin_sqrt(sq);
    if (t.word && (!__builtin_isfinite(rms) || rms > 4096.0 || (rms > 0.0 && rms < 0.0009765625))) atomicOr(t.word, 2u);
  } else {
    const double mean = s / (double)hw;
    double var = ss / (double)hw - mean * mean;
    if (!(var > 0.0)) var = var != var ? var : 0.0;      // clamp at 0, a NaN stays a NaN
    const double sc = (double)gamma[c] / __builtin_sqrt(var + 1e-5);
    scale[(size_t)img * C + c] = (float)sc;
    shift[(size_t)img * C + c] = (float)((double)beta[c] - mean * sc);
  }
}

// in place: y = relu?(fma(y, scale, shift) (+ res)); grid (blocks, N), grid-stride over the image's units.  The ReLU is each
// precision's own: fmaxf in f32 (a NaN becomes 0), the NaN-propagating maximum in f16x2.
template <int PREC, bool RELU, bool RES>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(unsigned char* __restrict__ y, const unsigned char* __restrict__ res,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            int hw, int C) {
  static_assert(PREC != 1, "a channel takes four bytes of its pixel here");
  constexpr int CH = Unit<PREC>::CH;
  __shared__ float4 tab[2][2048 / 4];
  const int img = blockIdx.y, C4 = C / 4, CU = C / CH;
  for (int i = threadIdx.x; i < C4; i += kThreads) {
    tab[0][i] = reinterpret_cast<const float4*>(scale + (size_t)img * C)[i];
    tab[1][i] = reinterpret_cast<const float4*>(shift + (size_t)img * C)[i];
  }
  __syncthreads();
  const size_t units = (size_t)hw * CU;
  unsigned char* yb = y + (size_t)img * hw * C * 4;
  const unsigned char* rb = RES ? res + (size_t)img * hw * C * 4 : nullptr;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < units; i += stride) {
    void* at = unit_at<PREC>(yb, i);
    const Unit<PREC> raw = unit_load<PREC>(at);
    Unit<PREC> rraw{};
    if constexpr (RES) rraw = unit_load<PREC>(unit_at<PREC>(rb, i));
    const int cu = (int)(i & (size_t)(CU - 1));            // C is a power of two
    float a[CH], b[CH], v[CH];
#pragma unroll
    for (int k = 0; k < CH / 4; ++k) {
      const float4 a4 = tab[0][cu * (CH / 4) + k], b4 = tab[1][cu * (CH / 4) + k];
      a[4 * k] = a4.x; a[4 * k + 1] = a4.y; a[4 * k + 2] = a4.z; a[4 * k + 3] = a4.w;
      b[4 * k] = b4.x; b[4 * k + 1] = b4.y; b[4 * k + 2] = b4.z; b[4 * k + 3] = b4.w;
    }
    unit_decode(raw, v);
#pragma unroll
    for (int e = 0; e < CH; ++e) v[e] = __builtin_fmaf(v[e], a[e], b[e]);
    if constexpr (RES) {
      float r[CH];
      unit_decode(rraw, r);
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] += r[e];
    }
    if constexpr (RELU) {
#pragma unroll
      for (int e = 0; e < CH; ++e) v[e] = PREC == 2 ? __builtin_elementwise_maximum(v[e], 0.f) : __builtin_fmaxf(v[e], 0.f);
    }
    unit_store(at, unit_encode<PREC>(v));
  }
}

bool bn_shape_ok(int N, int hw, int C) { return C >= 64 && C <= 2048 && (C & (C - 1)) == 0 && N >= 1 && N <= 65535 && hw >= 1; }

// the partial kernel's geometry: a block covers CB = min(C, 256) channels with 16 / 8 / 4 pixel lanes (256 threads in f32, 128 in
// f16x2, whose units hold twice the channels)
template <int PREC, int CB, int LANES>
void launch_partial(const void* y, double2* partial, int N, int hw, int C, int slices, hipStream_t s) {
  constexpr int UNITS = CB / Unit<PREC>::CH;
  hipLaunchKernelGGL((bn_stats_partial_kernel<PREC, UNITS, LANES>), dim3(slices, C / CB, N), dim3(UNITS * LANES), 0, s,
                     static_cast<const float*>(y), partial, hw, C, slices);
}

template <int PREC>
hipError_t bn_stats(const void* y, int N, int hw, int C, const float* gamma, const float* beta, const float* inv_r, int a_out, void* ws,
                    unsigned* word, hipStream_t s) {
  const int slices = bn_stats_slices(hw);
  double2* partial = static_cast<double2*>(ws);
  const BnTables t = bn_stats_tables(ws, N, hw, C);
  if (C == 64) launch_partial<PREC, 64, 16>(y, partial, N, hw, C, slices, s);
  else if (C == 128) launch_partial<PREC, 128, 8>(y, partial, N, hw, C, slices, s);
  else launch_partial<PREC, 256, 4>(y, partial, N, hw, C, slices, s);
  FinishTail<PREC> tail{};
  if constexpr (PREC == 2) tail = {inv_r, a_out, word};
  hipLaunchKernelGGL(bn_stats_finish_kernel<PREC>, dim3(C / 16, N), dim3(kThreads), 0, s, partial, gamma, beta, t.scale, t.shift, hw, C,
                     slices, tail);
  return hipGetLastError();
}

template <int PREC>
hipError_t bn_apply(void* y, const void* res, int N, int hw, int C, void* ws, int relu, hipStream_t s) {
  const size_t units = (size_t)hw * (C / Unit<PREC>::CH);
  const size_t per_block = (size_t)kThreads * 4 / Unit<PREC>::LOADS;   // about 64 bytes per lane
  size_t blocks = (units + per_block - 1) / per_block;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  const dim3 g((unsigned)blocks, N);
  const BnTables t = bn_stats_tables(ws, N, hw, C);
  unsigned char* yb = static_cast<unsigned char*>(y);
  const unsigned char* rb = static_cast<const unsigned char*>(res);
  if (res) {
    if (relu) hipLaunchKernelGGL((bn_apply_kernel<PREC, true, true>), g, dim3(kThreads), 0, s, yb, rb, t.scale, t.shift, hw, C);
    else hipLaunchKernelGGL((bn_apply_kernel<PREC, false, true>), g, dim3(kThreads), 0, s, yb, rb, t.scale, t.shift, hw, C);
  } else {
    if (relu) hipLaunchKernelGGL((bn_apply_kernel<PREC, true, false>), g, dim3(kThreads), 0, s, yb, rb, t.scale, t.shift, hw, C);
    else hipLaunchKernelGGL((bn_apply_kernel<PREC, false, false>), g, dim3(kThreads), 0, s, yb, rb, t.scale, t.shift, hw, C);
  }
  return hipGetLastError();
}

}  // namespace

int bn_stats_slices(int hw) {
  const int s = (hw + kSlicePixels - 1) / kSlicePixels;
  return s < kMaxSlices ? s : kMaxSlices;
}

size_t bn_stats_workspace_bytes(int N, int hw, int C) {
  return (size_t)N * bn_stats_slices(hw) * C * sizeof(double2) + 2 * (size_t)N * C * sizeof(float);
}

BnTables bn_stats_tables(void* ws, int N, int hw, int C) {
  float* scale = reinterpret_cast<float*>(static_cast<double2*>(ws) + (size_t)N * bn_stats_slices(hw) * C);
  return {scale, scale + (size_t)N * C};
}

hipError_t launch_bn_stats(const void* y, int N, int hw, int C, const float* gamma, const float* beta, const float* inv_r, int a_out,
                           void* ws, unsigned* word, int precision, hipStream_t s) {
  if (!bn_shape_ok(N, hw, C)) return hipErrorInvalidValue;
  return with_precision(precision, [&](auto P) {        // f32 reads none of inv_r, a_out and word
    if constexpr (P.value == 1) return hipErrorInvalidValue;
    else return bn_stats<P.value>(y, N, hw, C, gamma, beta, inv_r, a_out, ws, word, s);
  });
}

hipError_t launch_bn_apply(void* y, const void* res, int N, int hw, int C, void* ws, int relu, int precision, hipStream_t s) {
  if (!bn_shape_ok(N, hw, C)) return hipErrorInvalidValue;
  return with_precision(precision, [&](auto P) {
    if constexpr (P.value == 1) return hipErrorInvalidValue;
    else return bn_apply<P.value>(y, res, N, hw, C, ws, relu, s);
  });
}

}  // namespace nbc
