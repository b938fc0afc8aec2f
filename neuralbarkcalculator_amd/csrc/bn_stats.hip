// Per-image BatchNorm (NBC_BN_PER_IMAGE): the statistics of the image being run, as F.batch_norm(training=True) computes them
// on a batch of one -- the mode the shipped tool's forward runs in (models.py:212-250 never calls .eval() and feeds one image
// per forward).  f32 activations, NHWC [N][hw][C], C a multiple of 64 (the f16x2 variants on pieces follow the f32 kernels
// below).  The convolution in front has already run raw (unit scale, zero shift, no ReLU, no identity): what these kernels
// see is the conv output itself.
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
#include "split16.hpp"

namespace nbc {
namespace {

constexpr int kThreads = 256;
constexpr int kSlicePixels = 256;     // pixels per slice ...
constexpr int kMaxSlices = 1024;      // ... up to this many slices per image (larger maps: larger slices)

// (1) grid (slices, C / (4 TQ), N): sums of x and x^2 over the slice's pixels, per channel, as f64 pairs
template <int TQ>
__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(const float* __restrict__ y, double2* __restrict__ partial,
                                                                    int hw, int C, int slices) {
  constexpr int LANES = kThreads / TQ;                   // pixel lanes of the block
  __shared__ double red[LANES][TQ][8];
  const int slice = blockIdx.x, img = blockIdx.z;
  const int q = threadIdx.x % TQ, lane = threadIdx.x / TQ;
  const int c = (blockIdx.y * TQ + q) * 4;
  const int p0 = (int)(((long long)hw * slice) / slices), p1 = (int)(((long long)hw * (slice + 1)) / slices);
  const float* base = y + (size_t)img * hw * C + c;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
  int p = p0 + lane;
  for (; p + 3 * LANES < p1; p += 4 * LANES) {           // four pixels' loads in flight
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const float4*>(base + (size_t)(p + k * LANES) * C);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double a[4] = {(double)v[k].x, (double)v[k].y, (double)v[k].z, (double)v[k].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[e] += a[e]; ss[e] = __builtin_fma(a[e], a[e], ss[e]); }
    }
  }
  for (; p < p1; p += LANES) {
    const float4 v = *reinterpret_cast<const float4*>(base + (size_t)p * C);
    const double a[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] += a[e]; ss[e] = __builtin_fma(a[e], a[e], ss[e]); }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[lane][q][e] = s[e]; red[lane][q][4 + e] = ss[e]; }
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < LANES; ++l)                        // lane order: fixed
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[e] += red[l][q][e]; ss[e] += red[l][q][4 + e]; }
  double2* o = partial + ((size_t)img * slices + slice) * C + c;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = make_double2(s[e], ss[e]);
}

// (2) grid (C / 16, N), 256 threads = 16 channels x 16 slice lanes: lane l sums slices l, l + 16, ... in order (four loads in
// flight), the lanes are summed in lane order through LDS, then the image's f32 (scale, shift)
__global__ __launch_bounds__(kThreads) void bn_stats_finish_kernel(const double2* __restrict__ partial, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ scale,
                                                                   float* __restrict__ shift, int hw, int C, int slices) {
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
  const double mean = s / (double)hw;
  double var = ss / (double)hw - mean * mean;
  if (!(var > 0.0)) var = var != var ? var : 0.0;        // clamp at 0, a NaN stays a NaN
  const double sc = (double)gamma[c] / __builtin_sqrt(var + 1e-5);
  scale[(size_t)img * C + c] = (float)sc;
  shift[(size_t)img * C + c] = (float)((double)beta[c] - mean * sc);
}

// in place: y = relu?(fma(y, scale, shift) (+ res)); grid (blocks, N), grid-stride over the image's 16-byte chunks
template <bool RELU, bool RES>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(float* __restrict__ y, const float* __restrict__ res,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            int hw, int C) {
  __shared__ float4 tab[2][2048 / 4];
  const int img = blockIdx.y, C4 = C / 4;
  for (int i = threadIdx.x; i < C4; i += kThreads) {
    tab[0][i] = reinterpret_cast<const float4*>(scale + (size_t)img * C)[i];
    tab[1][i] = reinterpret_cast<const float4*>(shift + (size_t)img * C)[i];
  }
  __syncthreads();
  const size_t n4 = (size_t)hw * C4;
  float4* yv = reinterpret_cast<float4*>(y + (size_t)img * hw * C);
  const float4* rv = RES ? reinterpret_cast<const float4*>(res + (size_t)img * hw * C) : nullptr;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
    float4 v = yv[i];
    const int c4 = (int)(i & (size_t)(C4 - 1));            // C is a power of two
    const float4 a = tab[0][c4], b = tab[1][c4];
    v.x = __builtin_fmaf(v.x, a.x, b.x); v.y = __builtin_fmaf(v.y, a.y, b.y);
    v.z = __builtin_fmaf(v.z, a.z, b.z); v.w = __builtin_fmaf(v.w, a.w, b.w);
    if constexpr (RES) {
      const float4 r = rv[i];
      v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    if constexpr (RELU) {
      v.x = __builtin_fmaxf(v.x, 0.f); v.y = __builtin_fmaxf(v.y, 0.f);
      v.z = __builtin_fmaxf(v.z, 0.f); v.w = __builtin_fmaxf(v.w, 0.f);
    }
    yv[i] = v;
  }
}

bool bn_channels_ok(int C) { return C >= 64 && C <= 2048 && (C & (C - 1)) == 0; }

// ---- NBC_PREC_F16X2: the same three kernels on the piece layout (split16.hpp).  A pixel's channels lie in 128-byte groups of
// 32, [h0 x 32][h1 x 32]; a lane owns 8 channels: 16 bytes of high pieces and the 16 bytes of low pieces 64 bytes on (the access
// pattern of x2_store, f16x2_mma.hpp).  What the convolution in front has stored is 2^r_o conv_o, r_o the power of two that
// normalises channel o by its running statistics (nbc_pack_bn_raw); the finish kernel takes it off again in f64.

// byte offset of 8-channel chunk j of a run of 128-byte groups
__device__ __forceinline__ size_t x2_chunk(size_t j) { return (j >> 2) * 128 + (j & 3) * 16; }

// (1) grid (slices, C / (8 TO), N), TO channel octets x LANES pixel lanes: LANES, the slices and the orders of the sums are
// those of bn_stats_partial_kernel for the same C
template <int TO, int LANES>
__global__ __launch_bounds__(TO * LANES) void bn_stats_partial_x2_kernel(const unsigned char* __restrict__ y, double2* __restrict__ partial,
                                                                          int hw, int C, int slices) {
  __shared__ double red[LANES][TO][16];
  const int slice = blockIdx.x, img = blockIdx.z;
  const int q = threadIdx.x % TO, lane = threadIdx.x / TO;
  const int oct = blockIdx.y * TO + q, c = oct * 8;
  const int p0 = (int)(((long long)hw * slice) / slices), p1 = (int)(((long long)hw * (slice + 1)) / slices);
  const size_t pitch = (size_t)C * 4;                    // bytes of a pixel
  const unsigned char* base = y + (size_t)img * hw * pitch + x2_chunk(oct);
  double s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.0; ss[e] = 0.0; }
  int p = p0 + lane;
  for (; p + 3 * LANES < p1; p += 4 * LANES) {           // four pixels' loads in flight
    uint4 h0[4], h1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned char* px = base + (size_t)(p + k * LANES) * pitch;
      h0[k] = *reinterpret_cast<const uint4*>(px);
      h1[k] = *reinterpret_cast<const uint4*>(px + 64);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v[8];
      join16x8(h0[k], h1[k], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) { const double a = (double)v[e]; s[e] += a; ss[e] = __builtin_fma(a, a, ss[e]); }
    }
  }
  for (; p < p1; p += LANES) {
    const unsigned char* px = base + (size_t)p * pitch;
    const uint4 h0 = *reinterpret_cast<const uint4*>(px), h1 = *reinterpret_cast<const uint4*>(px + 64);
    float v[8];
    join16x8(h0, h1, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const double a = (double)v[e]; s[e] += a; ss[e] = __builtin_fma(a, a, ss[e]); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[lane][q][e] = s[e]; red[lane][q][8 + e] = ss[e]; }
  __syncthreads();
  if (lane != 0) return;
  for (int l = 1; l < LANES; ++l)                        // lane order: fixed
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] += red[l][q][e]; ss[e] += red[l][q][8 + e]; }
  double2* o = partial + ((size_t)img * slices + slice) * C + c;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = make_double2(s[e], ss[e]);
}

// (2) bn_stats_finish_kernel on sums of stored values 2^r x: inv_r[c] = 2^-r_c takes the power off the mean (and twice off the
// variance) in f64, exactly; the table carries the power 2^a_out the normalised tensor is stored with, and 2^-r_c for the stored
// value it multiplies: scale = f32(sc) 2^(a_out - r_c), shift = f32(beta - mean sc) 2^a_out.  The channel's stored rms decides
// the range bit: NBC_NONFINITE_BN_RANGE (2) into `word` when it is not finite, above 2^12, or positive and below 2^-10.
__global__ __launch_bounds__(kThreads) void bn_stats_finish_x2_kernel(const double2* __restrict__ partial, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, const float* __restrict__ inv_r,
                                                                      float* __restrict__ scale, float* __restrict__ shift, int hw, int C,
                                                                      int slices, int a_out, unsigned* __restrict__ word) {
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
  const double ir = (double)inv_r[c];
  const double ms = s / (double)hw, sq = ss / (double)hw;                      // of the stored values
  const double mean = ms * ir;
  double var = sq - ms * ms;
  if (!(var > 0.0)) var = var != var ? var : 0.0;        // clamp at 0, a NaN stays a NaN
  var = var * ir * ir;
  const double sc = (double)gamma[c] / __builtin_sqrt(var + 1e-5);
  scale[(size_t)img * C + c] = (float)__builtin_scalbn((double)(float)sc * ir, a_out);
  shift[(size_t)img * C + c] = (float)__builtin_scalbn((double)(float)((double)beta[c] - mean * sc), a_out);
  const double rms = __builtin_sqrt(sq);
  if (word && (!__builtin_isfinite(rms) || rms > 4096.0 || (rms > 0.0 && rms < 0.0009765625))) atomicOr(word, 2u);
}

// in place on pieces: join, fma(x, scale, shift) (+ joined identity), ReLU (NaN-propagating), split; grid (blocks, N),
// grid-stride over the image's 8-channel chunks
template <bool RELU, bool RES>
__global__ __launch_bounds__(kThreads) void bn_apply_x2_kernel(unsigned char* __restrict__ y, const unsigned char* __restrict__ res,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               int hw, int C) {
  __shared__ float4 tab[2][2048 / 4];
  const int img = blockIdx.y, C4 = C / 4, C8 = C / 8;
  for (int i = threadIdx.x; i < C4; i += kThreads) {
    tab[0][i] = reinterpret_cast<const float4*>(scale + (size_t)img * C)[i];
    tab[1][i] = reinterpret_cast<const float4*>(shift + (size_t)img * C)[i];
  }
  __syncthreads();
  const size_t n8 = (size_t)hw * C8;
  unsigned char* yb = y + (size_t)img * hw * C * 4;
  const unsigned char* rb = RES ? res + (size_t)img * hw * C * 4 : nullptr;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += stride) {
    const size_t off = x2_chunk(i);                        // the groups of a tensor are contiguous
    const uint4 h0 = *reinterpret_cast<const uint4*>(yb + off), h1 = *reinterpret_cast<const uint4*>(yb + off + 64);
    uint4 r0{}, r1{};
    if constexpr (RES) { r0 = *reinterpret_cast<const uint4*>(rb + off); r1 = *reinterpret_cast<const uint4*>(rb + off + 64); }
    const int c8 = (int)(i & (size_t)(C8 - 1));            // C is a power of two
    const float4 a0 = tab[0][2 * c8], a1 = tab[0][2 * c8 + 1], b0 = tab[1][2 * c8], b1 = tab[1][2 * c8 + 1];
    const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    float v[8];
    join16x8(h0, h1, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(v[e], a[e], b[e]);
    if constexpr (RES) {
      float r[8];
      join16x8(r0, r1, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += r[e];
    }
    if constexpr (RELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = __builtin_elementwise_maximum(v[e], 0.f);
    }
    uint4 o0, o1;
    split16x8(v, o0, o1);
    *reinterpret_cast<uint4*>(yb + off + 64) = o1;
    *reinterpret_cast<uint4*>(yb + off) = o0;
  }
}

}  // namespace

int bn_stats_slices(int hw) {
  const int s = (hw + kSlicePixels - 1) / kSlicePixels;
  return s < kMaxSlices ? s : kMaxSlices;
}

size_t bn_stats_workspace_bytes(int N, int hw, int C) {
  return (size_t)N * bn_stats_slices(hw) * C * sizeof(double2) + 2 * (size_t)N * C * sizeof(float);
}

hipError_t launch_bn_stats(const float* y, int N, int hw, int C, const float* gamma, const float* beta, void* ws, float* scale,
                           float* shift, hipStream_t s) {
  if (!bn_channels_ok(C) || N < 1 || N > 65535 || hw < 1) return hipErrorInvalidValue;
  const int slices = bn_stats_slices(hw);
  double2* partial = static_cast<double2*>(ws);
  if (C == 64) {
    hipLaunchKernelGGL(bn_stats_partial_kernel<16>, dim3(slices, 1, N), dim3(kThreads), 0, s, y, partial, hw, C, slices);
  } else if (C == 128) {
    hipLaunchKernelGGL(bn_stats_partial_kernel<32>, dim3(slices, 1, N), dim3(kThreads), 0, s, y, partial, hw, C, slices);
  } else {
    hipLaunchKernelGGL(bn_stats_partial_kernel<64>, dim3(slices, C / 256, N), dim3(kThreads), 0, s, y, partial, hw, C, slices);
  }
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(C / 16, N), dim3(kThreads), 0, s, partial, gamma, beta, scale, shift, hw, C,
                     slices);
  return hipGetLastError();
}

hipError_t launch_bn_apply(float* y, const float* res, int N, int hw, int C, const float* scale, const float* shift, int relu,
                           hipStream_t s) {
  if (!bn_channels_ok(C) || N < 1 || N > 65535 || hw < 1) return hipErrorInvalidValue;
  const size_t n4 = (size_t)hw * (C / 4);
  size_t blocks = (n4 + 4 * kThreads - 1) / (4 * kThreads);   // about four chunks per lane
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  const dim3 g((unsigned)blocks, N);
  if (res) {
    if (relu) hipLaunchKernelGGL((bn_apply_kernel<true, true>), g, dim3(kThreads), 0, s, y, res, scale, shift, hw, C);
    else hipLaunchKernelGGL((bn_apply_kernel<false, true>), g, dim3(kThreads), 0, s, y, res, scale, shift, hw, C);
  } else {
    if (relu) hipLaunchKernelGGL((bn_apply_kernel<true, false>), g, dim3(kThreads), 0, s, y, res, scale, shift, hw, C);
    else hipLaunchKernelGGL((bn_apply_kernel<false, false>), g, dim3(kThreads), 0, s, y, res, scale, shift, hw, C);
  }
  return hipGetLastError();
}

hipError_t launch_bn_stats_f16x2(const void* y, int N, int hw, int C, const float* gamma, const float* beta, const float* inv_r,
                                 int a_out, void* ws, float* scale, float* shift, unsigned* word, hipStream_t s) {
  if (!bn_channels_ok(C) || N < 1 || N > 65535 || hw < 1) return hipErrorInvalidValue;
  const int slices = bn_stats_slices(hw);
  const unsigned char* yb = static_cast<const unsigned char*>(y);
  double2* partial = static_cast<double2*>(ws);
  if (C == 64) {
    hipLaunchKernelGGL((bn_stats_partial_x2_kernel<8, 16>), dim3(slices, 1, N), dim3(128), 0, s, yb, partial, hw, C, slices);
  } else if (C == 128) {
    hipLaunchKernelGGL((bn_stats_partial_x2_kernel<16, 8>), dim3(slices, 1, N), dim3(128), 0, s, yb, partial, hw, C, slices);
  } else {
    hipLaunchKernelGGL((bn_stats_partial_x2_kernel<32, 4>), dim3(slices, C / 256, N), dim3(128), 0, s, yb, partial, hw, C, slices);
  }
  hipLaunchKernelGGL(bn_stats_finish_x2_kernel, dim3(C / 16, N), dim3(kThreads), 0, s, partial, gamma, beta, inv_r, scale, shift, hw,
                     C, slices, a_out, word);
  return hipGetLastError();
}

hipError_t launch_bn_apply_f16x2(void* y, const void* res, int N, int hw, int C, const float* scale, const float* shift, int relu,
                                 hipStream_t s) {
  if (!bn_channels_ok(C) || N < 1 || N > 65535 || hw < 1) return hipErrorInvalidValue;
  const size_t n8 = (size_t)hw * (C / 8);
  size_t blocks = (n8 + 2 * kThreads - 1) / (2 * kThreads);   // about two chunk pairs (64 bytes) per lane
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  const dim3 g((unsigned)blocks, N);
  unsigned char* yb = static_cast<unsigned char*>(y);
  const unsigned char* rb = static_cast<const unsigned char*>(res);
  if (res) {
    if (relu) hipLaunchKernelGGL((bn_apply_x2_kernel<true, true>), g, dim3(kThreads), 0, s, yb, rb, scale, shift, hw, C);
    else hipLaunchKernelGGL((bn_apply_x2_kernel<false, true>), g, dim3(kThreads), 0, s, yb, rb, scale, shift, hw, C);
  } else {
    if (relu) hipLaunchKernelGGL((bn_apply_x2_kernel<true, false>), g, dim3(kThreads), 0, s, yb, rb, scale, shift, hw, C);
    else hipLaunchKernelGGL((bn_apply_x2_kernel<false, false>), g, dim3(kThreads), 0, s, yb, rb, scale, shift, hw, C);
  }
  return hipGetLastError();
}

}  // namespace nbc
