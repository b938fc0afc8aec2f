// Per-image pixel-wise cross-entropy sums on the device: what the reference's CustomWeightedCrossEntropy
// (bark_calculator/utils.py:151-165: F.cross_entropy(reduction='none'), argmax, max(argmax, target), index_select of the
// class weights, multiply, mean), the plain cross-entropy (xloss, lovasz_losses.py:246-251) and MixedLoss (utils.py:185-192)
// need from the pixels, reduced so that the class weights stay host arithmetic.  Per image, with t the target class of a
// pixel, p = argmax of its three logits (first maximum wins, a NaN counts as the maximum: torch.argmax, and the forward's
// own argmax kernel in pointwise.hip) and ce = logsumexp(x) - x[t]:
//   S[t][p] = sum of ce over the pixels of cell (t, p)   (f64)
//   K[t][p] = number of those pixels                      (i64; the raw confusion of nbc_confusion)
// Only these 9 + 9 numbers per image leave the device; every loss of the family is a few host operations on them
// (neuralbarkcalculator_amd/metrics.py).
//
//   pixel_ce_partial  one block per (tile of 4096 pixels, image).  A thread owns four groups of four consecutive pixels,
//                     group g of the tile at pixel (g * 256 + tid) * 4: fixed by the pixel index alone.  A group whose three
//                     plane addresses are 16-byte aligned (and its target bytes 4-byte aligned) and that lies whole inside
//                     the image comes in by three 16-byte loads and one 4-byte load; any other group (the tail of an image,
//                     every group of an image whose planes start off a 16-byte boundary: H * W not a multiple of 4) by
//                     4-byte and 1-byte loads.  How a pixel was loaded reaches nothing: the entropy is evaluated in f64 from
//                     the f32 logits, m = max, log(sum exp(x_c - m)) - (x_t - m), and added to the thread's accumulator
//                     of its cell (a select, not a multiplication by 0: a non-finite entropy reaches its own cell only)
//                     in pixel order; then lanes (wave_sum), then the four waves in order through LDS.  One f64 and one
//                     u32 partial per (image, cell, tile) go to the workspace.  No atomics, no memset.
//   pixel_ce_finish   one wave per (image, cell): lane l adds the partials of tiles l, l + 64, ... in tile order, then
//                     wave_sum.
// The tile size and both orders depend on H * W alone, so an image's 18 numbers are bit-identical alone, anywhere in a
// batch and on any stream.  IEEE arithmetic gives torch's answers on non-finite input by itself: a NaN or +inf logit, or three
// -inf, make x_c - m NaN and with it the entropy; -inf at the target class alone makes it +inf.
// No library besides the HIP runtime.
#include <hip/hip_runtime.h>

#include <cmath>

#include "reduce.hpp"

using namespace nbc;

namespace {

constexpr int kClasses = 3;
constexpr int kCells = 9;
constexpr int kThreads = 256;                           // 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kGroup = 4;                               // consecutive pixels per load group
constexpr int kGroups = 4;                              // groups per thread and tile
constexpr int kTile = kThreads * kGroup * kGroups;      // 4096 pixels per tile
constexpr const char* kWho = "nbc_pixel_cross_entropy";

using u32 = unsigned;
using u64 = unsigned long long;

// adds one pixel's entropy and count to the accumulators of its cell
// (the counts packed 7 bits per cell, as in confusion.hip: a thread sees 16 pixels)
__device__ __forceinline__ void add_pixel(float a, float b, float c, u32 grey, double (&acc)[kCells], u64& packed) {
  const double x0 = (double)a, x1 = (double)b, x2 = (double)c;
  const double m = fmax(fmax(x0, x1), x2);              // skips a NaN, which poisons its own difference below
  const double s = exp(x0 - m) + exp(x1 - m) + exp(x2 - m);
  const u32 t = target_class(grey);
  const double xt = t == 0u ? x0 : t == 1u ? x1 : x2;
  const double ce = log(s) - (xt - m);
  const u32 best = argmax3(a, b, c);                    // the forward's own labels (upsample_argmax_kernel)
  const u32 cell = t * 3u + best;
  packed += 1ull << (7u * cell);
#pragma unroll
  for (int k = 0; k < kCells; ++k) acc[k] += cell == (u32)k ? ce : 0.0;
}

__global__ __launch_bounds__(kThreads) void pixel_ce_partial(const float* __restrict__ logits, const unsigned char* __restrict__ target,
                                                             long long P, int T, double* __restrict__ part_sum,
                                                             u32* __restrict__ part_cnt) {
  const int n = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* l0 = logits + (size_t)n * kClasses * P;
  const float* l1 = l0 + P;
  const float* l2 = l1 + P;
  const unsigned char* tg = target + (size_t)n * P;
  // group starts are multiples of 4 pixels: they keep whatever alignment the image's planes start with
  const bool vec = ((reinterpret_cast<uintptr_t>(l0) | reinterpret_cast<uintptr_t>(l1) | reinterpret_cast<uintptr_t>(l2)) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(tg) & 3u) == 0;
  const long long start = (long long)tile * kTile;

  double acc[kCells] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  u64 packed = 0;
  static_assert(kGroup * kGroups <= 127, "a thread's pixels must fit the 7-bit counters");
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const long long q = start + (long long)(g * kThreads + tid) * kGroup;
    if (q >= P) continue;
    if (vec && q + kGroup <= P) {
      const float4 a = *reinterpret_cast<const float4*>(l0 + q);
      const float4 b = *reinterpret_cast<const float4*>(l1 + q);
      const float4 c = *reinterpret_cast<const float4*>(l2 + q);
      const u32 t = *reinterpret_cast<const u32*>(tg + q);
      add_pixel(a.x, b.x, c.x, t & 255u, acc, packed);
      add_pixel(a.y, b.y, c.y, (t >> 8) & 255u, acc, packed);
      add_pixel(a.z, b.z, c.z, (t >> 16) & 255u, acc, packed);
      add_pixel(a.w, b.w, c.w, t >> 24, acc, packed);
    } else {
      const int left = (int)(P - q < kGroup ? P - q : kGroup);
      for (int k = 0; k < left; ++k) add_pixel(l0[q + k], l1[q + k], l2[q + k], tg[q + k], acc, packed);
    }
  }

  __shared__ double dred[kWaves][kCells];
  __shared__ u32 cred[kWaves][kCells];
#pragma unroll
  for (int k = 0; k < kCells; ++k) {
    const double v = wave_sum(acc[k]);
    const u32 c = wave_sum((u32)(packed >> (7 * k)) & 127u);
    if (lane == 0) { dred[w][k] = v; cred[w][k] = c; }
  }
  __syncthreads();
  if (tid < kCells) {
    double s = 0.0;
    u32 c = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) { s += dred[k][tid]; c += cred[k][tid]; }
    const size_t o = ((size_t)n * kCells + tid) * T + tile;
    part_sum[o] = s;
    part_cnt[o] = c;
  }
}

__global__ __launch_bounds__(64) void pixel_ce_finish(const double* __restrict__ part_sum, const u32* __restrict__ part_cnt, int T,
                                                      double* __restrict__ sums, u64* __restrict__ counts) {
  const size_t seg = blockIdx.x;                       // image * 9 + cell
  const int lane = threadIdx.x;
  const double* ps = part_sum + seg * T;
  const u32* pc = part_cnt + seg * T;
  double s = 0.0;
  u64 c = 0;
  for (int t = lane; t < T; t += 64) { s += ps[t]; c += pc[t]; }
  s = wave_sum(s);
  c = wave_sum(c);
  if (lane == 0) { sums[seg] = s; counts[seg] = c; }
}

struct Layout {
  size_t part_sum, part_cnt, total;
  int T;
};

// byte offsets of the workspace regions (include/nbc.h states the sum); false for a shape the call refuses
bool layout(int N, int H, int W, Layout* L) {
  if (!per_image_shape_ok(N, H, W)) return false;
  const size_t P = (size_t)H * (size_t)W;
  const size_t T = (P + kTile - 1) / kTile, S = (size_t)kCells * N;
  Carver ws;
  L->part_sum = ws.take(8 * S * T);
  L->part_cnt = ws.take(4 * S * T);
  L->total = ws.offset;
  L->T = (int)T;
  return true;
}

}  // namespace

extern "C" size_t nbc_pixel_ce_workspace_bytes(int N, int H, int W) {
  Layout L;
  return layout(N, H, W, &L) ? L.total : 0;
}

extern "C" int nbc_pixel_cross_entropy(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, void* workspace_dev,
                                       size_t workspace_bytes, double* sums_dev, int64_t* counts_dev, void* hip_stream) {
  if (!logits_full_dev || !target_dev || !workspace_dev || !sums_dev || !counts_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  Layout L;
  if (!layout(N, H, W, &L)) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  if (int rc = check_workspace(kWho, workspace_dev, workspace_bytes, L.total)) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  char* ws = static_cast<char*>(workspace_dev);
  double* part_sum = reinterpret_cast<double*>(ws + L.part_sum);
  u32* part_cnt = reinterpret_cast<u32*>(ws + L.part_cnt);
  const long long P = (long long)H * W;
  hipLaunchKernelGGL(pixel_ce_partial, dim3((unsigned)L.T, (unsigned)N), dim3(kThreads), 0, s, logits_full_dev, target_dev, P, L.T,
                     part_sum, part_cnt);
  hipLaunchKernelGGL(pixel_ce_finish, dim3((unsigned)(kCells * N)), dim3(64), 0, s, part_sum, part_cnt, L.T, sums_dev,
                     reinterpret_cast<u64*>(counts_dev));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
