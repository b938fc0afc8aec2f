// Per-image Lovasz-Softmax loss terms on the device: `LovaszSoftmax()(logits, target)` of
// the reference's bark_calculator/lovasz_losses.py:162-223 (softmax, then lovasz_softmax_flat with classes='present',
// ignore=None) for a batch of one, the objective the training script builds its Experiment with (__main__.py:236-239).
// One f64 term per (image, class) and the class's foreground count leave the device; the mean over the present classes
// is host arithmetic (neuralbarkcalculator_amd/metrics.py, lovasz_loss).
//
// Per (image, class) "segment" of P = H * W pixels:
//   lovasz_keys     reads the logits [3,H,W] and the u8 grey target once; writes one u32 key per (class, pixel),
//                   key = bits(e) << 1 | fg with e = |fg - softmax_c| in [0, 1] (so bits(e) <= 0x3F800000 is monotone in
//                   e and the key fits in 31 bits), the foreground count G of every class (integer atomics: their order
//                   reaches nothing) and a per-image flag when a pixel's softmax is not finite.
//   lovasz_hist / lovasz_scan / lovasz_scatter
//                   a keys-only LSD radix sort, descending, 8-bit digits in 4 passes, tiles of 8192 keys: per-tile digit
//                   histograms, their exclusive scan per segment, and a stable scatter (ranks from wave ballots, the tile
//                   sorted in LDS, then written out in runs).  Keys-only: any correct sort gives the same array.
//   lovasz_tile_fg  foreground keys per sorted tile (exact integers).
//   lovasz_partial  per tile: running fg / bg counts, J_i = 1 - I_i / U_i and J_{i-1} in f64, sum of e_(i) (J_i - J_{i-1})
//                   in f64 in the fixed order of reduce.hpp.
//   lovasz_finish   one thread per segment adds the tile partials in tile order.
// A segment whose class is absent (G = 0) or whose image has a non-finite softmax is not sorted: its term is
// 0 or NaN.  No library besides the HIP runtime.
//
// Pooled over groups (nbc_lovasz_softmax_groups: `LovaszSoftmax()` on a batch, per_image=False, lovasz_losses.py:169-191): the
// segment of (group, class) is the pixels of the group's g consecutive images, one after the other -- the per-image segment
// of the g images stacked along the height.  Only lovasz_keys knows about images: it writes the key of (image n, class c,
// pixel i) to segment (n / G, c) at (n mod G) P + i.  Everything after it works on segments whose length Segments::pixels
// gives (the last group may be shorter); the per-image pass is the case G = 1, same kernels, same tiles, same bits.
//
// The gradient (nbc_lovasz_gradient, per image) follows the same launches: a copy of the keys in pixel order before the sort, then
//   lovasz_fg_prefix       the foreground keys before every position of the sorted segment (lovasz_partial's running count),
//   lovasz_pixel_gradient  per pixel and class the run of its key in the sorted segment (a binary search), the run's mean slope,
//                          the softmax Jacobian in f64, the table's cross-entropy term beside it: three f64 planes per image,
// and the adjoint of the bicubic upsample (launch_bicubic_adjoint, head_refit.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "ce_gradient.hpp"
#include "reduce.hpp"

using namespace nbc;

namespace {

constexpr int kClasses = 3;
constexpr int kSortThreads = 512;                       // 8 waves
constexpr int kWaves = kSortThreads / 64;
constexpr int kItems = 16;                              // keys per lane and tile
constexpr int kTile = kSortThreads * kItems;            // 8192 keys per tile
constexpr int kRadix = 256;
constexpr int kPasses = 4;                              // 4 x 8 bits cover the 31-bit keys
constexpr int kKeyThreads = 256;
constexpr int kScanThreads = 1024;                      // 4 groups of 256 digit lanes
constexpr const char* kWho = "nbc_lovasz_softmax";
constexpr const char* kWhoGroups = "nbc_lovasz_softmax_groups";
constexpr int kMaxGroup = 64;                           // evaluate.py's MAX_POOL

using u32 = unsigned;
using u64 = unsigned long long;

// descending order: the digit of ~key, so that the ascending LSD sort puts large keys first
__device__ __forceinline__ u32 digit_of(u32 key, int shift) { return ((~key) >> shift) & (kRadix - 1u); }

__device__ __forceinline__ u64 lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the lanes of this wave that hold the same 8-bit digit (and are valid)
__device__ __forceinline__ u64 digit_peers(u32 d, bool valid) {
  u64 peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const u64 vote = __ballot(bit);
    peers &= bit ? vote : ~vote;
  }
  return peers;
}

// exclusive scan of v over threads 0..255; every thread of the block calls it (threads >= 256 pass anything and get garbage)
__device__ __forceinline__ u32 excl_scan_256(u32 v, u32* wsum /* LDS [4] */) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  u32 x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (w < 4 && lane == 63) wsum[w] = x;
  __syncthreads();
  u32 pre = 0;
  for (int k = 0; k < 4 && k < w; ++k) pre += wsum[k];
  return pre + x - v;
}

// Where the segments of a call lie: N images of P pixels in consecutive groups of `group` (the last one shorter when group
// does not divide N).  Group n holds its three segments back to back behind the 3 * group * P keys of every group before it.
struct Segments {
  long long P;
  int N, group;
  __host__ __device__ long long pixels(int n) const { const int left = N - n * group; return (long long)(left < group ? left : group) * P; }
  __host__ __device__ size_t keys_at(int n, int c) const { return (size_t)n * group * kClasses * P + (size_t)c * pixels(n); }
  __host__ __device__ int tiles(int n) const { return (int)((pixels(n) + kTile - 1) / kTile); }
};

__device__ __forceinline__ bool segment_idle(const u64* G, const u32* flag, int n, int seg) { return G[seg] == 0 || flag[n] != 0; }

__global__ __launch_bounds__(kKeyThreads) void lovasz_keys(const float* __restrict__ logits, const unsigned char* __restrict__ target,
                                                           Segments sg, u32* __restrict__ keys, u64* __restrict__ G,
                                                           u32* __restrict__ flag) {
  const int n = blockIdx.y, tid = threadIdx.x;                    // n: the image; grp: its group, where it is image number n - grp * group
  const long long P = sg.P;
  const int grp = n / sg.group;
  const float* lg = logits + (size_t)n * kClasses * P;
  const unsigned char* tg = target + (size_t)n * P;
  u32* k0 = keys + sg.keys_at(grp, 0) + (size_t)(n - grp * sg.group) * P;
  const size_t cstride = (size_t)sg.pixels(grp);
  u32 cnt[kClasses] = {0, 0, 0};
  bool bad = false;
  for (long long i = (long long)blockIdx.x * kKeyThreads + tid; i < P; i += (long long)gridDim.x * kKeyThreads) {
    const float a = lg[i], b = lg[P + i], c = lg[2 * P + i];
    const float m = fmaxf(fmaxf(a, b), c);                 // a NaN logit is skipped here and poisons its exp below
    const float ea = expf(a - m), eb = expf(b - m), ec = expf(c - m);
    const float s = ea + eb + ec;
    const float p[kClasses] = {ea / s, eb / s, ec / s};
    const bool finite = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    bad |= !finite;
    const u32 t = target_class(tg[i]);
#pragma unroll
    for (int cl = 0; cl < kClasses; ++cl) {
      const u32 fg = t == (u32)cl;
      const float e = finite ? fabsf((float)fg - p[cl]) : 0.f;
      k0[cl * cstride + i] = (__float_as_uint(e) << 1) | fg;
      cnt[cl] += fg;
    }
  }
  block_add<kKeyThreads, kClasses>(cnt, G + (size_t)grp * kClasses, [&] {
    if (__syncthreads_or(bad) && tid == 0) flag[grp] = 1u;
  });
}

// per-tile digit histogram: hist[seg][t][d]
__global__ __launch_bounds__(kSortThreads) void lovasz_hist(const u32* __restrict__ keys, Segments sg, int T, int shift,
                                                            u32* __restrict__ hist, const u64* __restrict__ G,
                                                            const u32* __restrict__ flag) {
  const int n = blockIdx.y, seg = n * kClasses + blockIdx.z, t = blockIdx.x;
  const long long P = sg.pixels(n);
  if (segment_idle(G, flag, n, seg) || (long long)t * kTile >= P) return;
  __shared__ u32 h[kRadix];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < kRadix) h[tid] = 0;
  __syncthreads();
  const long long start = (long long)t * kTile;
  const int nt = (int)min((long long)kTile, P - start);
  const u32* src = keys + sg.keys_at(n, blockIdx.z) + start;
#pragma unroll 4
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    const bool valid = idx < nt;
    const u32 d = valid ? digit_of(src[idx], shift) : 0u;
    const u64 peers = digit_peers(d, valid);
    if (valid && (peers & lanes_below(lane)) == 0) atomicAdd(&h[d], (u32)__popcll(peers));
  }
  __syncthreads();
  if (tid < kRadix) hist[((size_t)seg * T + t) * kRadix + tid] = h[tid];
}

// per segment: hist[seg][t][d] <- sum over t' < t of hist[seg][t'][d]; base[seg][d] <- keys of the segment with a digit below d
__global__ __launch_bounds__(kScanThreads) void lovasz_scan(u32* __restrict__ hist, Segments sg, int T, u32* __restrict__ base,
                                                            const u64* __restrict__ G, const u32* __restrict__ flag) {
  const int n = blockIdx.x, seg = n * kClasses + blockIdx.y;
  if (segment_idle(G, flag, n, seg)) return;
  __shared__ u32 gsum[kScanThreads / kRadix][kRadix];
  __shared__ u32 wsum[4];
  const int tid = threadIdx.x, d = tid & (kRadix - 1), g = tid / kRadix;
  constexpr int kGroups = kScanThreads / kRadix;
  const int Tn = sg.tiles(n);                          // the segment's own tiles; T is the stride of hist
  const int per = (Tn + kGroups - 1) / kGroups;
  const int t0 = min(Tn, g * per), t1 = min(Tn, t0 + per);
  u32* h = hist + (size_t)seg * T * kRadix + d;
  u32 sum = 0;
  for (int t = t0; t < t1; ++t) sum += h[(size_t)t * kRadix];
  gsum[g][d] = sum;
  __syncthreads();
  u32 run = 0, total = 0;
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    if (k < g) run += gsum[k][d];
    total += gsum[k][d];
  }
  for (int t = t0; t < t1; ++t) {
    const u32 v = h[(size_t)t * kRadix];
    h[(size_t)t * kRadix] = run;
    run += v;
  }
  const u32 ex = excl_scan_256(total, wsum);
  if (tid < kRadix) base[(size_t)seg * kRadix + d] = ex;
}

// one stable LSD pass of one tile: rank by wave ballots, sort the tile in LDS, write it out in runs of equal digits
__global__ __launch_bounds__(kSortThreads) void lovasz_scatter(const u32* __restrict__ in, u32* __restrict__ out, Segments sg, int T,
                                                               int shift, const u32* __restrict__ hist, const u32* __restrict__ base,
                                                               const u64* __restrict__ G, const u32* __restrict__ flag) {
  const int n = blockIdx.y, seg = n * kClasses + blockIdx.z, t = blockIdx.x;
  const long long P = sg.pixels(n);
  if (segment_idle(G, flag, n, seg) || (long long)t * kTile >= P) return;
  __shared__ u32 sorted[kTile];
  __shared__ u32 cnt[kWaves][kRadix];                 // per wave: digit counts, then the wave's start inside the digit
  __shared__ u32 dstart[kRadix];                      // start of each digit in the sorted tile
  __shared__ u32 gofs[kRadix];                        // segment position of sorted[i] = gofs[digit] + i
  __shared__ u32 wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int k = lane; k < kRadix; k += 64) cnt[w][k] = 0;
  __builtin_amdgcn_wave_barrier();
  const long long start = (long long)t * kTile;
  const int nt = (int)min((long long)kTile, P - start);
  const u32* src = in + sg.keys_at(n, blockIdx.z) + start;

  u32 key[kItems], rank[kItems];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    key[j] = idx < nt ? src[idx] : 0u;
  }
  // input order inside the tile: wave, then item j, then lane -- ranks follow it, so the pass is stable
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    const bool valid = idx < nt;
    const u32 d = digit_of(key[j], shift);
    const u64 peers = digit_peers(d, valid);
    const u32 below = (u32)__popcll(peers & lanes_below(lane));
    const u32 old = cnt[w][d];
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0) cnt[w][d] = old + (u32)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
    rank[j] = old + below;
  }
  __syncthreads();
  u32 total = 0;
  if (tid < kRadix) {
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const u32 v = cnt[k][tid];
      cnt[k][tid] = total;
      total += v;
    }
  }
  const u32 ds = excl_scan_256(total, wsum);
  if (tid < kRadix) {
    dstart[tid] = ds;
    gofs[tid] = base[(size_t)seg * kRadix + tid] + hist[((size_t)seg * T + t) * kRadix + tid] - ds;   // mod 2^32, >= 0 once i is added
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    if (idx < nt) {
      const u32 d = digit_of(key[j], shift);
      sorted[dstart[d] + cnt[w][d] + rank[j]] = key[j];
    }
  }
  __syncthreads();
  u32* dst = out + sg.keys_at(n, blockIdx.z);
  for (int i = tid; i < nt; i += kSortThreads) {
    const u32 k = sorted[i];
    dst[gofs[digit_of(k, shift)] + (u32)i] = k;
  }
}

__device__ __forceinline__ void block_sum_to(u32 v, u32* red /* LDS [kWaves] */, u32* out) {
  const int tid = threadIdx.x;
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    u32 s = 0;
    for (int k = 0; k < kWaves; ++k) s += red[k];
    *out = s;
  }
}

// foreground keys per tile of the sorted segment
__global__ __launch_bounds__(kSortThreads) void lovasz_tile_fg(const u32* __restrict__ keys, Segments sg, int T,
                                                               u32* __restrict__ tile_fg, const u64* __restrict__ G,
                                                               const u32* __restrict__ flag) {
  const int n = blockIdx.y, seg = n * kClasses + blockIdx.z, t = blockIdx.x;
  const long long P = sg.pixels(n);
  if (segment_idle(G, flag, n, seg) || (long long)t * kTile >= P) return;
  __shared__ u32 red[kWaves];
  const long long start = (long long)t * kTile;
  const int nt = (int)min((long long)kTile, P - start);
  const u32* src = keys + sg.keys_at(n, blockIdx.z) + start;
  u32 c = 0;
  for (int i = threadIdx.x; i < nt; i += kSortThreads) c += src[i] & 1u;
  block_sum_to(c, red, &tile_fg[(size_t)seg * T + t]);
}

// f64 partial sum of e_(i) (J_i - J_{i-1}) over one tile of the sorted segment
__global__ __launch_bounds__(kSortThreads) void lovasz_partial(const u32* __restrict__ keys, Segments sg, int T,
                                                               const u32* __restrict__ tile_fg, const u64* __restrict__ G,
                                                               const u32* __restrict__ flag, double* __restrict__ partial) {
  const int n = blockIdx.y, seg = n * kClasses + blockIdx.z, t = blockIdx.x;
  const long long P = sg.pixels(n);
  if (segment_idle(G, flag, n, seg) || (long long)t * kTile >= P) return;
  __shared__ u32 red[kWaves];
  __shared__ u32 wfg[kWaves];
  __shared__ u32 fg_before_tile;
  __shared__ double dred[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  u32 c = 0;
  for (int u = tid; u < t; u += kSortThreads) c += tile_fg[(size_t)seg * T + u];
  block_sum_to(c, red, &fg_before_tile);

  const long long start = (long long)t * kTile;
  const int nt = (int)min((long long)kTile, P - start);
  const u32* src = keys + sg.keys_at(n, blockIdx.z) + start;
  u32 key[kItems];
  u32 mine = 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    key[j] = idx < nt ? src[idx] : 0u;              // 0: not foreground, e = 0
    mine += key[j] & 1u;
  }
  mine = wave_sum(mine);
  if (lane == 0) wfg[w] = mine;
  __syncthreads();
  long long run = fg_before_tile;                    // foreground keys before this wave's first key
  for (int k = 0; k < w; ++k) run += wfg[k];
  const long long g_all = (long long)G[seg];
  const double gd = (double)g_all;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    const u32 g = key[j] & 1u;
    const u64 m = __ballot(g != 0);
    if (idx < nt) {
      const long long i = start + idx;              // position in the sorted segment
      const long long fg_before = run + __popcll(m & lanes_below(lane));
      const long long cum_fg = fg_before + g;
      const double J = 1.0 - (double)(g_all - cum_fg) / (gd + (double)(i + 1 - cum_fg));
      const double Jp = i == 0 ? 0.0 : 1.0 - (double)(g_all - fg_before) / (gd + (double)(i - fg_before));
      acc += (double)__uint_as_float(key[j] >> 1) * (J - Jp);
    }
    run += __popcll(m);
  }
  acc = wave_sum(acc);
  if (lane == 0) dred[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < kWaves; ++k) s += dred[k];
    partial[(size_t)seg * T + t] = s;
  }
}

__global__ __launch_bounds__(64) void lovasz_finish(const double* __restrict__ partial, Segments sg, int T, int S, const u64* __restrict__ G,
                                                    const u32* __restrict__ flag, double* __restrict__ terms) {
  const int seg = blockIdx.x * 64 + threadIdx.x;
  if (seg >= S) return;
  double s = 0.0;
  if (G[seg] == 0)
    s = 0.0;
  else if (flag[seg / kClasses])
    s = __builtin_nan("");
  else {
    const double* p = partial + (size_t)seg * T;
    const int Tn = sg.tiles(seg / kClasses);
    int t = 0;
    for (; t + 8 <= Tn; t += 8) {                     // eight loads in flight, added in tile order
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[t + k];
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; t < Tn; ++t) s += p[t];
  }
  terms[seg] = s;
}

// ---- the gradient (nbc_lovasz_gradient; the definitions: include/nbc.h) ------------------------------------------------------
// prefix[i] = foreground keys before position i of the sorted segment: lovasz_partial's running count, written out
__global__ __launch_bounds__(kSortThreads) void lovasz_fg_prefix(const u32* __restrict__ keys, Segments sg, int T,
                                                                 const u32* __restrict__ tile_fg, const u64* __restrict__ G,
                                                                 const u32* __restrict__ flag, u32* __restrict__ prefix) {
  const int n = blockIdx.y, seg = n * kClasses + blockIdx.z, t = blockIdx.x;
  const long long P = sg.pixels(n);
  if (segment_idle(G, flag, n, seg) || (long long)t * kTile >= P) return;
  __shared__ u32 red[kWaves];
  __shared__ u32 wfg[kWaves];
  __shared__ u32 fg_before_tile;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  u32 c = 0;
  for (int u = tid; u < t; u += kSortThreads) c += tile_fg[(size_t)seg * T + u];
  block_sum_to(c, red, &fg_before_tile);

  const long long start = (long long)t * kTile;
  const int nt = (int)min((long long)kTile, P - start);
  const size_t at = sg.keys_at(n, blockIdx.z) + start;
  u32 fg[kItems];
  u32 mine = 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    fg[j] = idx < nt ? keys[at + idx] & 1u : 0u;
    mine += fg[j];
  }
  mine = wave_sum(mine);
  if (lane == 0) wfg[w] = mine;
  __syncthreads();
  u32 run = fg_before_tile;                          // foreground keys before this wave's first key
  for (int k = 0; k < w; ++k) run += wfg[k];
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const int idx = w * (kItems * 64) + j * 64 + lane;
    const u64 m = __ballot(fg[j] != 0);
    if (idx < nt) prefix[at + idx] = run + (u32)__popcll(m & lanes_below(lane));
    run += (u32)__popcll(m);
  }
}

// J(k, F) = 1 - (G - F) / (G + k - F): the Jaccard loss once k sorted keys are counted, F of them foreground; J(0, 0) = 0
__device__ __forceinline__ double jaccard_at(long long G, long long k, long long F) {
  return 1.0 - (double)(G - F) / ((double)G + (double)(k - F));
}

// One thread per pixel and image.  Per class with a live segment and e > 0: the run of the pixel's key in the sorted segment
// (the lower bound of the three classes in lockstep, its number of rounds fixed by P; the run's end by doubling steps, since a
// run is one key long unless errors tie), the foreground keys before it, the run's mean slope in closed form, d_c = -+ slope /
// C_p.  Then g_k = q_k (d_k - sum_c d_c q_c) with q in f64 (ce_gradient.hpp), times lambda, beside the table's term.
// gw: f64 [N][3][P].  A key that is not where the sort must have put it gives NaN, never a quiet number.
__global__ __launch_bounds__(kKeyThreads) void lovasz_pixel_gradient(const float* __restrict__ logits, const unsigned char* __restrict__ target,
                                                                     const u32* __restrict__ pixel_keys, const u32* __restrict__ sorted,
                                                                     const u32* __restrict__ prefix, const u64* __restrict__ G,
                                                                     const u32* __restrict__ flag, long long P, CeTable T, int has_table,
                                                                     double lambda, double* __restrict__ gw) {
  const long long i = (long long)blockIdx.x * kKeyThreads + threadIdx.x;
  if (i >= P) return;
  const int n = blockIdx.y;
  const size_t img = (size_t)n * kClasses * P;
  const float a = logits[img + i], b = logits[img + P + i], c = logits[img + 2 * P + i];
  double q[3], g[3] = {0.0, 0.0, 0.0};
  pixel_softmax(a, b, c, q);
  if (has_table) pixel_gradient(a, b, c, target[(size_t)n * P + i], T, q, g);
  if (lambda != 0.0) {
    double lov[3];
    if (flag[n]) {
      lov[0] = lov[1] = lov[2] = __builtin_nan("");
    } else {
      long long Gc[kClasses];
      u32 key[kClasses];
      bool need[kClasses];
      int present = 0;
#pragma unroll
      for (int k = 0; k < kClasses; ++k) {
        Gc[k] = (long long)G[n * kClasses + k];
        present += Gc[k] > 0;
        key[k] = pixel_keys[img + (size_t)k * P + i];
        need[k] = Gc[k] > 0 && (key[k] >> 1) != 0u;
      }
      // keys above the pixel's own in the descending segment: the lower bound, three searches side by side
      long long lo[kClasses] = {0, 0, 0};
      for (long long len = P; len > 1;) {
        const long long half = len >> 1;
#pragma unroll
        for (int k = 0; k < kClasses; ++k)
          if (need[k] && sorted[img + (size_t)k * P + lo[k] + half - 1] > key[k]) lo[k] += half;
        len -= half;
      }
      double d[kClasses] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kClasses; ++k) {
        if (!need[k]) continue;
        const u32* s = sorted + img + (size_t)k * P;
        long long r = lo[k];
        r += s[r] > key[k];
        if (r >= P || s[r] != key[k]) {
          d[k] = __builtin_nan("");
          continue;
        }
        long long first = r + 1, last = P;            // the run's end lies in [first, last]
        for (long long step = 1; r + step < P; step <<= 1) {
          if (s[r + step] != key[k]) {
            last = r + step;
            break;
          }
          first = r + step + 1;
        }
        while (first < last) {
          const long long mid = first + ((last - first) >> 1);
          if (s[mid] == key[k]) first = mid + 1; else last = mid;
        }
        const long long run = first - r, F = (long long)prefix[img + (size_t)k * P + r];
        const bool fg = key[k] & 1u;
        const double slope = (jaccard_at(Gc[k], first, F + (fg ? run : 0)) - jaccard_at(Gc[k], r, F)) / (double)run / (double)present;
        d[k] = fg ? -slope : slope;
      }
      const double dot = d[0] * q[0] + d[1] * q[1] + d[2] * q[2];
#pragma unroll
      for (int k = 0; k < kClasses; ++k) lov[k] = q[k] * (d[k] - dot);
    }
#pragma unroll
    for (int k = 0; k < kClasses; ++k) g[k] = has_table ? g[k] + lambda * lov[k] : lambda * lov[k];
  }
  gw[img + i] = g[0];
  gw[img + P + i] = g[1];
  gw[img + 2 * P + i] = g[2];
}

struct Layout {
  size_t keys_a, keys_b, hist, base, tile_fg, partial, flag, total;
};

constexpr const char* kGroupShape = "bad group: 1 <= G <= 64 and g * H * W < 2^31 for the g = min(G, N) images of a group";

inline bool group_ok(int N, int H, int W, int G) {
  return G >= 1 && G <= kMaxGroup && (long long)(G < N ? G : N) * H * W <= 0x7fffffffLL;
}

// byte offsets of the workspace regions (include/nbc.h states the sum); false for a shape the call refuses
bool layout(int N, int H, int W, int G, Layout* L) {
  if (!per_image_shape_ok(N, H, W) || !group_ok(N, H, W, G)) return false;
  const size_t P = (size_t)H * (size_t)W;
  const size_t NG = ((size_t)N + G - 1) / G;           // groups
  const size_t S = (size_t)kClasses * NG, T = ((size_t)(G < N ? G : N) * P + kTile - 1) / kTile;
  Carver ws;
  L->keys_a = ws.take(4 * kClasses * N * P);
  L->keys_b = ws.take(4 * kClasses * N * P);
  L->hist = ws.take(4 * S * T * kRadix);
  L->base = ws.take(4 * S * kRadix);
  L->tile_fg = ws.take(4 * S * T);
  L->partial = ws.take(8 * S * T);
  L->flag = ws.take(4 * NG);
  L->total = ws.offset;
  return true;
}

// the per-image pass is the grouped one with groups of one image.  pixel_keys (nullable; nbc_lovasz_gradient, group = 1): a copy of
// the keys in pixel order [N][3][P], taken before the sort's first pass; the launches around it are the same either way.
int run(const char* who, const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int group, void* workspace_dev,
        size_t workspace_bytes, double* terms_dev, int64_t* fg_counts_dev, void* hip_stream, u32* pixel_keys = nullptr) {
  if (!logits_full_dev || !target_dev || !workspace_dev || !terms_dev || !fg_counts_dev) return fail(who, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W)) return fail(who, NBC_ERR_INVALID, kPerImageShape);
  Layout L;
  if (!layout(N, H, W, group, &L)) return fail(who, NBC_ERR_INVALID, kGroupShape);
  if (int rc = check_workspace(who, workspace_dev, workspace_bytes, L.total)) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  char* ws = static_cast<char*>(workspace_dev);
  u32* keys[2] = {reinterpret_cast<u32*>(ws + L.keys_a), reinterpret_cast<u32*>(ws + L.keys_b)};
  u32* hist = reinterpret_cast<u32*>(ws + L.hist);
  u32* base = reinterpret_cast<u32*>(ws + L.base);
  u32* tile_fg = reinterpret_cast<u32*>(ws + L.tile_fg);
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  u32* flag = reinterpret_cast<u32*>(ws + L.flag);
  u64* G = reinterpret_cast<u64*>(fg_counts_dev);
  const Segments sg{(long long)H * W, N, group};
  const long long P = sg.P;
  const int NG = (N + group - 1) / group, S = kClasses * NG, T = sg.tiles(0);   // the first group is never the short one

  hipError_t e = hipMemsetAsync(G, 0, sizeof(u64) * (size_t)S, s);
  if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(u32) * (size_t)NG, s);
  if (e != hipSuccess) return fail(who, NBC_ERR_HIP, hipGetErrorString(e));
  // about 4 pixels per thread and at most ~4096 blocks over the batch
  long long bx = (P + 4 * kKeyThreads - 1) / (4 * kKeyThreads);
  const long long cap = (4096 + N - 1) / N;
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(lovasz_keys, dim3((unsigned)bx, (unsigned)N), dim3(kKeyThreads), 0, s, logits_full_dev, target_dev, sg, keys[0], G,
                     flag);
  if (pixel_keys) {
    e = hipMemcpyAsync(pixel_keys, keys[0], sizeof(u32) * (size_t)kClasses * N * (size_t)P, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return fail(who, NBC_ERR_HIP, hipGetErrorString(e));
  }
  const dim3 tiles((unsigned)T, (unsigned)NG, (unsigned)kClasses);
  for (int pass = 0; pass < kPasses; ++pass) {
    const int shift = 8 * pass;
    const u32* in = keys[pass & 1];
    u32* out = keys[(pass & 1) ^ 1];
    hipLaunchKernelGGL(lovasz_hist, tiles, dim3(kSortThreads), 0, s, in, sg, T, shift, hist, G, flag);
    hipLaunchKernelGGL(lovasz_scan, dim3((unsigned)NG, (unsigned)kClasses), dim3(kScanThreads), 0, s, hist, sg, T, base, G, flag);
    hipLaunchKernelGGL(lovasz_scatter, tiles, dim3(kSortThreads), 0, s, in, out, sg, T, shift, hist, base, G, flag);
  }
  const u32* sorted = keys[kPasses & 1];             // an even number of passes ends where the keys started
  hipLaunchKernelGGL(lovasz_tile_fg, tiles, dim3(kSortThreads), 0, s, sorted, sg, T, tile_fg, G, flag);
  hipLaunchKernelGGL(lovasz_partial, tiles, dim3(kSortThreads), 0, s, sorted, sg, T, tile_fg, G, flag, partial);
  hipLaunchKernelGGL(lovasz_finish, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, s, partial, sg, T, S, G, flag, terms_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(who, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

struct GradLayout {
  Layout terms;                                        // nbc_lovasz_softmax's regions, first
  size_t pixel_keys, prefix, g, cols, total;
};

// byte offsets of nbc_lovasz_gradient's workspace regions (include/nbc.h states the sum); false for a shape the call refuses
bool grad_layout(int N, int H, int W, int h, int w, GradLayout* L) {
  if (!layout(N, H, W, 1, &L->terms) || h < 1 || w < 1 || h > H || w > W) return false;
  const size_t planes = (size_t)kClasses * N * (size_t)H * (size_t)W;
  Carver ws;
  ws.take(L->terms.total);
  L->pixel_keys = ws.take(4 * planes);
  L->prefix = ws.take(4 * planes);
  L->g = ws.take(8 * planes);
  L->cols = ws.take((size_t)8 * kClasses * N * (size_t)H * w);
  L->total = ws.offset;
  return true;
}

constexpr const char* kWhoGrad = "nbc_lovasz_gradient";

}  // namespace

extern "C" size_t nbc_lovasz_gradient_workspace_bytes(int N, int H, int W, int h, int w) {
  GradLayout L;
  return grad_layout(N, H, W, h, w, &L) ? L.total : 0;
}

extern "C" int nbc_lovasz_gradient(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int h, int w,
                                   const int32_t* row_idx_dev, const float* row_coeff_dev, const int32_t* row_lo_dev,
                                   const int32_t* row_hi_dev, const int32_t* col_idx_dev, const float* col_coeff_dev,
                                   const int32_t* col_lo_dev, const int32_t* col_hi_dev, const double* table9_host, double lovasz_weight,
                                   void* workspace_dev, size_t workspace_bytes, double* terms_dev, int64_t* fg_counts_dev,
                                   double* grad_lowres_dev, uint32_t* keys_dev, double* pixel_grad_dev, void* hip_stream) {
  if (!logits_full_dev || !target_dev || !row_idx_dev || !row_coeff_dev || !row_lo_dev || !row_hi_dev || !col_idx_dev || !col_coeff_dev ||
      !col_lo_dev || !col_hi_dev || !workspace_dev || !terms_dev || !fg_counts_dev || !grad_lowres_dev)
    return fail(kWhoGrad, NBC_ERR_INVALID, "null argument");
  GradLayout L;
  if (!grad_layout(N, H, W, h, w, &L))
    return fail(kWhoGrad, NBC_ERR_INVALID, std::string(kPerImageShape) + ", 1 <= h <= H and 1 <= w <= W");
  if (!std::isfinite(lovasz_weight)) return fail(kWhoGrad, NBC_ERR_INVALID, "lovasz_weight must be finite");
  const BicubicTaps taps{row_idx_dev, row_coeff_dev, row_lo_dev, row_hi_dev, col_idx_dev, col_coeff_dev, col_lo_dev, col_hi_dev};
  if (int rc = check_taps(kWhoGrad, logits_full_dev, taps)) return rc;
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((addr(grad_lowres_dev) | addr(terms_dev) | addr(fg_counts_dev) | addr(pixel_grad_dev)) & 7u)
    return fail(kWhoGrad, NBC_ERR_INVALID, "terms_dev, fg_counts_dev, grad_lowres_dev and pixel_grad_dev must be 8-byte aligned");
  if (addr(keys_dev) & 3u) return fail(kWhoGrad, NBC_ERR_INVALID, "keys_dev must be 4-byte aligned");
  if (int rc = check_workspace(kWhoGrad, workspace_dev, workspace_bytes, L.total)) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  char* ws = static_cast<char*>(workspace_dev);
  u32* pixel_keys = keys_dev ? keys_dev : reinterpret_cast<u32*>(ws + L.pixel_keys);
  u32* prefix = reinterpret_cast<u32*>(ws + L.prefix);
  double* g = pixel_grad_dev ? pixel_grad_dev : reinterpret_cast<double*>(ws + L.g);
  double* cols = reinterpret_cast<double*>(ws + L.cols);
  // the terms: nbc_lovasz_softmax's launches on the first region, the keys copied in pixel order on the way
  if (int rc = run(kWhoGrad, logits_full_dev, target_dev, N, H, W, 1, ws, L.terms.total, terms_dev, fg_counts_dev, hip_stream, pixel_keys))
    return rc;
  const u32* sorted = reinterpret_cast<const u32*>(ws + L.terms.keys_a);   // where run's even number of passes ends
  const u32* tile_fg = reinterpret_cast<const u32*>(ws + L.terms.tile_fg);
  const u32* flag = reinterpret_cast<const u32*>(ws + L.terms.flag);
  const u64* G = reinterpret_cast<const u64*>(fg_counts_dev);
  const Segments sg{(long long)H * W, N, 1};
  const long long P = sg.P;
  const int T = sg.tiles(0);
  CeTable tab{};
  if (table9_host)
    for (int k = 0; k < 9; ++k) tab.t[k] = table9_host[k];
  if (lovasz_weight != 0.0)
    hipLaunchKernelGGL(lovasz_fg_prefix, dim3((unsigned)T, (unsigned)N, (unsigned)kClasses), dim3(kSortThreads), 0, s, sorted, sg, T, tile_fg,
                       G, flag, prefix);
  hipLaunchKernelGGL(lovasz_pixel_gradient, dim3((unsigned)((P + kKeyThreads - 1) / kKeyThreads), (unsigned)N), dim3(kKeyThreads), 0, s,
                     logits_full_dev, target_dev, pixel_keys, sorted, prefix, G, flag, P, tab, table9_host ? 1 : 0, lovasz_weight, g);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = launch_bicubic_adjoint(g, P, N, H, W, h, w, taps, cols, grad_lowres_dev, s);
  if (e != hipSuccess) return fail(kWhoGrad, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}

extern "C" size_t nbc_lovasz_workspace_bytes(int N, int H, int W) {
  Layout L;
  return layout(N, H, W, 1, &L) ? L.total : 0;
}

extern "C" int nbc_lovasz_softmax(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, void* workspace_dev,
                                  size_t workspace_bytes, double* terms_dev, int64_t* fg_counts_dev, void* hip_stream) {
  return run(kWho, logits_full_dev, target_dev, N, H, W, 1, workspace_dev, workspace_bytes, terms_dev, fg_counts_dev, hip_stream);
}

extern "C" size_t nbc_lovasz_groups_workspace_bytes(int N, int H, int W, int G) {
  Layout L;
  return layout(N, H, W, G, &L) ? L.total : 0;
}

extern "C" int nbc_lovasz_softmax_groups(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int G,
                                         void* workspace_dev, size_t workspace_bytes, double* terms_dev, int64_t* counts_dev,
                                         void* hip_stream) {
  return run(kWhoGroups, logits_full_dev, target_dev, N, H, W, G, workspace_dev, workspace_bytes, terms_dev, counts_dev, hip_stream);
}
