// The operating-point sweep on the device: the 3 x 3 confusion of the label map at every point of a grid of (bark offset, node
// offset) pairs, from one pass over the full-resolution logits.  The definition (include/nbc.h): the decision at
// (bark[i], node[j]) is k = argmax3(x0, x1 + bark[i], x2 + node[j]) -- one f32 addition each, argmax3 of reduce.hpp -- and
// conf[n][i][j][t][p] counts the pixels of image n with target class t and decision p.  Integer from the comparison on.
//
// The switch-index form.  For a pixel and an i, a = argmax(x0, x1 + bark[i]) (the first step of argmax3) leaves the running
// maximum bv, and class 2 wins at j exactly when (x2 + node[j] > bv) or (x2 is a NaN and bv is not).  f32 addition is
// monotone in the addend and the node offsets ascend, so the predicate is false up to some index s and true from there on
// (constant for a NaN or infinite x2): the decision along j is a for j < s and 2 for j >= s, with s in 0..G2.  The kernel
// therefore counts one (t, a, s) per (pixel, i) instead of G2 decisions.
//
//   sweep_partial  one block per (tile of 4096 pixels, image), the pixel-to-lane map and the loads of softmax_census.hip.  A
//                  pixel's G2 sums x2 + node[j] are made once and held in registers (the node offsets are kernel arguments
//                  read at constant indices, padded with -inf up to the instantiation's kJ, which no comparison passes); per
//                  i it costs the bark addition, kJ compares and ONE integer LDS atomic into hist[i][t][a][s], u32 words,
//                  G1 * 6 * (G2 + 1) of them: 26 928 bytes at the full grid.  s = G2 - (number of j that pass).  The block
//                  writes its tile's table to the workspace as 16-bit counts (<= 4096), two to a word.
//                  kJ = 33, or 1 for G2 == 1 (a sweep of the bark offset alone compares once, not 33 times).
//   sweep_finish   one block per (i, image): eight slices of the tiles side by side, added through LDS in u64; a running sum
//                  along s gives C[t][a][j] = pixels with s <= j, and conf[i][j][t][2] = C[t][0][j] + C[t][1][j],
//                  conf[i][j][t][a] = total[t][a] - C[t][a][j].
// No float atomics, no memset, no global atomics, no library besides the HIP runtime.
#include <hip/hip_runtime.h>

#include <cmath>

#include "reduce.hpp"

using namespace nbc;

namespace {

using u32 = unsigned;
using u64 = unsigned long long;

constexpr int kThreads = 256;                           // 4 waves
constexpr int kGroup = 4;                               // consecutive pixels per load group
constexpr int kGroups = 4;                              // groups per thread and tile
constexpr int kTile = kThreads * kGroup * kGroups;      // 4096 pixels per tile
constexpr int kMaxG = NBC_SWEEP_MAX_GRID;               // 33
constexpr int kFinishLanes = 128, kFinishSlices = 8;    // packed words of an i-row (<= 3 * 34 = 102) x slices of the tiles
constexpr int kFinishThreads = kFinishLanes * kFinishSlices;
constexpr const char* kWho = "nbc_offset_sweep";
static_assert(kTile <= 65535, "a tile's count must fit 16 bits");
static_assert(3 * (kMaxG + 1) <= kFinishLanes, "an i-row's packed words must fit the finish block's lanes");

// the grid as the kernels take it: kernel arguments.  node[j] for j >= G2 is -inf: x2 + (-inf) is -inf or a NaN, which is
// greater than nothing
struct Offsets {
  float bark[kMaxG];
  float node[kMaxG];
};

// one pixel into the LDS table: G1 atomics
template <int kJ>
__device__ __forceinline__ void add_pixel(float x0, float x1, float x2, u32 t, int G1, int G2, const Offsets& off,
                                          const float* __restrict__ bark, u32* __restrict__ hist) {
  float c[kJ];
#pragma unroll
  for (int j = 0; j < kJ; ++j) c[j] = __fadd_rn(x2, off.node[j]);
  const bool x2_nan = x2 != x2;
  const int S = G2 + 1;
  u32* row = hist + t * 2u * (u32)S;
  for (int i = 0; i < G1; ++i) {
    const float b = __fadd_rn(x1, bark[i]);
    const bool one = (b > x0) || (b != b && x0 == x0);            // argmax3's first step
    const float bv = one ? b : x0;
    int pass = 0;
#pragma unroll
    for (int j = 0; j < kJ; ++j) pass += c[j] > bv ? 1 : 0;
    const int s = x2_nan ? (bv == bv ? 0 : G2) : G2 - pass;        // argmax3's second step, at every j at once
    atomicAdd(&row[(one ? S : 0) + s], 1u);
    row += 6 * S;
  }
}

template <int kJ>
__global__ __launch_bounds__(kThreads) void sweep_partial(const float* __restrict__ logits, const unsigned char* __restrict__ target,
                                                          long long P, int T, int G1, int G2, const Offsets off,
                                                          u32* __restrict__ part) {
  __shared__ u32 hist[kMaxG * 6 * (kJ + 1)];
  __shared__ float bark[kMaxG];
  const int n = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int words = G1 * 6 * (G2 + 1);                   // <= kMaxG * 6 * (kJ + 1): the host picks kJ >= G2
  for (int i = tid; i < words; i += kThreads) hist[i] = 0u;
  if (tid < kMaxG) bark[tid] = off.bark[tid];
  __syncthreads();

  const float* l0 = logits + (size_t)n * 3 * P;
  const float* l1 = l0 + P;
  const float* l2 = l1 + P;
  const unsigned char* tg = target + (size_t)n * P;
  // group starts are multiples of 4 pixels: they keep whatever alignment the image's planes start with
  const bool vec = ((reinterpret_cast<uintptr_t>(l0) | reinterpret_cast<uintptr_t>(l1) | reinterpret_cast<uintptr_t>(l2)) & 15u) == 0 &&
                   (reinterpret_cast<uintptr_t>(tg) & 3u) == 0;
  const long long start = (long long)tile * kTile;

#pragma unroll 1
  for (int g = 0; g < kGroups; ++g) {
    const long long q = start + (long long)(g * kThreads + tid) * kGroup;
    if (q >= P) continue;
    float a[kGroup], b[kGroup], c[kGroup];
    u32 t[kGroup];
    const int left = (int)(P - q < kGroup ? P - q : kGroup);
    if (vec && left == kGroup) {
      const float4 va = *reinterpret_cast<const float4*>(l0 + q);
      const float4 vb = *reinterpret_cast<const float4*>(l1 + q);
      const float4 vc = *reinterpret_cast<const float4*>(l2 + q);
      const u32 vt = *reinterpret_cast<const u32*>(tg + q);
      a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
      b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
      c[0] = vc.x; c[1] = vc.y; c[2] = vc.z; c[3] = vc.w;
      t[0] = vt & 255u; t[1] = (vt >> 8) & 255u; t[2] = (vt >> 16) & 255u; t[3] = vt >> 24;
    } else {
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        const long long at = k < left ? q + k : q;          // a pixel inside the image; the copies are not counted
        a[k] = l0[at]; b[k] = l1[at]; c[k] = l2[at];
        t[k] = tg[at];
      }
    }
#pragma unroll
    for (int k = 0; k < kGroup; ++k)
      if (k < left) add_pixel<kJ>(a[k], b[k], c[k], target_class(t[k]), G1, G2, off, bark, hist);
  }
  __syncthreads();

  u32* out = part + ((size_t)n * T + tile) * (size_t)(words / 2);
  for (int i = tid; i < words / 2; i += kThreads) out[i] = hist[2 * i] | (hist[2 * i + 1] << 16);
}

// one block per (i, image): thread (w, g) adds packed word w of the i-row over tiles g, g + 8, ..., then the slices through
// LDS; the running sum along s and the nine cells of every j.  Integer sums: the order reaches nothing.
__global__ __launch_bounds__(kFinishThreads) void sweep_finish(const u32* __restrict__ part, int T, int G1, int G2,
                                                               u64* __restrict__ conf) {
  __shared__ u64 acc[kFinishSlices][2 * kFinishLanes];
  __shared__ u64 cell[2 * kFinishLanes];
  const int tid = threadIdx.x, w = tid % kFinishLanes, g = tid / kFinishLanes;
  const int i = blockIdx.x, n = blockIdx.y;
  const int S = G2 + 1, RW = 3 * S;                      // packed words of an i-row
  const size_t W2 = (size_t)G1 * RW;                     // packed words of a tile
  u64 lo = 0, hi = 0;
  if (w < RW) {
    const u32* p = part + (size_t)n * T * W2 + (size_t)i * RW + w;
#pragma unroll 4
    for (int t = g; t < T; t += kFinishSlices) {
      const u32 v = p[(size_t)t * W2];
      lo += v & 0xffffu;
      hi += v >> 16;
    }
  }
  acc[g][2 * w] = lo;
  acc[g][2 * w + 1] = hi;
  __syncthreads();
  if (tid < 2 * RW) {
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < kFinishSlices; ++k) s += acc[k][tid];
    cell[tid] = s;
  }
  __syncthreads();
  if (tid < 6) {                                          // (t, a): pixels with switch index <= s; the last is the total
    u64 run = 0;
    for (int s = 0; s < S; ++s) {
      run += cell[tid * S + s];
      cell[tid * S + s] = run;
    }
  }
  __syncthreads();
  u64* out = conf + ((size_t)n * G1 + i) * (size_t)G2 * 9;
  for (int idx = tid; idx < G2 * 9; idx += kFinishThreads) {
    const int j = idx / 9, r = idx - j * 9, t = r / 3, p = r - t * 3;
    const u64 c0 = cell[(t * 2) * S + j], c1 = cell[(t * 2 + 1) * S + j];
    const u64 n0 = cell[(t * 2) * S + G2], n1 = cell[(t * 2 + 1) * S + G2];
    out[idx] = p == 2 ? c0 + c1 : p == 0 ? n0 - c0 : n1 - c1;
  }
}

bool grid_ok(int G) { return G >= 1 && G <= kMaxG; }

// the workspace (include/nbc.h states the formula): per image and tile G1 * 6 * (G2 + 1) 16-bit counts
bool layout(int N, int H, int W, int G1, int G2, size_t* total, int* T) {
  if (!per_image_shape_ok(N, H, W) || !grid_ok(G1) || !grid_ok(G2)) return false;
  const size_t P = (size_t)H * (size_t)W;
  const size_t tiles = (P + kTile - 1) / kTile;
  Carver ws;
  ws.take(12 * (size_t)G1 * (size_t)(G2 + 1) * (size_t)N * tiles);
  *total = ws.offset;
  *T = (int)tiles;
  return true;
}

// finite and strictly ascending
bool list_ok(const float* v, int G) {
  for (int i = 0; i < G; ++i)
    if (!std::isfinite(v[i]) || (i > 0 && !(v[i] > v[i - 1]))) return false;
  return true;
}

}  // namespace

extern "C" size_t nbc_offset_sweep_workspace_bytes(int N, int H, int W, int G1, int G2) {
  size_t total;
  int T;
  return layout(N, H, W, G1, G2, &total, &T) ? total : 0;
}

extern "C" int nbc_offset_sweep(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W,
                                const float* bark_offsets_host, int G1, const float* node_offsets_host, int G2, void* workspace_dev,
                                size_t workspace_bytes, uint64_t* conf_dev, void* hip_stream) {
  if (!logits_full_dev || !target_dev || !bark_offsets_host || !node_offsets_host || !workspace_dev || !conf_dev)
    return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W)) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  if (!grid_ok(G1) || !grid_ok(G2)) return fail(kWho, NBC_ERR_INVALID, "G1 and G2 must lie in 1..33");
  if (!list_ok(bark_offsets_host, G1) || !list_ok(node_offsets_host, G2))
    return fail(kWho, NBC_ERR_INVALID, "the offsets must be finite and strictly ascending");
  size_t total;
  int T;
  layout(N, H, W, G1, G2, &total, &T);
  if (int rc = check_workspace(kWho, workspace_dev, workspace_bytes, total)) return rc;
  Offsets off;
  for (int i = 0; i < kMaxG; ++i) {
    off.bark[i] = i < G1 ? bark_offsets_host[i] : 0.f;
    off.node[i] = i < G2 ? node_offsets_host[i] : -INFINITY;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  u32* part = static_cast<u32*>(workspace_dev);
  const long long P = (long long)H * W;
  const dim3 grid((unsigned)T, (unsigned)N);
  if (G2 == 1) hipLaunchKernelGGL(sweep_partial<1>, grid, dim3(kThreads), 0, s, logits_full_dev, target_dev, P, T, G1, G2, off, part);
  else hipLaunchKernelGGL(sweep_partial<kMaxG>, grid, dim3(kThreads), 0, s, logits_full_dev, target_dev, P, T, G1, G2, off, part);
  hipLaunchKernelGGL(sweep_finish, dim3((unsigned)G1, (unsigned)N), dim3(kFinishThreads), 0, s, part, T, G1, G2,
                     reinterpret_cast<u64*>(conf_dev));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
