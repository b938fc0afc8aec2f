// Per-image census of the softmax confidence on the device: what a reliability table, the expected calibration error, the
// Brier score, the one-vs-rest precision/recall curves and the soft Jaccard (the quantity the reference's JaccardLoss,
// bark_calculator/utils.py:168-182, is named after) need from the pixels, and the confidence plane of the plain forward.
// The definition (include/nbc.h) is integer from the quantisation on: per pixel with three finite logits, in f64 from the
// f32 logits, m = max, e_c = exp(x_c - m), s = (e_0 + e_1) + e_2, p_c = e_c / s, q_c = min(65535, floor(p_c * 65536));
// k = argmax3 (the forward's own rule), t the target class (0 without a target), hit = (k == t) (1 without a target).  A
// pixel with a NaN or infinite logit counts in `nonfinite` alone and gets confidence byte 0.  Per image one row of
// NBC_CENSUS_WORDS u64: H[t][c][q_c >> 8], R[hit][q_k >> 8], RS[hit][q_k >> 8] += q_k, M[t][c] += q_c,
// B[t] += sum_c (q_c - 65536 [c == t])^2, nonfinite.  Only integers are added, so no order reaches the result.
//
//   census_partial  one block per (tile of 4096 pixels, image), the pixel-to-lane map and the loads of pixel_ce.hip (a
//                   thread owns four groups of four consecutive pixels; 16-byte loads where the planes allow them).  The
//                   histograms live in LDS as u32 words, filled by integer LDS atomics -- except the end bins.  A trained
//                   network puts p_node in bin 0 and p_nothing / p_bark in bin 0 or 255 on almost every pixel, and the
//                   winner's confidence in bin 255: 64 lanes adding to one LDS word would serialise.  Bins 0 and 255 of H
//                   and bin 255 of R / RS therefore stay in the thread's registers (7-bit packed counters as in
//                   pixel_ce.hip: a thread sees 16 pixels), like M, B and nonfinite, which every pixel feeds; they go
//                   through wave_sum and reach LDS as one add per wave.  The block then writes its tile's partial row to
//                   the workspace in narrow words: a count fits 16 bits (<= 4096), a q sum 32 bits (<= 4096 * 65535), a
//                   Brier sum needs 64 (< 4096 * 2^33).
//   census_finish   one block per (32 words, image): eight slices of the tiles side by side, then added through LDS.
// No float atomics, no memset, no global atomics, no library besides the HIP runtime.
#include <hip/hip_runtime.h>

#include <cmath>

#include "softmax_census.hpp"

using namespace nbc;
using namespace nbc::census;

namespace {

constexpr int kFinishWords = 32, kFinishSlices = 8;
constexpr int kFinishThreads = kFinishWords * kFinishSlices;
constexpr const char* kWho = "nbc_softmax_census";

// one block per (32 words of the row, image): thread (w, g) adds word w of tiles g, g + 8, ..., the loads of a round
// independent of each other; then the eight slices through LDS.  Integer sums: the order reaches nothing.
__global__ __launch_bounds__(kFinishThreads) void census_finish(const u32* __restrict__ part_cnt, const u32* __restrict__ part_sum,
                                                                const u64* __restrict__ part_brier, int T, u64* __restrict__ rows) {
  __shared__ u64 part[kFinishSlices][kFinishWords];
  const int w = threadIdx.x % kFinishWords, g = threadIdx.x / kFinishWords;
  const int word = blockIdx.x * kFinishWords + w, n = blockIdx.y;
  const size_t first = (size_t)n * T;
  u64 s = 0;
  if (word < kCounts) {
    const u32* p = part_cnt + first * (kCounts / 2) + (word >> 1);
    const u32 shift = (word & 1) * 16;
#pragma unroll 4
    for (int t = g; t < T; t += kFinishSlices) s += (p[(size_t)t * (kCounts / 2)] >> shift) & 0xffffu;
  } else if (word < NBC_CENSUS_B || word == NBC_CENSUS_NONFINITE) {
    const int k = word == NBC_CENSUS_NONFINITE ? kSumNonfinite : word - kCounts;   // RS and M follow each other in both
    const u32* p = part_sum + first * kSums + k;
#pragma unroll 4
    for (int t = g; t < T; t += kFinishSlices) s += p[(size_t)t * kSums];
  } else if (word < NBC_CENSUS_WORDS) {
    const u64* p = part_brier + first * kBrier + (word - NBC_CENSUS_B);
#pragma unroll 4
    for (int t = g; t < T; t += kFinishSlices) s += p[(size_t)t * kBrier];
  }
  part[g][w] = s;
  __syncthreads();
  if (g == 0 && word < NBC_CENSUS_WORDS) {
#pragma unroll
    for (int k = 1; k < kFinishSlices; ++k) s += part[k][w];
    rows[(size_t)n * NBC_CENSUS_WORDS + word] = s;
  }
}

struct Layout {
  size_t part_cnt, part_sum, part_brier, total;
  int T;
};

// byte offsets of the workspace regions (include/nbc.h states the sum); false for a shape the call refuses
bool layout(int N, int H, int W, Layout* L) {
  if (!per_image_shape_ok(N, H, W)) return false;
  const size_t P = (size_t)H * (size_t)W;
  const size_t T = (P + kTile - 1) / kTile, S = (size_t)N * T;
  Carver ws;
  L->part_cnt = ws.take(2 * (size_t)kCounts * S);
  L->part_sum = ws.take(4 * (size_t)kSums * S);
  L->part_brier = ws.take(8 * (size_t)kBrier * S);
  L->total = ws.offset;
  L->T = (int)T;
  return true;
}

}  // namespace

extern "C" size_t nbc_softmax_census_workspace_bytes(int N, int H, int W) {
  Layout L;
  return layout(N, H, W, &L) ? L.total : 0;
}

extern "C" int nbc_softmax_census(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, void* workspace_dev,
                                  size_t workspace_bytes, uint64_t* rows_dev, uint8_t* confidence_dev, void* hip_stream) {
  if (!logits_full_dev || !workspace_dev || !rows_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  Layout L;
  if (!layout(N, H, W, &L)) return fail(kWho, NBC_ERR_INVALID, kPerImageShape);
  if (int rc = check_workspace(kWho, workspace_dev, workspace_bytes, L.total)) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  char* ws = static_cast<char*>(workspace_dev);
  u32* part_cnt = reinterpret_cast<u32*>(ws + L.part_cnt);
  u32* part_sum = reinterpret_cast<u32*>(ws + L.part_sum);
  u64* part_brier = reinterpret_cast<u64*>(ws + L.part_brier);
  const long long P = (long long)H * W;
  hipLaunchKernelGGL(census_partial<true>, dim3((unsigned)L.T, (unsigned)N), dim3(kThreads), 0, s, logits_full_dev, target_dev, confidence_dev,
                     P, L.T, part_cnt, part_sum, part_brier);
  hipLaunchKernelGGL(census_finish, dim3((NBC_CENSUS_WORDS + kFinishWords - 1) / kFinishWords, (unsigned)N), dim3(kFinishThreads), 0,
                     s, part_cnt, part_sum, part_brier, L.T, reinterpret_cast<u64*>(rows_dev));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(kWho, NBC_ERR_HIP, hipGetErrorString(e));
  return NBC_OK;
}
