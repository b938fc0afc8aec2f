// remove_small_zones on the GPU: the reference's src/bark_calculator/utils.py:135-148, called at
// models.py:271 between the argmax and the statistics.  Byte/index work, bound by HBM/L2 traffic.
//
// With m = (labels == 0) (the "Nothing" mask), skimage semantics (connectivity=2 = 8-neighbourhood):
//   1. remove_small_holes(m, 150):   8-connected components of ~m smaller than 150 px join m;
//   2. remove_small_objects(m, 150): 8-connected components of the filled m smaller than 150 px leave m;
//   3. pixels that left m and were class 0 become class 1; pixels that joined m become class 0.
// Both steps are "label the 8-connected components of a binary mask, drop the small ones".  The labelling is
// components.hpp's with one class (label_tile in LDS, then the border kernels on global memory); around it:
//   tile_label     writes the Nothing mask (phase 0) and counts the pixels of every tile-local root;
//   sum_sizes      every tile-local root adds its tile's pixel count to its final root;
//   apply          components below the threshold flip in the mask.
// The result (which pixels flip) depends only on component sizes, which are exact integers, so the
// output equals the CPU restatement (scipy.ndimage.label) bit for bit.
#include "components.hpp"
#include "nbc_kernels.hpp"
#include "reduce.hpp"

namespace nbc {
namespace {

constexpr int TILE = kLabelTile;

// phase 0: mask = (label != 0) is labelled ("holes" of the Nothing mask); phase 1: mask = bg.
// bg[] holds the Nothing mask (1 = background); written here in phase 0.
template <typename LabelT>
__global__ __launch_bounds__(TILE* TILE) void tile_label_kernel(const LabelT* __restrict__ labels, unsigned char* __restrict__ bg,
                                                                 int* __restrict__ parent, int* __restrict__ size,
                                                                 int H, int W, int phase) {
  __shared__ int s[TILE * TILE];
  __shared__ int cnt[TILE * TILE];
  __shared__ unsigned char sc[TILE * TILE];
  const int t = threadIdx.x;
  const int x = blockIdx.x * TILE + (t & (TILE - 1)), y = blockIdx.y * TILE + (t >> 5);
  const size_t img = (size_t)blockIdx.z * H * W;
  const bool inside = x < W && y < H;
  const int p = y * W + x;
  int m = 0;
  if (inside) {
    if (phase == 0) {
      m = labels[img + p] != 0;
      bg[img + p] = m ? 0 : 1;
    } else {
      m = bg[img + p] != 0;
    }
  }
  cnt[t] = 0;
  const int r = label_tile(m, s, sc);
  // pixels per tile-local root, one LDS atomic per distinct root per wave
  for_each_key(r >= 0, r, [&](int root, unsigned long long same) { atomicAdd(&cnt[root], (int)__popcll(same)); });
  __syncthreads();
  if (inside) {
    parent[img + p] = m ? (blockIdx.y * TILE + (r >> 5)) * W + blockIdx.x * TILE + (r & (TILE - 1)) : -1;   // index inside the image
    size[img + p] = r == t ? cnt[t] : 0;      // non-zero exactly at the tile-local roots
  }
}

// Component sizes: tile_label_kernel left the pixel count of every tile-local root in size[]; a local
// root that was linked under another root adds its count to its final root.  Only the (few thousand)
// local roots do anything here; their atomics spread over as many final roots as there are components.
__global__ void sum_sizes_kernel(int* __restrict__ parent, int* __restrict__ size, int H, int W) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  int* L = parent + (size_t)blockIdx.z * H * W;
  int* S = size + (size_t)blockIdx.z * H * W;
  const int p = y * W + x;
  const int mine = S[p];
  if (mine == 0) return;                      // not a tile-local root
  const int r = find_root(L, p);              // no links change any more: r is the component's root
  if (r != p) atomicAdd(&S[r], mine);
}

// phase 0: small components of ~bg join bg.  phase 1: small components of bg leave it, then the labels
// are rewritten (utils.py:145-146), optionally remapped 2 -> 1 (models.py:273-276) and counted.
template <typename LabelT>
__global__ void apply_kernel(LabelT* __restrict__ labels, unsigned char* __restrict__ bg, const int* __restrict__ parent,
                             const int* __restrict__ size, int H, int W, int min_pixels, int phase, int exclude_nodes,
                             unsigned long long* __restrict__ counts) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  const size_t img = (size_t)blockIdx.z * H * W;
  unsigned c1 = 0, c2 = 0;
  if (x < W) {
    const size_t q = img + (size_t)y * W + x;
    // parent[q] is the pixel's tile-local root (or, after pointer jumping, an ancestor of it): walk the
    // few remaining hops to the component's root, read-only
    int r = parent[q];
    if (r >= 0) {
      const int* L = parent + img;
      int up = L[r];
      while (up != r) { r = up; up = L[r]; }
    }
    const bool small = r >= 0 && size[img + r] < min_pixels;
    if (phase == 0) {
      if (small) bg[q] = 1;
    } else {
      const bool kept = bg[q] != 0 && !small;
      int v = (int)labels[q];
      if (!kept && v == 0) v = 1;
      if (kept && v != 0) v = 0;
      if (exclude_nodes && v == 2) v = 1;
      labels[q] = (LabelT)v;
      c1 = v == 1; c2 = v == 2;
    }
  }
  if (phase == 1 && counts) {              // one global atomic per class and block
    __shared__ unsigned blk[2];
    if (threadIdx.x < 2) blk[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      c1 += __shfl_xor(c1, off, 64);
      c2 += __shfl_xor(c2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      if (c1) atomicAdd(&blk[0], c1);
      if (c2) atomicAdd(&blk[1], c2);
    }
    __syncthreads();
    if (threadIdx.x < 2 && blk[threadIdx.x])
      atomicAdd(&counts[(size_t)blockIdx.z * 3 + 1 + threadIdx.x], (unsigned long long)blk[threadIdx.x]);
  }
}

__global__ void finish_counts_kernel(unsigned long long* counts, int N, unsigned long long pixels) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
    counts[(size_t)i * 3] = pixels - counts[(size_t)i * 3 + 1] - counts[(size_t)i * 3 + 2];
}

template <typename LabelT>
hipError_t run(LabelT* labels, int N, int H, int W, int min_pixels, int exclude_nodes, unsigned char* bg, int* parent,
               int* size, unsigned long long* counts, hipStream_t s) {
  const dim3 tiles((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, N);
  const dim3 rows((W + 255) / 256, H, N);
  if (counts) {
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 3 * N, s);
    if (e != hipSuccess) return e;
  }
  for (int phase = 0; phase < 2; ++phase) {
    hipLaunchKernelGGL(tile_label_kernel<LabelT>, tiles, dim3(TILE * TILE), 0, s, labels, bg, parent, size, H, W, phase);
    if (phase == 0) launch_borders(parent, ZeroIsSet{bg}, N, H, W, s);      // the mask is ~bg, then bg
    else launch_borders(parent, ClassPlane{bg}, N, H, W, s);
    hipLaunchKernelGGL(sum_sizes_kernel, rows, dim3(256), 0, s, parent, size, H, W);
    hipLaunchKernelGGL(apply_kernel<LabelT>, rows, dim3(256), 0, s, labels, bg, parent, size, H, W, min_pixels, phase,
                       exclude_nodes, counts);
  }
  if (counts) hipLaunchKernelGGL(finish_counts_kernel, dim3((N + 255) / 256), dim3(256), 0, s, counts, N, (unsigned long long)H * W);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_remove_small_zones(void* labels, int labels_i64, int N, int H, int W, int min_pixels, int exclude_nodes,
                                     unsigned char* bg, int* parent, int* size, unsigned long long* counts, hipStream_t s) {
  if (!per_image_shape_ok(N, H, W) || H > 65535) return hipErrorInvalidValue;      // grid.y carries the row
  if (labels_i64) return run(static_cast<long long*>(labels), N, H, W, min_pixels, exclude_nodes, bg, parent, size, counts, s);
  return run(static_cast<unsigned char*>(labels), N, H, W, min_pixels, exclude_nodes, bg, parent, size, counts, s);
}

}  // namespace nbc
