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
//
// Grouped (nbc_remove_small_zones_groups): the reference's PixelWiseF1 hands the [B,H,W] argmax of a batch to the same
// function (utils.py:211-214), and skimage's connectivity=2 on a 3-D array is generate_binary_structure(3, 2): besides the
// 8 neighbours inside its image, a pixel (b, y, x) touches (b +- 1, y, x) and the four edge neighbours of that pixel.  So G
// consecutive images form one volume (components.hpp: Volume) whose parents share one index space, and
//   link_images    one launch per phase, after the border kernels: the set pixels of an image that is not the first of
//                  its group make the links to the image before it;
// sum_sizes and apply then see components that span images.  G = 1 launches nothing more and is the per-image pass.
#include "components.hpp"
#include "nbc_ctx.hpp"
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
                                                                 int H, int W, int G, int phase) {
  __shared__ int s[TILE * TILE];
  __shared__ int cnt[TILE * TILE];
  __shared__ unsigned char sc[TILE * TILE];
  const int t = threadIdx.x;
  const int x = blockIdx.x * TILE + (t & (TILE - 1)), y = blockIdx.y * TILE + (t >> 5);
  const Volume vol(blockIdx.z, G, H, W);
  const size_t img = vol.image();
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
    parent[img + p] = m ? vol.off + (blockIdx.y * TILE + (r >> 5)) * W + blockIdx.x * TILE + (r & (TILE - 1)) : -1;   // index inside the volume
    size[img + p] = r == t ? cnt[t] : 0;      // non-zero exactly at the tile-local roots
  }
}

// Component sizes: tile_label_kernel left the pixel count of every tile-local root in size[]; a local
// root that was linked under another root adds its count to its final root.  Only the (few thousand)
// local roots do anything here; their atomics spread over as many final roots as there are components.
__global__ void sum_sizes_kernel(int* __restrict__ parent, int* __restrict__ size, int H, int W, int G) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const Volume vol(blockIdx.z, G, H, W);
  int* L = parent + vol.base;
  int* S = size + vol.base;
  const int p = vol.off + y * W + x;
  const int mine = S[p];
  if (mine == 0) return;                      // not a tile-local root
  const int r = find_root(L, p);              // no links change any more: r is the component's root
  if (r != p) atomicAdd(&S[r], mine);
}

// The links between consecutive images of a group, for the mask `set` (ZeroIsSet or ClassPlane of bg).  Where a pixel and
// the pixel at its place in the image before are both set (the two "overlap"), they belong together -- but only the first
// pixel of an overlap makes that union: one whose W or N neighbour overlaps as well is joined to that neighbour inside both
// images, and the neighbour (or the one it defers to) makes the link.  So the unions of a large zone that stays in place
// from image to image are as many as its overlap has upper-left corners, not as many as it has pixels.  Where the pixel
// before is not set: for each of the four edge directions, a union with the pixel before at that neighbour's place when
// it is set and the pixel's own neighbour there is not -- a set neighbour overlaps there and is joined to the pixel
// inside the image already.
template <typename ClassOf>
__global__ void link_images_kernel(int* __restrict__ parent, ClassOf set, int H, int W, int G) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  const Volume vol(blockIdx.z, G, H, W);
  if (x >= W || vol.off == 0) return;         // the first image of a group has none before it
  const size_t img = vol.image(), before = img - (size_t)H * W;
  const int p = y * W + x, P = H * W;
  if (!set(img + p)) return;
  int* L = parent + vol.base;
  const int v = vol.off + p;
  const auto overlaps = [&](int q) { return set(img + q) && set(before + q); };
  if (set(before + p)) {
    if (!(x > 0 && overlaps(p - 1)) && !(y > 0 && overlaps(p - W))) unite(L, v, v - P);
    return;
  }
  const auto side = [&](bool in_image, int d) {
    if (in_image && !set(img + p + d) && set(before + p + d)) unite(L, v, v - P + d);
  };
  side(x > 0, -1);
  side(x < W - 1, 1);
  side(y > 0, -W);
  side(y < H - 1, W);
}

// phase 0: small components of ~bg join bg.  phase 1: small components of bg leave it, then the labels
// are rewritten (utils.py:145-146), optionally remapped 2 -> 1 (models.py:273-276) and counted.
template <typename LabelT>
__global__ void apply_kernel(LabelT* __restrict__ labels, unsigned char* __restrict__ bg, const int* __restrict__ parent,
                             const int* __restrict__ size, int H, int W, int G, int min_pixels, int phase, int exclude_nodes,
                             unsigned long long* __restrict__ counts) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  const Volume vol(blockIdx.z, G, H, W);
  const size_t img = vol.image();
  unsigned c1 = 0, c2 = 0;
  if (x < W) {
    const size_t q = img + (size_t)y * W + x;
    // parent[q] is the pixel's tile-local root (or, after pointer jumping, an ancestor of it): walk the
    // few remaining hops to the component's root, read-only
    int r = parent[q];
    if (r >= 0) {
      const int* L = parent + vol.base;
      int up = L[r];
      while (up != r) { r = up; up = L[r]; }
    }
    const bool small = r >= 0 && size[vol.base + r] < min_pixels;
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
hipError_t run(LabelT* labels, int N, int H, int W, int G, int min_pixels, int exclude_nodes, unsigned char* bg, int* parent,
               int* size, unsigned long long* counts, hipStream_t s) {
  const dim3 tiles((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, N);
  const dim3 rows((W + 255) / 256, H, N);
  if (counts) {
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 3 * N, s);
    if (e != hipSuccess) return e;
  }
  for (int phase = 0; phase < 2; ++phase) {
    hipLaunchKernelGGL(tile_label_kernel<LabelT>, tiles, dim3(TILE * TILE), 0, s, labels, bg, parent, size, H, W, G, phase);
    if (phase == 0) {                                                        // the mask is ~bg, then bg
      launch_borders(parent, ZeroIsSet{bg}, N, H, W, s, G);
      if (G > 1 && N > 1) hipLaunchKernelGGL(link_images_kernel<ZeroIsSet>, rows, dim3(256), 0, s, parent, ZeroIsSet{bg}, H, W, G);
    } else {
      launch_borders(parent, ClassPlane{bg}, N, H, W, s, G);
      if (G > 1 && N > 1) hipLaunchKernelGGL(link_images_kernel<ClassPlane>, rows, dim3(256), 0, s, parent, ClassPlane{bg}, H, W, G);
    }
    hipLaunchKernelGGL(sum_sizes_kernel, rows, dim3(256), 0, s, parent, size, H, W, G);
    hipLaunchKernelGGL(apply_kernel<LabelT>, rows, dim3(256), 0, s, labels, bg, parent, size, H, W, G, min_pixels, phase,
                       exclude_nodes, counts);
  }
  if (counts) hipLaunchKernelGGL(finish_counts_kernel, dim3((N + 255) / 256), dim3(256), 0, s, counts, N, (unsigned long long)H * W);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_remove_small_zones(void* labels, int labels_i64, int N, int H, int W, int min_pixels, int exclude_nodes,
                                     unsigned char* bg, int* parent, int* size, unsigned long long* counts, hipStream_t s, int G) {
  if (!per_image_shape_ok(N, H, W) || H > 65535) return hipErrorInvalidValue;      // grid.y carries the row
  if (G < 1 || (long long)(G < N ? G : N) * H * W > 0x7fffffffLL) return hipErrorInvalidValue;   // a volume's index fits 31 bits
  if (labels_i64) return run(static_cast<long long*>(labels), N, H, W, G, min_pixels, exclude_nodes, bg, parent, size, counts, s);
  return run(static_cast<unsigned char*>(labels), N, H, W, G, min_pixels, exclude_nodes, bg, parent, size, counts, s);
}

namespace {

// Both entry points run in the context's workspace, 9 bytes per pixel: parent ints, size ints, bg bytes.
int run_in_context(nbc_ctx* c, void* labels_dev, int labels_dtype, int N, int H, int W, int G, int min_pixels, int exclude_nodes,
                   int64_t* counts_dev, void* hip_stream) {
  NBC_HIP(hipSetDevice(c->device));
  const size_t px = (size_t)N * H * W;
  NBC_HIP(c->zones_ws.reserve(px * 9 + 256, Grow::kMargin));   // grows by at least half, like the activation buffers
  int* parent = c->zones_ws.as<int>();
  int* size = parent + px;
  unsigned char* bg = reinterpret_cast<unsigned char*>(size + px);
  NBC_HIP(launch_remove_small_zones(labels_dev, labels_dtype == NBC_LABEL_I64 ? 1 : 0, N, H, W, min_pixels, exclude_nodes, bg,
                                    parent, size, reinterpret_cast<unsigned long long*>(counts_dev),
                                    static_cast<hipStream_t>(hip_stream), G));
  return NBC_OK;
}

}  // namespace
}  // namespace nbc

using namespace nbc;

extern "C" int nbc_remove_small_zones(nbc_ctx* c, void* labels_dev, int labels_dtype, int N, int H, int W, int min_pixels,
                                      int exclude_nodes, int64_t* counts_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_remove_small_zones";
  if (!c || !labels_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (N < 1 || N > 65535 || H < 1 || W < 1 || min_pixels < 0) return fail(kWho, NBC_ERR_INVALID, "bad shape");
  if (!label_dtype_ok(labels_dtype)) return fail(kWho, NBC_ERR_INVALID, "bad labels_dtype");
  return run_in_context(c, labels_dev, labels_dtype, N, H, W, 1, min_pixels, exclude_nodes, counts_dev, hip_stream);
}

extern "C" int nbc_remove_small_zones_groups(nbc_ctx* c, void* labels_dev, int labels_dtype, int N, int H, int W, int G,
                                             int min_pixels, int64_t* counts_dev, void* hip_stream) {
  constexpr const char* kWho = "nbc_remove_small_zones_groups";
  if (!c || !labels_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!per_image_shape_ok(N, H, W) || H > 65535 || min_pixels < 0) return fail(kWho, NBC_ERR_INVALID, "bad shape");
  if (G < 1 || G > 64 || (long long)(G < N ? G : N) * H * W > 0x7fffffffLL)
    return fail(kWho, NBC_ERR_INVALID, "bad group: 1 <= G <= 64 and g * H * W < 2^31 for the g = min(G, N) images of a group");
  if (!label_dtype_ok(labels_dtype)) return fail(kWho, NBC_ERR_INVALID, "bad labels_dtype");
  return run_in_context(c, labels_dev, labels_dtype, N, H, W, G, min_pixels, 0, counts_dev, hip_stream);
}
