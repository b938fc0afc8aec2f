// The zones of a label map (nbc_label_zones, include/nbc.h): the 8-connected components of each class c in {1, 2}, one
// record per zone -- first pixel, class, pixels, bounding box, coordinate sums, perimeter.  Integer work, exact against the
// host restatement (neuralbarkcalculator_amd/zones.py: scipy.ndimage.label per class plus numpy reductions).
//
// The labelling is components.hpp's: a pixel joins a neighbour only when both carry the same class, so the zones of class 1
// and of class 2 are labelled in one pass over one parent array.
//   zone_tile      label_tile; every pixel then points at its tile-local root (a pixel index of the image); the class
//                  (0 for any label outside {1, 2}) goes to a byte plane that every later kernel reads instead of the labels
//   border_rows / _cols   components.hpp's unions across the tile borders, on that plane
//   count_roots    a root is a pixel that points at itself; unite() roots at the smaller index, so a zone's root is its
//                  first pixel in raster order.  Roots per 1024 consecutive pixels,
//   scan_roots     their exclusive scan per image (one block per image) and the image's zone count,
//   assign_roots   every root's index within its image, in raster order: the root's parent becomes the code -2 - index and,
//                  below cap, its row is initialised
//   accumulate     one 32x32 tile per block again: every zone pixel walks to its root's code; a wave reduces its two rows per
//                  distinct zone from ballots alone (pixel count, coordinate sums and box from the bit mask, the perimeter from
//                  four side ballots), its leader adds that into an LDS hash slot of the tile, and every used slot issues one
//                  set of 64-bit global atomics (4 adds, 2 mins, 2 maxes) into the zone's row.  Rows at or above cap get nothing.
// Workspace: 4 B (parent) + 1 B (class) per pixel + 4 B per 1024 pixels.  Integer sums, mins and maxes do not depend on their
// order: an image's rows are the same alone, in any batch, on any stream and from run to run.
#include "components.hpp"
#include "nbc_ctx.hpp"
#include "nbc_kernels.hpp"
#include "reduce.hpp"

namespace nbc {
namespace {

constexpr int TILE = kLabelTile;
constexpr int kChunk = 1024;                 // consecutive pixels per block of the root count / scan / assign
constexpr int kRow = NBC_ZONE_ROW;           // int64 per zone
constexpr int kSlots = TILE * TILE;          // LDS hash slots per tile: at most 512 zones meet a tile (two per 2x2 pixels)

template <typename LabelT>
__global__ __launch_bounds__(TILE* TILE) void zone_tile_kernel(const LabelT* __restrict__ labels, unsigned char* __restrict__ cls,
                                                                int* __restrict__ parent, int H, int W) {
  __shared__ int s[TILE * TILE];
  __shared__ unsigned char sc[TILE * TILE];
  const int t = threadIdx.x;
  const int x = blockIdx.x * TILE + (t & (TILE - 1)), y = blockIdx.y * TILE + (t >> 5);
  const size_t img = (size_t)blockIdx.z * H * W;
  const bool inside = x < W && y < H;
  const int p = y * W + x;
  int c = 0;
  if (inside) {
    const LabelT v = labels[img + p];
    c = v == (LabelT)1 ? 1 : (v == (LabelT)2 ? 2 : 0);
  }
  const int r = label_tile(c, s, sc);
  if (inside) {
    parent[img + p] = c ? (blockIdx.y * TILE + (r >> 5)) * W + blockIdx.x * TILE + (r & (TILE - 1)) : -1;   // index inside the image
    cls[img + p] = (unsigned char)c;
  }
}

__global__ __launch_bounds__(kChunk) void count_roots_kernel(const int* __restrict__ parent, int* __restrict__ blocks, int P) {
  const long long q = (long long)blockIdx.x * kChunk + threadIdx.x;      // may pass 2^31 in the last block
  const bool root = q < P && parent[(size_t)blockIdx.y * P + q] == q;
  const int cnt = __syncthreads_count(root);
  if (threadIdx.x == 0) blocks[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = cnt;
}

// blocks[n][0..nb) -> their exclusive scan, num[n] = their sum.  One block per image.
__global__ __launch_bounds__(kChunk) void scan_roots_kernel(int* __restrict__ blocks, int nb, long long* __restrict__ num) {
  __shared__ int wsum[kChunk / 64];
  int* B = blocks + (size_t)blockIdx.x * nb;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;
  for (int base = 0; base < nb; base += kChunk) {
    const int i = base + t;
    const int v = i < nb ? B[i] : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(incl, off, 64);
      if (lane >= off) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kChunk / 64; ++k) {
      const int ws = wsum[k];
      if (k < wave) before += ws;
      total += ws;
    }
    if (i < nb) B[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (t == 0) num[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kChunk) void assign_roots_kernel(int* __restrict__ parent, const unsigned char* __restrict__ cls,
                                                              const int* __restrict__ blocks, int P, int H, int W,
                                                              long long* __restrict__ rows, int cap) {
  __shared__ int wsum[kChunk / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long q = (long long)blockIdx.x * kChunk + t;
  const size_t img = (size_t)blockIdx.y * P;
  const bool root = q < P && parent[img + q] == q;
  const unsigned long long bits = __ballot(root);
  if (lane == 0) wsum[wave] = (int)__popcll(bits);
  __syncthreads();
  if (!root) return;
  int idx = blocks[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + (int)__popcll(bits & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) idx += wsum[k];
  parent[img + q] = -2 - idx;
  if (idx < cap) {
    long long* row = rows + ((size_t)blockIdx.y * cap + idx) * kRow;
    row[0] = q;
    row[1] = cls[img + q];
    row[2] = 0;
    row[3] = W;      // the box: mins start above, maxes below every coordinate
    row[4] = H;
    row[5] = 0;
    row[6] = 0;
    row[7] = 0;
    row[8] = 0;
    row[9] = 0;
  }
}

// sum of the positions of the set bits of m
__device__ __forceinline__ int bit_position_sum(unsigned m) {
  return __popc(m & 0xAAAAAAAAu) + 2 * __popc(m & 0xCCCCCCCCu) + 4 * __popc(m & 0xF0F0F0F0u) + 8 * __popc(m & 0xFF00FF00u) +
         16 * __popc(m & 0xFFFF0000u);
}

enum { kPixels, kSumX, kSumY, kPerimeter, kMinX, kMinY, kMaxX, kMaxY, kFields };

__global__ __launch_bounds__(TILE* TILE) void accumulate_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ cls,
                                                                 int H, int W, long long* __restrict__ rows, int cap) {
  __shared__ int key[kSlots];
  __shared__ int acc[kFields][kSlots];
  const int t = threadIdx.x, tx = t & (TILE - 1), ty = t >> 5;
  const int x = blockIdx.x * TILE + tx, y = blockIdx.y * TILE + ty;
  const size_t img = (size_t)blockIdx.z * H * W;
  const int* L = parent + img;
  const unsigned char* C = cls + img;
  key[t] = -1;
#pragma unroll
  for (int f = 0; f < kFields; ++f) acc[f][t] = (f == kMinX || f == kMinY) ? 0x7fffffff : (f == kMaxX || f == kMaxY ? -1 : 0);
  __syncthreads();

  int idx = -1;
  bool dn = false, ds = false, dw = false, de = false;
  if (x < W && y < H) {
    const int p = y * W + x;
    const int c = C[p];
    if (c) idx = root_index(L, p);
    if (idx >= cap) idx = -1;
    if (idx >= 0) {                       // sides whose neighbour has another label or lies outside the image
      dn = y == 0 || C[p - W] != c;
      ds = y == H - 1 || C[p + W] != c;
      dw = x == 0 || C[p - 1] != c;
      de = x == W - 1 || C[p + 1] != c;
    }
  }
  const unsigned long long bn = __ballot(dn), bs = __ballot(ds), bw = __ballot(dw), be = __ballot(de);
  const int x_base = blockIdx.x * TILE, y_lo = blockIdx.y * TILE + (ty & ~1);      // the wave's two rows: y_lo, y_lo + 1
  for_each_key(idx >= 0, idx, [&](int k, unsigned long long same) {
    const unsigned lo = (unsigned)same, hi = (unsigned)(same >> 32), both = lo | hi;
    const int n_lo = __popc(lo), n_hi = __popc(hi);
    unsigned h = ((unsigned)k * 2654435761u) >> 22;                                 // 10 bits: kSlots
    while (true) {
      const int old = atomicCAS(&key[h], -1, k);
      if (old == -1 || old == k) break;
      h = (h + 1) & (kSlots - 1);
    }
    atomicAdd(&acc[kPixels][h], n_lo + n_hi);
    atomicAdd(&acc[kSumX][h], (n_lo + n_hi) * x_base + bit_position_sum(lo) + bit_position_sum(hi));
    atomicAdd(&acc[kSumY][h], n_lo * y_lo + n_hi * (y_lo + 1));
    atomicAdd(&acc[kPerimeter][h], (int)(__popcll(same & bn) + __popcll(same & bs) + __popcll(same & bw) + __popcll(same & be)));
    atomicMin(&acc[kMinX][h], x_base + (__ffs((int)both) - 1));
    atomicMax(&acc[kMaxX][h], x_base + 31 - __clz((int)both));
    atomicMin(&acc[kMinY][h], lo ? y_lo : y_lo + 1);
    atomicMax(&acc[kMaxY][h], hi ? y_lo + 1 : y_lo);
  });
  __syncthreads();
  const int k = key[t];
  if (k < 0) return;
  unsigned long long* row = reinterpret_cast<unsigned long long*>(rows) + ((size_t)blockIdx.z * cap + k) * kRow;
  atomicAdd(row + 2, (unsigned long long)acc[kPixels][t]);
  atomicMin(row + 3, (unsigned long long)acc[kMinX][t]);
  atomicMin(row + 4, (unsigned long long)acc[kMinY][t]);
  atomicMax(row + 5, (unsigned long long)acc[kMaxX][t]);
  atomicMax(row + 6, (unsigned long long)acc[kMaxY][t]);
  atomicAdd(row + 7, (unsigned long long)acc[kSumX][t]);
  atomicAdd(row + 8, (unsigned long long)acc[kSumY][t]);
  if (acc[kPerimeter][t]) atomicAdd(row + 9, (unsigned long long)acc[kPerimeter][t]);
}

}  // namespace

ZonesLayout zones_layout(int N, int H, int W) {
  const size_t P = (size_t)H * W, nb = (P + kChunk - 1) / kChunk;
  Carver ws;
  const size_t parent = ws.take(4 * P * N), cls = ws.take(P * N), blocks = ws.take(4 * nb * N);
  return {parent, cls, blocks, ws.offset};
}

hipError_t launch_label_zones(const void* labels, int labels_i64, int N, int H, int W, long long* rows, int cap, long long* num,
                              int* parent, unsigned char* cls, int* blocks, hipStream_t s) {
  if (!per_image_shape_ok(N, H, W) || H > 65535 || W > 65535 || cap < 1) return hipErrorInvalidValue;
  const int P = H * W, nb = (P + kChunk - 1) / kChunk;
  const dim3 tiles((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, N);
  if (labels_i64)
    hipLaunchKernelGGL(zone_tile_kernel<long long>, tiles, dim3(TILE * TILE), 0, s, static_cast<const long long*>(labels), cls, parent,
                       H, W);
  else
    hipLaunchKernelGGL(zone_tile_kernel<unsigned char>, tiles, dim3(TILE * TILE), 0, s, static_cast<const unsigned char*>(labels), cls,
                       parent, H, W);
  launch_borders(parent, ClassPlane{cls}, N, H, W, s);
  hipLaunchKernelGGL(count_roots_kernel, dim3(nb, N), dim3(kChunk), 0, s, parent, blocks, P);
  hipLaunchKernelGGL(scan_roots_kernel, dim3(N), dim3(kChunk), 0, s, blocks, nb, num);
  hipLaunchKernelGGL(assign_roots_kernel, dim3(nb, N), dim3(kChunk), 0, s, parent, cls, blocks, P, H, W, rows, cap);
  hipLaunchKernelGGL(accumulate_kernel, tiles, dim3(TILE * TILE), 0, s, parent, cls, H, W, rows, cap);
  return hipGetLastError();
}

bool zones_shape_ok(int N, int H, int W) { return per_image_shape_ok(N, H, W) && H <= 65535 && W <= 65535; }

}  // namespace nbc

using namespace nbc;

extern "C" size_t nbc_zones_workspace_bytes(int N, int H, int W) { return zones_shape_ok(N, H, W) ? zones_layout(N, H, W).total : 0; }

extern "C" int nbc_label_zones(nbc_ctx* c, const void* labels_dev, int labels_dtype, int N, int H, int W, int64_t* rows_dev, int cap,
                               int64_t* num_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
  constexpr const char* kWho = "nbc_label_zones";
  if (!c || !labels_dev || !rows_dev || !num_dev || !workspace_dev) return fail(kWho, NBC_ERR_INVALID, "null argument");
  if (!zones_shape_ok(N, H, W))
    return fail(kWho, NBC_ERR_INVALID, "bad shape: 1 <= N <= 65535, H and W in 1..65535 and H * W < 2^31");
  if (cap < 1) return fail(kWho, NBC_ERR_INVALID, "cap must be at least 1");
  if (!label_dtype_ok(labels_dtype)) return fail(kWho, NBC_ERR_INVALID, "bad labels_dtype");
  const ZonesLayout lay = zones_layout(N, H, W);
  if (const int rc = check_workspace(kWho, workspace_dev, workspace_bytes, lay.total)) return rc;
  NBC_HIP(hipSetDevice(c->device));
  unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
  NBC_HIP(launch_label_zones(labels_dev, labels_dtype == NBC_LABEL_I64 ? 1 : 0, N, H, W, reinterpret_cast<long long*>(rows_dev), cap,
                             reinterpret_cast<long long*>(num_dev), reinterpret_cast<int*>(ws + lay.parent), ws + lay.cls,
                             reinterpret_cast<int*>(ws + lay.blocks), static_cast<hipStream_t>(hip_stream)));
  return NBC_OK;
}
