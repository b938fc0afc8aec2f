// The 8-connected-component labelling under small_zones.hip, zones.hip and zone_match.hip, defined once: two pixels are joined
// when they are 8-neighbours of the same non-zero class.  small_zones.hip labels a binary mask (class 0 or 1), zones.hip
// classes 1 and 2 in one pass over one parent array (union_find.hpp).  The rule has three parts:
//   label_tile      one 32x32 tile per block in LDS: the runs of a tile row from a ballot, then one union per pair of touching
//                   runs of consecutive rows (link_up); every pixel ends at its tile-local root, so the chains in global
//                   memory only ever link tile roots;
//   border_rows     link_up again for the rows y = 32k (k >= 1), on global memory;
//   border_cols     the columns x = 32k (k >= 1): the straight link across the border, and the two diagonal ones.
// Only border pixels have anything to do in the last two, so their launches cover just them.
//
// The parents of an image index its own plane, except under small_zones.hip's grouped pass: there G consecutive images form
// one volume with one index space (Volume), their components get linked across images by that file, and everything here
// only adds the image's offset inside its volume to the indices it writes.  G = 1 is the plain per-image labelling.
#pragma once
#include "union_find.hpp"

namespace nbc {

// The one link a pixel makes to the row above, given which of its neighbours carry its class: through N unless its W
// neighbour already does (W and NW both set), or through NW / NE when only a diagonal touches and the run's next pixel on
// that side (W resp. E) does not make the link itself.  unite_to(d) joins the pixel with the one at N + d.
template <typename Unite>
__device__ __forceinline__ void link_up(bool w, bool e, bool n, bool nw, bool ne, Unite unite_to) {
  if (n) {
    if (!(w && nw)) unite_to(0);
  } else {
    if (nw && !w) unite_to(-1);
    if (ne && !e) unite_to(1);
  }
}

// Thread t of the block's 1024 is pixel (t & 31, t >> 5) of the tile and carries class c: 0 (belongs to nothing), 1 or 2.
// s (parents) and sc (classes) are LDS arrays of one entry per thread.  Returns the thread's tile-local root, a thread
// index, or -1 for class 0; s does not change any more after the return.
__device__ __forceinline__ int label_tile(int c, int* s, unsigned char* sc) {
  constexpr int TILE = kLabelTile;
  const int t = threadIdx.x, tx = t & (TILE - 1);
  // Horizontal runs first, without atomics: a wave holds two rows of the tile; a pixel points at the first pixel of its
  // run (the position after the nearest bit of another class to its left).
  const unsigned long long b1 = __ballot(c == 1), b2 = __ballot(c == 2);
  const unsigned row_bits = (unsigned)((c == 1 ? b1 : (c == 2 ? b2 : 0ull)) >> (32 * ((t >> 5) & 1)));
  const unsigned zeros_left = ~row_bits & ((1u << tx) - 1u);
  const int run_start = zeros_left ? 32 - __clz((int)zeros_left) : 0;
  s[t] = c ? (t - tx + run_start) : -1;
  sc[t] = (unsigned char)c;
  __syncthreads();
  // Then one union per pair of touching runs of consecutive rows: the rest of the run is already joined.
  if (c && t >= TILE) {
    const bool w = tx > 0 && ((row_bits >> (tx - 1)) & 1u), e = tx < TILE - 1 && ((row_bits >> (tx + 1)) & 1u);
    link_up(w, e, sc[t - TILE] == c, tx > 0 && sc[t - TILE - 1] == c, tx < TILE - 1 && sc[t - TILE + 1] == c,
            [&](int d) { unite_lds(s, t, t - TILE + d); });
  }
  __syncthreads();
  return c ? find_root_lds(s, t) : -1;
}

// The class of a pixel of the batch, for the border kernels: a byte plane as it stands, or one where 0 is the set value.
struct ClassPlane {
  const unsigned char* plane;
  __device__ int operator()(size_t q) const { return plane[q]; }
};
struct ZeroIsSet {
  const unsigned char* plane;
  __device__ int operator()(size_t q) const { return plane[q] == 0; }
};

// Image n of a batch whose consecutive groups of G images are volumes: `base` is the volume's first pixel in the batch (where
// its parent indices count from), `off` the image's first pixel inside the volume.  G * H * W < 2^31.
struct Volume {
  size_t base;
  int off;
  __device__ Volume(int n, int G, int H, int W) {
    const int first = n - n % G;
    base = (size_t)first * H * W;
    off = (n - first) * H * W;
  }
  __device__ size_t image() const { return base + (size_t)off; }
};

template <typename ClassOf>
__global__ void border_rows_kernel(int* __restrict__ parent, ClassOf cls, int H, int W, int G) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = (blockIdx.y + 1) * kLabelTile;
  if (x >= W || y >= H) return;
  const Volume vol(blockIdx.z, G, H, W);
  const size_t img = vol.image();
  int* L = parent + vol.base;
  const int p = y * W + x;
  const int c = cls(img + p);
  if (!c) return;
  const auto same = [&](int q) { return cls(img + q) == c; };
  link_up(x > 0 && same(p - 1), x < W - 1 && same(p + 1), same(p - W), x > 0 && same(p - W - 1), x < W - 1 && same(p - W + 1),
          [&](int d) { unite(L, vol.off + p, vol.off + p - W + d); });
}

// The pixel right of the border links to W.  The diagonals across a vertical border are needed only when neither the
// straight neighbour of the pixel's own tile (N) nor the pixel across the border in its own row (W resp. E) has the pixel's
// class: otherwise that neighbour's own link already joins the two.
template <typename ClassOf>
__global__ void border_cols_kernel(int* __restrict__ parent, ClassOf cls, int H, int W, int G) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x, x = (blockIdx.y + 1) * kLabelTile;   // x: first column right of a border
  if (y >= H || x >= W) return;
  const Volume vol(blockIdx.z, G, H, W);
  const size_t img = vol.image();
  int* L = parent + vol.base;
  const int p = y * W + x;                    // right of the border; p - 1 is left of it
  const int v = vol.off + p;                  // p as the volume counts it
  const int cr = cls(img + p), cl = cls(img + p - 1);
  if (cr && cr == cl) unite(L, v, v - 1);
  if ((y & (kLabelTile - 1)) == 0) return;    // rows on a horizontal border (and row 0) are border_rows_kernel's
  if (cr && cl != cr && cls(img + p - W) != cr && cls(img + p - W - 1) == cr) unite(L, v, v - W - 1);      // NW across the border
  if (cl && cr != cl && cls(img + p - 1 - W) != cl && cls(img + p - W) == cl) unite(L, v - 1, v - W);      // NE across the border
}

template <typename ClassOf>
inline void launch_borders(int* parent, ClassOf cls, int N, int H, int W, hipStream_t s, int G = 1) {
  constexpr int TILE = kLabelTile;
  if (H > TILE) hipLaunchKernelGGL(border_rows_kernel<ClassOf>, dim3((W + 255) / 256, (H - 1) / TILE, N), dim3(256), 0, s, parent, cls, H, W, G);
  if (W > TILE) hipLaunchKernelGGL(border_cols_kernel<ClassOf>, dim3((H + 255) / 256, (W - 1) / TILE, N), dim3(256), 0, s, parent, cls, H, W, G);
}

// One leader per distinct key among the valid lanes of a wave: body(key, same) runs in the first lane that holds the key,
// `same` being the mask of the lanes that share it.  Every lane of the wave must call this.
template <typename Key, typename Body>
__device__ __forceinline__ void for_each_key(bool valid, Key key, Body body) {
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const Key k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k) & todo;
    if ((int)(threadIdx.x & 63) == leader) body(k, same);
    todo &= ~same;
  }
}

// From pixel p up to its zone's root once assign_roots_kernel (zones.hip) has run: a parent's index is smaller than its
// child's and the root's parent holds the code -2 - index.  Returns the index, the zone's position in first-pixel order.
__device__ __forceinline__ int root_index(const int* L, int p) {
  int v = L[p];
  while (v >= 0) v = L[v];
  return -2 - v;
}

}  // namespace nbc
