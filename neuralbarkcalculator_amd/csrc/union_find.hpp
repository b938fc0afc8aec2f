// The union-find that components.hpp labels connected components with: one int per pixel that points at a pixel
// of the same component with a smaller or equal index (itself: a root), in LDS inside a 32x32 tile and in global memory across
// tiles.  unite() always roots at the smaller index, so a component's root is its first pixel in raster order.
#pragma once
#include <hip/hip_runtime.h>

namespace nbc {

constexpr int kLabelTile = 32;   // the tile one block labels in LDS (1024 threads, a wave holds two of its rows)

// Root of x with intermediate pointer jumping: every node passed is re-pointed at its grandparent.
// Parents only ever decrease and always stay inside the node's (eventual) component, so the plain
// stores race benignly with the atomicMin links of unite() (ECL-CC's "representative").
__device__ __forceinline__ int find_root(int* L, int x) {
  int curr = L[x];
  if (curr != x) {
    int prev = x, next;
    while (curr > (next = L[curr])) {
      L[prev] = next;
      prev = curr;
      curr = next;
    }
  }
  return curr;
}
__device__ __forceinline__ int find_root_lds(const volatile int* L, int x) {
  int p = L[x];
  while (p != x) { x = p; p = L[x]; }
  return x;
}
// link the larger root under the smaller one; retried when another thread re-rooted it meanwhile
__device__ __forceinline__ void unite(int* L, int a, int b) {
  while (true) {
    a = find_root(L, a);
    b = find_root(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a);
    if (old == b) return;
    b = old;
  }
}
__device__ __forceinline__ void unite_lds(int* L, int a, int b) {
  while (true) {
    a = find_root_lds(L, a);
    b = find_root_lds(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a);
    if (old == b) return;
    b = old;
  }
}

}  // namespace nbc
