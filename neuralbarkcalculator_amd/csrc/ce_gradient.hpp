// What the two pixel-gradient passes share (head_refit.hip: ce_pixel_gradient; lovasz.hip: lovasz_pixel_gradient): the softmax of
// a pixel in f64 from its f32 logits, the cross-entropy family's g_c = T[t][p] (q_c - [c = t]) on it, and the host checks of the
// tap tables both entry points take.  One statement of each, so that the table-only nbc_lovasz_gradient is nbc_ce_gradient bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "nbc_kernels.hpp"
#include "reduce.hpp"

namespace nbc {

struct CeTable {
  double t[9];                                          // T[target class][argmax class]
};

// q = softmax in f64 from the f32 logits
__device__ __forceinline__ void pixel_softmax(float a, float b, float c, double (&q)[3]) {
  const double x0 = (double)a, x1 = (double)b, x2 = (double)c;
  const double m = fmax(fmax(x0, x1), x2);
  const double e0 = exp(x0 - m), e1 = exp(x1 - m), e2 = exp(x2 - m);
  const double s = e0 + e1 + e2;
  q[0] = e0 / s;
  q[1] = e1 / s;
  q[2] = e2 / s;
}

// g_c = T[t][p] (q_c - [c = t]) of one pixel; p as the forward's argmax decides it
__device__ __forceinline__ void pixel_gradient(float a, float b, float c, unsigned grey, const CeTable& T, const double (&q)[3],
                                               double (&g)[3]) {
  const unsigned t = target_class(grey);
  const unsigned cell = t * 3u + (unsigned)argmax3(a, b, c);
  double wgt = T.t[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) wgt = cell == (unsigned)k ? T.t[k] : wgt;
  g[0] = wgt * (q[0] - (t == 0u ? 1.0 : 0.0));
  g[1] = wgt * (q[1] - (t == 1u ? 1.0 : 0.0));
  g[2] = wgt * (q[2] - (t == 2u ? 1.0 : 0.0));
}

// the tap tables and the logits as both entry points want them; 0 or the error set
inline int check_taps(const char* who, const void* logits_full_dev, const BicubicTaps& t) {
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  if ((addr(t.row_idx) | addr(t.row_coeff) | addr(t.col_idx) | addr(t.col_coeff)) & 15u)
    return fail(who, NBC_ERR_INVALID, "the tap index and coefficient tables must be 16-byte aligned");
  if (!aligned4(static_cast<const char*>(logits_full_dev), reinterpret_cast<const char*>(t.row_lo), reinterpret_cast<const char*>(t.row_hi),
                reinterpret_cast<const char*>(t.col_lo), reinterpret_cast<const char*>(t.col_hi)))
    return fail(who, NBC_ERR_INVALID, "logits_full_dev and the lo / hi tables must be 4-byte aligned");
  return NBC_OK;
}

}  // namespace nbc
