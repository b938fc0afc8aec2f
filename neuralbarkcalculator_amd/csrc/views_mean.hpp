// The mean of a stack of views, element by element (include/nbc.h: nbc_tta_merge, nbc_views_mean):
// m = (((v_0 + v_1) + v_2) + ...) / float(V) -- f32 adds in view order, one IEEE division.  The first view starts the sum, so
// V = 1 keeps the view's bits (-0 included); a NaN in any view gives NaN.  Each function is one operation: nothing to contract.
#pragma once
#include <hip/hip_runtime.h>

namespace nbc {

// the sum after view j (0-based) has been taken in
__device__ __forceinline__ float views_mean_add(float sum, float a, int j) { return j == 0 ? a : sum + a; }

// the mean of V views from their sum
__device__ __forceinline__ float views_mean_finish(float sum, int V) { return V == 1 ? sum : __fdiv_rn(sum, (float)V); }

}  // namespace nbc
