// classifier.4 (models.py:121): the 1x1 conv to the 3 classes with bias, in pieces: a lane's weight rows, its f32 fma chain over
// eight channels in channel order, the xor tree over the lanes of a pixel, and the store with the bias, the non-finite flag and
// the clearing of the class counters.  The kernel behind the live Dropout (dropout_head.hip) is built from all of them, the
// lane-strided kernel of the EfficientNet FCN heads (efficientnet.hip) from the tree and the epilogue, and the forward's two
// kernels (head1x1_body, pointwise.hip) from the rows, the chain and the clearing; their tree and store are the text of
// head_tree and head_store written out, for the reason given there.  "p = 0 gives the forward's logits bit for bit" is the chain
// both call, plus those two short pieces kept equal.
#pragma once
#include <hip/hip_runtime.h>

namespace nbc {

// the lane's weight rows: wr[c][e] = w[c][c8 + e], w f32 [3][cin]
__device__ __forceinline__ void head_weight_rows(const float* __restrict__ w, int cin, int c8, float (&wr)[3][8]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) wr[c][e] = w[c * cin + c8 + e];
}

// s[c] = sum over e of g(e, f[e]) * wr[c][e]: one fma chain per class from 0, in channel order.  g is applied to each decoded
// channel first: the identity in the forward (head_identity: no instruction), the keep factor behind the Dropout.
struct head_identity {
  __device__ __forceinline__ float operator()(int, float v) const { return v; }
};
template <typename G>
__device__ __forceinline__ void head_chain(const float (&f)[8], const float (&wr)[3][8], float (&s)[3], G g) {
  s[0] = s[1] = s[2] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = g(e, f[e]);
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = __builtin_fmaf(v, wr[c][e], s[c]);
  }
}

// the three sums over the LANES (64 or 32) neighbouring lanes that share a pixel, in every one of them: the xor butterfly from
// LANES / 2 down to 1, the three classes' shuffles of one offset together
template <int LANES>
__device__ __forceinline__ void head_tree(float (&s)[3]) {
#pragma unroll
  for (int off = LANES / 2; off >= 1; off >>= 1)
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += __shfl_xor(s[c], off, 64);
}

// logits = s + bias into the pixel's three planes (yp: its place in plane 0, planes hw floats apart); whether all are finite
__device__ __forceinline__ bool head_store(const float (&s)[3], const float (&b)[3], float* __restrict__ yp, int hw) {
  const float l0 = s[0] + b[0], l1 = s[1] + b[1], l2 = s[2] + b[2];
  yp[0] = l0;
  yp[(size_t)hw] = l1;
  yp[2 * (size_t)hw] = l2;
  return __builtin_isfinite(l0) && __builtin_isfinite(l1) && __builtin_isfinite(l2);
}

// a logit that is not finite (NaN / inf in the input or the weights; in f16x2 mode an activation beyond f16's range) raises
// the context's sticky flag: nbc_nonfinite_seen
__device__ __forceinline__ void head_raise(unsigned* __restrict__ nonfinite) {
  if (nonfinite) atomicOr(nonfinite, 1u);
}

// block 0 clears the ncounts (<= the block's 256 threads: head_clears_counts, nbc_kernels.hpp) class counters that the
// upsample / argmax launch behind this one adds to
__device__ __forceinline__ void head_clear_counts(unsigned long long* __restrict__ counts_zero, int ncounts) {
  if (counts_zero && blockIdx.x == 0 && threadIdx.x < ncounts) counts_zero[threadIdx.x] = 0ull;
}

}  // namespace nbc
