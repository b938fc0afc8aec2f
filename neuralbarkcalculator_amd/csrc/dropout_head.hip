// classifier.4 behind a live Dropout (models.py:113-124: FCNHead's Dropout(0.1) sits between the 3x3 head convolution and
// the 1x1 classifier, and the shipped predict.py never calls .eval()): the low-resolution logits of several random draws
// of the mask from ONE read of the stored input of classifier.4.  The definition of a draw is in include/nbc.h
// (nbc_dropout_draws); the generator is csrc/philox.hpp, shared with the host entry point nbc_dropout_mask below.
//
// The arithmetic is head1x1_body's (pointwise.hip): the weight rows and the chain are the same functions of head1x1.hpp, the
// tree and the store the functions whose text head1x1_body writes out, the operands come in through the same load8 / decode8 of
// stored.hpp.  The one difference is the chain's
// per-element hook, here the multiplication by the keep factor: one wave per pixel, lane l owns channels 8l .. 8l+7 -- elements
// 512 pixel + 8l .. + 7, i.e. quads 128 pixel + 2l and + 1: two Philox calls per lane, pixel and draw.  With p = 0 the factor is
// 1.0f for every element and the logits are bit for bit the forward's.
#include "head1x1.hpp"
#include "nbc_kernels.hpp"
#include "philox.hpp"
#include "reduce.hpp"
#include "stored.hpp"

namespace nbc {
namespace {

// grid = (ceil(hw / 32), images of this launch); a block is four waves of eight pixels each, like head1x1_kernel.
template <int PREC>
__global__ __launch_bounds__(256) void head1x1_dropout_kernel(const void* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y, int N,
                                                              int hw, int img0, DropoutIds ids, unsigned long long seed,
                                                              unsigned threshold, float keep_scale, int first_draw, int draws,
                                                              unsigned* __restrict__ nonfinite) {
  constexpr int CIN = 512;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int img = img0 + blockIdx.y;
  const unsigned long long id = ids.id[blockIdx.y];
  float wr[3][8];
  head_weight_rows(w, CIN, lane * 8, wr);
  const float b[3] = {bias[0], bias[1], bias[2]};
  const int first = (blockIdx.x * 4 + wave) * 8;
  if (first >= hw) return;                                // wave-uniform: the shuffles below see whole waves
  const unsigned char* xi = static_cast<const unsigned char*>(x) + (size_t)img * hw * CIN * (PREC == 1 ? 2 : 4);
  Eight<PREC> raw[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) raw[q] = load8<PREC>(eight_at<PREC>(xi + (size_t)min(first + q, hw - 1) * CIN * stored_elem_bytes(PREC), lane * 8));
  bool bad = false;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int pix = first + q;
    float f[8];
    decode8(raw[q], f);
    const unsigned quad = (unsigned)pix * 128u + 2u * (unsigned)lane;   // hw * 128 < 2^32 (checked by the caller)
    for (int d = 0; d < draws; ++d) {
      const Philox4 r0 = dropout_words(quad, (unsigned)(first_draw + d), id, seed);
      const Philox4 r1 = dropout_words(quad + 1u, (unsigned)(first_draw + d), id, seed);
      float s[3];
      head_chain(f, wr, s, [&](int e, float v) {
        const unsigned r = e < 4 ? r0.v[e] : r1.v[e - 4];
        return v * (r < threshold ? 0.f : keep_scale);                   // X (m keep)
      });
      head_tree<64>(s);
      if (lane == 0 && pix < hw) bad = !head_store(s, b, y + ((size_t)d * N + img) * 3 * hw + pix, hw) || bad;
    }
  }
  if (bad) head_raise(nonfinite);
}

}  // namespace

hipError_t launch_head1x1_dropout(const void* x, const float* w, const float* bias, float* y, int N, int hw, int precision,
                                  const uint64_t* ids_host, uint64_t seed, uint32_t threshold, float keep_scale, int first_draw,
                                  int draws, unsigned* nonfinite, hipStream_t s) {
  if (N < 1 || hw < 1 || (unsigned long long)hw * 128ull >= (1ull << 32) || draws < 1) return hipErrorInvalidValue;
  for (int img0 = 0; img0 < N; img0 += kDropoutIdsPerLaunch) {
    const int n = N - img0 < kDropoutIdsPerLaunch ? N - img0 : kDropoutIdsPerLaunch;
    DropoutIds ids{};
    for (int i = 0; i < n; ++i) ids.id[i] = ids_host[img0 + i];
    const dim3 grid((hw + 31) / 32, n);
    with_precision(precision, [&](auto P) {
      hipLaunchKernelGGL(head1x1_dropout_kernel<P.value>, grid, dim3(256), 0, s, x, w, bias, y, N, hw, img0, ids, seed, threshold,
                         keep_scale, first_draw, draws, nonfinite);
    });
  }
  return hipGetLastError();
}

}  // namespace nbc

using namespace nbc;

extern "C" int nbc_dropout_mask(uint64_t seed, uint64_t image_id, int draw, double p, uint64_t first_element, size_t count,
                                uint8_t* keep_host) {
  if (!dropout_p_ok(p)) return set_error(NBC_ERR_INVALID, "nbc_dropout_mask: p must lie in [0, 1)");
  if (draw < 0) return set_error(NBC_ERR_INVALID, "nbc_dropout_mask: draw must not be negative");
  if (count && !keep_host) return set_error(NBC_ERR_INVALID, "nbc_dropout_mask: null keep_host");
  if (first_element > (1ull << 34) || count > (1ull << 34) || first_element + count > (1ull << 34))
    return set_error(NBC_ERR_INVALID, "nbc_dropout_mask: elements beyond 2^34 (a quad index has 32 bits)");
  const uint32_t T = dropout_threshold(p);
  uint64_t quad = ~0ull;
  Philox4 r{};
  for (size_t i = 0; i < count; ++i) {
    const uint64_t e = first_element + i;
    if ((e >> 2) != quad) {
      quad = e >> 2;
      r = dropout_words((uint32_t)quad, (uint32_t)draw, image_id, seed);
    }
    keep_host[i] = r.v[e & 3] < T ? 0 : 1;
  }
  return NBC_OK;
}
