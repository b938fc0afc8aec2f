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
#include <algorithm>

#include "head1x1.hpp"
#include "nbc_ctx.hpp"
#include "nbc_kernels.hpp"
#include "philox.hpp"
#include "reduce.hpp"
#include "stored.hpp"

namespace nbc {

constexpr int kDropoutIdsPerLaunch = 64;
struct DropoutIds {
  unsigned long long id[kDropoutIdsPerLaunch];
};

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

// The low-resolution logits y [draws][N][3][hw] of draws first_draw .. first_draw + draws - 1 from one read of x [N][hw][512]
// stored elements.  ids_host: the N image identities, HOST memory, handed to the kernel by value (64 per launch: no copy, no
// synchronisation).  threshold / keep_scale: dropout_threshold(p) / dropout_scale(p) of philox.hpp.  hw * 128 < 2^32.
hipError_t launch_head1x1_dropout(const void* x, const float* w, const float* bias, float* y, int N, int hw, int precision,
                                  const uint64_t* ids_host, uint64_t seed, uint32_t threshold, float keep_scale, int first_draw,
                                  int draws, unsigned* nonfinite, hipStream_t s) {
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

// One pass of nbc_dropout_draws over `draws` draws of N images: its regions of the workspace.  nbc_dropout_workspace_bytes
// publishes `total` (include/nbc.h states the formula), the pass loop takes the offsets.
struct DropoutLayout {
  size_t lowres, labels, parent, size, bg, total;
};
DropoutLayout dropout_layout(int N, int H, int W, int h, int w, int draws) {
  const size_t I = (size_t)draws * N, px = I * H * W;
  Carver ws;
  const size_t lowres = ws.take(12 * I * h * w), labels = ws.take(px);                        // f32 [I][3][h][w], u8 [I][H][W]
  const size_t parent = ws.take(4 * px), size = ws.take(4 * px), bg = ws.take(px);           // remove_small_zones' int, int, u8
  return {lowres, labels, parent, size, bg, ws.offset};
}

// The pass loop behind nbc_dropout_draws and nbc_dropout_votes (`who` prefixes the error messages): the masked classifier,
// the upsample + argmax, remove_small_zones and the counts of each pass; with `with_votes`, the pass's final labels are
// counted into votes_dev before the next pass overwrites them.
int dropout_passes(const char* who, nbc_ctx* c, int N, int H, int W, const uint64_t* image_ids_host, double p, uint64_t seed,
                   int first_draw, int draws, int min_pixels, int exclude_nodes, float* logits_lowres_dev, int64_t* counts_dev,
                   bool with_votes, uint32_t* votes_dev, int accumulate, void* workspace_dev, size_t workspace_bytes,
                   void* hip_stream) {
  if (!dropout_p_ok(p)) return fail(who, NBC_ERR_INVALID, "p must lie in [0, 1)");
  if (draws < 1 || draws > 1024) return fail(who, NBC_ERR_INVALID, "draws must lie in 1..1024");
  if (first_draw < 0 || first_draw > 0x7fffffff - draws)
    return fail(who, NBC_ERR_INVALID, "first_draw must not be negative (and first_draw + draws < 2^31)");
  if (min_pixels < 0) return fail(who, NBC_ERR_INVALID, "min_pixels must not be negative");
  if (!c || !image_ids_host || !counts_dev || !workspace_dev || (with_votes && !votes_dev)) return fail(who, NBC_ERR_INVALID, "null argument");
  if (with_votes && reinterpret_cast<uintptr_t>(votes_dev) % 16 != 0) return fail(who, NBC_ERR_INVALID, "votes_dev must be 16-byte aligned");
  if (c->offsets_on)
    return fail(who, NBC_ERR_INVALID, "the context holds logit offsets (nbc_set_logit_offsets); the draws decide by the plain argmax");
  const Op* head = nullptr;
  if (const int rc = last_forward_head(who, c, N, H, W, &head,
                                       " (DeepLabHead's Dropout sits inside ASPP; the EfficientNet heads are left out)"))
    return rc;
  const size_t one = nbc_dropout_workspace_bytes(N, H, W, 1);
  if (one == 0) return fail(who, NBC_ERR_INVALID, "shape beyond the limits (N <= 65535, H * W < 2^31, h * w < 2^25)");
  if (reinterpret_cast<uintptr_t>(workspace_dev) % 256 != 0) return fail(who, NBC_ERR_INVALID, "the workspace must be 256-byte aligned");
  if (workspace_bytes < one)
    return fail(who, NBC_ERR_INVALID, "the workspace is smaller than nbc_dropout_workspace_bytes(N, H, W, 1)");
  const Plan& P = c->plan;
  int pass = std::min(draws, 65535 / N);
  while (pass > 1 && nbc_dropout_workspace_bytes(N, H, W, pass) > workspace_bytes) --pass;
  NBC_HIP(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const UnitPtrs up = unit_ptrs(c, head->unit);
  const int hw = P.h * P.w;
  const uint32_t T = dropout_threshold(p);
  const float m = dropout_scale(p);
  for (int d0 = 0; d0 < draws; d0 += pass) {
    const int D = std::min(pass, draws - d0);
    const int I = D * N;
    // the pass's slice of the workspace, sized for THIS pass (the last one may be shorter)
    const DropoutLayout L = dropout_layout(N, H, W, P.h, P.w, D);
    unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
    float* lowres = logits_lowres_dev ? logits_lowres_dev + (size_t)d0 * N * kNumClasses * hw : reinterpret_cast<float*>(ws + L.lowres);
    unsigned char* labels = ws + L.labels;
    int* parent = reinterpret_cast<int*>(ws + L.parent);
    int* size = reinterpret_cast<int*>(ws + L.size);
    unsigned char* bg = ws + L.bg;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_dev) + (size_t)d0 * N * kNumClasses;
    NBC_HIP(launch_head1x1_dropout(c->bufs[head->in_buf].get(), up.w, up.shift, lowres, N, hw, c->precision, image_ids_host, seed, T, m,
                                   first_draw + d0, D, c->nonfinite.as<unsigned>(), s));
    if (min_pixels > 0) {
      NBC_HIP(launch_upsample_argmax(lowres, I, P.h, P.w, H, W, nullptr, labels, 0, nullptr, 0, s));
      NBC_HIP(launch_remove_small_zones(labels, 0, I, H, W, min_pixels, exclude_nodes, bg, parent, size, counts, s));
    } else {
      NBC_HIP(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * kNumClasses * I, s));
      NBC_HIP(launch_upsample_argmax(lowres, I, P.h, P.w, H, W, nullptr, labels, 0, counts, exclude_nodes, s));
    }
    if (with_votes)                                 // the first pass of a call that does not accumulate stores the words
      NBC_HIP(launch_vote_accumulate(labels, D, N, (long long)H * W, votes_dev, !accumulate && d0 == 0, s));
  }
  return NBC_OK;
}

}  // namespace
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

extern "C" size_t nbc_dropout_workspace_bytes(int N, int H, int W, int draws_per_pass) {
  if (N < 1 || H < 8 || W < 8 || H > 65535 || draws_per_pass < 1 || (long long)H * W > 0x7fffffffLL) return 0;
  const unsigned long long I = (unsigned long long)draws_per_pass * (unsigned long long)N;
  if (I > 65535ull) return 0;
  int h = 0, w = 0;
  if (nbc_lowres_size(H, W, &h, &w) != NBC_OK || h < 1 || w < 1 || (unsigned long long)h * w >= (1ull << 25)) return 0;
  return dropout_layout(N, H, W, h, w, draws_per_pass).total;
}

extern "C" int nbc_dropout_draws(nbc_ctx* c, int N, int H, int W, const uint64_t* image_ids_host, double p, uint64_t seed,
                                 int first_draw, int draws, int min_pixels, int exclude_nodes, float* logits_lowres_dev,
                                 int64_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream) {
  return dropout_passes("nbc_dropout_draws", c, N, H, W, image_ids_host, p, seed, first_draw, draws, min_pixels, exclude_nodes,
                        logits_lowres_dev, counts_dev, false, nullptr, 0, workspace_dev, workspace_bytes, hip_stream);
}

extern "C" int nbc_dropout_votes(nbc_ctx* c, int N, int H, int W, const uint64_t* image_ids_host, double p, uint64_t seed,
                                 int first_draw, int draws, int min_pixels, int exclude_nodes, float* logits_lowres_dev,
                                 int64_t* counts_dev, uint32_t* votes_dev, int accumulate, void* workspace_dev,
                                 size_t workspace_bytes, void* hip_stream) {
  return dropout_passes("nbc_dropout_votes", c, N, H, W, image_ids_host, p, seed, first_draw, draws, min_pixels, exclude_nodes,
                        logits_lowres_dev, counts_dev, true, votes_dev, accumulate, workspace_dev, workspace_bytes, hip_stream);
}
