// Launchers of the gfx950 kernels that another file than their own calls: the forward's (definitions in conv_igemm_dma.hip,
// conv3x3_rows.hip, pointwise.hip, aspp.hip, bn_stats.hip and efficientnet.hip) and the few a second pass shares (small_zones.hip,
// zones.hip, dropout_votes.hip, head_refit.hip).  A pass whose entry point is its launcher's only caller declares nothing here.
// The host functions among them that size a launch (conv_rows_kind, choose_conv_tile, *_slices, dwconv_tiles,
// bn_stats_workspace_bytes) are what nbc_plan.cpp builds the launch plan from.  Two rules of the launchers that are not
// convolutions are written here once: with_precision (the run-time precision as a template argument) and grid_stride_blocks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "conv_tiles.hpp"

namespace nbc {

// Implicit-GEMM convolution on NHWC activations, fused  y = relu?(acc*scale + shift (+ res)).
// GEMM view: rows m = (image, oy, ox), columns n = cout, K = (kh, kw, ci) in 128-byte K-steps.
struct ConvArgs {
  const void* x;        // [N][Hi][Wi][Ci] elements
  const void* w;        // [Co][ksteps*128 bytes]
  const float* scale;   // [Co]
  const float* shift;   // [Co]
  const void* res;      // nullable, [M][Co] elements (the identity of a bottleneck)
  void* y;              // [M][Co] elements
  unsigned x_bytes;     // size of x in bytes (< 2 GiB): the buffer resource's range check zero-fills halo and tail lanes
  unsigned w_bytes;     // size of w in bytes
  int N, Hi, Wi, Ci;
  int Ho, Wo, Co;
  int KH, KW, stride, pad, dil;
  int M;                // N*Ho*Wo
  int ksteps;
  int relu;
  int stem;             // one 16-byte chunk per tap (Ci*elem == 16 bytes)
  int wo_shift;         // log2(Wo) when Wo is a power of two, else -1
  int hw_shift;         // log2(Ho*Wo) when it is a power of two, else -1 (batches: image index without a division)
  // Dual-branch launch (f16x2; x2 != nullptr): this convolution is a 1x1, stride 1, unpadded conv3 of at most 8 K-steps with
  // res == nullptr, and its identity is computed in the same block by a 1x1 convolution (padding 0, no ReLU: downsample.0)
  // of x2 onto the same Ho x Wo x Co map -- see kVarDualBranch in conv_igemm_dma.hip.
  const void* x2;       // [N][Hi2][Wi2][Ci2] elements
  const void* w2;       // [Co][ksteps2*128 bytes]
  const float* scale2;  // [Co]
  const float* shift2;  // [Co]
  unsigned x2_bytes, w2_bytes;
  int Ci2, Hi2, Wi2, stride2, ksteps2;
#ifdef NBC_STAMPS
  unsigned long long* stamps;   // diagnostic build only (tools/conv_timeline.hip): 8 stamps per block
#endif
};

// precision: 0 = f32 (v_mfma_f32_32x32x2_f32), 1 = bf16 (v_mfma_f32_16x16x32_bf16 / v_mfma_f32_32x32x16_bf16),
// 2 = f16x2 (two f16 pieces per f32 value, three v_mfma_f32_16x16x32_f16 per product: split16.hpp)
// LDS-DMA ring (conv_igemm_dma.hip).  tile < 0 = choose_conv_tile(M, Co, K, precision).
// The tile menu -- ids, shapes, precisions, forms, cost-model constants, CONV_TILE_COUNT -- is the one table of conv_tiles.hpp; the host
// functions below (conv_tiles.cpp) read it.
int conv_tile_rows(int tile);
int conv_tile_cols(int tile);
// Whether a convolution runs on the row-resident 3x3 kernels (conv3x3_rows.hip; f16x2, 3x3, stride 1, no identity): 0 no;
// 1: 128-pixel-wide maps, >= 256 output channels; 2: 128-pixel-wide maps, 64 / 128 output channels.  A property of the layer and its
// shape that fixes its K order: it runs on the menu's tiles of its kind only, every other convolution on those of kind 0.
int conv_rows_kind(int precision, int k, int stride, int pad, int dil, int Hi, int Wi, int Ho, int Wo, int Ci, int Co, bool has_res);
bool conv_tile_ok(int precision, int tile, int Co, int rows_kind);   // the tile exists for the precision and the kind of convolution and divides Co
bool conv_tile_has_dual(int precision, int tile);   // the tile has the dual-branch form (ConvArgs::x2)
// K = Cin*kh*kw; the default tile of a layer (cost model); rows_kind: conv_rows_kind
int choose_conv_tile(int M, int Co, int K, int precision, int rows_kind);
hipError_t launch_conv_dma(const ConvArgs& a, int precision, int tile, hipStream_t s);
hipError_t launch_conv3x3_rows(const ConvArgs& a, int tile, hipStream_t s);   // tile: a row-step tile of the convolution's kind

// f(tag) with the run-time precision as a compile-time tag.value: 0 -> f32, 2 -> f16x2, anything else -> bf16 (the numbering of
// every `template <int PREC>` of stored.hpp's users).  The conv kernels keep their own dispatch (launch_conv_dma).
template <typename F>
inline auto with_precision(int precision, F&& f) {
  if (precision == 0) return f(std::integral_constant<int, 0>{});
  if (precision == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 1>{});
}

// Blocks of a grid-stride kernel over `items` items, one per thread and round: enough to cover them once, at most blocks_per_cu
// on each of the 256 CUs, at least one.
inline unsigned grid_stride_blocks(size_t items, int threads, int blocks_per_cu) {
  const size_t blocks = (items + threads - 1) / threads, cap = (size_t)256 * blocks_per_cu;
  return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// float32 NCHW [N,3,H,W] -> NHWC elements padded to 16 bytes per pixel.
hipError_t launch_ingest_f32(const float* x, void* y, int N, int H, int W, int precision, hipStream_t s);
// uint8 NHWC [N,H,W,3] -> same, applying (u8/255 - mean)/std in f32 (dataset.py:175-186).
hipError_t launch_ingest_u8(const uint8_t* x, void* y, int N, int H, int W, const float mean[3],
                            const float stdv[3], int precision, hipStream_t s);
// MaxPool2d(3, stride 2, padding 1) on NHWC, C a multiple of the 16-byte chunk.
hipError_t launch_maxpool3x3s2(const void* x, void* y, int N, int Hi, int Wi, int C, int Ho, int Wo,
                               int precision, hipStream_t s);
// classifier.4 (its pieces: head1x1.hpp): 1x1 conv cin -> 3 with bias; f32 weights [3][cin]; output f32 NCHW [N,3,h,w].
// cin = 512 (FCNHead: a wave per pixel) or 256 (DeepLabHead: a half-wave per pixel), anything else is an invalid value.
// counts_zero (nullable): the 3 * N class counters, cleared by this launch for the upsample/argmax launch that follows it,
// which accumulates the per-class pixel counts there (saves a memset node) -- when head_clears_counts(N), else the caller
// clears them.  nonfinite (nullable): one device word that gets bit 0 set when a logit is NaN or infinite.
inline bool head_clears_counts(int N) { return 3 * N <= 256; }   // one thread of block 0 per counter
hipError_t launch_head1x1(const void* x, int cin, const float* w, const float* bias, float* y, int N, int hw, int precision,
                          unsigned long long* counts_zero, unsigned* nonfinite, hipStream_t s);
// The same for f32 and any cin that is a multiple of 64, its chain in lane-strided channel order (lane l: channels l, l + 64, ...):
// the FCN head of every EfficientNet, whatever its width -- other bits than launch_head1x1 at cin = 512.
hipError_t launch_head1x1_any(const float* x, const float* w, const float* bias, float* y, int N, int hw, int cin,
                              unsigned long long* counts_zero, unsigned* nonfinite, hipStream_t s);
// The votes of a pass of the Dropout draws (dropout_votes.hip; the definition: votes.hpp): the final labels u8 [draws][N][P]
// of the pass are counted into the vote words u32 [N][P] -- stored when `first`, added to what is there otherwise.
// draws <= 65535 (a 16-bit field per class), votes 16-byte aligned for the vector path; labels at any address.
hipError_t launch_vote_accumulate(const unsigned char* labels, int draws, int N, long long P, uint32_t* votes, bool first,
                                  hipStream_t s);
// The adjoint of the bicubic upsample (h, w) -> (H, W) on three f64 planes per image (head_refit.hip: ce_col_adjoint along the rows of
// the image, then ce_row_adjoint down them): g [N][3] planes of H * W values, g_plane apart -> cols [N][3][H][w] -> out [N][3][h][w].
// The eight device tables are nbc_bicubic_taps' (the index and coefficient tables 16-byte aligned).  What nbc_ce_gradient and
// nbc_lovasz_gradient both end in: the same two launches, the same order of every sum.
struct BicubicTaps {
  const int32_t* row_idx;
  const float* row_coeff;
  const int32_t *row_lo, *row_hi, *col_idx;
  const float* col_coeff;
  const int32_t *col_lo, *col_hi;
};
hipError_t launch_bicubic_adjoint(const double* g, long long g_plane, int N, int H, int W, int h, int w, const BicubicTaps& taps,
                                  double* cols, double* out, hipStream_t s);
// ASPP pooling branch of every DeepLab head (aspp.hip), per image: mean over hw pixels of x [N][hw][cin] (stored elements; cin a
// multiple of 64, at most 4096), the 1x1 conv with f32 weights w [cout][cin], relu(fma(., scale, shift)), stored as y [N][cout]
// elements.  Workspaces: partial N * aspp_pool_slices(hw) * cin floats, mean N * cin floats.
int aspp_pool_slices(int hw);
hipError_t launch_aspp_pool(const void* x, int N, int hw, int cin, const float* w, const float* scale, const float* shift, int cout,
                            float* partial, float* mean, void* y, int precision, hipStream_t s);
// ASPP concat: y [N*hw][1280] elements = the four branches [N*hw][256] then the image's pooled vector [N][256], per pixel.
hipError_t launch_aspp_concat(const void* const branch[4], const void* pooled, void* y, int N, int hw, int precision,
                              hipStream_t s);
// Per-image BatchNorm (bn_stats.hip) of NHWC y [N][hw][C], C a power of two in [64, 2048], precision 0 or 2 (1: invalid value).
// bn_stats: per (image, channel) mean and biased variance over hw pixels in two levels over bn_stats_slices(hw) fixed slices
// (f64), then scale[n][c] = gamma[c] / sqrt(var + 1e-5), shift[n][c] = beta[c] - mean * scale.  ws: bn_stats_workspace_bytes(N,
// hw, C) bytes: the slice partials (N * slices * C * 16 bytes), then the two [N][C] tables, where bn_stats_tables finds them.
// bn_apply: in place, y = relu?(fma(y, scale, shift) (+ res)) with the tables bn_stats left in ws, res nullable.
// f16x2 (same slices, lane and slice orders, workspace): y holds 2^r_c x per channel c, inv_r[c] = 2^-r_c (nbc_pack_bn_raw); the
// statistics are those of x, the table is for the stored value and carries the power 2^a_out the normalised tensor (and res) is
// stored with: scale = f32(sc) 2^(a_out - r_c), shift = f32(beta - mean sc) 2^a_out.  word (nullable) gets bit
// NBC_NONFINITE_BN_RANGE when a channel's stored rms is not finite, above 2^12 or positive and below 2^-10.  f32 reads none of
// inv_r, a_out and word.
struct BnTables {
  float* scale;   // [N][C]
  float* shift;   // [N][C]
};
int bn_stats_slices(int hw);
size_t bn_stats_workspace_bytes(int N, int hw, int C);
BnTables bn_stats_tables(void* ws, int N, int hw, int C);
hipError_t launch_bn_stats(const void* y, int N, int hw, int C, const float* gamma, const float* beta, const float* inv_r, int a_out,
                           void* ws, unsigned* word, int precision, hipStream_t s);
hipError_t launch_bn_apply(void* y, const void* res, int N, int hw, int C, void* ws, int relu, int precision, hipStream_t s);
// EfficientNet (efficientnet.hip), f32 NHWC, C a multiple of 64.
// Depthwise k x k conv (k 3 / 5, stride 1 / 2) of x [N][Hi][Wi][C] with weights [k*k][C], top / left pads pad_t / pad_l
// (a tap outside the image reads 0), y [N][Ho][Wo][C] = swish(fma(acc, scale, shift)); in_swish: x is stored before its
// swish, applied as it is read.  partial [N][dwconv_tiles(stride, Ho, Wo)][C]: per tile the sum of its outputs (the SE
// squeeze's first level).
struct DwArgs {
  const float* x;
  const float* w;
  const float* scale;
  const float* shift;
  float* y;
  float* partial;
  int N, Hi, Wi, C, Ho, Wo, k, stride, pad_t, pad_l, in_swish;
};
int dwconv_tiles_x(int Wo);
int dwconv_tiles(int stride, int Ho, int Wo);
hipError_t launch_dwconv(const DwArgs& a, hipStream_t s);
// Per image: mean = (sum of the tiles' partials in tile order) / hw, r = swish(wr [cse][C] . mean + br),
// gate [N][C] = sigmoid(we [C][cse] . r + be).
hipError_t launch_se_excite(const float* partial, int N, int tiles, int C, int hw, const float* wr, const float* br, int cse,
                            const float* we, const float* be, float* gate, hipStream_t s);
// wg [N][Co][Ci] = w [Co][Ci] * gate [N][Ci] (the project conv's weights, gated per image)
hipError_t launch_gate_weights(const float* w, const float* gate, float* wg, int N, int Co, int Ci, hipStream_t s);
// y = swish(y) in place, elems a multiple of 4
hipError_t launch_swish(float* y, size_t elems, hipStream_t s);
// Bicubic (A=-0.75, align_corners=False) upsample of f32 NCHW [N,3,h,w] to HxW, fused with the
// per-pixel argmax, the optional 2->1 remap and the per-class pixel counts.  `offsets` (null = the plain argmax and the plain
// kernels): the pair nbc_set_logit_offsets holds, added to the bark and the node logit of the decision alone.
hipError_t launch_upsample_argmax(const float* lowres, int N, int h, int w, int H, int W,
                                  float* logits_full, void* labels, int labels_i64,
                                  unsigned long long* counts, int exclude_nodes, hipStream_t s, const float* offsets = nullptr);
// remove_small_zones (utils.py:135-148) in place on device labels (u8 or i64, [N,H,W]): 8-connected
// components below min_pixels of the non-background, then of the filled background, flip; optional
// 2 -> 1 remap and per-class counts afterwards.  Workspaces: bg N*H*W bytes, parent and size N*H*W ints.
// G > 1: consecutive groups of G images are volumes whose zones also link across images (small_zones.hip).
hipError_t launch_remove_small_zones(void* labels, int labels_i64, int N, int H, int W, int min_pixels, int exclude_nodes,
                                     unsigned char* bg, int* parent, int* size, unsigned long long* counts, hipStream_t s, int G = 1);
// The zones of label maps (zones.hip; the contract: nbc_label_zones in include/nbc.h): rows int64 [N][cap][10], num int64 [N].
// zones_layout: the regions of the workspace (byte offsets, each 256-byte aligned) and its size.  zone_match.hip labels twice
// with these, in two such regions.  zones_shape_ok: 1 <= N <= 65535, H and W in 1..65535, H * W < 2^31.
struct ZonesLayout {
  size_t parent, cls, blocks, total;         // int [N][H*W], u8 [N][H*W], int [N][ceil(H*W / 1024)]
};
bool zones_shape_ok(int N, int H, int W);
ZonesLayout zones_layout(int N, int H, int W);
hipError_t launch_label_zones(const void* labels, int labels_i64, int N, int H, int W, long long* rows, int cap, long long* num,
                              int* parent, unsigned char* cls, int* blocks, hipStream_t s);
// Preprocessor (models.py:191-203): uint8 HWC [H,W,3] -> ToTensor -> skimage cubic resize with reflected borders,
// clipped to the input range -> any of: float32 HWC [out_h,out_w,3]; its uint8 form as imsave writes it; per output
// row the number of pixels trim_black counts as lit.  minmax: two uints of scratch.
hipError_t launch_resize_cubic_u8(const uint8_t* src, int H, int W, float* dst, uint8_t* dst_u8, int* row_lit, int out_h, int out_w,
                                  unsigned* minmax, hipStream_t s);
// NHWC elements -> float32 NCHW (debug read-back of activations).
hipError_t launch_nhwc_to_nchw_f32(const void* x, float* y, int N, int H, int W, int C, int precision,
                                   hipStream_t s);

// Largest finite |value| of `elems` stored activation elements (C channels per pixel) as float bits, atomicMax-ed into *out.
hipError_t launch_absmax(const void* x, size_t elems, int C, int precision, unsigned* out, hipStream_t s);

}  // namespace nbc
