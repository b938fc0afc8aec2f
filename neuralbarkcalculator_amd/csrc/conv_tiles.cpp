// Host logic over the tile menu (conv_tiles.hpp): which tile exists for what, and the default tile of a layer.
#include "../../include/nbc.h"
#include "nbc_kernels.hpp"

namespace nbc {

int conv_tile_rows(int tile) { return tile >= 0 && tile < CONV_TILE_COUNT ? kConvTiles[tile].rows() : 0; }
int conv_tile_cols(int tile) { return tile >= 0 && tile < CONV_TILE_COUNT ? kConvTiles[tile].cols() : 0; }

// Whether tile id `tile` exists for this precision and kind of convolution and divides the layer's output channels.
bool conv_tile_ok(int precision, int tile, int Co, int rows_kind) {
  if (tile < 0 || tile >= CONV_TILE_COUNT || precision < 0 || precision > 2) return false;
  const ConvTile& t = kConvTiles[tile];
  // the row-step 3x3 kernel's tiles and the generic ones are never mixed: refused for the wrong kind before the precision is
  // looked at (nbc_forward's tile_of: "does not fit -> planned tile")
  if (rows_kind != t.kind) return false;
  return t.s[precision] != 0 && Co % t.cols() == 0;
}

bool conv_tile_has_dual(int precision, int tile) {
  return precision == 2 && tile >= 0 && tile < CONV_TILE_COUNT && (kConvTiles[tile].flags & kTileDual) != 0;
}

// Whether a convolution runs on the row-step kernels (conv3x3_rows.hip; f16x2): 3x3, stride 1, padding = dilation <= 8, no identity, and
//   kind 1: 128-pixel-wide maps, 256 output channels or more (layer3 / layer4 conv2, classifier.0 of a 1024-pixel-wide image):
//           the two tiles of that kind (the same K order and bits; the cost model's default is the two-row one);
//   kind 2: 128-pixel-wide maps, 64 or 128 output channels (layer2.1-3 conv2): the one tile of that kind;
//   0: neither (the generic kernel).  A property of the layer and its shape: the K order follows from it (the head of that file).
int conv_rows_kind(int precision, int k, int stride, int pad, int dil, int Hi, int Wi, int Ho, int Wo, int Ci, int Co, bool has_res) {
  if (!(precision == 2 && k == 3 && stride == 1 && pad == dil && dil >= 1 && dil <= 8 && Ho == Hi && Wo == Wi && Ci % 32 == 0 && !has_res)) return 0;
  if (Wi == 128 && Co >= 256 && Co % 128 == 0) return 1;
  // (maps of 256 pixels -- layer1's conv2, two segments per row -- run on this kernel as well, and no faster than on the generic
  // tiles, which keep two blocks per CU there: profiles/r05_rowstep_kernel_layer1_layer2.log; left to them)
  if (Wi == 128 && Co % 64 == 0 && Co < 256) return 2;
  return 0;
}

// Default tile of a layer (what runs unless nbc_autotune has measured): the cheapest under a small cost model.
// A launch takes as long as the CU with the most blocks: b = ceil(blocks / 256) of them, run in groups of cap[t] -- the
// blocks of that tile a CU holds at once (LDS and registers): they share its matrix pipes, and their prologues and
// epilogues overlap -- that is g = b / cap full groups and a rest of r = b % cap blocks:
//   (g * cap / eff[t] + r / eff_r) * tile FLOPs / per-CU matrix rate  +  b * tile bytes * cb[t] / (50 GB/s)  +  ceil(b / cap) * ovh[t]
// (K = Cin*kh*kw products per output; tile bytes = the (rows + cols) x K operand panels + twice the output tile; eff_r
// lies between eff1[t], one block alone on its CU, and eff[t], cap blocks together).  What matters most is the block
// count: a 640x1024 image has 10 240 pixels at stride 8, so the head conv on 128x128 tiles is 320 blocks = two rounds of
// which the second is a quarter full, on 64x128 tiles 640 blocks = three per CU, a third faster; and whether a tile's
// blocks come in pairs: the f16x2 128x128 tile of eight waves at two blocks per CU runs the long-K layers at 0.51 of
// the mode's peak when every CU has two (or four) of them and at 0.33 when it has one, where the one-block-per-CU tiles
// (14 with loader waves, 5 with 64x64 wave tiles) reach 0.40-0.55.  Constants fitted to per-layer timings of every tile (scripts/tile_model_probe.py,
// scripts/fit_tile_model.py): f32 and bf16 on 28 (precision, batch, height) cases (profiles/r02_tile_model_fit.log:
// within 0.1-0.5 % (f32) / 0.4-4.4 % (bf16) of the per-layer best, which is where nbc_autotune lands too); f16x2 on
// eight cases (profiles/r04_tile_model_fit_f16x2.log: 0.2-1.6 % from the per-layer best, 0.9 % on average, and the same when
// every constant is perturbed by +-2 %: no choice sits on a knife edge).
int choose_conv_tile(int M, int Co, int K, int precision, int rows_kind) {
  if (precision < 0 || precision > 2) return -1;
  const double eb = precision == 1 ? 2.0 : 4.0;
  int best = -1;
  double best_cost = 0.0, best_area = 0.0;
  for (int t = 0; t < CONV_TILE_COUNT; ++t) {
    if (!conv_tile_ok(precision, t, Co, rows_kind)) continue;
    const TileCost& c = kConvTiles[t].cost[precision];
    const int irows = kConvTiles[t].rows(), icols = kConvTiles[t].cols();
    const double trows = irows, cols = icols;
    const long long blocks = (long long)((M + irows - 1) / irows) * (Co / icols);
    const long long b = (blocks + 255) / 256;
    const int cap = c.cap;
    const long long g = b / cap, rest = b % cap;
    const double eff_r = cap > 1 && rest > 0 ? c.eff1 + (c.eff - c.eff1) * (double)(rest - 1) / (double)(cap - 1) : c.eff;
    const double flops = trows * cols * 2.0 * K;
    const double prows = trows * kConvTiles[t].panel;        // operand panels per block
    const double bytes = (prows + cols) * K * eb + trows * cols * eb * 2.0;
    const double cost = ((double)(g * cap) / c.eff + (double)rest / eff_r) * flops / kCuFlopsPerUs[precision] +
                        (double)b * bytes * c.cb / 50.0e3 + (double)((b + cap - 1) / cap) * c.ovh_us;
    // ties (to 1e-9 relative) go to the larger tile: fewer L2 -> LDS bytes per FLOP
    if (best < 0 || cost < best_cost * (1.0 - 1e-9) || (cost <= best_cost * (1.0 + 1e-9) && trows * cols > best_area)) {
      best = t;
      best_cost = cost;
      best_area = trows * cols;
    }
  }
  return best;
}

}  // namespace nbc

extern "C" int nbc_conv_tile_info(int precision, int tile, int32_t* rows, int32_t* cols, int32_t* kind, int32_t* has_dual) {
  using namespace nbc;
  if (tile < 0 || tile >= CONV_TILE_COUNT || precision < 0 || precision > 2 || kConvTiles[tile].s[precision] == 0) return 0;
  if (rows) *rows = kConvTiles[tile].rows();
  if (cols) *cols = kConvTiles[tile].cols();
  if (kind) *kind = kConvTiles[tile].kind;
  if (has_dual) *has_dual = conv_tile_has_dual(precision, tile);
  return 1;
}
