// The convolution tile menu: ONE row per tile id, and the only place a tile's facts are written down.  launch_tile()
// (conv_igemm_dma.hip) and launch_conv3x3_rows() (conv3x3_rows.hip) instantiate their kernels from it, conv_tiles.cpp answers
// every host question from it (conv_tile_rows / _cols / _ok / _has_dual, choose_conv_tile), and nbc_conv_tile_info hands it to
// whatever lives outside csrc/.  A new tile is one more row here -- and its kernel, if it is a new form of one.
#pragma once

namespace nbc {

// Constants of choose_conv_tile's cost model (conv_tiles.cpp) for one tile in one precision: eff / eff1 -- share of the per-CU
// matrix rate with `cap` blocks together / one block alone on its CU; ovh_us per group of blocks; cb scales the bytes term.
struct TileCost {
  double eff, eff1, ovh_us, cb;
  int cap;                              // blocks of the tile a CU holds at once (LDS and registers)
};

constexpr unsigned kTileLoaderWaves = 1;   // f16x2: four more waves that only issue the ring's LDS-DMAs (kVarLoaderWaves; a stem launch ignores it)
constexpr unsigned kTileDual = 2;          // f16x2: has the dual-branch form (ConvArgs::x2, kVarDualBranch)
constexpr unsigned kTileBigW = 4;          // f16x2: identity layers with 3 MiB of weights or more take the BIGW form

struct ConvTile {
  int kind;                             // 0: conv_dma_kernel; 1 / 2: the row-step 3x3 kernel, for convolutions of conv_rows_kind 1 / 2
  int wm, wn, mt, nt;                   // MFMA waves (pixels x channels) and the wave's tile in 32 x 32 units: the block is
                                        // wm*mt*32 pixels x wn*nt*32 channels.  Row-step tiles: two waves per 128-pixel output
                                        // row, so wm / 2 is the kernel's OR (output rows of a block)
  int s[3];                             // LDS stages per precision (f32, bf16, f16x2); 0: the precision has no such tile.
                                        // Row-step tiles: the kernel's SB (weight stages)
  unsigned flags;                       // kTile*
  double panel;                         // cost model: pixel rows fetched per pixel row of the tile and K (row-step: a row of 144 pixels
                                        // for 128, once for a kernel row's three taps; the two-row tile: four rows for six pairs)
  TileCost cost[3];                     // per precision
  constexpr int rows() const { return wm * mt * 32; }
  constexpr int cols() const { return wn * nt * 32; }
};

// Per-CU matrix rate (FLOPs per us) the efficiencies refer to: f32 157.3 TF / 256 CUs; bf16 against the 1 400 TF/s the chip
// sustains on this kernel (power-limited); f16x2 f32-equivalent FLOPs against the 839 TF/s three f16 MFMAs per product allow (2 517 / 3)
constexpr double kCuFlopsPerUs[3] = {157.3e6 / 256.0, 1400.0e6 / 256.0, 839.0e6 / 256.0};

// rows x cols = pixels x channels; waves m x n; "blocks/CU" is what the LDS ring (and the registers) allow.
constexpr ConvTile kConvTiles[] = {
    // 0: 128x64, 2x2 waves of 64x32, 72 KiB, 2 blocks/CU
    {0, 2, 2, 2, 1, {3, 3, 3}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.888, 0.888, 1.19, 0.91, 1}, {0.421, 0.38, 3, 0.3, 2}}},
    // 1: 128x128, 2x2 waves of 64x64, 64 KiB, 2 blocks/CU
    {0, 2, 2, 2, 2, {2, 2, 2}, kTileBigW, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.52, 0.36, 3, 0.3, 2}}},
    // 2: 256x128, 4x2 waves of 64x64, 144 KiB, 1 block/CU (no f16x2 form: it spills)
    {0, 4, 2, 2, 2, {3, 3, 0}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.5, 0.5, 3, 0.3, 1}}},
    // 3: 256x256, 2x4 waves of 128x64, 128 KiB, 1 block/CU (bf16 only: f32 keeps two accumulator sets, f16x2 has no 128x64 wave tiles)
    {0, 2, 4, 4, 2, {0, 2, 0}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.897, 0.897, 2.78, 1.07, 1}, {0.5, 0.5, 3, 0.3, 1}}},
    // 4: 128x128, 2x2 waves of 64x64, 128 KiB, 1 block/CU (deeper prefetch; f32 / bf16)
    {0, 2, 2, 2, 2, {4, 4, 0}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.5, 0.5, 3, 0.3, 1}}},
    // 5: 128x256, 2x4 waves of 64x64, 144 KiB, 1 block/CU
    {0, 2, 4, 2, 2, {3, 3, 3}, 0, 1, {{0.896, 0.896, 4.0, 0, 1}, {0.911, 0.911, 4.0, 0.78, 1}, {0.535, 0.535, 3.45, 0.3, 1}}},
    // 6: 256x64, 4x2 waves of 64x32, 120 KiB, 1 block/CU
    {0, 4, 2, 2, 1, {3, 3, 3}, 0, 1, {{0.722, 0.722, 5.08, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.42, 0.42, 3.007, 0.309, 1}}},
    // 7: 128x64, 2x2 waves of 64x32, 48 KiB, 3 blocks/CU (short-K layers: K fits two stages)
    {0, 2, 2, 2, 1, {2, 2, 2}, 0, 1, {{0.811, 0.811, 3.14, 0, 1}, {0.85, 0.85, 0.0, 1.03, 1}, {0.476, 0.383, 3, 0.31, 3}}},
    // 8: 64x128, 1x4 waves of 64x32, 48 KiB, 3 blocks/CU (dual-branch form: conv3 of layer1.0 .. layer3.0 on small images)
    {0, 1, 4, 2, 1, {2, 2, 2}, kTileDual, 1, {{0.894, 0.894, 0.76, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.42, 0.36, 2.746, 0.272, 3}}},
    // 9: 128x128, 4x2 waves of 32x64, bf16 70 KiB, 2 blocks/CU; f32 three stages (96 KiB, fragment prefetch), f16x2 three as well
    //    (9 - 11: 8 / 16 waves for short-K layers, where the serial prologue/epilogue code dominates and more waves run it in parallel)
    {0, 4, 2, 1, 2, {3, 2, 3}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.754, 0.754, 0.5, 0.68, 1}, {0.42, 0.42, 3, 0.3, 1}}},
    // 10: 128x64, 4x2 waves of 32x32, bf16 48 KiB, 3 blocks/CU; f32 three stages (72 KiB, two blocks per CU), f16x2 three as well
    //     (dual-branch form: as 8)
    {0, 4, 2, 1, 1, {3, 2, 3}, kTileDual, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.455, 0.392, 2.868, 0.3, 2}}},
    // 11: 256x128, 4x4 waves of 64x32, 96 KiB, 1 block/CU (f16x2 has no 16-wave blocks)
    {0, 4, 4, 2, 1, {2, 2, 0}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.85, 0.85, 4.0, 1.0, 1}, {0.5, 0.5, 3, 0.3, 1}}},
    // 12: 256x256, 4x4 waves of 64x64, 128 KiB, 1 block/CU (bf16 only -- f32: 128-register budget --: short-K layers at batch >= 2;
    //     the matrix pipe is busier than with 8 waves, the clock lower: same TFLOP/s on long-K layers, 2-5 % faster
    //     epilogue-heavy 1x1 layers)
    {0, 4, 4, 2, 2, {0, 2, 0}, 0, 1, {{0.85, 0.85, 4.0, 0, 1}, {0.85, 0.85, 3.61, 1.0, 1}, {0.5, 0.5, 3, 0.3, 1}}},
    // 13: 128x128, 2x4 waves of 64x32, 96 KiB, 1 block/CU (8 waves)
    {0, 2, 4, 2, 1, {3, 3, 3}, 0, 1, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.44, 0.44, 2.518, 0.3, 1}}},
    // 14 - 17 are f16x2's (in bf16 a 256x128 tile with loader waves ties the one without: DESIGN.md section 6.4).
    // 14: 128x128, 2x4 + 4 waves of 64x32, 96 KiB, 1 block/CU (13 with four loader waves: the tile of a layer whose 128x128
    //     tiles number 256 or fewer, one per CU: layer3 at batch 1)
    {0, 2, 4, 2, 1, {0, 0, 3}, kTileLoaderWaves | kTileBigW, 1, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.47, 0.47, 3.874, 0.3, 1}}},
    // 15: 128x64, 4x2 + 4 waves of 32x32, 72 KiB, 1 block/CU (10 with four loader waves; layer2's 3x3 at batch 1)
    {0, 4, 2, 1, 1, {0, 0, 3}, kTileLoaderWaves, 1, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.4, 0.4, 3, 0.3, 1}}},
    // 16: 128x128, 2x2 + 4 waves of 64x64, 96 KiB, 1 block/CU (four MFMA waves + four loader waves: ties 14)
    {0, 2, 2, 2, 2, {0, 0, 3}, kTileLoaderWaves, 1, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.448, 0.448, 3, 0.3, 1}}},
    // 17: 128x128, 2x4 waves of 64x32, 64 KiB, 2 blocks/CU (13 with two stages at 128 registers: one block's barrier waits, prologue
    //     and epilogue under the other's MFMAs; the tile of every layer with two or more 128x128 tiles per CU: 0.51 of the mode's peak
    //     on the head conv and layer4's 3x3 against 0.45 for tile 14.  Dual-branch form: conv3 of layer1.0 .. layer3.0 at full size)
    {0, 2, 4, 2, 1, {0, 0, 2}, kTileDual | kTileBigW, 1, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.501, 0.36, 3.321, 0.195, 2}}},
    // The row-step kernel (conv3x3_rows.hip; f16x2): the pixel row stays in LDS for its three taps, one barrier per (channel block, kh).
    // 18: 128x128, ONE image row x 128 channels, eight 64x32 MFMA waves + four loader waves, 154 KiB: the 3x3 layers of 128-pixel-wide
    //     maps with 256 output channels or more run on it or on tile 20
    {1, 2, 4, 2, 1, {0, 0, 2}, 0, 1.125 / 3, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.50, 0.50, 4.0, 0.2, 1}}},
    // 19: 128x64, one image row x 64 channels, four MFMA + four loader waves, 128 KiB: likewise those with 64 / 128 output channels
    //     (layer2.1-3 conv2)
    {2, 2, 2, 2, 1, {0, 0, 3}, 0, 1.125 / 3, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.45, 0.45, 3.0, 0.3, 1}}},
    // 20: 256x64, TWO image rows, a dilation apart, x 64 channels, eight MFMA + four loader waves, 124 KiB: the layers of tile 18, same
    //     K order and bits, 27 % fewer bytes into LDS per product: their default
    {1, 4, 2, 2, 1, {0, 0, 2}, 0, 1.125 / 4, {{0.80, 0.80, 4.0, 0, 1}, {0.80, 0.80, 4.0, 1.0, 1}, {0.515, 0.515, 4.0, 0.2, 1}}},
};
constexpr int CONV_TILE_COUNT = sizeof(kConvTiles) / sizeof(kConvTiles[0]);

}  // namespace nbc
