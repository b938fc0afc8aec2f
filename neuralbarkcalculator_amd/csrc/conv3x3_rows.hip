// 3x3 stride-1 convolution on 128-pixel-wide feature maps in f16x2 (NBC_PREC_F16X2) whose pixel rows STAY IN LDS for the three
// taps of a kernel row, one barrier per ROW-STEP: layer3 / layer4 conv2 and classifier.0 (tiles 18 and 20) and layer2.1-3 conv2
// (tile 19) of a 1024-pixel-wide image -- half of the forward's time.
//
// Why.  The generic kernel (conv_igemm_dma.hip) fetches, for every K-step (tap, 32-channel block), the 128 pixel rows of its
// tile again: 16 KiB of pixels + 16-32 KiB of weights per step from L2 into LDS, behind one barrier per K-step.  Measured in the
// network (profiles/r05_f16x2_kloop_ablations_in_network.log): the head conv's K loop WITHOUT a single MFMA or fragment read --
// LDS-DMA and barriers only -- takes 423 of its 738 us (7.25 GB at 17 TB/s, the L2 -> LDS gather rate of this chip), the same
// loop without its DMAs 496: the L2 -> LDS stream is a bottleneck of its own beside the matrix pipe, and the chip's power
// limit couples the two.  The three taps (kh, kw = 0, 1, 2) of a kernel row read the SAME input row shifted by the dilation.
// Here a pipeline step is a ROW-STEP (channel block, kh): one input row (128 + 2 dil pixels x 128 bytes of the channel block,
// zero halo from the buffer resource's range check) fetched ONCE into a row slot and read by its three K-steps (kw) at a
// shifted pixel index, the three taps' weight panels in flight with it, ONE barrier and one LDS-DMA round trip for three
// K-steps of MFMAs.  Pixel traffic falls to a third (22 KiB per K-step where the generic 128 x 128 tile fetches 32, the
// 128 x 256 tile 48 for twice the outputs), barriers and round trips to a third.
// Measured (profiles/r05_rows_kernel_*.log, r05_rows_tile18_one_barrier_per_rowstep.log): the head conv 738 -> 680 us,
// layer4's conv2 187 -> 174, layer3's 57 -> 51, layer2.1-3's 23.5 -> 20.5; the forward +2.9 %.
// Tile 20 then takes TWO output rows a dilation apart x 64 channels per block: four input rows per channel block serve six (output
// row, kernel row) pairs and a weight panel is half as wide -- 72 KiB into LDS per output row and channel block where tile 18
// moves 99; same K order per output, same bits: head conv -2.3 ... -3.1 %, layer4's conv2 -1.4 ... -2.4 %, layer3's -1 %, the forward
// +1.4 % (profiles/r05_rowstep_two_output_rows.log).
// (Built, measured and removed on the way, same logs: the same rows with one barrier per K-step -- 128 x 128 with loader waves
// and a 256 x 128 tile of 64 x 64 wave tiles that halves the weight traffic as well: +2.0 % on the forward, every layer
// slower than on this kernel; 64 x 64 wave tiles here: +2-4 % time.)
//
// K order.  (channel block, kh, kw) -- the generic kernel walks (kh, kw, channel block).  The order is a property of the
// LAYER AND SHAPE, never of the tile: a convolution these kernels take (conv_rows_kind) runs on its one tile whatever the
// caller forces or the autotuner measures, so logits stay bit-identical across tiles.
//
// The sums.  Per 16x16 tile and K-step the same three products on v_mfma_f32_16x16x32_f16 as the generic kernel's, from the same
// fragments in the same order (f16x2_mma.hpp): P.X0 and Q.X0 into the chain that joins the running f32 sum every eighth K-step --
// and the low-piece product as P.X1, P AS STORED, into a third set `low` that runs over the tile's whole K loop and joins once
// behind it, sum = fma(low, 2^-11, sum) (x2_products_low, x2_join_low).  The generic kernel forms P 2^-11 in every K-step, eight
// v_pk_mul_f16 per 24 MFMAs, because its third products share the chain: its tiles have no registers for a third set.  A block
// here is alone on its compute unit with twelve waves, three per SIMD (tile 19: eight, two), which may take 168 registers each; the
// kernel takes 144-146 (116 before), no spill, no scratch, and its MFMA waves issue nothing in the loop but fragment reads and
// MFMAs.  Measured (profiles/rowstep_low_sum_*, one stream traced ... one process untraced): head conv -1.5 ... -3 %, layer4's
// conv2 -1 ... -2.5 %, layer3's -1 ... -2 %, layer2.1-3's -5 ... -8 %; the forward with two forwards in flight +1.0 %, all that a
// timing-only build without the multiply gave.  `low` is zeroed with the other two sets at a tile's
// start, a walking block's every tile included, and x2_flush never touches it; its K additions round at 2^-11 of the chain's
// scale.  f32 BN + ReLU epilogue through a per-wave LDS transpose, whole 256-byte row segments stored, as the generic
// kernel's.  This file reads the fragments and walks the tiles.
//
// LDS: three row slots (slot = kh: a channel block's three kernel rows; tile 20: four, its four input rows) of 144 pixels x 128 bytes, their 16-byte chunks
// rotated by the pixel index so that a fragment block may start at ANY pixel without bank conflicts (row_off), and two or
// three stages of three weight panels (one per kw).
//
// The tile walk (tiles 18 and 20).  A block of tile 20 takes 124 KiB of LDS and twelve waves: a compute unit holds ONE, and nothing
// becomes resident beside it.  With more tiles than compute units (the head conv and layer4's conv2 at 1024 x 1024: 512 tiles, two
// per unit) the epilogue of a unit's first tile, the exit of its waves, the dispatch of the next block, its index arithmetic, its
// table and the round trip of its first row-step ran strictly one after the other, no MFMA in flight.  So a launch has
// min(tiles, compute units) blocks, and block b computes tiles b, b + blocks, b + 2 blocks, ... -- each through the same
// XCD-aware index map, each exactly as a block of its own would (image, row pair, segment, channel tile, K order): which block
// computes which tile changes no bit.  After the barrier that ends a tile's K loop the loader waves do not leave: they request
// the next tile's scale/shift table and its first row-step (pixel slots 0 [and 1], weight stage 0) at once and go on with the
// usual protocol, while the MFMA waves run the epilogue and meet them at the next tile's first barrier with zeroed accumulators.
// The last tile of a block, or the only one, ends as before: the loaders leave after its K loop.
//   LDS of a walking block, tile 20 (tile 18): bytes
//          0 ..  73 728 ( 55 296)  four (three) pixel slots of 18 432; the epilogue scratch (eight waves x 32 rows x 144 bytes =
//                                  36 864) lies on the LAST TWO, from 36 864 (18 432): the next tile's first row-step does not
//                                  touch them, and its second is requested after that tile's first barrier, which every MFMA
//                                  wave reaches with its last scratch read behind it;
//     73 728 .. 122 880 (153 600)  two weight stages of 3 x 64 (128) x 128;
//    122 880 .. 126 976 (157 696)  two scale/shift tables of 2 048, one per tile in flight, used in turn: 124 KiB (154 KiB).
//   Waits.  Every LDS-DMA of the next tile, table included, is issued by the loader waves, which count their own vmcnt alone and
//   have nothing else in flight: the waits stay exact.  The MFMA waves still issue no load in the loop and wait for no vmcnt;
//   their epilogue's stores count on THEIR vmcnt, which no loader wave waits on, and are left to retire under the next K loop.
//   Registers of the MFMA waves: as a block of one tile (each tile computes its fragment and epilogue addressing anew).
#include "f16x2_mma.hpp"
#include "nbc_kernels.hpp"

namespace nbc {
namespace {

constexpr int kRowPx = 144;                         // pixels of a row slot: 128 + 2 * dil, dil <= 8, in whole 8-pixel DMAs
constexpr int kRowBytes = kRowPx * 128;
constexpr int kRowParts = kRowPx / 8 / 3;           // LDS-DMAs (8 pixels each) of one row per K-step: a row in three parts
static_assert(kRowParts * 24 == kRowPx && kRowParts % 2 == 0, "a row slot is three even parts of whole 8-pixel DMAs");

// Tile 20: the output rows of an image in pairs (oy, oy + dil): whole groups of 2 dil rows hold dil pairs each (pair q of group g: rows
// g 2 dil + q and + dil), a last group of fewer rows one pair per row of its first half (the second row of such a pair may lie below
// the image: computed on zero rows, not stored).  Pair index -> first row: (pr / dil) 2 dil + pr % dil in both cases.
__host__ __device__ inline int rowstep_pairs(int Ho, int dil) {
  const int groups = Ho / (2 * dil), rem = Ho - groups * 2 * dil;
  return groups * dil + (rem < dil ? rem : dil);
}

// Tiles 18 and 20 (SB 2) WALK: a launch has one block per compute unit at the most, and block b computes tiles b, b + blocks, ...
// (the kernel's comment).  LDS of a launch: the pixel slots, SB weight stages and a 2-KiB scale/shift table, two for a walking kernel.
constexpr bool rowstep_walks(int SB) { return SB == 2; }
constexpr int rowstep_tables(int SB) { return rowstep_walks(SB) ? 2 : 1; }
constexpr int rowstep_lds_bytes(int BN, int SB, int OR) { return (OR == 2 ? 4 : 3) * kRowBytes + SB * 3 * BN * 128 + rowstep_tables(SB) * 2048; }
static_assert(rowstep_lds_bytes(64, 2, 2) == 124 * 1024 && rowstep_lds_bytes(128, 2, 1) == 154 * 1024 && rowstep_lds_bytes(64, 3, 1) == 128 * 1024,
              "tile 20: 124 KiB, tile 18: 154 KiB, tile 19: 128 KiB of the CU's 160");

// Epilogue: the pieces of f16x2_mma.hpp, as conv_igemm_dma.hip's f16x2 path calls them, without identity: BN on the accumulators
// into a per-wave f32 scratch in the idle ring, read back row-wise, ReLU, split, whole row segments stored.
// acc16[j][i]: lane (r16, q16) holds pixel i*16 + r16 and channels j*16 + 4*q16 .. +3 of the wave's (MT*32) x (NT*32) tile.
// scratch: the block's scratch in LDS (CW x 32 x PITCH bytes, a slab per wave); table: the tile's scale/shift table.
template <int CW, int MT, int NT>
__device__ __forceinline__ void rows_epilogue(const ConvArgs& p, unsigned char* scratch, const unsigned char* table_base, f32x4 (&acc16)[2 * NT][2 * MT],
                                              int wave, int lane, int wm, int wn, int m0, int n0) {
  typedef EpiGeom<NT, 2> G;
  const int o_pix = lane / G::CPR, o_chunk = lane % G::CPR;
  const unsigned row_bytes = (unsigned)p.Co * 4u, lane_chunk = G::lane_chunk(o_chunk);
  unsigned char* ytile = static_cast<unsigned char*>(p.y) + ((size_t)m0 * p.Co + n0 + wn * G::SLAB_CH) * 4;
  const int rows_valid = p.M - m0;
  unsigned char* scr = scratch + wave * (32 * G::PITCH);
  const unsigned char* table = table_base + wn * G::SLAB_CH * 4;
  const bool relu = p.relu != 0;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    bn16_to_scratch<G::PITCH, false>(scr, table, acc16, acc16, i, lane & 15, lane >> 4);
    float v[G::PASSES][8];
    epi_read_rows<G>(scr, o_pix, o_chunk, v);
#pragma unroll
    for (int ps2 = 0; ps2 < G::PASSES; ++ps2) {
      const int row = wm * MT * 32 + o_pix + i * 32 + ps2 * G::PIX_PER_PASS;
      x2_store(v[ps2], relu, ytile + ((unsigned)row * row_bytes + lane_chunk), row < rows_valid);
    }
  }
}

// 128 pixels (an image row; a 128-pixel segment of a wider one) x BN = WN * NT * 32 channels per block: 2 x WN MFMA waves of
// 64 x (NT * 32) and four loader waves; three row slots of 18 KiB and SB stages of 3 x BN x 128 bytes of weights: a stage is
// refilled a whole row-step (three K-steps of MFMAs) ahead.
//   tile 18: WN 4 -> 128 channels, eight MFMA waves, SB 2 (150 KiB + tables): 256 output channels or more;
//   tile 19: WN 2 ->  64 channels, four MFMA waves,  SB 3 (126 KiB + table): the 64 / 128-channel layers, whose K loop ran at one
//            LDS-DMA round trip per K-step (DMA and barriers alone: 19-21 of their 21-25 us).
//   tile 20: OR 2, WN 2 -> TWO output rows (oy and oy + dilation: four input rows between them instead of six) x 64 channels,
//            eight MFMA waves (output row x pixel half x channel half), SB 2 (120 KiB + tables): per output row and channel block 72 KiB
//            of pixels and weights where tile 18 moves 99; the same K order per output, so the same bits as tile 18.
template <int WN, int NT, int SB, int OR>
__global__ __launch_bounds__((2 * WN * OR + 4) * 64, (2 * WN * OR + 4) / 4) void conv3x3_rowstep_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  static_assert(OR == 1 || (OR == 2 && SB == 2), "two output rows per block: every row-step's DMAs are waited for in full");
  constexpr int WM = 2, MT = 2, CW = WM * WN * OR, NW = 4;   // 2 x WN (x OR) MFMA waves of 64 x (NT * 32), four loader waves
  constexpr int BN = WN * NT * 32;
  constexpr bool WALK = rowstep_walks(SB);
  // pixel-row slots.  OR 1: slot = kh.  OR 2: slot k = input row oy + (k - 1) dil; row-step kh reads slots kh (first output row) and
  // kh + 1 (second): slots 0 and 1 are requested with kh 0's weights, 2 with kh 1's, 3 with kh 2's, each a row-step ahead, into a slot
  // last read two row-steps before.  (Rows requested TWO row-steps ahead through a ring of six slots: the same times,
  // profiles/r05_rowstep_two_output_rows.log.)
  constexpr int NSLOT = OR == 2 ? 4 : 3;
  constexpr int A_SLOT = kRowBytes, A_REGION = NSLOT * A_SLOT;
  constexpr int B_TAP = BN * 128, B_STEP = 3 * B_TAP;
  constexpr int TABLE_OFF = A_REGION + SB * B_STEP;   // the ring; the epilogue scratch (18 / 36 KiB) lies inside it
  // The epilogue scratch.  A walking block's loaders fill the next tile's first row-step (pixel slots 0 [and 1], weight stage 0) and
  // its table while the MFMA waves are in this tile's epilogue: the scratch lies on the LAST two pixel slots, which the next tile
  // requests only after its first barrier, and each of two tiles in flight has a table of its own.
  constexpr int SCRATCH = CW * 32 * (NT * 32 * 4 + 16);
  constexpr int SCRATCH_OFF = WALK ? (NSLOT - 2) * A_SLOT : 0;
  constexpr int FIRST_SLOTS = OR == 2 ? 2 : 1;        // pixel slots of a tile's first row-step
  static_assert(!WALK || SB == 2, "a walking block runs one row-step ahead: weight stage 0 and the first row-step's slots");
  static_assert(SCRATCH_OFF >= (WALK ? FIRST_SLOTS * A_SLOT : 0), "the scratch must not lie on the next tile's first row-step");
  static_assert(SCRATCH_OFF + SCRATCH <= A_REGION, "the scratch lies on pixel slots, below the weight stages and the tables");
  static_assert(TABLE_OFF + rowstep_tables(SB) * 2048 == rowstep_lds_bytes(BN, SB, OR), "the launch's LDS size is this layout");
  constexpr int NA = kRowPx / 8;                       // 18 pixel DMAs per row-step
  constexpr int LA_HI = (NA + NW - 1) / NW, LA_LO = NA / NW;
  constexpr int NBW = (BN / 8) / NW;                  // weight DMAs per loading wave and tap
  constexpr int LB = 3 * NBW;                         // ... and row-step
  constexpr int MT16 = 2 * MT, NT16 = 2 * NT;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_loader = wave >= CW;
  const int lw = __builtin_amdgcn_readfirstlane((wave - CW) & (NW - 1));
  const bool la_hi = lw < NA % NW;

  const int dil = p.dil;
  // OR 2: the output rows of an image in pairs (oy, oy + dil): rowstep_pairs
  const int pairs = OR == 2 ? rowstep_pairs(p.Ho, dil) : p.Ho;
  const int NH = p.N * pairs;
  const int segs = p.Wo / 128;                         // 128-pixel segments per row
  const int tiles_n = p.Co / BN;
  const int tiles_m = NH * segs;
  const int nblk = tiles_m * tiles_n;
  // tile tl of the launch (block b: tl = b, b + gridDim.x, ...): channel tile, image, (first) output row and segment
  struct Tile { int n0, img, oy, seg; };
  auto tile_at = [&](int tl) __attribute__((always_inline)) {
    const int bid = xcd_tile(tl, nblk);
    const int tile_n = bid % tiles_n, tile_m = bid / tiles_n;
    const int R = tile_m / segs, seg = tile_m - R * segs;
    const int img = R / pairs, pr = R - img * pairs;
    return Tile{tile_n * BN, img, OR == 2 ? (pr / dil) * 2 * dil + pr % dil : pr, seg};
  };

  const rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, p.x_bytes, 0x00020000);
  const rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
  const int pix_bytes = p.Ci * 4;
  const int cblocks = pix_bytes / 128;
  const int T = p.ksteps, RS = 3 * cblocks;
  const unsigned wrow_bytes = (unsigned)T * 128u;
  const unsigned tap_stride = (unsigned)cblocks * 128u;
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  const unsigned smem_base = (unsigned)(size_t)(lds_u8*)smem;

  if (is_loader) {
    const int lp = lane >> 3, ps = lane & 7;
    const int la = la_hi ? LA_HI : LA_LO;
    // Tile after tile.  The barrier that ends a tile's K loop retires every read of the ring, so the next tile's table and first
    // row-step go out at once, beside the MFMA waves' epilogue; the last tile's loaders leave there.
    for (int tl = blockIdx.x, table = TABLE_OFF;;) {
      const Tile c = tile_at(tl);
      const int n0 = c.n0, img = c.img, oy = c.oy, seg = c.seg;
      if (wave == CW && lane < BN / 4) dma_scale_shift(p.scale, p.shift, n0, lane, smem_base + (unsigned)table);
      unsigned w_off[NBW], a_col[LA_HI];
#pragma unroll
      for (int i = 0; i < NBW; ++i) {
        const int row = (lw + NW * i) * 8 + lp;
        w_off[i] = (unsigned)(n0 + row) * wrow_bytes + (unsigned)(ps ^ ((row >> 1) & 7)) * 16u;
      }
#pragma unroll
      for (int d = 0; d < LA_HI; ++d) {
        const int pp = (lw + NW * d) * 8 + lp;            // slot pixel
        const int ix = seg * 128 + pp - dil;
        const unsigned chunk = (unsigned)((ps - 2 * ((pp >> 1) & 3)) & 7) * 16u;
        a_col[d] = (unsigned)ix < (unsigned)p.Wi ? (unsigned)ix * (unsigned)pix_bytes + chunk : kOutOfRange;
      }
      int i_cb = 0, i_kh = 0, i_sb = 0;                   // the row-step issued next: channel block, kh (= its pixel slot), weight stage
      auto issue_row = [&](int k, int cb, int slot) __attribute__((always_inline)) {     // input row oy + (k - 1) dil of channel block cb
        const int iy = oy + (k - 1) * dil;
        const bool rowok = (unsigned)iy < (unsigned)p.Hi;
        const unsigned rowoff = (unsigned)((img * p.Hi + iy) * p.Wi) * (unsigned)pix_bytes;
#pragma unroll
        for (int d = 0; d < LA_HI; ++d)
          if (d < la)
            dma16_buf(rowok ? a_col[d] + rowoff : kOutOfRange, xrsrc, smem_base + (unsigned)(slot * A_SLOT) + (unsigned)(lw + NW * d) * 1024u,
                      (unsigned)cb * 128u);
      };
      auto issue_rowstep = [&]() __attribute__((always_inline)) {
        if constexpr (OR == 1) issue_row(i_kh, i_cb, i_kh);
        else if (i_kh == 0) { issue_row(0, i_cb, 0); issue_row(1, i_cb, 1); }
        else issue_row(i_kh + 1, i_cb, i_kh + 1);
        const unsigned soff = ((unsigned)(3 * i_kh) * (unsigned)cblocks + (unsigned)i_cb) * 128u;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int i = 0; i < NBW; ++i)
            dma16_buf(w_off[i], wrsrc, smem_base + (unsigned)(A_REGION + i_sb * B_STEP + kw * B_TAP) + (unsigned)(lw + NW * i) * 1024u,
                      soff + (unsigned)kw * tap_stride);
        if (++i_kh == 3) { i_kh = 0; ++i_cb; }
        if (++i_sb == SB) i_sb = 0;
      };
      // SB - 1 row-steps ahead (the pixel slots, three of them, never run short)
      int issued = 0;
#pragma unroll
      for (int k = 0; k < SB - 1; ++k)
        if (issued < RS) { issue_rowstep(); ++issued; }
      for (int rs = 0; rs < RS; ++rs) {
        // this wave's DMAs of row-step rs have landed when only the younger row-steps' (SB - 2 of them) are outstanding
        const int younger = issued - rs - 1;
        if (younger <= 0) wait_vmcnt<0>();
        else if (SB == 3 && younger == 1) { if (la_hi) wait_vmcnt<LB + LA_HI>(); else wait_vmcnt<LB + LA_LO>(); }
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (issued < RS) { issue_rowstep(); ++issued; }   // into the stage row-step rs-1 used: its reads retired at this barrier
      }
      __syncthreads();
      if (!WALK) return;
      tl += gridDim.x;
      if (tl >= nblk) return;
      table ^= TABLE_OFF ^ (TABLE_OFF + 2048);
    }
  }

  // ---- MFMA waves
  // Every tile of the walk runs the code of a block of one tile, its fragment and epilogue addressing included.  That addressing is
  // the same for every tile, and computed once, ahead of the tile loop, it would stay in some forty registers through the K loop and
  // the epilogue where a one-tile block computes it next to its use.  So the lane index is opaque to the compiler at a tile's start.
  const int wm = wave % WM, orow = OR == 2 ? (wave / WM) & 1 : 0, wn = wave / (WM * OR);
  auto row_off = [](int pix, int chunk) { return pix * 128 + (((chunk + 2 * ((pix >> 1) & 3)) & 7) << 4); };
  for (int tl = blockIdx.x, table = TABLE_OFF;;) {
    const Tile c = tile_at(tl);
    int tlane = lane;
    if constexpr (WALK) asm volatile("" : "+v"(tlane));
    const int r16 = tlane & 15, q16 = tlane >> 4;
    unsigned a_rd[3][2];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int pix = wm * 64 + kw * dil + r16;
      a_rd[kw][0] = (unsigned)row_off(pix, q16);
      a_rd[kw][1] = (unsigned)row_off(pix, 4 + q16);
    }
    const unsigned b_rd0 = (unsigned)(A_REGION + lds_off(wn * NT * 32 + r16, q16));
    const unsigned b_rd1 = (unsigned)(A_REGION + lds_off(wn * NT * 32 + r16, 4 + q16));
    // the running sum, the chain of P.X0 and Q.X0 that joins it every eighth K-step, and the sum of the unscaled low-piece products
    // P.X1, which runs over the tile's whole K loop and joins once, scaled, behind it: all three start every tile from zero
    f32x4 acc16[NT16][MT16], accI2[NT16][MT16], low[NT16][MT16];
#pragma unroll
    for (int j = 0; j < NT16; ++j)
#pragma unroll
      for (int i = 0; i < MT16; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc16[j][i][e] = 0.f; accI2[j][i][e] = 0.f; low[j][i][e] = 0.f; }
    unsigned a_off = (unsigned)(orow * A_SLOT), b_off = 0;   // byte offsets of the row-step's pixel slot (kh [+ 1]) and weight stage
    int t = 0;
    for (int rs = 0; rs < RS; ++rs) {
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int kw = 0; kw < 3; ++kw, ++t) {
        x2_flush(t, acc16, accI2);
        uint4 xp0[MT16], xp1[MT16], xw0[NT16], xw1[NT16];
#pragma unroll
        for (int i = 0; i < MT16; ++i) {
          xp0[i] = *reinterpret_cast<const uint4*>(smem + (a_rd[kw][0] + a_off) + i * 2048);
          xp1[i] = *reinterpret_cast<const uint4*>(smem + (a_rd[kw][1] + a_off) + i * 2048);
        }
#pragma unroll
        for (int j = 0; j < NT16; ++j) {
          xw0[j] = *reinterpret_cast<const uint4*>(smem + (b_rd0 + b_off) + (kw * B_TAP + j * 2048));
          xw1[j] = *reinterpret_cast<const uint4*>(smem + (b_rd1 + b_off) + (kw * B_TAP + j * 2048));
        }
        x2_products_low(xp0, xp1, xw0, xw1, accI2, low);
      }
      a_off = a_off == (unsigned)((2 + orow) * A_SLOT) ? (unsigned)(orow * A_SLOT) : a_off + (unsigned)A_SLOT;
      b_off = b_off == (unsigned)(SB - 1) * B_STEP ? 0u : b_off + (unsigned)B_STEP;
    }
    x2_join<false>(acc16, accI2);
    x2_join_low(acc16, low);
    __syncthreads();
    const int oyw = c.oy + orow * dil;                   // this wave's output row
    if (oyw < p.Ho)                                      // (the second row of a last, odd pair lies below the image: nothing to store)
      rows_epilogue<CW, MT, NT>(p, smem + SCRATCH_OFF, smem + table, acc16, wave, tlane, wm, wn, ((c.img * p.Ho + oyw) * segs + c.seg) * 128, c.n0);
    if (!WALK) return;
    tl += gridDim.x;
    if (tl >= nblk) return;
    table ^= TABLE_OFF ^ (TABLE_OFF + 2048);
  }
}

template <int WN, int NT, int SB, int OR = 1>
hipError_t launch_rowstep_cfg(const ConvArgs& a, hipStream_t s) {
  constexpr int BN = WN * NT * 32;
  constexpr int smem = rowstep_lds_bytes(BN, SB, OR);
  static std::atomic<unsigned long long> attr_done{0};
  static int cus[64];                                  // compute units per device: a walking launch has a block for each
  auto kern = &conv3x3_rowstep_kernel<WN, NT, SB, OR>;
  int dev = 0;
  if (hipError_t e = raise_lds_limit_once(attr_done, reinterpret_cast<const void*>(kern), smem, &dev, cus); e != hipSuccess) return e;
  if (a.Co % BN != 0 || a.Wo % 128 != 0) return hipErrorInvalidValue;
  const int pairs = OR == 2 ? rowstep_pairs(a.Ho, a.dil) : a.Ho;
  const int tiles = a.N * pairs * (a.Wo / 128) * (a.Co / BN);
  const int blocks = rowstep_walks(SB) && tiles > cus[dev] ? cus[dev] : tiles;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3((2 * WN * OR + 4) * 64), smem, s, a);
  return hipGetLastError();
}

// The row-step tile `tile` of the menu (conv_tiles.hpp) for a convolution of its kind: <WN, NT, SB, OR> from the row
template <int I = 0>
hipError_t launch_rows_tile(const ConvArgs& a, int tile, int kind, hipStream_t s) {
  if constexpr (I == CONV_TILE_COUNT) return hipErrorInvalidValue;
  else {
    constexpr ConvTile t = kConvTiles[I];
    if constexpr (t.kind != 0) {
      if (tile == I && kind == t.kind) return launch_rowstep_cfg<t.wn, t.nt, t.s[2], t.wm / 2>(a, s);
    }
    return launch_rows_tile<I + 1>(a, tile, kind, s);
  }
}

}  // namespace

hipError_t launch_conv3x3_rows(const ConvArgs& a, int tile, hipStream_t s) {
  if (a.x_bytes == 0 || a.x_bytes >= kOutOfRange || a.w_bytes == 0 || a.w_bytes >= kOutOfRange) return hipErrorInvalidValue;
  if (a.stem || a.KH != 3 || a.KW != 3 || a.ksteps != 9 * (a.Ci * 4 / 128) ||
      a.M != a.N * a.Ho * a.Wo)
    return hipErrorInvalidValue;
  return launch_rows_tile(a, tile, conv_rows_kind(2, a.KH, a.stride, a.pad, a.dil, a.Hi, a.Wi, a.Ho, a.Wo, a.Ci, a.Co, a.res != nullptr), s);
}

}  // namespace nbc
