// The per-pixel vote of the Dropout draws (include/nbc.h, nbc_dropout_votes / nbc_vote_summary).  One
// definition for the kernels (dropout_votes.hip) and the host entry point nbc_vote_decode, as philox.hpp is for the generator.
//
// A vote word is one uint32 per pixel: bits 0..15 hold n1, the draws whose final label is 1, bits 16..31 hold n2, the draws
// whose final label is 2; n0 = D - n1 - n2.  A label outside {0,1,2} votes nowhere (it lands in n0), as nbc_confusion counts
// such a label nowhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nbc {

constexpr int kVoteMaxDraws = 65535;   // what a 16-bit field holds

// what one draw's label adds to the pixel's word
__host__ __device__ __forceinline__ uint32_t vote_of_label(uint32_t label) {
  return label == 1u ? 1u : (label == 2u ? 0x10000u : 0u);
}

struct Vote {
  uint32_t n1, n2, n_win;   // n_win: the winner's votes (0 for an invalid word)
  uint32_t label, support;  // the winning class and floor(255 n_win / D)
  bool valid, unanimous;
};

// The decision on one word under D draws, 1 <= D <= 65535.  The class with the most votes wins and a tie goes to the lowest
// class index (torch.argmax: the first maximum).  The support byte is floor(255 n_win / D) in integers: 255 exactly when
// n_win = D, and never below 85 since the winner holds at least a third of the draws (255 ceil(D / 3) / D >= 85).  A word
// with n1 + n2 > D cannot come from D draws: it is invalid, label 0 and support 0.
__host__ __device__ __forceinline__ Vote vote_decide(uint32_t word, uint32_t draws) {
  Vote v;
  v.n1 = word & 0xffffu;
  v.n2 = word >> 16;
  v.valid = v.n1 + v.n2 <= draws;
  if (!v.valid) {
    v.n_win = v.label = v.support = 0u;
    v.unanimous = false;
    return v;
  }
  v.label = 0u;
  v.n_win = draws - v.n1 - v.n2;
  if (v.n1 > v.n_win) { v.label = 1u; v.n_win = v.n1; }
  if (v.n2 > v.n_win) { v.label = 2u; v.n_win = v.n2; }
  v.support = 255u * v.n_win / draws;      // 255 * 65535 < 2^24
  v.unanimous = v.n_win == draws;
  return v;
}

}  // namespace nbc
