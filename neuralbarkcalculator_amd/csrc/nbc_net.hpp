// Network description and packed-weight layout shared by the packer (host only) and the
// launcher.  The layer list restates /root/reference/src/bark_calculator/models.py:127-139
// (torchvision resnet50 with replace_stride_with_dilation=[False,True,True], cut at layer4)
// and models.py:113-124 (FCNHead), or for architecture 1 models.py:46-57 (DeepLabHead: ASPP +
// a 3x3 conv); see neuralbarkcalculator_amd/topology.py for the same tables in Python.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace nbc {

constexpr int kNumClasses = 3;
constexpr float kBnEps = 1e-5f;
constexpr int kKStepBytes = 128;   // one K-step of the implicit GEMM = 128 bytes of K per row
constexpr int kChunkBytes = 16;    // one lane-load

// Architectures (NBC_ARCH_* of nbc.h): the trunk is shared, the head differs.
constexpr int kArchFcn = 0;        // fcn_resnet50: FCNHead(2048, 3)
constexpr int kArchDeepLab = 1;    // deeplabv3_resnet50: DeepLabHead(2048, 3) = ASPP(2048, [12, 24, 36]) + 3x3 conv
constexpr int kNumArchs = 2;
inline bool known_arch(int arch) { return arch >= 0 && arch < kNumArchs; }
constexpr int kAsppBranchCh = 256;  // channels of every ASPP branch; the concat holds five of them

struct ConvUnit {
  std::string name;      // "backbone.layer1.0.conv1"
  std::string bn;        // "" when there is no BatchNorm (classifier.4)
  int cin, cout, k, stride, pad, dil;
  bool relu, bias, residual;
  int block_first;       // 1 when this is conv1 of a bottleneck (plan building)
  bool pooled = false;   // the ASPP pooling branch: global average pool, then this 1x1 conv in f32 (aspp.hip)
};

struct StateKey {
  std::string name;
  int64_t shape[4];
  int ndim;
  int dtype;             // 0 f32, 1 i64
};

const std::vector<ConvUnit>& conv_units(int arch = kArchFcn);
const std::vector<StateKey>& state_keys(int arch = kArchFcn);

// Floats of the per-image BatchNorm affine array (nbc_pack_bn_affine): gamma then beta of every conv unit with a BatchNorm,
// in conv-unit order; the unit's pair sits at the running sum of 2 * cout over the units before it.
size_t bn_affine_floats(int arch);

// bytes per activation / weight element: f32 4, bf16 2, f16x2 4 (two f16 pieces; a 128-byte group holds 32 channels:
// [h0 x 32][h1 x 32], so tensors, K-steps and LDS rows have the f32 mode's geometry)
inline int elem_bytes(int precision) { return precision == 1 ? 2 : 4; }
inline bool known_precision(int precision) { return precision >= 0 && precision <= 2; }

// Packed layout of one conv unit inside the blob.
struct PackedConv {
  size_t w_off;          // weights: [cout][ksteps*128 bytes]
  size_t scale_off;      // float[cout]
  size_t shift_off;      // float[cout]
  int cin_pad;           // channels per input pixel as the kernel sees them
  int ksteps;            // K-steps of 128 bytes
  bool stem;             // one 16-byte chunk per tap (cin_pad*elem = 16 bytes)
  bool head;             // classifier.4: weights kept f32 [3][cin], shift = bias
  bool pooled;           // ASPP pooling branch: weights kept f32 [cout][cin], f32 (scale, shift)
};

// Trailer of the blob: what a rank that receives the blob by broadcast must know besides the panels.
//   int32 meta[kMetaWords]: [0] kMetaMagic, [1] NBC_PACK_* flags, [2] number of conv units, [kMetaArch] the
//   architecture (0 for FCN: a word every FCN blob held as zero before it had this meaning),
//   [kMetaExpBase + u] the power of two the OUTPUT tensor of conv unit u is stored with (f16x2; 0 elsewhere): see
//   activation_exponents in nbc_net.cpp
constexpr int kMetaWords = 256;
constexpr int kMetaArch = 3;
constexpr int kMetaExpBase = 8;
constexpr int32_t kMetaMagic = 0x4e424335;   // "NBC5"

struct PackedLayout {
  std::vector<PackedConv> convs;
  size_t meta_off;       // int32[kMetaWords]
  size_t total_bytes;
};

// The trailer is the blob's last kMetaWords * 4 bytes (meta_off + kMetaWords * 4 == total_bytes).
PackedLayout packed_layout(int precision, int arch = kArchFcn);

}  // namespace nbc
