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
constexpr int kNumArchs = 2;       // the ResNet-50 pair; the EfficientNet ids follow (2 stays unused)
// EfficientNet trunks (efficientnet_pytorch 0.7 extract_features) under FCNHead / DeepLabHead(inplanes, 3): n = 0..7.
constexpr int kArchFcnEffB0 = 16;       // fcn_efficientnet(n): 16 + n
constexpr int kArchDeepLabEffB0 = 24;   // deeplabv3_efficientnet(n): 24 + n
inline bool is_effnet(int arch) { return arch >= kArchFcnEffB0 && arch < kArchDeepLabEffB0 + 8; }
inline int effnet_variant(int arch) { return arch & 7; }
inline bool is_deeplab_head(int arch) { return arch == kArchDeepLab || (arch >= kArchDeepLabEffB0 && arch < kArchDeepLabEffB0 + 8); }
inline bool known_arch(int arch) { return (arch >= 0 && arch < kNumArchs) || is_effnet(arch); }
constexpr int kArchSlots = kNumArchs + 16;   // table slots: the two ResNet-50 networks, then 16 + n, 24 + n
inline int arch_slot(int arch) { return is_effnet(arch) ? kNumArchs + (arch - kArchFcnEffB0) : (arch == kArchDeepLab ? 1 : 0); }
constexpr float kBnEpsEffNet = 1e-3f;   // every BatchNorm of the EfficientNet trunk (the heads keep torch's 1e-5)
constexpr int kEffChannelPad = 64;      // EfficientNet tensors: channels zero-padded to a multiple of this
constexpr int kAsppBranchCh = 256;  // channels of every ASPP branch; the concat holds five of them

enum { kUnitConv = 0, kUnitDepthwise = 1, kUnitSeReduce = 2, kUnitSeExpand = 3 };

struct ConvUnit {
  std::string name;      // "backbone.layer1.0.conv1"
  std::string bn;        // "" when there is no BatchNorm (classifier.4)
  int cin, cout, k, stride, pad, dil;
  bool relu, bias, residual;
  int block_first;       // 1 when this is conv1 of a bottleneck (plan building)
  bool pooled = false;   // the ASPP pooling branch: global average pool, then this 1x1 conv in f32 (aspp.hip)
  // EfficientNet (all defaults for the ResNet-50 networks)
  int kind = kUnitConv;  // kUnit*
  int pad_after = -1;    // bottom / right pad (TF "same": may differ from `pad`, the top / left one); -1 = pad
  bool swish = false;    // BatchNorm, then swish (stem and expand: deferred into the depthwise kernel's staging)
  float eps = kBnEps;
  int cin_pad = 0, cout_pad = 0;   // channels of the stored tensors (0 = cin / cout)
  int block = -1;        // MBConv block index
  bool in_swish = false; // depthwise: its input is a stored pre-swish tensor (stem or expand output)
  int inc() const { return cin_pad ? cin_pad : cin; }
  int outc() const { return cout_pad ? cout_pad : cout; }
  int pad_end() const { return pad_after < 0 ? pad : pad_after; }
};

struct StateKey {
  std::string name;
  int64_t shape[4];
  int ndim;
  int dtype;             // 0 f32, 1 i64
};

const std::vector<ConvUnit>& conv_units(int arch = kArchFcn);
const std::vector<StateKey>& state_keys(int arch = kArchFcn);

// The trunk's extra keys that no unit reads (EfficientNet: the ImageNet classifier _fc.weight / _fc.bias).
const std::vector<StateKey>& unused_keys(int arch);
// Channels of the EfficientNet trunk's output (models.py efficientnet_inplanes), 0 for another architecture.
int effnet_inplanes(int arch);
const char* arch_name(int arch);

// Output size of a convolution with pads (before, after) on an x-pixel input, floor((x + before + after - k) / s) + 1; 0 when the
// padded input is smaller than the kernel
inline int same_out(int x, int k, int s, int before, int after) {
  const int t = x + before + after - k;
  return t < 0 ? 0 : t / s + 1;
}

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
  int kind;              // kUnit*: depthwise [k*k][cout_pad] f32 + (scale, shift); SE reduce [cout][cin_pad] f32 + bias at
                         // shift_off; SE expand [cout_pad][cin] f32 + bias at shift_off
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
