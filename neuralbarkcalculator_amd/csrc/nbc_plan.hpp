// The launch plan of a forward: the ops of one (network, precision, batch, image size) in launch order and the sizes of the
// activation buffers they share.  Building one makes no device call (nbc_plan.cpp); the context (nbc_ctx.hpp) caches them and nbc_api.hip runs them.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/nbc.h"

namespace nbc {

enum OpKind { OP_INGEST, OP_CONV, OP_MAXPOOL, OP_HEAD1X1, OP_UPSAMPLE, OP_ASPP_POOL, OP_CONCAT, OP_BN_STATS, OP_BN_APPLY,
              OP_DWCONV, OP_SE_EXCITE, OP_GATE_WEIGHTS, OP_SWISH };

// Buffer 0 is a real buffer: an op names the buffers and units it uses, everything else stays -1.
struct Op {
  OpKind kind = OP_INGEST;
  int unit = -1;       // conv unit index (OP_CONV / OP_HEAD1X1 / OP_ASPP_POOL), -1 otherwise
  int in_buf = -1, out_buf = -1, res_buf = -1;
  int Hi = 0, Wi = 0, Ci = 0, Ho = 0, Wo = 0, Co = 0;
  std::string name;
  double flops = 0, bytes = 0;
  int tile = 0;        // OP_CONV: tile id of the LDS-DMA kernel (default choice or autotuned)
  int rows = 0;        // OP_CONV: conv_rows_kind: 0 generic tiles, 1 / 2 the row-resident 3x3 kernel (kind 1: tiles 18 or 20; kind 2: tile 19)
  int ws_buf = -1;     // OP_ASPP_POOL: workspace buffer (slice partials, then the per-image means)
  int cat_in[5] = {-1, -1, -1, -1, -1};   // OP_CONCAT: the four spatial branches' buffers and the pooled vectors' buffer
  bool raw = false;    // OP_CONV in NBC_BN_PER_IMAGE: unit scale, zero shift, no ReLU, no identity (the raw conv output)
  int relu = 0;        // OP_BN_APPLY: the unit's ReLU
  size_t affine_off = 0;   // OP_BN_STATS, raw OP_CONV: floats before the unit's pair in the affine array and in the raw array
  // EfficientNet
  int gate_buf = -1;   // OP_CONV: per-image weights [N][Co][Ci] (the SE-gated project conv: one launch per image);
                       // OP_SE_EXCITE / OP_GATE_WEIGHTS: the gate [N][C]
  int creal = 0;       // channels of the tensor the network defines (0 = Co): nbc_read_activation drops the pad channels
  int launches = 1;    // launches of the op per forward (profiling records)
  int tiles = 0;       // OP_DWCONV / OP_SE_EXCITE: SE squeeze partials per image
  int aux_unit = -1;   // OP_SE_EXCITE: the _se_expand unit (unit = _se_reduce); OP_GATE_WEIGHTS: the project unit
  int ds_op = -1;      // OP_CONV, conv3 of a (downsample.0, conv3) pair: index of the downsample op, which is the op before it
};

// Everything a plan depends on.
struct PlanKey {
  int N = 0, H = 0, W = 0, precision = -1, arch = 0;
  bool keep = false;                   // one buffer per op (layer-by-layer parity tests) instead of a recycled pool
  int bn = NBC_BN_RUNNING;             // NBC_BN_*
};

inline bool same_shape(const PlanKey& a, const PlanKey& b) {
  return a.N == b.N && a.H == b.H && a.W == b.W && a.precision == b.precision && a.keep == b.keep && a.arch == b.arch && a.bn == b.bn;
}

struct Plan : PlanKey {
  size_t bn_ws_bytes = 0;              // NBC_BN_PER_IMAGE: slice partials + [N][C] scale and shift of the largest BatchNorm
  int h = 0, w = 0;                    // low-res logits size
  std::vector<Op> ops;
  std::vector<size_t> buf_bytes;       // per activation buffer
  int identity_buf = -1;               // the buffer outside the pool that the downsample of every pair writes (-1: no pair)
};

// The launch list of `key` into *out, or the reason why this network cannot run on such an image (*out is then left alone).
// The key must name a known architecture in a precision it runs in, N >= 1 and H, W >= 8, and NBC_BN_PER_IMAGE only for
// NBC_ARCH_FCN_RESNET50 in NBC_PREC_FP32 or NBC_PREC_F16X2 (nbc_set_bn_statistics and nbc_reserve refuse the rest before they come here).
std::string build_plan(const PlanKey& key, Plan* out);

}  // namespace nbc
