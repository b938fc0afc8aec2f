// Builds the launch plan of a forward (nbc_plan.hpp): two trunks, ResNet-50 and EfficientNet, on one set of parts (buffer
// pool, ingest, convolution, FCN / DeepLab head).  Host code only.
#include "nbc_plan.hpp"

#include <algorithm>

#include "nbc_kernels.hpp"
#include "nbc_net.hpp"

namespace nbc {
namespace {

struct Tensor { int buf, H, W, C; };   // an activation: its buffer, its size and the channels it is stored with

struct Builder {
  Plan P;
  const int N, H, W, eb;
  const std::vector<ConvUnit>& units;
  std::vector<size_t> affine_off;      // per unit: floats of the affine array before its (gamma, beta)
  std::vector<bool> in_use;
  std::string refused;                 // the first op that cannot run on this image

  explicit Builder(const PlanKey& key)
      : N(key.N), H(key.H), W(key.W), eb(elem_bytes(key.precision)), units(conv_units(key.arch)), affine_off(units.size(), 0) {
    static_cast<PlanKey&>(P) = key;
    for (size_t u = 0, off = 0; u < units.size(); ++u)
      if (!units[u].bn.empty()) { affine_off[u] = off; off += 2 * (size_t)units[u].cout; }
  }

  // Activation buffers are recycled through a small pool unless `keep` asks for one buffer per op.  The order of the calls
  // decides which buffer an op gets and how large each one grows.
  int acquire(size_t bytes) {
    if (!P.keep)
      for (size_t i = 0; i < in_use.size(); ++i)
        if (!in_use[i]) { in_use[i] = true; P.buf_bytes[i] = std::max(P.buf_bytes[i], bytes); return (int)i; }
    in_use.push_back(true);
    P.buf_bytes.push_back(bytes);
    return (int)in_use.size() - 1;
  }
  void release(int b) { if (b >= 0 && !P.keep) in_use[b] = false; }
  // The one buffer outside the pool, which the pairs of a plan share: the identity between downsample.0 and the conv3 of its
  // pair when the two run as two launches (resnet50_trunk).  Never released, so no other op is given it.
  int identity(size_t bytes) {
    if (P.identity_buf < 0) { in_use.push_back(true); P.buf_bytes.push_back(0); P.identity_buf = (int)in_use.size() - 1; }
    P.buf_bytes[P.identity_buf] = std::max(P.buf_bytes[P.identity_buf], bytes);
    return P.identity_buf;
  }

  // image -> NHWC with one 16-byte pixel
  Tensor ingest(int creal) {
    const Tensor x{acquire((size_t)N * H * W * kChunkBytes), H, W, kChunkBytes / eb};
    Op o;
    o.kind = OP_INGEST; o.out_buf = x.buf;
    o.Hi = H; o.Wi = W; o.Ci = 3; o.Ho = H; o.Wo = W; o.Co = x.C; o.creal = creal; o.name = "ingest";
    P.ops.push_back(o);
    return x;
  }

  // Output size of unit u on `in`; a map without a pixel is refused (the ops are still planned, on one pixel's room).  No
  // ResNet-50 unit comes here with less than one: 3x3s pad by their dilation and the stem sees H, W >= 8.
  void out_size(const ConvUnit& u, const Tensor& in, int* Ho, int* Wo) {
    const int keff = u.dil * (u.k - 1) + 1;                          // the dilated extent (ASPP)
    *Ho = same_out(in.H, keff, u.stride, u.pad, u.pad_end());
    *Wo = same_out(in.W, keff, u.stride, u.pad, u.pad_end());
    if ((*Ho < 1 || *Wo < 1) && refused.empty())
      refused = "nbc_forward: a " + std::to_string(H) + "x" + std::to_string(W) + " image is too small for " + arch_name(P.arch) +
                " (" + u.name + " has no output pixel)";
  }

  // A conv_dma launch of unit ui; gate_buf >= 0: per image on the gated weights.  In NBC_BN_PER_IMAGE a unit with a BatchNorm
  // is the raw conv, then <bn>.stats and <bn>.apply (with the identity).  to_identity: the output goes to the identity buffer.
  Tensor add_conv(int ui, const Tensor& in, int res_buf = -1, int gate_buf = -1, bool to_identity = false) {
    const ConvUnit& u = units[ui];
    int Ho, Wo;
    out_size(u, in, &Ho, &Wo);
    const bool bn_ops = P.bn == NBC_BN_PER_IMAGE && !u.bn.empty();
    const int idt = res_buf;
    if (bn_ops) res_buf = -1;
    Op o;
    o.kind = OP_CONV; o.unit = ui; o.in_buf = in.buf; o.res_buf = res_buf; o.gate_buf = gate_buf; o.raw = bn_ops;
    o.affine_off = affine_off[ui];                                   // a raw f16x2 launch reads its scales from the raw array
    o.Hi = in.H; o.Wi = in.W; o.Ci = in.C; o.Ho = Ho; o.Wo = Wo; o.Co = u.outc(); o.name = u.name;
    o.creal = u.cout_pad ? u.cout : 0;                               // EfficientNet pads its channels, ResNet-50 does not
    const size_t out_bytes = (size_t)N * std::max(Ho, 1) * std::max(Wo, 1) * u.outc() * eb;
    o.out_buf = to_identity ? identity(out_bytes) : acquire(out_bytes);
    o.rows = conv_rows_kind(P.precision, u.k, u.stride, u.pad, u.dil, in.H, in.W, Ho, Wo, in.C, u.outc(), res_buf >= 0);
    // the tile's K and the bytes count the unit's channels (ResNet-50's stem: the 3 real ones of the 16-byte pixel)
    const int images = gate_buf >= 0 ? 1 : N;                        // per launch
    o.tile = choose_conv_tile(images * std::max(Ho * Wo, 1), u.outc(), u.inc() * u.k * u.k, P.precision, o.rows);
    o.launches = gate_buf >= 0 ? N : 1;
    const double M = (double)N * Ho * Wo;
    o.flops = 2.0 * M * u.cout * u.cin * u.k * u.k;
    o.bytes = ((double)N * in.H * in.W * u.inc() + (double)u.outc() * u.inc() * u.k * u.k * o.launches + M * u.outc() +
               (res_buf >= 0 ? M * u.outc() : 0.0)) * eb;
    P.ops.push_back(o);
    if (bn_ops) {
      // F.batch_norm(training=True) of a batch of one refuses a map of one pixel; so does this mode, for every image
      if (Ho * Wo == 1 && refused.empty())
        refused = "Expected more than 1 value per channel when training, got input size [1, " + std::to_string(u.cout) +
                  ", 1, 1] (" + u.bn + " of a " + std::to_string(H) + "x" + std::to_string(W) + " image; per-image BatchNorm)";
      const int hw = Ho * Wo;
      Op st = o;
      st.kind = OP_BN_STATS; st.in_buf = o.out_buf; st.res_buf = -1; st.raw = false; st.name = u.bn + ".stats";
      st.affine_off = affine_off[ui];
      st.launches = 2;                                                 // partial sums, then their sum and the table
      st.flops = 3.0 * M * u.cout;
      st.bytes = M * u.cout * 4.0 + (double)N * bn_stats_slices(hw) * u.cout * 16.0;
      P.ops.push_back(st);
      Op ap = o;
      ap.kind = OP_BN_APPLY; ap.in_buf = o.out_buf; ap.res_buf = idt; ap.raw = false; ap.name = u.bn + ".apply";
      ap.relu = u.relu ? 1 : 0;
      ap.flops = 2.0 * M * u.cout;
      ap.bytes = (2.0 + (idt >= 0 ? 1.0 : 0.0)) * M * u.cout * 4.0;
      P.ops.push_back(ap);
      P.bn_ws_bytes = std::max(P.bn_ws_bytes, bn_stats_workspace_bytes(N, hw, u.cout));
    }
    return {o.out_buf, Ho, Wo, u.outc()};
  }

  // torchvision's resnet50 cut at layer4: stem, max-pool, bottlenecks.  Returns layer4's output and the head's first unit.
  Tensor resnet50_trunk(int* head_unit) {
    Tensor cur = ingest(0);
    {
      const Tensor stem = add_conv(0, cur);
      release(cur.buf);
      cur = stem;
      const int pH = (cur.H - 1) / 2 + 1, pW = (cur.W - 1) / 2 + 1;
      Op o;
      o.kind = OP_MAXPOOL; o.in_buf = cur.buf;
      o.Hi = cur.H; o.Wi = cur.W; o.Ci = cur.C; o.Ho = pH; o.Wo = pW; o.Co = cur.C; o.name = "backbone.maxpool";
      o.out_buf = acquire((size_t)N * pH * pW * cur.C * eb);
      o.bytes = ((double)N * cur.H * cur.W * cur.C + (double)N * pH * pW * cur.C) * eb;
      P.ops.push_back(o);
      release(cur.buf);
      cur = {o.out_buf, pH, pW, cur.C};
    }
    int ui = 1;
    while (ui < (int)units.size() && units[ui].block_first) {
      const Tensor t1 = add_conv(ui, cur);
      const Tensor t2 = add_conv(ui + 1, t1);
      release(t1.buf);
      int idt = cur.buf, c3 = ui + 2;
      bool pair = false;
      if (!units[ui + 2].residual) {      // downsample present
        c3 = ui + 3;
        // A (downsample.0, conv3) pair, which a forward may run as one launch (the dual-branch form of the f16x2 kernel,
        // conv_igemm_dma.hip): BatchNorm folded, nothing else reading the identity (keep-activations off), conv3 short enough
        // to leave its second accumulator set free (<= 8 K-steps).  Its buffers serve both forms: the block's input, which
        // the one launch reads, stays acquired until conv3 has its output buffer, and the identity, which only the two
        // launches write and read, lies outside the pool.
        const ConvUnit& u3 = units[c3];
        pair = P.precision == NBC_PREC_F16X2 && P.bn == NBC_BN_RUNNING && !P.keep && u3.inc() * u3.k * u3.k * eb / kKStepBytes <= 8;
        idt = add_conv(ui + 2, cur, -1, -1, pair).buf;
        if (!pair) release(cur.buf);
      }
      const Tensor out = add_conv(c3, t2, idt);
      if (pair) P.ops.back().ds_op = (int)P.ops.size() - 2;
      release(t2.buf);
      release(pair ? cur.buf : idt);
      cur = out;
      ui = c3 + 1;
    }
    *head_unit = ui;
    return cur;
  }

  // EfficientNet (fp32): ingest, the stem on conv_dma (its swish deferred), per MBConv block [expand conv (swish deferred)],
  // depthwise conv (+ BN, swish, SE squeeze partials), SE excite (gate), gated project weights, project conv per image
  // (+ identity), then the head conv with a swish pass.  Channels padded (ConvUnit::outc); the SE partials, the gate and the
  // gated weights are f32 whatever the activations' element is.  Returns the trunk's output and the
  // head's first unit.
  Tensor effnet_trunk(int* head_unit) {
    Tensor cur = ingest(3);
    {
      const Tensor stem = add_conv(0, cur);                             // _conv_stem: BN, swish deferred
      release(cur.buf);
      cur = stem;
    }
    int ui = 1;
    while (ui < (int)units.size() && units[ui].block >= 0) {
      const Tensor in = cur;
      Tensor e = in;
      if (units[ui].kind == kUnitConv) e = add_conv(ui++, in);          // _expand_conv
      const ConvUnit& dw = units[ui];
      const int C = dw.outc();
      int Ho, Wo;
      out_size(dw, e, &Ho, &Wo);
      const int tiles = dwconv_tiles(dw.stride, std::max(Ho, 1), std::max(Wo, 1));
      const int ws = acquire((size_t)N * tiles * C * sizeof(float));
      Op d;
      d.kind = OP_DWCONV; d.unit = ui; d.in_buf = e.buf; d.ws_buf = ws; d.tiles = tiles;
      d.Hi = e.H; d.Wi = e.W; d.Ci = C; d.Ho = Ho; d.Wo = Wo; d.Co = C; d.creal = dw.cout; d.name = dw.name;
      d.out_buf = acquire((size_t)N * std::max(Ho, 1) * std::max(Wo, 1) * C * eb);
      d.flops = 2.0 * N * Ho * Wo * dw.cout * dw.k * dw.k;
      d.bytes = ((double)N * e.H * e.W * C + (double)N * Ho * Wo * C) * eb;
      P.ops.push_back(d);
      if (e.buf != in.buf) release(e.buf);
      const ConvUnit& red = units[ui + 1];
      const ConvUnit& exc = units[ui + 2];
      const ConvUnit& prj = units[ui + 3];
      const int gate = acquire((size_t)N * C * sizeof(float));
      Op se;
      se.kind = OP_SE_EXCITE; se.unit = ui + 1; se.aux_unit = ui + 2; se.in_buf = ws; se.tiles = tiles;
      se.out_buf = gate; se.gate_buf = gate;
      se.Hi = Ho; se.Wi = Wo; se.Ci = C; se.Ho = 1; se.Wo = 1; se.Co = C; se.creal = exc.cout; se.name = exc.name;
      se.flops = 4.0 * N * C * red.cout;
      se.bytes = ((double)N * tiles * C + 2.0 * C * red.cout + (double)N * C) * sizeof(float);
      P.ops.push_back(se);
      release(ws);
      const int wg = acquire((size_t)N * prj.outc() * prj.inc() * sizeof(float));
      Op gw;
      gw.kind = OP_GATE_WEIGHTS; gw.unit = ui + 3; gw.ws_buf = wg;
      gw.gate_buf = gate; gw.Ci = prj.inc(); gw.Co = prj.outc(); gw.name = prj.name + ".gated_weights";
      gw.flops = (double)N * prj.outc() * prj.inc();
      gw.bytes = ((double)prj.outc() * prj.inc() * (1 + N) + (double)N * C) * sizeof(float);
      P.ops.push_back(gw);
      release(gate);
      const Tensor out = add_conv(ui + 3, {d.out_buf, Ho, Wo, C}, prj.residual ? in.buf : -1, wg);
      release(d.out_buf);
      release(wg);
      release(in.buf);
      cur = out;
      ui += 4;
    }
    const Tensor h = add_conv(ui, cur);                                 // _conv_head, then its swish in place
    release(cur.buf);
    Op sw;
    sw.kind = OP_SWISH; sw.unit = ui; sw.in_buf = h.buf; sw.out_buf = h.buf;
    sw.Hi = h.H; sw.Wi = h.W; sw.Ci = h.C; sw.Ho = h.H; sw.Wo = h.W; sw.Co = h.C; sw.creal = units[ui].cout;
    sw.name = units[ui].name + ".swish";
    sw.flops = (double)N * h.H * h.W * units[ui].cout * 4;
    sw.bytes = 2.0 * N * h.H * h.W * h.C * eb;
    P.ops.push_back(sw);
    *head_unit = ui + 1;
    return h;
  }

  // FCNHead or DeepLabHead on the trunk's output, classifier.4, then the upsample with its argmax.
  void head(Tensor cur, int ui) {
    Tensor t;
    int cls = ui + 1;                                                        // classifier.4's unit
    if (is_deeplab_head(P.arch)) {
      // ASPP: four convolutions and the pooling branch all read the trunk's output (`cur`), which stays acquired until the
      // last of them; the concat then copies the five into one [M][1280] tensor.  Then project, classifier.1.
      Tensor br[4];
      for (int b = 0; b < 4; ++b) br[b] = add_conv(ui + b, cur);
      const ConvUnit& pu = units[ui + 4];
      const int hw = cur.H * cur.W, B = pu.cout;
      const int ws = acquire(((size_t)N * aspp_pool_slices(hw) + N) * pu.cin * sizeof(float));   // the slices' sums, then the means
      Op po;
      po.kind = OP_ASPP_POOL; po.unit = ui + 4; po.in_buf = cur.buf; po.ws_buf = ws;
      po.Hi = cur.H; po.Wi = cur.W; po.Ci = pu.cin; po.Ho = 1; po.Wo = 1; po.Co = B;
      po.name = "classifier.0.convs.4";                                      // the pooled vector: one pixel per image
      po.out_buf = acquire((size_t)N * B * eb);
      po.launches = 3;                                                       // partial sums, their sum, the 1x1 conv
      po.flops = 2.0 * N * B * pu.cin + (double)N * hw * pu.cin;
      po.bytes = (double)N * hw * pu.cin * eb + (double)B * pu.cin * 4 + (double)N * B * eb;
      P.ops.push_back(po);
      release(ws);
      release(cur.buf);
      Op co;
      co.kind = OP_CONCAT;
      for (int b = 0; b < 4; ++b) co.cat_in[b] = br[b].buf;
      co.cat_in[4] = po.out_buf;
      co.Hi = br[3].H; co.Wi = br[3].W; co.Ci = 5 * B; co.Ho = br[3].H; co.Wo = br[3].W; co.Co = 5 * B;
      co.name = "classifier.0.concat";
      co.out_buf = acquire((size_t)N * hw * 5 * B * eb);
      co.bytes = 2.0 * N * hw * 5 * B * eb;
      P.ops.push_back(co);
      for (int b = 0; b < 5; ++b) release(co.cat_in[b]);
      const Tensor pj = add_conv(ui + 5, {co.out_buf, co.Ho, co.Wo, co.Co});   // classifier.0.project
      release(co.out_buf);
      t = add_conv(ui + 6, pj);                                              // classifier.1
      release(pj.buf);
      cls = ui + 7;
    } else {
      t = add_conv(ui, cur);                                                 // classifier.0
      release(cur.buf);
    }
    const ConvUnit& cu = units[cls];
    Op o;
    o.kind = OP_HEAD1X1; o.unit = cls; o.in_buf = t.buf;
    o.Hi = t.H; o.Wi = t.W; o.Ci = cu.inc(); o.Ho = t.H; o.Wo = t.W; o.Co = kNumClasses; o.name = cu.name;
    o.flops = 2.0 * N * t.H * t.W * cu.cin * kNumClasses;
    o.bytes = (double)N * t.H * t.W * o.Ci * eb + (double)N * t.H * t.W * kNumClasses * 4;
    P.ops.push_back(o);
    release(t.buf);
    P.h = t.H; P.w = t.W;
    Op up;
    up.kind = OP_UPSAMPLE;
    up.Hi = t.H; up.Wi = t.W; up.Ci = kNumClasses; up.Ho = H; up.Wo = W; up.Co = kNumClasses; up.name = "upsample_argmax";
    up.bytes = (double)N * t.H * t.W * kNumClasses * 4 + (double)N * H * W;
    P.ops.push_back(up);
  }
};

}  // namespace

std::string build_plan(const PlanKey& key, Plan* out) {
  Builder b(key);
  int head_unit = 0;
  const Tensor x = is_effnet(key.arch) ? b.effnet_trunk(&head_unit) : b.resnet50_trunk(&head_unit);
  b.head(x, head_unit);
  if (b.refused.empty()) *out = b.P;
  return b.refused;
}

}  // namespace nbc
