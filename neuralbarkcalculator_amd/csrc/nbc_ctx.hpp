// The context of libnbc_hip.so (nbc_api.hip creates, fills and runs it) as the passes that read it see it: small_zones.hip,
// zones.hip, zone_match.hip, contours.hip, dropout_head.hip and head_refit.hip hold their entry points beside their kernels.
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.hpp"
#include "nbc_net.hpp"
#include "nbc_plan.hpp"
#include "reduce.hpp"

#define NBC_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return ::nbc::set_error(NBC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace nbc {

// The memory policy of the context's owners (device_mem.hpp), and an event owned the same way.
struct HipMem {
  using Error = hipError_t;
  static constexpr Error ok() { return hipSuccess; }
  static Error allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }          // synchronises: nothing of the block is in flight afterwards
  static void forget_error() { (void)hipGetLastError(); }
  static Error copy_in(void* dst, const void* host, size_t bytes) { return hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice); }
};
using DeviceBuffer = Buffer<HipMem>;
template <class T> using DeviceArray = Array<T, HipMem>;

struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : ev(std::exchange(o.ev, nullptr)) {}
  ~Event() { if (ev) (void)hipEventDestroy(ev); }
  hipError_t create() { return hipEventCreate(&ev); }
  operator hipEvent_t() const { return ev; }
};

}  // namespace nbc

// Everything the context holds on the device is a member that releases itself: nbc_destroy deletes the context.
struct nbc_ctx {
  int device = 0;
  int precision = -1;
  int arch = nbc::kArchFcn;                 // NBC_ARCH_* of the attached blob
  nbc::DeviceArray<unsigned char> weights;  // device blob: the caller's (nbc_attach_weights) or one loaded / received here
  nbc::PackedLayout layout;
  float mean[3] = {0.7399f, 0.6139f, 0.4401f};   // models.py:208
  float stdv[3] = {0.1068f, 0.1272f, 0.1271f};   // models.py:209
  nbc::Plan plan;                           // plan of the current (N,H,W)
  std::vector<nbc::Plan> plan_cache;        // plans (with their tuned tiles) of the other shapes seen, oldest first
  std::vector<nbc::DeviceBuffer> bufs;      // the plan's activation buffers: they only ever grow
  nbc::DeviceBuffer lowres;
  int conv_tile = -1;                       // tile override, -1 = per-layer choice
  bool fuse_downsample = true;              // nbc_set_fuse_downsample
  int fused_pairs = 0;                      // (downsample.0, conv3) pairs the last forward ran as one launch
  float logit_offsets[2] = {0.f, 0.f};      // nbc_set_logit_offsets: added to the bark and node logits of the decision alone
  bool offsets_on = false;                  // either one is not zero: the upsample + argmax launch takes its offset kernels
  bool keep = false;
  bool profiling = false;
  // profiling: one event set (nops+1 events) per profiled forward, read back lazily so that the
  // timed loop never synchronises; nbc_num_op_records() averages over the sets and resets.
  std::vector<std::vector<nbc::Event>> prof_sets;
  size_t prof_used = 0;
  std::vector<nbc::Op> prof_ops;
  int prof_arch = nbc::kArchFcn;            // architecture of prof_ops
  std::vector<nbc_op_record> records;
  std::map<std::string, int> act_of;        // conv unit name -> op index (keep mode)
  nbc::DeviceBuffer scratch256;             // 256 bytes of device scratch (min/max of the preprocessor resize)
  int pack_flags = 0;                       // NBC_PACK_* of the attached blob (its trailer)
  std::vector<int> act_exp;                 // per conv unit: power of two its output tensor is stored with (trailer)
  nbc::DeviceBuffer nonfinite;              // one device word, sticky: bit 0 = a forward produced a NaN / infinite logit,
                                            // NBC_NONFINITE_BN_RANGE = a per-image BatchNorm saw a channel outside the pieces' range
  nbc::DeviceBuffer zones_ws;               // remove_small_zones workspace: parent ints, size ints, bg bytes
  int bn_mode = NBC_BN_RUNNING;             // NBC_BN_*
  nbc::DeviceArray<float> bn_affine;        // gamma, beta per BatchNorm unit (nbc_pack_bn_affine)
  nbc::DeviceArray<float> bn_raw;           // f16x2: 2^(r - k - a_in), 2^-r per BatchNorm unit (nbc_pack_bn_raw)
  nbc::DeviceArray<float> bn_unit;          // 2048 ones, then 2048 zeros (the raw convolutions' scale and shift)
  nbc::DeviceBuffer bn_ws;                  // per-image BatchNorm workspace (Plan::bn_ws_bytes)
  // the (N, H, W) of the last completed nbc_forward while its activations and plan stand untouched (nbc_dropout_draws reads
  // the stored input of classifier.4): cleared by whatever parks the plan, retunes it or attaches other weights
  bool fwd_valid = false;
  int fwd_N = 0, fwd_H = 0, fwd_W = 0;
  nbc::DeviceBuffer refit_theta;            // nbc_head_logits: the caller's theta as classifier.4 reads it (kHeadThetaFloats)
};

namespace nbc {

inline PlanKey plan_key(const nbc_ctx* c, int N, int H, int W) {
  PlanKey k;
  k.N = N; k.H = H; k.W = W; k.precision = c->precision; k.arch = c->arch; k.keep = c->keep; k.bn = c->bn_mode;
  return k;
}

// A conv unit's arrays in the attached blob: f32 but for w of a conv_dma unit (panels of the precision's elements).
struct UnitPtrs {
  const float* w;
  const float* scale;
  const float* shift;
};
inline UnitPtrs unit_ptrs(const nbc_ctx* c, int unit) {
  const PackedConv& pc = c->layout.convs[unit];
  return {reinterpret_cast<const float*>(c->weights.data() + pc.w_off),
          reinterpret_cast<const float*>(c->weights.data() + pc.scale_off),
          reinterpret_cast<const float*>(c->weights.data() + pc.shift_off)};
}

// power of two the output of plan op `name` is stored with (nbc_api.hip)
bool stored_exponent(const nbc_ctx* c, const std::string& name, int* e);

// What the passes that read the stored input of classifier.4 ask of the context (the Dropout draws and votes, nbc_head_logits,
// nbc_head_gradient): its last forward was an NBC_ARCH_FCN_RESNET50 forward of this (N, H, W) and its plan stands untouched.
// *head: the plan's classifier.4.  `why_fcn_only` ends the refusal of another architecture.
inline int last_forward_head(const char* who, const nbc_ctx* c, int N, int H, int W, const Op** head, const char* why_fcn_only = "") {
  if (c->arch != kArchFcn)
    return fail(who, NBC_ERR_STATE, std::string("NBC_ARCH_FCN_RESNET50 only, the context holds ") + arch_name(c->arch) + why_fcn_only);
  if (!c->fwd_valid || c->fwd_N != N || c->fwd_H != H || c->fwd_W != W || !same_shape(c->plan, plan_key(c, N, H, W)))
    return fail(who, NBC_ERR_STATE, "the context's last forward was not one of this (N, H, W), or its plan has been touched since: run "
                                    "nbc_forward first");
  *head = nullptr;
  for (const Op& o : c->plan.ops)
    if (o.kind == OP_HEAD1X1) *head = &o;
  if (!*head || (*head)->Ci != 512 || (*head)->in_buf < 0 || !c->nonfinite)
    return fail(who, NBC_ERR_STATE, "the plan holds no classifier.4 of 512 input channels");
  return NBC_OK;
}

}  // namespace nbc
