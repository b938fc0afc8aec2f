// Context, plan cache, forward entry point and autotune of libnbc_hip.so; the launch plan itself is built in nbc_plan.cpp.
//
// nbc_forward replaces, at the C ABI, `outputs = self.model(batch[0].to(self.device))` followed
// by `torch.argmax(outputs, dim=1)` (/root/reference/src/bark_calculator/models.py:269-270).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nbc_ctx.hpp"
#include "nbc_kernels.hpp"
#include "reduce.hpp"

using namespace nbc;

namespace {

constexpr size_t kPlanCacheEntries = 64;

// Park the current plan (folders of height-trimmed images alternate between a few shapes: each keeps
// its launch list and its measured tile choice instead of being rebuilt on every change).
void stash_plan(nbc_ctx* c) {
  Plan& cur = c->plan;
  c->fwd_valid = false;
  if (cur.N == 0) return;
  for (Plan& p : c->plan_cache)
    if (same_shape(p, cur)) {
      p = cur; cur = Plan(); return;
    }
  if (c->plan_cache.size() >= kPlanCacheEntries) c->plan_cache.erase(c->plan_cache.begin());
  c->plan_cache.push_back(cur);
  cur = Plan();
}

// Room for buffer i of the current plan, grown with the margin (Buffer::reserve).
int ensure_buffer(nbc_ctx* c, int i) {
  const hipError_t e = c->bufs[i].reserve(c->plan.buf_bytes[i], Grow::kMargin);
  if (e != hipSuccess) return set_error(NBC_ERR_NOMEM, std::string("hipMalloc(workspace): ") + hipGetErrorString(e));
  return NBC_OK;
}

// Workspace of the current plan: a plan taken back from the cache finds its buffers large enough unless a later,
// smaller-indexed plan never needed that slot; a caller that knows its largest shape reserves it first (nbc_reserve).  The
// identity buffer is left to the first launch that writes it (launch_conv_op): the default path never does.
int ensure_buffers(nbc_ctx* c) {
  const Plan& P = c->plan;
  if (c->bufs.size() < P.buf_bytes.size()) c->bufs.resize(P.buf_bytes.size());
  for (int i = 0; i < (int)P.buf_bytes.size(); ++i)
    if (i != P.identity_buf) {
      const int rc = ensure_buffer(c, i);
      if (rc != NBC_OK) return rc;
    }
  if (P.bn == NBC_BN_PER_IMAGE) {
    if (!c->bn_unit.data()) {
      std::vector<float> unit(4096, 0.f);
      std::fill(unit.begin(), unit.begin() + 2048, 1.f);
      NBC_HIP(c->bn_unit.upload(unit.data(), unit.size()));
    }
    NBC_HIP(c->bn_ws.reserve(P.bn_ws_bytes));
  }
  NBC_HIP(c->lowres.reserve((size_t)P.N * kNumClasses * P.h * P.w * sizeof(float)));
  c->act_of.clear();
  for (size_t i = 0; i < P.ops.size(); ++i) c->act_of[P.ops[i].name] = (int)i;
  return NBC_OK;
}

// Checks a conv op's operand set against its packed unit and sizes it for the buffer resources (activations and weights stay
// below 2 GiB: kOutOfRange).
int conv_operand_bytes(const Op& o, const PackedConv& pc, int N, size_t eb, unsigned* x_bytes, unsigned* w_bytes) {
  if (o.Ci != pc.cin_pad) return set_error(NBC_ERR_STATE, "plan/channel mismatch at " + o.name);
  const size_t xb = (size_t)N * o.Hi * o.Wi * o.Ci * eb;
  const size_t wb = (size_t)o.Co * pc.ksteps * kKStepBytes;
  if (xb >= 0x80000000ull || wb >= 0x80000000ull)
    return set_error(NBC_ERR_INVALID, "activation of " + o.name + " exceeds 2 GiB: lower the batch size");
  *x_bytes = (unsigned)xb;
  *w_bytes = (unsigned)wb;
  return NBC_OK;
}

// One convolution launch of the plan (shared by nbc_forward and nbc_autotune).  ds: the downsample.0 op whose output is this
// op's identity, to be computed inside this launch (fusable_downsample below), or nullptr.  A downsample.0 of a pair that runs
// in a launch of its own finds the identity buffer here, allocated or grown on first use: that frees and allocates, so it
// synchronises the device as a change of shape does -- once per context and size, and only where the pair runs as two
// launches (the A/B switch, profiling, autotune, a forced or tuned tile without the dual-branch form).
int launch_conv_op(nbc_ctx* c, const Op& o, int N, int tile, hipStream_t s, hipError_t* err, const Op* ds = nullptr) {
  const ConvUnit& u = conv_units(c->arch)[o.unit];
  const PackedConv& pc = c->layout.convs[o.unit];
  const UnitPtrs p = unit_ptrs(c, o.unit);
  const int prec = c->precision;
  const size_t eb = elem_bytes(prec);
  ConvArgs a{};
  a.x = c->bufs[o.in_buf].get();
  a.w = p.w;
  a.scale = p.scale;
  a.shift = p.shift;
  a.res = o.res_buf >= 0 ? c->bufs[o.res_buf].get() : nullptr;
  if (o.raw) {                                         // per-image BatchNorm follows: fma(acc, 1, 0) = acc in f32
    if (o.Co > 2048) return set_error(NBC_ERR_STATE, "raw convolution wider than the unit table at " + o.name);
    a.scale = c->bn_unit.data();
    a.shift = c->bn_unit.data() + 2048;
    a.res = nullptr;
    // f16x2: the channel's power of two 2^(r - k - a_in) (nbc_pack_bn_raw), so that the pieces hold 2^r conv: exact in the fma
    if (prec == NBC_PREC_F16X2) a.scale = c->bn_raw.data() + o.affine_off;
  }
  if (o.out_buf == c->plan.identity_buf) {
    const int rc = ensure_buffer(c, o.out_buf);
    if (rc != NBC_OK) return rc;
  }
  a.y = c->bufs[o.out_buf].get();
  a.N = N; a.Hi = o.Hi; a.Wi = o.Wi; a.Ci = o.Ci;
  a.Ho = o.Ho; a.Wo = o.Wo; a.Co = o.Co;
  a.KH = u.k; a.KW = u.k; a.stride = u.stride; a.pad = u.pad; a.dil = u.dil;
  a.M = N * o.Ho * o.Wo;
  a.ksteps = pc.ksteps;
  a.relu = u.relu && !o.raw ? 1 : 0;
  a.stem = pc.stem ? 1 : 0;
  a.wo_shift = -1;
  a.hw_shift = -1;
  for (int sft = 0; sft < 31; ++sft) {
    if ((1 << sft) == o.Wo) a.wo_shift = sft;
    if ((1 << sft) == o.Ho * o.Wo) a.hw_shift = sft;
  }
  if (const int rc = conv_operand_bytes(o, pc, N, eb, &a.x_bytes, &a.w_bytes); rc != NBC_OK) return rc;
  if (ds) {                                            // the identity branch's operands; the tensor between the two is never stored
    const ConvUnit& u2 = conv_units(c->arch)[ds->unit];
    const PackedConv& pc2 = c->layout.convs[ds->unit];
    const UnitPtrs p2 = unit_ptrs(c, ds->unit);
    if (const int rc = conv_operand_bytes(*ds, pc2, N, eb, &a.x2_bytes, &a.w2_bytes); rc != NBC_OK) return rc;
    a.res = nullptr;
    a.x2 = c->bufs[ds->in_buf].get();
    a.w2 = p2.w;
    a.scale2 = p2.scale;
    a.shift2 = p2.shift;
    a.Ci2 = ds->Ci; a.Hi2 = ds->Hi; a.Wi2 = ds->Wi; a.stride2 = u2.stride; a.ksteps2 = pc2.ksteps;
  }
  if (o.gate_buf >= 0) {                               // EfficientNet's project conv: image n on its SE-gated weights
    const size_t xi = (size_t)o.Hi * o.Wi * o.Ci * eb, yi = (size_t)o.Ho * o.Wo * o.Co * eb;
    a.N = 1;
    a.M = o.Ho * o.Wo;
    a.x_bytes = (unsigned)xi;
    for (int n = 0; n < N; ++n) {
      a.x = static_cast<const unsigned char*>(c->bufs[o.in_buf].get()) + n * xi;
      a.w = static_cast<const unsigned char*>(c->bufs[o.gate_buf].get()) + n * (size_t)a.w_bytes;
      a.res = o.res_buf >= 0 ? static_cast<const unsigned char*>(c->bufs[o.res_buf].get()) + n * yi : nullptr;
      a.y = static_cast<unsigned char*>(c->bufs[o.out_buf].get()) + n * yi;
      *err = launch_conv_dma(a, prec, tile, s);
      if (*err != hipSuccess) break;
    }
    return NBC_OK;
  }
  *err = launch_conv_dma(a, prec, tile, s);
  return NBC_OK;
}

// Per-image BatchNorm statistics run on f32 activations and on f16x2 pieces of NBC_ARCH_FCN_RESNET50.
bool bn_per_image_ok(int precision, int arch) {
  return arch == kArchFcn && (precision == NBC_PREC_FP32 || precision == NBC_PREC_F16X2);
}

// Whether `conv3` is the conv3 of a (downsample.0, conv3) pair of the plan (Op::ds_op) that computes the downsample inside its
// own launch in this forward: fusion on, one timed launch per op not asked for (profiling off), conv3 on a tile (`tile3`) that
// has the dual-branch form.
bool fusable_downsample(const nbc_ctx* c, const Op& conv3, int tile3) {
  return conv3.ds_op >= 0 && c->fuse_downsample && !c->profiling && conv_tile_has_dual(c->precision, tile3);
}

const char* kernel_name(OpKind k) {
  switch (k) {
    case OP_INGEST: return "ingest";
    case OP_CONV: return "conv_dma";
    case OP_MAXPOOL: return "maxpool";
    case OP_HEAD1X1: return "head1x1";
    case OP_ASPP_POOL: return "aspp_pool";
    case OP_CONCAT: return "concat";
    case OP_BN_STATS: return "bn_stats";
    case OP_BN_APPLY: return "bn_apply";
    case OP_DWCONV: return "dwconv";
    case OP_SE_EXCITE: return "se_excite";
    case OP_GATE_WEIGHTS: return "gate_weights";
    case OP_SWISH: return "swish";
    default: return "upsample_argmax";
  }
}

}  // namespace

namespace nbc {

// power of two the output of plan op `name` is stored with: a conv unit's own, the max-pool keeps the stem's, the image has none
bool stored_exponent(const nbc_ctx* c, const std::string& name, int* e) {
  const auto& units = conv_units(c->arch);
  if (name == "ingest") { *e = 0; return true; }
  if (name == "backbone.maxpool") { *e = c->act_exp.empty() ? 0 : c->act_exp[0]; return true; }
  if (c->arch == kArchDeepLab && (name == "classifier.0.concat" || name == "classifier.0.convs.4")) {
    // the concat and the pooled vector: the power the five ASPP branches share (that of convs.0)
    return stored_exponent(c, "classifier.0.convs.0.0", e);
  }
  for (size_t u = 0; u < units.size(); ++u)
    if (units[u].name == name) { *e = u < c->act_exp.size() ? c->act_exp[u] : 0; return true; }
  return false;
}

}  // namespace nbc

extern "C" {

int nbc_create(nbc_ctx** out, int hip_device) {
  if (!out) return set_error(NBC_ERR_INVALID, "nbc_create: null out");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return set_error(NBC_ERR_HIP, std::string("nbc_create: no HIP device (") + hipGetErrorString(e) + ")");
  if (hip_device < 0 || hip_device >= ndev) return set_error(NBC_ERR_INVALID, "nbc_create: bad device index");
  NBC_HIP(hipSetDevice(hip_device));
  hipDeviceProp_t prop;
  NBC_HIP(hipGetDeviceProperties(&prop, hip_device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(NBC_ERR_HIP, std::string("nbc_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  nbc_ctx* c = new nbc_ctx();
  c->device = hip_device;
  *out = c;
  return NBC_OK;
}

int nbc_destroy(nbc_ctx* c) {
  if (!c) return NBC_OK;
  (void)hipSetDevice(c->device);
  delete c;
  return NBC_OK;
}

}  // extern "C"

namespace {

// nbc_attach_weights_arch.  `owned`: the block dev_blob lies in, which the context takes over once every check has passed
// (nbc_load_weights, the receiving nbc_bcast_weights), or nullptr for the caller's memory.  A refusal changes nothing.
int attach_weights(nbc_ctx* c, const void* dev_blob, size_t bytes, int precision, int arch, DeviceBuffer* owned) {
  if (!c || !dev_blob) return set_error(NBC_ERR_INVALID, "nbc_attach_weights: null argument");
  if (!known_precision(precision)) return set_error(NBC_ERR_INVALID, "nbc_attach_weights: unknown precision");
  if (!known_arch(arch)) return set_error(NBC_ERR_INVALID, "nbc_attach_weights: unknown architecture");
  if (is_effnet(arch) && precision != NBC_PREC_FP32)
    return set_error(NBC_ERR_INVALID, std::string("nbc_attach_weights: ") + arch_name(arch) + " runs in NBC_PREC_FP32 (fp32) only");
  PackedLayout L = packed_layout(precision, arch);
  if (bytes < L.total_bytes) return set_error(NBC_ERR_INVALID, "nbc_attach_weights: blob smaller than the packed layout");
  if (reinterpret_cast<uintptr_t>(dev_blob) % 256 != 0)
    return set_error(NBC_ERR_INVALID, "nbc_attach_weights: blob must be 256-byte aligned");
  // the trailer: pack flags and the powers of two the activation tensors are stored with (nbc_net.hpp)
  int32_t meta[kMetaWords];
  NBC_HIP(hipSetDevice(c->device));
  NBC_HIP(hipMemcpy(meta, static_cast<const unsigned char*>(dev_blob) + L.meta_off, sizeof(meta), hipMemcpyDeviceToHost));
  const int nunits = (int)conv_units(arch).size();
  if (meta[0] != kMetaMagic || meta[2] != nunits || meta[kMetaArch] != arch)
    return set_error(NBC_ERR_INVALID, "nbc_attach_weights: not a blob of this library's nbc_pack_weights for this architecture "
                                      "(trailer mismatch)");
  if (owned) c->weights.adopt(std::move(*owned), bytes);
  else c->weights.attach(static_cast<const unsigned char*>(dev_blob), bytes);
  c->pack_flags = meta[1];
  const int nexp = std::min(nunits, kMetaWords - kMetaExpBase);         // EfficientNet's trailer holds no exponents (f32)
  c->act_exp.assign(meta + kMetaExpBase, meta + kMetaExpBase + nexp);
  c->act_exp.resize(nunits, 0);
  if (is_effnet(arch)) std::fill(c->act_exp.begin(), c->act_exp.end(), 0);
  c->layout = L;
  c->fwd_valid = false;
  if (c->precision != precision || c->arch != arch) stash_plan(c);      // element size or network changed: another plan
  c->precision = precision;
  c->arch = arch;
  return NBC_OK;
}

// nbc_attach_bn_affine / nbc_attach_bn_raw: `what` names the array in the messages, `floats_of` is its
// nbc_arch_<what>_floats (0 for an architecture that has no such array).
int attach_bn_array(nbc_ctx* c, const std::string& what, size_t (*floats_of)(int), DeviceArray<float> nbc_ctx::*array,
                    const float* dev, size_t count) {
  if (!c || !dev) return set_error(NBC_ERR_INVALID, "nbc_attach_" + what + ": null argument");
  bool any = false;
  for (int a = 0; a < kArchDeepLabEffB0 + 8; ++a) any = any || (count > 0 && count == floats_of(a));
  if (!any)
    return set_error(NBC_ERR_INVALID, "nbc_attach_" + what + ": count is nbc_arch_" + what + "_floats of no architecture");
  NBC_HIP(hipSetDevice(c->device));
  (c->*array).attach(dev, count);                      // releasing an array owned before synchronises: nothing of it is in flight
  return NBC_OK;
}

}  // namespace

extern "C" {

int nbc_attach_weights_arch(nbc_ctx* c, const void* dev_blob, size_t bytes, int precision, int arch) {
  return attach_weights(c, dev_blob, bytes, precision, arch, nullptr);
}

int nbc_attach_weights(nbc_ctx* c, const void* dev_blob, size_t bytes, int precision) {
  return nbc_attach_weights_arch(c, dev_blob, bytes, precision, kArchFcn);
}

// Packs and uploads everything first, attaches afterwards: a refusal at any step leaves the context as it was.
int nbc_load_weights_arch(nbc_ctx* c, const nbc_tensor* tensors, int n, int precision, int arch) {
  if (!c) return set_error(NBC_ERR_INVALID, "nbc_load_weights: null context");
  const size_t bytes = nbc_arch_packed_weights_bytes(precision, arch);
  if (bytes == 0) return set_error(NBC_ERR_INVALID, "nbc_load_weights: unknown precision or architecture");
  std::vector<unsigned char> host(bytes);
  int rc = nbc_pack_weights_arch(tensors, n, precision, arch, host.data(), bytes);
  if (rc != NBC_OK) return rc;
  // the per-image BatchNorm affine array of the same tensors (already checked by the pack above)
  std::vector<float> affine(nbc_arch_bn_affine_floats(arch));
  rc = nbc_pack_bn_affine(tensors, n, arch, affine.data(), affine.size());
  if (rc != NBC_OK) return rc;
  // and, f16x2, the raw convolutions' powers of two (NBC_BN_PER_IMAGE on pieces) with their NBC_PACK_* bits
  std::vector<float> raw(precision == NBC_PREC_F16X2 && !is_effnet(arch) ? nbc_arch_bn_raw_floats(arch) : 0);
  const int raw_flags = raw.empty() ? 0 : nbc_pack_bn_raw(tensors, n, arch, raw.data(), raw.size());
  if (raw_flags < 0) return raw_flags;
  NBC_HIP(hipSetDevice(c->device));
  DeviceBuffer blob;
  DeviceArray<float> affine_dev, raw_dev;
  hipError_t e = blob.reserve(bytes);
  if (e == hipSuccess) e = HipMem::copy_in(blob.get(), host.data(), bytes);
  if (e != hipSuccess) return set_error(NBC_ERR_HIP, std::string("hipMemcpy(weights): ") + hipGetErrorString(e));
  e = affine_dev.upload(affine.data(), affine.size());
  if (e != hipSuccess) return set_error(NBC_ERR_HIP, std::string("hipMemcpy(bn affine): ") + hipGetErrorString(e));
  if (!raw.empty()) e = raw_dev.upload(raw.data(), raw.size());
  if (e != hipSuccess) return set_error(NBC_ERR_HIP, std::string("hipMemcpy(bn raw): ") + hipGetErrorString(e));
  rc = attach_weights(c, blob.get(), bytes, precision, arch, &blob);
  if (rc != NBC_OK) return rc;
  c->bn_affine = std::move(affine_dev);                // nothing below can fail; each old block is released as it is replaced
  if (!raw.empty()) { c->bn_raw = std::move(raw_dev); c->pack_flags |= raw_flags; }
  return NBC_OK;
}

int nbc_attach_bn_affine(nbc_ctx* c, const float* dev_affine, size_t count) {
  return attach_bn_array(c, "bn_affine", nbc_arch_bn_affine_floats, &nbc_ctx::bn_affine, dev_affine, count);
}

int nbc_attach_bn_raw(nbc_ctx* c, const float* dev_raw, size_t count) {
  return attach_bn_array(c, "bn_raw", nbc_arch_bn_raw_floats, &nbc_ctx::bn_raw, dev_raw, count);
}

int nbc_set_bn_statistics(nbc_ctx* c, int mode) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  if (mode != NBC_BN_RUNNING && mode != NBC_BN_PER_IMAGE) return set_error(NBC_ERR_INVALID, "nbc_set_bn_statistics: unknown mode");
  if (mode == NBC_BN_PER_IMAGE && !bn_per_image_ok(c->precision, c->arch))
    return set_error(NBC_ERR_STATE, "nbc_set_bn_statistics: per-image BatchNorm statistics need NBC_PREC_FP32 weights of "
                                    "NBC_ARCH_FCN_RESNET50 attached");
  if (c->bn_mode != mode) stash_plan(c);               // another launch list: park this one, like a precision change
  c->bn_mode = mode;
  return NBC_OK;
}

int nbc_load_weights(nbc_ctx* c, const nbc_tensor* tensors, int n, int precision) {
  return nbc_load_weights_arch(c, tensors, n, precision, kArchFcn);
}

// RCCL is resolved at call time from the host process (the library itself links libamdhip64 only):
// whatever librccl the host has loaded -- torch's own, or /opt/rocm's -- is the one whose communicator
// the caller hands in.
namespace {
typedef int (*nccl_bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_rank_fn)(void*, int*);
void* rccl_symbol(const char* name) {
  void* f = dlsym(RTLD_DEFAULT, name);
  if (f) return f;
  static void* handle = [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    return h ? h : dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  }();
  return handle ? dlsym(handle, name) : nullptr;
}
}  // namespace

int nbc_bcast_weights(nbc_ctx* c, void* rccl_comm, int root, int precision, void* hip_stream) {
  if (!c || !rccl_comm) return set_error(NBC_ERR_INVALID, "nbc_bcast_weights: null argument");
  if (c->arch != kArchFcn)
    return set_error(NBC_ERR_STATE, "nbc_bcast_weights: FCN-ResNet-50 only; broadcast the blob of another architecture yourself "
                                    "and attach it with nbc_attach_weights_arch");
  const size_t bytes = nbc_packed_weights_bytes(precision);
  if (bytes == 0) return set_error(NBC_ERR_INVALID, "nbc_bcast_weights: unknown precision");
  auto bcast = reinterpret_cast<nccl_bcast_fn>(rccl_symbol("ncclBroadcast"));
  auto user_rank = reinterpret_cast<nccl_rank_fn>(rccl_symbol("ncclCommUserRank"));
  if (!bcast || !user_rank) return set_error(NBC_ERR_STATE, "nbc_bcast_weights: no RCCL (librccl.so) in this process");
  int rank = -1;
  if (user_rank(rccl_comm, &rank) != 0) return set_error(NBC_ERR_INVALID, "nbc_bcast_weights: ncclCommUserRank failed (bad communicator?)");
  NBC_HIP(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  DeviceBuffer received;                               // a receiving rank's blob: the context's once the attach has taken it
  void* blob = nullptr;
  if (rank == root) {
    if (!c->weights.data() || c->precision != precision)
      return set_error(NBC_ERR_STATE, "nbc_bcast_weights: the root rank has no weights of this precision attached");
    blob = const_cast<unsigned char*>(c->weights.data());
  } else {
    NBC_HIP(received.reserve(bytes));
    blob = received.get();
  }
  const int rc = bcast(blob, blob, bytes, /*ncclUint8*/ 1, root, rccl_comm, s);
  if (rc != 0) return set_error(NBC_ERR_HIP, "nbc_bcast_weights: ncclBroadcast returned " + std::to_string(rc));
  // the blob held before is released by the attach (which synchronises: nothing of it is in flight), and only once it accepts
  return rank == root ? NBC_OK : attach_weights(c, blob, bytes, precision, kArchFcn, &received);
}

int nbc_weights_flags(nbc_ctx* c) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  if (!c->weights.data()) return set_error(NBC_ERR_STATE, "nbc_weights_flags: no weights attached");
  return c->pack_flags;
}

int nbc_activation_exponent(nbc_ctx* c, const char* name, int32_t* exponent) {
  if (!c || !name || !exponent) return set_error(NBC_ERR_INVALID, "nbc_activation_exponent: null argument");
  if (!c->weights.data()) return set_error(NBC_ERR_STATE, "nbc_activation_exponent: no weights attached");
  int e = 0;
  if (!stored_exponent(c, name, &e)) return set_error(NBC_ERR_INVALID, std::string("nbc_activation_exponent: unknown op ") + name);
  *exponent = e;
  return NBC_OK;
}

int nbc_set_normalization(nbc_ctx* c, const float mean[3], const float stdv[3]) {
  if (!c || !mean || !stdv) return set_error(NBC_ERR_INVALID, "nbc_set_normalization: null argument");
  for (int i = 0; i < 3; ++i) { c->mean[i] = mean[i]; c->stdv[i] = stdv[i]; }
  return NBC_OK;
}

int nbc_set_conv_tile(nbc_ctx* c, int tile) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  if (tile < -1 || tile >= CONV_TILE_COUNT) return set_error(NBC_ERR_INVALID, "nbc_set_conv_tile: bad tile id");
  c->conv_tile = tile;
  return NBC_OK;
}

int nbc_set_fuse_downsample(nbc_ctx* c, int on) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  c->fuse_downsample = on != 0;
  return NBC_OK;
}

int nbc_set_logit_offsets(nbc_ctx* c, float bark, float node) {
  if (!std::isfinite(bark) || !std::isfinite(node)) return set_error(NBC_ERR_INVALID, "nbc_set_logit_offsets: the offsets must be finite");
  if (!c) return set_error(NBC_ERR_INVALID, "nbc_set_logit_offsets: null context");
  c->logit_offsets[0] = bark;
  c->logit_offsets[1] = node;
  c->offsets_on = bark != 0.f || node != 0.f;
  return NBC_OK;
}

int nbc_fused_pairs(nbc_ctx* c) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  return c->fused_pairs;
}

int nbc_set_keep_activations(nbc_ctx* c, int on) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  if (c->keep != (on != 0)) stash_plan(c);
  c->keep = on != 0;
  return NBC_OK;
}

int nbc_nonfinite_seen(nbc_ctx* c, int reset) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  if (!c->nonfinite) return 0;                       // no forward yet
  NBC_HIP(hipSetDevice(c->device));
  unsigned v = 0;
  NBC_HIP(hipDeviceSynchronize());                   // every forward on every stream (non-blocking ones too) has finished
  NBC_HIP(hipMemcpy(&v, c->nonfinite.get(), sizeof(v), hipMemcpyDeviceToHost));
  if (reset && v) NBC_HIP(hipMemset(c->nonfinite.get(), 0, sizeof(v)));
  return v ? 1 : 0;
}

int nbc_nonfinite_peek_async(nbc_ctx* c, uint32_t* host_dst, void* hip_stream) {
  if (!c || !host_dst) return set_error(NBC_ERR_INVALID, "nbc_nonfinite_peek_async: null argument");
  NBC_HIP(hipSetDevice(c->device));
  {
    // pinned memory only: a copy to pageable memory is staged and may block (the contract is "no synchronisation")
    hipPointerAttribute_t at{};
    const hipError_t pe = hipPointerGetAttributes(&at, host_dst);
    if (pe != hipSuccess || at.type != hipMemoryTypeHost) {
      (void)hipGetLastError();
      return set_error(NBC_ERR_INVALID, "nbc_nonfinite_peek_async: host_dst must be pinned host memory (hipHostMalloc / hipHostRegister)");
    }
  }
  if (!c->nonfinite) { *host_dst = 0; return NBC_OK; }   // no forward yet
  NBC_HIP(hipMemcpyAsync(host_dst, c->nonfinite.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, static_cast<hipStream_t>(hip_stream)));
  return NBC_OK;
}

int nbc_set_profiling(nbc_ctx* c, int on) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  c->profiling = on != 0;
  return NBC_OK;
}

int nbc_reserve(nbc_ctx* c, int N, int H, int W) {
  if (!c) return set_error(NBC_ERR_INVALID, "null context");
  if (c->precision < 0) return set_error(NBC_ERR_STATE, "nbc_reserve: no weights attached");
  if (N < 1 || H < 8 || W < 8) return set_error(NBC_ERR_INVALID, "nbc_reserve: need N>=1, H>=8, W>=8");
  if (c->bn_mode == NBC_BN_PER_IMAGE) {
    if (!bn_per_image_ok(c->precision, c->arch))
      return set_error(NBC_ERR_STATE, "per-image BatchNorm statistics need NBC_PREC_FP32 weights of NBC_ARCH_FCN_RESNET50 attached");
    if (c->bn_affine.count() != nbc_arch_bn_affine_floats(c->arch))
      return set_error(NBC_ERR_STATE, "per-image BatchNorm statistics: no affine array of this architecture attached "
                                      "(nbc_attach_bn_affine)");
    if (c->precision == NBC_PREC_F16X2 && c->bn_raw.count() != nbc_arch_bn_raw_floats(c->arch))
      return set_error(NBC_ERR_STATE, "per-image BatchNorm statistics in NBC_PREC_F16X2: no raw-convolution array of this "
                                      "architecture attached (nbc_attach_bn_raw)");
  }
  NBC_HIP(hipSetDevice(c->device));
  const PlanKey key = plan_key(c, N, H, W);
  if (same_shape(c->plan, key)) return NBC_OK;
  stash_plan(c);
  bool found = false;
  for (const Plan& p : c->plan_cache)
    if (same_shape(p, key)) { c->plan = p; found = true; break; }
  if (!found) {
    const std::string refused = build_plan(key, &c->plan);
    if (!refused.empty()) return set_error(NBC_ERR_INVALID, refused);
  }
  int rc = ensure_buffers(c);
  if (rc != NBC_OK) c->plan = Plan();
  return rc;
}

int nbc_describe_plan(int arch, int precision, int N, int H, int W, int keep, int bn_mode, char* text, size_t capacity) {
  if (!known_arch(arch) || !known_precision(precision) || (is_effnet(arch) && precision != NBC_PREC_FP32))
    return set_error(NBC_ERR_INVALID, "nbc_describe_plan: unknown architecture or precision, or one the architecture does not run in");
  if (N < 1 || H < 8 || W < 8) return set_error(NBC_ERR_INVALID, "nbc_describe_plan: need N>=1, H>=8, W>=8");
  if (bn_mode != NBC_BN_RUNNING && (bn_mode != NBC_BN_PER_IMAGE || !bn_per_image_ok(precision, arch)))
    return set_error(NBC_ERR_INVALID, "nbc_describe_plan: per-image BatchNorm statistics need NBC_PREC_FP32 and NBC_ARCH_FCN_RESNET50");
  PlanKey key;
  key.N = N; key.H = H; key.W = W; key.precision = precision; key.arch = arch; key.keep = keep != 0; key.bn = bn_mode;
  Plan P;
  const std::string refused = build_plan(key, &P);
  if (!refused.empty()) return set_error(NBC_ERR_INVALID, refused);
  std::string out;
  const auto field = [&](const char* what, int v) { if (v >= 0) out += std::string(" ") + what + "=" + std::to_string(v); };
  for (const Op& o : P.ops) {
    out += "op " + o.name + " " + kernel_name(o.kind);
    field("in", o.in_buf); field("out", o.out_buf); field("res", o.res_buf); field("ws", o.ws_buf); field("gate", o.gate_buf);
    for (int b : o.cat_in) field("cat", b);
    if (o.kind == OP_CONV) field("tile", o.tile);
    field("launches", o.launches);
    if (o.ds_op >= 0) out += " ds=" + P.ops[o.ds_op].name;
    out += "\n";
  }
  for (size_t i = 0; i < P.buf_bytes.size(); ++i)
    out += "buf " + std::to_string(i) + " " + std::to_string(P.buf_bytes[i]) + ((int)i == P.identity_buf ? " identity\n" : "\n");
  if (text && capacity > 0) {
    const size_t n = std::min(out.size(), capacity - 1);
    std::memcpy(text, out.data(), n);
    text[n] = 0;
  }
  return (int)out.size() + 1;
}

int nbc_forward(nbc_ctx* c, const void* x_dev, int x_dtype, int N, int H, int W,
                float* logits_lowres_dev, float* logits_full_dev, void* labels_dev, int labels_dtype,
                int64_t* counts_dev, int exclude_nodes, void* hip_stream) {
  if (!c || !x_dev) return set_error(NBC_ERR_INVALID, "nbc_forward: null argument");
  if (!c->weights.data()) return set_error(NBC_ERR_STATE, "nbc_forward: no weights attached (load_state_dict first)");
  if (x_dtype != NBC_IN_F32_NCHW && x_dtype != NBC_IN_U8_NHWC) return set_error(NBC_ERR_INVALID, "nbc_forward: bad x_dtype");
  if (!label_dtype_ok(labels_dtype)) return set_error(NBC_ERR_INVALID, "nbc_forward: bad labels_dtype");
  c->fwd_valid = false;
  int rc = nbc_reserve(c, N, H, W);
  if (rc != NBC_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const Plan& P = c->plan;
  const int prec = c->precision;
  if (!c->nonfinite) {
    NBC_HIP(c->nonfinite.reserve(256));
    NBC_HIP(hipMemset(c->nonfinite.get(), 0, 256));
  }

  const size_t nops = P.ops.size();
  constexpr size_t kMaxProfSets = 4096;
  std::vector<Event>* evs = nullptr;
  if (c->profiling && c->prof_used < kMaxProfSets) {
    if (c->prof_used > 0 && c->prof_ops.size() != nops) c->prof_used = 0;   // plan changed: restart
    if (c->prof_sets.size() <= c->prof_used) c->prof_sets.emplace_back();
    evs = &c->prof_sets[c->prof_used];
    while (evs->size() < nops + 1) {
      Event ev;
      NBC_HIP(ev.create());
      evs->push_back(std::move(ev));
    }
    c->prof_ops = P.ops;
    c->prof_arch = P.arch;
  }
  float* lowres = logits_lowres_dev ? logits_lowres_dev : c->lowres.as<float>();

  c->fused_pairs = 0;
  if (evs) NBC_HIP(hipEventRecord((*evs)[0], s));
  for (size_t l = 0; l < nops; ++l) {
    const Op& o = P.ops[l];
    hipError_t e = hipSuccess;
    int rc = NBC_OK;
    switch (o.kind) {
      case OP_INGEST:
        if (x_dtype == NBC_IN_F32_NCHW)
          e = launch_ingest_f32(static_cast<const float*>(x_dev), c->bufs[o.out_buf].get(), N, H, W, prec, s);
        else
          e = launch_ingest_u8(static_cast<const uint8_t*>(x_dev), c->bufs[o.out_buf].get(), N, H, W, c->mean, c->stdv, prec, s);
        break;
      case OP_CONV: {
        const auto tile_of = [&](const Op& q) {
          // no override, or it does not fit (a generic tile on a layer of the row-resident kernel, or the reverse): planned tile
          return conv_tile_ok(prec, c->conv_tile, q.Co, q.rows) ? c->conv_tile : q.tile;
        };
        if (l + 1 < nops && P.ops[l + 1].ds_op == (int)l && fusable_downsample(c, P.ops[l + 1], tile_of(P.ops[l + 1])))
          break;                                       // downsample.0: the next op's launch computes it
        const Op* ds = fusable_downsample(c, o, tile_of(o)) ? &P.ops[o.ds_op] : nullptr;
        rc = launch_conv_op(c, o, N, tile_of(o), s, &e, ds);
        if (rc != NBC_OK) return rc;
        if (ds && e == hipSuccess) ++c->fused_pairs;
        break;
      }
      case OP_MAXPOOL:
        e = launch_maxpool3x3s2(c->bufs[o.in_buf].get(), c->bufs[o.out_buf].get(), N, o.Hi, o.Wi, o.Ci, o.Ho, o.Wo, prec, s);
        break;
      case OP_HEAD1X1: {
        const UnitPtrs p = unit_ptrs(c, o.unit);
        if (o.Ci != 512 && o.Ci != 256 && !is_effnet(c->arch))
          return set_error(NBC_ERR_STATE, "classifier.4 expects 512 or 256 input channels");
        // also clears the class counters (3 per image) when the batch is small enough (head_clears_counts; else OP_UPSAMPLE does)
        unsigned long long* cz = reinterpret_cast<unsigned long long*>(counts_dev);
        if (is_effnet(c->arch) && o.Ci != 256)             // FCNHead(inplanes, 3): inplanes / 4 channels, padded; at 512 (b5) too
          e = launch_head1x1_any(static_cast<const float*>(c->bufs[o.in_buf].get()), p.w, p.shift, lowres, N, o.Ho * o.Wo, o.Ci, cz,
                                 c->nonfinite.as<unsigned>(), s);
        else
          e = launch_head1x1(c->bufs[o.in_buf].get(), o.Ci, p.w, p.shift, lowres, N, o.Ho * o.Wo, prec, cz, c->nonfinite.as<unsigned>(), s);
        break;
      }
      case OP_ASPP_POOL: {
        const UnitPtrs p = unit_ptrs(c, o.unit);
        float* partial = static_cast<float*>(c->bufs[o.ws_buf].get());
        float* mean = partial + (size_t)N * aspp_pool_slices(o.Hi * o.Wi) * o.Ci;
        e = launch_aspp_pool(c->bufs[o.in_buf].get(), N, o.Hi * o.Wi, o.Ci, p.w, p.scale, p.shift, o.Co, partial, mean, c->bufs[o.out_buf].get(),
                             prec, s);
        break;
      }
      case OP_CONCAT: {
        const void* br[4] = {c->bufs[o.cat_in[0]].get(), c->bufs[o.cat_in[1]].get(), c->bufs[o.cat_in[2]].get(), c->bufs[o.cat_in[3]].get()};
        e = launch_aspp_concat(br, c->bufs[o.cat_in[4]].get(), c->bufs[o.out_buf].get(), N, o.Ho * o.Wo, prec, s);
        break;
      }
      case OP_BN_STATS: {                              // f16x2: the unit's 2^-r follows its raw scales; the table carries the tensor's 2^a_out
        const float* gamma = c->bn_affine.data() + o.affine_off;
        const bool x2 = prec == NBC_PREC_F16X2;
        e = launch_bn_stats(c->bufs[o.out_buf].get(), N, o.Ho * o.Wo, o.Co, gamma, gamma + o.Co,
                            x2 ? c->bn_raw.data() + o.affine_off + o.Co : nullptr, x2 ? c->act_exp[o.unit] : 0, c->bn_ws.get(),
                            c->nonfinite.as<unsigned>(), prec, s);
        break;
      }
      case OP_BN_APPLY:                                // with the tables the statistics op left in the workspace
        e = launch_bn_apply(c->bufs[o.out_buf].get(), o.res_buf >= 0 ? c->bufs[o.res_buf].get() : nullptr, N, o.Ho * o.Wo, o.Co,
                            c->bn_ws.get(), o.relu, prec, s);
        break;
      case OP_DWCONV: {
        const UnitPtrs p = unit_ptrs(c, o.unit);
        const ConvUnit& u = conv_units(c->arch)[o.unit];
        DwArgs a{};
        a.x = static_cast<const float*>(c->bufs[o.in_buf].get());
        a.w = p.w;
        a.scale = p.scale;
        a.shift = p.shift;
        a.y = static_cast<float*>(c->bufs[o.out_buf].get());
        a.partial = static_cast<float*>(c->bufs[o.ws_buf].get());
        a.N = N; a.Hi = o.Hi; a.Wi = o.Wi; a.C = o.Co; a.Ho = o.Ho; a.Wo = o.Wo;
        a.k = u.k; a.stride = u.stride; a.pad_t = u.pad; a.pad_l = u.pad; a.in_swish = u.in_swish ? 1 : 0;
        e = launch_dwconv(a, s);
        break;
      }
      case OP_SE_EXCITE: {
        const UnitPtrs pr = unit_ptrs(c, o.unit), pe = unit_ptrs(c, o.aux_unit);
        const ConvUnit& ur = conv_units(c->arch)[o.unit];
        e = launch_se_excite(static_cast<const float*>(c->bufs[o.in_buf].get()), N, o.tiles, o.Co, o.Hi * o.Wi, pr.w, pr.shift, ur.cout,
                             pe.w, pe.shift, static_cast<float*>(c->bufs[o.out_buf].get()), s);
        break;
      }
      case OP_GATE_WEIGHTS:
        e = launch_gate_weights(unit_ptrs(c, o.unit).w, static_cast<const float*>(c->bufs[o.gate_buf].get()),
                                static_cast<float*>(c->bufs[o.ws_buf].get()), N, o.Co, o.Ci, s);
        break;
      case OP_SWISH:
        e = launch_swish(static_cast<float*>(c->bufs[o.out_buf].get()), (size_t)N * o.Ho * o.Wo * o.Co, s);
        break;
      case OP_UPSAMPLE:
        if (counts_dev && !head_clears_counts(N)) {  // more counters than classifier.4's launch clears
          e = hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * 3 * N, s);
          if (e != hipSuccess) break;
        }
        if (logits_full_dev || labels_dev || counts_dev)
          e = launch_upsample_argmax(lowres, N, P.h, P.w, H, W, logits_full_dev, labels_dev,
                                     labels_dtype == NBC_LABEL_I64 ? 1 : 0,
                                     reinterpret_cast<unsigned long long*>(counts_dev), exclude_nodes, s,
                                     c->offsets_on ? c->logit_offsets : nullptr);
        break;
    }
    if (e != hipSuccess)
      return set_error(NBC_ERR_HIP, "launch of " + o.name + " failed: " + hipGetErrorString(e));
    if (evs) NBC_HIP(hipEventRecord((*evs)[l + 1], s));
  }
  if (evs) ++c->prof_used;
  c->fwd_valid = true;
  c->fwd_N = N; c->fwd_H = H; c->fwd_W = W;
  return NBC_OK;
}

}  // extern "C"

// Average the event sets recorded since the last call (synchronises on the last one), then reset.
static int collect_profile(nbc_ctx* c) {
  if (c->prof_used == 0) return NBC_OK;
  const auto& units = conv_units(c->prof_arch);
  const size_t nops = c->prof_ops.size();
  NBC_HIP(hipEventSynchronize(c->prof_sets[c->prof_used - 1][nops]));
  c->records.assign(nops, nbc_op_record{});
  std::vector<double> sum(nops, 0.0);
  for (size_t i = 0; i < nops; ++i)
    for (size_t k = 0; k < c->prof_used; ++k) {
      float ms = 0.f;
      NBC_HIP(hipEventElapsedTime(&ms, c->prof_sets[k][i], c->prof_sets[k][i + 1]));
      sum[i] += ms;
    }
  for (size_t i = 0; i < nops; ++i) {
    const Op& o = c->prof_ops[i];
    nbc_op_record& r = c->records[i];
    std::snprintf(r.name, sizeof(r.name), "%s", o.name.c_str());
    std::snprintf(r.kernel, sizeof(r.kernel), "%s", kernel_name(o.kind));
    r.ms = (float)(sum[i] / (double)c->prof_used);
    r.calls = (int32_t)c->prof_used;
    r.launches = o.launches;
    r.flops = o.flops;
    r.bytes = o.bytes;
    r.kh = r.kw = (o.kind == OP_CONV || o.kind == OP_HEAD1X1) ? units[o.unit].k : 0;
    r.cout = o.Co;
  }
  c->prof_used = 0;
  return NBC_OK;
}

extern "C" {

int nbc_autotune(nbc_ctx* c, const void* x_dev, int x_dtype, int N, int H, int W, int reps, int objective,
                 void* hip_stream) {
  if (!c || !x_dev) return set_error(NBC_ERR_INVALID, "nbc_autotune: null argument");
  if (reps < 1) reps = 3;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  // one real forward first: every activation buffer then holds realistic data for the timed launches
  int rc = nbc_forward(c, x_dev, x_dtype, N, H, W, nullptr, nullptr, nullptr, NBC_LABEL_U8, nullptr, 0, hip_stream);
  if (rc != NBC_OK) return rc;
  NBC_HIP(hipStreamSynchronize(s));
  c->fwd_valid = false;                    // the timed launches below rewrite activations (raw ones in NBC_BN_PER_IMAGE)
  Event e0, e1;
  NBC_HIP(e0.create());
  NBC_HIP(e1.create());
  Plan& P = c->plan;
  for (size_t oi = 0; oi < P.ops.size(); ++oi) {
    Op& o = P.ops[oi];
    if (o.kind != OP_CONV) continue;
    float best_ms = 1e30f;
    int best = o.tile;
    for (int tile = 0; tile < CONV_TILE_COUNT; ++tile) {
      if (!conv_tile_ok(c->precision, tile, o.Co, o.rows)) continue;
      hipError_t e = hipSuccess;
      rc = launch_conv_op(c, o, N, tile, s, &e);                         // warm-up (and attribute set-up)
      if (rc != NBC_OK || e != hipSuccess) continue;
      (void)hipEventRecord(e0, s);
      for (int k = 0; k < reps; ++k) (void)launch_conv_op(c, o, N, tile, s, &e);
      (void)hipEventRecord(e1, s);
      if (hipEventSynchronize(e1) != hipSuccess) continue;
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) continue;
      if (objective == 1) {
        // throughput objective: several forwards run concurrently on other streams, so a launch that
        // fills only part of the chip costs only that part: weigh the time by the fraction of CUs used
        const int tiles = ((N * o.Ho * o.Wo + conv_tile_rows(tile) - 1) / conv_tile_rows(tile)) * (o.Co / conv_tile_cols(tile));
        if (tiles < 256) ms *= (float)tiles / 256.0f;
      }
      if (ms < best_ms) { best_ms = ms; best = tile; }
    }
    o.tile = best;
  }
  return NBC_OK;
}

int nbc_get_plan_tiles(nbc_ctx* c, int32_t* tiles, int capacity) {
  if (!c || !tiles) return set_error(NBC_ERR_INVALID, "nbc_get_plan_tiles: null argument");
  int n = 0;
  for (const Op& o : c->plan.ops)
    if (o.kind == OP_CONV) { if (n < capacity) tiles[n] = o.tile; ++n; }
  return n;
}

int nbc_default_conv_tile(int M, int Cout, int K, int precision) {
  if (M < 1 || Cout < 1 || K < 1) return -1;
  return choose_conv_tile(M, Cout, K, precision, 0);
}

int nbc_set_plan_tiles(nbc_ctx* c, const int32_t* tiles, int n) {
  if (!c || !tiles) return set_error(NBC_ERR_INVALID, "nbc_set_plan_tiles: null argument");
  int convs = 0;
  for (const Op& o : c->plan.ops) convs += o.kind == OP_CONV;
  if (convs == 0) return set_error(NBC_ERR_STATE, "nbc_set_plan_tiles: no plan (nbc_reserve first)");
  if (n != convs) return set_error(NBC_ERR_INVALID, "nbc_set_plan_tiles: the plan has " + std::to_string(convs) + " convolutions");
  int k = 0;
  for (const Op& o : c->plan.ops) {
    if (o.kind != OP_CONV) continue;
    const int t = tiles[k++];
    if (!conv_tile_ok(c->precision, t, o.Co, o.rows))
      return set_error(NBC_ERR_INVALID, "nbc_set_plan_tiles: tile " + std::to_string(t) + " does not fit " + o.name);
  }
  k = 0;
  for (Op& o : c->plan.ops)
    if (o.kind == OP_CONV) o.tile = tiles[k++];
  return NBC_OK;
}

int nbc_upsample_argmax(nbc_ctx* c, const float* lowres, int N, int h, int w, int H, int W,
                        float* logits_full_dev, void* labels_dev, int labels_dtype,
                        int64_t* counts_dev, int exclude_nodes, void* hip_stream) {
  if (!c || !lowres) return set_error(NBC_ERR_INVALID, "nbc_upsample_argmax: null argument");
  if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return set_error(NBC_ERR_INVALID, "nbc_upsample_argmax: bad shape");
  if (!label_dtype_ok(labels_dtype)) return set_error(NBC_ERR_INVALID, "nbc_upsample_argmax: bad labels_dtype");
  NBC_HIP(hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (counts_dev) NBC_HIP(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * 3 * N, s));
  NBC_HIP(launch_upsample_argmax(lowres, N, h, w, H, W, logits_full_dev, labels_dev,
                                 labels_dtype == NBC_LABEL_I64 ? 1 : 0,
                                 reinterpret_cast<unsigned long long*>(counts_dev), exclude_nodes, s,
                                 c->offsets_on ? c->logit_offsets : nullptr));
  return NBC_OK;
}

int nbc_resize_cubic_u8(nbc_ctx* c, const uint8_t* src_dev, int H, int W, float* dst_dev, int out_h, int out_w,
                        void* hip_stream) {
  if (!c || !src_dev || !dst_dev) return set_error(NBC_ERR_INVALID, "nbc_resize_cubic_u8: null argument");
  if (H < 1 || W < 1 || out_h < 1 || out_w < 1) return set_error(NBC_ERR_INVALID, "nbc_resize_cubic_u8: bad shape");
  NBC_HIP(hipSetDevice(c->device));
  NBC_HIP(c->scratch256.reserve(256));
  unsigned* minmax = c->scratch256.as<unsigned>();
  NBC_HIP(launch_resize_cubic_u8(src_dev, H, W, dst_dev, nullptr, nullptr, out_h, out_w, minmax, static_cast<hipStream_t>(hip_stream)));
  return NBC_OK;
}

int nbc_preprocess_u8(nbc_ctx* c, const uint8_t* src_dev, int H, int W, uint8_t* dst_u8_dev, int32_t* row_lit_dev, int out_h,
                      int out_w, void* hip_stream) {
  if (!c || !src_dev || !dst_u8_dev) return set_error(NBC_ERR_INVALID, "nbc_preprocess_u8: null argument");
  if (H < 1 || W < 1 || out_h < 1 || out_w < 1) return set_error(NBC_ERR_INVALID, "nbc_preprocess_u8: bad shape");
  NBC_HIP(hipSetDevice(c->device));
  NBC_HIP(c->scratch256.reserve(256));
  unsigned* minmax = c->scratch256.as<unsigned>();
  NBC_HIP(launch_resize_cubic_u8(src_dev, H, W, nullptr, dst_u8_dev, row_lit_dev, out_h, out_w, minmax,
                                 static_cast<hipStream_t>(hip_stream)));
  return NBC_OK;
}

int nbc_num_op_records(nbc_ctx* c) {
  if (!c) return 0;
  if (collect_profile(c) != NBC_OK) return NBC_ERR_HIP;
  return (int)c->records.size();
}

int nbc_get_op_record(nbc_ctx* c, int index, nbc_op_record* out) {
  if (!c || !out || index < 0 || index >= (int)c->records.size())
    return set_error(NBC_ERR_INVALID, "nbc_get_op_record: bad index");
  *out = c->records[index];
  return NBC_OK;
}

int nbc_activation_peaks(nbc_ctx* c, float* peaks_host, int capacity) {
  if (!c || !peaks_host) return set_error(NBC_ERR_INVALID, "nbc_activation_peaks: null argument");
  if (!c->plan.keep) return set_error(NBC_ERR_STATE, "nbc_activation_peaks: keep-activations is off (nbc_set_keep_activations, then a forward)");
  const int nunits = (int)conv_units(c->plan.arch).size();
  if (capacity < nunits) return set_error(NBC_ERR_INVALID, "nbc_activation_peaks: need room for nbc_arch_num_convs() values");
  NBC_HIP(hipSetDevice(c->device));
  DeviceBuffer tmp;
  NBC_HIP(tmp.reserve(sizeof(unsigned) * nunits));
  unsigned* dev = tmp.as<unsigned>();
  hipError_t e = hipMemset(dev, 0, sizeof(unsigned) * nunits);
  const int N = c->plan.N;
  for (const Op& o : c->plan.ops) {
    if (e != hipSuccess) break;
    if ((o.kind != OP_CONV && o.kind != OP_ASPP_POOL) || o.out_buf < 0) continue;   // the pooling branch: its pooled vector
    e = launch_absmax(c->bufs[o.out_buf].get(), (size_t)N * o.Ho * o.Wo * o.Co, o.Co, c->precision, dev + o.unit, nullptr);
  }
  std::vector<unsigned> bits(nunits, 0u);
  if (e == hipSuccess) e = hipMemcpy(bits.data(), dev, sizeof(unsigned) * nunits, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return set_error(NBC_ERR_HIP, std::string("nbc_activation_peaks: ") + hipGetErrorString(e));
  for (int u = 0; u < nunits; ++u) std::memcpy(&peaks_host[u], &bits[u], 4);
  return nunits;
}

int nbc_read_activation(nbc_ctx* c, const char* name, float* dst_host, size_t capacity, int64_t shape[4]) {
  if (!c || !name || !dst_host) return set_error(NBC_ERR_INVALID, "nbc_read_activation: null argument");
  if (!c->plan.keep) return set_error(NBC_ERR_STATE, "nbc_read_activation: keep-activations is off");
  auto it = c->act_of.find(name);
  if (it == c->act_of.end()) return set_error(NBC_ERR_INVALID, std::string("nbc_read_activation: unknown op ") + name);
  const Op& o = c->plan.ops[it->second];
  if (o.out_buf < 0) return set_error(NBC_ERR_INVALID, "nbc_read_activation: op has no activation buffer");
  const int N = c->plan.N;
  const int creal = o.creal > 0 ? o.creal : o.Co;     // EfficientNet: the pad channels stay behind
  const size_t elems = (size_t)N * o.Ho * o.Wo * creal;
  if (capacity < elems) return set_error(NBC_ERR_INVALID, "nbc_read_activation: destination too small");
  NBC_HIP(hipSetDevice(c->device));
  const size_t img = (size_t)o.Ho * o.Wo * o.Co;        // NCHW of the (padded) tensor
  DeviceBuffer nchw;
  NBC_HIP(nchw.reserve((size_t)N * img * sizeof(float)));
  float* tmp = nchw.as<float>();
  hipError_t e = launch_nhwc_to_nchw_f32(c->bufs[o.out_buf].get(), tmp, N, o.Ho, o.Wo, o.Co, c->precision, nullptr);
  if (creal == o.Co) {
    if (e == hipSuccess) e = hipMemcpy(dst_host, tmp, elems * sizeof(float), hipMemcpyDeviceToHost);
  } else {                                             // each image's first creal channels
    for (int n = 0; n < N && e == hipSuccess; ++n)
      e = hipMemcpy(dst_host + (size_t)n * o.Ho * o.Wo * creal, tmp + n * img, (size_t)o.Ho * o.Wo * creal * sizeof(float),
                    hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return set_error(NBC_ERR_HIP, std::string("nbc_read_activation: ") + hipGetErrorString(e));
  int a = 0;
  if (stored_exponent(c, o.name, &a) && a != 0)        // f16x2: the tensor as the network defines it (power of two taken off, exact)
    for (size_t i = 0; i < elems; ++i) dst_host[i] = std::ldexp(dst_host[i], -a);
  if (shape) { shape[0] = N; shape[1] = creal; shape[2] = o.Ho; shape[3] = o.Wo; }
  return NBC_OK;
}

}  // extern "C"
