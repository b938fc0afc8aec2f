/*
 * nbc.h -- C ABI of the MI355X-native FCN-ResNet-50 segmentation path ("nbc" = neural bark
 * calculator).  One shared library, libnbc_hip.so, plain pointers and sizes only; no torch
 * types.  All file:line citations are into /root/reference/src/bark_calculator/.
 *
 * What this boundary replaces in the reference:
 *   - the object bound to `self.model`            models.py:221   fcn_resnet50(pretrained=False)
 *   - `self.model.load_state_dict(...)`           models.py:222   -> nbc_pack_weights / nbc_load_weights
 *   - `self.model.to(device)`                     models.py:223   -> nbc_create(device) + nbc_attach_weights
 *   - `outputs = self.model(batch[0].to(device))` models.py:269   -> nbc_forward (logits_full_dev)
 *   - `outputs = torch.argmax(outputs, dim=1)`    models.py:270   -> nbc_forward (labels_dev)
 *   - the `--exclude_nodes` remap 2 -> 1          models.py:273-276 -> nbc_forward (exclude_nodes)
 *   - the per-class pixel counting                models.py:324-331 -> nbc_forward (counts_dev)
 *   - ToTensor + Normalize of the loaded image    dataset.py:175-186, models.py:233-237
 *                                                 -> nbc_forward with NBC_IN_U8_NHWC
 *
 * Conventions: every function returns 0 (NBC_OK) or a negative error code; the message of the
 * last error on the calling thread is nbc_last_error().  Nothing throws across the ABI.  A
 * context is bound to one HIP device and is not thread-safe (the reference loop is
 * single-threaded, models.py:257-270).  The caller owns every input/output buffer; the context
 * owns its activation workspace (sized on the first call for an (N,H,W), then reused: no
 * allocation in steady state).  Work is enqueued on the caller's stream; outputs are valid
 * once that stream has been synchronised.
 *
 * Eval mode by default: BatchNorm uses running statistics, Dropout is the identity.  The shipped tool's
 * per-image BatchNorm statistics and its live Dropout are opt-in: nbc_set_bn_statistics, nbc_dropout_draws.
 */
#ifndef NBC_H
#define NBC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbc_ctx nbc_ctx;

enum {
  NBC_OK = 0,
  NBC_ERR_INVALID = -1,   /* bad argument / shape */
  NBC_ERR_KEYS = -2,      /* state_dict keys or shapes do not match (models.py:222 would raise) */
  NBC_ERR_HIP = -3,       /* HIP runtime error */
  NBC_ERR_STATE = -4,     /* call order (e.g. forward before weights) */
  NBC_ERR_NOMEM = -5
};

/* Arithmetic of the convolution stack. */
enum {
  NBC_PREC_FP32 = 0,  /* f32 activations/weights, v_mfma_f32_32x32x2_f32: the parity mode */
  NBC_PREC_BF16 = 1,  /* bf16 activations/weights, f32 accumulate + f32 BN epilogue: throughput mode */
  NBC_PREC_F16X2 = 2  /* f32-grade on the 16-bit matrix pipe: every f32 value is kept as two f16 pieces, 4 bytes per element
                         like f32.
                         Activations: X0 = f16(x), X1 = f16((x - X0) * 2^11); x = X0 + X1 * 2^-11 to 2^-23 relative at
                         worst (rms 4e-8: the f32 level) for |x| >= 2^-12 = 2.4e-4; below that X1 is an f16 subnormal
                         and the error is ABSOLUTE, at most 2^-36 (1.5e-11); beyond +-65504 (f16's range) a value turns
                         into NaN, never into a silently wrong number (nbc_nonfinite_seen).  A tensor between a
                         BatchNorm and the next convolution is scale-free, so a checkpoint may hold activations of any
                         magnitude: nbc_pack_weights therefore estimates every tensor's size from its producing
                         BatchNorm (max over channels of |beta| + 3 |gamma| sqrt(var / (var + eps))) and stores a tensor whose estimate lies
                         outside [2^-5, 2^7] times the power of two that brings it to [2, 4) -- folded into the
                         producing launch's f32 (scale, shift) and, inverted, into the scale of every launch that reads
                         it (one power per residual stream); exact, ReLU and max-pool being positively homogeneous, and
                         0 for every tensor of an ordinary checkpoint.  The 2^-36 floor is then 2^-37 of the tensor's
                         expected size or less, whatever that size was in the checkpoint; what remains is a tensor
                         whose running statistics do not describe its data (an untrained BatchNorm behind weights
                         of another scale), where the floor can reach the values again silently and overflow raises the
                         flag.  nbc_read_activation returns the tensor as the network defines it (power taken off).
                         Weights: nbc_pack_weights multiplies every output channel's row by the power of two that puts
                         its largest |w| into [2^14, 2^15) -- exact -- splits it into P = f16(w 2^k), Q = f16(w 2^k - P)
                         (to 2^-23 of the row's largest weight; a weight below 2^-15 of it loses low bits, an absolute
                         error of 2^-39 of the largest) and folds 2^-k into the channel's f32 BatchNorm scale -- exact.
                         The magnitude of a checkpoint's weights therefore does not matter (a convolution in front of a
                         BatchNorm is scale-free): 1e-6 or 1e6 pack to the same pieces.  Limits, reported and not
                         silent (nbc_packed_weights_flags / nbc_weights_flags): a row whose largest |w| lies below
                         2^-51 or above 2^81 is normalised only as far as k in [-66, 80] reaches (NBC_PACK_ROW_CLAMPED),
                         and a (scale, shift) that leaves f32's normal range under its powers of two is no longer exact
                         (NBC_PACK_SCALE_RANGE); a caller that sees either runs NBC_PREC_FP32 (the folder driver does).
                         A product is P*X0 + Q*X0 + (P*2^-11)*X1, three EXACT f16 products on v_mfma_f32_16x16x32_f16,
                         summed in ONE f32 chain per 256 channels that joins a running f32 sum (two levels, like the f32
                         mode); the dropped Q*X1 is 2^-22 relative at worst.  Error against float64 at the level of
                         NBC_PREC_FP32 (profiles/r04_fp64_adjudication_*: 4.2-5.2e-6 on logits of range 2-3.5, the f32
                         MFMA 4.0-6.2e-6, the CPU reference 3.6-4.5e-6), same tolerances in the tests. */
};

/* What nbc_pack_weights had to give up (bits of nbc_packed_weights_flags / nbc_weights_flags; 0 = nothing): NBC_PREC_F16X2 only. */
enum {
  NBC_PACK_ROW_CLAMPED = 1,  /* a weight row beyond the reach of the row normalisation (largest |w| < 2^-51 or > 2^81): its
                                pieces keep fewer bits than f32 */
  NBC_PACK_SCALE_RANGE = 2   /* a BatchNorm scale / shift left f32's normal range under the powers of two folded into it */
};

/* Networks the library runs (models.py:46-57, 127-139).  Both share the dilated ResNet-50 trunk (318 backbone.* keys)
 * and differ in the head.  Every function without an architecture argument is architecture 0. */
enum {
  NBC_ARCH_FCN_RESNET50 = 0,       /* FCNHead(2048, 3): 3x3 conv 2048 -> 512, BN, ReLU, 1x1 conv 512 -> 3 (326 keys) */
  NBC_ARCH_DEEPLABV3_RESNET50 = 1, /* DeepLabHead(2048, 3) of torchvision 0.3: ASPP(2048, [12, 24, 36]) -- 1x1 conv, three
                                      3x3 convs at dilation 12 / 24 / 36 and global-average-pool + 1x1 conv, each 256
                                      channels with BN + ReLU, concatenated (1280) and projected 1280 -> 256 with BN + ReLU --,
                                      3x3 conv 256 -> 256, BN, ReLU, 1x1 conv 256 -> 3 (362 keys).  Its activations have the
                                      conv unit names; the concat is "classifier.0.concat" and the pooled vector (one pixel per
                                      image) "classifier.0.convs.4". */
  /* 2 is not an architecture.  EfficientNet-b{n}, n = 0..7 (models.py:60-110): the trunk of efficientnet_pytorch 0.7
     (EfficientNet.from_pretrained('efficientnet-b{n}').extract_features, keys "backbone.model.*", its unused ImageNet
     classifier "backbone.model._fc.*" included) under FCNHead(inplanes, 3) / DeepLabHead(inplanes, 3), inplanes = 1280 ..
     2560.  NBC_PREC_FP32 only, running statistics only.  Output stride 32 (nbc_arch_lowres_size), bicubic x32.  Every
     BatchNorm of the trunk has eps 1e-3 (the heads' 1e-5); every convolution pads TF-"same" for the variant's native image
     size (nbc_arch_conv_ext).  Activations are stored NHWC f32 with their channels zero-padded to a multiple of 64; keep
     mode and nbc_read_activation return the real channels.  Keep-mode names are the torch module names:
     "<block>._expand_conv" and "_conv_stem" hold the BatchNorm output BEFORE its swish (the depthwise kernel applies it as
     it reads them), "<block>._depthwise_conv" the swish output before the SE gate, "<block>._se_expand" the gate
     (sigmoid, one pixel per image), "<block>._project_conv" the block's output, "_conv_head" the trunk's output (after its
     swish). */
  NBC_ARCH_FCN_EFFICIENTNET_B0 = 16,        /* + n: fcn_efficientnet(n) */
  NBC_ARCH_DEEPLABV3_EFFICIENTNET_B0 = 24   /* + n: deeplabv3_efficientnet(n) */
};

/* BatchNorm statistics (nbc_set_bn_statistics). */
enum {
  NBC_BN_RUNNING = 0,   /* eval mode (the default): the running statistics, folded into each conv's epilogue at pack time */
  NBC_BN_PER_IMAGE = 1  /* every BatchNorm normalises each image by that image's own per-channel mean and BIASED variance
                           over its H x W pixels (eps 1e-5) and applies the checkpoint's gamma and beta: F.batch_norm(training=
                           True) on a batch of one, what the shipped tool's forward does (models.py:212-250 never calls .eval()
                           and feeds one image at a time).  Running statistics are read by nothing and updated by nothing;
                           Dropout stays the identity (its expectation: live Dropout noise is what remains different from the
                           shipped tool; nbc_dropout_draws samples it).  NBC_ARCH_FCN_RESNET50 in NBC_PREC_FP32 or
                           NBC_PREC_F16X2 (see nbc_set_bn_statistics for the arithmetic on pieces). */
};

/* Bits of the context's sticky word (nbc_nonfinite_seen, nbc_nonfinite_peek_async). */
enum {
  NBC_NONFINITE_LOGIT = 1,     /* classifier.4 produced a logit that is NaN or infinite */
  NBC_NONFINITE_BN_RANGE = 2   /* NBC_BN_PER_IMAGE in NBC_PREC_F16X2: a channel's stored raw convolution output lies outside
                                  the range the pieces hold to 2^-23 (its rms over the image is not finite, above 2^12, or
                                  positive and below 2^-10): the running statistics misjudge the channel.  Raised by nothing
                                  outside that mode */
};

/* Layout of the image handed to nbc_forward. */
enum {
  NBC_IN_F32_NCHW = 0,  /* float32 [N,3,H,W], already normalised: exactly `batch[0]` of models.py:269 */
  NBC_IN_U8_NHWC = 1    /* uint8 [N,H,W,3] RGB as decoded by pil_loader (dataset.py:82-90); the
                           library applies ToTensor (/255) and Normalize((x-mean)/std) in f32 */
};

enum {
  NBC_LABEL_U8 = 0,   /* uint8 [N,H,W]  */
  NBC_LABEL_I64 = 1   /* int64 [N,H,W]: dtype of torch.argmax at models.py:270 */
};

/* One entry of a state_dict (models.py:222).  `data` is HOST memory, C-contiguous. */
typedef struct {
  const char* name;   /* e.g. "backbone.layer1.0.conv1.weight" */
  const void* data;
  int64_t shape[4];
  int32_t ndim;
  int32_t dtype;      /* 0 = float32, 1 = int64 (num_batches_tracked: checked for presence, unused) */
} nbc_tensor;

/* One convolution unit of the network, in execution order (introspection / tests). */
typedef struct {
  char name[64];      /* state_dict prefix of the conv */
  char bn[64];        /* state_dict prefix of its BatchNorm, "" for classifier.4 */
  int32_t cin, cout, k, stride, pad, dil;
  int32_t relu, bias, residual;
} nbc_conv_desc;

/* What nbc_conv_desc does not say about a unit (EfficientNet; for the ResNet-50 networks: kind 0, pad_after = pad, cin_pad /
 * cout_pad = cin / cout, block -1, eps 1e-5). */
typedef struct {
  int32_t kind;        /* 0 convolution, 1 depthwise (groups = channels; its weight is [C,1,k,k]), 2 SE reduce, 3 SE expand */
  int32_t pad_before;  /* top / left pad (= nbc_conv_desc.pad) */
  int32_t pad_after;   /* bottom / right pad */
  int32_t act;         /* after the BatchNorm (or the bias): 0 none, 1 ReLU, 2 swish (SE expand: its sigmoid is the gate) */
  int32_t cin_pad, cout_pad;   /* channels of the stored input / output tensors */
  int32_t block;       /* MBConv block index, -1 outside the blocks */
  int32_t in_swish;    /* depthwise: applies the swish its stored input was written without */
  float eps;           /* BatchNorm eps */
} nbc_conv_ext;

/* Per-op record of the last profiled forwards (nbc_set_profiling). */
typedef struct {
  char name[64];      /* conv unit name, or "ingest" / "maxpool" / "upsample_argmax" */
  char kernel[32];    /* kernel family: "conv_dma", "head1x1", ... */
  float ms;           /* mean HIP-event time of the op per forward on the forward's stream (all its launches together) */
  int32_t calls;      /* forwards averaged over */
  double flops;       /* algorithmic: 2*MAC of the convolution (0 for non-conv ops) */
  double bytes;       /* algorithmic: input read once + weights once + output once (+ identity) */
  int32_t kh, kw;     /* kernel extent (0 for non-conv) */
  int32_t cout;       /* output channels (conv ops): Co % 128 == 0 selects the wide-tile kernel */
  int32_t launches;   /* launches of the op per forward (1) */
} nbc_op_record;

const char* nbc_last_error(void);
const char* nbc_version(void);

/* ---- topology introspection (no GPU needed) ------------------------------------------- */
int nbc_num_convs(void);
int nbc_conv_info(int index, nbc_conv_desc* out);
int nbc_num_state_keys(void);                               /* 326 */
int nbc_state_key(int index, const char** name, int64_t shape[4], int32_t* ndim, int32_t* dtype);
/* The same for architecture `arch` (NBC_ARCH_*); NBC_ERR_INVALID for an unknown one. */
int nbc_arch_num_convs(int arch);
int nbc_arch_conv_info(int arch, int index, nbc_conv_desc* out);
int nbc_arch_num_state_keys(int arch);                      /* 326 / 362 */
int nbc_arch_state_key(int arch, int index, const char** name, int64_t shape[4], int32_t* ndim, int32_t* dtype);
/* The architecture whose key set (names, shapes, dtypes) the state_dict matches exactly, or NBC_ERR_KEYS with the message
 * strict loading into architecture 0 gives. */
int nbc_arch_of_state_dict(const nbc_tensor* tensors, int n);
/* Low-resolution logits size for an HxW input (three stride-2 stages). */
int nbc_lowres_size(int H, int W, int* h, int* w);
/* The same for architecture `arch`: the ResNet-50 networks as nbc_lowres_size; EfficientNet through its five stride-2
 * convolutions with their fixed pads, floor((H + before + after - k) / 2) + 1 each (not always ceil(H / 2)). */
int nbc_arch_lowres_size(int arch, int H, int W, int* h, int* w);
int nbc_arch_conv_ext(int arch, int index, nbc_conv_ext* out);

/* ---- weights (host side; no GPU needed) ------------------------------------------------ */
/* The two f16 pieces NBC_PREC_F16X2 keeps of each of n f32 ACTIVATION values (host arithmetic, bit patterns of IEEE
 * binary16): h0 = f16(x) rounded to nearest even, h1 = f16((x - h0) * 2^11).  What the kernels do to every activation
 * (nbc_pack_weights uses the same rounding on the normalised weight rows, with an unscaled low piece); exported so that
 * the conversion can be checked against another implementation of binary16 rounding. */
int nbc_split_f16x2(const float* x, size_t n, uint16_t* h0, uint16_t* h1);

/* Size in bytes of the packed weight blob for a precision (same on every rank). */
size_t nbc_packed_weights_bytes(int precision);
/* Strict key/shape check like nn.Module.load_state_dict (models.py:222): NBC_ERR_KEYS with a
 * message listing missing / unexpected / mis-shaped entries.  Folds each BatchNorm into an f32
 * (scale, shift) pair, reorders conv weights OIHW -> [O][kh][kw][I] (K-major panels, zero padded
 * to whole 128-byte K-steps), converts to the precision's element type, writes `blob`. */
int nbc_pack_weights(const nbc_tensor* tensors, int n, int precision, void* blob, size_t blob_bytes);
/* NBC_PACK_* bits of a packed blob in HOST memory (>= 0), or a negative error.  The bits ride in the blob's trailer, so
 * a rank that received the blob by broadcast reads the same ones (nbc_weights_flags on its context). */
int nbc_packed_weights_flags(const void* blob, size_t blob_bytes, int precision);
/* The same three for architecture `arch`.  The blob's trailer records the architecture in a word every blob of architecture
 * 0 holds as 0, so an FCN blob of nbc_pack_weights_arch(..., 0, ...) is byte for byte the one nbc_pack_weights wrote before
 * the word had this meaning.  f16x2: the five ASPP branches write one tensor, the concat, and share one power of two (from
 * the largest of their five BatchNorm estimates); the pooling branch keeps its weights in f32 like classifier.4. */
size_t nbc_arch_packed_weights_bytes(int precision, int arch);   /* 0 for an EfficientNet network outside NBC_PREC_FP32 */
int nbc_pack_weights_arch(const nbc_tensor* tensors, int n, int precision, int arch, void* blob, size_t blob_bytes);
int nbc_packed_weights_flags_arch(const void* blob, size_t blob_bytes, int precision, int arch);
/* The architecture recorded in a packed blob in HOST memory of exactly nbc_arch_packed_weights_bytes(precision, arch)
 * bytes, or NBC_ERR_INVALID. */
int nbc_packed_weights_arch(const void* blob, size_t blob_bytes, int precision);

/* The per-image BatchNorm affine array (NBC_BN_PER_IMAGE): gamma then beta of every conv unit that has a BatchNorm, in
 * conv-unit order (nbc_arch_conv_info), as f32.  It travels beside the blob, not in it (a blob's bytes do not depend on the
 * BatchNorm mode).  nbc_arch_bn_affine_floats: its length (2 x the summed cout of those units), 0 for an unknown
 * architecture.  nbc_pack_bn_affine: the strict key / shape check of nbc_pack_weights (same errors and messages), then the
 * array into `out` (at least that many floats). */
size_t nbc_arch_bn_affine_floats(int arch);
int nbc_pack_bn_affine(const nbc_tensor* tensors, int n, int arch, float* out, size_t count);

/* The second side array of NBC_BN_PER_IMAGE, read in NBC_PREC_F16X2 only: per conv unit that has a BatchNorm, in conv-unit
 * order, cout values 2^(r_o - k_o - a_in) and then cout values 2^-r_o, as f32 (the layout and length of the affine array).
 * k_o is the weight row's power of two and a_in the power of the tensor the unit reads, the very ones nbc_pack_weights folds
 * into the blob; r_o is the power of two that brings |running_mean_o| + 3 sqrt(max(running_var_o, 0)) into [2, 4) (0 for an
 * estimate that is 0 or not finite, clamped to [-100, 100]).  The raw convolution runs with the first as its scale table, so
 * what it stores is 2^r_o conv_o, where the pieces hold it to 2^-23; the statistics kernel takes 2^r_o off with the second.
 * nbc_arch_bn_raw_floats: the length, 0 for an unknown architecture or one without f16x2.  nbc_pack_bn_raw: the strict key /
 * shape check of nbc_pack_weights (same errors and messages), then the array into `out`; returns NBC_PACK_* bits (>= 0):
 * NBC_PACK_SCALE_RANGE when a power leaves f32's normal range, NBC_PACK_ROW_CLAMPED as nbc_pack_weights raises it. */
size_t nbc_arch_bn_raw_floats(int arch);
int nbc_pack_bn_raw(const nbc_tensor* tensors, int n, int arch, float* out, size_t count);

/* ---- context --------------------------------------------------------------------------- */
int nbc_create(nbc_ctx** out, int hip_device);
int nbc_destroy(nbc_ctx* ctx);
/* Attach a packed blob that already lives in DEVICE memory and stays owned by the caller
 * (e.g. a torch tensor that was the target of an RCCL broadcast).  Must outlive the context
 * or the next attach. */
int nbc_attach_weights(nbc_ctx* ctx, const void* dev_blob, size_t bytes, int precision);
/* The same for a blob of architecture `arch`: a blob whose trailer names another architecture is refused
 * (NBC_ERR_INVALID).  nbc_forward, nbc_reserve, nbc_autotune, the plan tiles, the profiling records, keep mode and the
 * calibration guard then run that architecture. */
int nbc_attach_weights_arch(nbc_ctx* ctx, const void* dev_blob, size_t bytes, int precision, int arch);
/* Convenience: pack on the host, allocate device memory owned by the context, upload; the BatchNorm affine array
 * (nbc_pack_bn_affine) of the same tensors is uploaded and attached as well, and in NBC_PREC_F16X2 the raw-convolution array
 * (nbc_pack_bn_raw), whose NBC_PACK_* bits join those nbc_weights_flags reports. */
int nbc_load_weights(nbc_ctx* ctx, const nbc_tensor* tensors, int n, int precision);
int nbc_load_weights_arch(nbc_ctx* ctx, const nbc_tensor* tensors, int n, int precision, int arch);
/* NBC_PACK_* bits of the attached blob (read from its trailer when it was attached: a 1-KiB device-to-host copy), >= 0,
 * or a negative error (no weights attached). */
int nbc_weights_flags(nbc_ctx* ctx);
/* The power of two a the output tensor of conv unit `name` (or "backbone.maxpool") is STORED with in the attached blob's
 * precision: stored = 2^a x the tensor the network defines (0 outside NBC_PREC_F16X2 and for every tensor of an ordinary
 * checkpoint; see NBC_PREC_F16X2).  Introspection / tests; NBC_ERR_INVALID for an unknown name. */
int nbc_activation_exponent(nbc_ctx* ctx, const char* name, int32_t* exponent);
/* Multi-GPU start-up (the reference has no counterpart: it is single-device,
 * predict.py:66-70): RCCL broadcast of the packed weight blob from rank `root` of `rccl_comm` (an
 * ncclComm_t of the host process, one rank per GPU) on `hip_stream`.  The root must have weights of
 * `precision` attached (nbc_load_weights / nbc_attach_weights: it alone read the checkpoint,
 * predict.py:57); every other rank allocates a blob the context owns, receives into it and attaches
 * it.  The RCCL entry points are looked up in the host process at call time (the library links
 * libamdhip64 only); NBC_ERR_STATE when the process holds no RCCL.  The blob is valid once the stream
 * has been synchronised.  NBC_ARCH_FCN_RESNET50 only: NBC_ERR_STATE on a context that holds another architecture (the
 * folder drivers broadcast the blob through torch.distributed). */
int nbc_bcast_weights(nbc_ctx* ctx, void* rccl_comm, int root, int precision, void* hip_stream);
/* Attach a per-image BatchNorm affine array (nbc_pack_bn_affine) that lives in DEVICE memory and stays owned by the caller
 * (must outlive the context or the next attach); `count` floats, nbc_arch_bn_affine_floats of the attached architecture.
 * nbc_bcast_weights does not carry it: a multi-rank caller broadcasts it itself and attaches it on each rank. */
int nbc_attach_bn_affine(nbc_ctx* ctx, const float* dev_affine, size_t count);
/* The same for the raw-convolution array (nbc_pack_bn_raw), `count` = nbc_arch_bn_raw_floats of the attached architecture. */
int nbc_attach_bn_raw(nbc_ctx* ctx, const float* dev_raw, size_t count);
/* NBC_BN_RUNNING (default) or NBC_BN_PER_IMAGE.  NBC_ERR_STATE for NBC_BN_PER_IMAGE unless the attached weights are
 * NBC_PREC_FP32 or NBC_PREC_F16X2 of NBC_ARCH_FCN_RESNET50 (bf16 rounds the raw pre-BatchNorm values; DeepLabV3's
 * pooling-branch BatchNorm sees one value per channel, which batch statistics refuse).
 * NBC_PREC_F16X2, unit u, output channel o: the raw launch's table is scale[o] = 2^(r_o - k_o - a_in), shift 0 (nbc_pack_bn_raw),
 * exact in fma(acc, 2^e, 0), so the buffer holds 2^r_o conv_o as pieces.  "<bn>.stats" sums the joined stored values and their
 * squares in f64 and finishes mean = (S / hw) 2^-r_o, var = max(SS / hw - (S / hw)^2, 0) 2^-2 r_o (exact scalings),
 * sc = gamma / sqrt(var + 1e-5), table scale = f32(sc) 2^(a_out - r_o), shift = f32(beta - mean sc) 2^a_out, a_out the power
 * the blob records for the unit's output (nbc_activation_exponent); it raises NBC_NONFINITE_BN_RANGE from the channel's stored
 * rms sqrt(SS / hw).  "<bn>.apply" joins, fma(x, scale, shift), adds the joined identity (stored with the same a_out: a
 * residual stream is one tensor), applies the ReLU (NaN-propagating) and splits again, in place.  Every reader of the
 * tensor is the one of NBC_BN_RUNNING.
 * The mode is part of the plan key, like the precision.  In NBC_BN_PER_IMAGE every BatchNorm'd convolution runs raw on the
 * same conv kernels and tiles (nbc_autotune, nbc_set_plan_tiles: the same list), followed by two plan ops named after the
 * BatchNorm: "<bn>.stats" (kernel "bn_stats": per-image sums over fixed pixel slices, f64, no atomics, so an image's bits do
 * not depend on its batch) and "<bn>.apply" (kernel "bn_apply": in place, with the identity and ReLU of the unit).  Keep
 * mode returns each unit's post-BatchNorm (post-ReLU) tensor under the unit's name.  nbc_forward / nbc_reserve then return
 * NBC_ERR_STATE without an affine array (in NBC_PREC_F16X2: or without a raw-convolution array) attached, and NBC_ERR_INVALID ("Expected more than 1 value per channel when
 * training") for an image whose low-resolution map is 1 x 1 (e.g. 8 x 8), which batch statistics cannot normalise. */
int nbc_set_bn_statistics(nbc_ctx* ctx, int mode);
/* mean/std used for NBC_IN_U8_NHWC input; defaults are models.py:208-209. */
int nbc_set_normalization(nbc_ctx* ctx, const float mean[3], const float std[3]);
/* Pre-size the workspace for an (N,H,W) so that the first nbc_forward does not allocate.  Buffers only grow, and a
 * growth frees and reallocates (which synchronises the device): a caller that will see many shapes reserves the
 * largest one first, as the folder driver does. */
int nbc_reserve(nbc_ctx* ctx, int N, int H, int W);
/* The launch plan nbc_reserve would build for such a context, as text (host only, no context, no device call), one line per
 * op in launch order and then one per activation buffer:
 *   op <name> <kernel> [in=B] [out=B] [res=B] [ws=B] [gate=B] [cat=B x 5] [tile=T] launches=L [ds=<name>]
 *   buf <index> <bytes> [identity]
 * B: buffer indices (a field the op does not use is left out); ds: on the conv3 of a (downsample.0, conv3) pair, the
 * downsample op in front of it (nbc_set_fuse_downsample); identity: the buffer outside the recycled pool that the downsamples
 * of the pairs write when they run in a launch of their own.  Returns the bytes the text needs with its terminating 0; at
 * most `capacity` are written (text may be null).  NBC_ERR_INVALID for what nbc_attach_weights_arch, nbc_set_bn_statistics or
 * nbc_reserve refuse, with nbc_reserve's message for an image the network cannot run on. */
int nbc_describe_plan(int arch, int precision, int N, int H, int W, int keep, int bn_mode, char* text, size_t capacity);

/* ---- the hot path ------------------------------------------------------------------------
 * x_dev                 device pointer, layout per x_dtype
 * logits_lowres_dev     nullable, float32 [N,3,h,w] (output of classifier.4, models.py:121)
 * logits_full_dev       nullable, float32 [N,3,H,W] (what self.model(x) returns, models.py:269)
 * labels_dev            nullable, [N,H,W] per labels_dtype (models.py:270; ties -> lowest index,
 *                       NaN counts as the maximum, like torch.argmax)
 * counts_dev            nullable, int64 [N,3]: pixels per class after the optional remap
 * exclude_nodes         non-zero: label 2 -> 1 after the argmax (models.py:273-276)
 * hip_stream            hipStream_t (NULL = default stream)
 */
int nbc_forward(nbc_ctx* ctx, const void* x_dev, int x_dtype, int N, int H, int W,
                float* logits_lowres_dev, float* logits_full_dev,
                void* labels_dev, int labels_dtype, int64_t* counts_dev,
                int exclude_nodes, void* hip_stream);

/* The tail of the path on its own: bicubic upsample (models.py:38-41) of caller-supplied
 * low-resolution logits float32 [N,3,h,w] to HxW + argmax (models.py:270) + remap + counts.
 * Same output arguments as nbc_forward.  Used to test tie / NaN behaviour with crafted logits. */
int nbc_upsample_argmax(nbc_ctx* ctx, const float* logits_lowres_dev, int N, int h, int w, int H, int W,
                        float* logits_full_dev, void* labels_dev, int labels_dtype,
                        int64_t* counts_dev, int exclude_nodes, void* hip_stream);

/* remove_small_zones of utils.py:135-148 (called at models.py:271, between the argmax and the
 * statistics) on device labels, in place: with m = (labels == 0), 8-connected components of ~m smaller
 * than min_pixels join m (skimage remove_small_holes, connectivity=2), then 8-connected components of
 * the filled m smaller than min_pixels leave it (remove_small_objects); pixels that left m and were
 * class 0 become class 1, pixels that joined it become class 0.  The reference uses 150 pixels.
 * labels_dev: uint8 or int64 [N,H,W] (labels_dtype NBC_LABEL_U8 / NBC_LABEL_I64).  exclude_nodes
 * applies the 2 -> 1 remap of models.py:273-276 afterwards; counts_dev (nullable, int64 [N,3]) receives
 * the pixels per class of the result (the counting of models.py:324-331).  N <= 65535. */
int nbc_remove_small_zones(nbc_ctx* ctx, void* labels_dev, int labels_dtype, int N, int H, int W, int min_pixels,
                           int exclude_nodes, int64_t* counts_dev, void* hip_stream);

/* remove_small_zones on batches, as the reference's PixelWiseF1 runs it (utils.py:211-214 hands the [B,H,W] argmax of a batch
 * to the same function): skimage's connectivity=2 on a 3-D array is generate_binary_structure(3, 2), so besides its 8
 * neighbours inside the image a pixel (b, y, x) touches (b +- 1, y', x') with |y - y'| + |x - x'| <= 1, and min_pixels counts
 * the pixels of the linked component over all its images.  Images n = 0 .. N-1 form consecutive groups of G
 * (the last one may be shorter); nothing links across a group boundary.  In place; no 2 -> 1 remap.
 * counts_dev (nullable, int64 [N,3]) receives the pixels per class of every image of the result.  With G = 1 the labels and
 * counts are those of nbc_remove_small_zones with exclude_nodes = 0, byte for byte.  Sizes are exact integers: a group's
 * bytes are the same alone, among other groups and on any stream.  The workspace is the context's, 9 bytes per pixel.
 * NBC_ERR_INVALID, before any HIP call: what nbc_remove_small_zones refuses, H > 65535, H * W >= 2^31, G < 1, G > 64,
 * g * H * W >= 2^31 for the g = min(G, N) images of a group (a parent index addresses the group's volume). */
int nbc_remove_small_zones_groups(nbc_ctx* ctx, void* labels_dev, int labels_dtype, int N, int H, int W, int G,
                                  int min_pixels, int64_t* counts_dev, void* hip_stream);

/* Per-image 3x3 confusion counts of predicted labels against a grey target mask: the pixel counting behind the evaluation
 * loop's lovasz `iou` (lovasz_losses.py:54-73) and `PixelWiseF1` (utils.py:201-235), called at __main__.py:331-332;
 * the ratios are host arithmetic (neuralbarkcalculator_amd/metrics.py).  No context: csrc/confusion.hip.
 * labels_dev  uint8 or int64 [N,H,W] (NBC_LABEL_U8 / NBC_LABEL_I64), values in {0,1,2}; other values are counted nowhere
 * target_dev  uint8 [N,H,W], grey levels as PIL 'L' gives them; class = round(2 * float32(v) / 255)
 *             (dataset.py:189-197): 0..63 -> 0, 64..191 -> 1, 192..255 -> 2
 * conf_dev    int64 [N,3,3], conf[n][t][p] = pixels with target class t and predicted class p; overwritten
 * Runs on hip_stream (the caller's current device); no synchronisation.  N <= 65535, H * W < 2^31. */
int nbc_confusion(const void* labels_dev, int labels_dtype, const uint8_t* target_dev,
                  int N, int H, int W, int64_t* conf_dev, void* hip_stream);

/* Exact per-image, per-channel integer moments of uint8 RGB frames: what compute_mean_std (utils.py:23-39: ToTensor, then
 * .mean(2) and .std(2) of every image's [3, H*W] view) needs from the pixels.  With S1 and S2 the two sums of a channel and
 * P = H * W, the image's mean is S1 / (255 P) and its unbiased standard deviation sqrt((P S2 - S1^2) / (P (P - 1) 65025)):
 * host arithmetic (neuralbarkcalculator_amd/stats.py).  No context: csrc/dataset_stats.hip.
 * x_dev        uint8 [N,H,W,3], the layout of NBC_IN_U8_NHWC; any alignment
 * moments_dev  uint64 [N,3,2]: moments[n][c] = { sum of v, sum of v*v } over the H*W pixels of channel c; overwritten
 * Integer sums: an image's six numbers are the same alone, in any batch and on any stream.  Runs on hip_stream (the caller's
 * current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a null pointer, N < 1 or N > 65535, H or
 * W < 1, H * W >= 2^31.  Every sum stays below 2^47. */
int nbc_image_moments(const uint8_t* x_dev, int N, int H, int W, uint64_t* moments_dev, void* hip_stream);

/* Per-image class counts of grey target masks: what compute_pos_weight (utils.py:51-69) counts with (targets == y).sum(), and
 * what get_splits' sample_weight (utils.py:94-95: the pixels that are not class 0) is made of.  No context:
 * csrc/dataset_stats.hip.
 * target_dev  uint8 [N,H,W]; class = round(2 * float32(v) / 255) exactly as nbc_confusion derives it
 * counts_dev  int64 [N,4]: pixels of class 0, 1, 2, and the pixels whose grey level is none of 0, 127, 255 (they are counted
 *             in their class as well; the fourth cell only reports them); overwritten
 * Runs on hip_stream; no synchronisation.  Limits and errors as nbc_image_moments. */
int nbc_target_counts(const uint8_t* target_dev, int N, int H, int W, int64_t* counts_dev, void* hip_stream);

/* Per-image Lovasz-Softmax loss terms: `LovaszSoftmax()(logits, target)` (lovasz_losses.py:162-223: softmax over the classes,
 * then lovasz_softmax_flat with classes='present', ignore=None) of each image as a batch of one -- the training objective of
 * __main__.py:236-239, which exp.test / test_model_on_checkpoint print as test_loss (__main__.py:179-197).  No context:
 * csrc/lovasz.hip.  Per image n and class c, with fg = (target class == c), p_c = softmax(logits)_c in f32 and
 * e = |fg - p_c| sorted descending (fg carried along), G = sum fg, I_i = G - sum_{k<=i} fg_(k), U_i = G + sum_{k<=i} (1 - fg_(k)),
 * J_i = 1 - I_i / U_i (f64), J_{-1} = 0:  terms[n][c] = sum_i e_(i) (J_i - J_{i-1})  (lovasz_grad, lovasz_losses.py:19-31),
 * summed in f64 in a fixed order.  The loss of an image is the mean of the terms of its present classes (fg_counts > 0) in
 * class order, a host division (neuralbarkcalculator_amd/metrics.py: lovasz_loss).
 * logits_full_dev  float32 [N,3,H,W], what nbc_forward writes to logits_full_dev (after the bicubic upsample)
 * target_dev       uint8 [N,H,W] grey levels; class = round(2 * float32(v) / 255) as nbc_confusion derives it
 * workspace_dev    at least nbc_lovasz_workspace_bytes(N, H, W) bytes of device memory, 256-byte aligned; contents scratch
 * terms_dev        float64 [N,3]: the term of each class; 0 for an absent class; NaN for every present class of an image
 *                  in which some pixel's softmax is not finite (a NaN or +inf logit, or all three -inf), as torch gives
 * fg_counts_dev    int64 [N,3]: G, the target pixels of each class (0 tells the caller the class is absent)
 * The sort is exact (keys-only LSD radix sort of the f32 errors, no binning) and every sum has a fixed order: an image's
 * terms are bit-identical alone, in any batch and on any stream.  Runs on hip_stream; no synchronisation.
 * NBC_ERR_INVALID: a null pointer, N < 1 or N > 65535, H or W < 1, H * W >= 2^31, or a workspace too small or misaligned.
 * With P = H * W, S = 3 N, T = ceil(P / 8192) and A(x) = x rounded up to a multiple of 256, the workspace is
 *   2 A(4 S P) + A(1024 S T) + A(1024 S) + A(4 S T) + A(8 S T) + A(4 N) bytes
 * (two key arrays, per-tile digit histograms, digit bases, per-tile foreground counts, per-tile f64 partials, non-finite
 * flags); nbc_lovasz_workspace_bytes returns 0 for a shape nbc_lovasz_softmax refuses. */
size_t nbc_lovasz_workspace_bytes(int N, int H, int W);
int nbc_lovasz_softmax(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W,
                       void* workspace_dev, size_t workspace_bytes, double* terms_dev, int64_t* fg_counts_dev,
                       void* hip_stream);

/* The Lovasz-Softmax terms of batches: `LovaszSoftmax()(logits, target)` on a batch runs with per_image=False
 * (lovasz_losses.py:169-191), flattens the batch and sorts the errors of all its images together, per class -- val_loss and
 * test_loss of the training log are that, per batch of 8.  Images n = 0 .. N-1 form consecutive groups of G
 * (the last one may be shorter); there are NG = ceil(N / G) groups.  terms[group][c] and counts[group][c] are what
 * nbc_lovasz_softmax defines for an image, the segment being the g * H * W pixels of the group's g images in image order:
 * the pooled loss of a group is the per-image loss of its images stacked along the height, so a group's terms are bit for bit
 * those of nbc_lovasz_softmax on the one image [1,3,g*H,W], and with G = 1 the call is nbc_lovasz_softmax.  No transposed
 * copy of the logits is made: only the kernel that writes the keys knows about images.
 * terms_dev   float64 [NG,3]; 0 for an absent class; NaN for every present class of a group in which some pixel's softmax is
 *             not finite -- of that group only
 * counts_dev  int64 [NG,3]: the target pixels of each class in the group (a class present in one image is present for the group)
 * A group's terms are added in the same fixed order whatever else is in the call and on any stream.  Runs on hip_stream; no
 * synchronisation.  NBC_ERR_INVALID, before any HIP call: what nbc_lovasz_softmax refuses, G < 1, G > 64, g * H * W >= 2^31
 * for g = min(G, N).  With P = H * W, S = 3 NG, T = ceil(g P / 8192), the workspace is
 *   2 A(12 N P) + A(1024 S T) + A(1024 S) + A(4 S T) + A(8 S T) + A(4 NG) bytes;
 * nbc_lovasz_groups_workspace_bytes returns 0 for what nbc_lovasz_softmax_groups refuses. */
size_t nbc_lovasz_groups_workspace_bytes(int N, int H, int W, int G);
int nbc_lovasz_softmax_groups(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int G,
                              void* workspace_dev, size_t workspace_bytes, double* terms_dev, int64_t* counts_dev,
                              void* hip_stream);

/* Per-image pixel-wise cross-entropy sums: what CustomWeightedCrossEntropy (utils.py:151-165: F.cross_entropy with
 * reduction='none', times the class weight at max(argmax, target), mean over the pixels), the plain cross-entropy (xloss,
 * lovasz_losses.py:246-251) and MixedLoss (utils.py:185-192) need from the pixels of each image as a batch of one, with the
 * weights (compute_pos_weight, utils.py:51-69; get_pos_weight, utils.py:72-73) left to the host.  No context:
 * csrc/pixel_ce.hip.  Per image n and pixel: t = target class, p = argmax of the three logits (first maximum wins, a NaN
 * counts as the maximum: torch.argmax and nbc_forward's labels), ce = logsumexp(x) - x[t], evaluated in f64 from the f32
 * logits as log(sum_c exp(x_c - m)) - (x_t - m) with m = max_c x_c:
 *   sums[n][t][p] = sum of ce over the pixels of cell (t, p), counts[n][t][p] = their number.
 * Then cross_entropy = sum(sums) / P, CustomWeightedCrossEntropy(w) = sum(w[max(t, p)] sums[t][p]) / P, and MixedLoss is that
 * / 4 plus the Lovasz-Softmax loss: host arithmetic (neuralbarkcalculator_amd/metrics.py).
 * logits_full_dev  float32 [N,3,H,W], what nbc_forward writes to logits_full_dev; any 4-byte alignment (an image whose three
 *                  planes start on 16-byte boundaries, i.e. H * W a multiple of 4 in an aligned buffer, is read by 16-byte loads)
 * target_dev       uint8 [N,H,W] grey levels; class = round(2 * float32(v) / 255) as nbc_confusion derives it
 * workspace_dev    at least nbc_pixel_ce_workspace_bytes(N, H, W) bytes of device memory, 256-byte aligned; contents scratch
 * sums_dev         float64 [N,3,3]; overwritten.  A pixel whose entropy is not finite reaches its own cell only: NaN for a
 *                  NaN or +inf logit or three -inf, +inf for -inf at the target class alone, as F.cross_entropy gives
 * counts_dev       int64 [N,3,3]; overwritten.  Equal to nbc_confusion's conf of the labels of the same forward
 * Every float sum has a fixed order that depends on H * W alone (pixels of a lane in order, lanes, waves, per-tile partials
 * in the workspace, tiles by a second launch) and there are no atomics: an image's 18 numbers are bit-identical alone,
 * anywhere in a batch and on any stream.  Runs on hip_stream (the caller's current device); no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null pointer, N < 1 or N > 65535, H or W < 1, H * W >= 2^31, or a workspace too
 * small or misaligned.  With P = H * W, T = ceil(P / 4096) and A(x) = x rounded up to a multiple of 256, the workspace is
 *   A(72 N T) + A(36 N T) bytes
 * (an f64 and a u32 partial per image, cell and tile); nbc_pixel_ce_workspace_bytes returns 0 for a shape
 * nbc_pixel_cross_entropy refuses. */
size_t nbc_pixel_ce_workspace_bytes(int N, int H, int W);
int nbc_pixel_cross_entropy(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W,
                            void* workspace_dev, size_t workspace_bytes, double* sums_dev, int64_t* counts_dev,
                            void* hip_stream);

/* Per-image census of the softmax confidence: what a reliability table, the expected calibration error, the Brier score,
 * one-vs-rest precision / recall curves of each class probability and the soft Jaccard need from the pixels -- the soft
 * Jaccard being the quantity the reference's JaccardLoss (utils.py:168-182) is named after, which its code does not compute
 * on the [B,H,W] targets it is given -- and the confidence plane of the plain forward.  The softmax
 * is the one of lovasz_losses.py:162-167 / F.cross_entropy; the class weights that pushed it off the class priors are
 * get_pos_weight (utils.py:72-73).  No context: csrc/softmax_census.hip.  The definition is integer from the quantisation
 * on, so nothing in the result depends on an order of addition.  Per pixel of image n:
 *   a pixel with a NaN or infinite logit adds 1 to `nonfinite`, takes part in nothing else and gets confidence byte 0;
 *   otherwise, in f64 from the f32 logits: m = max_c x_c, e_c = exp(x_c - m), s = (e_0 + e_1) + e_2, p_c = e_c / s,
 *   q_c = min(65535, floor(p_c * 65536));  k = argmax of the three logits (first maximum wins: nbc_forward's labels);
 *   t = the target class, hit = (k == t); without a target t = 0 and hit = 1;  the confidence byte is q_k >> 8.
 * The row of an image, NBC_CENSUS_WORDS unsigned 64-bit words:
 *   H[t][c][b]  at NBC_CENSUS_H + (t * 3 + c) * 256 + b:  pixels of target class t with q_c >> 8 == b
 *   R[hit][b]   at NBC_CENSUS_R + hit * 256 + b:          pixels with q_k >> 8 == b (the reliability counts)
 *   RS[hit][b]  at NBC_CENSUS_RS + hit * 256 + b:         the sum of q_k over those pixels (the exact confidence sums)
 *   M[t][c]     at NBC_CENSUS_M + t * 3 + c:              the sum of q_c over the pixels of target class t (the soft
 *                                                         confusion, in expected pixels x 65536)
 *   B[t]        at NBC_CENSUS_B + t:                      the sum of sum_c (q_c - 65536 [c == t])^2 (the Brier numerators)
 *   nonfinite   at NBC_CENSUS_NONFINITE
 * A pixel adds less than 2^33 to B[t] (its q sum to at most 65536, so (65536 - q_t)^2 and the two other squares together
 * stay below 2 * 65536^2), so with H * W < 2^31 every word stays below 2^64: u64 holds every shape the call admits.
 * logits_full_dev  float32 [N,3,H,W], what nbc_forward writes to logits_full_dev; any 4-byte alignment (16-byte loads where
 *                  an image's planes start on 16-byte boundaries, as nbc_pixel_cross_entropy reads them)
 * target_dev       nullable, uint8 [N,H,W] grey levels; class = round(2 * float32(v) / 255) as nbc_confusion derives it
 * workspace_dev    at least nbc_softmax_census_workspace_bytes(N, H, W) bytes of device memory, 256-byte aligned; scratch
 * rows_dev         uint64 [N][NBC_CENSUS_WORDS]; overwritten
 * confidence_dev   nullable, uint8 [N,H,W]; overwritten
 * Integer sums only (LDS integer atomics inside a tile, per-tile partials in the workspace, tiles added by a second launch;
 * no float atomics, no memset): an image's row and confidence plane are bit-identical alone, anywhere in a batch and on any
 * stream.  Runs on hip_stream (the caller's current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a
 * null logits, workspace or rows pointer, N < 1 or N > 65535, H or W < 1, H * W >= 2^31, or a workspace too small or
 * misaligned.  With P = H * W, T = ceil(P / 4096) and A(x) = x rounded up to a multiple of 256, the workspace is
 *   A(5632 N T) + A(2088 N T) + A(24 N T) bytes
 * (per image and tile: 2816 16-bit counts, 522 32-bit sums, 3 64-bit Brier sums); nbc_softmax_census_workspace_bytes
 * returns 0 for a shape nbc_softmax_census refuses. */
#define NBC_CENSUS_BINS 256
#define NBC_CENSUS_H 0
#define NBC_CENSUS_R 2304
#define NBC_CENSUS_RS 2816
#define NBC_CENSUS_M 3328
#define NBC_CENSUS_B 3337
#define NBC_CENSUS_NONFINITE 3340
#define NBC_CENSUS_WORDS 3341
size_t nbc_softmax_census_workspace_bytes(int N, int H, int W);
int nbc_softmax_census(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W,
                       void* workspace_dev, size_t workspace_bytes, uint64_t* rows_dev, uint8_t* confidence_dev,
                       void* hip_stream);

/* The operating-point sweep: the 3 x 3 confusion of the label map at every point of a grid of (bark offset, node offset)
 * pairs, from one pass over the full-resolution logits.  The checkpoints were trained with class weights (get_pos_weight,
 * utils.py:72-73); the standard correction is a constant per class added to the logits before the argmax, and this call
 * counts what every such pair would label.  No context: csrc/offset_sweep.hip.  The definition, per pixel of image n with
 * f32 logits x0, x1, x2 and target class t (round(2 * float32(v) / 255) of its grey level, as nbc_confusion derives it):
 *   the decision at (i, j) is k = argmax(x0, x1 (+) bark_offsets[i], x2 (+) node_offsets[j]), (+) one f32 addition, the
 *   argmax nbc_forward's (the first maximum wins, a NaN counts as the maximum); class 0's logit is never touched;
 *   conf[n][i][j][t][p] counts the pixels of target class t whose decision at (i, j) is p.
 * Non-finite logits decide like any other, so the nine cells of every grid point sum to H * W; at a point with both offsets
 * 0 the table is nbc_confusion of the labels nbc_forward made from the same logits.  The row layout: conf_dev is
 * uint64 [N][G1][G2][3][3], cell (t, p) of point (i, j) of image n at ((n * G1 + i) * G2 + j) * 9 + t * 3 + p.
 * logits_full_dev    float32 [N,3,H,W], what nbc_forward writes to logits_full_dev; any 4-byte alignment (16-byte loads
 *                    where an image's planes start on 16-byte boundaries)
 * target_dev         uint8 [N,H,W] grey levels
 * bark_offsets_host  G1 finite f32 values, strictly ascending, host memory, read before the call returns; 1 <= G1 <= 33
 * node_offsets_host  G2 of the same; 1 <= G2 <= 33.  The values travel as kernel arguments.
 * workspace_dev      at least nbc_offset_sweep_workspace_bytes(N, H, W, G1, G2) bytes of device memory, 256-byte aligned
 * conf_dev           overwritten
 * For a pixel and an i the decision along j is argmax(x0, x1 (+) bark_offsets[i]) up to some index and 2 from there on (f32
 * addition is monotone in the addend; class 2 wins on a strict > only); the kernel counts that one switch index per
 * (pixel, i).  Integer sums only (LDS integer atomics inside a tile, per-tile partials in the workspace, tiles added by a
 * second launch; no float atomics, no memset): an image's table is bit-identical alone, anywhere in a batch and on any
 * stream.  Runs on hip_stream (the caller's current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a
 * null pointer, N < 1 or N > 65535, H or W < 1, H * W >= 2^31, G1 or G2 outside 1..33, an offset that is not finite, a list
 * that is not strictly ascending, or a workspace too small or misaligned.  With P = H * W, T = ceil(P / 4096) and A(x) = x
 * rounded up to a multiple of 256, the workspace is
 *   A(12 G1 (G2 + 1) N T) bytes
 * (per image and tile: G1 * 6 * (G2 + 1) 16-bit counts); nbc_offset_sweep_workspace_bytes returns 0 for a shape or a grid
 * nbc_offset_sweep refuses.  Messages begin "nbc_offset_sweep:". */
#define NBC_SWEEP_MAX_GRID 33
size_t nbc_offset_sweep_workspace_bytes(int N, int H, int W, int G1, int G2);
int nbc_offset_sweep(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W,
                     const float* bark_offsets_host, int G1, const float* node_offsets_host, int G2,
                     void* workspace_dev, size_t workspace_bytes, uint64_t* conf_dev, void* hip_stream);

/* ---- the shipped tool's live Dropout --------------------------------------------------------
 * FCNHead's Dropout(0.1) (models.py:113-124) sits behind the 3x3 head convolution and in front of classifier.4, and the
 * shipped predict.py never calls .eval(): every number it wrote is one random draw of that mask.  torch's CPU random stream
 * is not reproduced; these calls sample the SAME distribution with a generator of the library's own, so that the spread
 * the shipped tool puts on a number can be measured.  The definition of a draw:
 *
 * For image n of the batch with 64-bit identity id, 64-bit seed S, draw number d >= 0 and probability p in [0, 1):
 *   X        the stored input of classifier.4 as the last nbc_forward left it: [h*w][512] per image, post-BatchNorm and
 *            post-ReLU (in NBC_BN_PER_IMAGE the in-place "<bn>.apply" has run on it)
 *   e        element index pixel * 512 + c, pixel = y * w + x; quad q = e >> 2, lane e & 3; h * w * 128 < 2^32
 *   r        Philox4x32-10(counter = (q, d, id & 0xffffffff, id >> 32), key = (S & 0xffffffff, S >> 32))[lane]
 *            (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds; counter and key
 *            all zero give 6627e8d5 e169c58d bc57ac4c 9b00dbd8)
 *   keep     r >= T, T = floor(p * 2^32) evaluated in double (p = 0.1: T = 429496729)
 *   m        float32(1) / float32(1.0 - p): what nn.Dropout multiplies a kept element by
 *   logits_d[k][pixel] = bias[k] + sum_c w[k][c] * (X[pixel][c] * (m * keep)), through the weights and in the summation
 *            order of the forward's classifier.4 launch (lane l owns channels 8l .. 8l+7, an f32 fma chain, a 64-lane xor
 *            tree, then the bias): with p = 0 a draw is BITWISE the forward's low-resolution logits.  A logit that is not
 *            finite raises the context's sticky word (nbc_nonfinite_seen).
 * then, as the forward and the folder driver do: bicubic upsample + argmax, remove_small_zones(min_pixels) unless 0, the
 * optional 2 -> 1 remap, per-class pixel counts.  A draw of an image depends on (X, id, S, d, p) alone: not on the batch
 * it runs in, its place in it, the stream, the context, or how many draws share a pass. */

/* Host only, no context, no device: keep_host[i] = 1 when element first_element + i of draw `draw` is kept, else 0
 * (count flags).  NBC_ERR_INVALID: p outside [0, 1), draw < 0, a null keep_host with count > 0, elements beyond 2^34. */
int nbc_dropout_mask(uint64_t seed, uint64_t image_id, int draw, double p, uint64_t first_element, size_t count,
                     uint8_t* keep_host);
/* Bytes of device workspace that let nbc_dropout_draws run draws_per_pass draws of an [N,3,H,W] forward in one pass.
 * With (h, w) = nbc_lowres_size(H, W), I = draws_per_pass * N and A(x) = x rounded up to a multiple of 256:
 *   A(12 I h w) + A(I H W) + 2 A(4 I H W) + A(I H W)
 * (low-resolution logits, uint8 labels, and remove_small_zones' parent / size ints and background bytes).  0 for what
 * nbc_dropout_draws refuses: N < 1, H or W < 8, draws_per_pass < 1, I > 65535, H > 65535, H * W >= 2^31, h * w >= 2^25. */
size_t nbc_dropout_workspace_bytes(int N, int H, int W, int draws_per_pass);
/* Draws first_draw .. first_draw + draws - 1 of every image of the context's last forward.
 * image_ids_host     HOST memory, N identities (read before the call returns)
 * logits_lowres_dev  nullable, float32 [draws][N][3][h][w]
 * counts_dev         int64 [draws][N][3]: pixels per class of each draw's final labels; overwritten
 * min_pixels         remove_small_zones' threshold (the reference: 150), 0 = none;  exclude_nodes: the 2 -> 1 remap
 * workspace_dev      256-byte aligned device memory, at least nbc_dropout_workspace_bytes(N, H, W, 1); contents scratch.  As
 *                    many draws share a pass (one read of X, the draws stacked as images on the upsample and
 *                    remove_small_zones launchers) as it has room for; results do not depend on that number.
 * Enqueues on hip_stream -- the stream of the forward, or one ordered behind it -- and does not synchronise; the context's
 * activations are read, nothing of the context is written but the sticky non-finite word.
 * NBC_ERR_INVALID: p outside [0, 1), draws < 1 or > 1024, first_draw < 0 or first_draw + draws > 2^31 - 1, min_pixels < 0,
 * a null context, identity, count or workspace pointer, a misaligned workspace or one too small for one draw per pass.
 * NBC_ERR_STATE: unless the context's last forward was an NBC_ARCH_FCN_RESNET50 forward of exactly this (N, H, W) and
 * nothing has touched its plan since (nbc_reserve of another shape, nbc_autotune, keep mode, BatchNorm mode, new weights).
 * Both BatchNorm modes and all three precisions are served. */
int nbc_dropout_draws(nbc_ctx* ctx, int N, int H, int W, const uint64_t* image_ids_host, double p, uint64_t seed,
                      int first_draw, int draws, int min_pixels, int exclude_nodes, float* logits_lowres_dev,
                      int64_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);

/* ---- per-pixel votes of the draws ------------------------------------------------------------
 * Where in the image the draws disagree.  The definition (csrc/votes.hpp), for D draws, 1 <= D <= 65535:
 *   vote word  one uint32 per pixel: bits 0..15 = n1, the draws whose final label is 1; bits 16..31 = n2, the draws whose
 *              final label is 2; n0 = D - n1 - n2.  A label outside {0,1,2} votes nowhere, as nbc_confusion counts it nowhere.
 *   winner     the class with the most votes; a tie goes to the lowest class index (torch.argmax's first maximum)
 *   support    floor(255 * n_win / D) in integer arithmetic: 255 exactly when the draws are unanimous, never below 85
 *   invalid    a word with n1 + n2 > D cannot come from D draws: label 0, support 0, and of the statistics below it reaches
 *              slot 7 alone
 *   statistics int64 [NBC_VOTE_STATS] per image: 0..2 pixels per winning class, 3..5 unanimous pixels per class, 6 the sum
 *              of n_win, 7 invalid words, 8 the sum of n1, 9 the sum of n2 */
#define NBC_VOTE_STATS 10
/* Host only, no context, no device: the winner and the support byte of one word under `draws` draws (either pointer may be
 * null).  NBC_ERR_INVALID: draws outside 1..65535. */
int nbc_vote_decode(uint32_t word, int draws, uint8_t* label, uint8_t* support);
/* nbc_dropout_draws -- the same arguments, workspace, refusals, stream semantics, and bit for bit the same logits and counts
 * -- which also counts each pass's final labels into the vote words before the next pass overwrites them.
 * votes_dev   uint32 [N][H][W], 16-byte aligned
 * accumulate  0: the words are overwritten (the first pass stores them; no memset is needed); 1: the draws are added to what
 *             the words hold.  The caller keeps the total of the draws added into a word at or below 65535.
 * NBC_ERR_INVALID as nbc_dropout_draws (draws > 1024 among them), and a null or misaligned votes_dev.  NBC_ERR_STATE as
 * nbc_dropout_draws.  Messages begin "nbc_dropout_votes:". */
int nbc_dropout_votes(nbc_ctx* ctx, int N, int H, int W, const uint64_t* image_ids_host, double p, uint64_t seed,
                      int first_draw, int draws, int min_pixels, int exclude_nodes, float* logits_lowres_dev,
                      int64_t* counts_dev, uint32_t* votes_dev, int accumulate, void* workspace_dev, size_t workspace_bytes,
                      void* hip_stream);
/* The decision on every word and the statistics of every image.  No context: csrc/dropout_votes.hip.
 * votes_dev    uint32 [N][H][W], any 4-byte alignment (a 16-byte aligned buffer is read by 16-byte loads)
 * draws        D, the draws the words hold
 * labels_dev   nullable, uint8 [N][H][W]: the winner
 * support_dev  nullable, uint8 [N][H][W]: the support byte
 * stats_dev    int64 [N][NBC_VOTE_STATS]; overwritten
 * Integer sums: an image's numbers are the same alone, in any batch and on any stream.  Runs on hip_stream (the caller's
 * current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a null votes_dev or stats_dev, N < 1 or
 * N > 65535, H or W < 1, H * W >= 2^31, draws outside 1..65535, a votes_dev that is not 4-byte aligned. */
int nbc_vote_summary(const uint32_t* votes_dev, int N, int H, int W, int draws, uint8_t* labels_dev, uint8_t* support_dev,
                     int64_t* stats_dev, void* hip_stream);
/* The vote words of D label maps of each image that are on the device already, whatever made them (the flip views below, or a
 * caller's own): the counting nbc_dropout_votes does pass by pass, on its own.  No context: csrc/dropout_votes.hip.
 * labels_dev  uint8 [D][N][H][W], map-major like the draws of a pass; any alignment.  A label outside {0,1,2} votes nowhere.
 * votes_dev   uint32 [N][H][W], 16-byte aligned
 * accumulate  0: the words are overwritten (no memset is needed); 1: the D maps are added to what the words hold.  The caller
 *             keeps the total of the maps added into a word at or below 65535.
 * Integer sums: an image's words are the same alone, in any batch and on any stream.  Runs on hip_stream (the caller's
 * current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a null pointer, N < 1 or N > 65535, H or W < 1,
 * H * W >= 2^31, D outside 1..65535, a votes_dev that is not 16-byte aligned. */
int nbc_vote_tally(const uint8_t* labels_dev, int N, int D, int H, int W, uint32_t* votes_dev, int accumulate, void* hip_stream);

/* ---- the flip views the training augmented over ------------------------------------------------
 * The reference trains with RandomHorizontalFlip and RandomVerticalFlip on the sample and its mask (__main__.py:160-164) and
 * never uses that at prediction time.  These two calls make the mirror images of a batch and bring the network's answers for
 * them back into one orientation; the forward between them is nbc_forward on the stack, as it stands.
 *   views    a mask of NBC_TTA_* bits, 1..15; its V views are taken in ascending bit order
 *   stack    view-major, like [draws][N] of nbc_dropout_draws: entry j * N + i is view j of image i
 *   aligned  the un-flipped view: a_j[i][c][y][x] = v_j[i][c][y'][x'], y' = h-1-y if view j mirrors rows, x' = w-1-x if it
 *            mirrors columns -- consistent with interpolate(align_corners=False) for every H and W
 *   merged   m = (((a_0 + a_1) + a_2) + a_3) / float(V): f32 adds in view order, no contraction, one IEEE f32 division; V = 1
 *            gives the view's own bits, a NaN in any view gives NaN */
enum {
  NBC_TTA_IDENTITY = 1,
  NBC_TTA_HFLIP = 2,    /* columns mirrored: x[..., W-1-j] */
  NBC_TTA_VFLIP = 4,    /* rows mirrored */
  NBC_TTA_HVFLIP = 8,   /* both */
  NBC_TTA_FLIPS = 15
};
/* The V views of a batch in one launch.  No context: csrc/tta.hip.
 * x_dev    NBC_IN_U8_NHWC (a pixel is 3 bytes: rows are mirrored by pixel; any alignment) or NBC_IN_F32_NCHW (per plane;
 *          4-byte aligned)
 * out_dev  [V][N] entries in x's layout; must not overlap x
 * Each source row is read once and written V times: H * W * 3 * (1 + V) bytes per u8 image.  Runs on hip_stream (the caller's
 * current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a null pointer, an unknown dtype, views outside
 * 1..15, N < 1 or V * N > 65535, H or W < 1, H * W >= 2^31, an f32 pointer that is not 4-byte aligned, out_dev overlapping
 * x_dev. */
int nbc_tta_views(const void* x_dev, int x_dtype, int N, int H, int W, int views, void* out_dev, void* hip_stream);
/* The aligned views and their mean from the low-resolution logits of a stacked forward.  No context: csrc/tta.hip.
 * lowres_views_dev  float32 [V][N][3][h][w]: view j's logits in view j's orientation
 * merged_dev        float32 [N][3][h][w]; overwritten
 * aligned_dev       nullable, float32 [V][N][3][h][w]; must not alias the input
 * An element of merged depends on the V elements it is made of alone: an image's bits are the same alone, in any batch and
 * on any stream.  NBC_ERR_INVALID, before any HIP call: as nbc_tta_views on h and w (every pointer 4-byte aligned), and an
 * output that overlaps the input. */
int nbc_tta_merge(const float* lowres_views_dev, int N, int h, int w, int views, float* merged_dev, float* aligned_dev,
                  void* hip_stream);

/* ---- the colour-jitter views the training augmented over ---------------------------------------
 * The reference trains with ColorJitter(saturation=0.2, brightness=0.1) on the sample (__main__.py:160) and never uses that at
 * prediction time.  These calls make the colour views of a batch and average the network's answers for them;
 * the forward between them is nbc_forward on the stack, as it stands.
 *   view     a triple of float32 factors (b, c, s), each finite and in [0, 4].  A view set is V triples, 1 <= V <=
 *            NBC_JITTER_MAX_VIEWS, taken in the order given.
 *   image    the view of a uint8 RGB frame is saturation_s(contrast_c(brightness_b(frame))); every step yields a uint8 image, as
 *            the PIL chain torchvision 0.3 runs does.  A step whose factor is exactly 1.0f is the identity.  The order
 *            brightness -> contrast -> saturation is this library's: torchvision shuffles the order per sample.
 *   step     blend(degenerate, image, f) per byte: t = float(d) + f * float(i - d) with d, i the degenerate and image bytes as
 *            ints -- one f32 multiply and one f32 add, no contraction; the result is 0 if t <= 0, 255 if t >= 255, else t
 *            truncated toward zero.
 *   degenerates  brightness: 0.  saturation: the pixel's grey L = (19595 R + 38470 G + 7471 B + 32768) >> 16 in all three
 *            channels.  contrast: every byte = m, the rounded mean grey of the image the step receives (after brightness): with
 *            S the sum of L over that image, m = floor((2 S + H W) / (2 H W)) -- PIL's int(mean + 0.5) for every H W < 2^31, an
 *            exact half rounds up.  m is per image and per view, never per batch.
 *   stack    view-major, like nbc_tta_views': entry j * N + i is view j of image i
 *   mean     m = (((v_0 + v_1) + v_2) + ...) / float(V): f32 adds in view order, no contraction, one IEEE f32 division; V = 1
 *            gives the view's own bits (-0 included), a NaN in any view gives NaN: nbc_tta_merge's rule without the un-flip,
 *            for V up to NBC_JITTER_MAX_VIEWS.
 * Left out: hue (the reference never jitters it), float32 NCHW input (torchvision's tensor path is other arithmetic), products
 * of colour and flip views, and the Gaussian sampling of the reference's NormColorJitter (a caller passes any factors). */
enum { NBC_JITTER_MAX_VIEWS = 16 };
/* The bytes nbc_jitter_views' workspace needs for N images and V views (8 V N), into *bytes.  NBC_ERR_INVALID: a null pointer,
 * V outside 1..16, N < 1 or V * N > 65535. */
int nbc_jitter_workspace_bytes(int N, int V, size_t* bytes);
/* The V views of a batch.  No context: csrc/jitter.hip.
 * x_dev          NBC_IN_U8_NHWC [N][H][W][3], any alignment
 * factors        HOST memory, float32 [V][3]: (b, c, s) per view; they travel as kernel arguments (no copy, no synchronisation)
 * out_dev        [V][N][H][W][3], any alignment; must not overlap x
 * workspace_dev  nbc_jitter_workspace_bytes(N, V) bytes, 8-byte aligned; cleared by the call on the stream.  Used when a view has
 *                c != 1: a pass before the views takes the uint64 grey sums (integer sums: they do not depend on arrival order;
 *                views with the same b share one).
 * The source is read once and every view written once: H * W * 3 * (1 + V) bytes per image (+ H * W * 3 per distinct b of the
 * contrast pass).  An image's bytes are the same alone, in any batch and on any stream.  Runs on hip_stream (the caller's
 * current device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a null pointer, V outside 1..16, N < 1 or
 * V * N > 65535, H or W < 1, H * W >= 2^31, a factor that is NaN, negative or above 4, overlapping buffers, a workspace that is
 * not 8-byte aligned. */
int nbc_jitter_views(const uint8_t* x_dev, int N, int H, int W, const float* factors, int V, uint8_t* out_dev, void* workspace_dev,
                     void* hip_stream);
/* The mean of the low-resolution logits of a stacked forward.  No context: csrc/jitter.hip.
 * lowres_views_dev  float32 [V][N][3][h][w]
 * mean_dev          float32 [N][3][h][w]; overwritten
 * An element of the mean depends on the V elements it is made of alone.  NBC_ERR_INVALID, before any HIP call: a null pointer,
 * V outside 1..16, N < 1 or V * N > 65535, h or w < 1, h * w >= 2^31, a pointer that is not 4-byte aligned, mean_dev
 * overlapping the input. */
int nbc_views_mean(const float* lowres_views_dev, int N, int V, int h, int w, float* mean_dev, void* hip_stream);

/* ---- the crop windows the training augmented over ----------------------------------------------
 * The reference trains on RandomCrop(crop_size) windows of a frame with crop_size = 512 (__main__.py:158-165, 260) and then
 * predicts from whole 1024-wide frames.  These calls cut a batch into windows of the training's size and blend the network's
 * answers for them back into the frame's grid; the forward between them is nbc_forward on the stack.
 *   S, T     the window side and the stride: S a multiple of 8 in 32..2048, T a multiple of 8 with 8 <= T <= S <= 8 T.  The
 *            cell is NBC_WINDOW_CELL = 8 pixels, the trunk's output stride.
 *   grid     per axis of length L >= 8 (H or W): L8 = 8 ceil(L / 8), the extent E = min(S, L8).  L8 <= S: one window at offset
 *            0.  Otherwise the offsets k T for every k with k T + S < L8, then a last offset L8 - S: n = 1 + ceil((L8 - S) / T)
 *            windows.  Every offset is a multiple of 8 (a window's stride-2 layers sample the frame's own pixel phase), every
 *            window of an image has the shape E_y x E_x, window k = r n_x + c has the offsets (oy_r, ox_c).  K = n_y n_x <=
 *            NBC_WINDOW_MAX_K and K N <= 65535.
 *   fill     rows L .. L8 - 1 (at most 7; columns alike) are filled by reflection without repeating the edge: index i reads
 *            index 2 (L - 1) - i -- padding_mode='reflect' of the training's pad_resize (utils.py:242-247), numpy.pad(mode=
 *            "reflect").  The reach stays inside the frame for every L >= 8.
 *   stack    window-major, like nbc_tta_views' stack: entry k N + i is window k of image i
 *   merged   on the low-resolution logits, a grid of h x w = L8_y / 8 x L8_x / 8 cells -- ceil(H / 8) x ceil(W / 8), the shape of
 *            the plain forward's own low-resolution logits.  Window k gives its cell (y - oy / 8, x - ox / 8) to frame cell
 *            (y, x).  With e = E / 8 and cap = max(1, e / 2) (integer division) the per-axis weight of window cell j is t(j) =
 *            min(dl, dr, cap): dl = j + 1 if the window's offset is > 0, dr = e - j if offset + E < L8, each unbounded
 *            otherwise (a window border that is the frame's own border is not down-weighted).  A window's weight at a cell is
 *            w = t_y t_x, an integer <= 16384 (NBC_BLEND_TENT), or 1 everywhere (NBC_BLEND_UNIFORM).  A cell that one window
 *            covers: m = v, the window's own bits (-0 included).  Otherwise acc = float(w_0) v_0, then acc = acc + float(w_k)
 *            v_k over the covering windows in ascending k -- every multiply and add a rounded f32 operation of its own, no
 *            contraction -- and m = acc / float(sum of w_k), one IEEE f32 division; the sum is an exact integer below 2^24.  A
 *            NaN in any covering window gives NaN.
 * The tail upsamples the h x w grid to H x W as interpolate(align_corners=False) does for the plain forward: where H is no
 * multiple of 8 that is the stretch of less than one cell the plain path has always made.
 * Left out: the EfficientNet networks (output stride 32 and fixed asymmetric pads: a grid of their own), per-image BatchNorm
 * statistics (a window's statistics are not the frame's), products with the flip or colour views and per-window votes (the
 * number of windows over a pixel varies).  The training's 1024 x 1024 pad_resize frame is nbc_training_frame, below. */
enum { NBC_WINDOW_CELL = 8, NBC_WINDOW_MAX_K = 1024 };
enum { NBC_BLEND_TENT = 0, NBC_BLEND_UNIFORM = 1 };
/* The window grid of an H x W frame: the one place Python and the kernels take it from.  Host only, no HIP call.
 * dims       int [4]: E_y, E_x, n_y, n_x
 * offsets_y  nullable, int [n_y] (NBC_WINDOW_MAX_K entries always suffice); offsets_x likewise, [n_x]
 * NBC_ERR_INVALID: a null dims, S or T outside the rules above, H or W < 8, H * W >= 2^31, K > NBC_WINDOW_MAX_K. */
int nbc_window_grid(int H, int W, int S, int T, int* dims, int* offsets_y, int* offsets_x);
/* The K windows of every image of a batch in one launch.  No context: csrc/windows.hip.
 * x_dev    NBC_IN_U8_NHWC [N][H][W][3] at any alignment, or NBC_IN_F32_NCHW [N][3][H][W], 4-byte aligned
 * out_dev  [K][N] entries of E_y x E_x in x's layout; must not overlap x
 * Each source row is read once and every window written once: 3 H W + 3 K E_y E_x bytes per u8 image.  An image's windows are
 * the same alone, in any batch and on any stream.  Runs on hip_stream (the caller's current device); no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null pointer, an unknown dtype, what nbc_window_grid refuses, N < 1 or K N > 65535, an
 * f32 pointer that is not 4-byte aligned, out_dev overlapping x_dev. */
int nbc_window_views(const void* x_dev, int x_dtype, int N, int H, int W, int S, int T, void* out_dev, void* hip_stream);
/* The merged low-resolution logits of a stacked forward of nbc_window_views' stack.  No context: csrc/windows.hip.
 * lowres_windows_dev  float32 [K][N][3][E_y / 8][E_x / 8]
 * H, W                the frame's size in pixels, as nbc_window_views took it
 * blend               NBC_BLEND_TENT or NBC_BLEND_UNIFORM
 * merged_dev          float32 [N][3][h][w]; overwritten
 * An element of merged depends on the window cells that cover it alone: an image's bits are the same alone, in any batch and
 * on any stream.  NBC_ERR_INVALID, before any HIP call: as nbc_window_views, an unknown blend, a pointer that is not 4-byte
 * aligned, merged_dev overlapping the input. */
int nbc_window_merge(const float* lowres_windows_dev, int N, int H, int W, int S, int T, int blend, float* merged_dev,
                     void* hip_stream);

/* ---- the training run's own frame --------------------------------------------------------------
 * The reference's test_dataset -- the one val_miou, ReduceLROnPlateau, EarlyStopping, the choice of checkpoint and the test_*
 * figures of exp.test read (__main__.py:209-228) -- passes every sample and its dual through pad_resize(img, 1024, 1024)
 * (utils.py:242-247), and RandomCrop(512) cuts the training's crops from the same frame (__main__.py:158-165).  These calls make
 * that frame on the device (the host restatement is neuralbarkcalculator_amd/training_frame.py).  Per axis, with L
 * the source length and Lt the frame's:
 *   pad       p = ceil((Lt - L) / 2) on both sides, Lp = L + 2 p, which is Lt or Lt + 1.  Padded index i reads source index
 *             r(i - p) with r(j) = -j for j < 0, r(j) = 2 (L - 1) - j for j >= L, else j: torchvision's pad(padding_mode=
 *             'reflect'), numpy.pad(mode="reflect").  L > Lt and p > L - 1 are refused: one reflection must reach.
 *   Lp == Lt  the axis is a pure index map.
 *   Lp == Lt + 1  PIL's 8-bit ImagingResample with the bilinear filter (what torchvision's resize ran): output o reads the
 *             padded indices first[o] .. first[o] + NBC_FRAME_TAPS - 1 with the integer coefficients k[o][.] in 22-bit fixed
 *             point (an unused tap is 0 and reads nothing) and is clip8((2^21 + sum v k) >> 22), >> arithmetic, clip8 to 0..255.
 *   order     the horizontal pass first, rounded to bytes, then the vertical pass on those bytes: PIL's order and its intermediate
 *             image.  Neither the padded nor the intermediate image is written: an output byte recomputes its at most 3 x 3 reads.
 * Left out: predict on the frame (a resampled axis has no integer map back to the scan's own rows) and frames that shrink an
 * axis.  The two figures of exp.test that need all images of a batch at once -- the batch-pooled Lovasz loss, and
 * remove_small_zones on the [B,H,W] batch, whose connectivity=2 on a 3-D array links zones of neighbouring images through the
 * batch axis -- are nbc_lovasz_softmax_groups and nbc_remove_small_zones_groups. */
enum { NBC_FRAME_TAPS = 3 };
/* PIL's table of the bilinear filter for in_size -> out_size (Resample.c: precompute_coeffs, then normalize_coeffs_8bpc), in
 * doubles in PIL's order, no contraction: support = scale = in / out, center = (o + 0.5) scale, xmin = (int)(center - support +
 * 0.5) clamped at 0, xmax = (int)(center + support + 0.5) clamped at in, weights 1 - |(x + xmin - center + 0.5) (1 / scale)| divided
 * by their sequential sum, then (int)(0.5 + w 2^22).  Host only, no HIP call.
 * first  int32 [out_size]; coeff  int32 [out_size][NBC_FRAME_TAPS]
 * NBC_ERR_INVALID: a null pointer, anything but in_size == out_size + 1 >= 2 (all that pad_resize can produce). */
int nbc_bilinear_taps(int in_size, int out_size, int32_t* first, int32_t* coeff);
/* pad_resize of a batch of equal-shape uint8 images in one launch.  No context: csrc/training_frame.hip.
 * x_dev         channels = 3: NBC_IN_U8_NHWC frames [N][H][W][3]; channels = 1: grey duals [N][H][W]; at any alignment
 * Ht, Wt        the frame's size
 * row_taps_dev  the table of the vertical pass, needed (and read) only where H + 2 p_y == Ht + 1: int32 [Ht][4] on the device,
 *               entry o = { first[o], coeff[o][0], coeff[o][1], coeff[o][2] } of nbc_bilinear_taps(Ht + 1, Ht); 4-byte aligned.
 *               The caller uploads it: the library makes no hidden copy and does not synchronise.  An index a foreign table
 *               names beyond the padded axis is clamped into it.
 * col_taps_dev  likewise for the horizontal pass, [Wt][4], where W + 2 p_x == Wt + 1
 * out_dev       uint8 [N][Ht][Wt][channels] at any alignment; must not overlap x.  A lane makes four consecutive bytes and stores
 *               the aligned dword they are; the bytes before the first and after the last aligned dword go singly.
 * About channels H W bytes are read and channels Ht Wt written per image.  An image's bytes are the same alone, in any batch and
 * on any stream.  Runs on hip_stream (the caller's current device); no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null x_dev or out_dev, channels not 1 or 3, N < 1 or N > 65535, a length < 1, H > Ht or
 * W > Wt, p > L - 1 on either axis, Ht * Wt >= 2^31, a missing table for a resampled axis, a table that is not 4-byte aligned,
 * out_dev overlapping x_dev. */
int nbc_training_frame(const void* x_dev, int channels, int N, int H, int W, int Ht, int Wt, const int32_t* row_taps_dev,
                       const int32_t* col_taps_dev, void* out_dev, void* hip_stream);

/* ---- refit of classifier.4: the loss's gradient on the device ------------------------------------
 * classifier.4 (models.py:121) is a 1x1 convolution 512 -> 3 with bias: 1 539 parameters, linear in the features the forward
 * leaves on the device.  These calls evaluate the pixel-wise cross-entropy family and its gradient with respect to those
 * parameters, through the bicubic upsample, for parameters other than the checkpoint's (the host restatement
 * and the driver are neuralbarkcalculator_amd/refit.py; the kernels csrc/head_refit.hip).  Gradients into classifier.0 or the
 * backbone, gradients of pooled groups (nbc_lovasz_softmax_groups) and the DeepLab / EfficientNet heads are left out.  The
 * Lovasz-Softmax gradient and MixedLoss's (utils.py:185-192) come in at item 4 through nbc_lovasz_gradient below.
 *
 * theta = (W f32 [3][512], b f32 [3]) in the state_dict's units: classifier.4.weight[:, :, 0, 0], then classifier.4.bias, 1 539
 * floats in that order.  Per image n, with P = H * W and (h, w) = nbc_lowres_size(H, W):
 *   1 trial logits   lowres = b + W X, X the stored input of classifier.4 as the last nbc_forward left it, through the forward's
 *                    own classifier.4 launch (lane l owns channels 8l .. 8l+7, an f32 fma chain, a 64-lane xor tree, then the
 *                    bias).  In NBC_PREC_F16X2 the stored X carries the power of two 2^a of its tensor
 *                    (nbc_activation_exponent("classifier.0")) and the weights are multiplied by 2^-a on the device, exactly as
 *                    nbc_pack_weights does: with theta the checkpoint's values the result is BITWISE nbc_forward's
 *                    logits_lowres, in every precision.
 *   2 full size      nbc_upsample_argmax on those logits: logits_full f32 [N,3,H,W] and the argmax p (first maximum wins).
 *   3 loss           nbc_pixel_cross_entropy: sums[n][t][p], counts[n][t][p].  For a table T of nine doubles indexed
 *                    [target class t][argmax class p] the objective of an image is sum T[t][p] sums[t][p]; over a folder that,
 *                    summed over the images and divided by the sum of their P.  T = 1: the plain cross-entropy; T[t][p] = w[t]:
 *                    the class-weighted one; T[t][p] = w[max(t, p)]: CustomWeightedCrossEntropy (utils.py:151-165).
 *   4 pixel gradient from the f32 logits_full in f64: m = max_c x_c, q_c = exp(x_c - m) / sum_k exp(x_k - m),
 *                    g_c = T[t][p] (q_c - [c = t]).  T[t][p] is a constant of the pixel (what autograd makes of the reference's
 *                    index_select of the weights); t from the grey level as nbc_confusion derives it.  No special case for a
 *                    logit that is not finite: NaN propagates.
 *   5 upsample adjoint  with the per-axis tables of nbc_bicubic_taps (iy, cy for h -> H; ix, cx for w -> W):
 *                    grad_lowres[n][c][i][j] = sum over (Y, a) with iy[Y][a] = i and (X, b) with ix[X][b] = j of
 *                    (double)cy[Y][a] (double)cx[X][b] g_c[Y][X], in f64, not normalised (no 1 / P).  Evaluated as the column
 *                    pass sum_(X, b) (double)cx g (X ascending over lo[j] .. hi[j], then b ascending), then the row pass on its
 *                    results (Y ascending over lo[i] .. hi[i], then a ascending).
 *   6 head gradient  grad_theta[n][c][k] = sum over the cells of grad_lowres[n][c][cell] (double)X[cell][k] for k < 512,
 *                    grad_theta[n][c][512] = sum over the cells of grad_lowres[n][c][cell]: f64 [N][3][513] in the state_dict's
 *                    units (the sums over the stored X times 2^-a, exact).
 *   7 determinism    every float sum has an order fixed by (H, W, h, w) alone and nothing is added atomically: an image's
 *                    numbers are bit-identical alone, anywhere in a batch and on any stream. */

/* Trial logits (1).  theta_dev: 1 539 floats on the device, 4-byte aligned; logits_lowres_dev: float32 [N,3,h,w], overwritten.
 * Enqueues on hip_stream -- the stream of the forward, or one ordered behind it -- and does not synchronise.  The context's
 * activations are read; of the context only a 1 539-float scratch array (allocated by the first call) and the sticky non-finite
 * word (a logit that is not finite raises it, as in nbc_forward) are written.
 * NBC_ERR_INVALID, before any HIP call: a null ctx, theta_dev or logits_lowres_dev; either one not 4-byte aligned; N < 1 or
 * N > 65535, H or W < 1, H * W >= 2^31.
 * NBC_ERR_STATE: nbc_dropout_draws' contract -- unless the context's last forward was an NBC_ARCH_FCN_RESNET50 forward of exactly
 * this (N, H, W) and nothing has touched its plan since.  Both BatchNorm modes and all three precisions are served. */
int nbc_head_logits(nbc_ctx* ctx, const float* theta_dev, int N, int H, int W, float* logits_lowres_dev, void* hip_stream);

/* The tap table of one axis of the bicubic upsample in_size -> out_size (align_corners = False), host only, no HIP call:
 * cubic_setup's arithmetic (csrc/pointwise.hip) in f32 with every operation rounded on its own (no fused multiply-add, so
 * that any host reproduces the table): scale = (float)in_size / (float)out_size, s = scale (o + 0.5) - 0.5,
 * i0 = min(floor(s), in_size - 1), t = s - i0 clamped to [0, 1], taps i0 - 1 .. i0 + 2 clamped to [0, in_size - 1], and
 * ATen's get_cubic_upsample_coefficients(t) with A = -0.75.
 * idx    int32 [out_size][4]; coeff  float32 [out_size][4]
 * lo, hi int32 [in_size]: lo[i] .. hi[i] is the range of outputs o with a tap on input i; i0 is monotone in o, so the range is
 *        contiguous.  An input that no output touches (in_size > out_size) gets lo = 0, hi = -1.
 * NBC_ERR_INVALID: a null pointer, in_size or out_size outside 1 .. 2^24. */
int nbc_bicubic_taps(int in_size, int out_size, int32_t* idx, float* coeff, int32_t* lo, int32_t* hi);

/* Pixel gradient and upsample adjoint (4, 5).  No context.
 * logits_full_dev  float32 [N,3,H,W], 4-byte aligned (an image whose three planes start on 16-byte boundaries is read by 16-byte
 *                  loads); target_dev  uint8 [N,H,W] grey levels
 * h, w             the low-resolution size, 1 <= h <= H, 1 <= w <= W
 * row_*_dev        nbc_bicubic_taps(h, H) on the device: idx int32 [H][4] and coeff float32 [H][4], both 16-byte aligned, lo and
 *                  hi int32 [h].  col_*_dev: likewise nbc_bicubic_taps(w, W).  The caller uploads them: the library makes no
 *                  hidden copy.  A foreign table's indices are only compared and its lo / hi are clamped into the axis: no read
 *                  leaves the buffers whatever the tables hold.
 * table9_host      HOST memory, T[t][p] as nine doubles (read before the call returns)
 * workspace_dev    at least nbc_ce_gradient_workspace_bytes(N, H, W, h, w) bytes, 256-byte aligned; contents scratch.  With
 *                  A(x) = x rounded up to a multiple of 256 and P' = H W rounded up to even:  A(24 N P') + A(24 N H w)
 *                  (g as f64 planes; the column pass's result)
 * grad_lowres_dev  float64 [N,3,h,w], 8-byte aligned; overwritten
 * Three launches: the pixel pass reads 13 P and writes 24 P bytes per image, the column pass reads those 24 P and writes 24 H w,
 * the row pass reads 24 H w and writes 24 h w.  Runs on hip_stream (the caller's current device); no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null pointer (any of the fourteen); N < 1 or N > 65535, H or W < 1, H * W >= 2^31;
 * h < 1, w < 1, h > H or w > W; an idx or coeff table that is not 16-byte aligned; logits_full_dev or a lo / hi table that is not
 * 4-byte aligned; grad_lowres_dev not 8-byte aligned; a workspace too small or not 256-byte aligned.
 * nbc_ce_gradient_workspace_bytes returns 0 for a shape nbc_ce_gradient refuses. */
size_t nbc_ce_gradient_workspace_bytes(int N, int H, int W, int h, int w);
int nbc_ce_gradient(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int h, int w,
                    const int32_t* row_idx_dev, const float* row_coeff_dev, const int32_t* row_lo_dev, const int32_t* row_hi_dev,
                    const int32_t* col_idx_dev, const float* col_coeff_dev, const int32_t* col_lo_dev, const int32_t* col_hi_dev,
                    const double* table9_host, void* workspace_dev, size_t workspace_bytes, double* grad_lowres_dev,
                    void* hip_stream);

/* The Lovasz-Softmax gradient, alone or beside the cross-entropy family's (MixedLoss, utils.py:185-192): nbc_lovasz_softmax's
 * terms and, in place of item 4, the pixel gradient of  sum T'[t][p] ce + lambda L,  L = (1 / C_p) sum over the present classes of
 * terms[n][c] the image's Lovasz-Softmax loss (C_p = the classes with fg_counts > 0); then item 5 by the same two launches.  No
 * context; csrc/lovasz.hip.  Per image and class c, on the keys nbc_lovasz_softmax sorts (key = bits(e) << 1 | fg, e = |fg - p_c| in
 * f32, descending):
 *   slope     J(k, F) = 1 - (G - F) / (G + k - F) with G the class's foreground count, k keys counted, F of them foreground
 *             (J(0, 0) = 0).  A pixel's key lies in a run of identical keys that starts at position r, is R keys long and has F_r
 *             foreground keys before it; every pixel of the run gets the run's mean slope
 *             [J(r + R, F_r + fg R) - J(r, F_r)] / R -- on an image without ties the reference's J_i - J_(i-1) at the pixel's
 *             position; with ties (which torch.sort leaves open) independent of the pixel order, equal e putting foreground first.
 *   d_c       - sign(fg - p_c) slope / C_p: negative for a foreground pixel, positive for a background one, 0 where e == 0
 *             (torch's abs'(0)) and for an absent class.  The order, the sign and the e == 0 test come from the f32 keys.
 *   softmax   g_k = q_k (d_k - sum_c d_c q_c), c ascending, q in f64 from the f32 logits as in item 4.
 *   pixel     g_k = T'[t][p] (q_k - [k = t]) + lambda (the above); the first term only with a table, the second only with
 *             lambda != 0 (with lambda == 0 the planes are nbc_ce_gradient's bit for bit).
 *   not finite  an image whose softmax is not finite somewhere has NaN terms (as nbc_lovasz_softmax) and, with lambda != 0, NaN in
 *             every pixel and so in every cell of its grad_lowres; no other image is touched.
 * logits_full_dev .. col_hi_dev   as nbc_ce_gradient takes them
 * table9_host      HOST memory, T' as nine doubles, already scaled by the caller; may be null (no cross-entropy term)
 * lovasz_weight    lambda, finite
 * workspace_dev    at least nbc_lovasz_gradient_workspace_bytes(N, H, W, h, w) bytes, 256-byte aligned; contents scratch.  With
 *                  A(x) = x rounded up to a multiple of 256 and P = H W:
 *                  nbc_lovasz_workspace_bytes(N, H, W) + 2 A(12 N P) + A(24 N P) + A(24 N H w)
 *                  (the terms' regions; the keys in pixel order and the foreground prefix; g; the column pass's result)
 * terms_dev, fg_counts_dev   float64 / int64 [N,3], 8-byte aligned: nbc_lovasz_softmax's outputs from its own launches, bit for bit
 * grad_lowres_dev  float64 [N,3,h,w], 8-byte aligned; overwritten, not normalised
 * keys_dev         nullable: uint32 [N,3,H,W], 4-byte aligned, the keys in pixel order (else they live in the workspace)
 * pixel_grad_dev   nullable: float64 [N,3,H,W], 8-byte aligned, the g planes (else they live in the workspace)
 * After nbc_lovasz_softmax's launches (a device-to-device copy of the 12 P bytes of keys per image among them): the prefix pass
 * reads 12 P and writes 12 P bytes per image; the pixel pass reads 13 P + 12 P, about log2(P) + 2 dependent 4-byte loads per
 * (pixel, class) into the sorted segment and one into the prefix, and writes 24 P; then the column and row passes.  Every float
 * sum has an order fixed by the shape, nothing is added atomically: item 7 holds.  Runs on hip_stream; no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null pointer other than table9_host, keys_dev and pixel_grad_dev; what nbc_ce_gradient
 * refuses of the shape, the tables and logits_full_dev; a lovasz_weight that is not finite; terms_dev, fg_counts_dev,
 * grad_lowres_dev or pixel_grad_dev not 8-byte aligned; keys_dev not 4-byte aligned; a workspace too small or not 256-byte
 * aligned.  nbc_lovasz_gradient_workspace_bytes returns 0 for a shape nbc_lovasz_gradient refuses. */
size_t nbc_lovasz_gradient_workspace_bytes(int N, int H, int W, int h, int w);
int nbc_lovasz_gradient(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int h, int w,
                        const int32_t* row_idx_dev, const float* row_coeff_dev, const int32_t* row_lo_dev, const int32_t* row_hi_dev,
                        const int32_t* col_idx_dev, const float* col_coeff_dev, const int32_t* col_lo_dev, const int32_t* col_hi_dev,
                        const double* table9_host, double lovasz_weight, void* workspace_dev, size_t workspace_bytes,
                        double* terms_dev, int64_t* fg_counts_dev, double* grad_lowres_dev, uint32_t* keys_dev,
                        double* pixel_grad_dev, void* hip_stream);

/* Head gradient (6): one read of X (2 048 bytes per cell; 1 024 in NBC_PREC_BF16), a block per 64 consecutive cells, a second
 * launch adds the blocks' partials in block order.
 * grad_lowres_dev  float64 [N,3,h,w], (h, w) = nbc_lowres_size(H, W); 8-byte aligned
 * workspace_dev    at least nbc_head_gradient_workspace_bytes(N, H, W) = A(8 * 1539 N ceil(h w / 64)) bytes, 256-byte aligned
 * grad_theta_dev   float64 [N][3][513], 8-byte aligned; overwritten
 * Stream semantics and NBC_ERR_STATE as nbc_head_logits; nothing of the context is written.
 * NBC_ERR_INVALID, before any HIP call: a null ctx, grad_lowres_dev, workspace_dev or grad_theta_dev; grad_lowres_dev or
 * grad_theta_dev not 8-byte aligned; N < 1 or N > 65535, H or W < 1, H * W >= 2^31; a workspace too small or not 256-byte
 * aligned.  nbc_head_gradient_workspace_bytes returns 0 for a shape nbc_head_gradient refuses. */
size_t nbc_head_gradient_workspace_bytes(int N, int H, int W);
int nbc_head_gradient(nbc_ctx* ctx, const double* grad_lowres_dev, int N, int H, int W, void* workspace_dev,
                      size_t workspace_bytes, double* grad_theta_dev, void* hip_stream);

/* ---- the zones of a label map ------------------------------------------------------------------
 * What the two percentages of an image are made of: how many nodes there are, how big each one is, where it lies, and
 * whether the bark is one sheet or many fragments.  The reference has no such code; the host restatement is
 * neuralbarkcalculator_amd/zones.py (scipy.ndimage.label per class plus numpy reductions), the kernels csrc/zones.hip.
 *
 * Zones of a label map: the 8-connected components of each class c in {1, 2} (pixels with any other value belong to no zone).
 * rows_dev  int64 [N, cap, NBC_ZONE_ROW], num_dev int64 [N].  num_dev[n] = the number of zones of image n (all of them, also
 * when > cap).  Rows 0 .. min(num, cap)-1 of image n, in ascending order of first_pixel; rows beyond are not written.
 * Row: { first_pixel (y*W+x of the zone's first pixel in raster order), class, pixels, x0, y0, x1, y1 (inclusive box),
 *        sum_x, sum_y (over the zone's pixels), perimeter }
 * perimeter: the number of pixel sides (4-neighbourhood) of the zone whose neighbour has another label or lies outside the
 * image.  A 4-neighbour of the same class is in the same zone, so the figure is local to the pixel and an exact integer.
 * labels_dev     uint8 or int64 [N,H,W] (labels_dtype NBC_LABEL_U8 / NBC_LABEL_I64); read, never written
 * workspace_dev  at least nbc_zones_workspace_bytes(N, H, W) bytes of device memory, 256-byte aligned; contents scratch
 * Everything is an integer sum, minimum or maximum: an image's rows are the same alone, in any batch, on any stream and from
 * run to run.  Runs on hip_stream (on the context's device); no synchronisation.  NBC_ERR_INVALID, before any HIP call: a null
 * pointer (ctx, labels_dev, rows_dev, num_dev, workspace_dev), N < 1 or N > 65535, H or W outside 1..65535, H * W >= 2^31,
 * cap < 1, another labels_dtype, a workspace that is too small or not 256-byte aligned. */
#define NBC_ZONE_ROW 10
/* With P = H * W and A(x) = x rounded up to a multiple of 256:  A(4 N P) + A(N P) + A(4 N ceil(P / 1024))
 * (a parent int and a class byte per pixel, and a root count per 1024 pixels): 5 bytes per pixel and a little.
 * 0 for a shape that nbc_label_zones refuses. */
size_t nbc_zones_workspace_bytes(int N, int H, int W);
int nbc_label_zones(nbc_ctx* ctx, const void* labels_dev, int labels_dtype, int N, int H, int W,
                    int64_t* rows_dev, int cap, int64_t* num_dev, void* workspace_dev, size_t workspace_bytes, void* hip_stream);

/* ---- output zones against target zones ----------------------------------------------------------
 * Which zone of a label map is which zone of its labelled mask, and how well they overlap: what the per-pixel metrics of
 * the evaluation hide (two nodes reported where the mask has one, every small node missed, three nodes glued into one).  The
 * reference has no such code; the host restatement is zones.match_cpu (scipy.ndimage.label per class, a zone-index plane
 * per map, numpy.unique on the joined key), the kernels csrc/zone_match.hip.
 *
 * out_rows_dev / out_num_dev   what nbc_label_zones gives for labels_dev: same rows, same order, same cap behaviour
 * tgt_rows_dev / tgt_num_dev   the same of the target's class map, the class of a grey level being nbc_confusion's
 *                              (0..63 -> 0, 64..191 -> 1, 192..255 -> 2); both int64 [N, cap, NBC_ZONE_ROW] / int64 [N]
 * pair_rows_dev  int64 [N, pair_cap, NBC_ZONE_PAIR_ROW], pair_num_dev int64 [N].
 * Pair row: { output zone index, target zone index, pixels }.  An index is the zone's position among its map's zones in
 * first-pixel order (the row number in out_rows / tgt_rows; valid for every zone, also at or above cap).  pixels: the pixels
 * that lie in both zones, > 0.  Only zones of the same class share pixels.  The rows of an image are sorted by (output index,
 * target index).  pair_num_dev[n] = the number of distinct pairs of image n when that is <= pair_cap; otherwise exactly
 * pair_cap + 1, and the image's pair_cap rows are unspecified.  Nothing outside an image's own rows is ever written, and
 * rows pair_num[n] onwards are not written when pair_num[n] <= pair_cap.
 * labels_dev / target_grey_dev  uint8 or int64 [N,H,W] / uint8 [N,H,W]; read, never written
 * workspace_dev  at least nbc_zone_match_workspace_bytes(N, H, W, pair_cap) bytes, 256-byte aligned; contents scratch
 * No loop of the pass depends on the data for its end: hash probes are bounded by their table's size, and an image with
 * more than pair_cap pairs stops inserting.  Integer counts and a sorted output: an image's three outputs are the same alone,
 * in any batch, on any stream and from run to run.  Runs on hip_stream (on the context's device); no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null pointer, the shapes, cap and labels_dtype nbc_label_zones refuses, pair_cap
 * outside 1..NBC_ZONE_PAIRS_MAX_CAP, a workspace that is too small or not 256-byte aligned. */
#define NBC_ZONE_PAIR_ROW 3
#define NBC_ZONE_PAIRS_MAX_CAP 4096   /* what the sort kernel's LDS holds: 4096 x (8-byte key + 4-byte count) = 48 KiB */
/* With P = H * W, T = the power of two >= 2 * pair_cap (at least 2) and A(x) = x rounded up to a multiple of 256:
 *   2 nbc_zones_workspace_bytes(N, H, W) + A(N P) + A(8 N T) + A(4 N T) + A(4 N)
 * (both labellings, the target's class map, and per image the pair table's keys and counts and a claim counter): 11 bytes
 * per pixel and a little.  0 for a shape or a pair_cap that nbc_match_zones refuses. */
size_t nbc_zone_match_workspace_bytes(int N, int H, int W, int pair_cap);
int nbc_match_zones(nbc_ctx* ctx, const void* labels_dev, int labels_dtype, const uint8_t* target_grey_dev, int N, int H, int W,
                    int64_t* out_rows_dev, int64_t* out_num_dev, int64_t* tgt_rows_dev, int64_t* tgt_num_dev, int cap,
                    int64_t* pair_rows_dev, int64_t* pair_num_dev, int pair_cap, void* workspace_dev, size_t workspace_bytes,
                    void* hip_stream);

/* ---- contour distances against the labelled masks -------------------------------------------------
 * How far the contours of a label map lie from the contours of its labelled mask: the error model of an area in mm^2 (a
 * zone's area error is about its perimeter times the displacement).  The reference has no such code; the host restatement
 * is contours.contours_cpu (scipy erosion for the contour, scipy's exact Euclidean distance transform by indices), the
 * kernels csrc/contours.hip.
 *
 * Class maps: the output's class is the label, 1 or 2 (any other value belongs to no class); the target's class is
 * nbc_confusion's (grey 0..63 -> 0, 64..191 -> 1, 192..255 -> 2).  A pixel is on the contour of class c iff it has class c
 * and at least one 4-neighbour inside the image does not (the inner 4-contour; a neighbour outside the image is no contour
 * side, so the frame that cuts both maps alike adds nothing).
 * Sets: four per image, s = 2 (c - 1) + dir for c = 1 (Bark), 2 (Node); dir 0: source = the output's contour, destination =
 * the target's; dir 1: source = the target's, destination = the output's.  For a source pixel p,
 * d2(p) = min over the destination pixels q of (px - qx)^2 + (py - qy)^2, an exact integer.
 * rows_dev  int64 [N, NBC_CONTOUR_SETS, NBC_CONTOUR_HEAD + bins].  Row: { n, m, sum_d2, max_d2, hist[bins] }: n the source
 *   contour pixels, m the destination contour pixels, sum_d2 and max_d2 the sum and the maximum of d2 over the source pixels,
 *   hist[k] for k < bins - 1 the source pixels with ceil(sqrt(d2)) == k, that is (k - 1)^2 < d2 <= k^2 (bin 0: d2 == 0), and
 *   hist[bins - 1] those with d2 > (bins - 2)^2.  The bin is computed on the integers.  With bins >= ceil(hypot(H - 1,
 *   W - 1)) + 1 the last bin is no overflow bin.  When n == 0 or m == 0, sum_d2, max_d2 and every bin are 0.
 * sum_d_dev  float64 [N, NBC_CONTOUR_SETS]: the sum of sqrt(d2) over the source pixels, 0.0 when n == 0 or m == 0.  The sum
 *   is added in an order fixed by the image alone: a row's source pixels, listed in an order their positions fix, go
 *   round-robin over the threads of a block, then the lanes of a wave by the xor butterfly, the waves in order, then the
 *   rows lane-strided and by the butterfly; no float atomics, and nothing in the order depends on the batch, the stream
 *   or the timing.  The integers are sums, maxima and counts, whose order does not matter.  An image's rows and sum_d
 *   therefore have the same bits alone, in any batch, on any stream and from run to run.
 * labels_dev / target_grey_dev  uint8 or int64 [N,H,W] / uint8 [N,H,W]; read, never written
 * workspace_dev  at least nbc_contours_workspace_bytes(N, H, W) bytes, 256-byte aligned; contents scratch
 * Every word of rows_dev and sum_d_dev is written on every call, zeros included; nothing outside them (and the workspace) is
 * written.  No loop of the pass depends on the data for its end: the row scan of a pixel takes at most W steps.
 * Runs on hip_stream (on the context's device); no synchronisation.
 * NBC_ERR_INVALID, before any HIP call: a null pointer, N outside 1..65535, H or W outside 1..NBC_CONTOUR_MAX_SIDE (d2 then
 * fits 32 bits and a row's column distances fit LDS), bins outside 2..5793 (= ceil(hypot(4095, 4095)) + 1), another
 * labels_dtype, a workspace that is too small or not 256-byte aligned. */
#define NBC_CONTOUR_SETS 4
#define NBC_CONTOUR_HEAD 4          /* n, m, sum_d2, max_d2 */
#define NBC_CONTOUR_MAX_SIDE 4096
/* With P = H * W and A(x) = x rounded up to a multiple of 256:
 *   A(N P) + A(8 N P) + A(8 * 4 N H)
 * (a mark byte per pixel, four u16 column distances per pixel, an f64 partial per image, set and row): 9 bytes per pixel
 * and N * 4 * H doubles.  0 for a shape that nbc_contour_distances refuses. */
size_t nbc_contours_workspace_bytes(int N, int H, int W);     /* 0 for a shape the call refuses */
int nbc_contour_distances(nbc_ctx* ctx, const void* labels_dev, int labels_dtype, const uint8_t* target_grey_dev,
                          int N, int H, int W, int64_t* rows_dev /* [N,4,NBC_CONTOUR_HEAD+bins] */, int bins,
                          double* sum_d_dev /* [N,4] */, void* workspace_dev, size_t workspace_bytes, void* hip_stream);

/* The resize of the reference's preprocessor (models.py:191-198): uint8 RGB [H,W,3] on the device ->
 * ToTensor (u8 / 255 in float32) -> skimage.transform.resize(order=3, mode='reflect',
 * anti_aliasing=False) to out_h x out_w (4-tap Catmull-Rom, all arithmetic in float32 like scikit-image's
 * compiled warp, reflected borders, clipped to the input range) -> float32 [out_h,out_w,3] on the device.
 * Bit-identical to the numpy restatement in neuralbarkcalculator_amd/predict.py, which equals
 * scikit-image 0.18.3's output value for value on the committed fixtures. */
int nbc_resize_cubic_u8(nbc_ctx* ctx, const uint8_t* src_dev, int H, int W, float* dst_dev, int out_h, int out_w,
                        void* hip_stream);
/* The same resize followed by what the reference does with its result (models.py:199-203), for a square
 * target: dst_u8_dev uint8 [out_h,out_w,3] = the bytes skimage.io.imsave writes for that float image
 * (uint8(float64(x) * 255 + 0.499999999), imageio's float -> uint8 path), and row_lit_dev (nullable, int32
 * [out_h]) = per row the number of pixels whose float32 channel sum exceeds 1e-3, i.e. trim_black's `lit`
 * test (models.py:158-159); the caller drops the leading / trailing rows with count / out_w <= 0.85. */
int nbc_preprocess_u8(nbc_ctx* ctx, const uint8_t* src_dev, int H, int W, uint8_t* dst_u8_dev, int32_t* row_lit_dev,
                      int out_h, int out_w, void* hip_stream);

/* Tuning / test knob for the convolution kernel: tile = -1 (per-layer choice) or a tile id of the menu, 0..20.  The menu --
 * every tile's shape, waves, stages, precisions and reason -- is the one table of csrc/conv_tiles.hpp; nbc_conv_tile_info
 * reports it.  18 / 19 / 20 are the row-resident 3x3 kernel of f16x2 (csrc/conv3x3_rows.hip): the stride-1 3x3 layers of
 * 128-pixel-wide maps run on 18 or 20 (256 output channels or more: same K order, same bits on both) or 19 (64 / 128) AND ON
 * NOTHING ELSE -- their K order (channel block, kh, kw) is the layer's, so a forced or measured generic tile leaves them where
 * they are -- and no other layer runs on them.  Forced wherever the layer's kind, Cout and the precision allow it; where they do
 * not, the planned tile runs. */
int nbc_set_conv_tile(nbc_ctx* ctx, int tile);

/* Per-layer tile choice by measurement: runs one forward on x (so that the workspace holds real
 * activations), then times every tile shape of the LDS-DMA kernel on every convolution of the
 * current (N,H,W) plan (`reps` launches each, HIP events) and keeps the fastest.  Results do not
 * depend on the tile, only speed does: every tile a layer may run on walks K in the same order with the same sums per
 * output (one accumulator; in f16x2 on the row-step tiles 18 / 19 / 20 two: the low-piece products have a sum of their
 * own, joined once behind the K loop -- on 18 and 20 alike).  Without this call a
 * plan runs on per-layer defaults from a cost model (rounds of blocks per CU x per-block time, fitted to
 * measurements), within 0.1-0.6 % (f32) / 0.5-4.4 % (bf16) of the measured best at any image height; the
 * measurement costs 0.5-0.9 s per shape.  The choice is
 * part of the plan; the context keeps the plans (and choices) of the last 64 shapes it has seen, so a
 * folder of height-trimmed images tunes each distinct (N,H,W) once.
 * nbc_get_plan_tiles copies the tile id of each conv launch of the plan; returns their number. */
int nbc_autotune(nbc_ctx* ctx, const void* x_dev, int x_dtype, int N, int H, int W, int reps, int objective,
                 void* hip_stream);   /* objective 0: time of the launch alone; 1: time x fraction of the 256
                                         CUs it occupies (forwards overlapped on several streams) */
int nbc_get_plan_tiles(nbc_ctx* ctx, int32_t* tiles, int capacity);
/* The default tile id the cost model gives a convolution with M = N*Ho*Wo output pixels, Cout output channels and
 * K = Cin*kh*kw products per output (host arithmetic only: no device needed); -1 for an unknown precision or a Cout
 * no tile divides. */
int nbc_default_conv_tile(int M, int Cout, int K, int precision);
/* The tile menu (host only: no context, no device): 1 and the tile's pixels (rows) x channels (cols), its kind (0 the generic
 * kernel, 1 / 2 the row-resident 3x3 kernel for 256 or more / 64 or 128 output channels) and whether it has the dual-branch
 * form (nbc_set_fuse_downsample), each through a non-null pointer; 0 if the precision has no such tile. */
int nbc_conv_tile_info(int precision, int tile, int32_t* rows, int32_t* cols, int32_t* kind, int32_t* has_dual);
/* Install a tile choice (one id per conv launch of the current plan, as nbc_get_plan_tiles returns them),
 * e.g. one measured in an earlier process: NBC_ERR_INVALID when the count or a tile does not fit. */
int nbc_set_plan_tiles(nbc_ctx* ctx, const int32_t* tiles, int n);

/* 1 when a forward of this context since the last reset raised a bit of the sticky word (NBC_NONFINITE_*), else 0 (negative:
 * error): a logit that is NaN or infinite, raised by classifier.4's launch at no measurable cost, or, in NBC_BN_PER_IMAGE on
 * NBC_PREC_F16X2, a channel outside the pieces' range (NBC_NONFINITE_BN_RANGE).  Either way the f16x2 run is not to be trusted.  NaN / inf in the input or the weights do
 * that in every mode, like in the reference; in NBC_PREC_F16X2 so does an activation beyond f16's range (+-65504), which
 * that mode cannot represent: a caller that runs unknown weights in f16x2 checks this after its last forward and falls
 * back to NBC_PREC_FP32 when it is raised (the folder driver does).  Synchronises the device. */
int nbc_nonfinite_seen(nbc_ctx* ctx, int reset);
/* The same word without a synchronisation: enqueues on hip_stream a copy of it to *host_dst, valid
 * once work enqueued behind it on that stream has been waited for; non-zero = raised by a forward that ran on this
 * context ahead of the copy.  host_dst must be PINNED host memory (hipHostMalloc / hipHostRegister): a copy to pageable
 * memory is staged and may block, which is what this call exists to avoid -- NBC_ERR_INVALID otherwise.  The folder driver sends it along with every batch's labels, so that an f16x2 run of
 * weights that mode cannot carry is abandoned at the first batch that shows it, not after the last. */
int nbc_nonfinite_peek_async(nbc_ctx* ctx, uint32_t* host_dst, void* hip_stream);

/* ---- the operating point ----------------------------------------------------------------- */
/* Logit offsets: with (bark, node) set, the upsample + argmax launch of nbc_forward and nbc_upsample_argmax decides by
 * k = argmax(x0, x1 (+) bark, x2 (+) node) -- the decision nbc_offset_sweep counts, (+) one f32 addition -- instead of the plain
 * argmax; the launch counts and remaps (exclude_nodes) after the decision, and everything downstream sees it.  Only the
 * decision moves: logits_lowres_dev and logits_full_dev receive the values they receive without offsets, and class 0's
 * logit is never touched.  (0, 0) is off, the default: the context then launches exactly the kernels it launched before
 * (the offset forms are kernels of their own).  Finite values only (NBC_ERR_INVALID otherwise).  nbc_dropout_draws and
 * nbc_dropout_votes answer NBC_ERR_INVALID on a context with offsets on: the draws have a tail of their own. */
int nbc_set_logit_offsets(nbc_ctx* ctx, float bark, float node);

/* ---- debugging / measurement ----------------------------------------------------------- */
/* NBC_PREC_F16X2: the first bottleneck of a ResNet stage computes its downsample.0 inside the launch of the conv3 that
 * adds it (one launch instead of two; the tensor between them is never written or read back) wherever conv3 has at most
 * 8 K-steps (layer1.0, layer2.0, layer3.0) and runs on a tile that has the dual-branch form (17, 8, 10).  Same bits either way.
 * On by default; off: two launches, as with keep-activations, profiling or NBC_BN_PER_IMAGE, and as in every other
 * precision.  The plan marks the pairs and gives them buffers that serve both forms (nbc_describe_plan); the identity buffer,
 * which only the two-launch form uses, is allocated by the first forward that runs a pair that way (that forward
 * synchronises the device, as one of a larger shape does).  A switch for tests and A/B runs. */
int nbc_set_fuse_downsample(nbc_ctx* ctx, int on);
/* (downsample.0, conv3) pairs the last nbc_forward ran as one launch. */
int nbc_fused_pairs(nbc_ctx* ctx);
/* Copy the activation written by conv unit `name` during the last forward to `dst_host` as
 * float32 NCHW.  `capacity` is in elements.  Only valid when keep-activations is on. */
int nbc_set_keep_activations(nbc_ctx* ctx, int on);
/* The calibration guard of NBC_PREC_F16X2 (any precision answers): after a forward with keep-activations on, the largest
 * finite |value| of every conv unit's output tensor AS STORED on the device (with the power of two nbc_pack_weights gave it),
 * one float per conv unit in nbc_conv_info order (0 for classifier.4, whose output is the logits); returns their number
 * (nbc_arch_num_convs() of the attached architecture) or a negative error.  DeepLabV3: the pooling branch's entry is its
 * pooled vector; the concat holds exactly the five branch tensors, so its peak is the largest of theirs.  nbc_pack_weights places a tensor by its BatchNorm's promise; this is what the
 * data did.  A tensor that peaks below 2^-8 has most of its values under f16x2's 2^-12 floor (absolute error 2^-36), one
 * beyond 2^14 is a factor four from f16's range: a caller that sees either on a frame of its data runs NBC_PREC_FP32
 * (the folder driver checks its first image: neuralbarkcalculator_amd/predict.py).  Synchronises the device. */
int nbc_activation_peaks(nbc_ctx* ctx, float* peaks_host, int capacity);
int nbc_read_activation(nbc_ctx* ctx, const char* name, float* dst_host, size_t capacity,
                        int64_t shape[4]);
/* When on, every launch of the next forwards is bracketed by HIP events on the forward's stream
 * (no synchronisation inside nbc_forward).  nbc_num_op_records() waits for the last profiled
 * forward, averages each launch over all forwards profiled since the previous call, resets the
 * accumulation and returns the number of records (one per launch of the plan). */
int nbc_set_profiling(nbc_ctx* ctx, int on);
int nbc_num_op_records(nbc_ctx* ctx);
int nbc_get_op_record(nbc_ctx* ctx, int index, nbc_op_record* out);

#ifdef __cplusplus
}
#endif
#endif /* NBC_H */
