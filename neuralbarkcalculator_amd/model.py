"""Host-side mirror of the reference's model object for the accelerated path.

``FCNResNet50`` stands where ``fcn_resnet50(pretrained=False)`` is bound to ``self.model`` in
``NeuralBarkCalculator.__init__`` (/root/reference/src/bark_calculator/models.py:221-223) and is
called at ``models.py:269``; ``DeepLabV3ResNet50`` stands for ``deeplabv3_resnet50()`` (``models.py:46-57``), the other
network the reference's training script offers (``__main__.py:230-232``).  They keep the reference's surface -- ``load_state_dict``, ``to``,
``eval``, ``__call__`` -- and adds the fused ``predict_labels`` (``models.py:269-270`` plus the
``--exclude_nodes`` remap ``models.py:273-276`` and the per-class counts ``models.py:324-331``).

All arithmetic happens in libnbc_hip.so (hand-written gfx950 kernels) through the C ABI of
``include/nbc.h``; torch only supplies device memory, the current stream and, for multi-GPU
runs, ``torch.distributed`` (RCCL) for the one-off weight broadcast.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib, topology
from .topology import NUM_CLASSES, out_hw

_PRECISIONS = {"fp32": _lib.PREC_FP32, "f32": _lib.PREC_FP32, "float32": _lib.PREC_FP32,
               "bf16": _lib.PREC_BF16, "bfloat16": _lib.PREC_BF16, "f16x2": _lib.PREC_F16X2}
# NBC_BN_*; "image" is per-image statistics on the f32 MFMA, "image_f16x2" the same mode on an "f16x2" model
BN_STATISTICS = {"running": _lib.BN_RUNNING, "image": _lib.BN_PER_IMAGE, "image_f16x2": _lib.BN_PER_IMAGE}
PER_IMAGE_MODES = ("image", "image_f16x2")


def _as_numpy(v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def _tensor_array(state_dict: Mapping[str, object]):
    """The state_dict as an array of nbc_tensor, and what keeps its memory alive during a call."""
    items = []
    keep = []   # keep numpy arrays / byte strings alive during the call
    for name, value in state_dict.items():
        a = _as_numpy(value)
        if a.dtype == np.int64:
            dt = 1
        else:
            a = a.astype(np.float32, copy=False)
            dt = 0
        shape = a.shape                      # ascontiguousarray promotes 0-dim to 1-dim
        a = np.ascontiguousarray(a)
        if len(shape) > 4:
            raise RuntimeError(f"state_dict entry {name!r} has {len(shape)} dims")
        t = _lib.NbcTensor()
        bname = name.encode()
        t.name = bname
        t.data = a.ctypes.data if a.size else None
        for i in range(4):
            t.shape[i] = shape[i] if i < len(shape) else 1
        t.ndim = len(shape)
        t.dtype = dt
        items.append(t)
        keep.append((a, bname))
    return (_lib.NbcTensor * len(items))(*items), len(items), keep


def pack_state_dict(state_dict: Mapping[str, object], precision: str = "fp32", arch="fcn_resnet50") -> np.ndarray:
    """Check keys like ``nn.Module.load_state_dict`` (strict) against architecture ``arch`` and return the packed weight
    blob (uint8 numpy array).  Raises ``RuntimeError`` listing missing / unexpected keys."""
    lib = _lib.load()
    prec = _PRECISIONS[precision]
    a = topology.arch_index(arch)
    arr, n, _keep = _tensor_array(state_dict)
    nbytes = lib.nbc_arch_packed_weights_bytes(prec, a)
    blob = np.zeros(nbytes, dtype=np.uint8)
    _lib.check(lib.nbc_pack_weights_arch(arr, n, prec, a, blob.ctypes.data, nbytes), "load_state_dict")
    return blob


def pack_bn_affine(state_dict: Mapping[str, object], arch="fcn_resnet50") -> np.ndarray:
    """The per-image BatchNorm affine array of ``state_dict`` (nbc_pack_bn_affine): float32, gamma then beta of every conv
    unit with a BatchNorm, in ``topology.conv_units`` order.  Same strict key check and ``RuntimeError`` as
    ``pack_state_dict``."""
    lib = _lib.load()
    a = topology.arch_index(arch)
    arr, n, _keep = _tensor_array(state_dict)
    count = lib.nbc_arch_bn_affine_floats(a)
    out = np.zeros(count, dtype=np.float32)
    _lib.check(lib.nbc_pack_bn_affine(arr, n, a, out.ctypes.data, count), "load_state_dict")
    return out


def _broadcast_side_array(arr: Optional[np.ndarray], count: int, who: str, what: str, arch, src: int, group, device) -> np.ndarray:
    """``torch.distributed`` broadcast of a float32 array of ``count`` elements from rank ``src``: ``who`` and ``what`` name
    the caller and the array in the source rank's refusal."""
    import torch.distributed as dist
    if dist.get_rank(group) == src:
        if arr is None or arr.size != count:
            raise RuntimeError("%s: the source rank holds no %s of %s" % (who, what, arch))
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    else:
        t = torch.empty(count, dtype=torch.float32)
    if device is not None:
        t = t.to(device)
    dist.broadcast(t, src=src, group=group)
    return t.cpu().numpy()


def broadcast_bn_affine(affine: Optional[np.ndarray], arch="fcn_resnet50", src: int = 0, group=None, device=None) -> np.ndarray:
    """``torch.distributed`` broadcast of the per-image BatchNorm affine array from rank ``src`` (which passes it; the
    other ranks pass None and get its copy).  ``device``: where the collective's tensor lives (an RCCL group needs the
    GPU; None = the host, for gloo)."""
    count = int(_lib.load().nbc_arch_bn_affine_floats(topology.arch_index(arch)))
    return _broadcast_side_array(affine, count, "broadcast_bn_affine", "affine array", arch, src, group, device)


def pack_bn_raw(state_dict: Mapping[str, object], arch="fcn_resnet50"):
    """``(array, flags)``: the raw-convolution array of ``state_dict`` for per-image BatchNorm statistics in "f16x2"
    (nbc_pack_bn_raw): float32 powers of two, per conv unit with a BatchNorm ``2^(r - k - a_in)`` then ``2^-r`` per channel,
    in ``topology.conv_units`` order, and its NBC_PACK_* bits.  Same strict key check and ``RuntimeError`` as
    ``pack_state_dict``."""
    lib = _lib.load()
    a = topology.arch_index(arch)
    arr, n, _keep = _tensor_array(state_dict)
    count = lib.nbc_arch_bn_raw_floats(a)
    out = np.zeros(count, dtype=np.float32)
    rc = lib.nbc_pack_bn_raw(arr, n, a, out.ctypes.data, count)
    if rc < 0:
        _lib.check(rc, "load_state_dict")
    return out, int(rc)


def bn_raw_flags(raw: np.ndarray) -> int:
    """``_lib.PACK_SCALE_RANGE`` when an entry of a raw-convolution array is not a normal f32 (a power of two that left the
    range), else 0: what a rank that received the array by broadcast can still tell."""
    a = np.abs(np.asarray(raw, dtype=np.float32))
    ok = np.isfinite(a) & (a >= np.finfo(np.float32).tiny)
    return 0 if bool(ok.all()) else _lib.PACK_SCALE_RANGE


def broadcast_bn_raw(raw: Optional[np.ndarray], arch="fcn_resnet50", src: int = 0, group=None, device=None) -> np.ndarray:
    """``torch.distributed`` broadcast of the raw-convolution array (``pack_bn_raw``) from rank ``src``, as
    ``broadcast_bn_affine`` sends the affine array."""
    count = int(_lib.load().nbc_arch_bn_raw_floats(topology.arch_index(arch)))
    return _broadcast_side_array(raw, count, "broadcast_bn_raw", "raw-convolution array", arch, src, group, device)


def arch_of_state_dict(state_dict: Mapping[str, object]) -> str:
    """The architecture (``topology.ARCHS``) whose key set the state_dict matches exactly (nbc_arch_of_state_dict);
    ``RuntimeError`` with the strict-load message of fcn_resnet50 when none does."""
    lib = _lib.load()
    arr, n, _keep = _tensor_array(state_dict)
    rc = lib.nbc_arch_of_state_dict(arr, n)
    if rc < 0:
        _lib.check(rc, "load_state_dict")
    return topology.arch_name(rc)


def describe_plan(arch: str, precision: str, n: int, h: int, w: int, keep: bool = False, bn_statistics: str = "running") -> str:
    """The launch plan of an [n, 3, h, w] forward as text (nbc_describe_plan; host only: no context, no GPU); ``RuntimeError``
    for what the library refuses."""
    lib = _lib.load()
    args = (topology.arch_index(arch), _PRECISIONS[precision], n, h, w, int(keep), BN_STATISTICS[bn_statistics])
    need = lib.nbc_describe_plan(*args, None, 0)
    if need < 0:
        _lib.check(need, "nbc_describe_plan")
    buf = C.create_string_buffer(need)
    lib.nbc_describe_plan(*args, buf, need)
    return buf.value.decode()


def conv_tile_info(precision: str, tile: int):
    """(rows, cols, kind, has_dual) of a tile id of the convolution menu (nbc_conv_tile_info; host only), or None where the
    precision has no such tile."""
    v = [C.c_int32() for _ in range(4)]
    if not _lib.load().nbc_conv_tile_info(_PRECISIONS[precision], tile, *[C.byref(x) for x in v]):
        return None
    return tuple(x.value for x in v)


TTA_VIEWS = {"hflip": _lib.TTA_IDENTITY | _lib.TTA_HFLIP, "vflip": _lib.TTA_IDENTITY | _lib.TTA_VFLIP, "flips": _lib.TTA_FLIPS}
TTA_VIEW_NAMES = ("identity", "hflip", "vflip", "hvflip")        # bit 0..3 of a view mask (NBC_TTA_*)


def resolve_tta_views(views) -> int:
    """The view mask (NBC_TTA_* bits, 1..15) of ``"hflip"`` (identity + hflip), ``"vflip"`` (identity + vflip), ``"flips"``
    (all four) or of a mask itself; ``ValueError`` otherwise."""
    if isinstance(views, str):
        if views not in TTA_VIEWS:
            raise ValueError("views must be one of %s or a mask in 1..15, got %r" % (", ".join(sorted(TTA_VIEWS)), views))
        return TTA_VIEWS[views]
    if isinstance(views, bool) or not isinstance(views, (int, np.integer)) or not 1 <= int(views) <= _lib.TTA_FLIPS:
        raise ValueError("views must be one of %s or a mask in 1..15, got %r" % (", ".join(sorted(TTA_VIEWS)), views))
    return int(views)


def tta_view_count(mask: int) -> int:
    return bin(int(mask)).count("1")


def tta_view_names(mask: int):
    """The names of the views of a mask, in the order of the stack."""
    return [TTA_VIEW_NAMES[b] for b in range(4) if (int(mask) >> b) & 1]


# the star of the training's amplitudes, ColorJitter(saturation=0.2, brightness=0.1) (__main__.py:160), identity first:
# (brightness, contrast, saturation) per view
JITTER_TRAINING = ((1.0, 1.0, 1.0), (0.9, 1.0, 1.0), (1.1, 1.0, 1.0), (1.0, 1.0, 0.8), (1.0, 1.0, 1.2))
JITTER_VIEWS = {"training": JITTER_TRAINING}


def resolve_jitter_views(views) -> np.ndarray:
    """The float32 ``[V,3]`` factors (brightness, contrast, saturation) of ``"training"`` (``JITTER_TRAINING``) or of a sequence
    of 1..16 triples, each factor finite and in [0, 4] (include/nbc.h, nbc_jitter_views); ``ValueError`` otherwise."""
    what = "views must be one of %s or a sequence of 1..%d (brightness, contrast, saturation) triples with every factor in " \
           "[0, 4], got %r" % (", ".join(sorted(JITTER_VIEWS)), _lib.JITTER_MAX_VIEWS, views)
    if isinstance(views, str):
        if views not in JITTER_VIEWS:
            raise ValueError(what)
        views = JITTER_VIEWS[views]
    if isinstance(views, (bytes, dict, set)) or views is None:
        raise ValueError(what)
    try:
        with np.errstate(over="ignore"):             # a factor beyond float32 becomes inf and is refused below
            f = np.array(views, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(what)
    if f.ndim != 2 or f.shape[1] != 3 or not 1 <= f.shape[0] <= _lib.JITTER_MAX_VIEWS or not bool(np.all((f >= 0) & (f <= 4))):
        raise ValueError(what)
    return np.ascontiguousarray(f)


def jitter_view_names(factors) -> List[str]:
    """The names of the views of a factor array, in the order of the stack: the non-unit factors joined by ``_`` (``b0.9``,
    ``b1.1_s0.8``; ``%g`` of the factor), ``identity`` for (1, 1, 1)."""
    names = []
    for triple in resolve_jitter_views(factors):
        parts = ["%s%g" % (tag, float(v)) for tag, v in zip("bcs", triple) if v != np.float32(1)]
        names.append("_".join(parts) if parts else "identity")
    return names


WINDOW_BLENDS = {"tent": _lib.BLEND_TENT, "uniform": _lib.BLEND_UNIFORM}


def resolve_window_blend(blend) -> int:
    """``NBC_BLEND_*`` of "tent" or "uniform"; ``ValueError`` otherwise."""
    if not isinstance(blend, str) or blend not in WINDOW_BLENDS:
        raise ValueError("blend must be one of %s, got %r" % (", ".join(sorted(WINDOW_BLENDS)), blend))
    return WINDOW_BLENDS[blend]


def window_grid(h: int, w: int, window: int = 512, stride: int = 256):
    """The window grid of an ``h x w`` frame (nbc_window_grid, the one place it is computed; include/nbc.h): ``(E_y, E_x, n_y,
    n_x, offsets_y, offsets_x)`` -- every window is ``E_y x E_x``, window ``k = r * n_x + c`` starts at ``(offsets_y[r],
    offsets_x[c])``.  ``ValueError`` for a window or stride outside the rules, a side below 8 or more than 1024 windows.  No
    device is touched."""
    lib = _lib.load()
    dims = (C.c_int * 4)()
    oy, ox = (C.c_int * _lib.WINDOW_MAX_K)(), (C.c_int * _lib.WINDOW_MAX_K)()
    try:
        args = [int(v) for v in (h, w, window, stride)]
    except (TypeError, ValueError):
        raise ValueError("window_grid takes integers, got %r" % ((h, w, window, stride),))
    if any(abs(v) >= 2 ** 31 for v in args):
        raise ValueError("window_grid: an argument beyond 32 bits in %r" % (args,))
    if lib.nbc_window_grid(args[0], args[1], args[2], args[3], dims, oy, ox) != 0:
        raise ValueError(_lib.last_error())
    return dims[0], dims[1], dims[2], dims[3], list(oy[:dims[2]]), list(ox[:dims[3]])


def bilinear_taps(n_in: int, n_out: int):
    """PIL's 8-bit bilinear table for ``n_in == n_out + 1`` (nbc_bilinear_taps, include/nbc.h): ``(first int32 [n_out], coeff
    int32 [n_out, 3])``.  ``ValueError`` for any other pair of sizes.  No device is touched."""
    try:
        n_in, n_out = int(n_in), int(n_out)
    except (TypeError, ValueError):
        raise ValueError("bilinear_taps takes integers, got %r" % ((n_in, n_out),))
    if not (0 < n_out < 2 ** 30 and 0 < n_in < 2 ** 31):
        raise ValueError("bilinear_taps: sizes out of range in %r" % ((n_in, n_out),))
    first = np.zeros(n_out, dtype=np.int32)
    coeff = np.zeros((n_out, _lib.FRAME_TAPS), dtype=np.int32)
    if _lib.load().nbc_bilinear_taps(n_in, n_out, first.ctypes.data_as(C.POINTER(C.c_int32)),
                                     coeff.ctypes.data_as(C.POINTER(C.c_int32))) != 0:
        raise ValueError(_lib.last_error())
    return first, coeff


def bicubic_taps(n_in: int, n_out: int):
    """One axis of the bicubic upsample ``n_in -> n_out`` as a table (nbc_bicubic_taps, include/nbc.h): ``(idx int32 [n_out, 4],
    coeff float32 [n_out, 4], lo int32 [n_in], hi int32 [n_in])`` -- the four clamped taps of every output with ATen's f32
    coefficients (A = -0.75), and per input the contiguous range of outputs that touch it.  ``ValueError`` for sizes outside
    1 .. 2^24.  No device is touched."""
    try:
        n_in, n_out = int(n_in), int(n_out)
    except (TypeError, ValueError):
        raise ValueError("bicubic_taps takes integers, got %r" % ((n_in, n_out),))
    if not (0 < n_in <= 2 ** 24 and 0 < n_out <= 2 ** 24):
        raise ValueError("bicubic_taps: sizes out of range in %r" % ((n_in, n_out),))
    idx = np.zeros((n_out, 4), dtype=np.int32)
    coeff = np.zeros((n_out, 4), dtype=np.float32)
    lo, hi = np.zeros(n_in, dtype=np.int32), np.zeros(n_in, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    if _lib.load().nbc_bicubic_taps(n_in, n_out, idx.ctypes.data_as(i32), coeff.ctypes.data_as(C.POINTER(C.c_float)),
                                    lo.ctypes.data_as(i32), hi.ctypes.data_as(i32)) != 0:
        raise ValueError(_lib.last_error())
    return idx, coeff, lo, hi


class FCNResNet50:
    """MI355X-native ``fcn_resnet50`` (3 classes, output stride 8, bicubic upsample), eval mode.

    precision: ``"fp32"`` -- f32 MFMA, the parity mode; ``"f16x2"`` -- f32-grade on the f16 matrix pipe: every f32
    value kept as two f16 pieces (to 2^-23 relative for |x| >= 2^-12, an absolute 2^-36 below; weight rows normalised by
    a power of two per output channel, so their magnitude does not matter), three exact f16 products per product, f32
    two-level sums (include/nbc.h, NBC_PREC_F16X2; same tolerances as "fp32" in the tests); ``"bf16"`` -- bf16 MFMA with
    f32 accumulation and f32 BatchNorm epilogue, the throughput mode.

    bn_statistics (``set_bn_statistics``): ``"running"`` (default) -- eval mode, BatchNorm on the running statistics;
    ``"image"`` -- every BatchNorm normalises each image by its own per-channel mean and biased variance, as the shipped
    tool's forward does (it never calls ``.eval()`` and feeds one image at a time), "fp32" only; ``"image_f16x2"`` -- the
    same statistics on an "f16x2" model, the raw convolution outputs kept as pieces.  Dropout is the identity
    in both (live Dropout noise is all that stays different from the shipped tool; ``dropout_draws`` samples it).
    """

    ARCH = "fcn_resnet50"                  # topology.ARCHS entry (NBC_ARCH_*) of the network this class runs

    def __init__(self, precision: str = "fp32"):
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        if topology.is_efficientnet(self.ARCH) and _PRECISIONS[precision] != _lib.PREC_FP32:
            raise ValueError("%s runs in precision 'fp32' only, not %r: swish and the SE gate are not positively homogeneous, "
                             "so f16x2's powers of two cannot be folded into its BatchNorm pairs" % (self.ARCH, precision))
        self._lib = _lib.load()            # fails loudly when libnbc_hip.so is not built
        self.precision = precision
        self._prec = _PRECISIONS[precision]
        self.bn_statistics = "running"
        self._blob_host: Optional[np.ndarray] = None
        self._blob_dev: Optional[torch.Tensor] = None
        self._affine_host: Optional[np.ndarray] = None     # per-image BatchNorm gamma / beta (pack_bn_affine)
        self._affine_dev: Optional[torch.Tensor] = None
        self._raw_host: Optional[np.ndarray] = None        # "f16x2": the raw convolutions' powers of two (pack_bn_raw)
        self._raw_dev: Optional[torch.Tensor] = None
        self._ctx = C.c_void_p()
        self._lovasz_ws: Optional[torch.Tensor] = None     # nbc_lovasz_softmax's workspace (grows, never shrinks)
        self._pixel_ce_ws: Optional[torch.Tensor] = None   # nbc_pixel_cross_entropy's, likewise
        self._dropout_ws: Optional[torch.Tensor] = None    # nbc_dropout_draws', likewise
        self._zones_ws: Optional[torch.Tensor] = None      # nbc_label_zones', likewise
        self._zone_match_ws: Optional[torch.Tensor] = None   # nbc_match_zones', likewise
        self._contours_ws: Optional[torch.Tensor] = None   # nbc_contour_distances', likewise
        self._census_ws: Optional[torch.Tensor] = None     # nbc_softmax_census', likewise
        self._sweep_ws: Optional[torch.Tensor] = None      # nbc_offset_sweep's, likewise
        self._ce_grad_ws: Optional[torch.Tensor] = None    # nbc_ce_gradient's, likewise
        self._head_grad_ws: Optional[torch.Tensor] = None  # nbc_head_gradient's, likewise
        self._lovasz_grad_ws: Optional[torch.Tensor] = None  # nbc_lovasz_gradient's, likewise
        self._bicubic_taps: dict = {}                      # ce_gradient: the device tables of each (n_in, n_out)
        self._logit_offsets: Tuple[float, float] = (0.0, 0.0)   # set_logit_offsets: (bark, node), (0, 0) = off
        self._last_shape: Optional[Tuple[int, int, int]] = None   # (N, H, W) of the last forward (dropout_draws)
        self._frame_taps: dict = {}                        # training_frame: the device table of each frame length
        self.device: Optional[torch.device] = None
        self.training = False

    # ---- nn.Module-like surface ---------------------------------------------------------
    def load_state_dict(self, state_dict: Mapping[str, object], strict: bool = True):
        if not strict:
            raise NotImplementedError("only strict=True is supported (the reference never passes strict=False)")
        self._blob_host = pack_state_dict(state_dict, self.precision, self.ARCH)
        self._affine_host = pack_bn_affine(state_dict, self.ARCH)
        self._raw_host = pack_bn_raw(state_dict, self.ARCH)[0] if self._has_bn_raw() else None
        if self.device is not None:
            self._upload()
        return self

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("FCNResNet50 runs on MI355X only (device 'cuda[:i]'); the CPU path is the reference itself")
        index = device.index if device.index is not None else torch.cuda.current_device()
        device = torch.device("cuda", index)
        if self.device is not None and self.device != device:
            self._destroy()
        if not self._ctx:
            ctx = C.c_void_p()
            _lib.check(self._lib.nbc_create(C.byref(ctx), index), "nbc_create")
            self._ctx = ctx
            if self._logit_offsets != (0.0, 0.0):
                _lib.check(self._lib.nbc_set_logit_offsets(self._ctx, *self._logit_offsets), "nbc_set_logit_offsets")
        self.device = device
        if self._blob_host is not None:
            self._upload()
        return self

    def cuda(self, index: Optional[int] = None):
        return self.to(torch.device("cuda", index if index is not None else torch.cuda.current_device()))

    def eval(self):
        """No-op: the path is eval-only (BN running stats, Dropout identity); see ``set_bn_statistics`` for the
        per-image BatchNorm statistics of the shipped tool."""
        return self

    def set_bn_statistics(self, mode: str):
        """``"running"`` (default): BatchNorm on the checkpoint's running statistics, folded into the convolutions.
        ``"image"``: every BatchNorm uses the statistics of the image being run -- per-channel mean and biased variance over
        its H x W pixels, eps 1e-5, the checkpoint's gamma and beta: ``F.batch_norm(training=True)`` on a batch of one, what
        the shipped tool computes.  Nothing is updated (this is not training: ``train(True)`` stays refused), and an image's
        result does not depend on the batch it runs in.  "fp32" FCN-ResNet-50 only (``ValueError`` otherwise, before the
        device is touched); an image whose low-resolution map is 1 x 1 (e.g. 8 x 8) raises ``ValueError`` like torch does.
        ``"image_f16x2"``: the same statistics on an "f16x2" FCN-ResNet-50 (``ValueError`` on another precision): each raw
        convolution output is stored as pieces, normalised per channel by a power of two taken from the running statistics;
        ``nonfinite_seen`` is raised when an image's channel falls outside the range the pieces hold."""
        if mode not in BN_STATISTICS:
            raise ValueError(f"bn_statistics must be one of {sorted(BN_STATISTICS)}, got {mode!r}")
        if mode in PER_IMAGE_MODES:
            if topology.is_efficientnet(self.ARCH):
                raise ValueError("per-image BatchNorm statistics are refused for %s: they are implemented for fcn_resnet50 "
                                 "only" % self.ARCH)
            if self.ARCH != "fcn_resnet50":
                raise ValueError("per-image BatchNorm statistics are refused for %s: its ASPP pooling branch's BatchNorm sees a "
                                 "[1, 256, 1, 1] tensor, which batch statistics cannot normalise (torch raises, and so would "
                                 "the reference)" % self.ARCH)
            if mode == "image" and self._prec != _lib.PREC_FP32:
                raise ValueError("per-image BatchNorm statistics run in precision 'fp32' only, not %r" % self.precision)
            if mode == "image_f16x2" and self._prec != _lib.PREC_F16X2:
                raise ValueError("bn_statistics 'image_f16x2' runs in precision 'f16x2' only, not %r ('image' is the fp32 "
                                 "mode)" % self.precision)
        self.bn_statistics = mode
        if self._ctx:
            _lib.check(self._lib.nbc_set_bn_statistics(self._ctx, BN_STATISTICS[mode]), "nbc_set_bn_statistics")
        return self

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("training mode is not part of the inference path")
        return self

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """``self.model(x)`` of models.py:269: f32 ``[N,3,H,W]`` -> f32 logits ``[N,3,H,W]``."""
        n, h, w = self._check_input(x)
        logits = torch.empty((n, NUM_CLASSES, h, w), dtype=torch.float32, device=self.device)
        self._forward(x, n, h, w, logits_full=logits)
        return logits

    forward = __call__

    # ---- fused extras ---------------------------------------------------------------------
    def predict_labels(self, x: torch.Tensor, exclude_nodes: bool = False,
                       labels_dtype: torch.dtype = torch.int64,
                       return_lowres: bool = False, small_zones: bool = False,
                       logits_full: Optional[torch.Tensor] = None):
        """Model call + argmax (+ optional 2->1 remap) + per-class pixel counts in one pass.
        ``small_zones=True`` also applies ``remove_small_zones`` (models.py:271) on the device, before
        the remap like the reference does (models.py:271-276); the counts are those of the final labels.
        ``logits_full``: an optional contiguous f32 ``[N,3,H,W]`` tensor on this model's device that receives the logits
        ``self(x)`` returns, from the same forward (what ``lovasz_softmax`` reads).

        Returns ``(labels [N,H,W], counts int64 [N,3])`` (+ ``lowres f32 [N,3,h,w]``)."""
        n, h, w = self._check_input(x)
        if labels_dtype not in (torch.int64, torch.uint8):
            raise ValueError("labels_dtype must be torch.int64 or torch.uint8")
        if logits_full is not None and (logits_full.device != self.device or logits_full.dtype != torch.float32
                                        or not logits_full.is_contiguous()
                                        or tuple(logits_full.shape) != (n, NUM_CLASSES, h, w)):
            raise ValueError("logits_full must be a contiguous float32 [%d,%d,%d,%d] tensor on %s" % (n, NUM_CLASSES, h, w,
                                                                                                    self.device))
        labels = torch.empty((n, h, w), dtype=labels_dtype, device=self.device)
        counts = torch.empty((n, NUM_CLASSES), dtype=torch.int64, device=self.device)
        lowres = None
        if return_lowres:
            lh, lw = out_hw(h, w, self.ARCH)
            lowres = torch.empty((n, NUM_CLASSES, lh, lw), dtype=torch.float32, device=self.device)
        self._forward(x, n, h, w, labels=labels, counts=counts, lowres=lowres, logits_full=logits_full,
                      exclude_nodes=exclude_nodes and not small_zones)
        if small_zones:
            labels, counts = self.remove_small_zones(labels, exclude_nodes=exclude_nodes)
        return (labels, counts, lowres) if return_lowres else (labels, counts)

    # ---- the flip views the training augmented over (include/nbc.h) ---------
    def tta_views(self, x: torch.Tensor, views="flips") -> torch.Tensor:
        """The mirror images of a batch on the device (nbc_tta_views): ``x`` as the model takes it (f32 ``[N,3,H,W]`` or uint8
        ``[N,H,W,3]``) -> the stack ``[V*N, ...]`` in the same layout, view-major (entry ``j * N + i`` is view j of image i), the
        views of the mask ``views`` (``resolve_tta_views``) in ascending bit order.  Runs on the current stream."""
        self._require_ctx()
        mask = resolve_tta_views(views)
        x, f32, n, h, w = self._check_model_input(x)
        out = torch.empty((tta_view_count(mask) * n,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_tta_views(x.data_ptr(), _lib.IN_F32_NCHW if f32 else _lib.IN_U8_NHWC, n, h, w, mask,
                                               out.data_ptr(), cur.cuda_stream), "nbc_tta_views")
        return out

    def tta_merge(self, lowres_views: torch.Tensor, n: int, views="flips", return_aligned: bool = False):
        """The merged low-resolution logits of a stacked forward (nbc_tta_merge): ``lowres_views`` f32 ``[V*N,3,h,w]`` (or
        ``[V,N,3,h,w]``), view j's logits in view j's orientation -> ``m`` f32 ``[N,3,h,w]``, the mean of the un-flipped views
        (f32 adds in view order, one IEEE division); with ``return_aligned`` also the un-flipped views f32 ``[V,N,3,h,w]``."""
        self._require_ctx()
        mask = resolve_tta_views(views)
        v, n = tta_view_count(mask), int(n)
        if self._stack_entries(lowres_views, n) != v:
            raise ValueError("lowres_views must be a non-empty float32 [%d*%d,3,h,w] tensor on %s" % (v, n, self.device))
        lowres_views = lowres_views.contiguous()
        lh, lw = int(lowres_views.shape[-2]), int(lowres_views.shape[-1])
        merged = torch.empty((n, NUM_CLASSES, lh, lw), dtype=torch.float32, device=self.device)
        aligned = torch.empty((v, n, NUM_CLASSES, lh, lw), dtype=torch.float32, device=self.device) if return_aligned else None
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_tta_merge(lowres_views.data_ptr(), n, lh, lw, mask, merged.data_ptr(),
                                               aligned.data_ptr() if aligned is not None else None, cur.cuda_stream), "nbc_tta_merge")
        return (merged, aligned) if return_aligned else merged

    def vote_tally(self, labels: torch.Tensor, n: int) -> torch.Tensor:
        """The vote words of D label maps per image (nbc_vote_tally; the definition: csrc/votes.hpp): ``labels`` contiguous
        uint8 ``[D*N,H,W]`` (or ``[D,N,H,W]``), map-major -> ``[N,H,W]`` int32 holding the uint32 words (n1 in the low half, n2
        in the high half).  A label outside {0,1,2} votes nowhere.  ``nbc_vote_summary`` decides on them."""
        self._require_ctx()
        n = int(n)
        if labels.device != self.device or labels.dtype != torch.uint8 or not labels.is_contiguous() or labels.dim() not in (3, 4) \
                or labels.numel() == 0 or n < 1 or int(np.prod(labels.shape[:-2])) % n:
            raise ValueError("labels must be a non-empty contiguous uint8 [D*N,H,W] tensor on %s" % (self.device,))
        d = int(np.prod(labels.shape[:-2])) // n
        h, w = int(labels.shape[-2]), int(labels.shape[-1])
        words = torch.empty((n, h, w), dtype=torch.int32, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_vote_tally(labels.data_ptr(), n, d, h, w, words.data_ptr(), 0, cur.cuda_stream), "nbc_vote_tally")
        return words

    def predict_labels_tta(self, x: torch.Tensor, views="flips", exclude_nodes: bool = False,
                           labels_dtype: torch.dtype = torch.int64, small_zones: bool = False,
                           logits_full: Optional[torch.Tensor] = None, return_lowres: bool = False,
                           return_views: bool = False, min_pixels: int = 150):
        """``predict_labels`` on the mean of the flip views the training augmented over.  A composition of
        calls and nothing more: ``tta_views``, one forward of the V*N stack, ``tta_merge``, then today's tail on the merged
        low-resolution logits ``m`` -- ``upsample_argmax`` (into ``logits_full`` when given), ``remove_small_zones``
        (``small_zones``, threshold ``min_pixels``), the ``exclude_nodes`` remap, the counts.  ``views``: "hflip", "vflip",
        "flips" or a mask of ``_lib.TTA_*`` bits; the mask 1 gives ``predict_labels``' own bits.

        Returns what ``predict_labels`` returns, for ``m`` (``return_lowres`` appends ``m`` itself).  ``return_views`` appends
        ``(view_counts int64 [V,N,3], support uint8 [N,H,W], stats int64 [N,10], aligned f32 [V,N,3,h,w])``: each un-flipped
        view taken through the same tail on its own -- its pixels per class --, and the per-pixel vote of the V final label
        maps (``dropout_votes``' support byte and ten statistics, D = V).  Afterwards no forward counts as the last one:
        ``dropout_draws`` raises until a plain forward has run."""
        n, h, w = self._check_input(x)
        mask = resolve_tta_views(views)

        def merge(lowres_views):
            return self.tta_merge(lowres_views, n, mask, True) if return_views else (self.tta_merge(lowres_views, n, mask), None)
        return self._predict_stacked((n, h, w), tta_view_count(mask), "views", lambda: self.tta_views(x, mask), merge,
                                     exclude_nodes=exclude_nodes, labels_dtype=labels_dtype, small_zones=small_zones,
                                     logits_full=logits_full, return_lowres=return_lowres, min_pixels=min_pixels)

    def _predict_stacked(self, shape, count: int, what: str, make_stack, merge, frame=None, *, labels_dtype, min_pixels, logits_full,
                         **tail):
        """What ``predict_labels_tta``, ``predict_labels_jitter`` and ``predict_labels_windows`` share, for a checked batch of
        ``shape = (n, h, w)``: the checks of the arguments they have in common, ``make_stack()`` -- ``count`` views or windows
        (``what``) of every image, entry-major, each a ``frame`` (default ``h x w``) --, one forward of the ``count * n`` stack,
        ``merge(lowres f32 [count,n,3,lh,lw])`` -> ``(merged f32 [n,3,.,.], the views to take through the tail one by one or
        None)``, then ``_views_tail``."""
        n, h, w = shape
        if labels_dtype not in (torch.int64, torch.uint8):
            raise ValueError("labels_dtype must be torch.int64 or torch.uint8")
        if int(min_pixels) < 0:
            raise ValueError("min_pixels must not be negative")
        if count * n > 65535:
            raise ValueError("the stack of %d %s of %d images exceeds 65535 entries" % (count, what, n))
        if logits_full is not None and (logits_full.device != self.device or logits_full.dtype != torch.float32
                                        or not logits_full.is_contiguous()
                                        or tuple(logits_full.shape) != (n, NUM_CLASSES, h, w)):
            raise ValueError("logits_full must be a contiguous float32 [%d,%d,%d,%d] tensor on %s" % (n, NUM_CLASSES, h, w,
                                                                                                    self.device))
        fh, fw = frame or (h, w)
        stack = make_stack()
        lowres = torch.empty((count, n, NUM_CLASSES) + out_hw(fh, fw, self.ARCH), dtype=torch.float32, device=self.device)
        try:
            self._forward(stack, count * n, fh, fw, lowres=lowres)
        finally:
            self._last_shape = None                  # the context holds the stack's features, not a batch a caller knows
        merged, aligned = merge(lowres)
        return self._views_tail(merged, aligned, n, h, w, labels_dtype=labels_dtype, min_pixels=min_pixels,
                                logits_full=logits_full, **tail)

    def _views_tail(self, merged: torch.Tensor, aligned: Optional[torch.Tensor], n: int, h: int, w: int, exclude_nodes: bool,
                    labels_dtype: torch.dtype, small_zones: bool, logits_full: Optional[torch.Tensor], return_lowres: bool,
                    min_pixels: int):
        """What ``predict_labels_tta`` and ``predict_labels_jitter`` do once the views' low-resolution logits are merged: today's
        tail on ``merged`` f32 ``[N,3,h,w]`` and, when ``aligned`` f32 ``[V,N,3,h,w]`` is given, the same tail on each view and
        the vote of the V final label maps."""
        lh, lw = int(merged.shape[-2]), int(merged.shape[-1])
        v = int(aligned.shape[0]) if aligned is not None else 0
        return_views = aligned is not None
        remap_late = bool(small_zones)               # remove_small_zones comes before the remap (models.py:271-276)
        labels, counts = self.upsample_argmax(merged, (h, w), exclude_nodes=exclude_nodes and not remap_late,
                                              labels_dtype=labels_dtype, logits_full=logits_full)
        if small_zones:
            labels, counts = self.remove_small_zones(labels, exclude_nodes=exclude_nodes, min_pixels=min_pixels)
        out = (labels, counts) + ((merged,) if return_lowres else ())
        if not return_views:
            return out
        vlabels, vcounts = self.upsample_argmax(aligned.view(v * n, NUM_CLASSES, lh, lw), (h, w),
                                                exclude_nodes=exclude_nodes and not remap_late, labels_dtype=torch.uint8)
        if small_zones:
            vlabels, vcounts = self.remove_small_zones(vlabels, exclude_nodes=exclude_nodes, min_pixels=min_pixels)
        words = self.vote_tally(vlabels, n)
        support = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        stats = torch.empty((n, _lib.VOTE_STATS), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_vote_summary(words.data_ptr(), n, h, w, v, None, support.data_ptr(), stats.data_ptr(),
                                                  cur.cuda_stream), "nbc_vote_summary")
        return out + (vcounts.view(v, n, NUM_CLASSES), support, stats, aligned)

    # ---- the colour-jitter views the training augmented over (include/nbc.h) ---------
    def jitter_views(self, x_u8: torch.Tensor, views="training") -> torch.Tensor:
        """The colour views of a batch on the device (nbc_jitter_views): ``x_u8`` uint8 ``[N,H,W,3]`` -> the stack uint8
        ``[V*N,H,W,3]``, view-major (entry ``j * N + i`` is view j of image i), the views of ``views``
        (``resolve_jitter_views``) in the order given.  Runs on the current stream."""
        factors = resolve_jitter_views(views)
        if isinstance(x_u8, torch.Tensor) and x_u8.dtype == torch.float32:
            raise ValueError("the colour views are made of uint8 [N,H,W,3] frames: a float32 input is refused (torchvision's "
                             "tensor path is other arithmetic)")
        self._require_ctx()
        if not isinstance(x_u8, torch.Tensor) or x_u8.device != self.device or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 \
                or x_u8.numel() == 0 or x_u8.shape[3] != 3:
            raise ValueError("x must be a non-empty uint8 [N,H,W,3] tensor on %s" % (self.device,))
        x_u8 = x_u8.contiguous()
        n, h, w = int(x_u8.shape[0]), int(x_u8.shape[1]), int(x_u8.shape[2])
        v = int(factors.shape[0])
        if v * n > 65535:
            raise ValueError("the stack of %d views of %d images exceeds 65535 entries" % (v, n))
        out = torch.empty((v * n, h, w, 3), dtype=torch.uint8, device=self.device)
        ws = torch.empty((v * n,), dtype=torch.int64, device=self.device)      # nbc_jitter_workspace_bytes: 8 V N
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_jitter_views(x_u8.data_ptr(), n, h, w, factors.ctypes.data, v, out.data_ptr(), ws.data_ptr(),
                                                  cur.cuda_stream), "nbc_jitter_views")
        return out

    def views_mean(self, lowres_views: torch.Tensor, n: int) -> torch.Tensor:
        """The mean of the low-resolution logits of a stacked forward (nbc_views_mean): ``lowres_views`` f32 ``[V*N,3,h,w]`` (or
        ``[V,N,3,h,w]``) -> ``m`` f32 ``[N,3,h,w]``: f32 adds in view order, one IEEE division; V = 1 keeps the view's bits."""
        self._require_ctx()
        n = int(n)
        v = self._stack_entries(lowres_views, n)
        if not 1 <= v <= _lib.JITTER_MAX_VIEWS:
            raise ValueError("lowres_views must be a non-empty float32 [V*%d,3,h,w] tensor on %s, V in 1..%d" % (
                n, self.device, _lib.JITTER_MAX_VIEWS))
        lowres_views = lowres_views.contiguous()
        lh, lw = int(lowres_views.shape[-2]), int(lowres_views.shape[-1])
        mean = torch.empty((n, NUM_CLASSES, lh, lw), dtype=torch.float32, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_views_mean(lowres_views.data_ptr(), n, v, lh, lw, mean.data_ptr(), cur.cuda_stream),
                       "nbc_views_mean")
        return mean

    def predict_labels_jitter(self, x: torch.Tensor, views="training", exclude_nodes: bool = False,
                              labels_dtype: torch.dtype = torch.int64, small_zones: bool = False,
                              logits_full: Optional[torch.Tensor] = None, return_lowres: bool = False,
                              return_views: bool = False, min_pixels: int = 150):
        """``predict_labels`` on the mean of the colour-jitter views the training augmented over.  A
        composition of calls and nothing more: ``jitter_views``, one forward of the V*N stack, ``views_mean``, then today's tail
        on the mean ``m`` of the low-resolution logits, as ``predict_labels_tta`` runs it.  ``x``: uint8 ``[N,H,W,3]`` (a
        float32 input is a ``ValueError``); ``views``: "training" or 1..16 (brightness, contrast, saturation) triples; the set
        ``[(1, 1, 1)]`` gives ``predict_labels``' own bits.

        Returns what ``predict_labels_tta`` returns: ``(labels, counts)`` for ``m`` (``return_lowres`` appends ``m``), and with
        ``return_views`` also ``(view_counts int64 [V,N,3], support uint8 [N,H,W], stats int64 [N,10], the views' low-resolution
        logits f32 [V,N,3,h,w])``.  Afterwards no forward counts as the last one: ``dropout_draws`` raises until a plain forward
        has run."""
        factors = resolve_jitter_views(views)
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
            raise ValueError("predict_labels_jitter takes uint8 [N,H,W,3] frames: a float32 input is refused (torchvision's "
                             "tensor path is other arithmetic)")
        n, h, w = self._check_input(x)
        return self._predict_stacked((n, h, w), int(factors.shape[0]), "views", lambda: self.jitter_views(x, factors),
                                     lambda lowres_views: (self.views_mean(lowres_views, n), lowres_views if return_views else None),
                                     exclude_nodes=exclude_nodes, labels_dtype=labels_dtype, small_zones=small_zones,
                                     logits_full=logits_full, return_lowres=return_lowres, min_pixels=min_pixels)

    # ---- the crop windows the training augmented over (include/nbc.h) ---------
    def window_grid(self, h: int, w: int, window: int = 512, stride: int = 256):
        """``model.window_grid``: ``(E_y, E_x, n_y, n_x, offsets_y, offsets_x)`` of an ``h x w`` frame."""
        return window_grid(h, w, window, stride)

    def _check_windows_served(self):
        if topology.is_efficientnet(self.ARCH):
            raise ValueError("the crop windows are refused for %s: its output stride is 32 and its fixed asymmetric pads need a "
                             "window grid of their own (left out, DESIGN.md 3.18)" % self.ARCH)
        if self.bn_statistics in PER_IMAGE_MODES:
            raise ValueError("the crop windows are refused under bn_statistics %r: statistics per window are not the shipped "
                             "tool's per-frame statistics" % self.bn_statistics)

    def window_views(self, x: torch.Tensor, window: int = 512, stride: int = 256) -> torch.Tensor:
        """The windows of a batch on the device (nbc_window_views): ``x`` as the model takes it (f32 ``[N,3,H,W]`` or uint8
        ``[N,H,W,3]``) -> the stack ``[K*N, ...]`` of ``E_y x E_x`` windows in the same layout, window-major (entry ``k * N + i``
        is window k of image i), rows and columns beyond the frame filled by reflection.  Runs on the current stream."""
        self._require_ctx()
        x, f32, n, h, w = self._check_model_input(x)
        ey, ex, ny, nx, _, _ = window_grid(h, w, window, stride)
        if ny * nx * n > 65535:
            raise ValueError("the stack of %d windows of %d images exceeds 65535 entries" % (ny * nx, n))
        out = torch.empty((ny * nx * n,) + ((3, ey, ex) if f32 else (ey, ex, 3)), dtype=x.dtype, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_window_views(x.data_ptr(), _lib.IN_F32_NCHW if f32 else _lib.IN_U8_NHWC, n, h, w, int(window),
                                                  int(stride), out.data_ptr(), cur.cuda_stream), "nbc_window_views")
        return out

    def window_merge(self, lowres_windows: torch.Tensor, n: int, h: int, w: int, window: int = 512, stride: int = 256,
                     blend: str = "tent") -> torch.Tensor:
        """The merged low-resolution logits of a stacked forward (nbc_window_merge): ``lowres_windows`` f32
        ``[K*N,3,E_y/8,E_x/8]`` (or ``[K,N,...]``) of the windows of ``n`` frames of ``h x w`` pixels -> ``m`` f32
        ``[N,3,ceil(h/8),ceil(w/8)]``, per cell the weighted mean of the windows that cover it (``blend``: "tent" or "uniform")
        in ascending window order; a cell one window covers keeps that window's bits."""
        self._require_ctx()
        b = resolve_window_blend(blend)
        n, h, w = int(n), int(h), int(w)
        ey, ex, ny, nx, _, _ = window_grid(h, w, window, stride)
        k = ny * nx
        if self._stack_entries(lowres_windows, n) != k or tuple(lowres_windows.shape[-2:]) != (ey // 8, ex // 8):
            raise ValueError("lowres_windows must be a float32 [%d*%d,3,%d,%d] tensor on %s" % (k, n, ey // 8, ex // 8, self.device))
        if k * n > 65535:
            raise ValueError("the stack of %d windows of %d images exceeds 65535 entries" % (k, n))
        lowres_windows = lowres_windows.contiguous()
        merged = torch.empty((n, NUM_CLASSES, (h + 7) // 8, (w + 7) // 8), dtype=torch.float32, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_window_merge(lowres_windows.data_ptr(), n, h, w, int(window), int(stride), b,
                                                  merged.data_ptr(), cur.cuda_stream), "nbc_window_merge")
        return merged

    # ---- the training run's own frame (include/nbc.h) ---------------------------
    def _frame_table(self, lt: int) -> torch.Tensor:
        """The device table of a resampled axis of frame length ``lt`` (int32 ``[lt, 4]``: first, three coefficients), built
        through nbc_bilinear_taps and uploaded once per length."""
        table = self._frame_taps.get(lt)
        if table is None:
            from .training_frame import table_of
            table = torch.from_numpy(table_of(*bilinear_taps(lt + 1, lt))).to(self.device)
            self._frame_taps[lt] = table
        return table

    def training_frame(self, x_u8: torch.Tensor, size=(1024, 1024)) -> torch.Tensor:
        """The training run's frame of a batch (nbc_training_frame): ``pad_resize(img, *size)`` of utils.py:242-247 on uint8
        ``[N,H,W,3]`` frames or ``[N,H,W]`` grey duals on the device -> uint8 ``[N,Ht,Wt,3]`` or ``[N,Ht,Wt]``, byte for byte
        ``training_frame.pad_resize_cpu`` of each image.  Runs on the current stream; the coefficient tables of the resampled
        axes are cached on the device per frame length.  ``ValueError`` for anything but such a tensor on the model's device, a
        source longer than the frame on an axis, or a pad that one reflection does not reach."""
        self._require_ctx()
        if not isinstance(x_u8, torch.Tensor) or x_u8.device != self.device or x_u8.dtype != torch.uint8 or x_u8.numel() == 0 \
                or not (x_u8.dim() == 3 or (x_u8.dim() == 4 and x_u8.shape[3] == 3)):
            raise ValueError("x_u8 must be a non-empty uint8 [N,H,W,3] or [N,H,W] tensor on %s" % (self.device,))
        from .training_frame import frame_geometry
        try:
            ht, wt = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("size must be (Ht, Wt), got %r" % (size,))
        x = x_u8.contiguous()
        n, h, w = (int(v) for v in x.shape[:3])
        channels = 3 if x.dim() == 4 else 1
        if n > 65535 or ht < 1 or wt < 1 or ht * wt >= 2 ** 31:
            raise ValueError("training_frame: N <= 65535 and Ht * Wt < 2^31, got N = %d, size %r" % (n, (ht, wt)))
        (_, hp), (_, wp) = frame_geometry(h, ht), frame_geometry(w, wt)
        rows = self._frame_table(ht) if hp != ht else None
        cols = self._frame_table(wt) if wp != wt else None
        out = torch.empty((n, ht, wt) + ((3,) if channels == 3 else ()), dtype=torch.uint8, device=self.device)
        with self._on_stream() as cur:
            for t in (rows, cols):
                if t is not None:
                    t.record_stream(cur)
            _lib.check(self._lib.nbc_training_frame(x.data_ptr(), channels, n, h, w, ht, wt,
                                                    rows.data_ptr() if rows is not None else None,
                                                    cols.data_ptr() if cols is not None else None, out.data_ptr(),
                                                    cur.cuda_stream), "nbc_training_frame")
        return out

    def predict_labels_windows(self, x: torch.Tensor, window: int = 512, stride: int = 256, blend: str = "tent",
                               exclude_nodes: bool = False, labels_dtype: torch.dtype = torch.int64, small_zones: bool = False,
                               logits_full: Optional[torch.Tensor] = None, return_lowres: bool = False, min_pixels: int = 150):
        """``predict_labels`` on sliding windows of the training's crop size, blended over their overlaps.  A
        composition of calls and nothing more: ``window_views``, one forward of the K*N stack at ``E_y x E_x``,
        ``window_merge``, then today's tail on the merged low-resolution logits ``m``, as ``predict_labels_tta`` runs it.  A frame
        whose sides are multiples of 8 and no longer than ``window`` gives ``predict_labels``' own bits.

        Returns what ``predict_labels`` returns, for ``m`` (``return_lowres`` appends ``m`` itself).  Refused (``ValueError``):
        the EfficientNet networks and per-image BatchNorm statistics.  Afterwards no forward counts as the last one:
        ``dropout_draws`` raises until a plain forward has run."""
        self._check_windows_served()
        resolve_window_blend(blend)
        n, h, w = self._check_input(x)
        ey, ex, ny, nx, _, _ = window_grid(h, w, window, stride)
        return self._predict_stacked((n, h, w), ny * nx, "windows", lambda: self.window_views(x, window, stride),
                                     lambda lowres_windows: (self.window_merge(lowres_windows, n, h, w, window, stride, blend), None),
                                     frame=(ey, ex), exclude_nodes=exclude_nodes, labels_dtype=labels_dtype, small_zones=small_zones,
                                     logits_full=logits_full, return_lowres=return_lowres, min_pixels=min_pixels)

    def lowres_logits(self, x: torch.Tensor) -> torch.Tensor:
        """Output of ``classifier.4`` (models.py:121) before the upsample: f32 ``[N,3,h,w]``."""
        n, h, w = self._check_input(x)
        lh, lw = out_hw(h, w, self.ARCH)
        lowres = torch.empty((n, NUM_CLASSES, lh, lw), dtype=torch.float32, device=self.device)
        self._forward(x, n, h, w, lowres=lowres)
        return lowres

    def remove_small_zones(self, labels: torch.Tensor, exclude_nodes: bool = False, min_pixels: int = 150):
        """``utils.remove_small_zones`` (utils.py:135-148, called at models.py:271) on the device, IN PLACE
        on ``labels`` (uint8 or int64 ``[N,H,W]`` / ``[H,W]`` on this model's device): 8-connected zones
        of fewer than ``min_pixels`` pixels of the non-background, then of the filled background, flip
        (class 0 <-> class 1).  ``exclude_nodes`` applies the 2 -> 1 remap of models.py:273-276
        afterwards.  Returns ``(labels, counts int64 [N,3])`` with the pixels per class of the result."""
        self._require_ctx()
        self._check_labels(labels)
        if labels.dim() not in (2, 3):
            raise ValueError("labels must be [H,W] or [N,H,W]")
        n, h, w = self._batch_hw(labels)
        counts = torch.empty((n, 3), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_remove_small_zones(self._ctx, labels.data_ptr(), self._label_code(labels),
                                                        n, h, w, int(min_pixels), int(bool(exclude_nodes)),
                                                        counts.data_ptr(), cur.cuda_stream), "nbc_remove_small_zones")
        return labels, counts

    def remove_small_zones_groups(self, labels: torch.Tensor, group: int, min_pixels: int = 150):
        """``utils.remove_small_zones`` on batches as the reference's ``PixelWiseF1`` runs it (utils.py:211-214) on the device
        (nbc_remove_small_zones_groups), IN PLACE on ``labels`` (contiguous uint8 or int64 ``[N,H,W]`` on this model's
        device): consecutive groups of ``group`` images (the last may be shorter) are volumes in which a pixel also touches
        the pixel at its place in the image before and after and that pixel's four edge neighbours (skimage's
        ``connectivity=2`` on a 3-D array), and ``min_pixels`` counts a zone over all its images.  ``group`` in 1..64 with
        ``min(group, N) * H * W < 2^31``; 1 is ``remove_small_zones``.  Runs on the current stream; the workspace is the
        context's.  Returns ``(labels, counts int64 [N,3])`` with the pixels per class of every image of the result."""
        self._require_ctx()
        self._check_labels(labels)
        if labels.dim() != 3 or labels.numel() == 0:
            raise ValueError("labels must be a non-empty [N,H,W]")
        n, h, w = (int(v) for v in labels.shape)
        group = self._check_group(group, n, h, w)
        if int(min_pixels) < 0:
            raise ValueError("min_pixels must be >= 0, got %r" % (min_pixels,))
        counts = torch.empty((n, 3), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_remove_small_zones_groups(self._ctx, labels.data_ptr(), self._label_code(labels),
                                                               n, h, w, group, int(min_pixels), counts.data_ptr(), cur.cuda_stream),
                       "nbc_remove_small_zones_groups")
        return labels, counts

    @staticmethod
    def _check_group(group, n: int, h: int, w: int) -> int:
        """``group`` as the grouped passes take it: an int in 1..64 whose volume of ``min(group, n)`` images is indexable."""
        if isinstance(group, bool) or not isinstance(group, int) or not 1 <= group <= 64:
            raise ValueError("group must be an int in 1..64, got %r" % (group,))
        if min(group, n) * h * w >= 2 ** 31:
            raise ValueError("a group of %d [%d,%d] images has 2^31 pixels or more" % (min(group, n), h, w))
        return group

    def label_zones(self, labels: torch.Tensor, cap: int = 1024) -> Tuple[torch.Tensor, torch.Tensor]:
        """The zones of label maps on the device (nbc_label_zones; include/nbc.h, csrc/zones.hip): the 8-connected components
        of each class in {1, 2}, one row of ten integers per zone (``zones.ZONE_FIELDS``: first pixel ``y * W + x``, class,
        pixels, inclusive box x0 y0 x1 y1, sum_x, sum_y, perimeter), sorted by first pixel.  ``labels``: contiguous uint8 or
        int64 ``[N,H,W]`` / ``[H,W]`` on this model's device, read only.  Runs on the current stream; the workspace (5 bytes
        per pixel) is cached on this object and only grows.  Returns ``(rows int64 [N,cap,10], num int64 [N])``: ``num[n]`` is
        the number of zones of image n, also when it exceeds ``cap``; rows ``min(num[n], cap)`` onwards are not written.
        Equal to ``zones.zones_cpu``, integer for integer; works for every architecture, since it only sees labels."""
        self._require_ctx()
        self._check_labels(labels)
        if labels.dim() not in (2, 3) or labels.numel() == 0:
            raise ValueError("labels must be a non-empty [H,W] or [N,H,W]")
        cap = int(cap)
        if cap < 1:
            raise ValueError("cap must be at least 1")
        n, h, w = self._batch_hw(labels)
        need = int(self._lib.nbc_zones_workspace_bytes(n, h, w))
        if need == 0:
            raise ValueError("nbc_label_zones refuses a [%d,%d,%d] batch (N <= 65535, H, W <= 65535, H * W < 2^31)" % (n, h, w))
        rows = torch.empty((n, cap, _lib.ZONE_ROW), dtype=torch.int64, device=self.device)
        num = torch.empty((n,), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_zones_ws", need, cur)
            _lib.check(self._lib.nbc_label_zones(self._ctx, labels.data_ptr(), self._label_code(labels), n, h, w,
                                                 rows.data_ptr(), cap, num.data_ptr(), ws.data_ptr(), ws.numel(), cur.cuda_stream),
                       "nbc_label_zones")
        return rows, num

    def match_zones(self, labels: torch.Tensor, target: torch.Tensor, cap: int = 1024, pair_cap: int = 2048):
        """The zones of label maps against the zones of their labelled masks on the device (nbc_match_zones; include/nbc.h,
        csrc/zone_match.hip).  ``labels`` as ``label_zones`` takes them, ``target`` the contiguous uint8 grey mask of the same
        shape as ``confusion`` takes it (class ``round(2 * v / 255)``); both read only.  Runs on the current stream; the
        workspace (11 bytes per pixel) is cached on this object and only grows.  Returns six int64 tensors ``(out_rows [N,cap,10],
        out_num [N], tgt_rows [N,cap,10], tgt_num [N], pair_rows [N,pair_cap,3], pair_num [N])``: both inventories as
        ``label_zones`` gives them, and per image the rows ``(output zone index, target zone index, shared pixels)`` of every
        pair of same-class zones that share a pixel, sorted, the indices being the zones' positions in first-pixel order
        (valid also at or above ``cap``).  ``pair_num[n]`` is the number of pairs, or ``pair_cap + 1`` when there are more
        (the image's pair rows are then unspecified); rows ``pair_num[n]`` onwards are not written.  Equal to
        ``zones.match_cpu``, integer for integer; works for every architecture, since it only sees labels."""
        self._require_ctx()
        self._check_labels(labels)
        self._check_target_like(labels, target)
        cap, pair_cap = int(cap), int(pair_cap)
        if cap < 1:
            raise ValueError("cap must be at least 1")
        if not 1 <= pair_cap <= _lib.PAIRS_MAX_CAP:
            raise ValueError("pair_cap must lie in 1..%d" % _lib.PAIRS_MAX_CAP)
        n, h, w = self._batch_hw(labels)
        need = int(self._lib.nbc_zone_match_workspace_bytes(n, h, w, pair_cap))
        if need == 0:
            raise ValueError("nbc_match_zones refuses a [%d,%d,%d] batch (N <= 65535, H, W <= 65535, H * W < 2^31)" % (n, h, w))
        out_rows, tgt_rows = (torch.empty((n, cap, _lib.ZONE_ROW), dtype=torch.int64, device=self.device) for _ in range(2))
        pair_rows = torch.empty((n, pair_cap, _lib.ZONE_PAIR_ROW), dtype=torch.int64, device=self.device)
        out_num, tgt_num, pair_num = (torch.empty((n,), dtype=torch.int64, device=self.device) for _ in range(3))
        with self._on_stream() as cur:
            ws = self._grown_workspace("_zone_match_ws", need, cur)
            _lib.check(self._lib.nbc_match_zones(self._ctx, labels.data_ptr(), self._label_code(labels), target.data_ptr(),
                                                 n, h, w, out_rows.data_ptr(), out_num.data_ptr(), tgt_rows.data_ptr(),
                                                 tgt_num.data_ptr(), cap, pair_rows.data_ptr(), pair_num.data_ptr(), pair_cap,
                                                 ws.data_ptr(), ws.numel(), cur.cuda_stream), "nbc_match_zones")
        return out_rows, out_num, tgt_rows, tgt_num, pair_rows, pair_num

    def contour_distances(self, labels: torch.Tensor, target: torch.Tensor, bins: Optional[int] = None):
        """How far the contours of label maps lie from the contours of their labelled masks, on the device
        (nbc_contour_distances; include/nbc.h, csrc/contours.hip).  ``labels`` as ``label_zones`` takes them, ``target`` the
        contiguous uint8 grey mask of the same shape as ``confusion`` takes it; both read only, H and W at most 4096.  Runs on
        the current stream; the workspace (9 bytes per pixel) is cached on this object and only grows.  Returns ``(rows int64
        [N,4,4+bins], sum_d float64 [N,4])``: per image and set (Bark output to target, Bark target to output, the same two of
        Node) the source and destination contour pixels, the sum and the maximum of the squared distances, the histogram of
        the distances rounded up to whole pixels, and the sum of the distances.  ``bins=None``: ``ceil(hypot(H-1, W-1)) + 1``,
        with which the last bin is no overflow bin.  The rows equal ``contours.contours_cpu`` integer for integer; an image's
        outputs have the same bits alone and in any batch.  Works for every architecture, since it only sees labels."""
        from . import contours as ct
        self._require_ctx()
        self._check_labels(labels)
        self._check_target_like(labels, target)
        n, h, w = self._batch_hw(labels)
        need = int(self._lib.nbc_contours_workspace_bytes(n, h, w))
        if need == 0:
            raise ValueError("nbc_contour_distances refuses a [%d,%d,%d] batch (N <= 65535, H, W <= %d)" % (n, h, w, ct.MAX_SIDE))
        bins = ct.default_bins(h, w) if bins is None else int(bins)
        if not 2 <= bins <= ct.MAX_BINS:
            raise ValueError("bins must lie in 2..%d" % ct.MAX_BINS)
        rows = torch.empty((n, _lib.CONTOUR_SETS, _lib.CONTOUR_HEAD + bins), dtype=torch.int64, device=self.device)
        sum_d = torch.empty((n, _lib.CONTOUR_SETS), dtype=torch.float64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_contours_ws", need, cur)
            _lib.check(self._lib.nbc_contour_distances(self._ctx, labels.data_ptr(), self._label_code(labels),
                                                       target.data_ptr(), n, h, w, rows.data_ptr(), bins, sum_d.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), cur.cuda_stream), "nbc_contour_distances")
        return rows, sum_d

    def confusion(self, labels: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """Per-image 3x3 confusion counts on the device (nbc_confusion): the pixel counting behind the evaluation loop's
        ``iou`` and ``PixelWiseF1`` (__main__.py:331-332).  ``labels``: contiguous uint8 or int64 ``[N,H,W]`` / ``[H,W]``
        with values in {0,1,2} (others are counted nowhere); ``target``: contiguous uint8 grey mask of the same shape, class
        ``round(2 * v / 255)`` (dataset.py:189-197); both on this model's device.  Runs on the current stream.  Returns int64
        ``[N,3,3]``: ``conf[n, t, p]`` = pixels of target class t predicted as p."""
        self._require_ctx()
        self._check_labels(labels)
        self._check_target_like(labels, target)
        n, h, w = self._batch_hw(labels)
        conf = torch.empty((n, NUM_CLASSES, NUM_CLASSES), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_confusion(labels.data_ptr(), self._label_code(labels),
                                               target.data_ptr(), n, h, w, conf.data_ptr(), cur.cuda_stream), "nbc_confusion")
        return conf

    def lovasz_softmax(self, logits_full: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-image Lovasz-Softmax terms on the device (nbc_lovasz_softmax): ``LovaszSoftmax()(logits, target)``
        (lovasz_losses.py:162-223), the training objective of __main__.py:236-239, for each image as a batch of one.
        ``logits_full``: contiguous f32 ``[N,3,H,W]`` (``self(x)``, or ``predict_labels(..., logits_full=)``); ``target``:
        contiguous uint8 grey mask ``[N,H,W]``, class ``round(2 * v / 255)`` as ``confusion`` reads it; both on this model's
        device.  Runs on the current stream; the workspace is cached on this object and only grows.  Returns
        ``(terms f64 [N,3], fg_counts int64 [N,3])``: the term of each class (0 for an absent class, whose fg_count is 0;
        NaN for every present class of an image whose softmax is not finite somewhere); ``metrics.lovasz_loss`` takes the
        mean over the present classes."""
        self._require_ctx()
        n, h, w = self._check_logits_target(logits_full, target)
        need = int(self._lib.nbc_lovasz_workspace_bytes(n, h, w))
        if need == 0:
            raise ValueError("nbc_lovasz_softmax refuses a [%d,3,%d,%d] batch (N <= 65535, H * W < 2^31)" % (n, h, w))
        terms = torch.empty((n, NUM_CLASSES), dtype=torch.float64, device=self.device)
        fg_counts = torch.empty((n, NUM_CLASSES), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_lovasz_ws", need, cur)
            _lib.check(self._lib.nbc_lovasz_softmax(logits_full.data_ptr(), target.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(),
                                                    terms.data_ptr(), fg_counts.data_ptr(), cur.cuda_stream), "nbc_lovasz_softmax")
        return terms, fg_counts

    def lovasz_softmax_groups(self, logits_full: torch.Tensor, target: torch.Tensor, group: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The Lovasz-Softmax terms of batches on the device (nbc_lovasz_softmax_groups): ``LovaszSoftmax()`` on a batch runs
        with ``per_image=False`` (lovasz_losses.py:169-191) and sorts the errors of all its images together, per class --
        ``val_loss`` / ``test_loss`` of the training log.  ``logits_full`` and ``target`` as ``lovasz_softmax`` takes them;
        images form consecutive groups of ``group`` (1..64, the last may be shorter).  Runs on the current stream; shares
        ``lovasz_softmax``'s cached workspace.  Returns ``(terms f64 [NG,3], counts int64 [NG,3])`` for the ``NG =
        ceil(N / group)`` groups: a group's terms are bit for bit ``lovasz_softmax`` of its images stacked along the height; a
        class present in one image is present for its group; a non-finite softmax makes its own group's terms NaN.
        ``metrics.lovasz_loss`` takes a group's mean over the present classes."""
        self._require_ctx()
        n, h, w = self._check_logits_target(logits_full, target)
        group = self._check_group(group, n, h, w)
        need = int(self._lib.nbc_lovasz_groups_workspace_bytes(n, h, w, group))
        if need == 0:
            raise ValueError("nbc_lovasz_softmax_groups refuses a [%d,3,%d,%d] batch in groups of %d (N <= 65535, g * H * W < 2^31)"
                             % (n, h, w, group))
        ng = (n + group - 1) // group
        terms = torch.empty((ng, NUM_CLASSES), dtype=torch.float64, device=self.device)
        counts = torch.empty((ng, NUM_CLASSES), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_lovasz_ws", need, cur)
            _lib.check(self._lib.nbc_lovasz_softmax_groups(logits_full.data_ptr(), target.data_ptr(), n, h, w, group, ws.data_ptr(),
                                                           ws.numel(), terms.data_ptr(), counts.data_ptr(), cur.cuda_stream),
                       "nbc_lovasz_softmax_groups")
        return terms, counts

    def pixel_cross_entropy(self, logits_full: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-image cross-entropy sums on the device (nbc_pixel_cross_entropy): what ``CustomWeightedCrossEntropy``
        (utils.py:151-165), the plain cross-entropy and ``MixedLoss`` (utils.py:185-192) need from the pixels, for each image
        as a batch of one.  ``logits_full`` and ``target`` as ``lovasz_softmax`` takes them.  Runs on the current stream; the
        workspace is cached on this object and only grows.  Returns ``(sums f64 [N,3,3], counts int64 [N,3,3])``:
        ``sums[n, t, p]`` = the sum of ``logsumexp(x) - x[t]`` over the pixels of target class t whose argmax is p,
        ``counts[n, t, p]`` their number (the raw ``confusion`` of the same forward).  ``metrics.cross_entropy``,
        ``weighted_cross_entropy`` and ``mixed_loss`` turn them into the losses, for any class weights."""
        self._require_ctx()
        n, h, w = self._check_logits_target(logits_full, target)
        need = int(self._lib.nbc_pixel_ce_workspace_bytes(n, h, w))
        if need == 0:
            raise ValueError("nbc_pixel_cross_entropy refuses a [%d,3,%d,%d] batch (N <= 65535, H * W < 2^31)" % (n, h, w))
        sums = torch.empty((n, NUM_CLASSES, NUM_CLASSES), dtype=torch.float64, device=self.device)
        counts = torch.empty((n, NUM_CLASSES, NUM_CLASSES), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_pixel_ce_ws", need, cur)
            _lib.check(self._lib.nbc_pixel_cross_entropy(logits_full.data_ptr(), target.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(),
                                                         sums.data_ptr(), counts.data_ptr(), cur.cuda_stream),
                       "nbc_pixel_cross_entropy")
        return sums, counts

    # ---- the refit of classifier.4 (include/nbc.h; the driver: refit.py) -------------------------------------
    def _refit_theta(self, theta) -> torch.Tensor:
        """theta as 1 539 contiguous float32 on this device: ``classifier.4.weight`` [3, 512] then ``classifier.4.bias`` [3]."""
        t = theta if isinstance(theta, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(theta))
        if t.dtype != torch.float32 or t.numel() != NUM_CLASSES * 513:
            raise ValueError("theta must hold 1539 float32 (classifier.4.weight [3,512], then classifier.4.bias [3])")
        return t.reshape(-1).to(self.device).contiguous()

    def _refit_last_shape(self, what: str) -> Tuple[int, int, int]:
        self._require_weights()
        if self._last_shape is None:
            raise RuntimeError("%s follows a forward (predict_labels / lowres_logits) of this object: none has run" % what)
        return self._last_shape

    def head_logits(self, theta) -> torch.Tensor:
        """``classifier.4`` with the parameters ``theta`` (1 539 float32 in the state_dict's units: the weight [3, 512], then the
        bias) on the features the LAST forward of this object left on the device (nbc_head_logits), on the current stream.
        Returns the low-resolution logits f32 ``[N,3,h,w]``; with the checkpoint's own values they are bit for bit the
        forward's.  ``RuntimeError``: no forward has run, its plan has been touched since, or another network than
        fcn_resnet50."""
        n, h, w = self._refit_last_shape("head_logits")
        th = self._refit_theta(theta)
        out = torch.empty((n, NUM_CLASSES) + out_hw(h, w, self.ARCH), dtype=torch.float32, device=self.device)
        with self._on_stream() as cur:
            rc = self._lib.nbc_head_logits(self._ctx, th.data_ptr(), n, h, w, out.data_ptr(), cur.cuda_stream)
        _lib.check(rc, "nbc_head_logits")
        return out

    def _taps_on_device(self, n_in: int, n_out: int):
        key = (int(n_in), int(n_out))
        if key not in self._bicubic_taps:
            self._bicubic_taps[key] = tuple(torch.from_numpy(a).to(self.device) for a in bicubic_taps(*key))
        return self._bicubic_taps[key]

    def ce_gradient(self, logits_full: torch.Tensor, target: torch.Tensor, lowres_size, table) -> torch.Tensor:
        """The gradient of ``sum T[t][p] ce`` of each image with respect to its low-resolution logits (nbc_ce_gradient):
        ``g_c = T[t][p] (softmax_c - [c = t])`` per pixel in f64, then the adjoint of the bicubic upsample ``lowres_size`` ->
        ``(H, W)`` with the tables of ``bicubic_taps`` (uploaded once per length).  ``logits_full`` and ``target`` as
        ``pixel_cross_entropy`` takes them; ``table``: nine numbers ``T[target class][argmax class]``.  Returns f64
        ``[N,3,h,w]``, not normalised; on the current stream."""
        self._require_ctx()
        n, h, w = self._check_logits_target(logits_full, target)
        lh, lw = int(lowres_size[0]), int(lowres_size[1])
        tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
        if tab.size != 9:
            raise ValueError("table must hold nine numbers T[target class][argmax class]")
        need = int(self._lib.nbc_ce_gradient_workspace_bytes(n, h, w, lh, lw))
        if need == 0:
            raise ValueError("nbc_ce_gradient refuses a [%d,3,%d,%d] batch with a %dx%d low-resolution map (N <= 65535, H * W < 2^31, "
                             "1 <= h <= H, 1 <= w <= W)" % (n, h, w, lh, lw))
        rows, cols = self._taps_on_device(lh, h), self._taps_on_device(lw, w)
        out = torch.empty((n, NUM_CLASSES, lh, lw), dtype=torch.float64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_ce_grad_ws", need, cur)
            rc = self._lib.nbc_ce_gradient(logits_full.data_ptr(), target.data_ptr(), n, h, w, lh, lw,
                                           *[t.data_ptr() for t in rows + cols], tab.ctypes.data_as(C.POINTER(C.c_double)),
                                           ws.data_ptr(), ws.numel(), out.data_ptr(), cur.cuda_stream)
        _lib.check(rc, "nbc_ce_gradient")
        return out

    def lovasz_gradient(self, logits_full: torch.Tensor, target: torch.Tensor, lowres_size, table=None, lovasz_weight: float = 1.0,
                        return_keys: bool = False, return_pixel_gradient: bool = False):
        """The Lovasz-Softmax terms of each image and the gradient of ``sum T'[t][p] ce + lovasz_weight * L`` with respect to its
        low-resolution logits (nbc_lovasz_gradient; the definitions: include/nbc.h, ``refit.lovasz_pixel_gradient_cpu``): ``L`` is
        the image's Lovasz-Softmax loss (``metrics.lovasz_loss`` of the terms), ``table`` nine numbers ``T'`` already scaled by
        the caller, or None for no cross-entropy term.  ``logits_full``, ``target`` and ``lowres_size`` as ``ce_gradient`` takes
        them.  Returns ``(terms f64 [N,3], fg_counts int64 [N,3], grad_lowres f64 [N,3,h,w])`` -- the first two bit for bit
        ``lovasz_softmax``'s -- then, when asked for, the keys in pixel order (int32 ``[N,3,H,W]`` holding the 31-bit keys
        ``bits(e) << 1 | fg``) and the pixel gradient f64 ``[N,3,H,W]``.  On the current stream."""
        self._require_ctx()
        n, h, w = self._check_logits_target(logits_full, target)
        lh, lw = int(lowres_size[0]), int(lowres_size[1])
        tab = None
        if table is not None:
            tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
            if tab.size != 9:
                raise ValueError("table must hold nine numbers T[target class][argmax class]")
        lam = float(lovasz_weight)
        if not math.isfinite(lam):
            raise ValueError("lovasz_weight must be finite, got %r" % (lovasz_weight,))
        need = int(self._lib.nbc_lovasz_gradient_workspace_bytes(n, h, w, lh, lw))
        if need == 0:
            raise ValueError("nbc_lovasz_gradient refuses a [%d,3,%d,%d] batch with a %dx%d low-resolution map (N <= 65535, "
                             "H * W < 2^31, 1 <= h <= H, 1 <= w <= W)" % (n, h, w, lh, lw))
        rows, cols = self._taps_on_device(lh, h), self._taps_on_device(lw, w)
        terms = torch.empty((n, NUM_CLASSES), dtype=torch.float64, device=self.device)
        fg_counts = torch.empty((n, NUM_CLASSES), dtype=torch.int64, device=self.device)
        out = torch.empty((n, NUM_CLASSES, lh, lw), dtype=torch.float64, device=self.device)
        keys = torch.empty((n, NUM_CLASSES, h, w), dtype=torch.int32, device=self.device) if return_keys else None
        pix = torch.empty((n, NUM_CLASSES, h, w), dtype=torch.float64, device=self.device) if return_pixel_gradient else None
        with self._on_stream() as cur:
            ws = self._grown_workspace("_lovasz_grad_ws", need, cur)
            rc = self._lib.nbc_lovasz_gradient(logits_full.data_ptr(), target.data_ptr(), n, h, w, lh, lw,
                                               *[t.data_ptr() for t in rows + cols],
                                               None if tab is None else tab.ctypes.data_as(C.POINTER(C.c_double)), lam,
                                               ws.data_ptr(), ws.numel(), terms.data_ptr(), fg_counts.data_ptr(), out.data_ptr(),
                                               None if keys is None else keys.data_ptr(), None if pix is None else pix.data_ptr(),
                                               cur.cuda_stream)
        _lib.check(rc, "nbc_lovasz_gradient")
        return (terms, fg_counts, out) + ((keys,) if return_keys else ()) + ((pix,) if return_pixel_gradient else ())

    def head_gradient(self, grad_lowres: torch.Tensor) -> torch.Tensor:
        """``grad_lowres`` f64 ``[N,3,h,w]`` (``ce_gradient``) carried onto the parameters of ``classifier.4`` through the features
        of the LAST forward (nbc_head_gradient): f64 ``[N,3,513]`` per image, a class's 512 weight columns and then its bias, in
        the state_dict's units.  On the current stream; the refusals of ``head_logits``."""
        n, h, w = self._refit_last_shape("head_gradient")
        lh, lw = out_hw(h, w, self.ARCH)
        if not isinstance(grad_lowres, torch.Tensor) or grad_lowres.device != self.device or grad_lowres.dtype != torch.float64 \
                or not grad_lowres.is_contiguous() or tuple(grad_lowres.shape) != (n, NUM_CLASSES, lh, lw):
            raise ValueError("grad_lowres must be a contiguous float64 [%d,3,%d,%d] tensor on %s" % (n, lh, lw, self.device))
        need = int(self._lib.nbc_head_gradient_workspace_bytes(n, h, w))
        if need == 0:
            raise ValueError("nbc_head_gradient refuses a [%d,3,%d,%d] batch" % (n, h, w))
        out = torch.empty((n, NUM_CLASSES, 513), dtype=torch.float64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_head_grad_ws", need, cur)
            rc = self._lib.nbc_head_gradient(self._ctx, grad_lowres.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                             cur.cuda_stream)
        _lib.check(rc, "nbc_head_gradient")
        return out

    def head_loss_and_gradient(self, target: torch.Tensor, theta, table, logits_full: Optional[torch.Tensor] = None,
                               lovasz_weight: Optional[float] = None):
        """The loss cells and their gradient for trial parameters ``theta`` on the images of the LAST forward: ``head_logits`` ->
        ``upsample_argmax`` -> ``pixel_cross_entropy`` -> ``ce_gradient`` -> ``head_gradient``.  ``target``: the uint8 ``[N,H,W]``
        grey masks of that forward's images; ``table`` as ``ce_gradient`` takes it; ``logits_full``: an optional f32
        ``[N,3,H,W]`` buffer for the upsampled logits.  Returns ``(sums f64 [N,3,3], counts int64 [N,3,3], grad f64 [N,3,513])``
        per image: the objective of the batch is ``sum(table * sums)`` and its gradient ``grad.sum(0)``, both not normalised.
        With a ``lovasz_weight`` the gradient is ``lovasz_gradient``'s in place of ``ce_gradient``'s -- of ``sum table[t][p] ce +
        lovasz_weight * L`` per image, ``table`` None for the Lovasz-Softmax loss alone -- and the image's ``(terms f64 [N,3],
        fg_counts int64 [N,3])`` follow the three."""
        n, h, w = self._refit_last_shape("head_loss_and_gradient")
        low = self.head_logits(theta)
        _, _, full = self.upsample_argmax(low, (h, w), labels_dtype=torch.uint8, return_logits=True, logits_full=logits_full)
        sums, counts = self.pixel_cross_entropy(full, target)
        if lovasz_weight is None:
            grad = self.head_gradient(self.ce_gradient(full, target, low.shape[2:], table))
            return sums, counts, grad
        terms, fg_counts, grad_lowres = self.lovasz_gradient(full, target, low.shape[2:], table, lovasz_weight)
        return sums, counts, self.head_gradient(grad_lowres), terms, fg_counts

    def softmax_census(self, logits_full: torch.Tensor, target: Optional[torch.Tensor] = None,
                       confidence: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Per-image census of the softmax confidence on the device (nbc_softmax_census; the definition: include/nbc.h,
        ``calibration.census_cpu``): the histograms of every class probability by target class, the reliability counts and
        exact confidence sums of the winning class, the soft confusion, the Brier numerators and the non-finite pixels.
        ``logits_full``: contiguous f32 ``[N,3,H,W]`` as ``lovasz_softmax`` takes it; ``target``: contiguous uint8 grey mask
        ``[N,H,W]`` or None (every pixel then counts as target class 0 and as a hit); ``confidence``: also the uint8
        ``[N,H,W]`` plane of ``q_k >> 8``, the winning class's probability in 1/256.  Runs on the current stream; the
        workspace is cached on this object and only grows.  Returns ``(rows uint64 [N, NBC_CENSUS_WORDS], plane or None)``;
        ``calibration.figures`` and ``calibration.curves`` turn a row into the numbers."""
        self._require_ctx()
        if target is None:
            if logits_full.device != self.device or logits_full.dtype != torch.float32 or not logits_full.is_contiguous() \
                    or logits_full.dim() != 4 or logits_full.shape[1] != NUM_CLASSES or logits_full.numel() == 0:
                raise ValueError("logits_full must be a contiguous non-empty float32 [N,3,H,W] tensor on %s" % (self.device,))
            n, _, h, w = (int(v) for v in logits_full.shape)
        else:
            n, h, w = self._check_logits_target(logits_full, target)
        need = int(self._lib.nbc_softmax_census_workspace_bytes(n, h, w))
        if need == 0:
            raise ValueError("nbc_softmax_census refuses a [%d,3,%d,%d] batch (N <= 65535, H * W < 2^31)" % (n, h, w))
        rows = torch.empty((n, _lib.CENSUS_WORDS), dtype=torch.uint64, device=self.device)
        plane = torch.empty((n, h, w), dtype=torch.uint8, device=self.device) if confidence else None
        with self._on_stream() as cur:
            ws = self._grown_workspace("_census_ws", need, cur)
            _lib.check(self._lib.nbc_softmax_census(logits_full.data_ptr(), None if target is None else target.data_ptr(), n, h, w,
                                                    ws.data_ptr(), ws.numel(), rows.data_ptr(),
                                                    None if plane is None else plane.data_ptr(), cur.cuda_stream),
                       "nbc_softmax_census")
        return rows, plane

    def set_logit_offsets(self, bark: float = 0.0, node: float = 0.0):
        """Move the operating point (nbc_set_logit_offsets): the upsample + argmax launch of every forward and of
        ``upsample_argmax`` decides by ``argmax(x0, x1 + bark, x2 + node)``, one float32 addition each, instead of the plain
        argmax; the counts, ``exclude_nodes`` and everything downstream follow that decision.  The logits the model returns
        are never offset.  ``(0, 0)`` is off, the default: the model then launches exactly the kernels it launched before.
        Finite values only (``ValueError``).  ``clone_shared`` carries the setting over; ``dropout_draws`` and
        ``dropout_votes`` refuse a model with offsets on.  ``operating.select`` proposes pairs from ``offset_sweep``."""
        bark, node = float(np.float32(bark)), float(np.float32(node))
        if not (math.isfinite(bark) and math.isfinite(node)):
            raise ValueError("logit offsets must be finite, got (%r, %r)" % (bark, node))
        if self._ctx:
            _lib.check(self._lib.nbc_set_logit_offsets(self._ctx, bark, node), "nbc_set_logit_offsets")
        self._logit_offsets = (bark + 0.0, node + 0.0)
        return self

    def logit_offsets(self) -> Tuple[float, float]:
        """The ``(bark, node)`` pair ``set_logit_offsets`` holds; ``(0.0, 0.0)`` when off."""
        return self._logit_offsets

    def offset_sweep(self, logits_full: torch.Tensor, target: torch.Tensor, bark_offsets, node_offsets) -> torch.Tensor:
        """The operating-point sweep on the device (nbc_offset_sweep; the definition: include/nbc.h, ``operating.sweep_cpu``):
        the 3 x 3 confusion of the label map ``argmax(x0, x1 + bark_offsets[i], x2 + node_offsets[j])`` against the target at
        every point of the grid.  ``logits_full``: contiguous f32 ``[N,3,H,W]``; ``target``: contiguous uint8 grey mask
        ``[N,H,W]``; the offsets: 1..33 finite float32 values each, strictly ascending.  Runs on the current stream; the
        workspace is cached on this object and only grows.  It ignores ``set_logit_offsets``: it describes the logits.
        Returns uint64 ``[N, G1, G2, 3, 3]`` on the device, cell ``[t][p]`` the pixels of target class t decided as p."""
        self._require_ctx()
        n, h, w = self._check_logits_target(logits_full, target)
        b1 = np.ascontiguousarray(np.asarray(bark_offsets, dtype=np.float32).reshape(-1))
        b2 = np.ascontiguousarray(np.asarray(node_offsets, dtype=np.float32).reshape(-1))
        g1, g2 = int(b1.size), int(b2.size)
        need = int(self._lib.nbc_offset_sweep_workspace_bytes(n, h, w, g1, g2))
        if need == 0:
            raise ValueError("nbc_offset_sweep refuses a [%d,3,%d,%d] batch on a %d x %d grid (N <= 65535, H * W < 2^31, 1..%d "
                             "offsets each)" % (n, h, w, g1, g2, _lib.SWEEP_MAX_GRID))
        conf = torch.empty((n, g1, g2, NUM_CLASSES, NUM_CLASSES), dtype=torch.uint64, device=self.device)
        fp = C.POINTER(C.c_float)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_sweep_ws", need, cur)
            _lib.check(self._lib.nbc_offset_sweep(logits_full.data_ptr(), target.data_ptr(), n, h, w, b1.ctypes.data_as(fp), g1,
                                                  b2.ctypes.data_as(fp), g2, ws.data_ptr(), ws.numel(), conf.data_ptr(),
                                                  cur.cuda_stream), "nbc_offset_sweep")
        return conf

    def dropout_draws(self, draws: int, image_ids, p: float = 0.1, seed: int = 0, first_draw: int = 0,
                      small_zones: bool = True, exclude_nodes: bool = False, return_lowres: bool = False, *,
                      min_pixels: int = 150, draws_per_pass: int = 8):
        """Random draws of the shipped tool's live ``Dropout(p)`` (``FCNHead``, models.py:113-124; its predict.py never calls
        ``.eval()``) on the images of the LAST forward of this object (``predict_labels`` / ``lowres_logits`` / ``__call__``),
        on the current stream (nbc_dropout_draws; the definition of a draw: include/nbc.h).  The trunk and the
        head convolution are not run again: each draw is a masked ``classifier.4`` on the stored features, the bicubic upsample
        + argmax, ``remove_small_zones`` (``small_zones``, threshold ``min_pixels``) and the ``exclude_nodes`` remap.
        ``image_ids``: one 64-bit identity per image of that forward (``folder_run.image_id``); an image's draws depend on its
        features, its identity, ``seed``, the draw number (``first_draw`` + 0 .. ``draws`` - 1) and ``p`` alone -- not on its
        batch, the stream, the object (``clone_shared``) or ``draws_per_pass`` (how many draws share one read of the features;
        it sizes the workspace cached on this object).  ``p = 0`` gives the forward's own logits bit for bit.
        Returns int64 ``[draws, N, 3]`` pixels per class (+ f32 ``[draws, N, 3, h, w]`` low-resolution logits with
        ``return_lowres``).  ``ValueError``: another network than fcn_resnet50, ``draws`` outside 1..1024, ``p`` outside
        [0, 1), a negative ``first_draw``, an id count other than the last forward's batch."""
        return self._dropout_run("dropout_draws", False, draws, image_ids, p, seed, first_draw, small_zones, exclude_nodes,
                                 return_lowres, min_pixels, draws_per_pass)

    def dropout_votes(self, draws: int, image_ids, p: float = 0.1, seed: int = 0, first_draw: int = 0,
                      small_zones: bool = True, exclude_nodes: bool = False, return_lowres: bool = False, *,
                      min_pixels: int = 150, draws_per_pass: int = 8, return_words: bool = False):
        """``dropout_draws`` -- the same arguments, checks, refusals and, bit for bit, the same counts and logits -- which also
        votes per pixel over the draws' final label maps while they are on the device (nbc_dropout_votes, nbc_vote_summary;
        the definition: include/nbc.h).  Returns ``(counts int64 [D,N,3], vote_labels uint8 [N,H,W], support
        uint8 [N,H,W], stats int64 [N,10])`` (+ ``lowres`` with ``return_lowres``): the class most draws give a pixel (a tie
        goes to the lowest class), ``floor(255 * n_win / D)`` (255 = every draw agrees, never below 85), and per image the
        pixels per winning class (0..2), the unanimous pixels per class (3..5), the sum of n_win (6), invalid words (7, always
        0 here) and the sums of the bark and node votes (8, 9: the draws' counts summed).  ``return_words`` appends the vote
        words themselves, ``[N,H,W]`` int32 holding the uint32 bits: n1 in the low half, n2 in the high half."""
        return self._dropout_run("dropout_votes", True, draws, image_ids, p, seed, first_draw, small_zones, exclude_nodes,
                                 return_lowres, min_pixels, draws_per_pass, return_words)

    def _dropout_run(self, what, votes, draws, image_ids, p, seed, first_draw, small_zones, exclude_nodes, return_lowres,
                     min_pixels, draws_per_pass, return_words=False):
        """The checks and the call behind ``dropout_draws`` and ``dropout_votes``."""
        if topology.is_efficientnet(self.ARCH):
            raise ValueError("dropout draws are refused for %s: EfficientNet's FCN head is left out (its Dropout is not "
                             "implemented)" % self.ARCH)
        if self.ARCH != "fcn_resnet50":
            raise ValueError("dropout draws are refused for %s: DeepLabHead's Dropout sits inside ASPP, in front of convolutions "
                             "that would have to run again for every draw" % self.ARCH)
        draws, first_draw, seed = int(draws), int(first_draw), int(seed)
        if not 1 <= draws <= 1024:
            raise ValueError("draws must lie in 1..1024, got %d" % draws)
        if not (0.0 <= float(p) < 1.0):
            raise ValueError("p must lie in [0, 1), got %r" % (p,))
        if first_draw < 0 or first_draw + draws > 2 ** 31 - 1:
            raise ValueError("first_draw must not be negative, got %d" % first_draw)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be an unsigned 64-bit integer, got %d" % seed)
        if int(min_pixels) < 0 or int(draws_per_pass) < 1:
            raise ValueError("min_pixels must not be negative and draws_per_pass must be positive")
        self._require_weights()
        if self._last_shape is None:
            raise RuntimeError("%s follows a forward (predict_labels / lowres_logits) of this object: none has run" % what)
        n, h, w = self._last_shape
        ids = [int(v) for v in image_ids]
        if len(ids) != n or any(not 0 <= v < 2 ** 64 for v in ids):
            raise ValueError("image_ids must hold one unsigned 64-bit identity per image of the last forward (%d), got %d"
                             % (n, len(ids)))
        ids_arr = (C.c_uint64 * n)(*ids)
        per_pass = max(1, min(draws, int(draws_per_pass), 65535 // n))
        need = int(self._lib.nbc_dropout_workspace_bytes(n, h, w, per_pass))
        if need == 0:
            raise ValueError("nbc_%s refuses a [%d,3,%d,%d] batch (draws x N <= 65535 per pass, H * W < 2^31)" % (what, n, h, w))
        counts = torch.empty((draws, n, NUM_CLASSES), dtype=torch.int64, device=self.device)
        lowres = None
        if return_lowres:
            lowres = torch.empty((draws, n, NUM_CLASSES) + out_hw(h, w, self.ARCH), dtype=torch.float32, device=self.device)
        min_px = int(min_pixels) if small_zones else 0
        low_ptr = lowres.data_ptr() if lowres is not None else None
        if not votes:
            with self._on_stream() as cur:
                ws = self._grown_workspace("_dropout_ws", need, cur)
                # the workspace handed over is exactly what per_pass draws need: a larger cached one must not change the pass
                rc = self._lib.nbc_dropout_draws(self._ctx, n, h, w, ids_arr, float(p), seed, first_draw, draws, min_px,
                                                 int(bool(exclude_nodes)), low_ptr, counts.data_ptr(), ws.data_ptr(), need,
                                                 cur.cuda_stream)
            _lib.check(rc, "nbc_dropout_draws")
            return (counts, lowres) if return_lowres else counts
        words = torch.empty((n, h, w), dtype=torch.int32, device=self.device)       # uint32 vote words (torch has no such dtype)
        vote_labels = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        support = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        stats = torch.empty((n, _lib.VOTE_STATS), dtype=torch.int64, device=self.device)
        with self._on_stream() as cur:
            ws = self._grown_workspace("_dropout_ws", need, cur)
            rc = self._lib.nbc_dropout_votes(self._ctx, n, h, w, ids_arr, float(p), seed, first_draw, draws, min_px,
                                             int(bool(exclude_nodes)), low_ptr, counts.data_ptr(), words.data_ptr(), 0,
                                             ws.data_ptr(), need, cur.cuda_stream)
            _lib.check(rc, "nbc_dropout_votes")
            _lib.check(self._lib.nbc_vote_summary(words.data_ptr(), n, h, w, draws, vote_labels.data_ptr(), support.data_ptr(),
                                                  stats.data_ptr(), cur.cuda_stream), "nbc_vote_summary")
        out = (counts, vote_labels, support, stats)
        return out + ((lowres,) if return_lowres else ()) + ((words,) if return_words else ())

    def resize_cubic_u8(self, image: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
        """The resize of the reference's preprocessor (models.py:191-198) on the device: uint8 RGB
        ``[H,W,3]`` -> ToTensor -> ``skimage.transform.resize(order=3, mode='reflect',
        anti_aliasing=False)`` -> float32 ``[out_h,out_w,3]``; bit-identical to
        ``predict.resize_bicubic_reflect(image.astype(float32) / 255, out_h, out_w)``."""
        self._require_ctx()
        self._check_rgb_u8(image)
        out = torch.empty((int(out_h), int(out_w), 3), dtype=torch.float32, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_resize_cubic_u8(self._ctx, image.data_ptr(), int(image.shape[0]), int(image.shape[1]),
                                                     out.data_ptr(), int(out_h), int(out_w), cur.cuda_stream), "nbc_resize_cubic_u8")
        return out

    def preprocess_u8(self, image: torch.Tensor, out_h: int, out_w: int):
        """``resize_cubic_u8`` followed by the float -> uint8 conversion of ``skimage.io.imsave`` (models.py:203)
        and ``trim_black``'s per-row lit-pixel counts (models.py:158-161), all on the device.  Returns
        ``(uint8 [out_h,out_w,3], int32 [out_h])``."""
        self._require_ctx()
        self._check_rgb_u8(image)
        out = torch.empty((int(out_h), int(out_w), 3), dtype=torch.uint8, device=self.device)
        lit = torch.empty((int(out_h),), dtype=torch.int32, device=self.device)
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_preprocess_u8(self._ctx, image.data_ptr(), int(image.shape[0]), int(image.shape[1]),
                                                   out.data_ptr(), lit.data_ptr(), int(out_h), int(out_w), cur.cuda_stream), "nbc_preprocess_u8")
        return out, lit

    def upsample_argmax(self, lowres: torch.Tensor, size: Tuple[int, int], exclude_nodes: bool = False,
                        labels_dtype: torch.dtype = torch.int64, return_logits: bool = False,
                        logits_full: Optional[torch.Tensor] = None):
        """Tail of the path on caller-supplied low-res logits f32 ``[N,3,h,w]``:
        bicubic to ``size`` (models.py:38-41), argmax (models.py:270), remap, counts.  ``logits_full``: an optional contiguous
        f32 ``[N,3,H,W]`` tensor on this model's device that receives the upsampled logits (``return_logits`` allocates one)."""
        self._require_ctx()
        if lowres.dtype != torch.float32 or lowres.dim() != 4 or lowres.shape[1] != NUM_CLASSES:
            raise RuntimeError("expected float32 [N,3,h,w]")
        lowres = lowres.contiguous()
        n, _, lh, lw = lowres.shape
        H, W = int(size[0]), int(size[1])
        labels = torch.empty((n, H, W), dtype=labels_dtype, device=self.device)
        counts = torch.empty((n, NUM_CLASSES), dtype=torch.int64, device=self.device)
        logits = logits_full
        if logits is not None and (logits.device != self.device or logits.dtype != torch.float32 or not logits.is_contiguous()
                                   or tuple(logits.shape) != (n, NUM_CLASSES, H, W)):
            raise ValueError("logits_full must be a contiguous float32 [%d,%d,%d,%d] tensor on %s" % (n, NUM_CLASSES, H, W, self.device))
        if logits is None and return_logits:
            logits = torch.empty((n, NUM_CLASSES, H, W), dtype=torch.float32, device=self.device)
        ldt = _lib.LABEL_I64 if labels_dtype == torch.int64 else _lib.LABEL_U8
        with self._on_stream() as cur:
            rc = self._lib.nbc_upsample_argmax(self._ctx, lowres.data_ptr(), n, lh, lw, H, W,
                                               logits.data_ptr() if logits is not None else None,
                                               labels.data_ptr(), ldt, counts.data_ptr(),
                                               int(bool(exclude_nodes)), cur.cuda_stream)
        _lib.check(rc, "nbc_upsample_argmax")
        return (labels, counts, logits) if return_logits else (labels, counts)

    def set_normalization(self, mean, std):
        """mean/std applied to uint8 NHWC input (defaults: models.py:208-209)."""
        m = (C.c_float * 3)(*[float(v) for v in mean])
        s = (C.c_float * 3)(*[float(v) for v in std])
        _lib.check(self._lib.nbc_set_normalization(self._require_ctx(), m, s), "set_normalization")

    def reserve(self, n: int, h: int, w: int):
        """Size the activation workspace ahead of the first call."""
        self._require_weights()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.nbc_reserve(self._ctx, n, h, w), "nbc_reserve")

    def clone_shared(self) -> "FCNResNet50":
        """A second model object on the same device that shares this one's packed weights (one copy
        in HBM) but owns its own context and activation workspace, so the two can run concurrently
        on different HIP streams (pipelined batch-1 serving)."""
        self._require_weights()
        other = self._like()
        other.bn_statistics = self.bn_statistics
        other._logit_offsets = self._logit_offsets      # applied when `to` creates the context
        other.to(self.device)
        other._attach(self._blob_dev, self._affine_dev, self._raw_dev)
        return other

    def _like(self) -> "FCNResNet50":
        """A fresh model object of this network and precision."""
        return type(self)(self.precision)

    # ---- multi-GPU: one process per GPU, weights read by one rank only ---------------------
    def broadcast_weights(self, src: int = 0, group=None):
        """RCCL broadcast of the packed weight blob from rank ``src`` (the only rank that needs
        ``load_state_dict``); the other ranks call this right after ``to(device)``."""
        import torch.distributed as dist
        if self.device is None:
            raise RuntimeError("call .to(device) before broadcast_weights")
        nbytes = self._lib.nbc_arch_packed_weights_bytes(self._prec, topology.arch_index(self.ARCH))
        if dist.get_rank(group) == src:
            self._require_weights()
            blob = self._blob_dev
        else:
            blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        dist.broadcast(blob, src=src, group=group)
        # the per-image BatchNorm affine array travels beside the blob (one more collective, every rank alike)
        affine = broadcast_bn_affine(self._affine_host if dist.get_rank(group) == src else None, self.ARCH, src, group,
                                     self.device)
        self._affine_host = affine
        raw = None
        if self._has_bn_raw():                             # and so does the f16x2 raw-convolution array
            self._raw_host = broadcast_bn_raw(self._raw_host if dist.get_rank(group) == src else None, self.ARCH, src, group,
                                              self.device)
            raw = torch.from_numpy(self._raw_host).to(self.device)
        self._attach(blob, torch.from_numpy(affine).to(self.device), raw)
        return self

    # ---- measurement / debugging ------------------------------------------------------------
    def set_profiling(self, on: bool):
        _lib.check(self._lib.nbc_set_profiling(self._require_ctx(), int(on)))

    def op_records(self):
        """Per-launch (name, kernel, ms, flops, bytes, k) of the last profiled forward."""
        out = []
        rec = _lib.NbcOpRecord()
        n = self._lib.nbc_num_op_records(self._require_ctx())
        if n < 0:
            _lib.check(n, "nbc_num_op_records")
        for i in range(n):
            _lib.check(self._lib.nbc_get_op_record(self._ctx, i, C.byref(rec)))
            out.append(dict(name=rec.name.decode(), kernel=rec.kernel.decode(), ms=float(rec.ms),
                            calls=int(rec.calls), flops=float(rec.flops), bytes=float(rec.bytes),
                            k=int(rec.kh), cout=int(rec.cout), launches=int(rec.launches)))
        return out

    @property
    def pack_flags(self) -> int:
        """NBC_PACK_* bits of the weights this model holds (0 = nothing given up): in "f16x2" mode a weight row beyond the
        reach of the row normalisation (``_lib.PACK_ROW_CLAMPED``) or a BatchNorm scale / shift pushed out of f32's normal
        range by the powers of two folded into it (``_lib.PACK_SCALE_RANGE``) -- run such a checkpoint in "fp32".  Read from
        the packed blob's trailer, so a rank that received the blob by broadcast sees the same bits.  In bn_statistics
        "image_f16x2" the bits of the raw-convolution array (``bn_raw_flags``) join them."""
        extra = bn_raw_flags(self._raw_host) if self.bn_statistics == "image_f16x2" and self._raw_host is not None else 0
        if self._ctx and self._blob_dev is not None:
            rc = self._lib.nbc_weights_flags(self._ctx)
            if rc < 0:
                _lib.check(rc, "nbc_weights_flags")
            return int(rc) | extra
        if self._blob_host is None:
            raise RuntimeError("no weights loaded")
        rc = self._lib.nbc_packed_weights_flags_arch(self._blob_host.ctypes.data, self._blob_host.size, self._prec,
                                                     topology.arch_index(self.ARCH))
        if rc < 0:
            _lib.check(rc, "nbc_packed_weights_flags")
        return int(rc) | extra

    def activation_exponent(self, name: str) -> int:
        """Power of two the output tensor of op ``name`` is stored with on the device (0 outside "f16x2" and for every
        tensor of an ordinary checkpoint; nbc_activation_exponent)."""
        e = C.c_int32(0)
        _lib.check(self._lib.nbc_activation_exponent(self._require_ctx(), name.encode(), C.byref(e)), "nbc_activation_exponent")
        return int(e.value)

    def activation_peaks(self, x: torch.Tensor) -> dict:
        """One forward of ``x`` with every activation kept, then the largest finite |value| of each conv unit's output AS
        STORED on the device (nbc_activation_peaks): ``{conv unit name: peak}``, classifier.4 left out.  The calibration
        guard of "f16x2": a tensor that peaks below 2^-8 (or beyond 2^14) on real data belongs in "fp32"
        (``f16x2_range_ok``)."""
        n, h, w = self._check_input(x)
        self.set_keep_activations(True)
        try:
            self._forward(x, n, h, w, lowres=torch.empty((n, NUM_CLASSES) + out_hw(h, w, self.ARCH), dtype=torch.float32, device=self.device))
            torch.cuda.synchronize(self.device)
            k = int(self._lib.nbc_arch_num_convs(topology.arch_index(self.ARCH)))
            buf = (C.c_float * k)()
            rc = self._lib.nbc_activation_peaks(self._require_ctx(), buf, k)
            if rc < 0:
                _lib.check(rc, "nbc_activation_peaks")
        finally:
            self.set_keep_activations(False)
        names = [u.name for u in topology.conv_units(self.ARCH)]
        return {names[i]: float(buf[i]) for i in range(k) if names[i] != "classifier.4"}

    @staticmethod
    def f16x2_range_ok(peaks: dict, low: float = 2.0 ** -8, high: float = 2.0 ** 14):
        """(ok, offenders): whether every stored tensor of ``activation_peaks`` lies where the f16 pieces hold f32 grade."""
        bad = {k: v for k, v in peaks.items() if not (low <= v <= high)}
        return (not bad), bad

    def nonfinite_seen(self, reset: bool = True) -> bool:
        """True when a forward since the last reset produced a NaN / infinite logit (nbc_nonfinite_seen; synchronises).
        In "f16x2" mode that also means an activation left f16's range, and in bn_statistics "image_f16x2" a channel
        whose raw values left the range the pieces hold (bit 2 of the word): rerun such weights in "fp32"."""
        rc = self._lib.nbc_nonfinite_seen(self._require_ctx(), int(reset))
        if rc < 0:
            _lib.check(rc, "nbc_nonfinite_seen")
        return rc == 1

    def nonfinite_peek_async(self, host_word: torch.Tensor):
        """Enqueue, on the current stream, a copy of the sticky non-finite word into ``host_word`` (pinned int32 [1]); no
        synchronisation (nbc_nonfinite_peek_async).  Non-zero once the stream has caught up = a forward of this context
        ahead of the copy produced a NaN / infinite logit."""
        if host_word.dtype != torch.int32 or host_word.numel() != 1 or host_word.is_cuda or not host_word.is_pinned():
            raise ValueError("host_word must be a pinned int32 CPU tensor with one element")
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_nonfinite_peek_async(self._require_ctx(), host_word.data_ptr(), cur.cuda_stream), "nbc_nonfinite_peek_async")

    def set_fuse_downsample(self, on: bool = True):
        """Test / A-B switch (f16x2): whether downsample.0 of a stage's first bottleneck runs inside the launch of the conv3
        that adds it (include/nbc.h, nbc_set_fuse_downsample; default on, same bits either way)."""
        _lib.check(self._lib.nbc_set_fuse_downsample(self._require_ctx(), int(on)), "nbc_set_fuse_downsample")

    def fused_pairs(self) -> int:
        """(downsample.0, conv3) pairs the last forward ran as one launch."""
        n = self._lib.nbc_fused_pairs(self._require_ctx())
        if n < 0:
            _lib.check(n, "nbc_fused_pairs")
        return int(n)

    def set_conv_tile(self, tile: int = -1):
        """Tuning/test knob: tile -1 = per-layer choice, 0..20 = one tile shape of the conv kernel (18 / 19 / 20: the row-resident 3x3
        kernel of f16x2, which its layers never leave; the menu:
        include/nbc.h, nbc_set_conv_tile; e.g. 5 = 128x256, 14 = 128x128 with four loader waves and 17 = 128x128 at two
        blocks per CU, both f16x2 only).  A tile that does not exist for the precision, or does not divide a layer's
        Cout, is ignored for that layer: the planned tile runs."""
        _lib.check(self._lib.nbc_set_conv_tile(self._require_ctx(), int(tile)), "nbc_set_conv_tile")

    def autotune(self, x: torch.Tensor, reps: int = 3, objective: str = "latency"):
        """Measure every conv tile shape on every layer for x's (N,H,W) and keep the fastest per
        layer (results are tile-independent).  objective "latency" minimises each launch alone;
        "throughput" weighs a launch by the share of the chip it occupies (use it when several
        forwards overlap on different streams).  Returns the chosen tile ids in launch order."""
        n, h, w = self._check_input(x)
        x = x.contiguous()
        x_dtype = _lib.IN_F32_NCHW if x.dtype == torch.float32 else _lib.IN_U8_NHWC
        with self._on_stream() as cur:
            _lib.check(self._lib.nbc_autotune(self._ctx, x.data_ptr(), x_dtype, n, h, w, int(reps),
                                              1 if objective == "throughput" else 0, cur.cuda_stream),
                       "nbc_autotune")
        return self.plan_tiles()

    def plan_tiles(self):
        buf = (C.c_int32 * 64)()
        n = self._lib.nbc_get_plan_tiles(self._require_ctx(), buf, 64)
        return [int(buf[i]) for i in range(min(n, 64))]

    def set_plan_tiles(self, tiles):
        """Install a per-layer tile choice (as ``plan_tiles`` / ``autotune`` return it) for the current
        (N,H,W) plan, e.g. one measured by an earlier process."""
        arr = (C.c_int32 * len(tiles))(*[int(t) for t in tiles])
        _lib.check(self._lib.nbc_set_plan_tiles(self._require_ctx(), arr, len(tiles)), "nbc_set_plan_tiles")

    def set_keep_activations(self, on: bool):
        _lib.check(self._lib.nbc_set_keep_activations(self._require_ctx(), int(on)))

    def read_activation(self, name: str, numel_hint: int) -> np.ndarray:
        """f32 NCHW copy of the activation the op ``name`` wrote in the last forward."""
        buf = np.empty(numel_hint, dtype=np.float32)
        shape = (C.c_int64 * 4)()
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.nbc_read_activation(self._require_ctx(), name.encode(), buf.ctypes.data,
                                                 buf.size, C.byref(shape)), "read_activation")
        shp = tuple(int(s) for s in shape)
        return buf[: int(np.prod(shp))].reshape(shp)

    # ---- internals --------------------------------------------------------------------------
    @contextlib.contextmanager
    def _on_stream(self):
        """Enters this model's device and yields the current stream there."""
        with torch.cuda.device(self.device):
            yield torch.cuda.current_stream(self.device)

    def _grown_workspace(self, attr: str, need: int, stream) -> torch.Tensor:
        """The workspace cached as ``self.<attr>``, grown (never shrunk) to ``need`` bytes; it may be used on several streams."""
        ws = getattr(self, attr)
        if ws is None or ws.numel() < need:
            setattr(self, attr, None)
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            setattr(self, attr, ws)
        ws.record_stream(stream)
        return ws

    def _check_labels(self, labels: torch.Tensor):
        if labels.device != self.device or labels.dtype not in (torch.uint8, torch.int64) or not labels.is_contiguous():
            raise ValueError("labels must be a contiguous uint8 or int64 tensor on %s" % (self.device,))

    def _check_target_like(self, labels: torch.Tensor, target: torch.Tensor):
        """``target``: the contiguous uint8 grey mask of checked ``labels``, ``[H,W]`` or ``[N,H,W]`` like them."""
        if target.device != self.device or target.dtype != torch.uint8 or not target.is_contiguous():
            raise ValueError("target must be a contiguous uint8 tensor on %s" % (self.device,))
        if labels.dim() not in (2, 3) or labels.shape != target.shape or labels.numel() == 0:
            raise ValueError("labels and target must both be [H,W] or [N,H,W] of the same non-empty shape")

    @staticmethod
    def _label_code(labels: torch.Tensor) -> int:
        return _lib.LABEL_I64 if labels.dtype == torch.int64 else _lib.LABEL_U8

    @staticmethod
    def _batch_hw(labels: torch.Tensor) -> Tuple[int, int, int]:
        """(N, H, W) of ``[N,H,W]`` labels, or (1, H, W) of ``[H,W]`` ones."""
        return 1 if labels.dim() == 2 else int(labels.shape[0]), int(labels.shape[-2]), int(labels.shape[-1])

    def _check_rgb_u8(self, image: torch.Tensor):
        if image.device != self.device or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3 \
                or not image.is_contiguous():
            raise ValueError("image must be a contiguous uint8 [H,W,3] tensor on %s" % (self.device,))

    def _check_logits_target(self, logits_full: torch.Tensor, target: torch.Tensor) -> Tuple[int, int, int]:
        """(N, H, W) of a contiguous f32 ``[N,3,H,W]`` and its contiguous uint8 ``[N,H,W]`` grey mask, both on this device."""
        if logits_full.device != self.device or logits_full.dtype != torch.float32 or not logits_full.is_contiguous() \
                or logits_full.dim() != 4 or logits_full.shape[1] != NUM_CLASSES:
            raise ValueError("logits_full must be a contiguous float32 [N,3,H,W] tensor on %s" % (self.device,))
        n, _, h, w = (int(v) for v in logits_full.shape)
        if target.device != self.device or target.dtype != torch.uint8 or not target.is_contiguous() \
                or tuple(target.shape) != (n, h, w) or target.numel() == 0:
            raise ValueError("target must be a contiguous uint8 [%d,%d,%d] tensor on %s" % (n, h, w, self.device))
        return n, h, w

    def _require_ctx(self):
        if not self._ctx:
            raise RuntimeError("call .to('cuda[:i]') first")
        return self._ctx

    def _require_weights(self):
        self._require_ctx()
        if self._blob_dev is None:
            raise RuntimeError("no weights: call load_state_dict (or broadcast_weights) first")

    def _upload(self):
        blob = torch.from_numpy(self._blob_host).to(self.device, non_blocking=False)
        affine = torch.from_numpy(self._affine_host).to(self.device) if self._affine_host is not None else None
        raw = torch.from_numpy(self._raw_host).to(self.device) if self._raw_host is not None else None
        self._attach(blob, affine, raw)

    def _has_bn_raw(self) -> bool:
        """Whether this model carries the raw-convolution array: an "f16x2" ResNet-50 network."""
        return self._prec == _lib.PREC_F16X2 and not topology.is_efficientnet(self.ARCH)

    def _attach(self, blob: torch.Tensor, affine: Optional[torch.Tensor] = None, raw: Optional[torch.Tensor] = None):
        assert blob.dtype == torch.uint8 and blob.is_contiguous() and blob.device == self.device
        _lib.check(self._lib.nbc_attach_weights_arch(self._require_ctx(), blob.data_ptr(), blob.numel(), self._prec,
                                                     topology.arch_index(self.ARCH)), "nbc_attach_weights")
        self._blob_dev = blob    # keep the device memory alive as long as it is attached
        if affine is not None:
            assert affine.dtype == torch.float32 and affine.is_contiguous() and affine.device == self.device
            _lib.check(self._lib.nbc_attach_bn_affine(self._ctx, affine.data_ptr(), affine.numel()), "nbc_attach_bn_affine")
            self._affine_dev = affine
        if raw is not None:
            assert raw.dtype == torch.float32 and raw.is_contiguous() and raw.device == self.device
            _lib.check(self._lib.nbc_attach_bn_raw(self._ctx, raw.data_ptr(), raw.numel()), "nbc_attach_bn_raw")
            self._raw_dev = raw
        _lib.check(self._lib.nbc_set_bn_statistics(self._ctx, BN_STATISTICS[self.bn_statistics]), "nbc_set_bn_statistics")

    def _check_input(self, x: torch.Tensor) -> Tuple[int, int, int]:
        self._require_weights()
        if not isinstance(x, torch.Tensor):
            raise TypeError("input must be a torch.Tensor")
        if x.device != self.device:
            raise RuntimeError(f"input is on {x.device}, model is on {self.device}")
        if x.dtype == torch.float32:
            if x.dim() != 4 or x.shape[1] != 3:
                raise RuntimeError(f"expected float32 [N,3,H,W], got {tuple(x.shape)}")
            n, _, h, w = x.shape
        elif x.dtype == torch.uint8:
            if x.dim() != 4 or x.shape[3] != 3:
                raise RuntimeError(f"expected uint8 [N,H,W,3], got {tuple(x.shape)}")
            n, h, w, _ = x.shape
        else:
            raise RuntimeError(f"unsupported input dtype {x.dtype}")
        if h < 8 or w < 8:
            raise RuntimeError("H and W must be >= 8")
        if min(out_hw(int(h), int(w), self.ARCH)) < 1:
            raise RuntimeError("a %dx%d image is too small for %s" % (h, w, self.ARCH))
        if self.bn_statistics in PER_IMAGE_MODES and out_hw(int(h), int(w)) == (1, 1):
            raise ValueError("Expected more than 1 value per channel when training: a %dx%d image has a 1x1 low-resolution "
                             "map, which per-image BatchNorm statistics cannot normalise" % (h, w))
        return int(n), int(h), int(w)

    def _check_model_input(self, x):
        """``(x contiguous, is float32, n, h, w)`` of a batch in either layout the model takes, for the view makers."""
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dim() != 4 or x.numel() == 0 or not (
                (x.dtype == torch.float32 and x.shape[1] == 3) or (x.dtype == torch.uint8 and x.shape[3] == 3)):
            raise ValueError("x must be a non-empty float32 [N,3,H,W] or uint8 [N,H,W,3] tensor on %s" % (self.device,))
        f32, s = x.dtype == torch.float32, x.shape
        return (x.contiguous(), f32, int(s[0])) + ((int(s[2]), int(s[3])) if f32 else (int(s[1]), int(s[2])))

    def _stack_entries(self, lowres, n: int) -> int:
        """The entries per image of a low-resolution stack, a non-empty float32 ``[E*n,3,h,w]`` (or ``[E,n,3,h,w]``) tensor on
        this model's device; 0 for anything else.  The callers word their own refusals."""
        if not isinstance(lowres, torch.Tensor) or lowres.device != self.device or lowres.dtype != torch.float32 \
                or lowres.dim() not in (4, 5) or lowres.numel() == 0 or lowres.shape[-3] != NUM_CLASSES or n < 1:
            return 0
        entries = int(np.prod(lowres.shape[:-3]))
        return 0 if entries % n else entries // n

    def _forward(self, x, n, h, w, logits_full=None, labels=None, counts=None, lowres=None,
                 exclude_nodes=False):
        x = x.contiguous()
        x_dtype = _lib.IN_F32_NCHW if x.dtype == torch.float32 else _lib.IN_U8_NHWC
        ldt = _lib.LABEL_I64 if (labels is None or labels.dtype == torch.int64) else _lib.LABEL_U8
        ptr = lambda t: (t.data_ptr() if t is not None else None)
        with self._on_stream() as cur:
            rc = self._lib.nbc_forward(self._ctx, x.data_ptr(), x_dtype, n, h, w, ptr(lowres), ptr(logits_full),
                                       ptr(labels), ldt, ptr(counts), int(bool(exclude_nodes)), cur.cuda_stream)
        _lib.check(rc, "nbc_forward")
        self._last_shape = (n, h, w)

    def _destroy(self):
        if self._ctx:
            self._lib.nbc_destroy(self._ctx)
            self._ctx = C.c_void_p()
        self._blob_dev = None
        self._lovasz_ws = None
        self._lovasz_grad_ws = None
        self._pixel_ce_ws = None
        self._dropout_ws = None
        self._zones_ws = None
        self._zone_match_ws = None
        self._contours_ws = None
        self._census_ws = None
        self._sweep_ws = None
        self._frame_taps = {}
        self._last_shape = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass


def fcn_resnet50(pretrained: bool = False, dropout: float = 0.1, precision: str = "fp32",
                 bn_statistics: str = "running") -> FCNResNet50:
    """Factory with the reference's name and arguments (models.py:127).  ``pretrained=True``
    would download ImageNet weights in the reference; there is no network here.  ``bn_statistics``:
    ``FCNResNet50.set_bn_statistics``."""
    if pretrained:
        raise RuntimeError("pretrained=True needs a download; load a local state_dict instead (predict.py:57)")
    del dropout  # identity in eval mode (and its expectation in train mode)
    return FCNResNet50(precision=precision).set_bn_statistics(bn_statistics)


class DeepLabV3ResNet50(FCNResNet50):
    """MI355X-native ``deeplabv3_resnet50`` (models.py:46-57): the same trunk and surface as ``FCNResNet50`` with
    torchvision 0.3's DeepLabHead -- ASPP(2048, [12, 24, 36]) (a 1x1 conv, three 3x3 convs at dilation 12 / 24 / 36 and a
    global-average-pool branch, concatenated and projected to 256 channels), a 3x3 conv and the 1x1 classifier -- then the
    same bicubic x8 upsample and argmax.  Strict loading takes exactly its 362 keys; an FCN checkpoint raises, like the
    reference's ``load_state_dict``.  ``broadcast_weights`` uses ``torch.distributed`` like the FCN model."""

    ARCH = "deeplabv3_resnet50"


class FCNEfficientNet(FCNResNet50):
    """MI355X-native ``fcn_efficientnet(n, dropout)`` (models.py:95-101): the trunk of efficientnet_pytorch 0.7's
    ``EfficientNet.from_pretrained('efficientnet-b{n}').extract_features`` -- stem, MBConv blocks with depthwise convolutions,
    swish and squeeze-and-excitation, head conv, output stride 32 -- under ``FCNHead(inplanes, 3)``, then the bicubic x32
    upsample and argmax.  "fp32" only (``ValueError`` otherwise), running BatchNorm statistics only.  Strict loading takes
    exactly the variant's keys, the trunk's unused ImageNet classifier (``backbone.model._fc.*``) included."""

    HEAD = "fcn"

    def __init__(self, n: int = 0, precision: str = "fp32"):
        if int(n) not in range(8):
            raise ValueError("EfficientNet variant n must be 0..7, got %r" % (n,))
        self.n = int(n)
        self.ARCH = "%s_efficientnet_b%d" % ("deeplabv3" if self.HEAD == "deeplab" else "fcn", self.n)
        super().__init__(precision)

    def _like(self):
        return type(self)(self.n, self.precision)


class DeepLabV3EfficientNet(FCNEfficientNet):
    """MI355X-native ``deeplabv3_efficientnet(n)`` (models.py:81-87): the EfficientNet-b{n} trunk of ``FCNEfficientNet``
    under ``DeepLabHead(inplanes, 3)``.  "fp32" only."""

    HEAD = "deeplab"


def fcn_efficientnet(n: int, dropout: float = 0.1, precision: str = "fp32") -> FCNEfficientNet:
    """Factory with the reference's name and arguments (models.py:95).  The reference starts from ImageNet weights that the
    checkpoint's load_state_dict replaces in full; here the weights come from load_state_dict alone."""
    del dropout  # identity in eval mode
    return FCNEfficientNet(n, precision=precision)


def deeplabv3_efficientnet(n: int, precision: str = "fp32") -> DeepLabV3EfficientNet:
    """Factory with the reference's name (models.py:81)."""
    return DeepLabV3EfficientNet(n, precision=precision)


MODELS = {"fcn_resnet50": FCNResNet50, "deeplabv3_resnet50": DeepLabV3ResNet50}
for _n in range(8):
    MODELS["fcn_efficientnet_b%d" % _n] = (lambda n: lambda precision="fp32": FCNEfficientNet(n, precision))(_n)
    MODELS["deeplabv3_efficientnet_b%d" % _n] = (lambda n: lambda precision="fp32": DeepLabV3EfficientNet(n, precision))(_n)


def deeplabv3_resnet50(precision: str = "fp32") -> DeepLabV3ResNet50:
    """Factory with the reference's name (models.py:46).  The reference builds its trunk with ImageNet weights, which the
    checkpoint's load_state_dict then replaces in full; here the weights come from load_state_dict alone."""
    return DeepLabV3ResNet50(precision=precision)
