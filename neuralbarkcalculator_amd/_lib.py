"""ctypes binding of libnbc_hip.so (C ABI declared in include/nbc.h).

The library is the product: there is no Python/torch fallback.  ``load()`` raises if the
shared object has not been built (``python -m neuralbarkcalculator_amd.build``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libnbc_hip.so")

NBC_OK = 0
NBC_ERR_INVALID, NBC_ERR_KEYS, NBC_ERR_HIP, NBC_ERR_STATE, NBC_ERR_NOMEM = -1, -2, -3, -4, -5
PREC_FP32, PREC_BF16, PREC_F16X2 = 0, 1, 2
IN_F32_NCHW, IN_U8_NHWC = 0, 1
LABEL_U8, LABEL_I64 = 0, 1
PACK_ROW_CLAMPED, PACK_SCALE_RANGE = 1, 2      # NBC_PACK_* of include/nbc.h
ARCH_FCN_RESNET50, ARCH_DEEPLABV3_RESNET50 = 0, 1   # NBC_ARCH_*
ARCH_FCN_EFFICIENTNET_B0, ARCH_DEEPLABV3_EFFICIENTNET_B0 = 16, 24   # + n, n = 0..7
BN_RUNNING, BN_PER_IMAGE = 0, 1                     # NBC_BN_*
VOTE_STATS = 10                                     # NBC_VOTE_STATS
ZONE_ROW = 10                                       # NBC_ZONE_ROW
ZONE_PAIR_ROW = 3                                   # NBC_ZONE_PAIR_ROW
PAIRS_MAX_CAP = 4096                                # NBC_ZONE_PAIRS_MAX_CAP
CONTOUR_SETS, CONTOUR_HEAD = 4, 4                   # NBC_CONTOUR_SETS, NBC_CONTOUR_HEAD
CONTOUR_MAX_SIDE = 4096                             # NBC_CONTOUR_MAX_SIDE
CENSUS_BINS, CENSUS_WORDS = 256, 3341               # NBC_CENSUS_BINS, NBC_CENSUS_WORDS
CENSUS_H, CENSUS_R, CENSUS_RS, CENSUS_M, CENSUS_B, CENSUS_NONFINITE = 0, 2304, 2816, 3328, 3337, 3340   # NBC_CENSUS_*
TTA_IDENTITY, TTA_HFLIP, TTA_VFLIP, TTA_HVFLIP, TTA_FLIPS = 1, 2, 4, 8, 15   # NBC_TTA_*
JITTER_MAX_VIEWS = 16                               # NBC_JITTER_MAX_VIEWS
WINDOW_CELL, WINDOW_MAX_K = 8, 1024                 # NBC_WINDOW_CELL, NBC_WINDOW_MAX_K
BLEND_TENT, BLEND_UNIFORM = 0, 1                    # NBC_BLEND_*
FRAME_TAPS = 3                                      # NBC_FRAME_TAPS
SWEEP_MAX_GRID = 33                                 # NBC_SWEEP_MAX_GRID


class NbcTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("shape", C.c_int64 * 4),
                ("ndim", C.c_int32), ("dtype", C.c_int32)]


class NbcConvDesc(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("bn", C.c_char * 64),
                ("cin", C.c_int32), ("cout", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("dil", C.c_int32),
                ("relu", C.c_int32), ("bias", C.c_int32), ("residual", C.c_int32)]


class NbcConvExt(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad_before", C.c_int32), ("pad_after", C.c_int32), ("act", C.c_int32),
                ("cin_pad", C.c_int32), ("cout_pad", C.c_int32), ("block", C.c_int32), ("in_swish", C.c_int32),
                ("eps", C.c_float)]


class NbcOpRecord(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("kernel", C.c_char * 32), ("ms", C.c_float), ("calls", C.c_int32),
                ("flops", C.c_double), ("bytes", C.c_double), ("kh", C.c_int32), ("kw", C.c_int32),
                ("cout", C.c_int32), ("launches", C.c_int32)]


# every symbol include/nbc.h declares: (restype, argtypes)
SIGNATURES = {
    "nbc_last_error": (C.c_char_p, []),
    "nbc_version": (C.c_char_p, []),
    "nbc_num_convs": (C.c_int, []),
    "nbc_conv_info": (C.c_int, [C.c_int, C.POINTER(NbcConvDesc)]),
    "nbc_num_state_keys": (C.c_int, []),
    "nbc_state_key": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64 * 4),
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "nbc_arch_num_convs": (C.c_int, [C.c_int]),
    "nbc_arch_conv_info": (C.c_int, [C.c_int, C.c_int, C.POINTER(NbcConvDesc)]),
    "nbc_arch_num_state_keys": (C.c_int, [C.c_int]),
    "nbc_arch_state_key": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64 * 4),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "nbc_arch_of_state_dict": (C.c_int, [C.POINTER(NbcTensor), C.c_int]),
    "nbc_lowres_size": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nbc_arch_lowres_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nbc_arch_conv_ext": (C.c_int, [C.c_int, C.c_int, C.POINTER(NbcConvExt)]),
    "nbc_packed_weights_bytes": (C.c_size_t, [C.c_int]),
    "nbc_split_f16x2": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "nbc_pack_weights": (C.c_int, [C.POINTER(NbcTensor), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "nbc_packed_weights_flags": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int]),
    "nbc_arch_packed_weights_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "nbc_pack_weights_arch": (C.c_int, [C.POINTER(NbcTensor), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "nbc_packed_weights_flags_arch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "nbc_packed_weights_arch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int]),
    "nbc_arch_bn_affine_floats": (C.c_size_t, [C.c_int]),
    "nbc_pack_bn_affine": (C.c_int, [C.POINTER(NbcTensor), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "nbc_attach_bn_affine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "nbc_arch_bn_raw_floats": (C.c_size_t, [C.c_int]),
    "nbc_pack_bn_raw": (C.c_int, [C.POINTER(NbcTensor), C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "nbc_attach_bn_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "nbc_set_bn_statistics": (C.c_int, [C.c_void_p, C.c_int]),
    "nbc_weights_flags": (C.c_int, [C.c_void_p]),
    "nbc_activation_exponent": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]),
    "nbc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "nbc_destroy": (C.c_int, [C.c_void_p]),
    "nbc_attach_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "nbc_load_weights": (C.c_int, [C.c_void_p, C.POINTER(NbcTensor), C.c_int, C.c_int]),
    "nbc_attach_weights_arch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "nbc_load_weights_arch": (C.c_int, [C.c_void_p, C.POINTER(NbcTensor), C.c_int, C.c_int, C.c_int]),
    "nbc_set_normalization": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "nbc_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "nbc_describe_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "nbc_nonfinite_seen": (C.c_int, [C.c_void_p, C.c_int]),
    "nbc_nonfinite_peek_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nbc_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                              C.c_void_p]),
    "nbc_upsample_argmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "nbc_remove_small_zones": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "nbc_remove_small_zones_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p]),
    "nbc_confusion": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_image_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_target_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_lovasz_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nbc_lovasz_softmax": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "nbc_lovasz_groups_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_lovasz_softmax_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "nbc_pixel_ce_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nbc_pixel_cross_entropy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "nbc_softmax_census_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nbc_softmax_census": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "nbc_offset_sweep_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_offset_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                   C.POINTER(C.c_float), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "nbc_set_logit_offsets": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "nbc_dropout_mask": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_double, C.c_uint64, C.c_size_t, C.c_void_p]),
    "nbc_dropout_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_dropout_draws": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_uint64, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nbc_vote_decode": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "nbc_dropout_votes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_uint64, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "nbc_vote_summary": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nbc_vote_tally": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "nbc_tta_views": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_tta_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nbc_jitter_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "nbc_jitter_views": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nbc_views_mean": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_window_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nbc_window_views": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_window_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_bilinear_taps": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "nbc_training_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "nbc_head_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nbc_bicubic_taps": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32)]),
    "nbc_ce_gradient_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_ce_gradient": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 +
                        [C.POINTER(C.c_double), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "nbc_lovasz_gradient_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_lovasz_gradient": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 +
                            [C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6),
    "nbc_head_gradient_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nbc_head_gradient": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_void_p]),
    "nbc_zones_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nbc_label_zones": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "nbc_zone_match_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_match_zones": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                  C.c_void_p]),
    "nbc_contours_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nbc_contour_distances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nbc_resize_cubic_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "nbc_preprocess_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p]),
    "nbc_autotune": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p]),
    "nbc_get_plan_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "nbc_set_plan_tiles": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "nbc_default_conv_tile": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "nbc_conv_tile_info": (C.c_int, [C.c_int, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "nbc_bcast_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "nbc_set_conv_tile": (C.c_int, [C.c_void_p, C.c_int]),
    "nbc_set_keep_activations": (C.c_int, [C.c_void_p, C.c_int]),
    "nbc_set_fuse_downsample": (C.c_int, [C.c_void_p, C.c_int]),
    "nbc_fused_pairs": (C.c_int, [C.c_void_p]),
    "nbc_activation_peaks": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "nbc_read_activation": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_int64 * 4)]),
    "nbc_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "nbc_num_op_records": (C.c_int, [C.c_void_p]),
    "nbc_get_op_record": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(NbcOpRecord)]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libnbc_hip.so; raise loudly when it is missing (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library is the only implementation of this path. "
            "Build it with `python -m neuralbarkcalculator_amd.build` (needs hipcc).")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().nbc_last_error().decode("utf-8", "replace")


def check(rc: int, what: str = "") -> None:
    """Map the C ABI's integer error convention to Python exceptions (models.py callers expect
    ``RuntimeError`` from a bad ``load_state_dict``)."""
    if rc == NBC_OK:
        return
    msg = last_error()
    raise RuntimeError(f"{what + ': ' if what else ''}{msg} (nbc error {rc})")
