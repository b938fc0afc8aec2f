"""The training run's own frame: ``pad_resize(img, T, T)`` (utils.py:242-247), restated on the host.

The reference's ``test_dataset`` -- the one ``val_miou`` and the ``test_*`` figures of ``exp.test`` come from
(__main__.py:209-228) -- passes every sample and its dual through ``pad_resize``: torchvision's ``pad(padding_mode='reflect')``
by ``ceil((T - L) / 2)`` on both sides of each axis, which is ``numpy.pad(mode="reflect")``, then ``resize`` to ``T x T``,
which is PIL's 8-bit bilinear ``ImagingResample`` and does something only where the padded length came out at ``T + 1``.

This module is the normative text of that arithmetic (include/nbc.h, nbc_training_frame): ``frame_geometry``
is the one rule of an axis, ``bilinear_taps`` PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for ``n + 1 -> n``,
``pad_resize_cpu`` the whole call in numpy integers.  The device kernel (csrc/training_frame.hip) is tested against it byte
for byte, and it against ``numpy.pad`` + ``PIL.Image.resize``.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

FRAME_TAPS = 3                                    # NBC_FRAME_TAPS: coefficients per output of a resampled axis
PRECISION_BITS = 22                               # PIL's 8bpc fixed point: 32 - 8 - 2


def frame_geometry(L: int, Lt: int) -> Tuple[int, int]:
    """``(p, Lp)`` of an axis of ``L`` source pixels framed to ``Lt``: the pad ``p = ceil((Lt - L) / 2)`` on both sides and the
    padded length ``Lp = L + 2 p``, which is ``Lt`` (a pure index map) or ``Lt + 1`` (the axis is resampled).  ``ValueError``
    for ``L < 1``, ``L > Lt`` (pad_resize would shrink: left out) and ``p > L - 1`` (one reflection must reach)."""
    L, Lt = int(L), int(Lt)
    if L < 1 or Lt < 1:
        raise ValueError("frame_geometry: lengths must be >= 1, got %d -> %d" % (L, Lt))
    if L > Lt:
        raise ValueError("frame_geometry: the source length %d exceeds the frame's %d" % (L, Lt))
    p = (Lt - L + 1) // 2
    if p > L - 1:
        raise ValueError("frame_geometry: a pad of %d needs more than one reflection of %d pixels" % (p, L))
    return p, L + 2 * p


def reflect_index(j: np.ndarray, L: int) -> np.ndarray:
    """``r(j)`` of ``numpy.pad(mode="reflect")`` for ``-(L - 1) <= j <= 2 (L - 1)``: ``-j`` below 0, ``2 (L - 1) - j`` from L on."""
    j = np.asarray(j, dtype=np.int64)
    return np.where(j < 0, -j, np.where(j >= L, 2 * (L - 1) - j, j))


def bilinear_taps(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """PIL's bilinear coefficient table for ``n_in = n_out + 1`` (Resample.c: ``precompute_coeffs`` then
    ``normalize_coeffs_8bpc``), in Python floats, which are C doubles, in the same order: ``first`` int32 ``[n_out]`` and
    ``coeff`` int32 ``[n_out, FRAME_TAPS]`` (unused taps are 0).  ``ValueError`` for any other pair of sizes."""
    n_in, n_out = int(n_in), int(n_out)
    if n_out < 1 or n_in != n_out + 1:
        raise ValueError("bilinear_taps serves in_size == out_size + 1 only, got %d -> %d" % (n_in, n_out))
    scale = float(n_in) / float(n_out)            # > 1: the filter is stretched by it
    support = 1.0 * scale
    ss = 1.0 / scale
    first = np.zeros(n_out, dtype=np.int32)
    coeff = np.zeros((n_out, FRAME_TAPS), dtype=np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        if xmax > FRAME_TAPS:
            raise ValueError("bilinear_taps: %d taps at output %d of %d -> %d" % (xmax, o, n_in, n_out))
        w, ww = [], 0.0
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coeff[o, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        first[o] = xmin
    return first, coeff


def _clip8(acc: np.ndarray) -> np.ndarray:
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _resample_axis0(a: np.ndarray, n_out: int) -> np.ndarray:
    """One pass of PIL's 8-bit resample along axis 0 of ``a`` (uint8, ``n_out + 1`` long there)."""
    first, coeff = bilinear_taps(a.shape[0], n_out)
    acc = np.full((n_out,) + a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for t in range(FRAME_TAPS):
        used = coeff[:, t] != 0
        idx = np.where(used, first + t, 0)        # an unused tap reads nothing: its index may lie beyond the axis
        k = coeff[:, t].astype(np.int64).reshape((n_out,) + (1,) * (a.ndim - 1))
        acc += a[idx].astype(np.int64) * k
    return _clip8(acc)


def pad_resize_cpu(img_u8: np.ndarray, Ht: int, Wt: int) -> np.ndarray:
    """``pad_resize`` (utils.py:242-247) of one uint8 image ``[H,W,3]`` or ``[H,W]`` to ``Ht x Wt``: the reflection pad as an
    index map, then per axis whose padded length is one too long PIL's 8-bit bilinear pass -- columns first, rounded to uint8,
    then rows on those bytes (``ImagingResample``'s order and its intermediate image)."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("pad_resize_cpu takes a uint8 [H,W,3] or [H,W] image")
    H, W = img.shape[:2]
    (py, Hp), (px, Wp) = frame_geometry(H, Ht), frame_geometry(W, Wt)
    a = img[reflect_index(np.arange(Hp) - py, H)][:, reflect_index(np.arange(Wp) - px, W)]
    if Wp != Wt:
        a = np.moveaxis(_resample_axis0(np.moveaxis(a, 1, 0), Wt), 0, 1)
    if Hp != Ht:
        a = _resample_axis0(a, Ht)
    return np.ascontiguousarray(a)


def table_of(first: np.ndarray, coeff: np.ndarray) -> np.ndarray:
    """The table nbc_training_frame reads for a resampled axis: int32 ``[n_out, 4]``, ``first[o]`` then ``coeff[o]``."""
    return np.ascontiguousarray(np.concatenate([np.asarray(first, dtype=np.int32)[:, None], np.asarray(coeff, dtype=np.int32)], axis=1))
