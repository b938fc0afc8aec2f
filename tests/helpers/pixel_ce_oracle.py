"""Two host restatements of the per-image cross-entropy sums that nbc_pixel_cross_entropy computes.

For one image with logits x [3,H,W] (float32) and a target class t per pixel (round(2 v / 255) of the dual's grey level):
the entropy of a pixel is ce = logsumexp(x) - x[t]; its predicted class p is the argmax of its logits (first maximum, a
NaN counts as the maximum).  S[a][b] is the sum of ce over the pixels with t == a and p == b, K[a][b] their number.  The
weighted loss the shipped checkpoint was trained on multiplies each pixel's entropy by w[max(p, t)] and takes the mean over
the pixels, which is sum(w[max(a, b)] S[a][b]) / P.

* ``sums_float64``: S and K in float64 from the float32 logits (the adjudicating value).
* ``reference_procedure_f32``: the weighted loss the training code's way, step by step in float32 torch.
* ``weighted_float64``: the same expression evaluated in float64 torch, pixel by pixel (no S in between).

All three are pinned to executed reference code: tests/test_reference_pins.py holds them (and ``target_classes``) to what
``CrossEntropyLoss``, ``CustomWeightedCrossEntropy`` (two weight vectors: the ``max(argmax, target)`` index) and ``MixedLoss``
returned on the images of tests/golden/ref_loss_*.npz (oracle/record_reference.py), a NaN image included, within the
recorded float32 rounding ``d_ref`` + 1e-7 relative.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def target_classes(grey: np.ndarray) -> np.ndarray:
    return ((np.asarray(grey).astype(np.int32) + 64) >> 7).astype(np.int64)


def pixel_entropies_float64(logits: np.ndarray, target_class: np.ndarray) -> np.ndarray:
    """ce [H,W] in float64 from float32 logits [3,H,W]: log(sum exp(x - m)) - (x_t - m) with m the largest logit."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    t = np.asarray(target_class).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.fmax(np.fmax(x[0], x[1]), x[2])
        s = np.exp(x[0] - m) + np.exp(x[1] - m) + np.exp(x[2] - m)
        xt = np.take_along_axis(x, t[None], axis=0)[0]
        return np.log(s) - (xt - m)


def _cell_sum(v: np.ndarray) -> float:
    if len(v) == 0:
        return 0.0
    if np.all(np.isfinite(v)):
        return math.fsum(v.tolist())
    with np.errstate(invalid="ignore"):
        return float(np.sum(v))


def sums_float64(logits: np.ndarray, target_grey: np.ndarray, labels: np.ndarray = None) -> Tuple[np.ndarray, np.ndarray]:
    """(S float64 [3,3], K int64 [3,3]) of one image; the predicted class is the argmax of the logits or, when given,
    ``labels`` [H,W]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    t = target_classes(target_grey)
    if labels is None:
        p = torch.argmax(torch.from_numpy(logits), dim=0).numpy()
    else:
        p = np.asarray(labels).astype(np.int64)
    ce = pixel_entropies_float64(logits, t)
    S, K = np.zeros((3, 3), np.float64), np.zeros((3, 3), np.int64)
    for a in range(3):
        for b in range(3):
            sel = (t == a) & (p == b)
            K[a, b] = int(sel.sum())
            S[a, b] = _cell_sum(ce[sel])
    return S, K


def _weighted(logits: np.ndarray, target_class: np.ndarray, weights: Sequence[float], dtype) -> float:
    x = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32))[None].to(dtype)
    true = torch.from_numpy(np.asarray(target_class).astype(np.int64))[None]
    w = torch.tensor([float(v) for v in weights], dtype=dtype)
    entropies = F.cross_entropy(x, true, reduction="none")
    larger = torch.max(torch.argmax(x, dim=1), true).flatten()
    per_pixel = torch.index_select(w, 0, larger).view(true.shape)
    return float((entropies * per_pixel).mean())


def reference_procedure_f32(logits: np.ndarray, target_class: np.ndarray, weights: Sequence[float]) -> float:
    """The weighted cross-entropy of one image as a batch of one, every step in float32."""
    return _weighted(logits, target_class, weights, torch.float32)


def weighted_float64(logits: np.ndarray, target_class: np.ndarray, weights: Sequence[float]) -> float:
    """The same steps on the float32 logits widened to float64."""
    return _weighted(logits, target_class, weights, torch.float64)
