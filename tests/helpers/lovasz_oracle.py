"""Two host restatements of the per-image Lovasz-Softmax value that nbc_lovasz_softmax computes.

For one image: p = softmax(logits) over the 3 classes in float32; the class of a pixel is round(2 v / 255) of its grey
level.  For each class c with at least one target pixel (G of them): e = |fg - p_c|; order e from the largest down,
carrying fg along; with the running foreground count F_i and background count B_i of the first i + 1 sorted pixels,
J_i = 1 - (G - F_i) / (G + B_i), and the class's term is sum_i e_(i) (J_i - J_{i-1}) with J_{-1} = 0.  The loss is the
mean of the present classes' terms.  An absent class has term 0 and count 0.

* ``terms_torch_f32``: what the training code evaluates -- torch.sort descending, float32 cumulative sums and Jaccard
  steps -- except that the last dot product adds its float32 products in float64: a float32 ``torch.dot`` adds them in an
  order that depends on the CPU (the constant-logits image of tests/golden/ref_loss_65x127 moves by 9e-7 between two
  machines), and a restatement must say the same thing everywhere.
* ``terms_float64``: numpy in float64 from the same float32 errors (the adjudicating value).

Both are pinned to executed reference code: tests/test_reference_pins.py holds them (and ``target_classes``) to what
``LovaszSoftmax``, ``lovasz_softmax_flat(classes=[c])`` and the decode of dataset.py:188-198 returned on the images of
tests/golden/ref_loss_*.npz (oracle/record_reference.py), the ``'present'`` rule included, within the recorded float32
rounding ``d_ref`` + 1e-7.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch


def target_classes(grey: np.ndarray) -> np.ndarray:
    return ((np.asarray(grey).astype(np.int32) + 64) >> 7).astype(np.int64)


def softmax_f32(logits: np.ndarray) -> np.ndarray:
    """float32 softmax over axis 0 of a [3,H,W] array, as torch computes it."""
    return torch.softmax(torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)), dim=0).numpy()


def errors_f32(probs: np.ndarray, classes: np.ndarray, c: int) -> Tuple[np.ndarray, np.ndarray]:
    """(e float32 [P], fg float32 [P]) of class c."""
    fg = (np.asarray(classes).ravel() == c).astype(np.float32)
    return np.abs(fg - np.asarray(probs, dtype=np.float32)[c].ravel()), fg


def terms_torch_f32(logits: np.ndarray, grey: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(terms float64 [3], fg counts int64 [3]) for one image, the float32 torch way up to the final sum."""
    probs = softmax_f32(logits)
    classes = target_classes(grey)
    terms, counts = np.zeros(3), np.zeros(3, np.int64)
    for c in range(3):
        e, fg = errors_f32(probs, classes, c)
        counts[c] = int(fg.sum())
        if counts[c] == 0:
            continue
        e_t, fg_t = torch.from_numpy(e), torch.from_numpy(fg)
        e_sorted, order = torch.sort(e_t, 0, descending=True)
        g = fg_t[order]
        total = g.sum()
        jac = 1.0 - (total - g.cumsum(0)) / (total + (1 - g).cumsum(0))
        if len(jac) > 1:
            jac[1:] = jac[1:] - jac[:-1].clone()
        terms[c] = float(torch.dot(e_sorted.double(), jac.double()))
    return terms, counts


def terms_float64_from_probs(probs: np.ndarray, classes: np.ndarray, tie: str = "fg_first",
                             seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """float64 terms from float32 probabilities [3,H,W] and target classes [H,W].  ``tie`` orders equal errors:
    "fg_first", "bg_first" or "random" (the value does not depend on it)."""
    terms, counts = np.zeros(3), np.zeros(3, np.int64)
    rng = np.random.default_rng(seed)
    for c in range(3):
        e, fg = errors_f32(probs, classes, c)
        g = fg.astype(np.int64)
        G = int(g.sum())
        counts[c] = G
        if G == 0:
            continue
        second = {"fg_first": -g, "bg_first": g, "random": rng.permutation(len(g))}[tie]
        order = np.lexsort((second, -e.astype(np.float64)))
        es, gs = e[order].astype(np.float64), g[order]
        F = np.cumsum(gs)
        B = np.arange(1, len(gs) + 1) - F
        J = 1.0 - (G - F).astype(np.float64) / (G + B).astype(np.float64)
        dJ = np.diff(J, prepend=0.0)
        terms[c] = float(np.sum(es * dJ))
    return terms, counts


def terms_float64(logits: np.ndarray, grey: np.ndarray, tie: str = "fg_first") -> Tuple[np.ndarray, np.ndarray]:
    """float64 terms of one image from its logits [3,H,W] and grey dual [H,W]."""
    return terms_float64_from_probs(softmax_f32(logits), target_classes(grey), tie)


def loss(terms: np.ndarray, counts: np.ndarray) -> float:
    present = [float(t) for t, n in zip(terms, counts) if n > 0]
    return sum(present) / len(present) if present else 0.0
