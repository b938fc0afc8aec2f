"""Refit ``classifier.4`` of an fcn_resnet50 checkpoint on a labelled folder, the loss's gradient computed on the device.

``python -m neuralbarkcalculator_amd.refit ROOT --out refit_model.pt [--model_path best_model.pt]
[--loss ce|class_ce|weighted_ce|lovasz|mixed] [--class_weights W0 W1 W2 | --class_weights_from PATH] [--l2 L] [--iterations 50]
[--subset split.txt] [--holdout split.txt] [--precision auto|fp32|f16x2] [--stats PATH | --mean R G B --std R G B] [--gpus G]
[--batch B] [--streams S]``

``classifier.4`` (models.py:121) is a 1x1 convolution 512 -> 3 with bias: 1 539 parameters theta, linear in the features the
forward leaves on the device.  The definitions are in include/nbc.h and DESIGN.md 3.22; this module holds

* their host restatements in numpy float64 (``bicubic_taps_cpu``, ``ce_gradient_cpu``, ``head_gradient_cpu``, and for the
  Lovasz-Softmax loss ``lovasz_slopes_cpu``, ``lovasz_pixel_gradient_cpu``, ``lovasz_gradient_cpu``), which the tests hold the
  kernels to;
* ``table_of`` (the nine weights ``T[target class][argmax class]`` of a loss of the family), ``objective`` (the folder's
  objective and gradient from the per-image rows) and the checkpoint writer (``replace_head``, ``write_checkpoint``);
* the driver ``refit_folder`` on the folder-run engine (``folder_run``): fcn_resnet50 and running BatchNorm statistics only.

Each objective evaluation is one pass over the folder: the forward (the trunk is run again for every evaluation), then
``FCNResNet50.head_loss_and_gradient`` with the current theta.  The per-image rows (9 sums, 9 counts, 1 539 gradient doubles)
are gathered with the engine's ``gather``; rank 0 adds them in list order in float64, so the result does not depend on the
number of ranks, the batch or the streams, adds ``L/2 |theta - theta0|^2`` and feeds ``scipy.optimize.minimize(method=
"L-BFGS-B", jac=True)`` (``--iterations`` iterations, at most ``2 * iterations + 2`` evaluations).  The next theta, rounded to float32, is broadcast; the other ranks follow rank 0's commands.  The
theta written is the float32 theta of the best objective evaluated.

``--loss lovasz`` and ``--loss mixed`` fit the reference's own objectives (``LovaszSoftmax()``, __main__.py:236-239; ``MixedLoss`` =
``CustomWeightedCrossEntropy / 4 + LovaszSoftmax``, utils.py:185-192), image by image as ``evaluate --loss`` / ``--ce`` report
them: the objective is the mean over the evaluated images, in list order in float64, of ``lovasz_i`` or of ``wce_i / 4 +
lovasz_i``; every image's row also carries its three terms and foreground counts.  The Lovasz-Softmax loss is piecewise linear in
the probabilities and ``weighted_ce`` (so ``mixed``) jumps where a pixel's argmax changes: L-BFGS-B assumes neither and may stop
early; the theta written is still the best one evaluated.

Outputs: ``--out`` (the input state_dict with ``classifier.4.weight`` / ``.bias`` replaced: shapes, dtypes and key order
kept), ``results/refit_log.csv`` (one row per evaluation) and ``results/refit_summary.json``.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
from typing import Sequence, Tuple

import numpy as np

from . import folder_run, metrics

LOSSES = ("ce", "class_ce", "weighted_ce")       # the pixel-wise cross-entropy family: a table T is the whole loss
LOVASZ_LOSSES = ("lovasz", "mixed")              # per-image objectives: a row carries terms[3] and fg_counts[3] as well
ALL_LOSSES = LOSSES + LOVASZ_LOSSES              # what --loss takes
CIN, CLASSES = 512, 3
THETA = CLASSES * CIN + CLASSES                  # classifier.4.weight [3, 512], then classifier.4.bias [3]
W_KEY, B_KEY = "classifier.4.weight", "classifier.4.bias"
ROW_WIDTH = 2 + 9 + 9 + THETA                    # (global_idx, status, sums[9] f64 bits, counts[9], grad[3][513] f64 bits)
LOVASZ_ROW_WIDTH = ROW_WIDTH + 3 + 3             # ... then terms[3] f64 bits, fg_counts[3]
LOG_CSV = os.path.join("results", "refit_log.csv")
SUMMARY_JSON = os.path.join("results", "refit_summary.json")
LOG_HEADER = ["evaluation", "objective", "data_term", "gradient_norm", "accepted"]
CMD_STOP, CMD_FIT, CMD_HOLDOUT = 0, 1, 2


# ---- host restatements ------------------------------------------------------------------------------------------------------
def bicubic_taps_cpu(n_in: int, n_out: int, dtype=np.float32):
    """``nbc_bicubic_taps`` on the host: ``(idx int32 [n_out, 4], coeff dtype [n_out, 4], lo int32 [n_in], hi int32 [n_in])``.
    In float32 (the default) it is the library's table operation for operation (numpy rounds every product and sum on its
    own); in float64 it is what ``F.interpolate(mode='bicubic', align_corners=False)`` computes on float64 tensors."""
    f = np.dtype(dtype).type
    n_in, n_out = int(n_in), int(n_out)
    scale = f(n_in) / f(n_out)
    o = np.arange(n_out).astype(f)
    s = scale * (o + f(0.5)) - f(0.5)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    t = np.minimum(np.maximum(s - i0.astype(f), f(0)), f(1))
    A, one = f(-0.75), f(1)
    x1, x2 = t, one - t
    coeff = np.stack([((A * (x1 + one) - f(5) * A) * (x1 + one) + f(8) * A) * (x1 + one) - f(4) * A,
                      ((A + f(2)) * x1 - (A + f(3))) * x1 * x1 + one,
                      ((A + f(2)) * x2 - (A + f(3))) * x2 * x2 + one,
                      ((A * (x2 + one) - f(5) * A) * (x2 + one) + f(8) * A) * (x2 + one) - f(4) * A], axis=1).astype(f)
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1).astype(np.int32)
    outs = np.repeat(np.arange(n_out, dtype=np.int64), 4)
    first = np.full(n_in, n_out, dtype=np.int64)
    hi = np.full(n_in, -1, dtype=np.int64)
    np.minimum.at(first, idx.ravel(), outs)
    np.maximum.at(hi, idx.ravel(), outs)
    lo = np.where(hi >= 0, first, 0)
    return idx, coeff, lo.astype(np.int32), hi.astype(np.int32)


def _adjoint_matrices(taps, n_in: int):
    """A [n_in, n_out] with A[i, o] = the sum of the coefficients of output o's taps on input i (float64), the same of their
    absolute values, and the number of those taps."""
    idx, coeff = np.asarray(taps[0]), np.asarray(taps[1], dtype=np.float64)
    n_out = idx.shape[0]
    outs = np.repeat(np.arange(n_out), 4)
    A, B, K = (np.zeros((n_in, n_out), dtype=np.float64) for _ in range(3))
    np.add.at(A, (idx.ravel(), outs), coeff.ravel())
    np.add.at(B, (idx.ravel(), outs), np.abs(coeff).ravel())
    np.add.at(K, (idx.ravel(), outs), 1.0)
    return A, B, K


def pixel_gradient_cpu(logits_full: np.ndarray, grey: np.ndarray, table) -> np.ndarray:
    """Item 4 of the definitions for one image: ``g_c = T[t][p] (softmax_c - [c = t])`` in float64 from the logits ``[3, H, W]``
    (float32 as the device holds them; float64 logits are taken as they are) and the grey mask ``[H, W]``; p = the first
    maximum of the logits as given (a NaN counts as the maximum)."""
    x32 = np.asarray(logits_full)
    x = x32.astype(np.float64)
    T = np.asarray(table, dtype=np.float64).reshape(3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax(np.fmax(x[0], x[1]), x[2])
        e = np.exp(x - m)
        q = e / e.sum(axis=0)
    t = metrics.target_classes(grey)
    p = np.argmax(x32, axis=0)
    onehot = (np.arange(3)[:, None, None] == t[None]).astype(np.float64)
    return T[t, p][None] * (q - onehot)


def _upsample_adjoint_cpu(g: np.ndarray, h: int, w: int, taps, mag=None):
    """Item 5 on the pixel gradient ``g`` float64 ``[3, H, W]``: ``grad`` float64 ``[3, h, w]``; with ``mag`` (a bound on the
    absolute value of every pixel's terms, ``[3, H, W]``) also the same sum over ``mag`` and each cell's number of taps."""
    H, W = g.shape[1:]
    if taps is None:
        taps = (bicubic_taps_cpu(h, H), bicubic_taps_cpu(w, W))
    Ay, By, Ky = _adjoint_matrices(taps[0], h)
    Ax, Bx, Kx = _adjoint_matrices(taps[1], w)
    bad = ~np.isfinite(g)
    grad = np.matmul(np.matmul(Ay, np.where(bad, 0.0, g)), Ax.T)
    if bad.any():                                    # a pixel that is not finite reaches the cells its taps land on, no other
        grad[np.matmul(np.matmul((Ky > 0).astype(np.float64), bad.astype(np.float64)), (Kx > 0).astype(np.float64).T) > 0] = np.nan
    if mag is None:
        return grad
    low = np.matmul(np.matmul(By, mag), Bx.T)
    terms = np.matmul(Ky, np.ones((H, W))) @ Kx.T
    return grad, low, np.broadcast_to(terms, grad.shape)


def ce_gradient_cpu(logits_full: np.ndarray, grey: np.ndarray, h: int, w: int, table, taps=None, return_abs: bool = False):
    """Items 4 and 5 for one image: float64 ``[3, h, w]``, the gradient of ``sum T[t][p] ce`` with respect to the
    low-resolution logits, not normalised.  ``taps``: ``(row_taps, col_taps)`` as ``bicubic_taps_cpu`` / ``model.bicubic_taps``
    return them (default: the float32 tables).  ``return_abs``: also the sum of the absolute values of every cell's terms
    and their number (what a bound on the summation order is stated against)."""
    g = pixel_gradient_cpu(logits_full, grey, table)
    return _upsample_adjoint_cpu(g, h, w, taps, np.abs(g) if return_abs else None)


# ---- the Lovasz-Softmax gradient (include/nbc.h, nbc_lovasz_gradient) ------------------------------------------------------------
def lovasz_keys_cpu(e: np.ndarray, fg: np.ndarray) -> np.ndarray:
    """The sort keys ``bits(e) << 1 | fg`` of errors ``e`` in [0, 1]: int32 from float32 errors (what the device sorts), int64
    from float64 errors (the same order at full precision, for a pin against float64 autograd)."""
    e = np.ascontiguousarray(e)
    if e.dtype == np.float32:
        return ((e.view(np.int32) << 1) | np.asarray(fg).astype(np.int32)).astype(np.int32)
    return (np.ascontiguousarray(e, dtype=np.float64).view(np.int64) << 1) | np.asarray(fg).astype(np.int64)


def _decode_keys(keys: np.ndarray):
    k = np.ascontiguousarray(keys)
    if k.dtype.itemsize == 8:
        return (k.view(np.int64) >> 1).view(np.float64), (k.view(np.int64) & 1).astype(bool)
    k = k.view(np.int32)
    return (k >> 1).view(np.float32), (k & 1).astype(bool)


def lovasz_slopes_cpu(e: np.ndarray, fg: np.ndarray) -> np.ndarray:
    """The slope of one class's Lovasz term with respect to every pixel's error: ``e`` (any float dtype, any shape) and the
    foreground mask ``fg`` of the class -> float64 of ``e``'s shape.  Sorted descending by ``(e, fg)`` -- equal ``e`` puts
    foreground first --, with ``J(k, F) = 1 - (G - F) / (G + k - F)`` after ``k`` keys of which ``F`` are foreground, every pixel of
    a run of identical ``(e, fg)`` that starts at position ``r``, is ``R`` long and has ``F_r`` foreground keys before it gets
    ``[J(r + R, F_r + fg R) - J(r, F_r)] / R``: ``J_i - J_(i-1)`` at the pixel's position where nothing ties.  0 where ``e == 0``
    and for a class without foreground."""
    e = np.asarray(e)
    shape = e.shape
    e = e.reshape(-1)
    f = np.asarray(fg).reshape(-1).astype(bool)
    out = np.zeros(e.size, dtype=np.float64)
    G = int(f.sum())
    if G == 0 or e.size == 0:
        return out.reshape(shape)
    order = np.lexsort((~f, -e))                     # e descending, then foreground first
    es, fs = e[order], f[order]
    new_run = np.concatenate([[True], (es[1:] != es[:-1]) | (fs[1:] != fs[:-1])])
    starts = np.flatnonzero(new_run)
    lengths = np.diff(np.concatenate([starts, [e.size]]))
    before = np.concatenate([[0], np.cumsum(fs)])[starts]
    J = lambda k, F: 1.0 - (G - F).astype(np.float64) / (G + k - F).astype(np.float64)
    mean = (J(starts + lengths, before + fs[starts] * lengths) - J(starts, before)) / lengths
    slopes = mean[np.cumsum(new_run) - 1]
    slopes[es == 0] = 0.0
    out[order] = slopes
    return out.reshape(shape)


def lovasz_pixel_gradient_cpu(logits_full: np.ndarray, grey: np.ndarray, keys=None, table=None, lovasz_weight: float = 1.0,
                              return_abs: bool = False):
    """The pixel gradient of ``sum T'[t][p] ce + lovasz_weight * L`` of one image, float64 ``[3, H, W]``: ``L`` the image's
    Lovasz-Softmax loss, ``g_k = T'[t][p] (q_k - [k = t]) + lovasz_weight * q_k (d_k - sum_c d_c q_c)`` with ``q`` the float64
    softmax of the logits as given, ``d_c = -sign(fg - p_c) slope_c / C_p`` (``lovasz_slopes_cpu``; ``C_p`` the classes with a
    foreground pixel).  ``keys``: ``[3, H, W]`` of ``bits(e) << 1 | fg`` (``lovasz_keys_cpu``; 32-bit from float32 errors, as the
    device exports them, or 64-bit from float64 ones) -- the order, the sign and the ``e == 0`` test come from them; default:
    the keys of torch's float32 softmax.  ``table``: nine numbers or None; the first term only with a table, the second only
    with a weight other than 0.  An image whose softmax is not finite somewhere has NaN in every pixel of the second term.
    ``return_abs``: also the sum of the absolute values of every element's terms, and a count of their roundings."""
    x32 = np.asarray(logits_full)
    x = x32.astype(np.float64)
    t = metrics.target_classes(grey)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax(np.fmax(x[0], x[1]), x[2])
        ex = np.exp(x - m)
        q = ex / ex.sum(axis=0)
    onehot = np.arange(3)[:, None, None] == t[None]
    g, mag = np.zeros_like(q), np.zeros_like(q)
    if table is not None:
        T = np.asarray(table, dtype=np.float64).reshape(3, 3)
        wgt = T[t, np.argmax(x32, axis=0)][None]
        g = wgt * (q - onehot)
        mag = np.abs(wgt) * np.abs(q - onehot)
    lam = float(lovasz_weight)
    if lam != 0.0:
        if not np.isfinite(q).all():
            lov = np.full_like(q, np.nan)
            lmag = lov
        else:
            if keys is None:
                import torch
                p32 = torch.softmax(torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)), dim=0).numpy()
                keys = lovasz_keys_cpu(np.abs(onehot.astype(np.float32) - p32), onehot)
            e, fg = _decode_keys(np.asarray(keys).reshape(3, -1))
            present = int(sum(bool(fg[c].any()) for c in range(3)))
            d = np.zeros((3, e.shape[1]), dtype=np.float64)
            for c in range(3):
                if fg[c].any():
                    d[c] = np.where(fg[c], -1.0, 1.0) * (lovasz_slopes_cpu(e[c], fg[c]) / present)
            d = d.reshape(q.shape)
            dot = d[0] * q[0] + d[1] * q[1] + d[2] * q[2]
            lov = q * (d - dot[None])
            lmag = q * (np.abs(d) + (np.abs(d) * q).sum(axis=0)[None])
        g = g + lam * lov if table is not None else lam * lov
        mag = mag + abs(lam) * lmag
    if not return_abs:
        return g
    return g, mag, np.full(g.shape, 8.0)


def lovasz_gradient_cpu(logits_full: np.ndarray, grey: np.ndarray, h: int, w: int, keys=None, table=None,
                        lovasz_weight: float = 1.0, taps=None, return_abs: bool = False):
    """``lovasz_pixel_gradient_cpu`` carried through the adjoint of the bicubic upsample (item 5): float64 ``[3, h, w]``, not
    normalised.  ``return_abs``: also the sum of the absolute values of every cell's terms and their number."""
    if not return_abs:
        return _upsample_adjoint_cpu(lovasz_pixel_gradient_cpu(logits_full, grey, keys, table, lovasz_weight), h, w, taps)
    g, mag, pixel_terms = lovasz_pixel_gradient_cpu(logits_full, grey, keys, table, lovasz_weight, return_abs=True)
    grad, low, terms = _upsample_adjoint_cpu(g, h, w, taps, mag)
    return grad, low, terms + float(pixel_terms.flat[0])


def head_gradient_cpu(grad_lowres: np.ndarray, X: np.ndarray, return_abs: bool = False):
    """Item 6 for one image: ``grad_lowres`` float64 ``[3, h, w]`` and the features ``X`` ``[512, h, w]`` (the network's
    units) -> float64 ``[3, 513]``: a class's 512 weight columns, then its bias."""
    G = np.asarray(grad_lowres, dtype=np.float64).reshape(CLASSES, -1)
    Xm = np.asarray(X).astype(np.float64).reshape(CIN, -1)
    out = np.concatenate([G @ Xm.T, G.sum(axis=1, keepdims=True)], axis=1)
    if not return_abs:
        return out
    mag = np.concatenate([np.abs(G) @ np.abs(Xm).T, np.abs(G).sum(axis=1, keepdims=True)], axis=1)
    return out, mag


# ---- the loss family, the objective, the checkpoint ---------------------------------------------------------------------------
def table_of(loss: str, weights=None) -> np.ndarray:
    """``T[target class t][argmax class p]`` as float64 ``[3, 3]``: ``ce`` -- 1; ``class_ce`` -- ``w[t]``; ``weighted_ce`` --
    ``w[max(t, p)]``, CustomWeightedCrossEntropy (utils.py:151-165); ``mixed`` -- that table as well (MixedLoss's
    cross-entropy part, before its division by four).  ``lovasz`` has no table.  ``weights`` default to the reference's."""
    if loss not in LOSSES + ("mixed",):
        raise ValueError("loss must be one of %s, got %r" % (", ".join(LOSSES + ("mixed",)), loss))
    if loss == "ce":
        return np.ones((3, 3), dtype=np.float64)
    w = np.asarray(metrics.REFERENCE_CLASS_WEIGHTS if weights is None else weights, dtype=np.float64).reshape(-1)
    if w.size != 3 or not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("class weights must be three finite numbers >= 0, got %r" % (weights,))
    t, p = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    return w[t] if loss == "class_ce" else w[np.maximum(t, p)]


def theta_vector(grad_rows: np.ndarray) -> np.ndarray:
    """``[3, 513]`` (a class's weights, then its bias) in theta's order: the weight ``[3, 512]``, then the bias ``[3]``."""
    g = np.asarray(grad_rows, dtype=np.float64).reshape(CLASSES, CIN + 1)
    return np.concatenate([g[:, :CIN].ravel(), g[:, CIN]])


def image_losses(row, table) -> Tuple[float, float]:
    """``(lovasz_i, wce_i / 4 + lovasz_i)`` of one image's row ``(sums, counts, grad, terms, fg_counts)``: the ``lovasz_softmax``
    and ``mixed_loss`` columns of ``evaluate``, ``wce_i = sum(T * sums) / P_i`` with ``P_i`` the image's pixels."""
    sums, counts, _, terms, fg = row
    lov = float(metrics.lovasz_loss(np.asarray(terms, dtype=np.float64).reshape(3), np.asarray(fg).reshape(3)))
    T = np.asarray(table, dtype=np.float64).reshape(3, 3)
    wce = float((T * np.asarray(sums, dtype=np.float64).reshape(3, 3)).sum()) / int(np.asarray(counts).sum())
    return lov, metrics.mixed_loss(wce, lov)


def loss_means(rows, table) -> Tuple[float, float]:
    """The folder's ``(lovasz_softmax, mixed_loss)``: the means of ``image_losses`` over the rows, added in list order."""
    lov = mixed = 0.0
    for row in rows:
        a, b = image_losses(row, table)
        lov, mixed = lov + a, mixed + b
    return lov / len(rows), mixed / len(rows)


def objective(rows, table, l2: float, theta, theta0, loss: str = None) -> Tuple[float, float, np.ndarray]:
    """The folder's objective at ``theta`` from the per-image ``rows`` (``(sums [3,3], counts [3,3], grad [3,513])`` each, in
    list order): ``(value, data term, gradient float64 [1539])``.  The data term is ``sum over images of sum(T * sums)``
    over the sum of their pixels, added image by image in float64; the value adds ``l2 / 2 |theta - theta0|^2``.
    ``loss`` ``"lovasz"`` / ``"mixed"``: the rows are ``(sums, counts, grad, terms [3], fg_counts [3])``, ``grad`` the gradient of
    the image's own loss (``image_losses``); the data term is the mean of those losses over the images and the gradient the
    mean of theirs, both added in list order."""
    T = np.asarray(table, dtype=np.float64).reshape(3, 3)
    if loss in LOVASZ_LOSSES:
        if not rows:
            raise ValueError("objective: no rows")
        total, grad = 0.0, np.zeros((CLASSES, CIN + 1), dtype=np.float64)
        for row in rows:
            total += image_losses(row, T)[loss == "mixed"]
            grad = grad + np.asarray(row[2], dtype=np.float64).reshape(CLASSES, CIN + 1)
        d = np.asarray(theta, dtype=np.float64).reshape(-1) - np.asarray(theta0, dtype=np.float64).reshape(-1)
        data = total / len(rows)
        return data + 0.5 * float(l2) * float(d @ d), data, theta_vector(grad) / len(rows) + float(l2) * d
    total, pixels, grad = 0.0, 0, np.zeros((CLASSES, CIN + 1), dtype=np.float64)
    for sums, counts, g in rows:
        total += float((T * np.asarray(sums, dtype=np.float64).reshape(3, 3)).sum())
        pixels += int(np.asarray(counts).sum())
        grad = grad + np.asarray(g, dtype=np.float64).reshape(CLASSES, CIN + 1)
    if pixels == 0:
        raise ValueError("objective: the rows hold no pixel")
    d = np.asarray(theta, dtype=np.float64).reshape(-1) - np.asarray(theta0, dtype=np.float64).reshape(-1)
    data = total / pixels
    return data + 0.5 * float(l2) * float(d @ d), data, theta_vector(grad) / pixels + float(l2) * d


def theta_of(state_dict) -> np.ndarray:
    """theta of a state_dict (torch tensors or numpy arrays): float32 ``[1539]``."""
    w, b = (np.asarray(state_dict[k].detach().cpu().numpy() if hasattr(state_dict[k], "detach") else state_dict[k]) for k in (W_KEY, B_KEY))
    if w.shape != (CLASSES, CIN, 1, 1) or b.shape != (CLASSES,):
        raise ValueError("%s / %s have shapes %r / %r, not [3,512,1,1] / [3]" % (W_KEY, B_KEY, w.shape, b.shape))
    return np.concatenate([w.reshape(-1), b.reshape(-1)]).astype(np.float32)


def replace_head(state_dict, theta):
    """A copy of ``state_dict`` (same keys in the same order, every other value the same object) with ``classifier.4.weight`` /
    ``.bias`` holding ``theta``: shapes ``[3,512,1,1]`` / ``[3]`` and each value's own type and dtype kept."""
    th = np.asarray(theta, dtype=np.float32).reshape(-1)
    if th.size != THETA:
        raise ValueError("theta must hold %d values" % THETA)
    theta_of(state_dict)                             # the shapes
    new = {W_KEY: th[:CLASSES * CIN].reshape(CLASSES, CIN, 1, 1), B_KEY: th[CLASSES * CIN:].copy()}
    out = type(state_dict)()
    for k, v in state_dict.items():
        if k in new:
            if hasattr(v, "detach"):
                import torch
                v = torch.from_numpy(np.ascontiguousarray(new[k])).to(v.dtype)
            else:
                v = np.ascontiguousarray(new[k]).astype(np.asarray(v).dtype)
        out[k] = v
    return out


def write_checkpoint(state_dict, theta, path: str) -> None:
    """``torch.save`` of ``replace_head(state_dict, theta)``: loadable by predict, evaluate and the reference's predict.py."""
    import torch
    torch.save(replace_head(state_dict, theta), path)


def _figures(conf) -> dict:
    conf = np.asarray(conf, dtype=np.int64).reshape(3, 3)
    return {"confusion": conf.tolist(), "iou": [float(v) for v in metrics.iou(conf)], "f1": [float(v) for v in metrics.f1(conf)]}


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def refit_folder(root: str, out: str, model_path: str = "./best_model.pt", loss: str = "ce", class_weights=None,
                 class_weights_source: str = "reference", l2: float = 0.0, iterations: int = 50, subset=None, holdout=None,
                 precision: str = "fp32", device_index: int = None, batch: int = None, streams: int = None,
                 target_size: int = 1024, window: int = 64, precision_auto: bool = False, calibrate: bool = True,
                 normalization=None, normalization_source: str = None, image_loss: str = None) -> dict:
    """Refits ``classifier.4`` of the checkpoint at ``model_path`` on the labelled samples of ``root`` (module docstring) and
    writes ``out``, ``results/refit_log.csv`` and ``results/refit_summary.json``.  ``subset`` / ``holdout``: a path or a list of
    ``wood_type/name`` lines; the held-out samples are never fitted on (without ``subset`` the fit runs on every other
    sample).  ``ValueError`` before any device is touched: an unknown loss, weights that are not three finite numbers >= 0, a
    negative or non-finite ``l2``, ``iterations`` < 1, a precision other than fp32 / f16x2, a sample on both lists, an empty
    list.  ``loss`` names a member of the pixel-pooled cross-entropy family (``LOSSES``) and nothing else; the per-image
    objectives are asked for with ``image_loss`` = ``"lovasz"`` or ``"mixed"`` (``LOVASZ_LOSSES``; ``loss`` then stays at its
    default), which is what ``--loss lovasz|mixed`` of the command line passes.  Returns the engine's statistics, with
    ``summary`` on rank 0."""
    import torch
    from . import evaluate as ev
    from .topology import out_hw
    if loss not in LOSSES:
        raise ValueError("loss must be one of %s (the per-image objectives %s are image_loss), got %r"
                         % (", ".join(LOSSES), ", ".join(LOVASZ_LOSSES), loss))
    if image_loss is not None:
        if image_loss not in LOVASZ_LOSSES:
            raise ValueError("image_loss must be one of %s, got %r" % (", ".join(LOVASZ_LOSSES), image_loss))
        if loss != "ce":
            raise ValueError("image_loss stands in place of loss: leave loss at its default, got %r" % (loss,))
        loss = image_loss                            # from here on the objective's name, as the summary has it
    T = table_of(loss, class_weights) if loss != "lovasz" else np.zeros((3, 3), dtype=np.float64)   # lovasz: no cross-entropy part
    lov = loss in LOVASZ_LOSSES                      # a per-image objective: rows carry the terms and foreground counts
    width = LOVASZ_ROW_WIDTH if lov else ROW_WIDTH
    l2, iterations = float(l2), int(iterations)
    if not (np.isfinite(l2) and l2 >= 0):
        raise ValueError("--l2 must be finite and >= 0, got %r" % (l2,))
    if iterations < 1:
        raise ValueError("--iterations must be >= 1, got %d" % iterations)
    if precision not in ("fp32", "f16x2"):
        raise ValueError("refit runs in precision fp32 or f16x2 (the gradient is for an f32-grade forward), not %r" % (precision,))
    listed = ev.list_labelled(root)
    lines = lambda s: ev.read_subset(s) if isinstance(s, str) else list(s)
    held = ev.apply_subset(listed, lines(holdout)) if holdout is not None else []
    held_keys = {d["wood"] + "/" + d["name"] for d in held}
    if subset is not None:
        items = ev.apply_subset(listed, lines(subset))
        both = [d["wood"] + "/" + d["name"] for d in items if d["wood"] + "/" + d["name"] in held_keys]
        if both:
            raise ValueError("--holdout: %r is on the --subset list as well: a held-out sample is never fitted on" % both[0])
    else:
        items = [d for d in listed if d["wood"] + "/" + d["name"] not in held_keys]
    if not items:
        raise ValueError("refit: no sample to fit on under %s" % root)

    r = folder_run.open_run(root, "refit", precision, device_index, batch, streams, target_size)
    dev, nb = r.dev, r.batch

    def warm(m):                                     # the workspaces of the largest batch, and the tap tables of its axes
        lg = torch.zeros((nb, 3, target_size, target_size), dtype=torch.float32, device=dev)
        tg = torch.zeros((nb, target_size, target_size), dtype=torch.uint8, device=dev)
        m.pixel_cross_entropy(lg, tg)
        if lov:
            m.lovasz_gradient(lg, tg, out_hw(target_size, target_size, "fcn_resnet50"), T if loss == "mixed" else None, 1.0)
        else:
            m.ce_gradient(lg, tg, out_hw(target_size, target_size, "fcn_resnet50"), T)
    folder_run.bring_up(r, model_path, "fcn_resnet50", "running", precision_auto,
                        lambda root_: os.makedirs(os.path.join(root_, "results"), exist_ok=True), warm, normalization=normalization)

    state_dict = torch.load(model_path, map_location="cpu", weights_only=True) if r.rank == 0 else None
    theta0 = theta_of(state_dict) if r.rank == 0 else np.zeros(THETA, dtype=np.float32)

    def command(code: int, theta) -> Tuple[int, np.ndarray]:
        """Rank 0's next step for every rank: one broadcast of (code, theta as float64)."""
        if r.dist is None:
            return code, np.asarray(theta, dtype=np.float32)
        msg = torch.zeros(1 + THETA, dtype=torch.float64)
        if r.rank == 0:
            msg[0] = code
            msg[1:] = torch.from_numpy(np.asarray(theta, dtype=np.float64))
        msg = msg.to(r.wire_dev)
        r.dist.broadcast(msg, src=0)
        msg = msg.cpu().numpy()
        return int(msg[0]), msg[1:].astype(np.float32)

    sizes_of = {}

    def size_of(d):
        if d["src"] not in sizes_of:
            sizes_of[d["src"]] = ev.image_hw(d["src"])
        return sizes_of[d["src"]]

    ring = [torch.empty((nb, 9 + THETA + (3 if lov else 0)), dtype=torch.float64).pin_memory() for _ in range(r.depth)]
    cring = [torch.empty((nb, 9 + (3 if lov else 0)), dtype=torch.int64).pin_memory() for _ in range(r.depth)]
    logits_buf = [torch.empty(nb * 3 * target_size * target_size, dtype=torch.float32, device=dev) for _ in range(r.n_streams)]
    passes = [0]

    def run_pass(which, theta):
        """One pass over ``which`` with ``theta`` on every rank: the gathered rows of the samples that could be evaluated, in
        list order, as ``(global index, sums, counts, grad)`` -- then ``terms, fg_counts`` for the Lovasz losses --, and the
        number of samples listed."""
        sizes = folder_run.shard(r, which, size_of)
        mine = r.mine
        rows = np.zeros((len(mine), width), dtype=np.int64)
        rows[:, 0], rows[:, 1] = mine, -1            # a row nobody filled counts nowhere
        theta_dev = torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float32)).to(dev)
        torch.cuda.synchronize(dev)                  # the side streams read it

        def prepare(k):
            gi = mine[k]
            h, w = sizes[gi]
            status = ev.dual_status(which[gi], h, w, target_size)
            if status == ev.STATUS_OK:
                frame, grey = ev._decode_rgb(which[gi]["src"]), ev.decode_dual(which[gi]["dual"])
                if grey.shape == frame.shape[:2]:
                    return frame, grey
                status = ev.STATUS_SHAPE_MISMATCH
            rows[k, :2] = (gi, status)
            return None

        def launch(slot, sid, part, x, tgt):
            mdl = r.models[sid]
            n, h, w = x.shape[:3]
            mdl.lowres_logits(x)                     # the trunk and classifier.0: the features stay on the device
            full = logits_buf[sid][: n * 3 * h * w].view(n, 3, h, w)
            if lov:                                  # the image's own loss: wce_i / 4 + lovasz_i has T / (4 P_i) on its pixels
                sums, counts, grad, terms, fg = mdl.head_loss_and_gradient(
                    tgt, theta_dev, T / (4.0 * h * w) if loss == "mixed" else None, logits_full=full, lovasz_weight=1.0)
                ring[slot][:n, 9 + THETA:].copy_(terms, non_blocking=True)
                cring[slot][:n, 9:].copy_(fg, non_blocking=True)
            else:
                sums, counts, grad = mdl.head_loss_and_gradient(tgt, theta_dev, T, logits_full=full)
            ring[slot][:n, :9].copy_(sums.view(n, 9), non_blocking=True)
            ring[slot][:n, 9:9 + THETA].copy_(grad.view(n, THETA), non_blocking=True)
            cring[slot][:n, :9].copy_(counts.view(n, 9), non_blocking=True)

        def consume(slot, part, n, h, w):
            vals, cnts = ring[slot].numpy(), cring[slot].numpy()
            for j, k in enumerate(part):
                rows[k, :2] = (mine[k], ev.STATUS_OK)
                rows[k, 2:11] = vals[j, :9].view(np.int64)
                rows[k, 11:20] = cnts[j, :9]
                rows[k, 20:ROW_WIDTH] = vals[j, 9:9 + THETA].view(np.int64)
                if lov:
                    rows[k, ROW_WIDTH:ROW_WIDTH + 3] = vals[j, 9 + THETA:].view(np.int64)
                    rows[k, ROW_WIDTH + 3:] = cnts[j, 9:]

        def first_frame():
            first = next((gi for gi in mine if max(sizes[gi]) <= target_size), None)
            return None if first is None else ev._decode_rgb(which[first]["src"])

        folder_run.run_loop(r, window, prepare, launch, consume, first_frame, calibrate and passes[0] == 0, bytes_per_pixel=(3, 1))
        passes[0] += 1
        allrows = folder_run.gather(r, rows, width)
        more = (lambda g: (g[ROW_WIDTH:ROW_WIDTH + 3].view(np.float64), g[ROW_WIDTH + 3:])) if lov else (lambda g: ())
        return [(int(g[0]), g[2:11].view(np.float64).reshape(3, 3), g[11:20].reshape(3, 3),
                 g[20:ROW_WIDTH].view(np.float64).reshape(3, CIN + 1)) + more(g)
                for g in allrows if int(g[1]) == ev.STATUS_OK], len(allrows)

    def follow():
        """Every rank but 0: the passes rank 0 asks for, until it says stop."""
        while True:
            code, theta = command(CMD_STOP, None)
            if code == CMD_STOP:
                return
            run_pass(items if code == CMD_FIT else held, theta)

    def held_figures(theta):
        command(CMD_HOLDOUT, theta)
        rows, _ = run_pass(held, theta)
        if not rows:
            return None
        value, data, _ = objective([g[1:] for g in rows], T, 0.0, theta, theta, loss)
        return dict(_figures(sum(g[2] for g in rows)), objective=data, images=len(rows), **named_means(rows))

    def named_means(rows) -> dict:
        """The folder's ``lovasz_softmax`` (and for ``mixed`` its ``mixed_loss``) from the rows of a pass; nothing otherwise."""
        if not lov:
            return {}
        means = loss_means([g[1:] for g in rows], T)
        return dict(lovasz_softmax=means[0], **({"mixed_loss": means[1]} if loss == "mixed" else {}))

    summary = None
    if r.rank != 0:
        follow()
    else:
        from scipy.optimize import minimize
        log, best, first_conf = [], None, []         # best: (objective, theta float32, pooled counts, data term, images, skipped,
        first_means = []                             #        named_means)

        class Stop(Exception):
            pass

        class Budget(Stop):
            pass

        def fun(x):
            nonlocal best
            theta = np.asarray(x, dtype=np.float64).astype(np.float32)
            if len(log) >= 2 * iterations + 2:       # scipy counts evaluations between iterations only: a long line search
                raise Budget("the budget of %d evaluations is spent" % len(log))
            command(CMD_FIT, theta)
            rows, listed_n = run_pass(items, theta)
            if not rows:
                raise ValueError("refit: none of the %d listed samples could be evaluated (no dual, another shape, or larger "
                                 "than %d pixels a side)" % (listed_n, target_size))
            value, data, grad = objective([g[1:] for g in rows], T, l2, theta, theta0, loss)
            accepted = bool(np.isfinite(value)) and (best is None or value <= best[0])
            if not log:
                first_conf.append(sum(g[2] for g in rows))
                first_means.append(named_means(rows))
            log.append([len(log) + 1, repr(float(value)), repr(float(data)), repr(float(np.sqrt(grad @ grad))), int(accepted)])
            if accepted:
                best = (float(value), theta.copy(), sum(g[2] for g in rows), float(data), len(rows), listed_n - len(rows),
                        named_means(rows))
            if not np.isfinite(value):
                raise Stop("evaluation %d: the objective is not finite (%r)" % (len(log), float(value)))
            return float(value), grad

        try:
            before_held = held_figures(theta0) if held else None
            stopped = None
            try:
                res = minimize(fun, theta0.astype(np.float64), jac=True, method="L-BFGS-B",
                               options={"maxiter": iterations, "maxfun": 2 * iterations + 2})
                message = res.message if isinstance(res.message, str) else res.message.decode()
            except Stop as e:
                message = str(e)
                stopped = None if isinstance(e, Budget) else message
            if best is None:
                raise RuntimeError("refit: " + message)
            first = log[0]
            after_held = held_figures(best[1]) if held else None
        except folder_run.NonFiniteLogits:
            raise                                    # every rank has raised alike: nobody waits for a command
        except BaseException:
            command(CMD_STOP, theta0)
            raise
        command(CMD_STOP, theta0)
        write_checkpoint(state_dict, best[1], out)
        with open(os.path.join(root, LOG_CSV), "w") as f:
            csv.writer(f, delimiter="\t").writerows([LOG_HEADER] + log)
        summary = {"loss": loss, "table": np.asarray(T).tolist(), "class_weights_source": class_weights_source if loss not in ("ce", "lovasz") else None,
                   "l2": l2, "iterations": iterations, "evaluations": len(log), "optimizer_message": message,
                   "stopped": stopped, "images": best[4], "skipped": best[5],
                   "objective": {"before": float(first[1]), "after": best[0]},
                   "data_term": {"before": float(first[2]), "after": best[3]},
                   "before": None, "after": _figures(best[2]), "model_path": model_path, "out": out,
                   "normalization": {"mean": list(normalization[0]), "std": list(normalization[1]), "source": normalization_source}
                   if normalization is not None else None,
                   "precision": r.precision, "ranks": r.world}
        summary["before"] = _figures(first_conf[0])
        for name in first_means[0]:                  # lovasz_softmax, mixed_loss: the Lovasz losses only
            summary[name] = {"before": first_means[0][name], "after": best[6][name]}
        if held:
            summary["holdout"] = {"before": before_held, "after": after_held}
        with open(os.path.join(root, SUMMARY_JSON), "w") as f:
            json.dump(summary, f, indent=1)
    stats = dict(folder_run.finish(r), summary=summary, evaluations=passes[0])
    return stats


def format_summary(s: dict) -> str:
    lines = ["refit of classifier.4 (%s, l2 %g): %d evaluations on %d images, objective %.6g -> %.6g"
             % (s["loss"], s["l2"], s["evaluations"], s["images"], s["objective"]["before"], s["objective"]["after"])]
    for key in ("before", "after"):
        lines.append("  %-6s IoU %s   F1 %s" % (key, " ".join("%.2f" % v for v in s[key]["iou"]), " ".join("%.2f" % v for v in s[key]["f1"])))
    for name in ("lovasz_softmax", "mixed_loss"):        # the Lovasz losses only: the folder's means over its images
        if name in s:
            lines.append("  %s %.6g -> %.6g" % (name, s[name]["before"], s[name]["after"]))
    if s.get("holdout") and s["holdout"]["before"] and s["holdout"]["after"]:
        for key in ("before", "after"):
            h = s["holdout"][key]
            lines.append("  held out, %-6s objective %.6g  IoU %s   F1 %s" % (key, h["objective"], " ".join("%.2f" % v for v in h["iou"]),
                                                                            " ".join("%.2f" % v for v in h["f1"])))
    return "\n".join(lines)


def main(argv=None):
    import sys
    raw = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(prog="python -m neuralbarkcalculator_amd.refit", description=__doc__.split("\n\n")[0])
    ap.add_argument("root_path")
    ap.add_argument("--out", required=True, help="the checkpoint to write: the input state_dict with classifier.4 replaced")
    ap.add_argument("--model_path", default="./best_model.pt")
    ap.add_argument("--loss", choices=list(ALL_LOSSES), default="ce",
                    help="ce: the plain cross-entropy; class_ce: weighted by the target class; weighted_ce: the reference's "
                         "CustomWeightedCrossEntropy, weighted by max(target class, argmax class); lovasz: the reference's "
                         "LovaszSoftmax per image; mixed: its MixedLoss, weighted_ce / 4 + lovasz per image")
    ap.add_argument("--class_weights", type=float, nargs=3, metavar=("W0", "W1", "W2"), default=None)
    ap.add_argument("--class_weights_from", metavar="PATH", default=None, help="the pos_weight of a results/dataset_stats.json")
    ap.add_argument("--l2", type=float, default=0.0, help="L of the penalty L/2 |theta - theta0|^2 (default 0)")
    ap.add_argument("--iterations", type=int, default=50, help="L-BFGS-B iterations (at most 2 x iterations + 2 evaluations)")
    ap.add_argument("--subset", metavar="PATH", default=None, help="fit on the samples this file lists (wood_type/name per line)")
    ap.add_argument("--holdout", metavar="PATH", default=None, help="samples that are never fitted on, scored before and after")
    ap.add_argument("--precision", choices=["auto", "fp32", "f16x2"], default="auto")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--mean", type=float, nargs=3, metavar=("R", "G", "B"), default=None)
    ap.add_argument("--std", type=float, nargs=3, metavar=("R", "G", "B"), default=None)
    ap.add_argument("--stats", metavar="PATH", default=None)
    args = ap.parse_args(raw)
    from . import evaluate as ev
    kw = {}
    try:
        normalization = folder_run.resolve_normalization(args.mean, args.std, args.stats)
        if args.class_weights is not None and args.class_weights_from is not None:
            raise ValueError("--class_weights and --class_weights_from exclude each other")
        if (args.class_weights is not None or args.class_weights_from is not None) and args.loss in ("ce", "lovasz"):
            raise ValueError("--class_weights and --class_weights_from need --loss class_ce, weighted_ce or mixed")
        if args.class_weights is not None:
            kw = dict(class_weights=ev.check_class_weights(args.class_weights), class_weights_source="arguments")
        elif args.class_weights_from is not None:
            kw = dict(class_weights=ev.class_weights_from(args.class_weights_from), class_weights_source=args.class_weights_from)
        if args.loss != "lovasz":
            table_of(args.loss, kw.get("class_weights"))
        if not (np.isfinite(args.l2) and args.l2 >= 0) or args.iterations < 1:
            raise ValueError("--l2 must be finite and >= 0 and --iterations >= 1")
        for name in ("subset", "holdout"):
            if getattr(args, name) is not None:
                ev.apply_subset(ev.list_labelled(args.root_path), ev.read_subset(getattr(args, name)))
    except (OSError, ValueError) as e:
        ap.error(str(e))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(folder_run.launch_ranks(args.gpus, raw, module="neuralbarkcalculator_amd.refit"))
    idx = None if "WORLD_SIZE" in os.environ else 0
    kw.update({"image_loss" if args.loss in LOVASZ_LOSSES else "loss": args.loss})
    kw.update(l2=args.l2, iterations=args.iterations, subset=args.subset, holdout=args.holdout, batch=args.batch, streams=args.streams)
    if normalization is not None:
        kw.update(normalization=normalization, normalization_source=args.stats)
    stats = folder_run.run_precision("refit", lambda precision, **over: refit_folder(
        args.root_path, args.out, args.model_path, precision=precision, device_index=idx, **dict(kw, **over)), args.precision)
    if stats["rank"] == 0:
        print(format_summary(stats["summary"]))
        print("%d passes over the folder: %.2f s" % (stats["evaluations"], stats["total_s"]), flush=True)


if __name__ == "__main__":
    main()
