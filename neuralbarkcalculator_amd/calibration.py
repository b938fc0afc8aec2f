"""The softmax confidence of a forward, tallied: the host restatement of ``nbc_softmax_census`` (include/nbc.h,
csrc/softmax_census.hip), the figures ``evaluate --calibration`` and ``predict --confidence`` derive from its rows, and the
reports they write.

The definition is integer from the quantisation on.  A pixel whose three float32 logits are finite has, in float64,
``m = max``, ``e_c = exp(x_c - m)``, ``s = (e_0 + e_1) + e_2``, ``p_c = e_c / s`` and ``q_c = min(65535, floor(p_c * 65536))``;
``k`` is the argmax of the logits (the first maximum wins, as the forward's labels), ``t`` the target class
(``metrics.target_classes`` of the grey dual; 0 without a target), ``hit = (k == t)`` (1 without a target), and the
confidence byte is ``q_k >> 8``.  A pixel with a NaN or infinite logit counts in ``nonfinite`` alone, with byte 0.  The row of
an image (``WORDS`` unsigned 64-bit integers, the order of ``NBC_CENSUS_*``):

* ``H[t][c][b]``: the pixels of target class t with ``q_c >> 8 == b`` -- the histogram of every class probability by target
  class, from which the one-vs-rest curves are read (``curves``);
* ``R[hit][b]`` and ``RS[hit][b]``: the pixels with ``q_k >> 8 == b`` and the sum of their ``q_k`` -- the reliability counts
  and the exact confidence sums per bin;
* ``M[t][c]``: the sum of ``q_c`` over the pixels of target class t -- the soft confusion, in expected pixels x 65536;
* ``B[t]``: the sum of ``sum_c (q_c - 65536 [c == t])**2`` -- the Brier numerators;
* ``nonfinite``.

Rows add: the row of a folder is the sum of its images' rows, exactly, in any order.  Every figure below is host arithmetic
on these integers.  The soft Jaccard is the quantity the reference's ``JaccardLoss`` (utils.py:168-182) is named after: its
own ``dims`` come out as ``(0, 2)`` on the ``[B,H,W]`` targets its dataset produces, which leaves a ``[3, W]`` per-column ratio
(``jaccard_loss_as_written``); here the sums run over all pixels of an image, the dims the name means."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from .metrics import target_classes
from .zones import MM_PER_PIXEL

BINS, WORDS = 256, 3341                              # NBC_CENSUS_BINS, NBC_CENSUS_WORDS
OFF_H, OFF_R, OFF_RS, OFF_M, OFF_B, OFF_NONFINITE = 0, 2304, 2816, 3328, 3337, 3340   # NBC_CENSUS_*
ONE = 65536                                          # the scale of q
CLASSES = ("Nothing", "Bark", "Node")
DEFAULT_ECE_BINS = 16
DEFAULT_CONFIDENCE_THRESHOLD = 0.9
JACCARD_EPS = 1e-7                                   # utils.py:169

CALIBRATION_COLUMNS = ["Name", "Type", "ECE", "MCE", "Accuracy", "Mean confidence", "Brier score"] + \
    ["Soft Jaccard %s" % c for c in CLASSES] + ["JaccardLoss", "Expected Bark %", "Bark %", "Expected Node %", "Node %",
                                                "Non-finite pixels"]
CURVE_COLUMNS = ["Table", "Class", "Bin", "Threshold", "Precision", "Recall", "F1", "Pixels", "Correct", "Accuracy",
                 "Mean confidence"]
CONFIDENCE_COLUMNS = ["Name", "Type", "Mean confidence", "Below threshold %", "Below threshold mm2", "Expected Bark %", "Bark %",
                      "Expected Bark mm2", "Bark mm2", "Expected Node %", "Node %", "Expected Node mm2", "Node mm2",
                      "Non-finite pixels"]


# ---- the definition ------------------------------------------------------------------------------------------------------
def census_cpu(logits, target=None):
    """``(rows uint64 [N, WORDS], confidence uint8 [N,H,W], margin)`` of float32 logits ``[N,3,H,W]`` (or ``[3,H,W]``) and
    the grey duals ``[N,H,W]`` (or None): what ``nbc_softmax_census`` leaves, restated in numpy float64 from the definition in
    the module docstring.  ``margin`` is the smallest distance of any ``v = p_c * 65536`` below 65535 to a bin edge that a
    rounding error could carry it across: ``floor(v) + 1 - v``, and ``v - floor(v)`` where ``floor(v) >= 1`` (no probability is
    negative, so nothing crosses the edge at 0); ``inf`` when there is no such value.  Two evaluations of the softmax that
    differ by less than the margin on that scale quantise every pixel alike."""
    x = np.asarray(logits)
    if x.dtype != np.float32:
        raise ValueError("logits must be float32")
    if x.ndim == 3:
        x = x[None]
        target = None if target is None else np.asarray(target)[None]
    if x.ndim != 4 or x.shape[1] != 3 or x.size == 0:
        raise ValueError("logits must be [N,3,H,W] or [3,H,W] and not empty")
    n, _, h, w = x.shape
    if target is not None:
        target = np.asarray(target)
        if target.shape != (n, h, w) or target.dtype != np.uint8:
            raise ValueError("target must be uint8 [%d,%d,%d]" % (n, h, w))
    rows = np.zeros((n, WORDS), dtype=np.uint64)
    plane = np.zeros((n, h, w), dtype=np.uint8)
    margin = math.inf
    for i in range(n):
        xi = x[i].reshape(3, -1)
        finite = np.isfinite(xi).all(axis=0)
        row = np.zeros(WORDS, dtype=np.int64)        # every word of these shapes stays far below 2^63
        row[OFF_NONFINITE] = int((~finite).sum())
        xf = xi[:, finite].astype(np.float64)
        if xf.shape[1]:
            e = np.exp(xf - xf.max(axis=0))
            v = e / ((e[0] + e[1]) + e[2]) * 65536.0
            fl = np.floor(v)
            q = np.minimum(65535, fl).astype(np.int64)
            below = v < 65535.0
            if below.any():
                up = (fl + 1.0 - v)[below]
                down = (v - fl)[below & (fl >= 1.0)]
                margin = min(margin, float(up.min()), float(down.min()) if down.size else math.inf)
            xs = xi[:, finite]
            k = np.zeros(xs.shape[1], dtype=np.int64)                # the first maximum wins
            k[xs[1] > xs[0]] = 1
            k[xs[2] > np.maximum(xs[0], xs[1])] = 2
            if target is None:
                t = np.zeros_like(k)
                hit = np.ones_like(k)
            else:
                t = target_classes(target[i].reshape(-1)[finite]).astype(np.int64)
                hit = (k == t).astype(np.int64)
            cols = np.arange(len(k))
            qk = q[k, cols]
            for c in range(3):
                np.add.at(row, OFF_H + (t * 3 + c) * BINS + (q[c] >> 8), 1)
                np.add.at(row, OFF_M + t * 3 + c, q[c])
            np.add.at(row, OFF_R + hit * BINS + (qk >> 8), 1)
            np.add.at(row, OFF_RS + hit * BINS + (qk >> 8), qk)
            d = q - ONE * (np.arange(3)[:, None] == t[None])
            np.add.at(row, OFF_B + t, (d * d).sum(axis=0))
            flat = plane[i].reshape(-1)
            flat[finite] = (qk >> 8).astype(np.uint8)
        rows[i] = row.astype(np.uint64)
    return rows, plane, margin


def split(row):
    """The fields of one row as Python-int arrays (dtype object): ``(H [3,3,256], R [2,256], RS [2,256], M [3,3], B [3],
    nonfinite)``.  Python integers: sums and products of the words cannot overflow on the way to a ratio."""
    r = np.asarray(row).reshape(WORDS)
    r = np.array([int(v) for v in (r.view(np.uint64) if r.dtype == np.int64 else r)], dtype=object)
    return (r[OFF_H:OFF_R].reshape(3, 3, BINS), r[OFF_R:OFF_RS].reshape(2, BINS), r[OFF_RS:OFF_M].reshape(2, BINS),
            r[OFF_M:OFF_B].reshape(3, 3), r[OFF_B:OFF_NONFINITE], int(r[OFF_NONFINITE]))


def pool(rows) -> np.ndarray:
    """uint64 ``[WORDS]``: the rows of ``[N, WORDS]`` added up -- the row of all their pixels together."""
    rows = np.asarray(rows)
    rows = (rows.view(np.uint64) if rows.dtype == np.int64 else rows.astype(np.uint64)).reshape(-1, WORDS)
    return rows.sum(axis=0, dtype=np.uint64)


def check_ece_bins(ece_bins) -> int:
    """``ece_bins`` as an integer power of two in 1..256; ValueError otherwise."""
    try:
        ok = float(ece_bins) == int(ece_bins) and 1 <= int(ece_bins) <= BINS and (int(ece_bins) & (int(ece_bins) - 1)) == 0
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("--ece_bins must be a power of two in 1..%d, got %r" % (BINS, ece_bins))
    return int(ece_bins)


def check_confidence_threshold(threshold) -> float:
    """The threshold as a float in (0, 1]; ValueError otherwise."""
    try:
        v = float(threshold)
    except (TypeError, ValueError):
        v = math.nan
    if not 0.0 < v <= 1.0:
        raise ValueError("--confidence_threshold must lie in (0, 1], got %r" % (threshold,))
    return v


# ---- what travels between the ranks --------------------------------------------------------------------------------------
def wire_width(ece_bins: int = DEFAULT_ECE_BINS) -> int:
    """Words of a ``wire_rows`` row: R and RS merged to ``ece_bins`` bins, M, B, nonfinite and the target pixels per class."""
    return 4 * check_ece_bins(ece_bins) + 9 + 3 + 1 + 3


def wire_rows(rows, ece_bins: int = DEFAULT_ECE_BINS) -> np.ndarray:
    """int64 ``[N, wire_width(ece_bins)]`` (the uint64 words bit-cast) from census rows ``[N, WORDS]``: per image ``R`` and
    ``RS`` with 256 / ``ece_bins`` neighbouring bins merged, ``M``, ``B``, ``nonfinite`` and the finite pixels of each target
    class (``sum_b H[t][0][b]``) -- everything ``figures_of_wire`` needs, 640 bytes at 16 bins instead of the row's 26 KB."""
    nb = check_ece_bins(ece_bins)
    rows = np.asarray(rows)
    rows = (rows.view(np.uint64) if rows.dtype == np.int64 else rows.astype(np.uint64)).reshape(-1, WORDS)
    out = np.zeros((len(rows), wire_width(nb)), dtype=np.uint64)
    out[:, : 2 * nb] = rows[:, OFF_R:OFF_RS].reshape(len(rows), 2 * nb, BINS // nb).sum(axis=2, dtype=np.uint64)
    out[:, 2 * nb: 4 * nb] = rows[:, OFF_RS:OFF_M].reshape(len(rows), 2 * nb, BINS // nb).sum(axis=2, dtype=np.uint64)
    out[:, 4 * nb: 4 * nb + 13] = rows[:, OFF_M: OFF_NONFINITE + 1]
    out[:, 4 * nb + 13:] = rows[:, OFF_H:OFF_R].reshape(len(rows), 3, 3, BINS)[:, :, 0, :].sum(axis=2, dtype=np.uint64)
    return out.view(np.int64)


def _ratio(a, b):
    return a / b if b else None


def figures_of_wire(wire, ece_bins: int = DEFAULT_ECE_BINS) -> dict:
    """The figures of one image (or of a pooled folder) from its ``wire_rows`` row, exact ratios of Python integers:

    * ``pixels`` (finite ones) and ``nonfinite``; ``accuracy`` (hits / pixels) and ``mean_confidence`` (``sum RS / 65536`` /
      pixels);
    * ``ece`` = ``sum_b n_b |acc_b - conf_b| / pixels`` and ``mce`` = ``max_b |acc_b - conf_b|`` over the ``ece_bins`` bins that
      hold pixels, with ``acc_b`` the hits of the bin over its pixels and ``conf_b`` its mean confidence *from RS*, not its
      centre;
    * ``brier`` = ``sum B / 65536**2 / pixels``: the mean squared distance of the probability vector to the one-hot target;
    * per class c (``soft_jaccard``, ``soft_dice``, lists of three): ``I = M[c][c]``, ``S = sum_t M[t][c]`` (the expected pixels
      of c), ``G`` the target pixels of c, all in pixels: ``I / (S + G - I + 1e-7)`` and ``2 I / (S + G)`` (None for a class
      with neither); ``jaccard_loss`` = 1 - the mean of the three soft Jaccards, ``JaccardLoss`` (utils.py:168-182) with the
      sums over all pixels of the image;
    * ``expected_percent``: ``100 S / pixels`` per class.

    Everything that divides by the pixels is None for an image without a finite pixel.  Without a target every pixel is of
    class 0 and a hit: only the mean confidence, the expected percentages and the counts mean something."""
    nb = check_ece_bins(ece_bins)
    w = np.ascontiguousarray(np.asarray(wire, dtype=np.int64).reshape(wire_width(nb))).view(np.uint64)
    w = [int(v) for v in w]
    R = [w[:nb], w[nb: 2 * nb]]
    RS = [w[2 * nb: 3 * nb], w[3 * nb: 4 * nb]]
    M = [w[4 * nb + 3 * t: 4 * nb + 3 * t + 3] for t in range(3)]
    B = w[4 * nb + 9: 4 * nb + 12]
    nonfinite, G = w[4 * nb + 12], w[4 * nb + 13:]
    pixels, hits = sum(R[0]) + sum(R[1]), sum(R[1])
    fig = {"pixels": pixels, "nonfinite": nonfinite, "hits": hits, "confidence_sum": sum(RS[0]) + sum(RS[1]),
           "brier_sum": sum(B), "soft_confusion": M, "target_pixels": G, "ece_bins": nb,
           "accuracy": _ratio(hits, pixels), "mean_confidence": _ratio(sum(RS[0]) + sum(RS[1]), ONE * pixels),
           "brier": _ratio(sum(B), ONE * ONE * pixels), "ece": None, "mce": None}
    if pixels:
        gaps = [(R[0][b] + R[1][b], abs(R[1][b] / (R[0][b] + R[1][b]) - (RS[0][b] + RS[1][b]) / (ONE * (R[0][b] + R[1][b]))))
                for b in range(nb) if R[0][b] + R[1][b]]
        fig["ece"] = math.fsum(n * g for n, g in gaps) / pixels
        fig["mce"] = max(g for _, g in gaps)
    jac, dice = [], []
    for c in range(3):
        inter, soft = M[c][c] / ONE, sum(M[t][c] for t in range(3)) / ONE
        jac.append(None if not pixels else inter / (soft + G[c] - inter + JACCARD_EPS))
        dice.append(None if not pixels or soft + G[c] == 0 else 2 * inter / (soft + G[c]))
    fig["soft_jaccard"], fig["soft_dice"] = jac, dice
    fig["jaccard_loss"] = None if not pixels else 1 - math.fsum(jac) / 3
    fig["expected_percent"] = [None if not pixels else 100 * sum(M[t][c] for t in range(3)) / (ONE * pixels) for c in range(3)]
    return fig


def figures(row, ece_bins: int = DEFAULT_ECE_BINS) -> dict:
    """``figures_of_wire`` of one census row ``[WORDS]``."""
    return figures_of_wire(wire_rows(np.asarray(row).reshape(1, WORDS), ece_bins)[0], ece_bins)


def below_threshold(row, threshold: float = DEFAULT_CONFIDENCE_THRESHOLD) -> int:
    """The finite pixels of a row whose confidence byte lies below ``ceil(threshold * 256)``: the threshold moves up to the
    next edge of the 256 bins, so a pixel counted as confident has ``p_k >= threshold``."""
    edge = min(BINS, math.ceil(check_confidence_threshold(threshold) * BINS))
    R = split(row)[1]
    return int(sum(R[0][:edge]) + sum(R[1][:edge]))


# ---- the one-vs-rest curves ----------------------------------------------------------------------------------------------
def curves(H) -> dict:
    """Per class (``"Nothing"``, ``"Bark"``, ``"Node"``) the one-vs-rest curve of its probability against the target, from
    ``H [3,3,256]``: a pixel is positive when its target class is c, and at threshold j / 256 (j = 0..255) it is called c when
    ``q_c >> 8 >= j``.  ``precision``, ``recall`` and ``f1`` are lists over j (None where undefined: no pixel called, or no
    positive); ``best_f1`` and ``best_threshold`` the largest F1 and the first threshold that reaches it;
    ``average_precision`` the step-wise sum ``sum_j (recall_j - recall_{j+1}) precision_j`` (recall_256 = 0); ``auroc`` the
    trapezoid over the bins, which is the rank statistic with the convention that *ties inside a bin count as half*: a
    positive and a negative pixel of the same bin are ordered right with probability 1/2.  ``positives`` / ``negatives`` are
    the pixel counts; a class without one of them has no AP / AUROC (None)."""
    H = np.asarray(H).reshape(3, 3, BINS)
    out = {}
    for c, name in enumerate(CLASSES):
        pos = [int(v) for v in H[c, c]]
        neg = [sum(int(H[t, c, b]) for t in range(3) if t != c) for b in range(BINS)]
        P, N = sum(pos), sum(neg)
        tp = fp = 0
        TP, FP = [0] * BINS, [0] * BINS
        for j in range(BINS - 1, -1, -1):
            tp += pos[j]
            fp += neg[j]
            TP[j], FP[j] = tp, fp
        precision = [_ratio(TP[j], TP[j] + FP[j]) for j in range(BINS)]
        recall = [_ratio(TP[j], P) for j in range(BINS)]
        f1 = [_ratio(2 * TP[j], 2 * TP[j] + FP[j] + (P - TP[j])) if P else None for j in range(BINS)]
        best_j = None
        if P:
            best_j = max(range(BINS), key=lambda j: (f1[j], -j))
        ap = auroc = None
        if P:
            ap = math.fsum((TP[j] - (TP[j + 1] if j + 1 < BINS else 0)) * precision[j] for j in range(BINS) if TP[j] + FP[j]) / P
        if P and N:
            below, acc = 0, 0
            for b in range(BINS):                      # twice the wins, to stay on the integers
                acc += pos[b] * (2 * below + neg[b])
                below += neg[b]
            auroc = acc / (2 * P * N)
        out[name] = {"positives": P, "negatives": N, "precision": precision, "recall": recall, "f1": f1,
                     "best_threshold": None if best_j is None else best_j / BINS, "best_f1": None if best_j is None else f1[best_j],
                     "average_precision": ap, "auroc": auroc}
    return out


def jaccard_loss_as_written(logits, target_classes_bhw, eps: float = JACCARD_EPS) -> float:
    """``JaccardLoss()(predict, true)`` (utils.py:168-182) as its code runs on a ``[B,H,W]`` class target, in float64: its
    ``dims`` are ``(0,) + tuple(range(2, true.ndimension()))`` = ``(0, 2)``, so the sums run over the batch and the rows only and
    the mean is taken over a ``[3, W]`` table of per-column ratios."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(target_classes_bhw)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    hot = (np.arange(3)[None, :, None, None] == t[:, None]).astype(np.float64)
    dims = (0,) + tuple(range(2, t.ndim))
    inter = (p * hot).sum(axis=dims)
    union = (p + hot).sum(axis=dims) - inter
    return float(1 - (inter / (union + eps)).mean())


# ---- reports -------------------------------------------------------------------------------------------------------------
def _six(v) -> str:
    return "" if v is None else "{:.6f}".format(float(v))


def _percent(count, total) -> Optional[float]:
    return None if not total else 100 * count / total


def calibration_rows(name: str, wood: str, fig: dict, hard_counts) -> List[List[str]]:
    """The row of ``calibration_evaluation.csv`` (``CALIBRATION_COLUMNS``) of one image, as a one-element list, from its
    figures and ``hard_counts``, the pixels per class of its raw argmax labels (the column sums of the raw confusion): six
    decimals, empty where undefined."""
    hard = [int(v) for v in hard_counts]
    total = sum(hard)
    row = [name, wood, _six(fig["ece"]), _six(fig["mce"]), _six(fig["accuracy"]), _six(fig["mean_confidence"]), _six(fig["brier"])]
    row += [_six(v) for v in fig["soft_jaccard"]] + [_six(fig["jaccard_loss"])]
    for c in (1, 2):
        row += [_six(fig["expected_percent"][c]), _six(_percent(hard[c], total))]
    return [row + [str(fig["nonfinite"])]]


def confidence_rows(name: str, wood: str, row, hard_counts, threshold: float = DEFAULT_CONFIDENCE_THRESHOLD) -> List[List[str]]:
    """The row of ``confidence_stats.csv`` (``CONFIDENCE_COLUMNS``) of one image, as a one-element list, from its census row
    (no target) and ``hard_counts``, the pixels per class of the labels the run wrote: the mean confidence, the share and the
    area of the pixels below the threshold (``below_threshold``), and per class the expected share and area
    (``sum p_c``, in pixels of 3.6 mm x 3.6 mm) beside the hard ones."""
    return confidence_rows_of_wire(name, wood, figures(row), below_threshold(row, threshold), hard_counts)


def confidence_rows_of_wire(name: str, wood: str, fig: dict, low: int, hard_counts) -> List[List[str]]:
    """``confidence_rows`` from what travels between the ranks: the image's figures (``figures_of_wire``) and ``low``, its
    pixels below the threshold."""
    hard = [int(v) for v in hard_counts]
    total, px = sum(hard), MM_PER_PIXEL * MM_PER_PIXEL
    out = [name, wood, _six(fig["mean_confidence"]), _six(_percent(low, fig["pixels"])), "{:.2f}".format(low * px)]
    for c in (1, 2):
        soft = sum(fig["soft_confusion"][t][c] for t in range(3)) / ONE
        out += [_six(fig["expected_percent"][c]), _six(_percent(hard[c], total)), "{:.2f}".format(soft * px),
                "{:.2f}".format(hard[c] * px)]
    return [out + [str(fig["nonfinite"])]]


def curve_rows(row, ece_bins: int = BINS) -> List[List[str]]:
    """The data rows of ``calibration_curves.csv`` (``CURVE_COLUMNS``) from a pooled census row: a ``curve`` row per class and
    threshold (precision, recall, F1) and a ``reliability`` row per bin of the 256 (pixels, correct ones, accuracy and mean
    confidence of the bin)."""
    H, R, RS = split(row)[:3]
    cv = curves(H)
    out = []
    for name in CLASSES:
        c = cv[name]
        out += [["curve", name, str(j), "{:.6f}".format(j / BINS), _six(c["precision"][j]), _six(c["recall"][j]), _six(c["f1"][j]),
                 "", "", "", ""] for j in range(BINS)]
    for b in range(BINS):
        n = int(R[0][b] + R[1][b])
        out.append(["reliability", "", str(b), "{:.6f}".format(b / BINS), "", "", "", str(n), str(int(R[1][b])),
                    _six(_ratio(int(R[1][b]), n)), _six(_ratio(int(RS[0][b] + RS[1][b]), ONE * n))])
    return out


def _public(fig: dict) -> dict:
    return {k: fig[k] for k in ("pixels", "nonfinite", "accuracy", "mean_confidence", "ece", "mce", "brier", "soft_jaccard",
                                "soft_dice", "jaccard_loss", "expected_percent")}


def calibration_summary(pooled_row, images: int, ece_bins: int = DEFAULT_ECE_BINS, raw_confusion=None) -> dict:
    """The ``"calibration"`` entry of ``evaluation_summary.json`` from the folder's pooled census row: the pooled figures at
    ``ece_bins``; per class the average precision, the AUROC, the threshold of best F1 and the F1 there, beside
    ``f1_at_argmax``, the one-vs-rest F1 of the raw argmax labels (from ``raw_confusion [3,3]``, target x output; None without
    it); and the pooled ``H``, ``R`` and ``RS``, from which any other bin count or threshold can be read off."""
    H, R, RS = split(pooled_row)[:3]
    doc = {"images": int(images), "ece_bins": check_ece_bins(ece_bins), "pooled": _public(figures(pooled_row, ece_bins))}
    cv = curves(H)
    conf = None if raw_confusion is None else np.asarray(raw_confusion, dtype=np.int64).reshape(3, 3)
    for c, name in enumerate(CLASSES):
        hard = None
        if conf is not None:
            tp, fp, fn = int(conf[c, c]), int(conf[:, c].sum() - conf[c, c]), int(conf[c].sum() - conf[c, c])
            hard = _ratio(2 * tp, 2 * tp + fp + fn)
        doc[name] = {"positives": cv[name]["positives"], "negatives": cv[name]["negatives"],
                     "average_precision": cv[name]["average_precision"], "auroc": cv[name]["auroc"],
                     "best_f1_threshold": cv[name]["best_threshold"], "best_f1": cv[name]["best_f1"], "f1_at_argmax": hard}
    doc["H"] = [[[int(v) for v in H[t, c]] for c in range(3)] for t in range(3)]
    doc["R"] = [[int(v) for v in R[h]] for h in range(2)]
    doc["RS"] = [[int(v) for v in RS[h]] for h in range(2)]
    return doc


def confidence_summary(pooled_row, images: int, threshold: float, hard_counts: Sequence[int]) -> dict:
    """``confidence_summary.json`` of ``predict --confidence`` from the folder's pooled census row (no target): the mean
    confidence, the pixels below the threshold, the expected and hard shares of Bark and Node, and the pooled ``R`` / ``RS``."""
    fig = figures(pooled_row)
    R, RS = split(pooled_row)[1:3]
    hard = [int(v) for v in hard_counts]
    low = below_threshold(pooled_row, threshold)
    return {"images": int(images), "confidence_threshold": float(threshold), "pixels": fig["pixels"], "nonfinite": fig["nonfinite"],
            "mean_confidence": fig["mean_confidence"], "below_threshold_pixels": low,
            "below_threshold_percent": _percent(low, fig["pixels"]), "mm_per_pixel": MM_PER_PIXEL,
            "expected_percent": dict(zip(CLASSES, fig["expected_percent"])),
            "hard_percent": dict(zip(CLASSES, [_percent(v, sum(hard)) for v in hard])),
            "R": [int(v) for v in R[1]], "RS": [int(v) for v in RS[1]]}
