"""Contour distances of a label map against its labelled mask: the host restatement of ``nbc_contour_distances``
(include/nbc.h, csrc/contours.hip), the figures ``evaluate --contours`` derives from the rows and the report it writes.

Class maps: the output's class is its label, 1 (Bark) or 2 (Node), any other value is no class; the target's is
``metrics.target_classes`` of the grey dual.  The contour of class c is the inner 4-contour: the pixels of class c with at
least one 4-neighbour *inside the image* that is not of class c -- ``m & ~binary_erosion(m, cross, border_value=1)``.  The
frame is no contour side (``zones.py``'s perimeter counts it; here it would add a zero distance on every frame pixel, since
the frame cuts the log in both maps alike).  Four sets per image, ``s = 2 (c - 1) + dir``: dir 0 goes from the output's
contour to the target's, dir 1 back.  Per set a row of ``HEAD + bins`` integers, ``n, m, sum_d2, max_d2, hist[bins]``, where
d2 is the squared Euclidean distance from a source contour pixel to the nearest destination contour pixel and ``hist[k]``
counts the source pixels with ``ceil(sqrt(d2)) == k`` (the last bin: everything above ``(bins - 2)**2``); beside the rows
``sum_d``, the float64 sum of ``sqrt(d2)``.  With ``n == 0`` or ``m == 0`` everything but n and m is 0.

``contours_cpu`` is built on scipy's erosion and exact Euclidean distance transform (by indices, so that no float enters
the integers); the device pass must equal its rows integer for integer.  The reference has no such code: nothing here restates
it but the 3.6 mm of a pixel side (models.py:210)."""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np

from .metrics import target_classes
from .zones import CLASS_NAMES, MM_PER_PIXEL

SETS, HEAD = 4, 4                                    # NBC_CONTOUR_SETS, NBC_CONTOUR_HEAD: n, m, sum_d2, max_d2
MAX_SIDE = 4096                                      # NBC_CONTOUR_MAX_SIDE
MAX_BINS = 5793                                      # ceil(hypot(4095, 4095)) + 1
DEFAULT_TOLERANCE = 2                                # pixels: 7.2 mm
SET_NAMES = ("Bark output to target", "Bark target to output", "Node output to target", "Node target to output")
# what travels between the ranks per image: the four heads, the four sum_d (bit-cast), the four within-tolerance counts and
# the four HD95 bins
WIRE_WIDTH = SETS * HEAD + 3 * SETS
CONTOUR_COLUMNS = ["Name", "Type"] + [
    "%s %s" % (name, col) for name in ("Bark", "Node")
    for col in ("output contour pixels", "target contour pixels", "contour precision", "contour recall", "contour F1",
                "mean contour distance (mm)", "HD95 (mm)", "HD (mm)")]


def default_bins(h: int, w: int) -> int:
    """The smallest ``bins`` whose last bin is no overflow bin on an ``h`` x ``w`` map: ``ceil(hypot(h - 1, w - 1)) + 1``,
    on the integers (1448 at 1024 x 1024), and at least the 2 the entry point asks for."""
    d2 = (int(h) - 1) ** 2 + (int(w) - 1) ** 2
    return max(2, ceil_sqrt(d2) + 1)


def ceil_sqrt(d2: int) -> int:
    """``ceil(sqrt(d2))`` of an integer >= 0, exactly: 0 for 0, ``isqrt(d2 - 1) + 1`` otherwise."""
    return 0 if d2 == 0 else math.isqrt(int(d2) - 1) + 1


def contour(mask: np.ndarray) -> np.ndarray:
    """The inner 4-contour of a boolean map: its pixels with a 4-neighbour inside the image that is not set."""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    return mask & ~ndimage.binary_erosion(mask, structure=ndimage.generate_binary_structure(2, 1), border_value=1)


def squared_distances(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """int64 d2 of every pixel of the boolean map ``src`` (raster order) to the nearest pixel of ``dst``, which is not empty:
    scipy's exact Euclidean distance transform gives the nearest pixel's indices, the squares are integer arithmetic."""
    from scipy import ndimage
    idx = ndimage.distance_transform_edt(~dst, return_distances=False, return_indices=True)
    ys, xs = np.nonzero(src)
    return (idx[0][ys, xs].astype(np.int64) - ys) ** 2 + (idx[1][ys, xs].astype(np.int64) - xs) ** 2


def contours_cpu(labels, target_grey, bins: int = None):
    """``(rows int64 [N, 4, HEAD + bins], sum_d float64 [N, 4])`` of ``labels`` and ``target_grey`` (integers of the same shape,
    ``[H,W]`` or ``[N,H,W]``; the grey dual as it is decoded): what ``nbc_contour_distances`` leaves.  ``bins``: 2..MAX_BINS,
    default ``default_bins(H, W)``.  ``sum_d`` is ``math.fsum`` of ``math.sqrt(d2)``: the correctly rounded sum of correctly
    rounded roots."""
    labels, grey = np.asarray(labels), np.asarray(target_grey)
    if labels.shape != grey.shape:
        raise ValueError("labels and target_grey must have the same shape")
    if labels.ndim == 2:
        labels, grey = labels[None], grey[None]
    if labels.ndim != 3 or not (1 <= labels.shape[1] <= MAX_SIDE and 1 <= labels.shape[2] <= MAX_SIDE):
        raise ValueError("labels must be [H,W] or [N,H,W] with H, W in 1..%d" % MAX_SIDE)
    bins = default_bins(*labels.shape[1:]) if bins is None else int(bins)
    if not 2 <= bins <= MAX_BINS:
        raise ValueError("bins must lie in 2..%d" % MAX_BINS)
    rows = np.zeros((len(labels), SETS, HEAD + bins), dtype=np.int64)
    sum_d = np.zeros((len(labels), SETS), dtype=np.float64)
    for i, (lab, g) in enumerate(zip(labels, grey)):
        tgt = target_classes(g.astype(np.uint8))
        for c in (1, 2):
            kinds = (contour(lab == c), contour(tgt == c))            # the output's contour, the target's
            for direction in (0, 1):
                src, dst = kinds[direction], kinds[1 - direction]
                row = rows[i, 2 * (c - 1) + direction]
                row[0], row[1] = int(src.sum()), int(dst.sum())
                if row[0] == 0 or row[1] == 0:
                    continue
                d2 = squared_distances(src, dst)
                row[2], row[3] = int(d2.sum()), int(d2.max())
                values, counts = np.unique(d2, return_counts=True)
                k = np.array([ceil_sqrt(v) for v in values.tolist()], dtype=np.int64)   # exact, per distinct value
                np.add.at(row[HEAD:], np.minimum(k, bins - 1), counts)
                sum_d[i, 2 * (c - 1) + direction] = math.fsum(math.sqrt(v) for v in d2.tolist())
    return rows, sum_d


def check_tolerance(tolerance) -> int:
    """The tolerance in pixels as an integer >= 0; ValueError otherwise."""
    try:
        ok = float(tolerance) == int(tolerance) and int(tolerance) >= 0
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("--contour_tolerance must be an integer >= 0, got %r" % (tolerance,))
    return int(tolerance)


def _hd95_bins(hist: np.ndarray, n: np.ndarray) -> np.ndarray:
    """Along the last axis of ``hist``, the smallest k with ``20 * (hist[0] + ... + hist[k]) >= 19 * n``: the distance, in
    whole pixels rounded up, that 95 % of the source pixels stay within."""
    return np.argmax(20 * np.cumsum(hist, axis=-1) >= 19 * np.asarray(n)[..., None], axis=-1)


def wire_rows(rows, sum_d, tolerance: int = DEFAULT_TOLERANCE) -> np.ndarray:
    """int64 ``[N, WIRE_WIDTH]`` from ``rows [N, 4, HEAD + bins]`` and ``sum_d [N, 4]``: per image the four heads, the four
    ``sum_d`` bit-cast to int64, the four counts of source pixels within ``tolerance`` pixels (``hist[0..tolerance]``) and the
    four HD95 bins (0 for a set without distances) -- everything ``figures_of_wire`` needs, without the histograms."""
    tolerance = check_tolerance(tolerance)
    rows = np.asarray(rows, dtype=np.int64)
    rows = rows.reshape((-1,) + rows.shape[-2:])
    sum_d = np.ascontiguousarray(np.asarray(sum_d, dtype=np.float64).reshape(-1, SETS))
    if rows.shape[1] != SETS or rows.shape[2] < HEAD + 2 or len(sum_d) != len(rows):
        raise ValueError("rows must be [N, 4, HEAD + bins] with bins >= 2 and sum_d [N, 4]")
    out = np.zeros((len(rows), WIRE_WIDTH), dtype=np.int64)
    out[:, : SETS * HEAD] = rows[:, :, :HEAD].reshape(len(rows), -1)
    out[:, SETS * HEAD: SETS * HEAD + SETS] = sum_d.view(np.int64)
    out[:, SETS * HEAD + SETS: SETS * HEAD + 2 * SETS] = rows[:, :, HEAD: HEAD + tolerance + 1].sum(axis=2)
    both = (rows[:, :, 0] > 0) & (rows[:, :, 1] > 0)
    out[:, SETS * HEAD + 2 * SETS:] = np.where(both, _hd95_bins(rows[:, :, HEAD:], rows[:, :, 0]), 0)
    return out


def _ratio(a, b):
    return a / b if b else None


def _f1(p, r):
    return None if p is None or r is None else (2 * p * r / (p + r) if p + r else 0.0)


def figures_of_wire(wire) -> dict:
    """The contour figures of one image from its ``wire_rows`` row, per class name (``"Bark"``, ``"Node"``):
    ``output_pixels`` / ``target_pixels`` (contour pixels of each map); ``precision`` (the share of the output's contour
    within the tolerance of the target's), ``recall`` (the same the other way) and ``f1``; ``mean_distance_mm`` (the mean
    symmetric contour distance, ``(sum_d0 + sum_d1) / (n0 + n1)`` x 3.6), ``hd95_mm`` (the larger of the two directions'
    95th-percentile distances, in whole pixels rounded up, x 3.6) and ``hd_mm`` (the Hausdorff distance,
    ``sqrt(max(max_d2))`` x 3.6).  A class with no contour in either map has None everywhere; with a contour in one map
    only (``one_sided``) precision, recall and F1 are 0.0 and the distances None.  The raw ``within_output``,
    ``within_target`` and ``sum_d`` (both directions) are kept for the pooled figures."""
    wire = np.ascontiguousarray(np.asarray(wire, dtype=np.int64).reshape(WIRE_WIDTH))
    head = wire[: SETS * HEAD].reshape(SETS, HEAD)
    sums = wire[SETS * HEAD: SETS * HEAD + SETS].view(np.float64)
    within, hd95 = wire[SETS * HEAD + SETS: SETS * HEAD + 2 * SETS], wire[SETS * HEAD + 2 * SETS:]
    fig = {}
    for c in (1, 2):
        a, b = 2 * (c - 1), 2 * (c - 1) + 1
        n0, n1 = int(head[a, 0]), int(head[b, 0])
        both, one_sided = n0 > 0 and n1 > 0, (n0 > 0) != (n1 > 0)
        f = {"output_pixels": n0, "target_pixels": n1, "one_sided": one_sided,
             "within_output": int(within[a]) if both else 0, "within_target": int(within[b]) if both else 0,
             "sum_d": (float(sums[a]), float(sums[b])) if both else (0.0, 0.0),
             "precision": None, "recall": None, "f1": None, "mean_distance_mm": None, "hd95_mm": None, "hd_mm": None}
        if one_sided:
            f.update(precision=0.0, recall=0.0, f1=0.0)
        elif both:
            p, r = within[a] / n0, within[b] / n1
            f.update(precision=float(p), recall=float(r), f1=_f1(float(p), float(r)),
                     mean_distance_mm=(float(sums[a]) + float(sums[b])) / (n0 + n1) * MM_PER_PIXEL,
                     hd95_mm=max(int(hd95[a]), int(hd95[b])) * MM_PER_PIXEL,
                     hd_mm=math.sqrt(max(int(head[a, 3]), int(head[b, 3]))) * MM_PER_PIXEL)
        fig[CLASS_NAMES[c]] = f
    return fig


def contour_figures(rows, sum_d, tolerance: int = DEFAULT_TOLERANCE) -> dict:
    """``figures_of_wire`` of one image's ``rows [4, HEAD + bins]`` and ``sum_d [4]`` at ``tolerance`` pixels."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.ndim != 2:
        raise ValueError("rows must be one image's [4, HEAD + bins]")
    return figures_of_wire(wire_rows(rows[None], np.asarray(sum_d, dtype=np.float64).reshape(1, SETS), tolerance)[0])


def _six(v) -> str:
    return "" if v is None else "{:.6f}".format(float(v))


def _three(v) -> str:
    return "" if v is None else "{:.3f}".format(float(v))


def contour_rows(name: str, wood: str, figures: dict) -> List[List[str]]:
    """The row of ``contour_evaluation.csv`` (``CONTOUR_COLUMNS``) of one image from its figures, as a one-element list: per
    class the two pixel counts, precision, recall and F1 to 6 decimals and the three distances in mm to 3 decimals, empty
    where undefined.  HD95 is a whole number of pixels, rounded up, times 3.6 mm."""
    row = [name, wood]
    for c in (1, 2):
        f = figures[CLASS_NAMES[c]]
        row += [str(f["output_pixels"]), str(f["target_pixels"]), _six(f["precision"]), _six(f["recall"]), _six(f["f1"]),
                _three(f["mean_distance_mm"]), _three(f["hd95_mm"]), _three(f["hd_mm"])]
    return [row]


def pooled_histogram(rows, bins: int) -> np.ndarray:
    """int64 ``[4, bins]``: the histograms of ``rows [N, 4, HEAD + b]`` with ``b <= bins`` added up, padded with empty bins."""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.zeros((SETS, int(bins)), dtype=np.int64)
    out[:, : rows.shape[2] - HEAD] = rows[:, :, HEAD:].sum(axis=0)
    return out


def contour_summary(figures: Sequence[dict], tolerance: int, histogram) -> dict:
    """The ``"contours"`` entry of ``evaluation_summary.json`` from the images' figures in image order and the folder's pooled
    histogram ``[4, bins]``: the tolerance in pixels and mm; per class the pooled contour pixels of both maps, those within the
    tolerance, precision, recall and F1 from these totals (an image with the class's contour in one map only adds its pixels
    and nothing within), the pooled mean symmetric distance in mm over the images with the contour in both maps, and the
    number of ``one_sided`` images; the pooled histogram, from which any other tolerance can be read off (sets in the order
    ``SET_NAMES``)."""
    hist = np.asarray(histogram, dtype=np.int64).reshape(SETS, -1)
    doc = {"images": len(figures), "tolerance_pixels": int(tolerance), "tolerance_mm": int(tolerance) * MM_PER_PIXEL,
           "mm_per_pixel": MM_PER_PIXEL}
    for c in (1, 2):
        per = [f[CLASS_NAMES[c]] for f in figures]
        n0, n1 = sum(p["output_pixels"] for p in per), sum(p["target_pixels"] for p in per)
        w0, w1 = sum(p["within_output"] for p in per), sum(p["within_target"] for p in per)
        two = [p for p in per if p["output_pixels"] and p["target_pixels"]]
        total = math.fsum(v for p in two for v in p["sum_d"])        # exact: it does not depend on the ranks or the order
        pixels = sum(p["output_pixels"] + p["target_pixels"] for p in two)
        precision, recall = _ratio(w0, n0), _ratio(w1, n1)
        if (n0 > 0) != (n1 > 0):
            precision = recall = 0.0
        doc[CLASS_NAMES[c]] = {"output_pixels": n0, "target_pixels": n1, "within_output": w0, "within_target": w1,
                               "precision": precision, "recall": recall, "f1": _f1(precision, recall),
                               "mean_distance_mm": None if not pixels else total / pixels * MM_PER_PIXEL,
                               "distance_pixels": pixels, "one_sided": sum(1 for p in per if p["one_sided"])}
    doc["sets"] = list(SET_NAMES)
    doc["histogram"] = hist.tolist()
    return doc
