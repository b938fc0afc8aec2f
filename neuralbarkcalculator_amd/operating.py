"""The operating point of a checkpoint: which constants, added to the bark and the node logit before the argmax, give the
best labelling (host side of ``evaluate --operating_points`` and ``--logit_offsets``).

The shipped checkpoint was trained with class weights 0.40 / 2.03 / 93.2 (``metrics.REFERENCE_CLASS_WEIGHTS``), which push
the node class far from its prior; the standard correction for a class-weighted loss is a constant per class added to the
logits before the argmax (first guess ``-log(w_c / w_0)``: -1.6 and -5.5 for those weights).  The definition
(include/nbc.h, nbc_offset_sweep):

* the decision with offsets ``(b1, b2)`` is ``k = argmax3(x0, x1 (+) b1, x2 (+) b2)`` on the f32 full-resolution logits,
  ``(+)`` one float32 addition, ``argmax3`` the forward's own rule (the first maximum wins, a NaN counts as the maximum);
  class 0's logit is never touched, and the logits the library returns are never offset;
* over a grid ``bark_offsets[G1]`` x ``node_offsets[G2]`` (finite float32, strictly ascending, 1..33 values each) an image's
  table is ``conf[i][j][t][p]``: the pixels of target class t (``metrics.target_classes``) whose decision at
  ``(bark_offsets[i], node_offsets[j])`` is p.  Non-finite logits decide like any other: the nine cells of every point sum
  to ``H W``.

``FCNResNet50.offset_sweep`` counts the tables on the device (csrc/offset_sweep.hip); ``sweep_cpu`` is the numpy
restatement, equal integer for integer.  ``figures`` turns a table into the IoU and F1 of every grid point with the
functions of ``metrics`` that ``evaluation_summary.json`` uses, ``select`` reads the named points off the pooled table,
and the writers produce ``results/operating_points.csv``, ``results/operating_evaluation.csv`` and the summary's
``"operating_points"`` entry.  The sweep is of the *raw* argmax, before ``remove_small_zones``, and its points are fitted on
the folder they are read from.
"""
from __future__ import annotations

import csv
import math
import os
from typing import List, Sequence

import numpy as np

from . import metrics

MAX_GRID = 33                                      # NBC_SWEEP_MAX_GRID
DEFAULT_GRID = "-8:8:0.5"                          # 33 values, all exact in f32, 0 on the grid
TABLE_BYTES_DEFAULT = MAX_GRID * MAX_GRID * 9 * 8  # 78 408 bytes per image ride back at the default grid
POINTS_CSV, EVALUATION_CSV = "operating_points.csv", "operating_evaluation.csv"
POINT_NAMES = ["argmax", "best_miou", "best_f1", "best_node_f1", "area_unbiased"]
EVALUATION_POINTS = ["argmax", "best_miou", "area_unbiased"]     # the columns of operating_evaluation.csv
POINTS_COLUMNS = ["bark_offset", "node_offset"] + ["iou_" + c for c in metrics.CLASS_NAMES] + ["miou"] + \
                 ["f1_" + c for c in metrics.CLASS_NAMES] + ["f1_mean", "Output Bark %", "Output Node %", "Target Bark %", "Target Node %"]
NOTE = ("the sweep is of the raw argmax (before remove_small_zones) and ignores --logit_offsets; the named points are fitted "
        "on this folder")


def parse_grid(text: str) -> np.ndarray:
    """``"LO:HI:STEP"`` -> the float32 values ``LO + k STEP`` for ``k = 0 .. floor((HI - LO) / STEP)`` (a relative 1e-9 of slack
    for a decimal STEP), computed in float64 and rounded once.  ``ValueError``: not three numbers, a non-finite one, STEP <= 0,
    HI < LO, more than 33 values, or values that are not strictly ascending once rounded to float32."""
    parts = str(text).split(":")
    if len(parts) != 3:
        raise ValueError("a grid is LO:HI:STEP, got %r" % (text,))
    try:
        lo, hi, step = (float(p) for p in parts)
    except ValueError:
        raise ValueError("a grid is LO:HI:STEP with three numbers, got %r" % (text,))
    if not all(math.isfinite(v) for v in (lo, hi, step)):
        raise ValueError("a grid's LO, HI and STEP must be finite, got %r" % (text,))
    if step <= 0:
        raise ValueError("a grid's STEP must be positive, got %r" % (text,))
    if hi < lo:
        raise ValueError("a grid's HI must not lie below LO, got %r" % (text,))
    count = int(math.floor((hi - lo) / step * (1 + 1e-9) + 1e-9)) + 1
    if count > MAX_GRID:
        raise ValueError("a grid holds at most %d values, %r has %d" % (MAX_GRID, text, count))
    return check_offsets(lo + step * np.arange(count, dtype=np.float64))


def check_offsets(values) -> np.ndarray:
    """The list as contiguous float32 ``[G]``; ``ValueError`` unless 1 <= G <= 33, every value is finite and they ascend
    strictly (as float32)."""
    with np.errstate(over="ignore"):
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1).astype(np.float32))
    if not 1 <= v.size <= MAX_GRID:
        raise ValueError("an offset list holds 1..%d values, got %d" % (MAX_GRID, v.size))
    if not np.all(np.isfinite(v)):
        raise ValueError("offsets must be finite")
    if np.any(np.diff(v) <= 0):
        raise ValueError("offsets must be strictly ascending")
    return v


def decide_cpu(logits, bark: float, node: float) -> np.ndarray:
    """The decision ``argmax3(x0, x1 (+) bark, x2 (+) node)`` of every pixel: ``logits`` float32 ``[...,3,H,W]`` -> uint8
    ``[...,H,W]``.  float32 additions; the first maximum wins, a NaN counts as the maximum (reduce.hpp's argmax3)."""
    x = np.asarray(logits, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = x[..., 0, :, :]
        b = x[..., 1, :, :] + np.float32(bark)
        c = x[..., 2, :, :] + np.float32(node)
        one = (b > a) | (np.isnan(b) & ~np.isnan(a))
        bv = np.where(one, b, a)
        two = (c > bv) | (np.isnan(c) & ~np.isnan(bv))
    return np.where(two, 2, np.where(one, 1, 0)).astype(np.uint8)


def sweep_cpu(logits, grey, bark_offsets, node_offsets) -> np.ndarray:
    """The numpy restatement of nbc_offset_sweep: ``logits`` float32 ``[3,H,W]`` or ``[N,3,H,W]``, ``grey`` the uint8 mask of
    the same pixels; returns int64 ``[G1,G2,3,3]`` (or ``[N,G1,G2,3,3]``): every grid point's own decision
    (``decide_cpu``) counted against the target classes."""
    x = np.asarray(logits, dtype=np.float32)
    g = np.asarray(grey)
    if x.ndim == 3:
        return sweep_cpu(x[None], g[None], bark_offsets, node_offsets)[0]
    b1, b2 = check_offsets(bark_offsets), check_offsets(node_offsets)
    if x.ndim != 4 or x.shape[1] != 3 or g.shape != (x.shape[0],) + x.shape[2:]:
        raise ValueError("logits must be [N,3,H,W] and grey [N,H,W]")
    out = np.zeros((x.shape[0], b1.size, b2.size, 3, 3), dtype=np.int64)
    for n in range(x.shape[0]):
        t = metrics.target_classes(g[n])
        for i, v1 in enumerate(b1):
            for j, v2 in enumerate(b2):
                out[n, i, j] = metrics.confusion_numpy(decide_cpu(x[n], v1, v2), t)
    return out


def figures(table) -> dict:
    """Per grid point of an int ``[G1,G2,3,3]`` table: ``iou`` and ``f1`` float64 ``[G1,G2,3]`` in percent (``metrics.iou`` and
    ``metrics.f1`` of the point's confusion, the functions under the pooled figures of ``evaluation_summary.json``), their
    means ``miou`` and ``f1_mean`` ``[G1,G2]``, and the output's and the target's Bark and Node as pixel counts ``out_bark``,
    ``out_node``, ``tgt_bark``, ``tgt_node`` (int64 ``[G1,G2]``, with ``pixels``) and as float64 percentages (``*_percent``)."""
    t = np.asarray(table).astype(np.int64)
    if t.ndim != 4 or t.shape[2:] != (3, 3):
        raise ValueError("a table is [G1,G2,3,3]")
    g1, g2 = t.shape[:2]
    iou, f1 = np.zeros((g1, g2, 3)), np.zeros((g1, g2, 3))
    for i in range(g1):
        for j in range(g2):
            iou[i, j], f1[i, j] = metrics.iou(t[i, j]), metrics.f1(t[i, j])
    pred, true = t.sum(axis=2), t.sum(axis=3)
    out = {"iou": iou, "f1": f1, "miou": iou.mean(axis=2), "f1_mean": f1.mean(axis=2),
           "out_bark": pred[..., 1], "out_node": pred[..., 2], "tgt_bark": true[..., 1], "tgt_node": true[..., 2],
           "pixels": t.sum(axis=(2, 3))}
    with np.errstate(divide="ignore", invalid="ignore"):
        for key in ("out_bark", "out_node", "tgt_bark", "tgt_node"):
            out[key + "_percent"] = 100.0 * out[key] / out["pixels"]
    return out


def _pick(score: np.ndarray, b1: np.ndarray, b2: np.ndarray, largest: bool):
    """The (i, j) of the best score; ties to the smallest |b1| + |b2|, then the smallest i, then the smallest j."""
    best = score.max() if largest else score.min()
    cands = [(abs(float(b1[i])) + abs(float(b2[j])), int(i), int(j)) for i, j in zip(*np.nonzero(score == best))]
    _, i, j = min(cands)
    return i, j


def select(table, bark_offsets, node_offsets) -> dict:
    """The named points of a (pooled) table: ``{name: {"i", "j", "bark_offset", "node_offset", "on_edge"}}`` for ``argmax``
    (the (0, 0) point; absent when it is not on the grid), ``best_miou``, ``best_f1`` (mean F1), ``best_node_f1`` and
    ``area_unbiased`` (the point minimising ``|out_bark - tgt_bark| + |out_node - tgt_node|`` in pixels).  Ties go to the
    smallest ``|b1| + |b2|``, then the smallest i, then the smallest j.  ``on_edge``: the point lies on the border of the grid
    along an axis that has more than one value -- the grid should be widened."""
    b1, b2 = check_offsets(bark_offsets), check_offsets(node_offsets)
    f = figures(table)
    if f["miou"].shape != (b1.size, b2.size):
        raise ValueError("the table is %s, the grids hold %d x %d values" % (f["miou"].shape, b1.size, b2.size))
    area = np.abs(f["out_bark"] - f["tgt_bark"]) + np.abs(f["out_node"] - f["tgt_node"])
    picks = {}
    zi, zj = np.nonzero(b1 == 0)[0], np.nonzero(b2 == 0)[0]
    if zi.size and zj.size:
        picks["argmax"] = (int(zi[0]), int(zj[0]))
    picks["best_miou"] = _pick(f["miou"], b1, b2, True)
    picks["best_f1"] = _pick(f["f1_mean"], b1, b2, True)
    picks["best_node_f1"] = _pick(f["f1"][..., 2], b1, b2, True)
    picks["area_unbiased"] = _pick(area, b1, b2, False)
    out = {}
    for name in POINT_NAMES:
        if name in picks:
            i, j = picks[name]
            edge = (b1.size > 1 and i in (0, b1.size - 1)) or (b2.size > 1 and j in (0, b2.size - 1))
            out[name] = {"i": i, "j": j, "bark_offset": float(b1[i]), "node_offset": float(b2[j]), "on_edge": bool(edge)}
    return out


def _offset_text(v: float) -> str:
    return repr(float(v))


def point_row(conf, bark: float, node: float) -> List[str]:
    """One row of ``operating_points.csv`` (``POINTS_COLUMNS``) from a point's 3 x 3 table: the figures to six decimals, the
    percentages in ``final_stats.csv``'s format (``metrics.percent``)."""
    conf = np.asarray(conf).astype(np.int64).reshape(3, 3)
    ious, f1s = metrics.iou(conf), metrics.f1(conf)
    pixels = int(conf.sum())
    pred, true = conf.sum(axis=0), conf.sum(axis=1)
    return [_offset_text(bark), _offset_text(node)] + ["%.6f" % v for v in ious] + ["%.6f" % ious.mean()] + \
           ["%.6f" % v for v in f1s] + ["%.6f" % f1s.mean()] + \
           [metrics.percent(int(pred[c]), pixels) for c in (1, 2)] + [metrics.percent(int(true[c]), pixels) for c in (1, 2)]


def write_points_csv(path: str, pooled, bark_offsets, node_offsets) -> None:
    """``operating_points.csv`` (tab separated, like ``evaluation_stats.csv``): a row per grid point of the pooled table, i
    outer, j inner."""
    b1, b2 = check_offsets(bark_offsets), check_offsets(node_offsets)
    pooled = np.asarray(pooled).astype(np.int64).reshape(b1.size, b2.size, 3, 3)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t")
        w.writerow(POINTS_COLUMNS)
        for i in range(b1.size):
            for j in range(b2.size):
                w.writerow(point_row(pooled[i, j], b1[i], b2[j]))


def evaluation_columns(points: dict) -> List[str]:
    cols = ["Name", "Type"]
    for name in EVALUATION_POINTS:
        if name in points:
            cols += ["%s %s" % (name, c) for c in ("miou", "iou_node", "Output Bark %", "Output Node %")]
    return cols + ["Target Bark %", "Target Node %"]


def write_evaluation_csv(path: str, images: Sequence[tuple], points: dict) -> None:
    """``operating_evaluation.csv`` (tab separated): a row per image of ``images`` = ``(name, wood, table [G1,G2,3,3])`` with its
    miou, iou_node, Output Bark % and Output Node % at the folder's ``argmax``, ``best_miou`` and ``area_unbiased`` points
    (``points`` = ``select`` of the pooled table), beside its target percentages."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t")
        w.writerow(evaluation_columns(points))
        for name, wood, table in images:
            table = np.asarray(table).astype(np.int64)
            row = [name, wood]
            conf = None
            for pt in EVALUATION_POINTS:
                if pt in points:
                    conf = table[points[pt]["i"], points[pt]["j"]]
                    ious, pixels, pred = metrics.iou(conf), int(conf.sum()), conf.sum(axis=0)
                    row += ["%.6f" % ious.mean(), "%.6f" % ious[2], metrics.percent(int(pred[1]), pixels), metrics.percent(int(pred[2]), pixels)]
            true, pixels = conf.sum(axis=1), int(conf.sum())
            w.writerow(row + [metrics.percent(int(true[c]), pixels) for c in (1, 2)])


def summary_entry(pooled, bark_offsets, node_offsets, logit_offsets=None) -> dict:
    """The ``"operating_points"`` entry of ``evaluation_summary.json``: both grids, every named point with its offsets, pooled
    3 x 3 table, figures, ``on_edge`` and a ready ``"--logit_offsets B N"`` string, and the note on what the sweep is of.
    ``logit_offsets``: the pair the run itself decided with (recorded; the sweep does not depend on it)."""
    b1, b2 = check_offsets(bark_offsets), check_offsets(node_offsets)
    pooled = np.asarray(pooled).astype(np.int64).reshape(b1.size, b2.size, 3, 3)
    points = select(pooled, b1, b2)
    entry = {"bark_offsets": [float(v) for v in b1], "node_offsets": [float(v) for v in b2], "points": {}, "note": NOTE,
             "run_logit_offsets": [float(v) for v in (logit_offsets or (0.0, 0.0))]}
    for name, p in points.items():
        conf = pooled[p["i"], p["j"]]
        ious, f1s = metrics.iou(conf), metrics.f1(conf)
        pixels, pred, true = int(conf.sum()), conf.sum(axis=0), conf.sum(axis=1)
        fig = {"miou": float(ious.mean()), "f1_mean": float(f1s.mean())}
        for c, cname in enumerate(metrics.CLASS_NAMES):
            fig["iou_" + cname], fig["f1_" + cname] = float(ious[c]), float(f1s[c])
        for key, cnt in (("Output Bark %", pred[1]), ("Output Node %", pred[2]), ("Target Bark %", true[1]), ("Target Node %", true[2])):
            fig[key] = metrics.percent(int(cnt), pixels) if pixels else None
        entry["points"][name] = dict(p, confusion=conf.tolist(), figures=fig,
                                     arguments="--logit_offsets %s %s" % (_offset_text(p["bark_offset"]), _offset_text(p["node_offset"])))
    return entry


def write_report(results_dir: str, images: Sequence[tuple], bark_offsets, node_offsets, logit_offsets=None) -> dict:
    """Both files under ``results_dir`` from the evaluated images' tables (``images`` as ``write_evaluation_csv`` takes them);
    returns ``summary_entry`` of their sum."""
    b1, b2 = check_offsets(bark_offsets), check_offsets(node_offsets)
    pooled = np.zeros((b1.size, b2.size, 3, 3), dtype=np.int64)
    for _, _, table in images:
        pooled += np.asarray(table).astype(np.int64)
    entry = summary_entry(pooled, b1, b2, logit_offsets)
    write_points_csv(os.path.join(results_dir, POINTS_CSV), pooled, b1, b2)
    write_evaluation_csv(os.path.join(results_dir, EVALUATION_CSV), images, entry["points"])
    return entry


def check_arguments(operating_points: bool, bark_offsets=None, node_offsets=None):
    """``ValueError`` for what ``--operating_points`` and its grids refuse before any device is touched: a grid without the
    flag, a grid ``parse_grid`` refuses.  Returns ``(bark_offsets, node_offsets)`` as float32 arrays, or None when off.  A grid
    is a ``"LO:HI:STEP"`` string or a list of values; the default for both is ``-8:8:0.5``."""
    if not operating_points:
        given = [n for n, v in (("--bark_offsets", bark_offsets), ("--node_offsets", node_offsets)) if v is not None]
        if given:
            raise ValueError("%s needs --operating_points" % ", ".join(given))
        return None
    grid = lambda v: parse_grid(DEFAULT_GRID if v is None else v) if v is None or isinstance(v, str) else check_offsets(v)
    return grid(bark_offsets), grid(node_offsets)
