"""The zones of a label map: the host restatement of ``nbc_label_zones`` (include/nbc.h, csrc/zones.hip) and the report
``predict --zones`` writes from the rows.

A zone is an 8-connected component of one class c in {1, 2} (Bark, Node); pixels of any other value belong to no zone.  Its
row is ten integers, ``ZONE_FIELDS``: the first pixel in raster order (``y * W + x``), the class, the pixel count, the
inclusive bounding box, the coordinate sums over its pixels and the perimeter -- the number of pixel sides (4-neighbourhood)
whose neighbour has another label or lies outside the image.  The rows of an image are sorted by first pixel.

``zones_cpu`` is built on ``scipy.ndimage.label`` per class plus numpy reductions and does not depend on scipy's numbering;
the device pass must equal it integer for integer.  The reference has no such code: nothing here restates it but the
millimetres of models.py:210 (3.6 mm per pixel side) and the float32 area arithmetic of ``predict.stats_row``.

The second half is the same for ``nbc_match_zones`` (csrc/zone_match.hip) and ``evaluate --zones``: ``match_cpu`` restates the
pairing of output zones and target zones, ``match_figures`` applies the matching rule, and the formatters write
``zone_matches.csv``, ``zone_evaluation.csv`` and the summary's ``"zones"`` entry."""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np

ZONE_FIELDS = ("first_pixel", "class", "pixels", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "perimeter")
ZONE_ROW = len(ZONE_FIELDS)                          # NBC_ZONE_ROW of include/nbc.h
DEFAULT_CAP = 1024                                   # rows per image the device pass keeps (--zones_cap)
MM_PER_PIXEL = 3.6                                   # models.py:210: a pixel is 3.6 mm x 3.6 mm
MM2_PER_PIXEL = 3.6 * 3.6
CLASS_NAMES = {1: "Bark", 2: "Node"}
ZONE_COLUMNS = ["Name", "Type", "Zone", "Class", "Pixels", "Area (mm^2)", "Left", "Top", "Right", "Bottom", "Centroid x",
                "Centroid y", "Perimeter (mm)", "Diameter (mm)", "Touches edge"]
SUMMARY_COLUMNS = ["Name", "Type", "Bark zones", "Nodes", "Largest bark zone (mm^2)", "Largest node (mm^2)", "Mean node (mm^2)",
                   "Nodes touching edge"]


def _zones_of_map(labels: np.ndarray) -> np.ndarray:
    from scipy import ndimage
    h, w = labels.shape
    lab = np.asarray(labels).astype(np.int64)
    padded = np.full((h + 2, w + 2), -1, dtype=np.int64)          # outside the image: a label no pixel carries
    padded[1:-1, 1:-1] = lab
    sides = ((padded[:-2, 1:-1] != lab).astype(np.int64) + (padded[2:, 1:-1] != lab) + (padded[1:-1, :-2] != lab)
             + (padded[1:-1, 2:] != lab)).ravel()
    out = []
    for c in (1, 2):
        comp, k = ndimage.label(lab == c, structure=np.ones((3, 3), dtype=bool))
        if k == 0:
            continue
        at = np.flatnonzero(comp)                                 # raster order
        ids = comp.ravel()[at]
        order = np.argsort(ids, kind="stable")                    # by component, raster order inside each
        at, ids = at[order], ids[order]
        starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
        ends = np.r_[starts[1:], len(ids)]
        ys, xs = np.divmod(at, w)
        rows = np.empty((k, ZONE_ROW), dtype=np.int64)
        rows[:, 0] = at[starts]
        rows[:, 1] = c
        rows[:, 2] = ends - starts
        rows[:, 3] = np.minimum.reduceat(xs, starts)
        rows[:, 4] = ys[starts]
        rows[:, 5] = np.maximum.reduceat(xs, starts)
        rows[:, 6] = ys[ends - 1]
        rows[:, 7] = np.add.reduceat(xs, starts)
        rows[:, 8] = np.add.reduceat(ys, starts)
        rows[:, 9] = np.add.reduceat(sides[at], starts)
        out.append(rows)
    if not out:
        return np.zeros((0, ZONE_ROW), dtype=np.int64)
    rows = np.concatenate(out)
    return rows[np.argsort(rows[:, 0], kind="stable")]


def zones_cpu(labels) -> List[np.ndarray]:
    """The zone rows of every image of ``labels`` (integers, ``[H,W]`` or ``[N,H,W]``): a list of int64 ``[k, 10]`` arrays
    (``ZONE_FIELDS``), the zones of both classes merged and sorted by first pixel."""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[None]
    if labels.ndim != 3 or labels.shape[1] < 1 or labels.shape[2] < 1:
        raise ValueError("labels must be [H,W] or [N,H,W] with H, W >= 1")
    return [_zones_of_map(m) for m in labels]


def area_mm2(pixels: int) -> float:
    """``float32(pixels) * 12.96`` as ``predict.stats_row`` computes an area."""
    return float(np.float32(pixels) * np.float32(MM2_PER_PIXEL))


def _touching(rows: np.ndarray, h: int, w: int) -> np.ndarray:
    """Per row of an int64 ``[k, 10]`` array: does the zone's box reach an edge of the ``h x w`` image."""
    return (rows[:, 3] == 0) | (rows[:, 4] == 0) | (rows[:, 5] == w - 1) | (rows[:, 6] == h - 1)


def touches_edge(row: Sequence[int], h: int, w: int) -> bool:
    return bool(_touching(np.asarray(row, dtype=np.int64)[None], h, w)[0])


def zone_rows(name: str, wood: str, h: int, w: int, rows) -> List[List[str]]:
    """The rows of ``zones.csv`` (``ZONE_COLUMNS``) of one image from its zone rows, in their order."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    areas = (rows[:, 2].astype(np.float32) * np.float32(MM2_PER_PIXEL)).astype(np.float64).tolist()     # area_mm2 of every row
    edge = _touching(rows, h, w).tolist()
    out = []
    for k, ((_, c, px, x0, y0, x1, y1, sx, sy, per), area, e) in enumerate(zip(rows.tolist(), areas, edge)):
        out.append([name, wood, str(k + 1), CLASS_NAMES[c], str(px), "{:.5f}".format(area), str(x0), str(y0), str(x1), str(y1),
                    "{:.3f}".format(sx / px), "{:.3f}".format(sy / px), "{:.3f}".format(per * MM_PER_PIXEL),
                    "{:.3f}".format(2.0 * math.sqrt(area / math.pi)), str(int(e))])
    return out


def image_figures(h: int, w: int, rows) -> dict:
    """What ``summary_rows`` prints and the folder totals add up, of one image."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    bark, nodes = rows[rows[:, 1] == 1], rows[rows[:, 1] == 2]
    return {"bark_zones": len(bark), "nodes": len(nodes),
            "largest_bark_pixels": int(bark[:, 2].max()) if len(bark) else None,
            "largest_node_pixels": int(nodes[:, 2].max()) if len(nodes) else None,
            "node_pixels": int(nodes[:, 2].sum()),
            "nodes_touching_edge": int(_touching(nodes, h, w).sum())}


def summary_rows(name: str, wood: str, h: int, w: int, rows) -> List[List[str]]:
    """The row of ``zones_summary.csv`` (``SUMMARY_COLUMNS``) of one image, as a one-element list.  Areas as ``zone_rows``
    prints them; the mean node is the image's node area (``final_stats.csv``'s figure) over its nodes; a figure of a class
    without a zone stays empty."""
    f = image_figures(h, w, rows)

    def area(px):
        return "" if px is None else "{:.5f}".format(area_mm2(px))
    mean = "{:.5f}".format(area_mm2(f["node_pixels"]) / f["nodes"]) if f["nodes"] else ""
    return [[name, wood, str(f["bark_zones"]), str(f["nodes"]), area(f["largest_bark_pixels"]), area(f["largest_node_pixels"]), mean,
             str(f["nodes_touching_edge"])]]


def folder_summary(figures: Sequence[dict], cap: int, host_fallbacks: int) -> dict:
    """``zones_summary.json``: the folder totals and per-image means of ``image_figures``, the cap and the host fallbacks."""
    n = len(figures)
    tot = {k: sum(f[k] for f in figures) for k in ("bark_zones", "nodes", "nodes_touching_edge", "node_pixels")}
    return {"images": n, "cap": int(cap), "host_fallbacks": int(host_fallbacks),
            "totals": {k: tot[k] for k in ("bark_zones", "nodes", "nodes_touching_edge")},
            "means": {"bark_zones_per_image": tot["bark_zones"] / n if n else None, "nodes_per_image": tot["nodes"] / n if n else None,
                      "node_mm2": area_mm2(tot["node_pixels"]) / tot["nodes"] if tot["nodes"] else None}}


# ---- output zones against target zones: the host restatement of nbc_match_zones (csrc/zone_match.hip) and the report of
# ``evaluate --zones`` ------------------------------------------------------------------------------------------------------
# A pair row is three integers, ``PAIR_FIELDS``: the output zone's and the target zone's index (the row number in the map's
# zone rows, i.e. the position in first-pixel order) and the pixels that lie in both.  Only zones of the same class share
# pixels.  ``match_cpu`` builds a zone-index plane per map from ``scipy.ndimage.label`` and counts the joined key with
# ``numpy.unique``: nothing of the device's method (union-find codes, hash tables, a sort).  The reference has no such code.
from .metrics import target_classes  # noqa: E402,F401  (the grey -> class rule of the duals, shared with ``evaluate``)

PAIR_FIELDS = ("output_zone", "target_zone", "pixels")
PAIR_ROW = len(PAIR_FIELDS)                          # NBC_ZONE_PAIR_ROW of include/nbc.h
PAIRS_MAX_CAP = 4096                                 # NBC_ZONE_PAIRS_MAX_CAP: the sort kernel's LDS, 4096 x 12 bytes = 48 KiB
DEFAULT_PAIR_CAP = 2048                              # pair rows per image the device pass keeps (--zone_pairs_cap)
DEFAULT_MATCH_IOU = 0.5
MATCH_COLUMNS = ["Name", "Type", "Class", "Target zone", "Output zone", "Target pixels", "Output pixels", "Overlap pixels", "IoU",
                 "Status"]
_COUNT_KEYS = ("targets", "outputs", "matched", "missed", "spurious", "split_targets", "merged_outputs")
_CLASS_COLUMNS = ["target zones", "output zones", "matched", "missed", "spurious", "split targets", "merged outputs", "zone recall",
                  "zone precision", "zone F1", "mean matched IoU", "missed target area (mm^2)", "spurious output area (mm^2)"]
EVALUATION_COLUMNS = ["Name", "Type"] + ["%s %s" % (CLASS_NAMES[c], k) for c in (1, 2) for k in _CLASS_COLUMNS]


def _zone_index_plane(lab: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """Per pixel the index of its zone among ``rows`` (``_zones_of_map(lab)``), -1 outside every zone."""
    from scipy import ndimage
    plane = np.full(lab.shape, -1, dtype=np.int64)
    for c in (1, 2):
        comp, k = ndimage.label(lab == c, structure=np.ones((3, 3), dtype=bool))
        if k == 0:
            continue
        flat = comp.ravel()
        at = np.flatnonzero(flat)                                 # raster order
        ids, first = np.unique(flat[at], return_index=True)       # a component's first pixel: its first occurrence
        lut = np.zeros(k + 1, dtype=np.int64)
        lut[ids] = np.searchsorted(rows[:, 0], at[first])         # its position in first-pixel order, both classes merged
        plane[comp > 0] = lut[comp[comp > 0]]
    return plane


def match_cpu(labels, target_classes) -> List[tuple]:
    """Per image of ``labels`` and ``target_classes`` (integers of the same shape, ``[H,W]`` or ``[N,H,W]``; the target as
    ``target_classes(grey)`` gives it): ``(out_rows, tgt_rows, pairs)`` -- the zone rows of both maps (``zones_cpu``) and the
    int64 ``[k, 3]`` pair rows (``PAIR_FIELDS``) sorted by (output index, target index)."""
    labels, tc = np.asarray(labels), np.asarray(target_classes)
    if labels.shape != tc.shape:
        raise ValueError("labels and target_classes must have the same shape")
    if labels.ndim == 2:
        labels, tc = labels[None], tc[None]
    if labels.ndim != 3 or labels.shape[1] < 1 or labels.shape[2] < 1:
        raise ValueError("labels must be [H,W] or [N,H,W] with H, W >= 1")
    out = []
    for lab, tgt in zip(labels, tc):
        lab, tgt = lab.astype(np.int64), tgt.astype(np.int64)
        out_rows, tgt_rows = _zones_of_map(lab), _zones_of_map(tgt)
        po, pt = _zone_index_plane(lab, out_rows), _zone_index_plane(tgt, tgt_rows)
        both = (po >= 0) & (pt >= 0) & (lab == tgt)
        width = len(tgt_rows) + 1
        keys, counts = np.unique(po[both] * width + pt[both], return_counts=True)
        out.append((out_rows, tgt_rows, np.stack([keys // width, keys % width, counts], axis=1).astype(np.int64).reshape(-1, PAIR_ROW)))
    return out


def check_match_iou(iou) -> float:
    """The matching threshold as a float in [0.5, 1); ValueError otherwise.  From 0.5 on and with a strict ``>`` a zone has at
    most one partner: two partners of zone i would each hold more than half of i's pixels."""
    try:
        v = float(iou)
    except (TypeError, ValueError):
        raise ValueError("--match_iou must be a number in [0.5, 1)")
    if not 0.5 <= v < 1.0:
        raise ValueError("--match_iou must lie in [0.5, 1), got %r" % (iou,))
    return v


def match_details(out_rows, tgt_rows, pairs, iou: float = DEFAULT_MATCH_IOU) -> dict:
    """Who matches whom.  Output zone i and target zone j match iff ``inter > iou * (|i| + |j| - inter)``.  Returns
    ``{"partner_of_target": int64 [T] (output index or -1), "partner_of_output": int64 [O] (target index or -1),
    "best_of_target": int64 [T] (the output zone with the largest overlap, the lower index on a tie, or -1), "overlap":
    {(i, j): pixels}, "iou": {(i, j): float64 of every pair}, "outputs_on_target": int64 [T], "targets_on_output": int64 [O]}``
    (the last two: how many zones of the other map overlap each zone).  The order of ``pairs`` does not matter."""
    iou = check_match_iou(iou)
    out_rows = np.asarray(out_rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    tgt_rows = np.asarray(tgt_rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, PAIR_ROW)
    n_out, n_tgt = len(out_rows), len(tgt_rows)
    partner_t, partner_o = np.full(n_tgt, -1, dtype=np.int64), np.full(n_out, -1, dtype=np.int64)
    best_t, best_px = np.full(n_tgt, -1, dtype=np.int64), np.zeros(n_tgt, dtype=np.int64)
    on_t, on_o = np.zeros(n_tgt, dtype=np.int64), np.zeros(n_out, dtype=np.int64)
    overlap, ious = {}, {}
    for i, j, inter in pairs.tolist():
        if out_rows[i, 1] != tgt_rows[j, 1] or inter < 1:
            raise ValueError("pair (%d, %d): zones of different classes, or no shared pixel" % (i, j))
        union = int(out_rows[i, 2]) + int(tgt_rows[j, 2]) - inter
        overlap[(i, j)], ious[(i, j)] = inter, inter / union
        on_t[j] += 1
        on_o[i] += 1
        if inter > best_px[j] or (inter == best_px[j] and i < best_t[j]):
            best_t[j], best_px[j] = i, inter
        if inter > iou * union:
            partner_t[j], partner_o[i] = i, j
    return {"partner_of_target": partner_t, "partner_of_output": partner_o, "best_of_target": best_t, "overlap": overlap, "iou": ious,
            "outputs_on_target": on_t, "targets_on_output": on_o}


def _ratio(a, b):
    return a / b if b else None


def match_figures(out_rows, tgt_rows, pairs, iou: float = DEFAULT_MATCH_IOU) -> dict:
    """The zone figures of one image, per class name (``"Bark"``, ``"Node"``): the counts ``targets``, ``outputs``,
    ``matched``, ``missed`` (targets without a partner), ``spurious`` (outputs without one), ``split_targets`` (target zones
    overlapped by two or more output zones) and ``merged_outputs`` (output zones overlapping two or more target zones); the
    zones' ``recall`` (matched / targets), ``precision`` (matched / outputs) and ``f1`` (2 matched / (targets + outputs)), None
    where the denominator is 0; ``mean_iou`` of the matched pairs (None without one) and their ``iou_sum``; the pixels of the
    missed targets and of the spurious outputs."""
    out_rows = np.asarray(out_rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    tgt_rows = np.asarray(tgt_rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    d = match_details(out_rows, tgt_rows, pairs, iou)
    fig = {}
    for c in (1, 2):
        t, o = tgt_rows[:, 1] == c, out_rows[:, 1] == c
        found = t & (d["partner_of_target"] >= 0)
        lone = o & (d["partner_of_output"] < 0)
        matched = int(found.sum())
        iou_sum = math.fsum(d["iou"][(int(d["partner_of_target"][j]), int(j))] for j in np.flatnonzero(found))
        n_t, n_o = int(t.sum()), int(o.sum())
        fig[CLASS_NAMES[c]] = {
            "targets": n_t, "outputs": n_o, "matched": matched, "missed": n_t - matched, "spurious": int(lone.sum()),
            "split_targets": int((t & (d["outputs_on_target"] >= 2)).sum()),
            "merged_outputs": int((o & (d["targets_on_output"] >= 2)).sum()),
            "recall": _ratio(matched, n_t), "precision": _ratio(matched, n_o), "f1": _ratio(2 * matched, n_t + n_o),
            "mean_iou": _ratio(iou_sum, matched), "iou_sum": iou_sum,
            "missed_pixels": int(tgt_rows[t & ~found, 2].sum()), "spurious_pixels": int(out_rows[lone, 2].sum())}
    return fig


def _six(v) -> str:
    return "" if v is None else "{:.6f}".format(float(v))


def match_rows(name: str, wood: str, out_rows, tgt_rows, pairs, iou: float = DEFAULT_MATCH_IOU) -> List[List[str]]:
    """The rows of ``zone_matches.csv`` (``MATCH_COLUMNS``) of one image: one per target zone in their order (``matched`` with
    its partner; ``missed`` with the output zone of the largest overlap, the lower index on a tie, or with those four cells
    empty), then one per spurious output zone (no target zone, target pixels, overlap or IoU).  Zones are numbered from 1 as
    ``zone_rows`` numbers them; the IoU is printed to 6 decimals from float64."""
    out_rows = np.asarray(out_rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    tgt_rows = np.asarray(tgt_rows, dtype=np.int64).reshape(-1, ZONE_ROW)
    d = match_details(out_rows, tgt_rows, pairs, iou)
    rows = []
    for j, tr in enumerate(tgt_rows.tolist()):
        i = int(d["partner_of_target"][j])
        status = "matched" if i >= 0 else "missed"
        if i < 0:
            i = int(d["best_of_target"][j])
        seen = [str(i + 1), str(int(out_rows[i, 2])), str(d["overlap"][(i, j)]), _six(d["iou"][(i, j)])] if i >= 0 else [""] * 4
        rows.append([name, wood, CLASS_NAMES[tr[1]], str(j + 1), seen[0], str(tr[2]), seen[1], seen[2], seen[3], status])
    for i in np.flatnonzero(d["partner_of_output"] < 0).tolist():
        rows.append([name, wood, CLASS_NAMES[int(out_rows[i, 1])], "", str(i + 1), "", str(int(out_rows[i, 2])), "", "", "spurious"])
    return rows


def evaluation_rows(name: str, wood: str, figures: dict) -> List[List[str]]:
    """The row of ``zone_evaluation.csv`` (``EVALUATION_COLUMNS``) of one image from its ``match_figures``, as a one-element
    list: per class the seven counts, recall, precision, F1 and the mean matched IoU to 6 decimals (empty where undefined), and
    the areas of the missed targets and of the spurious outputs as ``zone_rows`` prints an area."""
    row = [name, wood]
    for c in (1, 2):
        f = figures[CLASS_NAMES[c]]
        row += [str(f[k]) for k in _COUNT_KEYS] + [_six(f["recall"]), _six(f["precision"]), _six(f["f1"]), _six(f["mean_iou"]),
                                                   "{:.5f}".format(area_mm2(f["missed_pixels"])),
                                                   "{:.5f}".format(area_mm2(f["spurious_pixels"]))]
    return [row]


def match_summary(figures: Sequence[dict], iou: float, cap: int, pair_cap: int, host_fallbacks: int) -> dict:
    """The ``"zones"`` entry of ``evaluation_summary.json``: per class the folder totals of the counts, recall, precision and F1
    pooled from those totals and the mean IoU over every matched pair of the folder; the threshold, both caps and the number
    of images matched on the host."""
    doc = {"images": len(figures), "match_iou": float(iou), "zones_cap": int(cap), "zone_pairs_cap": int(pair_cap),
           "host_fallbacks": int(host_fallbacks)}
    for c in (1, 2):
        per = [f[CLASS_NAMES[c]] for f in figures]
        tot = {k: sum(p[k] for p in per) for k in _COUNT_KEYS}
        doc[CLASS_NAMES[c]] = dict(tot, recall=_ratio(tot["matched"], tot["targets"]), precision=_ratio(tot["matched"], tot["outputs"]),
                                   f1=_ratio(2 * tot["matched"], tot["targets"] + tot["outputs"]),
                                   mean_iou=_ratio(math.fsum(p["iou_sum"] for p in per), tot["matched"]))
    return doc
