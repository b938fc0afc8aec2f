"""The zones of a label map: the host restatement of ``nbc_label_zones`` (include/nbc.h, csrc/zones.hip) and the report
``predict --zones`` writes from the rows.

A zone is an 8-connected component of one class c in {1, 2} (Bark, Node); pixels of any other value belong to no zone.  Its
row is ten integers, ``ZONE_FIELDS``: the first pixel in raster order (``y * W + x``), the class, the pixel count, the
inclusive bounding box, the coordinate sums over its pixels and the perimeter -- the number of pixel sides (4-neighbourhood)
whose neighbour has another label or lies outside the image.  The rows of an image are sorted by first pixel.

``zones_cpu`` is built on ``scipy.ndimage.label`` per class plus numpy reductions and does not depend on scipy's numbering;
the device pass must equal it integer for integer.  The reference has no such code: nothing here restates it but the
millimetres of models.py:210 (3.6 mm per pixel side) and the float32 area arithmetic of ``predict.stats_row``."""
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
