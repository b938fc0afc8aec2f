"""`evaluate --contours` without a GPU: the host restatement contours.contours_cpu against answers worked out by hand and
against a brute-force minimum over all pairs (so that the oracle of tests/test_gpu_contours.py is not its own witness), the
figures of contours.contour_figures on hand-made rows, the refusals of nbc_contour_distances in front of the device, the
formatting of the report, the command line's refusals and the gather of the per-image rows and pooled histograms over gloo."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from neuralbarkcalculator_amd import _lib, contours, folder_run, zones
from neuralbarkcalculator_amd import evaluate as drv
from neuralbarkcalculator_amd.metrics import target_classes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = contours.HEAD
GREY = np.array([0, 128, 255], dtype=np.uint8)       # a grey level of each class


def one(labels, target_classes_, bins=None):
    rows, sum_d = contours.contours_cpu(np.array(labels, dtype=np.uint8), GREY[np.array(target_classes_)], bins)
    assert rows.dtype == np.int64 and sum_d.dtype == np.float64 and rows.shape[:2] == (1, 4) and sum_d.shape == (1, 4)
    return rows[0], sum_d[0]


def test_constants_and_signatures(built_lib):
    assert contours.SETS == _lib.CONTOUR_SETS == 4 and contours.HEAD == _lib.CONTOUR_HEAD == 4
    assert contours.MAX_SIDE == _lib.CONTOUR_MAX_SIDE == 4096
    assert contours.MAX_BINS == contours.default_bins(4096, 4096) == math.ceil(math.hypot(4095, 4095)) + 1 == 5793
    assert contours.default_bins(1024, 1024) == math.ceil(math.hypot(1023, 1023)) + 1 == 1448
    assert contours.default_bins(1, 1) == 2 and contours.default_bins(1, 2) == 2 and contours.default_bins(1, 3) == 3
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for line in ("#define NBC_CONTOUR_SETS 4", "#define NBC_CONTOUR_HEAD 4", "#define NBC_CONTOUR_MAX_SIDE 4096",
                 "size_t nbc_contours_workspace_bytes(int N, int H, int W);",
                 "int nbc_contour_distances(nbc_ctx* ctx, const void* labels_dev, int labels_dtype, const uint8_t* target_grey_dev,"):
        assert line in header, line
    assert hasattr(built_lib, "nbc_contour_distances") and hasattr(built_lib, "nbc_contours_workspace_bytes")
    assert _lib.SIGNATURES["nbc_contours_workspace_bytes"] == (C.c_size_t, [C.c_int] * 3)
    assert _lib.SIGNATURES["nbc_contour_distances"][0] == C.c_int and len(_lib.SIGNATURES["nbc_contour_distances"][1]) == 13


def test_contour_distances_refusals_come_before_the_device(built_lib):
    """No context exists on a machine without a GPU: every refusal below comes from the argument checks in front of it."""
    fake = 1 << 40
    a = lambda x: (x + 255) // 256 * 256
    for n, h, w in ((2, 64, 64), (1, 1, 1), (3, 37, 53), (8, 1024, 1024), (1, 4096, 4096), (65535, 1, 1)):
        # a mark byte per pixel, four u16 column distances per pixel, an f64 partial per image, set and row
        assert built_lib.nbc_contours_workspace_bytes(n, h, w) == a(n * h * w) + a(8 * n * h * w) + a(8 * 4 * n * h), (n, h, w)
    for shape in ((0, 64, 64), (65536, 64, 64), (1, 0, 64), (1, 64, 0), (1, 4097, 1), (1, 1, 4097), (-1, 8, 8)):
        assert built_lib.nbc_contours_workspace_bytes(*shape) == 0, shape
    need = built_lib.nbc_contours_workspace_bytes(2, 64, 64)

    def call(ctx=fake, labels=fake, dtype=_lib.LABEL_U8, target=fake, N=2, H=64, W=64, rows=fake, bins=91, sum_d=fake, ws=fake,
             ws_bytes=need):
        return built_lib.nbc_contour_distances(ctx, labels, dtype, target, N, H, W, rows, bins, sum_d, ws, ws_bytes, None)

    nulls = [(dict([(k, None)]), "null argument") for k in ("ctx", "labels", "target", "rows", "sum_d", "ws")]
    for kw, text in nulls + [(dict(N=0), "bad shape"), (dict(N=65536), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"),
                             (dict(H=-3), "bad shape"), (dict(H=4097), "bad shape"), (dict(W=4097), "bad shape"),
                             (dict(bins=1), "bins must lie in 2..5793"), (dict(bins=0), "bins must lie in 2..5793"),
                             (dict(bins=5794), "bins must lie in 2..5793"), (dict(bins=-7), "bins must"),
                             (dict(dtype=7), "bad labels_dtype"), (dict(ws_bytes=need - 1), "workspace of"),
                             (dict(ws_bytes=0), "workspace of"), (dict(N=3), "workspace of"),
                             (dict(ws=fake + 128), "256-byte aligned")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        err = _lib.last_error()
        assert err.startswith("nbc_contour_distances:") and text in err, (kw, err)


def test_model_object_refusals():
    from neuralbarkcalculator_amd.model import FCNResNet50
    with pytest.raises(RuntimeError):                                    # no device: no context
        FCNResNet50("fp32").contour_distances(np.zeros((4, 4)), np.zeros((4, 4)))


RECT = np.zeros((5, 7), dtype=np.uint8)
RECT[1:4, 1:5] = 1                                   # a 3 x 4 rectangle: its contour is its ring of 10, the 2 inside are not


def test_a_rectangle_whose_contour_is_its_ring():
    ring = contours.contour(RECT == 1)
    assert ring.astype(int).tolist() == [[0, 0, 0, 0, 0, 0, 0],
                                         [0, 1, 1, 1, 1, 0, 0],
                                         [0, 1, 0, 0, 1, 0, 0],
                                         [0, 1, 1, 1, 1, 0, 0],
                                         [0, 0, 0, 0, 0, 0, 0]]
    rows, sum_d = one(RECT, RECT)                                        # against itself: every distance is 0
    assert contours.default_bins(5, 7) == 9 and rows.shape == (4, HEAD + 9)
    assert rows[0].tolist() == [10, 10, 0, 0, 10] + [0] * 8 and rows[1].tolist() == rows[0].tolist()
    assert not rows[2:].any() and sum_d.tolist() == [0.0] * 4
    moved = np.roll(RECT, 1, axis=1)                                     # the target one pixel to the right
    rows, sum_d = one(RECT, moved)
    # the output's ring spans x = 1..4, the target's x = 2..5.  Rows 1 and 3 of the output's ring: x = 1 is 1 away, x = 2, 3, 4
    # lie on the target's ring.  Row 2: x = 1 is 1 away from (2, 2), and x = 4 is 1 away from (2, 5) and from (1, 4).
    # Six pixels at distance 0 and four at distance 1, and the same the other way round by symmetry
    assert rows[0, :HEAD].tolist() == [10, 10, 4, 1] and rows[0, HEAD:HEAD + 2].tolist() == [6, 4] and sum_d[0] == 4.0
    assert rows[1, :HEAD].tolist() == [10, 10, 4, 1] and rows[1, HEAD:HEAD + 2].tolist() == [6, 4] and sum_d[1] == 4.0


def test_the_frame_is_no_contour_side():
    m = np.zeros((5, 7), dtype=np.uint8)
    m[:3, :4] = 1                                    # the same rectangle in the corner: only its two inner sides are contour
    assert contours.contour(m == 1).astype(int).tolist() == [[0, 0, 0, 1, 0, 0, 0],
                                                            [0, 0, 0, 1, 0, 0, 0],
                                                            [1, 1, 1, 1, 0, 0, 0],
                                                            [0, 0, 0, 0, 0, 0, 0],
                                                            [0, 0, 0, 0, 0, 0, 0]]
    rows, _ = one(m, m)
    assert rows[0, :HEAD].tolist() == [6, 6, 0, 0]
    # zones.py's perimeter counts the frame: 14 sides for the same zone
    assert zones.zones_cpu(m)[0][0, 9] == 14
    filled = np.ones((5, 7), dtype=np.uint8)         # a filled map has no contour at all
    assert not contours.contour(filled == 1).any()
    rows, sum_d = one(filled, filled)
    assert not rows.any() and not sum_d.any()
    rows, sum_d = one(filled, RECT)                  # nothing to start from in the output, 10 ring pixels with no destination
    assert rows[0].tolist() == [0, 10] + [0] * 11 and rows[1].tolist() == [10, 0] + [0] * 11 and not sum_d.any()
    strip = np.ones((1, 6), dtype=np.uint8)          # a single row: the vertical neighbours lie outside
    strip[0, 4:] = 0
    assert contours.contour(strip == 1).astype(int).tolist() == [[0, 0, 0, 1, 0, 0]]


def test_single_pixels_and_the_bin_rule():
    lab, tgt = np.zeros((6, 8), dtype=np.uint8), np.zeros((6, 8), dtype=np.uint8)
    lab[2, 2] = 2
    rows, sum_d = one(lab, lab)
    assert rows[2].tolist() == [1, 1, 0, 0, 1] + [0] * (rows.shape[1] - 5) and rows[3].tolist() == rows[2].tolist()
    one_px = np.array([[1]], dtype=np.uint8)         # a 1 x 1 map: its pixel has no neighbour inside the image
    rows, _ = one(one_px, one_px)
    assert rows.shape == (4, HEAD + 2) and not rows.any()
    # two single pixels at offsets (k, 0) and (k, 1), k = 3: d2 = 9 lands in bin 3, d2 = 10 in bin 4
    k = 3
    tgt[1, 1] = 1
    for off, d2, b in (((k, 0), 9, 3), ((k, 1), 10, 4), ((0, k), 9, 3), ((1, k), 10, 4)):
        lab = np.zeros((6, 8), dtype=np.uint8)
        lab[1 + off[0], 1 + off[1]] = 1
        rows, sum_d = one(lab, tgt)
        for s in (0, 1):
            assert rows[s, :HEAD].tolist() == [1, 1, d2, d2], (off, s)
            assert np.flatnonzero(rows[s, HEAD:]).tolist() == [b] and rows[s, HEAD + b] == 1
            assert sum_d[s] == math.sqrt(d2)
        rows, _ = one(lab, tgt, bins=4)              # bins 0..2 and the overflow bin 3: everything above 2 * 2
        assert rows[0, HEAD:].tolist() == [0, 0, 0, 1]
    for d2 in list(range(0, 300)) + [v * v + j for v in (1447, 4095, 5791) for j in (-1, 0, 1)]:
        b = contours.ceil_sqrt(d2)
        assert (b == 0 and d2 == 0) or (b - 1) ** 2 < d2 <= b * b


def brute(lab, grey, bins):
    """The definition itself: the minimum over all pairs, the contour from padded shifts."""
    tgt = target_classes(grey)
    rows, sums = np.zeros((4, HEAD + bins), dtype=np.int64), np.zeros(4)

    def ring(m):
        p = np.pad(m, 1, constant_values=True)
        return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])
    for c in (1, 2):
        kinds = (ring(lab == c), ring(tgt == c))
        for direction in (0, 1):
            s, src, dst = 2 * (c - 1) + direction, kinds[direction], kinds[1 - direction]
            rows[s, 0], rows[s, 1] = src.sum(), dst.sum()
            if not rows[s, 0] or not rows[s, 1]:
                continue
            (ys, xs), (qy, qx) = np.nonzero(src), np.nonzero(dst)
            d2 = ((ys[:, None] - qy[None]) ** 2 + (xs[:, None] - qx[None]) ** 2).min(axis=1)
            rows[s, 2], rows[s, 3] = d2.sum(), d2.max()
            for v in d2.tolist():
                rows[s, HEAD + min(contours.ceil_sqrt(v), bins - 1)] += 1
            sums[s] = math.fsum(math.sqrt(v) for v in d2.tolist())
    return rows, sums


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (5, 7), (37, 53), (3, 300)])
def test_restatement_equals_the_brute_force_minimum(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    for trial in range(4):
        if trial < 2:                                # three classes per pixel, every grey level, labels outside 0..2
            lab = rng.integers(0, 4, size=(h, w)).astype(np.uint8)
            grey = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        else:                                        # sparse: a few pixels of each class
            lab = (rng.random((h, w)) < 0.05).astype(np.uint8) * rng.integers(1, 3, size=(h, w)).astype(np.uint8)
            grey = GREY[(rng.random((h, w)) < 0.05).astype(np.uint8) * rng.integers(1, 3, size=(h, w))]
        for bins in (None, 2, 5):
            rows, sum_d = contours.contours_cpu(lab, grey, bins)
            want_rows, want_sum = brute(lab, grey, rows.shape[2] - HEAD)
            assert np.array_equal(rows[0], want_rows) and np.array_equal(sum_d[0], want_sum), (h, w, trial, bins)
    both = contours.contours_cpu(np.stack([lab, lab]), np.stack([grey, grey]))      # a batch comes back per image
    assert np.array_equal(both[0][0], both[0][1]) and np.array_equal(both[0][0], contours.contours_cpu(lab, grey)[0][0])
    with pytest.raises(ValueError):
        contours.contours_cpu(np.zeros((2, 2)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        contours.contours_cpu(np.zeros((2, 2)), np.zeros((2, 2)), bins=1)


def hand_rows(bins=12, **sets):
    """rows [4, HEAD + bins] and sum_d [4] from ``s0=dict(hist={bin: count}, max_d2=.., sum_d=.., m=..)`` ..."""
    rows, sum_d = np.zeros((4, HEAD + bins), dtype=np.int64), np.zeros(4)
    for key, d in sets.items():
        s = int(key[1])
        for b, c in d.get("hist", {}).items():
            rows[s, HEAD + b] = c
        rows[s, 0] = d.get("n", rows[s, HEAD:].sum())
        rows[s, 1], rows[s, 2], rows[s, 3] = d.get("m", 1), d.get("sum_d2", 0), d.get("max_d2", 0)
        sum_d[s] = d.get("sum_d", 0.0)
    return rows, sum_d


def test_hd95_at_the_exact_boundary():
    # n = 20: 19 pixels in bin 1 are exactly 95 %, so HD95 is 1 pixel; n = 21 with 19 there is below 95 %: the next used bin
    rows, sum_d = hand_rows(s0=dict(hist={1: 19, 7: 1}, m=5, max_d2=49), s1=dict(hist={0: 5}, m=20))
    f = contours.contour_figures(rows, sum_d, 2)["Bark"]
    assert f["hd95_mm"] == 1 * 3.6 and f["hd_mm"] == 7 * 3.6 and f["output_pixels"] == 20 and f["target_pixels"] == 5
    rows, sum_d = hand_rows(s0=dict(hist={1: 19, 7: 2}, m=5, max_d2=49), s1=dict(hist={0: 5}, m=21))
    assert contours.contour_figures(rows, sum_d, 2)["Bark"]["hd95_mm"] == 7 * 3.6
    rows, sum_d = hand_rows(s0=dict(hist={1: 18, 7: 2}, m=5, max_d2=49), s1=dict(hist={0: 5}, m=20))
    assert contours.contour_figures(rows, sum_d, 2)["Bark"]["hd95_mm"] == 7 * 3.6
    # the larger of the two directions
    rows, sum_d = hand_rows(s2=dict(hist={0: 20}, m=4), s3=dict(hist={3: 4}, m=20, max_d2=9))
    f = contours.contour_figures(rows, sum_d, 2)["Node"]
    assert f["hd95_mm"] == 3 * 3.6 and f["hd_mm"] == 3 * 3.6


def test_precision_recall_f1_and_the_mm_factors():
    rows, sum_d = hand_rows(s0=dict(hist={0: 6, 1: 2, 2: 1, 3: 1}, m=4, max_d2=8, sum_d=7.5),
                            s1=dict(hist={0: 1, 2: 1, 5: 2}, m=10, max_d2=25, sum_d=12.5))
    f = contours.contour_figures(rows, sum_d, 2)["Bark"]
    assert f["precision"] == 0.9 and f["recall"] == 0.5 and f["f1"] == 2 * 0.9 * 0.5 / 1.4
    assert f["mean_distance_mm"] == (7.5 + 12.5) / 14 * 3.6 and f["hd_mm"] == 5 * 3.6 and not f["one_sided"]
    assert f["within_output"] == 9 and f["within_target"] == 2 and f["sum_d"] == (7.5, 12.5)
    f0 = contours.contour_figures(rows, sum_d, 0)["Bark"]                 # tolerance 0: only the pixels on the other contour
    assert f0["precision"] == 0.6 and f0["recall"] == 0.25 and f0["f1"] == 2 * 0.6 * 0.25 / 0.85
    assert contours.contour_figures(rows, sum_d, 50)["Bark"]["precision"] == 1.0   # beyond the last bin: everything
    rows0, sum0 = hand_rows(s0=dict(hist={3: 2}, m=1), s1=dict(hist={3: 1}, m=2))
    f = contours.contour_figures(rows0, sum0, 0)["Bark"]                  # nothing within: F1 is 0, not undefined
    assert f["precision"] == 0.0 and f["recall"] == 0.0 and f["f1"] == 0.0
    assert zones.MM_PER_PIXEL == 3.6 and contours.DEFAULT_TOLERANCE == 2
    for bad in (-1, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError):
            contours.contour_figures(rows, sum_d, bad)


def test_empty_and_one_sided_classes():
    rows, sum_d = hand_rows(s0=dict(n=7, m=0), s1=dict(n=0, m=7))         # bark in the output only; no node anywhere
    fig = contours.contour_figures(rows, sum_d, 2)
    b, n = fig["Bark"], fig["Node"]
    assert (b["output_pixels"], b["target_pixels"], b["one_sided"]) == (7, 0, True)
    assert b["precision"] == 0.0 and b["recall"] == 0.0 and b["f1"] == 0.0
    assert b["mean_distance_mm"] is None and b["hd95_mm"] is None and b["hd_mm"] is None
    assert (n["output_pixels"], n["target_pixels"], n["one_sided"]) == (0, 0, False)
    assert all(n[k] is None for k in ("precision", "recall", "f1", "mean_distance_mm", "hd95_mm", "hd_mm"))
    assert contours.contour_rows("a.png", "sapin", fig) == [["a.png", "sapin", "7", "0", "0.000000", "0.000000", "0.000000", "", "", "",
                                                             "0", "0", "", "", "", "", "", ""]]


def test_rows_and_summary_formatting():
    assert contours.CONTOUR_COLUMNS[:4] == ["Name", "Type", "Bark output contour pixels", "Bark target contour pixels"]
    assert len(contours.CONTOUR_COLUMNS) == 2 + 2 * 8 and contours.CONTOUR_COLUMNS[10] == "Node output contour pixels"
    assert contours.CONTOUR_COLUMNS[8] == "Bark HD95 (mm)" and contours.WIRE_WIDTH == 28
    r1 = hand_rows(s0=dict(hist={0: 6, 1: 2, 2: 1, 3: 1}, m=4, max_d2=8, sum_d=7.5),
                   s1=dict(hist={0: 1, 2: 1, 5: 2}, m=10, max_d2=25, sum_d=12.5))
    r2 = hand_rows(s0=dict(n=7, m=0), s1=dict(n=0, m=7), s2=dict(hist={1: 4}, m=4, max_d2=1, sum_d=4.0),
                   s3=dict(hist={1: 4}, m=4, max_d2=1, sum_d=4.0))
    f1, f2 = contours.contour_figures(*r1, 2), contours.contour_figures(*r2, 2)
    assert contours.contour_rows("a.png", "sapin", f1) == [
        ["a.png", "sapin", "10", "4", "0.900000", "0.500000", "0.642857", "5.143", "18.000", "18.000", "0", "0", "", "", "", "", "", ""]]
    assert contours.contour_rows("b.png", "sapin", f2)[0][10:] == ["4", "4", "1.000000", "1.000000", "1.000000", "3.600", "3.600", "3.600"]
    hist = contours.pooled_histogram(np.stack([r1[0], r2[0]]), 16)
    assert hist.shape == (4, 16) and hist[0, :4].tolist() == [6, 2, 1, 1] and hist[2, 1] == 4 and hist.sum() == 22
    doc = contours.contour_summary([f1, f2], 2, hist)
    assert doc["images"] == 2 and doc["tolerance_pixels"] == 2 and doc["tolerance_mm"] == 7.2
    # the one-sided image adds its 7 output pixels to the denominator and nothing within
    assert doc["Bark"] == {"output_pixels": 17, "target_pixels": 4, "within_output": 9, "within_target": 2, "precision": 9 / 17,
                           "recall": 0.5, "f1": 2 * (9 / 17) * 0.5 / (9 / 17 + 0.5), "mean_distance_mm": 20.0 / 14 * 3.6,
                           "distance_pixels": 14, "one_sided": 1}
    assert doc["Node"]["precision"] == 1.0 and doc["Node"]["mean_distance_mm"] == 3.6 and doc["Node"]["one_sided"] == 0
    assert doc["histogram"] == hist.tolist() and len(doc["sets"]) == 4
    assert contours.contour_summary([f2, f1], 2, hist)["Bark"] == doc["Bark"]      # the pooled sums do not depend on the order
    empty = contours.contour_summary([], 2, np.zeros((4, 3), dtype=np.int64))
    assert empty["Bark"]["precision"] is None and empty["Bark"]["mean_distance_mm"] is None
    json.dumps(doc)
    # what travels is enough: the figures from the wire row equal the figures from the full rows
    wire = contours.wire_rows(np.stack([r1[0], r2[0]]), np.stack([r1[1], r2[1]]), 2)
    assert wire.shape == (2, 28) and wire.dtype == np.int64
    assert contours.figures_of_wire(wire[0]) == f1 and contours.figures_of_wire(wire[1]) == f2


def test_report_files(tmp_path):
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}, {"name": "c.png", "wood": "epinette_gelee"}]
    allrows = np.zeros((3, drv.ROW_WIDTH), dtype=np.int64)
    allrows[:, 0] = (0, 1, 2)
    allrows[1, 3] = drv.STATUS_NO_DUAL                                   # b.png was skipped: its row is empty and it has no line
    ra, rc = contours.contours_cpu(RECT, GREY[np.roll(RECT, 1, axis=1)]), contours.contours_cpu(RECT, GREY[RECT * 0])
    wire = np.zeros((3, 1 + contours.WIRE_WIDTH), dtype=np.int64)
    wire[:, 0] = (0, 1, 2)
    wire[0, 1:], wire[2, 1:] = contours.wire_rows(*ra, 1)[0], contours.wire_rows(*rc, 1)[0]
    hist = contours.pooled_histogram(ra[0], 12) + contours.pooled_histogram(rc[0], 12)
    doc = drv.write_contour_report(str(tmp_path), items, allrows, wire, hist, 1)
    assert sorted(os.listdir(tmp_path)) == ["contour_evaluation.csv"]
    table = [line.split("\t") for line in open(tmp_path / "contour_evaluation.csv").read().splitlines()]
    fa, fc = contours.contour_figures(ra[0][0], ra[1][0], 1), contours.contour_figures(rc[0][0], rc[1][0], 1)
    assert table == [contours.CONTOUR_COLUMNS] + contours.contour_rows("a.png", "sapin", fa) + \
        contours.contour_rows("c.png", "epinette_gelee", fc)
    assert table[1][2:10] == ["10", "10", "1.000000", "1.000000", "1.000000", "1.440", "3.600", "3.600"]
    assert table[2][2:10] == ["10", "0", "0.000000", "0.000000", "0.000000", "", "", ""]
    assert doc == contours.contour_summary([fa, fc], 1, hist) and doc["Bark"]["one_sided"] == 1
    line = drv.format_summary({"images_evaluated": 2, "precision": "bf16", "model_path": "m.pt", "images_skipped": 1,
                               "skipped": {}, "contours": json.loads(json.dumps(doc))}).splitlines()[-1]
    assert line.startswith("contours within 1 px (3.6 mm): Bark precision 0.500, recall 1.000") and "Node precision -" in line


def _cli(*argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--contour_tolerance", "2"], "--contour_tolerance needs --contours"),
                                       (["--contours", "--contour_tolerance", "-1"], "--contour_tolerance must be an integer >= 0"),
                                       (["--contours", "--contour_tolerance", "1.5"], "invalid int value")])
def test_command_line_refusals(argv, text):
    p = _cli(*argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike():
    for kw, text in [(dict(contour_tolerance=2), "--contour_tolerance needs --contours"),
                     (dict(contours=True, contour_tolerance=-1), "must be an integer >= 0"),
                     (dict(contours=True, contour_tolerance=0.5), "must be an integer >= 0"),
                     (dict(contours=True, contour_tolerance="x"), "must be an integer >= 0")]:
        with pytest.raises(ValueError, match=text):
            drv.evaluate_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", **kw)
    drv.check_contour_arguments(True, 0)
    drv.check_contour_arguments(True, None)
    drv.check_contour_arguments(False)


WIDTH = 1 + contours.WIRE_WIDTH
BINS = 6
PER_RANK = [[0, 3], [1, 2, 4]]                       # the global indices of each rank's images: unequal shards


def _wire_of(g):
    return np.arange(WIDTH, dtype=np.int64) * (g + 1) + g


def _hist_of(rank):
    return (np.arange(4 * BINS, dtype=np.int64).reshape(4, BINS) + 1) * (rank + 1)


def _gather_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        local = np.stack([_wire_of(g) for g in PER_RANK[rank]])
        local[:, 0] = PER_RANK[rank]
        got = folder_run.gather_rows(local, 5, world, dist, None, cap=3, width=WIDTH)
        hist = folder_run.gather_ragged(np.concatenate([[rank], _hist_of(rank).ravel()])[None], world, dist, None, width=1 + 4 * BINS)
        np.save(os.path.join(out_dir, "wire_%d.npy" % rank), got)
        np.save(os.path.join(out_dir, "hist_%d.npy" % rank), hist)
    finally:
        dist.destroy_process_group()


def test_two_rank_gather_of_wire_rows_and_pooled_histograms(tmp_path):
    mp.spawn(_gather_worker, args=(2, 29699, str(tmp_path)), nprocs=2, join=True)
    want = np.stack([_wire_of(g) for g in range(5)])
    want[:, 0] = range(5)
    for r in range(2):
        got = np.load(os.path.join(str(tmp_path), "wire_%d.npy" % r))
        assert got.tolist() == want.tolist(), r
        hist = np.load(os.path.join(str(tmp_path), "hist_%d.npy" % r))
        assert hist[:, 0].tolist() == [0, 1]
        assert hist[:, 1:].sum(axis=0).reshape(4, BINS).tolist() == (_hist_of(0) + _hist_of(1)).tolist()
