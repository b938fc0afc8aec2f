"""The host side of the softmax census without a GPU: census_cpu against a per-pixel loop, figures and curves against direct
computations on the quantised probabilities, pooling, the JaccardLoss statement of DESIGN.md section 5, the CSV rows and
the command-line options."""
import math
import os
import sys

import numpy as np
import pytest

from neuralbarkcalculator_amd import calibration as cal
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as pr
from neuralbarkcalculator_amd.metrics import target_classes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import calibration_cases as cc  # noqa: E402


def _pixels(logits, grey):
    """Per finite pixel of one image, by a plain loop in Python floats: (q [3], k, t)."""
    out, nonfinite = [], 0
    h, w = logits.shape[1:]
    for y in range(h):
        for x in range(w):
            v = [float(logits[c, y, x]) for c in range(3)]
            if not all(math.isfinite(a) for a in v):
                nonfinite += 1
                out.append(None)
                continue
            m = max(v)
            e = [math.exp(a - m) for a in v]
            s = (e[0] + e[1]) + e[2]
            q = [min(65535, math.floor(a / s * 65536)) for a in e]
            k = 0
            for c in (1, 2):
                if v[c] > v[k]:
                    k = c
            t = 0 if grey is None else (int(grey[y, x]) + 64) >> 7
            out.append((q, k, t))
    return out, nonfinite


def _row_by_loop(logits, grey):
    px, nonfinite = _pixels(logits, grey)
    row = [0] * cal.WORDS
    plane = np.zeros(logits.shape[1:], np.uint8).reshape(-1)
    row[cal.OFF_NONFINITE] = nonfinite
    for i, p in enumerate(px):
        if p is None:
            continue
        q, k, t = p
        hit = 1 if grey is None else int(k == t)
        for c in range(3):
            row[cal.OFF_H + (t * 3 + c) * 256 + (q[c] >> 8)] += 1
            row[cal.OFF_M + t * 3 + c] += q[c]
            row[cal.OFF_B + t] += (q[c] - (65536 if c == t else 0)) ** 2
        row[cal.OFF_R + hit * 256 + (q[k] >> 8)] += 1
        row[cal.OFF_RS + hit * 256 + (q[k] >> 8)] += q[k]
        plane[i] = q[k] >> 8
    return row, plane.reshape(logits.shape[1:])


def test_census_cpu_equals_a_per_pixel_loop():
    logits, grey = (np.array(a) for a in cc.case(1, 7, 13)[:2])
    logits[0, 1, 3, 4] = np.nan
    logits[0, 2, 6, 12] = -np.inf
    assert (target_classes(grey[0]) == (grey[0].astype(int) + 64) >> 7).all()
    for g in (grey, None):
        rows, plane, margin = cal.census_cpu(logits, g)
        want, want_plane = _row_by_loop(logits[0], None if g is None else g[0])
        assert [int(v) for v in rows[0]] == want and np.array_equal(plane[0], want_plane)
        assert rows.dtype == np.uint64 and plane.dtype == np.uint8 and margin > 0
        assert want[cal.OFF_NONFINITE] == 2 and plane[0, 3, 4] == 0 and sum(want[:cal.OFF_R]) == 3 * (7 * 13 - 2)
    # [3,H,W] is a batch of one
    one = cal.census_cpu(logits[0], grey[0])
    assert np.array_equal(one[0], cal.census_cpu(logits, grey)[0])
    with pytest.raises(ValueError):
        cal.census_cpu(logits.astype(np.float64))
    with pytest.raises(ValueError):
        cal.census_cpu(logits, grey[:, :-1])


def test_the_test_inputs_hold_their_margin_and_their_special_pixels():
    """What tests/test_gpu_calibration.py relies on, decided by the reference alone."""
    for shape in cc.SHAPES:
        logits, grey, with_t, without = cc.case(*shape)
        assert with_t[2] > cc.MARGIN and without[2] > cc.MARGIN, (shape, with_t[2])
        n, h, w = shape
        flat = logits.reshape(n, 3, -1)
        i = np.arange(h * w)
        top = np.sort(flat[:, :, i % 7 == 0], axis=1)
        assert (top[:, 2] - top[:, 1] > 40).all()
        assert (flat[:, 0, i % 7 == 1] == flat[:, 1, i % 7 == 1]).all() and (flat[:, 0, i % 7 == 1] == flat[:, 2, i % 7 == 1]).all()
        plane = with_t[1].reshape(n, -1)
        assert (plane[:, i % 7 == 0] == 255).all() and (plane[:, i % 7 == 1] == 85).all()      # q = 65535; q = 21845
    # the margin ignores the edge at 0, which no probability can cross: a saturated pixel alone has none
    sat = np.array([25.0, -20.0, -20.0], np.float32).reshape(3, 1, 1)
    assert cal.census_cpu(sat)[2] > 0.99
    near = np.array([0.0, 0.0, math.log(2.0)], np.float32).reshape(3, 1, 1)       # 1/4, 1/4, 1/2 up to the rounding of log 2
    assert cal.census_cpu(near)[2] < 1e-2


def _direct(px, ece_bins):
    """ECE, MCE, accuracy, mean confidence, Brier, soft Jaccard and expected percentages straight from the pixels."""
    px = [p for p in px if p is not None]
    n = len(px)
    conf = [q[k] / 65536 for q, k, t in px]
    hit = [int(k == t) for q, k, t in px]
    ece, mce = 0.0, 0.0
    for b in range(ece_bins):
        idx = [i for i, (q, k, t) in enumerate(px) if (q[k] >> 8) // (256 // ece_bins) == b]
        if idx:
            gap = abs(sum(hit[i] for i in idx) / len(idx) - sum(conf[i] for i in idx) / len(idx))
            ece += len(idx) * gap / n
            mce = max(mce, gap)
    brier = sum(sum((q[c] / 65536 - (c == t)) ** 2 for c in range(3)) for q, k, t in px) / n
    jac, expected = [], []
    for c in range(3):
        inter = sum(q[c] / 65536 for q, k, t in px if t == c)
        soft = sum(q[c] / 65536 for q, k, t in px)
        hard = sum(1 for q, k, t in px if t == c)
        jac.append(inter / (soft + hard - inter + 1e-7))
        expected.append(100 * soft / n)
    return dict(ece=ece, mce=mce, accuracy=sum(hit) / n, mean_confidence=sum(conf) / n, brier=brier, soft_jaccard=jac,
                jaccard_loss=1 - sum(jac) / 3, expected_percent=expected)


@pytest.mark.parametrize("ece_bins", [1, 4, 16, 256])
def test_figures_match_direct_computation(ece_bins):
    logits, grey, with_t, _ = cc.case(3, 33, 65)
    px, _ = _pixels(logits[1], grey[1])
    fig = cal.figures(with_t[0][1], ece_bins)
    want = _direct(px, ece_bins)
    assert fig["pixels"] == 33 * 65 and fig["nonfinite"] == 0 and fig["ece_bins"] == ece_bins
    for key in ("ece", "mce", "accuracy", "mean_confidence", "brier", "jaccard_loss"):
        assert fig[key] == pytest.approx(want[key], rel=1e-12, abs=1e-15), key
    assert fig["soft_jaccard"] == pytest.approx(want["soft_jaccard"], rel=1e-12)
    assert fig["expected_percent"] == pytest.approx(want["expected_percent"], rel=1e-12)
    assert sum(fig["expected_percent"]) <= 100 and sum(fig["expected_percent"]) > 99.99     # floors lose < 3 / 65536 per pixel
    for c in range(3):
        inter = sum(q[c] / 65536 for q, k, t in px if t == c)
        card = sum(q[c] / 65536 for q, k, t in px) + sum(1 for q, k, t in px if t == c)
        assert fig["soft_dice"][c] == pytest.approx(2 * inter / card, rel=1e-12)
    if ece_bins == 1:
        assert fig["ece"] == pytest.approx(abs(fig["accuracy"] - fig["mean_confidence"]), rel=1e-12) == fig["mce"]
    for bad in (0, 3, 512, 2.5, "x"):
        with pytest.raises(ValueError):
            cal.figures(with_t[0][1], bad)
    empty = cal.figures(np.zeros(cal.WORDS, np.uint64))
    assert empty["pixels"] == 0 and empty["ece"] is None and empty["brier"] is None and empty["soft_jaccard"] == [None] * 3


def test_curves_match_a_brute_force_sweep():
    logits, grey, with_t, _ = cc.case(3, 33, 65)
    px, _ = _pixels(logits[2], grey[2])
    H = cal.split(with_t[0][2])[0]
    cv = cal.curves(H)
    for c, name in enumerate(cal.CLASSES):
        score = [q[c] >> 8 for q, k, t in px]
        pos = [t == c for q, k, t in px]
        P, N = sum(pos), len(pos) - sum(pos)
        assert (cv[name]["positives"], cv[name]["negatives"]) == (P, N) and P and N
        prev_recall, ap = 0.0, 0.0
        for j in range(255, -1, -1):
            called = [s >= j for s in score]
            tp = sum(1 for a, b in zip(called, pos) if a and b)
            fp = sum(called) - tp
            precision = tp / (tp + fp) if tp + fp else None
            recall = tp / P
            f1 = 2 * tp / (2 * tp + fp + (P - tp))
            assert cv[name]["precision"][j] == (pytest.approx(precision, rel=1e-14) if precision is not None else None)
            assert cv[name]["recall"][j] == pytest.approx(recall, rel=1e-14) and cv[name]["f1"][j] == pytest.approx(f1, rel=1e-14)
            if precision is not None:
                ap += (recall - prev_recall) * precision
            prev_recall = recall
        top = max(cv[name]["f1"])
        assert cv[name]["best_f1"] == top and cv[name]["best_threshold"] == cv[name]["f1"].index(top) / 256   # the first reaching it
        assert cv[name]["average_precision"] == pytest.approx(ap, rel=1e-12)
        # the rank statistic: pairs ordered right, ties inside a bin half
        wins = sum((sp > sn) + 0.5 * (sp == sn) for sp, p in zip(score, pos) if p for sn, q in zip(score, pos) if not q)
        assert cv[name]["auroc"] == pytest.approx(wins / (P * N), rel=1e-12)
    # a class without a positive has no curve figures
    H0 = np.array(H)
    H0[2] = 0
    lone = cal.curves(H0)["Node"]
    assert lone["positives"] == 0 and lone["average_precision"] is None and lone["auroc"] is None and lone["best_f1"] is None


def test_pooled_rows_are_the_row_of_the_concatenated_pixels():
    logits, grey, with_t, without = cc.case(3, 33, 65)
    side = np.concatenate(list(logits), axis=2)[None]                    # the three images side by side: one image of 33 x 195
    side_grey = np.concatenate(list(grey), axis=1)[None]
    assert np.array_equal(cal.pool(with_t[0]), cal.census_cpu(np.ascontiguousarray(side), np.ascontiguousarray(side_grey))[0][0])
    assert np.array_equal(cal.pool(without[0]), cal.census_cpu(np.ascontiguousarray(side))[0][0])
    assert np.array_equal(cal.pool(with_t[0].view(np.int64)), cal.pool(with_t[0]))         # the bit-cast rows of the wire too
    # the wire rows add like the rows, and give the figures of the row
    wire = cal.wire_rows(with_t[0], 16)
    assert wire.shape == (3, cal.wire_width(16)) and wire.dtype == np.int64 and cal.wire_width(16) == 80
    assert np.array_equal(wire.sum(axis=0), cal.wire_rows(cal.pool(with_t[0])[None], 16)[0])
    assert cal.figures_of_wire(wire[0], 16) == cal.figures(with_t[0][0], 16)
    # the merged bins hold what their 256 / 16 bins held
    R = cal.split(with_t[0][0])[1]
    assert wire[0][:16].tolist() == [int(sum(R[0][16 * b: 16 * b + 16])) for b in range(16)]


def test_jaccard_loss_as_the_reference_wrote_it_is_not_the_soft_jaccard():
    """with a [B,H,W] target the reference's dims are (0, 2), a [3, W] table of per-column ratios."""
    import torch
    import torch.nn.functional as F
    logits, grey, with_t, _ = cc.case(3, 33, 65)
    x, t = logits[:1], target_classes(grey[:1])
    as_written = cal.jaccard_loss_as_written(x, t)
    # the reference's lines, in torch float64
    true = torch.from_numpy(t.astype(np.int64))
    hot = torch.eye(3, dtype=torch.float64)[true.squeeze(1)].permute(0, 3, 1, 2)
    p = F.softmax(torch.from_numpy(x.astype(np.float64)), dim=1)
    dims = (0,) + tuple(range(2, true.ndimension()))
    assert dims == (0, 2)
    inter = torch.sum(p * hot, dims)
    union = torch.sum(p + hot, dims) - inter
    assert tuple(inter.shape) == (3, 65)
    assert as_written == pytest.approx(float(1 - (inter / (union + 1e-7)).mean()), rel=1e-12)
    # the dims the name means: the soft Jaccard of the census, up to the quantisation (< 3 / 65536 per pixel)
    inter, union = torch.sum(p * hot, (0, 2, 3)), torch.sum(p + hot, (0, 2, 3)) - torch.sum(p * hot, (0, 2, 3))
    meant = float(1 - (inter / (union + 1e-7)).mean())
    ours = cal.figures(with_t[0][0])["jaccard_loss"]
    assert abs(ours - meant) < 1e-4
    assert abs(ours - as_written) > 1e-3 and as_written != meant


def test_csv_rows_and_summaries():
    logits, grey, with_t, without = cc.case(3, 33, 65)
    fig = cal.figures(with_t[0][0])
    hard = [1000, 900, 245]
    row, = cal.calibration_rows("a.png", "sapin", fig, hard)
    assert len(row) == len(cal.CALIBRATION_COLUMNS) == 16 and row[:2] == ["a.png", "sapin"]
    assert row[2] == "{:.6f}".format(fig["ece"]) and row[6] == "{:.6f}".format(fig["brier"]) and row[-1] == "0"
    assert row[11] == "{:.6f}".format(fig["expected_percent"][1]) and row[12] == "{:.6f}".format(100 * 900 / 2145)
    assert cal.calibration_rows("a", "b", cal.figures(np.zeros(cal.WORDS, np.uint64)), [0, 0, 0])[0][2:] == [""] * 13 + ["0"]
    pooled = cal.pool(with_t[0])
    conf = np.array([[700, 10, 5], [20, 600, 8], [3, 9, 790]])
    doc = cal.calibration_summary(pooled, 3, 16, conf)
    assert list(doc) == ["images", "ece_bins", "pooled", "Nothing", "Bark", "Node", "H", "R", "RS"]
    assert doc["pooled"]["pixels"] == 3 * 33 * 65 and doc["Bark"]["f1_at_argmax"] == 2 * 600 / (2 * 600 + 19 + 28)
    assert np.array(doc["H"]).shape == (3, 3, 256) and np.array(doc["R"]).shape == (2, 256) == np.array(doc["RS"]).shape
    assert cal.figures(np.array(doc["H"]).ravel().tolist() + np.array(doc["R"]).ravel().tolist() + np.array(doc["RS"]).ravel().tolist()
                       + [int(v) for v in pooled[cal.OFF_M:]], 64)["ece"] == cal.figures(pooled, 64)["ece"]
    import json
    json.dumps(doc)
    curve = cal.curve_rows(pooled)
    assert len(curve) == 3 * 256 + 256 and all(len(r) == len(cal.CURVE_COLUMNS) for r in curve)
    assert curve[0][:4] == ["curve", "Nothing", "0", "0.000000"] and curve[768][0] == "reliability"
    assert sum(int(r[7]) for r in curve[768:]) == 3 * 33 * 65
    # predict --confidence: no target
    r0 = without[0][0]
    low = cal.below_threshold(r0, 0.9)
    plane = without[1][0]
    assert low == int((plane < 231).sum()) and math.ceil(0.9 * 256) == 231
    assert cal.below_threshold(r0, 1.0) == 33 * 65 and cal.below_threshold(r0, 1 / 256) == 0     # no bin proves p_k >= 1
    crow, = cal.confidence_rows("a.png", "sapin", r0, hard, 0.9)
    assert len(crow) == len(cal.CONFIDENCE_COLUMNS) and crow[3] == "{:.6f}".format(100 * low / 2145)
    assert crow[4] == "{:.2f}".format(low * 12.96) and crow[8] == "{:.2f}".format(900 * 12.96)
    assert crow == cal.confidence_rows_of_wire("a.png", "sapin", cal.figures_of_wire(cal.wire_rows(r0[None])[0]), low, hard)[0]
    summary = cal.confidence_summary(cal.pool(without[0]), 3, 0.9, [3000, 2700, 735])
    assert summary["pixels"] == 3 * 33 * 65 and summary["hard_percent"]["Bark"] == 100 * 2700 / 6435 and len(summary["R"]) == 256
    json.dumps(summary)
    for bad in (0, 1.5, -1, "x"):
        with pytest.raises(ValueError):
            cal.check_confidence_threshold(bad)


# ---- the command line ---------------------------------------------------------------------------------------------------
def _fake(seen, key):
    def fake(root, model_path, precision, *a, **kw):
        seen.append(kw)
        return {"rank": 0, "summary": {"images_evaluated": 0, "precision": precision, "model_path": model_path,
                                       "images_skipped": 0, "skipped": {}},
                "images_total": 0, "images_this_rank": 0, "batches": 0, "total_s": 0.0, "images_per_s_loop": 0.0}
    return fake


def test_options_parse_reach_the_folder_runs_and_are_refused(monkeypatch, tmp_path, capsys):
    seen = []
    monkeypatch.setattr(ev, "evaluate_folder", _fake(seen, "ev"))
    monkeypatch.setattr(pr, "predict_folder", _fake(seen, "pr"))
    root = str(tmp_path)
    ev.main([root, "--precision", "fp32"])
    assert "calibration" not in seen[-1] and "ece_bins" not in seen[-1]
    ev.main([root, "--precision", "fp32", "--calibration"])
    assert seen[-1]["calibration"] is True and seen[-1]["ece_bins"] is None
    ev.main([root, "--precision", "fp32", "--calibration", "--ece_bins", "64", "--ce"])
    assert seen[-1]["calibration"] is True and seen[-1]["ece_bins"] == 64 and seen[-1]["ce"] is True
    pr.main([root, "--precision", "fp32"])
    assert "confidence" not in seen[-1]
    pr.main([root, "--precision", "fp32", "--confidence", "--confidence_threshold", "0.75"])
    assert seen[-1]["confidence"] is True and seen[-1]["confidence_threshold"] == 0.75
    n = len(seen)
    for tool, argv in ((ev, [root, "--ece_bins", "16"]), (ev, [root, "--calibration", "--ece_bins", "12"]),
                       (ev, [root, "--calibration", "--ece_bins", "512"]), (pr, [root, "--confidence_threshold", "0.5"]),
                       (pr, [root, "--confidence", "--confidence_threshold", "0"]),
                       (pr, [root, "--confidence", "--confidence_threshold", "1.5"]),
                       (pr, [root, "--confidence", "--dropout_draws", "4"]), (pr, [root, "--confidence", "--only_preprocess"]),
                       (pr, [root, "--calibration"]), (ev, [root, "--confidence"])):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2, argv
        assert "error:" in capsys.readouterr().err, argv
    assert len(seen) == n
    with pytest.raises(ValueError):
        ev.check_calibration_arguments(False, 16)
    with pytest.raises(ValueError):
        pr.check_confidence_arguments(True, None, 4)
