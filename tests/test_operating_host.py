"""The host side of the operating-point sweep without a GPU: operating.sweep_cpu against a scalar transcription of argmax3,
the facts that follow from the definition, figures / select / parse_grid, and what the drivers refuse."""
import math

import numpy as np
import pytest

from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import folder_run, metrics
from neuralbarkcalculator_amd import operating as op
from neuralbarkcalculator_amd import predict as pr

GRID = op.parse_grid(op.DEFAULT_GRID)


def _argmax3(a, b, c):
    """reduce.hpp's argmax3, line for line, on Python floats that hold float32 values."""
    best, bv = 0, a
    if (b > bv) or (b != b and bv == bv):
        best, bv = 1, b
    if (c > bv) or (c != c and bv == bv):
        best, bv = 2, c
    return best


def _crafted():
    """5 x 7 logits from multiples of 0.5 in [-8, 8] with NaN and +-inf pixels, and a grey mask over all three classes."""
    rng = np.random.default_rng(5)
    logits = (rng.integers(-16, 17, size=(3, 5, 7)) * 0.5).astype(np.float32)
    logits[:, 0, 0] = (np.nan, 0.0, 0.0)
    logits[:, 0, 1] = (0.0, np.nan, 0.5)
    logits[:, 0, 2] = (0.0, 1.0, np.nan)
    logits[:, 1, 3] = (np.nan, np.nan, np.nan)
    logits[:, 2, 4] = (np.inf, 0.0, 0.0)
    logits[:, 3, 5] = (0.0, -np.inf, np.inf)
    logits[:, 4, 6] = (-np.inf, -np.inf, -np.inf)
    logits[:, 4, 0] = (1.0, np.nan, np.inf)
    logits[:, 2, 2] = (2.0, 2.0, 2.0)
    grey = np.array([10, 100, 200, 63, 64, 191, 192], np.uint8)[rng.integers(0, 7, size=(5, 7))]
    return logits, grey


def test_sweep_cpu_equals_the_scalar_transcription():
    logits, grey = _crafted()
    got = op.sweep_cpu(logits, grey, GRID, GRID)
    want = np.zeros((33, 33, 3, 3), np.int64)
    t = metrics.target_classes(grey)
    ties = 0
    for i, b1 in enumerate(GRID):
        for j, b2 in enumerate(GRID):
            for y in range(5):
                for x in range(7):
                    a = float(logits[0, y, x])
                    with np.errstate(invalid="ignore"):
                        b, c = float(np.float32(logits[1, y, x]) + np.float32(b1)), float(np.float32(logits[2, y, x]) + np.float32(b2))
                    ties += c == a or c == b or b == a
                    want[i, j, t[y, x], _argmax3(a, b, c)] += 1
    assert ties > 500                                           # exact ties occur at many grid points
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (got.sum(axis=(2, 3)) == 35).all()                   # non-finite pixels decide like any other
    # the (0, 0) point is the confusion of numpy's argmax (first maximum, NaN as the maximum)
    plain = metrics.confusion_numpy(np.argmax(logits, axis=0), t)
    assert np.array_equal(got[16, 16], plain) and GRID[16] == 0
    # along j a pixel leaves for class 2 once and never returns: the counts decided as 2 only grow, the others only shrink
    assert (np.diff(got[:, :, :, 2], axis=1) >= 0).all() and (np.diff(got[:, :, :, :2], axis=1) <= 0).all()
    batch = op.sweep_cpu(np.stack([logits, logits[:, ::-1]]), np.stack([grey, grey[::-1]]), GRID[:3], GRID[30:])
    assert batch.shape == (2, 3, 3, 3, 3) and np.array_equal(batch[0], got[:3, 30:]) and np.array_equal(batch[1], got[:3, 30:])


def test_decide_cpu_uses_float32_additions():
    x = np.zeros((3, 1, 2), np.float32)
    x[0] = 1.0
    x[2, 0, 0] = np.float32(1.0) - np.float32(2.0 ** -24)       # + 2^-26 rounds back to itself in f32: still below x0 = 1
    x[2, 0, 1] = 16777216.0                                      # 2^24 + 1 rounds to 2^24 in f32: a tie with x0 = 2^24, class 0
    x[0, 0, 1] = 16777216.0                                      # wins (in f64 the sum would exceed x0 and class 2 would win)
    assert op.decide_cpu(x, 0.0, 2.0 ** -26).tolist() == [[0, 0]]
    assert op.decide_cpu(x, 0.0, 1.0).tolist() == [[2, 0]]
    assert op.decide_cpu(x, 0.0, 2.0).tolist() == [[2, 2]]


def test_figures_at_the_origin_are_the_metrics_of_the_confusion():
    logits, grey = _crafted()
    table = op.sweep_cpu(logits, grey, GRID, GRID)
    f = op.figures(table)
    conf = table[16, 16]
    assert np.array_equal(f["iou"][16, 16], metrics.iou(conf)) and np.array_equal(f["f1"][16, 16], metrics.f1(conf))
    assert f["miou"][16, 16] == metrics.iou(conf).mean() and f["f1_mean"][16, 16] == metrics.f1(conf).mean()
    assert f["out_bark"][16, 16] == conf[:, 1].sum() and f["tgt_node"][3, 4] == conf[2].sum() and (f["pixels"] == 35).all()
    assert f["out_node_percent"][16, 16] == 100.0 * conf[:, 2].sum() / 35 and f["tgt_bark_percent"][0, 0] == 100.0 * conf[1].sum() / 35
    row = op.point_row(conf, 0.0, 0.0)
    assert row[:2] == ["0.0", "0.0"] and row[2:5] == ["%.6f" % v for v in metrics.iou(conf)] and len(row) == len(op.POINTS_COLUMNS)
    assert row[-4:] == [metrics.percent(int(conf[:, 1].sum()), 35), metrics.percent(int(conf[:, 2].sum()), 35),
                        metrics.percent(int(conf[1].sum()), 35), metrics.percent(int(conf[2].sum()), 35)]


def _table(g1, g2, fill):
    """A table whose every point is the perfect confusion diag(fill), to be spoiled point by point."""
    t = np.zeros((g1, g2, 3, 3), np.int64)
    t[:, :, range(3), range(3)] = fill
    return t


def test_select_tie_rules_and_edges():
    b = np.array([-2, -1, 0, 1, 2], np.float32)
    worse = _table(5, 5, 10)
    worse[:, :, 0, 1] += 5                                       # every point equally imperfect ...
    t = worse.copy()
    for i, j in ((0, 4), (1, 2), (3, 2), (2, 1)):                # ... except four perfect ones
        t[i, j] = _table(1, 1, 10)[0, 0]
    s = op.select(t, b, b)
    # |b1| + |b2|: (0,4) 4, (1,2) 1, (3,2) 1, (2,1) 1 -> the smallest i among the three: (1, 2)
    for name in ("best_miou", "best_f1", "area_unbiased"):
        assert (s[name]["i"], s[name]["j"]) == (1, 2) and not s[name]["on_edge"], name
        assert (s[name]["bark_offset"], s[name]["node_offset"]) == (-1.0, 0.0)
    assert (s["argmax"]["i"], s["argmax"]["j"]) == (2, 2) and list(s) == op.POINT_NAMES
    t[1, 2] = worse[1, 2]                                        # then the smallest i of (3,2), (2,1): (2, 1)
    assert (op.select(t, b, b)["best_miou"]["i"], op.select(t, b, b)["best_miou"]["j"]) == (2, 1)
    t[2, 1] = worse[2, 1]
    t[3, 2] = worse[3, 2]
    s = op.select(t, b, b)
    assert (s["best_miou"]["i"], s["best_miou"]["j"]) == (0, 4) and s["best_miou"]["on_edge"]
    # same i, same distance: the smallest j
    t = worse.copy()
    t[2, 1] = t[2, 3] = _table(1, 1, 10)[0, 0]
    assert op.select(t, b, b)["best_f1"]["j"] == 1
    # the node F1 alone, and the area rule in pixels (a point may trade node for bark pixel for pixel)
    t = worse.copy()
    t[:, :, 2, 2], t[:, :, 2, 0] = 9, 1                          # a node pixel lost everywhere ...
    t[4, 0, 2, 2], t[4, 0, 2, 0] = 10, 0                         # ... but here, where bark is no better than elsewhere
    s = op.select(t, b, b)
    assert (s["best_node_f1"]["i"], s["best_node_f1"]["j"]) == (4, 0) and s["best_node_f1"]["on_edge"]
    t = worse.copy()                                             # every point puts 5 pixels too many on bark ...
    t[3, 3, 0, 1], t[3, 3, 0, 0] = 2, 13                         # ... this one only 2
    s = op.select(t, b, b)
    assert (s["area_unbiased"]["i"], s["area_unbiased"]["j"]) == (3, 3)
    # a grid without the origin has no argmax point; an axis of one value has no edge
    s = op.select(worse[:, :1], b, np.array([0.5], np.float32))
    assert "argmax" not in s and not s["best_miou"]["on_edge"] and s["best_miou"]["i"] == 2
    assert op.select(worse[:1, :1], [0.0], [0.0])["argmax"]["on_edge"] is False
    with pytest.raises(ValueError):
        op.select(worse, b[:4], b)


def test_parse_grid_values_and_refusals():
    g = op.parse_grid("-8:8:0.5")
    assert g.dtype == np.float32 and g.size == 33 and g[0] == -8 and g[16] == 0 and g[32] == 8 and (np.diff(g) == 0.5).all()
    assert op.parse_grid("0:0:1").tolist() == [0.0] and op.parse_grid("-1:1:0.1").size == 21 and op.parse_grid("0:1:0.3").size == 4
    for bad in ("-8:8.5:0.5", "0:1:0", "0:1:-1", "nan:1:1", "0:inf:1", "0:1:nan", "1:0:1", "0:1", "0:1:1:1", "a:b:c", "", "0:1e-30:1e-40"):
        with pytest.raises(ValueError):
            op.parse_grid(bad)
    for bad in ([], [0.0] * 2, [1.0, 0.0], [0.0, np.nan], [np.inf], list(range(34)), [0.0, 1e-46]):
        with pytest.raises(ValueError):
            op.check_offsets(bad)
    assert op.TABLE_BYTES_DEFAULT == 78408


def test_summary_entry_and_files(tmp_path):
    logits, grey = _crafted()
    t1 = op.sweep_cpu(logits, grey, GRID, GRID)
    t2 = op.sweep_cpu(logits[:, ::-1], grey, GRID, GRID)
    entry = op.write_report(str(tmp_path), [("a.png", "sapin", t1), ("b.png", "sapin", t2)], GRID, GRID, (1.5, -2.0))
    assert entry["bark_offsets"] == GRID.tolist() and entry["run_logit_offsets"] == [1.5, -2.0] and "raw argmax" in entry["note"]
    pooled = t1 + t2
    for name, p in entry["points"].items():
        assert p["confusion"] == pooled[p["i"], p["j"]].tolist()
        assert p["arguments"] == "--logit_offsets %r %r" % (p["bark_offset"], p["node_offset"])
        assert p["figures"]["miou"] == float(metrics.iou(pooled[p["i"], p["j"]]).mean())
    rows = [r.split("\t") for r in open(tmp_path / op.POINTS_CSV).read().splitlines()]
    assert rows[0] == op.POINTS_COLUMNS and len(rows) == 1 + 33 * 33
    assert rows[1 + 16 * 33 + 16] == op.point_row(pooled[16, 16], 0.0, 0.0)
    per = [r.split("\t") for r in open(tmp_path / op.EVALUATION_CSV).read().splitlines()]
    assert per[0] == op.evaluation_columns(entry["points"]) and len(per) == 3 and len(per[0]) == 2 + 3 * 4 + 2
    assert per[1][2] == "%.6f" % metrics.iou(t1[16, 16]).mean() and per[2][0] == "b.png"
    import json
    json.dumps(entry)


def test_the_drivers_refuse_before_any_device():
    assert op.check_arguments(False) is None
    b1, b2 = op.check_arguments(True)
    assert b1.tolist() == GRID.tolist() == b2.tolist()
    b1, b2 = op.check_arguments(True, "-1:1:1", [0.0, 0.25])
    assert b1.tolist() == [-1, 0, 1] and b2.tolist() == [0, 0.25]
    for kw in (dict(bark_offsets="-1:1:1"), dict(node_offsets="0:0:1")):
        with pytest.raises(ValueError, match="needs --operating_points"):
            op.check_arguments(False, **kw)
    with pytest.raises(ValueError):
        op.check_arguments(True, "0:100:1")
    assert folder_run.check_logit_offsets(None) is None
    assert folder_run.check_logit_offsets([0.1, -5.5]) == (float(np.float32(0.1)), -5.5)
    for bad in ([1.0], [1.0, 2.0, 3.0], [math.nan, 0.0], [0.0, math.inf], ["a", 1.0]):
        with pytest.raises(ValueError):
            folder_run.check_logit_offsets(bad)
    with pytest.raises(ValueError, match="dropout_draws"):
        folder_run.check_logit_offsets([1.0, 2.0], dropout_draws=4)
    with pytest.raises(ValueError, match="confidence"):
        folder_run.check_logit_offsets([1.0, 2.0], confidence=True)
    # the folder functions refuse before they open a run (the root does not exist: nothing else could have raised ValueError)
    with pytest.raises(ValueError, match="needs --operating_points"):
        ev.evaluate_folder("/nonexistent-root", bark_offsets="-1:1:1")
    with pytest.raises(ValueError):
        ev.evaluate_folder("/nonexistent-root", logit_offsets=(math.nan, 0.0))
    with pytest.raises(ValueError, match="dropout_draws"):
        pr.predict_folder("/nonexistent-root", logit_offsets=(1.0, 2.0), dropout_draws=2)
    with pytest.raises(ValueError, match="confidence"):
        pr.predict_folder("/nonexistent-root", logit_offsets=(1.0, 2.0), confidence=True)


@pytest.mark.parametrize("argv", [["ROOT", "--bark_offsets", "-1:1:1"], ["ROOT", "--node_offsets", "-1:1:1"],
                                  ["ROOT", "--operating_points", "--bark_offsets", "0:100:1"],
                                  ["ROOT", "--logit_offsets", "nan", "0"], ["ROOT", "--logit_offsets", "1"]])
def test_evaluate_command_line_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        ev.main(argv)
    assert e.value.code == 2 and "error" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["ROOT", "--logit_offsets", "1", "2", "--dropout_draws", "4"],
                                  ["ROOT", "--logit_offsets", "1", "2", "--confidence"], ["ROOT", "--logit_offsets", "inf", "2"]])
def test_predict_command_line_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        pr.main(argv)
    assert e.value.code == 2 and "error" in capsys.readouterr().err
