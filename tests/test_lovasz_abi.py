"""The Lovasz-Softmax loss of `evaluate --loss` without a GPU: the C ABI's symbols, workspace formula and argument checks,
metrics.lovasz_loss, hand-worked values of the host restatements (tests/helpers/lovasz_oracle.py), the CLI flag and the
CSV / summary layout."""
import os
import sys

import numpy as np
import pytest

from neuralbarkcalculator_amd import _lib, metrics
from neuralbarkcalculator_amd import evaluate as ev

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lovasz_oracle as lo  # noqa: E402


def _a256(x):
    return (x + 255) // 256 * 256


def _want_bytes(n, h, w):
    p, s = h * w, 3 * n
    t = (p + 8191) // 8192
    return 2 * _a256(4 * s * p) + _a256(1024 * s * t) + _a256(1024 * s) + _a256(4 * s * t) + _a256(8 * s * t) + _a256(4 * n)


def test_symbols_exist_and_workspace_formula_holds(built_lib):
    assert "nbc_lovasz_softmax" in _lib.SIGNATURES and "nbc_lovasz_workspace_bytes" in _lib.SIGNATURES
    for n, h, w in [(1, 1, 1), (1, 1, 7), (2, 33, 65), (3, 203, 317), (2, 520, 1024), (8, 1024, 1024), (1, 8192, 1),
                    (1, 8193, 1), (65535, 1, 1), (1, 46340, 46340)]:
        assert built_lib.nbc_lovasz_workspace_bytes(n, h, w) == _want_bytes(n, h, w), (n, h, w)
    for n, h, w in [(0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 32768)]:
        assert built_lib.nbc_lovasz_workspace_bytes(n, h, w) == 0, (n, h, w)


def test_every_invalid_argument_is_refused_before_the_device_is_touched(built_lib):
    """Fake but aligned device addresses: each call must return NBC_ERR_INVALID from its argument checks alone."""
    fake = 1 << 40
    n, h, w = 2, 16, 16
    need = built_lib.nbc_lovasz_workspace_bytes(n, h, w)

    def call(logits=fake, target=fake, N=n, H=h, W=w, ws=fake, ws_bytes=need, terms=fake, counts=fake):
        return built_lib.nbc_lovasz_softmax(logits, target, N, H, W, ws, ws_bytes, terms, counts, None)

    bad = [dict(logits=None), dict(target=None), dict(ws=None), dict(terms=None), dict(counts=None),
           dict(N=0), dict(N=-3), dict(N=65536), dict(H=0), dict(W=-1), dict(H=65536, W=32768),
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=fake + 8)]
    for kw in bad:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        assert _lib.last_error().startswith("nbc_lovasz_softmax:"), kw


def test_lovasz_loss_is_the_mean_over_present_classes():
    assert metrics.lovasz_loss([0.25, 0.0, 0.0], [10, 0, 0]) == 0.25
    assert metrics.lovasz_loss([0.25, 0.0, 0.5], [10, 0, 3]) == 0.375
    assert metrics.lovasz_loss([0.1, 0.2, 0.4], [1, 2, 3]) == (0.1 + 0.2 + 0.4) / 3
    assert metrics.lovasz_loss([0.0, 0.0, 0.0], [0, 0, 0]) == 0.0            # the reference's empty value
    assert np.isnan(metrics.lovasz_loss([np.nan, 0.0, np.nan], [4, 0, 5]))
    out = metrics.lovasz_loss([[0.25, 0.0, 0.5], [0.1, 0.3, 0.0]], [[1, 0, 1], [2, 2, 0]])
    assert out.dtype == np.float64 and out.tolist() == [0.375, 0.2]
    with pytest.raises(ValueError):
        metrics.lovasz_loss([0.1, 0.2], [1, 1])
    assert metrics.loss_cells([0.5, 0.0, 0.1], [3, 0, 1]) == [repr(0.5), "", repr(0.1), repr(0.3)]


def _logits_for(probs):
    """Logits whose float32 softmax is the given probabilities (to float32 rounding)."""
    return np.log(np.asarray(probs, dtype=np.float64)).astype(np.float32)


def test_one_pixel_image():
    """1 x 1: the present class has e = 1 - p, J_0 = 1, so its term and the loss are 1 - p_c."""
    logits = np.zeros((3, 1, 1), np.float32)
    for grey, c in ((0, 0), (128, 1), (255, 2)):
        g = np.full((1, 1), grey, np.uint8)
        for fn in (lo.terms_float64, lo.terms_torch_f32):
            terms, counts = fn(logits, g)
            assert counts.tolist() == [int(k == c) for k in range(3)]
            p = float(lo.softmax_f32(logits)[c, 0, 0])
            assert terms[c] == pytest.approx(1 - p, abs=1e-7)
            assert terms[c] == pytest.approx(2 / 3, abs=1e-7)
            assert [terms[k] for k in range(3) if k != c] == [0.0, 0.0]
            assert metrics.lovasz_loss(terms, counts) == pytest.approx(2 / 3, abs=1e-7)


def test_two_by_two_worked_by_hand():
    """Classes [[0,0],[1,1]].  Class 0: errors 0.9 (fg), 0.5 (fg), 0.2, 0.1, G = 2: J = 1/2, 1, 1, 1, term
    0.9/2 + 0.5/2 = 0.7.  Class 1: errors 0.6, 0.25 (bg), 0.5, 0.125 (fg): sorted 0.6, 0.5, 0.25, 0.125 with
    J = 1/3, 2/3, 3/4, 1, term 0.6/3 + 0.5/3 + 0.25/12 + 0.125/4 = 0.41875.  Class 2 absent: loss 0.559375."""
    p0 = np.array([[0.1, 0.5], [0.2, 0.1]])
    p1 = np.array([[0.6, 0.25], [0.5, 0.875]])
    probs = np.stack([p0, p1, 1 - p0 - p1])
    grey = np.array([[0, 40], [100, 191]], np.uint8)
    terms, counts = lo.terms_float64_from_probs(probs.astype(np.float32), lo.target_classes(grey))
    assert counts.tolist() == [2, 2, 0]
    np.testing.assert_allclose(terms, [0.7, 0.41875, 0.0], atol=1e-7)
    assert metrics.lovasz_loss(terms, counts) == pytest.approx(0.559375, abs=1e-7)
    for fn in (lo.terms_float64, lo.terms_torch_f32):
        t, c = fn(_logits_for(probs), grey)
        assert c.tolist() == [2, 2, 0]
        np.testing.assert_allclose(t, [0.7, 0.41875, 0.0], atol=1e-6)
    # saturated and wrong everywhere: every error 0 or 1, each present term 1
    logits = np.full((3, 2, 2), -80, np.float32)
    logits[2] = 80
    for fn in (lo.terms_float64, lo.terms_torch_f32):
        t, c = fn(logits, grey)
        assert t.tolist() == [1.0, 1.0, 0.0] and c.tolist() == [2, 2, 0]


def test_a_class_on_every_pixel_gives_the_mean_error():
    """G = P and no background: J_i = (i + 1) / P, so the term is the mean of 1 - p_c."""
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(3, 9, 11)).astype(np.float32)
    grey = np.full((9, 11), 150, np.uint8)
    p = lo.softmax_f32(logits)
    want = float(np.mean(1.0 - p[1].astype(np.float64)))
    for fn in (lo.terms_float64, lo.terms_torch_f32):
        t, c = fn(logits, grey)
        assert c.tolist() == [0, 99, 0]
        assert t[1] == pytest.approx(want, abs=1e-7) and t[0] == 0.0 and t[2] == 0.0


def test_ties_do_not_change_the_value():
    """Heavy ties (errors quantised to 8 levels, foreground and background mixed inside each run): every tie order gives
    the same float64 term."""
    rng = np.random.default_rng(11)
    h, w = 40, 50
    classes = rng.integers(0, 3, size=(h, w))
    q = rng.integers(0, 8, size=(3, h, w)).astype(np.float64) / 8
    probs = (q / np.maximum(q.sum(axis=0, keepdims=True), 1e-9)).astype(np.float32)
    ref, counts = lo.terms_float64_from_probs(probs, classes, "fg_first")
    assert (counts > 0).all()
    for tie in ("bg_first", "random"):
        t, c = lo.terms_float64_from_probs(probs, classes, tie)
        np.testing.assert_array_equal(c, counts)
        np.testing.assert_allclose(t, ref, rtol=0, atol=1e-12)
    # the float32 torch order breaks the same ties its own way: it lands on the float64 value of the same logits
    logits, grey = np.log(np.maximum(probs, 1e-30)).astype(np.float32), classes.astype(np.uint8) * 127
    np.testing.assert_allclose(lo.terms_torch_f32(logits, grey)[0], lo.terms_float64(logits, grey)[0], rtol=0, atol=1e-6)


def test_loss_flag_parses_and_reaches_the_folder_run(monkeypatch, tmp_path):
    seen = []

    def fake(root, model_path, precision, idx, **kw):
        seen.append((precision, kw))
        return {"rank": 0, "summary": {"images_evaluated": 0, "precision": precision, "model_path": model_path,
                                       "images_skipped": 0, "skipped": {}},
                "images_total": 0, "images_this_rank": 0, "batches": 0, "total_s": 0.0, "images_per_s_loop": 0.0}

    monkeypatch.setattr(ev, "evaluate_folder", fake)
    ev.main([str(tmp_path), "--loss", "--precision", "fp32"])
    ev.main([str(tmp_path), "--precision", "bf16"])
    ev.main([str(tmp_path), "--loss", "--bn_stats", "image"])
    assert seen[0] == ("fp32", dict(batch=None, streams=None, arch="auto", bn_stats="running", loss=True))
    assert seen[1] == ("bf16", dict(batch=None, streams=None, arch="auto", bn_stats="running"))
    assert seen[2][0] == "fp32" and seen[2][1]["loss"] is True and seen[2][1]["bn_stats"] == "image"


def test_loss_with_exclude_nodes_is_still_refused():
    with pytest.raises(SystemExit) as e:
        ev.main(["/nonexistent", "--loss", "--exclude_nodes"])
    assert "--exclude_nodes" in str(e.value)


def test_csv_header_with_and_without_loss(tmp_path):
    assert ev.csv_header() == metrics.EVAL_CSV_HEADER and len(ev.csv_header()) == 15
    assert ev.csv_header(loss=True) == metrics.EVAL_CSV_HEADER + ["loss_nothing", "loss_bark", "loss_node", "lovasz_softmax"]
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}, {"name": "c.png", "wood": "sapin"}]
    raw_a = np.array([[3, 1, 0], [0, 4, 0], [0, 0, 0]], np.int64)         # node absent
    raw_c = np.array([[1, 0, 0], [0, 2, 0], [0, 1, 6]], np.int64)
    allrows = np.stack([np.concatenate([[0, 2, 4, ev.STATUS_OK], raw_a.ravel(), raw_a.ravel()]),
                        np.concatenate([[1, 4, 4, ev.STATUS_NO_DUAL], np.zeros(18, np.int64)]),
                        np.concatenate([[2, 2, 5, ev.STATUS_OK], raw_c.ravel(), raw_c.ravel()])])
    terms = np.array([[0.25, 0.5, 0.0], [0.0, 0.0, 0.0], [0.125, 0.375, 0.0625]])
    loss_rows = np.concatenate([np.arange(3)[:, None], terms.view(np.int64)], axis=1)
    rows, summary = ev.report(items, allrows, "fp32", "m.pt", loss_rows=loss_rows)
    assert rows[0] == metrics.eval_row("a.png", "sapin", raw_a, raw_a) + ["0.25", "0.5", "", "0.375"]
    assert rows[1][-4:] == ["0.125", "0.375", "0.0625", repr((0.125 + 0.375 + 0.0625) / 3)]
    ls = summary["lovasz_softmax"]
    assert ls["mean_over_images"] == pytest.approx((0.375 + (0.125 + 0.375 + 0.0625) / 3) / 2)
    assert ls["per_class_mean"] == {"nothing": 0.1875, "bark": 0.4375, "node": 0.0625}
    assert "lovasz_softmax loss: mean over images" in ev.format_summary(summary)
    path = os.path.join(str(tmp_path), "with.csv")
    ev.write_stats_csv(path, rows, loss=True)
    assert open(path).read().splitlines()[0].split("\t") == ev.csv_header(loss=True)
    # without the loss: the 15 columns and no summary key, as before
    rows0, summary0 = ev.report(items, allrows, "fp32", "m.pt")
    assert rows0 == [r[:15] for r in rows] and "lovasz_softmax" not in summary0
    assert "lovasz_softmax" not in ev.format_summary(summary0)
    ev.write_stats_csv(path, rows0)
    assert open(path).read().splitlines()[0].split("\t") == metrics.EVAL_CSV_HEADER
