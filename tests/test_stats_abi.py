"""Dataset statistics without a device: what nbc_image_moments / nbc_target_counts refuse, the host arithmetic of
neuralbarkcalculator_amd/stats.py against an independent exact truth and against the reference's procedure restated in torch,
and the --mean / --std / --stats options of the predict and evaluate drivers."""
import ctypes as C
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib, folder_run, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd import stats as st


# ---- 1. the entry points' argument checks ----------------------------------------------------------------------------
@pytest.mark.parametrize("symbol", ["nbc_image_moments", "nbc_target_counts"])
def test_entry_points_refuse_bad_arguments_without_a_device(built_lib, symbol):
    assert symbol in _lib.SIGNATURES
    fn = getattr(built_lib, symbol)
    buf = (C.c_uint8 * 64)()
    out = (C.c_uint64 * 16)()
    p, o = C.addressof(buf), C.addressof(out)
    bad = [(None, 1, 2, 2, o), (p, 1, 2, 2, None), (p, 0, 2, 2, o), (p, -1, 2, 2, o), (p, 65536, 2, 2, o), (p, 1, 0, 2, o),
           (p, 1, 2, 0, o), (p, 1, -3, 2, o), (p, 1, 65536, 32768, o), (p, 1, 2 ** 31 - 1, 2, o)]
    for x, n, h, w, dst in bad:
        assert fn(x, n, h, w, dst, None) == _lib.NBC_ERR_INVALID, (n, h, w)
        msg = _lib.last_error()
        assert msg.startswith(symbol + ": ") and len(msg) > len(symbol) + 2
    assert "2^31" in msg                             # the last case: H * W = 2^32 - 2


# ---- 2. host arithmetic against an exact truth -----------------------------------------------------------------------
def _moments(img):
    """numpy uint64 sums: [3][2]."""
    v = img.reshape(-1, 3).astype(np.uint64)
    return [[int(v[:, c].sum()), int((v[:, c] * v[:, c]).sum())] for c in range(3)]


def _truth_mean_std(img):
    """Per channel: float(Fraction) of the exact mean, sqrt of float(Fraction) of the exact unbiased variance."""
    p = img.shape[0] * img.shape[1]
    mean, std = [], []
    for s1, s2 in _moments(img):
        mean.append(float(Fraction(s1, 255 * p)))
        std.append(math.sqrt(float(Fraction(p * s2 - s1 * s1, p * (p - 1) * 65025))) if p > 1 else math.nan)
    return mean, std


SHAPES = [(1024, 1024), (611, 1024), (64, 48), (1, 7), (203, 317)]


def _frames():
    return [synth.make_frame(20 + i, h, w) for i, (h, w) in enumerate(SHAPES)]


def test_per_image_mean_and_std_equal_the_exact_rationals_to_the_bit():
    rng = np.random.default_rng(1)
    extra = [rng.integers(0, 256, size=(37, 41, 3), dtype=np.uint8), np.full((16, 16, 3), 255, np.uint8),
             np.zeros((5, 3, 3), np.uint8), np.full((4096, 4096, 3), 255, np.uint8)[:1]]
    for img in _frames() + extra:
        h, w = img.shape[:2]
        mean, std = st.image_mean_std(h, w, _moments(img))
        want_mean, want_std = _truth_mean_std(img)
        assert mean == want_mean and std == want_std, (h, w)
    # the largest sums a real folder produces: one all-255 4096 x 4096 frame, as integers
    p = 4096 * 4096
    mean, std = st.image_mean_std(4096, 4096, [[255 * p, 65025 * p]] * 3)
    assert mean == [1.0] * 3 and std == [0.0] * 3
    mean, std = st.image_mean_std(1, 1, [[9, 81]] * 3)
    assert mean == [9 / 255] * 3 and all(math.isnan(v) for v in std)      # torch.std of one value


def _rows(frames, greys, statuses):
    rows = []
    for i, (img, g, s) in enumerate(zip(frames, greys, statuses)):
        cnt = [0, 0, 0, 0]
        if s == st.STATUS_OK:
            cls = metrics.target_classes(g)
            cnt = [int((cls == y).sum()) for y in range(3)] + [int(((g != 0) & (g != 127) & (g != 255)).sum())]
        rows.append([i, img.shape[0], img.shape[1], s] + [v for pair in _moments(img) for v in pair] + cnt)
    return np.asarray(rows, dtype=np.int64)


def test_dataset_values_class_counts_and_pos_weight():
    frames = _frames()
    rng = np.random.default_rng(2)
    greys = [rng.choice(np.array([0, 127, 255, 3, 130], np.uint8), size=f.shape[:2], p=[0.6, 0.25, 0.1, 0.03, 0.02]) for f in frames]
    statuses = [st.STATUS_OK, st.STATUS_NO_DUAL, st.STATUS_OK, st.STATUS_SHAPE_MISMATCH, st.STATUS_OK]
    items = [{"name": "f%d.png" % i, "wood": "sapin"} for i in range(len(frames))]
    rows = _rows(frames, greys, statuses)
    csv_rows, summary = st.report(items, rows)
    per = [_truth_mean_std(f) for f in frames]
    for c in range(3):                               # every image weighs the same, with or without a dual
        assert summary["mean"][c] == math.fsum(m[c] for m, _ in per) / len(per)
        want = math.fsum(s[c] for _, s in per) / len(per)
        assert summary["std"][c] == want or (math.isnan(want) and math.isnan(summary["std"][c]))
    ok = [i for i, s in enumerate(statuses) if s == st.STATUS_OK]
    counts = [sum(int((metrics.target_classes(greys[i]) == y).sum()) for i in ok) for y in range(3)]
    assert summary["class_counts"] == counts and sum(counts) == sum(frames[i].shape[0] * frames[i].shape[1] for i in ok)
    assert summary["pos_weight"] == [sum(counts) / (3 * c) for c in counts]
    assert summary["off_level_pixels"] == sum(int(np.isin(greys[i], [3, 130]).sum()) for i in ok) > 0
    assert summary["images"] == 5 and summary["images_with_dual"] == 3
    assert summary["skipped"] == {"no_dual": ["sapin/f1.png"], "shape_mismatch": ["sapin/f3.png"]}
    assert [r[:4] for r in csv_rows] == [["f%d.png" % i, "sapin", str(f.shape[0]), str(f.shape[1])] for i, f in enumerate(frames)]
    assert csv_rows[0][4:10] == [repr(v) for v in per[0][0] + per[0][1]] and csv_rows[1][10:] == ["", "", "", ""]
    assert int(csv_rows[0][11]) + int(csv_rows[0][12]) == int((metrics.target_classes(greys[0]) != 0).sum())   # sample_weight
    # the order of the rows (the ranks' shards) changes nothing
    for perm in (rows[::-1], rows[[2, 0, 4, 1, 3]]):
        again_rows, again = st.report(items, perm)
        assert json.dumps(again) == json.dumps(summary) and again_rows == csv_rows


def test_a_class_without_a_pixel_has_no_weight():
    assert st.pos_weight([10, 5, 0]) == [15 / 30, 15 / 15, None]
    assert st.pos_weight([0, 0, 0]) == [None, None, None]
    frames = _frames()[2:3]
    rows = _rows(frames, [np.zeros(frames[0].shape[:2], np.uint8)], [st.STATUS_OK])
    _, summary = st.report([{"name": "a.png", "wood": "sapin"}], rows)
    assert summary["class_counts"] == [64 * 48, 0, 0] and summary["pos_weight"] == [1 / 3, None, None]
    assert json.loads(json.dumps(summary))["pos_weight"] == [1 / 3, None, None]


# ---- 3. the reference's procedure, restated in torch on the CPU ------------------------------------------------------
def test_dataset_mean_std_against_the_float32_procedure_of_the_reference():
    """utils.py:23-39 on the frames synth.make_frame(20 + i, h, w) of SHAPES, the frames the bound was derived on: ToTensor
    (float32 / 255, CHW), .view(1, 3, -1), .mean(2), .std(2), summed over the images and divided by their number, all in
    float32.  That procedure lies within 1.53e-7 (mean) and 7.8e-8 (std) of the exact value on these shapes; the bound of
    1e-6 is about 6x that and 17 float32 ulps.  It ties the semantics (per-image, unbiased, unweighted) to the reference;
    the precision criterion is the exact test above."""
    frames = [f for f in _frames() if f.shape[0] * f.shape[1] > 1]
    mean = torch.zeros(3)
    std = torch.zeros(3)
    for f in frames:
        data = (torch.from_numpy(f).permute(2, 0, 1).contiguous().to(torch.float32) / 255)[None]
        data = data.view(1, 3, -1)
        mean += data.mean(2).sum(0)
        std += data.std(2).sum(0)
    mean /= len(frames)
    std /= len(frames)
    items = [{"name": "f%d" % i, "wood": "sapin"} for i in range(len(frames))]
    _, summary = st.report(items, _rows(frames, [None] * len(frames), [st.STATUS_NO_DUAL] * len(frames)))
    for c in range(3):
        rel_m = abs(float(mean[c]) - summary["mean"][c]) / summary["mean"][c]
        rel_s = abs(float(std[c]) - summary["std"][c]) / summary["std"][c]
        print("channel %d: relative difference mean %.3g, std %.3g" % (c, rel_m, rel_s))
        assert rel_m <= 1e-6 and rel_s <= 1e-6


# ---- 4. the options ---------------------------------------------------------------------------------------------------
def test_resolve_normalization():
    assert folder_run.resolve_normalization() is None
    pair = folder_run.resolve_normalization([0.7, 0.6, 0.4], [0.1, 0.2, 0.3])
    assert pair == ((0.7, 0.6, 0.4), (0.1, 0.2, 0.3))
    for mean, std in (([0.7, 0.6, 0.4], None), (None, [0.1, 0.2, 0.3]), ([0.7, 0.6, 0.4], [0.1, 0.0, 0.3]),
                      ([0.7, 0.6, 0.4], [0.1, -0.2, 0.3]), ([0.7, 0.6, 0.4], [0.1, math.nan, 0.3]),
                      ([0.7, 0.6, 0.4], [0.1, math.inf, 0.3]), ([0.7, math.nan, 0.4], [0.1, 0.2, 0.3]),
                      ([0.7, math.inf, 0.4], [0.1, 0.2, 0.3]), ([0.7, 0.6], [0.1, 0.2, 0.3])):
        with pytest.raises(ValueError):
            folder_run.resolve_normalization(mean, std)


def _stats_file(tmp_path, doc, name="s.json"):
    path = tmp_path / name
    path.write_text(doc if isinstance(doc, str) else json.dumps(doc))
    return str(path)


@pytest.mark.parametrize("main", [ev.main, drv.main])
def test_bad_normalization_options_are_argument_errors(main, tmp_path, capsys):
    good = _stats_file(tmp_path, {"mean": [0.5, 0.5, 0.5], "std": [0.1, 0.1, 0.1]})
    no_std = _stats_file(tmp_path, {"mean": [0.5, 0.5, 0.5]}, "no_std.json")
    not_json = _stats_file(tmp_path, "mean = 3", "bad.json")
    nan_std = _stats_file(tmp_path, '{"mean": [0.5, 0.5, 0.5], "std": [0.1, NaN, 0.1]}', "nan.json")
    for extra in (["--mean", "0.5", "0.5", "0.5"], ["--std", "0.1", "0.1", "0.1"],
                  ["--stats", good, "--mean", "0.5", "0.5", "0.5", "--std", "0.1", "0.1", "0.1"],
                  ["--stats", good, "--mean", "0.5", "0.5", "0.5"],
                  ["--mean", "0.5", "0.5", "0.5", "--std", "0.1", "0", "0.1"],
                  ["--mean", "0.5", "0.5", "0.5", "--std", "0.1", "-0.1", "0.1"],
                  ["--mean", "0.5", "0.5", "0.5", "--std", "0.1", "nan", "0.1"],
                  ["--mean", "0.5", "inf", "0.5", "--std", "0.1", "0.1", "0.1"],
                  ["--mean", "0.5", "0.5", "--std", "0.1", "0.1", "0.1"],
                  ["--stats", no_std], ["--stats", not_json], ["--stats", nan_std], ["--stats", str(tmp_path / "missing.json")]):
        with pytest.raises(SystemExit) as e:
            main([str(tmp_path)] + extra)
        assert e.value.code == 2, extra               # argparse's error exit
        assert "error:" in capsys.readouterr().err


def _fake_stats(precision, model_path="m"):
    return {"rank": 0, "summary": {"images_evaluated": 0, "precision": precision, "model_path": model_path,
                                   "images_skipped": 0, "skipped": {}},
            "images_total": 0, "images_this_rank": 0, "batches": 0, "total_s": 0.0, "images_per_s_loop": 0.0}


def test_evaluate_main_hands_normalization_on_only_when_given(monkeypatch, tmp_path):
    seen = []
    monkeypatch.setattr(ev, "evaluate_folder", lambda root, model_path, precision, idx, **kw: (
        seen.append(kw), _fake_stats(precision))[1])
    base = dict(batch=None, streams=None, arch="auto", bn_stats="running")
    ev.main([str(tmp_path), "--precision", "fp32"])
    assert seen[-1] == base
    ev.main([str(tmp_path), "--precision", "fp32", "--mean", "0.7", "0.6", "0.4", "--std", "0.1", "0.2", "0.3"])
    assert seen[-1] == dict(base, normalization=((0.7, 0.6, 0.4), (0.1, 0.2, 0.3)))
    # a file as stats.py writes it: the pair read back is the pair written, bit for bit
    frames = _frames()[2:]
    _, summary = st.report([{"name": "f%d" % i, "wood": "sapin"} for i in range(len(frames))],
                           _rows(frames, [None] * len(frames), [st.STATUS_NO_DUAL] * len(frames)))
    path = str(tmp_path / "dataset_stats.json")
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)
    ev.main([str(tmp_path), "--precision", "fp32", "--loss", "--stats", path])
    assert seen[-1] == dict(base, loss=True, normalization=(tuple(summary["mean"]), tuple(summary["std"])),
                            normalization_source=path)


def test_predict_main_hands_normalization_on_only_when_given(monkeypatch, tmp_path, capsys):
    seen = []

    def fake(root, model_path, precision, *args, **kw):
        seen.append(kw)
        return dict(_fake_stats(precision), rank=0)
    monkeypatch.setattr(drv, "predict_folder", fake)
    base = dict(batch=None, autotune=False, streams=None, arch="auto", bn_stats="running")
    drv.main([str(tmp_path), "--precision", "fp32"])
    assert seen[-1] == base and "normalised" not in capsys.readouterr().out
    path = _stats_file(tmp_path, {"mean": [0.71, 0.62, 0.43], "std": [0.11, 0.12, 0.13], "images": 3})
    drv.main([str(tmp_path), "--precision", "fp32", "--stats", path])
    assert seen[-1] == dict(base, normalization=((0.71, 0.62, 0.43), (0.11, 0.12, 0.13)))
    out = capsys.readouterr().out
    assert "mean [0.71, 0.62, 0.43], std [0.11, 0.12, 0.13]" in out and path in out


def test_summary_names_the_pair_only_when_given():
    items = [{"name": "a.png", "wood": "sapin"}]
    conf = np.array([[3, 1, 0], [0, 4, 0], [0, 1, 7]], np.int64)
    allrows = np.concatenate([[0, 4, 4, ev.STATUS_OK], conf.ravel(), conf.ravel()])[None]
    _, plain = ev.report(items, allrows, "fp32", "m.pt")
    assert "normalization" not in plain
    pair = ((0.7, 0.6, 0.4), (0.1, 0.2, 0.3))
    _, named = ev.report(items, allrows, "fp32", "m.pt", normalization=pair, normalization_source="x.json")
    assert named["normalization"] == {"mean": [0.7, 0.6, 0.4], "std": [0.1, 0.2, 0.3], "source": "x.json"}
    assert {k: v for k, v in named.items() if k != "normalization"} == plain
    assert "mean [0.7, 0.6, 0.4], std [0.1, 0.2, 0.3] (x.json)" in ev.format_summary(named)
    assert ev.format_summary(plain) in ev.format_summary(named).replace(
        "\nnormalised with mean [0.7, 0.6, 0.4], std [0.1, 0.2, 0.3] (x.json)", "")


def test_wrappers_validate_before_the_library(built_lib):
    for fn, good in ((st.image_moments, torch.zeros((2, 4, 4, 3), dtype=torch.uint8)),
                     (st.target_counts, torch.zeros((2, 4, 4), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            fn(good)                                 # on the host
        with pytest.raises(ValueError):
            fn(good.numpy())
