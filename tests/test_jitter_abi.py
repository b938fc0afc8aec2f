"""The colour-jitter views (`--jitter`) without a GPU: the C ABI's symbols, signatures and constants, every refusal in front of
the device, the numpy restatement of tests/helpers/jitter_oracle.py against PIL's ImageEnhance and plain Python, the report
arithmetic and the command line's refusals."""
import csv
import ctypes as C
import json
import os
import re
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from neuralbarkcalculator_amd import _lib, folder_run, metrics
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd import predict as drv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import jitter_oracle as jo  # noqa: E402
import vote_oracle as vo  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40


def test_symbols_signatures_and_constants(built_lib):
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for name in ("nbc_jitter_workspace_bytes", "nbc_jitter_views", "nbc_views_mean"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name) and ("int %s(" % name) in header
    assert _lib.SIGNATURES["nbc_jitter_workspace_bytes"] == (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)])
    assert _lib.SIGNATURES["nbc_jitter_views"] == (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 3)
    assert _lib.SIGNATURES["nbc_views_mean"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 2)
    flat = re.sub(r"\s+", " ", header)
    assert "int nbc_jitter_workspace_bytes(int N, int V, size_t* bytes);" in flat
    assert ("int nbc_jitter_views(const uint8_t* x_dev, int N, int H, int W, const float* factors, int V, uint8_t* out_dev, "
            "void* workspace_dev, void* hip_stream);") in flat
    assert "int nbc_views_mean(const float* lowres_views_dev, int N, int V, int h, int w, float* mean_dev, void* hip_stream);" in flat
    for text in ("(19595 R + 38470 G + 7471 B + 32768) >> 16", "m = floor((2 S + H W) / (2 H W))", "t = float(d) + f * float(i - d)",
                 "saturation_s(contrast_c(brightness_b(frame)))", "torchvision shuffles the order per sample"):
        assert text in flat, text
    assert re.search(r"NBC_JITTER_MAX_VIEWS = 16\b", header) and _lib.JITTER_MAX_VIEWS == 16
    # the named set: the star of the training's amplitudes, identity first, as the float32 nearest to the decimals
    want = np.array(jo.TRAINING, dtype=np.float32)
    assert mdl.JITTER_TRAINING == jo.TRAINING and np.array_equal(mdl.resolve_jitter_views("training"), want)
    assert mdl.resolve_jitter_views("training").dtype == np.float32 and mdl.resolve_jitter_views(jo.TRAINING).shape == (5, 3)
    assert mdl.jitter_view_names("training") == folder_run.jitter_view_names(want) == jo.TRAINING_NAMES
    assert mdl.jitter_view_names([(1, 1, 1), (0.95, 1.05, 1), (1, 2, 0), (1.37, 0.5, 1.2)]) == ["identity", "b0.95_c1.05", "c2_s0",
                                                                                                "b1.37_c0.5_s1.2"]
    assert np.array_equal(mdl.resolve_jitter_views([[0, 4, 1]]), np.array([[0, 4, 1]], dtype=np.float32))
    assert mdl.resolve_jitter_views([(1, 1, 1)] * 16).shape == (16, 3)
    for bad in ("flips", "none", None, 5, 1.5, [], [(1, 1)], [(1, 1, 1, 1)], [(1, 1, -0.1)], [(1, 4.5, 1)], [(1, float("nan"), 1)],
                [(float("inf"), 1, 1)], [(1, 1, 1)] * 17, [("a", 1, 1)], (1, 1, 1), b"training", {"b": 1}):
        with pytest.raises(ValueError):
            mdl.resolve_jitter_views(bad)
    # nothing published about the flip views has moved
    assert _lib.SIGNATURES["nbc_tta_merge"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3)


def _refused(rc, who, text):
    err = _lib.last_error()
    assert rc == _lib.NBC_ERR_INVALID and err.startswith(who + ":") and text in err, (rc, err, text)


def test_workspace_bytes(built_lib):
    n = C.c_size_t(0)
    assert built_lib.nbc_jitter_workspace_bytes(3, 5, C.byref(n)) == _lib.NBC_OK and n.value == 8 * 3 * 5
    assert built_lib.nbc_jitter_workspace_bytes(4095, 16, C.byref(n)) == _lib.NBC_OK and n.value == 8 * 4095 * 16
    _refused(built_lib.nbc_jitter_workspace_bytes(3, 5, None), "nbc_jitter_workspace_bytes", "null argument")
    for N, V, text in ((0, 5, "bad shape"), (1, 0, "V must lie"), (1, 17, "V must lie"), (4096, 16, "bad shape"), (-1, 1, "bad shape")):
        _refused(built_lib.nbc_jitter_workspace_bytes(N, V, C.byref(n)), "nbc_jitter_workspace_bytes", text)


def test_views_arguments_are_refused_before_the_device_is_touched(built_lib):
    good = np.array(jo.TRAINING, dtype=np.float32)
    size = 2 * 64 * 64 * 3

    def call(x=FAKE, N=2, H=64, W=64, factors=good, V=5, out=FAKE + (1 << 30), ws=FAKE + (2 << 30)):
        f = None if factors is None else np.ascontiguousarray(factors, dtype=np.float32)
        return built_lib.nbc_jitter_views(x, N, H, W, None if f is None else f.ctypes.data, V, out, ws, None)

    def with_factor(value, at=(2, 1)):
        f = good.copy()
        f[at] = value
        return f

    for kw, text in [(dict(x=None), "null argument"), (dict(out=None), "null argument"), (dict(factors=None), "null argument"),
                     (dict(ws=None), "null argument"), (dict(V=0), "V must lie in 1..16"), (dict(V=17), "V must lie"),
                     (dict(V=-1), "V must lie"), (dict(N=0), "bad shape"), (dict(N=13108), "bad shape"), (dict(N=65535, V=2), "bad shape"),
                     (dict(H=0), "bad shape"), (dict(W=0), "bad shape"), (dict(W=-3), "bad shape"), (dict(H=65536, W=32768), "bad shape"),
                     (dict(factors=with_factor(np.nan)), "factor 1 of view 2"), (dict(factors=with_factor(-0.5, (0, 0))), "factor 0 of view 0"),
                     (dict(factors=with_factor(4.0001, (4, 2))), "factor 2 of view 4"), (dict(factors=with_factor(np.inf)), "must be finite"),
                     (dict(out=FAKE), "must not overlap"), (dict(out=FAKE + 100), "must not overlap"),
                     (dict(out=FAKE - 5 * size + 1), "must not overlap"), (dict(ws=FAKE + 8), "workspace_dev must not overlap"),
                     (dict(ws=FAKE + (1 << 30) + 5 * size - 8), "workspace_dev must not overlap"),
                     (dict(ws=FAKE + (2 << 30) + 4), "8-byte aligned"), (dict(ws=FAKE + (2 << 30) + 1), "8-byte aligned")]:
        _refused(call(**kw), "nbc_jitter_views", text)


def test_mean_arguments_are_refused_before_the_device_is_touched(built_lib):
    def call(x=FAKE, N=2, V=5, h=8, w=8, mean=FAKE + (1 << 30)):
        return built_lib.nbc_views_mean(x, N, V, h, w, mean, None)

    for kw, text in [(dict(x=None), "null argument"), (dict(mean=None), "null argument"), (dict(V=0), "V must lie"), (dict(V=17), "V must lie"),
                     (dict(N=0), "bad shape"), (dict(N=13108), "bad shape"), (dict(h=0), "bad shape"), (dict(w=0), "bad shape"),
                     (dict(h=65536, w=32768), "bad shape"), (dict(x=FAKE + 1), "4-byte aligned"), (dict(mean=FAKE + (1 << 30) + 2), "4-byte aligned"),
                     (dict(mean=FAKE + 16), "must not overlap"), (dict(mean=FAKE + 5 * 2 * 3 * 64 * 4 - 4), "must not overlap"),
                     (dict(mean=FAKE - 2 * 3 * 64 * 4 + 4), "must not overlap")]:
        _refused(call(**kw), "nbc_views_mean", text)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
PIL_FACTORS = [0, 0.5, 0.9, 1, 1.1, 1.2, 2]


def _frame():
    rng = np.random.default_rng(37 * 53)
    img = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    img[3] = 0
    img[4] = 0
    img[20] = 255
    img[36] = 255
    return img


def test_oracle_is_pil_image_enhance_byte_for_byte():
    img = _frame()
    pil = Image.fromarray(img, mode="RGB")
    for f in PIL_FACTORS:
        f32 = float(np.float32(f))                     # the factor the device sees
        assert np.array_equal(jo.brightness(img, f), np.asarray(ImageEnhance.Brightness(pil).enhance(f32))), f
        assert np.array_equal(jo.contrast(img, f), np.asarray(ImageEnhance.Contrast(pil).enhance(f32))), f
        assert np.array_equal(jo.saturation(img, f), np.asarray(ImageEnhance.Color(pil).enhance(f32))), f
    for b in PIL_FACTORS:
        for c in (0, 0.9, 1, 1.2, 2):
            for s in (0, 0.5, 1, 1.1):
                want = pil
                for enhancer, f in ((ImageEnhance.Brightness, b), (ImageEnhance.Contrast, c), (ImageEnhance.Color, s)):
                    want = enhancer(want).enhance(float(np.float32(f)))
                assert np.array_equal(jo.view(img, (b, c, s)), np.asarray(want)), (b, c, s)
    # the stack: view-major, the contrast mean per image
    x = np.stack([img, 255 - img // 3])
    views = [(1, 1, 1), (0.9, 1.2, 1), (1, 0.5, 1.1)]
    st = jo.stack(x, views)
    assert st.shape == (6, 37, 53, 3) and st.dtype == np.uint8 and np.array_equal(st[:2], x)
    for j, t in enumerate(views):
        for i in range(2):
            assert np.array_equal(st[j * 2 + i], jo.view(x[i], t))
    assert jo.mean_grey(x[0]) != jo.mean_grey(x[1])
    assert np.array_equal(jo.stack(x, "training")[2:4], np.stack([jo.brightness(x[0], 0.9), jo.brightness(x[1], 0.9)]))


def test_contrast_tie_rounds_up():
    img = np.array([[[0, 0, 0], [1, 1, 1]]], dtype=np.uint8)       # greys 0 and 1: the mean 0.5 is an exact half
    assert jo.grey(img).tolist() == [[0, 1]] and jo.mean_grey(img) == 1
    assert jo.contrast(img, 0).tolist() == [[[1, 1, 1], [1, 1, 1]]]
    assert np.array_equal(jo.contrast(img, 0), np.asarray(ImageEnhance.Contrast(Image.fromarray(img, mode="RGB")).enhance(0.0)))
    three = np.array([[[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0]]], dtype=np.uint8)   # mean 0.25 rounds down
    assert jo.mean_grey(three) == 0


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _blend_py(d, i, f):
    """blend in plain Python: a product and a sum of float32 values are exact in a double here, so rounding each once to
    float32 is the float32 operation."""
    t = _f32(float(d) + _f32(_f32(f) * float(i - d)))
    return 0 if t <= 0 else 255 if t >= 255 else int(t)


def test_oracle_on_a_hand_made_case():
    px = [(200, 100, 50), (10, 20, 201)]
    img = np.array([px], dtype=np.uint8)
    # brightness alone: 0.5 * 201 = 100.5 truncates to 100, 2 * 200 saturates
    assert jo.brightness(img, 0.5).tolist() == [[[100, 50, 25], [5, 10, 100]]]
    assert jo.brightness(img, 2).tolist() == [[[255, 200, 100], [20, 40, 255]]]
    assert jo.brightness(img, 0).tolist() == [[[0, 0, 0], [0, 0, 0]]]
    # saturation 0 is the grey in every channel
    greys = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16 for r, g, b in px]
    assert greys == [124, 38] and jo.saturation(img, 0).tolist() == [[[124] * 3, [38] * 3]]
    # the chain (1.1, 0.5, 1.2), step by step
    b, c, s = 1.1, 0.5, 1.2
    step1 = [tuple(_blend_py(0, v, b) for v in p) for p in px]
    assert step1 == [(220, 110, 55), (11, 22, 221)]
    g1 = [(19595 * r + 38470 * g + 7471 * bb + 32768) >> 16 for r, g, bb in step1]
    m = (2 * sum(g1) + 2) // 4
    assert g1 == [137, 41] and m == 89
    step2 = [tuple(_blend_py(m, v, c) for v in p) for p in step1]
    assert step2 == [(154, 99, 72), (50, 55, 155)]
    g2 = [(19595 * r + 38470 * g + 7471 * bb + 32768) >> 16 for r, g, bb in step2]
    step3 = [tuple(_blend_py(l, v, s) for v in p) for p, l in zip(step2, g2)]
    assert jo.view(img, (b, c, s)).tolist() == [[list(p) for p in step3]]
    assert jo.view(img, (1, 1, 1)).tolist() == [[list(p) for p in px]]
    # every byte against every factor of the issue's list, plain Python against numpy
    ramp = np.arange(256, dtype=np.uint8)
    for f in (0, 0.5, 0.8, 0.9, 0.95, 1.05, 1.1, 1.2, 1.37, 2.0, 4.0):
        for d in (0, 89, 255):
            assert jo.blend(np.uint8(d), ramp, f).tolist() == [_blend_py(d, i, f) for i in range(256)], (f, d)


def test_mean_on_hand_made_values():
    # section 3.15's values: (((a0 + a1) + a2) + a3) / 4, each operation rounded to f32
    vals = [np.float32(v) for v in (1e8, 1.0, -1e8, 3.0)]
    stackv = np.array(vals, dtype=np.float32).reshape(4, 1, 1, 1, 1)
    assert jo.mean(stackv)[0, 0, 0, 0] == np.float32(0.75)                               # 1e8 + 1 rounds to 1e8: order matters
    one = np.array([-0.0], dtype=np.float32).reshape(1, 1, 1, 1, 1)
    assert np.signbit(jo.mean(one)[0, 0, 0, 0])                                         # V = 1: the view's own bits
    assert np.isnan(jo.mean(np.array([1.0, np.nan, 2.0], dtype=np.float32).reshape(3, 1, 1, 1, 1))[0, 0, 0, 0])
    assert np.isnan(jo.mean(np.array([np.inf, -np.inf], dtype=np.float32).reshape(2, 1, 1, 1, 1))[0, 0, 0, 0])
    seven = [np.float32(v) for v in (0.1, 0.2, 0.3, 1e8, -1e8, 0.7, 7.0)]
    want = np.float32(0)
    for j, v in enumerate(seven):
        want = v if j == 0 else np.float32(want + v)
    want = np.float32(want / np.float32(7))
    got = jo.mean(np.array(seven, dtype=np.float32).reshape(7, 1, 1, 1, 1))[0, 0, 0, 0]
    assert got == want == np.float32(np.float32(7.7) / np.float32(7))                    # 0.6 is lost under 1e8, 0.7 + 7 survive
    # the views' own figures: D = V through vote_oracle
    labels = np.array([[[[0, 1, 2, 1]]], [[[0, 1, 2, 2]]], [[[0, 1, 1, 0]]], [[[0, 1, 0, 0]]], [[[0, 1, 0, 2]]]], dtype=np.uint8)
    counts, support, stats = jo.view_figures(labels)
    assert counts.tolist() == [[[1, 2, 1]], [[1, 1, 2]], [[2, 2, 0]], [[3, 1, 0]], [[2, 1, 1]]]
    assert np.array_equal(stats, vo.stats(vo.tally(labels), 5)) and support[0, 0, :2].tolist() == [255, 255]


# ---- the reports ---------------------------------------------------------------------------------------------------------------
def _f(v):
    return "{:.5f}".format(v)


def test_jitter_report_on_hand_made_counts():
    h, w = 129, 65
    px = h * w
    mc = [px - 900 - 30, 900, 30]
    vc = [[px - 1000 - 20, 1000, 20], [px - 800 - 50, 800, 50], [px - 950 - 30, 950, 30], [px - 870 - 0, 870, 0], [px - 990 - 10, 990, 10]]
    st = [px - 900, 880, 20, px - 2000, 500, 10, 5 * px - 3333, 0, 3620, 100]
    images = [("a.png", "sapin", h, w, mc, vc, st)]
    table, summary = folder_run.jitter_report(images, mdl.resolve_jitter_views("training"))
    assert table[0] == ["Name", "Type", "Views", "identity Bark %", "identity Node %", "b0.9 Bark %", "b0.9 Node %", "b1.1 Bark %",
                        "b1.1 Node %", "s0.8 Bark %", "s0.8 Node %", "s1.2 Bark %", "s1.2 Node %", "Bark %", "Node %", "Bark % spread",
                        "Node % spread", "Unanimous %", "Mean support"]
    a = table[1]
    assert a[:3] == ["a.png", "sapin", "identity+b0.9+b1.1+s0.8+s1.2"]
    for j in range(5):
        assert a[3 + 2 * j: 5 + 2 * j] == [folder_run.percent_string(vc[j][1], px), folder_run.percent_string(vc[j][2], px)]
    assert a[13:15] == [drv.stats_row("a.png", "sapin", h, w, 900, 30)[i] for i in (2, 4)]
    assert a[15] == _f(float(Fraction(100 * 200, px))) and a[16] == _f(float(Fraction(100 * 50, px)))
    assert a[17] == _f(float(Fraction(100 * (px - 2000 + 510), px))) and a[18] == _f(float(Fraction(5 * px - 3333, 5 * px)))
    assert summary["images"] == 1 and summary["views"] == jo.TRAINING_NAMES
    m = summary["means"]
    assert set(m) == {"merged_bark", "merged_node", "identity_bark", "identity_node", "abs_diff_bark", "abs_diff_node", "bark_spread",
                      "node_spread", "unanimous", "mean_support"}
    assert m["identity_bark"] == float(Fraction(100 * 1000, px)) and m["abs_diff_node"] == float(Fraction(100 * 10, px))
    # the identity view anywhere in the set, or nowhere
    moved = [(0.9, 1, 1), (1, 1, 1)]
    t2, s2 = folder_run.jitter_report([("a.png", "sapin", h, w, mc, vc[:2], st)], moved)
    assert t2[0][3:7] == ["b0.9 Bark %", "b0.9 Node %", "identity Bark %", "identity Node %"]
    assert s2["means"]["identity_bark"] == float(Fraction(100 * 800, px)) and s2["means"]["abs_diff_bark"] == float(Fraction(100 * 100, px))
    t3, s3 = folder_run.jitter_report([("a.png", "sapin", h, w, mc, vc[:2], st)], [(0.9, 1, 1), (1, 1.5, 1)])
    assert "identity_bark" not in s3["means"] and s3["views"] == ["b0.9", "c1.5"]
    # the flip views' report is the same helper under their names: nothing of it has moved
    t4, s4 = folder_run.tta_report([("a.png", "sapin", h, w, mc, vc[:4], st)], 15)
    assert t4[0] == folder_run.tta_columns(15) and [r[3:] for r in t4[1:]] == [
        r[3:] for r in folder_run.views_report([("a.png", "sapin", h, w, mc, vc[:4], st)], ["identity", "hflip", "vflip", "hvflip"], 0)[0][1:]]
    assert folder_run.jitter_report([], "training") == ([folder_run.view_columns(jo.TRAINING_NAMES)],
                                                        {"images": 0, "views": jo.TRAINING_NAMES, "means": {}})


def test_jitter_report_files(tmp_path):
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}]
    allrows = np.array([[0, 16, 16, 100, 5], [1, 16, 32, 200, 9]], dtype=np.int64)
    allt = np.array([[1, 303, 200, 9] + [300, 205, 7, 310, 195, 11] + [310, 195, 7, 300, 190, 5, 1010, 0, 400, 18],
                     [0, 151, 100, 5] + [150, 101, 5, 152, 99, 5] + [150, 101, 5, 148, 99, 5, 510, 0, 200, 10]], dtype=np.int64)
    factors = mdl.resolve_jitter_views([(1, 1, 1), (1, 1, 0.8)])
    s = drv.write_jitter_report(str(tmp_path), items, allrows, allt, factors, "fp32", "running")
    assert sorted(os.listdir(tmp_path)) == ["jitter_stats.csv", "jitter_summary.json"]
    rows = list(csv.reader(open(tmp_path / "jitter_stats.csv"), delimiter="\t"))
    want, wsum = folder_run.jitter_report([("a.png", "sapin", 16, 16, [151, 100, 5], [[150, 101, 5], [152, 99, 5]], allt[1, 10:]),
                                           ("b.png", "sapin", 16, 32, [303, 200, 9], [[300, 205, 7], [310, 195, 11]], allt[0, 10:])], factors)
    assert rows == want
    doc = json.load(open(tmp_path / "jitter_summary.json"))
    assert doc == json.loads(json.dumps(s)) and doc["precision"] == "fp32" and doc["bn_stats"] == "running"
    assert doc["views"] == ["identity", "s0.8"] and doc["means"] == json.loads(json.dumps(wsum["means"])) and doc["images"] == 2


def test_jitter_evaluation_on_hand_made_counts(tmp_path):
    ident = np.array([[900, 60, 40], [50, 800, 50], [10, 20, 70]], dtype=np.int64)          # conf[t][p]
    dark = np.array([[950, 30, 20], [150, 700, 50], [30, 40, 30]], dtype=np.int64)
    rows, doc = ev.jitter_evaluation(["identity", "b0.9"], [ident, dark])
    assert rows[0] == ["View"] + ev.JITTER_FIGURES + ["d " + k for k in ev.JITTER_FIGURES] and len(rows) == 3
    for row, conf in zip(rows[1:], (ident, dark)):
        ious, f1s = metrics.iou(conf), metrics.f1(conf)
        assert row[1:5] == ["{:.3f}".format(v) for v in ious] + ["{:.3f}".format(ious.mean())]
        assert row[5:9] == ["{:.3f}".format(v) for v in f1s] + ["{:.3f}".format(f1s.mean())]
        assert row[9:11] == [_f(100 * int(conf[:, 1].sum()) / 2000), _f(100 * int(conf[:, 2].sum()) / 2000)]
    assert rows[1][0] == "identity" and rows[1][11:] == ["0.000"] * 8 + ["0.00000"] * 2
    assert rows[2][9:11] == ["38.50000", "5.00000"] and rows[2][19:21] == ["-5.50000", "-3.00000"]
    assert rows[2][1] == "{:.3f}".format(100 * 950 / (1000 + 1130 - 950))
    assert rows[2][11] == "{:.3f}".format(100 * 950 / 1180 - 100 * 900 / 1060)
    assert doc["b0.9"]["figures"]["Bark %"] == 38.5 and doc["b0.9"]["difference"]["Node %"] == -3.0
    assert doc["identity"]["difference"]["iou_mean"] == 0.0 and list(doc) == ["identity", "b0.9"]
    # a set without the identity view has no differences
    rows2, doc2 = ev.jitter_evaluation(["b0.9", "s1.2"], [dark, ident])
    assert rows2[0] == ["View"] + ev.JITTER_FIGURES and len(rows2[1]) == 11 and doc2["s1.2"]["difference"] is None
    # the file, from gathered rows: a skipped image's row does not count
    allrows = np.zeros((3, ev.ROW_WIDTH), dtype=np.int64)
    allrows[:, 0], allrows[:, 3] = [0, 1, 2], [ev.STATUS_OK, ev.STATUS_NO_DUAL, ev.STATUS_OK]
    half = ident // 2
    all_views = np.array([[0] + list(half.ravel()) + list(dark.ravel()), [2] + list((ident - half).ravel()) + [0] * 9,
                          [1] + [7] * 18], dtype=np.int64)
    entry = ev.write_jitter_evaluation(str(tmp_path), allrows, all_views, mdl.resolve_jitter_views([(1, 1, 1), (0.9, 1, 1)]))
    assert list(csv.reader(open(tmp_path / ev.JITTER_EVALUATION_CSV), delimiter="\t")) == rows
    assert entry["views"] == ["identity", "b0.9"] and entry["evaluation"] == doc
    assert entry["factors"] == [[1.0, 1.0, 1.0], [float(np.float32(0.9)), 1.0, 1.0]]
    # what the command line prints of it
    text = ev.format_summary({"images_evaluated": 2, "precision": "fp32", "model_path": "m.pt", "images_skipped": 1,
                              "skipped": {"no_dual": ["sapin/x.png"]}, "jitter": entry})
    assert "view b0.9 (its own final labels, pooled): " in text and "Bark % 38.500 (-5.500), Node % 5.000 (-3.000)" in text
    assert "view identity" in text and "Bark % 44.000 (+0.000)" in text


# ---- the command line and the library keywords -----------------------------------------------------------------------------
def _cli(module, *argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd." + module, "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--jitter", "training", "--tta", "flips"], "--jitter cannot go with --tta"),
                                       (["--jitter_views", "1,1,1;0.9,1,1", "--tta", "hflip"], "--jitter cannot go with --tta"),
                                       (["--jitter", "training", "--dropout_draws", "4"], "--jitter cannot go with --dropout_draws"),
                                       (["--jitter", "training", "--only_preprocess"], "--jitter runs the network"),
                                       (["--jitter", "training", "--jitter_views", "1,1,1"], "exclude each other"),
                                       (["--jitter_votes"], "--jitter_votes needs --jitter"),
                                       (["--jitter", "flips"], "invalid choice"),
                                       (["--jitter_views", "1,1"], "--jitter_views takes triples"),
                                       (["--jitter_views", "1,1,1;"], "--jitter_views takes triples"),
                                       (["--jitter_views", "1,a,1"], "--jitter_views takes triples"),
                                       (["--jitter_views", "1,1,4.5"], "[0, 4]"),
                                       (["--jitter_views", "1,nan,1"], "[0, 4]"),
                                       (["--jitter_views", ";".join(["1,1,1"] * 17)], "1..16")])
def test_predict_refuses_with_code_2(argv, text):
    p = _cli("predict", *argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


@pytest.mark.parametrize("argv,text", [(["--jitter", "training", "--tta", "flips"], "--jitter cannot go with --tta"),
                                       (["--jitter", "training", "--jitter_views", "1,1,1"], "exclude each other"),
                                       (["--jitter_views", "1,1,-1"], "[0, 4]"),
                                       (["--jitter", "rot90"], "invalid choice"),
                                       (["--jitter", "training", "--jitter_votes"], "unrecognized arguments")])   # predict only
def test_evaluate_refuses_with_code_2(argv, text):
    p = _cli("evaluate", *argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike(built_lib):
    nowhere = ("/nonexistent/folder", "/nonexistent/ckpt.pt")
    with pytest.raises(ValueError, match="--jitter_votes needs --jitter"):
        drv.predict_folder(*nowhere, jitter_votes=True)
    with pytest.raises(ValueError, match="cannot go with --tta"):
        drv.predict_folder(*nowhere, jitter="training", tta="flips")
    with pytest.raises(ValueError, match="cannot go with --dropout_draws"):
        drv.predict_folder(*nowhere, jitter="training", dropout_draws=4)
    with pytest.raises(ValueError, match="--jitter must be one of"):
        drv.predict_folder(*nowhere, jitter="flips")
    with pytest.raises(ValueError, match="exclude each other"):
        drv.predict_folder(*nowhere, jitter="training", jitter_views=[(1, 1, 1)])
    with pytest.raises(ValueError, match="--jitter_views"):
        drv.predict_folder(*nowhere, jitter_views=[(1, 1, 5)])
    with pytest.raises(ValueError, match="--jitter must be one of"):
        ev.evaluate_folder(*nowhere, jitter="flips")
    with pytest.raises(ValueError, match="cannot go with --tta"):
        ev.evaluate_folder(*nowhere, jitter_views="1,1,1;1,1,0.8", tta="hflip")
    assert folder_run.check_jitter_arguments() is None and folder_run.check_jitter_arguments("none", tta="flips") is None
    assert np.array_equal(folder_run.check_jitter_arguments("training", jitter_votes=True), mdl.resolve_jitter_views("training"))
    assert np.array_equal(folder_run.check_jitter_arguments(jitter_views="1,1,1;0.9,1.05,1", tta="none"),
                          np.array([[1, 1, 1], [0.9, 1.05, 1]], dtype=np.float32))
    assert folder_run.parse_jitter_views("1,1,1; 0.9 ,1,1e0") == [(1.0, 1.0, 1.0), (0.9, 1.0, 1.0)]
    with pytest.raises(ValueError, match="--only_preprocess"):
        folder_run.check_jitter_arguments("training", only_preprocess=True)
    m = mdl.FCNResNet50("fp32")
    with pytest.raises(ValueError, match="float32 input is refused"):               # before the missing device is noticed
        m.predict_labels_jitter(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(ValueError, match="float32 input is refused"):
        m.jitter_views(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(ValueError):
        m.predict_labels_jitter(torch.zeros((1, 64, 64, 3), dtype=torch.uint8), views="flips")
    with pytest.raises(RuntimeError):                              # no device, no weights
        m.predict_labels_jitter(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        m.jitter_views(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        m.views_mean(torch.zeros((5, 3, 8, 8)), 1)


def test_folders_of_the_support_only_with_the_flag(tmp_path):
    for tag, on in (("off", False), ("on", True)):
        root = tmp_path / tag
        (root / "samples" / "sapin").mkdir(parents=True)
        drv.generate_folders(str(root), jitter_votes=on)
        assert sorted(os.listdir(root / "results")) == sorted(["combined_images", "outputs"] + (["jitter_support"] if on else []))
