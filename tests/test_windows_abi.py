"""The crop windows (`--windows`) without a GPU: the C ABI's symbols, signatures and constants, every refusal in front of the
device, nbc_window_grid and the numpy restatement of tests/helpers/window_oracle.py against numpy.pad and plain Python in
Fractions, the report arithmetic and the command line's refusals."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib, folder_run
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd import predict as drv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import window_oracle as wo  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40


def test_symbols_signatures_and_constants(built_lib):
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for name in ("nbc_window_grid", "nbc_window_views", "nbc_window_merge"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name) and ("int %s(" % name) in header
    ints = C.POINTER(C.c_int)
    assert _lib.SIGNATURES["nbc_window_grid"] == (C.c_int, [C.c_int] * 4 + [ints] * 3)
    assert _lib.SIGNATURES["nbc_window_views"] == (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 2)
    assert _lib.SIGNATURES["nbc_window_merge"] == (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 2)
    flat = re.sub(r"\s+", " ", header)
    assert "int nbc_window_grid(int H, int W, int S, int T, int* dims, int* offsets_y, int* offsets_x);" in flat
    assert ("int nbc_window_views(const void* x_dev, int x_dtype, int N, int H, int W, int S, int T, void* out_dev, "
            "void* hip_stream);") in flat
    assert ("int nbc_window_merge(const float* lowres_windows_dev, int N, int H, int W, int S, int T, int blend, "
            "float* merged_dev, void* hip_stream);") in flat
    for name, value in (("WINDOW_CELL", 8), ("WINDOW_MAX_K", 1024), ("BLEND_TENT", 0), ("BLEND_UNIFORM", 1)):
        assert re.search(r"NBC_%s = %d\b" % (name, value), header), name
        assert getattr(_lib, name) == value
    assert (wo.CELL, wo.TENT, wo.UNIFORM) == (_lib.WINDOW_CELL, _lib.BLEND_TENT, _lib.BLEND_UNIFORM)
    assert mdl.WINDOW_BLENDS == {"tent": 0, "uniform": 1} and tuple(sorted(mdl.WINDOW_BLENDS)) == folder_run.WINDOW_BLENDS
    for cite in ("__main__.py:158-165", "utils.py:242-247"):
        assert cite in header
    for bad in ("gauss", None, 0, True):
        with pytest.raises(ValueError):
            mdl.resolve_window_blend(bad)
    # nothing published about the flip views has moved
    assert _lib.SIGNATURES["nbc_tta_views"] == (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 2)


def _refused(rc, who, text):
    err = _lib.last_error()
    assert rc == _lib.NBC_ERR_INVALID and err.startswith(who + ":") and text in err, (rc, err, text)


GRID_REFUSALS = [(dict(S=24), "window must be"), (dict(S=2056), "window must be"), (dict(S=60), "window must be"), (dict(S=-64), "window must be"),
                 (dict(T=0), "stride must be"), (dict(T=4), "stride must be"), (dict(T=12), "stride must be"), (dict(T=72), "stride must be"),
                 (dict(S=128, T=8), "stride must be"), (dict(H=7), "H, W >= 8"), (dict(W=0), "H, W >= 8"), (dict(W=-8), "H, W >= 8"),
                 (dict(H=65536, W=32768), "H * W < 2^31"), (dict(H=1024, W=1024, S=32, T=8), "more than 1024 windows")]


def test_grid_arguments_are_refused(built_lib):
    dims, oy, ox = (C.c_int * 4)(), (C.c_int * 1024)(), (C.c_int * 1024)()

    def call(H=64, W=64, S=64, T=32, d=dims):
        return built_lib.nbc_window_grid(H, W, S, T, d, oy, ox)

    for kw, text in [(dict(d=None), "null argument")] + GRID_REFUSALS:
        _refused(call(**kw), "nbc_window_grid", text)
    assert call() == _lib.NBC_OK and list(dims) == [64, 64, 1, 1]
    assert built_lib.nbc_window_grid(64, 200, 64, 32, dims, None, None) == _lib.NBC_OK and list(dims) == [64, 64, 1, 6]


def test_views_arguments_are_refused_before_the_device_is_touched(built_lib):
    def call(x=FAKE, dtype=_lib.IN_U8_NHWC, N=2, H=64, W=64, S=64, T=32, out=FAKE + (1 << 30)):
        return built_lib.nbc_window_views(x, dtype, N, H, W, S, T, out, None)

    for kw, text in [(dict(x=None), "null argument"), (dict(out=None), "null argument"), (dict(dtype=2), "bad x_dtype"),
                     (dict(dtype=-1), "bad x_dtype"), (dict(N=0), "N >= 1"), (dict(N=-1), "N >= 1"),
                     (dict(N=65535, H=128), "K * N <= 65535"), (dict(N=200, H=1024, W=520, S=64, T=32), "K * N <= 65535"),
                     (dict(dtype=_lib.IN_F32_NCHW, x=FAKE + 2), "4-byte aligned"),
                     (dict(dtype=_lib.IN_F32_NCHW, out=FAKE + (1 << 30) + 1), "4-byte aligned"),
                     (dict(out=FAKE), "must not overlap"), (dict(out=FAKE + 100), "must not overlap"),
                     # 129 x 65 at S = 64, T = 32: 4 x 2 windows of 64 x 64 -- the stack is larger than the batch
                     (dict(H=129, W=65, out=FAKE - 8 * 2 * 64 * 64 * 3 + 1), "must not overlap")] + GRID_REFUSALS:
        _refused(call(**kw), "nbc_window_views", text)


def test_merge_arguments_are_refused_before_the_device_is_touched(built_lib):
    def call(x=FAKE, N=2, H=64, W=64, S=64, T=32, blend=0, merged=FAKE + (1 << 30)):
        return built_lib.nbc_window_merge(x, N, H, W, S, T, blend, merged, None)

    for kw, text in [(dict(x=None), "null argument"), (dict(merged=None), "null argument"), (dict(blend=2), "bad blend"),
                     (dict(blend=-1), "bad blend"), (dict(N=0), "N >= 1"), (dict(N=65535, H=128), "K * N <= 65535"),
                     (dict(x=FAKE + 1), "4-byte aligned"), (dict(merged=FAKE + (1 << 30) + 2), "4-byte aligned"),
                     (dict(merged=FAKE), "must not overlap"), (dict(merged=FAKE + 16), "must not overlap"),
                     (dict(H=129, W=65, merged=FAKE + 8 * 2 * 3 * 8 * 8 * 4 - 4), "must not overlap"),
                     (dict(merged=FAKE - 2 * 3 * 8 * 8 * 4 + 4), "must not overlap")] + GRID_REFUSALS:
        _refused(call(**kw), "nbc_window_merge", text)


# ---- the grid and the restatement ------------------------------------------------------------------------------------------
GRID_CASES = [(8, 32, 8), (13, 32, 16), (40, 32, 16), (75, 32, 16), (129, 64, 32), (191, 64, 32), (200, 64, 24),
              (601, 512, 256), (730, 512, 256), (1024, 512, 256), (1024, 64, 8)]


@pytest.mark.parametrize("case", GRID_CASES)
def test_grid_is_the_rule(built_lib, case):
    L, S, T = case
    L8, E, offsets = wo.grid(L, S, T)
    assert L8 == 8 * ((L + 7) // 8) and E == min(S, L8)
    n = 1 if L8 <= S else 1 + -(-(L8 - S) // T)
    assert len(offsets) == n and all(o % 8 == 0 for o in offsets) and offsets == sorted(set(offsets))
    assert offsets[0] == 0 and offsets[-1] + E == L8 and all(b - a <= T for a, b in zip(offsets, offsets[1:]))
    for other in (8, 72):                            # the axes are independent
        ey, ex, ny, nx, oys, oxs = mdl.window_grid(L, other, S, T)
        assert (ey, ny, oys) == (E, n, offsets) and (ex, nx, oxs) == (wo.grid(other, S, T)[1], len(wo.grid(other, S, T)[2]), wo.grid(other, S, T)[2])
        ey, ex, ny, nx, oys, oxs = mdl.window_grid(other, L, S, T)
        assert (ex, nx, oxs) == (E, n, offsets)
    # every cell is covered, with a weight sum >= 1, by at most 9 windows
    cover, wsum = np.zeros(L8 // 8, dtype=np.int64), np.zeros(L8 // 8, dtype=np.int64)
    for k, o in enumerate(offsets):
        w = wo.axis_weights(L, S, T, k)
        assert w.min() >= 1 and w.max() <= max(1, E // 16)
        cover[o // 8: (o + E) // 8] += 1
        wsum[o // 8: (o + E) // 8] += w
    assert cover.min() >= 1 and cover.max() <= 9 and wsum.min() >= 1
    if case == (1024, 64, 8):
        assert cover.max() == 8
    if case == (129, 64, 32):
        assert offsets == [0, 32, 64, 72]
    if case == (200, 64, 24):
        assert offsets[-1] == 136


def test_grid_of_the_defaults():
    assert mdl.window_grid(1024, 1024)[:4] == (512, 512, 3, 3)
    assert mdl.window_grid(601, 1024)[:4] == (512, 512, 2, 3) and mdl.window_grid(600, 1024)[:4] == (512, 512, 2, 3)
    assert mdl.window_grid(512, 1024)[:4] == (512, 512, 1, 3) and mdl.window_grid(505, 1024)[:4] == (512, 512, 1, 3)
    assert mdl.window_grid(200, 1024)[:4] == (200, 512, 1, 3)
    for bad in ((1024, 1024, 500, 256), (1024, 1024, 512, 32), (4, 64, 64, 32), ("a", 64, 64, 32), (2 ** 40, 64, 64, 32)):
        with pytest.raises(ValueError):
            mdl.window_grid(*bad)
    m = mdl.FCNResNet50("fp32")
    assert m.window_grid(129, 191, 64, 32) == (64, 64, 4, 5, [0, 32, 64, 72], [0, 32, 64, 96, 128])


@pytest.mark.parametrize("hw", [(8, 8), (13, 21), (9, 16), (15, 33), (40, 75)])
def test_fill_is_numpy_pad_reflect(hw):
    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    u8 = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
    f32 = rng.standard_normal((2, 3, h, w)).astype(np.float32)
    assert np.array_equal(wo.fill(u8, 1, 2), np.pad(u8, ((0, 0), (0, -h % 8), (0, -w % 8), (0, 0)), mode="reflect"))
    assert np.array_equal(wo.fill(f32, 2, 3), np.pad(f32, ((0, 0), (0, 0), (0, -h % 8), (0, -w % 8)), mode="reflect"))
    for L in range(8, 64):                           # the reach stays inside the frame
        assert all(0 <= wo.reflect_index(i, L) < L for i in range(8 * ((L + 7) // 8)))
    s = wo.stack(u8, 32, 16)
    ey, ex, ny, nx, oys, oxs = mdl.window_grid(h, w, 32, 16)
    assert s.shape == (ny * nx * 2, ey, ex, 3)
    pad = wo.fill(u8, 1, 2)
    assert np.array_equal(s[(ny * nx - 1) * 2 + 1], pad[1, oys[-1]: oys[-1] + ey, oxs[-1]: oxs[-1] + ex])   # entry k * N + i


@pytest.mark.parametrize("blend", [wo.TENT, wo.UNIFORM])
def test_merge_against_fractions(blend):
    """One axis of 8 cells (the other a single window): integer-valued logits make every f32 operation exact, so the
    restatement must equal the weighted mean in Fractions."""
    H, W, S, T = 8, 64, 32, 16                       # offsets 0, 16, 32; e = 4, cap = 2
    _, _, offsets = wo.grid(W, S, T)
    assert offsets == [0, 16, 32]
    rng = np.random.default_rng(5)
    v = rng.integers(-8, 9, size=(3, 1, 3, 1, 4)).astype(np.float32)
    got = wo.merge(v.reshape(3, 3, 1, 4), 1, H, W, S, T, blend)
    assert got.shape == (1, 3, 1, 8)
    weights = [[1, 1, 1, 1]] * 3 if blend == wo.UNIFORM else [[2, 2, 2, 1], [1, 2, 2, 1], [1, 2, 2, 2]]
    for k in range(3):
        assert wo.axis_weights(W, S, T, k, blend).tolist() == weights[k]
    for c in range(3):
        for x in range(8):
            terms = [(weights[k][x - o // 8], int(v[k, 0, c, 0, x - o // 8])) for k, o in enumerate(offsets) if 0 <= x - o // 8 < 4]
            want = Fraction(terms[0][1]) if len(terms) == 1 else Fraction(sum(w * t for w, t in terms), sum(w for w, _ in terms))
            assert Fraction(float(got[0, c, 0, x])) == Fraction(float(np.float32(float(want)))), (c, x, terms)
            assert len(terms) == (1 if x in (0, 1, 6, 7) else 2)
    # a cell one window covers keeps that window's bits; a NaN poisons the cells it covers and no other
    z = np.zeros((3, 3, 1, 4), dtype=np.float32)
    z[0, :, 0, 0] = np.float32(-0.0)
    z[1, 0, 0, 1] = np.float32("nan")
    m = wo.merge(z, 1, H, W, S, T, blend)
    assert m.view(np.uint32)[0, 0, 0, 0] == 0x80000000 and np.isnan(m[0, 0, 0, 3]) and int(np.isnan(m).sum()) == 1


def test_merge_two_axes_against_fractions():
    H, W, S, T = 40, 75, 32, 16
    ey, ex, ny, nx, oys, oxs = mdl.window_grid(H, W, S, T)
    rng = np.random.default_rng(9)
    v = rng.integers(-4, 5, size=(ny * nx, 2, 3, 4, 4)).astype(np.float32)
    got, cover = wo.merge(v.reshape(-1, 3, 4, 4), 2, H, W, S, T, return_cover=True)
    assert got.shape == (2, 3, 5, 10) and cover.max() == 4 and cover[0, 0] == 1
    for y in range(5):
        for x in range(10):
            num, den = Fraction(0), 0
            for r, oy in enumerate(oys):
                for c, ox in enumerate(oxs):
                    jy, jx = y - oy // 8, x - ox // 8
                    if 0 <= jy < 4 and 0 <= jx < 4:
                        w = int(wo.axis_weights(H, S, T, r)[jy] * wo.axis_weights(W, S, T, c)[jx])
                        num += w * int(v[r * nx + c, 1, 2, jy, jx])
                        den += w
            assert Fraction(float(got[1, 2, y, x])) == Fraction(float(np.float32(float(num / den)))), (y, x)


# ---- the report ------------------------------------------------------------------------------------------------------------
def test_report_arithmetic(tmp_path):
    images = [("a.png", "sapin", 600, 1024, (512, 512, 2, 3), [400000, 200000, 14400], [390000, 209000, 15400], 12345),
              ("b.png", "epinette_gelee", 512, 1024, (512, 512, 1, 3), [500000, 24000, 288], [500000, 24288, 0], 300)]
    rows, summary = folder_run.windows_report(images, 512, 256, "tent", compare=True)
    assert rows[0] == folder_run.WINDOW_COLUMNS + folder_run.WINDOW_COMPARE_COLUMNS and len(rows) == 3
    px = 600 * 1024
    assert rows[1] == ["a.png", "sapin", "600", "1024", "512x512", "2x3", folder_run.percent_string(200000, px),
                       folder_run.percent_string(14400, px), folder_run.percent_string(209000, px), folder_run.percent_string(15400, px),
                       "{:.5f}".format(100 * (200000 - 209000) / px), "{:.5f}".format(100 * (14400 - 15400) / px),
                       "{:.5f}".format(100 * 12345 / px)]
    assert rows[1][6] == drv.stats_row("a.png", "sapin", 600, 1024, 200000, 14400)[2]          # final_stats.csv's own digits
    px2 = 512 * 1024
    means = summary["means"]
    assert means["merged_bark"] == (100 * 200000 / px + 100 * 24000 / px2) / 2
    assert means["abs_diff_node"] == (100 * 1000 / px + 100 * 288 / px2) / 2 and means["changed"] == (100 * 12345 / px + 100 * 300 / px2) / 2
    assert summary["grids"] == {"512x512 1x3": 1, "512x512 2x3": 1} and summary["images"] == 2
    assert (summary["window"], summary["stride"], summary["blend"]) == (512, 256, "tent")
    plain_rows, plain_summary = folder_run.windows_report(images, 512, 256, "uniform")
    assert plain_rows[0] == folder_run.WINDOW_COLUMNS and [r[:8] for r in rows] == plain_rows
    assert sorted(plain_summary["means"]) == ["merged_bark", "merged_node"]
    # the writer: rows gathered as the driver gathers them
    items = [dict(name="a.png", wood="sapin"), dict(name="b.png", wood="epinette_gelee")]
    allrows = np.array([[0, 600, 1024, 200000, 14400], [1, 512, 1024, 24000, 288]], dtype=np.int64)
    allw = np.array([[0] + images[0][5] + images[0][6] + [12345], [1] + images[1][5] + images[1][6] + [300]], dtype=np.int64)
    wn = folder_run.check_windows_arguments(512, windows_compare=True)
    s = drv.write_windows_report(str(tmp_path), items, allrows, allw, wn, "f16x2")
    import csv
    assert list(csv.reader(open(tmp_path / "windows_stats.csv"), delimiter="\t")) == rows
    doc = json.load(open(tmp_path / "windows_summary.json"))
    assert doc == json.loads(json.dumps(s)) and doc["precision"] == "f16x2" and doc["means"] == json.loads(json.dumps(summary["means"]))
    # evaluate's table: jitter_evaluation on the two pooled confusions
    conf = np.array([[[50, 3, 0], [4, 30, 1], [0, 2, 10]], [[48, 5, 0], [2, 33, 0], [1, 1, 10]]], dtype=np.int64)
    all_win = np.array([[0] + list(conf[0].reshape(-1)) + list(conf[1].reshape(-1)), [-1] + [7] * 18], dtype=np.int64)
    evrows = np.array([[0, 10, 10, ev.STATUS_OK] + [0] * 18], dtype=np.int64)
    os.makedirs(tmp_path / "ev")
    doc = ev.write_windows_evaluation(str(tmp_path / "ev"), evrows, all_win)
    table, want = ev.jitter_evaluation(["identity", "windows"], conf)
    assert doc == want and list(csv.reader(open(tmp_path / "ev" / ev.WINDOWS_EVALUATION_CSV), delimiter="\t")) == table
    assert doc["windows"]["difference"]["Bark %"] == want["windows"]["figures"]["Bark %"] - want["identity"]["figures"]["Bark %"]


def test_argument_rules():
    chk = folder_run.check_windows_arguments
    assert chk() is None
    wn = chk(512)
    assert (wn.window, wn.stride, wn.blend, wn.compare) == (512, 256, "tent", False)
    assert chk(200).stride == 96 and chk(40).stride == 16 and folder_run.default_window_stride(56) == 24
    wn = chk(64, 24, "uniform", True, tta="none", bn_stats="running", arch="deeplabv3_resnet50")
    assert (wn.window, wn.stride, wn.blend, wn.compare) == (64, 24, "uniform", True)
    for kw, text in [(dict(windows_stride=32), "--windows_stride needs --windows"), (dict(windows_blend="tent"), "--windows_blend needs --windows"),
                     (dict(windows_compare=True), "--windows_compare needs --windows"),
                     (dict(windows=500), "--windows must be"), (dict(windows=24), "--windows must be"), (dict(windows=4096), "--windows must be"),
                     (dict(windows=64, windows_stride=4), "--windows_stride must be"), (dict(windows=64, windows_stride=72), "--windows_stride must be"),
                     (dict(windows=512, windows_stride=32), "--windows_stride must be"), (dict(windows=64, windows_blend="gauss"), "--windows_blend must be"),
                     (dict(windows=64, tta="flips"), "cannot go with --tta"), (dict(windows=64, jitter="training"), "cannot go with --jitter"),
                     (dict(windows=64, jitter_views="1,1,1"), "cannot go with --jitter"), (dict(windows=64, dropout_draws=4), "cannot go with --dropout_draws"),
                     (dict(windows=64, only_preprocess=True), "--only_preprocess"), (dict(windows=64, bn_stats="image"), "--bn_stats image"),
                     (dict(windows=64, bn_stats="image_f16x2"), "--bn_stats image_f16x2"),
                     (dict(windows=64, arch="fcn_efficientnet_b0"), "output stride is 32"),
                     (dict(windows=64, arch="deeplabv3_efficientnet_b3"), "output stride is 32")]:
        with pytest.raises(ValueError, match=re.escape(text)):
            chk(**kw)


# ---- the command line and the library keywords -----------------------------------------------------------------------------
def _cli(module, *argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd." + module, "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--windows_stride", "32"], "--windows_stride needs --windows"),
                                       (["--windows_compare"], "--windows_compare needs --windows"),
                                       (["--windows", "512", "--tta", "flips"], "--windows cannot go with --tta"),
                                       (["--windows", "512", "--jitter", "training"], "--windows cannot go with --jitter"),
                                       (["--windows", "512", "--jitter_views", "1,1,1"], "--windows cannot go with --jitter"),
                                       (["--windows", "512", "--dropout_draws", "4"], "--windows cannot go with --dropout_draws"),
                                       (["--windows", "512", "--only_preprocess"], "--windows runs the network"),
                                       (["--windows", "512", "--bn_stats", "image"], "--windows cannot go with --bn_stats image"),
                                       (["--windows", "512", "--bn_stats", "image_f16x2", "--precision", "f16x2"], "--windows cannot go with --bn_stats"),
                                       (["--windows", "512", "--arch", "fcn_efficientnet_b0"], "output stride is 32"),
                                       (["--windows", "500"], "--windows must be"),
                                       (["--windows", "512", "--windows_stride", "48"], "--windows_stride must be"),
                                       (["--windows", "512", "--windows_blend", "gauss"], "invalid choice")])
def test_predict_refuses_with_code_2(argv, text):
    p = _cli("predict", *argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


@pytest.mark.parametrize("argv,text", [(["--windows_blend", "uniform"], "--windows_blend needs --windows"),
                                       (["--windows", "512", "--tta", "hflip"], "--windows cannot go with --tta"),
                                       (["--windows", "512", "--jitter", "training"], "--windows cannot go with --jitter"),
                                       (["--windows", "512", "--bn_stats", "image"], "--windows cannot go with --bn_stats image"),
                                       (["--windows", "512", "--arch", "deeplabv3_efficientnet_b0"], "output stride is 32"),
                                       (["--windows", "36"], "--windows must be")])
def test_evaluate_refuses_with_code_2(argv, text):
    p = _cli("evaluate", *argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike(built_lib):
    with pytest.raises(ValueError, match="--windows_compare needs --windows"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", windows_compare=True)
    with pytest.raises(ValueError, match="cannot go with --dropout_draws"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", windows=512, dropout_draws=4)
    with pytest.raises(ValueError, match="cannot go with --tta"):
        ev.evaluate_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", windows=512, tta="flips")
    with pytest.raises(ValueError, match="--bn_stats image"):
        ev.evaluate_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", windows=512, bn_stats="image")
    m = mdl.FCNResNet50("fp32")
    with pytest.raises(RuntimeError):                              # no device, no weights
        m.predict_labels_windows(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(RuntimeError):
        m.window_views(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(RuntimeError):
        m.window_merge(torch.zeros((1, 3, 8, 8)), 1, 64, 64)
    e = mdl.fcn_efficientnet(0)
    with pytest.raises(ValueError, match="output stride is 32"):   # the reason comes before the device
        e.predict_labels_windows(torch.zeros((1, 3, 64, 64)))
