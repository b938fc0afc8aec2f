"""The training run's frame (`evaluate --frame training`) without a GPU: the C ABI's symbols, signatures and constants,
nbc_bilinear_taps against its host restatement integer for integer, every refusal of nbc_training_frame in front of the device
with its exact boundaries, and the driver's refusals, `--subset` included."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd import training_frame as tf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40
I32 = C.POINTER(C.c_int32)


def test_symbols_signatures_and_constants(built_lib):
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for name in ("nbc_bilinear_taps", "nbc_training_frame"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name) and ("int %s(" % name) in header
    assert _lib.SIGNATURES["nbc_bilinear_taps"] == (C.c_int, [C.c_int, C.c_int, I32, I32])
    assert _lib.SIGNATURES["nbc_training_frame"] == (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4)
    flat = re.sub(r"\s+", " ", header)
    assert "int nbc_bilinear_taps(int in_size, int out_size, int32_t* first, int32_t* coeff);" in flat
    assert ("int nbc_training_frame(const void* x_dev, int channels, int N, int H, int W, int Ht, int Wt, const int32_t* row_taps_dev, "
            "const int32_t* col_taps_dev, void* out_dev, void* hip_stream);") in flat
    assert re.search(r"NBC_FRAME_TAPS = 3\b", header) and _lib.FRAME_TAPS == tf.FRAME_TAPS == 3
    for cite in ("utils.py:242-247", "__main__.py:209-228"):
        assert cite in header
    # the frame has left the windows' left-out list
    assert "and the training's exact" not in flat
    # nothing published about the windows has moved
    assert _lib.SIGNATURES["nbc_window_views"] == (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 2)
    assert "training_frame.hip" in __import__("neuralbarkcalculator_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("n", [8, 24, 32, 160, 1024])
def test_the_c_table_is_the_host_restatement(built_lib, n):
    first, coeff = mdl.bilinear_taps(n + 1, n)
    want_first, want_coeff = tf.bilinear_taps(n + 1, n)
    assert first.dtype == coeff.dtype == np.int32
    np.testing.assert_array_equal(first, want_first)
    np.testing.assert_array_equal(coeff, want_coeff)
    assert (np.abs(coeff.sum(axis=1).astype(np.int64) - (1 << 22)) <= (coeff != 0).sum(axis=1) // 2 + 1).all()
    table = tf.table_of(first, coeff)
    assert table.dtype == np.int32 and table.shape == (n, 4) and table.flags.c_contiguous
    np.testing.assert_array_equal(table[:, 0], first)
    np.testing.assert_array_equal(table[:, 1:], coeff)


def _refused(rc, who, text):
    err = _lib.last_error()
    assert rc == _lib.NBC_ERR_INVALID and err.startswith(who + ":") and text in err, (rc, err, text)


def test_table_sizes_are_refused(built_lib):
    first, coeff = (C.c_int32 * 64)(), (C.c_int32 * 192)()
    for n_in, n_out in ((32, 32), (34, 32), (31, 32), (1, 0), (0, -1), (64, 32)):
        _refused(built_lib.nbc_bilinear_taps(n_in, n_out, first, coeff), "nbc_bilinear_taps", "in_size must be out_size + 1")
    _refused(built_lib.nbc_bilinear_taps(33, 32, None, coeff), "nbc_bilinear_taps", "null argument")
    _refused(built_lib.nbc_bilinear_taps(33, 32, first, None), "nbc_bilinear_taps", "null argument")
    assert built_lib.nbc_bilinear_taps(33, 32, first, coeff) == _lib.NBC_OK
    for bad in ((32, 32), (None, 8), ("a", 8), (2 ** 31, 2 ** 31 - 1)):
        with pytest.raises(ValueError):
            mdl.bilinear_taps(*bad)


def test_frame_arguments_are_refused_before_the_device_is_touched(built_lib):
    """No GPU is here: a call that got past its argument check would fail in the launch (NBC_ERR_HIP) or crash, so a refusal with
    NBC_ERR_INVALID and its message is a refusal in front of the device; a call that passes the check must not be made."""
    out0 = FAKE + (1 << 32)

    def call(x=FAKE, channels=3, N=2, H=21, W=23, Ht=32, Wt=32, rows=FAKE + (1 << 33), cols=FAKE + (1 << 34), out=out0):
        return built_lib.nbc_training_frame(x, channels, N, H, W, Ht, Wt, rows, cols, out, None)

    reach = "more than one reflection"
    for kw, text in [(dict(x=None), "null argument"), (dict(out=None), "null argument"),
                     (dict(channels=0), "channels must be 1 or 3"), (dict(channels=2), "channels must be 1 or 3"), (dict(channels=4), "channels must be 1 or 3"),
                     (dict(N=0), "1 <= N <= 65535"), (dict(N=-1), "1 <= N <= 65535"), (dict(N=65536), "1 <= N <= 65535"),
                     (dict(H=0), "H, W, Ht, Wt >= 1"), (dict(W=-3), "H, W, Ht, Wt >= 1"), (dict(Ht=0), "H, W, Ht, Wt >= 1"),
                     (dict(H=33), "the source exceeds the frame"), (dict(W=33), "the source exceeds the frame"),
                     (dict(H=1025, W=8, Ht=1024, Wt=8), "the source exceeds the frame"),
                     # p = ceil((Lt - L) / 2) against L - 1: 8 -> 24 has p = 8 = L, 9 -> 24 has p = 8 = L - 1 (below)
                     (dict(H=8, Ht=24, W=24, Wt=24), reach), (dict(H=24, Ht=24, W=8, Wt=24), reach), (dict(H=11), reach), (dict(W=11), reach),
                     (dict(H=1, Ht=2), reach), (dict(H=341, W=1024, Ht=1024, Wt=1024), reach),
                     (dict(H=40000, W=30000, Ht=65536, Wt=32768), "Ht * Wt < 2^31"),
                     (dict(rows=None), "needs its table"), (dict(cols=None), "needs its table"),
                     (dict(H=22, W=21, rows=None, cols=None), "needs its table"),
                     (dict(rows=FAKE + 2), "4-byte aligned"), (dict(cols=FAKE + 1), "4-byte aligned"),
                     (dict(out=FAKE), "must not overlap"), (dict(out=FAKE + 2 * 21 * 23 * 3 - 1), "must not overlap"),
                     (dict(out=FAKE - 2 * 32 * 32 * 3 + 1), "must not overlap"),
                     (dict(channels=1, out=FAKE + 2 * 21 * 23 - 1), "must not overlap")]:
        _refused(call(**kw), "nbc_training_frame", text)
    # the boundaries of the argument check, read off the one refusal that follows the geometry's: 9 -> 24 (p = L - 1) and
    # 12 -> 32 pass it and are refused only for the missing table; an axis that is not resampled needs none and gets that far too
    _refused(call(H=9, Ht=24, W=24, Wt=24, rows=None, cols=None), "nbc_training_frame", "needs its table")
    _refused(call(H=24, Ht=24, W=9, Wt=24, rows=None, cols=None), "nbc_training_frame", "needs its table")
    _refused(call(H=342, W=1024, Ht=1024, Wt=1024, rows=None, cols=None, out=FAKE), "nbc_training_frame", "must not overlap")
    _refused(call(H=22, W=32, rows=None, cols=None, out=FAKE + 5), "nbc_training_frame", "must not overlap")
    _refused(call(N=65535, H=22, W=32, rows=None, cols=None, out=FAKE + 5), "nbc_training_frame", "must not overlap")
    _refused(call(H=32768, W=65535, Ht=32768, Wt=65535, rows=None, cols=None, out=FAKE + 5), "nbc_training_frame", "must not overlap")


def test_model_refuses_without_a_device(built_lib):
    m = mdl.FCNResNet50("fp32")
    with pytest.raises(RuntimeError):                              # no device
        m.training_frame(torch.zeros((1, 21, 23, 3), dtype=torch.uint8))


# ---- the driver ------------------------------------------------------------------------------------------------------------
def test_frame_argument_rules():
    chk = ev.check_frame_arguments
    assert chk() == (None, None) and chk("scan") == (None, None) and chk(None) == (None, None)
    assert chk("training") == (1024, 8) and chk("training", 160, 3) == (160, 3) and chk("training", 8, 64) == (8, 64)
    assert chk("training", target_size=512) == (512, 8) and chk("training", 512, 1, target_size=512) == (512, 1)
    for kw, text in [(dict(frame_size=160), "--frame_size needs --frame training"), (dict(pool=8), "--pool needs --frame training"),
                     (dict(frame="scan", frame_size=160, pool=2), "--frame_size, --pool needs --frame training"),
                     (dict(frame="validation"), "--frame must be one of"), (dict(frame=True), "--frame must be one of"),
                     (dict(frame="training", frame_size=7), "--frame_size must be"), (dict(frame="training", frame_size=1025), "--frame_size must be"),
                     (dict(frame="training", frame_size=513, target_size=512), "--frame_size must be"),
                     (dict(frame="training", frame_size=160.0), "--frame_size must be"), (dict(frame="training", frame_size=True), "--frame_size must be"),
                     (dict(frame="training", pool=0), "--pool must be"), (dict(frame="training", pool=65), "--pool must be"),
                     (dict(frame="training", pool=2.5), "--pool must be")]:
        with pytest.raises(ValueError, match=re.escape(text)):
            chk(**kw)
    # what the frame says of a scan: the boundaries of nbc_training_frame's own check
    assert ev.frame_status(96, 128, 160) == ev.STATUS_OK and ev.frame_status(160, 160, 160) == ev.STATUS_OK
    assert ev.frame_status(54, 160, 160) == ev.STATUS_OK and ev.frame_status(53, 160, 160) == ev.STATUS_TOO_SMALL   # 54: p = 53 = L - 1; 53: p = 54 > L - 1
    assert ev.frame_status(40, 160, 160) == ev.STATUS_TOO_SMALL and ev.frame_status(160, 40, 160) == ev.STATUS_TOO_SMALL
    assert ev.frame_status(161, 100, 160) == ev.STATUS_TOO_LARGE and ev.frame_status(100, 161, 160) == ev.STATUS_TOO_LARGE
    assert ev.STATUS_TOO_SMALL not in ev.SKIP_REASONS and ev.TOO_SMALL == "too_small"


def test_report_names_too_small_only_with_the_flag():
    items = [dict(name="a.png", wood="sapin"), dict(name="b.png", wood="sapin"), dict(name="c.png", wood="sapin")]
    conf = [50, 3, 0, 4, 30, 1, 0, 2, 9]
    rows = np.array([[0, 9, 11, ev.STATUS_OK] + conf + conf, [1, 40, 160, ev.STATUS_TOO_SMALL] + [0] * 18,
                     [2, 9, 11, ev.STATUS_OK] + conf[::-1] + conf[::-1]], dtype=np.int64)
    _, summary = ev.report(items, rows, "fp32", "ckpt.pt", frame=True)
    assert summary["skipped"] == {"no_dual": [], "shape_mismatch": [], "too_large": [], "too_small": ["sapin/b.png"]}
    assert summary["images_evaluated"] == 2 and summary["images_skipped"] == 1
    _, plain = ev.report(items, rows[[0, 2]], "fp32", "ckpt.pt")
    assert sorted(plain["skipped"]) == ["no_dual", "shape_mismatch", "too_large"]
    doc = ev.frame_report(rows, 24, 8)
    from neuralbarkcalculator_amd import metrics
    want = metrics.pooled_over_groups([conf, conf[::-1]], [conf, conf[::-1]], 8)
    assert doc == dict(kind="training", size=24, resampled_rows=2, resampled_cols=2, **want) and len(doc["groups"]) == 1
    assert ev.frame_report(rows, 25, 1)["resampled_rows"] == 0 and len(ev.frame_report(rows, 25, 1)["groups"]) == 2
    text = ev.format_summary(dict(summary, frame=doc))
    assert "on the training's 24 x 24 frame" in text and "groups of 8" in text and "too_small: sapin/b.png" in text


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    root = tmp_path_factory.mktemp("listed")
    for wood, name in (("epinette_gelee", "a1.png"), ("epinette_gelee", "a2.png"), ("sapin", "s1.png")):
        os.makedirs(root / "samples" / wood, exist_ok=True)
        Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(root / "samples" / wood / name)
    return root


def test_subset_orders_the_list_and_quotes_an_unknown_line(listed, tmp_path):
    items = ev.list_labelled(str(listed))
    assert [d["wood"] + "/" + d["name"] for d in items] == ["epinette_gelee/a1.png", "epinette_gelee/a2.png", "sapin/s1.png"]
    path = tmp_path / "split.txt"
    path.write_text("sapin/s1.png\n\n  epinette_gelee/a1.png  \n")
    lines = ev.read_subset(str(path))
    assert lines == ["sapin/s1.png", "epinette_gelee/a1.png"]
    picked = ev.apply_subset(items, lines)
    assert [d["name"] for d in picked] == ["s1.png", "a1.png"] and picked[0] is items[2]
    assert ev.apply_subset(items, []) == []
    with pytest.raises(ValueError, match=re.escape("--subset: 'sapin/s9.png' names no listed sample")):
        ev.apply_subset(items, ["sapin/s1.png", "sapin/s9.png"])
    with pytest.raises(ValueError, match="named twice"):
        ev.apply_subset(items, ["sapin/s1.png", "sapin/s1.png"])
    # the library call refuses alike, before any device is touched
    with pytest.raises(ValueError, match="names no listed sample"):
        ev.evaluate_folder(str(listed), "/nonexistent/ckpt.pt", subset=["sapin/s9.png"])
    bad = tmp_path / "bad.txt"
    bad.write_text("epinette_gelee/a2.png\nsapin/nope.png\n")
    p = _cli(str(listed), "--subset", str(bad))
    assert p.returncode == 2 and "'sapin/nope.png' names no listed sample" in p.stderr, (p.returncode, p.stderr[-500:])
    p = _cli(str(listed), "--subset", str(tmp_path / "missing.txt"))
    assert p.returncode == 2 and "missing.txt" in p.stderr, (p.returncode, p.stderr[-500:])


def _cli(root, *argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", root] + list(argv), cwd=REPO, capture_output=True,
                          text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--frame_size", "160"], "--frame_size needs --frame training"),
                                       (["--pool", "8"], "--pool needs --frame training"),
                                       (["--frame", "scan", "--pool", "8"], "--pool needs --frame training"),
                                       (["--frame", "validation"], "--frame must be one of scan, training"),
                                       (["--frame", "training", "--frame_size", "7"], "--frame_size must be"),
                                       (["--frame", "training", "--frame_size", "1025"], "--frame_size must be"),
                                       (["--frame", "training", "--pool", "0"], "--pool must be"),
                                       (["--frame", "training", "--pool", "65"], "--pool must be")])
def test_evaluate_refuses_with_code_2(argv, text):
    p = _cli("/nonexistent/folder", *argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike(built_lib):
    for kw, text in [(dict(frame_size=160), "--frame_size needs"), (dict(pool=4), "--pool needs"), (dict(frame="test"), "--frame must be"),
                     (dict(frame="training", frame_size=2048), "--frame_size must be"), (dict(frame="training", pool=100), "--pool must be"),
                     (dict(frame="training", frame_size=600, target_size=512), "--frame_size must be")]:
        with pytest.raises(ValueError, match=text):
            ev.evaluate_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", **kw)
