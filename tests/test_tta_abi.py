"""The flip views (`--tta`) without a GPU: the C ABI's symbols, signatures and constants, every refusal in front of the
device, the numpy restatement of tests/helpers/tta_oracle.py against torch.flip and plain Python, the report arithmetic and
the command line's refusals."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib, folder_run
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd import predict as drv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tta_oracle as to  # noqa: E402
import vote_oracle as vo  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40


def test_symbols_signatures_and_constants(built_lib):
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for name in ("nbc_tta_views", "nbc_tta_merge", "nbc_vote_tally"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name) and ("int %s(" % name) in header
    assert _lib.SIGNATURES["nbc_tta_views"] == (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 2)
    assert _lib.SIGNATURES["nbc_tta_merge"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3)
    assert _lib.SIGNATURES["nbc_vote_tally"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p])
    flat = re.sub(r"\s+", " ", header)
    assert ("int nbc_tta_views(const void* x_dev, int x_dtype, int N, int H, int W, int views, void* out_dev, "
            "void* hip_stream);") in flat
    assert ("int nbc_tta_merge(const float* lowres_views_dev, int N, int h, int w, int views, float* merged_dev, "
            "float* aligned_dev, void* hip_stream);") in flat
    assert ("int nbc_vote_tally(const uint8_t* labels_dev, int N, int D, int H, int W, uint32_t* votes_dev, int accumulate, "
            "void* hip_stream);") in flat
    for name, value in (("IDENTITY", 1), ("HFLIP", 2), ("VFLIP", 4), ("HVFLIP", 8), ("FLIPS", 15)):
        assert re.search(r"NBC_TTA_%s = %d\b" % (name, value), header), name
        assert getattr(_lib, "TTA_" + name) == getattr(to, name) == value
    assert mdl.TTA_VIEWS == to.NAMED == {k: v for k, v in folder_run.TTA_MASKS.items() if k != "none"}
    assert [mdl.resolve_tta_views(v) for v in ("hflip", "vflip", "flips", 1, 10, 15)] == [3, 5, 15, 1, 10, 15]
    assert mdl.tta_view_names(10) == folder_run.tta_view_names(10) == ["hflip", "hvflip"] and mdl.tta_view_count(7) == 3
    for bad in (0, 16, -1, "none", "rot90", True, 1.5, None):
        with pytest.raises(ValueError):
            mdl.resolve_tta_views(bad)
    # nothing published about the votes has moved
    assert _lib.SIGNATURES["nbc_vote_summary"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4)


def _refused(rc, who, text):
    err = _lib.last_error()
    assert rc == _lib.NBC_ERR_INVALID and err.startswith(who + ":") and text in err, (rc, err, text)


def test_views_arguments_are_refused_before_the_device_is_touched(built_lib):
    def call(x=FAKE, dtype=_lib.IN_U8_NHWC, N=2, H=64, W=64, views=15, out=FAKE + (1 << 30)):
        return built_lib.nbc_tta_views(x, dtype, N, H, W, views, out, None)

    for kw, text in [(dict(x=None), "null argument"), (dict(out=None), "null argument"), (dict(dtype=2), "bad x_dtype"),
                     (dict(dtype=-1), "bad x_dtype"), (dict(views=0), "views must be"), (dict(views=16), "views must be"),
                     (dict(views=-1), "views must be"), (dict(N=0), "bad shape"), (dict(N=16384), "bad shape"),
                     (dict(N=65535, views=3), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"), (dict(W=-3), "bad shape"),
                     (dict(H=65536, W=32768), "bad shape"),
                     (dict(dtype=_lib.IN_F32_NCHW, x=FAKE + 2), "4-byte aligned"),
                     (dict(dtype=_lib.IN_F32_NCHW, out=FAKE + (1 << 30) + 1), "4-byte aligned"),
                     (dict(out=FAKE), "must not overlap"), (dict(out=FAKE + 100), "must not overlap"),
                     (dict(out=FAKE - 4 * 2 * 64 * 64 * 3 + 1), "must not overlap")]:
        _refused(call(**kw), "nbc_tta_views", text)


def test_merge_arguments_are_refused_before_the_device_is_touched(built_lib):
    def call(x=FAKE, N=2, h=8, w=8, views=15, merged=FAKE + (1 << 30), aligned=FAKE + (2 << 30)):
        return built_lib.nbc_tta_merge(x, N, h, w, views, merged, aligned, None)

    for kw, text in [(dict(x=None), "null argument"), (dict(merged=None), "null argument"), (dict(views=0), "views must be"),
                     (dict(views=16), "views must be"), (dict(N=0), "bad shape"), (dict(N=16384), "bad shape"), (dict(h=0), "bad shape"),
                     (dict(w=0), "bad shape"), (dict(h=65536, w=32768), "bad shape"), (dict(x=FAKE + 1), "4-byte aligned"),
                     (dict(merged=FAKE + (1 << 30) + 2), "4-byte aligned"), (dict(aligned=FAKE + (2 << 30) + 3), "4-byte aligned"),
                     (dict(aligned=FAKE), "must not alias"), (dict(aligned=FAKE + 8), "must not alias"),
                     (dict(merged=FAKE + 16), "must not overlap"), (dict(aligned=FAKE + (1 << 30)), "must not alias")]:
        _refused(call(**kw), "nbc_tta_merge", text)


def test_tally_arguments_are_refused_before_the_device_is_touched(built_lib):
    def call(labels=FAKE, N=2, D=4, H=64, W=64, votes=FAKE + (1 << 30), accumulate=0):
        return built_lib.nbc_vote_tally(labels, N, D, H, W, votes, accumulate, None)

    for kw, text in [(dict(labels=None), "null argument"), (dict(votes=None), "null argument"), (dict(N=0), "bad shape"),
                     (dict(N=65536), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"), (dict(H=65536, W=32768), "bad shape"),
                     (dict(D=0), "D must lie in 1..65535"), (dict(D=65536), "D must lie"), (dict(D=-2), "D must lie"),
                     (dict(votes=FAKE + (1 << 30) + 4), "16-byte aligned"), (dict(votes=FAKE + (1 << 30) + 8, accumulate=1), "16-byte aligned")]:
        _refused(call(**kw), "nbc_vote_tally", text)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_oracle_on_a_hand_made_case():
    # one 2 x 3 image; plain Python spells the four views out
    a = [[1, 2, 3], [4, 5, 6]]
    views = [a, [r[::-1] for r in a], a[::-1], [r[::-1] for r in a[::-1]]]
    x = np.zeros((1, 3, 2, 3), dtype=np.float32)
    for c in range(3):
        x[0, c] = np.array(a, dtype=np.float32) * (c + 1)
    s = to.stack(x, 15)
    assert s.shape == (4, 3, 2, 3)
    for j in range(4):
        for c in range(3):
            assert s[j, c].tolist() == [[v * (c + 1) for v in row] for row in views[j]]
    xt = torch.from_numpy(x)
    assert torch.equal(torch.from_numpy(s), torch.cat([xt, torch.flip(xt, [3]), torch.flip(xt, [2]), torch.flip(xt, [2, 3])]))
    assert np.array_equal(to.stack(x, 10), s[[1, 3]]) and np.array_equal(to.stack(x, 1), x) and to.view_bits(5) == [0, 2]
    u8 = np.arange(2 * 2 * 3 * 3, dtype=np.uint8).reshape(2, 2, 3, 3)                    # [N,H,W,3]: pixels are mirrored, not bytes
    su = to.stack(u8, 3)
    assert su.shape == (4, 2, 3, 3) and su[2, 0, 0].tolist() == u8[0, 0, 2].tolist() and su[3, 1, 2].tolist() == u8[1, 1, 0].tolist()
    ut = torch.from_numpy(u8)
    assert torch.equal(torch.from_numpy(to.stack(u8, 15)), torch.cat([ut, torch.flip(ut, [2]), torch.flip(ut, [1]), torch.flip(ut, [1, 2])]))
    # un-flipping the stack gives the image back in every view: a flip is its own inverse
    al = to.align(s, 1, 15)
    assert al.shape == (4, 1, 3, 2, 3) and all(np.array_equal(al[j, 0], x[0]) for j in range(4))
    # the mean in the stated order, each operation rounded to f32: (((a0 + a1) + a2) + a3) / 4, and / 3 for three views
    vals = [np.float32(v) for v in (1e8, 1.0, -1e8, 3.0)]
    stackv = np.array(vals, dtype=np.float32).reshape(4, 1, 1, 1, 1)
    want4 = np.float32(np.float32(np.float32(np.float32(vals[0] + vals[1]) + vals[2]) + vals[3]) / np.float32(4))
    assert to.merge(stackv)[0, 0, 0, 0] == want4 == np.float32(0.75)                     # 1e8 + 1 rounds to 1e8: order matters
    want3 = np.float32(np.float32(np.float32(vals[1] + vals[3]) + vals[3]) / np.float32(3))
    got3 = to.merge(np.array([vals[1], vals[3], vals[3]], dtype=np.float32).reshape(3, 1, 1, 1, 1))[0, 0, 0, 0]
    assert got3 == want3
    one = np.array([-0.0], dtype=np.float32).reshape(1, 1, 1, 1, 1)
    assert np.signbit(to.merge(one)[0, 0, 0, 0])                                        # V = 1: the view's own bits
    assert np.isnan(to.merge(np.array([1.0, np.nan], dtype=np.float32).reshape(2, 1, 1, 1, 1))[0, 0, 0, 0])
    assert np.isnan(to.merge(np.array([np.inf, -np.inf], dtype=np.float32).reshape(2, 1, 1, 1, 1))[0, 0, 0, 0])
    # the views' own figures: D = V through vote_oracle
    labels = np.array([[[[0, 1, 2, 1]]], [[[0, 1, 2, 2]]], [[[0, 1, 1, 0]]], [[[0, 1, 0, 0]]]], dtype=np.uint8)     # [V=4, N=1, 1, 4]
    counts, support, stats = to.view_figures(labels)
    assert counts.tolist() == [[[1, 2, 1]], [[1, 1, 2]], [[2, 2, 0]], [[3, 1, 0]]]
    assert support.tolist() == [[[255, 255, 127, 127]]] and np.array_equal(stats, vo.stats(vo.tally(labels), 4))
    assert stats.tolist() == [[2, 1, 1, 1, 1, 0, 12, 0, 6, 3]]


# ---- the report ----------------------------------------------------------------------------------------------------------------
def _f(v):
    return "{:.5f}".format(v)


def test_tta_report_on_hand_made_counts():
    h, w = 129, 65
    px = h * w
    mc = [px - 900 - 30, 900, 30]
    vc = [[px - 1000 - 20, 1000, 20], [px - 800 - 50, 800, 50], [px - 950 - 30, 950, 30], [px - 870 - 0, 870, 0]]
    st = [px - 900, 880, 20, px - 2000, 500, 10, 4 * px - 3333, 0, 3620, 100]
    images = [("a.png", "sapin", h, w, mc, vc, st), ("b.png", "epinette_gelee", 16, 16, [256, 0, 0], np.array([[256, 0, 0]] * 4), [256, 0, 0, 256, 0, 0, 1024, 0, 0, 0])]
    table, summary = folder_run.tta_report(images, 15)
    assert table[0] == ["Name", "Type", "Views", "identity Bark %", "identity Node %", "hflip Bark %", "hflip Node %", "vflip Bark %",
                        "vflip Node %", "hvflip Bark %", "hvflip Node %", "Bark %", "Node %", "Bark % spread", "Node % spread",
                        "Unanimous %", "Mean support"]
    a, b = table[1], table[2]
    assert a[:3] == ["a.png", "sapin", "identity+hflip+vflip+hvflip"]
    for j in range(4):
        assert a[3 + 2 * j: 5 + 2 * j] == [folder_run.percent_string(vc[j][1], px), folder_run.percent_string(vc[j][2], px)]
    assert a[11:13] == [drv.stats_row("a.png", "sapin", h, w, 900, 30)[i] for i in (2, 4)]
    assert a[13] == _f(float(Fraction(100 * 200, px))) and a[14] == _f(float(Fraction(100 * 50, px)))
    assert a[15] == _f(float(Fraction(100 * (px - 2000 + 510), px))) and a[16] == _f(float(Fraction(4 * px - 3333, 4 * px)))
    assert b[3:] == ["0.00000"] * 12 + ["100.00000", "1.00000"]
    assert summary["images"] == 2 and summary["views"] == ["identity", "hflip", "vflip", "hvflip"]
    m = summary["means"]
    assert set(m) == {"merged_bark", "merged_node", "identity_bark", "identity_node", "abs_diff_bark", "abs_diff_node", "bark_spread",
                      "node_spread", "unanimous", "mean_support"}
    assert m["merged_bark"] == float(Fraction(100 * 900, px)) / 2 and m["identity_node"] == float(Fraction(100 * 20, px)) / 2
    assert m["abs_diff_bark"] == float(Fraction(100 * 100, px)) / 2 and m["abs_diff_node"] == float(Fraction(100 * 10, px)) / 2
    assert m["bark_spread"] == float(Fraction(100 * 200, px)) / 2 and m["unanimous"] == (float(Fraction(100 * (px - 1490), px)) + 100.0) / 2
    # two views; a mask without the identity view has no identity pair
    t2, s2 = folder_run.tta_report([("a.png", "sapin", h, w, mc, vc[:2], st)], 3)
    assert t2[0][3:7] == ["identity Bark %", "identity Node %", "hflip Bark %", "hflip Node %"] and len(t2[1]) == 13
    assert t2[1][12] == _f(float(Fraction(4 * px - 3333, 2 * px)))
    t3, s3 = folder_run.tta_report([("a.png", "sapin", h, w, mc, vc[:2], st)], 10)
    assert "identity_bark" not in s3["means"] and s3["views"] == ["hflip", "hvflip"]
    # the empty folder
    assert folder_run.tta_report([], 15) == ([folder_run.tta_columns(15)], {"images": 0, "views": ["identity", "hflip", "vflip", "hvflip"], "means": {}})


def test_report_files(tmp_path):
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}]
    allrows = np.array([[0, 16, 16, 100, 5], [1, 16, 32, 200, 9]], dtype=np.int64)
    allt = np.array([[1, 303, 200, 9] + [300, 205, 7, 310, 195, 11] + [310, 195, 7, 300, 190, 5, 1010, 0, 400, 18],
                     [0, 151, 100, 5] + [150, 101, 5, 152, 99, 5] + [150, 101, 5, 148, 99, 5, 510, 0, 200, 10]], dtype=np.int64)
    s = drv.write_tta_report(str(tmp_path), items, allrows, allt, 3, "fp32", "running")
    assert sorted(os.listdir(tmp_path)) == ["tta_stats.csv", "tta_summary.json"]
    import csv
    import json
    rows = list(csv.reader(open(tmp_path / "tta_stats.csv"), delimiter="\t"))
    want, wsum = folder_run.tta_report([("a.png", "sapin", 16, 16, [151, 100, 5], [[150, 101, 5], [152, 99, 5]], allt[1, 10:]),
                                        ("b.png", "sapin", 16, 32, [303, 200, 9], [[300, 205, 7], [310, 195, 11]], allt[0, 10:])], 3)
    assert rows == want
    doc = json.load(open(tmp_path / "tta_summary.json"))
    assert doc == json.loads(json.dumps(s)) and doc["precision"] == "fp32" and doc["bn_stats"] == "running"
    assert doc["views"] == ["identity", "hflip"] and doc["means"] == json.loads(json.dumps(wsum["means"])) and doc["images"] == 2


# ---- the command line and the library keywords -----------------------------------------------------------------------------
def _cli(module, *argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd." + module, "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--tta", "flips", "--dropout_draws", "4"], "--tta cannot go with --dropout_draws"),
                                       (["--tta", "hflip", "--only_preprocess"], "--tta runs the network"),
                                       (["--tta_votes"], "--tta_votes needs --tta"),
                                       (["--tta_votes", "--tta", "none"], "--tta_votes needs --tta"),
                                       (["--tta", "rot90"], "invalid choice")])
def test_predict_refuses_with_code_2(argv, text):
    p = _cli("predict", *argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_evaluate_refuses_an_unknown_view_set_with_code_2():
    p = _cli("evaluate", "--tta", "rot90")
    assert p.returncode == 2 and "invalid choice" in p.stderr, (p.returncode, p.stderr[-500:])
    p = _cli("evaluate", "--tta_votes")                              # predict only
    assert p.returncode == 2 and "unrecognized arguments" in p.stderr


def test_library_keywords_are_refused_alike(built_lib):
    with pytest.raises(ValueError, match="--tta_votes needs --tta"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", tta_votes=True)
    with pytest.raises(ValueError, match="cannot go with --dropout_draws"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", tta="flips", dropout_draws=4)
    with pytest.raises(ValueError, match="--tta must be one of"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", tta="rot90")
    from neuralbarkcalculator_amd import evaluate as ev
    with pytest.raises(ValueError, match="--tta must be one of"):
        ev.evaluate_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", tta="rot90")
    assert folder_run.check_tta_arguments("none") == folder_run.check_tta_arguments(None) == 0
    assert folder_run.check_tta_arguments("flips", True) == 15 and folder_run.check_tta_arguments("vflip") == 5
    with pytest.raises(ValueError, match="--only_preprocess"):
        folder_run.check_tta_arguments("hflip", only_preprocess=True)
    m = mdl.FCNResNet50("fp32")
    with pytest.raises(RuntimeError):                              # no device, no weights
        m.predict_labels_tta(torch.zeros((1, 3, 64, 64)))
    with pytest.raises(RuntimeError):
        m.tta_views(torch.zeros((1, 3, 64, 64)))


def test_stacked_predicts_refuse_their_common_arguments_alike(built_lib, monkeypatch):
    """predict_labels_tta, predict_labels_jitter and predict_labels_windows word the refusals of the arguments they share the
    same way, before anything reaches a device: the batch check is stood in for, so no context is needed."""
    m = mdl.FCNResNet50("fp32")
    m.device = torch.device("cpu")
    x = torch.zeros((1, 64, 64, 3), dtype=torch.uint8)
    calls = [("views", 4, lambda **kw: m.predict_labels_tta(x, "flips", **kw)),
             ("views", 5, lambda **kw: m.predict_labels_jitter(x, "training", **kw)),
             ("windows", 9, lambda **kw: m.predict_labels_windows(x, 32, 16, **kw))]       # 64 x 64 in windows of 32 every 16: 3 x 3
    for what, count, call in calls:
        monkeypatch.setattr(m, "_check_input", lambda x: (2, 64, 64))
        for kw, text in [(dict(labels_dtype=torch.int32), "labels_dtype must be torch.int64 or torch.uint8"),
                         (dict(min_pixels=-1), "min_pixels must not be negative"),
                         (dict(logits_full=torch.zeros((2, 3, 64, 32))), "logits_full must be a contiguous float32 [2,3,64,64] tensor on cpu"),
                         (dict(logits_full=torch.zeros((2, 3, 64, 64), dtype=torch.float64)),
                          "logits_full must be a contiguous float32 [2,3,64,64] tensor on cpu"),
                         (dict(logits_full=torch.zeros((2, 3, 64, 128))[..., ::2]),
                          "logits_full must be a contiguous float32 [2,3,64,64] tensor on cpu")]:
            with pytest.raises(ValueError) as e:
                call(**kw)
            assert str(e.value) == text, (what, kw)
        n = 65535 // count + 1
        monkeypatch.setattr(m, "_check_input", lambda x: (n, 64, 64))
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "the stack of %d %s of %d images exceeds 65535 entries" % (count, what, n)
        with pytest.raises(ValueError) as e:                          # the order of the refusals
            call(labels_dtype=torch.float32, min_pixels=-1, logits_full=x)
        assert str(e.value) == "labels_dtype must be torch.int64 or torch.uint8"
        with pytest.raises(ValueError) as e:
            call(min_pixels=-1, logits_full=x)
        assert str(e.value) == "min_pixels must not be negative"


def test_folders_of_the_support_only_with_the_flag(tmp_path):
    for tag, on in (("off", False), ("on", True)):
        root = tmp_path / tag
        (root / "samples" / "sapin").mkdir(parents=True)
        drv.generate_folders(str(root), tta_votes=on)
        assert sorted(os.listdir(root / "results")) == sorted(["combined_images", "outputs"] + (["tta_support"] if on else []))
