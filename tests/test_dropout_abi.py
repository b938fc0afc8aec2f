"""The Dropout draws (`predict --dropout_draws`) without a GPU: Philox against its known answers, the host mask entry point
against the numpy restatement (tests/helpers/dropout_oracle.py), the extremes of p, the drop rate, the restatement against
the CPU oracle, the C ABI's symbols / workspace formula / argument checks, and the driver's identities, refusals, report
arithmetic and compare reader."""
import ctypes as C
import csv
import math
import os
import statistics
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib, folder_run
from neuralbarkcalculator_amd import predict as drv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dropout_oracle as do  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [folder_run.image_id("sapin", "a.png"), folder_run.image_id("epinette_gelee", "EPN 9 A.png")]
COMBOS = [(seed, iid, draw) for seed in (0, 42) for iid in IDS for draw in (0, 31)]     # the eight of the issue
IMAGE_ELEMENTS = 128 * 128 * 512


def lib_mask(lib, seed, iid, draw, p, first, count):
    out = np.full(count + 2, 7, dtype=np.uint8)          # two guard bytes behind the flags
    rc = lib.nbc_dropout_mask(seed, iid, draw, p, first, count, out.ctypes.data)
    assert rc == _lib.NBC_OK, _lib.last_error()
    assert out[count] == 7 and out[count + 1] == 7
    return out[:count]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = do.philox4x32_10(ctr, key)
        assert " ".join("%08x" % int(v) for v in got) == want
    # vectorised over the first counter word = one call per value
    many = do.philox4x32_10((np.arange(5, dtype=np.uint64), 3, 2, 1), (9, 8))
    for q in range(5):
        assert np.array_equal(many[q], do.philox4x32_10((q, 3, 2, 1), (9, 8)))


def test_threshold_and_scale():
    assert do.threshold(0.1) == 429496729 and do.threshold(0.0) == 0 and do.threshold(0.5) == 1 << 31
    assert do.keep_scale(0.0) == np.float32(1.0) and do.keep_scale(0.5) == np.float32(2.0)
    assert do.keep_scale(0.1) == np.float32(1.0) / np.float32(0.9)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_mask_parity_with_the_restatement(built_lib, p):
    for seed, iid, draw in COMBOS:
        for first, count in ((0, 4096), (1, 1), (2, 5), (3, 1030), (511, 514), (4 * 9999 + 3, 2)):   # starts inside a quad
            want = do.keep_flags(seed, iid, draw, p, first, count)
            got = lib_mask(built_lib, seed, iid, draw, p, first, count)
            assert np.array_equal(got, want), (seed, hex(iid), draw, p, first, count)
    # high quad indices and the upper half of a 64-bit identity and seed reach the counter and the key
    big_id, big_seed = 0xfedcba9876543210, 0x8000000000000001
    first = (1 << 33) + 1
    assert np.array_equal(lib_mask(built_lib, big_seed, big_id, 5, 0.5, first, 64), do.keep_flags(big_seed, big_id, 5, 0.5, first, 64))
    a = lib_mask(built_lib, big_seed, big_id, 5, 0.5, 0, 4096)
    assert not np.array_equal(a, lib_mask(built_lib, big_seed, big_id & 0xffffffff, 5, 0.5, 0, 4096))
    assert not np.array_equal(a, lib_mask(built_lib, big_seed & 0xffffffff, big_id, 5, 0.5, 0, 4096))
    assert not np.array_equal(a, lib_mask(built_lib, big_seed, big_id, 6, 0.5, 0, 4096))


def test_extremes_of_p(built_lib):
    assert lib_mask(built_lib, 42, IDS[0], 0, 0.0, 0, 1 << 16).all()          # p = 0 keeps everything
    top = (2.0 ** 32 - 1) / 2.0 ** 32                                        # the largest T: 2^32 - 1
    assert do.threshold(top) == 2 ** 32 - 1 and do.threshold(math.nextafter(1.0, 0.0)) == 2 ** 32 - 1
    got = lib_mask(built_lib, 42, IDS[0], 0, top, 0, 1 << 16)
    assert np.array_equal(got, do.keep_flags(42, IDS[0], 0, top, 0, 1 << 16)) and got.sum() <= 1
    out = np.zeros(4, np.uint8)
    for bad in (1.0, 1.5, -1e-9, float("nan"), float("inf")):
        assert built_lib.nbc_dropout_mask(0, 0, 0, bad, 0, 4, out.ctypes.data) == _lib.NBC_ERR_INVALID, bad
        assert _lib.last_error().startswith("nbc_dropout_mask:")
    assert built_lib.nbc_dropout_mask(0, 0, -1, 0.1, 0, 4, out.ctypes.data) == _lib.NBC_ERR_INVALID
    assert built_lib.nbc_dropout_mask(0, 0, 0, 0.1, 0, 4, None) == _lib.NBC_ERR_INVALID
    assert built_lib.nbc_dropout_mask(0, 0, 0, 0.1, 0, 0, None) == _lib.NBC_OK


@pytest.mark.parametrize("seed,iid,draw", COMBOS)
def test_drop_rate_within_five_sigma(built_lib, seed, iid, draw):
    """128 x 128 x 512 elements of one image at p = 0.1: sigma = sqrt(0.09 / 8 388 608) = 1.04e-4.  The cap is a condition
    (a binomial proportion), not a measurement."""
    sigma = math.sqrt(0.1 * 0.9 / IMAGE_ELEMENTS)
    keep = lib_mask(built_lib, seed, iid, draw, 0.1, 0, IMAGE_ELEMENTS)
    dropped = 1.0 - float(keep.sum(dtype=np.int64)) / IMAGE_ELEMENTS
    z = (dropped - do.threshold(0.1) / 2.0 ** 32) / sigma
    print("dropout drop rate seed %d id %016x draw %d: %.6f (%+.2f sigma)" % (seed, iid, draw, dropped, z))
    assert abs(z) <= 5.0, (dropped, z)
    # the restatement on a slice of the same image
    assert np.array_equal(keep[123457:123457 + 70001], do.keep_flags(seed, iid, draw, 0.1, 123457, 70001))


def test_restatement_against_the_cpu_oracle(oracle_model, sd_np):
    from neuralbarkcalculator_amd import synth
    x = torch.from_numpy(np.stack([synth.make_input(3, 64, 96), synth.make_input(4, 64, 96)]))
    feats = do.features(oracle_model, x)
    n, c, h, w = feats.shape
    assert (c, h, w) == (512, 8, 12)
    with torch.no_grad():
        want = oracle_model.lowres_logits(x)
    # all-keep: p = 0, and an all-true mask at p = 0
    assert torch.equal(do.draw_lowres(oracle_model, feats, IDS, 42, 0, 0.0), want)
    assert torch.equal(do.masked_lowres(oracle_model, feats, np.ones(feats.shape, bool), 0.0), want)
    # a random mask: classifier[4](features * keep * m) by hand
    keep = np.stack([do.keep_image(42, IDS[i], 31, 0.1, h, w) for i in range(n)])
    assert 0.05 < 1.0 - keep.mean() < 0.15
    got = do.draw_lowres(oracle_model, feats, IDS, 42, 31, 0.1)
    m = torch.tensor(float(do.keep_scale(0.1)), dtype=torch.float32)
    hand = torch.nn.functional.conv2d(feats * torch.from_numpy(keep).to(torch.float32) * m,
                                      torch.from_numpy(sd_np["classifier.4.weight"]), torch.from_numpy(sd_np["classifier.4.bias"]))
    assert torch.equal(got, hand)
    assert float((got - want).abs().max()) > 1e-3 * float(want.abs().max())          # the mask is live
    l64, mag = do.by_hand(sd_np["classifier.4.weight"], sd_np["classifier.4.bias"], feats.numpy(), keep, 0.1)
    assert float(np.abs(got.numpy() - l64).max()) <= 600 * 2.0 ** -24 * float(mag.max())   # f32 sums of 512 terms, any order
    # element order: pixel-major, channel-minor
    flat = do.keep_flags(42, IDS[1], 31, 0.1, 0, h * w * 512)
    assert bool(keep[1, 7, 2, 5]) == bool(flat[(2 * w + 5) * 512 + 7])


def _a256(x):
    return (x + 255) // 256 * 256


def _want_bytes(n, hh, ww, d):
    h, w = (hh + 7) // 8, (ww + 7) // 8
    i = d * n
    return _a256(12 * i * h * w) + _a256(i * hh * ww) + 2 * _a256(4 * i * hh * ww) + _a256(i * hh * ww)


def test_symbols_signatures_and_workspace_formula(built_lib):
    for name in ("nbc_dropout_mask", "nbc_dropout_workspace_bytes", "nbc_dropout_draws"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name)
    assert _lib.SIGNATURES["nbc_dropout_mask"] == (C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_double, C.c_uint64, C.c_size_t,
                                                             C.c_void_p])
    assert _lib.SIGNATURES["nbc_dropout_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    res, args = _lib.SIGNATURES["nbc_dropout_draws"]
    assert res is C.c_int and len(args) == 16 and args[5] is C.c_double and args[6] is C.c_uint64 and args[14] is C.c_size_t
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for name in ("nbc_dropout_mask", "nbc_dropout_workspace_bytes", "nbc_dropout_draws"):
        assert ("int %s(" % name) in header or ("size_t %s(" % name) in header
    for n, hh, ww, d in [(1, 1024, 1024, 1), (1, 1024, 1024, 8), (2, 256, 256, 3), (2, 203, 317, 1024), (1, 8, 8, 1),
                         (3, 600, 1024, 32)]:
        hl, wl = C.c_int(), C.c_int()
        assert built_lib.nbc_lowres_size(hh, ww, C.byref(hl), C.byref(wl)) == 0
        assert (hl.value, wl.value) == ((hh + 7) // 8, (ww + 7) // 8)
        assert built_lib.nbc_dropout_workspace_bytes(n, hh, ww, d) == _want_bytes(n, hh, ww, d) > 0, (n, hh, ww, d)
    for n, hh, ww, d in [(0, 64, 64, 1), (1, 7, 64, 1), (1, 64, 7, 1), (1, 64, 64, 0), (64, 64, 64, 1024), (1, 65536, 64, 1),
                         (1, 65535, 65535, 1)]:
        assert built_lib.nbc_dropout_workspace_bytes(n, hh, ww, d) == 0, (n, hh, ww, d)


def test_draws_arguments_are_refused_before_the_device_is_touched(built_lib):
    """No context exists on a machine without a GPU: every refusal below comes from the argument checks in front of it."""
    fake = 1 << 40
    ids = (C.c_uint64 * 2)(1, 2)

    def call(ctx=None, N=2, H=64, W=64, ids_=ids, p=0.1, seed=0, first=0, draws=4, minpx=150, lowres=None, counts=fake, ws=fake,
             ws_bytes=1 << 30):
        return built_lib.nbc_dropout_draws(ctx, N, H, W, ids_, p, seed, first, draws, minpx, 0, lowres, counts, ws, ws_bytes, None)

    for kw, text in [(dict(p=1.0), "p must lie in [0, 1)"), (dict(p=-0.1), "p must lie"), (dict(p=float("nan")), "p must lie"),
                     (dict(draws=0), "draws must lie in 1..1024"), (dict(draws=1025), "draws must lie"),
                     (dict(first=-1), "first_draw"), (dict(first=2 ** 31 - 2), "first_draw"), (dict(minpx=-1), "min_pixels"),
                     (dict(), "null argument")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        err = _lib.last_error()
        assert err.startswith("nbc_dropout_draws:") and text in err, (kw, err)


def test_image_id_is_fnv1a_64():
    assert folder_run.image_id("sapin", "a.png") == 0x57c5cd64a6eb00c9
    assert folder_run.image_id("", "") == ((0xcbf29ce484222325 ^ 0x2f) * 0x100000001b3) % 2 ** 64      # one byte: "/"
    assert folder_run.image_id("sapin", "a.png") != folder_run.image_id("sapin", "b.png")
    assert 0 <= folder_run.image_id("\u00e9pinette", "\u00f1.png") < 2 ** 64                            # UTF-8 bytes


def _cli(*argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [
    (["--dropout_draws", "4", "--arch", "deeplabv3_resnet50"], "DeepLabHead's Dropout sits inside ASPP"),
    (["--dropout_draws", "4", "--arch", "fcn_efficientnet_b0"], "EfficientNet's FCN head is left out"),
    (["--dropout_draws", "0"], "1..1024"), (["--dropout_draws", "1025"], "1..1024"), (["--dropout_draws", "-3"], "1..1024"),
    (["--dropout_draws", "4", "--dropout_p", "1.0"], "[0, 1)"), (["--dropout_draws", "4", "--dropout_p", "-0.5"], "[0, 1)"),
    (["--dropout_compare", "old.csv"], "needs --dropout_draws"), (["--dropout_p", "0.2"], "needs --dropout_draws"),
    (["--dropout_seed", "5"], "needs --dropout_draws"),
    (["--dropout_draws", "4", "--only_preprocess"], "--only_preprocess"),
])
def test_argument_refusals_exit_with_code_2(argv, text):
    p = _cli(*argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike():
    for kw in (dict(dropout_draws=2000), dict(dropout_draws=4, dropout_p=1.0), dict(dropout_draws=4, arch="deeplabv3_resnet50")):
        with pytest.raises(ValueError):
            drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", **kw)
    with pytest.raises(ValueError):
        folder_run.check_dropout_arch("deeplabv3_efficientnet_b3")
    folder_run.check_dropout_arch("fcn_resnet50")
    folder_run.check_dropout_arguments(None)
    folder_run.check_dropout_arguments(1024, 0.0, 2 ** 64 - 1, "x.csv", "auto")


def _f(v):
    return "{:.5f}".format(v)


def test_report_arithmetic_on_crafted_counts():
    px = 200 * 256
    dc = [[px - 1000 - 10, 1000, 10], [px - 1300 - 40, 1300, 40], [px - 1100 - 10, 1100, 10], [px - 1250 - 0, 1250, 0]]
    images = [("a.png", "sapin", 200, 256, 1111, 22, dc)]
    table, summary = folder_run.dropout_report(images, 4)
    assert table[0] == ["Name", "Type", "Output Bark %", "Output Node %", "bark_mean", "bark_std", "bark_min", "bark_max",
                        "node_mean", "node_std", "node_min", "node_max", "draws"]
    row = table[1]
    assert row[:4] == ["a.png", "sapin"] + [drv.stats_row("a.png", "sapin", 200, 256, 1111, 22)[i] for i in (2, 4)]
    for col, base in ((1, 4), (2, 8)):
        pct = [Fraction(100 * d[col], px) for d in dc]
        assert row[base] == _f(float(sum(pct) / 4))
        assert row[base + 1] == _f(math.sqrt(float(statistics.variance(pct))))           # unbiased (n - 1), exact rational
        assert row[base + 2] == _f(float(min(pct))) and row[base + 3] == _f(float(max(pct)))
    assert row[12] == "4" and len(row) == 13
    assert summary["draws"] == 4 and summary["images"] == 1
    assert abs(summary["means"]["bark_mean"] - 100 * 1162.5 / px) < 1e-12
    st = folder_run.draw_statistics([d[1] for d in dc], px)
    assert st["mean"] == 100 * 4650 / (4 * px) and st["min"] == 100 * 1000 / px and st["max"] == 100 * 1300 / px

    # one draw: the std is empty
    t1, s1 = folder_run.dropout_report([("a.png", "sapin", 200, 256, 1111, 22, dc[:1])], 1)
    assert t1[1][5] == "" and t1[1][9] == "" and t1[1][4] == _f(100 * 1000 / px) and "bark_std" not in s1["means"]
    # equal counts (what p = 0 gives): std 0, mean = the deterministic percentage
    eq = [[px - 1111 - 22, 1111, 22]] * 5
    t5, _ = folder_run.dropout_report([("a.png", "sapin", 200, 256, 1111, 22, eq)], 5)
    assert t5[1][5] == "0.00000" and t5[1][9] == "0.00000"
    assert t5[1][4] == t5[1][6] == t5[1][7] == _f(100 * 1111 / px) == t5[1][2]


def test_compare_reader_and_columns(tmp_path):
    """The shipped tool's file: seven header names over six columns per row; rows are read by position."""
    old = tmp_path / "old_final_stats.csv"
    px = 256 * 256
    rows = [drv.stats_row("a.png", "sapin", 256, 256, 1200, 30), drv.stats_row("b.png", "sapin", 256, 256, 9000, 500)]
    assert len(drv.CSV_HEADER) == 7 and all(len(r) == 6 for r in rows)
    drv.write_stats_csv(str(old), rows)
    got = folder_run.read_shipped_stats(str(old))
    assert got == {("a.png", "sapin"): (float(rows[0][2]), float(rows[0][4])), ("b.png", "sapin"): (float(rows[1][2]), float(rows[1][4]))}
    dca = [[px - 1230, 1200, 30], [px - 1300, 1250, 50], [px - 1120, 1100, 20]]     # a: old values are draw 0's: inside
    dcb = [[px - 8000, 7900, 100], [px - 8200, 8000, 200], [px - 8100, 7950, 150]]  # b: old values above every draw
    dcc = [[px - 3, 2, 1]] * 3                                                      # c: not in the old file
    images = [("a.png", "sapin", 256, 256, 1190, 28, dca), ("b.png", "sapin", 256, 256, 7990, 140, dcb),
              ("c.png", "epinette_gelee", 256, 256, 2, 1, dcc)]
    table, summary = folder_run.dropout_report(images, 3, got)
    assert table[0][13:] == ["old_bark", "old_node", "bark_inside", "node_inside", "bark_z", "node_z"]
    a, b, c = table[1], table[2], table[3]
    assert a[13:17] == [_f(float(rows[0][2])), _f(float(rows[0][4])), "1", "1"]
    sa = folder_run.draw_statistics([d[1] for d in dca], px)
    assert a[17] == _f((float(rows[0][2]) - sa["mean"]) / sa["std"])
    assert b[15:17] == ["0", "0"] and float(b[17]) > 0 and float(b[18]) > 0
    assert c[13:] == [""] * 6 and c[5] == "0.00000"
    assert summary["compare"] == {"images_compared": 2, "bark_inside": 1, "node_inside": 1,
                                  "missing_from_old": ["epinette_gelee/c.png"]}
    # std 0: no z score
    t0, _ = folder_run.dropout_report([("a.png", "sapin", 256, 256, 1200, 30, [dca[0]] * 2)], 2, got)
    assert t0[1][15:] == ["1", "1", "", ""]
    with pytest.raises(ValueError):
        folder_run.read_shipped_stats(str(tmp_path / "missing.csv"))
    bad = tmp_path / "bad.csv"
    bad.write_text("Name\tType\nx\ty\n")
    with pytest.raises(ValueError):
        folder_run.read_shipped_stats(str(bad))


def test_report_files(tmp_path):
    import json
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}]
    allrows = np.array([[0, 16, 16, 100, 5], [1, 16, 32, 200, 9]], dtype=np.int64)
    alld = np.array([[1, 300, 200, 12, 310, 190, 12], [0, 150, 101, 5, 152, 99, 5]], dtype=np.int64)   # any order
    s = drv.write_dropout_report(str(tmp_path), items, allrows, alld, 2, 0.1, 42, "f16x2", "running")
    rows = list(csv.reader(open(tmp_path / "dropout_stats.csv"), delimiter="\t"))
    assert rows[0] == folder_run.DROPOUT_COLUMNS and [r[0] for r in rows[1:]] == ["a.png", "b.png"]
    assert rows[1][6:8] == [_f(100 * 99 / 256), _f(100 * 101 / 256)] and rows[2][12] == "2"
    doc = json.load(open(tmp_path / "dropout_summary.json"))
    assert doc == json.loads(json.dumps(s))
    assert (doc["p"], doc["seed"], doc["draws"], doc["precision"], doc["bn_stats"], doc["images"]) == (0.1, 42, 2, "f16x2", "running", 2)
    assert set(doc["means"]) == {"%s_%s" % (c, k) for c in ("bark", "node") for k in ("mean", "std", "min", "max")}


def test_other_networks_refuse_the_draws_with_their_reasons(built_lib):
    from neuralbarkcalculator_amd.model import DeepLabV3EfficientNet, DeepLabV3ResNet50, FCNEfficientNet, FCNResNet50
    with pytest.raises(ValueError, match="DeepLabHead's Dropout sits inside ASPP"):
        DeepLabV3ResNet50("fp32").dropout_draws(4, [1])
    for cls in (FCNEfficientNet, DeepLabV3EfficientNet):
        with pytest.raises(ValueError, match="EfficientNet's FCN head is left out"):
            cls(0).dropout_draws(4, [1])
    m = FCNResNet50("fp32")
    for kw in (dict(draws=0), dict(draws=1025), dict(draws=1, p=1.0), dict(draws=1, p=-0.1), dict(draws=1, first_draw=-1),
               dict(draws=1, seed=-1), dict(draws=1, seed=2 ** 64)):
        with pytest.raises(ValueError):
            m.dropout_draws(image_ids=[1], **kw)
    with pytest.raises(RuntimeError):                       # no device, no weights, no forward
        m.dropout_draws(1, [1])
