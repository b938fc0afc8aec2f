"""The per-pixel votes of the Dropout draws (`predict --dropout_draws D --dropout_votes`) without a GPU: the C ABI's symbols and
signatures, the definition (nbc_vote_decode against the numpy restatement of tests/helpers/vote_oracle.py, exhaustively, and
the spelled-out ties), the refusals in front of the device, the report arithmetic and the command line's refusals."""
import ctypes as C
import csv
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from neuralbarkcalculator_amd import _lib, folder_run
from neuralbarkcalculator_amd import predict as drv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import vote_oracle as vo  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def word(n1, n2):
    return (n2 << 16) | n1


def lib_decode(lib, w, draws):
    label, support = C.c_uint8(77), C.c_uint8(77)
    assert lib.nbc_vote_decode(w, draws, C.byref(label), C.byref(support)) == _lib.NBC_OK, _lib.last_error()
    return label.value, support.value


def test_symbols_and_signatures(built_lib):
    for name in ("nbc_vote_decode", "nbc_dropout_votes", "nbc_vote_summary"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name)
    assert _lib.SIGNATURES["nbc_vote_decode"] == (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)])
    res, args = _lib.SIGNATURES["nbc_dropout_votes"]
    draws_args = _lib.SIGNATURES["nbc_dropout_draws"][1]
    # nbc_dropout_draws' arguments with (votes_dev, accumulate) in front of the workspace
    assert res is C.c_int and len(args) == 18 and args[:13] == draws_args[:13] and args[13] is C.c_void_p and args[14] is C.c_int
    assert args[15:] == draws_args[13:]
    assert _lib.SIGNATURES["nbc_vote_summary"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4)
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    for name in ("nbc_vote_decode", "nbc_dropout_votes", "nbc_vote_summary"):
        assert ("int %s(" % name) in header
    assert "#define NBC_VOTE_STATS 10" in header and _lib.VOTE_STATS == folder_run.VOTE_STATS == vo.VOTE_STATS == 10
    # nothing published about the draws has moved
    assert len(draws_args) == 16 and _lib.SIGNATURES["nbc_dropout_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)


@pytest.mark.parametrize("draws", [1, 2, 3, 4, 7, 255, 1024])
def test_decode_is_the_restatement_for_every_valid_word(built_lib, draws):
    pairs = [(n1, n2) for n1 in range(draws + 1) for n2 in range(draws + 1 - n1)]
    words = np.array([word(n1, n2) for n1, n2 in pairs], dtype=np.uint32)
    label, support, n_win, valid = vo.decode(words, draws)
    assert valid.all() and len(pairs) == (draws + 1) * (draws + 2) // 2
    fn = built_lib.nbc_vote_decode
    lab, sup = C.c_uint8(), C.c_uint8()
    got = np.empty((len(pairs), 2), dtype=np.uint8)
    for i, w in enumerate(words.tolist()):
        assert fn(w, draws, C.byref(lab), C.byref(sup)) == _lib.NBC_OK
        got[i] = (lab.value, sup.value)
    assert np.array_equal(got[:, 0], label) and np.array_equal(got[:, 1], support)
    # what the definition promises of the support byte, on the restatement and therefore on the library
    assert int(support.min()) >= 85 and np.array_equal(support == 255, n_win == draws)
    # the restatement itself against the definition in plain Python
    for (n1, n2), l, s in list(zip(pairs, label.tolist(), support.tolist()))[:: max(1, len(pairs) // 997)]:
        votes = [draws - n1 - n2, n1, n2]
        assert l == votes.index(max(votes)) and s == 255 * max(votes) // draws


def test_spelled_out_cases(built_lib):
    # (n0, n1, n2) -> winner: ties go to the lowest class index
    for (n0, n1, n2), want in (((2, 2, 0), 0), ((0, 2, 2), 1), ((2, 0, 2), 0)):
        assert lib_decode(built_lib, word(n1, n2), 4)[0] == want, (n0, n1, n2)
    assert lib_decode(built_lib, word(1, 1), 3) == (0, 85)
    for draws in (1, 2, 3, 4, 7, 255, 1024, 65535):
        assert lib_decode(built_lib, word(0, 0), draws) == (0, 255)
        assert lib_decode(built_lib, word(draws, 0), draws) == (1, 255)
        assert lib_decode(built_lib, word(0, draws), draws) == (2, 255)
        # n1 + n2 > D: invalid
        for n1, n2 in ((draws + 1, 0), (0, draws + 1), (draws, 1), (1, draws), (65535, 65535)):
            if n1 <= 65535 and n2 <= 65535:
                assert lib_decode(built_lib, word(n1, n2), draws) == (0, 0), (draws, n1, n2)
                l, s, nw, valid = vo.decode(np.array([word(n1, n2)], dtype=np.uint32), draws)
                assert (int(l[0]), int(s[0]), int(nw[0]), bool(valid[0])) == (0, 0, 0, False)
    # just short of unanimous is below 255
    assert lib_decode(built_lib, word(1023, 0), 1024) == (1, 254) and lib_decode(built_lib, word(65534, 0), 65535) == (1, 254)
    # either output may be left out
    lab = C.c_uint8(9)
    assert built_lib.nbc_vote_decode(word(3, 0), 4, C.byref(lab), None) == _lib.NBC_OK and lab.value == 1
    assert built_lib.nbc_vote_decode(word(3, 0), 4, None, None) == _lib.NBC_OK
    for bad in (0, -1, 65536, 2 ** 31 - 1):
        assert built_lib.nbc_vote_decode(0, bad, C.byref(lab), None) == _lib.NBC_ERR_INVALID, bad
        assert _lib.last_error().startswith("nbc_vote_decode:")


def test_restatement_statistics_on_a_hand_made_image():
    labels = np.array([[[0, 1, 2, 1]], [[0, 1, 2, 2]], [[0, 1, 1, 0]], [[0, 1, 3, 0]]])       # D = 4, one image of 1 x 4
    words = vo.tally(labels)
    assert words.tolist() == [[word(0, 0), word(4, 0), word(1, 2), word(1, 1)]]                # the label 3 votes nowhere
    label, support, n_win, valid = vo.decode(words, 4)
    assert label.tolist() == [[0, 1, 2, 0]] and support.tolist() == [[255, 255, 127, 127]] and valid.all()
    assert vo.stats(words[None], 4).tolist() == [[2, 1, 1, 1, 1, 0, 12, 0, 6, 3]]
    planted = np.array([[word(3, 2), word(0, 0)]], dtype=np.uint32)                            # an invalid word reaches slot 7 alone
    assert vo.stats(planted[None], 4).tolist() == [[1, 0, 0, 1, 0, 0, 4, 1, 0, 0]]


def test_votes_arguments_are_refused_before_the_device_is_touched(built_lib):
    """No context exists on a machine without a GPU: every refusal below comes from the argument checks in front of it."""
    fake = 1 << 40
    ids = (C.c_uint64 * 2)(1, 2)

    def call(ctx=None, N=2, H=64, W=64, ids_=ids, p=0.1, seed=0, first=0, draws=4, minpx=150, lowres=None, counts=fake,
             votes=fake, accumulate=0, ws=fake, ws_bytes=1 << 30):
        return built_lib.nbc_dropout_votes(ctx, N, H, W, ids_, p, seed, first, draws, minpx, 0, lowres, counts, votes, accumulate,
                                           ws, ws_bytes, None)

    for kw, text in [(dict(p=1.0), "p must lie in [0, 1)"), (dict(p=float("nan")), "p must lie"),
                     (dict(draws=0), "draws must lie in 1..1024"), (dict(draws=1025), "draws must lie"),
                     (dict(draws=65536), "draws must lie"), (dict(first=-1), "first_draw"), (dict(minpx=-1), "min_pixels"),
                     (dict(), "null argument"), (dict(ctx=fake, votes=None), "null argument"),
                     (dict(ctx=fake, counts=None), "null argument"), (dict(ctx=fake, ids_=None), "null argument"),
                     (dict(ctx=fake, votes=fake + 4), "16-byte aligned"), (dict(ctx=fake, votes=fake + 8, accumulate=1), "16-byte aligned")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        err = _lib.last_error()
        assert err.startswith("nbc_dropout_votes:") and text in err, (kw, err)


def test_summary_arguments_are_refused_before_the_device_is_touched(built_lib):
    fake = 1 << 40

    def call(votes=fake, N=2, H=64, W=64, draws=4, labels=fake, support=fake, stats=fake):
        return built_lib.nbc_vote_summary(votes, N, H, W, draws, labels, support, stats, None)

    for kw, text in [(dict(votes=None), "null argument"), (dict(stats=None), "null argument"), (dict(N=0), "bad shape"),
                     (dict(N=65536), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"),
                     (dict(H=65536, W=32768), "bad shape"), (dict(draws=0), "draws must lie in 1..65535"),
                     (dict(draws=65536), "draws must lie"), (dict(draws=-1), "draws must lie"), (dict(votes=fake + 2), "4-byte aligned")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        err = _lib.last_error()
        assert err.startswith("nbc_vote_summary:") and text in err, (kw, err)


def _f(v):
    return "{:.5f}".format(v)


def test_vote_report_arithmetic_on_crafted_stats():
    h, w, d = 200, 256, 7
    px = h * w
    #        won 0, 1, 2              unanimous 0, 1, 2      sum n_win  invalid  sum n1  sum n2
    st_a = [px - 9000 - 300, 9000, 300, px - 12000, 8000, 100, 7 * px - 11111, 0, 61000, 2222]
    st_b = [px - 1, 1, 0, px - 1, 1, 0, 7 * px, 0, 7, 0]
    images = [("a.png", "sapin", h, w, st_a, 345), ("b.png", "epinette_gelee", h, w, np.array(st_b, dtype=np.int64), 0)]
    table, summary = folder_run.vote_report(images, d)
    assert table[0] == folder_run.VOTE_COLUMNS == ["Name", "Type", "draws", "Vote Bark %", "Vote Node %", "unanimous %",
                                                   "mean_support", "changed_pixels"]
    a, b = table[1], table[2]
    assert a[:3] == ["a.png", "sapin", "7"] and b[:3] == ["b.png", "epinette_gelee", "7"]
    # the vote percentages as final_stats.csv prints a percentage
    assert a[3:5] == [drv.stats_row("a.png", "sapin", h, w, 9000, 300)[i] for i in (2, 4)]
    assert a[3:5] == [folder_run.percent_string(9000, px), folder_run.percent_string(300, px)]
    # one correctly rounded division of exact integers each: float(Fraction) rounds the exact quotient once
    assert a[5] == _f(float(Fraction(100 * (px - 12000 + 8000 + 100), px)))
    assert a[6] == _f(float(Fraction(7 * px - 11111, d * px))) and a[7] == "345"
    assert b[5] == "100.00000" and b[6] == "1.00000" and b[7] == "0"
    assert summary["images"] == 2
    means = summary["means"]
    assert set(means) == {"vote_bark", "vote_node", "unanimous", "mean_support", "changed_pixels"}
    assert means["changed_pixels"] == 172.5
    assert means["vote_bark"] == (float(Fraction(100 * 9000, px)) + float(Fraction(100, px))) / 2
    assert means["mean_support"] == (float(Fraction(7 * px - 11111, d * px)) + 1.0) / 2
    assert means["unanimous"] == (float(Fraction(100 * (px - 3900), px)) + 100.0) / 2
    # a division whose double differs from a float32 one in the fifth decimal would show here: an awkward denominator
    t, _ = folder_run.vote_report([("c.png", "sapin", 129, 65, [8385 - 1, 1, 0, 8384, 0, 0, 3 * 8385 - 1, 0, 2, 0], 1)], 3)
    assert t[1][5] == _f(float(Fraction(100 * 8384, 8385))) and t[1][6] == _f(float(Fraction(3 * 8385 - 1, 3 * 8385)))
    assert folder_run.vote_report([], 3) == ([folder_run.VOTE_COLUMNS], {"images": 0, "means": {}})


def test_report_files_with_votes(tmp_path):
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}]
    allrows = np.array([[0, 16, 16, 100, 5], [1, 16, 32, 200, 9]], dtype=np.int64)
    alld = np.array([[1, 300, 200, 12, 310, 190, 12], [0, 150, 101, 5, 152, 99, 5]], dtype=np.int64)
    allv = np.array([[1, 310, 195, 7, 300, 190, 5, 1010, 0, 390, 24, 6], [0, 150, 101, 5, 148, 99, 5, 510, 0, 200, 10, 3]], dtype=np.int64)
    plain = tmp_path / "plain"
    voted = tmp_path / "voted"
    plain.mkdir()
    voted.mkdir()
    drv.write_dropout_report(str(plain), items, allrows, alld, 2, 0.1, 42, "fp32", "running")
    s = drv.write_dropout_report(str(voted), items, allrows, alld, 2, 0.1, 42, "fp32", "running", allv=allv)
    assert sorted(os.listdir(plain)) == ["dropout_stats.csv", "dropout_summary.json"]
    assert sorted(os.listdir(voted)) == ["dropout_stats.csv", "dropout_summary.json", "dropout_votes.csv"]
    assert open(plain / "dropout_stats.csv", "rb").read() == open(voted / "dropout_stats.csv", "rb").read()
    rows = list(csv.reader(open(voted / "dropout_votes.csv"), delimiter="\t"))
    want, wsum = folder_run.vote_report([("a.png", "sapin", 16, 16, allv[1, 1:11], 3), ("b.png", "sapin", 16, 32, allv[0, 1:11], 6)], 2)
    assert rows == want and [r[7] for r in rows[1:]] == ["3", "6"]
    doc, doc0 = json.load(open(voted / "dropout_summary.json")), json.load(open(plain / "dropout_summary.json"))
    assert doc == json.loads(json.dumps(s)) and doc["votes"] == json.loads(json.dumps(wsum["means"]))
    assert "votes" not in doc0 and {k: v for k, v in doc.items() if k != "votes"} == doc0


def _cli(*argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv", [["--dropout_votes"], ["--dropout_votes", "--precision", "fp32"], ["--dropout_votes", "--only_preprocess"]])
def test_votes_without_draws_exit_with_code_2(argv):
    p = _cli(*argv)
    assert p.returncode == 2 and "--dropout_votes needs --dropout_draws" in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike(built_lib):
    with pytest.raises(ValueError, match="needs --dropout_draws"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", dropout_votes=True)
    with pytest.raises(ValueError):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", dropout_draws=4, dropout_votes=True, arch="deeplabv3_resnet50")
    with pytest.raises(ValueError, match="needs --dropout_draws"):
        folder_run.check_dropout_arguments(None, votes=True)
    folder_run.check_dropout_arguments(4, votes=True)
    folder_run.check_dropout_arguments(None)
    from neuralbarkcalculator_amd.model import DeepLabV3EfficientNet, DeepLabV3ResNet50, FCNEfficientNet, FCNResNet50
    with pytest.raises(ValueError, match="DeepLabHead's Dropout sits inside ASPP"):
        DeepLabV3ResNet50("fp32").dropout_votes(4, [1])
    for cls in (FCNEfficientNet, DeepLabV3EfficientNet):
        with pytest.raises(ValueError, match="EfficientNet's FCN head is left out"):
            cls(0).dropout_votes(4, [1])
    m = FCNResNet50("fp32")
    for kw in (dict(draws=0), dict(draws=1025), dict(draws=1, p=1.0), dict(draws=1, first_draw=-1), dict(draws=1, seed=2 ** 64)):
        with pytest.raises(ValueError):
            m.dropout_votes(image_ids=[1], **kw)
    with pytest.raises(RuntimeError):                       # no device, no weights, no forward
        m.dropout_votes(1, [1])


def test_folders_of_the_votes_only_with_the_flag(tmp_path):
    for tag, votes in (("off", False), ("on", True)):
        root = tmp_path / tag
        (root / "samples" / "sapin").mkdir(parents=True)
        drv.generate_folders(str(root), votes=votes)
        assert sorted(os.listdir(root / "results")) == sorted(["combined_images", "outputs"] + (["dropout_support", "dropout_votes"] if votes else []))
