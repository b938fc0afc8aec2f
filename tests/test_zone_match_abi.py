"""`evaluate --zones` without a GPU: the host restatement zones.match_cpu and the figures of zones.match_figures against answers
worked out by hand (so that the oracle of tests/test_gpu_zone_match.py is not its own witness), the refusals of nbc_match_zones
in front of the device, the formatting of the three files, the command line's refusals and the gather of unequal per-rank pair
row counts over gloo."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from neuralbarkcalculator_amd import _lib, folder_run, zones
from neuralbarkcalculator_amd import evaluate as drv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#          x: 0  1  2  3  4  5  6
ONE_NODE = [[0, 0, 0, 0, 0, 0, 0],
            [0, 2, 2, 2, 2, 2, 0],      # one node of 5 pixels, first pixel 8
            [0, 0, 0, 0, 0, 0, 0]]
TWO_NODES = [[0, 0, 0, 0, 0, 0, 0],
             [0, 2, 0, 2, 2, 2, 0],     # a node of 1 pixel (first pixel 8) and one of 3 (first pixel 10)
             [0, 0, 0, 0, 0, 0, 0]]


def one(labels, target):
    got = zones.match_cpu(np.array(labels, dtype=np.uint8), np.array(target, dtype=np.uint8))
    assert len(got) == 1 and all(a.dtype == np.int64 for a in got[0])
    return got[0]


def test_constants_and_signatures(built_lib):
    assert zones.PAIR_ROW == _lib.ZONE_PAIR_ROW == 3 and zones.PAIRS_MAX_CAP == _lib.PAIRS_MAX_CAP == 4096
    assert zones.PAIRS_MAX_CAP >= 2048 and 1 <= zones.DEFAULT_PAIR_CAP <= zones.PAIRS_MAX_CAP
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    assert "#define NBC_ZONE_PAIR_ROW 3" in header and "#define NBC_ZONE_PAIRS_MAX_CAP 4096" in header
    assert "size_t nbc_zone_match_workspace_bytes(int N, int H, int W, int pair_cap);" in header
    assert "int nbc_match_zones(nbc_ctx* ctx, const void* labels_dev, int labels_dtype, const uint8_t* target_grey_dev," in header
    assert hasattr(built_lib, "nbc_match_zones") and hasattr(built_lib, "nbc_zone_match_workspace_bytes")
    assert _lib.SIGNATURES["nbc_zone_match_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert _lib.SIGNATURES["nbc_match_zones"][0] == C.c_int and len(_lib.SIGNATURES["nbc_match_zones"][1]) == 18


def test_match_zones_refusals_come_before_the_device(built_lib):
    """No context exists on a machine without a GPU: every refusal below comes from the argument checks in front of it."""
    fake = 1 << 40
    zones_ws = built_lib.nbc_zones_workspace_bytes(2, 64, 64)
    need = built_lib.nbc_zone_match_workspace_bytes(2, 64, 64, 16)
    # both labellings, a class byte per pixel, per image 32 slots of 8 + 4 bytes, 2 claim counters; regions rounded up to 256
    assert need == 2 * zones_ws + 2 * 4096 + 8 * 2 * 32 + 4 * 2 * 32 + 256
    assert built_lib.nbc_zone_match_workspace_bytes(1, 1024, 1024, 4096) == \
        2 * built_lib.nbc_zones_workspace_bytes(1, 1024, 1024) + (1 << 20) + 8 * 8192 + 4 * 8192 + 256
    assert built_lib.nbc_zone_match_workspace_bytes(1, 8, 8, 1) == 2 * built_lib.nbc_zones_workspace_bytes(1, 8, 8) + 4 * 256
    for shape in ((0, 64, 64), (65536, 64, 64), (1, 0, 64), (1, 64, 0), (1, 65536, 1), (1, 1, 65536), (1, 65535, 32769)):
        assert built_lib.nbc_zone_match_workspace_bytes(*shape, 16) == 0, shape
    for pair_cap in (0, -1, 4097):
        assert built_lib.nbc_zone_match_workspace_bytes(2, 64, 64, pair_cap) == 0, pair_cap

    def call(ctx=fake, labels=fake, dtype=_lib.LABEL_U8, target=fake, N=2, H=64, W=64, out_rows=fake, out_num=fake, tgt_rows=fake,
             tgt_num=fake, cap=16, pair_rows=fake, pair_num=fake, pair_cap=16, ws=fake, ws_bytes=need):
        return built_lib.nbc_match_zones(ctx, labels, dtype, target, N, H, W, out_rows, out_num, tgt_rows, tgt_num, cap, pair_rows,
                                         pair_num, pair_cap, ws, ws_bytes, None)

    nulls = [(dict([(k, None)]), "null argument") for k in ("ctx", "labels", "target", "out_rows", "out_num", "tgt_rows", "tgt_num",
                                                          "pair_rows", "pair_num", "ws")]
    for kw, text in nulls + [(dict(N=0), "bad shape"), (dict(N=65536), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"),
                             (dict(H=-3), "bad shape"), (dict(H=65536, W=1), "bad shape"), (dict(W=65536, H=1), "bad shape"),
                             (dict(H=65535, W=32769, N=1), "bad shape"), (dict(cap=0), "cap must be at least 1"),
                             (dict(pair_cap=0), "pair_cap must lie in 1..4096"), (dict(pair_cap=4097), "pair_cap must lie in 1..4096"),
                             (dict(pair_cap=-5), "pair_cap must"), (dict(dtype=7), "bad labels_dtype"),
                             (dict(ws_bytes=need - 1), "workspace of"), (dict(ws_bytes=0), "workspace of"),
                             (dict(pair_cap=17), "workspace of"),          # the next table size: 64 slots per image
                             (dict(ws=fake + 128), "256-byte aligned")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        err = _lib.last_error()
        assert err.startswith("nbc_match_zones:") and text in err, (kw, err)


def test_model_object_refusals():
    from neuralbarkcalculator_amd.model import FCNResNet50
    with pytest.raises(RuntimeError):                                    # no device: no context
        FCNResNet50("fp32").match_zones(np.zeros((4, 4)), np.zeros((4, 4)))


def test_grey_levels_on_both_sides_of_the_class_boundaries():
    grey = np.array([0, 63, 64, 127, 191, 192, 255], dtype=np.uint8)
    assert zones.target_classes(grey).tolist() == [0, 0, 1, 1, 1, 2, 2]
    from neuralbarkcalculator_amd import metrics
    assert zones.target_classes is metrics.target_classes                # one rule, the one nbc_confusion's oracle uses
    assert zones.target_classes(np.arange(256, dtype=np.uint8)).tolist() == [0] * 64 + [1] * 128 + [2] * 64


def test_a_target_node_split_in_two_by_the_output():
    o, t, p = one(TWO_NODES, ONE_NODE)
    assert o[:, :3].tolist() == [[8, 2, 1], [10, 2, 3]] and t[:, :3].tolist() == [[8, 2, 5]]
    assert np.array_equal(o, zones.zones_cpu(np.array(TWO_NODES))[0]) and np.array_equal(t, zones.zones_cpu(np.array(ONE_NODE))[0])
    assert p.tolist() == [[0, 0, 1], [1, 0, 3]]
    f = zones.match_figures(o, t, p)                                     # 3 / (3 + 5 - 3) = 0.6 matches, 1 / 5 does not
    assert f["Node"] == {"targets": 1, "outputs": 2, "matched": 1, "missed": 0, "spurious": 1, "split_targets": 1, "merged_outputs": 0,
                         "recall": 1.0, "precision": 0.5, "f1": 2 / 3, "mean_iou": 0.6, "iou_sum": 0.6, "missed_pixels": 0,
                         "spurious_pixels": 1}
    assert f["Bark"] == {"targets": 0, "outputs": 0, "matched": 0, "missed": 0, "spurious": 0, "split_targets": 0, "merged_outputs": 0,
                         "recall": None, "precision": None, "f1": None, "mean_iou": None, "iou_sum": 0.0, "missed_pixels": 0,
                         "spurious_pixels": 0}
    strict = zones.match_figures(o, t, p, iou=0.75)["Node"]              # 0.6 is no match at 0.75
    assert (strict["matched"], strict["missed"], strict["spurious"], strict["mean_iou"]) == (0, 1, 2, None)
    assert zones.match_figures(o, t, p[::-1])["Node"] == f["Node"]       # the order of the pair rows does not matter


def test_two_target_nodes_merged_by_one_output_zone():
    o, t, p = one(ONE_NODE, TWO_NODES)
    assert p.tolist() == [[0, 0, 1], [0, 1, 3]]
    f = zones.match_figures(o, t, p)["Node"]
    assert f == {"targets": 2, "outputs": 1, "matched": 1, "missed": 1, "spurious": 0, "split_targets": 0, "merged_outputs": 1,
                 "recall": 0.5, "precision": 1.0, "f1": 2 / 3, "mean_iou": 0.6, "iou_sum": 0.6, "missed_pixels": 1, "spurious_pixels": 0}
    # the missed 1-pixel target names the output zone that covers it: the only one, IoU 1 / 5
    assert zones.match_rows("a.png", "sapin", o, t, p) == [
        ["a.png", "sapin", "Node", "1", "1", "1", "5", "1", "0.200000", "missed"],
        ["a.png", "sapin", "Node", "2", "1", "3", "5", "3", "0.600000", "matched"]]


def test_an_iou_of_exactly_one_half_is_no_match():
    tgt = [[2, 2, 2, 2, 0, 0]]
    out = [[2, 2, 0, 0, 0, 0]]                                           # 2 / (2 + 4 - 2) = 0.5 exactly
    o, t, p = one(out, tgt)
    assert p.tolist() == [[0, 0, 2]]
    f = zones.match_figures(o, t, p, iou=0.5)["Node"]
    assert (f["matched"], f["missed"], f["spurious"], f["split_targets"], f["merged_outputs"]) == (0, 1, 1, 0, 0)
    assert f["recall"] == 0.0 and f["precision"] == 0.0 and f["f1"] == 0.0 and f["mean_iou"] is None
    out3 = [[2, 2, 2, 0, 0, 0]]                                          # 3 / 4: a match
    assert zones.match_figures(*one(out3, tgt))["Node"]["matched"] == 1
    # the same zone twice is IoU 1: matched at every threshold below 1
    assert zones.match_figures(*one(tgt, tgt), iou=0.999)["Node"]["mean_iou"] == 1.0
    for bad in (0.49, 1.0, -1, float("nan"), "x"):
        with pytest.raises(ValueError):
            zones.match_figures(o, t, p, iou=bad)


def test_crossing_diagonals_of_the_two_classes():
    m = np.zeros((4, 4), dtype=np.uint8)
    for i in range(4):
        m[i, i] = 1                      # bark down the main diagonal
        m[i, 3 - i] = 2                  # nodes down the other one: the lines cross between pixels
    o, t, p = one(m, m)
    assert p.tolist() == [[0, 0, 4], [1, 1, 4]]                          # each line is one zone and pairs with itself alone
    swapped = np.where(m == 0, 0, 3 - m).astype(np.uint8)
    o, t, p = one(m, swapped)                                            # the classes swapped: not one pixel of equal class
    assert p.shape == (0, 3)
    f = zones.match_figures(o, t, p)
    assert all((f[c]["targets"], f[c]["outputs"], f[c]["missed"], f[c]["spurious"]) == (1, 1, 1, 1) for c in ("Bark", "Node"))
    # 5x5: the lines cross AT the centre pixel; the class written last owns it and cuts the other line in two
    a = np.zeros((5, 5), dtype=np.uint8)
    b = np.zeros((5, 5), dtype=np.uint8)
    for i in range(5):
        a[i, i] = 1
        b[i, 4 - i] = 2
    for i in range(5):
        a[i, 4 - i] = 2                  # a: node line whole, bark line cut: bark (0,0)(1,1), node line, bark (3,3)(4,4)
        b[i, i] = 1                      # b: bark line whole, node line cut: bark line, node (0,4)(1,3), node (3,1)(4,0)
    o, t, p = one(a, b)
    assert o[:, :3].tolist() == [[0, 1, 2], [4, 2, 5], [18, 1, 2]] and t[:, :3].tolist() == [[0, 1, 5], [4, 2, 2], [16, 2, 2]]
    assert p.tolist() == [[0, 0, 2], [1, 1, 2], [1, 2, 2], [2, 0, 2]]    # the centre pixel is node in a and bark in b: nobody's
    f = zones.match_figures(o, t, p)                                     # every IoU is 2 / 5
    assert (f["Bark"]["split_targets"], f["Bark"]["merged_outputs"], f["Bark"]["missed"], f["Bark"]["spurious"]) == (1, 0, 1, 2)
    assert (f["Node"]["split_targets"], f["Node"]["merged_outputs"], f["Node"]["missed"], f["Node"]["spurious"]) == (0, 1, 2, 1)


def test_missed_targets_with_and_without_a_best_overlap_and_ties():
    tgt = [[1, 1, 1, 1, 1, 1, 0, 2],
           [0, 0, 0, 0, 0, 0, 0, 0],
           [2, 2, 0, 0, 0, 0, 0, 0]]
    out = [[1, 1, 0, 1, 1, 0, 0, 0],     # two bark zones of 2 on a target of 6: a tie, the lower index is named
           [0, 0, 0, 0, 0, 0, 0, 0],
           [2, 2, 0, 0, 1, 0, 0, 0]]     # the node (0,2)(1,2) is found; the node at (7,0) is seen by nobody; a bark zone on nothing
    o, t, p = one(out, tgt)
    assert o[:, :3].tolist() == [[0, 1, 2], [3, 1, 2], [16, 2, 2], [20, 1, 1]]
    assert t[:, :3].tolist() == [[0, 1, 6], [7, 2, 1], [16, 2, 2]]
    assert p.tolist() == [[0, 0, 2], [1, 0, 2], [2, 2, 2]]
    assert zones.match_rows("b.png", "sapin", o, t, p) == [
        ["b.png", "sapin", "Bark", "1", "1", "6", "2", "2", "0.333333", "missed"],
        ["b.png", "sapin", "Node", "2", "", "1", "", "", "", "missed"],
        ["b.png", "sapin", "Node", "3", "3", "2", "2", "2", "1.000000", "matched"],
        ["b.png", "sapin", "Bark", "", "1", "", "2", "", "", "spurious"],
        ["b.png", "sapin", "Bark", "", "2", "", "2", "", "", "spurious"],
        ["b.png", "sapin", "Bark", "", "4", "", "1", "", "", "spurious"]]
    f = zones.match_figures(o, t, p)
    assert f["Bark"]["missed_pixels"] == 6 and f["Bark"]["spurious_pixels"] == 5 and f["Node"]["missed_pixels"] == 1
    d = zones.match_details(o, t, p)
    assert d["partner_of_target"].tolist() == [-1, -1, 2] and d["best_of_target"].tolist() == [0, -1, 2]
    assert d["partner_of_output"].tolist() == [-1, -1, 2, -1]


def test_an_image_with_no_zones_at_all_and_other_inputs():
    o, t, p = one(np.zeros((3, 4)), np.zeros((3, 4)))
    assert o.shape == (0, 10) and t.shape == (0, 10) and p.shape == (0, 3) and p.dtype == np.int64
    f = zones.match_figures(o, t, p)
    for c in ("Bark", "Node"):
        assert all(f[c][k] == 0 for k in ("targets", "outputs", "matched", "missed", "spurious", "split_targets", "merged_outputs"))
        assert f[c]["recall"] is None and f[c]["precision"] is None and f[c]["f1"] is None and f[c]["mean_iou"] is None
    assert zones.match_rows("z.png", "sapin", o, t, p) == []
    # labels outside {1, 2} belong to no zone, on either side; a batch comes back per image
    got = zones.match_cpu(np.array([[[3, 1], [257, 2]], [[0, 0], [0, 0]]]), np.array([[[1, 1], [1, 2]], [[2, 2], [2, 2]]]))
    assert got[0][2].tolist() == [[0, 0, 1], [1, 1, 1]] and got[1][2].shape == (0, 3) and len(got[1][1]) == 1
    with pytest.raises(ValueError):
        zones.match_cpu(np.zeros((2, 2)), np.zeros((2, 3)))
    with pytest.raises(ValueError):                                      # a pair of zones of different classes is no pair
        zones.match_figures([[0, 1, 1, 0, 0, 0, 0, 0, 0, 4]], [[0, 2, 1, 0, 0, 0, 0, 0, 0, 4]], [[0, 0, 1]])


def test_evaluation_rows_and_summary_formatting():
    assert zones.MATCH_COLUMNS == ["Name", "Type", "Class", "Target zone", "Output zone", "Target pixels", "Output pixels",
                                   "Overlap pixels", "IoU", "Status"]
    assert zones.EVALUATION_COLUMNS[:4] == ["Name", "Type", "Bark target zones", "Bark output zones"]
    assert len(zones.EVALUATION_COLUMNS) == 2 + 2 * 13 and zones.EVALUATION_COLUMNS[15] == "Node target zones"
    f1 = zones.match_figures(*one(TWO_NODES, ONE_NODE))
    f2 = zones.match_figures(*one(ONE_NODE, TWO_NODES))
    assert zones.evaluation_rows("a.png", "sapin", f1) == [
        ["a.png", "sapin", "0", "0", "0", "0", "0", "0", "0", "", "", "", "", "0.00000", "0.00000",
         "1", "2", "1", "0", "1", "1", "0", "1.000000", "0.500000", "0.666667", "0.600000", "0.00000", "12.96000"]]
    assert zones.evaluation_rows("b.png", "sapin", f2)[0][15:] == \
        ["2", "1", "1", "1", "0", "0", "1", "0.500000", "1.000000", "0.666667", "0.600000", "12.96000", "0.00000"]
    doc = zones.match_summary([f1, f2], 0.5, 1024, 2048, 1)
    assert doc["images"] == 2 and doc["match_iou"] == 0.5 and doc["zones_cap"] == 1024 and doc["zone_pairs_cap"] == 2048
    assert doc["host_fallbacks"] == 1
    assert doc["Node"] == {"targets": 3, "outputs": 3, "matched": 2, "missed": 1, "spurious": 1, "split_targets": 1, "merged_outputs": 1,
                           "recall": 2 / 3, "precision": 2 / 3, "f1": 2 / 3, "mean_iou": 0.6}
    assert doc["Bark"]["targets"] == 0 and doc["Bark"]["recall"] is None and doc["Bark"]["mean_iou"] is None
    json.dumps(doc)


def test_report_files(tmp_path):
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}, {"name": "c.png", "wood": "epinette_gelee"}]
    allrows = np.zeros((3, drv.ROW_WIDTH), dtype=np.int64)
    allrows[:, 0] = (0, 1, 2)
    allrows[1, 3] = drv.STATUS_NO_DUAL                                   # b.png was skipped: it has no rows and no line
    a, c = one(TWO_NODES, ONE_NODE), one(ONE_NODE, TWO_NODES)

    def tag(g, rows):
        return np.concatenate([np.full((len(rows), 1), g, dtype=np.int64), rows], axis=1)
    doc = drv.write_zone_match_report(str(tmp_path), items, allrows, np.concatenate([tag(0, a[0]), tag(2, c[0])]),
                                      np.concatenate([tag(0, a[1]), tag(2, c[1])]), np.concatenate([tag(0, a[2]), tag(2, c[2])]),
                                      0.5, 8, 16, 0)
    assert sorted(os.listdir(tmp_path)) == ["zone_evaluation.csv", "zone_matches.csv"]
    table = [line.split("\t") for line in open(tmp_path / "zone_matches.csv").read().splitlines()]
    assert table == [zones.MATCH_COLUMNS,
                     ["a.png", "sapin", "Node", "1", "2", "5", "3", "3", "0.600000", "matched"],
                     ["a.png", "sapin", "Node", "", "1", "", "1", "", "", "spurious"]] + \
        zones.match_rows("c.png", "epinette_gelee", *c)
    ev = [line.split("\t") for line in open(tmp_path / "zone_evaluation.csv").read().splitlines()]
    assert ev == [zones.EVALUATION_COLUMNS] + zones.evaluation_rows("a.png", "sapin", zones.match_figures(*a)) + \
        zones.evaluation_rows("c.png", "epinette_gelee", zones.match_figures(*c))
    assert doc == zones.match_summary([zones.match_figures(*a), zones.match_figures(*c)], 0.5, 8, 16, 0)


def _cli(*argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--zones_cap", "8"], "--zones_cap needs --zones"),
                                       (["--zone_pairs_cap", "8"], "--zone_pairs_cap needs --zones"),
                                       (["--match_iou", "0.6"], "--match_iou needs --zones"),
                                       (["--zones", "--zones_cap", "0"], "--zones_cap must lie in 1..65536"),
                                       (["--zones", "--zone_pairs_cap", "4097"], "--zone_pairs_cap must lie in 1..4096"),
                                       (["--zones", "--zone_pairs_cap", "0"], "--zone_pairs_cap must lie in 1..4096"),
                                       (["--zones", "--match_iou", "0.49"], "--match_iou must lie in [0.5, 1)"),
                                       (["--zones", "--match_iou", "1"], "--match_iou must lie in [0.5, 1)")])
def test_command_line_refusals(argv, text):
    p = _cli(*argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike():
    for kw, text in [(dict(zones_cap=4), "--zones_cap needs --zones"), (dict(zone_pairs_cap=4), "--zone_pairs_cap needs --zones"),
                     (dict(match_iou=0.5), "--match_iou needs --zones"), (dict(zones=True, zones_cap=0), "must lie in"),
                     (dict(zones=True, zone_pairs_cap=4097), "must lie in 1..4096"), (dict(zones=True, match_iou=1.0), "must lie in"),
                     (dict(zones=True, match_iou=0.3), "must lie in")]:
        with pytest.raises(ValueError, match=text.replace("[", r"\[").replace(")", r"\)")):
            drv.evaluate_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", **kw)
    drv.check_zone_match_arguments(True, 1, 1, 0.5)
    drv.check_zone_match_arguments(True, None, 4096, 0.999)
    drv.check_zone_match_arguments(False)


WIDTH = 1 + zones.PAIR_ROW
# scenario -> per rank, the (global index, pair count) of its images
SCENARIOS = {"empty_rank": [[(0, 0), (2, 0)], [(1, 5), (3, 1)]],         # rank 0 has images but not one pair
             "one_large": [[(0, 2), (3, 0)], [(1, 7), (2, 1)]]}          # image 1 alone has more rows than rank 0 in all


def _rows_of(images):
    return np.array([[g, k // 2, k, 10 * g + k + 1] for g, n in images for k in range(n)], dtype=np.int64).reshape(-1, WIDTH)


def _ragged_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for tag, per_rank in SCENARIOS.items():
            got = folder_run.gather_ragged(_rows_of(per_rank[rank]), world, dist, None, width=WIDTH)
            np.save(os.path.join(out_dir, "%s_%d.npy" % (tag, rank)), got)
    finally:
        dist.destroy_process_group()


def test_two_rank_gather_of_unequal_pair_row_counts(tmp_path):
    mp.spawn(_ragged_worker, args=(2, 29673, str(tmp_path)), nprocs=2, join=True)
    for tag, per_rank in SCENARIOS.items():
        everything = sorted(per_rank[0] + per_rank[1])
        want = _rows_of(everything)                                      # what one rank yields: an image's rows together, in order
        assert len(want) in (6, 10)
        for r in range(2):
            got = np.load(os.path.join(str(tmp_path), "%s_%d.npy" % (tag, r)))
            assert got.shape == want.shape and got.tolist() == want.tolist(), (tag, r)
