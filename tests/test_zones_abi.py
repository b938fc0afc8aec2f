"""The zone inventory of `predict --zones` without a GPU: the host restatement zones.zones_cpu against answers worked out by
hand (so that the oracle of tests/test_gpu_zones.py is not its own witness), the refusals of nbc_label_zones in front of the
device, the CSV formatting, the command line's refusals and the gather of unequal per-rank row counts over gloo."""
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
from neuralbarkcalculator_amd import predict as drv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#            x: 0  1  2  3  4  5  6
MAP_6x7 = [[1, 1, 0, 0, 2, 2, 0],       # y 0    A = bark (0,0) (1,0) (1,1) and, through a diagonal, (2,2)
           [0, 1, 0, 0, 0, 2, 0],       # y 1    B = node (4,0) (5,0) (5,1)
           [0, 0, 1, 0, 0, 0, 0],       # y 2
           [0, 0, 0, 0, 3, 0, 2],       # y 3    C = node (6,3) and, through a diagonal, (5,4); the 3 at (4,3) is no zone
           [2, 0, 0, 0, 0, 2, 0],       # y 4    D = node (0,4) (0,5) (1,5)
           [2, 2, 0, 1, 0, 0, 0]]       # y 5    E = bark (3,5)
# first_pixel, class, pixels, x0, y0, x1, y1, sum_x, sum_y, perimeter -- counted by hand, side by side:
#   A: (0,0) N W S = 3, (1,0) N E = 2, (1,1) S W E = 3, (2,2) all 4      B: (4,0) N W S = 3, (5,0) N E = 2, (5,1) S W E = 3
#   C: 4 + 4 (a diagonal shares no side)                                 D: (0,4) N W E = 3, (0,5) S W = 2, (1,5) N S E = 3
ZONES_6x7 = [[0, 1, 4, 0, 0, 2, 2, 4, 3, 12],
             [4, 2, 3, 4, 0, 5, 1, 14, 1, 8],
             [27, 2, 2, 5, 3, 6, 4, 11, 7, 8],
             [28, 2, 3, 0, 4, 1, 5, 1, 14, 8],
             [38, 1, 1, 3, 5, 3, 5, 3, 5, 4]]


def test_constants_and_signatures(built_lib):
    assert zones.ZONE_ROW == _lib.ZONE_ROW == 10 and len(zones.ZONE_FIELDS) == 10
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    assert "#define NBC_ZONE_ROW 10" in header and "size_t nbc_zones_workspace_bytes(int N, int H, int W);" in header
    assert "int nbc_label_zones(nbc_ctx* ctx, const void* labels_dev, int labels_dtype, int N, int H, int W," in header
    assert hasattr(built_lib, "nbc_label_zones") and hasattr(built_lib, "nbc_zones_workspace_bytes")
    assert _lib.SIGNATURES["nbc_zones_workspace_bytes"] == (C.c_size_t, [C.c_int] * 3)
    assert len(_lib.SIGNATURES["nbc_label_zones"][1]) == 12


@pytest.mark.parametrize("dtype", [np.uint8, np.int64, np.int32])
def test_hand_counted_map(dtype):
    got = zones.zones_cpu(np.array(MAP_6x7, dtype=dtype))
    assert len(got) == 1 and got[0].dtype == np.int64 and got[0].tolist() == ZONES_6x7
    both = zones.zones_cpu(np.stack([np.array(MAP_6x7, dtype=dtype), np.zeros((6, 7), dtype=dtype)]))
    assert both[0].tolist() == ZONES_6x7 and both[1].shape == (0, 10)


def test_crossing_diagonals_are_two_zones():
    m = np.zeros((4, 4), dtype=np.uint8)
    for i in range(4):
        m[i, i] = 1                      # bark down the main diagonal
        m[i, 3 - i] = 2                  # nodes down the other one: the lines cross between pixels
    # 8-connected, so each line is ONE zone (not four pixels), and the classes never merge (not one zone)
    assert zones.zones_cpu(m)[0].tolist() == [[0, 1, 4, 0, 0, 3, 3, 6, 6, 16], [3, 2, 4, 0, 0, 3, 3, 6, 6, 16]]


def test_single_pixel_edges_and_foreign_labels():
    m = np.zeros((5, 6), dtype=np.uint8)
    m[2, 3] = 2
    assert zones.zones_cpu(m)[0].tolist() == [[15, 2, 1, 3, 2, 3, 2, 3, 2, 4]]
    assert zones.zones_cpu(np.ones((1, 1), dtype=np.uint8))[0].tolist() == [[0, 1, 1, 0, 0, 0, 0, 0, 0, 4]]
    plus = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint8)               # touches all four edges
    z = zones.zones_cpu(plus)[0]
    assert z.tolist() == [[1, 1, 5, 0, 0, 2, 2, 5, 5, 12]] and zones.touches_edge(z[0], 3, 3)
    full = zones.zones_cpu(np.full((3, 4), 2, dtype=np.uint8))[0]
    assert full.tolist() == [[0, 2, 12, 0, 0, 3, 2, 18, 12, 14]]
    assert zones.zones_cpu(np.full((4, 4), 3, dtype=np.uint8))[0].shape == (0, 10)   # a value of 3: no zone
    m = np.array([[3, 1, 3], [3, 1, 1]], dtype=np.uint8)                             # ... but another label for a side
    assert zones.zones_cpu(m)[0].tolist() == [[1, 1, 3, 1, 0, 2, 1, 4, 2, 8]]
    # the (y + x) % 2 checkerboard of the two classes: a labelling that forgets the class merges it
    yy, xx = np.mgrid[0:8, 0:8]
    c = zones.zones_cpu(((yy + xx) % 2 + 1).astype(np.uint8))[0]
    assert c[:, :3].tolist() == [[0, 1, 32], [1, 2, 32]] and c[:, 9].tolist() == [128, 128]
    with pytest.raises(ValueError):
        zones.zones_cpu(np.zeros((2, 2, 2, 2), dtype=np.uint8))


def test_label_zones_refusals_come_before_the_device(built_lib):
    """No context exists on a machine without a GPU: every refusal below comes from the argument checks in front of it."""
    fake = 1 << 40
    need = built_lib.nbc_zones_workspace_bytes(2, 64, 64)
    # a parent int and a class byte per pixel, a count per 1024 pixels, each region rounded up to 256 bytes
    assert need == 4 * 2 * 4096 + 2 * 4096 + 256
    assert built_lib.nbc_zones_workspace_bytes(1, 1024, 1024) == 5 * (1 << 20) + 4096
    assert built_lib.nbc_zones_workspace_bytes(1, 31, 33) == 4096 + 1024 + 256
    for shape in ((0, 64, 64), (65536, 64, 64), (1, 0, 64), (1, 64, 0), (1, 65536, 1), (1, 1, 65536), (1, 65535, 32769)):
        assert built_lib.nbc_zones_workspace_bytes(*shape) == 0, shape
    assert built_lib.nbc_zones_workspace_bytes(1, 65535, 32768) > 0      # H * W = 2^31 - 32768

    def call(ctx=fake, labels=fake, dtype=_lib.LABEL_U8, N=2, H=64, W=64, rows=fake, cap=16, num=fake, ws=fake, ws_bytes=need):
        return built_lib.nbc_label_zones(ctx, labels, dtype, N, H, W, rows, cap, num, ws, ws_bytes, None)

    for kw, text in [(dict(ctx=None), "null argument"), (dict(labels=None), "null argument"), (dict(rows=None), "null argument"),
                     (dict(num=None), "null argument"), (dict(ws=None), "null argument"),
                     (dict(N=0), "bad shape"), (dict(N=65536), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"),
                     (dict(H=-3), "bad shape"), (dict(H=65536, W=1), "bad shape"), (dict(W=65536, H=1), "bad shape"),
                     (dict(H=65535, W=32769, N=1), "bad shape"), (dict(cap=0), "cap must be at least 1"), (dict(cap=-1), "cap must"),
                     (dict(dtype=7), "bad labels_dtype"), (dict(ws_bytes=need - 1), "workspace of"), (dict(ws_bytes=0), "workspace of"),
                     (dict(ws=fake + 128), "256-byte aligned")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        err = _lib.last_error()
        assert err.startswith("nbc_label_zones:") and text in err, (kw, err)


def test_model_object_refusals():
    from neuralbarkcalculator_amd.model import FCNResNet50
    with pytest.raises(RuntimeError):                                    # no device: no context
        FCNResNet50("fp32").label_zones(np.zeros((4, 4)))


def test_zone_rows_formatting():
    assert zones.ZONE_COLUMNS == ["Name", "Type", "Zone", "Class", "Pixels", "Area (mm^2)", "Left", "Top", "Right", "Bottom",
                                  "Centroid x", "Centroid y", "Perimeter (mm)", "Diameter (mm)", "Touches edge"]
    rows = zones.zone_rows("a.png", "sapin", 6, 7, ZONES_6x7)
    assert rows == [
        ["a.png", "sapin", "1", "Bark", "4", "51.84000", "0", "0", "2", "2", "1.000", "0.750", "43.200", "8.124", "1"],
        ["a.png", "sapin", "2", "Node", "3", "38.88000", "4", "0", "5", "1", "4.667", "0.333", "28.800", "7.036", "1"],
        ["a.png", "sapin", "3", "Node", "2", "25.92000", "5", "3", "6", "4", "5.500", "3.500", "28.800", "5.745", "1"],
        ["a.png", "sapin", "4", "Node", "3", "38.88000", "0", "4", "1", "5", "0.333", "4.667", "28.800", "7.036", "1"],
        ["a.png", "sapin", "5", "Bark", "1", "12.96000", "3", "5", "3", "5", "3.000", "5.000", "14.400", "4.062", "1"]]
    # the area in float32, as final_stats.csv prints one: 123457 x 12.96 = 1600002.72, whose float32 product is ...2.75
    big = [[5, 2, 123457, 5, 0, 900, 1023, 61728500, 70000000, 4001]]
    assert zones.zone_rows("b.png", "sapin", 1024, 1024, big)[0][4:] == \
        ["123457", drv.stats_row("b.png", "sapin", 1024, 1024, 0, 123457)[5], "5", "0", "900", "1023", "500.000", "566.999", "14403.600",
         "1427.301", "1"]
    assert drv.stats_row("b.png", "sapin", 1024, 1024, 0, 123457)[5] == "1600002.75000"
    inner = [[11, 1, 4, 1, 1, 2, 2, 6, 6, 8]]                            # a 2x2 square away from the edges of a 10x10 map
    assert zones.zone_rows("c.png", "sapin", 10, 10, inner)[0][-1] == "0"
    for h, w, box in ((10, 10, (0, 1, 2, 2)), (10, 10, (1, 0, 2, 2)), (10, 10, (1, 1, 9, 2)), (10, 10, (1, 1, 2, 9)), (3, 10, (1, 1, 2, 2))):
        assert zones.zone_rows("c.png", "sapin", h, w, [[11, 1, 4, *box, 6, 6, 8]])[0][-1] == "1", (h, w, box)
    assert zones.zone_rows("c.png", "sapin", 10, 10, np.zeros((0, 10), dtype=np.int64)) == []


def test_summary_rows_and_folder_summary():
    assert zones.SUMMARY_COLUMNS == ["Name", "Type", "Bark zones", "Nodes", "Largest bark zone (mm^2)", "Largest node (mm^2)",
                                     "Mean node (mm^2)", "Nodes touching edge"]
    # nodes of 3 + 2 + 3 pixels: 8 x 12.96 / 3 = 34.56; all three touch an edge
    assert zones.summary_rows("a.png", "sapin", 6, 7, ZONES_6x7) == [["a.png", "sapin", "2", "3", "51.84000", "38.88000", "34.56000", "3"]]
    assert zones.summary_rows("b.png", "sapin", 10, 10, np.zeros((0, 10))) == [["b.png", "sapin", "0", "0", "", "", "", "0"]]
    only_bark = [[11, 1, 4, 1, 1, 2, 2, 6, 6, 8]]
    assert zones.summary_rows("c.png", "sapin", 10, 10, only_bark) == [["c.png", "sapin", "1", "0", "51.84000", "", "", "0"]]
    doc = zones.folder_summary([zones.image_figures(6, 7, ZONES_6x7), zones.image_figures(10, 10, np.zeros((0, 10)))], 1024, 1)
    assert doc == {"images": 2, "cap": 1024, "host_fallbacks": 1, "totals": {"bark_zones": 2, "nodes": 3, "nodes_touching_edge": 3},
                   "means": {"bark_zones_per_image": 1.0, "nodes_per_image": 1.5, "node_mm2": zones.area_mm2(8) / 3}}
    assert zones.folder_summary([], 7, 0)["means"] == {"bark_zones_per_image": None, "nodes_per_image": None, "node_mm2": None}


def test_report_files(tmp_path):
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}, {"name": "c.png", "wood": "epinette_gelee"}]
    allrows = np.array([[0, 6, 7, 5, 8], [1, 10, 10, 0, 0], [2, 10, 10, 4, 0]], dtype=np.int64)
    allz = np.array([[0] + r for r in ZONES_6x7] + [[2, 11, 1, 4, 1, 1, 2, 2, 6, 6, 8]], dtype=np.int64)
    doc = drv.write_zones_report(str(tmp_path), items, allrows, allz, 16, 0)
    assert sorted(os.listdir(tmp_path)) == ["zones.csv", "zones_summary.csv", "zones_summary.json"]
    table = [line.split("\t") for line in open(tmp_path / "zones.csv").read().splitlines()]
    assert table == [zones.ZONE_COLUMNS] + zones.zone_rows("a.png", "sapin", 6, 7, ZONES_6x7) + \
        zones.zone_rows("c.png", "epinette_gelee", 10, 10, [allz[5, 1:]])
    summary = [line.split("\t") for line in open(tmp_path / "zones_summary.csv").read().splitlines()]
    assert summary == [zones.SUMMARY_COLUMNS, ["a.png", "sapin", "2", "3", "51.84000", "38.88000", "34.56000", "3"],
                       ["b.png", "sapin", "0", "0", "", "", "", "0"], ["c.png", "epinette_gelee", "1", "0", "51.84000", "", "", "0"]]
    assert json.load(open(tmp_path / "zones_summary.json")) == json.loads(json.dumps(doc))
    assert doc["images"] == 3 and doc["cap"] == 16 and doc["totals"] == {"bark_zones": 3, "nodes": 3, "nodes_touching_edge": 3}


def _cli(*argv):
    return subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", "/nonexistent/folder"] + list(argv),
                          cwd=REPO, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("argv,text", [(["--zones", "--only_preprocess"], "refused with --only_preprocess"),
                                       (["--zones_cap", "8"], "--zones_cap needs --zones"),
                                       (["--zones", "--zones_cap", "0"], "--zones_cap must lie in 1..65536")])
def test_command_line_refusals(argv, text):
    p = _cli(*argv)
    assert p.returncode == 2 and text in p.stderr, (p.returncode, p.stderr[-500:])


def test_library_keywords_are_refused_alike():
    with pytest.raises(ValueError, match="--zones_cap needs --zones"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", zones_cap=4)
    with pytest.raises(ValueError, match="must lie in"):
        drv.predict_folder("/nonexistent/folder", "/nonexistent/ckpt.pt", zones=True, zones_cap=0)
    with pytest.raises(ValueError, match="--only_preprocess"):
        folder_run.check_zones_arguments(True, None, True)
    folder_run.check_zones_arguments(True, 1)
    folder_run.check_zones_arguments(False)


WIDTH = 1 + zones.ZONE_ROW
# scenario -> per rank, the (global index, zone count) of its images
SCENARIOS = {"empty_rank": [[(0, 0), (2, 0)], [(1, 5), (3, 1)]],         # rank 0 has images but not one zone
             "one_large": [[(0, 2), (3, 0)], [(1, 7), (2, 1)]]}          # image 1 alone has more rows than rank 0 in all


def _rows_of(images):
    out = [[g, 100 * g + k, 1 + (k & 1), k + 1, k, g, k + 3, g + 5, 7 * k, 11 * g, 4 + k] for g, n in images for k in range(n)]
    return np.array(out, dtype=np.int64).reshape(-1, WIDTH)


def _ragged_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for tag, per_rank in SCENARIOS.items():
            got = folder_run.gather_ragged(_rows_of(per_rank[rank]), world, dist, None, width=WIDTH)
            np.save(os.path.join(out_dir, "%s_%d.npy" % (tag, rank)), got)
    finally:
        dist.destroy_process_group()


def test_two_rank_gather_of_unequal_zone_row_counts(tmp_path):
    mp.spawn(_ragged_worker, args=(2, 29671, str(tmp_path)), nprocs=2, join=True)
    for tag, per_rank in SCENARIOS.items():
        everything = sorted(per_rank[0] + per_rank[1])
        want = folder_run.gather_ragged(_rows_of(everything), 1, None, None, width=WIDTH)        # what one rank yields
        assert want.tolist() == _rows_of(everything).tolist() and len(want) in (6, 10)
        for r in range(2):
            got = np.load(os.path.join(str(tmp_path), "%s_%d.npy" % (tag, r)))
            assert got.shape == want.shape and got.tolist() == want.tolist(), (tag, r)
    assert folder_run.gather_ragged(np.zeros((0, WIDTH), dtype=np.int64), 1, None, None, width=WIDTH).shape == (0, WIDTH)
