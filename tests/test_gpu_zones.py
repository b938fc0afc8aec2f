"""The zones of label maps on the GPU (csrc/zones.hip, nbc_label_zones, FCNResNet50.label_zones, predict --zones) against the
host restatement zones.zones_cpu (scipy.ndimage.label per class + numpy reductions, itself pinned by the hand-written answers
of test_zones_abi.py).  Integer work: every comparison is exact."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import synth, zones
from neuralbarkcalculator_amd.model import FCNResNet50

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def model(built_lib, sd_np):
    return FCNResNet50("bf16").load_state_dict(sd_np).to(DEV)


def run_gpu(model, labels_np, dtype=torch.uint8, cap=1024):
    """(rows [N,cap,10], num [N]) of FCNResNet50.label_zones; the labels must come back untouched."""
    t = torch.from_numpy(np.ascontiguousarray(labels_np)).to(dtype).to(DEV)
    before = t.clone()
    rows, num = model.label_zones(t, cap=cap)
    torch.cuda.synchronize()
    assert torch.equal(t, before)                                  # the labels are read only
    return rows.cpu().numpy(), num.cpu().numpy()


def run_with_sentinel(model, labels_np, dtype, cap):
    """The C entry point on a row buffer filled with a sentinel: what lies behind an image's last row must stay."""
    from neuralbarkcalculator_amd import _lib
    t = torch.from_numpy(np.ascontiguousarray(labels_np)).to(dtype).to(DEV)
    n, h, w = t.shape
    rows = torch.full((n, cap, zones.ZONE_ROW), SENTINEL, dtype=torch.int64, device=DEV)
    num = torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV)
    need = int(model._lib.nbc_zones_workspace_bytes(n, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    cur = torch.cuda.current_stream(DEV)
    rc = model._lib.nbc_label_zones(model._ctx, t.data_ptr(), _lib.LABEL_I64 if dtype == torch.int64 else _lib.LABEL_U8, n, h, w,
                                    rows.data_ptr(), cap, num.data_ptr(), ws.data_ptr(), need, cur.cuda_stream)
    _lib.check(rc, "nbc_label_zones")
    torch.cuda.synchronize()
    return rows.cpu().numpy(), num.cpu().numpy()


def assert_equal_oracle(rows, num, want, cap, what=""):
    for i, w in enumerate(want):
        assert int(num[i]) == len(w), f"{what} image {i}: {int(num[i])} zones, the oracle has {len(w)}"
        k = min(len(w), cap)
        if not np.array_equal(rows[i, :k], w[:k]):
            bad = np.flatnonzero((rows[i, :k] != w[:k]).any(axis=1))
            raise AssertionError(f"{what} image {i}: {len(bad)} of {k} rows differ, first {bad[0]}: got {rows[i, bad[0]].tolist()}, "
                                 f"want {w[bad[0]].tolist()}")


def blobs(seed, n, h, w, p_bg, smooth):
    """Random class maps with zones of every size: thresholded smoothed noise plus salt (test_gpu_small_zones.py's generator)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, h, w))
    for _ in range(smooth):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5.0
    q = np.quantile(f, [p_bg, p_bg + (1 - p_bg) * 0.6])
    lab = np.where(f < q[0], 0, np.where(f < q[1], 1, 2)).astype(np.uint8)
    salt = rng.random((n, h, w)) < 0.01
    lab[salt] = rng.integers(0, 3, size=int(salt.sum()), dtype=np.uint8)
    return lab


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("shape,p_bg,smooth", [((3, 200, 333), 0.5, 3), ((2, 33, 95), 0.3, 1), ((1, 31, 31), 0.5, 0),
                                              ((1, 64, 1), 0.5, 0), ((1, 1, 64), 0.5, 0), ((1, 520, 1024), 0.1, 8)])
def test_random_maps_equal_cpu_restatement(model, shape, p_bg, smooth, dtype):
    n, h, w = shape
    lab = blobs(sum(shape), n, h, w, p_bg, smooth)
    want = zones.zones_cpu(lab)
    cap = max(1, max(len(z) for z in want))
    rows, num = run_with_sentinel(model, lab, dtype, cap)
    assert_equal_oracle(rows, num, want, cap, str(shape))
    for i, z in enumerate(want):                                   # rows beyond an image's zones are not written
        assert (rows[i, len(z):] == SENTINEL).all()
    assert sum(len(z) for z in want) > 0


def test_other_label_values_belong_to_no_zone(model):
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 5, size=(2, 70, 45)).astype(np.uint8)    # 3 and 4: no zone, but a side towards them counts
    want = zones.zones_cpu(lab)
    rows, num = run_gpu(model, lab, cap=max(len(z) for z in want))
    assert_equal_oracle(rows, num, want, rows.shape[1])
    big = lab.astype(np.int64)
    big[lab == 3] = 257                                            # an int64 label whose low byte is 1
    big[lab == 4] = -1
    rows, num = run_gpu(model, big, torch.int64, cap=rows.shape[1])
    assert_equal_oracle(rows, num, want, rows.shape[1])


def test_many_random_small_maps(model):
    """Tile-border rules with two classes (runs touching across horizontal / vertical borders, diagonals through tile corners,
    a neighbour of the other class where the binary labelling had a set one): 300 random maps around the 32-pixel tile grid."""
    rng = np.random.default_rng(2025)
    for k in range(300):
        h = int(rng.integers(1, 100)); w = int(rng.integers(1, 100))
        if k % 3 == 0:
            h, w = int(rng.choice([31, 32, 33, 63, 64, 65, 96])), int(rng.choice([31, 32, 33, 63, 64, 65, 96]))
        dens = float(rng.choice([0.0, 0.1, 0.3, 0.41, 0.5, 0.7, 0.9]))     # the share of 0; each class near percolation at 0.2
        r = rng.random((h, w))
        lab = np.where(r < dens, 0, rng.integers(1, 3, size=(h, w))).astype(np.uint8)
        if k % 5 == 0:                                                  # one class only at 0.41: that class near percolation
            lab = np.minimum(lab, 1)
        want = zones.zones_cpu(lab)
        rows, num = run_gpu(model, lab, torch.int64 if k % 2 else torch.uint8, cap=max(1, len(want[0])))
        assert_equal_oracle(rows, num, want, rows.shape[1], f"case {k}: {h}x{w} density {dens}")


def worst_cases():
    h = w = 256
    spiral = np.zeros((h, w), np.uint8)
    y0, x0, y1, x1 = 0, 0, h - 1, w - 1
    while y0 <= y1 and x0 <= x1:
        spiral[y0, x0:x1 + 1] = 1; spiral[y0:y1 + 1, x1] = 1
        if y1 > y0: spiral[y1, x0 + 2:x1 + 1] = 1
        if x1 > x0 + 2: spiral[y0 + 2:y1 + 1, x0 + 2] = 1
        y0 += 2; x0 += 2; y1 -= 2; x1 -= 2
    comb = np.zeros((h, w), np.uint8); comb[:, ::2] = 2; comb[0, :] = 2
    yy, xx = np.mgrid[0:h, 0:w]
    checker = ((yy + xx) % 2 + 1).astype(np.uint8)
    return {"spiral": spiral, "comb": comb, "checker": checker, "zeros": np.zeros((h, w), np.uint8), "ones": np.ones((h, w), np.uint8)}


def test_worst_case_shapes(model):
    cases = worst_cases()
    want = {k: zones.zones_cpu(v) for k, v in cases.items()}
    assert len(want["checker"][0]) == 2 and want["checker"][0][:, 1].tolist() == [1, 2]     # two zones, one per class
    assert want["checker"][0][:, 2].tolist() == [32768, 32768]
    for name, lab in cases.items():
        rows, num = run_gpu(model, lab[None], cap=8)
        assert_equal_oracle(rows, num, want[name], 8, name)
        if name != "zeros" and name != "ones":                     # the classes swapped: the other class's path
            swapped = np.where(lab == 0, 0, 3 - lab).astype(np.uint8)
            rows, num = run_gpu(model, swapped[None], torch.int64, cap=8)
            assert_equal_oracle(rows, num, zones.zones_cpu(swapped), 8, name + " swapped")
    rows, num = run_gpu(model, cases["zeros"][None], cap=8)
    assert num.tolist() == [0]
    rows, num = run_gpu(model, cases["ones"][None], cap=8)
    assert num.tolist() == [1]
    assert rows[0, 0].tolist() == [0, 1, 65536, 0, 0, 255, 255, 255 * 128 * 256, 255 * 128 * 256, 1024]


def test_capacity_below_the_zone_count(model):
    lab = blobs(11, 3, 97, 130, 0.5, 1)
    want = zones.zones_cpu(lab)
    counts = [len(z) for z in want]
    cap = min(counts) // 2
    assert cap >= 4
    alloc = cap + 3                                                # three more rows behind every image's cap rows
    t = torch.from_numpy(lab).to(DEV)
    for dtype in (torch.uint8, torch.int64):
        rows, num = run_with_sentinel(model, lab, dtype, cap)
        assert num.tolist() == counts
        for i in range(3):
            assert np.array_equal(rows[i], want[i][:cap])
    # a buffer of [N, cap] rows with sentinel rows between the images: a row at index cap of image n would land on them
    from neuralbarkcalculator_amd import _lib
    buf = torch.full((3 * alloc, zones.ZONE_ROW), SENTINEL, dtype=torch.int64, device=DEV)
    num_t = torch.empty(3, dtype=torch.int64, device=DEV)
    need = int(model._lib.nbc_zones_workspace_bytes(1, 97, 130))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    for i in range(3):
        rc = model._lib.nbc_label_zones(model._ctx, t[i].data_ptr(), _lib.LABEL_U8, 1, 97, 130, buf[i * alloc:].data_ptr(), cap,
                                        num_t[i:].data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream(DEV).cuda_stream)
        _lib.check(rc, "nbc_label_zones")
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(3, alloc, zones.ZONE_ROW)
    assert num_t.tolist() == counts
    for i in range(3):
        assert np.array_equal(got[i, :cap], want[i][:cap]) and (got[i, cap:] == SENTINEL).all()


def test_a_batch_of_100_maps(model):
    rng = np.random.default_rng(17)
    labs = (rng.random((100, 48, 80)) < 0.45).astype(np.uint8) * rng.integers(1, 3, size=(100, 48, 80)).astype(np.uint8)
    want = zones.zones_cpu(labs)
    cap = max(len(z) for z in want)
    rows, num = run_gpu(model, labs, cap=cap)
    assert_equal_oracle(rows, num, want, cap)


def test_determinism_and_batch_independence(model):
    lab = blobs(23, 3, 150, 201, 0.4, 2)
    want = zones.zones_cpu(lab)
    cap = max(len(z) for z in want)
    a = run_with_sentinel(model, lab, torch.uint8, cap)
    b = run_with_sentinel(model, lab, torch.uint8, cap)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        for i in range(3):                                         # alone, on another stream
            rows, num = run_with_sentinel(model, lab[i:i + 1], torch.uint8, cap)
            assert rows[0].tobytes() == a[0][i].tobytes() and int(num[0]) == int(a[1][i])
    assert_equal_oracle(a[0], a[1], want, cap)


def test_on_network_labels(model):
    x = torch.from_numpy(np.stack([synth.make_input(60 + k, 512, 512) for k in range(2)])).to(DEV)
    labels, counts = model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
    rows, num = model.label_zones(labels, cap=4096)
    torch.cuda.synchronize()
    rows, num, counts = rows.cpu().numpy(), num.cpu().numpy(), counts.cpu().numpy()
    assert (num <= 4096).all()
    for i in range(2):
        z = rows[i, :int(num[i])]
        for c in (1, 2):
            assert int(z[z[:, 1] == c, 2].sum()) == int(counts[i, c])
    assert_equal_oracle(rows, num, zones.zones_cpu(labels.cpu().numpy()), 4096)


# ---- the folder driver ---------------------------------------------------------------------------------------------------
def _make_root(path, sizes):
    from PIL import Image
    d = os.path.join(path, "samples", "epinette_gelee")
    os.makedirs(d, exist_ok=True)
    for k, (h, w) in enumerate(sizes):
        img = (synth.make_input(300 + k, h, w).transpose(1, 2, 0) * 60 + 128).clip(0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(d, "z%02d.png" % k))
    return path


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _outputs(root):
    out = {}
    base = os.path.join(root, "results", "outputs")
    for wood in sorted(os.listdir(base)):
        for name in sorted(os.listdir(os.path.join(base, wood))):
            out[(wood, name)] = _read(os.path.join(base, wood, name))
    return out


def _expected_tables(root):
    """zones.csv and zones_summary.csv as zones_cpu and the formatters give them on the label PNGs the run wrote."""
    from PIL import Image
    table, summary = [zones.ZONE_COLUMNS], [zones.SUMMARY_COLUMNS]
    base = os.path.join(root, "results", "outputs")
    for wood in sorted(os.listdir(base)):
        for name in sorted(os.listdir(os.path.join(base, wood))):
            png = np.asarray(Image.open(os.path.join(base, wood, name)))
            lab = np.zeros(png.shape, np.uint8)
            lab[png == 127] = 1
            lab[png == 255] = 2
            z = zones.zones_cpu(lab)[0]
            table += zones.zone_rows(name, wood, lab.shape[0], lab.shape[1], z)
            summary += zones.summary_rows(name, wood, lab.shape[0], lab.shape[1], z)
    return table, summary


def _tables(root):
    res = os.path.join(root, "results")
    return (list(csv.reader(open(os.path.join(res, "zones.csv")), delimiter="\t")),
            list(csv.reader(open(os.path.join(res, "zones_summary.csv")), delimiter="\t")))


def test_folder_with_and_without_zones(built_lib, sd_np, tmp_path):
    from neuralbarkcalculator_amd.predict import predict_folder
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    sizes = [(256, 256), (256, 256), (200, 256), (256, 256), (200, 256)]
    kw = dict(precision="bf16", device_index=0, batch=2, target_size=256, calibrate=False)
    plain = _make_root(str(tmp_path / "plain"), sizes)
    predict_folder(plain, ckpt, **kw)
    assert not any(n.startswith("zones") for n in os.listdir(os.path.join(plain, "results")))

    full = _make_root(str(tmp_path / "full"), sizes)
    st = predict_folder(full, ckpt, zones=True, **kw)
    assert _read(os.path.join(full, "results", "final_stats.csv")) == _read(os.path.join(plain, "results", "final_stats.csv"))
    assert _outputs(full) == _outputs(plain) and len(_outputs(full)) == len(sizes)
    table, summary = _tables(full)
    want_table, want_summary = _expected_tables(full)
    assert table == want_table and summary == want_summary
    assert len(table) > 1 + len(sizes)                             # the synthetic frames have more than one zone each
    assert st["zones_host_fallbacks"] == 0
    doc = json.load(open(os.path.join(full, "results", "zones_summary.json")))
    assert doc["cap"] == 1024 and doc["host_fallbacks"] == 0 and doc["images"] == len(sizes)
    assert doc["totals"]["bark_zones"] + doc["totals"]["nodes"] == len(table) - 1

    tiny = _make_root(str(tmp_path / "tiny"), sizes)
    st1 = predict_folder(tiny, ckpt, zones=True, zones_cap=1, **kw)
    assert st1["zones_host_fallbacks"] > 0
    for name in ("zones.csv", "zones_summary.csv", "final_stats.csv"):
        assert _read(os.path.join(tiny, "results", name)) == _read(os.path.join(full, "results", name)), name
    doc1 = json.load(open(os.path.join(tiny, "results", "zones_summary.json")))
    assert doc1["cap"] == 1 and doc1["host_fallbacks"] == st1["zones_host_fallbacks"]
    assert {k: v for k, v in doc1.items() if k not in ("cap", "host_fallbacks")} == \
           {k: v for k, v in doc.items() if k not in ("cap", "host_fallbacks")}

    bark = _make_root(str(tmp_path / "bark"), sizes)
    predict_folder(bark, ckpt, zones=True, exclude_nodes=True, **kw)
    table_x, summary_x = _tables(bark)
    assert (table_x, summary_x) == _expected_tables(bark)
    assert len(table_x) > 1 and all(r[3] == "Bark" for r in table_x[1:]) and all(r[3] == "0" for r in summary_x[1:])


def test_folder_on_two_ranks(built_lib, sd_np, tmp_path):
    """Two gloo ranks sharing the GPU (as tests/test_gpu_dropout_votes.py sets them up): the ranks hold unequal numbers of zone
    rows, rank 0 writes what zones_cpu and the formatters give on the label PNGs."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = str(tmp_path / "ckpt.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    sizes = [(256, 256), (200, 256), (256, 256), (200, 256), (256, 256)]
    root = _make_root(str(tmp_path / "w2"), sizes)
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import predict\n"
            "dist.init_process_group('gloo')\n"
            "st = predict.predict_folder(%r, %r, precision='bf16', device_index=0, batch=2, target_size=256, calibrate=False, zones=True)\n"
            "assert st['world'] == 2 and st['images_total'] == %d and st['zones_host_fallbacks'] == 0\n"
            "dist.destroy_process_group()\n" % (repo, root, ckpt, len(sizes)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29677", str(script)],
                       cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    table, summary = _tables(root)
    assert (table, summary) == _expected_tables(root) and len(summary) == 1 + len(sizes) and len(table) > 1 + len(sizes)
    doc = json.load(open(os.path.join(root, "results", "zones_summary.json")))
    assert doc["images"] == len(sizes) and doc["totals"]["bark_zones"] + doc["totals"]["nodes"] == len(table) - 1
