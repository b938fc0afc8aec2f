"""Dataset statistics on the GPU: nbc_image_moments / nbc_target_counts against numpy's integer sums, the stats folder
driver against what the decoded files give on the host, and the --mean / --std / --stats normalisation in the predict and
evaluate drivers."""
import csv
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd import stats as st
from neuralbarkcalculator_amd.postprocess import remove_small_zones

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 8
SHAPES = [(1, 1), (7, 13), (33, 65), (520, 1024), (731, 977), (1024, 1024), (1500, 2048)]
PAIR = ((0.52, 0.47, 0.61), (0.21, 0.16, 0.19))     # far from models.py:208-209


def _want_moments(x: np.ndarray) -> np.ndarray:
    """numpy uint64 sums per image and channel: [N,3,2]."""
    v = x.reshape(x.shape[0], -1, 3).astype(np.uint64)
    return np.stack([v.sum(axis=1), (v * v).sum(axis=1)], axis=-1)


def _want_counts(g: np.ndarray) -> np.ndarray:
    out = []
    for a in g:
        off = int(((a != 0) & (a != 127) & (a != 255)).sum())
        out.append(list(np.bincount(metrics.target_classes(a).ravel(), minlength=3)) + [off])
    return np.asarray(out, dtype=np.int64)


def _guarded(n_cells):
    return torch.full((n_cells + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)


def _check_guarded(buf, n_cells):
    got = buf.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n_cells:] == SENTINEL).all()
    return got[GUARD: GUARD + n_cells]


def _moments_call(lib, x: torch.Tensor, n, h, w, out_ptr):
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(lib.nbc_image_moments(x.data_ptr(), n, h, w, out_ptr, stream), "nbc_image_moments")


def _counts_call(lib, g: torch.Tensor, n, h, w, out_ptr):
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(lib.nbc_target_counts(g.data_ptr(), n, h, w, out_ptr, stream), "nbc_target_counts")


# ---- 5. nbc_image_moments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_image_moments_equal_numpy_sums(built_lib, n, hw):
    """Random bytes; sentinel words on both sides of the output stay; the input at offsets 0, 1, 3 and 5 from a 16-byte
    boundary (with odd H*W*3 the later images of a batch start unaligned anyway); each image alone gives the six numbers
    it gives in the batch."""
    h, w = hw
    rng = np.random.default_rng(h * 7919 + w * 31 + n)
    x = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    want = _want_moments(x).astype(np.int64)
    size = x.size
    for off in (0, 1, 3, 5):
        big = torch.zeros(size + 16, dtype=torch.uint8, device=DEV)
        assert big.data_ptr() % 16 == 0
        big[off: off + size] = torch.from_numpy(x.ravel()).to(DEV)
        buf = _guarded(n * 6)
        _moments_call(built_lib, big[off:], n, h, w, buf.data_ptr() + GUARD * 8)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_check_guarded(buf, n * 6).reshape(n, 3, 2), want, err_msg="offset %d" % off)
    xd = torch.from_numpy(x).to(DEV)
    for i in range(n):
        alone = st.image_moments(xd[i])
        assert alone.shape == (1, 3, 2) and alone.dtype == torch.int64
        np.testing.assert_array_equal(alone.cpu().numpy()[0], want[i])


def test_image_moments_of_the_largest_sums(built_lib):
    """All-255 frames: 16 x 65025 per chunk and slot, the case a 32-bit running sum of squares cannot carry."""
    for n, h, w in ((2, 1024, 1024), (1, 4096, 4096)):
        x = torch.full((n, h, w, 3), 255, dtype=torch.uint8, device=DEV)
        got = st.image_moments(x).cpu().numpy()
        p = h * w
        assert got.tolist() == [[[255 * p, 65025 * p]] * 3] * n, (n, h, w)
        del x


# ---- 6. nbc_target_counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_target_counts_equal_bincount(built_lib, n, hw):
    """Every grey level present (where the image has 256 pixels), a single-level image in the batch of three, guarded
    output, unaligned starts."""
    h, w = hw
    rng = np.random.default_rng(h * 104729 + w * 17 + n)
    g = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    g.reshape(-1)[: min(256, g.size)] = np.arange(min(256, g.size), dtype=np.uint8)
    exact = rng.random((n, h, w)) < 0.3
    g[exact] = rng.choice(np.array([0, 127, 255], np.uint8), size=int(exact.sum()))
    if n == 3:
        g[1] = 127
    want = _want_counts(g)
    assert (want[:, :3].sum(axis=1) == h * w).all()
    for off in (0, 1, 3, 5):
        big = torch.zeros(g.size + 16, dtype=torch.uint8, device=DEV)
        big[off: off + g.size] = torch.from_numpy(g.ravel()).to(DEV)
        buf = _guarded(n * 4)
        _counts_call(built_lib, big[off:], n, h, w, buf.data_ptr() + GUARD * 8)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_check_guarded(buf, n * 4).reshape(n, 4), want, err_msg="offset %d" % off)
    gd = torch.from_numpy(g).to(DEV)
    for i in range(n):
        np.testing.assert_array_equal(st.target_counts(gd[i]).cpu().numpy()[0], want[i])


# ---- 7. the wrappers -------------------------------------------------------------------------------------------------
def test_wrappers_validate_and_order_after_the_producer_on_their_stream(built_lib):
    h, w = 512, 1024
    rng = np.random.default_rng(9)
    src_x = torch.from_numpy(rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)).to(DEV)
    src_g = torch.from_numpy(rng.integers(0, 256, size=(2, h, w), dtype=np.uint8)).to(DEV)
    x = torch.zeros_like(src_x)
    g = torch.zeros_like(src_g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)                                   # the producer is late on its stream
        x.copy_(src_x)
        g.copy_(src_g)
        mom = st.image_moments(x)
        cnt = st.target_counts(g)
    s.synchronize()
    assert mom.shape == (2, 3, 2) and mom.dtype == torch.int64 and cnt.shape == (2, 4) and cnt.dtype == torch.int64
    np.testing.assert_array_equal(mom.cpu().numpy(), _want_moments(src_x.cpu().numpy()).astype(np.int64))
    np.testing.assert_array_equal(cnt.cpu().numpy(), _want_counts(src_g.cpu().numpy()))
    for bad in (x.float(), x[:, :, :-1], x.cpu(), x[..., :2].contiguous(), x[None], x[0, 0]):
        with pytest.raises(ValueError):
            st.image_moments(bad)
    for bad in (g.to(torch.int64), g[:, :, :-1], g.cpu(), g[None, None], g[0, 0]):
        with pytest.raises(ValueError):
            st.target_counts(bad)


# ---- 8. the folder driver ---------------------------------------------------------------------------------------------
STATS_LAYOUT = [("epinette_gelee", "a01.bmp", 80, 128, 128), ("epinette_gelee", "a02.png", 81, 96, 128),
                ("epinette_gelee", "bmp_a03.bmp", 82, 1100, 64), ("epinette_non_gelee", "n1.png", 83, 128, 128),
                ("epinette_non_gelee", "n2.png", 84, 96, 128), ("epinette_non_gelee", "n3.png", 85, 37, 41),
                ("sapin", "s1.png", 86, 128, 128), ("sapin", "s2_nodual.png", 87, 96, 128),
                ("sapin", "s3_mismatch.png", 88, 128, 128), ("sapin", "s4.png", 89, 128, 128)]


@pytest.fixture(scope="module")
def stats_root(tmp_path_factory):
    """Ten samples of four shapes (one of 1100 rows), eight usable duals with every grey level, one sample without a dual,
    one dual narrower than its sample."""
    root = str(tmp_path_factory.mktemp("stats"))
    rng = np.random.default_rng(77)
    for wood, fname, idx, h, w in STATS_LAYOUT:
        name = fname.replace("bmp", "png")
        os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
        os.makedirs(os.path.join(root, "duals", wood), exist_ok=True)
        Image.fromarray(synth.make_frame(idx, h, w), mode="RGB").save(os.path.join(root, "samples", wood, fname))
        if "nodual" in name:
            continue
        grey = rng.choice(np.array([0, 127, 255], np.uint8), size=(h, w), p=[0.7, 0.2, 0.1])
        stray = rng.random((h, w)) < 0.02
        grey[stray] = rng.integers(0, 256, size=int(stray.sum()), dtype=np.uint8)
        if "mismatch" in name:
            grey = np.ascontiguousarray(grey[:, : w - 8])
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
    return root


def _host_truth(root):
    """JSON and CSV text from the decoded files alone: numpy uint64 sums and fractions.Fraction."""
    items = ev.list_labelled(root)
    means, stds, csv_rows = [], [], []
    counts, off_level, with_dual, skipped = [0, 0, 0], 0, 0, {"no_dual": [], "shape_mismatch": []}
    for d in items:
        img = np.array(Image.open(d["src"]).convert("RGB"))
        h, w = img.shape[:2]
        p = h * w
        v = img.reshape(-1, 3).astype(np.uint64)
        s1, s2 = [int(a) for a in v.sum(axis=0)], [int(a) for a in (v * v).sum(axis=0)]
        mean = [float(Fraction(a, 255 * p)) for a in s1]
        std = [math.sqrt(float(Fraction(p * b - a * a, p * (p - 1) * 65025))) for a, b in zip(s1, s2)]
        means.append(mean)
        stds.append(std)
        cells = ["", "", "", ""]
        grey = np.array(Image.open(d["dual"]).convert("L")) if os.path.isfile(d["dual"]) else None
        if grey is None:
            skipped["no_dual"].append(d["wood"] + "/" + d["name"])
        elif grey.shape != (h, w):
            skipped["shape_mismatch"].append(d["wood"] + "/" + d["name"])
        else:
            c = _want_counts(grey[None])[0]
            for y in range(3):
                counts[y] += int(c[y])
            off_level += int(c[3])
            with_dual += 1
            cells = [str(int(a)) for a in c]
        csv_rows.append([d["name"], d["wood"], str(h), str(w)] + [repr(a) for a in mean + std] + cells)
    n = len(items)
    total = sum(counts)
    summary = {"mean": [math.fsum(m[c] for m in means) / n for c in range(3)],
               "std": [math.fsum(s[c] for s in stds) / n for c in range(3)],
               "class_counts": counts, "pos_weight": [total / (3 * c) if c else None for c in counts],
               "off_level_pixels": off_level, "images": n, "images_with_dual": with_dual, "skipped": skipped}
    return summary, [st.CSV_HEADER] + csv_rows


def test_stats_folder_equals_the_host_truth(stats_root, built_lib):
    root = stats_root
    want_summary, want_csv = _host_truth(root)
    assert want_summary["skipped"] == {"no_dual": ["sapin/s2_nodual.png"], "shape_mismatch": ["sapin/s3_mismatch.png"]}
    assert want_summary["off_level_pixels"] > 0 and all(c > 0 for c in want_summary["class_counts"])
    for kw in (dict(), dict(batch=1, streams=1), dict(batch=3, streams=2, window=4)):
        run = st.stats_folder(root, device_index=0, **kw)
        assert run["images_total"] == len(STATS_LAYOUT) and run["summary"] == want_summary
        assert json.load(open(os.path.join(root, st.STATS_JSON))) == want_summary
        assert list(csv.reader(open(os.path.join(root, st.STATS_CSV)), delimiter="\t")) == want_csv
    assert not os.path.exists(os.path.join(root, "processed"))


def test_two_rank_stats_and_cli_write_the_same_files(stats_root, tmp_path):
    root = stats_root
    st.stats_folder(root, device_index=0)
    want = [open(os.path.join(root, p), "rb").read() for p in (st.STATS_JSON, st.STATS_CSV)]
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import stats\n"
            "dist.init_process_group('gloo')\n"
            "run = stats.stats_folder(%r, device_index=0, batch=2)\n"
            "assert run['world'] == 2 and run['images_total'] == %d and 0 < run['images_this_rank'] < %d\n"
            "dist.destroy_process_group()\n" % (REPO, root, len(STATS_LAYOUT), len(STATS_LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    for p in (st.STATS_JSON, st.STATS_CSV):
        os.remove(os.path.join(root, p))
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29691", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [open(os.path.join(root, q), "rb").read() for q in (st.STATS_JSON, st.STATS_CSV)] == want
    for q in (st.STATS_JSON, st.STATS_CSV):
        os.remove(os.path.join(root, q))
    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.stats", root, "--streams", "2"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert [open(os.path.join(root, q), "rb").read() for q in (st.STATS_JSON, st.STATS_CSV)] == want
    assert "10 images, 8 with a usable dual" in p.stdout and "no_dual: sapin/s2_nodual.png" in p.stdout


# ---- 9. the normalisation on the device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model32(sd_np, built_lib):
    from neuralbarkcalculator_amd.model import FCNResNet50
    return FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)


def test_uint8_ingest_with_another_pair_equals_float_input(sd_np, built_lib):
    """The non-default twin of test_uint8_ingest_equals_float_input: ToTensor + Normalize(mean, std) bit-exactly."""
    from neuralbarkcalculator_amd.model import FCNResNet50
    m = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    img = np.stack([synth.make_frame(11, 136, 200), synth.make_frame(12, 136, 200)])
    xu = torch.from_numpy(img).to(DEV)
    default = m(xu)
    m.set_normalization(*PAIR)
    xf = torch.from_numpy(np.stack([synth.normalize_frame(i, *PAIR) for i in img])).to(DEV)
    a, b = m(xf), m(xu)
    assert torch.equal(a, b)
    assert not torch.equal(b, default)
    clone = m.clone_shared()                        # a clone starts on the defaults: why bring_up sets every object
    assert torch.equal(clone(xu), default)


def _dark(img):
    """A frame far from the default mean: every byte halved."""
    return (img >> 1).astype(np.uint8)


EVAL_LAYOUT = [("epinette_gelee", "a01.bmp", 90, 128, 128), ("epinette_gelee", "a02.png", 91, 96, 128),
               ("epinette_non_gelee", "n1.png", 92, 128, 128), ("epinette_non_gelee", "n2.png", 93, 96, 128),
               ("sapin", "s1.png", 94, 128, 128), ("sapin", "s2.png", 95, 136, 128), ("sapin", "s3.png", 96, 128, 128)]


@pytest.fixture(scope="module")
def dark_labelled(tmp_path_factory, sd_np):
    """Seven dark samples with a dual each (grey levels from the green channel: every class occurs) and the checkpoint."""
    root = str(tmp_path_factory.mktemp("dark"))
    frames = {}
    for wood, fname, idx, h, w in EVAL_LAYOUT:
        name = fname.replace("bmp", "png")
        os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
        os.makedirs(os.path.join(root, "duals", wood), exist_ok=True)
        img = _dark(synth.make_frame(idx, h, w))
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, fname))
        Image.fromarray(np.ascontiguousarray(img[..., 1] * 2), mode="L").save(os.path.join(root, "duals", wood, name))
        frames[(wood, name)] = img
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    return root, ckpt, frames


def _eval_csv(root):
    return open(os.path.join(root, ev.STATS_CSV)).read()


def test_evaluate_folder_with_a_pair_reaches_every_stream(dark_labelled, built_lib):
    root, ckpt, _ = dark_labelled
    one = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, batch=1, streams=1, normalization=PAIR)
    csv_one = _eval_csv(root)
    many = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, batch=1, streams=3, normalization=PAIR)
    assert many["rows"] == one["rows"] and _eval_csv(root) == csv_one
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["normalization"] == {"mean": list(PAIR[0]), "std": list(PAIR[1]), "source": "arguments"}
    assert summary["images_evaluated"] == len(EVAL_LAYOUT)
    plain = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, batch=1, streams=3)
    assert plain["rows"] != one["rows"]                                  # the option is not a no-op
    assert "normalization" not in json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert [r[:4] for r in plain["rows"]] == [r[:4] for r in one["rows"]]


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_predict_folder_with_a_pair_writes_what_the_model_gives(dark_labelled, sd_np, built_lib, precision, tmp_path):
    from neuralbarkcalculator_amd.model import FCNResNet50
    src_root, ckpt, frames = dark_labelled
    root = str(tmp_path)
    for wood, fname, *_ in EVAL_LAYOUT:
        os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
        with open(os.path.join(src_root, "samples", wood, fname), "rb") as f, \
                open(os.path.join(root, "samples", wood, fname), "wb") as g:
            g.write(f.read())
    drv.predict_folder(root, ckpt, precision=precision, device_index=0, streams=3, batch=2, normalization=PAIR)
    m = FCNResNet50(precision).load_state_dict(sd_np).to(DEV)
    default_differs = 0
    rows = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert len(rows) == 1 + len(EVAL_LAYOUT)
    for row in rows[1:]:
        img = frames[(row[1], row[0])]
        assert img.shape[0] != img.shape[1] or np.array_equal(drv.preprocess_image(img), img)   # nothing trimmed
        x = torch.from_numpy(img[None]).to(DEV)
        m.set_normalization(*PAIR)
        lab = remove_small_zones(m.predict_labels(x, labels_dtype=torch.uint8)[0][0].cpu().numpy())
        got = np.asarray(Image.open(os.path.join(root, "results", "outputs", row[1], row[0])))
        assert np.array_equal(got, drv.label_png(lab)), row[:2]
        assert row == drv.stats_row(row[0], row[1], lab.shape[0], lab.shape[1], int((lab == 1).sum()), int((lab == 2).sum()))
        m.set_normalization(synth.DEFAULT_MEAN, synth.DEFAULT_STD)
        default_differs += int((m.predict_labels(x, labels_dtype=torch.uint8)[0][0].cpu().numpy() != lab).sum())
    assert default_differs > 0


# ---- 10. end to end ---------------------------------------------------------------------------------------------------
def test_stats_then_evaluate_with_the_file_equals_the_numbers_typed_out(dark_labelled, built_lib):
    root, ckpt, _ = dark_labelled
    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.stats", root], cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    path = os.path.join(root, st.STATS_JSON)
    doc = json.load(open(path))
    assert doc["images"] == doc["images_with_dual"] == len(EVAL_LAYOUT) and all(0.1 < v < 0.5 for v in doc["mean"])
    base = [sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", root, "--model_path", ckpt, "--precision", "fp32"]
    p = subprocess.run(base + ["--stats", path], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    from_file, summary_file = _eval_csv(root), json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert "normalised with mean" in p.stdout and path in p.stdout
    p = subprocess.run(base + ["--mean"] + [repr(v) for v in doc["mean"]] + ["--std"] + [repr(v) for v in doc["std"]],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    typed, summary_typed = _eval_csv(root), json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert typed == from_file
    assert summary_file["normalization"] == {"mean": doc["mean"], "std": doc["std"], "source": path}
    assert summary_typed["normalization"] == {"mean": doc["mean"], "std": doc["std"], "source": "arguments"}
    assert {k: v for k, v in summary_file.items() if k != "normalization"} == \
           {k: v for k, v in summary_typed.items() if k != "normalization"}
