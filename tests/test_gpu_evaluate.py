"""The evaluation path on the GPU: nbc_confusion against np.bincount, and the labelled-folder driver
(neuralbarkcalculator_amd/evaluate.py) against the metrics of the CPU oracle's labels."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd.postprocess import remove_small_zones

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def _want(labels: np.ndarray, grey: np.ndarray) -> np.ndarray:
    """np.bincount(3 t + p) per image, labels outside {0,1,2} dropped: int64 [N,3,3]."""
    out = []
    for lab, g in zip(labels, grey):
        p = lab.astype(np.int64).ravel()
        t = metrics.target_classes(g).astype(np.int64).ravel()
        ok = (p >= 0) & (p < 3)
        out.append(np.bincount(3 * t[ok] + p[ok], minlength=9).reshape(3, 3))
    return np.stack(out)


def _call(lib, labels: torch.Tensor, grey: torch.Tensor, n, h, w, conf_ptr):
    dt = _lib.LABEL_I64 if labels.dtype == torch.int64 else _lib.LABEL_U8
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(lib.nbc_confusion(labels.data_ptr(), dt, grey.data_ptr(), n, h, w, conf_ptr, stream), "nbc_confusion")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (7, 13), (33, 65), (520, 1024), (731, 977), (1024, 1024)])
def test_confusion_equals_bincount(built_lib, dtype, n, hw):
    """Every grey level, labels in {0,1,2} with out-of-range values sprinkled in (counted nowhere), a single-class image,
    odd H*W (so later images start unaligned), and 64 sentinel bytes on each side of the output left untouched."""
    h, w = hw
    rng = np.random.default_rng(h * 7919 + w * 31 + n)
    grey = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    grey.reshape(-1)[: min(256, grey.size)] = np.arange(min(256, grey.size), dtype=np.uint8)
    lab = rng.integers(0, 3, size=(n, h, w)).astype(np.int64)
    bad = rng.random((n, h, w)) < 0.05
    if dtype == torch.uint8:
        lab[bad] = rng.choice([3, 7, 128, 255], size=int(bad.sum()))
    else:
        lab[bad] = rng.choice([3, -1, 256, 1 << 40, -(1 << 62)], size=int(bad.sum()))
    if n == 3:
        lab[1] = 2                                                    # a single-class image
    labels = torch.from_numpy(lab).to(dtype).to(DEV)
    target = torch.from_numpy(grey).to(DEV)
    guard = 8
    buf = torch.full((n * 9 + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    _call(built_lib, labels, target, n, h, w, buf.data_ptr() + guard * 8)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:guard] == 0x5A5A5A5A5A5A5A5A).all() and (got[guard + n * 9:] == 0x5A5A5A5A5A5A5A5A).all()
    want = _want(lab.astype(np.uint8) if dtype == torch.uint8 else lab, grey)
    np.testing.assert_array_equal(got[guard: guard + n * 9].reshape(n, 3, 3), want)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_confusion_with_buffers_not_16_byte_aligned(built_lib, dtype):
    """Labels and target starting at odd addresses (and at different offsets from a 16-byte boundary): the body of
    16-byte loads is left to the scalar path where it cannot be aligned for both."""
    n, h, w = 2, 37, 41
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 3, size=(n, h, w))
    grey = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    want = _want(lab, grey)
    for lab_off, tgt_off in ((1, 0), (0, 3), (5, 5)):
        big_l = torch.zeros(n * h * w + 8, dtype=dtype, device=DEV)
        big_t = torch.zeros(n * h * w + 8, dtype=torch.uint8, device=DEV)
        big_l[lab_off: lab_off + n * h * w] = torch.from_numpy(lab.ravel()).to(dtype).to(DEV)
        big_t[tgt_off: tgt_off + n * h * w] = torch.from_numpy(grey.ravel()).to(DEV)
        conf = torch.empty((n, 3, 3), dtype=torch.int64, device=DEV)
        _call(built_lib, big_l[lab_off:], big_t[tgt_off:], n, h, w, conf.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(conf.cpu().numpy(), want, err_msg=str((lab_off, tgt_off)))


@pytest.fixture(scope="module")
def model32(sd_np, built_lib):
    from neuralbarkcalculator_amd.model import FCNResNet50
    return FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)


def test_model_confusion_validates_and_orders_after_the_producer_on_its_stream(model32):
    m = model32
    h, w = 512, 1024
    rng = np.random.default_rng(9)
    grey = torch.from_numpy(rng.integers(0, 256, size=(h, w), dtype=np.uint8)).to(DEV)
    src = torch.from_numpy(rng.integers(0, 3, size=(h, w)).astype(np.uint8)).to(DEV)
    labels = torch.full((h, w), 255, dtype=torch.uint8, device=DEV)     # counted nowhere until the producer has run
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)                                   # the producer is late on its stream
        labels.copy_(src)
        conf = m.confusion(labels, grey)
    s.synchronize()
    assert conf.shape == (1, 3, 3) and conf.dtype == torch.int64
    np.testing.assert_array_equal(conf.cpu().numpy(), _want(src.cpu().numpy()[None], grey.cpu().numpy()[None]))
    with pytest.raises(ValueError):
        m.confusion(labels.float(), grey)
    with pytest.raises(ValueError):
        m.confusion(labels, grey.to(torch.int64))
    with pytest.raises(ValueError):
        m.confusion(labels[:, :-1], grey[:, :-1])                        # not contiguous
    with pytest.raises(ValueError):
        m.confusion(labels, grey[:-1])                                  # shapes differ
    with pytest.raises(ValueError):
        m.confusion(labels.cpu(), grey.cpu())                           # wrong device
    with pytest.raises(ValueError):
        m.confusion(labels[None, None], grey[None, None])               # 4-D


# ---- end to end ------------------------------------------------------------------------------------------------------
BANDS = [(0, 63), (64, 191), (192, 255)]
LAYOUT = [("epinette_gelee", "a01.bmp", 70, 128, 128), ("epinette_gelee", "a02.png", 71, 96, 128),
          ("epinette_gelee", "bmp_a03.bmp", 72, 136, 128), ("epinette_non_gelee", "n1.png", 73, 128, 128),
          ("epinette_non_gelee", "n2.png", 74, 96, 128), ("sapin", "s1.png", 75, 128, 128),
          ("sapin", "s2_nodual.png", 76, 96, 128), ("sapin", "s3_mismatch.png", 77, 128, 128)]


@pytest.fixture(scope="module")
def labelled(tmp_path_factory, sd_np, oracle_model):
    """Eight samples from synth.make_frame, six duals made from the CPU oracle's labels with some pixels perturbed and the
    classes written as grey levels spread over all three decode bands; one sample without a dual, one whose dual is
    narrower than its sample.  Returns (root, checkpoint, {(wood, name): (frame, grey, oracle raw labels)})."""
    from oracle.fcn_resnet50_oracle import predict_labels
    root = str(tmp_path_factory.mktemp("labelled"))
    rng = np.random.default_rng(2024)
    truth = {}
    for wood, fname, idx, h, w in LAYOUT:
        name = fname.replace("bmp", "png")
        os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
        os.makedirs(os.path.join(root, "duals", wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, fname))
        if "nodual" in name:
            continue
        x = torch.from_numpy(synth.normalize_frame(img))[None]
        lab = predict_labels(oracle_model, x)[0][0].numpy().astype(np.uint8)
        cls = lab.copy()
        flip = rng.random(cls.shape) < 0.08
        cls[flip] = rng.integers(0, 3, size=int(flip.sum()))
        lo = np.array([b[0] for b in BANDS])[cls]
        hi = np.array([b[1] for b in BANDS])[cls]
        grey = (lo + (rng.random(cls.shape) * (hi - lo + 1)).astype(np.int64)).astype(np.uint8)
        assert np.array_equal(metrics.target_classes(grey), cls)
        if "mismatch" in name:
            grey = np.ascontiguousarray(grey[:, : w - 8])
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
        truth[(wood, name)] = (img, grey, lab)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    return root, ckpt, truth


def _read_csv(root):
    return list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))


def _check_against_labels(root, truth, sd_np, precision):
    """Every CSV row equals metrics.py on this precision's own labels (the counting is exact), and those labels equal the
    oracle's but for exact-tie flips (then the row equals the oracle's too)."""
    from neuralbarkcalculator_amd.model import FCNResNet50
    m = FCNResNet50(precision).load_state_dict(sd_np).to(DEV)
    rows = _read_csv(root)
    assert rows[0] == metrics.EVAL_CSV_HEADER
    names = [(r[1], r[0]) for r in rows[1:]]
    assert names == [(w, n.replace("bmp", "png")) for w, n, *_ in LAYOUT if "nodual" not in n and "mismatch" not in n]
    flips = 0
    for r in rows[1:]:
        img, grey, lab_ref = truth[(r[1], r[0])]
        lab = m.predict_labels(torch.from_numpy(img[None]).to(DEV), labels_dtype=torch.uint8)[0][0].cpu().numpy()
        t = metrics.target_classes(grey)
        assert r == metrics.eval_row(r[0], r[1], metrics.confusion_numpy(lab, t), metrics.confusion_numpy(remove_small_zones(lab), t))
        n_flip = int((lab != lab_ref).sum())
        flips += n_flip
        ref = metrics.eval_row(r[0], r[1], metrics.confusion_numpy(lab_ref, t), metrics.confusion_numpy(remove_small_zones(lab_ref), t))
        if n_flip == 0:
            assert r == ref
    assert flips <= 4, flips
    return rows


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_evaluate_folder_matches_the_oracle(labelled, sd_np, precision):
    root, ckpt, truth = labelled
    st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0)
    assert st["images_total"] == len(LAYOUT) and st["images_evaluated_this_rank"] == 6
    _check_against_labels(root, truth, sd_np, precision)
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["precision"] == precision and summary["model_path"] == ckpt
    assert summary["images_evaluated"] == 6 and summary["images_skipped"] == 2
    assert summary["skipped"] == {"no_dual": ["sapin/s2_nodual.png"], "shape_mismatch": ["sapin/s3_mismatch.png"], "too_large": []}
    rows = _read_csv(root)[1:]
    for j, col in enumerate(metrics.EVAL_CSV_HEADER[3:], start=3):
        assert summary["column_means"][col] == pytest.approx(np.mean([float(r[j]) for r in rows]))
    raw = sum(np.asarray(r[4:13]).reshape(3, 3) for r in st["rows"] if r[3] == ev.STATUS_OK)
    clean = sum(np.asarray(r[13:22]).reshape(3, 3) for r in st["rows"] if r[3] == ev.STATUS_OK)
    assert summary["pooled"]["iou_bark"] == pytest.approx(metrics.iou(raw)[1], abs=1e-12)
    assert summary["pooled"]["f1_node"] == pytest.approx(metrics.f1(clean)[2], abs=1e-12)
    assert not os.path.exists(os.path.join(root, "processed"))


def test_evaluate_bf16_counts_every_pixel(labelled):
    root, ckpt, _ = labelled
    st = ev.evaluate_folder(root, ckpt, precision="bf16", device_index=0)
    ok = [r for r in st["rows"] if r[3] == ev.STATUS_OK]
    assert len(ok) == 6
    for r in ok:
        assert sum(r[4:13]) == r[1] * r[2] and sum(r[13:22]) == r[1] * r[2]
    assert json.load(open(os.path.join(root, ev.SUMMARY_JSON)))["precision"] == "bf16"


def test_two_rank_rehearsal_and_cli_match_the_library_call(labelled, tmp_path):
    """Two ranks (torch.distributed.run, gloo) on one GPU write the CSV one rank writes; so does the CLI."""
    root, ckpt, _ = labelled
    ev.evaluate_folder(root, ckpt, precision="f16x2", device_index=0)
    want = open(os.path.join(root, ev.STATS_CSV)).read()
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import evaluate\n"
            "dist.init_process_group('gloo')\n"
            "st = evaluate.evaluate_folder(%r, %r, precision='f16x2', device_index=0)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, root, ckpt, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29687", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(os.path.join(root, ev.STATS_CSV)).read() == want
    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", root, "--model_path", ckpt, "--precision", "f16x2",
                        "--streams", "2"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(os.path.join(root, ev.STATS_CSV)).read() == want
    assert "evaluated 6 images in f16x2" in p.stdout and "no_dual: sapin/s2_nodual.png" in p.stdout
