"""Evaluation metrics from confusion counts (neuralbarkcalculator_amd/metrics.py) against direct restatements of the
reference's definitions, the dual discovery and skip rules of the evaluation driver, and its row gather over gloo."""
import csv
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import metrics


def lovasz_iou(pred, label, C=3, EMPTY=1.0):
    """lovasz_losses.py:54-73 for one image, on label maps (the argmax already taken)."""
    out = []
    for i in range(C):
        inter = ((label == i) & (pred == i)).sum()
        union = ((label == i) | (pred == i)).sum()
        out.append(EMPTY if not union else float(inter) / float(union))
    return 100 * np.array(out)


def sklearn021_f1(y_true, y_pred):
    """f1_score(y_true, y_pred, labels=[0, 1, 2], average=None) of scikit-learn 0.21 (precision_recall_fscore_support:
    multilabel_confusion_matrix sums, _prf_divide's zero-denominator -> 0, denom[denom == 0] = 1), then the absent-class
    rule of utils.py:222-226."""
    tp = np.array([((y_true == c) & (y_pred == c)).sum() for c in range(3)], dtype=np.float64)
    pred_sum = np.array([(y_pred == c).sum() for c in range(3)], dtype=np.float64)
    true_sum = np.array([(y_true == c).sum() for c in range(3)], dtype=np.float64)

    def prf_divide(num, den):
        mask = den == 0.0
        den = den.copy()
        den[mask] = 1
        res = num / den
        res[mask] = 0.0
        return res
    precision, recall = prf_divide(tp, pred_sum), prf_divide(tp, true_sum)
    beta2 = 1.0
    denom = beta2 * precision + recall
    denom[denom == 0.0] = 1
    scores = (1 + beta2) * precision * recall / denom
    targets_count = np.bincount(y_true, minlength=3)
    outputs_count = np.bincount(y_pred, minlength=3)
    for i, count_i in enumerate(targets_count):
        if count_i == 0 and outputs_count[i] == 0:
            scores[i] = np.delete(scores, i).mean()
    return scores * 100


def _random_maps(rng, h, w, classes=(0, 1, 2)):
    t = rng.choice(classes, size=(h, w))
    p = t.copy()
    flip = rng.random((h, w)) < rng.uniform(0.0, 0.6)
    p[flip] = rng.choice(classes, size=int(flip.sum()))
    return t.astype(np.int64), p.astype(np.int64)


def test_iou_and_f1_from_confusion_equal_the_reference_definitions():
    rng = np.random.default_rng(11)
    for trial in range(200):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        classes = [(0, 1, 2), (0, 1), (1, 2), (0, 2), (1,), (2,)][trial % 6]
        t, p = _random_maps(rng, h, w, classes)
        if trial % 7 == 3:
            p = rng.choice((0, 1, 2), size=(h, w))             # unrelated prediction: classes missing on one side only
        conf = metrics.confusion_numpy(p, t)
        assert conf.sum() == h * w
        np.testing.assert_allclose(metrics.iou(conf), lovasz_iou(p, t), rtol=0, atol=1e-12)
        np.testing.assert_allclose(metrics.f1(conf), sklearn021_f1(t.ravel(), p.ravel()), rtol=0, atol=1e-12)


def test_metric_edge_cases():
    # all bark predicted as all bark: empty unions give EMPTY = 1 (100 %); F1's absent classes take the mean of the others
    # in order, on the array as already updated: [0, 1, 0] -> [0.5, 1, 0] -> [0.5, 1, 0.75]
    conf = np.zeros((3, 3), np.int64)
    conf[1, 1] = 50
    np.testing.assert_array_equal(metrics.iou(conf), [100.0, 100.0, 100.0])
    np.testing.assert_allclose(metrics.f1(conf), [50.0, 100.0, 75.0], rtol=0, atol=1e-12)
    # a class present in the target but never predicted: precision 0 / 0 -> 0, F1 0; IoU 0
    conf = np.array([[10, 5, 0], [0, 20, 0], [0, 7, 0]])
    f = metrics.f1(conf)
    assert f[2] == 0.0 and metrics.iou(conf)[2] == 0.0
    # predicted but absent from the target: recall 0 / 0 -> 0
    conf = np.array([[10, 0, 3], [0, 20, 0], [0, 0, 0]])
    assert metrics.f1(conf)[2] == 0.0 and metrics.iou(conf)[2] == 0.0
    # a single-class map, perfectly predicted, for each class
    for c in range(3):
        conf = np.zeros((3, 3), np.int64)
        conf[c, c] = 7
        assert metrics.f1(conf)[c] == 100.0
        np.testing.assert_allclose(metrics.f1(conf), sklearn021_f1(np.full(7, c), np.full(7, c)), rtol=0, atol=1e-12)
        np.testing.assert_array_equal(metrics.iou(conf), [100.0, 100.0, 100.0])


def test_target_classes_is_the_datasets_decode_for_every_grey_level():
    grey = np.arange(256, dtype=np.uint8)
    want = (torch.arange(256, dtype=torch.float32) / 255 * 2).round().to(torch.uint8).numpy()
    np.testing.assert_array_equal(metrics.target_classes(grey), want)
    assert metrics.target_classes(np.array([63, 64, 191, 192], np.uint8)).tolist() == [0, 1, 1, 2]
    with pytest.raises(ValueError):
        metrics.target_classes(np.zeros(3, np.int64))


def test_confusion_numpy_counts_out_of_range_labels_nowhere():
    t = np.array([0, 1, 2, 2, 0], np.uint8)
    p = np.array([0, 1, 3, 255, 2], np.uint8)
    conf = metrics.confusion_numpy(p, t)
    assert conf.sum() == 3 and conf[0, 0] == 1 and conf[1, 1] == 1 and conf[0, 2] == 1


def test_csv_header_and_row_formatting(tmp_path):
    assert metrics.EVAL_CSV_HEADER == [
        'Name', 'Type', 'Split', 'iou_nothing', 'iou_bark', 'iou_node', 'iou_mean', 'f1_nothing', 'f1_bark', 'f1_node',
        'f1_mean', 'Output Bark %', 'Output Node %', 'Target Bark %', 'Target Node %']       # __main__.py:307-311
    raw = np.array([[30, 2, 0], [5, 50, 3], [0, 1, 9]], np.int64)
    clean = np.array([[31, 1, 0], [4, 52, 2], [0, 2, 8]], np.int64)
    row = metrics.eval_row("a.png", "sapin", raw, clean)
    ious, f1s = metrics.iou(raw), metrics.f1(clean)
    pixels = np.float32(raw.sum())
    pct = lambda c: "{:.5f}".format(float(np.float32(c) / pixels * np.float32(100)))
    assert row == ["a.png", "sapin", "all"] + ["{:.3f}".format(v) for v in ious] + ["{:.3f}".format(ious.mean())] + \
        ["{:.3f}".format(v) for v in f1s] + ["{:.3f}".format(f1s.mean())] + \
        [pct(raw[:, 1].sum()), pct(raw[:, 2].sum()), pct(raw[1].sum()), pct(raw[2].sum())]
    assert row[3] == "{:.3f}".format(100 * 30 / 37)
    path = str(tmp_path / "s.csv")
    ev.write_stats_csv(path, [row])
    back = list(csv.reader(open(path), delimiter="\t"))
    assert back == [metrics.EVAL_CSV_HEADER, row]
    s = metrics.summarize([row, row], raw * 2, clean * 2)
    assert s["pooled"]["iou_bark"] == pytest.approx(ious[1]) and s["column_means"]["f1_mean"] == float(row[10])


def test_dual_discovery_and_skip_rules(tmp_path):
    from PIL import Image
    root = str(tmp_path)

    def img(path, h, w, mode="RGB"):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.zeros((h, w, 3) if mode == "RGB" else (h, w), np.uint8), mode=mode).save(path)
    s, d = os.path.join(root, "samples"), os.path.join(root, "duals")
    img(os.path.join(s, "sapin", "a.bmp"), 12, 10)
    img(os.path.join(d, "sapin", "a.png"), 12, 10, "L")                     # a.bmp -> a.png
    img(os.path.join(s, "sapin", "bmp_scan.bmp"), 9, 9)
    img(os.path.join(d, "sapin", "png_scan.png"), 9, 9, "L")                # every "bmp" replaced, like dataset.py:58
    img(os.path.join(d, "sapin", "bmp_scan.png"), 9, 9, "L")                # (the literal-suffix name is not the dual)
    img(os.path.join(s, "sapin", "c.png"), 8, 8)                            # no dual
    img(os.path.join(s, "epinette_gelee", "m.png"), 16, 8)
    img(os.path.join(d, "epinette_gelee", "m.png"), 8, 16, "L")             # transposed: shape mismatch
    img(os.path.join(s, "epinette_gelee", "z.png"), 8, 1100)
    img(os.path.join(d, "epinette_gelee", "z.png"), 8, 1100, "L")           # wider than the 1024 target
    items = ev.list_labelled(root)
    assert [(d_["wood"], d_["name"]) for d_ in items] == [
        ("epinette_gelee", "m.png"), ("epinette_gelee", "z.png"),
        ("sapin", "a.png"), ("sapin", "png_scan.png"), ("sapin", "c.png")]
    assert items[3]["dual"] == os.path.join(d, "sapin", "png_scan.png")
    status = [ev.dual_status(it, *ev.image_hw(it["src"])) for it in items]
    assert status == [ev.STATUS_SHAPE_MISMATCH, ev.STATUS_TOO_LARGE, ev.STATUS_OK, ev.STATUS_OK, ev.STATUS_NO_DUAL]
    grey = ev.decode_dual(items[2]["dual"])
    assert grey.dtype == np.uint8 and grey.shape == (12, 10)


def test_report_builds_rows_and_skips_from_gathered_rows():
    items = [{"name": "a.png", "wood": "sapin"}, {"name": "b.png", "wood": "sapin"}]
    raw = np.array([[3, 1, 0], [0, 4, 0], [0, 0, 2]], np.int64)
    r0 = np.concatenate([[0, 2, 5, ev.STATUS_OK], raw.ravel(), raw.ravel()])
    r1 = np.concatenate([[1, 4, 4, ev.STATUS_NO_DUAL], np.zeros(18, np.int64)])
    rows, summary = ev.report(items, np.stack([r0, r1]), "fp32", "m.pt")
    assert rows == [metrics.eval_row("a.png", "sapin", raw, raw)]
    assert summary["images_evaluated"] == 1 and summary["images_skipped"] == 1
    assert summary["skipped"] == {"no_dual": ["sapin/b.png"], "shape_mismatch": [], "too_large": []}
    assert summary["precision"] == "fp32" and summary["model_path"] == "m.pt"


def _eval_row(i):
    return [i, 100 + i, 64, i % 4] + list(range(i, i + 18))


def _eval_gather_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from neuralbarkcalculator_amd import predict as drv
        px = [1, 1, 1, 1, 1, 9, 9]                                        # unequal shards: 5 + 2 images
        shards = drv.shard_by_pixels(px, world)
        rows = np.array([_eval_row(i) for i in shards[rank]], dtype=np.int64).reshape(-1, ev.ROW_WIDTH)
        allrows = drv.gather_rows(rows, len(px), world, dist, cap=max(len(s) for s in shards), width=ev.ROW_WIDTH)
        np.save(os.path.join(out_dir, f"erow{rank}.npy"), allrows)
    finally:
        dist.destroy_process_group()


def test_evaluation_row_gather_over_gloo(tmp_path):
    mp.spawn(_eval_gather_worker, args=(2, 29670, str(tmp_path)), nprocs=2, join=True)
    want = np.array([_eval_row(i) for i in range(7)], dtype=np.int64)
    for r in range(2):
        np.testing.assert_array_equal(np.load(os.path.join(str(tmp_path), f"erow{r}.npy")), want)


def test_exclude_nodes_is_refused():
    with pytest.raises(SystemExit) as e:
        ev.main(["/nonexistent", "--exclude_nodes"])
    assert "--exclude_nodes" in str(e.value)
