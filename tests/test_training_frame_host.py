"""The training run's frame (`evaluate --frame training`) on the host: training_frame.pad_resize_cpu against numpy.pad(reflect) +
PIL.Image.resize(BILINEAR) byte for byte, the coefficient table's own properties, and metrics.pooled_* against a direct
restatement of the reference's `iou` (lovasz_losses.py:54-77) and `PixelWiseF1` (utils.py:201-235) on concatenated label arrays."""
import numpy as np
import pytest
from PIL import Image

from neuralbarkcalculator_amd import metrics
from neuralbarkcalculator_amd import training_frame as tf

# (H, W) -> (Ht, Wt): no resample, rows only, columns only, both, p = L - 1 exactly (9 -> 24), the training's own size
SHAPES = [((21, 32), (32, 32)), ((22, 32), (32, 32)), ((32, 21), (32, 32)), ((21, 23), (32, 32)), ((27, 32), (32, 32)),
          ((32, 32), (32, 32)), ((17, 17), (32, 32)), ((13, 24), (24, 24)), ((9, 24), (24, 24)), ((521, 1024), (1024, 1024))]


def make_image(h, w, channels, seed=0):
    """RGB: every byte value; L: drawn from {0, 127, 255}, so that the blended greys cross the 63/64 and 191/192 thresholds."""
    rng = np.random.default_rng(1000 * h + w + 7 * channels + seed)
    if channels == 3:
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return rng.choice(np.array([0, 127, 255], dtype=np.uint8), size=(h, w))


def pil_pad_resize(img, ht, wt):
    """utils.py:242-247 as torchvision ran it: numpy.pad(mode="reflect") by ceil((Lt - L) / 2), then PIL's bilinear resize."""
    h, w = img.shape[:2]
    py, px = -((h - ht) // 2), -((w - wt) // 2)
    padded = np.pad(img, ((py, py), (px, px)) + (((0, 0),) if img.ndim == 3 else ()), mode="reflect")
    return np.array(Image.fromarray(padded).resize((wt, ht), Image.BILINEAR))


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_pad_resize_cpu_is_numpy_pad_then_pil_resize(src, dst, channels):
    img = make_image(*src, channels)
    want, got = pil_pad_resize(img, *dst), tf.pad_resize_cpu(img, *dst)
    assert got.dtype == np.uint8 and got.shape == want.shape == tuple(dst) + ((3,) if channels == 3 else ())
    np.testing.assert_array_equal(got, want)
    if channels == 1:
        np.testing.assert_array_equal(metrics.target_classes(got), metrics.target_classes(want))
        (_, hp), (_, wp) = tf.frame_geometry(src[0], dst[0]), tf.frame_geometry(src[1], dst[1])
        if (hp, wp) != dst:                          # a resampled dual does blend: greys that are none of the three drawn
            assert len(np.setdiff1d(np.unique(got), [0, 127, 255])) > 0


def test_frame_geometry_and_its_boundaries():
    assert tf.frame_geometry(32, 32) == (0, 32) and tf.frame_geometry(21, 32) == (6, 33) and tf.frame_geometry(22, 32) == (5, 32)
    assert tf.frame_geometry(521, 1024) == (252, 1025) and tf.frame_geometry(640, 1024) == (192, 1024)
    assert tf.frame_geometry(9, 24) == (8, 25)       # p = L - 1: the last pad one reflection reaches
    for L, Lt in ((8, 24), (11, 32), (1, 2), (33, 32), (0, 8), (8, 0)):
        with pytest.raises(ValueError):
            tf.frame_geometry(L, Lt)
    assert tf.frame_geometry(1, 1) == (0, 1)
    np.testing.assert_array_equal(tf.reflect_index(np.arange(-3, 8), 5), [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1])
    for L, Lt in ((21, 32), (9, 24), (13, 24)):      # the index map is numpy.pad's
        p, lp = tf.frame_geometry(L, Lt)
        np.testing.assert_array_equal(tf.reflect_index(np.arange(lp) - p, L), np.pad(np.arange(L), p, mode="reflect"))


@pytest.mark.parametrize("n", [8, 24, 32, 160, 1024])
def test_table_properties(n):
    first, coeff = tf.bilinear_taps(n + 1, n)
    assert first.dtype == coeff.dtype == np.int32 and first.shape == (n,) and coeff.shape == (n, tf.FRAME_TAPS)
    used = coeff != 0
    assert (coeff >= 0).all() and used[:, 0].all()
    # every row sums to 2^22 but for the rounding of its taps: each is off by at most a half
    assert (np.abs(coeff.sum(axis=1).astype(np.int64) - (1 << 22)) <= used.sum(axis=1) // 2 + 1).all()
    # a used tap lies inside the padded axis, and the rows walk it in order
    last = first + used.sum(axis=1) - 1
    assert first.min() == 0 and last.max() == n and (last <= n).all() and (np.diff(first) >= 0).all()
    # what the window of support 1 + 1/n means: output o blends padded indices o and o + 1, weighted towards the nearer end
    np.testing.assert_array_equal(first, np.arange(n))
    assert coeff[0, 0] > coeff[0, 1] and coeff[n - 1, 0] < coeff[n - 1, 1]


def test_table_refuses_other_sizes():
    for n_in, n_out in ((32, 32), (34, 32), (31, 32), (1, 0), (0, -1), (2048, 1024)):
        with pytest.raises(ValueError, match="in_size == out_size \\+ 1"):
            tf.bilinear_taps(n_in, n_out)
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            tf.pad_resize_cpu(bad, 8, 8)
    with pytest.raises(ValueError):
        tf.pad_resize_cpu(np.zeros((8, 24), np.uint8), 24, 24)   # p = L on the rows


# ---- the batch-pooled figures ----------------------------------------------------------------------------------------------
def reference_miou(pred, label):
    """`miou` of lovasz_losses.py:54-77 on the argmax labels of a batch (per_image is not an argument there: one pool)."""
    ious = []
    for i in range(3):
        inter, union = int(((label == i) & (pred == i)).sum()), int(((label == i) | (pred == i)).sum())
        ious.append(1.0 if not union else float(inter) / float(union))
    return float(np.mean(100 * np.array(ious)))


def reference_f1(pred, label):
    """`PixelWiseF1(None)` of utils.py:201-235 on final labels, f1_score(average=None) written out; times 100."""
    pred, label = pred.reshape(-1), label.reshape(-1)
    scores = np.zeros(3)
    for c in range(3):
        tp = float(((pred == c) & (label == c)).sum())
        p = tp / (pred == c).sum() if (pred == c).any() else 0.0
        r = tp / (label == c).sum() if (label == c).any() else 0.0
        scores[c] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    targets_count, outputs_count = np.bincount(label, minlength=3), np.bincount(pred, minlength=3)
    for i, count_i in enumerate(targets_count):
        if count_i == 0 and outputs_count[i] == 0:
            scores[i] = np.delete(scores, i).mean()
    return float(scores.mean() * 100)


def _labels(seed, classes):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(classes), size=(9, 11)), rng.choice(np.array(classes), size=(9, 11))


def test_pooled_figures_are_the_references_on_the_concatenated_group():
    # 3 images of 9 x 11, B = 2: the last group is short; class 2 is absent from the whole first group, target and output
    raw = [_labels(1, [0, 1]), _labels(2, [0, 1]), _labels(3, [0, 1, 2])]
    clean = [_labels(4, [0, 1]), _labels(5, [0, 1]), _labels(6, [0, 1, 2])]
    conf_raw = [metrics.confusion_numpy(p, t) for p, t in raw]
    conf_clean = [metrics.confusion_numpy(p, t) for p, t in clean]
    doc = metrics.pooled_over_groups(conf_raw, conf_clean, 2)
    assert doc["pool"] == 2 and [g["images"] for g in doc["groups"]] == [2, 1]
    want_miou, want_f1 = [], []
    for a, b in ((0, 2), (2, 3)):
        want_miou.append(reference_miou(np.stack([p for p, _ in raw[a:b]]), np.stack([t for _, t in raw[a:b]])))
        want_f1.append(reference_f1(np.stack([p for p, _ in clean[a:b]]), np.stack([t for _, t in clean[a:b]])))
    for g, m, f in zip(doc["groups"], want_miou, want_f1):
        assert g["miou"] == pytest.approx(m, abs=1e-12) and g["pixelwise_f1"] == pytest.approx(f, abs=1e-12)
    # the absent class: its IoU counts as 100, its F1 takes the mean of the other two
    assert metrics.iou(sum(conf_raw[:2]))[2] == 100.0
    f = metrics.f1(sum(conf_clean[:2]))
    assert f[2] == pytest.approx((f[0] + f[1]) / 2)
    # weighted by group size, as the trainer weights a step by its batch size
    assert doc["miou"] == pytest.approx((2 * want_miou[0] + want_miou[1]) / 3, abs=1e-12)
    assert doc["pixelwise_f1"] == pytest.approx((2 * want_f1[0] + want_f1[1]) / 3, abs=1e-12)
    assert metrics.pooled_miou(conf_raw[:2]) == doc["groups"][0]["miou"] and metrics.pooled_f1(conf_clean[2:]) == doc["groups"][1]["pixelwise_f1"]
    # B = 1: the per-image columns of the CSV, before their rounding
    one = metrics.pooled_over_groups(conf_raw, conf_clean, 1)
    assert [g["images"] for g in one["groups"]] == [1, 1, 1]
    for g, cr, cc in zip(one["groups"], conf_raw, conf_clean):
        assert g["miou"] == float(metrics.iou(cr).mean()) and g["pixelwise_f1"] == float(metrics.f1(cc).mean())
        row = metrics.eval_row("n", "w", cr, cc)
        assert row[6] == "{:.3f}".format(g["miou"]) and row[10] == "{:.3f}".format(g["pixelwise_f1"])
    # a pool beyond the folder is one group; no image, no figure
    assert len(metrics.pooled_over_groups(conf_raw, conf_clean, 64)["groups"]) == 1
    empty = metrics.pooled_over_groups([], [], 8)
    assert empty == {"pool": 8, "miou": None, "pixelwise_f1": None, "groups": []}
    with pytest.raises(ValueError):
        metrics.pooled_over_groups(conf_raw, conf_clean, 0)
    with pytest.raises(ValueError):
        metrics.pooled_over_groups(conf_raw, conf_clean[:2], 2)
