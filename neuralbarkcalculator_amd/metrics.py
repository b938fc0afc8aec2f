"""The evaluation metrics of the reference, from 3x3 confusion counts (host-side float64 arithmetic).

The reference's evaluation loop (/root/reference/src/bark_calculator/__main__.py:299-437) writes one tab-separated row
per labelled image (header at ``__main__.py:307-311``).  Its two metrics are ratios of pixel counts, so they are
computed here from ``conf[t][p]`` (pixels of target class t predicted as p; ``FCNResNet50.confusion`` counts them on the
device):

* IoU: lovasz ``iou`` (lovasz_losses.py:54-73) on the argmax of the logits (``__main__.py:331``).  ``IoU_c = tp / union``
  as Python floats, ``EMPTY = 1.0`` when the union is empty, times 100.  The ``remove_small_zones`` the loop applies to the
  float logits first (``__main__.py:324``) changes nothing but exact-0.0 logits, which it turns into 1.0; that quirk is
  not reproduced: the IoU here is that of the raw argmax.
* F1: ``PixelWiseF1('all')`` (utils.py:201-235), i.e. sklearn 0.21's ``f1_score(average=None)`` on the labels AFTER
  ``remove_small_zones`` (150 pixels): ``p = tp / (tp + fp)``, ``r = tp / (tp + fn)`` (0 on a zero denominator),
  ``f = 2 p r / (p + r)`` (0 when ``p + r == 0``), then the absent-class rule of utils.py:222-226 in class order on the
  array as already updated (a class absent from target and output takes the mean of the other two scores), times 100.
* The loss (``evaluate --loss``): ``LovaszSoftmax()`` (lovasz_losses.py:162-223) of each image as a batch of one, the
  objective of __main__.py:236-239.  ``FCNResNet50.lovasz_softmax`` computes one term per class on the device;
  ``lovasz_loss`` is the mean over the present classes (lovasz_losses.py:258-276).  Four trailing CSV columns
  (``LOSS_CSV_COLUMNS``), written with ``repr`` so that they carry every bit of the float64 values.
* The cross-entropy family (``evaluate --ce``): ``FCNResNet50.pixel_cross_entropy`` sums each image's pixel entropies per
  (target class, argmax class) cell on the device; from the nine float64 sums ``cross_entropy`` is ``F.cross_entropy`` (xloss,
  lovasz_losses.py:246-251), ``weighted_cross_entropy`` is ``CustomWeightedCrossEntropy`` (utils.py:151-165: each pixel's
  entropy times the class weight at ``max(argmax, target)``, mean over the pixels) for any weights, and ``mixed_loss`` is
  ``MixedLoss`` (utils.py:185-192).  Two or three trailing CSV columns, written with ``repr``.
* The percent columns: float32 ``count / (H W) * 100`` with ``'{:.5f}'`` (``__main__.py:392-398``), like
  ``predict.stats_row``; "Output" from the raw argmax, "Target" from the target.
* The figures of a training log (``evaluate --frame training --pool B [--as_logged]``): ``pooled_over_groups`` from per-image
  confusions; ``as_logged_over_groups`` from per-group rows, where the loss is ``lovasz_loss`` of the group's pooled terms
  (``FCNResNet50.lovasz_softmax_groups``) and the clean confusion comes from ``remove_small_zones`` on the group's ``[B,H,W]``
  array (``remove_small_zones_groups``).
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np

CLASS_NAMES = ["nothing", "bark", "node"]
EVAL_CSV_HEADER = ["Name", "Type", "Split", "iou_nothing", "iou_bark", "iou_node", "iou_mean", "f1_nothing", "f1_bark",
                   "f1_node", "f1_mean", "Output Bark %", "Output Node %", "Target Bark %", "Target Node %"]   # __main__.py:307-311
LOSS_CSV_COLUMNS = ["loss_nothing", "loss_bark", "loss_node", "lovasz_softmax"]   # evaluate --loss: after the 15 above
CE_CSV_COLUMNS = ["cross_entropy", "weighted_cross_entropy"]                      # evaluate --ce: after those
MIXED_CSV_COLUMN = "mixed_loss"                                                   # --ce and --loss together: the last one
REFERENCE_CLASS_WEIGHTS = (0.4004, 2.0334, 93.1921)   # get_pos_weight(), utils.py:72-73: compute_pos_weight of its dataset, frozen
SPLIT = "all"                     # the Split column: the tool has no train / valid / test split (__main__.py:375-377)


def target_classes(grey: np.ndarray) -> np.ndarray:
    """Class of each grey level of a dual, as dataset.py:189-197 decodes it after ToTensor: ``round(2 * float32(v) / 255)``
    -- 0 for 0..63, 1 for 64..191, 2 for 192..255 (no level lands on a half).  What the kernel of ``nbc_confusion`` does
    with ``(v + 64) >> 7``."""
    grey = np.asarray(grey)
    if grey.dtype != np.uint8:
        raise ValueError("grey must be uint8")
    return ((grey.astype(np.int32) + 64) >> 7).astype(np.uint8)


def confusion_numpy(labels: np.ndarray, target_class: np.ndarray) -> np.ndarray:
    """conf[t][p] of one image on the host: int64 [3,3] (labels outside {0,1,2} counted nowhere)."""
    p = np.asarray(labels).astype(np.int64).ravel()
    t = np.asarray(target_class).astype(np.int64).ravel()
    ok = (p >= 0) & (p < 3)
    return np.bincount(3 * t[ok] + p[ok], minlength=9).reshape(3, 3)


def iou(conf) -> np.ndarray:
    """lovasz ``iou`` (lovasz_losses.py:54-73) of one image from its raw-argmax confusion: float64 [3], in percent."""
    conf = np.asarray(conf, dtype=np.int64).reshape(3, 3)
    out = []
    for c in range(3):
        inter = int(conf[c, c])
        union = int(conf[c, :].sum() + conf[:, c].sum()) - inter
        out.append(1.0 if union == 0 else float(inter) / float(union))
    return 100 * np.array(out)


def f1(conf) -> np.ndarray:
    """``PixelWiseF1('all')`` (utils.py:201-235) of one image from its confusion after remove_small_zones: float64 [3], in
    percent (the ``* 100`` of __main__.py:332)."""
    conf = np.asarray(conf, dtype=np.int64).reshape(3, 3)
    tp = np.diag(conf).astype(np.float64)
    pred = conf.sum(axis=0).astype(np.float64)        # tp + fp
    true = conf.sum(axis=1).astype(np.float64)        # tp + fn
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(pred > 0, tp / np.where(pred > 0, pred, 1), 0.0)
        r = np.where(true > 0, tp / np.where(true > 0, true, 1), 0.0)
        den = p + r
        scores = np.where(den > 0, 2.0 * p * r / np.where(den > 0, den, 1), 0.0)
    for i in range(3):                                # utils.py:222-226, sequential on the updated array
        if true[i] == 0 and pred[i] == 0:
            scores[i] = np.delete(scores, i).mean()
    return scores * 100


def percent(count: int, pixels: int) -> str:
    """``'{:.5f}'.format((x == c).float().mean() * 100)`` in float32 (__main__.py:392-398)."""
    frac = np.float32(count) / np.float32(pixels)
    return "{:.5f}".format(float(frac * np.float32(100)))


def eval_row(name: str, wood: str, conf_raw, conf_clean) -> List[str]:
    """One row of the evaluation CSV (__main__.py:371-398) from the image's two confusions."""
    raw = np.asarray(conf_raw, dtype=np.int64).reshape(3, 3)
    ious, f1s = iou(raw), f1(conf_clean)
    pixels = int(raw.sum())
    row = [name, wood, SPLIT]
    row += ["{:.3f}".format(v) for v in ious] + ["{:.3f}".format(ious.mean())]
    row += ["{:.3f}".format(v) for v in f1s] + ["{:.3f}".format(f1s.mean())]
    pred, true = raw.sum(axis=0), raw.sum(axis=1)
    row += [percent(int(pred[c]), pixels) for c in (1, 2)] + [percent(int(true[c]), pixels) for c in (1, 2)]
    return row


def summarize(rows: Sequence[Sequence[str]], conf_raw_total, conf_clean_total) -> dict:
    """Pooled metrics (summed confusions over every evaluated image) and the mean of each numeric CSV column."""
    out = {"pooled": {}, "column_means": {}}
    ious, f1s = iou(conf_raw_total), f1(conf_clean_total)
    for c, name in enumerate(CLASS_NAMES):
        out["pooled"]["iou_" + name] = float(ious[c])
        out["pooled"]["f1_" + name] = float(f1s[c])
    out["pooled"]["iou_mean"], out["pooled"]["f1_mean"] = float(ious.mean()), float(f1s.mean())
    for j, col in enumerate(EVAL_CSV_HEADER[3:], start=3):
        out["column_means"][col] = float(np.mean([float(r[j]) for r in rows])) if rows else None
    return out


def lovasz_loss(terms, fg_counts) -> np.ndarray:
    """The Lovasz-Softmax loss of each image from its per-class terms (``FCNResNet50.lovasz_softmax``): the terms of the
    classes with ``fg_counts > 0``, added in class order and divided once by their number, as the reference's ``mean``
    (lovasz_losses.py:258-276) takes it over the present classes.  ``terms`` float [N,3] or [3], ``fg_counts`` int of the
    same shape; returns float64 [N] (or a float for one image).  An image with no present class (no pixel) gives 0, the
    reference's ``empty`` value; a NaN term gives NaN."""
    terms = np.asarray(terms, dtype=np.float64)
    counts = np.asarray(fg_counts)
    if terms.shape != counts.shape or terms.shape[-1] != 3:
        raise ValueError("terms and fg_counts must both be [N,3] or [3]")
    t2, c2 = terms.reshape(-1, 3), counts.reshape(-1, 3)
    out = np.zeros(len(t2), dtype=np.float64)
    for i, (t, c) in enumerate(zip(t2, c2)):
        present = [float(t[k]) for k in range(3) if c[k] > 0]
        if present:
            acc = 0.0
            for v in present:
                acc += v
            out[i] = acc / len(present)
    return float(out[0]) if terms.ndim == 1 else out


def loss_cells(terms, fg_counts) -> List[str]:
    """The four loss cells of one CSV row: each class's term (empty for an absent class), then the image's loss."""
    terms = np.asarray(terms, dtype=np.float64).reshape(3)
    counts = np.asarray(fg_counts).reshape(3)
    return [repr(float(terms[k])) if counts[k] > 0 else "" for k in range(3)] + [repr(lovasz_loss(terms, counts))]


def summarize_loss(rows: Sequence[Sequence[str]], first: int) -> dict:
    """``{"mean_over_images", "per_class_mean"}`` from the loss cells of the CSV rows (columns ``first`` .. ``first + 3``):
    the mean of the image losses, and per class the mean of its term over the images where the class is present (None
    when it is present nowhere)."""
    per_class = {}
    for k, name in enumerate(CLASS_NAMES):
        vals = [float(r[first + k]) for r in rows if r[first + k] != ""]
        per_class[name] = float(np.mean(vals)) if vals else None
    losses = [float(r[first + 3]) for r in rows]
    return {"mean_over_images": float(np.mean(losses)) if losses else None, "per_class_mean": per_class}


def _ce_sums(sums) -> np.ndarray:
    s = np.asarray(sums, dtype=np.float64)
    if s.size != 9:
        raise ValueError("sums must hold the 9 cells of one image")
    return s.reshape(3, 3)


def _fsum(values) -> float:
    """``math.fsum``, and what IEEE addition gives where it refuses (an infinity beside a NaN or the other infinity)."""
    values = [float(v) for v in values]
    if all(math.isfinite(v) for v in values):
        return math.fsum(values)
    return float(np.sum(np.array(values, dtype=np.float64)))


def cross_entropy(sums, pixels: int) -> float:
    """``F.cross_entropy(logits, target)`` of one image from its cell sums (``FCNResNet50.pixel_cross_entropy``): the nine
    sums added exactly, one division by the number of pixels."""
    return _fsum(_ce_sums(sums).ravel()) / float(pixels)


def weighted_cross_entropy(sums, pixels: int, weights) -> float:
    """``CustomWeightedCrossEntropy(weights)`` (utils.py:151-165) of one image as a batch of one: the cell of target class a
    and argmax class b carries the weight of class ``max(a, b)``.  ``0 * inf`` is NaN, as in torch."""
    s = _ce_sums(sums)
    w = [float(v) for v in weights]
    if len(w) != 3:
        raise ValueError("weights must hold one value per class")
    with np.errstate(invalid="ignore"):
        products = [float(np.float64(w[max(a, b)]) * s[a, b]) for a in range(3) for b in range(3)]
    return _fsum(products) / float(pixels)


def mixed_loss(weighted: float, lovasz: float) -> float:
    """``MixedLoss`` (utils.py:185-192): the weighted cross-entropy over four plus the Lovasz-Softmax loss."""
    return float(weighted) / 4 + float(lovasz)


def ce_cells(sums, pixels: int, weights, lovasz: float = None) -> List[str]:
    """The cross-entropy cells of one CSV row (``repr``: every bit); with ``lovasz`` (the image's Lovasz-Softmax loss) the
    mixed loss as well."""
    wce = weighted_cross_entropy(sums, pixels, weights)
    cells = [repr(cross_entropy(sums, pixels)), repr(wce)]
    if lovasz is not None:
        cells.append(repr(mixed_loss(wce, lovasz)))
    return cells


def summarize_ce(rows: Sequence[Sequence[str]], first: int, sums_total, pixels_total, weights, weights_source: str,
                 mixed: bool = False) -> dict:
    """The summary's ``"cross_entropy"`` entry: the means of the CSV cells (columns from ``first``), and the same formulas on
    the cell sums and pixel counts added over every evaluated image (``pooled``), with the totals themselves so that a
    reader can re-weight the folder.  ``mixed``: the rows carry the mixed loss as well (it has no pooled value:
    the Lovasz-Softmax loss does not pool)."""
    names = CE_CSV_COLUMNS + ([MIXED_CSV_COLUMN] if mixed else [])
    mean = {name: (float(np.mean([float(r[first + k]) for r in rows])) if rows else None) for k, name in enumerate(names)}
    total = _ce_sums(sums_total)
    pixels = np.asarray(pixels_total, dtype=np.int64).reshape(3, 3)
    p = int(pixels.sum())
    pooled = {}
    if p:
        pooled = {"cross_entropy": cross_entropy(total, p), "weighted_cross_entropy": weighted_cross_entropy(total, p, weights)}
    return {"class_weights": [float(v) for v in weights], "class_weights_source": weights_source, "mean_over_images": mean,
            "pooled": pooled, "sums": total.tolist(), "pixels": pixels.tolist()}


def pooled_miou(confs_raw) -> float:
    """``val_miou`` / ``test_miou`` of one batch (``iou(..., per_image=False)``, lovasz_losses.py:54-77): the mean over the three
    classes of ``100 iou`` of the batch's *summed* raw-argmax confusions, an empty union counting as 100."""
    total = np.asarray(confs_raw, dtype=np.int64).reshape(-1, 3, 3).sum(axis=0)
    return float(iou(total).mean())


def pooled_f1(confs_clean) -> float:
    """``PixelWiseF1`` of one batch (utils.py:201-235): ``f1`` -- its absent-class rule of utils.py:219-229 included -- of the
    batch's *summed* confusions after remove_small_zones, then the mean over the three classes."""
    total = np.asarray(confs_clean, dtype=np.int64).reshape(-1, 3, 3).sum(axis=0)
    return float(f1(total).mean())


def pooled_over_groups(confs_raw, confs_clean, pool: int) -> dict:
    """The batch-pooled figures of ``evaluate --frame training --pool B``: the images, in their order, form consecutive groups
    of ``pool`` (the last may be shorter), as the reference's ``valid_loader`` batches its ``test_dataset`` (__main__.py:209-228);
    each group gives ``pooled_miou`` and ``pooled_f1``, and the folder's figure is their mean weighted by group size, as the
    trainer weights a step by its batch size.  Returns ``{"pool", "miou", "pixelwise_f1", "groups"}``; the figures are None when
    there is no image."""
    pool = int(pool)
    if pool < 1:
        raise ValueError("pool must be >= 1")
    raw = np.asarray(confs_raw, dtype=np.int64).reshape(-1, 3, 3)
    clean = np.asarray(confs_clean, dtype=np.int64).reshape(-1, 3, 3)
    if len(raw) != len(clean):
        raise ValueError("one raw and one clean confusion per image")
    groups = []
    for a in range(0, len(raw), pool):
        groups.append({"images": int(len(raw[a:a + pool])), "miou": pooled_miou(raw[a:a + pool]),
                       "pixelwise_f1": pooled_f1(clean[a:a + pool])})
    n = len(raw)
    mean = lambda key: (_fsum(g[key] * g["images"] for g in groups) / n) if n else None
    return {"pool": pool, "miou": mean("miou"), "pixelwise_f1": mean("pixelwise_f1"), "groups": groups}


def as_logged_over_groups(confs_raw, confs_clean, terms, counts, sizes) -> dict:
    """The three figures a training run of the reference logs per epoch (loss, ``miou``, ``PixelWiseF1``; ``evaluate --frame
    training --pool B --as_logged``), from one row per group: the group's summed raw-argmax confusion, the confusion of its
    labels after ``remove_small_zones`` on the group's ``[B,H,W]`` array (``remove_small_zones_groups``), the three Lovasz terms
    and class counts of the group (``lovasz_softmax_groups``) and its number of images.  A group's loss is ``lovasz_loss`` of
    its terms and counts -- a class present in one image of the group is present for the group --, its ``miou`` is
    ``pooled_miou`` and its ``pixelwise_f1`` is ``pooled_f1``.  Each figure of the folder is the mean over the groups weighted
    by group size, as ``pooled_over_groups`` weights.  Returns ``{"loss", "miou", "pixelwise_f1", "groups"}``; the figures
    are None when there is no group."""
    raw = np.asarray(confs_raw, dtype=np.int64).reshape(-1, 3, 3)
    clean = np.asarray(confs_clean, dtype=np.int64).reshape(-1, 3, 3)
    terms = np.asarray(terms, dtype=np.float64).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    sizes = [int(v) for v in np.asarray(sizes).reshape(-1)]
    if not (len(raw) == len(clean) == len(terms) == len(counts) == len(sizes)):
        raise ValueError("one raw confusion, clean confusion, terms, counts and size per group")
    if any(v < 1 for v in sizes):
        raise ValueError("a group holds at least one image")
    groups = []
    for g in range(len(sizes)):
        groups.append({"images": sizes[g], "loss": float(lovasz_loss(terms[g], counts[g])),
                       "loss_terms": [float(v) for v in terms[g]], "present": [bool(v > 0) for v in counts[g]],
                       "miou": pooled_miou(raw[g]), "pixelwise_f1": pooled_f1(clean[g])})
    n = sum(sizes)
    mean = lambda key: (_fsum(g[key] * g["images"] for g in groups) / n) if n else None
    return {"loss": mean("loss"), "miou": mean("miou"), "pixelwise_f1": mean("pixelwise_f1"), "groups": groups}
