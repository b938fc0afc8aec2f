"""Evaluation of a checkpoint on a labelled folder: per-image IoU and F1, sharded over the GPUs of a node.

The counterpart of the reference's evaluation loop (/root/reference/src/bark_calculator/__main__.py:299-437) on the
accelerated path.  It answers what a choice of arithmetic mode or a retrained checkpoint costs in the metrics the model
was selected by.

* input: ``ROOT/samples/<wood_type>/<name>`` listed as ``predict.list_images`` lists them (dataset.py:41-68), each with its
  dual ``ROOT/duals/<wood_type>/<name.replace("bmp", "png")>`` (every ``bmp`` replaced, dataset.py:58), decoded with PIL
  ``convert('L')``;
* the network sees each sample as it is, through the uint8 ingest and, by default, the default mean / std of the predict
  driver (models.py:208-209); ``--mean R G B --std R G B`` or ``--stats PATH`` (``normalization=``) name another pair, as
  the reference's loop does with the ``compute_mean_std`` of its folder (__main__.py:204; ``python -m
  neuralbarkcalculator_amd.stats`` computes it), and the summary then says which.  The reference's evaluation never runs
  the preprocessor, its labelled folder is already at model resolution.  Nothing is written under ``processed/``;
* on the device, per batch of equal-sized frames: forward -> argmax labels -> ``confusion`` (raw) -> ``remove_small_zones``
  (150 pixels) -> ``confusion`` (clean).  Only the two int64 ``[N,3,3]`` results come back; ``metrics.py`` turns them into
  the row of ``__main__.py:371-398`` (IoU from the raw argmax, F1 after remove_small_zones, see there);
* output: ``ROOT/results/evaluation_stats.csv`` (tab separated, the header of ``__main__.py:307-311`` verbatim, ``Split`` =
  ``all``: there is no training split here) and ``ROOT/results/evaluation_summary.json`` (precision used, checkpoint,
  images evaluated and skipped with reasons and names, per-class IoU and F1 pooled over every pixel from the summed
  confusions, mean of each CSV column).  The summary is printed as well.

Deliberate departures from the reference:

* a sample with no dual is skipped (reason ``no_dual``); the reference scores it against an all-"Nothing" mask;
* a dual whose shape differs from its sample's is skipped (``shape_mismatch``) instead of crashing the run;
* a sample larger than the 1024 target on either side is skipped (``too_large``);
* ``--exclude_nodes`` is refused: the metrics are defined on three classes;
* no label PNGs and no matplotlib figures are written.

``--loss`` (``loss=True``) adds the training objective: each batch also writes its full-resolution logits, and
``FCNResNet50.lovasz_softmax`` turns them and the duals into per-class Lovasz-Softmax terms on the batch's stream
(``LovaszSoftmax()`` of lovasz_losses.py:162-223 per image, the loss of __main__.py:236-239; the batch-pooled loss of
``exp.test`` is not computed).  The ``[n,3]`` float64 terms ride back beside the confusions; each rank keeps them in rows
``(global_idx, 3 terms as int64 bit patterns)`` that a second ``all_gather`` brings to rank 0.  The CSV gains the four
columns of ``metrics.LOSS_CSV_COLUMNS`` and the summary a ``"lovasz_softmax"`` entry.  Without the flag nothing changes.

``--ce`` (``ce=True``) adds the loss the shipped checkpoint was trained on: each batch writes its full-resolution logits as
under ``--loss`` (one buffer per stream serves both flags), and ``FCNResNet50.pixel_cross_entropy`` sums the pixel entropies
per (target class, argmax class) cell on the batch's stream.  The ``[n,9]`` float64 sums ride back beside the confusions; each
rank keeps rows ``(global_idx, 9 sums as int64 bit patterns)`` that one more ``all_gather`` brings to rank 0 (the kernel's
counts are not gathered: they are the raw confusion of the rank rows).  ``metrics.py`` turns them into the plain
cross-entropy, ``CustomWeightedCrossEntropy`` (utils.py:151-165) for the class weights of ``--class_weights W0 W1 W2`` or
``--class_weights_from PATH`` (the ``pos_weight`` of a ``stats`` run; default ``metrics.REFERENCE_CLASS_WEIGHTS``, the
reference's ``get_pos_weight()``) and, with ``--loss`` too, ``MixedLoss`` (utils.py:185-192).  The CSV gains the columns of
``metrics.CE_CSV_COLUMNS`` (and ``mixed_loss``) after those of ``--loss``, the summary a ``"cross_entropy"`` entry that also
holds the cell sums and pixel counts of the whole folder, so that it can be re-weighted without another run.  The
reference's ``JaccardLoss`` is not computed as its code runs; ``--calibration`` reports the soft Jaccard
its name means.  Without the flag nothing changes.

``--zones`` (``zones=True``) asks what the pixel metrics hide: which zone of the final labels is which zone of the dual, and
how well they overlap.  After the second ``confusion``, on the labels ``PixelWiseF1`` sees, ``FCNResNet50.match_zones`` leaves
the zone rows of both maps (``predict --zones``' inventory; the dual's classes by ``metrics.target_classes``) and the
``(output zone, target zone, shared pixels)`` rows of every overlapping pair of the same class (csrc/zone_match.hip).  Up to
``--zones_cap`` (1024) zone rows per map and ``--zone_pairs_cap`` (2048) pair rows per image ride back per batch; an image
over a cap is matched by ``zones.match_cpu`` from the two planes, which ride back too, so the files do not depend on the
caps.  Three ragged gathers (``folder_run.gather_ragged``) bring the rows to rank 0, which writes
``results/zone_matches.csv`` (a row per target zone, ``matched`` or ``missed``, then a row per ``spurious`` output zone),
``results/zone_evaluation.csv`` (a row per image: ``zones.match_figures`` for Bark and Node) and a ``"zones"`` entry in the
summary (``zones.match_summary``).  Two zones match iff their IoU exceeds ``--match_iou`` (0.5 <= T < 1, default 0.5), so a
zone has at most one partner.  ``evaluation_stats.csv`` does not change, and without the flag nothing does.

``--contours`` (``contours=True``) asks how far the output's contours lie from the labelled ones, in millimetres: for a tool
whose product is an area, contour displacement is the error model.  After the second ``confusion``, on the same labels,
``FCNResNet50.contour_distances`` leaves per image and set (Bark and Node, output to target and back) the contour pixels, the
sum and maximum of the squared distances, their histogram by whole pixels and the float64 sum of the distances
(csrc/contours.hip; the host restatement is ``contours.contours_cpu``).  The rows ride back with the batch; each rank turns
them into one fixed-width row per image (``contours.wire_rows``: the heads, the sums, the counts within ``--contour_tolerance``
pixels -- default 2, 7.2 mm -- and the HD95 bins) and one pooled histogram, and only these travel.  Rank 0 writes
``results/contour_evaluation.csv`` (``contours.CONTOUR_COLUMNS``: per class the contour pixels of both maps, contour
precision, recall and F1 at the tolerance, the mean symmetric contour distance, HD95 -- whole pixels, rounded up -- and the
Hausdorff distance in mm) and a ``"contours"`` entry in the summary (``contours.contour_summary``) with the pooled histogram,
from which any other tolerance can be read off.  ``evaluation_stats.csv`` does not change, and without the flag nothing does.

``--operating_points`` (``operating_points=True``) sweeps the operating point: beside ``confusion``, on the batch's stream and on
the same full-resolution logits, ``FCNResNet50.offset_sweep`` counts the 3 x 3 confusion of ``argmax(x0, x1 + b1, x2 + b2)`` at
every point of a grid of (bark, node) offsets (csrc/offset_sweep.hip; the host restatement is ``operating.sweep_cpu``).  The
tables ride back in a pinned ring and rank 0 writes ``results/operating_points.csv``, ``results/operating_evaluation.csv`` and
the summary's ``"operating_points"`` entry (``operating.write_report``).  ``--logit_offsets BARK NODE`` (``logit_offsets=``)
applies one pair: every stream's model decides by that rule in the forward's own upsample + argmax launch, so both confusions
and every pass on the labels are of the offset labels; the passes on the logits (``--loss``, ``--ce``, ``--calibration``, the
sweep itself) do not change.

``--calibration`` (``calibration=True``) asks whether the network's confidence is worth anything.  Each batch writes its
full-resolution logits as under ``--loss`` / ``--ce`` (one buffer per stream serves all three flags), and after the raw
``confusion``, on the batch's stream, ``FCNResNet50.softmax_census`` tallies the softmax against the dual
(csrc/softmax_census.hip; the host restatement is ``calibration.census_cpu``): the census describes the *raw* softmax, before
``remove_small_zones`` -- with ``--tta`` the softmax of the merged logits.  The rows ride back with the batch; each rank turns
them into one fixed-width row per image (``calibration.wire_rows``: the reliability counts and confidence sums at
``--ece_bins`` bins -- default 16 --, the soft confusion, the Brier numerators) and one pooled census, and only these travel:
integer sums are exact in any order.  Rank 0 writes ``results/calibration_evaluation.csv``
(``calibration.CALIBRATION_COLUMNS``: ECE and MCE with the mean confidence of each bin from its exact sum, accuracy, mean
confidence, the Brier score, the soft Jaccard per class and the ``JaccardLoss`` value with the sums its name means, expected
beside hard Bark / Node %, the non-finite pixels), ``results/calibration_curves.csv`` from the pooled folder (per class and
threshold j / 256 the one-vs-rest precision, recall and F1 of "p_c >= threshold", and the reliability table of the 256 bins)
and a ``"calibration"`` entry in the summary (``calibration.calibration_summary``: the pooled figures, per class AP, AUROC,
the best-F1 threshold and the F1 there beside the F1 at argmax, and the pooled ``H``, ``R`` and ``RS``, from which any other
bin count can be read off).  ``evaluation_stats.csv`` does not change, and without the flag nothing does.

``--jitter training`` / ``--jitter_views "b,c,s;..."`` scores the mean of the colour-jitter views the training augmented over
 in every metric and option above, as ``--tta`` scores the mean of the flip views, and asks how far one view
moves the answer: each view's own final labels (after ``remove_small_zones``) go through ``confusion`` against the dual on the
batch's stream, their nine counts ride back with the batch, and rank 0 writes ``results/jitter_evaluation.csv``
(``jitter_evaluation``: a row per view pooled over the folder -- IoU and F1 per class with their means, Bark % and Node %, and
each figure's difference from the ``identity`` view's) and a ``"jitter"`` entry in the summary.  ``evaluation_stats.csv``
keeps its columns.

``--windows S`` (with ``--windows_stride``, ``--windows_blend``) scores sliding-window inference at the training's crop size
 in every metric and option above: ``predict_labels_windows`` stands where ``predict_labels`` does and the
summary notes ``"windows": {window, stride, blend}``.  ``--windows_compare`` also runs the plain forward of each frame; the
confusion of its final labels rides back with the batch and rank 0 writes ``results/windows_evaluation.csv``
(``jitter_evaluation`` on the rows ``identity`` -- the frame -- and ``windows``, pooled over the folder).

``--frame training`` (with ``--frame_size T``, ``--pool B``) scores the checkpoint on the frames it was selected on
(DESIGN.md 3.19): ``val_miou`` -- what ``ReduceLROnPlateau``, ``EarlyStopping`` and the choice of checkpoint read -- and the
``test_*`` figures of ``exp.test`` come from ``test_dataset`` (__main__.py:209-228), where every sample and its dual go through
``pad_resize(img, 1024, 1024)`` (utils.py:242-247).  At the top of each batch the scans and their duals are replaced by that
frame (``FCNResNet50.training_frame``, csrc/training_frame.hip); everything above then runs on the frame, in the training's own
order frame -> jitter / flips / windows (__main__.py:158-165).  A scan whose pad one reflection does not reach is skipped
(``too_small``).  The summary gains ``"frame"``: the images resampled per axis and the batch-pooled ``miou`` and
``pixelwise_f1`` over consecutive groups of B evaluated images in list order (``metrics.pooled_over_groups``; default 8, the
reference's validation batch), the figures a training log holds.  ``--subset PATH`` (one ``wood_type/name`` per line) evaluates
only the named samples, in the file's order: the pooled figures mean ``val_miou`` only on the split they were logged for.
Without the flags nothing changes.

``--as_logged`` (with ``--frame training``) adds the other two figures of a training log as the log computed
them: ``LovaszSoftmax()`` on a batch sorts the errors of all its images together (lovasz_losses.py:169-191), and ``PixelWiseF1``
runs ``remove_small_zones`` on the ``[B,H,W]`` argmax, where connectivity=2 links zones of neighbouring images through the batch
axis (utils.py:211-214).  Both need a whole group on one device: the shards are cut at group boundaries, each rank keeps the
low-resolution logits and the framed dual of every evaluated image on its device and, after the loop, runs
``FCNResNet50.lovasz_softmax_groups`` and ``remove_small_zones_groups`` group by group; ``summary["frame"]["as_logged"]`` holds
``loss``, ``miou``, ``pixelwise_f1`` and the groups (``metrics.as_logged_over_groups``).  Every other file and key is what the
run writes without the flag.

The machinery is ``folder_run``'s, shared with the predict driver: equal-shape batches, ``streams`` batches in flight on their own HIP streams and
model objects sharing one copy of the weights, contiguous pixel-balanced shards, ``--gpus N`` starting the ranks, the
f16x2 calibration guard on the first image and the non-finite word riding back with every batch, and ``--precision auto``
running f16x2 and the folder again in fp32 when that mode cannot carry the weights.  Each rank fills fixed-width int64
rows ``(global_idx, H, W, status, 9 raw counts, 9 counts after remove_small_zones)`` that one ``all_gather`` brings to
rank 0.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
from typing import List, Sequence, Tuple

import numpy as np

from . import folder_run, metrics
from .folder_run import NonFiniteLogits, launch_ranks      # noqa: F401 (NonFiniteLogits: what evaluate_folder raises)
from .predict import _decode_rgb, list_images

ROW_WIDTH = 22                                   # (global_idx, H, W, status, conf_raw[9], conf_clean[9])
LOSS_ROW_WIDTH = 4                               # --loss: (global_idx, 3 float64 terms viewed as int64)
CE_ROW_WIDTH = 10                                # --ce: (global_idx, 9 float64 cell sums viewed as int64)
STATUS_OK, STATUS_NO_DUAL, STATUS_SHAPE_MISMATCH, STATUS_TOO_LARGE = 0, 1, 2, 3
SKIP_REASONS = {STATUS_NO_DUAL: "no_dual", STATUS_SHAPE_MISMATCH: "shape_mismatch", STATUS_TOO_LARGE: "too_large"}
STATUS_TOO_SMALL = 4                             # --frame training: a pad that one reflection of the scan does not reach
TOO_SMALL = "too_small"                          # its reason: a key of summary["skipped"] only with the flag
FRAMES = ("scan", "training")                    # --frame
DEFAULT_POOL, MAX_POOL = 8, 64                   # --pool: the reference's valid_loader batches its test_dataset by 8
GROUP_ROW_WIDTH = 17                             # --as_logged: (first global_idx, images, conf_clean[9], 3 f64 terms as int64, counts[3])
AS_LOGGED_MAX_BYTES = 32 << 30                   # --as_logged: what a rank may hold on its device for it
STATS_CSV = os.path.join("results", "evaluation_stats.csv")
SUMMARY_JSON = os.path.join("results", "evaluation_summary.json")
MATCHES_CSV, ZONE_EVALUATION_CSV = "zone_matches.csv", "zone_evaluation.csv"     # --zones, under results/
CONTOUR_CSV = "contour_evaluation.csv"                                           # --contours, under results/
CALIBRATION_CSV, CURVES_CSV = "calibration_evaluation.csv", "calibration_curves.csv"   # --calibration, under results/


def list_labelled(root: str) -> List[dict]:
    """Every sample with the path its dual would have (dataset.py:41-68): ``{"src", "name", "wood", "dual"}``."""
    return [{"src": path, "name": name, "wood": wood, "dual": os.path.join(root, "duals", wood, name)}
            for path, name, wood in list_images(root)]


def image_hw(path: str) -> Tuple[int, int]:
    from PIL import Image
    with open(path, "rb") as f:
        w, h = Image.open(f).size                # header only: nothing is decoded
    return h, w


def dual_status(item: dict, h: int, w: int, target_size: int = 1024) -> int:
    """Whether a sample of ``h`` x ``w`` pixels can be evaluated: STATUS_OK or the reason it is skipped."""
    if not os.path.isfile(item["dual"]):
        return STATUS_NO_DUAL
    if image_hw(item["dual"]) != (h, w):
        return STATUS_SHAPE_MISMATCH
    if max(h, w) > target_size:
        return STATUS_TOO_LARGE
    return STATUS_OK


def decode_dual(path: str) -> np.ndarray:
    """The dual as PIL ``convert('L')`` gives it: uint8 [H,W] grey levels (classes: ``metrics.target_classes``)."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("L"))


def csv_header(loss: bool = False, ce: bool = False) -> List[str]:
    return metrics.EVAL_CSV_HEADER + (metrics.LOSS_CSV_COLUMNS if loss else []) + (metrics.CE_CSV_COLUMNS if ce else []) + \
        ([metrics.MIXED_CSV_COLUMN] if ce and loss else [])


def write_stats_csv(path: str, rows, loss: bool = False, ce: bool = False) -> None:
    with open(path, "w") as f:                   # __main__.py:433-437
        csv.writer(f, delimiter="\t").writerows([csv_header(loss, ce)] + [list(r) for r in rows])


def class_weights_from(path: str) -> Tuple[float, float, float]:
    """The ``pos_weight`` of a ``results/dataset_stats.json`` (``python -m neuralbarkcalculator_amd.stats``) as class weights;
    ValueError when the file has none, or a null in it (a class without a pixel has no weight)."""
    with open(path) as f:
        doc = json.load(f)
    w = doc.get("pos_weight") if isinstance(doc, dict) else None
    if not isinstance(w, list) or len(w) != 3:
        raise ValueError("%s holds no pos_weight of three classes" % path)
    if any(v is None for v in w):
        raise ValueError("%s: pos_weight has a null: a class without a pixel has no weight" % path)
    return check_class_weights(w)


def check_class_weights(weights) -> Tuple[float, float, float]:
    """Three finite weights >= 0 as floats; ValueError otherwise."""
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError("class weights must be three numbers")
    if len(w) != 3 or not all(np.isfinite(v) and v >= 0 for v in w):
        raise ValueError("class weights must be three finite numbers >= 0, got %r" % (list(weights),))
    return w


def check_zone_match_arguments(zones: bool, zones_cap=None, zone_pairs_cap=None, match_iou=None) -> None:
    """``ValueError`` for what ``--zones`` and its options refuse before any device is touched: an option without the flag, a
    cap out of range (``folder_run.ZONES_MAX_CAP``, ``zones.PAIRS_MAX_CAP``), a threshold outside [0.5, 1)."""
    from . import zones as zn
    folder_run.check_zones_arguments(zones, zones_cap)
    if not zones:
        if zone_pairs_cap is not None:
            raise ValueError("--zone_pairs_cap needs --zones")
        if match_iou is not None:
            raise ValueError("--match_iou needs --zones")
        return
    if zone_pairs_cap is not None and not 1 <= int(zone_pairs_cap) <= zn.PAIRS_MAX_CAP:
        raise ValueError("--zone_pairs_cap must lie in 1..%d" % zn.PAIRS_MAX_CAP)
    if match_iou is not None:
        zn.check_match_iou(match_iou)


def _rows_of_image(allz: np.ndarray, indices) -> list:
    """The rows of each global index of ``indices`` in gathered ``(global_idx, fields...)`` rows, without the index column."""
    starts, ends = np.searchsorted(allz[:, 0], indices, side="left"), np.searchsorted(allz[:, 0], indices, side="right")
    return [allz[a:b, 1:] for a, b in zip(starts, ends)]


def write_zone_match_report(results_dir: str, items, allrows, all_out, all_tgt, all_pairs, match_iou: float, cap: int,
                            pair_cap: int, host_fallbacks: int) -> dict:
    """``zone_matches.csv`` and ``zone_evaluation.csv`` (tab separated, like ``evaluation_stats.csv``) from the gathered rows,
    for the evaluated images of ``allrows`` in their order: ``all_out`` / ``all_tgt`` the ``(global_idx, 10 zone fields)`` rows
    of the output's and the target's zones, ``all_pairs`` the ``(global_idx, 3 pair fields)`` rows.  Returns the ``"zones"``
    entry of the summary (``zones.match_summary``)."""
    from . import zones as zn
    all_out = np.asarray(all_out, dtype=np.int64).reshape(-1, 1 + zn.ZONE_ROW)
    all_tgt = np.asarray(all_tgt, dtype=np.int64).reshape(-1, 1 + zn.ZONE_ROW)
    all_pairs = np.asarray(all_pairs, dtype=np.int64).reshape(-1, 1 + zn.PAIR_ROW)
    done = [int(g[0]) for g in allrows if int(g[3]) == STATUS_OK]
    matches, evaluation, figures = [list(zn.MATCH_COLUMNS)], [list(zn.EVALUATION_COLUMNS)], []
    for gi, o, t, p in zip(done, _rows_of_image(all_out, done), _rows_of_image(all_tgt, done), _rows_of_image(all_pairs, done)):
        d = items[gi]
        matches += zn.match_rows(d["name"], d["wood"], o, t, p, match_iou)
        figures.append(zn.match_figures(o, t, p, match_iou))
        evaluation += zn.evaluation_rows(d["name"], d["wood"], figures[-1])
    for name, rows_ in ((MATCHES_CSV, matches), (ZONE_EVALUATION_CSV, evaluation)):
        with open(os.path.join(results_dir, name), "w") as f:
            csv.writer(f, delimiter="\t").writerows(rows_)
    return zn.match_summary(figures, match_iou, cap, pair_cap, host_fallbacks)


def check_contour_arguments(contours: bool, contour_tolerance=None) -> None:
    """``ValueError`` for what ``--contours`` and its option refuse before any device is touched: the option without the flag,
    a tolerance that is no integer >= 0."""
    from . import contours as ct
    if not contours:
        if contour_tolerance is not None:
            raise ValueError("--contour_tolerance needs --contours")
        return
    if contour_tolerance is not None:
        ct.check_tolerance(contour_tolerance)


def write_contour_report(results_dir: str, items, allrows, all_wire, histogram, tolerance: int) -> dict:
    """``contour_evaluation.csv`` (tab separated, like ``evaluation_stats.csv``) from the gathered ``(global_idx,
    contours.WIRE_WIDTH fields)`` rows ``all_wire``, for the evaluated images of ``allrows`` in their order.  Returns the
    ``"contours"`` entry of the summary (``contours.contour_summary`` of the figures and the folder's pooled ``histogram``)."""
    from . import contours as ct
    wire = {int(g[0]): g[1:] for g in np.asarray(all_wire, dtype=np.int64).reshape(-1, 1 + ct.WIRE_WIDTH)}
    table, figures = [list(ct.CONTOUR_COLUMNS)], []
    for g in allrows:
        if int(g[3]) != STATUS_OK:
            continue
        d = items[int(g[0])]
        figures.append(ct.figures_of_wire(wire[int(g[0])]))
        table += ct.contour_rows(d["name"], d["wood"], figures[-1])
    with open(os.path.join(results_dir, CONTOUR_CSV), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    return ct.contour_summary(figures, tolerance, histogram)


def check_calibration_arguments(calibration: bool, ece_bins=None) -> None:
    """``ValueError`` for what ``--calibration`` and its option refuse before any device is touched: the option without the
    flag, a bin count that is no power of two in 1..256."""
    from . import calibration as cal
    if not calibration:
        if ece_bins is not None:
            raise ValueError("--ece_bins needs --calibration")
        return
    if ece_bins is not None:
        cal.check_ece_bins(ece_bins)


def check_frame_arguments(frame="scan", frame_size=None, pool=None, target_size: int = 1024, as_logged: bool = False):
    """``ValueError`` for what ``--frame`` and its options refuse before any device is touched: an unknown frame,
    ``--frame_size``, ``--pool`` or ``--as_logged`` without ``--frame training``, a frame size outside ``8 .. target_size``, a
    pool outside ``1 .. MAX_POOL``.  Returns ``(T, B)``: the side of the training frame and the images per pooled group, or
    ``(None, None)`` for ``frame="scan"``, today's behaviour."""
    if frame is None:
        frame = "scan"
    if frame not in FRAMES:
        raise ValueError("--frame must be one of %s, got %r" % (", ".join(FRAMES), frame))
    if frame == "scan":
        given = [n for n, v in (("--frame_size", frame_size), ("--pool", pool), ("--as_logged", as_logged or None)) if v is not None]
        if given:
            raise ValueError("%s needs --frame training" % ", ".join(given))
        return None, None
    size = target_size if frame_size is None else frame_size
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 8 <= int(size) <= int(target_size):
        raise ValueError("--frame_size must be an integer in 8..%d, got %r" % (target_size, size))
    b = DEFAULT_POOL if pool is None else pool
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= int(b) <= MAX_POOL:
        raise ValueError("--pool must be an integer in 1..%d, got %r" % (MAX_POOL, b))
    return int(size), int(b)


def frame_status(h: int, w: int, size: int) -> int:
    """What ``--frame training`` says of a scan of ``h x w`` pixels that could otherwise be evaluated: STATUS_TOO_LARGE where a
    side exceeds the frame's, STATUS_TOO_SMALL where nbc_training_frame would refuse an axis (its pad needs more than one
    reflection), else STATUS_OK."""
    from .training_frame import frame_geometry
    if max(h, w) > size:
        return STATUS_TOO_LARGE
    try:
        frame_geometry(h, size), frame_geometry(w, size)
    except ValueError:
        return STATUS_TOO_SMALL
    return STATUS_OK


def pooled_groups(ok: Sequence[bool], pool: int) -> Tuple[List[List[int]], List[int]]:
    """The groups ``--pool`` forms, known before the loop: ``ok[i]`` says whether image i of the list passes the header checks.
    Returns the groups (consecutive runs of ``pool`` such images, by list index) and, for ``folder_run.shard_by_units``, the
    unit of every image of the list: its group's number, an image that is skipped going with the next group (the last one
    when none follows)."""
    good = [i for i, v in enumerate(ok) if v]
    groups = [good[a:a + pool] for a in range(0, len(good), pool)]
    unit, g = [], 0
    for i in range(len(ok)):
        while g + 1 < len(groups) and i > groups[g][-1]:
            g += 1
        unit.append(g)
    return groups, unit


def as_logged_bytes(images: int, size: int, pool: int) -> int:
    """The device memory ``--as_logged`` holds on a rank whose shard has ``images`` evaluated frames of side ``size``: per image
    the low-resolution logits (three f32 planes at the output stride of 8, an upper bound for the other networks) and the
    framed dual, and for the pass over one group of ``pool`` frames after the loop its full logits (12 bytes per pixel), labels
    (1), the two key arrays of ``lovasz_softmax_groups`` (24) and the workspace of ``remove_small_zones_groups`` (9)."""
    low = (size + 7) // 8
    return images * (12 * low * low + size * size) + min(pool, max(images, 1)) * size * size * (12 + 1 + 24 + 9)


def as_logged_report(allrows, group_rows, pool: int) -> dict:
    """The ``"as_logged"`` entry of the summary's ``"frame"`` from the gathered image rows and the gathered ``GROUP_ROW_WIDTH``
    rows of the groups (in the order of their first image): ``metrics.as_logged_over_groups``, the raw confusion of a group
    being the sum of its images' rows."""
    done = [g for g in allrows if int(g[3]) == STATUS_OK]
    group_rows = np.asarray(group_rows, dtype=np.int64).reshape(-1, GROUP_ROW_WIDTH)
    raw = [np.sum([np.asarray(g[4:13], dtype=np.int64) for g in done[a:a + pool]], axis=0) for a in range(0, len(done), pool)]
    if len(raw) != len(group_rows) or any(int(done[k * pool][0]) != int(g[0]) or len(done[k * pool:(k + 1) * pool]) != int(g[1])
                                           for k, g in enumerate(group_rows)):
        raise RuntimeError("--as_logged: the groups that ran are not the groups of the evaluated images")
    return metrics.as_logged_over_groups(raw, group_rows[:, 2:11], np.ascontiguousarray(group_rows[:, 11:14]).view(np.float64),
                                         group_rows[:, 14:17], group_rows[:, 1])


def read_subset(path: str) -> List[str]:
    """The lines of a ``--subset`` file: one ``wood_type/name`` per line, blank lines dropped."""
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def apply_subset(items: List[dict], lines) -> List[dict]:
    """The listed samples that ``lines`` (``wood_type/name`` each) name, in the order of the lines: the file's order becomes the
    list order, and so the grouping of ``--pool``.  ``ValueError`` quoting the first line that names no listed sample, or one
    named twice."""
    by_key = {d["wood"] + "/" + d["name"]: d for d in items}
    out, seen = [], set()
    for line in lines:
        if line not in by_key:
            raise ValueError("--subset: %r names no listed sample" % line)
        if line in seen:
            raise ValueError("--subset: %r is named twice" % line)
        seen.add(line)
        out.append(by_key[line])
    return out


def frame_report(allrows, size: int, pool: int) -> dict:
    """The ``"frame"`` entry of the summary from the gathered rows: the evaluated images whose padded height (width) came out
    at ``size + 1``, so that the axis was resampled, and the batch-pooled figures of ``metrics.pooled_over_groups`` over the
    evaluated images in list order."""
    from .training_frame import frame_geometry
    done = [g for g in allrows if int(g[3]) == STATUS_OK]
    doc = {"kind": "training", "size": int(size),
           "resampled_rows": sum(1 for g in done if frame_geometry(int(g[1]), size)[1] != size),
           "resampled_cols": sum(1 for g in done if frame_geometry(int(g[2]), size)[1] != size)}
    doc.update(metrics.pooled_over_groups([g[4:13] for g in done], [g[13:22] for g in done], pool))
    return doc


def write_operating_report(results_dir: str, items, allrows, all_op, grids, logit_offsets=None) -> dict:
    """``operating_points.csv`` and ``operating_evaluation.csv`` from the gathered ``(global_idx, G1 G2 9 counts)`` rows
    ``all_op``, for the evaluated images of ``allrows`` in their order.  Returns the ``"operating_points"`` entry of the summary
    (``operating.write_report``)."""
    from . import operating as opm
    b1, b2 = grids
    shape = (b1.size, b2.size, 3, 3)
    tables = {int(g[0]): g[1:] for g in np.asarray(all_op, dtype=np.int64).reshape(-1, 1 + b1.size * b2.size * 9)}
    images = [(items[int(g[0])]["name"], items[int(g[0])]["wood"], tables[int(g[0])].reshape(shape))
              for g in allrows if int(g[3]) == STATUS_OK]
    return opm.write_report(results_dir, images, b1, b2, logit_offsets)


def write_calibration_report(results_dir: str, items, allrows, all_wire, pooled, ece_bins: int) -> dict:
    """``calibration_evaluation.csv`` and ``calibration_curves.csv`` (tab separated, like ``evaluation_stats.csv``) from the
    gathered ``(global_idx, calibration.wire_width(ece_bins) fields)`` rows ``all_wire`` and the folder's pooled census row, for
    the evaluated images of ``allrows`` in their order.  Returns the ``"calibration"`` entry of the summary
    (``calibration.calibration_summary``)."""
    from . import calibration as cal
    width = cal.wire_width(ece_bins)
    wire = {int(g[0]): g[1:] for g in np.asarray(all_wire, dtype=np.int64).reshape(-1, 1 + width)}
    table, raw_total, images = [list(cal.CALIBRATION_COLUMNS)], np.zeros((3, 3), np.int64), 0
    for g in allrows:
        if int(g[3]) != STATUS_OK:
            continue
        d, raw = items[int(g[0])], np.asarray(g[4:13], dtype=np.int64).reshape(3, 3)
        raw_total += raw
        images += 1
        table += cal.calibration_rows(d["name"], d["wood"], cal.figures_of_wire(wire[int(g[0])], ece_bins), raw.sum(axis=0))
    for name, rows_ in ((CALIBRATION_CSV, table), (CURVES_CSV, [list(cal.CURVE_COLUMNS)] + cal.curve_rows(pooled))):
        with open(os.path.join(results_dir, name), "w") as f:
            csv.writer(f, delimiter="\t").writerows(rows_)
    return cal.calibration_summary(pooled, images, ece_bins, raw_total)


JITTER_EVALUATION_CSV = "jitter_evaluation.csv"                                  # --jitter, under results/
JITTER_FIGURES = ["iou_nothing", "iou_bark", "iou_node", "iou_mean", "f1_nothing", "f1_bark", "f1_node", "f1_mean", "Bark %", "Node %"]


def jitter_evaluation(names, confusions) -> Tuple[List[List[str]], dict]:
    """The robustness table of ``--jitter``: one row per view from the confusion ``conf[t][p]`` of its final labels (after
    ``remove_small_zones``) against the duals, pooled over the folder.  Per view: ``metrics.iou`` and ``metrics.f1`` of the
    pooled counts with their means, and the share of the pixels labelled bark and node, ``100 count / pixels`` in float64; where
    the set has an ``identity`` view, each figure's difference from that view's (the view's minus the identity's, of the
    unrounded figures).  IoU and F1 are printed '{:.3f}' as ``evaluation_stats.csv`` prints them, the shares '{:.5f}'.  Returns
    the CSV rows (header first) and ``{name: {"figures": {...}, "difference": {...} or None}}`` in the order of the stack."""
    names = list(names)
    figures = []
    for conf in confusions:
        conf = np.asarray(conf, dtype=np.int64).reshape(3, 3)
        ious, f1s = metrics.iou(conf), metrics.f1(conf)
        pixels, pred = int(conf.sum()), conf.sum(axis=0)
        shares = [(100 * int(pred[c])) / pixels if pixels else 0.0 for c in (1, 2)]
        figures.append([float(v) for v in ious] + [float(ious.mean())] + [float(v) for v in f1s] + [float(f1s.mean())] + shares)
    identity = names.index("identity") if "identity" in names else None
    spec = ["{:.3f}"] * 8 + ["{:.5f}"] * 2
    rows = [["View"] + JITTER_FIGURES + (["d " + k for k in JITTER_FIGURES] if identity is not None else [])]
    doc = {}
    for name, f in zip(names, figures):
        diff = [a - b for a, b in zip(f, figures[identity])] if identity is not None else None
        rows.append([name] + [s.format(v) for s, v in zip(spec, f)] + ([s.format(v) for s, v in zip(spec, diff)] if diff is not None else []))
        doc[name] = {"figures": dict(zip(JITTER_FIGURES, f)), "difference": dict(zip(JITTER_FIGURES, diff)) if diff is not None else None}
    return rows, doc


def write_jitter_evaluation(results_dir: str, allrows, all_views, factors) -> dict:
    """``jitter_evaluation.csv`` (tab separated, like ``evaluation_stats.csv``) from the gathered ``(global_idx, V x 9 confusion
    cells)`` rows ``all_views``, summed over the evaluated images of ``allrows``.  Returns the ``"jitter"`` entry of the summary."""
    names = folder_run.jitter_view_names(factors)
    done = {int(g[0]) for g in allrows if int(g[3]) == STATUS_OK}
    total = np.zeros((len(names), 3, 3), dtype=np.int64)
    for g in np.asarray(all_views, dtype=np.int64).reshape(-1, 1 + 9 * len(names)):
        if int(g[0]) in done:
            total += g[1:].reshape(len(names), 3, 3)
    table, doc = jitter_evaluation(names, total)
    with open(os.path.join(results_dir, JITTER_EVALUATION_CSV), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    return {"views": names, "factors": [[float(v) for v in t] for t in factors], "evaluation": doc}


WINDOWS_EVALUATION_CSV = "windows_evaluation.csv"                                # --windows_compare, under results/
WINDOWS_EVALUATION_ROWS = ["identity", "windows"]                                # the plain forward of the frame, the blend of its windows


def write_windows_evaluation(results_dir: str, allrows, all_win) -> dict:
    """``windows_evaluation.csv`` (tab separated, like ``jitter_evaluation.csv``) from the gathered ``(global_idx, the plain
    forward's 9 confusion cells, the windows' 9)`` rows ``all_win`` (final labels, after ``remove_small_zones``), summed over the
    evaluated images of ``allrows``: ``jitter_evaluation`` on the two pooled confusions, the windows' row with its difference
    from the frame's.  Returns the ``"evaluation"`` entry of the summary's ``"windows"``."""
    done = {int(g[0]) for g in allrows if int(g[3]) == STATUS_OK}
    total = np.zeros((2, 3, 3), dtype=np.int64)
    for g in np.asarray(all_win, dtype=np.int64).reshape(-1, 1 + 9 * 2):
        if int(g[0]) in done:
            total += g[1:].reshape(2, 3, 3)
    table, doc = jitter_evaluation(WINDOWS_EVALUATION_ROWS, total)
    with open(os.path.join(results_dir, WINDOWS_EVALUATION_CSV), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    return doc


def report(items: List[dict], allrows: np.ndarray, precision: str, model_path: str,
           bn_stats: str = "running", loss_rows: np.ndarray = None, normalization=None,
           normalization_source: str = "arguments", ce_rows: np.ndarray = None,
           class_weights=metrics.REFERENCE_CLASS_WEIGHTS,
           class_weights_source: str = "reference", frame: bool = False) -> Tuple[List[List[str]], dict]:
    """CSV rows and summary from the gathered rank rows (rank 0); ``loss_rows``: the gathered ``LOSS_ROW_WIDTH`` rows of
    ``--loss`` (None without it); ``normalization``: the ``(mean, std)`` the run was given (None: the defaults, and no entry
    in the summary); ``ce_rows``: the gathered ``CE_ROW_WIDTH`` rows of ``--ce`` (None without it), weighted with
    ``class_weights``; ``frame``: the run framed its scans (``--frame training``), so ``too_small`` is a reason to skip one."""
    reasons = dict(SKIP_REASONS)
    if frame:
        reasons[STATUS_TOO_SMALL] = TOO_SMALL
    terms = ce_sums = None
    if loss_rows is not None:
        terms = {int(r[0]): np.ascontiguousarray(r[1:]).view(np.float64) for r in loss_rows}
    if ce_rows is not None:
        ce_sums = {int(r[0]): np.ascontiguousarray(r[1:]).view(np.float64) for r in ce_rows}
    ce_cells_of = [[] for _ in range(9)]             # per cell: the sums of the evaluated images
    rows, skipped = [], {r: [] for r in reasons.values()}
    raw_total, clean_total = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)
    for r in allrows:
        d = items[int(r[0])]
        if int(r[3]) != STATUS_OK:
            skipped[reasons[int(r[3])]].append(d["wood"] + "/" + d["name"])
            continue
        raw, clean = r[4:13].reshape(3, 3), r[13:22].reshape(3, 3)
        raw_total += raw
        clean_total += clean
        row = metrics.eval_row(d["name"], d["wood"], raw, clean)
        if terms is not None:                    # a class is present where its target row of the confusion is not empty
            row += metrics.loss_cells(terms[int(r[0])], raw.sum(axis=1))
        if ce_sums is not None:
            cells = ce_sums[int(r[0])]
            for k in range(9):
                ce_cells_of[k].append(float(cells[k]))
            row += metrics.ce_cells(cells, int(raw.sum()), class_weights, float(row[-1]) if terms is not None else None)
        rows.append(row)
    summary = {"precision": precision, "bn_statistics": bn_stats, "model_path": model_path, "images_evaluated": len(rows),
               "images_skipped": sum(len(v) for v in skipped.values()), "skipped": skipped}
    if rows:
        summary.update(metrics.summarize(rows, raw_total, clean_total))
    if terms is not None:
        summary["lovasz_softmax"] = metrics.summarize_loss(rows, len(metrics.EVAL_CSV_HEADER))
    if ce_sums is not None:
        first = len(metrics.EVAL_CSV_HEADER) + (len(metrics.LOSS_CSV_COLUMNS) if terms is not None else 0)
        summary["cross_entropy"] = metrics.summarize_ce(rows, first, [metrics._fsum(v) for v in ce_cells_of], raw_total,
                                                        class_weights, class_weights_source, mixed=terms is not None)
    if normalization is not None:
        summary["normalization"] = {"mean": list(normalization[0]), "std": list(normalization[1]),
                                    "source": normalization_source}
    return rows, summary


def evaluate_folder(root: str, model_path: str = "./best_model.pt", precision: str = "fp32", device_index: int = None,
                    batch: int = None, window: int = 64, target_size: int = 1024, calibrate: bool = True,
                    streams: int = None, arch: str = "auto", bn_stats: str = "running", precision_auto: bool = False,
                    loss: bool = False, normalization=None, normalization_source: str = "arguments", ce: bool = False,
                    class_weights=metrics.REFERENCE_CLASS_WEIGHTS, class_weights_source: str = "reference", zones: bool = False,
                    zones_cap: int = None, zone_pairs_cap: int = None, match_iou: float = None, contours: bool = False,
                    contour_tolerance: int = None, tta="none", calibration: bool = False, ece_bins: int = None,
                    jitter=None, jitter_views=None, windows: int = None, windows_stride: int = None, windows_blend: str = None,
                    windows_compare: bool = False, frame: str = "scan", frame_size: int = None, pool: int = None,
                    subset=None, as_logged: bool = False, logit_offsets=None, operating_points: bool = False,
                    bark_offsets=None, node_offsets=None) -> dict:
    """Evaluate the checkpoint on the labelled folder ``root`` (module docstring); returns this rank's statistics, with
    the summary on rank 0.  ``arch``: the network (``predict.resolve_arch``; ``"auto"`` = the one the checkpoint's keys
    name).  ``bn_stats``: ``"running"`` (eval mode) or ``"image"``, the shipped tool's per-image BatchNorm statistics
    ("fp32", FCN only; ``predict.resolve_bn_stats``), or ``"image_f16x2"``, the same on the f16x2 pipe ("f16x2" only).  ``loss``: also the per-image Lovasz-Softmax loss (module
    docstring).  ``normalization``: the ``(mean, std)`` of the ingest (``folder_run.resolve_normalization``; None: the
    defaults), set on every stream's model object; ``normalization_source``: what the summary says of where it came from.
    ``ce``: also the cross-entropy family (module docstring), weighted with ``class_weights`` (three finite values >= 0);
    ``class_weights_source``: what the summary says of where they came from.
    ``zones``: also match the zones of the final labels against the zones of the duals (module docstring): ``zones_cap`` zone
    rows per map and ``zone_pairs_cap`` pair rows per image stay on the device path (defaults ``zones.DEFAULT_CAP``,
    ``zones.DEFAULT_PAIR_CAP``), ``match_iou`` is the matching threshold in [0.5, 1) (default 0.5).  The returned dict gains
    ``zones_host_fallbacks``, this rank's images that were matched on the host.
    ``contours``: also the contour distances of the final labels against the duals (module docstring), with
    ``contour_tolerance`` pixels (an integer >= 0, default ``contours.DEFAULT_TOLERANCE``) as the tolerance of the contour
    precision, recall and F1.
    ``tta`` ("hflip", "vflip", "flips"; "none" = off): ``FCNResNet50.predict_labels_tta`` stands where ``predict_labels`` does,
    so every row and every optional pass is about the mean of the flip views; ``batch`` keeps counting images
    (default 1, 2 in bf16) and the summary gains ``"tta": {"views": [...]}``.
    ``calibration``: also the census of the softmax confidence (module docstring), with ``ece_bins`` bins (a power of two in
    1..256, default ``calibration.DEFAULT_ECE_BINS``) under the expected calibration error.
    ``jitter`` ("training") or ``jitter_views`` (1..16 (brightness, contrast, saturation) triples, or the string of
    ``--jitter_views``; not with ``tta``): ``FCNResNet50.predict_labels_jitter`` stands where ``predict_labels`` does, so every
    row and every optional pass is about the mean of the colour-jitter views; ``batch`` keeps counting images
    (default 1, 2 in bf16).  Each view's own final labels (after ``remove_small_zones``) go through ``confusion`` against the
    dual as well: rank 0 writes ``results/jitter_evaluation.csv`` (``jitter_evaluation``: a row per view, pooled over the
    folder) and the summary gains ``"jitter": {"views": [...], "factors": [...], "evaluation": {...}}``.
    ``windows`` = S (with ``windows_stride``, default S / 2 rounded down to a multiple of 8, and ``windows_blend`` "tent" or
    "uniform"; not with ``tta``, ``jitter`` or per-image ``bn_stats``; ResNet-50 networks only):
    ``FCNResNet50.predict_labels_windows`` stands where ``predict_labels`` does, so every row and every optional pass is about
    the blend of the S x S windows; ``batch`` keeps counting images (default 1, 2 in bf16) and the summary gains
    ``"windows": {"window", "stride", "blend"}``.  ``windows_compare``: the plain forward of each frame runs as well and the
    confusion of its final labels (after ``remove_small_zones``) rides back; rank 0 writes ``results/windows_evaluation.csv``
    (``jitter_evaluation`` on the rows "identity" -- the frame -- and "windows", pooled over the folder) and the summary's entry
    gains ``"evaluation"``.
    ``frame`` = "training" (with ``frame_size`` = T, default ``target_size``, 8 <= T <= ``target_size``): every scan and its dual
    are replaced by the training run's own ``T x T`` frame, ``pad_resize`` of utils.py:242-247 (``FCNResNet50.training_frame``,
    DESIGN.md 3.19), at the top of each batch; everything after that is the code above on the frame, in the training's own order
    frame -> jitter / flips / windows (__main__.py:158-165).  The rows' ``H, W`` stay the scan's.  A scan whose pad one
    reflection does not reach is skipped (``too_small``, a key of ``summary["skipped"]`` only here), one with a side beyond T
    as ``too_large``.  The summary gains ``"frame": {"kind", "size", "resampled_rows", "resampled_cols", "pool", "miou",
    "pixelwise_f1", "groups"}``: the batch-pooled figures of ``metrics.pooled_over_groups`` over consecutive groups of ``pool``
    evaluated images in list order (default 8, 1..64), host arithmetic on rank 0 from the gathered rows.  ``frame="scan"``
    (default) is the behaviour without it; ``frame_size`` and ``pool`` are refused then.
    ``as_logged`` (with ``frame="training"``; refused without): also the two figures of the training log that need a whole
    group on one device.  The shards are cut at group boundaries (``pooled_groups``; membership is known from
    the header reads), the rank keeps the low-resolution logits and the framed dual of every evaluated image on the device
    (``as_logged_bytes``; a shard beyond ``AS_LOGGED_MAX_BYTES`` is refused before the loop) and, after the loop, on one stream
    and group by group: upsample + argmax, ``lovasz_softmax_groups``, ``remove_small_zones_groups``, ``confusion``.  One
    ``GROUP_ROW_WIDTH`` row per group travels to rank 0 and ``summary["frame"]`` gains ``"as_logged": {"loss", "miou",
    "pixelwise_f1", "groups"}`` (``metrics.as_logged_over_groups``); everything else the run writes is what it writes without
    the flag.  An image that passed the header checks but dropped out in the loop (a dual that decodes to another shape than
    its header promised) would move every later group: the run then fails after the loop, on every rank alike, naming it.
    ``logit_offsets`` = ``(bark, node)``: every stream's model decides by ``argmax(x0, x1 + bark, x2 + node)``
    (``FCNResNet50.set_logit_offsets``), so the raw and the clean confusion, ``zones``, ``contours`` and the views' merges are
    all of the offset labels; ``loss``, ``ce`` and ``calibration`` describe the logits and do not change.  The summary gains
    ``"logit_offsets"``.
    ``operating_points`` (with ``bark_offsets`` / ``node_offsets``: ``"LO:HI:STEP"`` or a list, default ``-8:8:0.5``; refused
    without the flag): beside ``confusion``, on the batch's stream, ``FCNResNet50.offset_sweep`` counts the 3 x 3 confusion of
    the raw decision at every point of the grid (``operating``; it ignores ``logit_offsets``); a table of ``G1 G2 9`` int64 per
    image rides back, and rank 0 writes ``results/operating_points.csv``, ``results/operating_evaluation.csv`` and the
    summary's ``"operating_points"`` entry (``operating.write_report``).
    ``subset``: the path of a file with one ``wood_type/name`` per line, or such a list: only these samples are evaluated, in
    that order (``apply_subset``).
    Raises ``NonFiniteLogits`` on every rank alike when f16x2 cannot carry the weights."""
    import torch
    from . import zones as zn
    FT, POOL = check_frame_arguments(frame, frame_size, pool, target_size, as_logged)   # the training frame's side, None = off
    AL = bool(as_logged)
    Z = bool(zones)
    check_zone_match_arguments(Z, zones_cap, zone_pairs_cap, match_iou)     # refusals first: nothing has touched a device yet
    ZCAP = int(zones_cap) if zones_cap is not None else zn.DEFAULT_CAP
    PCAP = int(zone_pairs_cap) if zone_pairs_cap is not None else zn.DEFAULT_PAIR_CAP
    IOU = zn.check_match_iou(match_iou) if match_iou is not None else zn.DEFAULT_MATCH_IOU
    from . import contours as ct
    K = bool(contours)
    check_contour_arguments(K, contour_tolerance)
    TOL = ct.check_tolerance(contour_tolerance) if contour_tolerance is not None else ct.DEFAULT_TOLERANCE
    CBINS = ct.default_bins(target_size, target_size)   # the bins of the largest frame: the pooled histogram's
    from . import calibration as cal
    CAL = bool(calibration)
    check_calibration_arguments(CAL, ece_bins)
    EB = cal.check_ece_bins(ece_bins) if ece_bins is not None else cal.DEFAULT_ECE_BINS
    from . import operating as opm
    LO = folder_run.check_logit_offsets(logit_offsets)
    OPS = opm.check_arguments(operating_points, bark_offsets, node_offsets)   # the two grids, None = off
    OPW = OPS[0].size * OPS[1].size * 9 if OPS else 0                         # int64 per image
    if ce:
        class_weights = check_class_weights(class_weights)
    T = folder_run.check_tta_arguments(tta)         # the view mask, 0 = off
    J = folder_run.check_jitter_arguments(jitter, jitter_views, tta=tta)   # the colour views' factors, None = off
    NV = len(J) if J is not None else 0
    WN = folder_run.check_windows_arguments(windows, windows_stride, windows_blend, windows_compare, tta, jitter, jitter_views,
                                            bn_stats=bn_stats, arch=arch)   # the crop windows, None = off
    WC = WN is not None and WN.compare
    items = list_labelled(root)
    if subset is not None:                           # a refusal like the others: nothing has touched a device yet
        items = apply_subset(items, read_subset(subset) if isinstance(subset, str) else list(subset))
    r = folder_run.open_run(root, "evaluate", precision, device_index, batch, streams, target_size,
                            stack=max(1, NV, len(folder_run.tta_view_names(T))), windows=WN)
    dev, batch = r.dev, r.batch

    def warm(m):                                     # the remove_small_zones workspace (--jitter: of the views' stack) and, with ``loss`` / ``ce``, theirs
        m.remove_small_zones(torch.zeros((batch * max(1, NV), target_size, target_size), dtype=torch.uint8, device=dev))
        if loss:
            m.lovasz_softmax(torch.zeros((batch, 3, target_size, target_size), dtype=torch.float32, device=dev),
                             torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev))
        if ce:
            m.pixel_cross_entropy(torch.zeros((batch, 3, target_size, target_size), dtype=torch.float32, device=dev),
                                  torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev))
        if CAL:
            m.softmax_census(torch.zeros((batch, 3, target_size, target_size), dtype=torch.float32, device=dev),
                             torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev))
        if OPS:
            m.offset_sweep(torch.zeros((batch, 3, target_size, target_size), dtype=torch.float32, device=dev),
                           torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev), *OPS)
        if Z:                                        # match_zones' (11 bytes per pixel)
            plane = torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev)
            m.match_zones(plane, plane, cap=ZCAP, pair_cap=PCAP)
        if K:                                        # contour_distances' (9 bytes per pixel)
            plane = torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev)
            m.contour_distances(plane, plane)
        if FT:                                       # the coefficient table of a resampled axis, uploaded before the loop
            m._frame_table(FT)
        if AL and m is r.models[0]:                  # the pass after the loop runs on the first model object: its workspaces for one group
            plane = torch.zeros((POOL, FT, FT), dtype=torch.uint8, device=dev)
            m.remove_small_zones_groups(plane, POOL)
            m.lovasz_softmax_groups(torch.zeros((POOL, 3, FT, FT), dtype=torch.float32, device=dev), plane, POOL)
    folder_run.bring_up(r, model_path, arch, bn_stats, precision_auto,
                        lambda root: os.makedirs(os.path.join(root, "results"), exist_ok=True), warm,
                        normalization=normalization, logit_offsets=LO)

    def header_status(gi, h, w):                     # what the header reads say of image gi
        status = dual_status(items[gi], h, w, target_size)
        if status == STATUS_OK and FT:
            status = frame_status(h, w, FT)
        return status

    groups = header_ok = None
    if AL:                                           # groups stay whole: the shards are cut between them
        def units(sizes):
            nonlocal groups, header_ok
            header_ok = list(r.pool.map(lambda gi: header_status(gi, *sizes[gi]) == STATUS_OK, range(len(items))))
            groups, unit = pooled_groups(header_ok, POOL)
            return unit
        sizes = folder_run.shard(r, items, lambda d: image_hw(d["src"]), units=units)
        held = max(as_logged_bytes(sum(1 for gi in sh if header_ok[gi]), FT, POOL) for sh in r.shards)
        if held > AS_LOGGED_MAX_BYTES:               # every rank sees every shard: all refuse alike, before any batch
            r.pool.shutdown(wait=True, cancel_futures=True)
            raise ValueError("--as_logged would hold %d bytes on one device (the bound is %d): use more ranks or a --subset"
                             % (held, AS_LOGGED_MAX_BYTES))
    else:
        sizes = folder_run.shard(r, items, lambda d: image_hw(d["src"]))
    mine = r.mine
    kept = {}                                        # --as_logged: k -> (low-resolution logits, framed dual) on the device
    rows = np.zeros((len(mine), ROW_WIDTH), dtype=np.int64)
    loss_rows = np.zeros((len(mine), LOSS_ROW_WIDTH), dtype=np.int64) if loss else None
    if loss:
        loss_rows[:, 0] = mine
    ce_rows = np.zeros((len(mine), CE_ROW_WIDTH), dtype=np.int64) if ce else None
    if ce:
        ce_rows[:, 0] = mine

    def prepare(k):
        """Pool: the RGB frame and the grey dual of an image that can be evaluated; its status row and None otherwise."""
        gi = mine[k]
        h, w = sizes[gi]
        status = header_status(gi, h, w)
        if status == STATUS_OK:
            frame, grey = _decode_rgb(items[gi]["src"]), decode_dual(items[gi]["dual"])
            if grey.shape == frame.shape[:2]:
                return frame, grey
            status = STATUS_SHAPE_MISMATCH
        rows[k, :4] = (gi, h, w, status)
        return None

    ring = [torch.empty((2, batch, 3, 3), dtype=torch.int64).pin_memory() for _ in range(r.depth)]   # raw, clean
    loss_ring = [torch.empty((batch, 3), dtype=torch.float64).pin_memory() for _ in range(r.depth)] if loss else None
    logits_buf = [torch.empty(batch * 3 * target_size * target_size, dtype=torch.float32, device=dev)
                  for _ in range(r.n_streams)] if loss or ce or CAL or OPS else None
    ce_ring = [torch.empty((batch, 9), dtype=torch.float64).pin_memory() for _ in range(r.depth)] if ce else None
    # --zones: per slot the two zone inventories, the pair rows, the three counts per image, and the two planes an image over
    # a cap is matched from on the host
    zring = [(torch.empty((2, batch, ZCAP, zn.ZONE_ROW), dtype=torch.int64).pin_memory(),
              torch.empty((batch, PCAP, zn.PAIR_ROW), dtype=torch.int64).pin_memory(),
              torch.empty((3, batch), dtype=torch.int64).pin_memory(),
              torch.empty(2 * batch * target_size * target_size, dtype=torch.uint8).pin_memory()) for _ in range(r.depth)] if Z else None
    zres = {}                                        # k -> (output zone rows, target zone rows, pair rows)
    zfallbacks = []                                  # the k matched on the host: zones or pairs over a cap
    # --contours: per slot the rows of a batch (flat: their width follows the batch's shape) and its sum_d; per image the row
    # that travels; the rank's pooled histogram
    cring = [(torch.empty(batch * ct.SETS * (ct.HEAD + CBINS), dtype=torch.int64).pin_memory(),
              torch.empty((batch, ct.SETS), dtype=torch.float64).pin_memory()) for _ in range(r.depth)] if K else None
    cwire = np.zeros((len(mine), 1 + ct.WIRE_WIDTH), dtype=np.int64) if K else None
    if K:
        cwire[:, 0] = mine
    chist = np.zeros((ct.SETS, CBINS), dtype=np.int64) if K else None
    # --calibration: per slot the census rows of a batch; per image the row that travels; the rank's pooled census
    cal_ring = [torch.empty((batch, cal.WORDS), dtype=torch.int64).pin_memory() for _ in range(r.depth)] if CAL else None
    cal_wire = np.zeros((len(mine), 1 + cal.wire_width(EB)), dtype=np.int64) if CAL else None
    if CAL:
        cal_wire[:, 0] = mine
    cal_pool = np.zeros(cal.WORDS, dtype=np.uint64) if CAL else None
    # --operating_points: per slot the tables of a batch; per image the table that travels
    op_ring = [torch.empty((batch, OPW), dtype=torch.int64).pin_memory() for _ in range(r.depth)] if OPS else None
    op_wire = np.zeros((len(mine), 1 + OPW), dtype=np.int64) if OPS else None
    if OPS:
        op_wire[:, 0] = mine
    # --jitter: per slot the confusion of each view's final labels; per image the row that travels
    jring = [torch.empty((NV, batch, 3, 3), dtype=torch.int64).pin_memory() for _ in range(r.depth)] if NV else None
    jrows = np.zeros((len(mine), 1 + 9 * NV), dtype=np.int64) if NV else None
    if NV:
        jrows[:, 0] = -1                                              # a skipped image has no row

    # --windows_compare: per slot the confusion of the plain forward's final labels; per image the row that travels
    wring = [torch.empty((batch, 3, 3), dtype=torch.int64).pin_memory() for _ in range(r.depth)] if WC else None
    wrows = np.zeros((len(mine), 1 + 9 * 2), dtype=np.int64) if WC else None
    if WC:
        wrows[:, 0] = -1                                              # a skipped image has no row

    forward, _ = folder_run.stacked_call(T, J, WN)                    # the run's forward: plain, or on its views or windows

    def launch(slot, sid, part, x, tgt):
        mdl = r.models[sid]
        if FT:                                                        # the training's frame of the scan and of its dual
            x, tgt = mdl.training_frame(x, (FT, FT)), mdl.training_frame(tgt, (FT, FT))
        n, h, w = x.shape[:3]
        lg = logits_buf[sid][: n * 3 * h * w].view(n, 3, h, w) if loss or ce or CAL or OPS else None
        kw = dict(labels_dtype=torch.uint8, logits_full=lg,           # __main__.py:323
                  **(dict(return_lowres=True) if AL else {}))         # --as_logged: the merged low-resolution logits as well
        if NV:                                                        # the colour views; each view's own final labels beside the mean's
            labels, _, *low, _, _, _, vlow = forward(mdl, x, return_views=True, **kw)
            vlab, _ = mdl.upsample_argmax(vlow.view((NV * n,) + tuple(vlow.shape[2:])), (h, w), labels_dtype=torch.uint8)
            mdl.remove_small_zones(vlab)
            jring[slot][:, :n].copy_(mdl.confusion(vlab, tgt.repeat(NV, 1, 1)).view(NV, n, 3, 3), non_blocking=True)
        else:                                                         # the plain call, or the same on the flip views or the crop windows
            labels, _, *low = forward(mdl, x, **kw)
            if WC:                                                    # the plain forward's final labels beside the windows'
                plab, _ = mdl.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
                wring[slot][:n].copy_(mdl.confusion(plab, tgt), non_blocking=True)
        if AL:                                                        # copies of their own: nothing of the batch stays alive for them
            for j, k in enumerate(part):
                kept[k] = (low[0][j].clone(), tgt[j].clone())
        conf_raw = mdl.confusion(labels, tgt)                         # iou: the raw argmax (:331)
        if ce:                                                        # CustomWeightedCrossEntropy (utils.py:151-165)
            sums, _ = mdl.pixel_cross_entropy(lg, tgt)
            ce_ring[slot][:n].copy_(sums.view(n, 9), non_blocking=True)
        if CAL:                                                       # the raw softmax, before remove_small_zones
            census, _ = mdl.softmax_census(lg, tgt)
            cal_ring[slot][:n].copy_(census.view(torch.int64), non_blocking=True)
        if OPS:                                                       # the raw decision at every grid point, like the census
            tables = mdl.offset_sweep(lg, tgt, *OPS)
            op_ring[slot][:n].copy_(tables.view(torch.int64).view(n, OPW), non_blocking=True)
        if loss:                                                      # LovaszSoftmax (:236-239)
            terms, _ = mdl.lovasz_softmax(lg, tgt)
            loss_ring[slot][:n].copy_(terms, non_blocking=True)
        mdl.remove_small_zones(labels)                                # PixelWiseF1 (utils.py:213)
        conf_clean = mdl.confusion(labels, tgt)
        ring[slot][0, :n].copy_(conf_raw, non_blocking=True)
        ring[slot][1, :n].copy_(conf_clean, non_blocking=True)
        if Z:                                                         # the labels PixelWiseF1 sees, against the same dual
            zr, pr, nums, planes = zring[slot]
            o_rows, o_num, t_rows, t_num, p_rows, p_num = mdl.match_zones(labels, tgt, cap=ZCAP, pair_cap=PCAP)
            zr[0, :n].copy_(o_rows, non_blocking=True)
            zr[1, :n].copy_(t_rows, non_blocking=True)
            pr[:n].copy_(p_rows, non_blocking=True)
            for i, t in enumerate((o_num, t_num, p_num)):
                nums[i, :n].copy_(t, non_blocking=True)
            planes[: n * h * w].copy_(labels.reshape(-1), non_blocking=True)
            planes[n * h * w: 2 * n * h * w].copy_(tgt.reshape(-1), non_blocking=True)
        if K:                                                         # the same labels against the same dual
            c_rows, c_sum = mdl.contour_distances(labels, tgt)
            cring[slot][0][: c_rows.numel()].copy_(c_rows.reshape(-1), non_blocking=True)
            cring[slot][1][:n].copy_(c_sum, non_blocking=True)

    def match_on_host(k, lab, grey):                 # pool: an image over a cap, from the two planes
        zres[k] = zn.match_cpu(lab, zn.target_classes(grey))[0]

    def consume(slot, part, n, h, w):
        conf = ring[slot][:, :n].numpy().reshape(2, n, 9)
        futures = []
        fh, fw = (FT, FT) if FT else (h, w)          # the planes' shape: the frame's under --frame training, else the scan's
        if Z:
            zr, pr, nums, planes = (t.numpy() for t in zring[slot])
            for j, k in enumerate(part):
                no, nt, npairs = (int(v) for v in nums[:, j])
                if no > ZCAP or nt > ZCAP or npairs > PCAP:
                    zfallbacks.append(k)
                    lab, grey = (planes[a * n * fh * fw:][j * fh * fw: (j + 1) * fh * fw].reshape(fh, fw).copy() for a in (0, 1))
                    futures.append(r.pool.submit(match_on_host, k, lab, grey))
                else:
                    zres[k] = (zr[0, j, :no].copy(), zr[1, j, :nt].copy(), pr[j, :npairs].copy())
        if K:
            width = ct.HEAD + ct.default_bins(fh, fw)
            c_rows = cring[slot][0][: n * ct.SETS * width].numpy().reshape(n, ct.SETS, width)
            wire = ct.wire_rows(c_rows, cring[slot][1][:n].numpy(), TOL)
            chist[...] += ct.pooled_histogram(c_rows, CBINS)
            for j, k in enumerate(part):
                cwire[k, 1:] = wire[j]
        if CAL:
            census = cal_ring[slot][:n].numpy()
            cal_pool[...] += cal.pool(census)
            wire = cal.wire_rows(census, EB)
            for j, k in enumerate(part):
                cal_wire[k, 1:] = wire[j]
        if OPS:
            tables = op_ring[slot][:n].numpy()
            for j, k in enumerate(part):
                op_wire[k, 1:] = tables[j]
        for j, k in enumerate(part):
            rows[k, :4] = (mine[k], h, w, STATUS_OK)
            rows[k, 4:13], rows[k, 13:] = conf[0, j], conf[1, j]
            if loss:
                loss_rows[k, 1:] = loss_ring[slot][j].numpy().view(np.int64)
            if ce:
                ce_rows[k, 1:] = ce_ring[slot][j].numpy().view(np.int64)
            if NV:
                jrows[k, 0], jrows[k, 1:] = mine[k], jring[slot][:, j].numpy().reshape(-1)
            if WC:                                                    # the frame's confusion, then the windows' (the clean one)
                wrows[k, 0], wrows[k, 1:10], wrows[k, 10:] = mine[k], wring[slot][j].numpy().reshape(-1), conf[1, j]
        return futures

    def first_frame():                               # the calibration guard's: this rank's first image that fits
        first = next((gi for gi in mine if max(sizes[gi]) <= target_size and (not FT or frame_status(*sizes[gi], FT) == STATUS_OK)), None)
        if first is None:
            return None
        rgb = _decode_rgb(items[first]["src"])
        if FT:                                       # framed like every batch
            rgb = r.models[0].training_frame(torch.from_numpy(np.ascontiguousarray(rgb[None])).to(dev), (FT, FT))[0].cpu().numpy()
        return rgb

    folder_run.run_loop(r, window, prepare, launch, consume, first_frame, calibrate, bytes_per_pixel=(3, 1))
    group_rows = None
    if AL:                                           # the loop has drained (run_loop synchronises): one stream from here on
        local = {gi: k for k, gi in enumerate(mine)}
        whole = all(rows[k, 3] == STATUS_OK for k, gi in enumerate(mine) if header_ok[gi])
        todo = [g for g in groups if g[0] in local] if whole else []   # a drop-out moves the groups: the run fails below
        group_rows = np.zeros((len(todo), GROUP_ROW_WIDTH), dtype=np.int64)
        mdl = r.models[0]
        with torch.cuda.stream(r.gpu_streams[0]):
            for i, g in enumerate(todo):
                low = torch.stack([kept[local[gi]][0] for gi in g])
                tgt = torch.stack([kept[local[gi]][1] for gi in g])
                lg = torch.empty((len(g), 3, FT, FT), dtype=torch.float32, device=dev)
                labels, _ = mdl.upsample_argmax(low, (FT, FT), labels_dtype=torch.uint8, logits_full=lg)   # the loop's own bits
                terms, counts = mdl.lovasz_softmax_groups(lg, tgt, len(g))                                 # LovaszSoftmax on the batch
                mdl.remove_small_zones_groups(labels, len(g))                                             # PixelWiseF1 (utils.py:211-214)
                clean = mdl.confusion(labels, tgt).sum(dim=0)
                group_rows[i, 0], group_rows[i, 1] = g[0], len(g)
                group_rows[i, 2:11] = clean.reshape(-1).cpu().numpy()
                group_rows[i, 11:14] = terms[0].cpu().numpy().view(np.int64)
                group_rows[i, 14:17] = counts[0].cpu().numpy()
        torch.cuda.synchronize(dev)
        kept.clear()
    allrows = folder_run.gather(r, rows, ROW_WIDTH)
    if AL:                                           # every rank holds every row: all of them fail alike
        dropped = [int(g[0]) for g in allrows if header_ok[int(g[0])] and int(g[3]) != STATUS_OK]
        all_groups = folder_run.gather_ragged(group_rows, r.world, r.dist, r.wire_dev, width=GROUP_ROW_WIDTH)
        if dropped:
            if r.dist is not None:
                r.dist.barrier()
            raise RuntimeError("--as_logged: %s passed the header checks but could not be evaluated (%s): every later group "
                               "would move; take the sample out with --subset" % (
                                   ", ".join(items[gi]["wood"] + "/" + items[gi]["name"] for gi in dropped),
                                   ", ".join(sorted({SKIP_REASONS.get(int(g[3]), TOO_SMALL) for g in allrows if int(g[0]) in dropped}))))
    all_loss = folder_run.gather(r, loss_rows, LOSS_ROW_WIDTH) if loss else None
    all_ce = folder_run.gather(r, ce_rows, CE_ROW_WIDTH) if ce else None
    all_zones = n_fallbacks = None
    if Z:                                            # three ragged row sets, an image's rows together and in order
        def local(which, width):
            parts = [np.concatenate([np.full((len(zres[k][which]), 1), mine[k], dtype=np.int64), zres[k][which]], axis=1)
                     for k in sorted(zres)]
            return np.concatenate(parts) if parts else np.zeros((0, 1 + width), dtype=np.int64)
        all_zones = [folder_run.gather_ragged(local(i, wd), r.world, r.dist, r.wire_dev, width=1 + wd)
                     for i, wd in enumerate((zn.ZONE_ROW, zn.ZONE_ROW, zn.PAIR_ROW))]
        n_fallbacks = len(folder_run.gather(r, np.array([[mine[k]] for k in sorted(zfallbacks)], dtype=np.int64).reshape(-1, 1), 1))
    all_wire = all_hist = None
    if K:                                            # a fixed-width row per image and one pooled histogram per rank
        all_wire = folder_run.gather(r, cwire, 1 + ct.WIRE_WIDTH)
        all_hist = folder_run.gather_ragged(np.concatenate([[r.rank], chist.ravel()])[None], r.world, r.dist, r.wire_dev,
                                            width=1 + chist.size)[:, 1:].sum(axis=0).reshape(chist.shape)
    all_cal = all_census = None
    if CAL:                                          # a fixed-width row per image and one pooled census per rank
        all_cal = folder_run.gather(r, cal_wire, 1 + cal.wire_width(EB))
        all_census = cal.pool(folder_run.gather_ragged(np.concatenate([[r.rank], cal_pool.view(np.int64)])[None], r.world, r.dist,
                                                       r.wire_dev, width=1 + cal.WORDS)[:, 1:])
    all_op = folder_run.gather(r, op_wire, 1 + OPW) if OPS else None
    all_views = folder_run.gather(r, jrows, 1 + 9 * NV) if NV else None
    all_win = folder_run.gather(r, wrows, 1 + 9 * 2) if WC else None
    summary = gathered = None
    if r.rank == 0:
        gathered = allrows.tolist()
        csv_rows, summary = report(items, allrows, r.precision, model_path, bn_stats, loss_rows=all_loss,
                                   normalization=normalization, normalization_source=normalization_source,
                                   **(dict(ce_rows=all_ce, class_weights=class_weights,
                                           class_weights_source=class_weights_source) if ce else {}),
                                   **(dict(frame=True) if FT else {}))
        write_stats_csv(os.path.join(root, STATS_CSV), csv_rows, loss=loss, **(dict(ce=True) if ce else {}))
        if Z:
            summary["zones"] = write_zone_match_report(os.path.join(root, "results"), items, allrows, *all_zones, IOU, ZCAP, PCAP,
                                                       n_fallbacks)
        if K:
            summary["contours"] = write_contour_report(os.path.join(root, "results"), items, allrows, all_wire, all_hist, TOL)
        if CAL:
            summary["calibration"] = write_calibration_report(os.path.join(root, "results"), items, allrows, all_cal, all_census, EB)
        if LO is not None:
            summary["logit_offsets"] = list(LO)
        if OPS:
            summary["operating_points"] = write_operating_report(os.path.join(root, "results"), items, allrows, all_op, OPS, LO)
        if FT:
            summary["frame"] = frame_report(allrows, FT, POOL)
        if AL:
            summary["frame"]["as_logged"] = as_logged_report(allrows, all_groups, POOL)
        if T:
            summary["tta"] = {"views": folder_run.tta_view_names(T)}
        if NV:
            summary["jitter"] = write_jitter_evaluation(os.path.join(root, "results"), allrows, all_views, J)
        if WN is not None:
            summary["windows"] = {"window": WN.window, "stride": WN.stride, "blend": WN.blend}
            if WC:
                summary["windows"]["evaluation"] = write_windows_evaluation(os.path.join(root, "results"), allrows, all_win)
        with open(os.path.join(root, SUMMARY_JSON), "w") as f:
            json.dump(summary, f, indent=1)
    out = dict(folder_run.finish(r), images_evaluated_this_rank=int((rows[:, 3] == STATUS_OK).sum()), summary=summary,
               rows=gathered)
    if loss:                                     # rank 0: {global_idx: float64 [3] terms}
        out["loss_terms"] = None if r.rank != 0 else {
            int(g[0]): np.ascontiguousarray(g[1:]).view(np.float64).copy() for g in all_loss}
    if Z:
        out["zones_host_fallbacks"] = len(zfallbacks)
    if ce:                                       # rank 0: {global_idx: float64 [3,3] cell sums}
        out["ce_sums"] = None if r.rank != 0 else {
            int(g[0]): np.ascontiguousarray(g[1:]).view(np.float64).reshape(3, 3).copy() for g in all_ce}
    return out


def format_summary(summary: dict) -> str:
    lines = ["evaluated %d images in %s%s (checkpoint %s), skipped %d%s" % (
        summary["images_evaluated"], summary["precision"],
        ", per-image BatchNorm statistics" if summary.get("bn_statistics") in ("image", "image_f16x2") else "", summary["model_path"],
        summary["images_skipped"],
        "".join("; %s: %s" % (r, ", ".join(v)) for r, v in summary["skipped"].items() if v))]
    if "normalization" in summary:
        nm = summary["normalization"]
        lines.append("normalised with mean %s, std %s (%s)" % (nm["mean"], nm["std"], nm["source"]))
    if "pooled" in summary:
        p = summary["pooled"]
        lines.append("pooled over all pixels: " + ", ".join("%s %.3f" % (k, p[k]) for k in p))
        m = summary["column_means"]
        lines.append("mean over images: " + ", ".join("%s %.3f" % (k, m[k]) for k in m))
    if summary.get("lovasz_softmax"):
        ls = summary["lovasz_softmax"]
        fmt = lambda v: "-" if v is None else "%.6f" % v
        lines.append("lovasz_softmax loss: mean over images %s (per class, over the images where it is present: %s)" % (
            fmt(ls["mean_over_images"]), ", ".join("%s %s" % (k, fmt(v)) for k, v in ls["per_class_mean"].items())))
    if summary.get("cross_entropy"):
        ce = summary["cross_entropy"]
        fmt = lambda v: "-" if v is None else "%.6f" % v
        lines.append("cross-entropy: mean over images %s; class weights %s (%s)" % (
            ", ".join("%s %s" % (k, fmt(v)) for k, v in ce["mean_over_images"].items()),
            " ".join(repr(v) for v in ce["class_weights"]), ce["class_weights_source"]))
    if summary.get("zones"):
        z = summary["zones"]
        fmt = lambda v: "-" if v is None else "%.3f" % v
        for name in ("Bark", "Node"):
            c = z[name]
            lines.append("%s zones at IoU > %s: %d of %d target zones matched (%d output zones, %d spurious; %d split targets, %d "
                         "merged outputs): recall %s, precision %s, F1 %s, mean matched IoU %s" % (
                             name, z["match_iou"], c["matched"], c["targets"], c["outputs"], c["spurious"], c["split_targets"],
                             c["merged_outputs"], fmt(c["recall"]), fmt(c["precision"]), fmt(c["f1"]), fmt(c["mean_iou"])))
        if z["host_fallbacks"]:
            lines.append("%d images over a cap were matched on the host" % z["host_fallbacks"])
    if summary.get("calibration"):
        c = summary["calibration"]
        fmt = lambda v, spec="%.4f": "-" if v is None else spec % v
        p = c["pooled"]
        lines.append("calibration over %d bins: ECE %s, MCE %s, accuracy %s, mean confidence %s, Brier %s; " % (
            c["ece_bins"], fmt(p["ece"]), fmt(p["mce"]), fmt(p["accuracy"]), fmt(p["mean_confidence"]), fmt(p["brier"])) + "; ".join(
            "%s AP %s, AUROC %s, best F1 %s at p >= %s (argmax: %s)" % (
                name, fmt(c[name]["average_precision"]), fmt(c[name]["auroc"]), fmt(c[name]["best_f1"]),
                fmt(c[name]["best_f1_threshold"], "%.3f"), fmt(c[name]["f1_at_argmax"])) for name in ("Bark", "Node")))
    if summary.get("logit_offsets"):
        lines.append("labels decided by argmax(x0, x1 + %r, x2 + %r) (--logit_offsets)" % tuple(summary["logit_offsets"]))
    if summary.get("operating_points"):
        for name, p in summary["operating_points"]["points"].items():
            f = p["figures"]
            lines.append("operating point %s: %s%s: miou %.3f, f1_mean %.3f, f1_node %.3f, Output Bark %% %s (target %s), Output "
                         "Node %% %s (target %s)" % (name, p["arguments"], " (on the grid's edge: widen it)" if p["on_edge"] else "",
                                                     f["miou"], f["f1_mean"], f["f1_node"], f["Output Bark %"], f["Target Bark %"],
                                                     f["Output Node %"], f["Target Node %"]))
    if summary.get("frame"):
        fr = summary["frame"]
        fmt = lambda v: "-" if v is None else "%.3f" % v
        lines.append("on the training's %d x %d frame (%d images resampled along rows, %d along columns); pooled over groups of "
                     "%d: miou %s, pixelwise_f1 %s" % (fr["size"], fr["size"], fr["resampled_rows"], fr["resampled_cols"], fr["pool"],
                                                       fmt(fr["miou"]), fmt(fr["pixelwise_f1"])))
        if fr.get("as_logged"):
            al = fr["as_logged"]
            lines.append("as the training logged it (the loss and the small zones of each group as one batch): loss %s, miou %s, "
                         "pixelwise_f1 %s" % ("-" if al["loss"] is None else "%.6f" % al["loss"], fmt(al["miou"]), fmt(al["pixelwise_f1"])))
    if summary.get("jitter"):
        for name, entry in summary["jitter"]["evaluation"].items():
            f, d = entry["figures"], entry["difference"]
            lines.append("view %s (its own final labels, pooled): " % name + ", ".join(
                "%s %.3f%s" % (k, f[k], "" if d is None else " (%+.3f)" % d[k]) for k in ("iou_mean", "f1_mean", "Bark %", "Node %")))
    if summary.get("windows"):
        wn = summary["windows"]
        lines.append("crop windows of %d pixels every %d, %s blend" % (wn["window"], wn["stride"], wn["blend"]))
        for name, entry in (wn.get("evaluation") or {}).items():
            f, d = entry["figures"], entry["difference"]
            lines.append("%s (final labels, pooled): " % ("the frame" if name == "identity" else "the windows") + ", ".join(
                "%s %.3f (%+.3f)" % (k, f[k], d[k]) for k in ("iou_mean", "f1_mean", "Bark %", "Node %")))
    if summary.get("contours"):
        c = summary["contours"]
        fmt = lambda v, spec: "-" if v is None else spec % v
        lines.append("contours within %d px (%.1f mm): " % (c["tolerance_pixels"], c["tolerance_mm"]) + "; ".join(
            "%s precision %s, recall %s, F1 %s, mean distance %s mm (%d one-sided images)" % (
                name, fmt(c[name]["precision"], "%.3f"), fmt(c[name]["recall"], "%.3f"), fmt(c[name]["f1"], "%.3f"),
                fmt(c[name]["mean_distance_mm"], "%.2f"), c[name]["one_sided"]) for name in ("Bark", "Node")))
    return "\n".join(lines)


def main(argv=None):
    import sys
    ap = argparse.ArgumentParser(description="MI355X evaluation of a checkpoint on a labelled folder (samples/ + duals/): "
                                             "per-image IoU and F1 like bark_calculator/__main__.py")
    ap.add_argument("root_path", metavar="ROOT")
    folder_run.add_shared_arguments(ap)
    ap.add_argument("--loss", action="store_true",
                    help="also the per-image Lovasz-Softmax loss, the training objective (four more CSV columns, computed on the GPU)")
    ap.add_argument("--ce", action="store_true",
                    help="also the cross-entropy the shipped checkpoint was trained on: cross_entropy and weighted_cross_entropy "
                         "columns (and mixed_loss with --loss), summed on the GPU")
    ap.add_argument("--class_weights", type=float, nargs=3, metavar=("W0", "W1", "W2"), default=None,
                    help="--ce: the class weights (default: the reference's 0.4004 2.0334 93.1921)")
    ap.add_argument("--class_weights_from", metavar="PATH", default=None,
                    help="--ce: take the class weights from the pos_weight of a dataset_stats.json (python -m "
                         "neuralbarkcalculator_amd.stats)")
    ap.add_argument("--zones", action="store_true",
                    help="also match the zones of the final labels against the zones of the duals on the device (which output "
                         "zone is which target zone, and how well they overlap) and write results/zone_matches.csv, "
                         "zone_evaluation.csv and a \"zones\" entry in the summary")
    ap.add_argument("--zones_cap", type=int, default=None, metavar="ROWS",
                    help="with --zones: zone rows per map the device pass keeps (default 1024); an image over a cap is matched "
                         "on the host, the files do not depend on it")
    ap.add_argument("--zone_pairs_cap", type=int, default=None, metavar="ROWS",
                    help="with --zones: (output zone, target zone) rows per image the device pass keeps (default 2048, at most 4096)")
    ap.add_argument("--match_iou", type=float, default=None, metavar="T",
                    help="with --zones: two zones match when their IoU exceeds T, 0.5 <= T < 1 (default 0.5)")
    ap.add_argument("--contours", action="store_true",
                    help="also measure how far the contours of the final labels lie from the contours of the duals, on the "
                         "device, and write results/contour_evaluation.csv (contour precision / recall / F1, mean contour "
                         "distance, HD95 and Hausdorff distance in mm) and a \"contours\" entry in the summary")
    ap.add_argument("--contour_tolerance", type=int, default=None, metavar="PX",
                    help="with --contours: a contour pixel within PX pixels of the other contour counts as found, an integer "
                         ">= 0 (default 2: 7.2 mm)")
    ap.add_argument("--calibration", action="store_true",
                    help="also tally the softmax confidence against the duals on the device (raw softmax, before "
                         "remove_small_zones) and write results/calibration_evaluation.csv (ECE, MCE, accuracy, mean confidence, "
                         "Brier score, soft Jaccard, expected class shares), results/calibration_curves.csv (precision / recall / "
                         "F1 per class and threshold, the reliability table) and a \"calibration\" entry in the summary")
    ap.add_argument("--ece_bins", type=int, default=None, metavar="BINS",
                    help="with --calibration: the bins under ECE and MCE, a power of two in 1..256 (default 16)")
    ap.add_argument("--operating_points", action="store_true",
                    help="also sweep the operating point on the device: the 3 x 3 confusion of argmax(x0, x1 + b1, x2 + b2) of the "
                         "raw logits (before remove_small_zones; --logit_offsets does not reach it) at every point of a grid of "
                         "(bark, node) offsets, and write results/operating_points.csv, results/operating_evaluation.csv and an "
                         "\"operating_points\" entry in the summary that names the best-mIoU, best-F1 and area-unbiased points as "
                         "ready --logit_offsets arguments.  G1 * G2 * 9 int64 per image ride back: 78 408 bytes at the default grid")
    ap.add_argument("--bark_offsets", default=None, metavar="LO:HI:STEP",
                    help="with --operating_points: the grid of the bark offset, at most 33 values (default -8:8:0.5)")
    ap.add_argument("--node_offsets", default=None, metavar="LO:HI:STEP",
                    help="with --operating_points: the grid of the node offset, at most 33 values (default -8:8:0.5)")
    ap.add_argument("--frame", default="scan", metavar="{scan,training}",
                    help="training: score every scan and its dual on the training run's own frame, pad_resize to T x T (reflection "
                         "pad, PIL's bilinear resize where the padded length is T + 1), made on the device; everything else runs "
                         "on that frame, and the summary gains the batch-pooled miou and pixelwise_f1 that the training log holds.  "
                         "scan (default): each scan at its own shape")
    ap.add_argument("--frame_size", type=int, default=None, metavar="T",
                    help="with --frame training: the frame's side, 8 <= T <= 1024 (default 1024)")
    ap.add_argument("--pool", type=int, default=None, metavar="B",
                    help="with --frame training: the images per pooled group, in list order, 1..64 (default 8, the reference's "
                         "validation batch)")
    ap.add_argument("--as_logged", action="store_true",
                    help="with --frame training: also the loss and the PixelWiseF1 exactly as a training run logged them, each group "
                         "of --pool frames as one batch (the Lovasz-Softmax loss sorts the errors of the whole group; "
                         "remove_small_zones links zones of neighbouring frames of a group); summary[\"frame\"][\"as_logged\"].  Holds "
                         "the low-resolution logits and the framed dual of every evaluated frame of a rank's shard on its device "
                         "until the loop ends (1.2 MB per frame at T = 1024) and about 46 bytes per pixel of one group after it "
                         "(0.4 GB at --pool 8, 3.1 GB at 64); a shard that would need more than 32 GiB is refused")
    ap.add_argument("--subset", default=None, metavar="PATH",
                    help="evaluate only the samples this file names, one wood_type/name per line, in the file's order")
    ap.add_argument("--exclude_nodes", action="store_true", help=argparse.SUPPRESS)
    raw = list(sys.argv[1:] if argv is None else argv)
    args = ap.parse_args(raw)
    folder_run.resolve_arguments(ap, args)
    try:
        check_zone_match_arguments(args.zones, args.zones_cap, args.zone_pairs_cap, args.match_iou)
        check_contour_arguments(args.contours, args.contour_tolerance)
        check_calibration_arguments(args.calibration, args.ece_bins)
        folder_run.check_jitter_arguments(args.jitter, args.jitter_views, tta=args.tta)
        folder_run.check_windows_arguments(args.windows, args.windows_stride, args.windows_blend, args.windows_compare, args.tta,
                                           args.jitter, args.jitter_views, bn_stats=args.bn_stats, arch=args.arch)
        check_frame_arguments(args.frame, args.frame_size, args.pool, as_logged=args.as_logged)
        from . import operating as opm
        opm.check_arguments(args.operating_points, args.bark_offsets, args.node_offsets)
        args.logit_offsets = folder_run.check_logit_offsets(args.logit_offsets)
        if args.subset is not None:
            apply_subset(list_labelled(args.root_path), read_subset(args.subset))
    except (OSError, ValueError) as e:
        ap.error(str(e))
    if args.exclude_nodes:
        raise SystemExit("evaluate: --exclude_nodes is not supported: IoU and F1 are defined on the three classes "
                         "(nothing, bark, node) of the duals")
    if args.class_weights is not None and args.class_weights_from is not None:
        ap.error("--class_weights and --class_weights_from exclude each other")
    if (args.class_weights is not None or args.class_weights_from is not None) and not args.ce:
        ap.error("--class_weights and --class_weights_from need --ce")
    ce_kw = {}
    if args.ce:
        try:
            if args.class_weights is not None:
                ce_kw = dict(class_weights=check_class_weights(args.class_weights), class_weights_source="arguments")
            elif args.class_weights_from is not None:
                ce_kw = dict(class_weights=class_weights_from(args.class_weights_from),
                             class_weights_source=args.class_weights_from)
        except (OSError, ValueError) as e:
            ap.error(str(e))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, raw, module="neuralbarkcalculator_amd.evaluate"))
    idx = None if "WORLD_SIZE" in os.environ else 0
    kw = dict(batch=args.batch, streams=args.streams, arch=args.arch, bn_stats=args.bn_stats)
    if args.loss:
        kw["loss"] = True
    if args.ce:
        kw.update(ce=True, **ce_kw)
    if args.zones:
        kw.update(zones=True, zones_cap=args.zones_cap, zone_pairs_cap=args.zone_pairs_cap, match_iou=args.match_iou)
    if args.contours:
        kw.update(contours=True, contour_tolerance=args.contour_tolerance)
    if args.calibration:
        kw.update(calibration=True, ece_bins=args.ece_bins)
    if args.tta != "none":
        kw["tta"] = args.tta
    if args.jitter is not None or args.jitter_views is not None:
        kw.update(jitter=args.jitter, jitter_views=args.jitter_views)
    if args.windows is not None:
        kw.update(windows=args.windows, windows_stride=args.windows_stride, windows_blend=args.windows_blend,
                  windows_compare=args.windows_compare)
    if args.frame != "scan":
        kw.update(frame=args.frame, frame_size=args.frame_size, pool=args.pool)
        if args.as_logged:
            kw["as_logged"] = True
    if args.subset is not None:
        kw["subset"] = args.subset
    if args.logit_offsets is not None:
        kw["logit_offsets"] = args.logit_offsets
    if args.operating_points:
        kw.update(operating_points=True, bark_offsets=args.bark_offsets, node_offsets=args.node_offsets)
    if args.normalization is not None:
        kw["normalization"] = args.normalization
        if args.stats is not None:
            kw["normalization_source"] = args.stats
    stats = folder_run.run_precision("evaluate", lambda precision, **over: evaluate_folder(
        args.root_path, args.model_path, precision, idx, **dict(kw, **over)), args.precision, args.bn_stats)
    if stats["rank"] == 0:
        print(format_summary(stats["summary"]))
        print("%(images_total)d images (%(images_this_rank)d on rank 0, %(batches)d batches): %(total_s).2f s, "
              "%(images_per_s_loop).1f images/s in the loop on this rank" % stats, flush=True)


if __name__ == "__main__":
    main()
