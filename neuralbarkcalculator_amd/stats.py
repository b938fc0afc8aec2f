"""Dataset statistics of a labelled folder, counted on the GPU: the per-channel mean / std the network's input is normalised
with, and the class counts behind the loss's class weights.

The reference prints these two things first (__main__.py:204-208) and evaluates with the first of them:

* ``compute_mean_std`` (utils.py:23-39): per image, ``ToTensor`` then the mean and the unbiased standard deviation of each
  channel over the pixels; the dataset's value is the **mean over images of the per-image values** (not the pooled
  standard deviation, and an image's size does not weigh it);
* ``compute_pos_weight`` (utils.py:51-69): the pixels of each class over every target, ``total / (3 * count)``.

Here the pixels are only counted on the device: ``image_moments`` (nbc_image_moments) returns each image's exact integer
``sum v`` and ``sum v*v`` per channel, ``target_counts`` (nbc_target_counts) its pixels per class.  Everything after that is
exact integer arithmetic on the host until the last step (``image_mean_std``): one rounding for a mean, two for a standard
deviation, and ``math.fsum`` over the images, so the result depends neither on the order of the images nor on the number of
ranks.  (The reference sums float32 values pixel by pixel; it lands within 1e-6 relative of these, tests/test_stats_abi.py.)

``python -m neuralbarkcalculator_amd.stats ROOT [--gpus N] [--batch B] [--streams S]`` (``stats_folder``):

* input: the listing of ``evaluate.list_labelled`` (``ROOT/samples/<wood_type>/<name>`` and the dual each would have).  No
  checkpoint is read and no model object is made;
* the machinery is ``folder_run``'s: contiguous pixel-balanced shards, equal-shape batches on their own HIP streams, pinned
  rings; per batch the two kernels run on the batch's stream and ``[n,3,2]`` + ``[n,4]`` integers come back.  A frame of any
  size with ``H * W < 2^31`` is taken as it is (there is no ``too_large``);
* statuses: ``ok``; ``no_dual``: the sample still contributes to mean / std, and nothing to the class counts -- the reference
  would count an all-"Nothing" mask there, the same departure ``evaluate`` makes; ``shape_mismatch`` (a dual of another
  shape): the sample is counted, the dual is not, and the summary lists it.  Such an image travels with an all-zero mask
  whose counts the host drops;
* each rank fills int64 rows ``(global_idx, H, W, status, 6 moments, 4 counts)`` that one ``all_gather`` brings to rank 0;
* output: ``ROOT/results/dataset_stats.json`` (``mean``, ``std``: three floats each, every bit kept; ``class_counts``;
  ``pos_weight``, null for a class with no pixel in the folder, where the reference divides by zero; ``off_level_pixels``:
  dual pixels whose grey level is none of 0, 127, 255; ``images``; ``images_with_dual``; ``skipped``) -- the file
  ``predict --stats`` and ``evaluate --stats`` read -- and ``ROOT/results/dataset_stats.csv``, one tab-separated row per
  image (``CSV_HEADER``; the count cells are empty without a usable dual).  ``n_bark + n_node`` of a row is the
  ``sample_weight`` of ``get_splits`` (utils.py:94-95).  The summary is printed as well.
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, folder_run
from .evaluate import decode_dual, image_hw, list_labelled
from .folder_run import launch_ranks
from .predict import _decode_rgb

ROW_WIDTH = 14                                   # (global_idx, H, W, status, moments[3][2], counts[4])
STATUS_OK, STATUS_NO_DUAL, STATUS_SHAPE_MISMATCH = 0, 1, 2
SKIP_REASONS = {STATUS_NO_DUAL: "no_dual", STATUS_SHAPE_MISMATCH: "shape_mismatch"}
STATS_JSON = os.path.join("results", "dataset_stats.json")
STATS_CSV = os.path.join("results", "dataset_stats.csv")
CSV_HEADER = ["Name", "Type", "H", "W", "mean_r", "mean_g", "mean_b", "std_r", "std_g", "std_b",
              "n_nothing", "n_bark", "n_node", "off_level"]


# ---- the two entry points on tensors ---------------------------------------------------------------------------------
def _check_u8(t, what: str, dims: Sequence[int]):
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.uint8 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous uint8 tensor on a GPU" % what)
    if t.dim() not in dims or t.numel() == 0:
        raise ValueError("%s has the wrong number of dimensions, or is empty" % what)


def image_moments(x_u8):
    """nbc_image_moments: contiguous uint8 ``[N,H,W,3]`` / ``[H,W,3]`` RGB frames on a GPU -> int64 ``[N,3,2]`` on the same
    device, ``[n, c] = (sum v, sum v*v)`` over the pixels of channel c (every sum is below 2^47, so int64 holds the library's
    uint64 unchanged).  Runs on the current stream."""
    import torch
    _check_u8(x_u8, "x_u8", (3, 4))
    if x_u8.shape[-1] != 3:
        raise ValueError("x_u8 must be [N,H,W,3] or [H,W,3]")
    n = 1 if x_u8.dim() == 3 else int(x_u8.shape[0])
    h, w = int(x_u8.shape[-3]), int(x_u8.shape[-2])
    out = torch.empty((n, 3, 2), dtype=torch.int64, device=x_u8.device)
    with torch.cuda.device(x_u8.device):
        stream = torch.cuda.current_stream(x_u8.device).cuda_stream
        _lib.check(_lib.load().nbc_image_moments(x_u8.data_ptr(), n, h, w, out.data_ptr(), stream), "nbc_image_moments")
    return out


def target_counts(grey):
    """nbc_target_counts: contiguous uint8 ``[N,H,W]`` / ``[H,W]`` grey masks on a GPU -> int64 ``[N,4]`` on the same device:
    the pixels of class 0, 1, 2 (``metrics.target_classes``) and the pixels whose level is none of 0, 127, 255.  Runs on
    the current stream."""
    import torch
    _check_u8(grey, "grey", (2, 3))
    n = 1 if grey.dim() == 2 else int(grey.shape[0])
    h, w = int(grey.shape[-2]), int(grey.shape[-1])
    out = torch.empty((n, 4), dtype=torch.int64, device=grey.device)
    with torch.cuda.device(grey.device):
        stream = torch.cuda.current_stream(grey.device).cuda_stream
        _lib.check(_lib.load().nbc_target_counts(grey.data_ptr(), n, h, w, out.data_ptr(), stream), "nbc_target_counts")
    return out


# ---- host arithmetic -------------------------------------------------------------------------------------------------
def image_mean_std(h: int, w: int, moments) -> Tuple[List[float], List[float]]:
    """An image's per-channel mean and unbiased standard deviation on the [0, 1] scale (utils.py:32-33 after ``ToTensor``)
    from its six integer moments ``[(S1, S2)] * 3``.  Exact integers up to one correctly rounded quotient per value, and
    one correctly rounded square root for a standard deviation; a single pixel gives NaN as ``torch.std`` does."""
    p = int(h) * int(w)
    mean, std = [], []
    for s1, s2 in np.asarray(moments).reshape(3, 2).tolist():
        s1, s2 = int(s1), int(s2)
        mean.append(s1 / (255 * p))
        std.append(math.sqrt((p * s2 - s1 * s1) / (p * (p - 1) * 65025)) if p > 1 else math.nan)
    return mean, std


def pos_weight(class_counts: Sequence[int]) -> list:
    """utils.py:62-67: ``total / (3 * count)`` per class; None for a class without a pixel (the reference divides by zero)."""
    total = sum(int(c) for c in class_counts)
    return [total / (3 * int(c)) if int(c) > 0 else None for c in class_counts]


def report(items: List[dict], allrows) -> Tuple[List[List[str]], dict]:
    """CSV rows and the summary from the gathered ``ROW_WIDTH`` rows (any order: every dataset value is an exact integer
    sum or a ``math.fsum``)."""
    per_image, skipped = [], {r: [] for r in SKIP_REASONS.values()}
    class_counts, off_level, with_dual = [0, 0, 0], 0, 0
    csv_rows = []
    for r in sorted((np.asarray(r).tolist() for r in allrows), key=lambda r: r[0]):
        d = items[int(r[0])]
        h, w, status = int(r[1]), int(r[2]), int(r[3])
        mean, std = image_mean_std(h, w, r[4:10])
        per_image.append((mean, std))
        cells = ["", "", "", ""]
        if status == STATUS_OK:
            with_dual += 1
            for y in range(3):
                class_counts[y] += int(r[10 + y])
            off_level += int(r[13])
            cells = [str(int(v)) for v in r[10:14]]
        else:
            skipped[SKIP_REASONS[status]].append(d["wood"] + "/" + d["name"])
        csv_rows.append([d["name"], d["wood"], str(h), str(w)] + [repr(v) for v in mean + std] + cells)
    n = len(per_image)
    summary = {
        "mean": [math.fsum(m[c] for m, _ in per_image) / n for c in range(3)] if n else None,
        "std": [math.fsum(s[c] for _, s in per_image) / n for c in range(3)] if n else None,
        "class_counts": class_counts, "pos_weight": pos_weight(class_counts), "off_level_pixels": off_level,
        "images": n, "images_with_dual": with_dual, "skipped": skipped}
    return csv_rows, summary


def write_stats_csv(path: str, rows) -> None:
    with open(path, "w") as f:
        csv.writer(f, delimiter="\t").writerows([CSV_HEADER] + [list(r) for r in rows])


# ---- the folder driver -----------------------------------------------------------------------------------------------
def stats_folder(root: str, device_index: int = None, batch: int = None, window: int = 64, target_size: int = 1024,
                 streams: int = None) -> dict:
    """The statistics of the labelled folder ``root`` (module docstring); returns this rank's run statistics, with the
    summary and the gathered rows on rank 0.  ``batch``: frames of equal size per call (default 8); ``target_size`` only
    sizes the pinned staging, a larger frame re-pins its slot."""
    import torch
    r = folder_run.open_run(root, "stats", "fp32", device_index, 8 if batch is None else batch, streams, target_size)
    batch = r.batch
    folder_run.bring_up_without_model(r, lambda root: os.makedirs(os.path.join(root, "results"), exist_ok=True))

    items = list_labelled(root)
    sizes = folder_run.shard(r, items, lambda d: image_hw(d["src"]))
    mine = r.mine
    rows = np.zeros((len(mine), ROW_WIDTH), dtype=np.int64)

    def prepare(k):
        """Pool: the RGB frame and its grey dual; an all-zero mask (and the status that drops its counts) without a usable one."""
        gi = mine[k]
        d = items[gi]
        frame = _decode_rgb(d["src"])
        h, w = frame.shape[:2]
        status, grey = STATUS_OK, None
        if not os.path.isfile(d["dual"]):
            status = STATUS_NO_DUAL
        elif image_hw(d["dual"]) != (h, w):
            status = STATUS_SHAPE_MISMATCH
        else:
            grey = decode_dual(d["dual"])
            if grey.shape != (h, w):
                status, grey = STATUS_SHAPE_MISMATCH, None
        rows[k, :4] = (gi, h, w, status)
        return frame, np.zeros((h, w), dtype=np.uint8) if grey is None else grey

    mom_ring = [torch.empty((batch, 6), dtype=torch.int64).pin_memory() for _ in range(r.depth)]
    cnt_ring = [torch.empty((batch, 4), dtype=torch.int64).pin_memory() for _ in range(r.depth)]

    def launch(slot, sid, part, x, tgt):
        n = x.shape[0]
        mom_ring[slot][:n].copy_(image_moments(x).view(n, 6), non_blocking=True)       # utils.py:32-33
        cnt_ring[slot][:n].copy_(target_counts(tgt), non_blocking=True)               # utils.py:59-60

    def consume(slot, part, n, h, w):
        mom, cnt = mom_ring[slot][:n].numpy(), cnt_ring[slot][:n].numpy()
        for j, k in enumerate(part):
            rows[k, 4:10] = mom[j]
            if rows[k, 3] == STATUS_OK:
                rows[k, 10:14] = cnt[j]

    folder_run.run_loop(r, window, prepare, launch, consume, lambda: None, calibrate=False, bytes_per_pixel=(3, 1))
    if os.environ.get("NBC_FOLDER_PROFILE"):
        print("rank %d stage seconds: %s; loop wall %.2f s" % (
            r.rank, ", ".join("%s %.2f" % kv for kv in sorted(r.prof.items())), r.t_done - r.t_loop), flush=True)
    allrows = folder_run.gather(r, rows, ROW_WIDTH)
    summary = gathered = None
    if r.rank == 0:
        gathered = allrows.tolist()
        csv_rows, summary = report(items, allrows)
        write_stats_csv(os.path.join(root, STATS_CSV), csv_rows)
        with open(os.path.join(root, STATS_JSON), "w") as f:
            json.dump(summary, f, indent=1)
    return dict(folder_run.finish(r), summary=summary, rows=gathered)


def format_summary(summary: dict) -> str:
    lines = ["%d images, %d with a usable dual%s" % (
        summary["images"], summary["images_with_dual"],
        "".join("; %s: %s" % (k, ", ".join(v)) for k, v in summary["skipped"].items() if v))]
    if summary["mean"] is not None:
        lines.append("mean " + " ".join(repr(v) for v in summary["mean"]))
        lines.append("std  " + " ".join(repr(v) for v in summary["std"]))
    lines.append("class counts (nothing, bark, node) %s, %d pixels off the levels 0 / 127 / 255" % (
        summary["class_counts"], summary["off_level_pixels"]))
    lines.append("pos_weight " + " ".join("-" if v is None else repr(v) for v in summary["pos_weight"]))
    return "\n".join(lines)


def main(argv=None):
    import sys
    ap = argparse.ArgumentParser(description="MI355X dataset statistics of a labelled folder (samples/ + duals/): the mean / std "
                                             "and class weights of bark_calculator/utils.py, counted on the GPU")
    ap.add_argument("root_path", metavar="ROOT")
    ap.add_argument("--gpus", type=int, default=1, help="shard the folder over N GPUs of this node (one process each, RCCL)")
    ap.add_argument("--batch", type=int, default=None, help="frames of equal size per call (default 8)")
    ap.add_argument("--streams", type=int, default=None, help="batches in flight, each on its own HIP stream (default 4)")
    raw = list(sys.argv[1:] if argv is None else argv)
    args = ap.parse_args(raw)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, raw, module="neuralbarkcalculator_amd.stats"))
    idx = None if "WORLD_SIZE" in os.environ else 0
    stats = stats_folder(args.root_path, idx, batch=args.batch, streams=args.streams)
    if stats["rank"] == 0:
        print(format_summary(stats["summary"]))
        print("%(images_total)d images (%(images_this_rank)d on rank 0, %(batches)d batches): %(total_s).2f s, "
              "%(images_per_s_loop).1f images/s in the loop on this rank" % stats, flush=True)


if __name__ == "__main__":
    main()
