"""Evaluation of a checkpoint on a labelled folder: per-image IoU and F1, sharded over the GPUs of a node.

The counterpart of the reference's evaluation loop (/root/reference/src/bark_calculator/__main__.py:299-437) on the
accelerated path.  It answers what a choice of arithmetic mode or a retrained checkpoint costs in the metrics the model
was selected by.

* input: ``ROOT/samples/<wood_type>/<name>`` listed as ``predict.list_images`` lists them (dataset.py:41-68), each with its
  dual ``ROOT/duals/<wood_type>/<name.replace("bmp", "png")>`` (every ``bmp`` replaced, dataset.py:58), decoded with PIL
  ``convert('L')``;
* the network sees each sample as it is, through the uint8 ingest and the default mean / std of the predict driver: the
  reference's evaluation never runs the preprocessor, its labelled folder is already at model resolution.  Nothing is
  written under ``processed/``;
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

The machinery is the predict driver's: equal-shape batches, ``streams`` batches in flight on their own HIP streams and
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
from typing import List, Tuple

import numpy as np

from . import metrics
from .predict import (ARCH_CHOICES, BN_STATS, AbandonMarker, NonFiniteLogits, _decode_rgb, _host_workers, check_bn_stats_arch,
                      gather_rows, launch_ranks, list_images, resolve_arch_precision, resolve_bn_stats, shard_by_pixels)

ROW_WIDTH = 22                                   # (global_idx, H, W, status, conf_raw[9], conf_clean[9])
LOSS_ROW_WIDTH = 4                               # --loss: (global_idx, 3 float64 terms viewed as int64)
STATUS_OK, STATUS_NO_DUAL, STATUS_SHAPE_MISMATCH, STATUS_TOO_LARGE = 0, 1, 2, 3
SKIP_REASONS = {STATUS_NO_DUAL: "no_dual", STATUS_SHAPE_MISMATCH: "shape_mismatch", STATUS_TOO_LARGE: "too_large"}
STATS_CSV = os.path.join("results", "evaluation_stats.csv")
SUMMARY_JSON = os.path.join("results", "evaluation_summary.json")


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


def csv_header(loss: bool = False) -> List[str]:
    return metrics.EVAL_CSV_HEADER + (metrics.LOSS_CSV_COLUMNS if loss else [])


def write_stats_csv(path: str, rows, loss: bool = False) -> None:
    with open(path, "w") as f:                   # __main__.py:433-437
        csv.writer(f, delimiter="\t").writerows([csv_header(loss)] + [list(r) for r in rows])


def report(items: List[dict], allrows: np.ndarray, precision: str, model_path: str,
           bn_stats: str = "running", loss_rows: np.ndarray = None) -> Tuple[List[List[str]], dict]:
    """CSV rows and summary from the gathered rank rows (rank 0); ``loss_rows``: the gathered ``LOSS_ROW_WIDTH`` rows of
    ``--loss`` (None without it)."""
    terms = None
    if loss_rows is not None:
        terms = {int(r[0]): np.ascontiguousarray(r[1:]).view(np.float64) for r in loss_rows}
    rows, skipped = [], {r: [] for r in SKIP_REASONS.values()}
    raw_total, clean_total = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64)
    for r in allrows:
        d = items[int(r[0])]
        if int(r[3]) != STATUS_OK:
            skipped[SKIP_REASONS[int(r[3])]].append(d["wood"] + "/" + d["name"])
            continue
        raw, clean = r[4:13].reshape(3, 3), r[13:22].reshape(3, 3)
        raw_total += raw
        clean_total += clean
        row = metrics.eval_row(d["name"], d["wood"], raw, clean)
        if terms is not None:                    # a class is present where its target row of the confusion is not empty
            row += metrics.loss_cells(terms[int(r[0])], raw.sum(axis=1))
        rows.append(row)
    summary = {"precision": precision, "bn_statistics": bn_stats, "model_path": model_path, "images_evaluated": len(rows),
               "images_skipped": sum(len(v) for v in skipped.values()), "skipped": skipped}
    if rows:
        summary.update(metrics.summarize(rows, raw_total, clean_total))
    if terms is not None:
        summary["lovasz_softmax"] = metrics.summarize_loss(rows, len(metrics.EVAL_CSV_HEADER))
    return rows, summary


def evaluate_folder(root: str, model_path: str = "./best_model.pt", precision: str = "fp32", device_index: int = None,
                    batch: int = None, window: int = 64, target_size: int = 1024, calibrate: bool = True,
                    streams: int = None, arch: str = "auto", bn_stats: str = "running", precision_auto: bool = False,
                    loss: bool = False) -> dict:
    """Evaluate the checkpoint on the labelled folder ``root`` (module docstring); returns this rank's statistics, with
    the summary on rank 0.  ``arch``: the network (``predict.resolve_arch``; ``"auto"`` = the one the checkpoint's keys
    name).  ``bn_stats``: ``"running"`` (eval mode) or ``"image"``, the shipped tool's per-image BatchNorm statistics
    ("fp32", FCN only; ``predict.resolve_bn_stats``).  ``loss``: also the per-image Lovasz-Softmax loss (module
    docstring).  Raises ``NonFiniteLogits`` on every rank alike when f16x2 cannot carry the weights."""
    import sys
    import time
    from collections import defaultdict, deque
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from .model import MODELS, FCNResNet50
    from .predict import check_bn_stats_arch, resolve_arch, resolve_arch_precision
    t_start = time.perf_counter()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if device_index is None else device_index
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if batch is None:
        batch = 8 if precision == "bf16" else 2
    n_streams = 4 if streams is None else max(1, int(streams))

    marker = AbandonMarker(root)
    if rank == 0:
        os.makedirs(os.path.join(root, "results"), exist_ok=True)
        marker.clear()
    if dist is not None:
        dist.barrier()
    state_dict = None
    if rank == 0:                                    # only one rank touches the checkpoint
        state_dict = torch.load(model_path, map_location="cpu", weights_only=True)
    arch = resolve_arch(arch, state_dict, dist, dev)
    check_bn_stats_arch(bn_stats, arch)
    precision = resolve_arch_precision(arch, precision, precision_auto)   # EfficientNet: fp32
    model = MODELS[arch](precision).set_bn_statistics(bn_stats).to(dev)
    if rank == 0:
        model.load_state_dict(state_dict)
    del state_dict
    if dist is not None:
        model.broadcast_weights(src=0)
    if precision == "f16x2" and model.pack_flags:
        err = NonFiniteLogits("the packed weights carry NBC_PACK flags %d: f16x2 would not be f32 grade on this checkpoint; "
                              "rerun with --precision fp32" % model.pack_flags)
        err.batches_run, err.images_this_rank = 0, 0
        raise err
    models = [model] + [model.clone_shared() for _ in range(n_streams - 1)]
    gpu_streams = [torch.cuda.Stream(dev) for _ in range(n_streams)]
    for m in models:                                 # the largest workspaces once (a context's buffers only grow)
        m.reserve(batch, target_size, target_size)
        m.remove_small_zones(torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev))
        if loss:                                     # and the loss workspace
            m.lovasz_softmax(torch.zeros((batch, 3, target_size, target_size), dtype=torch.float32, device=dev),
                             torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize(dev)
    t_ready = time.perf_counter()

    items = list_labelled(root)
    n_total = len(items)
    workers = _host_workers()
    pool = ThreadPoolExecutor(max_workers=workers)
    sizes = list(pool.map(lambda d: image_hw(d["src"]), items))
    shards = shard_by_pixels([h * w for h, w in sizes], world)
    mine = shards[rank]
    rows = np.zeros((len(mine), ROW_WIDTH), dtype=np.int64)
    loss_rows = np.zeros((len(mine), LOSS_ROW_WIDTH), dtype=np.int64) if loss else None
    if loss:
        loss_rows[:, 0] = mine

    def prepare(k):
        """Pool: status, and for an image that can be evaluated the RGB frame and the grey dual."""
        gi = mine[k]
        h, w = sizes[gi]
        status = dual_status(items[gi], h, w, target_size)
        if status != STATUS_OK:
            return status, None, None
        frame, grey = _decode_rgb(items[gi]["src"]), decode_dual(items[gi]["dual"])
        if grey.shape != frame.shape[:2]:
            return STATUS_SHAPE_MISMATCH, None, None
        return STATUS_OK, frame, grey

    depth = n_streams + 1
    full = batch * target_size * target_size
    stage = [{"x": torch.empty(full * 3, dtype=torch.uint8).pin_memory(), "t": torch.empty(full, dtype=torch.uint8).pin_memory(),
              "ev": torch.cuda.Event()} for _ in range(depth)]
    ring = [torch.empty((2, batch, 3, 3), dtype=torch.int64).pin_memory() for _ in range(depth)]   # raw, clean
    ring_ev = [torch.cuda.Event() for _ in range(depth)]
    loss_ring = [torch.empty((batch, 3), dtype=torch.float64).pin_memory() for _ in range(depth)] if loss else None
    logits_buf = [torch.empty(batch * 3 * target_size * target_size, dtype=torch.float32, device=dev)
                  for _ in range(n_streams)] if loss else None
    flag_host = torch.zeros(depth, dtype=torch.int32).pin_memory()
    check_flag = precision == "f16x2"
    bad_seen = [False]
    pending = deque()                                # (slot, [k], n), oldest first
    n_batches = 0

    def consume(p):
        slot, ks, n = p
        ring_ev[slot].synchronize()
        if check_flag and int(flag_host[slot]) != 0:
            bad_seen[0] = True                       # this batch's counts (and every later one's) are not valid
            if world > 1:
                marker.set()
            return
        conf = ring[slot][:, :n].numpy().reshape(2, n, 9)
        for j, k in enumerate(ks):
            h, w = sizes[mine[k]]
            rows[k, :4] = (mine[k], h, w, STATUS_OK)
            rows[k, 4:13], rows[k, 13:] = conf[0, j], conf[1, j]
            if loss:
                loss_rows[k, 1:] = loss_ring[slot][j].numpy().view(np.int64)

    # f16x2 calibration guard (predict.predict_folder): rank 0 runs its first image that fits once with every activation kept
    if check_flag and calibrate:
        verdict = torch.zeros(1, dtype=torch.int32)
        offenders = {}
        first = next((gi for gi in mine if max(sizes[gi]) <= target_size), None)
        if rank == 0 and first is not None:
            frame = _decode_rgb(items[first]["src"])
            peaks = models[0].activation_peaks(torch.from_numpy(np.ascontiguousarray(frame[None])).to(dev))
            ok, offenders = FCNResNet50.f16x2_range_ok(peaks)
            verdict[0] = 0 if ok else 1
        if dist is not None:
            vd = verdict.to(dev) if dist.get_backend() == "nccl" else verdict
            dist.broadcast(vd, src=0)
            verdict = vd.cpu()
        if int(verdict[0]) != 0:
            pool.shutdown(wait=True, cancel_futures=True)
            worst = ", ".join("%s %.3g" % kv for kv in sorted(offenders.items(), key=lambda kv: kv[1])[:4])
            err = NonFiniteLogits("calibration on the first image: an activation tensor lies outside the range the f16 pieces hold "
                                  "at f32 grade%s; rerun with --precision fp32" % ((" (" + worst + ")") if worst else ""))
            err.batches_run, err.images_this_rank = 0, len(mine)
            raise err

    switch = sys.getswitchinterval()
    sys.setswitchinterval(2e-4)                      # the GPU loop shares the interpreter with the pool (predict_folder)
    try:
        windows = [list(range(a, min(a + window, len(mine)))) for a in range(0, len(mine), window)]
        futs = {k: pool.submit(prepare, k) for k in (windows[0] if windows else [])}
        t_loop = time.perf_counter()
        for wi, win in enumerate(windows):
            if check_flag and world > 1 and not bad_seen[0] and marker.is_set():
                bad_seen[0] = True
            if bad_seen[0]:
                break
            if wi + 1 < len(windows):
                for k in windows[wi + 1]:
                    futs[k] = pool.submit(prepare, k)
            got = {k: futs.pop(k).result() for k in win}
            groups = defaultdict(list)
            for k, (status, frame, _) in got.items():
                if status != STATUS_OK:
                    h, w = sizes[mine[k]]
                    rows[k, :4] = (mine[k], h, w, status)
                else:
                    groups[frame.shape].append(k)
            for shape, ks in sorted(groups.items()):
                for a in range(0, len(ks), batch):
                    if bad_seen[0]:
                        break
                    part = ks[a:a + batch]
                    n, (h, w) = len(part), shape[:2]
                    slot, sid = n_batches % depth, n_batches % n_streams
                    mdl, st = models[sid], stage[slot]
                    st["ev"].synchronize()                    # the copies that last read these buffers have finished
                    xb = st["x"][: n * h * w * 3].view(n, h, w, 3)
                    tb = st["t"][: n * h * w].view(n, h, w)
                    xnp, tnp = xb.numpy(), tb.numpy()
                    for j, k in enumerate(part):
                        xnp[j] = got[k][1]
                        tnp[j] = got[k][2]
                    with torch.cuda.stream(gpu_streams[sid]):
                        x = xb.to(dev, non_blocking=True)     # uint8 NHWC; normalised on the device
                        tgt = tb.to(dev, non_blocking=True)
                        st["ev"].record()
                        lg = logits_buf[sid][: n * 3 * h * w].view(n, 3, h, w) if loss else None
                        labels, _ = mdl.predict_labels(x, labels_dtype=torch.uint8, logits_full=lg)   # __main__.py:323
                        conf_raw = mdl.confusion(labels, tgt)                         # iou: the raw argmax (:331)
                        if loss:                                                      # LovaszSoftmax (:236-239)
                            terms, _ = mdl.lovasz_softmax(lg, tgt)
                            loss_ring[slot][:n].copy_(terms, non_blocking=True)
                        mdl.remove_small_zones(labels)                                # PixelWiseF1 (utils.py:213)
                        conf_clean = mdl.confusion(labels, tgt)
                        ring[slot][0, :n].copy_(conf_raw, non_blocking=True)
                        ring[slot][1, :n].copy_(conf_clean, non_blocking=True)
                        if check_flag:
                            mdl.nonfinite_peek_async(flag_host[slot:slot + 1])
                        ring_ev[slot].record()
                    pending.append((slot, part, n))
                    while len(pending) > n_streams:
                        consume(pending.popleft())
                    n_batches += 1
            got.clear()
        while pending:
            consume(pending.popleft())
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
        sys.setswitchinterval(switch)
    torch.cuda.synchronize()
    t_done = time.perf_counter()
    if precision == "f16x2":                         # as predict_folder: every rank learns of it before the row gather
        bad = any([m.nonfinite_seen() for m in models]) or bad_seen[0]
        if dist is not None:
            flag = torch.tensor([int(bad)], dtype=torch.int32, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            bad = bool(int(flag.item()))
            if rank == 0:
                marker.clear()
        if bad:
            err = NonFiniteLogits("a forward produced non-finite logits in f16x2 mode: the evaluation was abandoned; rerun with "
                                  "--precision fp32")
            err.batches_run, err.images_this_rank = n_batches, len(mine)
            raise err

    cap = max(len(s) for s in shards) if shards else 0
    gather_dev = dev if dist is not None and dist.get_backend() == "nccl" else None
    allrows = gather_rows(rows, n_total, world, dist, gather_dev, cap=cap, width=ROW_WIDTH)
    all_loss = gather_rows(loss_rows, n_total, world, dist, gather_dev, cap=cap, width=LOSS_ROW_WIDTH) if loss else None
    summary = gathered = None
    if rank == 0:
        gathered = allrows.tolist()
        csv_rows, summary = report(items, allrows, precision, model_path, bn_stats, loss_rows=all_loss)
        write_stats_csv(os.path.join(root, STATS_CSV), csv_rows, loss=loss)
        with open(os.path.join(root, SUMMARY_JSON), "w") as f:
            json.dump(summary, f, indent=1)
    if dist is not None:
        dist.barrier()
    t_end = time.perf_counter()
    n_eval = int(sum(1 for k in range(len(mine)) if rows[k, 3] == STATUS_OK))
    out = {"rank": rank, "world": world, "images_total": n_total, "images_this_rank": len(mine),
           "images_evaluated_this_rank": n_eval, "batches": n_batches, "batch": batch, "streams": n_streams,
           "setup_s": t_ready - t_start, "loop_s": t_done - t_loop, "total_s": t_end - t_start,
           "images_per_s_loop": len(mine) / max(t_done - t_loop, 1e-9), "summary": summary, "rows": gathered}
    if loss:                                     # rank 0: {global_idx: float64 [3] terms}
        out["loss_terms"] = None if all_loss is None or rank != 0 else {
            int(r[0]): np.ascontiguousarray(r[1:]).view(np.float64).copy() for r in all_loss}
    return out


def format_summary(summary: dict) -> str:
    lines = ["evaluated %d images in %s%s (checkpoint %s), skipped %d%s" % (
        summary["images_evaluated"], summary["precision"],
        ", per-image BatchNorm statistics" if summary.get("bn_statistics") == "image" else "", summary["model_path"],
        summary["images_skipped"],
        "".join("; %s: %s" % (r, ", ".join(v)) for r, v in summary["skipped"].items() if v))]
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
    return "\n".join(lines)


def main(argv=None):
    import sys
    ap = argparse.ArgumentParser(description="MI355X evaluation of a checkpoint on a labelled folder (samples/ + duals/): "
                                             "per-image IoU and F1 like bark_calculator/__main__.py")
    ap.add_argument("root_path", metavar="ROOT")
    ap.add_argument("--model_path", default="./best_model.pt")
    ap.add_argument("--precision", choices=["auto", "fp32", "f16x2", "bf16"], default="auto",
                    help="auto (default): f16x2, and a second run in fp32 if the weights leave that mode's range; see predict")
    ap.add_argument("--gpus", type=int, default=1, help="shard the folder over N GPUs of this node (one process each, RCCL)")
    ap.add_argument("--batch", type=int, default=None, help="frames of equal size per forward (default 2, 8 in bf16)")
    ap.add_argument("--streams", type=int, default=None, help="batches in flight, each on its own HIP stream (default 4)")
    ap.add_argument("--arch", choices=["auto"] + list(ARCH_CHOICES), default="auto",
                    help="the network of the checkpoint; auto (default): the one whose state_dict keys it holds")
    ap.add_argument("--bn_stats", choices=list(BN_STATS), default="running",
                    help="running (default): BatchNorm on the running statistics (eval mode); image: each image's own statistics, "
                         "as the shipped tool ran them (fp32, FCN-ResNet-50 only; --precision auto then means fp32)")
    ap.add_argument("--loss", action="store_true",
                    help="also the per-image Lovasz-Softmax loss, the training objective (four more CSV columns, computed on the GPU)")
    ap.add_argument("--exclude_nodes", action="store_true", help=argparse.SUPPRESS)
    raw = list(sys.argv[1:] if argv is None else argv)
    args = ap.parse_args(raw)
    try:
        args.precision = resolve_bn_stats(args.bn_stats, args.precision)
        if args.arch != "auto":
            check_bn_stats_arch(args.bn_stats, args.arch)
        args.precision = resolve_arch_precision(args.arch, args.precision)
    except ValueError as e:
        ap.error(str(e))
    if args.exclude_nodes:
        raise SystemExit("evaluate: --exclude_nodes is not supported: IoU and F1 are defined on the three classes "
                         "(nothing, bark, node) of the duals")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, raw, module="neuralbarkcalculator_amd.evaluate"))
    idx = None if "WORLD_SIZE" in os.environ else 0
    kw = dict(batch=args.batch, streams=args.streams, arch=args.arch, bn_stats=args.bn_stats)
    if args.loss:
        kw["loss"] = True
    if args.precision == "auto":
        stats = None
        try:
            stats = evaluate_folder(args.root_path, args.model_path, "f16x2", idx, precision_auto=True, **kw)
        except NonFiniteLogits as e:                 # raised on every rank alike
            if int(os.environ.get("RANK", "0")) == 0:
                print("evaluate: %s -- evaluating the folder again on the f32 MFMA" % e, flush=True)
        if stats is None:
            import gc
            import torch
            gc.collect()
            torch.cuda.empty_cache()
            stats = evaluate_folder(args.root_path, args.model_path, "fp32", idx, **kw)
    else:
        stats = evaluate_folder(args.root_path, args.model_path, args.precision, idx, **kw)
    if stats["rank"] == 0:
        print(format_summary(stats["summary"]))
        print("%(images_total)d images (%(images_this_rank)d on rank 0, %(batches)d batches): %(total_s).2f s, "
              "%(images_per_s_loop).1f images/s in the loop on this rank" % stats, flush=True)


if __name__ == "__main__":
    main()
