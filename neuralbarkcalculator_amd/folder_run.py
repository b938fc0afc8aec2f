"""The folder-run engine under the predict and evaluate drivers: everything that must be the same on every rank and in
both tools, written once.

A driver (``predict.predict_folder``, ``evaluate.evaluate_folder``) calls, in this order:

* ``open_run``: the rank context (rank, world, ``dist`` or None, device, the batch and stream defaults);
* ``bring_up``: rank 0's folders and the start barrier, the checkpoint on rank 0 alone, architecture (one broadcast under
  ``--arch auto``) and precision, the weight broadcast, the ``pack_flags`` refusal, one model object and side stream per
  batch in flight, the ingest's mean / std on every one of them (``normalization``), the largest workspaces once (``warm``:
  the driver's own); ``bring_up_without_model`` for a driver that runs no network (``stats``);
* ``shard``: the host pool and this rank's contiguous, pixel-balanced share of the driver's item list;
* ``run_loop``: the f16x2 calibration guard (one verdict broadcast), the batch loop, and the non-finite settlement (one MAX
  all-reduce in f16x2).  The driver supplies ``prepare(k)`` (pool: the arrays of local image k, or None to skip it),
  ``launch`` (the device work of one batch, on its stream) and ``consume`` (one finished slot, on the host);
* ``gather`` (once per row kind) and ``finish`` (the final barrier and the statistics every driver returns).

No collective sits in the per-image path: ranks with different numbers of windows tell each other of an abandoned f16x2
run through ``AbandonMarker``.  ``run_precision``, ``add_shared_arguments``, ``resolve_arguments`` and
``resolve_normalization`` are the predict and evaluate drivers' shared command-line tail.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import List, Sequence

import numpy as np


class NonFiniteLogits(RuntimeError):
    """A forward produced NaN / infinite logits: in f16x2 mode an activation beyond f16's range (or NaN/inf weights) -- or the
    packer reported weights the f16 pieces cannot carry at f32 grade (``FCNResNet50.pack_flags``), before any forward ran."""

    def __init__(self, text: str, batches_run: int = 0, images_this_rank: int = 0):
        super().__init__(text)
        self.batches_run, self.images_this_rank = batches_run, images_this_rank


class AbandonMarker:
    """How the ranks of one node tell each other that an f16x2 run is being abandoned: a file under ``results/`` that the
    rank that sees the non-finite word creates and every rank looks for once per window of images (``os.path.exists``: no
    collective, so ranks with different numbers of windows cannot wait for each other).  The folder driver's ranks share a
    node (``--gpus N`` starts them on this one) and the folder's file system with it.  Rank 0 clears a stale marker before
    the start barrier and the final one after the flag all-reduce."""

    def __init__(self, root: str):
        self.path = os.path.join(root, "results", ".f16x2_abandoned")

    def set(self):
        try:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            open(self.path, "w").close()
        except OSError:
            pass                                         # the flag all-reduce at the end still tells every rank

    def is_set(self) -> bool:
        return os.path.exists(self.path)

    def clear(self):
        try:
            os.remove(self.path)
        except OSError:
            pass


def _host_workers() -> int:
    return max(1, min(32, int(os.environ.get("NBC_HOST_WORKERS", "16"))))


def shard_indices(n: int, rank: int, world: int) -> List[int]:
    """Round-robin shard: images r, r+W, r+2W, ... (frames of equal size: bench.py)."""
    return list(range(rank, n, world))


def shard_by_pixels(pixels: Sequence[int], world: int) -> List[List[int]]:
    """Contiguous, pixel-balanced shards of the sorted image list (folders of height-trimmed
    or differently sized scans): image i goes to the rank whose share of the total pixel count contains the
    midpoint of i's own span.  Every rank gets a contiguous range; ranges are empty only when there are
    fewer images than ranks."""
    total = float(sum(pixels))
    shards: List[List[int]] = [[] for _ in range(world)]
    acc = 0.0
    for i, p in enumerate(pixels):
        mid = acc + 0.5 * p
        r = min(world - 1, int(mid * world / total)) if total > 0 else i % world
        shards[r].append(i)
        acc += p
    return shards


def shard_by_units(pixels: Sequence[int], unit_of: Sequence[int], world: int) -> List[List[int]]:
    """``shard_by_pixels`` in units that must not be cut: ``unit_of[i]`` is the unit of image i, non-decreasing along the list.
    The units are balanced by their summed pixels; every rank gets a contiguous range of whole units."""
    if len(pixels) != len(unit_of) or any(b < a for a, b in zip(unit_of, unit_of[1:])):
        raise ValueError("one unit per image, non-decreasing along the list")
    members = {}
    for i, u in enumerate(unit_of):
        members.setdefault(u, []).append(i)
    order = sorted(members)
    shards: List[List[int]] = [[] for _ in range(world)]
    for rank, units in enumerate(shard_by_pixels([sum(pixels[i] for i in members[u]) for u in order], world)):
        for j in units:
            shards[rank].extend(members[order[j]])
    return shards


def windows(n: int, window: int) -> List[List[int]]:
    """The local images 0..n-1 in windows of ``window``, in order: the pool works one window ahead of the GPU."""
    return [list(range(a, min(a + window, n))) for a in range(0, n, window)]


def batches_of(win: Sequence[int], shapes: dict, batch: int) -> List[tuple]:
    """The batches of one window, in the order they run: ``(shape, [k, ...])`` with the window's images grouped by frame
    shape (``shapes[k]``; None: image k is skipped), shapes in sorted order, each group cut into runs of up to ``batch``."""
    groups = {}
    for k in win:
        if shapes[k] is not None:
            groups.setdefault(shapes[k], []).append(k)
    return [(shape, ks[a:a + batch]) for shape, ks in sorted(groups.items()) for a in range(0, len(ks), batch)]


def collective_device(dist, device):
    """Where a collective's tensors live: RCCL takes device tensors (``device``); a gloo group (one-GPU rehearsals of the
    multi-rank path) and a single rank take host tensors (None)."""
    return device if dist is not None and dist.get_backend() == "nccl" else None


def _on_wire(t, wire_dev):
    return t if wire_dev is None else t.to(wire_dev)


def gather_rows(local_rows: np.ndarray, n_total: int, world: int, dist=None, device=None, cap: int = None,
                width: int = 5) -> np.ndarray:
    """all_gather of fixed-size per-rank row buffers; returns the rows sorted by global index.
    ``local_rows``: int64 [k, width] with k <= ``cap`` (default ceil(n_total / world), the round-robin
    bound; pixel-balanced shards pass the largest shard's size)."""
    import torch
    if cap is None:
        cap = (n_total + world - 1) // world if n_total else 0
    buf = torch.full((max(cap, 1), width), -1, dtype=torch.int64)
    if len(local_rows):
        buf[: len(local_rows)] = torch.from_numpy(np.asarray(local_rows, dtype=np.int64))
    if dist is None or world == 1:
        allrows = buf
    else:
        if device is not None:
            buf = buf.to(device)
        parts = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(parts, buf)
        allrows = torch.cat(parts).cpu()
    allrows = allrows.numpy()
    allrows = allrows[allrows[:, 0] >= 0]
    return allrows[np.argsort(allrows[:, 0], kind="stable")]


def gather_ragged(local_rows: np.ndarray, world: int, dist=None, device=None, width: int = 5) -> np.ndarray:
    """``gather_rows`` for row sets whose per-rank length no rank can predict (several rows per image, or none, as the zone
    rows of ``predict --zones``): one extra all_reduce of the largest per-rank count gives every rank the same ``cap``.  The
    rows come back sorted by their first column, the global image index; the rows of one image keep their order."""
    cap = len(local_rows)
    if dist is not None and world > 1:
        import torch
        t = _on_wire(torch.tensor([cap], dtype=torch.int64), device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        cap = int(t.cpu()[0])
    return gather_rows(np.asarray(local_rows, dtype=np.int64).reshape(-1, width), 0, world, dist, device, cap=cap, width=width)


def resolve_arch(arch: str, state_dict=None, dist=None, device=None) -> str:
    """The network a folder driver runs (``--arch``).  ``"auto"``: rank 0, the one rank that read the checkpoint, picks
    the architecture whose key set ``state_dict`` matches (``model.arch_of_state_dict``) and broadcasts its NBC_ARCH_*
    index, so that every other rank sizes its blob for it.  A checkpoint no architecture matches raises on every rank
    alike (rank 0 with the strict-load message of fcn_resnet50).  A named architecture is taken as it stands: strict
    loading then refuses a checkpoint of the other one."""
    from . import topology
    if arch != "auto":
        return topology.arch_name(topology.arch_index(arch))
    rank = dist.get_rank() if dist is not None else 0
    code, err = -1, None
    if rank == 0:
        from .model import arch_of_state_dict
        try:
            code = topology.arch_index(arch_of_state_dict(state_dict))
        except RuntimeError as e:
            err = e
    if dist is not None:
        import torch
        t = _on_wire(torch.tensor([code], dtype=torch.int32), collective_device(dist, device))
        dist.broadcast(t, src=0)
        code = int(t.cpu()[0])
    if err is not None:
        raise err
    if code < 0:
        raise RuntimeError("rank 0 found no architecture matching the checkpoint's keys")
    return topology.arch_name(code)


def resolve_arch_precision(arch: str, precision: str, precision_auto: bool = False) -> str:
    """The precision a folder driver runs ``arch`` in.  EfficientNet networks run "fp32" only: ``--precision auto`` means
    "fp32" for them (``precision_auto``: the precision came from auto), an explicit "f16x2" or "bf16" raises ``ValueError``
    naming fp32.  Every other network keeps ``precision``.  Called with the architecture ``resolve_arch`` returned (every
    rank alike), or at argument time with a named one."""
    from . import topology
    if arch == "auto" or not topology.is_efficientnet(arch) or precision in ("fp32", "auto"):
        return "fp32" if arch != "auto" and topology.is_efficientnet(arch) else precision
    if precision_auto:
        return "fp32"
    raise ValueError("%s runs in --precision fp32 (or auto) only, not %s: swish and the SE gate are not positively "
                     "homogeneous, so f16x2's powers of two cannot be folded into its BatchNorm pairs" % (arch, precision))


BN_STATS = ("running", "image", "image_f16x2")
ARCH_CHOICES = ("fcn_resnet50", "deeplabv3_resnet50") + tuple("fcn_efficientnet_b%d" % n for n in range(8)) + \
    tuple("deeplabv3_efficientnet_b%d" % n for n in range(8))


def resolve_bn_stats(bn_stats: str, precision: str) -> str:
    """The precision a folder driver runs with ``--bn_stats`` (``FCNResNet50.set_bn_statistics``).  ``"running"`` leaves
    ``precision`` as it is.  ``"image"`` (the shipped tool's per-image BatchNorm statistics) runs the f32 MFMA only:
    ``"auto"`` means ``"fp32"`` (no f16x2 run, no calibration), ``"f16x2"`` and ``"bf16"`` raise ``ValueError``.
    ``"image_f16x2"`` is the same statistics on the f16x2 pipe: ``"f16x2"`` runs it, ``"auto"`` stays ``"auto"`` (f16x2
    under its guards, and ``--bn_stats image`` in fp32 when one of them speaks: ``run_precision``), ``"fp32"`` and ``"bf16"``
    raise ``ValueError``."""
    if bn_stats not in BN_STATS:
        raise ValueError("--bn_stats must be one of %s, got %r" % (", ".join(BN_STATS), bn_stats))
    if bn_stats == "running":
        return precision
    if bn_stats == "image_f16x2":
        if precision in ("auto", "f16x2"):
            return precision
        raise ValueError("--bn_stats image_f16x2 runs in --precision f16x2 (or auto) only, not %s: --bn_stats image is the "
                         "fp32 mode" % precision)
    if precision in ("auto", "fp32"):
        return "fp32"
    raise ValueError("--bn_stats image runs in --precision fp32 (or auto) only, not %s: the f16x2 form of the mode is "
                     "--bn_stats image_f16x2, and bf16 rounds raw pre-BatchNorm values too coarsely for the mean "
                     "subtraction" % precision)


def check_bn_stats_arch(bn_stats: str, arch: str) -> None:
    """``ValueError`` for ``--bn_stats image`` (or ``image_f16x2``) on a network other than FCN-ResNet-50.  Called with the architecture
    ``resolve_arch`` returned, which every rank holds alike, so every rank refuses alike."""
    from . import topology
    image = bn_stats in ("image", "image_f16x2")
    if image and topology.is_efficientnet(arch):
        raise ValueError("--bn_stats image is refused for %s: per-image BatchNorm statistics are implemented for fcn_resnet50 "
                         "only" % arch)
    if image and arch != "fcn_resnet50":
        raise ValueError("--bn_stats image is refused for %s: its ASPP pooling branch's BatchNorm sees a [1, 256, 1, 1] tensor, "
                         "which batch statistics cannot normalise (torch raises, and so would the reference)" % arch)


# ---- the shipped tool's live Dropout (--dropout_draws): identities, argument checks, the report -----------------------
DROPOUT_MAX_DRAWS = 1024
DROPOUT_COLUMNS = ["Name", "Type", "Output Bark %", "Output Node %", "bark_mean", "bark_std", "bark_min", "bark_max",
                   "node_mean", "node_std", "node_min", "node_max", "draws"]
DROPOUT_COMPARE_COLUMNS = ["old_bark", "old_node", "bark_inside", "node_inside", "bark_z", "node_z"]
VOTE_COLUMNS = ["Name", "Type", "draws", "Vote Bark %", "Vote Node %", "unanimous %", "mean_support", "changed_pixels"]
VOTE_STATS = 10                                      # NBC_VOTE_STATS of include/nbc.h


def image_id(wood: str, name: str) -> int:
    """The 64-bit identity of a folder image for ``FCNResNet50.dropout_draws``: FNV-1a-64 (offset 0xcbf29ce484222325, prime
    0x100000001b3) of the UTF-8 bytes of ``wood + "/" + name``.  An image's draws therefore depend neither on what else is in
    the folder, nor on batch, streams or ranks."""
    h = 0xcbf29ce484222325
    for b in (wood + "/" + name).encode("utf-8"):
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def check_dropout_arguments(draws, p=None, seed=None, compare=None, arch: str = "auto", only_preprocess: bool = False,
                            votes: bool = False) -> None:
    """``ValueError`` for what ``--dropout_draws`` and its companions refuse before any device is touched.  ``draws``: None =
    the flag is off, and then ``p``, ``seed`` and ``compare`` must be None and ``votes`` (``--dropout_votes``) false too.  On:
    ``draws`` in 1..1024, ``p`` in [0, 1), ``seed`` an unsigned 64-bit integer, a named ``arch`` fcn_resnet50 (``check_dropout_arch`` once ``"auto"`` is resolved),
    and not ``only_preprocess``."""
    if draws is None:
        given = [n for n, v in (("--dropout_p", p), ("--dropout_seed", seed), ("--dropout_compare", compare)) if v is not None]
        if votes:
            given.append("--dropout_votes")
        if given:
            raise ValueError("%s needs --dropout_draws" % ", ".join(given))
        return
    if not 1 <= int(draws) <= DROPOUT_MAX_DRAWS:
        raise ValueError("--dropout_draws must lie in 1..%d, got %r" % (DROPOUT_MAX_DRAWS, draws))
    if p is not None and not (0.0 <= float(p) < 1.0):
        raise ValueError("--dropout_p must lie in [0, 1), got %r" % (p,))
    if seed is not None and not 0 <= int(seed) < 2 ** 64:
        raise ValueError("--dropout_seed must be an unsigned 64-bit integer, got %r" % (seed,))
    if only_preprocess:
        raise ValueError("--dropout_draws runs the network: it cannot go with --only_preprocess")
    if arch != "auto":
        check_dropout_arch(arch)


ZONES_MAX_CAP = 65536


def check_zones_arguments(zones: bool, zones_cap=None, only_preprocess: bool = False) -> None:
    """``ValueError`` for what ``--zones`` and ``--zones_cap`` refuse before any device is touched: a cap without the flag, the
    flag with ``--only_preprocess`` (there is no label map to inventory), a cap outside 1..65536."""
    if not zones:
        if zones_cap is not None:
            raise ValueError("--zones_cap needs --zones")
        return
    if only_preprocess:
        raise ValueError("--zones inventories the label maps: it is refused with --only_preprocess")
    if zones_cap is not None and not 1 <= int(zones_cap) <= ZONES_MAX_CAP:
        raise ValueError("--zones_cap must lie in 1..%d" % ZONES_MAX_CAP)


def check_dropout_arch(arch: str) -> None:
    """``ValueError`` for ``--dropout_draws`` on a network other than FCN-ResNet-50 (every rank holds the resolved architecture
    alike, so every rank refuses alike)."""
    from . import topology
    if topology.is_efficientnet(arch):
        raise ValueError("--dropout_draws is refused for %s: EfficientNet's FCN head is left out" % arch)
    if arch != "fcn_resnet50":
        raise ValueError("--dropout_draws is refused for %s: DeepLabHead's Dropout sits inside ASPP" % arch)


def percent_string(count: int, pixels: int) -> str:
    """A class percentage as ``final_stats.csv`` prints it: float32 arithmetic and '{:.5f}' (models.py:321-332)."""
    return "{:.5f}".format(float(np.float32(count) / np.float32(pixels) * np.float32(100)))


def draw_statistics(counts: Sequence[int], pixels: int) -> dict:
    """mean, unbiased std (None for one draw), min and max of the percentages ``100 * count / pixels`` of one class over the
    draws, from the integer counts: sums and the variance's numerator are exact integers, each figure one correctly rounded
    division (and one square root) away from them."""
    import math
    cs = [int(c) for c in counts]
    d, s1, s2 = len(cs), sum(cs), sum(c * c for c in cs)
    out = {"mean": (100 * s1) / (d * pixels), "min": (100 * min(cs)) / pixels, "max": (100 * max(cs)) / pixels, "std": None}
    if d > 1:
        out["std"] = math.sqrt((10000 * (d * s2 - s1 * s1)) / (d * (d - 1) * pixels * pixels))
    return out


def read_shipped_stats(path: str) -> dict:
    """``{(name, type): (bark %, node %)}`` of a ``final_stats.csv`` as the shipped tool writes it: tab separated, seven header
    names over SIX columns per row (models.py:252-255 against :321-332), so rows are read by position -- name, type, bark %
    at 2, node % at 4.  ``ValueError`` for a file that cannot be read that way."""
    import csv
    old = {}
    try:
        with open(path, newline="") as f:
            for i, row in enumerate(csv.reader(f, delimiter="\t")):
                if i == 0 or not row:
                    continue
                if len(row) < 5:
                    raise ValueError("row %d has %d columns, not the six of the shipped tool" % (i + 1, len(row)))
                old[(row[0], row[1])] = (float(row[2]), float(row[4]))
    except OSError as e:
        raise ValueError("--dropout_compare %s: %s" % (path, e))
    except ValueError as e:
        raise ValueError("--dropout_compare %s: %s" % (path, e))
    return old


def dropout_report(images: Sequence[tuple], draws: int, old: dict = None):
    """The rows of ``dropout_stats.csv`` (header first) and the folder summary.  ``images``: per image
    ``(name, wood, h, w, count_1, count_2, draw_counts)`` with the deterministic forward's bark / node pixels and
    ``draw_counts`` int ``[draws][3]``.  Figures are formatted '{:.5f}'; the std is empty for one draw.  ``old``
    (``read_shipped_stats``): adds the old file's two percentages, whether each lies within [min, max] of the draws -- the
    bounds taken as the shipped tool prints them (``percent_string`` of the extreme counts), since the old value went through
    that rounding -- and its z score (empty when the std is 0 or absent, or the image is missing from the old file)."""
    fmt = lambda v: "" if v is None else "{:.5f}".format(v)
    header = list(DROPOUT_COLUMNS) + (list(DROPOUT_COMPARE_COLUMNS) if old is not None else [])
    rows, sums, nstd = [header], {}, 0
    inside = {"bark": 0, "node": 0}
    missing, compared = [], 0
    for name, wood, h, w, c1, c2, dc in images:
        px = h * w
        dc = [[int(v) for v in d3] for d3 in dc]
        assert len(dc) == draws
        st = {"bark": draw_statistics([d3[1] for d3 in dc], px), "node": draw_statistics([d3[2] for d3 in dc], px)}
        row = [name, wood, percent_string(c1, px), percent_string(c2, px)]
        for cls in ("bark", "node"):
            row += [fmt(st[cls][k]) for k in ("mean", "std", "min", "max")]
            for k in ("mean", "std", "min", "max"):
                if st[cls][k] is not None:
                    sums[cls + "_" + k] = sums.get(cls + "_" + k, 0.0) + st[cls][k]
        row.append(str(draws))
        if old is not None:
            o = old.get((name, wood))
            if o is None:
                missing.append("%s/%s" % (wood, name))
                row += [""] * len(DROPOUT_COMPARE_COLUMNS)
            else:
                compared += 1
                ins, zs = [], []
                for cls, col, v in (("bark", 1, o[0]), ("node", 2, o[1])):
                    lo = float(percent_string(min(d3[col] for d3 in dc), px))
                    hi = float(percent_string(max(d3[col] for d3 in dc), px))
                    ok = lo <= v <= hi
                    inside[cls] += int(ok)
                    ins.append("1" if ok else "0")
                    zs.append(fmt((v - st[cls]["mean"]) / st[cls]["std"]) if st[cls]["std"] else "")
                row += [fmt(o[0]), fmt(o[1])] + ins + zs
        rows.append(row)
    n = len(images)
    summary = {"draws": draws, "images": n,
               "means": {k: (v / n if n else None) for k, v in sorted(sums.items())}}
    if old is not None:
        summary["compare"] = {"images_compared": compared, "bark_inside": inside["bark"], "node_inside": inside["node"],
                              "missing_from_old": missing}
    return rows, summary


def vote_report(images: Sequence[tuple], draws: int):
    """The rows of ``dropout_votes.csv`` (header first) and the folder means.  ``images``: per image ``(name, wood, h, w, stats,
    changed)`` with the ten integers of nbc_vote_summary (include/nbc.h: pixels per winning class, unanimous pixels per class,
    the sum of n_win, invalid words, the sums of n1 and n2) and the pixels on which the vote mask differs from the
    deterministic label.  The vote percentages are printed as ``final_stats.csv`` prints a percentage (``percent_string``);
    the unanimous percentage ``100 (u0 + u1 + u2) / (h w)`` and the mean support ``sum n_win / (draws h w)`` are each one
    correctly rounded division of exact integers, formatted '{:.5f}'."""
    rows, sums = [list(VOTE_COLUMNS)], {}
    for name, wood, h, w, st, changed in images:
        px = h * w
        st = [int(v) for v in st]
        assert len(st) == VOTE_STATS
        figures = {"vote_bark": (100 * st[1]) / px, "vote_node": (100 * st[2]) / px, "unanimous": (100 * (st[3] + st[4] + st[5])) / px,
                   "mean_support": st[6] / (draws * px), "changed_pixels": int(changed)}
        rows.append([name, wood, str(draws), percent_string(st[1], px), percent_string(st[2], px),
                     "{:.5f}".format(figures["unanimous"]), "{:.5f}".format(figures["mean_support"]), str(int(changed))])
        for k, v in figures.items():
            sums[k] = sums.get(k, 0.0) + v
    n = len(images)
    return rows, {"images": n, "means": {k: (v / n if n else None) for k, v in sorted(sums.items())}}


# ---- the flip views the training augmented over (--tta): masks, argument checks, the report -------------------------------
TTA_CHOICES = ("none", "hflip", "vflip", "flips")
TTA_MASKS = {"none": 0, "hflip": 3, "vflip": 5, "flips": 15}          # NBC_TTA_* bits of include/nbc.h; identity is bit 0


def tta_mask(tta) -> int:
    """The view mask of ``--tta`` (0 = off): one of ``TTA_CHOICES``, None (off) or a mask in 1..15 itself."""
    if tta is None:
        return 0
    if isinstance(tta, str):
        if tta not in TTA_MASKS:
            raise ValueError("--tta must be one of %s, got %r" % (", ".join(TTA_CHOICES), tta))
        return TTA_MASKS[tta]
    if isinstance(tta, bool) or not 0 <= int(tta) <= 15:
        raise ValueError("--tta must be one of %s, got %r" % (", ".join(TTA_CHOICES), tta))
    return int(tta)


def tta_view_names(mask: int) -> List[str]:
    """``model.tta_view_names``: the names of the views of a mask, in the order of the stack (ascending bit order)."""
    from .model import tta_view_names as names
    return names(mask)


def check_tta_arguments(tta, tta_votes: bool = False, dropout_draws=None, only_preprocess: bool = False) -> int:
    """``ValueError`` for what ``--tta`` and ``--tta_votes`` refuse before any device is touched: ``--tta`` with
    ``--dropout_draws`` (the draws read the features of a plain forward) or with ``--only_preprocess`` (no network runs),
    ``--tta_votes`` without ``--tta``.  Returns the view mask (0 = off)."""
    mask = tta_mask(tta)
    if not mask:
        if tta_votes:
            raise ValueError("--tta_votes needs --tta")
        return 0
    if dropout_draws:
        raise ValueError("--tta cannot go with --dropout_draws: TTA under Dropout draws is left out (the draws read the features "
                         "of a plain forward)")
    if only_preprocess:
        raise ValueError("--tta runs the network: it cannot go with --only_preprocess")
    return mask


def tta_columns(mask: int) -> List[str]:
    return view_columns(tta_view_names(mask))


def tta_report(images: Sequence[tuple], views: int):
    """The rows of ``tta_stats.csv`` (header first) and the folder summary.  ``images``: per image ``(name, wood, h, w,
    merged_counts [3], view_counts [V][3], stats [10])`` with the pixels per class of the merged final labels, of each view's
    own final labels (the order of the stack) and the ten integers of nbc_vote_summary over the views (D = V).  Every
    percentage is printed as ``final_stats.csv`` prints one (``percent_string``); the spreads ``100 (max - min) / (h w)`` over
    the views' counts, the unanimous percentage and the mean support are each one correctly rounded division of exact
    integers, formatted '{:.5f}' (``vote_report``'s arithmetic).  The summary's means: the merged and the identity pair (None
    for a mask without the identity view), their mean absolute difference, the spreads and the unanimous share."""
    return views_report(images, tta_view_names(views), 0 if int(views) & 1 else None)


def view_columns(names: Sequence[str]) -> List[str]:
    cols = ["Name", "Type", "Views"]
    for v in names:
        cols += ["%s Bark %%" % v, "%s Node %%" % v]
    return cols + ["Bark %", "Node %", "Bark % spread", "Node % spread", "Unanimous %", "Mean support"]


def views_report(images: Sequence[tuple], names: Sequence[str], identity: int = None):
    """``tta_report``'s and ``jitter_report``'s rows and summary for views called ``names``, in the order of the stack;
    ``identity``: the position of the identity view in it, None for a set without one (no identity pair in the summary)."""
    names = list(names)
    nv = len(names)
    has_identity = identity is not None
    rows, sums = [view_columns(names)], {}
    for name, wood, h, w, mc, vc, st in images:
        px = h * w
        mc, st = [int(v) for v in mc], [int(v) for v in st]
        vc = [[int(v) for v in c3] for c3 in vc]
        assert len(vc) == nv and len(st) == VOTE_STATS and len(mc) == 3
        row = [name, wood, "+".join(names)]
        for c3 in vc:
            row += [percent_string(c3[1], px), percent_string(c3[2], px)]
        spread = [(100 * (max(c3[k] for c3 in vc) - min(c3[k] for c3 in vc))) / px for k in (1, 2)]
        figures = {"merged_bark": (100 * mc[1]) / px, "merged_node": (100 * mc[2]) / px, "bark_spread": spread[0],
                   "node_spread": spread[1], "unanimous": (100 * (st[3] + st[4] + st[5])) / px, "mean_support": st[6] / (nv * px)}
        if has_identity:
            ic = vc[identity]
            figures.update(identity_bark=(100 * ic[1]) / px, identity_node=(100 * ic[2]) / px,
                           abs_diff_bark=abs(100 * (mc[1] - ic[1])) / px, abs_diff_node=abs(100 * (mc[2] - ic[2])) / px)
        row += [percent_string(mc[1], px), percent_string(mc[2], px), "{:.5f}".format(spread[0]), "{:.5f}".format(spread[1]),
                "{:.5f}".format(figures["unanimous"]), "{:.5f}".format(figures["mean_support"])]
        rows.append(row)
        for k, v in figures.items():
            sums[k] = sums.get(k, 0.0) + v
    n = len(images)
    return rows, {"images": n, "views": names, "means": {k: (v / n if n else None) for k, v in sorted(sums.items())}}


# ---- the colour-jitter views the training augmented over (--jitter): view sets, argument checks, the report ------------------
JITTER_CHOICES = ("training",)


def parse_jitter_views(text: str) -> List[tuple]:
    """The triples of ``--jitter_views "b,c,s;b,c,s;..."`` (brightness, contrast, saturation per view); ``ValueError`` for
    anything that is not 1..16 triples of numbers."""
    views = []
    for part in str(text).split(";"):
        fields = part.split(",")
        try:
            triple = tuple(float(f) for f in fields)
        except ValueError:
            triple = ()
        if len(fields) != 3 or len(triple) != 3:
            raise ValueError("--jitter_views takes triples \"b,c,s;b,c,s;...\" of numbers, got %r" % (text,))
        views.append(triple)
    return views


def jitter_factors(jitter=None, jitter_views=None):
    """The float32 ``[V,3]`` factors of ``--jitter NAME`` or ``--jitter_views`` (its string, or a sequence of triples), None
    when neither is given; ``ValueError`` for both at once, an unknown name, or triples ``model.resolve_jitter_views``
    refuses (malformed, more than 16, a factor outside [0, 4])."""
    if jitter in (None, "none") and jitter_views is None:
        return None
    if jitter not in (None, "none") and jitter_views is not None:
        raise ValueError("--jitter and --jitter_views exclude each other: name a view set or spell one out")
    from .model import resolve_jitter_views
    if jitter_views is None:
        if not isinstance(jitter, str) or jitter not in JITTER_CHOICES:
            raise ValueError("--jitter must be one of %s, got %r" % (", ".join(JITTER_CHOICES), jitter))
        return resolve_jitter_views(jitter)
    try:
        return resolve_jitter_views(parse_jitter_views(jitter_views) if isinstance(jitter_views, str) else jitter_views)
    except ValueError as e:
        raise ValueError("--jitter_views: %s" % e)


def jitter_view_names(factors) -> List[str]:
    """The names of the views of a factor array, in the order of the stack (``model.jitter_view_names``)."""
    from .model import jitter_view_names as names
    return names(factors)


def check_jitter_arguments(jitter=None, jitter_views=None, jitter_votes: bool = False, tta=None, dropout_draws=None,
                           only_preprocess: bool = False):
    """``ValueError`` for what ``--jitter``, ``--jitter_views`` and ``--jitter_votes`` refuse before any device is touched: both
    view options at once, malformed or out-of-range triples, a view set with ``--tta`` (products of colour and flip views are
    left out), with ``--dropout_draws`` (the draws read the features of a plain forward) or with ``--only_preprocess`` (no
    network runs), ``--jitter_votes`` without a view set.  Returns the float32 ``[V,3]`` factors, None = off."""
    factors = jitter_factors(jitter, jitter_views)
    if factors is None:
        if jitter_votes:
            raise ValueError("--jitter_votes needs --jitter or --jitter_views")
        return None
    if tta_mask(tta):
        raise ValueError("--jitter cannot go with --tta: products of colour and flip views are left out")
    if dropout_draws:
        raise ValueError("--jitter cannot go with --dropout_draws: colour views under Dropout draws are left out (the draws read "
                         "the features of a plain forward)")
    if only_preprocess:
        raise ValueError("--jitter runs the network: it cannot go with --only_preprocess")
    return factors


def jitter_report(images: Sequence[tuple], factors):
    """The rows of ``jitter_stats.csv`` (header first) and the folder summary: ``tta_report``'s columns and entries
    (``views_report``) under the names of the colour views.  ``images``: per image ``(name, wood, h, w, mean_counts [3],
    view_counts [V][3], stats [10])``."""
    names = jitter_view_names(factors)
    return views_report(images, names, names.index("identity") if "identity" in names else None)


def add_jitter_arguments(ap) -> None:
    """``--jitter`` and ``--jitter_views`` of the predict and evaluate drivers (``check_jitter_arguments`` holds their rules)."""
    ap.add_argument("--jitter", choices=list(JITTER_CHOICES), default=None,
                    help="average the colour-jitter views the training augmented over: training = the image, brightness 0.9 and "
                         "1.1, saturation 0.8 and 1.2; the low-resolution logits of the views are averaged and everything "
                         "downstream is about that mean.  --batch keeps counting images (default 1, 2 in bf16)")
    ap.add_argument("--jitter_views", metavar="\"B,C,S;B,C,S;...\"", default=None,
                    help="the same with views spelled out: 1..16 triples of brightness, contrast and saturation factors in "
                         "[0, 4], applied in that order (not with --jitter)")


# ---- the crop windows the training augmented over (--windows): argument checks, the grid, the report ------------------------
WINDOW_BLENDS = ("tent", "uniform")
WINDOW_COLUMNS = ["Name", "Type", "Height", "Width", "Window", "Grid", "Bark %", "Node %"]
WINDOW_COMPARE_COLUMNS = ["Plain Bark %", "Plain Node %", "Bark % difference", "Node % difference", "Changed pixels %"]


def default_window_stride(window: int) -> int:
    """``--windows_stride`` when it is not given: half the window, rounded down to a multiple of 8."""
    return int(window) // 2 // 8 * 8


def check_windows_arguments(windows=None, windows_stride=None, windows_blend=None, windows_compare: bool = False, tta=None,
                            jitter=None, jitter_views=None, dropout_draws=None, only_preprocess: bool = False,
                            bn_stats: str = None, arch: str = None):
    """``ValueError`` for what ``--windows`` and its companions refuse before any device is touched: a companion without
    ``--windows``; a window that is no multiple of 8 in 32..2048, a stride that is no multiple of 8 with 8 <= stride <= window
    <= 8 stride, an unknown blend (include/nbc.h, nbc_window_grid); ``--windows`` with ``--tta``, ``--jitter`` /
    ``--jitter_views`` (products of views are left out), ``--dropout_draws`` (the draws read the features of a plain forward),
    ``--only_preprocess`` (no network runs), ``--bn_stats image*`` (statistics per window are not the frame's) or a named
    EfficientNet ``arch`` (``check_windows_arch`` once ``"auto"`` is resolved).  Returns ``SimpleNamespace(window, stride, blend,
    compare)``, None = off."""
    if windows is None:
        given = [n for n, v in (("--windows_stride", windows_stride), ("--windows_blend", windows_blend)) if v is not None]
        if windows_compare:
            given.append("--windows_compare")
        if given:
            raise ValueError("%s needs --windows" % ", ".join(given))
        return None
    if isinstance(windows, bool) or int(windows) != windows or int(windows) % 8 or not 32 <= int(windows) <= 2048:
        raise ValueError("--windows must be a multiple of 8 in 32..2048, got %r" % (windows,))
    window = int(windows)
    stride = default_window_stride(window) if windows_stride is None else windows_stride
    if isinstance(stride, bool) or int(stride) != stride or int(stride) % 8 or not 8 <= int(stride) <= window <= 8 * int(stride):
        raise ValueError("--windows_stride must be a multiple of 8 with 8 <= stride <= window <= 8 * stride, got %r for "
                         "--windows %d" % (stride, window))
    blend = "tent" if windows_blend is None else windows_blend
    if blend not in WINDOW_BLENDS:
        raise ValueError("--windows_blend must be one of %s, got %r" % (", ".join(WINDOW_BLENDS), blend))
    if tta_mask(tta):
        raise ValueError("--windows cannot go with --tta: products of crop windows and flip views are left out")
    if jitter not in (None, "none") or jitter_views is not None:
        raise ValueError("--windows cannot go with --jitter or --jitter_views: products of crop windows and colour views are left out")
    if dropout_draws:
        raise ValueError("--windows cannot go with --dropout_draws: the draws read the features of a plain forward")
    if only_preprocess:
        raise ValueError("--windows runs the network: it cannot go with --only_preprocess")
    if bn_stats in ("image", "image_f16x2"):
        raise ValueError("--windows cannot go with --bn_stats %s: statistics per window are not the shipped tool's per-frame "
                         "statistics" % bn_stats)
    if arch not in (None, "auto"):
        check_windows_arch(arch)
    return SimpleNamespace(window=window, stride=int(stride), blend=blend, compare=bool(windows_compare))


def check_windows_arch(arch: str) -> None:
    """``ValueError`` for ``--windows`` on an EfficientNet network (every rank holds the resolved architecture alike, so every
    rank refuses alike)."""
    from . import topology
    if topology.is_efficientnet(arch):
        raise ValueError("--windows is refused for %s: its output stride is 32 and its fixed asymmetric pads need a window grid "
                         "of their own" % arch)


def stacked_call(views_mask: int = 0, factors=None, windows=None):
    """The forward of a run, picked once from what the three ``check_*_arguments`` returned (at most one is on): ``(predict,
    make_stack)``.  ``predict(mdl, x, **kw)`` is ``mdl.predict_labels`` or its form on the flip views, the colour views or the
    crop windows; ``make_stack(mdl, x)`` is the batch that forward runs the network on (what ``autotune`` tunes for)."""
    if views_mask:
        return (lambda mdl, x, **kw: mdl.predict_labels_tta(x, views_mask, **kw)), (lambda mdl, x: mdl.tta_views(x, views_mask))
    if factors is not None:
        return (lambda mdl, x, **kw: mdl.predict_labels_jitter(x, factors, **kw)), (lambda mdl, x: mdl.jitter_views(x, factors))
    if windows is not None:
        wn = windows
        return ((lambda mdl, x, **kw: mdl.predict_labels_windows(x, wn.window, wn.stride, wn.blend, **kw)),
                (lambda mdl, x: mdl.window_views(x, wn.window, wn.stride)))
    return (lambda mdl, x, **kw: mdl.predict_labels(x, **kw)), (lambda mdl, x: x)


def windows_report(images: Sequence[tuple], window: int, stride: int, blend: str, compare: bool = False):
    """The rows of ``windows_stats.csv`` (header first) and the folder summary.  ``images``: per image ``(name, wood, h, w,
    (E_y, E_x, n_y, n_x), merged_counts [3], plain_counts [3] or None, changed pixels or None)`` with the pixels per class of the
    merged final labels and -- ``compare`` -- of the plain forward's, and the pixels on which the two label maps differ.  Every
    percentage is printed as ``final_stats.csv`` prints one (``percent_string``); a difference (merged minus plain) and the
    changed share are each one correctly rounded division of exact integers, formatted '{:.5f}'.  The summary: the folder means
    of the merged pair (with ``compare``: of the plain pair, of the absolute differences and of the changed share) and the
    images per grid shape."""
    rows, sums, grids = [WINDOW_COLUMNS + (WINDOW_COMPARE_COLUMNS if compare else [])], {}, {}
    for name, wood, h, w, grid, mc, pc, changed in images:
        px = int(h) * int(w)
        ey, ex, ny, nx = (int(v) for v in grid)
        mc = [int(v) for v in mc]
        shape = "%dx%d %dx%d" % (ey, ex, ny, nx)
        grids[shape] = grids.get(shape, 0) + 1
        row = [name, wood, str(int(h)), str(int(w)), "%dx%d" % (ey, ex), "%dx%d" % (ny, nx), percent_string(mc[1], px),
               percent_string(mc[2], px)]
        figures = {"merged_bark": (100 * mc[1]) / px, "merged_node": (100 * mc[2]) / px}
        if compare:
            pc = [int(v) for v in pc]
            diff = [(100 * (mc[c] - pc[c])) / px for c in (1, 2)]
            figures.update(plain_bark=(100 * pc[1]) / px, plain_node=(100 * pc[2]) / px, abs_diff_bark=abs(diff[0]),
                           abs_diff_node=abs(diff[1]), changed=(100 * int(changed)) / px)
            row += [percent_string(pc[1], px), percent_string(pc[2], px), "{:.5f}".format(diff[0]), "{:.5f}".format(diff[1]),
                    "{:.5f}".format(figures["changed"])]
        rows.append(row)
        for k, v in figures.items():
            sums[k] = sums.get(k, 0.0) + v
    n = len(rows) - 1
    return rows, {"images": n, "window": int(window), "stride": int(stride), "blend": blend,
                  "means": {k: (v / n if n else None) for k, v in sorted(sums.items())}, "grids": dict(sorted(grids.items()))}


def add_windows_arguments(ap) -> None:
    """``--windows`` and its companions of the predict and evaluate drivers (``check_windows_arguments`` holds their rules)."""
    ap.add_argument("--windows", type=int, default=None, metavar="S",
                    help="sliding-window inference at the training's crop size: every frame is cut into S x S windows (S a "
                         "multiple of 8 in 32..2048; the training used 512), one stacked forward runs them, their "
                         "low-resolution logits are blended over the overlaps and everything downstream is about that blend.  "
                         "--batch keeps counting images (default 1, 2 in bf16)")
    ap.add_argument("--windows_stride", type=int, default=None, metavar="T",
                    help="with --windows: the distance between windows, a multiple of 8 with 8 <= T <= S <= 8 T (default: S / 2 "
                         "rounded down to a multiple of 8)")
    ap.add_argument("--windows_blend", choices=list(WINDOW_BLENDS), default=None,
                    help="with --windows: tent (default) weighs a window cell by its distance from the window's inner borders, "
                         "uniform weighs every covering window alike")
    ap.add_argument("--windows_compare", action="store_true",
                    help="with --windows: also run the plain forward of each frame and report how far the two differ")


def open_run(root: str, tool: str, precision: str, device_index: int = None, batch: int = None, streams: int = None,
             target_size: int = 1024, stack: int = 1, windows=None) -> SimpleNamespace:
    """The rank context of one folder run, and the state its later steps fill in.  An already initialised process group (gloo
    in the one-GPU rehearsals) is used as it is; ``wire_dev`` is where its collectives' tensors live (``collective_device``).
    ``stack``: the entries the forward runs per image (the V views of ``--tta`` or ``--jitter``; 1 otherwise): ``batch`` keeps counting
    images, and its default shrinks so that the stack stays at a size the forward is already run at (4, or 8 in bf16).
    ``windows``: what ``check_windows_arguments`` returned (None = ``--windows`` is off): the forward runs the windows of
    ``batch`` images, so the default batch shrinks likewise, and ``bring_up`` reserves for the window stack of the largest
    frame (``K(target_size, target_size) x batch`` entries of ``E x E``; with ``--windows_compare`` for the plain frame too)."""
    import time
    from collections import defaultdict
    import torch
    r = SimpleNamespace(root=root, tool=tool, precision=precision, target_size=target_size, t_start=time.perf_counter(),
                        world=int(os.environ.get("WORLD_SIZE", "1")), rank=int(os.environ.get("RANK", "0")), dist=None)
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if device_index is None else device_index
    if r.world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        r.dist = dist
    r.dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(r.dev)
    r.wire_dev = collective_device(r.dist, r.dev)
    r.stack = max(1, int(stack))
    r.windows = windows
    if r.stack > 1 or windows is not None:
        r.batch = (2 if precision == "bf16" else 1) if batch is None else batch
    else:
        r.batch = (8 if precision == "bf16" else 2) if batch is None else batch
    r.n_streams = 4 if streams is None else max(1, int(streams))
    r.depth = r.n_streams + 1                        # slots of the pinned rings: one more than batches in flight
    r.marker = AbandonMarker(root)
    r.prof = defaultdict(float)                      # seconds per stage, summed over threads
    r.shape_count = defaultdict(int)                 # images seen per frame shape, the running window included
    r.n_batches = 0
    return r


def _start(r, make_dirs) -> None:
    """Rank 0's ``make_dirs(root)`` and the start barrier."""
    if r.rank == 0:
        make_dirs(r.root)
        r.marker.clear()
    if r.dist is not None:
        r.dist.barrier()


def bring_up_without_model(r, make_dirs) -> None:
    """``bring_up`` for a driver that reads no checkpoint and runs no network (``stats``): rank 0's ``make_dirs(root)``, the
    start barrier and the side streams.  ``r.models`` holds no object, one None per stream: ``run_loop`` touches a model only
    for the f16x2 guards, which ``r.precision`` = "fp32" (required here) never runs."""
    import time
    import torch
    if r.precision != "fp32":
        raise ValueError("a run without a model has no arithmetic mode: precision must be 'fp32', not %r" % (r.precision,))
    _start(r, make_dirs)
    r.arch = None
    r.models = [None] * r.n_streams
    r.gpu_streams = [torch.cuda.Stream(r.dev) for _ in range(r.n_streams)]
    r.t_ready = time.perf_counter()


def bring_up(r, model_path: str, arch: str, bn_stats: str, precision_auto: bool, make_dirs, warm=None,
             normalization=None, stack: int = 1, logit_offsets=None) -> None:
    """Rank 0's ``make_dirs(root)`` and the start barrier, then ``r.models`` (``r.n_streams`` objects on one copy of the
    weights), ``r.gpu_streams``, and the resolved ``r.arch`` / ``r.precision``.  ``warm(model)``: the driver's own workspaces, grown
    to their largest size once like the forward's.  ``normalization``: the ``(mean, std)`` of the uint8 ingest
    (``resolve_normalization``), set on every model object before anything runs (a clone owns its context and would start on
    the defaults); None leaves the defaults of models.py:208-209.  ``stack``: the entries the forward runs per image (the views
    of ``--tta``; ``open_run``'s ``stack`` counts as well): the workspace is reserved for ``stack x r.batch`` entries.
    ``logit_offsets``: the ``(bark, node)`` pair of ``--logit_offsets`` (``check_logit_offsets``), set on every model object
    like the normalisation; None leaves the plain argmax."""
    import time
    import torch
    from .model import MODELS
    _start(r, make_dirs)
    state_dict = None
    if r.rank == 0:                                  # only one rank touches the checkpoint
        state_dict = torch.load(model_path, map_location="cpu", weights_only=True)
    r.arch = resolve_arch(arch, state_dict, r.dist, r.dev)
    check_bn_stats_arch(bn_stats, r.arch)
    if r.windows is not None:
        check_windows_arch(r.arch)                   # --arch auto: the checkpoint's keys have named the network by now
    r.precision = resolve_arch_precision(r.arch, r.precision, precision_auto)   # EfficientNet: fp32
    model = MODELS[r.arch](r.precision).set_bn_statistics(bn_stats).to(r.dev)
    if r.rank == 0:
        model.load_state_dict(state_dict)
    del state_dict
    if r.dist is not None:
        model.broadcast_weights(src=0)
    if r.precision == "f16x2" and model.pack_flags:
        # what the packer had to give up rides in the blob's trailer: every rank reads the same bits and leaves here alike
        raise NonFiniteLogits("the packed weights carry NBC_PACK flags %d (a weight row beyond the reach of the f16x2 row "
                              "normalisation, or a BatchNorm scale outside f32's normal range under its powers of two): f16x2 "
                              "would not be f32 grade on this checkpoint; rerun with --precision fp32" % model.pack_flags)
    r.models = [model] + [model.clone_shared() for _ in range(r.n_streams - 1)]
    if normalization is not None:                    # every rank parsed the same arguments: no collective
        for m in r.models:
            m.set_normalization(*normalization)
    if logit_offsets is not None:
        for m in r.models:
            m.set_logit_offsets(*logit_offsets)
    # side streams only: the default stream stays with whatever else the driver runs on the device
    r.gpu_streams = [torch.cuda.Stream(r.dev) for _ in range(r.n_streams)]
    for m in r.models:                               # the largest workspace once: a context's buffers only grow, and a folder of
        if r.windows is not None:                    # --windows: the window stack of the largest frame
            from .model import window_grid
            ey, ex, ny, nx, _, _ = window_grid(r.target_size, r.target_size, r.windows.window, r.windows.stride)
            m.reserve(r.batch * ny * nx, ey, ex)
        if r.windows is None or r.windows.compare:
            m.reserve(r.batch * max(r.stack, int(stack)), r.target_size, r.target_size)   # rising heights would otherwise free and reallocate them shape after shape
        if warm is not None:
            warm(m)
    torch.cuda.synchronize(r.dev)                    # weights uploaded / received before any side stream reads them
    r.t_ready = time.perf_counter()


def shard(r, items: Sequence, size_of, units=None) -> list:
    """Starts the host pool (``r.pool``) and cuts ``items`` into contiguous, pixel-balanced shards by ``size_of(item)`` ->
    ``(h, w)`` (a header read, on the pool); ``r.mine``: this rank's global indices; ``r.shards``: every rank's.  ``units``:
    ``units(sizes)`` -> the unit of every item (``shard_by_units``: a unit stays on one rank), called once the pool runs and
    the sizes are known.  Returns every item's size."""
    from concurrent.futures import ThreadPoolExecutor
    r.workers = _host_workers()
    r.pool = ThreadPoolExecutor(max_workers=r.workers)
    sizes = list(r.pool.map(size_of, items))
    if units is None:
        shards = shard_by_pixels([h * w for h, w in sizes], r.world)
    else:
        shards = shard_by_units([h * w for h, w in sizes], units(sizes), r.world)
    r.n_total, r.mine, r.cap, r.shards = len(items), shards[r.rank], max(len(s) for s in shards), shards
    return sizes


def _calibration_guard(r, first_frame) -> None:
    """f16x2: nbc_pack_weights places every tensor by its BatchNorm's promise (|beta| + 3 |gamma|); whether the DATA keeps that
    promise shows on the first image: rank 0 runs it once with every activation kept and looks at each stored tensor's
    largest value.  One below 2^-8 sits mostly under the f16 pieces' 2^-12 floor -- finite logits, nothing for the
    non-finite flag to see --, one beyond 2^14 is a factor four from f16's range: either way the folder belongs on the f32
    MFMA, and every rank leaves here alike (one scalar broadcast), before any batch has run."""
    import torch
    from .model import FCNResNet50
    verdict = torch.zeros(1, dtype=torch.int32)
    offenders = {}
    first = first_frame() if r.rank == 0 else None
    if first is not None:
        peaks = r.models[0].activation_peaks(torch.from_numpy(np.ascontiguousarray(first[None])).to(r.dev))
        ok, offenders = FCNResNet50.f16x2_range_ok(peaks)
        verdict[0] = 0 if ok else 1
    if r.dist is not None:
        verdict = _on_wire(verdict, r.wire_dev)
        r.dist.broadcast(verdict, src=0)
    if int(verdict.cpu()[0]) != 0:
        r.pool.shutdown(wait=True, cancel_futures=True)
        worst = ", ".join("%s %.3g" % kv for kv in sorted(offenders.items(), key=lambda kv: kv[1])[:4])
        raise NonFiniteLogits("calibration on the first image: an activation tensor lies outside the range the f16 pieces hold "
                              "at f32 grade (stored peak below 2^-8 or beyond 2^14%s): f16x2 would lose bits silently on this "
                              "checkpoint; rerun with --precision fp32" % ((": " + worst) if worst else ""), 0, len(r.mine))


def run_loop(r, window: int, prepare, launch, consume, first_frame, calibrate: bool = True,
             bytes_per_pixel: Sequence[int] = (3,), on_abandon=None, abandon_note: str = "") -> None:
    """The calibration guard, the batch loop over ``r.mine`` and the non-finite settlement.

    Local image k (global ``r.mine[k]``) is prepared on the pool one window ahead: ``prepare(k)`` returns a tuple of uint8
    arrays, the ``[h, w, 3]`` frame first, or None for an image that is skipped.  A window's frames are grouped by shape
    (``batches_of``); batch number b takes stream and model ``b % n_streams`` and slot ``b % depth`` of the pinned staging
    buffers (``bytes_per_pixel``: one buffer per array of the tuple), which an event guards against the copy that last read
    them.  On its stream, ``launch(slot, sid, part, *device_arrays)`` queues the driver's work and the copies into the
    driver's own result ring; the context's sticky non-finite word rides back behind them (f16x2: nbc_nonfinite_peek_async,
    no synchronisation) and an event closes the slot.  Once more than ``n_streams`` batches are pending the oldest is waited
    for and ``consume(slot, part, n, h, w)`` takes its results; the futures it returns are waited for before the pool
    closes.  A non-zero word abandons the run at that batch: nothing of it is consumed, the other ranks of the node learn of it
    through the marker at their next window, and after the MAX all-reduce every rank raises ``NonFiniteLogits`` alike
    (``on_abandon()`` first: the driver's clean-up; ``abandon_note``: what the message says of it).
    ``first_frame()``: rank 0's first frame for the calibration guard, or None."""
    import sys
    import time
    from collections import deque
    import torch
    clock, prof, mine, pool = time.perf_counter, r.prof, r.mine, r.pool
    dev, models, n_streams, depth, batch = r.dev, r.models, r.n_streams, r.depth, r.batch
    check_flag = r.precision == "f16x2"
    if check_flag and calibrate:
        _calibration_guard(r, first_frame)
    # pinned staging, allocated once for the largest batch: pinning memory costs milliseconds, and a folder of rising
    # heights would otherwise re-pin at every new shape
    full = batch * r.target_size * r.target_size
    stage = [[torch.empty(full * c, dtype=torch.uint8).pin_memory() for c in bytes_per_pixel] for _ in range(depth)]
    stage_ev = [torch.cuda.Event() for _ in range(depth)]
    ring_ev = [torch.cuda.Event() for _ in range(depth)]
    flag_host = torch.zeros(depth, dtype=torch.int32).pin_memory()
    bad = False
    pending = deque()                                # (slot, [k], n, h, w), oldest first
    done = []

    def settle(p):
        nonlocal bad
        ring_ev[p[0]].synchronize()
        if check_flag and int(flag_host[p[0]]) != 0:
            bad = True                               # this batch's results (and every later one's) are not valid: none is consumed
            if r.world > 1:
                r.marker.set()                       # the other ranks of the node stop at their next window
            return
        done.extend(consume(*p) or ())

    # the GPU loop runs in this thread next to up to 32 busy pool threads: a short switch interval keeps it
    # from waiting 5 ms for the interpreter lock at every step (restored below)
    switch = sys.getswitchinterval()
    sys.setswitchinterval(2e-4)
    try:
        wins = windows(len(mine), window)
        futs = {k: pool.submit(prepare, k) for k in (wins[0] if wins else [])}
        r.t_loop = clock()
        for wi, win in enumerate(wins):
            if check_flag and r.world > 1 and not bad and r.marker.is_set():
                bad = True                               # another rank of the node saw the word
            if bad:                                      # f16x2 cannot carry these weights: the run is abandoned here
                break
            if wi + 1 < len(wins):                       # the pool starts on the next window before the GPU gets this one
                for k in wins[wi + 1]:
                    futs[k] = pool.submit(prepare, k)
            t0 = clock()
            got = {k: futs.pop(k).result() for k in win}
            prof["main.wait_for_frames"] += clock() - t0
            parts = batches_of(win, {k: None if g is None else g[0].shape for k, g in got.items()}, batch)
            for shape, part in parts:
                r.shape_count[shape] += len(part)
            for shape, part in parts:
                if bad:
                    break
                n, (h, w) = len(part), shape[:2]
                t0 = clock()
                slot, sid = r.n_batches % depth, r.n_batches % n_streams   # free: at most n_streams batches are pending, on other slots
                bufs = stage[slot]                            # frames are packed while the GPU runs the batches before
                for i, c in enumerate(bytes_per_pixel):       # a stale file under processed/ with no sample is predicted as it
                    if bufs[i].numel() < n * h * w * c:       # is, at any size: the one frame larger than target_size
                        bufs[i] = torch.empty(n * h * w * c, dtype=torch.uint8).pin_memory()
                stage_ev[slot].synchronize()                  # the copies that last read these buffers have finished
                host = [b[: n * h * w * c].view((n,) + a.shape) for b, c, a in zip(bufs, bytes_per_pixel, got[part[0]])]
                views = [t.numpy() for t in host]
                for j, k in enumerate(part):
                    for v, a in zip(views, got[k]):
                        v[j] = a
                t1 = clock()
                with torch.cuda.stream(r.gpu_streams[sid]):
                    on_dev = [t.to(dev, non_blocking=True) for t in host]   # uint8, the frame NHWC; normalised on the device
                    stage_ev[slot].record()
                    launch(slot, sid, part, *on_dev)
                    if check_flag:
                        models[sid].nonfinite_peek_async(flag_host[slot:slot + 1])
                    ring_ev[slot].record()
                t2 = clock()
                pending.append((slot, part, n, h, w))
                while len(pending) > n_streams:               # the oldest batch's results, while the newer ones run
                    settle(pending.popleft())
                prof["main.pack"] += t1 - t0; prof["main.h2d_and_launch"] += t2 - t1; prof["main.consume"] += clock() - t2
                r.n_batches += 1
            got.clear()
        while pending:
            settle(pending.popleft())
        for f in done:
            f.result()
    finally:                                         # also on an exception from a worker: no stray threads, switch interval restored
        pool.shutdown(wait=True, cancel_futures=True)
        sys.setswitchinterval(switch)
    torch.cuda.synchronize()
    r.t_done = clock()
    if check_flag:
        # f16x2 keeps every value as two f16 pieces: an activation beyond +-65504 cannot be represented and turns into NaN
        # (never into a silently wrong number).  Unknown weights that do this belong in the f32 MFMA mode.  Every rank
        # learns of it (one more tiny collective) so that all of them leave before the row gather, none waits in it.
        # The word rides back with every batch (settle), so a rank that sees it stops at that batch instead of finishing its
        # shard; the contexts are all read (and reset) here once more, whatever the first one says.
        bad = any([m.nonfinite_seen() for m in models]) or bad
        if r.dist is not None:
            flag = _on_wire(torch.tensor([int(bad)], dtype=torch.int32), r.wire_dev)
            r.dist.all_reduce(flag, op=r.dist.ReduceOp.MAX)
            bad = bool(int(flag.item()))
            if r.rank == 0:
                r.marker.clear()                     # every rank is past its loop (the all-reduce above)
        if bad:
            if on_abandon is not None:
                on_abandon()
            raise NonFiniteLogits("a forward produced non-finite logits in f16x2 mode (an activation beyond f16's range, or NaN/inf "
                                  "in the weights): the %s run was abandoned after %d of this rank's %d images%s; rerun with "
                                  "--precision fp32" % (r.tool, min(r.n_batches * batch, len(mine)), len(mine), abandon_note),
                                  r.n_batches, len(mine))


def gather(r, rows: np.ndarray, width: int) -> np.ndarray:
    """One ``all_gather`` of this rank's rows, the largest shard as the cap."""
    return gather_rows(rows, r.n_total, r.world, r.dist, r.wire_dev, cap=r.cap, width=width)


def finish(r) -> dict:
    """The final barrier, and the statistics of this rank that every driver returns."""
    import time
    if r.dist is not None:
        r.dist.barrier()
    loop_s = r.t_done - r.t_loop
    return {"rank": r.rank, "world": r.world, "images_total": r.n_total, "images_this_rank": len(r.mine), "batches": r.n_batches,
            "batch": r.batch, "streams": r.n_streams, "setup_s": r.t_ready - r.t_start, "loop_s": loop_s,
            "total_s": time.perf_counter() - r.t_start, "images_per_s_loop": len(r.mine) / max(loop_s, 1e-9)}


def launch_ranks(n: int, argv: Sequence[str], module: str = "neuralbarkcalculator_amd.predict") -> int:
    """``--gpus N`` without a torchrun environment: start N ranks (one per GPU) of ``module`` as a child process."""
    import socket
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < n:                # counts devices without initialising HIP
        print("predict: --gpus %d but this node shows %d GPU(s)" % (n, torch.cuda.device_count()), file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", module] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def add_shared_arguments(ap) -> None:
    """The options the predict and evaluate drivers take."""
    ap.add_argument("--model_path", default="./best_model.pt")       # predict.py:57
    ap.add_argument("--precision", choices=["auto", "fp32", "f16x2", "bf16"], default="auto",
                    help="auto (default): the f32-grade f16x2 mode, 2.4x faster than the f32 MFMA at the same tolerances, and a "
                         "second run in fp32 if the weights drive an activation beyond f16's range (the library says so); fp32: "
                         "f32 MFMA; bf16: throughput mode, not f32 grade")
    ap.add_argument("--gpus", type=int, default=1, help="shard the folder over N GPUs of this node (one process each, RCCL)")
    ap.add_argument("--batch", type=int, default=None, help="frames of equal size per forward (default 2, 8 in bf16)")
    ap.add_argument("--streams", type=int, default=None, help="batches in flight, each on its own HIP stream (default 4)")
    ap.add_argument("--arch", choices=["auto"] + list(ARCH_CHOICES), default="auto",
                    help="the network of the checkpoint; auto (default): the one whose state_dict keys it holds")
    ap.add_argument("--bn_stats", choices=list(BN_STATS), default="running",
                    help="running (default): BatchNorm on the running statistics (eval mode); image: each image's own statistics, "
                         "as the shipped tool ran them (fp32, FCN-ResNet-50 only; --precision auto then means fp32); image_f16x2: "
                         "the same statistics on the f16x2 pipe (--precision f16x2, or auto: f16x2 under its guards, else image "
                         "in fp32)")
    ap.add_argument("--tta", choices=list(TTA_CHOICES), default="none",
                    help="average the flip views the training augmented over: hflip / vflip (the image and its mirror image) or "
                         "flips (all four); the low-resolution logits of the un-flipped views are averaged and everything "
                         "downstream is about that mean.  --batch keeps counting images (default 1, 2 in bf16)")
    add_jitter_arguments(ap)
    add_windows_arguments(ap)
    ap.add_argument("--logit_offsets", type=float, nargs=2, metavar=("BARK", "NODE"), default=None,
                    help="move the operating point: the label of a pixel is argmax(x0, x1 + BARK, x2 + NODE) of its logits "
                         "instead of the plain argmax, decided in the forward's own upsample + argmax launch; everything "
                         "downstream sees that decision, the logits themselves (--loss, --ce, --calibration) do not change.  "
                         "evaluate --operating_points proposes pairs")
    ap.add_argument("--mean", type=float, nargs=3, metavar=("R", "G", "B"), default=None,
                    help="per-channel mean of the training folder, on the [0, 1] scale, that the frames are normalised with "
                         "(with --std; default: the constants of the reference's model class)")
    ap.add_argument("--std", type=float, nargs=3, metavar=("R", "G", "B"), default=None,
                    help="per-channel standard deviation that goes with --mean")
    ap.add_argument("--stats", metavar="PATH", default=None,
                    help="take mean and std from this JSON (results/dataset_stats.json of python -m neuralbarkcalculator_amd.stats) "
                         "instead of --mean / --std")


def add_zones_arguments(ap) -> None:
    """``--zones`` and ``--zones_cap`` of ``predict`` (``check_zones_arguments`` holds their rules)."""
    ap.add_argument("--zones", action="store_true",
                    help="also inventory the bark zones and nodes of every label map (8-connected components per class, on the "
                         "device) and write results/zones.csv, zones_summary.csv and zones_summary.json")
    ap.add_argument("--zones_cap", type=int, default=None, metavar="ROWS",
                    help="with --zones: zone rows per image the device pass keeps (default 1024); an image with more zones is "
                         "inventoried on the host from its label map instead")


def add_dropout_arguments(ap) -> None:
    """``--dropout_draws`` and its companions (the predict driver)."""
    ap.add_argument("--dropout_draws", type=int, default=None, metavar="D",
                    help="also sample D random draws (1..1024) of the live Dropout the shipped tool ran with, per image, and write "
                         "results/dropout_stats.csv and dropout_summary.json (fcn_resnet50 only)")
    ap.add_argument("--dropout_votes", action="store_true",
                    help="with --dropout_draws: vote per pixel over the draws and write results/dropout_votes/ (the majority "
                         "mask), results/dropout_support/ (grey, 255 = every draw agrees) and results/dropout_votes.csv")
    ap.add_argument("--dropout_p", type=float, default=None, help="the Dropout probability (default 0.1, FCNHead's)")
    ap.add_argument("--dropout_seed", type=int, default=None, help="64-bit seed of the draws (default 0)")
    ap.add_argument("--dropout_compare", metavar="OLD_final_stats.csv", default=None,
                    help="a final_stats.csv of the shipped tool: report where its numbers lie within the draws")


def check_logit_offsets(logit_offsets, dropout_draws=None, confidence: bool = False):
    """``ValueError`` for what ``--logit_offsets BARK NODE`` refuses before any device is touched: a pair that is not two finite
    numbers, ``--dropout_draws`` (the draws have a tail of their own, which decides by the plain argmax) and ``predict
    --confidence`` (the confidence byte is the raw argmax's probability).  Returns the pair as float32-exact floats, or None
    when the option is not given."""
    import math
    if logit_offsets is None:
        return None
    try:
        pair = tuple(float(np.float32(v)) for v in logit_offsets)
    except (TypeError, ValueError):
        raise ValueError("--logit_offsets takes two numbers, BARK and NODE")
    if len(pair) != 2 or not all(math.isfinite(v) for v in pair):
        raise ValueError("--logit_offsets takes two finite numbers, BARK and NODE, got %r" % (logit_offsets,))
    if dropout_draws:
        raise ValueError("--logit_offsets cannot go with --dropout_draws: offsets under the Dropout draws are left out (the draws "
                         "decide by the plain argmax)")
    if confidence:
        raise ValueError("--logit_offsets cannot go with --confidence: the confidence byte is the raw argmax's probability")
    return pair


def resolve_normalization(mean=None, std=None, stats: str = None):
    """The ``(mean, std)`` pair (two tuples of three floats) the drivers' ``--mean R G B --std R G B`` or ``--stats PATH``
    name, or None when none of them is given.  ``ValueError``: one of ``mean`` / ``std`` without the other, ``stats`` beside
    them, a file that cannot be read as JSON or lacks one of the two keys, a value count other than three, a mean that is not
    finite, a std that is not finite and positive."""
    import json
    import math
    if stats is not None:
        if mean is not None or std is not None:
            raise ValueError("--stats names the mean and std: --mean / --std cannot be given beside it")
        try:
            with open(stats) as f:
                doc = json.load(f)
        except (OSError, ValueError) as e:
            raise ValueError("--stats %s: %s" % (stats, e))
        if not isinstance(doc, dict) or "mean" not in doc or "std" not in doc:
            raise ValueError("--stats %s: the file holds no \"mean\" and \"std\"" % stats)
        mean, std = doc["mean"], doc["std"]
    if mean is None and std is None:
        return None
    if mean is None or std is None:
        raise ValueError("--mean and --std go together: both or neither")
    try:
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    except (TypeError, ValueError):
        raise ValueError("mean and std must be three numbers each")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std must be three numbers each")
    if not all(math.isfinite(v) for v in mean):
        raise ValueError("mean must be finite, got %r" % (mean,))
    if not all(math.isfinite(v) and v > 0 for v in std):
        raise ValueError("std must be finite and positive, got %r" % (std,))
    return mean, std


def resolve_arguments(ap, args) -> None:
    """``args.precision`` as ``--bn_stats`` and a named ``--arch`` leave it, and ``args.normalization``
    (``resolve_normalization``: the pair, or None); what they refuse ends in ``ap.error``."""
    try:
        args.normalization = resolve_normalization(args.mean, args.std, args.stats)
        args.precision = resolve_bn_stats(args.bn_stats, args.precision)
        if args.arch != "auto":
            check_bn_stats_arch(args.bn_stats, args.arch)
        args.precision = resolve_arch_precision(args.arch, args.precision)
    except ValueError as e:
        ap.error(str(e))


def run_precision(tool: str, run, precision: str, bn_stats: str = "running") -> dict:
    """``run(precision)``; for ``"auto"``, ``run("f16x2", precision_auto=True)`` and, when that mode cannot carry the weights
    (``NonFiniteLogits``, raised on every rank alike), the folder again as ``run("fp32")``.  ``bn_stats`` "image_f16x2" has no
    fp32 form of its own: the second run is ``run("fp32", bn_stats="image")``, the same statistics on the f32 MFMA."""
    if precision != "auto":
        return run(precision)
    try:
        return run("f16x2", precision_auto=True)
    except NonFiniteLogits as e:
        if int(os.environ.get("RANK", "0")) == 0:
            print("%s: %s -- running the folder again on the f32 MFMA" % (tool, e), flush=True)
    # outside the except block: the exception's traceback holds the first run's frame (the model contexts with their
    # workspaces, the pinned rings, the streams) for as long as the block lasts
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    if bn_stats == "image_f16x2":
        return run("fp32", bn_stats="image")
    return run("fp32")
