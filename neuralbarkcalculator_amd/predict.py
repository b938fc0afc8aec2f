"""Folder-level batch prediction: the caller side of the hot path, sharded over the GPUs of a node.

Reproduces the file contract of the reference's inference entry point
(/root/reference/src/bark_calculator/predict.py:10-58 and models.py:230-364) around the
accelerated model call:

* input  ``ROOT/samples/<wood_type>/*.{bmp,png,...}``; wood types and order of ``dataset.py:50-58``
  (``epinette_gelee, epinette_non_gelee, sapin``; file names sorted; ``"bmp" -> "png"`` in the
  output name, every occurrence, like ``str.replace`` there);
* ``ROOT/processed/samples/<wood_type>/<name>.png`` (``models.py:173-203``: the bicubic resize to
  1024 x 1024 of larger images, ``trim_black`` on square ones; host-side numpy, pinned by
  scikit-image 0.18.3 fixtures);
* ``ROOT/results/outputs/<wood_type>/<name>.png``: uint8 {0,127,255} mode 'L' (``models.py:349-356``);
* ``ROOT/results/final_stats.csv``: tab separated, the reference's 7-name header and 6-value rows
  (``models.py:252-255,315-332,360-364``: ``img_size`` is dropped by the re-initialisation at
  ``models.py:321``; reproduced verbatim).  The matplotlib figure of ``models.py:280-347``
  (about 10 s per image) is not produced.

Multi-GPU (one process per GPU, ``torch.distributed`` over RCCL; ``--gpus N`` starts the ranks): the
sorted list is cut into contiguous, pixel-balanced shards; rank 0 alone reads the checkpoint and
broadcasts the packed weights; every rank fills int64 rows ``(global_idx, H, W, count_1, count_2)``
which one ``all_gather`` brings to rank 0 for the CSV.  No collective sits in the per-image path.  The ranks, the model
bring-up, the batch loop and the f16x2 guards are ``folder_run``'s, shared with the evaluate driver.
"""
from __future__ import annotations

import argparse
import csv
import os
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import folder_run
from .folder_run import (ARCH_CHOICES, BN_STATS, AbandonMarker, NonFiniteLogits, _host_workers, check_bn_stats_arch,  # noqa: F401
                         gather_rows, launch_ranks, resolve_arch, resolve_arch_precision, resolve_bn_stats, shard_by_pixels,
                         shard_indices)      # the folder-run engine's helpers, under the names they have always had here

WOOD_TYPES = ["epinette_gelee", "epinette_non_gelee", "sapin"]            # dataset.py:50
IMG_EXTENSIONS = [".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", "webp"]  # dataset.py:77-79
MM2_PER_PIXEL = 3.6 * 3.6                                                  # models.py:210
CSV_HEADER = ["Name", "Type", "Image Size", "Output Bark %", "Bark area (mm^2)",
              "Output Node %", "Node area (mm^2)"]                         # models.py:252-255
ROW_WIDTH = 5                                                              # (global_idx, H, W, count_1, count_2)


def generate_folders(root: str, only_preprocess: bool = False, votes: bool = False, tta_votes: bool = False,
                     confidence: bool = False, jitter_votes: bool = False) -> None:
    """predict.py:10-48.  ``votes``: the two directories of ``--dropout_votes`` as well; ``tta_votes``: the one of ``--tta_votes``;
    ``confidence``: the one of ``--confidence``; ``jitter_votes``: the one of ``--jitter_votes``."""
    present = os.listdir(os.path.join(root, "samples"))
    wood_types = [w for w in WOOD_TYPES if w in present]
    for w in wood_types:
        os.makedirs(os.path.join(root, "processed", "samples", w), exist_ok=True)
    if not only_preprocess:
        for level in ("combined_images", "outputs") + (("dropout_votes", "dropout_support") if votes else ()) + \
                (("tta_support",) if tta_votes else ()) + (("confidence",) if confidence else ()) + \
                (("jitter_support",) if jitter_votes else ()):
            for w in wood_types:
                os.makedirs(os.path.join(root, "results", level, w), exist_ok=True)


def list_images(dir_: str) -> List[Tuple[str, str, str]]:
    """(sample_path, output_name, wood_type) in the order of dataset.py:41-68."""
    samples = os.path.join(dir_, "samples")
    if not os.path.isdir(samples):
        raise IOError("Root folder should have a 'samples' subfolder !")   # dataset.py:45-46
    out = []
    for wood in WOOD_TYPES:
        d = os.path.join(samples, wood)
        for _, _, fnames in sorted(os.walk(d)):
            for fname in sorted(fnames):
                if any(fname.lower().endswith(e) for e in IMG_EXTENSIONS):
                    out.append((os.path.join(d, fname), fname.replace("bmp", "png"), wood))
    return out


def trim_black(image: np.ndarray) -> np.ndarray:
    """models.py:157-166 on a float HWC image in [0,1]: drop leading/trailing rows in which 15 % or
    more of the pixels are black (channel sum <= 1e-3)."""
    lit = np.sum(image, axis=-1) > 1e-3
    clear = np.mean(lit, axis=-1) > 0.85
    first = int(np.argmax(clear))
    last = image.shape[0] - int(np.argmax(clear[::-1]))
    return image[first:last]


def _cubic(x, f0, f1, f2, f3):
    """scikit-image's cubic_interpolation (Catmull-Rom, a = -0.5): values at -1, 0, 1, 2; x in [0, 1].
    Evaluated in the image's own float type throughout, in the order its Cython source is written
    (``f1 + 0.5*x*(f2 - f0 + x*(2*f0 - 5*f1 + 4*f2 - f3 + x*(3*(f1 - f2) + f3 - f0)))``), one rounding per
    operation: this is what the compiled _warp_fast does for a float32 image (checked value for value
    against scikit-image 0.18.3, tests/golden/preprocess_*.npz ``float32``)."""
    t = x.dtype.type
    return f1 + t(0.5) * x * (f2 - f0 + x * (t(2.0) * f0 - t(5.0) * f1 + t(4.0) * f2 - f3 + x * (t(3.0) * (f1 - f2) + f3 - f0)))


def _reflect(i: np.ndarray, n: int) -> np.ndarray:
    """numpy.pad 'reflect' indexing (mirror without repeating the edge)."""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return np.where(i >= n, period - i, i)


def resize_bicubic_reflect(image: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """``skimage.transform.resize(image, (out_h, out_w), order=3, mode='reflect',
    anti_aliasing=False)`` (models.py:194-198) for a float HWC image, as scikit-image 0.18.3 computes it:
    ``resize`` builds the metric transform ``[[fx, 0, fx/2 - 1/2], [0, fy, fy/2 - 1/2]]`` (f = in / out) in
    double, ``warp`` casts it to the image's float type and ``_warp_fast`` evaluates everything in that
    type: the sample position of output pixel i is ``f * i + (f/2 - 1/2)`` (one product, one sum, each
    rounded), its fractional part is taken in the same type, the 4 x 4 taps (reflected borders) go
    through ``_cubic`` row-wise then column-wise, and the result is clipped to the input range
    (``clip=True``).  Bit-identical to scikit-image's output on the committed fixtures, integer and
    non-integer zoom factors alike."""
    h, w = image.shape[:2]
    dt = image.dtype if image.dtype in (np.float32, np.float64) else np.float64
    t = np.dtype(dt).type
    img = image.astype(dt, copy=False)
    fy, fx = h / out_h, w / out_w                                    # Python doubles, like resize's `factors`
    ry = t(fy) * np.arange(out_h, dtype=dt) + t(fy * 0.5 - 0.5)
    rx = t(fx) * np.arange(out_w, dtype=dt) + t(fx * 0.5 - 0.5)
    y0 = np.floor(ry).astype(np.int64)
    x0 = np.floor(rx).astype(np.int64)
    ty = (ry - y0.astype(dt)).reshape(-1, 1, 1)
    tx = (rx - x0.astype(dt)).reshape(1, -1, 1)
    cols = [_reflect(x0 + k - 1, w) for k in range(4)]
    fr = []
    for k in range(4):
        rows = img[_reflect(y0 + k - 1, h)]
        fr.append(_cubic(tx, *[rows[:, c] for c in cols]))
    out = _cubic(ty, *fr)
    assert out.dtype == dt
    return np.clip(out, img.min(), img.max())


def _float_to_u8(image: np.ndarray) -> np.ndarray:
    """``skimage.io.imsave`` of a float image in [0, 1] (models.py:203) goes through imageio's
    ``image_as_uint``: ``uint8(float64(x) * 255 + 0.499999999)`` (exact halves round down)."""
    return np.clip(image.astype(np.float64) * 255.0 + 0.499999999, 0, 255).astype(np.uint8)


# uint8 -> ToTensor (float32 / 255) -> imsave's float -> uint8: a 256-entry table (it is the identity, which
# tests/test_driver.py asserts; the table keeps the code honest should a platform's float division differ)
_U8_ROUND_TRIP = _float_to_u8(np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255))
_U8_ROUND_TRIP_IS_IDENTITY = bool(np.array_equal(_U8_ROUND_TRIP, np.arange(256, dtype=np.uint8)))


def _trim_rows(clear: np.ndarray) -> Tuple[int, int]:
    """models.py:162-166: first / one-past-last row of the ``clear`` (enough lit pixels) flags."""
    first = int(np.argmax(clear))
    last = clear.shape[0] - int(np.argmax(clear[::-1]))
    return first, last


def preprocess_image(img_u8: np.ndarray, target_size: int = 1024, model=None) -> np.ndarray:
    """models.py:191-203 for one decoded RGB image: ToTensor (u8 -> float32 / 255), resize to
    ``target_size`` x ``target_size`` when either side is larger, ``trim_black`` when square,
    float -> uint8 like ``skimage.io.imsave`` does through imageio.  Byte-identical to what scikit-image
    0.18.3 writes (tests/golden/preprocess_*.npz).  Three routes, same bytes:

    * no resize needed: the float round trip maps every byte to itself and a pixel is "lit" (float32 channel
      sum > 1e-3) exactly when one of its bytes is non-zero, so the image is trimmed as uint8;
    * resize with ``model`` (an ``FCNResNet50`` on a device): resize, float -> uint8 and the per-row lit
      counts on the device (``nbc_preprocess_u8``), the row trim here;
    * resize without a device: the numpy restatement (about 1 s for a 4096 x 4096 scan)."""
    if max(img_u8.shape[:2]) <= target_size:
        out = img_u8 if _U8_ROUND_TRIP_IS_IDENTITY else _U8_ROUND_TRIP[img_u8]
        if out.shape[0] == out.shape[1]:
            lit = (out[..., 0] | out[..., 1] | out[..., 2]) != 0     # == out.any(axis=-1), ten times faster
            first, last = _trim_rows(np.mean(lit, axis=-1) > 0.85)
            out = out[first:last]
        return np.ascontiguousarray(out)
    if model is not None:
        import torch
        dev_img = torch.from_numpy(np.ascontiguousarray(img_u8)).to(model.device)
        out_dev, lit_dev = model.preprocess_u8(dev_img, target_size, target_size)
        out, lit = out_dev.cpu().numpy(), lit_dev.cpu().numpy()
        first, last = _trim_rows(lit / np.float64(target_size) > 0.85)          # np.mean of booleans: float64 count / n
        return np.ascontiguousarray(out[first:last])
    image = resize_bicubic_reflect(img_u8.astype(np.float32) / np.float32(255), target_size, target_size)
    if image.shape[0] == image.shape[1]:
        image = trim_black(image)
    return _float_to_u8(image)


def _bmp24_layout(head: bytes, size: int):
    """(pixel offset, width, rows, row stride, bottom_up) of an uncompressed 24-bit BMP from its first 54 bytes and
    the file size; None for any other flavour."""
    import struct
    if len(head) < 54 or head[:2] != b"BM":
        return None
    off, = struct.unpack_from("<I", head, 10)
    hdr, w, h, planes, bpp, comp = struct.unpack_from("<IiiHHI", head, 14)
    if hdr < 40 or planes != 1 or bpp != 24 or comp != 0 or w <= 0 or h == 0:
        return None
    rows, stride = abs(h), (w * 3 + 3) & ~3
    if off + stride * rows > size:
        return None
    return off, w, rows, stride, h > 0


def _decode_bmp24(buf: bytes):
    """Uncompressed 24-bit BMP (what the scanner writes, predict.py:15-17) straight into an RGB array: three
    strided numpy copies (which drop the GIL) instead of PIL's decoder loop; None for any other flavour."""
    lay = _bmp24_layout(buf[:54], len(buf))
    if lay is None:
        return None
    off, w, rows, stride, bottom_up = lay
    a = np.frombuffer(buf, np.uint8, stride * rows, off).reshape(rows, stride)[:, : w * 3].reshape(rows, w, 3)
    if bottom_up:
        a = a[::-1]                                  # bottom-up rows
    out = np.empty((rows, w, 3), dtype=np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = a[..., 2], a[..., 1], a[..., 0]     # BGR -> RGB
    return out


def _decode_rgb(path: str) -> np.ndarray:
    """pil_loader (dataset.py:82-90): the file as an RGB uint8 array (own, contiguous copy)."""
    import io
    from PIL import Image
    with open(path, "rb") as f:
        buf = f.read()
    img = _decode_bmp24(buf)
    if img is None:
        img = np.array(Image.open(io.BytesIO(buf)).convert("RGB"))
    return img


_pinned = threading.local()      # one pinned read buffer per pool thread (allocated on first use, grown on demand)


def preprocess_bmp_scan_on_device(path: str, target_size: int, model, lock) -> Optional[np.ndarray]:
    """models.py:173-203 for one raw scan that needs the resize, without touching its pixels on the host: the file
    is read straight into pinned memory, the pixel array goes to the device as the scanner stored it (BGR,
    bottom-up, padded rows), is put into RGB top-down order there and runs through ``nbc_preprocess_u8``; only the
    1024 x 1024 result comes back.  Same bytes as ``preprocess_image(_decode_rgb(path), target_size, model)``; a
    4096 x 4096 scan takes 20-30 ms of a pool thread instead of 150.  None when the file is not an uncompressed
    24-bit BMP or is small enough to need no resize (the caller then takes the host route)."""
    import torch
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        lay = _bmp24_layout(f.read(54), size)
        if lay is None or max(lay[1], lay[2]) <= target_size:
            return None
        off, w, rows, stride, bottom_up = lay
        buf = getattr(_pinned, "buf", None)
        if buf is None or buf.numel() < size:
            buf = _pinned.buf = torch.empty(size + (size >> 3), dtype=torch.uint8).pin_memory()
        f.seek(0)
        if f.readinto(buf.numpy()[:size]) != size:
            return None
    with lock:                                       # one context, one stream: device work of the pool is serialised
        raw = buf[off: off + stride * rows].to(model.device, non_blocking=True)
        img = raw.view(rows, stride)[:, : w * 3].reshape(rows, w, 3)
        if bottom_up:
            img = img.flip(0)
        img = img.flip(2).contiguous()               # BGR -> RGB
        out_dev, lit_dev = model.preprocess_u8(img, target_size, target_size)
        out, lit = out_dev.cpu().numpy(), lit_dev.cpu().numpy()      # .cpu() waits for the stream: buf is free again
    first, last = _trim_rows(lit / np.float64(target_size) > 0.85)
    return np.ascontiguousarray(out[first:last])


def _png_level(kind: str) -> int:
    """zlib level of the PNGs the driver writes.  The files carry pixel values (models.py:203,349-356 pin
    values, not bytes): processed frames default to stored (level 0: noise-like photographs barely
    compress and deflate costs 100 ms per 1024x1024 frame), label maps to level 1 (a few ms, 20x smaller)."""
    return int(os.environ.get("NBC_PNG_LEVEL_" + kind.upper(), "0" if kind == "processed" else "1"))


def preprocess_images(root: str, target_size: int = 1024, model=None) -> None:
    """models.py:173-203 as a stand-alone pass (``--only_preprocess``): decode, resize / trim, save as PNG
    under processed/, on a thread pool; a device resize, when ``model`` is given, is serialised."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    from .pngio import write_png
    lock = threading.Lock()

    def one(item):
        path, name, wood = item
        out = preprocess_bmp_scan_on_device(path, target_size, model, lock) if model is not None else None
        if out is None:
            img = _decode_rgb(path)
            if model is not None and max(img.shape[:2]) > target_size:
                with lock:
                    out = preprocess_image(img, target_size, model)
            else:
                out = preprocess_image(img, target_size)
        write_png(os.path.join(root, "processed", "samples", wood, name), out, _png_level("processed"))

    with ThreadPoolExecutor(max_workers=_host_workers()) as pool:
        list(pool.map(one, list_images(root)))


def stats_row(name: str, wood: str, h: int, w: int, count_1: int, count_2: int) -> List[str]:
    """One CSV row, float32 arithmetic and '{:.5f}' formatting of models.py:321-332."""
    row = [name, wood]
    pixels = np.float32(h * w)
    for c in (count_1, count_2):
        frac = np.float32(c) / pixels                 # (outputs == c).float().mean(): exact sum / N in f32
        row.append("{:.5f}".format(float(frac * np.float32(100))))
        row.append("{:.5f}".format(float(np.float32(c) * np.float32(MM2_PER_PIXEL))))
    return row


def write_stats_csv(path: str, rows: Sequence[Sequence[str]]) -> None:
    with open(path, "w") as f:                       # models.py:360-364 (no newline='' there either)
        csv.writer(f, delimiter="\t").writerows([CSV_HEADER] + [list(r) for r in rows])


def write_dropout_report(results_dir: str, items, allrows, alld, draws: int, p: float, seed: int, precision: str, bn_stats: str,
                         old_stats=None, compare_path: str = None, allv=None) -> dict:
    """``dropout_stats.csv`` (tab separated) and ``dropout_summary.json`` from the gathered rows: ``allrows`` as
    ``final_stats.csv`` is written from, ``alld`` the ``(global_idx, D x 3 counts)`` rows of the draws.  ``allv``
    (``--dropout_votes``): the ``(global_idx, 10 stats, changed)`` rows of the votes, which make ``dropout_votes.csv``
    (``folder_run.vote_report``) and the summary's ``"votes"`` entry.  Returns the summary."""
    import json
    by_idx = {int(g[0]): g[1:].reshape(draws, 3) for g in alld}
    images = [(items[int(g[0])]["name"], items[int(g[0])]["wood"], int(g[1]), int(g[2]), int(g[3]), int(g[4]), by_idx[int(g[0])])
              for g in allrows]
    table, summary = folder_run.dropout_report(images, draws, old_stats)
    with open(os.path.join(results_dir, "dropout_stats.csv"), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    summary = dict({"p": float(p), "seed": int(seed), "precision": precision, "bn_stats": bn_stats}, **summary)
    if compare_path is not None:
        summary["compare"]["file"] = os.path.basename(compare_path)
    if allv is not None:
        by_idx = {int(g[0]): g[1:] for g in allv}
        vimages = [(items[int(g[0])]["name"], items[int(g[0])]["wood"], int(g[1]), int(g[2]),
                    by_idx[int(g[0])][:folder_run.VOTE_STATS], int(by_idx[int(g[0])][folder_run.VOTE_STATS])) for g in allrows]
        vtable, vsummary = folder_run.vote_report(vimages, draws)
        with open(os.path.join(results_dir, "dropout_votes.csv"), "w") as f:
            csv.writer(f, delimiter="\t").writerows(vtable)
        summary["votes"] = vsummary["means"]
    with open(os.path.join(results_dir, "dropout_summary.json"), "w") as f:
        json.dump(summary, f, indent=2, sort_keys=True)
        f.write("\n")
    return summary


def write_tta_report(results_dir: str, items, allrows, allt, views: int, precision: str, bn_stats: str) -> dict:
    """``tta_stats.csv`` (tab separated) and ``tta_summary.json`` from the gathered rows: ``allrows`` as ``final_stats.csv`` is
    written from (the merged labels' counts), ``allt`` the ``(global_idx, merged counts 3, V x 3 view counts, 10 vote
    statistics)`` rows of ``--tta``.  Returns the summary."""
    return _write_views_report(results_dir, "tta", items, allrows, allt, len(folder_run.tta_view_names(views)),
                               lambda images: folder_run.tta_report(images, views), precision, bn_stats)


def write_jitter_report(results_dir: str, items, allrows, allt, factors, precision: str, bn_stats: str) -> dict:
    """``jitter_stats.csv`` (tab separated) and ``jitter_summary.json`` from the gathered rows, as ``write_tta_report`` writes
    its two files: ``allt`` the ``(global_idx, the mean's counts 3, V x 3 view counts, 10 vote statistics)`` rows of ``--jitter``,
    ``factors`` the float32 ``[V,3]`` view set.  Returns the summary."""
    return _write_views_report(results_dir, "jitter", items, allrows, allt, len(factors),
                               lambda images: folder_run.jitter_report(images, factors), precision, bn_stats)


def _write_views_report(results_dir: str, stem: str, items, allrows, allt, nv: int, report, precision: str, bn_stats: str) -> dict:
    """``<stem>_stats.csv`` and ``<stem>_summary.json`` of a run over ``nv`` views; ``report(images)``: the table and summary."""
    import json
    by_idx = {int(g[0]): g[1:] for g in allt}
    images = []
    for g in allrows:
        t = by_idx[int(g[0])]
        images.append((items[int(g[0])]["name"], items[int(g[0])]["wood"], int(g[1]), int(g[2]), t[:3], t[3: 3 + 3 * nv].reshape(nv, 3),
                       t[3 + 3 * nv:]))
    table, summary = report(images)
    with open(os.path.join(results_dir, stem + "_stats.csv"), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    summary = dict({"precision": precision, "bn_stats": bn_stats}, **summary)
    with open(os.path.join(results_dir, stem + "_summary.json"), "w") as f:
        json.dump(summary, f, indent=2, sort_keys=True)
        f.write("\n")
    return summary


def write_windows_report(results_dir: str, items, allrows, allw, windows, precision: str) -> dict:
    """``windows_stats.csv`` (tab separated) and ``windows_summary.json`` from the gathered rows: ``allrows`` as
    ``final_stats.csv`` is written from (the merged labels' counts), ``allw`` the ``(global_idx, merged counts 3, the plain
    forward's counts 3, changed pixels)`` rows of ``--windows``; ``windows``: what ``folder_run.check_windows_arguments``
    returned.  Returns the summary."""
    import json
    from .model import window_grid
    by_idx = {int(g[0]): g[1:] for g in allw}
    images = []
    for g in allrows:
        t, h, w = by_idx[int(g[0])], int(g[1]), int(g[2])
        images.append((items[int(g[0])]["name"], items[int(g[0])]["wood"], h, w, window_grid(h, w, windows.window, windows.stride)[:4],
                       t[:3], t[3:6] if windows.compare else None, int(t[6]) if windows.compare else None))
    table, summary = folder_run.windows_report(images, windows.window, windows.stride, windows.blend, windows.compare)
    with open(os.path.join(results_dir, "windows_stats.csv"), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    summary = dict({"precision": precision}, **summary)
    with open(os.path.join(results_dir, "windows_summary.json"), "w") as f:
        json.dump(summary, f, indent=2, sort_keys=True)
        f.write("\n")
    return summary


def write_zones_report(results_dir: str, items, allrows, allz, cap: int, host_fallbacks: int) -> dict:
    """``zones.csv``, ``zones_summary.csv`` (tab separated, like ``final_stats.csv``) and ``zones_summary.json`` from the
    gathered rows: ``allrows`` as ``final_stats.csv`` is written from (one per image: its size), ``allz`` the
    ``(global_idx, 10 zone fields)`` rows of every zone, an image's rows in first-pixel order.  Returns the summary."""
    import json
    from . import zones as zn
    allz = np.asarray(allz, dtype=np.int64).reshape(-1, 1 + zn.ZONE_ROW)
    starts = np.searchsorted(allz[:, 0], [int(g[0]) for g in allrows], side="left")
    ends = np.searchsorted(allz[:, 0], [int(g[0]) for g in allrows], side="right")
    table, summary, figures = [list(zn.ZONE_COLUMNS)], [list(zn.SUMMARY_COLUMNS)], []
    for g, a, b in zip(allrows, starts, ends):
        d, h, w, z = items[int(g[0])], int(g[1]), int(g[2]), allz[a:b, 1:]
        table += zn.zone_rows(d["name"], d["wood"], h, w, z)
        summary += zn.summary_rows(d["name"], d["wood"], h, w, z)
        figures.append(zn.image_figures(h, w, z))
    for name, rows_ in (("zones.csv", table), ("zones_summary.csv", summary)):
        with open(os.path.join(results_dir, name), "w") as f:
            csv.writer(f, delimiter="\t").writerows(rows_)
    doc = zn.folder_summary(figures, cap, host_fallbacks)
    with open(os.path.join(results_dir, "zones_summary.json"), "w") as f:
        json.dump(doc, f, indent=2, sort_keys=True)
        f.write("\n")
    return doc


def check_confidence_arguments(confidence: bool, confidence_threshold=None, dropout_draws=None, only_preprocess: bool = False) -> None:
    """``ValueError`` for what ``--confidence`` and its option refuse before any device is touched: the threshold without the
    flag or outside (0, 1], and the flag with ``--dropout_draws`` or ``--only_preprocess``."""
    from . import calibration as cal
    if not confidence:
        if confidence_threshold is not None:
            raise ValueError("--confidence_threshold needs --confidence")
        return
    if dropout_draws:
        raise ValueError("--confidence describes the plain forward: it does not go with --dropout_draws")
    if only_preprocess:
        raise ValueError("--confidence needs the forward: it does not go with --only_preprocess")
    if confidence_threshold is not None:
        cal.check_confidence_threshold(confidence_threshold)


def write_confidence_report(results_dir: str, items, allrows, all_wire, pooled, threshold: float, precision: str, bn_stats: str) -> dict:
    """``confidence_stats.csv`` (tab separated) and ``confidence_summary.json`` from the gathered rows: ``allrows`` as
    ``final_stats.csv`` is written from, ``all_wire`` the ``(global_idx, pixels below the threshold, calibration.wire_rows
    fields)`` rows, ``pooled`` the folder's census row.  Returns the summary."""
    import json
    from . import calibration as cal
    width = cal.wire_width()
    wire = {int(g[0]): g[1:] for g in np.asarray(all_wire, dtype=np.int64).reshape(-1, 2 + width)}
    table, hard_total = [list(cal.CONFIDENCE_COLUMNS)], [0, 0, 0]
    for g in allrows:
        d, pixels, c1, c2 = items[int(g[0])], int(g[1]) * int(g[2]), int(g[3]), int(g[4])
        hard = [pixels - c1 - c2, c1, c2]
        hard_total = [a + b for a, b in zip(hard_total, hard)]
        w = wire[int(g[0])]
        table += cal.confidence_rows_of_wire(d["name"], d["wood"], cal.figures_of_wire(w[1:]), int(w[0]), hard)
    with open(os.path.join(results_dir, "confidence_stats.csv"), "w") as f:
        csv.writer(f, delimiter="\t").writerows(table)
    summary = dict(cal.confidence_summary(pooled, len(allrows), threshold, hard_total), precision=precision, bn_statistics=bn_stats)
    with open(os.path.join(results_dir, "confidence_summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return summary


def label_png(labels: np.ndarray) -> np.ndarray:
    """models.py:349-353: uint8 map with Bark = 127, Node = 255."""
    out = np.zeros(labels.shape, dtype=np.uint8)
    out[labels == 1] = 127
    out[labels == 2] = 255
    return out


def plan_items(root: str) -> List[dict]:
    """What the reference's two passes end up predicting, in its order: every file that will exist under
    processed/samples/<wood>/ once the preprocessor has run (models.py:173-189 writes
    ``fname.replace("bmp", "png")`` for each sample, a later sample of the same output name overwriting an
    earlier one; files already there stay), listed like dataset.py:41-68 lists them."""
    by_key = {}
    for path, name, wood in list_images(root):
        by_key[(wood, name)] = {"name": name, "wood": wood, "src": path}
    pdir = os.path.join(root, "processed")
    if os.path.isdir(os.path.join(pdir, "samples")):
        for path, name, wood in list_images(pdir):
            key = (wood, name.replace("bmp", "png"))
            if key not in by_key:                      # stale processed file without a sample: predicted as it is
                by_key[key] = {"name": key[1], "wood": wood, "src": None, "processed": path}
    order = {w: i for i, w in enumerate(WOOD_TYPES)}
    items = sorted(by_key.values(), key=lambda d: (order[d["wood"]], d["name"]))
    for d in items:
        d.setdefault("processed", os.path.join(pdir, "samples", d["wood"], d["name"]))
    return items


def predict_folder(root: str, model_path: str = "./best_model.pt", precision: str = "fp32",
                   exclude_nodes: bool = False, small_zones: bool = True, device_index: int = None,
                   batch: int = None, window: int = 64, target_size: int = 1024, autotune: bool = False, calibrate: bool = True,
                   streams: int = None, arch: str = "auto", bn_stats: str = "running", precision_auto: bool = False,
                   normalization=None, dropout_draws: int = 0, dropout_p: float = 0.1, dropout_seed: int = 0,
                   dropout_compare: str = None, dropout_votes: bool = False, zones: bool = False, zones_cap: int = None,
                   tta="none", tta_votes: bool = False, confidence: bool = False, confidence_threshold: float = None,
                   jitter=None, jitter_views=None, jitter_votes: bool = False, windows: int = None, windows_stride: int = None,
                   windows_blend: str = None, windows_compare: bool = False, logit_offsets=None) -> dict:
    """predict.py:51-58 + models.py:230-364 with the model call on the MI355X path.

    One pass per image instead of the reference's two (preprocess everything, then predict everything):
    a rank decodes and preprocesses its own images on a host thread pool (writing processed/ as the
    reference does), hands the uint8 frames to the GPU in windows of ``window`` images while the pool
    already works on the next window, runs equal-sized frames of a window as batches of up to ``batch``,
    and writes each label PNG from the pool as soon as its labels are on the host (pinned ring,
    asynchronous copies).  ``streams`` batches are in flight at once, each on its own HIP stream and model
    object (``clone_shared``: one copy of the weights): a scan of 520-730 rows leaves the last round of tiles of
    many layers a quarter full, and the next image's kernels fill it (measured at batch 1 in f32: 154 -> 222
    images/s at 528 rows, 146 -> 168 at 720, 118 -> 119 at 1024; default 4).  Every shape runs on the library's default per-layer tiles (a cost model that
    lands within 0.1-0.5 % of the measured best in f32); ``autotune=True`` measures them once per distinct
    full-batch shape instead, which costs 0.5-0.9 s per shape and pays only for many thousands of images of one
    shape.  In "f16x2" mode ``calibrate`` (default) runs the first image once with every activation kept and leaves with
    ``NonFiniteLogits`` -- before any batch -- when a stored tensor lies outside the range the f16 pieces hold at f32 grade
    (``FCNResNet50.activation_peaks``: the silent counterpart of the non-finite word, which still rides back with every batch).
    ``arch`` (``resolve_arch``): the network, ``"auto"`` = the one the checkpoint's keys name.  ``bn_stats``: ``"running"``
    (eval mode), ``"image"``, the per-image BatchNorm statistics the shipped tool ran with ("fp32", FCN only) or
    ``"image_f16x2"``, the same on the f16x2 pipe ("f16x2", FCN only:
    ``resolve_bn_stats``, ``check_bn_stats_arch``).  EfficientNet networks run "fp32" (``resolve_arch_precision``;
    ``precision_auto``: ``precision`` came from ``--precision auto``).  ``normalization``: the ``(mean, std)`` the frames are
    normalised with (``--mean`` / ``--std`` / ``--stats``, ``folder_run.resolve_normalization``), set on every stream's model
    object, the calibration guard's included; None: the defaults of models.py:208-209.
    ``dropout_draws`` = D > 0 (fcn_resnet50 only): after each batch's forward, on its stream and model object, D draws of the
    live ``Dropout(dropout_p)`` the shipped tool ran with (``FCNResNet50.dropout_draws`` under ``dropout_seed``, each image
    under its ``folder_run.image_id``, with this run's ``small_zones`` and ``exclude_nodes``); their counts ride back beside
    the labels and rank 0 writes ``results/dropout_stats.csv`` and ``results/dropout_summary.json``
    (``folder_run.dropout_report``; ``dropout_compare``: a ``final_stats.csv`` of the shipped tool to place within the draws).
    Everything else the run writes is byte for byte what it writes without the draws.
    ``dropout_votes`` (with ``dropout_draws`` only): the draws run through ``FCNResNet50.dropout_votes``, whose per-pixel
    majority mask and support byte ride back beside the labels: ``results/dropout_votes/<wood>/<name>`` (the mask, written as
    the label PNGs are), ``results/dropout_support/<wood>/<name>`` (grey, 255 = every draw agrees),
    ``results/dropout_votes.csv`` (``folder_run.vote_report``, with the pixels on which the mask differs from the label PNG)
    and a ``"votes"`` entry in ``dropout_summary.json``; every other file stays byte for byte what it is without the flag.
    ``zones``: after ``predict_labels``, on the same stream and model object, ``FCNResNet50.label_zones`` inventories the
    final label maps (after ``remove_small_zones`` and the ``exclude_nodes`` remap): up to ``zones_cap`` (default 1024) rows
    per image ride back beside the labels; an image with more zones gets its rows from ``zones.zones_cpu`` on the label plane
    already on the host.  Rank 0 writes ``results/zones.csv`` (a row per zone), ``results/zones_summary.csv`` (a row per
    image) and ``results/zones_summary.json`` (``write_zones_report``); every other file stays byte for byte what it is
    without the flag.  The returned dict gains ``zones_host_fallbacks``, this rank's images that took the host path, and ``zones_report_s``, the
    seconds the gather and (on rank 0) the three files took after the loop.
    ``tta`` ("hflip", "vflip", "flips"; "none" = off; not with ``dropout_draws``): ``FCNResNet50.predict_labels_tta`` stands where
    ``predict_labels`` does, so the label PNGs, ``final_stats.csv`` and ``zones`` are those of the mean of the flip views
    (DESIGN.md 3.15).  ``batch`` keeps counting images (default 1, 2 in bf16): the forward runs V x batch entries.  Each view's
    own counts and the vote statistics over the views ride back beside the labels; rank 0 writes ``results/tta_stats.csv``
    and ``results/tta_summary.json`` (``folder_run.tta_report``).  ``tta_votes`` (with ``tta`` only): also
    ``results/tta_support/<wood>/<name>``, the support byte of the views' vote (grey, 255 = every view agrees).
    ``logit_offsets`` = ``(bark, node)`` (not with ``dropout_draws`` or ``confidence``): every stream's model decides by
    ``argmax(x0, x1 + bark, x2 + node)`` (``FCNResNet50.set_logit_offsets``); the label PNGs, the percentages, ``--zones`` and the
    views' merges all see that decision.
    ``confidence`` (not with ``dropout_draws``): the forward also writes its full-resolution logits, and
    ``FCNResNet50.softmax_census`` (no target, the plane on) leaves the softmax confidence of the plain forward, which costs no
    further forward: ``results/confidence/<wood>/<name>`` (grey, the winning class's probability in 1/256: the raw softmax,
    before ``remove_small_zones`` and the ``exclude_nodes`` remap), ``results/confidence_stats.csv``
    (``calibration.CONFIDENCE_COLUMNS``: the mean confidence, the share and mm2 of the pixels below ``confidence_threshold``
    -- default 0.9 --, expected Bark / Node % and mm2 beside the hard ones) and ``results/confidence_summary.json``.
    ``final_stats.csv`` and the label PNGs stay byte for byte what they are without the flag.
    ``jitter`` ("training") or ``jitter_views`` (1..16 (brightness, contrast, saturation) triples, or the string of
    ``--jitter_views``; not with ``tta`` or ``dropout_draws``): ``FCNResNet50.predict_labels_jitter`` stands where
    ``predict_labels`` does, so the label PNGs, ``final_stats.csv`` and ``zones`` are those of the mean of the colour-jitter views
    (DESIGN.md 3.17).  ``batch`` keeps counting images (default 1, 2 in bf16).  Rank 0 writes ``results/jitter_stats.csv`` and
    ``results/jitter_summary.json`` (``folder_run.jitter_report``: ``tta_stats.csv``'s columns under the views' names).
    ``jitter_votes`` (with a view set only): also ``results/jitter_support/<wood>/<name>``, the support byte of the views' vote.
    ``windows`` = S (with ``windows_stride``, default S / 2 rounded down to a multiple of 8, and ``windows_blend`` "tent" or
    "uniform"; not with ``tta``, ``jitter``, ``dropout_draws`` or per-image ``bn_stats``; ResNet-50 networks only):
    ``FCNResNet50.predict_labels_windows`` stands where ``predict_labels`` does, so the label PNGs, ``final_stats.csv`` and
    ``zones`` are those of the blended S x S windows.  ``batch`` keeps counting images (default 1, 2 in bf16).
    Rank 0 writes ``results/windows_stats.csv`` and ``results/windows_summary.json`` (``folder_run.windows_report``).
    ``windows_compare``: the plain forward of each frame runs as well; its counts and the pixels on which the two final label
    maps differ (the off-diagonal of ``FCNResNet50.confusion``) ride back and fill the report's comparison columns.
    Returns timing / count statistics of this rank."""
    import time
    import torch
    from PIL import Image
    from . import zones as zn
    from .model import FCNResNet50
    from .pngio import write_png
    D = int(dropout_draws or 0)
    V = bool(dropout_votes)
    Z = bool(zones)
    folder_run.check_zones_arguments(Z, zones_cap)   # refusals first: nothing has touched a device yet
    ZCAP = int(zones_cap) if zones_cap is not None else zn.DEFAULT_CAP
    T = folder_run.check_tta_arguments(tta, tta_votes, D)   # the view mask, 0 = off
    J = folder_run.check_jitter_arguments(jitter, jitter_views, jitter_votes, tta, D)   # the colour views' factors, None = off
    NV = len(J) if J is not None else len(folder_run.tta_view_names(T))
    TS = bool(tta_votes) or bool(jitter_votes)
    VIEWS = bool(T) or J is not None                 # the forward runs a stack of views: the flip views or the colour views
    SUPPORT = "jitter_support" if J is not None else "tta_support"
    WN = folder_run.check_windows_arguments(windows, windows_stride, windows_blend, windows_compare, tta, jitter, jitter_views, D,
                                            bn_stats=bn_stats, arch=arch)   # the crop windows, None = off
    from . import calibration as cal
    C = bool(confidence)
    check_confidence_arguments(C, confidence_threshold, D)
    LO = folder_run.check_logit_offsets(logit_offsets, D, C)
    CT = cal.check_confidence_threshold(confidence_threshold) if confidence_threshold is not None else cal.DEFAULT_CONFIDENCE_THRESHOLD
    old_stats = None
    if V and not D:
        raise ValueError("--dropout_votes needs --dropout_draws")
    if D:                                            # refusals first: nothing has touched a device yet
        folder_run.check_dropout_arguments(D, dropout_p, dropout_seed, dropout_compare, arch)
        if dropout_compare is not None:
            old_stats = folder_run.read_shipped_stats(dropout_compare)
    r = folder_run.open_run(root, "predict", precision, device_index, batch, streams, target_size, stack=max(NV, 1), windows=WN)
    dev, batch, prof, clock = r.dev, r.batch, r.prof, time.perf_counter
    pre_model = FCNResNet50(precision).to(dev)      # its own context: the pool's device resizes never touch the predictor's

    def warm(m):                                     # the remove_small_zones workspace (9 bytes per pixel; --tta: of the views' stack)
        if small_zones:
            m.remove_small_zones(torch.zeros((batch * r.stack, target_size, target_size), dtype=torch.uint8, device=dev))
        if Z:                                        # and label_zones' (5 bytes per pixel)
            m.label_zones(torch.zeros((batch, target_size, target_size), dtype=torch.uint8, device=dev), cap=ZCAP)
        if C:
            m.softmax_census(torch.zeros((batch, 3, target_size, target_size), dtype=torch.float32, device=dev), confidence=True)
    folder_run.bring_up(r, model_path, arch, bn_stats, precision_auto,
                        lambda root_: generate_folders(root_, votes=V, tta_votes=bool(tta_votes), confidence=C,
                                                       jitter_votes=bool(jitter_votes)), warm, normalization=normalization,
                        logit_offsets=LO)
    if D:
        folder_run.check_dropout_arch(r.arch)        # --arch auto: the checkpoint's keys have named the network by now

    items = plan_items(root)

    def header_size(d):
        with open(d["src"] or d["processed"], "rb") as f:
            w, h = Image.open(f).size                # header only: nothing is decoded
        return h, w
    folder_run.shard(r, items, header_size)
    mine, pool = r.mine, r.pool
    rows = np.zeros((len(mine), ROW_WIDTH), dtype=np.int64)
    drows = np.zeros((len(mine), 1 + 3 * D), dtype=np.int64)     # (global_idx, D x 3 counts) of the Dropout draws
    VROW = 2 + folder_run.VOTE_STATS
    vrows = np.zeros((len(mine), VROW), dtype=np.int64)          # (global_idx, 10 vote statistics, changed pixels)
    TROW = 1 + 3 + 3 * NV + folder_run.VOTE_STATS
    trows = np.zeros((len(mine), TROW), dtype=np.int64)          # (global_idx, merged counts, V x 3 view counts, 10 vote statistics)
    CROW = 2 + cal.wire_width()
    crows = np.zeros((len(mine), CROW), dtype=np.int64)          # (global_idx, pixels below the threshold, calibration.wire_rows)
    WROW = 1 + 3 + 3 + 1
    wrows = np.zeros((len(mine), WROW), dtype=np.int64)          # (global_idx, merged counts, the plain forward's counts, changed pixels)
    cpool = np.zeros(cal.WORDS, dtype=np.uint64)                 # this rank's pooled census (--confidence)
    zrows = {}                                       # k -> the image's zone rows int64 [zones, 10] (--zones)
    zfallbacks = []                                  # the k whose rows came from the host: more zones than ZCAP
    resize_lock = threading.Lock()                   # the default stream is the pool's: its device resizes are serialised
    lvl_proc, lvl_lab = _png_level("processed"), _png_level("labels")

    def prepare(k):
        """Pool: decode + preprocess + write processed/ -> the uint8 frame the model sees."""
        d = items[mine[k]]
        t0 = clock()
        if d["src"] is None:
            return (_decode_rgb(d["processed"]),)
        out = preprocess_bmp_scan_on_device(d["src"], target_size, pre_model, resize_lock)     # raw scans: no host decode
        t1 = t2 = clock()
        if out is None:
            img = _decode_rgb(d["src"])
            t1 = clock()
            if max(img.shape[:2]) > target_size:
                with resize_lock:
                    out = preprocess_image(img, target_size, pre_model)
            else:
                out = preprocess_image(img, target_size)
            t2 = clock()
        write_png(d["processed"], out, lvl_proc)
        t3 = clock()
        prof["pool.decode"] += t1 - t0; prof["pool.preprocess"] += t2 - t1; prof["pool.write_processed"] += t3 - t2
        return (out,)

    label_paths = []                                 # label PNGs this rank has written (removed again if the run turns out invalid)

    def finish(k, lab, c1, c2, draws=None, votes=None, zone=None, views=None, conf=None, win=None):
        """Pool: label PNG (models.py:349-356) + the image's row (+ the vote mask and support PNGs and the votes' row; + the
        zone rows: ``zone`` = (the device's rows, or None when the image has more zones than the cap: the host computes them);
        + the confidence PNG: ``conf`` = the plane)."""
        d = items[mine[k]]
        t0 = clock()
        path = os.path.join(root, "results", "outputs", d["wood"], d["name"])
        label_paths.append(path)
        write_png(path, label_png(lab), lvl_lab)
        rows[k] = (mine[k], lab.shape[0], lab.shape[1], c1, c2)
        if draws is not None:
            drows[k, 0], drows[k, 1:] = mine[k], draws.reshape(-1)
        if votes is not None:
            vlab, sup, vstats = votes
            for level, img in (("dropout_votes", label_png(vlab)), ("dropout_support", sup)):
                vpath = os.path.join(root, "results", level, d["wood"], d["name"])
                label_paths.append(vpath)
                write_png(vpath, img, lvl_lab)
            vrows[k, 0], vrows[k, 1:-1], vrows[k, -1] = mine[k], vstats, int(np.count_nonzero(vlab != lab))
        if views is not None:                        # --tta / --jitter: (merged counts, the views' counts, the vote statistics, the support plane or None)
            mcounts, vcounts, tstats, sup = views
            trows[k, 0], trows[k, 1:4], trows[k, 4: 4 + 3 * NV], trows[k, 4 + 3 * NV:] = mine[k], mcounts, vcounts.reshape(-1), tstats
            if sup is not None:
                spath = os.path.join(root, "results", SUPPORT, d["wood"], d["name"])
                label_paths.append(spath)
                write_png(spath, sup, lvl_lab)
        if win is not None:                          # --windows: (merged counts, the plain forward's counts, changed pixels)
            wrows[k, 0], wrows[k, 1:4], wrows[k, 4:7], wrows[k, 7] = mine[k], win[0], win[1], win[2]
        if conf is not None:
            cpath = os.path.join(root, "results", "confidence", d["wood"], d["name"])
            label_paths.append(cpath)
            write_png(cpath, conf, lvl_lab)
        prof["pool.write_labels"] += clock() - t0
        if zone is not None:
            t1 = clock()
            if zone[0] is None:
                zfallbacks.append(k)
                zrows[k] = zn.zones_cpu(lab)[0]
            else:
                zrows[k] = zone[0]
            prof["pool.zones"] += clock() - t1

    # the result ring, one slot per staging slot: labels + counts coming back (pinned once for the largest batch)
    full = batch * target_size * target_size
    ring = [(torch.empty(full, dtype=torch.uint8).pin_memory(), torch.empty((batch, 3), dtype=torch.int64).pin_memory())
            for _ in range(r.depth)]
    dring = [torch.empty(D * batch * 3, dtype=torch.int64).pin_memory() for _ in range(r.depth)] if D else None
    # the votes' slots: the mask and the support plane, one after the other, and the ten statistics per image
    vring = [(torch.empty(2 * full, dtype=torch.uint8).pin_memory(),
              torch.empty((batch, folder_run.VOTE_STATS), dtype=torch.int64).pin_memory()) for _ in range(r.depth)] if V else None
    # the zones' slots: ZCAP rows per image and the zone counts
    zring = [(torch.empty((batch, ZCAP, zn.ZONE_ROW), dtype=torch.int64).pin_memory(), torch.empty(batch, dtype=torch.int64).pin_memory())
             for _ in range(r.depth)] if Z else None
    # --tta / --jitter: per slot the views' counts and the vote statistics per image, and (--tta_votes, --jitter_votes) the support planes
    tring = [(torch.empty((NV, batch, 3), dtype=torch.int64).pin_memory(),
              torch.empty((batch, folder_run.VOTE_STATS), dtype=torch.int64).pin_memory(),
              torch.empty(full if TS else 0, dtype=torch.uint8).pin_memory()) for _ in range(r.depth)] if VIEWS else None
    # --windows_compare: per slot the plain forward's counts and the confusion of the two final label maps per image
    wring = [(torch.empty((batch, 3), dtype=torch.int64).pin_memory(), torch.empty((batch, 3, 3), dtype=torch.int64).pin_memory())
             for _ in range(r.depth)] if WN is not None and WN.compare else None
    # --confidence: per stream the full-resolution logits; per slot the confidence planes and the census rows
    logits_buf = [torch.empty(3 * full, dtype=torch.float32, device=dev) for _ in range(r.n_streams)] if C else None
    cring = [(torch.empty(full, dtype=torch.uint8).pin_memory(), torch.empty((batch, cal.WORDS), dtype=torch.int64).pin_memory())
             for _ in range(r.depth)] if C else None
    tuned = set()
    forward, make_stack = folder_run.stacked_call(T, J, WN)   # the run's forward: plain, or on its views or windows

    def launch(slot, sid, part, x):
        (n, h, w), mdl = x.shape[:3], r.models[sid]
        need = n * h * w
        if ring[slot][0].numel() < need or ring[slot][1].shape[0] < n:   # an oversized stale processed frame (run_loop)
            ring[slot] = (torch.empty(need, dtype=torch.uint8).pin_memory(), torch.empty((n, 3), dtype=torch.int64).pin_memory())
        if autotune and (sid, (n, h, w)) not in tuned and n == batch and r.shape_count[tuple(x.shape[1:])] >= 2 * batch:
            mdl.autotune(make_stack(mdl, x))          # once per distinct full-batch shape and model object
            tuned.add((sid, (n, h, w)))
        lg = None
        if C:                                        # the forward writes its full-resolution logits as well
            lg = (logits_buf[sid][: 3 * need] if 3 * need <= logits_buf[sid].numel() else
                  torch.empty(3 * need, dtype=torch.float32, device=dev)).view(n, 3, h, w)
        kw = dict(exclude_nodes=exclude_nodes, labels_dtype=torch.uint8, small_zones=small_zones,   # models.py:269-276 on the device
                  **(dict(logits_full=lg) if C else {}))
        if VIEWS:                                   # the same tail on the mean of the views; the views' own figures beside it
            if tring[slot][0].shape[1] < n or (TS and tring[slot][2].numel() < need):
                tring[slot] = (torch.empty((NV, n, 3), dtype=torch.int64).pin_memory(),
                               torch.empty((n, folder_run.VOTE_STATS), dtype=torch.int64).pin_memory(),
                               torch.empty(need if TS else 0, dtype=torch.uint8).pin_memory())
            labels, counts, vcounts, sup, tstats, _ = forward(mdl, x, return_views=True, **kw)
            tring[slot][0][:, :n].copy_(vcounts, non_blocking=True)
            tring[slot][1][:n].copy_(tstats, non_blocking=True)
            if TS:
                tring[slot][2][:need].copy_(sup.reshape(-1), non_blocking=True)
        else:                                        # the plain forward, or the same tail on the blend of the windows
            labels, counts = forward(mdl, x, **kw)
            if WN is not None and WN.compare:        # the plain forward beside it: its counts and where its labels differ
                if wring[slot][0].shape[0] < n:
                    wring[slot] = (torch.empty((n, 3), dtype=torch.int64).pin_memory(), torch.empty((n, 3, 3), dtype=torch.int64).pin_memory())
                plabels, pcounts = mdl.predict_labels(x, exclude_nodes=exclude_nodes, labels_dtype=torch.uint8, small_zones=small_zones)
                wring[slot][0][:n].copy_(pcounts, non_blocking=True)
                wring[slot][1][:n].copy_(mdl.confusion(labels, plabels * 127), non_blocking=True)   # grey 0 / 127 / 254: classes 0 / 1 / 2
        ring[slot][0][:need].copy_(labels.reshape(-1), non_blocking=True)
        ring[slot][1][:n].copy_(counts, non_blocking=True)
        if C:                                        # the raw softmax of the forward: no target, the plane on
            if cring[slot][0].numel() < need or cring[slot][1].shape[0] < n:
                cring[slot] = (torch.empty(need, dtype=torch.uint8).pin_memory(), torch.empty((n, cal.WORDS), dtype=torch.int64).pin_memory())
            census, plane = mdl.softmax_census(lg, None, confidence=True)
            cring[slot][0][:need].copy_(plane.reshape(-1), non_blocking=True)
            cring[slot][1][:n].copy_(census.view(torch.int64), non_blocking=True)
        if Z:                                        # the labels are final here: after remove_small_zones and the remap
            if zring[slot][1].shape[0] < n:
                zring[slot] = (torch.empty((n, ZCAP, zn.ZONE_ROW), dtype=torch.int64).pin_memory(),
                               torch.empty(n, dtype=torch.int64).pin_memory())
            zr, znum = mdl.label_zones(labels, cap=ZCAP)
            zring[slot][0][:n].copy_(zr, non_blocking=True)
            zring[slot][1][:n].copy_(znum, non_blocking=True)
        if D:                                        # the draws read the features this forward left, on the same stream
            if dring[slot].numel() < D * n * 3:
                dring[slot] = torch.empty(D * n * 3, dtype=torch.int64).pin_memory()
            ids = [folder_run.image_id(items[mine[k]]["wood"], items[mine[k]]["name"]) for k in part]
            if V:
                if vring[slot][0].numel() < 2 * need or vring[slot][1].shape[0] < n:
                    vring[slot] = (torch.empty(2 * need, dtype=torch.uint8).pin_memory(),
                                   torch.empty((n, folder_run.VOTE_STATS), dtype=torch.int64).pin_memory())
                dcounts, vlab, sup, vstats = mdl.dropout_votes(D, ids, p=dropout_p, seed=dropout_seed, small_zones=small_zones,
                                                               exclude_nodes=exclude_nodes)
                vring[slot][0][:need].copy_(vlab.reshape(-1), non_blocking=True)
                vring[slot][0][need: 2 * need].copy_(sup.reshape(-1), non_blocking=True)
                vring[slot][1][:n].copy_(vstats, non_blocking=True)
            else:
                dcounts = mdl.dropout_draws(D, ids, p=dropout_p, seed=dropout_seed, small_zones=small_zones,
                                            exclude_nodes=exclude_nodes)
            dring[slot][: D * n * 3].copy_(dcounts.reshape(-1), non_blocking=True)

    def consume(slot, part, n, h, w):
        lab_host, cnt_host = ring[slot]
        labs = lab_host[: n * h * w].numpy().reshape(n, h, w).copy()
        cnts = cnt_host[:n].numpy().copy()
        dc = dring[slot][: D * n * 3].numpy().reshape(D, n, 3).copy() if D else None
        votes = zone = [None] * n
        if V:
            planes = vring[slot][0][: 2 * n * h * w].numpy().reshape(2, n, h, w).copy()
            vst = vring[slot][1][:n].numpy().copy()
            votes = [(planes[0, j], planes[1, j], vst[j]) for j in range(n)]
        if Z:                                        # (rows,) per image; (None,) = more zones than the cap: the host's turn
            znum = zring[slot][1][:n].numpy()
            zone = [(zring[slot][0][j, :int(znum[j])].numpy().copy() if znum[j] <= ZCAP else None,) for j in range(n)]
        views = [None] * n
        if VIEWS:
            vc, tst = tring[slot][0][:, :n].numpy().copy(), tring[slot][1][:n].numpy().copy()
            sups = tring[slot][2][: n * h * w].numpy().reshape(n, h, w).copy() if TS else [None] * n
            views = [(cnts[j], vc[:, j], tst[j], sups[j]) for j in range(n)]
        wins = [None] * n
        if WN is not None:
            pc = wring[slot][0][:n].numpy().copy() if WN.compare else np.zeros((n, 3), dtype=np.int64)
            cf = wring[slot][1][:n].numpy().copy() if WN.compare else np.zeros((n, 3, 3), dtype=np.int64)
            wins = [(cnts[j], pc[j], int(cf[j].sum() - np.trace(cf[j]))) for j in range(n)]
        confs = [None] * n
        if C:
            confs = cring[slot][0][: n * h * w].numpy().reshape(n, h, w).copy()
            census = cring[slot][1][:n].numpy()
            cpool[...] += cal.pool(census)
            wire = cal.wire_rows(census)
            for j, k in enumerate(part):
                crows[k, 0], crows[k, 1], crows[k, 2:] = mine[k], cal.below_threshold(census[j], CT), wire[j]
        return [pool.submit(finish, k, labs[j], int(cnts[j, 1]), int(cnts[j, 2]), dc[:, j] if D else None, votes[j], zone[j], views[j],
                            confs[j], wins[j]) for j, k in enumerate(part)]

    def remove_labels():                             # this rank's label PNGs of the invalid run: a crash before the rerun
        for path in label_paths:                     # must not leave them behind (the processed/ images do not depend on
            try:                                     # the arithmetic and stay)
                os.remove(path)
            except OSError:
                pass

    folder_run.run_loop(r, window, prepare, launch, consume, lambda: prepare(0)[0] if mine else None, calibrate,
                        on_abandon=remove_labels, abandon_note=" and its label PNGs removed")
    if os.environ.get("NBC_FOLDER_PROFILE"):
        print("rank %d stage seconds (pool stages summed over %d threads): %s; loop wall %.2f s" %
              (r.rank, r.workers, ", ".join("%s %.2f" % kv for kv in sorted(prof.items())), r.t_done - r.t_loop), flush=True)
    allrows = folder_run.gather(r, rows, ROW_WIDTH)
    if r.rank == 0:
        write_stats_csv(os.path.join(root, "results", "final_stats.csv"),
                        [stats_row(items[int(g[0])]["name"], items[int(g[0])]["wood"], int(g[1]), int(g[2]), int(g[3]), int(g[4]))
                         for g in allrows])
    if D:
        alld = folder_run.gather(r, drows, 1 + 3 * D)       # one more all_gather, as evaluate's --loss rows take
        allv = folder_run.gather(r, vrows, VROW) if V else None
        if r.rank == 0:
            write_dropout_report(os.path.join(root, "results"), items, allrows, alld, D, dropout_p, dropout_seed, r.precision,
                                 bn_stats, old_stats, dropout_compare, allv)
    if VIEWS:
        allt = folder_run.gather(r, trows, TROW)             # one more all_gather, as the draws' rows take
        if r.rank == 0 and T:
            write_tta_report(os.path.join(root, "results"), items, allrows, allt, T, r.precision, bn_stats)
        if r.rank == 0 and J is not None:
            write_jitter_report(os.path.join(root, "results"), items, allrows, allt, J, r.precision, bn_stats)
    if WN is not None:
        allw = folder_run.gather(r, wrows, WROW)             # one more all_gather, as the views' rows take
        if r.rank == 0:
            write_windows_report(os.path.join(root, "results"), items, allrows, allw, WN, r.precision)
    if C:                                            # a fixed-width row per image and one pooled census per rank
        allc = folder_run.gather(r, crows, CROW)
        census = cal.pool(folder_run.gather_ragged(np.concatenate([[r.rank], cpool.view(np.int64)])[None], r.world, r.dist, r.wire_dev,
                                                   width=1 + cal.WORDS)[:, 1:])
        if r.rank == 0:
            write_confidence_report(os.path.join(root, "results"), items, allrows, allc, census, CT, r.precision, bn_stats)
    extra = {}
    if Z:                                          # (global_idx, 10 zone fields) rows, an image's rows together and in order
        t_report = clock()
        local = [np.concatenate([np.full((len(zrows[k]), 1), mine[k], dtype=np.int64), zrows[k]], axis=1) for k in sorted(zrows)]
        local = np.concatenate(local) if local else np.zeros((0, 1 + zn.ZONE_ROW), dtype=np.int64)
        allz = folder_run.gather_ragged(local, r.world, r.dist, r.wire_dev, width=1 + zn.ZONE_ROW)
        fb = folder_run.gather(r, np.array([[mine[k]] for k in sorted(zfallbacks)], dtype=np.int64).reshape(-1, 1), 1)
        if r.rank == 0:
            write_zones_report(os.path.join(root, "results"), items, allrows, allz, ZCAP, len(fb))
        extra.update(zones_host_fallbacks=len(zfallbacks), zones_report_s=clock() - t_report)
    return dict(folder_run.finish(r), host_workers=r.workers, distinct_shapes=len(r.shape_count),
                autotuned_shapes=len({k for _, k in tuned}), **extra)


def main(argv=None):
    import sys
    ap = argparse.ArgumentParser(description="MI355X folder prediction (mirrors bark_calculator/predict.py)")
    ap.add_argument("root_path", metavar="DIR")
    ap.add_argument("--device", default="cuda:0", help="cuda:N (the CPU path is the reference itself)")
    ap.add_argument("--exclude_nodes", action="store_true")
    ap.add_argument("--only_preprocess", action="store_true")
    ap.add_argument("--no_small_zones", action="store_true")
    ap.add_argument("--autotune", action="store_true",
                    help="measure the conv tile shapes once per distinct full-batch image shape (0.5-0.9 s each) instead of the default choice")
    folder_run.add_shared_arguments(ap)
    folder_run.add_dropout_arguments(ap)
    folder_run.add_zones_arguments(ap)
    ap.add_argument("--tta_votes", action="store_true",
                    help="with --tta: also write results/tta_support/ (grey, 255 = every view gives the pixel the same label)")
    ap.add_argument("--jitter_votes", action="store_true",
                    help="with --jitter or --jitter_views: also write results/jitter_support/ (grey, 255 = every view gives the "
                         "pixel the same label)")
    ap.add_argument("--confidence", action="store_true",
                    help="also write the softmax confidence of the plain forward: results/confidence/ (grey, the winning class's "
                         "probability in 1/256, before remove_small_zones), results/confidence_stats.csv and "
                         "results/confidence_summary.json; no further forward")
    ap.add_argument("--confidence_threshold", type=float, default=None, metavar="P",
                    help="with --confidence: the pixels whose confidence lies below P are reported as a share and in mm2, "
                         "0 < P <= 1 (default 0.9)")
    raw = list(sys.argv[1:] if argv is None else argv)
    args = ap.parse_args(raw)
    folder_run.resolve_arguments(ap, args)
    try:                                                 # refused as argument errors, before any device is touched
        check_confidence_arguments(args.confidence, args.confidence_threshold, args.dropout_draws, args.only_preprocess)
        folder_run.check_tta_arguments(args.tta, args.tta_votes, args.dropout_draws, args.only_preprocess)
        folder_run.check_jitter_arguments(args.jitter, args.jitter_views, args.jitter_votes, args.tta, args.dropout_draws,
                                          args.only_preprocess)
        folder_run.check_windows_arguments(args.windows, args.windows_stride, args.windows_blend, args.windows_compare, args.tta,
                                           args.jitter, args.jitter_views, args.dropout_draws, args.only_preprocess, args.bn_stats,
                                           args.arch)
        folder_run.check_dropout_arguments(args.dropout_draws, args.dropout_p, args.dropout_seed, args.dropout_compare, args.arch,
                                           args.only_preprocess, args.dropout_votes)
        if args.dropout_compare is not None:
            folder_run.read_shipped_stats(args.dropout_compare)
        folder_run.check_zones_arguments(args.zones, args.zones_cap, args.only_preprocess)
        args.logit_offsets = folder_run.check_logit_offsets(args.logit_offsets, args.dropout_draws, args.confidence)
    except ValueError as e:
        ap.error(str(e))
    if not args.device.startswith("cuda"):
        raise SystemExit("this package is the MI355X path; run the reference for --device=cpu")
    if args.only_preprocess:                             # predict.py:53-55: the resize runs on the device here too
        from .model import FCNResNet50
        generate_folders(args.root_path, True)
        preprocess_images(args.root_path, model=FCNResNet50("fp32").to(args.device))   # a context for the resize kernel: no weights, no arithmetic mode involved
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, raw))
    idx = None
    if "WORLD_SIZE" not in os.environ and ":" in args.device:
        idx = int(args.device.split(":")[1])
    kw = dict(batch=args.batch, autotune=args.autotune, streams=args.streams, arch=args.arch, bn_stats=args.bn_stats)
    if args.dropout_draws:
        kw.update(dropout_draws=args.dropout_draws, dropout_p=0.1 if args.dropout_p is None else args.dropout_p,
                  dropout_seed=args.dropout_seed or 0, dropout_compare=args.dropout_compare, dropout_votes=args.dropout_votes)
    if args.zones:
        kw.update(zones=True, zones_cap=args.zones_cap)
    if args.tta != "none":
        kw.update(tta=args.tta, tta_votes=args.tta_votes)
    if args.jitter is not None or args.jitter_views is not None:
        kw.update(jitter=args.jitter, jitter_views=args.jitter_views, jitter_votes=args.jitter_votes)
    if args.windows is not None:
        kw.update(windows=args.windows, windows_stride=args.windows_stride, windows_blend=args.windows_blend,
                  windows_compare=args.windows_compare)
    if args.confidence:
        kw.update(confidence=True, confidence_threshold=args.confidence_threshold)
    if args.normalization is not None:
        kw["normalization"] = args.normalization
        if int(os.environ.get("RANK", "0")) == 0:
            print("predict: frames normalised with mean %s, std %s (%s)" % (
                list(args.normalization[0]), list(args.normalization[1]), args.stats or "arguments"), flush=True)
    if args.logit_offsets is not None:
        kw["logit_offsets"] = args.logit_offsets
        if int(os.environ.get("RANK", "0")) == 0:
            print("predict: labels decided by argmax(x0, x1 + %r, x2 + %r) (--logit_offsets)" % args.logit_offsets, flush=True)
    stats = folder_run.run_precision("predict", lambda precision, **over: predict_folder(
        args.root_path, args.model_path, precision, args.exclude_nodes, not args.no_small_zones, idx, **dict(kw, **over)),
        args.precision, args.bn_stats)
    if stats["rank"] == 0:
        print("predicted %(images_total)d images (%(images_this_rank)d on rank 0, %(batches)d batches): %(total_s).2f s, "
              "%(images_per_s_loop).1f images/s in the loop on this rank" % stats)


if __name__ == "__main__":
    main()
