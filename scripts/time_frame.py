#!/usr/bin/env python3
"""The training run's frame of `evaluate --frame training` on one GPU.
  --kernels     nbc_training_frame alone, by device events over back-to-back calls: one and two RGB scans of 640 x 1024 (a
                pure index map) and of 1023 x 1024 (the rows resampled) -> 1024 x 1024, and the grey duals of the same shapes --
                with the bytes each moves and the rate that makes, beside nbc_window_views on the same input
  --folder N    evaluate_folder on a synthetic labelled folder of N height-trimmed scans (heights cycling through --rows, 1024
                wide) with and without frame = "training", alternated, twice each: images/s end to end and in the loop
usage: python scripts/time_frame.py [--kernels] [--folder N] [--rows R ...] [--precision f16x2 ...]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import numpy as np
import torch

from neuralbarkcalculator_amd import synth
from neuralbarkcalculator_amd.model import FCNResNet50

HW = 1024


def _timed(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_kernels(reps=50):
    dev = torch.device("cuda", 0)
    m = FCNResNet50("fp32").to(dev)
    for rows in (640, 1023):
        for n in (1, 2):
            rgb = torch.from_numpy(np.stack([synth.make_frame(3 + i, rows, HW) for i in range(n)])).to(dev)
            grey = rgb[..., 1].contiguous()
            cases = [("nbc_training_frame RGB", lambda: m.training_frame(rgb, (HW, HW)), 3 * n * (rows * HW + HW * HW)),
                     ("nbc_training_frame grey", lambda: m.training_frame(grey, (HW, HW)), n * (rows * HW + HW * HW)),
                     ("nbc_window_views uint8 (512 every 256)", lambda: m.window_views(rgb, 512, 256), None)]
            for name, call, nbytes in cases:
                ms = _timed(call, reps)
                moved = "" if nbytes is None else f", {nbytes / 2**20:.2f} MiB moved = {nbytes / ms / 1e9:.2f} TB/s"
                print(f"{name}: {n} x {rows}x{HW}: {1e3 * ms:.1f} us per call over {reps} calls (output allocation included)"
                      f"{moved}", flush=True)


def make_folder(root, n, rows_list, distinct=40):
    """n labelled samples, 1024 wide, their heights cycling through rows_list (distinct frames repeated), and the checkpoint of
    the seed-7 weights as best_model.pt."""
    from PIL import Image
    woods = ("epinette_gelee", "epinette_non_gelee", "sapin")
    distinct = min(n, distinct)
    frames = [synth.make_frame(i, rows_list[i % len(rows_list)], HW) for i in range(distinct)]
    duals = [np.where(f[..., 0] > 160, 255, np.where(f[..., 1] > 96, 127, 0)).astype(np.uint8) for f in frames]
    for i in range(n):
        for sub, arr, mode in (("samples", frames[i % distinct], "RGB"), ("duals", duals[i % distinct], "L")):
            d = os.path.join(root, sub, woods[i % 3])
            os.makedirs(d, exist_ok=True)
            Image.fromarray(arr, mode=mode).save(os.path.join(d, "f%04d.png" % i))
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_state_dict("trained_like", seed=7).items()}, ckpt)
    return ckpt


def time_folder(n, precision, rows_list):
    from neuralbarkcalculator_amd import evaluate as ev
    root = tempfile.mkdtemp(prefix="nbc_frame_")
    try:
        ckpt = make_folder(root, n, rows_list)
        modes = ["scan", "training"]
        loop, e2e = {t: [] for t in modes}, {t: [] for t in modes}
        for rep in range(2):
            for t in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, frame=t)
                dt = time.perf_counter() - t0
                loop[t].append(st["images_per_s_loop"])
                e2e[t].append(n / dt)
                print(f"evaluate {precision} rows {rows_list} frame={t} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} "
                      f"images/s (setup {st['setup_s']:.2f} s included, batch {st['batch']}); steady loop "
                      f"{st['images_per_s_loop']:.1f} images/s", flush=True)
        for t in modes:
            print(f"evaluate {precision} frame={t}: best loop {max(loop[t]):.1f} images/s "
                  f"({100 * max(loop[t]) / max(loop['scan']):.1f} % of scan), best end to end {max(e2e[t]):.1f} images/s", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--rows", type=int, nargs="+", default=[600, 641, 700, 733, 800, 901, 1023, 1024])
    ap.add_argument("--precision", nargs="+", default=["f16x2"])
    args = ap.parse_args()
    if args.kernels:
        time_kernels()
    if args.folder:
        for precision in args.precision:
            time_folder(args.folder, precision, args.rows)


if __name__ == "__main__":
    main()
