#!/usr/bin/env python3
"""The crop windows of `predict --windows` / `evaluate --windows` on one GPU.
  --kernels     the two entry points alone, by device events over back-to-back calls at 1024 x 1024 with the defaults
                (512-pixel windows every 256: nine windows): nbc_window_views on a uint8 and on a float32 frame,
                nbc_window_merge on the nine 64 x 64 logit maps -- with the bytes each moves and the rate that makes
  --calls       FCNResNet50.predict_labels_windows against predict_labels on the same box, per precision, at the folder
                driver's default batch (1; 2 in bf16), with remove_small_zones and uint8 labels: the windows call per image
                over K E_y E_x / (H W) x the plain call per image, at 1024 x 1024 and at --rows x 1024, and the share of the
                two new kernels in the call (their --kernels times over the call's)
  --folder N    predict_folder on a synthetic folder of N samples of --rows x 1024 (default 1024) with and without
                windows = 512, alternated, twice each: images/s end to end and in the loop
usage: python scripts/time_windows.py [--kernels] [--calls] [--folder N] [--rows R ...] [--precision fp32 f16x2 bf16]"""
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
from neuralbarkcalculator_amd.model import FCNResNet50, window_grid

HW, S, T = 1024, 512, 256


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


def time_kernels(n=1, rows=HW, reps=50):
    """{name: ms} of the two kernels for n images of rows x 1024."""
    dev = torch.device("cuda", 0)
    m = FCNResNet50("fp32").to(dev)
    ey, ex, ny, nx, _, _ = window_grid(rows, HW, S, T)
    k = ny * nx
    u8 = torch.from_numpy(np.stack([synth.make_frame(3 + i, rows, HW) for i in range(n)])).to(dev)
    f32 = torch.from_numpy(np.stack([synth.make_input(3 + i, rows, HW) for i in range(n)])).to(dev)
    low = torch.randn((k * n, 3, ey // 8, ex // 8), device=dev)
    px, wpx = n * rows * HW, n * k * ey * ex
    cases = [("nbc_window_views uint8", lambda: m.window_views(u8, S, T), 3 * (px + wpx)),
             ("nbc_window_views float32", lambda: m.window_views(f32, S, T), 12 * (px + wpx)),
             ("nbc_window_merge", lambda: m.window_merge(low, n, rows, HW, S, T), 12 * (wpx + n * ((rows + 7) // 8 * 8) * HW) // 64)]
    out = {}
    for name, call, nbytes in cases:
        ms = _timed(call, reps)
        out[name] = ms
        print(f"{name}: {n} x {rows}x{HW}, {k} windows of {ey}x{ex}: {1e3 * ms:.1f} us per call over {reps} calls (output "
              f"allocation included), {nbytes / 2**20:.2f} MiB moved = {nbytes / ms / 1e9:.2f} TB/s", flush=True)
    return out


def time_calls(precisions, rows_list, reps=20):
    dev = torch.device("cuda", 0)
    sd = synth.make_state_dict("trained_like", seed=7)
    for precision in precisions:
        n = 2 if precision == "bf16" else 1
        model = FCNResNet50(precision).load_state_dict(sd).to(dev)
        for rows in rows_list:
            kern = time_kernels(n, rows, reps=20)
            ey, ex, ny, nx, _, _ = window_grid(rows, HW, S, T)
            cost = ny * nx * ey * ex / (rows * HW)
            x = torch.from_numpy(np.stack([synth.make_frame(3 + i, rows, HW) for i in range(n)])).to(dev)
            plain = _timed(lambda: model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True), reps)
            win = _timed(lambda: model.predict_labels_windows(x, S, T, labels_dtype=torch.uint8, small_zones=True), reps)
            new = kern["nbc_window_views uint8"] + kern["nbc_window_merge"]
            print(f"{precision} batch {n}, {rows}x{HW}: predict_labels {plain / n:.3f} ms per image ({1e3 * n / plain:.1f} images/s); "
                  f"predict_labels_windows ({ny}x{nx} windows of {ey}x{ex}) {win / n:.3f} ms per image ({1e3 * n / win:.1f} images/s) = "
                  f"{win / plain:.3f} plain calls = {win / (cost * plain):.3f} x ({cost:.3f} x the plain call); the new kernels' "
                  f"share: {100 * new / win:.2f} % of the call", flush=True)


def make_folder(root, n, rows, distinct=40):
    """n samples of rows x 1024 (distinct frames repeated) and the checkpoint of the seed-7 weights as best_model.pt."""
    from PIL import Image
    woods = ("epinette_gelee", "epinette_non_gelee", "sapin")
    distinct = min(n, distinct)
    frames = [synth.make_frame(i, rows, HW) for i in range(distinct)]
    for i in range(n):
        d = os.path.join(root, "samples", woods[i % 3])
        os.makedirs(d, exist_ok=True)
        Image.fromarray(frames[i % distinct], mode="RGB").save(os.path.join(d, "f%04d.bmp" % i))
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_state_dict("trained_like", seed=7).items()}, ckpt)
    return ckpt


def time_folder(n, precision, rows):
    from neuralbarkcalculator_amd import predict as drv
    root = tempfile.mkdtemp(prefix="nbc_windows_")
    try:
        ckpt = make_folder(root, n, rows)
        modes = [None, S]
        loop, e2e = {t: [] for t in modes}, {t: [] for t in modes}
        for rep in range(2):
            for t in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.predict_folder(root, ckpt, precision=precision, device_index=0, windows=t)
                dt = time.perf_counter() - t0
                loop[t].append(st["images_per_s_loop"])
                e2e[t].append(n / dt)
                print(f"predict {precision} {rows}x{HW} windows={t} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} "
                      f"images/s (setup {st['setup_s']:.2f} s included, batch {st['batch']}); steady loop "
                      f"{st['images_per_s_loop']:.1f} images/s", flush=True)
        for t in modes:
            print(f"predict {precision} {rows}x{HW} windows={t}: best loop {max(loop[t]):.1f} images/s "
                  f"({100 * max(loop[t]) / max(loop[None]):.1f} % of none), best end to end {max(e2e[t]):.1f} images/s", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--rows", type=int, nargs="+", default=[HW])
    ap.add_argument("--precision", nargs="+", default=["f16x2"])
    args = ap.parse_args()
    if args.kernels:
        time_kernels()
    if args.calls:
        time_calls(args.precision, args.rows)
    if args.folder:
        for precision in args.precision:
            for rows in args.rows:
                time_folder(args.folder, precision, rows)


if __name__ == "__main__":
    main()
