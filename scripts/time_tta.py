#!/usr/bin/env python3
"""The flip views of `predict --tta` / `evaluate --tta` on one GPU.
  --kernels     the three entry points alone, by device events over back-to-back calls at 1024 x 1024: nbc_tta_views on a
                uint8 and on a float32 frame (four views), nbc_tta_merge on the 128 x 128 logits of four views (with the
                aligned views), nbc_vote_tally on four uint8 label maps -- with the bytes each moves and the rate that makes
  --calls       FCNResNet50.predict_labels_tta("flips") against predict_labels on the same box, per precision, at the
                folder driver's default batch (1; 2 in bf16), with remove_small_zones: the TTA call per image over V x the
                plain call per image, with and without the views' own figures (return_views), and the share of the three
                new kernels in the call (their --kernels times over the call's)
  --folder N    predict_folder on a synthetic folder of N 1024 x 1024 samples (scripts/time_evaluate.py's folder) with
                tta = none and flips, alternated, twice each: images/s end to end and in the loop
usage: python scripts/time_tta.py [--kernels] [--calls] [--folder N] [--precision fp32 f16x2 bf16]"""
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

HW, V = 1024, 4


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


def time_kernels(n=1, reps=50):
    """{name: ms} of the three kernels for n images of 1024 x 1024 and four views."""
    dev = torch.device("cuda", 0)
    m = FCNResNet50("fp32").to(dev)
    u8 = torch.from_numpy(np.stack([synth.make_frame(3 + i, HW, HW) for i in range(n)])).to(dev)
    f32 = torch.from_numpy(np.stack([synth.make_input(3 + i, HW, HW) for i in range(n)])).to(dev)
    low = torch.randn((V * n, 3, HW // 8, HW // 8), device=dev)
    labels = torch.randint(0, 3, (V * n, HW, HW), dtype=torch.uint8, device=dev)
    px = n * HW * HW
    cases = [("nbc_tta_views uint8", lambda: m.tta_views(u8, 15), px * 3 * (1 + V)),
             ("nbc_tta_views float32", lambda: m.tta_views(f32, 15), px * 12 * (1 + V)),
             ("nbc_tta_merge + aligned", lambda: m.tta_merge(low, n, 15, return_aligned=True), n * 3 * (HW // 8) ** 2 * 4 * (2 * V + 1)),
             ("nbc_vote_tally", lambda: m.vote_tally(labels, n), px * (V + 4))]
    out = {}
    for name, call, nbytes in cases:
        ms = _timed(call, reps)
        out[name] = ms
        print(f"{name}: {n} x {HW}x{HW}, {V} views: {1e3 * ms:.1f} us per call over {reps} calls (output allocation included), "
              f"{nbytes / 2**20:.1f} MiB moved = {nbytes / ms / 1e9:.2f} TB/s", flush=True)
    return out


def time_calls(precisions, reps=20):
    dev = torch.device("cuda", 0)
    sd = synth.make_state_dict("trained_like", seed=7)
    for precision in precisions:
        n = 2 if precision == "bf16" else 1
        kern = time_kernels(n, reps=20)
        model = FCNResNet50(precision).load_state_dict(sd).to(dev)
        x = torch.from_numpy(np.stack([synth.make_frame(3 + i, HW, HW) for i in range(n)])).to(dev)
        plain = _timed(lambda: model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True), reps)
        big = torch.from_numpy(np.stack([synth.make_frame(3 + i, HW, HW) for i in range(V * n)])).to(dev)
        plain_stack = _timed(lambda: model.predict_labels(big, labels_dtype=torch.uint8, small_zones=True), reps)
        tta = _timed(lambda: model.predict_labels_tta(x, "flips", labels_dtype=torch.uint8, small_zones=True), reps)
        full = _timed(lambda: model.predict_labels_tta(x, "flips", labels_dtype=torch.uint8, small_zones=True, return_views=True), reps)
        new = kern["nbc_tta_views uint8"] + kern["nbc_tta_merge + aligned"]
        print(f"{precision} batch {n}: predict_labels {plain / n:.3f} ms per image ({1e3 * n / plain:.1f} images/s); at batch {V * n} "
              f"{plain_stack / (V * n):.3f} ms per image; predict_labels_tta flips {tta / n:.3f} ms per image "
              f"({1e3 * n / tta:.1f} images/s) = {tta / (V * plain):.3f} x (V x the plain call); with the views' own figures "
              f"{full / n:.3f} ms per image ({1e3 * n / full:.1f} images/s) = {full / (V * plain):.3f} x; the new kernels' share: "
              f"{100 * new / tta:.2f} % of the call, {100 * (new + kern['nbc_vote_tally']) / full:.2f} % with the figures", flush=True)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import predict as drv
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_tta_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        shutil.rmtree(os.path.join(root, "duals"), ignore_errors=True)
        modes = ["none", "flips"]
        loop, e2e = {t: [] for t in modes}, {t: [] for t in modes}
        for rep in range(2):
            for t in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.predict_folder(root, ckpt, precision=precision, device_index=0, tta=t)
                dt = time.perf_counter() - t0
                loop[t].append(st["images_per_s_loop"])
                e2e[t].append(n / dt)
                print(f"predict {precision} tta={t} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} images/s (setup "
                      f"{st['setup_s']:.2f} s included, batch {st['batch']}); steady loop {st['images_per_s_loop']:.1f} images/s", flush=True)
        for t in modes:
            print(f"predict {precision} tta={t}: best loop {max(loop[t]):.1f} images/s ({100 * max(loop[t]) / max(loop['none']):.1f} % of "
                  f"none), best end to end {max(e2e[t]):.1f} images/s", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--precision", nargs="+", default=["f16x2"])
    args = ap.parse_args()
    if args.kernels:
        time_kernels()
    if args.calls:
        time_calls(args.precision)
    if args.folder:
        for precision in args.precision:
            time_folder(args.folder, precision)


if __name__ == "__main__":
    main()
