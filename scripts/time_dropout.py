#!/usr/bin/env python3
"""The Dropout draws of `predict --dropout_draws` on one GPU.
  --kernels     one 1024x1024 forward (batch 1, one stream), then FCNResNet50.dropout_draws on it: passes of 8 draws, timed
                with device events over back-to-back calls, without and with remove_small_zones (run it under
                `rocprofv3 --kernel-trace --stats` for the per-kernel split: every head1x1_dropout_kernel launch is a pass of
                8, and the pass's upsample_argmax_tiled_kernel and remove_small_zones launches have 8 images in their grid)
  --folder N    predict_folder on a synthetic folder of N 1024x1024 samples (scripts/time_evaluate.py's folder) with
                dropout_draws = 0, 8 and 32, alternated, twice each: images/s end to end and in the loop.  D = 0 is the run
                without the flag.
  --votes       both legs also run the per-pixel votes (`--dropout_votes`): --kernels times FCNResNet50.dropout_votes beside
                dropout_draws (under rocprofv3 the added launches are vote_accumulate_kernel, one per pass, and
                vote_summary_kernel, one per call); --folder runs every D > 0 with the votes off and on, alternated.
usage: python scripts/time_dropout.py [--kernels] [--folder N] [--precision f16x2] [--draws 0 8 32] [--votes]"""
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

from neuralbarkcalculator_amd import folder_run, synth
from neuralbarkcalculator_amd.model import FCNResNet50


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


def time_kernels(precision, reps=20, hw=1024, per_pass=8, votes=False):
    dev = torch.device("cuda", 0)
    model = FCNResNet50(precision).load_state_dict(synth.make_state_dict("trained_like", seed=7)).to(dev)
    x = torch.from_numpy(synth.make_input(3, hw, hw)[None]).to(dev)
    ids = [folder_run.image_id("sapin", "f0000.png")]
    model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
    torch.cuda.synchronize()
    read = (hw // 8) ** 2 * 512 * (2 if precision == "bf16" else 4)
    for label, kw in (("masked classifier + upsample", dict(small_zones=False)),
                      ("masked classifier + upsample + remove_small_zones", dict(small_zones=True))):
        ms = _timed(lambda: model.dropout_draws(per_pass, ids, p=0.1, seed=0, draws_per_pass=per_pass, **kw), reps)
        print(f"dropout_draws {precision} 1x{hw}x{hw}, a pass of {per_pass} draws, {label}: {ms:.4f} ms per call, "
              f"{1e3 * ms / per_pass:.1f} us per draw over {reps} calls", flush=True)
        if votes:
            mv = _timed(lambda: model.dropout_votes(per_pass, ids, p=0.1, seed=0, draws_per_pass=per_pass, **kw), reps)
            print(f"dropout_votes {precision} 1x{hw}x{hw}, a pass of {per_pass} draws, {label} + votes and summary: {mv:.4f} ms per "
                  f"call, {1e3 * (mv - ms):+.1f} us against dropout_draws over {reps} calls", flush=True)
    print(f"the masked classifier reads {read / 2**20:.0f} MiB once per pass of {per_pass} draws and writes "
          f"{per_pass * 3 * (hw // 8) ** 2 * 4 / 2**20:.2f} MiB of logits", flush=True)


def time_folder(n, precision, draws, votes=False):
    from neuralbarkcalculator_amd import predict as drv
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_dropout_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        shutil.rmtree(os.path.join(root, "duals"), ignore_errors=True)
        draws = [(d, v) for d in draws for v in ((False, True) if votes and d else (False,))]
        loop, e2e = {d: [] for d in draws}, {d: [] for d in draws}
        for rep in range(2):
            for d in draws:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.predict_folder(root, ckpt, precision=precision, device_index=0, dropout_draws=d[0], dropout_votes=d[1])
                dt = time.perf_counter() - t0
                loop[d].append(st["images_per_s_loop"])
                e2e[d].append(n / dt)
                print(f"predict {precision} dropout_draws={d[0]} votes={int(d[1])} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} images/s "
                      f"(setup {st['setup_s']:.2f} s included); steady loop {st['images_per_s_loop']:.1f} images/s", flush=True)
        base = max(loop[draws[0]])
        for d in draws:
            print(f"predict {precision} D={d[0]} votes={int(d[1])}: best loop {max(loop[d]):.1f} images/s "
                  f"({100 * max(loop[d]) / base:.1f} % of D={draws[0][0]}), "
                  f"best end to end {max(e2e[d]):.1f} images/s", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--draws", type=int, nargs="+", default=[0, 8, 32])
    ap.add_argument("--votes", action="store_true")
    args = ap.parse_args()
    if args.kernels:
        time_kernels(args.precision, votes=args.votes)
    if args.folder:
        time_folder(args.folder, args.precision, args.draws, args.votes)


if __name__ == "__main__":
    main()
