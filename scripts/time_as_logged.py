#!/usr/bin/env python3
"""The two grouped passes of `evaluate --frame training --pool B --as_logged` on one GPU.
  --kernels     a group of 8 at 1024 x 1024, by device events over back-to-back calls: nbc_remove_small_zones_groups (G = 8)
                beside nbc_remove_small_zones on the same eight label maps (N = 8), and nbc_lovasz_softmax_groups (G = 8)
                beside nbc_lovasz_softmax on the same eight images (N = 8); the label maps are the network's own argmax of
                eight synthetic frames, the logits its own
  --folder N    evaluate_folder with frame = "training", pool = 8 on a synthetic labelled folder of N height-trimmed scans,
                without and with as_logged, alternated, twice each: images/s end to end and in the loop, and the seconds
                the pass after the loop adds
usage: python scripts/time_as_logged.py [--kernels] [--folder N] [--precision f16x2 ...]"""
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
from time_frame import _timed, make_folder

HW, GROUP = 1024, 8


def time_kernels(reps=20):
    dev = torch.device("cuda", 0)
    m = FCNResNet50("f16x2").load_state_dict(synth.make_state_dict("trained_like", seed=7)).to(dev)
    frames = [synth.make_frame(3 + i, HW, HW) for i in range(GROUP)]
    logits = torch.empty((GROUP, 3, HW, HW), dtype=torch.float32, device=dev)
    labels = torch.empty((GROUP, HW, HW), dtype=torch.uint8, device=dev)
    for a in range(0, GROUP, 2):                                    # the forward at the batch it is run at
        x = torch.from_numpy(np.stack(frames[a:a + 2])).to(dev)
        labels[a:a + 2] = m.predict_labels(x, labels_dtype=torch.uint8, logits_full=logits[a:a + 2])[0]
    grey = torch.from_numpy(np.stack([np.where(f[..., 0] > 160, 255, np.where(f[..., 1] > 96, 127, 0)).astype(np.uint8)
                                      for f in frames])).to(dev)
    work = labels.clone()

    def zones(call):
        work.copy_(labels)                                          # in place: every call starts from the raw argmax
        call(work)
    copy_ms = _timed(lambda: work.copy_(labels), reps)
    cases = [("nbc_remove_small_zones, N = 8", lambda: zones(lambda t: m.remove_small_zones(t))),
             ("nbc_remove_small_zones_groups, G = 8", lambda: zones(lambda t: m.remove_small_zones_groups(t, GROUP))),
             ("nbc_lovasz_softmax, N = 8", lambda: m.lovasz_softmax(logits, grey)),
             ("nbc_lovasz_softmax_groups, G = 8", lambda: m.lovasz_softmax_groups(logits, grey, GROUP))]
    for name, call in cases:
        ms = _timed(call, reps)
        note = f" (the {1e3 * copy_ms:.0f} us copy of the labels included)" if "zones" in name else ""
        print(f"{name}: 8 x {HW}x{HW}: {ms:.3f} ms per call over {reps} calls{note}", flush=True)
    per, grouped = m.remove_small_zones(labels.clone())[0], m.remove_small_zones_groups(labels.clone(), GROUP)[0]
    print(f"pixels the batch axis changes on these eight maps: {100 * float((per != grouped).float().mean()):.3f} %", flush=True)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as ev
    root = tempfile.mkdtemp(prefix="nbc_as_logged_")
    try:
        ckpt = make_folder(root, n, [600, 641, 700, 733, 800, 901, 1023, 1024])
        modes = [False, True]
        loop, e2e = {t: [] for t in modes}, {t: [] for t in modes}
        for rep in range(2):
            for t in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, frame="training", pool=GROUP,
                                        **(dict(as_logged=True) if t else {}))
                dt = time.perf_counter() - t0
                loop[t].append(st["images_per_s_loop"])
                e2e[t].append(dt)
                print(f"evaluate {precision} frame=training pool={GROUP} as_logged={t} run {rep}: {n} images end to end in {dt:.2f} s = "
                      f"{n / dt:.1f} images/s (setup {st['setup_s']:.2f} s included, batch {st['batch']}); steady loop "
                      f"{st['images_per_s_loop']:.1f} images/s", flush=True)
        print(f"evaluate {precision}: best loop {max(loop[False]):.1f} images/s without, {max(loop[True]):.1f} with the flag; best end to "
              f"end {min(e2e[False]):.2f} s without, {min(e2e[True]):.2f} s with: {min(e2e[True]) - min(e2e[False]):+.2f} s for "
              f"{(n + GROUP - 1) // GROUP} groups", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--precision", nargs="+", default=["f16x2"])
    args = ap.parse_args()
    if args.kernels:
        time_kernels()
    if args.folder:
        for precision in args.precision:
            time_folder(args.folder, precision)


if __name__ == "__main__":
    main()
