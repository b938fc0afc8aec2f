#!/usr/bin/env python3
"""Labelled-folder evaluation against folder prediction on one GPU: a synthetic folder of n 1024x1024 .bmp samples with a
grey .png dual each (samples/ + duals/), then evaluate_folder and predict_folder on it, alternated, twice each.  The
evaluation decodes one grey PNG per image more and writes no label PNG and no processed/ frame.
usage: python scripts/time_evaluate.py [n_images=1000] [precision=f16x2]
       python scripts/time_evaluate.py --make DIR [n_images=16]      (only make the folder, e.g. for a profiler run)"""
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from concurrent.futures import ThreadPoolExecutor
from PIL import Image
from neuralbarkcalculator_amd import evaluate as ev, predict as drv, synth
from neuralbarkcalculator_amd.pngio import write_png

WOODS = ("epinette_gelee", "epinette_non_gelee", "sapin")


def make_folder(root, n, distinct=40):
    """n samples (distinct frames repeated) with duals: grey levels from the frame's green channel, so that every decode
    band occurs; the checkpoint of the seed-7 weights as best_model.pt."""
    distinct = min(n, distinct)
    for wood in WOODS:
        os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
        os.makedirs(os.path.join(root, "duals", wood), exist_ok=True)
    src = os.path.join(root, "_distinct")
    os.makedirs(src, exist_ok=True)

    def one(i):
        f = synth.make_frame(i, 1024, 1024)
        Image.fromarray(f, mode="RGB").save(os.path.join(src, "%d.bmp" % i))
        write_png(os.path.join(src, "%d.png" % i), np.ascontiguousarray(f[..., 1]), 1)

    def place(i):
        wood, name = WOODS[i % 3], "f%04d" % i
        shutil.copyfile(os.path.join(src, "%d.bmp" % (i % distinct)), os.path.join(root, "samples", wood, name + ".bmp"))
        shutil.copyfile(os.path.join(src, "%d.png" % (i % distinct)), os.path.join(root, "duals", wood, name + ".png"))
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, range(distinct)))
        list(pool.map(place, range(n)))
    shutil.rmtree(src)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_state_dict("trained_like", seed=7).items()}, ckpt)
    return ckpt


def main():
    if sys.argv[1:2] == ["--make"]:
        root, n = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 16
        make_folder(root, n)
        print("made", root, n)
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    prec = sys.argv[2] if len(sys.argv) > 2 else "f16x2"
    root = tempfile.mkdtemp(prefix="nbc_eval_")
    try:
        t0 = time.perf_counter()
        ckpt = make_folder(root, n)
        print(f"folder of {n} synthetic 1024x1024 .bmp samples with grey .png duals made in {time.perf_counter() - t0:.1f} s; "
              f"host workers {drv._host_workers()}, cores available {len(os.sched_getaffinity(0))}", flush=True)
        for rep in range(2):
            for what in ("evaluate", "predict"):
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)
                t0 = time.perf_counter()
                if what == "evaluate":
                    st = ev.evaluate_folder(root, ckpt, precision=prec, device_index=0)
                else:
                    st = drv.predict_folder(root, ckpt, precision=prec, device_index=0)
                dt = time.perf_counter() - t0
                print(f"{what} {prec} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} images/s "
                      f"(setup {st['setup_s']:.2f} s included); steady loop {st['images_per_s_loop']:.1f} images/s", flush=True)
                if what == "evaluate":
                    print("  " + ev.format_summary(st["summary"]).replace("\n", "\n  "), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
