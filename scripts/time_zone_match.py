#!/usr/bin/env python3
"""The zone matching of `evaluate --zones` on one GPU.
  kernels       FCNResNet50.match_zones (nbc_match_zones) by device events over back-to-back calls on a batch of eight
                1024x1024 maps -- the network's labels on synthetic frames against perturbed duals -- beside, in the same run
                and alternated, the part that exists without it: two FCNResNet50.label_zones calls on the same two sets of
                maps; and zones.match_cpu on this host.  Under `rocprofv3 --kernel-trace --stats` the launches of the pass
                beyond the two labellings are target_class_plane_kernel, pair_clear_kernel, pair_accumulate_kernel and
                pair_sort_kernel.
  folder [N]    evaluate_folder on a synthetic labelled folder of N 1024x1024 samples (scripts/time_evaluate.py's folder)
                without and with zones, alternated, twice each: images/s end to end and in the loop.
usage: python scripts/time_zone_match.py kernels | folder [N] [--precision f16x2]"""
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

from neuralbarkcalculator_amd import synth, zones
from neuralbarkcalculator_amd.model import FCNResNet50

GREY = np.array([0, 127, 255], dtype=np.uint8)


def _window(call, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_kernels(reps=50, rounds=5, flip=0.001):
    dev = torch.device("cuda", 0)
    model = FCNResNet50("f16x2").load_state_dict(synth.make_state_dict("trained_like", seed=7)).to(dev)
    x = torch.from_numpy(np.stack([synth.make_input(60 + k, 1024, 1024) for k in range(8)])).to(dev)
    labels = model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)[0]
    lab = labels.cpu().numpy()
    rng = np.random.default_rng(61)
    tgt = lab.copy()
    m = rng.random(tgt.shape) < flip
    tgt[m] = rng.integers(0, 3, size=int(m.sum()), dtype=np.uint8)
    grey = torch.from_numpy(GREY[tgt]).to(dev)
    tgt_dev = torch.from_numpy(tgt).to(dev)

    t0 = time.perf_counter()
    want = zones.match_cpu(lab, tgt)
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    most_zones = max(max(len(o), len(t)) for o, t, _ in want)
    most_pairs = max(len(p) for _, _, p in want)
    cap, pair_cap = max(1024, most_zones), min(zones.PAIRS_MAX_CAP, max(zones.DEFAULT_PAIR_CAP, most_pairs))
    got = [g.cpu().numpy() for g in model.match_zones(labels, grey, cap=cap, pair_cap=pair_cap)]
    ok = all(int(got[1][i]) == len(o) and int(got[3][i]) == len(t) and int(got[5][i]) == len(p) and
             np.array_equal(got[0][i, :len(o)], o) and np.array_equal(got[2][i, :len(t)], t) and np.array_equal(got[4][i, :len(p)], p)
             for i, (o, t, p) in enumerate(want)) if most_pairs <= pair_cap else None

    def match():
        model.match_zones(labels, grey, cap=cap, pair_cap=pair_cap)

    def two_labellings():
        model.label_zones(labels, cap=cap)
        model.label_zones(tgt_dev, cap=cap)
    for call in (match, two_labellings):                          # warm both, then alternate the timed windows
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    ms_match, ms_label = [], []
    for _ in range(rounds):
        ms_match.append(_window(match, reps))
        ms_label.append(_window(two_labellings, reps))
    a, b = float(np.median(ms_match)), float(np.median(ms_label))
    print(f"8x1024x1024, network labels against duals with {100 * flip:.1f} % of the pixels redrawn: at most {most_zones} zones "
          f"and {most_pairs} pairs per image (cap {cap}, pair_cap {pair_cap}); equal to match_cpu: {ok}", flush=True)
    print(f"match_zones {1e3 * a:.1f} us per call ({1e3 * a / 8:.1f} per image; windows {min(ms_match) * 1e3:.1f} .. "
          f"{max(ms_match) * 1e3:.1f}), two label_zones calls {1e3 * b:.1f} us ({1e3 * b / 8:.1f} per image; windows "
          f"{min(ms_label) * 1e3:.1f} .. {max(ms_label) * 1e3:.1f}), ratio {a / b:.2f}; {rounds} alternated windows of {reps} "
          f"calls each, medians; zones.match_cpu {cpu_ms:.0f} ms ({cpu_ms / 8:.0f} per image)", flush=True)


def _realistic_duals(root, ckpt, precision, flip=0.001):
    """Replace the folder's duals (grey noise: tens of thousands of zones, every image a host fallback) by what a labelled
    mask looks like next to a good checkpoint: the label PNGs of a predict run with a share ``flip`` of the pixels redrawn."""
    from PIL import Image
    from neuralbarkcalculator_amd import predict
    predict.predict_folder(root, ckpt, precision=precision, device_index=0)
    out = os.path.join(root, "results", "outputs")
    rng = np.random.default_rng(5)
    for wood in sorted(os.listdir(out)):
        for name in sorted(os.listdir(os.path.join(out, wood))):
            png = np.asarray(Image.open(os.path.join(out, wood, name)))
            cls = zones.target_classes(png).astype(np.int64)      # the label PNG's levels 0 / 127 / 255
            m = rng.random(cls.shape) < flip
            cls[m] = rng.integers(0, 3, size=int(m.sum()))
            Image.fromarray(GREY[cls], mode="L").save(os.path.join(root, "duals", wood, name))
    shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
    shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as drv
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_zone_match_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        _realistic_duals(root, ckpt, precision)
        loop, e2e = {False: [], True: []}, {False: [], True: []}
        for rep in range(2):
            for flag in (False, True):
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.evaluate_folder(root, ckpt, precision=precision, device_index=0, **(dict(zones=True) if flag else {}))
                dt = time.perf_counter() - t0
                loop[flag].append(st["images_per_s_loop"])
                e2e[flag].append(n / dt)
                note = ""
                if flag:
                    z = st["summary"]["zones"]
                    note = (f"; {z['Bark']['targets'] + z['Node']['targets']} target zones, "
                            f"{z['Bark']['outputs'] + z['Node']['outputs']} output zones, {st['zones_host_fallbacks']} host fallbacks")
                print(f"evaluate {precision} zones={int(flag)} run {rep}: {n} images ({st['summary']['images_evaluated']} evaluated) "
                      f"end to end in {dt:.2f} s = {n / dt:.1f} images/s "
                      f"(setup {st['setup_s']:.2f} s included); steady loop {st['images_per_s_loop']:.1f} images/s{note}", flush=True)
        for flag in (False, True):
            print(f"evaluate {precision} zones={int(flag)}: best loop {max(loop[flag]):.1f} images/s "
                  f"({100 * max(loop[flag]) / max(loop[False]):.1f} % of the run without), best end to end {max(e2e[flag]):.1f} images/s",
                  flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "folder"])
    ap.add_argument("n", type=int, nargs="?", default=96, help="folder: the number of samples")
    ap.add_argument("--precision", default="f16x2")
    args = ap.parse_args()
    if args.what == "kernels":
        time_kernels()
    else:
        time_folder(args.n, args.precision)


if __name__ == "__main__":
    main()
