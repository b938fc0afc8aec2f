#!/usr/bin/env python3
"""Forward timing of fcn_resnet50 in fp32 at batch 1, 1024^2, with BatchNorm on the running statistics (folded into the
conv epilogues) and with per-image statistics (--bn_stats image: raw conv, then a statistics and an apply kernel per
BatchNorm).  One stream, HIP events around the timed forwards, then one profiled pass per mode: the time of the
statistics and apply ops, and on the 64 MB and 128 MB layer3/4 outputs their achieved bytes per second against the
6.29 TB/s the HBM delivers to a streaming kernel.
usage: python scripts/time_bn_stats.py [steps=30] [warmup=5] [out.json]   (one JSON line per configuration; all of them
       together in out.json when it is given)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from neuralbarkcalculator_amd import synth
from neuralbarkcalculator_amd.model import fcn_resnet50

STREAM_TBPS = 6.29


def measure(mode, steps, warmup):
    sd = synth.make_state_dict("trained_like", seed=7)
    m = fcn_resnet50(precision="fp32", bn_statistics=mode).load_state_dict(sd).to("cuda:0")
    x = torch.from_numpy(np.stack([synth.make_input(0, 1024, 1024)])).to("cuda:0")
    for _ in range(warmup):
        m.lowres_logits(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        m.lowres_logits(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    m.set_profiling(True)
    for _ in range(5):
        m.lowres_logits(x)
    recs = m.op_records()
    m.set_profiling(False)
    return ms, recs


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out = {}
    for mode in ("running", "image"):
        ms, recs = measure(mode, steps, warmup)
        row = {"ms_per_forward": ms, "images_per_s": 1000.0 / ms}
        bn = [r for r in recs if r["kernel"] in ("bn_stats", "bn_apply")]
        if bn:
            row["bn_ms"] = sum(r["ms"] for r in bn)
            row["conv_ms"] = sum(r["ms"] for r in recs if r["kernel"] == "conv_dma")
            big = []
            for r in bn:
                mb = r["cout"] * 128 * 128 * 4 / 2 ** 20            # the tensor at 1024^2 (layer2-4 maps are 128 x 128)
                if r["name"].startswith(("backbone.layer3", "backbone.layer4")) and mb in (64.0, 128.0):
                    big.append({"name": r["name"], "kernel": r["kernel"], "tensor_mb": mb, "ms": round(r["ms"], 4),
                                "tb_per_s": round(r["bytes"] / (r["ms"] * 1e9), 2),
                                "frac_of_stream": round(r["bytes"] / (r["ms"] * 1e9) / STREAM_TBPS, 3)})
            row["large_tensors"] = big
            for k in ("bn_stats", "bn_apply"):
                sel = [b for b in big if b["kernel"] == k]
                if sel:
                    row[k + "_median_frac_of_stream"] = float(np.median([b["frac_of_stream"] for b in sel]))
        out["fp32 b1 " + mode] = row
        print(json.dumps({"config": "fcn_resnet50 fp32 b1 bn_stats=" + mode,
                          **{k: v for k, v in row.items() if k != "large_tensors"}}), flush=True)
    out["image_over_running"] = out["fp32 b1 image"]["images_per_s"] / out["fp32 b1 running"]["images_per_s"]
    print(json.dumps({"image_over_running": out["image_over_running"]}), flush=True)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
