#!/usr/bin/env python3
"""Forward timing of the EfficientNet networks at 1024^2 in fp32 (bench.py keeps measuring fcn_resnet50): images/s of
b0 and b5, both heads, at batch 1 and 2 (one stream, HIP events around the timed forwards), then one profiled pass per
configuration: per kernel family the summed time, and for each new kernel (dwconv, se_excite, gate_weights, swish, aspp_pool)
its achieved bytes/s against the 6.29 TB/s streaming figure of DESIGN section 3.6; the depthwise launches on tensors of
64 MB or more are listed on their own.
usage: python scripts/time_efficientnet.py [steps=20] [warmup=3] [out.json]   (one JSON line per configuration; all of
       them together in out.json when it is given)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from neuralbarkcalculator_amd import synth
from neuralbarkcalculator_amd.model import MODELS

STREAM_TBPS = 6.29                      # DESIGN: measured streaming copy rate of the MI355X
NEW_KERNELS = ("dwconv", "se_excite", "gate_weights", "swish", "aspp_pool")
CONFIGS = [(arch, batch) for arch in ("fcn_efficientnet_b0", "deeplabv3_efficientnet_b0", "fcn_efficientnet_b5",
                                      "deeplabv3_efficientnet_b5") for batch in (1, 2)]


def measure(arch, batch, steps, warmup, size=1024):
    sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
    m = MODELS[arch]("fp32").load_state_dict(sd).to("cuda:0")
    x = torch.from_numpy(np.stack([synth.make_input(i, size, size) for i in range(batch)])).to("cuda:0")
    for _ in range(warmup + 1):
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
    for _ in range(3):
        m.lowres_logits(x)
    recs = m.op_records()
    m.set_profiling(False)
    return ms, recs


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    out = {}
    for arch, batch in CONFIGS:
        ms, recs = measure(arch, batch, steps, warmup)
        row = {"ms_per_forward": round(ms, 3), "images_per_s": round(1000.0 * batch / ms, 1), "kernels": {}}
        for r in recs:
            k = row["kernels"].setdefault(r["kernel"], {"ms": 0.0, "bytes": 0.0, "launches": 0})
            k["ms"] += r["ms"]
            k["bytes"] += r["bytes"]
            k["launches"] += r["launches"]
        for name, k in row["kernels"].items():
            k["ms"] = round(k["ms"], 4)
            if name in NEW_KERNELS and k["ms"] > 0:
                k["tb_per_s"] = round(k["bytes"] / (k["ms"] * 1e9), 2)
                k["frac_of_stream"] = round(k["bytes"] / (k["ms"] * 1e9) / STREAM_TBPS, 3)
            k.pop("bytes")
        big = [r for r in recs if r["kernel"] == "dwconv" and r["bytes"] >= 64e6]
        row["dwconv_64mb"] = [{"name": r["name"], "mb": round(r["bytes"] / 1e6, 1), "ms": round(r["ms"], 4),
                               "frac_of_stream": round(r["bytes"] / (r["ms"] * 1e9) / STREAM_TBPS, 3)} for r in big]
        key = "%s fp32 b%d" % (arch, batch)
        out[key] = row
        print(json.dumps({"config": key, **row}), flush=True)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
