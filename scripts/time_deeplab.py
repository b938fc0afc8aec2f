#!/usr/bin/env python3
"""Forward timing of deeplabv3_resnet50 at 1024^2 (bench.py keeps measuring fcn_resnet50): images/s of f16x2 batch 1, the
f32 MFMA at batch 1 and bf16 at batch 8 (one stream, HIP events around the timed forwards), then one profiled pass per
configuration: the per-op times of the head from nbc_op_record, the dilated convolutions' share of the mode's matrix peak,
and the pooling branch against its byte bound.  FCN at the same settings for comparison.
usage: python scripts/time_deeplab.py [steps=30] [warmup=5] [out.json]   (one JSON line per configuration; all of them
       together in out.json when it is given)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from neuralbarkcalculator_amd import synth
from neuralbarkcalculator_amd.model import MODELS

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "f16x2": 2500.0 / 3.0}   # as bench.py: dense MFMA peaks, f16x2 a third of f16's
HBM_TBPS = 8.0                                                           # MI355X HBM3E peak
CONFIGS = (("f16x2", 1), ("fp32", 1), ("bf16", 8))


def measure(arch, precision, batch, steps, warmup):
    sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
    m = MODELS[arch](precision).load_state_dict(sd).to("cuda:0")
    x = torch.from_numpy(np.stack([synth.make_input(i, 1024, 1024) for i in range(batch)])).to("cuda:0")
    lowres = m.lowres_logits(x)
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
    del lowres
    return ms, recs


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out = {}
    for precision, batch in CONFIGS:
        for arch in ("deeplabv3_resnet50", "fcn_resnet50"):
            ms, recs = measure(arch, precision, batch, steps, warmup)
            row = {"ms_per_forward": ms, "images_per_s": 1000.0 * batch / ms}
            if arch == "deeplabv3_resnet50":
                names = [r["name"] for r in recs]
                head = recs[names.index("classifier.0.convs.0.0"):]
                peak = PEAK_TFLOPS[precision]
                row["head_ms"] = sum(r["ms"] for r in head)
                row["head_ops"] = [{"name": r["name"], "kernel": r["kernel"], "ms": round(r["ms"], 4),
                                    "tflops": round(r["flops"] / (r["ms"] * 1e9), 1) if r["flops"] else None,
                                    "frac_of_peak": round(r["flops"] / (r["ms"] * 1e9) / peak, 3) if r["flops"] else None,
                                    "tb_per_s": round(r["bytes"] / (r["ms"] * 1e9), 2)} for r in head]
                dil = [r for r in head if r["name"] in ("classifier.0.convs.1.0", "classifier.0.convs.2.0", "classifier.0.convs.3.0")]
                row["dilated_frac_of_peak"] = sum(r["flops"] for r in dil) / (sum(r["ms"] for r in dil) * 1e9) / peak
                pool = next(r for r in head if r["kernel"] == "aspp_pool")
                row["pool_bytes_bound_ms"] = pool["bytes"] / (HBM_TBPS * 1e9)
                row["pool_ms"] = pool["ms"]
            out["%s %s b%d" % (arch, precision, batch)] = row
            print(json.dumps({"config": "%s %s b%d" % (arch, precision, batch), **row}), flush=True)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
