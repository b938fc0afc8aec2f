"""Readers of the recorded reference results (tests/golden/ref_*.npz, written by oracle/record_reference.py) for
tests/test_reference_pins.py and tests/test_gpu_reference_pins.py.  They read nothing but tests/golden/."""
from __future__ import annotations

import glob
import os
from typing import Dict, List

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
LOSS_SHAPES = [(1, 1), (1, 7), (33, 65), (65, 127)]
HEAD_SHAPES = [(64, 64), (40, 72)]
PER_IMAGE = ["case", "logits", "grey", "classes", "lovasz", "present", "lovasz_terms", "ce", "wce", "mixed", "d_lovasz",
             "d_lovasz_terms", "d_ce", "d_wce", "d_mixed"]


def cpu_name() -> str:
    """What decides the order in which torch's CPU kernels add float32 numbers: the vector extension torch dispatches on
    and the processor's model name.  A float32 result is reproduced bit for bit only where this and ``torch.__version__``
    are the recorded ones."""
    import torch
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((line.split(":", 1)[1].strip() for line in f if line.startswith("model name")), "")
    except OSError:
        pass
    return "%s, %s" % (torch.backends.cpu.get_cpu_capability(), model)


def same_build(g) -> bool:
    """True where float32 results of this process can be compared bit for bit with the fixture ``g``."""
    import torch
    return str(g["torch_version"]) == torch.__version__ and str(g["cpu"]) == cpu_name()


def load(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def fixture_names() -> List[str]:
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ref_*.npz")))


_loss_cache: Dict[tuple, dict] = {}


def loss_fixture(h: int, w: int) -> dict:
    """The six images of one shape, its part files joined in case order: the per-image arrays of ``PER_IMAGE`` (logits as
    float32 [6,3,H,W]), ``weights`` float32 [2,3] and ``torch_version``.  Read once; do not modify."""
    if (h, w) not in _loss_cache:
        names = [n for n in fixture_names() if n == "ref_loss_%dx%d" % (h, w) or n.startswith("ref_loss_%dx%d_" % (h, w))]
        parts = sorted((load(n) for n in names), key=lambda g: int(g["case"][0]))
        out = {k: np.concatenate([g[k] for g in parts]) for k in PER_IMAGE}
        assert out["case"].tolist() == list(range(6)), (names, out["case"])
        out["logits"] = out["logits"].astype(np.float32)
        out["weights"], out["torch_version"] = parts[0]["weights"], str(parts[0]["torch_version"])
        _loss_cache[(h, w)] = out
    return _loss_cache[(h, w)]


def stats_fixture() -> dict:
    g = load("ref_stats")
    n = sum(k.startswith("frame_") for k in g.files)
    return {"frames": [g["frame_%d" % i] for i in range(n)], "greys": [g["grey_%d" % i] for i in range(n)],
            "classes": [g["classes_%d" % i] for i in range(n)], "mean": g["mean"], "std": g["std"],
            "pos_weight": g["pos_weight"], "d_mean": g["d_mean"], "d_std": g["d_std"]}


def within_one_f32_ulp(value: float, recorded: np.float32) -> bool:
    """``value`` (a double) against a float32 the reference rounded from its own double."""
    return abs(float(value) - float(recorded)) <= float(np.spacing(np.float32(abs(recorded))))
