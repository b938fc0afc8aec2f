"""The exact gather probe on the device (tests/helpers/gather_probe.py): one-hot conv rows and a BatchNorm of powers of two and
dyadic biases, under which every conv unit's stored output is known to the bit from the operands it read -- in f16x2, fp32 and
bf16 alike, whatever the order of summation, at any K.  Keep mode at the planned tiles; each unit's operands are the tensors
its producers stored; the comparison is uint32 equality on every element, and a failure names the unit, its planned tile, the
first differing (n, c, y, x) and the K position its row selects.  Nine rounds move every row's K position so that every K
position of every unit with K <= 4608, and every K-step and channel slot of the K = 18 432 units, carries a value once
(tests/test_gather_probe_cover.py).  What the probe cannot hold -- the weights' low piece Q, a neighbour's alpha, the activation
powers -- tests/test_gpu_f32_grade_operands.py bounds; what that bound cannot see at long K or at the store, this sees."""
import os
import sys

import numpy as np
import pytest

from neuralbarkcalculator_amd import topology
from neuralbarkcalculator_amd.model import MODELS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gather_probe as gp  # noqa: E402
import kept_operands as ko  # noqa: E402

pytestmark = pytest.mark.gpu
FCN, DL = "fcn_resnet50", "deeplabv3_resnet50"
PRECISIONS = ("f16x2", "fp32", "bf16")
# 2 x 40 x 72: 5 x 9 maps, fewer pixels than any tile, an image boundary inside a tile; 1 x 16 x 1024: 128-pixel-wide maps, the
# row-step kernel's tiles 18 / 19 / 20 on two rows
FCN_SHAPES = [(2, 40, 72), (1, 16, 1024)]
# the head at 2 x 96 x 96 (12 x 12: every dilated tap but the centre reads padding) in every round; at 1 x 640 x 640 (80 x 80: the
# taps of dilation 36 inside the image) in one
CASES = [(FCN, s, r) for s in FCN_SHAPES for r in range(gp.ROUNDS)] + [(DL, (2, 96, 96), r) for r in range(gp.ROUNDS)] + [(DL, (1, 640, 640), 0)]

_MODELS = {}


def model_of(arch, precision):
    """One model per (architecture, precision) for the module: a round loads its checkpoint into it"""
    if (arch, precision) not in _MODELS:
        _MODELS[(arch, precision)] = MODELS[arch](precision)
    return _MODELS[(arch, precision)]


@pytest.fixture(scope="module", autouse=True)
def release_models():
    yield
    _MODELS.clear()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("arch,shape,r", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, tuple) else "round%d" % v)
def test_every_unit_stores_the_selected_operand_bit_for_bit(built_lib, arch, shape, r, precision):
    n, h, w = shape
    sd, sel = gp.probe_state_dict(arch, r)
    m = model_of(arch, precision).load_state_dict(sd).to(ko.DEV)
    assert m.pack_flags == 0
    x = ko.frames(range(40, 40 + n), h, w)
    names, reads, shapes, tiles = ko.plan_of(arch, precision, n, h, w)
    units = [u for u in topology.conv_units(arch) if u.bn is not None and not u.pooled
             and (arch == FCN or u.name.startswith("classifier."))]
    wanted = sorted({u.name for u in units} | {reads[(u.name, k)] for u in units for k in ("in", "res") if (u.name, k) in reads} - {"ingest"})
    acts, low = ko.stored(m, x, shapes, wanted)
    assert not m.nonfinite_seen() and np.isfinite(low).all()
    assert all(m.activation_exponent(u.name) == 0 for u in topology.conv_units(arch) if u.bn is not None)
    if precision == "f16x2":
        ok, bad = m.f16x2_range_ok(m.activation_peaks(x.to(ko.DEV)))
        assert ok, bad
    acts["ingest"] = gp.ingested(x.numpy(), precision)
    differing = []
    for u in units:
        xin = acts[reads[(u.name, "in")]]
        res = acts[reads[(u.name, "res")]] if u.residual else None
        pos, sg = sel[u.name]
        want = gp.expected_unit(xin, u, pos, sg, sd[u.bn + ".bias"], res, precision)
        # the reference alone, before any comparison: the probe is not vacuous on these operands
        if precision != "bf16":                         # a bf16 value has no low piece
            assert gp.low_piece_share(xin) >= 0.5, (u.name, gp.low_piece_share(xin))
        assert (xin != 0).mean() >= 0.5 and (want != 0).mean() >= 0.25, (u.name, float((want != 0).mean()))
        msg = gp.first_difference(acts[u.name], want, u, pos, tiles.get(u.name))
        if msg is not None:
            differing.append(msg)
    print("%s %s %dx%dx%d round %d: %d units, %d with differing words" % (arch, precision, n, h, w, r, len(units), len(differing)), flush=True)
    assert not differing, "\n".join(differing)
