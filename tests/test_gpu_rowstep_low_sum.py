"""The row-step 3x3 kernel's low-piece sum on the device (csrc/conv3x3_rows.hip: the products P X1 summed apart, unscaled, over a
tile's whole K loop and joined once with 2^-11).

The exact gather probe (tests/helpers/gather_probe.py) at 1 x 520 x 1024: 65 map rows of 128 pixels, so classifier.0 has 264 tiles
on tile 20 (33 row pairs x 8 channel tiles) and 260 on tile 18 -- more than the chip has compute units, so some block walks to a
second tile, whose low sum must start from zero.  Restricted to the units whose planned tile is a row-step tile, every probe
round, uint32 equality, once on the planned tiles and once with tile 18 installed.  Under the probe a stored output is one
operand times a power of two: its low piece reaches the output through the low sum alone, at whichever K-step the round selects.
The probe, not the bound, sees a low sum cleared at a flush (the value of a K-step before the last flush loses its low piece), one
joined with another power or not at all, and one carried into a block's next tile.

The rescaled checkpoint of tests/test_gpu_f32_grade_operands.py (every activation at 2^-20 of its usual size) at 1 x 16 x 1024,
where the row-step tiles run (that module runs it at 104 x 136, where none does): every row-step unit within the bound of
tests/helpers/f32_grade_bound.py at c = 2."""
import os
import sys

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import topology
from neuralbarkcalculator_amd.model import MODELS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import f32_grade_bound as fb  # noqa: E402
import gather_probe as gp  # noqa: E402
import kept_operands as ko  # noqa: E402
import operand_bound as ob  # noqa: E402

pytestmark = pytest.mark.gpu
FCN = "fcn_resnet50"
PROBE_SHAPE = (1, 520, 1024)
RESCALED_SHAPE = (1, 16, 1024)
FRAME0 = 40
ROWSTEP_UNITS = 13                      # layer2.1-3, layer3.0-5 and layer4.0-2 conv2, classifier.0

_MODEL = {}


@pytest.fixture(scope="module")
def probe_model(built_lib):
    _MODEL["m"] = MODELS[FCN]("f16x2")
    yield _MODEL["m"]
    _MODEL.clear()


@pytest.fixture(scope="module")
def probe_plan():
    n, h, w = PROBE_SHAPE
    names, reads, shapes, tiles = ko.plan_of(FCN, "f16x2", n, h, w)
    units = [u for u in topology.conv_units(FCN) if u.bn is not None and tiles.get(u.name) in ko.ROWSTEP_TILES]
    return reads, shapes, tiles, units


def test_the_probe_shape_walks(probe_plan):
    """Host arithmetic on the plan: 13 row-step units, tiles 19 and 20 planned, and classifier.0 with more tiles than compute units
    on tile 20 and on tile 18"""
    reads, shapes, tiles, units = probe_plan
    assert len(units) == ROWSTEP_UNITS and {tiles[u.name] for u in units} == {19, 20}
    head = next(u for u in units if u.name == "classifier.0")
    n, c, ho, wo = shapes["classifier.0"]
    assert (ho, wo, c, head.dil) == (65, 128, 512, 1) and tiles["classifier.0"] == 20
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    on20, on18 = n * (ho // 2 + ho % 2) * (c // 64), n * ho * (c // 128)
    assert (on20, on18) == (264, 260) and min(on20, on18) > cus, (on20, on18, cus)


@pytest.mark.parametrize("r", range(gp.ROUNDS), ids=lambda r: "round%d" % r)
def test_rowstep_units_store_the_selected_operand_bit_for_bit(probe_model, probe_plan, r):
    n, h, w = PROBE_SHAPE
    reads, shapes, tiles, units = probe_plan
    sd, sel = gp.probe_state_dict(FCN, r)
    m = probe_model.load_state_dict(sd).to(ko.DEV)
    assert m.pack_flags == 0 and all(m.activation_exponent(u.name) == 0 for u in topology.conv_units(FCN) if u.bn is not None)
    x = ko.frames(range(FRAME0, FRAME0 + n), h, w)
    ok, bad = m.f16x2_range_ok(m.activation_peaks(x.to(ko.DEV)))
    assert ok, bad
    wanted = sorted({u.name for u in units} | {reads[(u.name, "in")] for u in units})
    assert "ingest" not in wanted and not any(u.residual for u in units)
    differing = []
    for tile in (-1, 18):
        acts, low = ko.stored(m, x, shapes, wanted, tile)
        assert not m.nonfinite_seen() and np.isfinite(low).all()
        for u in units:
            xin = acts[reads[(u.name, "in")]]
            pos, sg = sel[u.name]
            want = gp.expected_unit(xin, u, pos, sg, sd[u.bn + ".bias"], None, "f16x2")
            # the reference alone, before any comparison: the probe is not vacuous on these operands
            assert gp.low_piece_share(xin) >= 0.5, (u.name, gp.low_piece_share(xin))
            assert (xin != 0).mean() >= 0.5 and (want != 0).mean() >= 0.25, (u.name, float((want != 0).mean()))
            msg = gp.first_difference(acts[u.name], want, u, pos, tiles[u.name] if tile == -1 else "18 installed (planned %d)" % tiles[u.name])
            if msg is not None:
                differing.append(msg)
    print("probe f16x2 %dx%dx%d round %d: %d row-step units on the planned tiles and with tile 18, %d differing" % (n, h, w, r, len(units), len(differing)),
          flush=True)
    assert not differing, "\n".join(differing)


def test_rescaled_checkpoint_rowstep_units_within_the_bound(sd_np, built_lib):
    """Every tensor between a BatchNorm and the next convolution at 2^-20 of its usual size, on 128-pixel-wide maps"""
    from conftest import rescale_activations
    sd = rescale_activations(sd_np, 2.0 ** -20, "all")
    m = MODELS[FCN]("f16x2").load_state_dict(sd).to(ko.DEV)
    n, h, w = RESCALED_SHAPE
    names, reads, shapes, tiles = ko.plan_of(FCN, "f16x2", n, h, w)
    units = [u for u in topology.conv_units(FCN) if u.bn is not None and tiles.get(u.name) in ko.ROWSTEP_TILES]
    assert len(units) == ROWSTEP_UNITS and {tiles[u.name] for u in units} == {19, 20}
    powers = {u.name: m.activation_exponent(u.name) for u in units}
    assert any(powers.values()), powers
    x = ko.frames(range(20, 20 + n), h, w)
    wanted = sorted({u.name for u in units} | {reads[(u.name, "in")] for u in units})
    acts, low = ko.stored(m, x, shapes, wanted)
    assert m.pack_flags == 0 and not m.nonfinite_seen()
    over = []
    for u in units:
        xin, got = acts[reads[(u.name, "in")]], acts[u.name]
        alpha, beta = ob.bn_pair(sd[u.bn + ".weight"], sd[u.bn + ".bias"], sd[u.bn + ".running_mean"], sd[u.bn + ".running_var"])
        y_ref, mag, tiny = fb.conv_unit_reference(xin, sd[u.name + ".weight"], "f16x2", alpha, beta, None, u.relu, u.stride, u.pad, u.dil)
        assert got.shape == y_ref.shape and np.isfinite(got).all(), u.name
        assert (xin != 0).mean() >= 0.25 and (got != 0).mean() >= 0.05, u.name
        K = u.cin * u.k * u.k
        ratio = np.abs(got.astype(np.float64) - y_ref) / fb.unit_bound("f16x2", y_ref, mag, tiny, alpha, beta, None, K, powers[u.name])
        worst = float(ratio.max())
        print("rescaled f16x2 %dx%dx%d %-28s K %5d tile %2d power %3d  worst %.2e of the bound (c = 2)" % (n, h, w, u.name, K, tiles[u.name], powers[u.name], worst),
              flush=True)
        if worst > 1.0:
            over.append((u.name, worst))
    assert not over, over
