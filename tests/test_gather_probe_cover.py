"""What the nine rounds of the gather probe (tests/helpers/gather_probe.py) reach, computed without a GPU, and the probe's
non-vacuity on a network simulated on the CPU.  Every K position of every conv unit with K <= 9 Cout is selected by some row in
some round; the K = 18 432 units (classifier.0, the ASPP 3x3 branches) have every K-step (a tap x a 32-channel block), every
channel slot of a K-step -- the 32 of f16x2 and fp32 and the 64 of bf16 -- and every residue of the K-step index mod 8 (the flush
cadence) selected.  Whether a border pixel's selected tap lies outside the image is geometry alone, so that condition of the
probe is settled here, per unit and shape over the rounds the GPU test runs there: at least a quarter of the outputs at
image-border pixels of every k > 1 unit come from padding (a 1x1 kernel has no tap to lose, and neither has a border pixel whose
whole window lies inside the image: the bottom row and right column of the one stride-2 3x3 convolution, layer2.0.conv2, on the
even-sized maps of these shapes -- gather_probe.border_share leaves those out)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gather_probe as gp  # noqa: E402
import kept_operands as ko  # noqa: E402

from neuralbarkcalculator_amd import topology  # noqa: E402

FCN, DL = "fcn_resnet50", "deeplabv3_resnet50"
# the GPU test's cases: (arch, (N, H, W), rounds)
CASES = [(FCN, (2, 40, 72), range(gp.ROUNDS)), (FCN, (1, 16, 1024), range(gp.ROUNDS)), (DL, (2, 96, 96), range(gp.ROUNDS)),
         (DL, (1, 640, 640), (0,))]


@pytest.fixture(scope="module", autouse=True)
def _lib(built_lib):
    """the plans come through the library's C ABI: built on a tree that has none, as tests/test_conv_matrix_ledger.py does"""
    return built_lib


def probed(arch):
    return [(i, u) for i, u in enumerate(topology.conv_units(arch)) if u.bn is not None and not u.pooled]


@pytest.mark.parametrize("arch", [FCN, DL])
def test_nine_rounds_select_every_k_position_or_every_k_step(arch):
    long_units = []
    for _, u in probed(arch):
        K = u.cin * u.k * u.k
        pos = np.concatenate([gp.positions(u, r) for r in range(gp.ROUNDS)])
        assert pos.min() >= 0 and pos.max() < K
        for r in range(gp.ROUNDS):
            assert len(set(gp.positions(u, r).tolist())) == min(u.cout, K) or K < u.cout, (u.name, r)
        if not gp.is_long(u):
            assert K <= 4608 and len(np.unique(pos)) == K, (u.name, K, len(np.unique(pos)))
            continue
        long_units.append(u.name)
        assert K == 18432
        for width in (32, 64):                          # channels of a K-step: f16x2 and fp32, bf16
            step, slot = pos // width, pos % width
            assert len(np.unique(step)) == K // width, (u.name, width)
            assert len(np.unique(slot)) == width, (u.name, width)
            assert len(np.unique(step % 8)) == 8
        assert len(np.unique(pos // u.cin)) == 9        # every tap
    assert long_units == (["classifier.0"] if arch == FCN else ["classifier.0.convs.%d.0" % i for i in (1, 2, 3)])


@pytest.mark.parametrize("arch,shape,rounds", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, tuple) else "")
def test_a_quarter_of_the_border_outputs_read_padding(arch, shape, rounds):
    n, h, w = shape
    _, reads, shapes, _ = ko.plan_of(arch, "f16x2", n, h, w)
    head = arch == DL
    for _, u in probed(arch):
        if u.k == 1 or (head and not u.name.startswith("classifier.")):
            continue
        hi, wi = shapes[reads[(u.name, "in")]][2:]
        got = [gp.border_share(u, gp.positions(u, r), hi, wi) for r in rounds]
        share = sum(s * c for s, c in got) / sum(c for _, c in got)
        assert share >= 0.25, (u.name, shape, share)


@pytest.mark.parametrize("arch,shape", [(FCN, (2, 40, 72)), (DL, (2, 96, 96))])
def test_the_simulated_probe_network_is_alive(arch, shape):
    """The probe's conditions on values, on the CPU: every unit of FCN-ResNet-50 at 2 x 40 x 72 and of DeepLabV3-ResNet-50 (trunk,
    ASPP branches, pooled vector, concat, projection, classifier.1) at 2 x 96 x 96, in two rounds, reads a tensor of which at
    least half has a non-zero f16x2 low piece and stores one of which at least a quarter is non-zero; every stored tensor stays
    where the calibration guard wants it, and the activation powers stay 0 (the BatchNorm estimate |beta| + 3 gamma is at most 4)."""
    n, h, w = shape
    x = ko.frames(range(40, 40 + n), h, w).numpy()
    _, reads, shapes, _ = ko.plan_of(arch, "f16x2", n, h, w)
    for r in (0, 4):
        sd, sel = gp.probe_state_dict(arch, r)
        acts = gp.simulate(arch, sd, sel, reads, x, "f16x2")
        for name in acts:
            assert acts[name].shape == shapes[name] and np.isfinite(acts[name]).all(), (r, name)
        for _, u in probed(arch):
            assert gp.low_piece_share(acts[reads[(u.name, "in")]]) >= 0.5, (r, u.name)
            assert (acts[u.name] != 0).mean() >= 0.25, (r, u.name)
            assert 2.0 ** -8 <= np.abs(acts[u.name]).max() <= 2.0 ** 14, (r, u.name)
            assert 2.0 ** -5 <= (np.abs(sd[u.bn + ".bias"]) + 3 * sd[u.bn + ".weight"]).max() <= 2.0 ** 7
        if arch == DL:
            assert (acts["classifier.0.convs.4"] != 0).any() and acts["classifier.0.concat"].shape[1] == 1280
