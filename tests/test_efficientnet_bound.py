"""The per-element bounds of tests/helpers/efficientnet_bound.py without a GPU.  The depthwise kernel's and the SE kernel's
arithmetic restated on the CPU (emulate_dwconv, emulate_se_gate) stay within the bounds on every element, for every (k, stride)
instantiation, with and without the deferred swish, on maps with ragged tiles; each of the eight seeded faults is rejected on
some element, and the fault that is local to a border column is rejected on a tensor where the error it
causes stays under 4e-6 of the tensor's range -- what the chain tests' max-norm (tests/test_gpu_efficientnet.py) lets pass.  Then
the figures the bound's header states (swish's Lipschitz constant, the two floors), the shape rule of
tests/helpers/kept_operands.py for these networks, and the cover ledger: what the cases of
tests/test_gpu_efficientnet_operands.py contain between them, computed from the topology, the keep-mode plan and the tile rule,
and asserted, so that a later change of shapes cannot make the cover vacuous."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import efficientnet_bound as eb  # noqa: E402
import kept_operands as ko  # noqa: E402
import operand_bound as ob  # noqa: E402

from neuralbarkcalculator_amd import topology  # noqa: E402

MAX_NORM = 4e-6                         # LAYER_RTOL_FP32 of tests/test_gpu_efficientnet.py
# kind: (k, stride, (before, after), in_swish, N, C, Hi, Wi) -> the output map and its tiles
KINDS = {
    "3x3/1": (3, 1, (1, 1), True, 2, 40, 11, 21),            # 11 x 21: 2 x 2 tiles, both ragged
    "3x3/1 read as stored": (3, 1, (1, 1), False, 1, 24, 9, 17),
    "3x3/2 (0,1)": (3, 2, (0, 1), True, 2, 96, 13, 37),      # 6 x 18: 2 x 2 tiles; odd rows: the last reads no pad
    "3x3/2 (1,1)": (3, 2, (1, 1), True, 1, 32, 12, 34),      # 6 x 17
    "5x5/1": (5, 1, (2, 2), True, 3, 33, 9, 19),             # 9 x 19: 2 x 2 tiles
    "5x5/2 (1,2)": (5, 2, (1, 2), True, 2, 48, 14, 40),      # 7 x 20
    "5x5/2 (2,2)": (5, 2, (2, 2), True, 1, 64, 13, 67),      # 7 x 34: 3 tile columns x 2 rows = 6 tiles
}


def make(kind, quiet=False):
    """A depthwise unit with its SE pair as the networks have them.  quiet: the inputs of the last three output columns are 2^-18
    of the rest and every beta is 0, so that what a fault does there is small against the tensor's range and large against the
    element."""
    k, s, pads, in_swish, n, c, hi, wi = KINDS[kind]
    rng = np.random.default_rng(100 * k + 10 * s + c + (7 if quiet else 0))
    gain = np.logspace(-0.5, 0.5, c, dtype=np.float32)[rng.permutation(c)]
    x = rng.standard_normal((n, c, hi, wi), dtype=np.float32) * gain[None, :, None, None] * np.float32(1.5)
    if quiet:
        x[..., wi - 3 * s - k:] *= np.float32(2.0 ** -18)
    else:
        x[0, 0, 0, :4] = (-90.0, -104.0, -87.5, 60.0)         # where expf overflows, where 1 / (1 + e) is subnormal
    w = rng.standard_normal((c, 1, k, k), dtype=np.float32) / np.float32(k)
    bias = np.zeros(c) if quiet else 0.4 * rng.standard_normal(c)
    mean = np.zeros(c) if quiet else 0.2 * rng.standard_normal(c)
    alpha, beta = ob.bn_pair(rng.uniform(0.5, 1.5, c), bias, mean, rng.uniform(0.25, 1.0, c), eps=topology.BN_EPS_EFFICIENTNET)
    cse = max(1, c // 8)
    se = dict(wr=rng.standard_normal((cse, c, 1, 1), dtype=np.float32) / np.float32(np.sqrt(c)), br=0.3 * rng.standard_normal(cse).astype(np.float32),
              we=rng.standard_normal((c, cse, 1, 1), dtype=np.float32) / np.float32(np.sqrt(cse)), be=0.5 * rng.standard_normal(c).astype(np.float32))
    return dict(x=x, w=w, alpha=alpha, beta=beta, stride=s, pads=pads, in_swish=in_swish), se


_CASES = {}


def case(kind, quiet=False):
    """The unit, its faithful emulation, the float64 references and the bounds: computed once, shared, never written to."""
    if (kind, quiet) not in _CASES:
        torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))
        u, se = make(kind, quiet)
        k = u["w"].shape[-1]
        v_ref, mag, wsum = eb.dwconv_reference(**u)
        y_ref, bound = eb.dwconv_bound(v_ref, mag, wsum, u["alpha"], u["beta"], k, u["in_swish"])
        _, tight = eb.dwconv_bound(v_ref, mag, wsum, u["alpha"], u["beta"], k, u["in_swish"], eb.TIGHT)
        y, partials = eb.emulate_dwconv(**u)
        g_ref, g_bound = eb.gate_reference(y, stride=u["stride"], **se)
        for a in (y_ref, bound, tight, y, partials, g_ref, g_bound):
            a.setflags(write=False)
        _CASES[(kind, quiet)] = u, se, y_ref, bound, tight, y, partials, g_ref, g_bound
    return _CASES[(kind, quiet)]


def worst(got, ref, bound):
    r = np.abs(got.astype(np.float64) - ref) / bound
    at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
    return float(r.max()), at


def of_range(got, ref):
    """the chain tests' figure: the largest error over the tensor's largest value"""
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_faithful_depthwise_arithmetic_is_within_the_bound_on_every_element(kind):
    u, se, y_ref, bound, tight, y, partials, _, _ = case(kind)
    k, s, pads, _, n, c, hi, wi = KINDS[kind]
    ho, wo = eb.dw_out(hi, k, s, pads), eb.dw_out(wi, k, s, pads)
    tx, ty = eb.dw_tiles(s, ho, wo)
    assert y.shape == y_ref.shape == (n, c, ho, wo) and partials.shape == (n, tx * ty, c) and np.isfinite(y).all()
    assert tx >= 2 and ty >= 2 and wo % eb.DW_TW and ho % eb.DW_TH[s]                  # ragged on both sides
    assert float(np.abs(y_ref).max()) > 1.0 and (np.abs(y) > 0.05).mean() > 0.25        # a live tensor
    r, at = worst(y, y_ref, bound)
    rt, _ = worst(y, y_ref, tight)
    print("faithful dwconv %-22s %dx%d -> %dx%d, %d tiles: worst %.3f of the bound at %s (granted), %.3f (1 ulp, rounded division)"
          % (kind, hi, wi, ho, wo, tx * ty, r, at, rt), flush=True)
    assert r <= 1.0, (kind, r, at)
    # the partials are the stored values' sums, tile by tile: a plain float64 sum of each tile agrees to the mean's roundings
    th = eb.DW_TH[s]
    for t in (0, tx * ty - 1):
        rows, cols = slice(t // tx * th, (t // tx + 1) * th), slice(t % tx * eb.DW_TW, (t % tx + 1) * eb.DW_TW)
        tile = y[:, :, rows, cols].astype(np.float64)
        assert (np.abs(partials[:, t] - tile.sum(axis=(2, 3))) <= ob.gamma(th * eb.DW_TW) * np.abs(tile).sum(axis=(2, 3)) + 1e-300).all()


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_faithful_gate_arithmetic_is_within_the_bound_on_every_element(kind):
    u, se, _, _, _, y, partials, g_ref, g_bound = case(kind)
    gate = eb.emulate_se_gate(partials, y.shape[2], y.shape[3], u["stride"], **se)
    assert gate.shape == g_ref.shape and (gate > 0).all() and (gate < 1).all()
    assert float(g_ref.max() - g_ref.min()) > 0.3                                       # not a constant
    r, at = worst(gate, g_ref, g_bound)
    rt, _ = worst(gate, g_ref, eb.gate_reference(y, stride=u["stride"], g=eb.TIGHT, **se)[1])
    print("faithful gate   %-22s C %3d cse %2d: worst %.3f of the bound at %s (granted), %.3f (1 ulp, rounded division); the bound "
          "is at most %.2e" % (kind, y.shape[1], se["wr"].shape[0], r, at, rt, float(g_bound.max())), flush=True)
    assert r <= 1.0, (kind, r, at)


def faulty(kind, fault, quiet=False):
    """(what the fault stores, its reference, its bound): the depthwise output for a depthwise fault that changes it, else the
    gate -- from the faithful depthwise output, as the device's gate is checked"""
    u, se, y_ref, bound, _, y, partials, g_ref, g_bound = case(kind, quiet)
    if fault in eb.DW_FAULTS and fault != "ragged_pixels":
        return eb.emulate_dwconv(fault=fault, **u)[0], y_ref, bound
    if fault == "ragged_pixels":
        partials = eb.emulate_dwconv(fault=fault, **u)[1]
    gate = eb.emulate_se_gate(partials, y.shape[2], y.shape[3], u["stride"], fault=None if fault == "ragged_pixels" else fault, **se)
    return gate, g_ref, g_bound


def applies(kind, fault):
    k, s, pads, in_swish = KINDS[kind][:4]
    return not ((fault == "pads_swapped" and pads[0] == pads[1]) or (fault == "no_in_swish" and not in_swish))


def test_every_seeded_fault_is_rejected_on_some_element():
    table = {}
    for kind in KINDS:
        for f in eb.FAULTS:
            if applies(kind, f):
                got, ref, bound = faulty(kind, f)
                r, at = worst(got, ref, bound)
                table[(f, kind)] = r
                print("fault %-14s %-22s %10.3g of the bound at (n, c, y, x) = %-16s %.2e of the tensor's range  %s"
                      % (f, kind, r, at, of_range(got, ref), "rejected" if r > 1 else "passes"), flush=True)
    for f in eb.FAULTS:
        kinds = [k for k in KINDS if (f, k) in table]
        assert kinds and all(table[(f, k)] > 1.0 for k in kinds), (f, {k: table[(f, k)] for k in kinds})
    assert [k for k in KINDS if ("pads_swapped", k) in table] == ["3x3/2 (0,1)", "5x5/2 (1,2)"]


# The fault confined to a border column: on the quiet tensors the chain tests' figure stays under their 4e-6 and the element's
# bound is passed many times over.  For the faults that reach the gate alone (ragged_pixels, tile_area, last_tile, gate_channel)
# this cannot be arranged: the gate's own bound is up to 8e-6 on these units, of the order of 4e-6 of a range of 1, so the bound
# rejects them where they move the gate by more than that -- which they do on every unit above -- and the table prints both
# figures.  The other three (pads_swapped, no_in_swish, channel) change every element of a tensor.
LOCAL = [("tap", "3x3/1"), ("tap", "3x3/2 (0,1)"), ("tap", "5x5/1"), ("tap", "5x5/2 (1,2)")]


@pytest.mark.parametrize("fault,kind", LOCAL)
def test_a_local_fault_is_rejected_where_the_max_norm_lets_it_pass(fault, kind):
    u, se, y_ref, bound, _, y, partials, g_ref, g_bound = case(kind, quiet=True)
    assert worst(y, y_ref, bound)[0] <= 1.0                                             # the faithful arithmetic, here too
    assert worst(eb.emulate_se_gate(partials, y.shape[2], y.shape[3], u["stride"], **se), g_ref, g_bound)[0] <= 1.0
    got, ref, b = faulty(kind, fault, quiet=True)
    r, at = worst(got, ref, b)
    rng = of_range(got, ref)
    print("local fault %-14s %-14s %10.3g of the bound at (n, c, y, x) = %s, %.2e of the tensor's range (the chain tests allow %.0e)"
          % (fault, kind, r, at, rng, MAX_NORM), flush=True)
    assert r > 1.0 and rng < MAX_NORM, (fault, kind, r, rng)


def test_the_figures_the_bound_takes_for_granted():
    """sup |swish'| < 1.1 and sup sigmoid' = 1/4 on a grid in float64; the floors: below -87.4 sigmoid is under the smallest normal
    f32 and |swish| under 2^-119; the emulated f32 swish and sigmoid, whose expf is numpy's, lie within the granted relative
    errors plus the floors of the float64 ones on 2 million values, the overflow range included"""
    t = np.linspace(-60.0, 60.0, 2_400_001)
    sg = eb.sigmoid64(t)
    d = sg * (1.0 + t * (1.0 - sg))
    assert 1.09 < float(np.abs(d).max()) < eb.SWISH_LIPSCHITZ and float((sg * (1 - sg)).max()) <= eb.SIGMOID_LIPSCHITZ
    assert eb.sigmoid64(-87.4) < eb.SIGMOID_FLOOR < eb.sigmoid64(-87.3) and 87.4 * eb.SIGMOID_FLOOR < eb.SWISH_FLOOR
    low = np.linspace(-200.0, -87.4, 100_001)
    assert float(np.abs(eb.swish64(low)).max()) < eb.SWISH_FLOOR
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-110, 110, 1_000_000), rng.standard_normal(1_000_000) * 3]).astype(np.float32)
    for f32, f64, rel, floor in ((eb.swish_f32, eb.swish64, eb.swish_rel(), eb.SWISH_FLOOR),
                                 (eb.sigmoid_f32, eb.sigmoid64, eb.sigmoid_rel(), eb.SIGMOID_FLOOR)):
        ref = f64(x)
        got = f32(x)
        assert np.isfinite(got).all() and float((np.abs(got - ref) / (rel * np.abs(ref) + floor)).max()) <= 1.0
    assert eb.GRANTED == (2.0, 2.5) and eb.TIGHT == (1.0, 0.5) and eb.swish_rel(eb.TIGHT) < eb.swish_rel()
    assert eb.mean_roundings(1, 1) == 16 + 7 + 1 + 3 + 2 + 1 and eb.mean_roundings(2, 9) == 8 + 7 + 3 + 3 + 2 + 1


# ---- the shape rule and the cover ledger: host only, through the library's plan ------------------------------------------------
@pytest.fixture(scope="module")
def plans(built_lib):
    """{case: (units by name, names, reads, shapes)} of the GPU test's cases"""
    out = {}
    for arch, (n, h, w) in eb.GPU_CASES:
        names, reads, shapes, tiles = ko.plan_of(arch, "fp32", n, h, w)
        out[(arch, (n, h, w))] = ({u.name: u for u in topology.conv_units(arch)}, names, reads, shapes, tiles)
    return out


def test_every_op_of_the_plan_has_a_shape_but_the_gated_weights(plans):
    for (arch, (n, h, w)), (units, names, reads, shapes, tiles) in plans.items():
        for name in names:
            if name.endswith(".gated_weights") or name == "upsample_argmax" or name == "classifier.4":
                assert name not in shapes
            else:
                assert name in shapes and len(shapes[name]) == 4 and shapes[name][0] == n and min(shapes[name]) >= 1, (arch, name)
        head = "backbone.model._conv_head"
        assert shapes[head + ".swish"] == shapes[head] == (n, topology.efficientnet_inplanes(topology.efficientnet_variant(arch))) + topology.out_hw(h, w, arch)
        assert shapes["backbone.model._blocks.1._se_expand"] == (n, units["backbone.model._blocks.1._depthwise_conv"].cout, 1, 1)
        for name, u in units.items():
            if u.kind == "dw":
                src = shapes[reads[(name, "in")]]
                assert shapes[name] == (n, u.cout) + tuple(eb.dw_out(v, u.k, u.stride, (u.pad, u.pad_after)) for v in src[2:])
                assert reads[(name[:-len("_depthwise_conv")] + "_se_expand", "in")] == name
    # the ResNet-50 networks: as before the rule knew these (the stem halves, the max-pool halves, layer2 halves, 2048 wide)
    _, _, shapes, _ = ko.plan_of("fcn_resnet50", "f16x2", 2, 104, 136)
    assert shapes["backbone.conv1"] == (2, 64, 52, 68) and shapes["backbone.maxpool"] == (2, 64, 26, 34)
    assert shapes["backbone.layer4.2.conv3"] == (2, 2048, 13, 17) and shapes["classifier.0"] == (2, 512, 13, 17) and len(shapes) == 56


def test_the_cover_ledger_of_the_gpu_cases(plans):
    seen = dict(inst=set(), pads=set(), ragged_columns=0, ragged_rows=0, one_tile=0, one_pixel=0, few_tiles=set(), uneven_tiles=set(),
                bottom_pad=set(), padded_channels=set(), residual=set(), batch=set(), in_swish=set(), even_tiles=set())
    for (arch, (n, h, w)), (units, names, reads, shapes, tiles) in plans.items():
        seen["batch"].add(n)
        for name, u in units.items():
            if u.kind == "conv" and name.endswith("._project_conv"):
                assert (reads.get((name, "res")) is not None) == u.residual
                seen["residual"].add(u.residual)
            if u.kind != "dw":
                continue
            assert (u.k, u.stride) in ((3, 1), (3, 2), (5, 1), (5, 2)) and u.cout_pad % 64 == 0
            hi, wi = shapes[reads[(name, "in")]][2:]
            ho, wo = shapes[name][2:]
            tx, ty = eb.dw_tiles(u.stride, ho, wo)
            t = tx * ty
            seen["inst"].add((u.k, u.stride))
            seen["in_swish"].add(u.in_swish)
            if u.stride == 2:
                seen["pads"].add((u.pad, u.pad_after))
                seen["bottom_pad"].add(eb.reads_after_pad(hi, u.k, 2, (u.pad, u.pad_after)))
                seen["bottom_pad"].add(("columns", eb.reads_after_pad(wi, u.k, 2, (u.pad, u.pad_after))))
            seen["ragged_columns"] += tx >= 2 and wo % eb.DW_TW != 0
            seen["ragged_rows"] += ty >= 2 and ho % eb.DW_TH[u.stride] != 0
            seen["one_tile"] += t == 1
            seen["one_pixel"] += (ho, wo) == (1, 1)
            (seen["few_tiles"] if t < 4 else seen["uneven_tiles"] if t % 4 else seen["even_tiles"]).add(t)
            if u.cout_pad != u.cout:
                seen["padded_channels"].add((u.cout, u.cout_pad))
    print("cover ledger of %d cases: %s" % (len(plans), {k: (sorted(v, key=str) if isinstance(v, set) else v) for k, v in seen.items()}), flush=True)
    assert seen["inst"] == {(3, 1), (3, 2), (5, 1), (5, 2)}
    assert seen["pads"] == {(0, 1), (1, 2), (1, 1), (2, 2)}
    assert seen["ragged_columns"] >= 1 and seen["ragged_rows"] >= 1 and seen["one_tile"] >= 1 and seen["one_pixel"] >= 1
    assert {1, 2, 3} <= seen["few_tiles"] and seen["uneven_tiles"] and seen["even_tiles"]
    assert {True, False, ("columns", True), ("columns", False)} <= seen["bottom_pad"]
    assert {(96, 128), (144, 192)} <= seen["padded_channels"]
    assert seen["residual"] == {True, False} and seen["batch"] == {1, 2, 3} and seen["in_swish"] == {True, False}
    assert len(eb.GPU_CASES) <= 6 and {a for a, _ in eb.GPU_CASES} == {eb.B0F, eb.B0D, eb.B5F, eb.B5D}
