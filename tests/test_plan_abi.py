"""The launch plan without a GPU (nbc_describe_plan): which (downsample.0, conv3) pairs the builder marks and the buffers it
gives them, that no op writes a buffer it reads, that every read finds the tensor the topology implies -- with the pairs as
two launches and as one --, the pool's sizes, and the launches of an op."""
import json
import os
import sys

import pytest

from neuralbarkcalculator_amd import topology
from neuralbarkcalculator_amd.model import conv_tile_info, describe_plan

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from plan_reads import expected_reads, parse  # noqa: E402

FCN, DL, EFF = "fcn_resnet50", "deeplabv3_resnet50", "fcn_efficientnet_b0"
SHAPES = [(n, h, w) for n in (1, 2, 3) for h, w in ((8, 8), (24, 1024), (40, 72), (72, 136), (128, 128), (520, 1024), (1024, 1024))]
# (architecture, precision, BatchNorm statistics): every precision a network runs in, both modes where per-image is allowed
MODES = ([(FCN, p, "running") for p in ("fp32", "bf16", "f16x2")] + [(FCN, "fp32", "image")] +
         [(DL, p, "running") for p in ("fp32", "bf16", "f16x2")] + [(EFF, "fp32", "running")])
CASES = [m + (keep,) + s for m in MODES for keep in (False, True) for s in SHAPES]


def refused(arch, bn, h, w):
    """Per-image statistics refuse a 1x1 low-resolution map; EfficientNet-B0 has no output pixel left on 8 or 24 rows."""
    return (bn == "image" and (h, w) == (8, 8)) or (arch == EFF and h < 40)


@pytest.fixture(scope="module")
def plans(built_lib):
    out = {}
    for case in CASES:
        arch, prec, bn, keep, n, h, w = case
        if refused(arch, bn, h, w):
            with pytest.raises(RuntimeError, match="Expected more than 1 value per channel" if bn == "image" else "too small"):
                describe_plan(arch, prec, n, h, w, keep, bn)
        else:
            out[case] = parse(describe_plan(arch, prec, n, h, w, keep, bn))
    return out


def test_tiles_are_those_recorded_before_the_menu_became_one_table(built_lib, plans):
    """tests/golden/plan_tiles.json, recorded from the revision whose tile menu was still spread over switches, id lists and
    parallel arrays: the planned tile of every conv launch of every plan (recorded without keep-activations, which changed no
    tile then and may change none now), nbc_default_conv_tile over the grid test_abi.py walks, and which precision has which
    of the 21 tiles."""
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "plan_tiles.json")))
    assert len(plans) == 2 * len(gold["plans"]) == 318
    for (arch, prec, bn, keep, n, h, w), (ops, bufs, identity) in plans.items():
        want = gold["plans"][" ".join(str(x) for x in (arch, prec, bn, n, h, w))]
        assert [o["tile"] for o in ops if o["kernel"] == "conv_dma"] == want, (arch, prec, bn, keep, n, h, w)
    g = gold["default_tile"]
    got = [built_lib.nbc_default_conv_tile(m, co, k, p) for p in g["precision"] for co in g["cout"] for m in g["m"] for k in g["k"]]
    assert len(got) == 3 * 6 * 8 * 4 and got == g["tile"]
    exists = [[int(conv_tile_info(p, t) is not None) for t in range(21)] for p in ("fp32", "bf16", "f16x2")]
    assert exists == gold["exists"]
    kinds = {conv_tile_info("f16x2", t)[2] for t in (18, 20)}, conv_tile_info("f16x2", 19)[2], {conv_tile_info(p, t)[2] for p in ("fp32", "bf16", "f16x2") for t in range(18) if conv_tile_info(p, t)}
    assert kinds == ({1}, 2, {0})


# what an op reads and writes, by kernel, as fields of its line.  bn_stats names the tensor it reads as `out` as well and
# writes the BatchNorm workspace only; aspp_pool writes its workspace before it reads it; se_excite's `gate` is its
# output once more; bn_apply and swish work in place.
IO = {"ingest": ((), ("out",)), "conv_dma": (("in", "res", "gate"), ("out",)), "maxpool": (("in",), ("out",)),
      "head1x1": (("in",), ()), "upsample_argmax": ((), ()), "aspp_pool": (("in",), ("ws", "out")),
      "concat": (("cat",), ("out",)), "bn_stats": (("in",), ()), "bn_apply": (("in", "res"), ("out",)),
      "dwconv": (("in",), ("ws", "out")), "se_excite": (("in",), ("out",)), "gate_weights": (("gate",), ("ws",)),
      "swish": (("in",), ("out",))}
IN_PLACE = ("bn_apply", "swish")


def fields(o, names):
    """[(field, buffer)] of the named fields the op has; the concat's five inputs as cat0 .. cat4"""
    out = []
    for f in names:
        if f == "cat":
            out += [("cat%d" % i, b) for i, b in enumerate(o["cat"])]
        elif f in o:
            out.append((f, o[f]))
    return out


def pairs_of(ops):
    return [(ops[i - 1], o) for i, o in enumerate(ops) if "ds" in o]


def test_three_pairs_in_f16x2_with_running_statistics_and_none_elsewhere(plans):
    for (arch, prec, bn, keep, n, h, w), (ops, bufs, identity) in plans.items():
        case = (arch, prec, bn, keep, n, h, w)
        got = [(d["name"], o["name"], o["ds"]) for d, o in pairs_of(ops)]
        if arch in (FCN, DL) and prec == "f16x2" and bn == "running" and not keep:
            want = [("backbone.layer%d.0.downsample.0" % s, "backbone.layer%d.0.conv3" % s, "backbone.layer%d.0.downsample.0" % s)
                    for s in (1, 2, 3)]                      # the op in front of conv3 is the one it names; layer4.0: no pair
            assert got == want and identity is not None, case
        else:
            assert got == [] and identity is None, case


def test_a_pair_s_buffers_serve_both_launch_forms(plans):
    seen = 0
    for case, (ops, bufs, identity) in plans.items():
        for d, o in pairs_of(ops):
            seen += 1
            assert o["out"] not in (o["in"], d["in"]), case      # the one launch reads both while it writes
            assert d["out"] == identity and o["res"] == identity, case
            assert "res" not in d and len({d["in"], o["in"], o["out"], identity}) == 4, case
        users = [o["name"] for o in ops if identity is not None and identity in [b for _, b in fields(o, ("in", "out", "res", "ws", "gate", "cat"))]]
        assert users == [x["name"] for p in pairs_of(ops) for x in p], case   # nobody else names the identity buffer
    assert seen == 3 * 2 * len(SHAPES)


def test_no_op_writes_a_buffer_it_reads(plans):
    for case, (ops, bufs, identity) in plans.items():
        for o in ops:
            reads, writes = IO[o["kernel"]]
            if o["kernel"] in IN_PLACE:
                assert o["in"] == o["out"], (case, o)
                continue
            r, w = fields(o, reads), fields(o, writes)
            assert not {b for _, b in r} & {b for _, b in w}, (case, o)
            assert len({b for _, b in w}) == len(w), (case, o)
            for _, b in r + w:
                assert 0 <= b < len(bufs), (case, o)


def replay(ops, fused):
    """{(op, field): the op that last wrote the buffer read there}, the ops taken in order"""
    by_name = {o["name"]: o for o in ops}
    last, got = {}, {}
    for o in ops:
        if fused and o["name"] in fused:
            continue                                        # the next op's launch computes it and stores nothing
        reads, writes = IO[o["kernel"]]
        r = fields(o, reads)
        if fused and o["name"] in fused.values():
            r = [(f, b) for f, b in r if f != "res"] + [("x2", by_name[o["ds"]]["in"])]
        for f, b in r:
            got[(o["name"], f)] = last.get(b)
        for _, b in fields(o, writes):
            last[b] = o["name"]
    return got


def test_every_read_finds_its_producer_in_both_launch_forms(plans):
    for case, (ops, bufs, identity) in plans.items():
        arch, bn = case[0], case[2]
        names = [o["name"] for o in ops]
        pairs = {d["name"]: o["name"] for d, o in pairs_of(ops)}
        for fused in ([None, pairs] if pairs else [None]):
            got, want = replay(ops, fused), expected_reads(arch, bn, names, fused)
            assert got == want, (case, "fused" if fused else "two launches",
                                 {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})


def pool_and_identity(plan):
    ops, bufs, identity = plan
    return [b for i, b in enumerate(bufs) if i != identity], None if identity is None else bufs[identity]


def test_pool_and_identity_bytes_of_the_flagship_plan(plans):
    # the pool of the revision that paired at run time: its Plan::buf_bytes for the same key
    assert pool_and_identity(plans[(FCN, "f16x2", "running", False, 1, 1024, 1024)]) == ([134217728, 134217728, 33554432], 67108864)
    # 65 x 128 x 1024 x 4: layer3.0.downsample.0's output, that revision's buf_bytes for it with keep-activations on
    assert pool_and_identity(plans[(FCN, "f16x2", "running", False, 1, 520, 1024)]) == ([68157440, 68157440, 17039360], 34078720)
    assert 34078720 == 65 * 128 * 1024 * 4


# Plan::buf_bytes of the plans that hold no pair, dumped once from the revision before the builder marked the pairs
# (the commit "Run downsample.0 inside conv3's launch in f16x2"), its build_plan called from a host program.
M = 1 << 20
KEEP_F16X2_1024 = [16, 64, 16, 16, 16, 64, 64, 16, 16, 64, 16, 16, 64, 32, 8, 32, 32, 8, 8, 32, 8, 8, 32, 8, 8, 32, 16, 16, 64, 64, 16,
                   16, 64, 16, 16, 64, 16, 16, 64, 16, 16, 64, 16, 16, 64, 32, 32, 128, 128, 32, 32, 128, 32, 32, 128, 32]
UNCHANGED = {
    (FCN, "fp32", "running", False, 1, 1024, 1024): [128 * M, 128 * M, 32 * M],
    (FCN, "fp32", "image", False, 1, 1024, 1024): [128 * M, 128 * M, 32 * M],
    (FCN, "bf16", "running", False, 1, 1024, 1024): [64 * M, 64 * M, 16 * M],
    (DL, "fp32", "running", False, 1, 1024, 1024): [128 * M, 128 * M, 32 * M, 16 * M, 16 * M, 2105344, 1024],
    (DL, "bf16", "running", False, 1, 1024, 1024): [64 * M, 64 * M, 16 * M, 8 * M, 8 * M, 2105344, 512],
    (EFF, "fp32", "running", False, 1, 1024, 1024): [128 * M, 64 * M, 64 * M, 64 * M],
    (FCN, "f16x2", "running", True, 1, 1024, 1024): [k * M for k in KEEP_F16X2_1024],
    (FCN, "fp32", "running", True, 1, 1024, 1024): [k * M for k in KEEP_F16X2_1024],
}


@pytest.mark.parametrize("case", list(UNCHANGED), ids=lambda c: "-".join(str(x) for x in c))
def test_plans_without_a_pair_keep_their_buffers(plans, case):
    ops, bufs, identity = plans[case]
    assert identity is None and bufs == UNCHANGED[case]


def test_launches_of_an_op(plans):
    for case, (ops, bufs, identity) in plans.items():
        arch, n = case[0], case[4]
        for o in ops:
            if o["kernel"] == "aspp_pool":
                want = 3                                    # partial sums, their sum, the 1x1 conv
                assert arch == DL and o["name"] == "classifier.0.convs.4", case
            elif o["kernel"] == "bn_stats":
                want = 2
            elif o["kernel"] == "conv_dma" and "gate" in o:
                want = n                                    # the SE-gated project conv: one launch per image
            else:
                want = 1
            assert o["launches"] == want, (case, o)
        assert [o["name"] for o in ops if o["name"].endswith(".stats")] == (
            [u.bn + ".stats" for u in topology.conv_units(arch) if u.bn] if case[2] == "image" else []), case
        if arch == DL:
            assert sum(o["kernel"] == "aspp_pool" for o in ops) == 1, case
    dl_eff = parse(describe_plan("deeplabv3_efficientnet_b0", "fp32", 2, 72, 136))[0]
    assert [(o["name"], o["launches"]) for o in dl_eff if o["kernel"] == "aspp_pool"] == [("classifier.0.convs.4", 3)]


# (network, precision, channels of the trunk's output as stored)
POOL_CASES = [(DL, "fp32", 2048), (DL, "bf16", 2048), (DL, "f16x2", 2048),
              ("deeplabv3_efficientnet_b0", "fp32", 1280), ("deeplabv3_efficientnet_b7", "fp32", 2560)]


@pytest.mark.parametrize("arch,prec,cin", POOL_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("n,h,w", [(2, 72, 136), (1, 1024, 1024)], ids=lambda v: str(v))
def test_one_pooling_branch_for_every_deeplab_head(built_lib, arch, prec, cin, n, h, w):
    """Every DeepLab head has exactly one aspp_pool op, classifier.0.convs.4 in three launches, whose workspace holds the
    slices' partial sums (min(hw, 256) slices per image, hw the trunk output's pixels) and the per-image means, cin floats each;
    no plan holds the `pool` op the EfficientNets had."""
    ops, bufs, identity = parse(describe_plan(arch, prec, n, h, w))
    pools = [o for o in ops if o["kernel"] == "aspp_pool"]
    assert [(o["name"], o["launches"]) for o in pools] == [("classifier.0.convs.4", 3)]
    assert not [o for o in ops if o["kernel"] == "pool"]
    ho, wo = topology.out_hw(h, w, arch)                    # the head keeps the trunk's map: classifier.4's is the trunk's
    hw = ho * wo
    assert bufs[pools[0]["ws"]] == (n * min(hw, 256) + n) * cin * 4


def test_the_text_is_cut_to_the_capacity_and_bad_keys_are_refused(built_lib):
    import ctypes as C
    args = (topology.arch_index(FCN), 2, 1, 40, 72, 0, 0)
    need = built_lib.nbc_describe_plan(*args, None, 0)
    full, short = C.create_string_buffer(need), C.create_string_buffer(b"\xff" * 64, 64)
    assert built_lib.nbc_describe_plan(*args, full, need) == need and len(full.value) == need - 1
    assert built_lib.nbc_describe_plan(*args, short, 32) == need
    assert short.raw[:32] == full.raw[:31] + b"\0" and short.raw[32:] == b"\xff" * 32
    for bad in ((FCN, "f16x2", 0, 40, 72), (FCN, "f16x2", 1, 7, 72), (EFF, "bf16", 1, 40, 72)):
        with pytest.raises(RuntimeError):
            describe_plan(*bad)
    with pytest.raises(RuntimeError, match="per-image"):
        describe_plan(DL, "fp32", 1, 40, 72, False, "image")
