"""The EfficientNet kernels (csrc/efficientnet.hip: dwconv in its four instantiations, se_excite, gate_weights, swish,
head1x1_any) and the conv_dma launches around them, per element on the operands they read.  One keep-mode forward per case at the
planned tiles; every op's stored tensor is read back, every op is evaluated in float64 on the tensors its producers stored (the
producer map of tests/helpers/plan_reads.py), and every stored element must be finite and within the bound of
tests/helpers/efficientnet_bound.py / f32_grade_bound.py -- derived from the roundings of the arithmetic, measured from nothing.
The stem and the expand conv are stored before their swish and the depthwise kernel applies it while staging; the gate is
checked from the stored depthwise output (which checks the squeeze partials, the tiles' order and the mean's divisor); the project
conv is evaluated per image on float32(W gate[n]) with the gate as read back (which checks gate_weights and the per-image
launch); the head conv is read after its in-place swish.  The chain tests (tests/test_gpu_efficientnet.py, the EfficientNet cases
of tests/test_gpu_conv_matrix.py: the largest error over the tensor's largest value, 4e-6, at block outputs) cannot see a fault
confined to a ragged tile, a border column or one step of a sum.  The cases are efficientnet_bound.GPU_CASES;
tests/test_efficientnet_bound.py asserts on the host what they contain between them.  Every case prints its worst ratio per kind
under the granted constants (c = 2; expf 2 ulp, division 2.5 ulp) and under the tighter ones (c = 1; 1 ulp, a correctly rounded
division)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import synth, topology
from neuralbarkcalculator_amd.model import MODELS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import efficientnet_bound as eb  # noqa: E402
import f32_grade_bound as fb  # noqa: E402
import kept_operands as ko  # noqa: E402
import operand_bound as ob  # noqa: E402

pytestmark = pytest.mark.gpu
TRUNK = "backbone.model."


@pytest.fixture(scope="module", autouse=True)
def reference_threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))


@pytest.fixture(scope="module")
def network(built_lib):
    """(state_dict, model) of one architecture at a time: asking for another releases the one before"""
    held = {}

    def get(arch):
        if arch not in held:
            held.clear()
            sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
            held[arch] = (sd, MODELS[arch]("fp32").load_state_dict(sd).to(ko.DEV))
        return held[arch]
    yield get
    held.clear()


def pair_of(sd, u):
    return ob.bn_pair(sd[u.bn + ".weight"], sd[u.bn + ".bias"], sd[u.bn + ".running_mean"], sd[u.bn + ".running_var"], eps=u.eps)


def judge(tag, name, form, kind, got, y_ref, bound, tight, worst):
    """Every element finite and within the bound; the failure names the op, its form, the count over the bound and the worst
    element.  worst: {kind: [under the granted constants, under the tighter ones]}"""
    assert got.shape == y_ref.shape, (tag, name, got.shape, y_ref.shape)
    assert np.isfinite(got).all(), (tag, name)
    err = np.abs(got.astype(np.float64) - y_ref)
    r2 = err / bound
    r1 = float((err / tight).max())
    at = tuple(int(i) for i in np.unravel_index(int(r2.argmax()), r2.shape))
    print("%s %-52s %-30s worst %.4f of the bound (granted), %.4f (tighter)  at %s" % (tag, name, form, float(r2.max()), r1, at), flush=True)
    w = worst.setdefault(kind, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(r2.max())), max(w[1], r1)
    over = int((r2 > 1.0).sum())
    assert over == 0, "%s %s (%s): %d of %d elements over the bound, the worst %.3f times at (n, c, y, x) = %s: got %r, float64 %r" % (
        tag, name, form, over, r2.size, float(r2.max()), at, float(got[at]), float(y_ref[at]))


def conv_unit(u, sd, acts, reads, pads=None):
    """A conv_dma unit on its stored operands: (y_ref before any swish, bound at c = 2, bound at c = 1)"""
    x = acts[reads[(u.name, "in")]]
    res = acts[reads[(u.name, "res")]] if u.residual else None
    alpha, beta = pair_of(sd, u)
    y, mag, _ = fb.conv_unit_reference(x, sd[u.name + ".weight"], "fp32", alpha, beta, res, u.relu, u.stride, u.pad, u.dil, pads=pads)
    K = u.cin * u.k * u.k
    return y, fb.fp32_unit_bound(y, mag, alpha, beta, res, K), fb.fp32_unit_bound(y, mag, alpha, beta, res, K, c=1)


def head_kind(u):
    if u.name.startswith("classifier.0.convs."):
        return "ASPP 1x1" if u.k == 1 else "ASPP 3x3 dilation %d" % u.dil
    return {"classifier.0.project.0": "projection", "classifier.0": "classifier.0 (FCN)", "classifier.1": "classifier.1"}[u.name]


def run_case(m, sd, arch, n, h, w):
    tag = "%s %dx%dx%d" % (arch.replace("_efficientnet_", " "), n, h, w)
    t0 = time.time()
    x = ko.frames(range(50, 50 + n), h, w)
    names, reads, shapes, tiles = ko.plan_of(arch, "fp32", n, h, w)
    wanted = [k for k in shapes if k != "ingest"]
    acts, low = ko.stored(m, x, shapes, wanted)
    assert m.pack_flags == 0 and not m.nonfinite_seen()
    acts["ingest"] = x.numpy()
    units = topology.conv_units(arch)
    by = {u.name: u for u in units}
    worst, checked = {}, set()
    for u in units:
        name = u.name
        if u.kind == "dw":
            src = reads[(name, "in")]
            assert u.in_swish == (src.endswith("_conv_stem") or src.endswith("_expand_conv")), (name, src)
            alpha, beta = pair_of(sd, u)
            v_ref, mag, wsum = eb.dwconv_reference(acts[src], sd[name + ".weight"], alpha, beta, u.stride, (u.pad, u.pad_after), u.in_swish)
            y_ref, bound = eb.dwconv_bound(v_ref, mag, wsum, alpha, beta, u.k, u.in_swish)
            _, tight = eb.dwconv_bound(v_ref, mag, wsum, alpha, beta, u.k, u.in_swish, eb.TIGHT)
            ho, wo = y_ref.shape[2:]
            form = "k %d s %d pads (%d,%d) %dx%d tiles %dx%d%s" % ((u.k, u.stride, u.pad, u.pad_after, ho, wo) + eb.dw_tiles(u.stride, ho, wo)
                                                                 + ("" if u.in_swish else " as stored",))
            judge(tag, name, form, "dwconv %d/%d" % (u.k, u.stride), acts[name], y_ref, bound, tight, worst)
        elif u.kind == "se_reduce":
            continue                                        # inside se_excite, under the name of _se_expand
        elif u.kind == "se_expand":
            blk = name[:-len("_se_expand")]
            dw = by[blk + "_depthwise_conv"]
            assert reads[(name, "in")] == dw.name
            se = (sd[blk + "_se_reduce.weight"], sd[blk + "_se_reduce.bias"], sd[name + ".weight"], sd[name + ".bias"])
            g_ref, bound = eb.gate_reference(acts[dw.name], *se, dw.stride)
            _, tight = eb.gate_reference(acts[dw.name], *se, dw.stride, eb.TIGHT)
            ho, wo = acts[dw.name].shape[2:]
            form = "C %d cse %d tiles %d hw %d" % (u.cout, u.cin, int(np.prod(eb.dw_tiles(dw.stride, ho, wo))), ho * wo)
            judge(tag, name, form, "gate", acts[name], g_ref, bound, tight, worst)
        elif name.endswith("._project_conv"):
            blk = name[:-len("_project_conv")]
            assert reads[(name, "in")] == blk + "_depthwise_conv" and reads[(name, "gate")] == name + ".gated_weights"
            assert reads[(name + ".gated_weights", "gate")] == blk + "_se_expand"
            res = acts[reads[(name, "res")]] if u.residual else None
            alpha, beta = pair_of(sd, u)
            y_ref, bound, tight = eb.project_reference(acts[blk + "_depthwise_conv"], sd[name + ".weight"], acts[blk + "_se_expand"], alpha, beta, res)
            judge(tag, name, "K %d tile %d, %d launches" % (u.cin, tiles[name], n), "project + identity" if u.residual else "project",
                  acts[name], y_ref, bound, tight, worst)
        elif name == TRUNK + "_conv_head":
            v_ref, e2, e1 = conv_unit(u, sd, acts, reads)
            y_ref, bound = eb.swish_after(v_ref, e2)
            _, tight = eb.swish_after(v_ref, e1, eb.TIGHT)
            assert ko.same_bits(acts[name], acts[name + ".swish"])            # one buffer: read after the in-place swish
            checked.add(name + ".swish")
            judge(tag, name, "K %d tile %d, swish in place" % (u.cin, tiles[name]), "head conv + swish", acts[name], y_ref, bound, tight, worst)
        elif u.pooled:
            alpha, beta = pair_of(sd, u)
            trunk = reads[("classifier.0.convs.4", "in")]
            assert trunk == TRUNK + "_conv_head.swish"
            y_ref, bound = fb.pooled_reference(acts[trunk], sd[name + ".weight"], alpha, beta, "fp32")
            judge(tag, "classifier.0.convs.4", "K %d hw %d" % (u.cin, int(np.prod(acts[trunk].shape[2:]))), "pooled", acts["classifier.0.convs.4"],
                  y_ref, bound, bound, worst)
            checked.add("classifier.0.convs.4")
            continue
        elif u.bn is None:
            assert name == "classifier.4"
            y_ref, bound = ob.head_reference(acts[reads[(name, "in")]], sd[name + ".weight"], sd[name + ".bias"])
            judge(tag, name, "K %d" % u.cin, "classifier.4", low, y_ref, bound, bound, worst)
            continue
        else:
            stem = name == TRUNK + "_conv_stem"
            trunk_unit = name.startswith(TRUNK)
            assert stem or name.endswith("._expand_conv") or not trunk_unit, name
            assert u.eps == (topology.BN_EPS_EFFICIENTNET if trunk_unit else topology.BN_EPS) and u.relu == (not trunk_unit)
            y_ref, bound, tight = conv_unit(u, sd, acts, reads, (u.pad, u.pad_after) if stem else None)
            kind = "stem" if stem else "expand" if trunk_unit else head_kind(u)
            judge(tag, name, "K %d tile %d%s" % (u.cin * u.k * u.k, tiles[name], ", before its swish" if trunk_unit else ""), kind,
                  acts[name], y_ref, bound, tight, worst)
        checked.add(name)
    if "classifier.0.concat" in shapes:
        branches = ["classifier.0.convs.%d.0" % i for i in range(4)]
        hh, ww = shapes[branches[0]][2:]
        want = np.concatenate([acts[b] for b in branches] + [np.broadcast_to(acts["classifier.0.convs.4"], (n, 256, hh, ww))], axis=1)
        assert ko.same_bits(acts["classifier.0.concat"], np.ascontiguousarray(want))
        checked.add("classifier.0.concat")
    assert checked == set(wanted), sorted(set(wanted) ^ checked)
    for kind in sorted(worst):
        print("%s worst per kind: %-24s %.4f (granted)  %.4f (tighter)" % (tag, kind, worst[kind][0], worst[kind][1]), flush=True)
    print("%s: %d ops checked in %.1f s" % (tag, len(checked), time.time() - t0), flush=True)
    return worst


@pytest.mark.parametrize("arch,shape", eb.GPU_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_op_on_the_operands_it_read(network, arch, shape):
    sd, m = network(arch)
    worst = run_case(m, sd, arch, *shape)
    want = {"stem", "expand", "gate", "project", "project + identity", "head conv + swish", "classifier.4"}
    want |= {"dwconv %d/%d" % ks for ks in ((3, 1), (3, 2), (5, 1), (5, 2))}
    want |= {"pooled", "projection", "classifier.1", "ASPP 1x1"} if arch.startswith("deeplabv3") else {"classifier.0 (FCN)"}
    assert want <= set(worst), sorted(want - set(worst))
