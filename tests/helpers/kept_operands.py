"""What the per-element tests share (tests/test_gpu_bf16_operands.py, tests/test_gpu_f32_grade_operands.py,
tests/test_gpu_gather_probe.py, and the plans of tests/test_gather_probe_cover.py): the keep-mode plan of a network (op names, who produced what each op reads, the shape
each op stores, the planned tile of each conv launch) and one keep-mode forward read back op by op."""
import numpy as np
import torch

from neuralbarkcalculator_amd import synth, topology
from neuralbarkcalculator_amd.model import describe_plan

from plan_reads import expected_reads, parse

DEV = "cuda:0"
ROWSTEP_TILES = (18, 19, 20)            # the row-resident 3x3 kernel of f16x2 (csrc/conv3x3_rows.hip)


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


def conv_out(size, u):
    """a unit's output size; the EfficientNet units carry a bottom / right pad of their own (TF "same", from the native size)"""
    after = u.pad if u.pad_after is None else u.pad_after
    return (size + u.pad + after - u.dil * (u.k - 1) - 1) // u.stride + 1


def plan_of(arch, precision, n, h, w):
    """(op names, producer map, {op: shape of the tensor it stores}, {conv op: planned tile}) of the keep-mode plan; host only"""
    ops = parse(describe_plan(arch, precision, n, h, w, True))[0]
    names = [o["name"] for o in ops]
    tiles = {o["name"]: o["tile"] for o in ops if "tile" in o}
    reads = expected_reads(arch, "running", names, None)
    units = {u.name: u for u in topology.conv_units(arch)}
    shapes = {"ingest": (n, 3, h, w)}
    for name in names:
        src = shapes.get(reads.get((name, "in")))
        if name == "backbone.maxpool":
            shapes[name] = src[:2] + ((src[2] - 1) // 2 + 1, (src[3] - 1) // 2 + 1)
        elif name == "classifier.0.convs.4":
            shapes[name] = (n, 256, 1, 1)
        elif name == "classifier.0.concat":
            shapes[name] = (n, 1280) + shapes[reads[(name, "cat0")]][2:]
        elif name.endswith(".swish"):                       # in place: its producer's buffer
            shapes[name] = src
        elif name in units and units[name].kind == "se_expand":
            shapes[name] = (n, units[name].cout, 1, 1)       # the gate
        elif name in units and units[name].bn is not None:   # the depthwise convs with their two pads too
            u = units[name]
            shapes[name] = (n, u.cout, conv_out(src[2], u), conv_out(src[3], u))
    return names, reads, shapes, tiles


def stored(m, x, shapes, wanted, tile=-1):
    """({op: what it stored, f32 NCHW}, low-resolution logits) of one keep-mode forward of x at the planned tiles (or with
    `tile` forced where a layer has it)"""
    m.set_conv_tile(tile)
    m.set_keep_activations(True)
    try:
        low = m.lowres_logits(x.to(DEV))
        torch.cuda.synchronize()
        acts = {}
        for name in wanted:
            acts[name] = m.read_activation(name, int(np.prod(shapes[name]))).copy()
            assert acts[name].shape == shapes[name], (name, acts[name].shape, shapes[name])
        return acts, low.cpu().numpy()
    finally:
        m.set_keep_activations(False)
        m.set_conv_tile(-1)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
