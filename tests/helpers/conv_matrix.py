"""The convolution kernel matrix: which tile of the menu (csrc/conv_tiles.hpp) runs on which kind of layer of which network,
as host arithmetic over launch plans (nbc_describe_plan), the menu (nbc_conv_tile_info) and the topology.  Nothing here
touches a GPU.  tests/test_conv_matrix_ledger.py checks the cover this gives; tests/test_gpu_conv_matrix.py runs it.

A tile FITS a layer (conv_tile_ok of csrc/conv_tiles.cpp, restated): the precision has the tile, the tile's columns divide
the layer's stored output channels, and the tile is of the kind of kernel the layer runs on (0: the generic kernel; 1 / 2:
the row-step 3x3 kernel), which the layer's planned tile shows."""
import functools

import numpy as np

from neuralbarkcalculator_amd import model, topology

import plan_reads

PRECISIONS = ("fp32", "bf16", "f16x2")
_RESNET_SHAPES_FCN = ((2, 104, 136), (1, 128, 128), (3, 40, 72))
_RESNET_SHAPES_DEEPLAB = ((1, 296, 296), (2, 104, 136))
_EFFICIENTNET_SHAPES = ((2, 104, 136), (1, 128, 128))
# (architecture, precisions, (N, H, W) shapes)
CASES = (("fcn_resnet50", ("fp32", "f16x2", "bf16"), _RESNET_SHAPES_FCN),
         ("deeplabv3_resnet50", ("fp32", "f16x2", "bf16"), _RESNET_SHAPES_DEEPLAB),
         ("fcn_efficientnet_b0", ("fp32",), _EFFICIENTNET_SHAPES),
         ("deeplabv3_efficientnet_b0", ("fp32",), _EFFICIENTNET_SHAPES))
BIGW_BYTES = 3 << 20                    # f16x2: an identity layer with this many bytes of weights takes the BIGW form (launch_tile)


def flat_cases(cases=CASES):
    """[(arch, precision, (n, h, w))], one per GPU test case."""
    return [(arch, p, s) for arch, precisions, shapes in cases for p in precisions for s in shapes]


def case_id(case):
    arch, precision, (n, h, w) = case
    return "%s-%s-%dx%dx%d" % (arch, precision, n, h, w)


def tile_ids():
    """Every tile id the menu has in some precision."""
    ids, t = [], 0
    while any(model.conv_tile_info(p, t) for p in PRECISIONS):
        ids.append(t)
        t += 1
    return ids


def tiles_of(precision, kind=0):
    """The tiles of `kind` the precision has."""
    return [t for t in tile_ids() if (model.conv_tile_info(precision, t) or (None, None, None))[2] == kind]


def generic_tile_ids():
    """Ids of the generic kernel's tiles (kind 0 in whatever precision has them)."""
    return sorted({t for p in PRECISIONS for t in tiles_of(p)})


def missing_tiles(precision):
    """The generic tiles this precision does not have."""
    return [t for t in generic_tile_ids() if model.conv_tile_info(precision, t) is None]


def library_fits(precision, tile, cout_pad, kind):
    info = model.conv_tile_info(precision, tile)
    return info is not None and cout_pad % info[1] == 0 and info[2] == kind


def form_of(unit):
    """What the kernel has to do on a conv_dma layer, as a short key: the stem's pixel gather (and the asymmetric pads of
    EfficientNet's), else the window (size, stride, dilation), then the epilogue's identity -- with 3 MiB of weights or more the
    BIGW form in f16x2 --, and `gated` for the convolution of an MBConv block that has no activation: the project convolution,
    launched per image on its SE-gated weights."""
    if unit.cin == 3:
        return "stem.asym" if unit.pad_after not in (None, unit.pad) else "stem"
    key = "%dx%d" % (unit.k, unit.k)
    if unit.stride != 1:
        key += "s%d" % unit.stride
    if unit.dil != 1:
        key += "d%d" % unit.dil
    if unit.kind == "conv" and unit.block >= 0 and not unit.swish:
        key += ".gated"
    if unit.residual:
        weights = (unit.cout_pad or unit.cout) * (unit.cin_pad or unit.cin) * unit.k * unit.k * 4
        key += "+id.bigw" if weights >= BIGW_BYTES else "+id"
    return key


@functools.lru_cache(maxsize=None)
def plan(arch, precision, n, h, w, keep):
    return plan_reads.parse(model.describe_plan(arch, precision, n, h, w, keep=keep))


def conv_launches(arch, precision, n, h, w, keep=True):
    """The plan's conv_dma ops in launch order, each with its `unit` (topology.ConvUnit) and stored output channels `co`."""
    units = {u.name: u for u in topology.conv_units(arch)}
    ops = [dict(o) for o in plan(arch, precision, n, h, w, keep)[0] if o["kernel"] == "conv_dma"]
    for o in ops:
        o["unit"] = units[o["name"]]
        o["co"] = o["unit"].cout_pad or o["unit"].cout
    return ops


def planned_kind(precision, op):
    return model.conv_tile_info(precision, op["tile"])[2]


def install_list(arch, precision, n, h, w, tile, fits=library_fits, keep=True):
    """(tiles, took): the per-launch tile list (nbc_set_plan_tiles' order) that puts `tile` on every layer it fits and leaves
    the planned tile elsewhere, and the names of the layers that took it."""
    tiles, took = [], []
    for o in conv_launches(arch, precision, n, h, w, keep):
        if fits(precision, tile, o["co"], planned_kind(precision, o)):
            tiles.append(tile)
            took.append(o["name"])
        else:
            tiles.append(o["tile"])
    return tiles, took


def forms(arch):
    """{layer name: form} of the conv_dma layers of `arch` (those the plan launches on the convolution kernels)."""
    n, h, w = next(shapes for a, _, shapes in CASES if a == arch)[0]
    precision = next(ps for a, ps, _ in CASES if a == arch)[0]
    return {o["name"]: form_of(o["unit"]) for o in conv_launches(arch, precision, n, h, w)}


def ledger(cases, fits=library_fits):
    """{(precision, tile, form): layers} summed over `cases` (flat_cases' entries): what a run of every generic tile of the
    precision on every case puts where."""
    out = {}
    for arch, precision, (n, h, w) in cases:
        form = forms(arch)
        for tile in tiles_of(precision):
            for name in install_list(arch, precision, n, h, w, tile, fits)[1]:
                key = (precision, tile, form[name])
                out[key] = out.get(key, 0) + 1
    return out


def expected_fused_pairs(arch, precision, n, h, w, tile):
    """(downsample.0, conv3) pairs a keep-off forward under nbc_set_conv_tile(tile) runs as one launch: the pairs of the plan
    whose conv3 ends up -- forced where the tile fits, planned elsewhere -- on a tile with the dual-branch form."""
    pairs = 0
    for o in conv_launches(arch, precision, n, h, w, keep=False):
        if "ds" in o:
            t = tile if library_fits(precision, tile, o["co"], planned_kind(precision, o)) else o["tile"]
            pairs += model.conv_tile_info(precision, t)[3]
    return pairs


def readable_ops(arch, precision, n, h, w):
    """[(op name, upper bound of its elements)] of the keep-mode plan's ops that leave a tensor of their own behind
    (everything but the image and an in-place pass), for nbc_read_activation."""
    ops, bufs, _ = plan(arch, precision, n, h, w, True)
    eb = 2 if precision == "bf16" else 4
    return [(o["name"], bufs[o["out"]] // eb) for o in ops
            if "out" in o and o["kernel"] != "ingest" and o.get("in") != o["out"]]


def first_difference(got, want):
    """None when the two f32 arrays hold the same words (NaN payloads and signed zeros count), else (the first index that
    differs, the number of words that differ)."""
    if got.shape != want.shape:
        return ("shape %s against %s" % (got.shape, want.shape), -1)
    a = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    b = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    diff = np.flatnonzero(a.ravel() != b.ravel())
    if diff.size == 0:
        return None
    return (tuple(int(i) for i in np.unravel_index(diff[0], got.shape)), int(diff.size))
