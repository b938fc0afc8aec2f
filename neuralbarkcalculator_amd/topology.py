"""Static description of the networks the path runs: the reference's ``fcn_resnet50``, ``deeplabv3_resnet50``,
``fcn_efficientnet(n)`` and ``deeplabv3_efficientnet(n)`` (``models.py:60-110``; named ``fcn_efficientnet_b{n}`` /
``deeplabv3_efficientnet_b{n}`` here).

Restates the layer list of ``/root/reference/src/bark_calculator/models.py:127-139``
(torchvision ``resnet50(replace_stride_with_dilation=[False, True, True])`` cut at
``layer4`` + ``FCNHead(2048, 3)`` from ``models.py:113-124``), or for ``deeplabv3_resnet50``
(``models.py:46-57``) the same trunk + torchvision 0.3's ``DeepLabHead(2048, 3)``, as plain data, so that
the host side can (a) check a state_dict's keys the way ``load_state_dict``
(``models.py:222``) does and (b) walk the conv units in execution order.

The same table exists in C++ (``csrc/nbc_net.cpp``); ``tests/test_abi.py::test_topology_through_the_abi``
checks that the two agree through the C-ABI (``nbc_num_convs`` / ``nbc_conv_info``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

NUM_CLASSES = 3
BN_EPS = 1e-5
BN_EPS_EFFICIENTNET = 1e-3                          # every BatchNorm of the EfficientNet trunk (the heads keep 1e-5)
# name -> NBC_ARCH_* of include/nbc.h (2 is no architecture)
ARCH_IDS = dict([("fcn_resnet50", 0), ("deeplabv3_resnet50", 1)]
                + [(f"fcn_efficientnet_b{n}", 16 + n) for n in range(8)]
                + [(f"deeplabv3_efficientnet_b{n}", 24 + n) for n in range(8)])
ARCHS = tuple(ARCH_IDS)
EFFICIENTNET_ARCHS = tuple(a for a in ARCHS if "efficientnet" in a)
ASPP_RATES = (12, 24, 36)

# efficientnet_pytorch 0.7: stages (repeats, k, stride, expand, in, out), SE ratio 0.25; per variant (width, depth, native size)
EFFICIENTNET_STAGES = ((1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80),
                       (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320))
EFFICIENTNET_PARAMS = ((1.0, 1.0, 224), (1.0, 1.1, 240), (1.1, 1.2, 260), (1.2, 1.4, 300),
                       (1.4, 1.8, 380), (1.6, 2.2, 456), (1.8, 2.6, 528), (2.0, 3.1, 600))
CHANNEL_PAD = 64                                     # EfficientNet tensors: channels zero-padded to a multiple of this


def arch_index(arch) -> int:
    """NBC_ARCH_* of an architecture given by name or id."""
    if isinstance(arch, str):
        if arch not in ARCH_IDS:
            raise ValueError(f"unknown architecture {arch!r}; one of {ARCHS}")
        return ARCH_IDS[arch]
    if int(arch) not in ARCH_IDS.values():
        raise ValueError(f"unknown architecture {arch!r}")
    return int(arch)


def arch_name(arch) -> str:
    """The name of an architecture given by name or NBC_ARCH_* id."""
    a = arch_index(arch)
    return next(k for k, v in ARCH_IDS.items() if v == a)


def is_efficientnet(arch) -> bool:
    return arch_name(arch) in EFFICIENTNET_ARCHS


def efficientnet_variant(arch) -> int:
    return arch_index(arch) & 7


def round_filters(f: int, width: float) -> int:
    """efficientnet_pytorch's channel rounding."""
    x = f * width
    nf = max(8, int(x + 4) // 8 * 8)
    if nf < 0.9 * x:
        nf += 8
    return int(nf)


def efficientnet_inplanes(n: int) -> int:
    """models.py efficientnet_inplanes[n]: channels of the trunk's output."""
    return round_filters(1280, EFFICIENTNET_PARAMS[n][0])


def same_pads(i: int, k: int, s: int) -> Tuple[int, int]:
    """TF-"same" (before, after) pads of Conv2dStaticSamePadding for a native input size i."""
    p = max((-(-i // s) - 1) * s + k - i, 0)
    return p // 2, p - p // 2


def _pad64(c: int) -> int:
    return -(-c // CHANNEL_PAD) * CHANNEL_PAD


@dataclass(frozen=True)
class ConvUnit:
    """One convolution with what is fused behind it."""
    name: str                 # state_dict prefix of the conv ("backbone.layer1.0.conv1")
    bn: Optional[str]         # state_dict prefix of its BatchNorm, None for classifier.4
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    dil: int
    relu: bool
    bias: bool = False
    residual: bool = False    # conv3: += identity before the ReLU
    pooled: bool = False      # the ASPP pooling branch: global average pool, then this 1x1 conv
    # EfficientNet (defaults: the ResNet-50 networks)
    kind: str = "conv"        # "conv", "dw" (depthwise), "se_reduce", "se_expand"
    pad_after: Optional[int] = None   # bottom / right pad (None = pad)
    swish: bool = False       # BatchNorm, then swish
    eps: float = BN_EPS
    cin_pad: Optional[int] = None     # channels of the stored tensors (None = cin / cout)
    cout_pad: Optional[int] = None
    block: int = -1
    in_swish: bool = False    # depthwise: applies the swish its stored input was written without


def _efficientnet_units(arch) -> List[ConvUnit]:
    width, depth, native = EFFICIENTNET_PARAMS[efficientnet_variant(arch)]
    m = "backbone.model."
    units: List[ConvUnit] = []

    def unit(name, bn, cin, cout, k, s, pads, kind, swish, bias=False, residual=False, block=-1, in_swish=False):
        cin_pad = 4 if cin == 3 else (cin if kind == "se_expand" else _pad64(cin))
        cout_pad = cout if kind == "se_reduce" else _pad64(cout)
        units.append(ConvUnit(name, bn, cin, cout, k, s, pads[0], 1, False, bias, residual, kind=kind, pad_after=pads[1],
                              swish=swish, eps=BN_EPS_EFFICIENTNET, cin_pad=cin_pad, cout_pad=cout_pad, block=block,
                              in_swish=in_swish))

    size = native
    unit(m + "_conv_stem", m + "_bn0", 3, round_filters(32, width), 3, 2, same_pads(size, 3, 2), "conv", True)
    size = -(-size // 2)
    bi, prev_swish = 0, True
    for reps, k, stride, expand, c_in, c_out in EFFICIENTNET_STAGES:
        for r in range(int(math.ceil(depth * reps))):
            cin = round_filters(c_in if r == 0 else c_out, width)
            cout = round_filters(c_out, width)
            s = stride if r == 0 else 1
            cexp = cin * expand
            b = f"{m}_blocks.{bi}."
            if expand != 1:
                unit(b + "_expand_conv", b + "_bn0", cin, cexp, 1, 1, (0, 0), "conv", True, block=bi)
            unit(b + "_depthwise_conv", b + "_bn1", cexp, cexp, k, s, same_pads(size, k, s), "dw", True, block=bi,
                 in_swish=expand != 1 or prev_swish)
            size = -(-size // s)
            cse = max(1, int(cin * 0.25))
            unit(b + "_se_reduce", None, cexp, cse, 1, 1, (0, 0), "se_reduce", True, bias=True, block=bi)
            unit(b + "_se_expand", None, cse, cexp, 1, 1, (0, 0), "se_expand", False, bias=True, block=bi)
            unit(b + "_project_conv", b + "_bn2", cexp, cout, 1, 1, (0, 0), "conv", False, residual=(s == 1 and cin == cout),
                 block=bi)
            bi += 1
            prev_swish = False
    inplanes = round_filters(1280, width)
    unit(m + "_conv_head", m + "_bn1", round_filters(320, width), inplanes, 1, 1, (0, 0), "conv", True)

    def head(name, bn, cin, cout, k, pad, relu, bias=False, pooled=False):
        units.append(ConvUnit(name, bn, cin, cout, k, 1, pad, pad if k == 3 else 1, relu, bias, pooled=pooled,
                              cin_pad=_pad64(cin), cout_pad=cout if (bn is None or pooled) else _pad64(cout)))

    if arch_name(arch).startswith("deeplabv3"):
        head("classifier.0.convs.0.0", "classifier.0.convs.0.1", inplanes, 256, 1, 0, True)
        for i, r in enumerate(ASPP_RATES, start=1):
            head(f"classifier.0.convs.{i}.0", f"classifier.0.convs.{i}.1", inplanes, 256, 3, r, True)
        head("classifier.0.convs.4.1", "classifier.0.convs.4.2", inplanes, 256, 1, 0, True, pooled=True)
        head("classifier.0.project.0", "classifier.0.project.1", 1280, 256, 1, 0, True)
        head("classifier.1", "classifier.2", 256, 256, 3, 1, True)
        head("classifier.4", None, 256, NUM_CLASSES, 1, 0, False, bias=True)
    else:
        head("classifier.0", "classifier.1", inplanes, inplanes // 4, 3, 1, True)
        head("classifier.4", None, inplanes // 4, NUM_CLASSES, 1, 0, False, bias=True)
    return units


def conv_units(arch="fcn_resnet50") -> List[ConvUnit]:
    """The conv units of ``arch`` in execution order."""
    a = arch_index(arch)
    if is_efficientnet(a):
        return _efficientnet_units(a)
    units = [ConvUnit("backbone.conv1", "backbone.bn1", 3, 64, 7, 2, 3, 1, True)]
    inplanes, dilation = 64, 1
    for li, (planes, blocks, stride, dilate) in enumerate(
            [(64, 3, 1, False), (128, 4, 2, False), (256, 6, 2, True), (512, 3, 2, True)], start=1):
        prev_dil = dilation
        if dilate:
            dilation *= stride
            stride = 1
        for bi in range(blocks):
            p = f"backbone.layer{li}.{bi}"
            s = stride if bi == 0 else 1
            d = prev_dil if bi == 0 else dilation
            units.append(ConvUnit(p + ".conv1", p + ".bn1", inplanes, planes, 1, 1, 0, 1, True))
            units.append(ConvUnit(p + ".conv2", p + ".bn2", planes, planes, 3, s, d, d, True))
            if bi == 0:
                units.append(ConvUnit(p + ".downsample.0", p + ".downsample.1",
                                      inplanes, planes * 4, 1, s, 0, 1, False))
            units.append(ConvUnit(p + ".conv3", p + ".bn3", planes, planes * 4, 1, 1, 0, 1, True,
                                  residual=True))
            inplanes = planes * 4
    if a == 1:
        # DeepLabHead: ASPP branches (1x1, three dilated 3x3, pooling), the projection, a 3x3 conv, the classifier
        units.append(ConvUnit("classifier.0.convs.0.0", "classifier.0.convs.0.1", 2048, 256, 1, 1, 0, 1, True))
        for i, r in enumerate(ASPP_RATES, start=1):
            units.append(ConvUnit(f"classifier.0.convs.{i}.0", f"classifier.0.convs.{i}.1", 2048, 256, 3, 1, r, r, True))
        units.append(ConvUnit("classifier.0.convs.4.1", "classifier.0.convs.4.2", 2048, 256, 1, 1, 0, 1, True, pooled=True))
        units.append(ConvUnit("classifier.0.project.0", "classifier.0.project.1", 1280, 256, 1, 1, 0, 1, True))
        units.append(ConvUnit("classifier.1", "classifier.2", 256, 256, 3, 1, 1, 1, True))
        units.append(ConvUnit("classifier.4", None, 256, NUM_CLASSES, 1, 1, 0, 1, False, bias=True))
        return units
    units.append(ConvUnit("classifier.0", "classifier.1", 2048, 512, 3, 1, 1, 1, True))
    units.append(ConvUnit("classifier.4", None, 512, NUM_CLASSES, 1, 1, 0, 1, False, bias=True))
    return units


def state_dict_spec(arch="fcn_resnet50") -> List[Tuple[str, Tuple[int, ...], str]]:
    """(key, shape, dtype) of ``arch``'s state_dict in ``nn.Module.state_dict()`` order."""
    spec = []

    def bn(prefix, c):
        spec.append((prefix + ".weight", (c,), "float32"))
        spec.append((prefix + ".bias", (c,), "float32"))
        spec.append((prefix + ".running_mean", (c,), "float32"))
        spec.append((prefix + ".running_var", (c,), "float32"))
        spec.append((prefix + ".num_batches_tracked", (), "int64"))

    # nn.Module order inside a Bottleneck: conv1,bn1,conv2,bn2,conv3,bn3,downsample.{0,1}
    units = {u.name: u for u in conv_units(arch)}
    ordered = []
    for u in conv_units(arch):
        if u.name.endswith(".downsample.0"):
            continue
        ordered.append(u)
        if u.name.endswith(".conv3"):
            ds = u.name[:-len("conv3")] + "downsample.0"
            if ds in units:
                ordered.append(units[ds])
    for u in ordered:
        if u.name in ("classifier.0", "classifier.0.convs.0.0") and is_efficientnet(arch):
            c = efficientnet_inplanes(efficientnet_variant(arch))     # the unused ImageNet classifier ends the trunk
            spec.append(("backbone.model._fc.weight", (1000, c), "float32"))
            spec.append(("backbone.model._fc.bias", (1000,), "float32"))
        spec.append((u.name + ".weight", (u.cout, 1 if u.kind == "dw" else u.cin, u.k, u.k), "float32"))
        if u.bias:
            spec.append((u.name + ".bias", (u.cout,), "float32"))
        if u.bn is not None:
            bn(u.bn, u.cout)
    return spec


def out_hw(h: int, w: int, arch="fcn_resnet50") -> Tuple[int, int]:
    """Spatial size of the low-resolution logits for an ``h x w`` input (three stride-2 stages; EfficientNet: its five
    stride-2 convolutions with their fixed pads, ``floor((h + before + after - k) / 2) + 1`` each)."""
    if is_efficientnet(arch):
        for u in conv_units(arch):
            if u.stride == 2:
                h = max(h + u.pad + u.pad_after - u.k, -2) // 2 + 1
                w = max(w + u.pad + u.pad_after - u.k, -2) // 2 + 1
        return h, w
    for _ in range(3):
        h = (h - 1) // 2 + 1
        w = (w - 1) // 2 + 1
    return h, w
