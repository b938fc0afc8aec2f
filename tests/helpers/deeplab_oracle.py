"""CPU oracle of ``deeplabv3_resnet50`` for the tests (test infrastructure only; no product module imports it).

``deeplabv3_resnet50()`` of the reference (models.py:46-57) = the dilated ResNet-50 trunk of the FCN oracle +
torchvision 0.3's ``DeepLabHead(2048, 3)`` + the bicubic x8 upsample of ``SimpleSegmentationModel`` (models.py:27-43).
The head is restated here in torch with child names that give exactly the 362 state_dict keys:

    classifier = Sequential(ASPP(2048, [12, 24, 36]), Conv2d(256, 256, 3, padding=1, bias=False), BatchNorm2d(256), ReLU(),
                            Conv2d(256, 3, 1))
    ASPP.convs = [1x1 conv + BN + ReLU, three 3x3 convs at padding = dilation = 12 / 24 / 36 + BN + ReLU,
                  AdaptiveAvgPool2d(1) + 1x1 conv + BN + ReLU + bilinear resize back (a broadcast)]
    ASPP.project = 1x1 conv 1280 -> 256 + BN + ReLU + Dropout(0.5)

Eval mode by construction: Dropout is the identity.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.fcn_resnet50_oracle import NUM_CLASSES, DilatedResNet50Trunk


class ASPPConv(nn.Sequential):
    def __init__(self, in_channels, out_channels, dilation):
        super().__init__(nn.Conv2d(in_channels, out_channels, 3, padding=dilation, dilation=dilation, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())


class ASPPPooling(nn.Sequential):
    def __init__(self, in_channels, out_channels):
        super().__init__(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False),
                         nn.BatchNorm2d(out_channels), nn.ReLU())

    def forward(self, x):
        size = x.shape[-2:]
        x = super().forward(x)
        return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


class ASPP(nn.Module):
    def __init__(self, in_channels, atrous_rates):
        super().__init__()
        out_channels = 256
        modules = [nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU())]
        for rate in atrous_rates:
            modules.append(ASPPConv(in_channels, out_channels, rate))
        modules.append(ASPPPooling(in_channels, out_channels))
        self.convs = nn.ModuleList(modules)
        self.project = nn.Sequential(nn.Conv2d(5 * out_channels, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels),
                                     nn.ReLU(), nn.Dropout(0.5))

    def branches(self, x):
        return [conv(x) for conv in self.convs]

    def forward(self, x):
        return self.project(torch.cat(self.branches(x), dim=1))


class DeepLabHead(nn.Sequential):
    def __init__(self, in_channels, num_classes):
        super().__init__(ASPP(in_channels, [12, 24, 36]), nn.Conv2d(256, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256),
                         nn.ReLU(), nn.Conv2d(256, num_classes, 1))


class OracleDeepLabV3ResNet50(nn.Module):
    """models.py:27-57, eval mode by construction."""

    def __init__(self):
        super().__init__()
        self.backbone = DilatedResNet50Trunk()
        self.classifier = DeepLabHead(2048, NUM_CLASSES)
        self.eval()

    def lowres_logits(self, x):
        return self.classifier(self.backbone(x))

    def forward(self, x):
        y = self.lowres_logits(x)
        return F.interpolate(y, size=x.shape[-2:], mode="bicubic", align_corners=False)


def load(sd_np) -> OracleDeepLabV3ResNet50:
    """The oracle holding a numpy state_dict (strict)."""
    m = OracleDeepLabV3ResNet50()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return m


@torch.no_grad()
def predict_labels(model: OracleDeepLabV3ResNet50, x: torch.Tensor):
    """(labels int64 [N,H,W], counts int64 [N,3], logits f32 [N,3,H,W], lowres f32 [N,3,h,w])."""
    lowres = model.lowres_logits(x)
    logits = F.interpolate(lowres, size=x.shape[-2:], mode="bicubic", align_corners=False)
    labels = torch.argmax(logits, dim=1)
    counts = torch.stack([(labels == c).flatten(1).sum(1) for c in range(NUM_CLASSES)], dim=1)
    return labels, counts, logits, lowres


@torch.no_grad()
def head_outputs(model: OracleDeepLabV3ResNet50, x: torch.Tensor):
    """Every head tensor under the name the library gives it in keep mode: the conv units' outputs, the pooled vector
    ("classifier.0.convs.4", [N,256,1,1]) and the concat ("classifier.0.concat"); plus "layer4" (the trunk's output)."""
    t = model.backbone(x)
    aspp, h = model.classifier[0], model.classifier
    outs = {"layer4": t}
    br = aspp.branches(t)
    for i in range(4):
        outs[f"classifier.0.convs.{i}.0"] = br[i]
    outs["classifier.0.convs.4"] = aspp.convs[4][3](aspp.convs[4][2](aspp.convs[4][1](aspp.convs[4][0](t))))
    cat = torch.cat(br, dim=1)
    outs["classifier.0.concat"] = cat
    p = aspp.project(cat)
    outs["classifier.0.project.0"] = p
    c1 = h[3](h[2](h[1](p)))
    outs["classifier.1"] = c1
    outs["classifier.4"] = h[4](c1)
    return outs
