"""CPU oracle of fcn_efficientnet(n) / deeplabv3_efficientnet(n) (models.py:60-110) in torch, f32 or float64.

A restatement of efficientnet_pytorch 0.7's ``EfficientNet.from_pretrained('efficientnet-b{n}').extract_features`` in
eval mode (written from its description: neither efficientnet_pytorch nor torchvision's segmentation heads are needed)
and of the FCNHead / DeepLabHead the reference puts on it, then the bicubic upsample of SimpleSegmentationModel.  It
shares no code with the package: the stage table, the channel rounding and the TF-"same" pads are spelled out here.
``forward(..., keep=dict)`` stores every block's output under "backbone.model._blocks.{i}._project_conv" and the trunk's
output under "backbone.model._conv_head".
"""
import math

import torch
import torch.nn.functional as F

STAGES = ((1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80),
          (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320))
PARAMS = {0: (1.0, 1.0, 224), 1: (1.0, 1.1, 240), 2: (1.1, 1.2, 260), 3: (1.2, 1.4, 300),
          4: (1.4, 1.8, 380), 5: (1.6, 2.2, 456), 6: (1.8, 2.6, 528), 7: (2.0, 3.1, 600)}


def round_filters(f, width):
    f *= width
    nf = max(8, int(f + 4) // 8 * 8)
    if nf < 0.9 * f:
        nf += 8
    return int(nf)


def static_same_conv(x, w, stride, native, bias=None, groups=1):
    """Conv2dStaticSamePadding: the pads come from the native size, not from x."""
    k = w.shape[-1]
    out = math.ceil(native / stride)
    pad = max((out - 1) * stride + k - native, 0)
    if pad:
        x = F.pad(x, (pad // 2, pad - pad // 2, pad // 2, pad - pad // 2))
    return F.conv2d(x, w, bias, stride, 0, 1, groups)


def swish(x):
    return x * torch.sigmoid(x)


class EfficientNetOracle:
    def __init__(self, state_dict, n, head, dtype=torch.float32):
        self.n, self.head, self.dtype = n, head, dtype
        self.sd = {k: (torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v))
                   for k, v in state_dict.items()}

    def bn(self, x, p, eps):
        g = self.sd
        return F.batch_norm(x, g[p + ".running_mean"], g[p + ".running_var"], g[p + ".weight"], g[p + ".bias"], False, 0.0, eps)

    def trunk(self, x, keep=None):
        g, m = self.sd, "backbone.model."
        width, depth, size = PARAMS[self.n]
        x = swish(self.bn(static_same_conv(x, g[m + "_conv_stem.weight"], 2, size), m + "_bn0", 1e-3))
        size = math.ceil(size / 2)
        idx = 0
        for reps, k, stride, expand, cin0, cout0 in STAGES:
            for r in range(int(math.ceil(depth * reps))):
                cin = round_filters(cin0 if r == 0 else cout0, width)
                cout = round_filters(cout0, width)
                s = stride if r == 0 else 1
                b = f"{m}_blocks.{idx}."
                inp = x
                if expand != 1:
                    x = swish(self.bn(F.conv2d(x, g[b + "_expand_conv.weight"]), b + "_bn0", 1e-3))
                x = swish(self.bn(static_same_conv(x, g[b + "_depthwise_conv.weight"], s, size, groups=x.shape[1]), b + "_bn1", 1e-3))
                size = math.ceil(size / s)
                q = F.adaptive_avg_pool2d(x, 1)
                q = swish(F.conv2d(q, g[b + "_se_reduce.weight"], g[b + "_se_reduce.bias"]))
                q = F.conv2d(q, g[b + "_se_expand.weight"], g[b + "_se_expand.bias"])
                x = torch.sigmoid(q) * x
                x = self.bn(F.conv2d(x, g[b + "_project_conv.weight"]), b + "_bn2", 1e-3)
                if s == 1 and cin == cout:
                    x = x + inp
                if keep is not None:
                    keep[b + "_project_conv"] = x
                idx += 1
        x = swish(self.bn(F.conv2d(x, g[m + "_conv_head.weight"]), m + "_bn1", 1e-3))
        if keep is not None:
            keep[m + "_conv_head"] = x
        return x

    def classifier(self, x):
        g = self.sd
        if self.head == "fcn":
            x = F.relu(self.bn(F.conv2d(x, g["classifier.0.weight"], padding=1), "classifier.1", 1e-5))
            return F.conv2d(x, g["classifier.4.weight"], g["classifier.4.bias"])
        br = [F.relu(self.bn(F.conv2d(x, g["classifier.0.convs.0.0.weight"]), "classifier.0.convs.0.1", 1e-5))]
        for i, r in enumerate((12, 24, 36), start=1):
            br.append(F.relu(self.bn(F.conv2d(x, g[f"classifier.0.convs.{i}.0.weight"], padding=r, dilation=r),
                                     f"classifier.0.convs.{i}.1", 1e-5)))
        p = F.adaptive_avg_pool2d(x, 1)
        p = F.relu(self.bn(F.conv2d(p, g["classifier.0.convs.4.1.weight"]), "classifier.0.convs.4.2", 1e-5))
        br.append(F.interpolate(p, size=x.shape[-2:], mode="bilinear", align_corners=False))
        x = torch.cat(br, dim=1)
        x = F.relu(self.bn(F.conv2d(x, g["classifier.0.project.0.weight"]), "classifier.0.project.1", 1e-5))
        x = F.relu(self.bn(F.conv2d(x, g["classifier.1.weight"], padding=1), "classifier.2", 1e-5))
        return F.conv2d(x, g["classifier.4.weight"], g["classifier.4.bias"])

    @torch.no_grad()
    def forward(self, x, keep=None):
        """x float [N,3,H,W] (normalised) -> (lowres logits, full-size logits), both in the oracle's dtype."""
        x = x.to(self.dtype)
        low = self.classifier(self.trunk(x, keep))
        full = F.interpolate(low, size=x.shape[-2:], mode="bicubic", align_corners=False)
        return low, full
