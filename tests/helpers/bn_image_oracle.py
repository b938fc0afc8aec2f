"""CPU oracle of FCN-ResNet-50 with per-image BatchNorm statistics, as the shipped tool runs it (test infrastructure only;
no product module imports it).

The shipped ``NeuralBarkCalculator`` never calls ``.eval()`` and feeds one image per forward (models.py:212-250), so every
BatchNorm normalises by the image's own per-channel mean and biased variance.  Here: the FCN oracle of
``oracle.fcn_resnet50_oracle`` with every BatchNorm in train mode at ``momentum = 0`` (the running buffers never move),
Dropout in eval (its expectation: the one difference left from the shipped tool), and one image per forward.
``double_of`` gives the float64 form used to adjudicate ties.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.fcn_resnet50_oracle import NUM_CLASSES, OracleFCNResNet50
from oracle.fcn_resnet50_oracle import layer_outputs as _layer_outputs


def image_mode(model: OracleFCNResNet50) -> OracleFCNResNet50:
    """In place: BatchNorm on batch statistics with momentum 0, Dropout the identity."""
    model.eval()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.train()
            m.momentum = 0.0
    return model


def load(sd) -> OracleFCNResNet50:
    m = OracleFCNResNet50()
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return image_mode(m)


def double_of(model: OracleFCNResNet50) -> OracleFCNResNet50:
    return image_mode(copy.deepcopy(model).double())


@torch.no_grad()
def lowres_logits(model: OracleFCNResNet50, x: torch.Tensor) -> torch.Tensor:
    return torch.cat([model.lowres_logits(x[i:i + 1]) for i in range(x.shape[0])])


@torch.no_grad()
def predict_labels(model: OracleFCNResNet50, x: torch.Tensor):
    """(labels int64 [N,H,W], counts int64 [N,3], logits [N,3,H,W], lowres [N,3,h,w]), one image per forward."""
    lowres = lowres_logits(model, x)
    logits = F.interpolate(lowres, size=x.shape[-2:], mode="bicubic", align_corners=False)
    labels = torch.argmax(logits, dim=1)
    counts = torch.stack([(labels == c).flatten(1).sum(1) for c in range(NUM_CLASSES)], dim=1)
    return labels, counts, logits, lowres


@torch.no_grad()
def layer_outputs(model: OracleFCNResNet50, x: torch.Tensor):
    """Every conv unit's output (post BatchNorm / identity / ReLU) and the max-pool, like ``layer_outputs`` of the FCN
    oracle, one image per forward, concatenated over the batch."""
    per = [_layer_outputs(model, x[i:i + 1]) for i in range(x.shape[0])]
    return {k: torch.cat([p[k] for p in per]) for k in per[0]}
