"""Records the reference's own Lovasz-Softmax gradients as tests/golden/lovasz_gradient_ref.npz.  TEST INFRASTRUCTURE ONLY.

usage: python scripts/record_lovasz_gradient.py REFERENCE_DIR [--out tests/golden/lovasz_gradient_ref.npz]

REFERENCE_DIR holds the reference's ``lovasz_losses.py``; the module is imported from there and called, no line of it is copied.
Two 16 x 24 images, one with all three classes and one without class 2.  Per image k:

  logits_k      float32 [3,16,24]
  grey_k        uint8 [16,24], the dual (class = round(2 v / 255))
  probs_k       float64 [3,16,24]: torch.softmax of the logits as float64
  dloss_dprobs_k   float64 [3,16,24]: autograd of ``lovasz_softmax_flat(probs, labels)`` with respect to those probabilities
  dloss_dlogits_k  float64 [3,16,24]: autograd of ``LovaszSoftmax()(logits, labels)`` with respect to the float64 logits
  loss_k        float64: the loss itself

The reference's ``fg = (labels == c).float()`` is float32 whatever the probabilities are, and its ``torch.dot`` refuses mixed dtypes.
So the labels go in as ``WideLabels``, a ``torch.Tensor`` subclass whose ``.float()`` returns float64: the reference's own lines
then run in float64 from the comparison on, and the recorded gradients carry float64 rounding only.

``torch.sort`` leaves the order of equal errors open, so the reference's gradient is defined only where no two errors of a class
are equal: the recorder searches seeds until that holds in both images, and asserts it.
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 16, 24


class WideLabels(torch.Tensor):
    """Labels whose ``.float()`` is float64 (module docstring); comparisons and indexing keep the subclass."""

    def float(self):
        return self.double()


def image(seed: int, classes):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((3, H, W)) * 2.0).astype(np.float32)
    grey = rng.choice(np.array([0, 128, 255], dtype=np.uint8)[list(classes)], size=(H, W)).astype(np.uint8)
    return logits, grey


def tie_free(probs: np.ndarray, labels: np.ndarray) -> bool:
    for c in range(3):
        e = np.abs((labels == c).astype(np.float64) - probs[c]).ravel()
        if np.unique(e).size != e.size or (e == 0).any():
            return False
    return True


def record(ll, seed: int, classes):
    sys.path.insert(0, REPO)
    from neuralbarkcalculator_amd import metrics
    while True:
        logits, grey = image(seed, classes)
        labels = metrics.target_classes(grey)
        x = torch.from_numpy(logits.astype(np.float64))[None].requires_grad_(True)
        probs = torch.softmax(x.detach(), dim=1)
        if tie_free(probs[0].numpy(), labels) and sorted(np.unique(labels)) == sorted(classes):
            break
        seed += 1000
    assert tie_free(probs[0].numpy(), labels)
    lab = torch.from_numpy(labels)[None].as_subclass(WideLabels)
    loss = ll.LovaszSoftmax()(x, lab)
    loss.backward()
    p = probs.clone().requires_grad_(True)
    flat = ll.lovasz_softmax_flat(*ll.flatten_probas(p, lab, None), classes="present")
    flat.backward()
    loss, flat = loss.detach(), flat.detach()
    assert float(flat) == float(loss)
    return {"logits": logits, "grey": grey, "probs": probs[0].numpy(), "dloss_dprobs": p.grad[0].numpy().copy(),
            "dloss_dlogits": x.grad[0].numpy().copy(), "loss": np.float64(float(loss)), "seed": np.int64(seed)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference", help="the directory that holds the reference's lovasz_losses.py")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "lovasz_gradient_ref.npz"))
    args = ap.parse_args()
    if not os.path.isfile(os.path.join(args.reference, "lovasz_losses.py")):
        raise SystemExit("no lovasz_losses.py in %s" % args.reference)
    sys.path.insert(0, args.reference)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # `is` with a literal in the reference
        import lovasz_losses as ll
    out = {}
    for k, (seed, classes) in enumerate([(1, (0, 1, 2)), (2, (0, 1))]):
        for name, value in record(ll, seed, classes).items():
            out["%s_%d" % (name, k)] = value
    np.savez_compressed(args.out, **out)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
