"""Records what the reference's own code returns, as fixtures under tests/golden/ref_*.npz.  TEST INFRASTRUCTURE ONLY.

``python -m oracle.record_reference [--reference DIR] [--out DIR]`` is run by hand on a machine that holds the reference
(default ``/root/reference/src/bark_calculator``); tests/test_reference_pins.py re-runs it into a temporary folder where
that directory exists and compares the result with the committed files.  Nothing else reads the reference.

How the reference's modules are made to import: the packages it names but never calls on the recorded paths
(``STUBBED``: torchvision, skimage, poutyne, efficientnet_pytorch) are put into ``sys.modules`` as empty modules whose
every attribute is an empty class.  ``lovasz_losses``, ``dataset``, ``utils`` and ``models`` then import from their own
directory.  No line of the reference is copied here; the recipe only calls it:

* ``ref_decode``: the decode lines of ``RegressionDatasetFolder.__getitem__`` (dataset.py:188-198) on all 256 grey levels.
  Every target class below goes through the same call, so no fixture depends on our reading of the decode;
* ``ref_loss_<H>x<W>[_k]``: ``LovaszSoftmax``, ``lovasz_softmax_flat(classes=[c])``, ``CrossEntropyLoss``,
  ``CustomWeightedCrossEntropy`` and ``MixedLoss`` (lovasz_losses.py:162-223, utils.py:151-192) of each image as a batch of
  one, for two weight vectors, on the five cases of tests/test_gpu_lovasz.py::_cases and one image with a NaN logit;
* ``ref_stats``: ``compute_mean_std`` and ``compute_pos_weight`` (utils.py:23-69) of a list dataset of four frames;
* ``ref_metrics``: ``lovasz_losses.iou`` and ``sklearn.metrics.f1_score`` as the evaluation loop calls them
  (__main__.py:331, utils.py:219) on three small label / target pairs;
* ``ref_head_<H>x<W>``: the reference's ``SimpleSegmentationModel`` (models.py:27-43) around the reference's
  ``FCNHead(2048, 3)`` (models.py:113-124), in ``eval()``, on OUR trunk (``DilatedResNet50Trunk``: torchvision is absent,
  the trunk stays unpinned), and the ``state_dict`` keys of that head.

Every float result is stored beside ``d_ref``, its distance from our float64 restatement at generation time, and the
recipe refuses to write a loss fixture whose ``d_ref`` exceeds ``D_REF_MAX`` (absolute for the Lovasz values, which lie in
[0, 1]; relative for the cross-entropies): a misread definition moves these values by percent, float32 rounding by 1e-7.
Logits are float16-representable and stored as float16, so the cast back to float32 is exact.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_REFERENCE = "/root/reference/src/bark_calculator"
DEFAULT_OUT = os.path.join(REPO, "tests", "golden")
STUBBED = ["torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.models",
           "torchvision.models.segmentation", "torchvision.models.segmentation.deeplabv3", "torchvision.models.detection",
           "torchvision.models.detection.backbone_utils", "skimage", "skimage.morphology", "skimage.segmentation",
           "skimage.transform", "skimage.io", "poutyne", "poutyne.framework", "poutyne.framework.callbacks",
           "efficientnet_pytorch"]
D_REF_MAX = 1e-6
LOSS_SHAPES = [(1, 1), (1, 7), (33, 65), (65, 127)]
SECOND_WEIGHTS = (1.5, 0.25, 7.0)              # no two alike, no order shared with get_pos_weight(): a swapped index shows
FILE_BUDGET = 160 * 1024                       # bytes of logits + dual per fixture file (the largest committed one: 181 KB)
HEAD_INPUTS = [(3, 64, 64), (4, 40, 72)]       # synth.make_input(index, H, W)
STATS_FRAMES = [(50, 1, 2), (51, 7, 5), (52, 33, 20), (53, 64, 48)]
TRUNK_NOTE = ("backbone = this repository's DilatedResNet50Trunk (torchvision is absent: the trunk is NOT pinned); "
              "classifier, interpolate and eval() are the reference's")


def _helpers():
    for p in (REPO, os.path.join(REPO, "tests", "helpers")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import lovasz_oracle
    import pixel_ce_oracle
    import reference_pins
    from neuralbarkcalculator_amd import metrics, stats, synth
    global _CPU
    _CPU = reference_pins.cpu_name()
    return lovasz_oracle, pixel_ce_oracle, metrics, stats, synth


def import_reference(directory: str):
    """The reference's modules, imported from ``directory`` with ``STUBBED`` standing in for the absent packages."""
    if not os.path.isfile(os.path.join(directory, "lovasz_losses.py")):
        raise SystemExit("no reference at %s" % directory)
    for name in STUBBED:
        try:
            __import__(name)
            continue                                   # installed after all: use it
        except ImportError:
            pass
        m = types.ModuleType(name)
        m.__path__ = []
        m.__getattr__ = lambda attr: type(attr, (), {})   # every name is an empty class
        sys.modules[name] = m
    sys.path.insert(0, directory)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # `is` with a literal, lovasz_losses.py:209
        import lovasz_losses
        import dataset
        import utils
        import models
    return types.SimpleNamespace(lovasz=lovasz_losses, dataset=dataset, utils=utils, models=models)


def decode(ref, grey: np.ndarray) -> np.ndarray:
    """Target classes of a grey dual [H,W] uint8 as dataset.py:188-198 decodes what ``ToTensor`` yields: int64 [H,W]."""
    ds = object.__new__(ref.dataset.RegressionDatasetFolder)
    ds.in_memory, ds.transform, ds.input_only_transform, ds.include_fname = True, None, None, False
    h, w = grey.shape
    target = torch.from_numpy(np.ascontiguousarray(grey)).float()[None] / 255
    ds.samples = [(torch.zeros(3, h, w), target, "a.png", "sapin")]
    return ds[0][1].reshape(h, w).numpy().astype(np.int64)


def loss_cases(h: int, w: int):
    """The five images of tests/test_gpu_lovasz.py::_cases (random; one class absent; one class everywhere; constant
    logits; saturated +-80) with float16-representable logits, and the random image again with one NaN logit."""
    rng = np.random.default_rng(h * 131 + w)
    logits = (rng.normal(size=(5, 3, h, w)) * 3).astype(np.float16).astype(np.float32)
    grey = rng.integers(0, 256, size=(5, h, w), dtype=np.uint8)
    grey[1] = np.where(rng.random((h, w)) < 0.5, rng.integers(0, 64, size=(h, w)), rng.integers(192, 256, size=(h, w)))
    grey[2] = 130
    logits[3] = np.array([0.5, -1.0, 2.0], np.float32)[:, None, None]
    sat = rng.integers(0, 3, size=(h, w))
    logits[4] = -80
    for c in range(3):
        logits[4, c][sat == c] = 80
    nan = logits[0].copy()
    nan[1, h // 2, w // 3] = np.nan
    return np.concatenate([logits, nan[None]]), np.concatenate([grey, grey[:1]])


_CPU = ""


def _savez(path: str, **arrays) -> None:
    """``np.savez`` with fixed member timestamps (the same arrays give the same bytes on every run), and where the values
    were made: ``torch_version`` and ``cpu`` (tests/helpers/reference_pins.py::cpu_name)."""
    import io
    import zipfile
    arrays = dict(arrays, torch_version=np.array(torch.__version__), cpu=np.array(_CPU))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def _rel(a: float, b: float) -> float:
    if np.isnan(a) and np.isnan(b):
        return 0.0
    return abs(a - b) / abs(b) if b != 0 else abs(a - b)


def record_loss_image(ref, helpers, logits: np.ndarray, grey: np.ndarray, weights: np.ndarray) -> dict:
    """Everything the loss fixtures hold for one image: the reference's values and their d_ref."""
    lo, po, metrics = helpers[0], helpers[1], helpers[2]
    x = torch.from_numpy(logits)[None]
    cls = decode(ref, grey)
    t = torch.from_numpy(cls)[None]
    out = {"classes": cls.astype(np.uint8)}
    with torch.no_grad():
        out["lovasz"] = float(ref.lovasz.LovaszSoftmax()(x, t))
        flat = ref.lovasz.flatten_probas(torch.softmax(x, dim=1), t)
        present = np.array([bool((cls == c).any()) for c in range(3)])
        out["present"] = present
        out["lovasz_terms"] = np.array([float(ref.lovasz.lovasz_softmax_flat(*flat, classes=[c])) if present[c] else 0.0
                                        for c in range(3)])
        out["ce"] = float(torch.nn.CrossEntropyLoss()(x, t))
        out["wce"] = np.array([float(ref.utils.CustomWeightedCrossEntropy(torch.from_numpy(wv))(x, t)) for wv in weights])
        out["mixed"] = np.array([float(ref.utils.MixedLoss(torch.from_numpy(wv))(x, t)) for wv in weights])
    terms64, counts = lo.terms_float64(logits, grey)
    lov64 = metrics.lovasz_loss(terms64, counts)
    wce64 = [po.weighted_float64(logits, cls, [float(v) for v in wv]) for wv in weights]
    nan = bool(np.isnan(logits).any())
    out["d_lovasz"] = 0.0 if nan else abs(out["lovasz"] - lov64)
    out["d_lovasz_terms"] = np.zeros(3) if nan else np.abs(out["lovasz_terms"] - terms64)
    out["d_ce"] = _rel(out["ce"], po.weighted_float64(logits, cls, (1.0, 1.0, 1.0)))
    out["d_wce"] = np.array([_rel(a, b) for a, b in zip(out["wce"], wce64)])
    out["d_mixed"] = np.array([_rel(a, metrics.mixed_loss(b, lov64)) for a, b in zip(out["mixed"], wce64)])
    if nan:
        if not all(np.isnan(v) for v in [out["lovasz"], out["ce"], *out["wce"], *out["mixed"]]):
            raise SystemExit("the NaN image must give NaN losses in the reference")
    else:
        worst = max(out["d_lovasz"], out["d_lovasz_terms"].max(), out["d_ce"], out["d_wce"].max(), out["d_mixed"].max())
        if not worst <= D_REF_MAX:
            raise SystemExit("d_ref %.3g above %.1g: replace the input, do not relax the condition" % (worst, D_REF_MAX))
    return out


def record_losses(ref, helpers, out_dir: str) -> list:
    weights = np.stack([ref.utils.get_pos_weight().numpy().astype(np.float32), np.array(SECOND_WEIGHTS, np.float32)])
    written = []
    for h, w in LOSS_SHAPES:
        logits, grey = loss_cases(h, w)
        per_file = max(1, FILE_BUDGET // (h * w * 7))          # 3 float16 logits + 1 dual byte per pixel
        parts = [list(range(i, min(i + per_file, len(logits)))) for i in range(0, len(logits), per_file)]
        for k, part in enumerate(parts):
            rec = [record_loss_image(ref, helpers, logits[i], grey[i], weights) for i in part]
            name = "ref_loss_%dx%d%s" % (h, w, "" if len(parts) == 1 else "_%d" % k)
            half = logits[part].astype(np.float16)
            assert np.array_equal(half.astype(np.float32), logits[part], equal_nan=True)
            arrays = {"case": np.array(part, np.int64), "logits": half, "grey": grey[part], "weights": weights}
            for key in rec[0]:
                arrays[key] = np.stack([np.asarray(r[key]) for r in rec])
            _savez(os.path.join(out_dir, name + ".npz"), **arrays)
            written.append(name)
    return written


def record_decode(ref, out_dir: str) -> list:
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16)
    _savez(os.path.join(out_dir, "ref_decode.npz"), grey=grey, classes=decode(ref, grey).astype(np.uint8))
    return ["ref_decode"]


def stats_inputs(synth):
    """Four frames of different sizes (one of them 1x2) and a crafted dual each: the three levels the tools write, levels
    next to the two class boundaries, and one dual without a node."""
    rng = np.random.default_rng(4242)
    levels = np.array([0, 127, 255, 63, 64, 191, 192, 3, 130], np.uint8)
    frames, greys = [], []
    for k, (idx, h, w) in enumerate(STATS_FRAMES):
        frames.append(synth.make_frame(idx, h, w))
        g = levels[rng.integers(0, 7 if k == 2 else len(levels), size=(h, w))]
        if k == 2:
            g[g >= 192] = 127
        greys.append(np.ascontiguousarray(g))
    greys[0] = np.array([[255, 64]], np.uint8)
    return frames, greys


def record_stats(ref, helpers, out_dir: str) -> list:
    metrics, stats, synth = helpers[2], helpers[3], helpers[4]
    frames, greys = stats_inputs(synth)
    data = [(torch.from_numpy(f).permute(2, 0, 1).contiguous().float() / 255, torch.from_numpy(decode(ref, g)))
            for f, g in zip(frames, greys)]
    mean, std = ref.utils.compute_mean_std(data)
    pos_weight = ref.utils.compute_pos_weight(data)
    rows = []
    for i, (f, g) in enumerate(zip(frames, greys)):
        v = f.reshape(-1, 3).astype(np.uint64)
        cls = metrics.target_classes(g)
        rows.append([i, f.shape[0], f.shape[1], stats.STATUS_OK] + [int(s) for c in range(3) for s in (v[:, c].sum(), (v[:, c] ** 2).sum())]
                    + [int((cls == y).sum()) for y in range(3)] + [0])
    _, summary = stats.report([{"name": str(i), "wood": "sapin"} for i in range(len(frames))], np.asarray(rows, np.int64))
    d_mean = np.array([_rel(a, b) for a, b in zip(mean, summary["mean"])])
    d_std = np.array([_rel(a, b) for a, b in zip(std, summary["std"])])
    if not max(d_mean.max(), d_std.max()) <= D_REF_MAX:
        raise SystemExit("statistics: d_ref %.3g / %.3g above %.1g" % (d_mean.max(), d_std.max(), D_REF_MAX))
    arrays = {"mean": np.array(mean, np.float64), "std": np.array(std, np.float64), "pos_weight": pos_weight.numpy(),
              "d_mean": d_mean, "d_std": d_std}
    for i, (f, g) in enumerate(zip(frames, greys)):
        arrays["frame_%d" % i], arrays["grey_%d" % i] = f, g
        arrays["classes_%d" % i] = decode(ref, g).astype(np.uint8)
    _savez(os.path.join(out_dir, "ref_stats.npz"), **arrays)
    return ["ref_stats"]


def metrics_inputs():
    """Three label / dual pairs [12,10]: all classes on both sides; class 2 on neither side (the EMPTY case of ``iou``);
    class 1 predicted but not present."""
    rng = np.random.default_rng(99)
    levels = np.array([0, 127, 255], np.uint8)
    pred = rng.integers(0, 3, size=(3, 12, 10)).astype(np.uint8)
    tcls = rng.integers(0, 3, size=(3, 12, 10))
    pred[1], tcls[1] = pred[1] % 2, tcls[1] % 2
    tcls[2][tcls[2] == 1] = 2
    return pred, levels[tcls]


def record_metrics(ref, out_dir: str) -> list:
    from sklearn.metrics import f1_score
    import warnings
    pred, grey = metrics_inputs()
    ious, f1s, classes = [], [], []
    for p, g in zip(pred, grey):
        cls = decode(ref, g)
        outputs = torch.nn.functional.one_hot(torch.from_numpy(p.astype(np.int64)), 3).permute(2, 0, 1)[None].float()
        target = torch.from_numpy(cls)[None]
        ious.append(np.asarray(ref.lovasz.iou(outputs, target), np.float64))                       # __main__.py:331
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                                        # a class on neither side
            f1s.append(np.asarray(f1_score(target.reshape(-1), torch.argmax(outputs, 1).reshape(-1), labels=[0, 1, 2],
                                           average=None), np.float64))                             # utils.py:212-219
        classes.append(cls.astype(np.uint8))
    _savez(os.path.join(out_dir, "ref_metrics.npz"), pred=pred, grey=grey, classes=np.stack(classes), iou=np.stack(ious),
             f1_score=np.stack(f1s))
    return ["ref_metrics"]


def record_head(ref, helpers, out_dir: str) -> list:
    synth = helpers[4]
    from oracle.fcn_resnet50_oracle import DilatedResNet50Trunk, OracleFCNResNet50

    class Backbone(DilatedResNet50Trunk):
        def forward(self, x):
            return {"out": super().forward(x)}

    torch.manual_seed(0)
    model = ref.models.SimpleSegmentationModel(Backbone(), ref.models.FCNHead(2048, 3))
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("trained_like", seed=7).items()}
    model.load_state_dict(sd)
    model.eval()
    ours = OracleFCNResNet50()
    ours.load_state_dict(sd)
    ours64 = OracleFCNResNet50().double()
    ours64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    keys = np.array(list(ref.models.FCNHead(64, 3).state_dict().keys()))
    written = []
    for idx, h, w in HEAD_INPUTS:
        frame = synth.make_frame(idx, h, w)
        x = torch.from_numpy(synth.normalize_frame(frame))[None]
        with torch.no_grad():
            logits = model(x)
            want64 = ours64(x.double())
            if not torch.equal(logits, ours(x)):
                raise SystemExit("head %dx%d: OracleFCNResNet50.forward differs from the reference's forward" % (h, w))
        d_ref = float((logits.double() - want64).abs().max() / want64.abs().max())
        if not d_ref <= 5e-6:
            raise SystemExit("head %dx%d: d_ref %.3g of the logit range" % (h, w, d_ref))
        name = "ref_head_%dx%d" % (h, w)
        _savez(os.path.join(out_dir, name + ".npz"), frame_index=np.int64(idx), frame=frame, logits=logits[0].numpy(),
                 labels=torch.argmax(logits, 1)[0].numpy().astype(np.uint8), d_ref=np.float64(d_ref), head_keys=keys,
                 note=np.array(TRUNK_NOTE))
        written.append(name)
    return written


def record_all(reference: str = DEFAULT_REFERENCE, out_dir: str = DEFAULT_OUT) -> list:
    helpers = _helpers()
    ref = import_reference(reference)
    os.makedirs(out_dir, exist_ok=True)
    torch.set_num_threads(1)                   # one summation order, whatever the machine
    return (record_decode(ref, out_dir) + record_losses(ref, helpers, out_dir) + record_stats(ref, helpers, out_dir)
            + record_metrics(ref, out_dir) + record_head(ref, helpers, out_dir))


def main(argv=None):
    ap = argparse.ArgumentParser(description="record the reference's own results as tests/golden/ref_*.npz")
    ap.add_argument("--reference", default=DEFAULT_REFERENCE, help="directory of the reference's bark_calculator modules")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args(argv)
    for name in record_all(args.reference, args.out):
        print("%s.npz  %d bytes" % (name, os.path.getsize(os.path.join(args.out, name + ".npz"))))


if __name__ == "__main__":
    main()
