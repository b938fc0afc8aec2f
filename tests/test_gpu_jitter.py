"""The colour-jitter views on the GPU (nbc_jitter_views, nbc_views_mean, FCNResNet50.predict_labels_jitter, predict / evaluate
--jitter).  The kernels are compared byte for byte and bit for bit with the numpy restatement of tests/helpers/jitter_oracle.py
(itself held to PIL's ImageEnhance in tests/test_jitter_abi.py); the stacked forward with single forwards of the oracle-made
views, bit for bit; the logits with the CPU oracle run on each PIL-made view, under the tolerances of tests/test_gpu_parity.py."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from neuralbarkcalculator_amd import _lib, folder_run, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import FCNResNet50, fcn_efficientnet, resolve_jitter_views

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import jitter_oracle as jo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the constants of tests/test_gpu_parity.py (LOGIT_RTOL_FP32, LOGIT_RTOL_BF16, MAX_TIE_FLIPS_FRAC), restated
LOGIT_RTOL_FP32 = 5e-6
LOGIT_RTOL_BF16 = 4e-2
MAX_TIE_FLIPS_FRAC = 4e-6


def u8_frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_frame(int(i), h, w) for i in idx]))


@pytest.fixture(scope="module")
def models(sd_np, built_lib):
    return {m: FCNResNet50(m).load_state_dict(sd_np).to(DEV) for m in ("fp32", "f16x2", "bf16")}


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(got, want):
    """Bitwise equality, NaN positions compared as a mask."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ---- 1. the views kernel ---------------------------------------------------------------------------------------------------
VIEW_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 8, 21), (1, 8, 22), (3, 40, 72), (1, 129, 65)]
CONTRAST_SET = [(1, 0.5, 1), (0.9, 1.2, 1), (0.9, 0.8, 1.1), (1.1, 2, 0.5)]            # contrast in every view; two views share b
SIXTEEN = [(1, 1, 1), (0.9, 1, 1), (1.1, 1, 1), (1, 1, 0.8), (1, 1, 1.2), (0.95, 1.05, 1), (1.05, 0.95, 1), (0.9, 1, 0.8),
           (1.1, 1, 1.2), (0.5, 1.5, 0.5), (1.37, 1, 1.37), (2, 0.5, 2), (0, 1, 1), (4, 4, 4), (1, 4, 0), (0.9, 0.9, 0.9)]
VIEW_SETS = ["training", CONTRAST_SET, [(0, 1, 1), (2, 2, 2), (1, 0, 1), (1, 1, 0)], [(0.9, 1.1, 1.2)], SIXTEEN]
GUARD = 48


def run_views(lib, x, factors, offset, out_offset=0, ws=None):
    """nbc_jitter_views on x uint8 [N,H,W,3] placed `offset` bytes into a guarded buffer; returns the views' bytes after
    checking every guard byte, the source included."""
    n, h, w = x.shape[:3]
    v = len(factors)
    raw = x.reshape(-1)
    src = torch.full((raw.size + 2 * GUARD + offset,), 0x5C, dtype=torch.uint8, device=DEV)
    src[GUARD + offset: GUARD + offset + raw.size] = torch.from_numpy(raw.copy())
    before = src.cpu().numpy()
    lead = GUARD + out_offset
    out = torch.full((v * raw.size + lead + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    if ws is None:
        ws = torch.full((v * n,), -1, dtype=torch.int64, device=DEV)      # stale words: the zeroing is the call's job
    f = np.ascontiguousarray(factors, dtype=np.float32)
    rc = lib.nbc_jitter_views(src.data_ptr() + GUARD + offset, n, h, w, f.ctypes.data, v, out.data_ptr() + lead, ws.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.NBC_OK, _lib.last_error()
    got = out.cpu().numpy()
    assert (got[:lead] == 0xAB).all() and (got[lead + v * raw.size:] == 0xAB).all(), "a guard byte of the views was written"
    assert np.array_equal(src.cpu().numpy(), before), "the source or its guard bytes were written"
    return got[lead: lead + v * raw.size].reshape((v * n, h, w, 3))


@pytest.mark.parametrize("shape", VIEW_SHAPES)
def test_views_kernel_is_the_restatement(built_lib, shape):
    n, h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    if h > 4:
        x[:, 1] = 0
        x[:, 3] = 255
    if n > 1:
        x[1] //= 3                                                  # another mean grey than image 0's
        assert jo.mean_grey(x[0]) != jo.mean_grey(x[1])
    for views in VIEW_SETS:
        factors = jo.factors_of(views)
        want = jo.stack(x, factors)
        for offset in (0, 1, 5):
            got = run_views(built_lib, x, factors, offset)
            assert np.array_equal(got, want), (shape, views if isinstance(views, str) else len(views), offset)
    # the views at another alignment than the source's
    factors = jo.factors_of(CONTRAST_SET)
    assert np.array_equal(run_views(built_lib, x, factors, 0, out_offset=3), jo.stack(x, factors))
    assert np.array_equal(run_views(built_lib, x, factors, 5, out_offset=9), jo.stack(x, factors))


def test_contrast_tie_and_a_reused_workspace(built_lib):
    # 8 x 22 pixels, half of grey 1 and half of grey 0: S = 88, mean 0.5, m = 1 (rounded down it would be 0)
    x = np.zeros((1, 8, 22, 3), dtype=np.uint8)
    x[0, ::2] = 1
    assert jo.mean_grey(x[0]) == 1 and int(jo.grey(x[0]).sum()) * 2 == 8 * 22
    views = [(1, 0, 1), (1, 0.5, 1), (2, 0, 1), (1, 1, 1)]           # brightness 2: greys 2 and 0, mean 1 exactly
    factors = jo.factors_of(views)
    want = jo.stack(x, factors)
    assert (want[0] == 1).all() and (want[2] == 1).all()
    ws = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    for _ in range(2):                                               # the second call finds the first call's sums in the workspace
        assert np.array_equal(run_views(built_lib, x, factors, 0, ws=ws), want)
    # two images with different sums, twice on one workspace, then a set without contrast on the same words
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, size=(2, 40, 72, 3), dtype=np.uint8)
    y[1] //= 2
    ws = torch.full((8,), 12345, dtype=torch.int64, device=DEV)
    fc = jo.factors_of(CONTRAST_SET)
    for _ in range(2):
        assert np.array_equal(run_views(built_lib, y, fc, 1, ws=ws), jo.stack(y, fc))
    ft = jo.factors_of("training")
    assert np.array_equal(run_views(built_lib, y, ft, 1, ws=torch.full((10,), 7, dtype=torch.int64, device=DEV)), jo.stack(y, ft))


def test_views_method(models):
    m = models["fp32"]
    x = u8_frames([3, 4], 40, 72)
    s = m.jitter_views(x.to(DEV), "training")
    assert s.shape == (10, 40, 72, 3) and s.dtype == torch.uint8
    assert np.array_equal(s.cpu().numpy(), jo.stack(x.numpy(), "training"))
    pil = Image.fromarray(x.numpy()[1], mode="RGB")                  # PIL itself, once on the device's bytes
    assert np.array_equal(s[2 * 1 + 1].cpu().numpy(), np.asarray(ImageEnhance.Brightness(pil).enhance(float(np.float32(0.9)))))
    assert np.array_equal(s[2 * 4 + 1].cpu().numpy(), np.asarray(ImageEnhance.Color(pil).enhance(float(np.float32(1.2)))))
    assert torch.equal(m.jitter_views(x.to(DEV), [(1, 1, 1)]), x.to(DEV))
    assert np.array_equal(m.jitter_views(x.to(DEV), CONTRAST_SET).cpu().numpy(), jo.stack(x.numpy(), CONTRAST_SET))   # the method's own workspace
    with pytest.raises(ValueError):
        m.jitter_views(x.to(DEV), "flips")
    with pytest.raises(ValueError):
        m.jitter_views(x.to(DEV).float(), "training")


# ---- 2. the mean -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (5, 9), (17, 9)])
def test_mean_is_the_restatement(built_lib, hw, n):
    h, w = hw
    rng = np.random.default_rng(100 * h + w + n)
    for v in (1, 5, 16):
        x = (rng.standard_normal((v, n, 3, h, w)) * 10.0 ** rng.integers(-3, 4, size=(v, n, 3, h, w))).astype(np.float32)
        flat = x.reshape(-1)
        specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, 3.4e38, -3.4e38]
        pos = rng.choice(flat.size, size=min(flat.size, 4 * len(specials)), replace=False)
        for k, q in enumerate(pos):
            flat[q] = np.float32(specials[k % len(specials)])
        x[:, :, :, h // 2, w // 2] = np.float32(-0.0)                # -0 in every view: the mean keeps the sign
        want = jo.mean(x)
        total = n * 3 * h * w
        out = torch.full((total + 8,), 7.0, dtype=torch.float32, device=DEV)
        rc = built_lib.nbc_views_mean(torch.from_numpy(x).to(DEV).data_ptr(), n, v, h, w, out.data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == _lib.NBC_OK, _lib.last_error()
        got = out.cpu().numpy()
        assert (got[total:] == 7.0).all()
        assert same_floats(got[:total].reshape(want.shape), want), (hw, n, v)
        assert np.signbit(got[:total].reshape(want.shape)[:, :, h // 2, w // 2]).all()
        if v == 1:
            assert same_floats(got[:total].reshape(want.shape), x[0])


# ---- 3. the stack is the single forwards; predict_labels_jitter is its parts -----------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_stack_is_the_single_forwards_and_the_call_is_its_parts(models, mode):
    m = models[mode]
    n, h, w = 2, 129, 191
    x = u8_frames([10, 11], h, w)
    xd = x.to(DEV)
    views = jo.stack(x.numpy(), "training").reshape(5, n, h, w, 3)
    singles = torch.stack([m.lowres_logits(torch.from_numpy(views[j]).to(DEV)) for j in range(5)])   # each view run alone
    before = m.predict_labels(xd, small_zones=True, return_lowres=True)
    for kw in (dict(), dict(small_zones=True), dict(small_zones=True, exclude_nodes=True, min_pixels=40)):
        lg = torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV)
        labels, counts, mean, vcounts, support, stats, lowres_views = m.predict_labels_jitter(
            xd, "training", labels_dtype=torch.uint8, logits_full=lg, return_lowres=True, return_views=True, **kw)
        assert lowres_views.shape == singles.shape and torch.equal(lowres_views, singles), kw
        assert same_floats(mean.cpu().numpy(), jo.mean(singles.cpu().numpy()))
        assert torch.equal(mean, m.views_mean(lowres_views, n)) and torch.equal(mean, m.views_mean(lowres_views.view(5 * n, 3, *mean.shape[-2:]), n))
        zones, remap, minpx = kw.get("small_zones", False), kw.get("exclude_nodes", False), kw.get("min_pixels", 150)

        def tail(low):
            lab, cnt, full = m.upsample_argmax(low, (h, w), exclude_nodes=remap and not zones, labels_dtype=torch.uint8, return_logits=True)
            if zones:
                lab, cnt = m.remove_small_zones(lab, exclude_nodes=remap, min_pixels=minpx)
            return lab, cnt, full

        lab_w, cnt_w, full_w = tail(mean)
        assert torch.equal(labels, lab_w) and torch.equal(counts, cnt_w) and torch.equal(lg, full_w), kw
        assert (counts.sum(1) == h * w).all()
        view_labels = np.stack([tail(lowres_views[j])[0].cpu().numpy() for j in range(5)])
        c_w, s_w, st_w = jo.view_figures(view_labels)
        assert np.array_equal(vcounts.cpu().numpy(), c_w) and np.array_equal(support.cpu().numpy(), s_w), kw
        assert np.array_equal(stats.cpu().numpy(), st_w), kw
        assert vcounts.shape == (5, n, 3) and vcounts.dtype == torch.int64 and support.dtype == torch.uint8
    assert not torch.equal(lowres_views[0], lowres_views[1])        # the network is not colour-invariant: the views differ
    # without the extras: the pair of predict_labels, int64 labels by default
    pair = m.predict_labels_jitter(xd, "training", small_zones=True)
    assert len(pair) == 2 and pair[0].dtype == torch.int64
    # the call left no forward behind for the draws; a plain predict_labels afterwards has the same bits
    with pytest.raises(RuntimeError, match="none has run"):
        m.dropout_draws(2, [1, 2])
    after = m.predict_labels(xd, small_zones=True, return_lowres=True)
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert not m.nonfinite_seen()


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_the_identity_set_is_predict_labels(models, mode):
    m = models[mode]
    n, h, w = 2, 129, 191
    xd = u8_frames([12, 13], h, w).to(DEV)
    lg0, lg1 = (torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV) for _ in range(2))
    a = m.predict_labels(xd, logits_full=lg0, small_zones=True, return_lowres=True)
    b = m.predict_labels_jitter(xd, [(1, 1, 1)], logits_full=lg1, small_zones=True, return_lowres=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(lg0, lg1)
    a = m.predict_labels(xd, exclude_nodes=True)
    b = m.predict_labels_jitter(xd, [(1, 1, 1)], exclude_nodes=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. against the CPU oracle ---------------------------------------------------------------------------------------------
ORACLE_SHAPE, ORACLE_FIRST = (2, 129, 191), 30
_oracle_cache = {}


def pil_view(img, triple):
    out = Image.fromarray(img, mode="RGB")
    for enhancer, f in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), triple):
        out = enhancer(out).enhance(float(np.float32(f)))
    return np.asarray(out)


def oracle_views(oracle_model):
    """The oracle on each PIL-made view, normalised as the uint8 ingest does: (frames, views' lowres [5,N,3,h,w], their mean,
    the mean's full-resolution logits, its labels).  Computed once."""
    if not _oracle_cache:
        import torch.nn.functional as F
        from oracle.fcn_resnet50_oracle import predict_labels
        n, h, w = ORACLE_SHAPE
        x = u8_frames(range(ORACLE_FIRST, ORACLE_FIRST + n), h, w)
        lows = []
        for triple in jo.TRAINING:
            xin = torch.from_numpy(np.stack([synth.normalize_frame(pil_view(img, triple)) for img in x.numpy()]))
            lows.append(predict_labels(oracle_model, xin)[3])
        lows = torch.stack(lows)
        mean = torch.from_numpy(jo.mean(lows.numpy()))
        logits = F.interpolate(mean, size=(h, w), mode="bicubic", align_corners=False)
        _oracle_cache["v"] = (x, lows, mean, logits, torch.argmax(logits, dim=1))
    return _oracle_cache["v"]


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16"])
def test_against_the_cpu_oracle(oracle_model, models, mode):
    n, h, w = ORACLE_SHAPE
    x, lows_ref, mean_ref, logits_ref, labels_ref = oracle_views(oracle_model)
    m = models[mode]
    lg = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    labels, counts, mean, vcounts, support, stats, lows = m.predict_labels_jitter(x.to(DEV), "training", logits_full=lg,
                                                                                  return_lowres=True, return_views=True)
    scale = float(logits_ref.abs().max())
    rtol = LOGIT_RTOL_BF16 if mode == "bf16" else LOGIT_RTOL_FP32
    errs = [float((lows[j].cpu() - lows_ref[j]).abs().max()) for j in range(5)]
    err_m = float((mean.cpu() - mean_ref).abs().max())
    err = float((lg.cpu() - logits_ref).abs().max())
    print(mode, ORACLE_SHAPE, "view errs", errs, "mean", err_m, "full", err, "scale", scale)
    for e in errs + [err_m, err]:
        assert e <= rtol * scale, (e, scale)
    if mode == "bf16":
        return                                                     # logits only
    # the rule of tests/test_gpu_parity.py::check_labels: identical outside a band of twice the measured error
    top2 = torch.topk(logits_ref, 2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    mism = labels.cpu() != labels_ref
    n_mism = int(mism.sum())
    print(mode, "label mismatches", n_mism, "of", mism.numel())
    if n_mism:
        assert float(margin[mism].max()) <= 2.0 * max(err, 1e-7 * scale)
    assert n_mism <= max(2, MAX_TIE_FLIPS_FRAC * mism.numel()), n_mism


# ---- 5. the other networks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["deeplabv3_resnet50", "fcn_efficientnet_b0"])
def test_other_networks(built_lib, arch):
    from neuralbarkcalculator_amd.model import DeepLabV3ResNet50
    sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
    m = (DeepLabV3ResNet50("fp32") if arch == "deeplabv3_resnet50" else fcn_efficientnet(0)).load_state_dict(sd).to(DEV)
    n, h, w = 1, 160, 160
    x = u8_frames([80], h, w)
    lg = torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV)
    labels, counts, mean, vcounts, support, stats, lows = m.predict_labels_jitter(x.to(DEV), "training", labels_dtype=torch.uint8,
                                                                                  logits_full=lg, small_zones=True,
                                                                                  return_lowres=True, return_views=True)
    views = jo.stack(x.numpy(), "training")
    want = torch.stack([m.lowres_logits(torch.from_numpy(np.ascontiguousarray(views[j][None])).to(DEV)) for j in range(5)])
    assert torch.equal(lows, want)
    assert same_floats(mean.cpu().numpy(), jo.mean(want.cpu().numpy()))
    lab_w, _, full_w = m.upsample_argmax(mean, (h, w), labels_dtype=torch.uint8, return_logits=True)
    lab_w, cnt_w = m.remove_small_zones(lab_w)
    assert torch.equal(labels, lab_w) and torch.equal(counts, cnt_w) and torch.equal(lg, full_w)
    view_labels = []
    for j in range(5):
        lab, _ = m.upsample_argmax(lows[j], (h, w), labels_dtype=torch.uint8)
        view_labels.append(m.remove_small_zones(lab)[0].cpu().numpy())
    c_w, s_w, st_w = jo.view_figures(np.stack(view_labels))
    assert np.array_equal(vcounts.cpu().numpy(), c_w) and np.array_equal(support.cpu().numpy(), s_w)
    assert np.array_equal(stats.cpu().numpy(), st_w)


# ---- 6. folders ------------------------------------------------------------------------------------------------------------
# the LAYOUT of tests/test_gpu_tta.py, restated
LAYOUT = [("sapin", "s00.bmp", 40, 128, 192), ("sapin", "s01.png", 41, 128, 192), ("sapin", "s02.bmp", 42, 96, 192),
          ("epinette_gelee", "e00.png", 43, 128, 192), ("epinette_gelee", "e01.png", 44, 160, 160),
          ("epinette_non_gelee", "n00.png", 45, 96, 192)]


def _make_folder(root, sd_np):
    for wood, name, idx, h, w in LAYOUT:
        d = os.path.join(root, "samples", wood)
        os.makedirs(d, exist_ok=True)
        Image.fromarray(synth.make_frame(idx, h, w), mode="RGB").save(os.path.join(d, name))
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    return ckpt


def _result_bytes(root):
    out = {}
    for base, _, names in sorted(os.walk(os.path.join(root, "results"))):
        for n in sorted(names):
            path = os.path.join(base, n)
            out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out


def test_predict_folder(tmp_path, sd_np, built_lib):
    roots = {}
    for tag, kw in (("before", {}), ("jitter", dict(jitter="training", jitter_votes=True)), ("after", {})):
        roots[tag] = str(tmp_path / tag)
        ckpt = _make_folder(roots[tag], sd_np)
        st = drv.predict_folder(roots[tag], ckpt, precision="fp32", device_index=0, **kw)
        assert st["images_total"] == len(LAYOUT) and st["batch"] == (1 if kw else 2)
    files = {tag: _result_bytes(root) for tag, root in roots.items()}
    assert len(files["before"]) == 1 + len(LAYOUT)                 # final_stats.csv and the label PNGs
    assert files["after"] == files["before"]                        # without the flag: the tree made before the run with it
    new = {"results/jitter_stats.csv", "results/jitter_summary.json"}
    support = {"results/jitter_support/%s/%s" % (wood, name.replace("bmp", "png")) for wood, name, _, _, _ in LAYOUT}
    assert set(files["jitter"]) == set(files["before"]) | new | support
    assert files["jitter"]["results/final_stats.csv"] != files["before"]["results/final_stats.csv"]   # the mean's labels differ

    # jitter_stats.csv, final_stats.csv and the PNGs: model-level calls, one image at a time
    root = roots["jitter"]
    model = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    images, stats_rows = [], []
    for _, name, wood in drv.list_images(os.path.join(root, "processed")):
        frame = np.asarray(Image.open(os.path.join(root, "processed", "samples", wood, name)).convert("RGB"))
        x = torch.from_numpy(np.array(frame[None])).to(DEV)
        labels, counts, vcounts, sup, stats, _ = model.predict_labels_jitter(x, "training", labels_dtype=torch.uint8, small_zones=True,
                                                                             return_views=True)
        h, w = frame.shape[:2]
        images.append((name, wood, h, w, counts.cpu().numpy()[0], vcounts.cpu().numpy()[:, 0], stats.cpu().numpy()[0]))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "outputs", wood, name))), drv.label_png(labels.cpu().numpy()[0]))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "jitter_support", wood, name))), sup.cpu().numpy()[0])
        c = counts.cpu().numpy()[0]
        stats_rows.append(drv.stats_row(name, wood, h, w, int(c[1]), int(c[2])))
    table, summary = folder_run.jitter_report(images, resolve_jitter_views("training"))
    got = list(csv.reader(open(os.path.join(root, "results", "jitter_stats.csv")), delimiter="\t"))
    assert got == table and len(got) == 1 + len(LAYOUT)
    final = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert final[1:] == [[str(v) for v in r] for r in stats_rows]
    doc = json.load(open(os.path.join(root, "results", "jitter_summary.json")))
    assert doc["views"] == jo.TRAINING_NAMES and doc["precision"] == "fp32" and doc["bn_stats"] == "running"
    assert doc["means"] == json.loads(json.dumps(summary["means"])) and doc["images"] == len(LAYOUT)


def test_evaluate_folder(tmp_path, sd_np, built_lib):
    """evaluate --jitter training: every row is metrics.py on the model-level labels of the mean; the identity row of the
    robustness table is the plain run's pooled confusion; the run without the flag is what it was."""
    root = str(tmp_path / "labelled")
    rng = np.random.default_rng(7)
    truth = {}
    for wood, fname, idx, h, w in LAYOUT:
        name = fname.replace("bmp", "png")
        os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
        os.makedirs(os.path.join(root, "duals", wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, fname))
        grey = np.repeat(np.repeat(rng.choice(np.array([0, 127, 255], dtype=np.uint8), size=(h // 16, w // 16)), 16, axis=0), 16, axis=1)
        Image.fromarray(np.ascontiguousarray(grey), mode="L").save(os.path.join(root, "duals", wood, name))
        truth[(wood, name)] = (img, grey)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    plain = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0)
    before = _result_bytes(root)
    assert "jitter" not in json.load(open(os.path.join(root, ev.SUMMARY_JSON))) and set(before) == {ev.STATS_CSV, ev.SUMMARY_JSON}
    clean_total = np.sum([np.asarray(r[13:22]).reshape(3, 3) for r in plain["rows"]], axis=0)

    st = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, jitter="training")
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["jitter"]["views"] == jo.TRAINING_NAMES and st["summary"]["jitter"]["views"] == jo.TRAINING_NAMES
    assert summary["images_evaluated"] == len(LAYOUT) and st["batch"] == 1
    assert set(_result_bytes(root)) == set(before) | {os.path.join("results", ev.JITTER_EVALUATION_CSV)}
    rows = list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))
    assert rows[0] == metrics.EVAL_CSV_HEADER and len(rows) == 1 + len(LAYOUT)       # evaluation_stats.csv keeps its columns
    m = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    pooled = np.zeros((5, 3, 3), dtype=np.int64)
    for r in rows[1:]:
        img, grey = truth[(r[1], r[0])]
        h, w = img.shape[:2]
        x = torch.from_numpy(img[None]).to(DEV)
        lab, _, _, _, _, lows = m.predict_labels_jitter(x, "training", labels_dtype=torch.uint8, return_views=True)
        raw = lab.cpu().numpy()[0].copy()
        clean = m.remove_small_zones(lab)[0].cpu().numpy()[0]
        t = metrics.target_classes(grey)
        assert r == metrics.eval_row(r[0], r[1], metrics.confusion_numpy(raw, t), metrics.confusion_numpy(clean, t))
        for j in range(5):
            vlab, _ = m.upsample_argmax(lows[j], (h, w), labels_dtype=torch.uint8)
            pooled[j] += metrics.confusion_numpy(m.remove_small_zones(vlab)[0].cpu().numpy()[0], t)
    table, doc = ev.jitter_evaluation(jo.TRAINING_NAMES, pooled)
    got = list(csv.reader(open(os.path.join(root, "results", ev.JITTER_EVALUATION_CSV)), delimiter="\t"))
    assert got == table and [g[0] for g in got[1:]] == jo.TRAINING_NAMES
    assert summary["jitter"]["evaluation"] == json.loads(json.dumps(doc))
    # the identity row: what the pooled confusion of the plain run gives
    assert np.array_equal(pooled[0], clean_total)
    ious, f1s = metrics.iou(clean_total), metrics.f1(clean_total)
    assert got[1][1:9] == ["{:.3f}".format(v) for v in list(ious) + [ious.mean()] + list(f1s) + [f1s.mean()]]
    assert got[1][11:] == ["0.000"] * 8 + ["0.00000"] * 2 and any(g[11:] != got[1][11:] for g in got[2:])   # some view moves the answer

    os.remove(os.path.join(root, "results", ev.JITTER_EVALUATION_CSV))
    ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0)
    assert _result_bytes(root) == before                            # without the flag: the tree made before the run with it
