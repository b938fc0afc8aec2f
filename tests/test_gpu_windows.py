"""The crop windows on the GPU (nbc_window_views, nbc_window_merge, FCNResNet50.predict_labels_windows, predict / evaluate
--windows).  The kernels are compared bit for bit with the numpy restatement of tests/helpers/window_oracle.py; the stacked
forward with single forwards of windows cut with numpy, bit for bit; the logits with the CPU oracle run on each window, under the
tolerances of tests/test_gpu_parity.py."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, folder_run, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import DeepLabV3ResNet50, FCNResNet50, fcn_efficientnet, window_grid

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import window_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the constants of tests/test_gpu_parity.py (LOGIT_RTOL_FP32, LOGIT_RTOL_BF16, MAX_TIE_FLIPS_FRAC), restated
LOGIT_RTOL_FP32 = 5e-6
LOGIT_RTOL_BF16 = 4e-2
MAX_TIE_FLIPS_FRAC = 4e-6


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


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
# (1, 9, 4101, 2048, 1024): a row longer than the mover's segment of 4096 units -- four windows across, a reflected row band (rows
# 9..15 of the padded 16) and three reflected columns that fall in the short last segment
CASES = [(1, 8, 8, 32, 8), (2, 13, 21, 32, 16), (1, 40, 75, 32, 16), (3, 129, 65, 64, 32), (1, 64, 64, 64, 64), (1, 72, 200, 64, 24),
         (1, 9, 4101, 2048, 1024)]


@pytest.mark.parametrize("case", CASES)
def test_views_kernel_is_the_numpy_windows(built_lib, case):
    n, h, w, S, T = case
    rng = np.random.default_rng(h * 1000 + w)
    u8 = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f32 = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    f32.reshape(-1)[(h * w) // 2] = np.float32("nan")
    f32[:, :, -2, -2] = np.float32("nan")                          # a pixel the corner's reflection repeats
    for x, dtype in ((u8, _lib.IN_U8_NHWC), (f32, _lib.IN_F32_NCHW)):
        want = np.frombuffer(wo.stack(x, S, T).tobytes(), dtype=np.uint8)
        for offset in ((0, 1) if x.dtype == np.uint8 else (0,)):   # a uint8 source one byte into its buffer
            raw = np.frombuffer(x.tobytes(), dtype=np.uint8)
            src = torch.zeros(raw.size + 64, dtype=torch.uint8, device=DEV)
            src[offset: offset + raw.size] = torch.from_numpy(raw.copy())
            guard = 48 + 3 * offset                                # the uint8 destination off its 16-byte alignment as well
            out = torch.full((want.size + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
            rc = built_lib.nbc_window_views(src.data_ptr() + offset, dtype, n, h, w, S, T, out.data_ptr() + guard, stream())
            torch.cuda.synchronize()
            assert rc == _lib.NBC_OK, _lib.last_error()
            got = out.cpu().numpy()
            assert (got[:guard] == 0xAB).all() and (got[guard + want.size:] == 0xAB).all(), (case, offset)
            assert np.array_equal(got[guard: guard + want.size], want), (case, str(x.dtype), offset)


def test_views_method_and_numpy_pad(models):
    m = models["fp32"]
    x = frames([3, 4], 13, 21)
    s = m.window_views(x.to(DEV), 32, 16)
    assert s.shape == (2, 3, 16, 24)
    assert same_floats(s.cpu().numpy(), np.pad(x.numpy(), ((0, 0), (0, 0), (0, 3), (0, 3)), mode="reflect"))
    u = torch.from_numpy(np.stack([synth.make_frame(5, 40, 75)]))
    s = m.window_views(u.to(DEV), 32, 16).cpu().numpy()
    ey, ex, ny, nx, oys, oxs = m.window_grid(40, 75, 32, 16)
    assert (ey, ex, ny, nx, oys, oxs) == (32, 32, 2, 4, [0, 8], [0, 16, 32, 48]) and s.shape == (8, 32, 32, 3)
    pad = np.pad(u.numpy(), ((0, 0), (0, 0), (0, 5), (0, 0)), mode="reflect")
    for r, oy in enumerate(oys):
        for c, ox in enumerate(oxs):
            assert np.array_equal(s[r * nx + c], pad[0, oy: oy + 32, ox: ox + 32])
    with pytest.raises(ValueError):
        m.window_views(u.to(DEV), 36, 16)
    with pytest.raises(ValueError):
        m.window_views(u.to(DEV), 64, 4)


# ---- 2. the merge ----------------------------------------------------------------------------------------------------------
def crafted_logits(rng, shape):
    """Random logits over seven decades with the specials of tests/test_gpu_tta.py::test_merge_is_the_restatement planted."""
    x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(np.float32)
    flat = x.reshape(-1)
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, 3.4e38, -3.4e38]
    pos = rng.choice(flat.size, size=min(flat.size, 4 * len(specials)), replace=False)
    for k, q in enumerate(pos):
        flat[q] = np.float32(specials[k % len(specials)])
    return x


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_merge_is_the_restatement(built_lib, case, n):
    _, h, w, S, T = case
    ey, ex, ny, nx, oys, oxs = window_grid(h, w, S, T)
    k = ny * nx
    lh, lw = (h + 7) // 8, (w + 7) // 8
    rng = np.random.default_rng(100 * h + w + n)
    x = crafted_logits(rng, (k * n, 3, ey // 8, ex // 8))
    x[:, :, 0, 0] = np.float32(-0.0)                               # -0 in a cell one window covers, and in overlaps
    src = torch.from_numpy(x).to(DEV)
    total = n * 3 * lh * lw
    for blend in (wo.TENT, wo.UNIFORM):
        want, cover = wo.merge(x, n, h, w, S, T, blend, return_cover=True)
        merged = torch.full((total + 8,), 7.0, dtype=torch.float32, device=DEV)
        rc = built_lib.nbc_window_merge(src.data_ptr(), n, h, w, S, T, blend, merged.data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == _lib.NBC_OK, _lib.last_error()
        mg = merged.cpu().numpy()
        assert (mg[total:] == 7.0).all()
        got = mg[:total].reshape(want.shape)
        assert same_floats(got, want), (case, n, blend)
        # cells one window covers hold that window's bits
        v5 = x.reshape(k, n, 3, ey // 8, ex // 8)
        single = cover == 1
        assert single[0, 0] and bits(got)[0, 0, 0, 0] == 0x80000000
        for r, oy in enumerate(oys):
            for c, ox in enumerate(oxs):
                ys, xs = slice(oy // 8, oy // 8 + ey // 8), slice(ox // 8, ox // 8 + ex // 8)
                sel = np.broadcast_to(single[ys, xs], (n, 3, ey // 8, ex // 8))
                assert same_floats(got[:, :, ys, xs][sel], v5[r * nx + c][sel]), (case, r, c)
        if k == 1:
            assert same_floats(got, x)
    if k > 1:
        assert int(cover.max()) > 1


# ---- 3. the stack is the single forwards -----------------------------------------------------------------------------------
def window_cuts(x, S, T):
    """The windows of f32 [N,3,H,W] cut with numpy.pad and slicing: a list over k of [N,3,E_y,E_x] tensors."""
    n, _, h, w = x.shape
    ey, ex, ny, nx, oys, oxs = window_grid(h, w, S, T)
    pad = np.pad(x.numpy(), ((0, 0), (0, 0), (0, -h % 8), (0, -w % 8)), mode="reflect")
    return [torch.from_numpy(np.ascontiguousarray(pad[:, :, oy: oy + ey, ox: ox + ex])) for oy in oys for ox in oxs]


@pytest.mark.parametrize("mode,arch", [("fp32", "fcn_resnet50"), ("f16x2", "fcn_resnet50"), ("bf16", "fcn_resnet50"),
                                       ("fp32", "deeplabv3_resnet50")])
def test_stack_is_the_single_forwards(models, mode, arch):
    if arch == "fcn_resnet50":
        m = models[mode]
    else:
        m = DeepLabV3ResNet50("fp32").load_state_dict(synth.make_state_dict("trained_like", seed=7, arch=arch)).to(DEV)
    n, h, w, S, T = 2, 129, 191, 64, 32
    x = frames(range(10, 10 + n), h, w)
    cuts = window_cuts(x, S, T)
    assert len(cuts) == 20
    stack = m.window_views(x.to(DEV), S, T)
    assert torch.equal(stack.cpu(), torch.cat(cuts))
    low = torch.empty((20 * n, 3, 8, 8), dtype=torch.float32, device=DEV)
    m._forward(stack, 20 * n, 64, 64, lowres=low)
    want = torch.cat([m.lowres_logits(c.to(DEV)) for c in cuts])
    assert torch.equal(low, want)
    merged = m.predict_labels_windows(x.to(DEV), S, T, return_lowres=True)[2]
    assert same_floats(merged.cpu().numpy(), wo.merge(want.cpu().numpy(), n, h, w, S, T))
    assert not torch.equal(want[0], want[n])                       # neighbouring windows give different logits


# ---- 4. against the CPU oracle ---------------------------------------------------------------------------------------------
ORACLE_CASES = [((2, 129, 191), 64, 32, 30), ((1, 200, 121), 96, 48, 50)]
_oracle_cache = {}


def oracle_windows(oracle_model, case):
    """The oracle on each window, merged with the numpy restatement: (x, merged [N,3,h,w], merged logits, merged labels,
    the plain forward's labels)."""
    if case not in _oracle_cache:
        import torch.nn.functional as F
        from oracle.fcn_resnet50_oracle import predict_labels
        (n, h, w), S, T, first = case
        x = frames(range(first, first + n), h, w)
        low = torch.cat([predict_labels(oracle_model, c)[3] for c in window_cuts(x, S, T)])
        merged = torch.from_numpy(wo.merge(low.numpy(), n, h, w, S, T))
        logits = F.interpolate(merged, size=(h, w), mode="bicubic", align_corners=False)
        plain = F.interpolate(predict_labels(oracle_model, x)[3], size=(h, w), mode="bicubic", align_corners=False)
        _oracle_cache[case] = (x, merged, logits, torch.argmax(logits, dim=1), torch.argmax(plain, dim=1))
    return _oracle_cache[case]


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_against_the_cpu_oracle(oracle_model, models, case, mode):
    (n, h, w), S, T, _ = case
    x, merged_ref, logits_ref, labels_ref, plain_ref = oracle_windows(oracle_model, case)
    m = models[mode]
    lg = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    labels, counts, merged = m.predict_labels_windows(x.to(DEV), S, T, logits_full=lg, return_lowres=True)
    scale = float(logits_ref.abs().max())
    rtol = LOGIT_RTOL_BF16 if mode == "bf16" else LOGIT_RTOL_FP32
    err_m = float((merged.cpu() - merged_ref).abs().max())
    err = float((lg.cpu() - logits_ref).abs().max())
    print(mode, case, "merged", err_m, "full", err, "scale", scale)
    for e in (err_m, err):
        assert e <= rtol * scale, (e, scale)
    plain_labels, _ = m.predict_labels(x.to(DEV))
    changed = int((labels != plain_labels).sum())
    print(mode, case, "pixels the windows change", changed, "of", labels.numel())
    assert changed >= 1                                            # the feature does something
    assert int((labels_ref != plain_ref).sum()) >= 1
    if mode == "bf16":
        return                                                     # logits only
    # the rule of tests/test_gpu_parity.py::check_labels: identical outside a band of twice the measured error
    top2 = torch.topk(logits_ref, 2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    mism = labels.cpu() != labels_ref
    n_mism = int(mism.sum())
    if n_mism:
        assert float(margin[mism].max()) <= 2.0 * max(err, 1e-7 * scale)
    assert n_mism <= max(2, MAX_TIE_FLIPS_FRAC * mism.numel()), n_mism


# ---- 5. predict_labels_windows is its parts --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_predict_labels_windows_is_its_parts(models, mode):
    m = models[mode]
    n, h, w, S, T = 2, 129, 191, 64, 32
    x = frames([70, 71], h, w).to(DEV)
    before = m.predict_labels(x, small_zones=True, return_lowres=True)
    for blend in ("tent", "uniform"):
        stack = m.window_views(x, S, T)
        low = torch.empty((20 * n, 3, 8, 8), dtype=torch.float32, device=DEV)
        m._forward(stack, 20 * n, 64, 64, lowres=low)
        merged_w = m.window_merge(low, n, h, w, S, T, blend)
        assert merged_w.shape == (n, 3, 17, 24)
        for kw in (dict(), dict(small_zones=True), dict(small_zones=True, exclude_nodes=True), dict(exclude_nodes=True),
                   dict(small_zones=True, min_pixels=40)):
            lg = torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV)
            labels, counts, merged = m.predict_labels_windows(x, S, T, blend, labels_dtype=torch.uint8, logits_full=lg,
                                                              return_lowres=True, **kw)
            zones, remap, minpx = kw.get("small_zones", False), kw.get("exclude_nodes", False), kw.get("min_pixels", 150)
            assert torch.equal(merged, merged_w)
            lab_w, cnt_w, full_w = m.upsample_argmax(merged, (h, w), exclude_nodes=remap and not zones, labels_dtype=torch.uint8,
                                                     return_logits=True)
            if zones:
                lab_w, cnt_w = m.remove_small_zones(lab_w, exclude_nodes=remap, min_pixels=minpx)
            assert torch.equal(labels, lab_w) and torch.equal(counts, cnt_w) and torch.equal(lg, full_w), kw
            assert int(counts.sum()) == n * h * w and (counts.sum(1) == h * w).all()
            if not zones:
                want = torch.argmax(lg, dim=1)
                if remap:
                    want[want == 2] = 1
                assert torch.equal(labels.long(), want)
    assert not torch.equal(m.predict_labels_windows(x, S, T, "tent", return_lowres=True)[2],
                           m.predict_labels_windows(x, S, T, "uniform", return_lowres=True)[2])
    # without the extras: the pair of predict_labels, int64 labels by default
    pair = m.predict_labels_windows(x, S, T, small_zones=True)
    assert len(pair) == 2 and pair[0].dtype == torch.int64
    # a frame that is one window is predict_labels itself
    x8 = frames([75, 76], 128, 192).to(DEV)
    for S1 in (192, 512):
        one = m.predict_labels_windows(x8, S1, 96, small_zones=True, return_lowres=True)
        assert all(torch.equal(a, b) for a, b in zip(one, m.predict_labels(x8, small_zones=True, return_lowres=True)))
    lg0, lg1 = (torch.zeros((2, 3, 128, 192), dtype=torch.float32, device=DEV) for _ in range(2))
    a = m.predict_labels(x8, logits_full=lg0, exclude_nodes=True)
    b = m.predict_labels_windows(x8, 256, 128, logits_full=lg1, exclude_nodes=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(lg0, lg1)
    # one image alone equals itself at each position of a batch of 3
    xa = frames([72], h, w).to(DEV)
    fill = frames([73, 74], h, w).to(DEV)
    alone = m.predict_labels_windows(xa, S, T, small_zones=True, return_lowres=True)
    for pos in range(3):
        xs = list(fill)
        xs.insert(pos, xa[0])
        got = m.predict_labels_windows(torch.stack(xs), S, T, small_zones=True, return_lowres=True)
        for k in range(3):
            assert torch.equal(got[k][pos], alone[k][0]), (pos, k)
    # a plain predict_labels afterwards has the same bits, and the call left no forward behind for the draws
    with pytest.raises(RuntimeError, match="none has run"):
        m.dropout_draws(2, [1, 2])
    after = m.predict_labels(x, small_zones=True, return_lowres=True)
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert not m.nonfinite_seen()
    with pytest.raises(ValueError, match="blend"):
        m.predict_labels_windows(x, S, T, "gauss")
    with pytest.raises(ValueError, match="nbc_window_grid"):
        m.predict_labels_windows(x, 60, T)


def test_refusals(sd_np, built_lib):
    e = fcn_efficientnet(0).load_state_dict(synth.make_state_dict("trained_like", seed=7, arch="fcn_efficientnet_b0")).to(DEV)
    x = frames([80], 160, 160).to(DEV)
    with pytest.raises(ValueError, match="output stride is 32"):
        e.predict_labels_windows(x, 64, 32)
    for mode, bn in (("fp32", "image"), ("f16x2", "image_f16x2")):
        m = FCNResNet50(mode).load_state_dict(sd_np).to(DEV).set_bn_statistics(bn)
        with pytest.raises(ValueError, match="per-frame statistics"):
            m.predict_labels_windows(x, 64, 32)
        m.set_bn_statistics("running")
        assert len(m.predict_labels_windows(x, 64, 32)) == 2


# ---- 6. folders ------------------------------------------------------------------------------------------------------------
# the LAYOUT of tests/test_gpu_tta.py, restated
LAYOUT = [("sapin", "s00.bmp", 40, 128, 192), ("sapin", "s01.png", 41, 128, 192), ("sapin", "s02.bmp", 42, 96, 192),
          ("epinette_gelee", "e00.png", 43, 128, 192), ("epinette_gelee", "e01.png", 44, 160, 160),
          ("epinette_non_gelee", "n00.png", 45, 96, 192)]
S, T = 64, 32


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
    for tag, kw in (("plain", {}), ("windows", dict(windows=S, windows_stride=T)),
                    ("b1s4", dict(windows=S, windows_stride=T, batch=1, streams=4)),
                    ("compare", dict(windows=S, windows_stride=T, windows_compare=True))):
        roots[tag] = str(tmp_path / tag)
        ckpt = _make_folder(roots[tag], sd_np)
        st = drv.predict_folder(roots[tag], ckpt, precision="fp32", device_index=0, **kw)
        assert st["images_total"] == len(LAYOUT)
    files = {tag: _result_bytes(root) for tag, root in roots.items()}
    assert len(files["plain"]) == 1 + len(LAYOUT)                  # final_stats.csv and the label PNGs: untouched by the feature
    new = {"results/windows_stats.csv", "results/windows_summary.json"}
    assert set(files["windows"]) == set(files["plain"]) | new
    assert files["b1s4"] == files["windows"]
    assert set(files["compare"]) == set(files["windows"])
    assert {k: v for k, v in files["compare"].items() if k not in new} == {k: v for k, v in files["windows"].items() if k not in new}
    assert files["windows"]["results/final_stats.csv"] != files["plain"]["results/final_stats.csv"]  # the merged labels differ

    # windows_stats.csv, final_stats.csv and the PNGs: model-level calls, one image at a time
    root = roots["compare"]
    model = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    images, stats_rows = [], []
    for _, name, wood in drv.list_images(os.path.join(root, "processed")):
        frame = np.asarray(Image.open(os.path.join(root, "processed", "samples", wood, name)).convert("RGB"))
        x = torch.from_numpy(np.ascontiguousarray(frame[None])).to(DEV)
        labels, counts = model.predict_labels_windows(x, S, T, labels_dtype=torch.uint8, small_zones=True)
        plabels, pcounts = model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
        h, w = frame.shape[:2]
        conf = model.confusion(labels, plabels * 127).cpu().numpy()[0]
        changed = int(conf.sum() - np.trace(conf))
        assert changed == int((labels != plabels).sum()) and changed > 0
        images.append((name, wood, h, w, window_grid(h, w, S, T)[:4], counts.cpu().numpy()[0], pcounts.cpu().numpy()[0], changed))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "outputs", wood, name))), drv.label_png(labels.cpu().numpy()[0]))
        assert open(os.path.join(root, "results", "outputs", wood, name), "rb").read() == \
            files["windows"]["results/outputs/%s/%s" % (wood, name)]
        c = counts.cpu().numpy()[0]
        stats_rows.append(drv.stats_row(name, wood, h, w, int(c[1]), int(c[2])))
    table, summary = folder_run.windows_report(images, S, T, "tent", compare=True)
    got = list(csv.reader(open(os.path.join(root, "results", "windows_stats.csv")), delimiter="\t"))
    assert got == table and len(got) == 1 + len(LAYOUT) and got[0][-1] == "Changed pixels %"
    short = list(csv.reader(open(os.path.join(roots["windows"], "results", "windows_stats.csv")), delimiter="\t"))
    assert short == [r[:8] for r in table]
    final = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert final[1:] == [[str(v) for v in r] for r in stats_rows]
    doc = json.load(open(os.path.join(root, "results", "windows_summary.json")))
    assert (doc["window"], doc["stride"], doc["blend"], doc["precision"], doc["images"]) == (S, T, "tent", "fp32", len(LAYOUT))
    assert doc["means"] == json.loads(json.dumps(summary["means"])) and "abs_diff_bark" in doc["means"]
    assert doc["grids"] == {"64x64 2x5": 2, "64x64 3x5": 3, "64x64 4x4": 1}

    # two gloo ranks sharing the GPU, as tests/test_gpu_tta.py sets them up
    root2 = str(tmp_path / "w2")
    ckpt2 = _make_folder(root2, sd_np)
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import predict\n"
            "dist.init_process_group('gloo')\n"
            "st = predict.predict_folder(%r, %r, precision='fp32', device_index=0, windows=%d, windows_stride=%d)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, root2, ckpt2, S, T, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29653", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _result_bytes(root2) == files["windows"]


def test_evaluate_folder(tmp_path, sd_np, built_lib):
    """evaluate --windows: every row is metrics.py on the model-level merged labels; windows_evaluation.csv is jitter_evaluation
    on the two pooled confusions; the run without the flag reproduces the plain bytes."""
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
    ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0)
    plain_csv = open(os.path.join(root, ev.STATS_CSV), "rb").read()
    assert "windows" not in json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    st = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, windows=S, windows_stride=T, loss=True)
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["windows"] == {"window": S, "stride": T, "blend": "tent"} and st["summary"]["windows"] == summary["windows"]
    assert summary["images_evaluated"] == len(LAYOUT) and st["batch"] == 1
    assert not os.path.exists(os.path.join(root, "results", ev.WINDOWS_EVALUATION_CSV))
    rows = list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))
    ncol = len(metrics.EVAL_CSV_HEADER)
    assert rows[0][:ncol] == metrics.EVAL_CSV_HEADER and len(rows) == 1 + len(LAYOUT)
    m = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    pooled = np.zeros((2, 3, 3), dtype=np.int64)
    for r in rows[1:]:
        img, grey = truth[(r[1], r[0])]
        x = torch.from_numpy(img[None]).to(DEV)
        lg = torch.empty((1, 3) + img.shape[:2], dtype=torch.float32, device=DEV)
        lab, _ = m.predict_labels_windows(x, S, T, labels_dtype=torch.uint8, logits_full=lg)
        tgt = torch.from_numpy(np.ascontiguousarray(grey[None])).to(DEV)
        terms, _ = m.lovasz_softmax(lg, tgt)
        raw = lab.cpu().numpy()[0].copy()
        clean = m.remove_small_zones(lab)[0].cpu().numpy()[0]
        t = metrics.target_classes(grey)
        want = metrics.eval_row(r[0], r[1], metrics.confusion_numpy(raw, t), metrics.confusion_numpy(clean, t))
        assert r[:ncol] == want
        assert r[ncol:] == metrics.loss_cells(terms.cpu().numpy()[0], metrics.confusion_numpy(raw, t).sum(axis=1))
        plain = m.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)[0].cpu().numpy()[0]
        pooled[0] += metrics.confusion_numpy(plain, t)
        pooled[1] += metrics.confusion_numpy(clean, t)
    st = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, windows=S, windows_stride=T, windows_compare=True)
    win_csv = open(os.path.join(root, ev.STATS_CSV), "rb").read()
    assert win_csv != plain_csv                                    # the merged labels are not the frame's
    table, doc = ev.jitter_evaluation(["identity", "windows"], pooled)
    got = list(csv.reader(open(os.path.join(root, "results", ev.WINDOWS_EVALUATION_CSV)), delimiter="\t"))
    assert got == table and [r[0] for r in got] == ["View", "identity", "windows"]
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["windows"]["evaluation"] == json.loads(json.dumps(doc))
    assert {k: v for k, v in summary["windows"].items() if k != "evaluation"} == {"window": S, "stride": T, "blend": "tent"}
    ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0)
    assert open(os.path.join(root, ev.STATS_CSV), "rb").read() == plain_csv
