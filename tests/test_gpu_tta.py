"""The flip views on the GPU (nbc_tta_views, nbc_tta_merge, nbc_vote_tally, FCNResNet50.predict_labels_tta, predict / evaluate
--tta).  The kernels are compared bit for bit with the numpy restatement of tests/helpers/tta_oracle.py; the stacked forward
with single forwards of the flipped inputs, bit for bit; the logits with the CPU oracle run on each flipped input, under the
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
from neuralbarkcalculator_amd.model import FCNResNet50, fcn_efficientnet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tta_oracle as to  # noqa: E402
import vote_oracle as vo  # noqa: E402

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


# ---- 1. the views kernel ---------------------------------------------------------------------------------------------------
# (1, 2, 4101): a row longer than the mover's segment of 4096 units -- a second segment of five units whose mirror lands at the row's start
VIEW_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 40, 72), (1, 129, 65), (1, 8, 21), (1, 8, 22), (1, 2, 4101)]
VIEW_MASKS = [15, 3, 5, 9, 1, 10]


@pytest.mark.parametrize("shape", VIEW_SHAPES)
def test_views_kernel_is_the_numpy_flips(built_lib, shape):
    n, h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    u8 = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f32 = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    f32.reshape(-1)[0] = np.float32("nan")
    for mask in VIEW_MASKS:
        v = len(to.view_bits(mask))
        for x, dtype in ((u8, _lib.IN_U8_NHWC), (f32, _lib.IN_F32_NCHW)):
            for offset in ((0, 1) if x.dtype == np.uint8 else (0,)):      # a uint8 source one byte into its buffer
                raw = np.frombuffer(x.tobytes(), dtype=np.uint8)
                src = torch.zeros(raw.size + 64, dtype=torch.uint8, device=DEV)
                src[offset: offset + raw.size] = torch.from_numpy(raw.copy())
                guard = 48
                out = torch.full((v * raw.size + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
                rc = built_lib.nbc_tta_views(src.data_ptr() + offset, dtype, n, h, w, mask, out.data_ptr() + guard, stream())
                torch.cuda.synchronize()
                assert rc == _lib.NBC_OK, _lib.last_error()
                got = out.cpu().numpy()
                assert (got[:guard] == 0xAB).all() and (got[guard + v * raw.size:] == 0xAB).all(), (mask, offset)
                want = np.frombuffer(to.stack(x, mask).tobytes(), dtype=np.uint8)
                assert np.array_equal(got[guard: guard + v * raw.size], want), (shape, mask, str(x.dtype), offset)


def test_views_method_and_torch_flip(models):
    m = models["fp32"]
    x = frames([3, 4], 40, 72).to(DEV)
    s = m.tta_views(x, "flips")
    assert s.shape == (8, 3, 40, 72)
    want = torch.cat([x, torch.flip(x, dims=[3]), torch.flip(x, dims=[2]), torch.flip(x, dims=[2, 3])])
    assert torch.equal(s, want)
    u = torch.from_numpy(np.stack([synth.make_frame(5, 24, 40)])).to(DEV)
    assert torch.equal(m.tta_views(u, "hflip"), torch.cat([u, torch.flip(u, dims=[2])]))
    assert torch.equal(m.tta_views(u, "vflip"), torch.cat([u, torch.flip(u, dims=[1])]))
    assert torch.equal(m.tta_views(u, 1), u)
    with pytest.raises(ValueError):
        m.tta_views(u, 0)
    with pytest.raises(ValueError):
        m.tta_views(u, "rot90")


# ---- 2. the merge ----------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(got, want):
    """Bitwise equality, NaN positions compared as a mask."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (5, 9), (17, 9), (16, 16)])
def test_merge_is_the_restatement(built_lib, hw, n):
    h, w = hw
    rng = np.random.default_rng(100 * h + w + n)
    for mask in (15, 7, 3, 1, 10):
        v = len(to.view_bits(mask))
        x = (rng.standard_normal((v * n, 3, h, w)) * 10.0 ** rng.integers(-3, 4, size=(v * n, 3, h, w))).astype(np.float32)
        flat = x.reshape(-1)
        specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, 3.4e38, -3.4e38]
        pos = rng.choice(flat.size, size=min(flat.size, 4 * len(specials)), replace=False)
        for k, q in enumerate(pos):
            flat[q] = np.float32(specials[k % len(specials)])
        x[:, :, h // 2, w // 2] = np.float32(-0.0) if (h % 2 and w % 2) else x[:, :, h // 2, w // 2]   # the centre maps to itself: -0 in every view
        aligned_want = to.align(x, n, mask)
        merged_want = to.merge(aligned_want)
        src = torch.from_numpy(x).to(DEV)
        for want_aligned in (True, False):
            merged = torch.full((n * 3 * h * w + 8,), 7.0, dtype=torch.float32, device=DEV)
            aligned = torch.full((v * n * 3 * h * w + 8,), 7.0, dtype=torch.float32, device=DEV)
            rc = built_lib.nbc_tta_merge(src.data_ptr(), n, h, w, mask, merged.data_ptr(), aligned.data_ptr() if want_aligned else None,
                                         stream())
            torch.cuda.synchronize()
            assert rc == _lib.NBC_OK, _lib.last_error()
            mg, al = merged.cpu().numpy(), aligned.cpu().numpy()
            assert (mg[n * 3 * h * w:] == 7.0).all() and (al[v * n * 3 * h * w:] == 7.0).all()
            assert same_floats(mg[: n * 3 * h * w].reshape(merged_want.shape), merged_want), (hw, n, mask)
            if want_aligned:
                assert same_floats(al[: v * n * 3 * h * w].reshape(aligned_want.shape), aligned_want), (hw, n, mask)
                if v == 1:
                    assert same_floats(mg[: n * 3 * h * w].reshape(x.shape), to.align(x, n, mask)[0])
            else:
                assert (al == 7.0).all()


# ---- 3. the tally ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 4, 7])
@pytest.mark.parametrize("shape", [(1, 7, 9), (3, 31, 45), (2, 129, 65)])
def test_vote_tally_on_crafted_labels(built_lib, shape, d):
    n, h, w = shape
    rng = np.random.default_rng(d * 100 + h)
    labels = rng.integers(0, 4, size=(d, n, h, w), dtype=np.uint8)        # 3 votes nowhere
    labels[:, :, 0, :3] = 1
    labels[:, :, -1, -3:] = 2
    more = rng.integers(0, 4, size=(d, n, h, w), dtype=np.uint8)
    words = torch.full((n * h * w + 8,), -1, dtype=torch.int32, device=DEV)
    for lab, accumulate in ((labels, 0), (more, 1)):
        dev = torch.from_numpy(lab).to(DEV)
        rc = built_lib.nbc_vote_tally(dev.data_ptr(), n, d, h, w, words.data_ptr(), accumulate, stream())
        torch.cuda.synchronize()
        assert rc == _lib.NBC_OK, _lib.last_error()
    got = words.cpu().numpy().view(np.uint32)
    assert (got[n * h * w:] == 0xffffffff).all()
    assert np.array_equal(got[: n * h * w].reshape(n, h, w), vo.tally(labels) + vo.tally(more))
    m_words = vo.tally(labels)
    assert int((m_words & 0xffff).max()) == d and int((m_words >> 16).max()) == d


# ---- 4. the stack is the single forwards -----------------------------------------------------------------------------------
def singles(m, x, mask):
    """[V,N,3,h,w]: model.lowres_logits of each flipped input, un-flipped with torch."""
    out = []
    for b in to.view_bits(mask):
        rows, cols = to.mirrors(b)
        dims = ([2] if rows else []) + ([3] if cols else [])
        xf = torch.flip(x, dims=dims).contiguous() if dims else x
        low = m.lowres_logits(xf)
        out.append(torch.flip(low, dims=dims) if dims else low)
    return torch.stack(out)


@pytest.mark.parametrize("mode,bn,shape", [("fp32", "running", (2, 129, 191)), ("f16x2", "running", (2, 129, 191)),
                                           ("bf16", "running", (2, 129, 191)), ("fp32", "image", (1, 129, 191))])
def test_stack_is_the_single_forwards(models, sd_np, mode, bn, shape):
    m = models[mode]
    if bn != "running":
        m = FCNResNet50(mode).load_state_dict(sd_np).to(DEV).set_bn_statistics(bn)
    n, h, w = shape
    x = frames(range(10, 10 + n), h, w).to(DEV)
    out = m.predict_labels_tta(x, "flips", return_lowres=True, return_views=True)
    merged, aligned = out[2], out[6]
    want = singles(m, x, 15)
    assert torch.equal(aligned, want)
    assert same_floats(merged.cpu().numpy(), to.merge(want.cpu().numpy()))
    assert not torch.equal(aligned[0], aligned[1])                 # the network is not flip-equivariant: the views differ


# ---- 5. against the CPU oracle ---------------------------------------------------------------------------------------------
ORACLE_CASES = [((2, 129, 191), 30), ((1, 200, 121), 50), ((2, 160, 160), 60)]
_oracle_cache = {}


def oracle_views(oracle_model, shape, first):
    """The oracle on each flipped input, un-flipped: (aligned [4,N,3,h,w], merged [N,3,h,w], merged logits, merged labels)."""
    key = (shape, first)
    if key not in _oracle_cache:
        import torch.nn.functional as F
        from oracle.fcn_resnet50_oracle import predict_labels
        n, h, w = shape
        x = frames(range(first, first + n), h, w)
        al = []
        for b in range(4):
            rows, cols = to.mirrors(b)
            dims = ([2] if rows else []) + ([3] if cols else [])
            low = predict_labels(oracle_model, torch.flip(x, dims=dims).contiguous() if dims else x)[3]
            al.append(torch.flip(low, dims=dims) if dims else low)
        al = torch.stack(al)
        merged = torch.from_numpy(to.merge(al.numpy()))
        logits = F.interpolate(merged, size=(h, w), mode="bicubic", align_corners=False)
        _oracle_cache[key] = (x, al, merged, logits, torch.argmax(logits, dim=1))
    return _oracle_cache[key]


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_against_the_cpu_oracle(oracle_model, models, case, mode):
    shape, first = case
    n, h, w = shape
    x, al_ref, merged_ref, logits_ref, labels_ref = oracle_views(oracle_model, shape, first)
    m = models[mode]
    lg = torch.empty((n, 3, h, w), dtype=torch.float32, device=DEV)
    labels, counts, merged, vcounts, support, stats, aligned = m.predict_labels_tta(x.to(DEV), "flips", logits_full=lg,
                                                                                    return_lowres=True, return_views=True)
    scale = float(logits_ref.abs().max())
    rtol = LOGIT_RTOL_BF16 if mode == "bf16" else LOGIT_RTOL_FP32
    errs = [float((aligned[j].cpu() - al_ref[j]).abs().max()) for j in range(4)]
    err_m = float((merged.cpu() - merged_ref).abs().max())
    err = float((lg.cpu() - logits_ref).abs().max())
    print(mode, shape, "view errs", errs, "merged", err_m, "full", err, "scale", scale)
    for e in errs + [err_m, err]:
        assert e <= rtol * scale, (e, scale)
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
    assert len(torch.unique(labels_ref)) == 3                      # the merged maps hold all three classes
    unanimous = float(stats[:, 3:6].sum().cpu()) / (n * h * w)
    assert unanimous < 0.5, unanimous                              # the views disagree on most pixels of this checkpoint


# ---- 6. predict_labels_tta is its parts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_predict_labels_tta_is_its_parts(models, mode):
    m = models[mode]
    n, h, w = 2, 129, 191
    x = frames([70, 71], h, w).to(DEV)
    before = m.predict_labels(x, small_zones=True, return_lowres=True)
    for kw in (dict(), dict(small_zones=True), dict(small_zones=True, exclude_nodes=True), dict(exclude_nodes=True),
               dict(small_zones=True, min_pixels=40)):
        lg = torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV)
        labels, counts, merged, vcounts, support, stats, aligned = m.predict_labels_tta(
            x, "flips", labels_dtype=torch.uint8, logits_full=lg, return_lowres=True, return_views=True, **kw)
        zones, remap, minpx = kw.get("small_zones", False), kw.get("exclude_nodes", False), kw.get("min_pixels", 150)

        def tail(low):
            lab, cnt, full = m.upsample_argmax(low, (h, w), exclude_nodes=remap and not zones, labels_dtype=torch.uint8, return_logits=True)
            if zones:
                lab, cnt = m.remove_small_zones(lab, exclude_nodes=remap, min_pixels=minpx)
            return lab, cnt, full

        lab_w, cnt_w, full_w = tail(merged)
        assert torch.equal(labels, lab_w) and torch.equal(counts, cnt_w) and torch.equal(lg, full_w), kw
        assert int(counts.sum()) == n * h * w and (counts.sum(1) == h * w).all()
        if not zones:
            want = torch.argmax(lg, dim=1)
            if remap:
                want[want == 2] = 1
            assert torch.equal(labels.long(), want)
        view_labels = np.stack([tail(aligned[j])[0].cpu().numpy() for j in range(4)])
        c_w, s_w, st_w = to.view_figures(view_labels)
        assert np.array_equal(vcounts.cpu().numpy(), c_w) and np.array_equal(support.cpu().numpy(), s_w), kw
        assert np.array_equal(stats.cpu().numpy(), st_w), kw
        assert vcounts.shape == (4, n, 3) and vcounts.dtype == torch.int64 and support.dtype == torch.uint8
    # without the extras: the pair of predict_labels, int64 labels by default
    pair = m.predict_labels_tta(x, "flips", small_zones=True)
    assert len(pair) == 2 and pair[0].dtype == torch.int64
    # the mask 1 is predict_labels itself
    one = m.predict_labels_tta(x, 1, small_zones=True, return_lowres=True)
    assert all(torch.equal(a, b) for a, b in zip(one, before))
    lg0, lg1 = (torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV) for _ in range(2))
    a = m.predict_labels(x, logits_full=lg0, exclude_nodes=True)
    b = m.predict_labels_tta(x, 1, logits_full=lg1, exclude_nodes=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(lg0, lg1)
    # one image alone equals itself at each position of a batch of 3
    xa = frames([72], h, w).to(DEV)
    fill = frames([73, 74], h, w).to(DEV)
    alone = m.predict_labels_tta(xa, "flips", small_zones=True, return_lowres=True, return_views=True)
    for pos in range(3):
        xs = list(fill)
        xs.insert(pos, xa[0])
        got = m.predict_labels_tta(torch.stack(xs), "flips", small_zones=True, return_lowres=True, return_views=True)
        for k in (0, 1, 2, 4, 5):
            assert torch.equal(got[k][pos], alone[k][0]), (pos, k)
        assert torch.equal(got[3][:, pos], alone[3][:, 0]) and torch.equal(got[6][:, pos], alone[6][:, 0]), pos
    # a plain predict_labels afterwards has the same bits, and the TTA call left no forward behind for the draws
    m.predict_labels_tta(x, "hflip")
    with pytest.raises(RuntimeError, match="none has run"):
        m.dropout_draws(2, [1, 2])
    after = m.predict_labels(x, small_zones=True, return_lowres=True)
    assert all(torch.equal(a, b) for a, b in zip(after, before))
    assert not m.nonfinite_seen()


# ---- 7. the other networks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["deeplabv3_resnet50", "fcn_efficientnet_b0"])
def test_other_networks(built_lib, arch):
    from neuralbarkcalculator_amd.model import DeepLabV3ResNet50
    sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
    m = (DeepLabV3ResNet50("fp32") if arch == "deeplabv3_resnet50" else fcn_efficientnet(0)).load_state_dict(sd).to(DEV)
    n, h, w = 1, 160, 160
    x = frames([80], h, w).to(DEV)
    lg = torch.zeros((n, 3, h, w), dtype=torch.float32, device=DEV)
    labels, counts, merged, vcounts, support, stats, aligned = m.predict_labels_tta(x, "flips", labels_dtype=torch.uint8, logits_full=lg,
                                                                                    small_zones=True, return_lowres=True, return_views=True)
    want = singles(m, x, 15)
    assert torch.equal(aligned, want)
    assert same_floats(merged.cpu().numpy(), to.merge(want.cpu().numpy()))
    lab_w, _, full_w = m.upsample_argmax(merged, (h, w), labels_dtype=torch.uint8, return_logits=True)
    lab_w, cnt_w = m.remove_small_zones(lab_w)
    assert torch.equal(labels, lab_w) and torch.equal(counts, cnt_w) and torch.equal(lg, full_w)
    view_labels = []
    for j in range(4):
        lab, _ = m.upsample_argmax(aligned[j], (h, w), labels_dtype=torch.uint8)
        view_labels.append(m.remove_small_zones(lab)[0].cpu().numpy())
    c_w, s_w, st_w = to.view_figures(np.stack(view_labels))
    assert np.array_equal(vcounts.cpu().numpy(), c_w) and np.array_equal(support.cpu().numpy(), s_w)
    assert np.array_equal(stats.cpu().numpy(), st_w)


# ---- 8. folders ------------------------------------------------------------------------------------------------------------
# the LAYOUT of tests/test_gpu_dropout_votes.py, restated
LAYOUT = [("sapin", "s00.bmp", 40, 128, 192), ("sapin", "s01.png", 41, 128, 192), ("sapin", "s02.bmp", 42, 96, 192),
          ("epinette_gelee", "e00.png", 43, 128, 192), ("epinette_gelee", "e01.png", 44, 160, 160),
          ("epinette_non_gelee", "n00.png", 45, 96, 192)]


def _make_folder(root, sd_np, masks=False):
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
    for tag, kw in (("plain", {}), ("tta", dict(tta="flips")), ("votes", dict(tta="flips", tta_votes=True)),
                    ("votes_b1s4", dict(tta="flips", tta_votes=True, batch=1, streams=4))):
        roots[tag] = str(tmp_path / tag)
        ckpt = _make_folder(roots[tag], sd_np)
        st = drv.predict_folder(roots[tag], ckpt, precision="fp32", device_index=0, **kw)
        assert st["images_total"] == len(LAYOUT)
    files = {tag: _result_bytes(root) for tag, root in roots.items()}
    assert len(files["plain"]) == 1 + len(LAYOUT)                  # final_stats.csv and the label PNGs: untouched by the feature
    new = {"results/tta_stats.csv", "results/tta_summary.json"}
    support = {"results/tta_support/%s/%s" % (wood, name.replace("bmp", "png")) for wood, name, _, _, _ in LAYOUT}
    assert set(files["tta"]) == set(files["plain"]) | new
    assert set(files["votes"]) == set(files["tta"]) | support
    assert {k: v for k, v in files["votes"].items() if k not in support} == files["tta"]
    assert files["votes_b1s4"] == files["votes"]
    assert files["tta"]["results/final_stats.csv"] != files["plain"]["results/final_stats.csv"]      # the merged labels differ

    # tta_stats.csv, final_stats.csv and the PNGs: model-level calls, one image at a time
    root = roots["votes"]
    model = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    images, stats_rows = [], []
    for _, name, wood in drv.list_images(os.path.join(root, "processed")):
        frame = np.asarray(Image.open(os.path.join(root, "processed", "samples", wood, name)).convert("RGB"))
        x = torch.from_numpy(np.ascontiguousarray(frame[None])).to(DEV)
        labels, counts, vcounts, sup, stats, _ = model.predict_labels_tta(x, "flips", labels_dtype=torch.uint8, small_zones=True,
                                                                          return_views=True)
        h, w = frame.shape[:2]
        images.append((name, wood, h, w, counts.cpu().numpy()[0], vcounts.cpu().numpy()[:, 0], stats.cpu().numpy()[0]))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "outputs", wood, name))), drv.label_png(labels.cpu().numpy()[0]))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "tta_support", wood, name))), sup.cpu().numpy()[0])
        c = counts.cpu().numpy()[0]
        stats_rows.append(drv.stats_row(name, wood, h, w, int(c[1]), int(c[2])))
    table, summary = folder_run.tta_report(images, 15)
    got = list(csv.reader(open(os.path.join(root, "results", "tta_stats.csv")), delimiter="\t"))
    assert got == table and len(got) == 1 + len(LAYOUT)
    final = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert final[1:] == [[str(v) for v in r] for r in stats_rows]
    doc = json.load(open(os.path.join(root, "results", "tta_summary.json")))
    assert doc["views"] == ["identity", "hflip", "vflip", "hvflip"] and doc["precision"] == "fp32" and doc["bn_stats"] == "running"
    assert doc["means"] == json.loads(json.dumps(summary["means"])) and doc["images"] == len(LAYOUT)

    # two gloo ranks sharing the GPU, as tests/test_gpu_dropout_votes.py sets them up
    root2 = str(tmp_path / "w2")
    ckpt2 = _make_folder(root2, sd_np)
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import predict\n"
            "dist.init_process_group('gloo')\n"
            "st = predict.predict_folder(%r, %r, precision='fp32', device_index=0, tta='flips', tta_votes=True)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, root2, ckpt2, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29647", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _result_bytes(root2) == files["votes"]


def test_evaluate_folder(tmp_path, sd_np, built_lib):
    """evaluate --tta flips: every row is metrics.py on the model-level merged labels; the run without the flag differs."""
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
    assert "tta" not in json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    st = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, tta="flips", loss=True)
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["tta"] == {"views": ["identity", "hflip", "vflip", "hvflip"]} and st["summary"]["tta"] == summary["tta"]
    assert summary["images_evaluated"] == len(LAYOUT) and st["batch"] == 1
    rows = list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))
    ncol = len(metrics.EVAL_CSV_HEADER)
    assert rows[0][:ncol] == metrics.EVAL_CSV_HEADER and len(rows) == 1 + len(LAYOUT)
    m = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    for r in rows[1:]:
        img, grey = truth[(r[1], r[0])]
        x = torch.from_numpy(img[None]).to(DEV)
        lg = torch.empty((1, 3) + img.shape[:2], dtype=torch.float32, device=DEV)
        lab, _ = m.predict_labels_tta(x, "flips", labels_dtype=torch.uint8, logits_full=lg)
        tgt = torch.from_numpy(np.ascontiguousarray(grey[None])).to(DEV)
        terms, _ = m.lovasz_softmax(lg, tgt)
        raw = lab.cpu().numpy()[0].copy()
        clean = m.remove_small_zones(lab)[0].cpu().numpy()[0]
        t = metrics.target_classes(grey)
        want = metrics.eval_row(r[0], r[1], metrics.confusion_numpy(raw, t), metrics.confusion_numpy(clean, t))
        assert r[:ncol] == want
        assert r[ncol:] == metrics.loss_cells(terms.cpu().numpy()[0], metrics.confusion_numpy(raw, t).sum(axis=1))
    ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, tta="flips")
    tta_csv = open(os.path.join(root, ev.STATS_CSV), "rb").read()
    assert tta_csv != plain_csv                                    # the merged labels are not the identity view's
    ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0)
    assert open(os.path.join(root, ev.STATS_CSV), "rb").read() == plain_csv
