"""The Dropout draws on the GPU (nbc_dropout_draws, FCNResNet50.dropout_draws, predict --dropout_draws) against the numpy
restatement of tests/helpers/dropout_oracle.py and the CPU oracle: p = 0 is the forward bit for bit, the kernel on the
operands it read, the CPU oracle under the same mask, the counts, the invariances (batch, stream, object, call split, pass
size), what must not move, and the folder driver."""
import copy
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, folder_run, synth
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import DeepLabV3ResNet50, FCNResNet50, fcn_resnet50

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dropout_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the FCN parity suite's tolerances (tests/test_gpu_parity.py), restated because they bound the same quantity: the error of
# low-resolution logits against the CPU oracle, relative to the oracle's largest logit
LOGIT_RTOL_FP32 = 5e-6
LOGIT_RTOL_BF16 = 4e-2
MAX_TIE_FLIPS_FRAC = 4e-6
# the masked classifier against float64 on its own operands: 17 roundings of 2^-24 relative each -- the mask multiply, the
# product, 7 chain adds, 6 tree adds, the bias, and one of slack for f16x2's join -- of the sum of magnitudes
KERNEL_ROUNDINGS = 17

ID_A, ID_B = folder_run.image_id("sapin", "a.png"), folder_run.image_id("epinette_gelee", "EPN 9 A.png")


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


@pytest.fixture(scope="module")
def models(sd_np, built_lib):
    return {m: FCNResNet50(m).load_state_dict(sd_np).to(DEV) for m in ("fp32", "f16x2", "bf16")}


@pytest.fixture(scope="module")
def image_model(sd_np, built_lib):
    return fcn_resnet50(precision="fp32", bn_statistics="image").load_state_dict(sd_np).to(DEV)


def check_labels(labels_gpu, labels_ref, logits_ref, err, band_scale=2.0, max_frac=MAX_TIE_FLIPS_FRAC):
    """The parity suite's rule: identical outside the tie band, bounded inside it."""
    top2 = torch.topk(logits_ref, 2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    mism = labels_gpu.cpu() != labels_ref
    n_mism = int(mism.sum())
    if n_mism:
        worst = float(margin[mism].max())
        assert worst <= band_scale * err, f"{n_mism} label flips, one at oracle margin {worst} > {band_scale}*{err}"
    assert n_mism <= max(2, max_frac * mism.numel()), f"{n_mism} label flips of {mism.numel()}"
    return n_mism


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16", "fp32-image"])
def test_p_zero_is_the_forward_bit_for_bit(models, image_model, mode):
    m = image_model if mode == "fp32-image" else models[mode]
    x = frames([5, 6], 96, 160).to(DEV)
    for small_zones, exclude in ((True, False), (False, True)):
        labels, counts, lowres = m.predict_labels(x, exclude_nodes=exclude, return_lowres=True, small_zones=small_zones)
        dcounts, dlow = m.dropout_draws(3, [ID_A, ID_B], p=0.0, seed=42, small_zones=small_zones, exclude_nodes=exclude,
                                        return_lowres=True)
        assert dlow.shape == (3, 2, 3, 12, 20) and dcounts.shape == (3, 2, 3) and dcounts.dtype == torch.int64
        for d in range(3):
            assert torch.equal(dlow[d], lowres), (mode, d)
            assert torch.equal(dcounts[d], counts), (mode, d)
    assert not m.nonfinite_seen()


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16"])
def test_kernel_on_the_operands_it_read(models, sd_np, mode):
    """X as the device stored it (keep mode), the definition in float64 under the restatement's mask: every logit within
    17 * 2^-24 * (sum_c |w X m keep| + |bias|).  Derived from the roundings of the arithmetic, not measured."""
    m = models[mode]
    x = frames([7, 8], 128, 192)
    p, seed, ids = 0.1, 42, [ID_A, ID_B]
    m.set_keep_activations(True)
    try:
        m.lowres_logits(x.to(DEV))
        _, dlow = m.dropout_draws(2, ids, p=p, seed=seed, first_draw=30, return_lowres=True)
        torch.cuda.synchronize()
        feats = m.read_activation("classifier.0", 2 * 512 * 16 * 24)
        assert m.activation_exponent("classifier.0") == 0
    finally:
        m.set_keep_activations(False)
    assert feats.shape == (2, 512, 16, 24)
    worst = 0.0
    for d in range(2):
        keep = np.stack([do.keep_image(seed, ids[i], 30 + d, p, 16, 24) for i in range(2)])
        want, mag = do.by_hand(sd_np["classifier.4.weight"], sd_np["classifier.4.bias"], feats, keep, p)
        ratio = np.abs(dlow[d].cpu().numpy().astype(np.float64) - want) / (KERNEL_ROUNDINGS * 2.0 ** -24 * mag)
        worst = max(worst, float(ratio.max()))
    print("dropout kernel %s: worst error is %.3f of the 17-rounding bound" % (mode, worst), flush=True)
    assert worst <= 1.0, worst


_ORACLE_CACHE = {}


def _oracle_case(oracle_model, case):
    if case not in _ORACLE_CACHE:
        idx, h, w = case
        x = frames(idx, h, w)
        _ORACLE_CACHE[case] = (x, do.features(oracle_model, x))
    return _ORACLE_CACHE[case]


@pytest.mark.parametrize("case,draws", [(((11, 12), 256, 256), 3), (((13,), 1024, 1024), 1)])
@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16"])
def test_against_the_cpu_oracle_under_the_same_mask(models, oracle_model, mode, case, draws):
    m = models[mode]
    x, feats = _oracle_case(oracle_model, case)
    n, (h, w) = x.shape[0], x.shape[-2:]
    ids = [ID_A, ID_B][:n]
    p, seed = 0.1, 42
    m.lowres_logits(x.to(DEV))
    _, dlow = m.dropout_draws(draws, ids, p=p, seed=seed, return_lowres=True, small_zones=False)
    dlow = dlow.cpu()
    rtol = LOGIT_RTOL_BF16 if mode == "bf16" else LOGIT_RTOL_FP32
    for d in range(draws):
        want = do.draw_lowres(oracle_model, feats, ids, seed, d, p)
        scale = float(want.abs().max())
        err = float((dlow[d] - want).abs().max())
        print("dropout %s %dx%dx%d draw %d: logit err %.3e of range %.4g = %.3e relative" % (mode, n, h, w, d, err, scale, err / scale),
              flush=True)
        if err > rtol * scale:
            # adjudicated as tests/test_gpu_bn_stats.py does: the GPU within 1.5x of the f32 oracle's own distance to float64
            o64 = copy.deepcopy(oracle_model).double()
            w64 = do.draw_lowres(o64, do.features(o64, x.double()), ids, seed, d, p)
            e_gpu = float((dlow[d].double() - w64).abs().max())
            e_ref = float((want.double() - w64).abs().max())
            print("dropout %s %dx%dx%d draw %d adjudicated against float64: gpu %.3e, f32 oracle %.3e" % (mode, n, h, w, d, e_gpu, e_ref),
                  flush=True)
            assert e_gpu <= max(rtol * scale, 1.5 * e_ref), (mode, case, d, e_gpu, e_ref, scale)
        if mode != "bf16":
            labels_ref, logits_ref = do.upsample_labels(want, (h, w))
            labels, _ = m.upsample_argmax(dlow[d].to(DEV), (h, w))
            check_labels(labels, labels_ref, logits_ref, max(err, 1e-7 * scale))


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_counts_are_those_of_the_returned_logits(models, mode):
    m = models[mode]
    x = frames([15, 16], 200, 256).to(DEV)
    m.lowres_logits(x)
    ids = [ID_A, ID_B]
    for kw in (dict(small_zones=True, exclude_nodes=False), dict(small_zones=True, exclude_nodes=True),
               dict(small_zones=True, exclude_nodes=False, min_pixels=0), dict(small_zones=False, exclude_nodes=True),
               dict(small_zones=True, exclude_nodes=False, min_pixels=2000)):
        dcounts, dlow = m.dropout_draws(5, ids, p=0.1, seed=1, return_lowres=True, **kw)
        zones = kw["small_zones"] and kw.get("min_pixels", 150) > 0
        for d in range(5):
            labels, counts = m.upsample_argmax(dlow[d], (200, 256), exclude_nodes=kw["exclude_nodes"] and not zones,
                                               labels_dtype=torch.uint8)
            if zones:
                labels, counts = m.remove_small_zones(labels, exclude_nodes=kw["exclude_nodes"], min_pixels=kw.get("min_pixels", 150))
            assert torch.equal(dcounts[d], counts), (mode, kw, d)
            assert int(dcounts[d].sum()) == 2 * 200 * 256
        assert len({tuple(dcounts[d].flatten().tolist()) for d in range(5)}) > 1      # the draws differ


@pytest.mark.parametrize("mode", ["fp32", "f16x2", "bf16", "fp32-image"])
def test_invariance(models, image_model, mode):
    m = image_model if mode == "fp32-image" else models[mode]
    xa, xb = frames([21], 96, 160), frames([22], 96, 160) * 0.5 + 0.3
    kw = dict(p=0.1, seed=7, return_lowres=True)

    def run(model, x, ids, draws=8, **more):
        model.lowres_logits(x.to(DEV))
        c, low = model.dropout_draws(draws, ids, **dict(kw, **more))
        return c.cpu(), low.cpu()

    c_ab, l_ab = run(m, torch.cat([xa, xb]), [ID_A, ID_B])
    c_ba, l_ba = run(m, torch.cat([xb, xa]), [ID_B, ID_A])
    c_a, l_a = run(m, xa, [ID_A])
    c_b, l_b = run(m, xb, [ID_B])
    # alone, or as either member of a batch of two
    assert torch.equal(l_ab[:, 0], l_a[:, 0]) and torch.equal(l_ba[:, 1], l_a[:, 0]) and torch.equal(l_ab[:, 1], l_b[:, 0])
    assert torch.equal(c_ab[:, 0], c_a[:, 0]) and torch.equal(c_ba[:, 1], c_a[:, 0]) and torch.equal(c_ba[:, 0], c_b[:, 0])
    # another stream, another object on the same weights
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c_s, l_s = run(m, xa, [ID_A])
    torch.cuda.synchronize()
    assert torch.equal(l_s, l_a) and torch.equal(c_s, c_a)
    c_c, l_c = run(m.clone_shared(), xa, [ID_A])
    assert torch.equal(l_c, l_a) and torch.equal(c_c, c_a)
    # draws 0..7 in one call, or 0..3 then 4..7
    m.lowres_logits(xa.to(DEV))
    c0, l0 = m.dropout_draws(4, [ID_A], **kw)
    c1, l1 = m.dropout_draws(4, [ID_A], first_draw=4, **kw)
    assert torch.equal(torch.cat([l0, l1]).cpu(), l_a) and torch.equal(torch.cat([c0, c1]).cpu(), c_a)
    # a workspace for one draw per pass, or for eight (the default above), or for three (a ragged last pass)
    for per_pass in (1, 3):
        c_p, l_p = run(m, xa, [ID_A], draws_per_pass=per_pass)
        assert torch.equal(l_p, l_a) and torch.equal(c_p, c_a), per_pass
    # the same id twice in a batch (on the same image): equal rows
    c_aa, l_aa = run(m, torch.cat([xa, xa]), [ID_A, ID_A])
    assert torch.equal(l_aa[:, 0], l_aa[:, 1]) and torch.equal(c_aa[:, 0], c_aa[:, 1]) and torch.equal(l_aa[:, 0], l_a[:, 0])
    # another id, another seed, another draw: another mask
    _, l_id = run(m, torch.cat([xa, xa]), [ID_A, ID_B])
    assert not torch.equal(l_id[:, 0], l_id[:, 1])
    _, l_seed = run(m, xa, [ID_A], seed=8)
    assert not torch.equal(l_seed, l_a)
    assert not torch.equal(l_a[0], l_a[1])


def _record_keys(recs):
    return [(r["name"], r["kernel"], r["launches"], r["flops"], r["bytes"], r["k"], r["cout"]) for r in recs]


def test_nothing_else_moves(models, sd_np):
    m = models["fp32"]
    x = frames([25, 26], 128, 192).to(DEV)

    def profiled():
        m.set_profiling(True)
        try:
            m.lowres_logits(x)
            return m.op_records()
        finally:
            m.set_profiling(False)

    before = profiled()
    labels0, counts0 = m.predict_labels(x, small_zones=True)
    m.dropout_draws(4, [ID_A, ID_B], p=0.3, seed=3)
    labels1, counts1 = m.predict_labels(x, small_zones=True)
    assert torch.equal(labels0, labels1) and torch.equal(counts0, counts1)
    m.dropout_draws(2, [ID_A, ID_B])
    after = profiled()
    assert _record_keys(before) == _record_keys(after) and len(before) > 50
    assert "dropout" not in " ".join(r["kernel"] + r["name"] for r in after)

    # call order: the C ABI answers NBC_ERR_STATE for a shape other than the last forward's ...
    lib = m._lib
    ids = (C.c_uint64 * 2)(ID_A, ID_B)
    ws = torch.empty(int(lib.nbc_dropout_workspace_bytes(2, 128, 192, 1)), dtype=torch.uint8, device=DEV)
    counts = torch.empty((1, 2, 3), dtype=torch.int64, device=DEV)

    def call(ctx, n, h, w, nbytes=None):
        return lib.nbc_dropout_draws(ctx, n, h, w, ids, 0.1, 0, 0, 1, 150, 0, None, counts.data_ptr(), ws.data_ptr(),
                                     ws.numel() if nbytes is None else nbytes, None)

    m.lowres_logits(x)
    assert call(m._ctx, 2, 128, 192) == _lib.NBC_OK
    for shape in ((1, 128, 192), (2, 128, 200), (2, 136, 192)):
        assert call(m._ctx, *shape) == _lib.NBC_ERR_STATE, shape
        assert _lib.last_error().startswith("nbc_dropout_draws:")
    assert call(m._ctx, 2, 128, 192, ws.numel() - 1) == _lib.NBC_ERR_INVALID          # too small for one draw per pass
    m.reserve(1, 64, 64)                                                                # the plan has moved on
    assert call(m._ctx, 2, 128, 192) == _lib.NBC_ERR_STATE
    torch.cuda.synchronize()
    fresh = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)                          # no forward yet
    assert call(fresh._ctx, 2, 128, 192) == _lib.NBC_ERR_STATE
    with pytest.raises(RuntimeError):
        fresh.dropout_draws(1, [ID_A])
    # ... and for a DeepLab context
    dl = DeepLabV3ResNet50("fp32").load_state_dict(synth.make_state_dict("trained_like", seed=7, arch="deeplabv3_resnet50")).to(DEV)
    dl.lowres_logits(x)
    assert call(dl._ctx, 2, 128, 192) == _lib.NBC_ERR_STATE and "NBC_ARCH_FCN_RESNET50" in _lib.last_error()
    with pytest.raises(ValueError, match="DeepLabHead's Dropout sits inside ASPP"):
        dl.dropout_draws(1, [ID_A, ID_B])
    with pytest.raises(ValueError):
        m.dropout_draws(0, [ID_A, ID_B])
    with pytest.raises(ValueError):
        m.dropout_draws(1, [ID_A, ID_B], p=1.0)


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


def test_folder_driver(tmp_path, sd_np, built_lib):
    D = 4
    plain = str(tmp_path / "plain")
    ckpt = _make_folder(plain, sd_np)
    drv.predict_folder(plain, ckpt, precision="fp32", device_index=0)
    want_files = _result_bytes(plain)
    assert "results/final_stats.csv" in want_files and len(want_files) == 1 + len(LAYOUT)

    runs = {}
    for tag, kw in (("default", {}), ("b1s1", dict(batch=1, streams=1)), ("b2s4", dict(batch=2, streams=4)),
                    ("b1s4", dict(batch=1, streams=4))):
        root = str(tmp_path / tag)
        ckpt = _make_folder(root, sd_np)
        st = drv.predict_folder(root, ckpt, precision="fp32", device_index=0, dropout_draws=D, dropout_seed=42, **kw)
        assert st["images_total"] == len(LAYOUT)
        runs[tag] = _result_bytes(root)
    for tag, files in runs.items():
        # everything a run without the flag writes is byte for byte the same, and two files are new
        assert set(files) == set(want_files) | {"results/dropout_stats.csv", "results/dropout_summary.json"}, tag
        for k, v in want_files.items():
            assert files[k] == v, (tag, k)
        assert files["results/dropout_stats.csv"] == runs["default"]["results/dropout_stats.csv"], tag
        assert files["results/dropout_summary.json"] == runs["default"]["results/dropout_summary.json"], tag

    # the table: model-level draws, one image at a time under image_id(wood, name)
    root = str(tmp_path / "default")
    model = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    images, draw0 = [], []
    for _, name, wood in drv.list_images(os.path.join(root, "processed")):
        frame = np.asarray(Image.open(os.path.join(root, "processed", "samples", wood, name)).convert("RGB"))
        x = torch.from_numpy(np.ascontiguousarray(frame[None])).to(DEV)
        _, counts = model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
        dc = model.dropout_draws(D, [folder_run.image_id(wood, name)], p=0.1, seed=42, small_zones=True).cpu().numpy()[:, 0]
        counts = counts.cpu().numpy()[0]
        images.append((name, wood, frame.shape[0], frame.shape[1], int(counts[1]), int(counts[2]), dc))
        draw0.append(drv.stats_row(name, wood, frame.shape[0], frame.shape[1], int(dc[0, 1]), int(dc[0, 2])))
    table, summary = folder_run.dropout_report(images, D)
    got = list(csv.reader(open(os.path.join(root, "results", "dropout_stats.csv")), delimiter="\t"))
    assert got == table and got[0] == folder_run.DROPOUT_COLUMNS and len(got) == 1 + len(LAYOUT)
    final = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert [(r[0], r[1], r[2], r[3]) for r in got[1:]] == [(r[0], r[1], r[2], r[4]) for r in final[1:]]
    doc = json.load(open(os.path.join(root, "results", "dropout_summary.json")))
    assert (doc["p"], doc["seed"], doc["draws"], doc["precision"], doc["bn_stats"], doc["images"]) == (0.1, 42, D, "fp32", "running", 6)
    assert doc["means"] == json.loads(json.dumps(summary["means"]))
    assert any(float(r[5]) > 0 for r in got[1:])                                      # the draws are live

    # two gloo ranks sharing the GPU, as tests/test_gpu_folder.py sets them up
    root2 = str(tmp_path / "w2")
    ckpt2 = _make_folder(root2, sd_np)
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import predict\n"
            "dist.init_process_group('gloo')\n"
            "st = predict.predict_folder(%r, %r, precision='fp32', device_index=0, dropout_draws=%d, dropout_seed=42)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, root2, ckpt2, D, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29641", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _result_bytes(root2) == runs["default"]

    # --dropout_compare against a file made of draw 0's own counts, through the command line: every image inside
    root3 = str(tmp_path / "cmp")
    ckpt3 = _make_folder(root3, sd_np)
    old = str(tmp_path / "old_final_stats.csv")
    drv.write_stats_csv(old, draw0)
    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", root3, "--model_path", ckpt3, "--precision", "fp32",
                        "--dropout_draws", str(D), "--dropout_seed", "42", "--dropout_compare", old],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    files3 = _result_bytes(root3)
    for k, v in want_files.items():
        assert files3[k] == v, k
    rows = list(csv.reader(open(os.path.join(root3, "results", "dropout_stats.csv")), delimiter="\t"))
    assert rows[0] == folder_run.DROPOUT_COLUMNS + folder_run.DROPOUT_COMPARE_COLUMNS
    assert [r[:13] for r in rows[1:]] == table[1:]
    assert all(r[15] == "1" and r[16] == "1" for r in rows[1:]), [r[13:] for r in rows[1:]]
    doc3 = json.load(open(os.path.join(root3, "results", "dropout_summary.json")))
    assert doc3["compare"]["bark_inside"] == doc3["compare"]["node_inside"] == doc3["compare"]["images_compared"] == len(LAYOUT)
    assert doc3["compare"]["missing_from_old"] == []
