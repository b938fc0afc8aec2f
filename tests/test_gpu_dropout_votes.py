"""The per-pixel votes of the Dropout draws on the GPU (nbc_dropout_votes, nbc_vote_summary, FCNResNet50.dropout_votes,
predict --dropout_votes).  The oracle: each draw's returned low-resolution logits through the existing upsample_argmax and
remove_small_zones methods (which have tests of their own), tallied in numpy by tests/helpers/vote_oracle.py.  Everything is
integers and compared exactly: no tolerance anywhere."""
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
from neuralbarkcalculator_amd.model import DeepLabV3ResNet50, FCNResNet50

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import vote_oracle as vo  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID_A, ID_B = folder_run.image_id("sapin", "a.png"), folder_run.image_id("epinette_gelee", "EPN 9 A.png")


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


@pytest.fixture(scope="module")
def models(sd_np, built_lib):
    return {m: FCNResNet50(m).load_state_dict(sd_np).to(DEV) for m in ("fp32", "f16x2")}


def u32(t):
    """The uint32 vote words of an int32 tensor."""
    return t.cpu().numpy().view(np.uint32)


def oracle_words(m, dlow, hw, small_zones=True, exclude_nodes=False, min_pixels=150):
    """The draws' final label maps as tests/test_gpu_dropout.py::test_counts_are_those_of_the_returned_logits makes them, and
    their tally.  Returns (words uint32 [N,H,W], counts int64 [D,N,3])."""
    zones = small_zones and min_pixels > 0
    maps, counts = [], []
    for d in range(dlow.shape[0]):
        labels, cnt = m.upsample_argmax(dlow[d], hw, exclude_nodes=exclude_nodes and not zones, labels_dtype=torch.uint8)
        if zones:
            labels, cnt = m.remove_small_zones(labels, exclude_nodes=exclude_nodes, min_pixels=min_pixels)
        maps.append(labels.cpu().numpy())
        counts.append(cnt.cpu().numpy())
    return vo.tally(np.stack(maps)), np.stack(counts)


def check_against_oracle(m, out, hw, draws, **kw):
    counts, vlab, sup, stats, low, words = out
    want_words, want_counts = oracle_words(m, low, hw, **kw)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    got = u32(words)
    assert np.array_equal(got, want_words)
    label, support, _, valid = vo.decode(want_words, draws)
    assert valid.all()
    assert np.array_equal(vlab.cpu().numpy(), label) and np.array_equal(sup.cpu().numpy(), support)
    st = stats.cpu().numpy()
    assert st.dtype == np.int64 and np.array_equal(st, vo.stats(want_words, draws))
    # the votes are the draws' counts summed, and every pixel has a winner
    cn = counts.cpu().numpy()
    assert np.array_equal(st[:, 8], cn[:, :, 1].sum(0)) and np.array_equal(st[:, 9], cn[:, :, 2].sum(0))
    assert (st[:, 0:3].sum(1) == hw[0] * hw[1]).all() and (st[:, 7] == 0).all()
    return got, st


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_main_case_against_the_oracle(models, mode):
    m = models[mode]
    h, w, D = 200, 256, 5
    m.lowres_logits(frames([15, 16], h, w).to(DEV))
    ids = [ID_A, ID_B]
    counts0, low0 = m.dropout_draws(D, ids, p=0.1, seed=1, return_lowres=True)
    out = m.dropout_votes(D, ids, p=0.1, seed=1, return_lowres=True, return_words=True)
    counts, vlab, sup, stats, low, words = out
    assert vlab.shape == sup.shape == (2, h, w) and vlab.dtype == sup.dtype == torch.uint8
    assert stats.shape == (2, 10) and stats.dtype == torch.int64 and counts.shape == (D, 2, 3)
    # counts and logits are bitwise those of dropout_draws on the same forward
    assert torch.equal(counts, counts0) and torch.equal(low, low0)
    _, st = check_against_oracle(m, out, (h, w), D)
    # not vacuous: the draws disagree somewhere
    assert (st[:, 3:6].sum(1) < h * w).any(), st
    # without the extras the tuple is the four of the interface
    four = m.dropout_votes(D, ids, p=0.1, seed=1)
    assert len(four) == 4 and all(torch.equal(a, b) for a, b in zip(four, (counts, vlab, sup, stats)))
    assert not m.nonfinite_seen()


@pytest.mark.parametrize("per_pass", [1, 3, 8])
def test_ragged_case_against_the_oracle(models, per_pass):
    """H * W = 8385 is odd: image 1 and, with more than one draw in a pass, every draw plane start off a 16-byte boundary."""
    m = models["fp32"]
    h, w, D = 129, 65, 5
    m.lowres_logits(frames([31, 32], h, w).to(DEV))
    ids = [ID_A, ID_B]
    for kw in (dict(min_pixels=0), dict(exclude_nodes=True), dict(min_pixels=0, exclude_nodes=True), dict()):
        out = m.dropout_votes(D, ids, p=0.5, seed=1, return_lowres=True, return_words=True, draws_per_pass=per_pass, **kw)
        words, st = check_against_oracle(m, out, (h, w), D, **kw)
        if kw.get("exclude_nodes"):
            assert (words >> 16).max() == 0 and (st[:, 9] == 0).all() and (st[:, 2] == 0).all()
        assert (st[:, 3:6].sum(1) < h * w).any(), kw             # the draws disagree somewhere


def c_votes(m, shape, ids, first, draws, words, accumulate, per_pass=8, p=0.1, seed=7, min_pixels=150, workspace_bytes=None):
    """nbc_dropout_votes through the C ABI on the current stream; returns (rc, counts)."""
    n, h, w = shape
    need = int(m._lib.nbc_dropout_workspace_bytes(n, h, w, per_pass))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=DEV)
    counts = torch.zeros((draws, n, 3), dtype=torch.int64, device=DEV)
    rc = m._lib.nbc_dropout_votes(m._ctx, n, h, w, (C.c_uint64 * n)(*ids), p, seed, first, draws, min_pixels, 0, None,
                                  counts.data_ptr(), words.data_ptr(), accumulate, ws.data_ptr(),
                                  need if workspace_bytes is None else workspace_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, counts


@pytest.mark.parametrize("mode", ["fp32", "f16x2"])
def test_invariance(models, mode):
    m = models[mode]
    h, w = 96, 160
    xa, xb = frames([21], h, w), frames([22], h, w) * 0.5 + 0.3
    kw = dict(p=0.1, seed=7, return_words=True)

    def run(model, x, ids, **more):
        model.lowres_logits(x.to(DEV))
        c, vlab, sup, st, words = model.dropout_votes(8, ids, **dict(kw, **more))
        return c.cpu(), vlab.cpu(), sup.cpu(), st.cpu(), words.cpu()

    def same(a, b, i=0, j=0):
        return torch.equal(a[0][:, i], b[0][:, j]) and all(torch.equal(a[k][i], b[k][j]) for k in (1, 2, 3, 4))

    alone = run(m, xa, [ID_A])
    ab, ba = run(m, torch.cat([xa, xb]), [ID_A, ID_B]), run(m, torch.cat([xb, xa]), [ID_B, ID_A])
    b_alone = run(m, xb, [ID_B])
    assert same(ab, alone, 0, 0) and same(ba, alone, 1, 0) and same(ab, b_alone, 1, 0) and same(ba, b_alone, 0, 0)
    assert not torch.equal(alone[4], b_alone[4])
    # another stream, another object on the same weights
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run(m, xa, [ID_A])
    torch.cuda.synchronize()
    assert same(on_side, alone)
    assert same(run(m.clone_shared(), xa, [ID_A]), alone)
    # the pass size: one draw per pass, three (a ragged last pass), eight (the default above)
    for per_pass in (1, 3):
        assert same(run(m, xa, [ID_A], draws_per_pass=per_pass), alone), per_pass
    # the C call: draws 0..7 at once, or 0..3 and then 4..7 added to them; words that hold rubbish are overwritten
    m.lowres_logits(xa.to(DEV))
    once = torch.full((1, h, w), -1, dtype=torch.int32, device=DEV)
    rc, c_once = c_votes(m, (1, h, w), [ID_A], 0, 8, once, 0)
    assert rc == _lib.NBC_OK, _lib.last_error()
    split = torch.full((1, h, w), -1, dtype=torch.int32, device=DEV)
    rc0, c0 = c_votes(m, (1, h, w), [ID_A], 0, 4, split, 0, per_pass=3)
    rc1, c1 = c_votes(m, (1, h, w), [ID_A], 4, 4, split, 1, per_pass=8)
    assert rc0 == rc1 == _lib.NBC_OK, _lib.last_error()
    assert torch.equal(once.cpu(), alone[4]) and torch.equal(split.cpu(), alone[4])
    assert torch.equal(c_once.cpu(), alone[0]) and torch.equal(torch.cat([c0, c1]).cpu(), alone[0])
    # accumulate = 1 on the same draws again doubles every field
    rc, _ = c_votes(m, (1, h, w), [ID_A], 0, 8, once, 1)
    assert rc == _lib.NBC_OK and np.array_equal(u32(once), 2 * u32(alone[4]))


def summary(lib, words, draws, want_labels=True, want_support=True, offset=0):
    """nbc_vote_summary on uint32 words [N,H,W] (numpy); the byte planes carry 32 guard bytes.  `offset`: the words start that
    many uint32 past a 16-byte boundary."""
    n, h, w = words.shape
    px = n * h * w
    buf = torch.zeros(px + 4, dtype=torch.int32, device=DEV)
    wt = buf[offset: offset + px]
    wt.copy_(torch.from_numpy(words.view(np.int32).reshape(-1)))
    lab = torch.full((px + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    sup = torch.full((px + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    stats = torch.full((n, 10), -7, dtype=torch.int64, device=DEV)
    rc = lib.nbc_vote_summary(wt.data_ptr(), n, h, w, draws, lab.data_ptr() if want_labels else None,
                              sup.data_ptr() if want_support else None, stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.NBC_OK, _lib.last_error()
    lab, sup = lab.cpu().numpy(), sup.cpu().numpy()
    assert (lab[px:] == 0xAB).all() and (sup[px:] == 0xAB).all()
    return lab[:px].reshape(n, h, w), sup[:px].reshape(n, h, w), stats.cpu().numpy()


@pytest.mark.parametrize("draws", [1, 4, 1024])
@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 31, 45), (2, 129, 65)])
def test_summary_on_crafted_words(built_lib, shape, draws):
    rng = np.random.default_rng(1000 * draws + shape[1])
    n, h, w = shape
    n1 = rng.integers(0, draws + 1, size=shape)
    n2 = (rng.integers(0, draws + 1, size=shape) * (draws - n1)) // max(draws, 1)      # valid: n1 + n2 <= D
    n2[rng.random(shape) < 0.3] = 0
    n1[rng.random(shape) < 0.3] = 0                                                      # unanimous pixels of every class
    full = rng.random(shape) < 0.1
    n1[full], n2[full] = draws, 0
    assert (n1 + n2 <= draws).all()
    words = (n1 | (n2 << 16)).astype(np.uint32)
    flat = words.reshape(n, -1)
    if draws >= 4:                                                                       # planted ties, in every image
        half = draws // 2                                                                # 0 ties 1, 0 ties 2, 1 ties 2, 1 ties 2 below 0
        for k, (a, b) in enumerate([(half, 0), (0, half), (half, half), (half // 2, half // 2)]):
            flat[:, 3 + 5 * k] = a | (b << 16)
    flat[:, 1] = (draws + 1)                                                             # invalid words: in the head, ...
    flat[:, h * w // 2] = draws | (1 << 16)                                              # ... the body ...
    flat[:, -1] = 0xffffffff                                                             # ... and the tail
    words = flat.reshape(shape)
    label, support, _, valid = vo.decode(words, draws)
    want = vo.stats(words, draws)
    assert (want[:, 7] == 3).all() and (~valid).sum() == 3 * n
    for want_labels, want_support, offset in ((True, True, 0), (False, True, 0), (True, False, 0), (False, False, 0), (True, True, 1)):
        lab, sup, st = summary(built_lib, words, draws, want_labels, want_support, offset)
        assert np.array_equal(st, want), (want_labels, want_support, offset)
        assert np.array_equal(lab, label) if want_labels else (lab == 0xAB).all()
        assert np.array_equal(sup, support) if want_support else (sup == 0xAB).all()


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
    m.dropout_votes(4, [ID_A, ID_B], p=0.3, seed=3)
    labels1, counts1 = m.predict_labels(x, small_zones=True)
    assert torch.equal(labels0, labels1) and torch.equal(counts0, counts1)
    m.dropout_votes(2, [ID_A, ID_B])
    after = profiled()
    assert _record_keys(before) == _record_keys(after) and len(before) > 50
    assert "vote" not in " ".join(r["kernel"] + r["name"] for r in after)
    # the published workspace is what it was: the votes live in the caller's words, not in the workspace
    assert m._lib.nbc_dropout_workspace_bytes(2, 128, 192, 3) == 12 * 6 * 16 * 24 + 10 * 6 * 128 * 192      # both multiples of 256

    # call order: NBC_ERR_STATE as nbc_dropout_draws answers it, under this entry point's own prefix
    shape = (2, 128, 192)
    words = torch.zeros(shape, dtype=torch.int32, device=DEV)
    ids = [ID_A, ID_B]

    def call(model, n, h, w, **kw):
        return c_votes(model, (n, h, w), ids[:n], 0, 1, words, 0, per_pass=1, **kw)[0]

    m.lowres_logits(x)
    assert call(m, *shape) == _lib.NBC_OK
    for other in ((1, 128, 192), (2, 128, 200), (2, 136, 192)):
        assert call(m, *other) == _lib.NBC_ERR_STATE, other
        assert _lib.last_error().startswith("nbc_dropout_votes:")
    need = int(m._lib.nbc_dropout_workspace_bytes(2, 128, 192, 1))
    assert call(m, *shape, workspace_bytes=need - 1) == _lib.NBC_ERR_INVALID and _lib.last_error().startswith("nbc_dropout_votes:")
    m.reserve(1, 64, 64)                                                                # the plan has moved on
    assert call(m, *shape) == _lib.NBC_ERR_STATE
    torch.cuda.synchronize()
    fresh = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)                          # no forward yet
    assert call(fresh, *shape) == _lib.NBC_ERR_STATE and _lib.last_error().startswith("nbc_dropout_votes:")
    with pytest.raises(RuntimeError):
        fresh.dropout_votes(1, [ID_A])
    dl = DeepLabV3ResNet50("fp32").load_state_dict(synth.make_state_dict("trained_like", seed=7, arch="deeplabv3_resnet50")).to(DEV)
    dl.lowres_logits(x)
    assert call(dl, *shape) == _lib.NBC_ERR_STATE
    assert _lib.last_error().startswith("nbc_dropout_votes:") and "NBC_ARCH_FCN_RESNET50" in _lib.last_error()
    with pytest.raises(ValueError, match="DeepLabHead's Dropout sits inside ASPP"):
        dl.dropout_votes(1, [ID_A, ID_B])


# the LAYOUT of tests/test_gpu_dropout.py, restated
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
    """The summary's one exception to 'every file is byte-identical': dropout_summary.json gains the "votes" entry the flag
    asks for, so it is compared as a document -- without that entry it is the document of the run without the flag, and the
    file written from it is that run's file byte for byte."""
    D = 4
    roots = {}
    for tag, kw in (("plain", {}), ("draws", dict(dropout_draws=D, dropout_seed=42)),
                    ("votes", dict(dropout_draws=D, dropout_seed=42, dropout_votes=True)),
                    ("votes_b1s4", dict(dropout_draws=D, dropout_seed=42, dropout_votes=True, batch=1, streams=4))):
        roots[tag] = str(tmp_path / tag)
        ckpt = _make_folder(roots[tag], sd_np)
        st = drv.predict_folder(roots[tag], ckpt, precision="fp32", device_index=0, **kw)
        assert st["images_total"] == len(LAYOUT)
    files = {tag: _result_bytes(root) for tag, root in roots.items()}
    assert "results/dropout_votes.csv" not in files["draws"] and len(files["plain"]) == 1 + len(LAYOUT)
    assert not os.path.exists(os.path.join(roots["draws"], "results", "dropout_votes"))
    new = {"results/dropout_votes.csv"} | {"results/%s/%s/%s" % (level, wood, name.replace("bmp", "png"))
                                          for level in ("dropout_votes", "dropout_support") for wood, name, _, _, _ in LAYOUT}
    assert len(new) == 1 + 2 * len(LAYOUT)
    for tag in ("votes", "votes_b1s4"):
        assert set(files[tag]) == set(files["draws"]) | new, tag
        for base in ("plain", "draws"):
            for k, v in files[base].items():
                if k != "results/dropout_summary.json":
                    assert files[tag][k] == v, (tag, base, k)
        doc = json.loads(files[tag]["results/dropout_summary.json"])
        votes_entry = doc.pop("votes")
        assert (json.dumps(doc, indent=2, sort_keys=True) + "\n").encode() == files["draws"]["results/dropout_summary.json"], tag
    assert files["votes_b1s4"] == files["votes"]

    # the CSV and the PNGs: model-level votes, one image at a time under image_id(wood, name)
    root = roots["votes"]
    model = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    images, live = [], 0
    for _, name, wood in drv.list_images(os.path.join(root, "processed")):
        frame = np.asarray(Image.open(os.path.join(root, "processed", "samples", wood, name)).convert("RGB"))
        x = torch.from_numpy(np.ascontiguousarray(frame[None])).to(DEV)
        labels, _ = model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
        _, vlab, sup, stats = model.dropout_votes(D, [folder_run.image_id(wood, name)], p=0.1, seed=42, small_zones=True)
        vlab, sup, stats = vlab.cpu().numpy()[0], sup.cpu().numpy()[0], stats.cpu().numpy()[0]
        changed = int(np.count_nonzero(vlab != labels.cpu().numpy()[0]))
        images.append((name, wood, frame.shape[0], frame.shape[1], stats, changed))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "dropout_votes", wood, name))), drv.label_png(vlab))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "results", "dropout_support", wood, name))), sup)
        assert np.array_equal(drv.label_png(labels.cpu().numpy()[0]), np.asarray(Image.open(os.path.join(root, "results", "outputs", wood, name))))
        live += int(stats[3:6].sum() < frame.shape[0] * frame.shape[1])
    assert live > 0                                                                    # some draws disagree somewhere
    table, summary = folder_run.vote_report(images, D)
    got = list(csv.reader(open(os.path.join(root, "results", "dropout_votes.csv")), delimiter="\t"))
    assert got == table and got[0] == folder_run.VOTE_COLUMNS and len(got) == 1 + len(LAYOUT)
    assert votes_entry == json.loads(json.dumps(summary["means"]))

    # two gloo ranks sharing the GPU, as tests/test_gpu_dropout.py sets them up
    root2 = str(tmp_path / "w2")
    ckpt2 = _make_folder(root2, sd_np)
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import predict\n"
            "dist.init_process_group('gloo')\n"
            "st = predict.predict_folder(%r, %r, precision='fp32', device_index=0, dropout_draws=%d, dropout_seed=42, dropout_votes=True)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, root2, ckpt2, D, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29643", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _result_bytes(root2) == files["votes"]
