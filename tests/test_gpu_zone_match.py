"""Output zones against target zones on the GPU (csrc/zone_match.hip, nbc_match_zones, FCNResNet50.match_zones, evaluate --zones)
against the host restatement zones.match_cpu (scipy.ndimage.label per class, a zone-index plane per map, numpy.unique on the
joined key; itself pinned by the hand-written answers of test_zone_match_abi.py).  Integer work: every comparison is exact."""
import csv
import json
import os
import shutil

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib, synth, zones
from neuralbarkcalculator_amd.model import FCNResNet50

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x5A5A5A5A5A5A5A5A
BANDS = ((0, 63), (64, 191), (192, 255))             # the grey levels of each target class


@pytest.fixture(scope="module")
def model(built_lib, sd_np):
    return FCNResNet50("bf16").load_state_dict(sd_np).to(DEV)


def grey_of(classes, seed=0):
    """A grey dual whose classes are ``classes``, its levels spread over the whole band of each class."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([b[0] for b in BANDS])[classes], np.array([b[1] for b in BANDS])[classes]
    grey = (lo + (rng.random(classes.shape) * (hi - lo + 1)).astype(np.int64)).astype(np.uint8)
    assert np.array_equal(zones.target_classes(grey), classes)
    return grey


def run_with_sentinel(model, labels_np, target_classes_np, dtype=torch.uint8, cap=1024, pair_cap=2048, grey_seed=0):
    """The C entry point on buffers filled with a sentinel; labels and target must come back untouched.  Returns numpy
    (out_rows, out_num, tgt_rows, tgt_num, pair_rows, pair_num)."""
    lab = torch.from_numpy(np.ascontiguousarray(labels_np)).to(dtype).to(DEV)
    grey = torch.from_numpy(grey_of(np.ascontiguousarray(target_classes_np), grey_seed)).to(DEV)
    lab0, grey0 = lab.clone(), grey.clone()
    n, h, w = lab.shape
    rows = [torch.full((n, cap, zones.ZONE_ROW), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(2)]
    pairs = torch.full((n, pair_cap, zones.PAIR_ROW), SENTINEL, dtype=torch.int64, device=DEV)
    nums = [torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3)]
    need = int(model._lib.nbc_zone_match_workspace_bytes(n, h, w, pair_cap))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    cur = torch.cuda.current_stream(DEV)
    rc = model._lib.nbc_match_zones(model._ctx, lab.data_ptr(), _lib.LABEL_I64 if dtype == torch.int64 else _lib.LABEL_U8,
                                    grey.data_ptr(), n, h, w, rows[0].data_ptr(), nums[0].data_ptr(), rows[1].data_ptr(),
                                    nums[1].data_ptr(), cap, pairs.data_ptr(), nums[2].data_ptr(), pair_cap, ws.data_ptr(), need,
                                    cur.cuda_stream)
    _lib.check(rc, "nbc_match_zones")
    torch.cuda.synchronize()
    assert torch.equal(lab, lab0) and torch.equal(grey, grey0)      # read only
    return (rows[0].cpu().numpy(), nums[0].cpu().numpy(), rows[1].cpu().numpy(), nums[1].cpu().numpy(), pairs.cpu().numpy(),
            nums[2].cpu().numpy())


def assert_equal_oracle(got, want, cap, pair_cap, what="", sentinel=True):
    """``got`` of run_with_sentinel against ``want`` of zones.match_cpu: both inventories as nbc_label_zones truncates them, the
    pair rows complete and in order, and (``sentinel``) nothing written behind an image's last row."""
    o_rows, o_num, t_rows, t_num, p_rows, p_num = got
    for i, (wo, wt, wp) in enumerate(want):
        for name, rows, num, w in (("output", o_rows, o_num, wo), ("target", t_rows, t_num, wt)):
            assert int(num[i]) == len(w), f"{what} image {i}: {int(num[i])} {name} zones, the oracle has {len(w)}"
            k = min(len(w), cap)
            assert np.array_equal(rows[i, :k], w[:k]), f"{what} image {i}: {name} zone rows differ"
            if sentinel:
                assert (rows[i, k:] == SENTINEL).all(), f"{what} image {i}: a row behind the {name} zones was written"
        assert len(wp) <= pair_cap, f"{what} image {i}: the test's pair_cap {pair_cap} is below the oracle's {len(wp)} pairs"
        assert int(p_num[i]) == len(wp), f"{what} image {i}: {int(p_num[i])} pairs, the oracle has {len(wp)}"
        if not np.array_equal(p_rows[i, :len(wp)], wp):
            bad = np.flatnonzero((p_rows[i, :len(wp)] != wp).any(axis=1))
            raise AssertionError(f"{what} image {i}: {len(bad)} of {len(wp)} pair rows differ, first {bad[0]}: got "
                                 f"{p_rows[i, bad[0]].tolist()}, want {wp[bad[0]].tolist()}")
        if sentinel:
            assert (p_rows[i, len(wp):] == SENTINEL).all(), f"{what} image {i}: a row behind the pairs was written"


def caps_of(want):
    return (max(1, max(max(len(o), len(t)) for o, t, _ in want)), max(1, max(len(p) for _, _, p in want)))


def blobs(seed, n, h, w, p_bg, smooth):
    """Random class maps with zones of every size: thresholded smoothed noise plus salt (tests/test_gpu_zones.py's generator)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, h, w))
    for _ in range(smooth):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5.0
    q = np.quantile(f, [p_bg, p_bg + (1 - p_bg) * 0.6])
    lab = np.where(f < q[0], 0, np.where(f < q[1], 1, 2)).astype(np.uint8)
    salt = rng.random((n, h, w)) < 0.01
    lab[salt] = rng.integers(0, 3, size=int(salt.sum()), dtype=np.uint8)
    return lab


def perturbed(seed, target, flip, roll=False):
    """The target with a share ``flip`` of its pixels redrawn uniformly from {0, 1, 2}; ``roll``: also moved by (1, 2) pixels."""
    rng = np.random.default_rng(seed)
    out = target.copy()
    m = rng.random(target.shape) < flip
    out[m] = rng.integers(0, 3, size=int(m.sum()), dtype=np.uint8)
    return np.roll(out, (1, 2), axis=(-2, -1)) if roll else out


def totals(want, key):
    figs = [zones.match_figures(*w) for w in want]
    return sum(f[c][key] for f in figs for c in ("Bark", "Node"))


RANDOM_CASES = [((3, 200, 333), 0.5, 3, 0.02), ((2, 33, 95), 0.3, 1, 0.05), ((1, 31, 31), 0.5, 0, 0.1), ((2, 97, 130), 0.5, 1, 0.02),
                ((1, 520, 1024), 0.1, 8, 0.002), ((1, 64, 1), 0.5, 0, 0.1), ((1, 1, 64), 0.5, 0, 0.1)]
_oracle_cache = {}


def random_case(shape, p_bg, smooth, flip, roll):
    """(output, target, match_cpu of them), computed once per case and shared by the two label dtypes."""
    key = (shape, roll)
    if key not in _oracle_cache:
        n, h, w = shape
        tgt = blobs(sum(shape), n, h, w, p_bg, smooth)
        out = perturbed(1000 + sum(shape), tgt, flip, roll)
        _oracle_cache[key] = (out, tgt, zones.match_cpu(out, tgt))
    return _oracle_cache[key]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("shape,p_bg,smooth,flip", RANDOM_CASES)
def test_random_maps_equal_cpu_restatement(model, shape, p_bg, smooth, flip, dtype):
    out, tgt, want = random_case(shape, p_bg, smooth, flip, False)
    assert totals(want, "matched") >= 1
    if shape in [c[0] for c in RANDOM_CASES[:4]]:
        assert totals(want, "split_targets") >= 1 and totals(want, "merged_outputs") >= 1
    cap, pair_cap = caps_of(want)
    assert_equal_oracle(run_with_sentinel(model, out, tgt, dtype, cap, pair_cap), want, cap, pair_cap, str(shape))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("shape,p_bg,smooth,flip", RANDOM_CASES)
def test_rolled_random_maps_equal_cpu_restatement(model, shape, p_bg, smooth, flip, dtype):
    """The output also moved by (1, 2) pixels: few matches, many partial overlaps."""
    out, tgt, want = random_case(shape, p_bg, smooth, flip, True)
    assert sum(len(p) for _, _, p in want) >= 1
    if shape in [c[0] for c in RANDOM_CASES[:4]]:
        assert totals(want, "split_targets") >= 1 and totals(want, "merged_outputs") >= 1
        assert totals(want, "matched") < totals(want, "targets") // 2
    cap, pair_cap = caps_of(want)
    assert_equal_oracle(run_with_sentinel(model, out, tgt, dtype, cap, pair_cap), want, cap, pair_cap, str(shape))


def stripes():
    out, tgt = np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8)
    out[:, ::2] = 2                                                # vertical one-pixel stripes on the even columns
    tgt[::2, :] = 2                                                # horizontal ones on the even rows
    return out, tgt


def test_stripes_at_and_below_the_pair_cap(model):
    """32 x 32 zones and 1 024 one-pixel pairs: all of them in order at pair_cap 1024; at 1023 the image reports exactly 1024,
    its neighbours in the batch are unaffected and nothing is written behind any image's rows."""
    s_out, s_tgt = stripes()
    want1 = zones.match_cpu(s_out, s_tgt)
    assert len(want1[0][0]) == 32 and len(want1[0][1]) == 32
    assert want1[0][2].tolist() == [[i, j, 1] for i in range(32) for j in range(32)]
    got = run_with_sentinel(model, s_out[None], s_tgt[None], cap=32, pair_cap=1024)
    assert_equal_oracle(got, want1, 32, 1024, "stripes")

    side = blobs(9, 2, 64, 64, 0.5, 2)
    out = np.stack([side[0], s_out, side[1]])
    tgt = np.stack([perturbed(3, side[0], 0.03), s_tgt, perturbed(4, side[1], 0.03)])
    want = zones.match_cpu(out, tgt)
    assert 0 < len(want[0][2]) < 1023 and 0 < len(want[2][2]) < 1023
    cap = caps_of(want)[0]
    got = run_with_sentinel(model, out, tgt, cap=cap, pair_cap=1023)
    assert got[5].tolist() == [len(want[0][2]), 1024, len(want[2][2])]
    for i in (0, 2):
        assert np.array_equal(got[4][i, :len(want[i][2])], want[i][2]) and (got[4][i, len(want[i][2]):] == SENTINEL).all()
    for i in range(3):                                             # the zone inventories do not depend on the pair cap
        assert got[1][i] == len(want[i][0]) and np.array_equal(got[0][i, :len(want[i][0])], want[i][0])
        assert got[3][i] == len(want[i][1]) and np.array_equal(got[2][i, :len(want[i][1])], want[i][1])

    # one image at a time into a buffer with three sentinel rows behind each image's pair_cap rows
    pair_cap, alloc = 1023, 1026
    buf = torch.full((3 * alloc, zones.PAIR_ROW), SENTINEL, dtype=torch.int64, device=DEV)
    num = torch.full((3, 3), SENTINEL, dtype=torch.int64, device=DEV)
    zr = torch.empty((2, cap, zones.ZONE_ROW), dtype=torch.int64, device=DEV)
    need = int(model._lib.nbc_zone_match_workspace_bytes(1, 64, 64, pair_cap))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lab, grey = torch.from_numpy(out).to(DEV), torch.from_numpy(grey_of(tgt)).to(DEV)
    for i in range(3):
        rc = model._lib.nbc_match_zones(model._ctx, lab[i].data_ptr(), _lib.LABEL_U8, grey[i].data_ptr(), 1, 64, 64, zr[0].data_ptr(),
                                        num[i, 0:].data_ptr(), zr[1].data_ptr(), num[i, 1:].data_ptr(), cap, buf[i * alloc:].data_ptr(),
                                        num[i, 2:].data_ptr(), pair_cap, ws.data_ptr(), need, torch.cuda.current_stream(DEV).cuda_stream)
        _lib.check(rc, "nbc_match_zones")
    torch.cuda.synchronize()
    rows = buf.cpu().numpy().reshape(3, alloc, zones.PAIR_ROW)
    assert num[:, 2].tolist() == [len(want[0][2]), 1024, len(want[2][2])]
    for i in range(3):
        assert (rows[i, pair_cap:] == SENTINEL).all(), i
        if i != 1:
            assert np.array_equal(rows[i, :len(want[i][2])], want[i][2]) and (rows[i, len(want[i][2]):] == SENTINEL).all()


@pytest.mark.parametrize("h,w", [(64, 64), (33, 65)])
def test_the_tile_hash_at_its_bound(model, h, w):
    """Rows alternating 1, 2, 1, 2, ... between zero rows, matched against itself: every pixel is a zone of its own and a pair of
    its own, 512 pairs in every full 32 x 32 tile -- the most that can meet one."""
    m = np.zeros((h, w), np.uint8)
    m[::2, :] = 1 + (np.arange(w) % 2)
    want = zones.match_cpu(m, m)
    k = ((h + 1) // 2) * w
    assert len(want[0][0]) == k and want[0][2].tolist() == [[i, i, 1] for i in range(k)]
    for dtype in (torch.uint8, torch.int64):
        assert_equal_oracle(run_with_sentinel(model, m[None], m[None], dtype, cap=k, pair_cap=zones.PAIRS_MAX_CAP), want, k,
                            zones.PAIRS_MAX_CAP, f"{h}x{w}")


def worst_cases():
    h = w = 256
    spiral = np.zeros((h, w), np.uint8)
    y0, x0, y1, x1 = 0, 0, h - 1, w - 1
    while y0 <= y1 and x0 <= x1:
        spiral[y0, x0:x1 + 1] = 1; spiral[y0:y1 + 1, x1] = 1
        if y1 > y0: spiral[y1, x0 + 2:x1 + 1] = 1
        if x1 > x0 + 2: spiral[y0 + 2:y1 + 1, x0 + 2] = 1
        y0 += 2; x0 += 2; y1 -= 2; x1 -= 2
    comb = np.zeros((h, w), np.uint8); comb[:, ::2] = 2; comb[0, :] = 2
    yy, xx = np.mgrid[0:h, 0:w]
    checker = ((yy + xx) % 2 + 1).astype(np.uint8)
    return {"spiral": spiral, "comb": comb, "checker": checker, "zeros": np.zeros((h, w), np.uint8)}


def test_worst_case_shapes_against_each_other(model):
    cases = worst_cases()
    names = ["checker", "comb", "spiral"]
    out = np.stack([cases[a] for a in names for b in names] + [cases["zeros"], cases["checker"], cases["zeros"]])
    tgt = np.stack([cases[b] for a in names for b in names] + [cases["checker"], cases["zeros"], cases["zeros"]])
    want = zones.match_cpu(out, tgt)
    assert want[0][2].tolist() == [[0, 0, 32768], [1, 1, 32768]]   # the checker against itself
    # the checker's nodes (y + x odd) on the comb: the even columns of the 128 odd rows, and the 128 odd columns of row 0
    assert want[1][2].tolist() == [[1, 0, 128 * 128 + 128]]
    assert all(len(want[i][2]) == 0 for i in (5, 7, 9, 10, 11))    # comb x spiral share no class; all-zero against anything
    cap, pair_cap = caps_of(want)
    assert_equal_oracle(run_with_sentinel(model, out, tgt, cap=cap, pair_cap=pair_cap), want, cap, pair_cap, "worst cases")
    swapped = np.where(out == 0, 0, 3 - out).astype(np.uint8)      # the classes swapped on the output side
    want = zones.match_cpu(swapped, tgt)
    cap, pair_cap = caps_of(want)
    assert_equal_oracle(run_with_sentinel(model, swapped, tgt, torch.int64, cap, pair_cap), want, cap, pair_cap, "swapped")


def test_zone_cap_below_the_zone_counts(model):
    """The pair rows are complete (their indices run past cap), the zone rows truncated as nbc_label_zones truncates them."""
    tgt = blobs(11, 3, 97, 130, 0.5, 1)
    out = perturbed(12, tgt, 0.03)
    want = zones.match_cpu(out, tgt)
    cap = min(min(len(o), len(t)) for o, t, _ in want) // 2
    assert cap >= 4 and all(p[:, 0].max() >= cap and p[:, 1].max() >= cap for _, _, p in want)
    pair_cap = caps_of(want)[1]
    for dtype in (torch.uint8, torch.int64):
        got = run_with_sentinel(model, out, tgt, dtype, cap, pair_cap)
        assert_equal_oracle(got, want, cap, pair_cap, "cap %d" % cap)
        lab = torch.from_numpy(out).to(dtype).to(DEV)
        rows, num = model.label_zones(lab, cap=cap)                # the very rows of nbc_label_zones
        assert np.array_equal(rows.cpu().numpy(), got[0]) and np.array_equal(num.cpu().numpy(), got[1])


def test_many_random_small_maps(model):
    """300 random pairs of maps around the 32-pixel tile grid (test_gpu_zones.py's sizes and densities): independent maps,
    perturbed copies and shifted copies."""
    rng = np.random.default_rng(2026)
    for k in range(300):
        h = int(rng.integers(1, 100)); w = int(rng.integers(1, 100))
        if k % 3 == 0:
            h, w = int(rng.choice([31, 32, 33, 63, 64, 65, 96])), int(rng.choice([31, 32, 33, 63, 64, 65, 96]))
        dens = float(rng.choice([0.0, 0.1, 0.3, 0.41, 0.5, 0.7, 0.9]))
        tgt = np.where(rng.random((h, w)) < dens, 0, rng.integers(1, 3, size=(h, w))).astype(np.uint8)
        if k % 5 == 0:
            tgt = np.minimum(tgt, 1)
        if k % 4 == 0:
            out = np.where(rng.random((h, w)) < dens, 0, rng.integers(1, 3, size=(h, w))).astype(np.uint8)
        else:
            out = perturbed(k, tgt, 0.05, roll=k % 4 == 1)
        want = zones.match_cpu(out, tgt)
        cap, pair_cap = caps_of(want)
        if pair_cap > zones.PAIRS_MAX_CAP:
            continue
        got = run_with_sentinel(model, out[None], tgt[None], torch.int64 if k % 2 else torch.uint8, cap, pair_cap, grey_seed=k)
        assert_equal_oracle(got, want, cap, pair_cap, f"case {k}: {h}x{w} density {dens}")


def test_a_batch_of_100_maps(model):
    rng = np.random.default_rng(17)
    tgt = (rng.random((100, 48, 80)) < 0.45).astype(np.uint8) * rng.integers(1, 3, size=(100, 48, 80)).astype(np.uint8)
    out = perturbed(18, tgt, 0.05)
    want = zones.match_cpu(out, tgt)
    cap, pair_cap = caps_of(want)
    assert_equal_oracle(run_with_sentinel(model, out, tgt, cap=cap, pair_cap=pair_cap), want, cap, pair_cap)


def test_determinism_and_batch_independence(model):
    tgt = blobs(23, 3, 150, 201, 0.4, 2)
    out = perturbed(24, tgt, 0.02)
    want = zones.match_cpu(out, tgt)
    cap, pair_cap = caps_of(want)
    a = run_with_sentinel(model, out, tgt, cap=cap, pair_cap=pair_cap)
    b = run_with_sentinel(model, out, tgt, cap=cap, pair_cap=pair_cap)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    side = torch.cuda.Stream(DEV)
    grey = grey_of(tgt)
    with torch.cuda.stream(side):
        for i in range(3):                                         # alone, on another stream, through the model object
            got = model.match_zones(torch.from_numpy(out[i]).to(DEV), torch.from_numpy(grey[i]).to(DEV), cap=cap, pair_cap=pair_cap)
            side.synchronize()
            got = [g.cpu().numpy() for g in got]
            for j in (0, 2, 4):
                k = int(a[j + 1][i])
                assert int(got[j + 1][0]) == k and got[j][0, :k].tobytes() == a[j][i, :k].tobytes()
    assert_equal_oracle(a, want, cap, pair_cap)


def test_model_object_checks(model):
    lab = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    for bad in (dict(cap=0), dict(pair_cap=0), dict(pair_cap=zones.PAIRS_MAX_CAP + 1)):
        with pytest.raises(ValueError):
            model.match_zones(lab, lab, **bad)
    with pytest.raises(ValueError):
        model.match_zones(lab, lab[:1])
    with pytest.raises(ValueError):
        model.match_zones(lab, lab.to(torch.int64))
    with pytest.raises(ValueError):
        model.match_zones(lab.float(), lab)
    got = model.match_zones(lab, lab)
    assert [tuple(g.shape) for g in got] == [(2, 1024, 10), (2,), (2, 1024, 10), (2,), (2, 2048, 3), (2,)]
    assert all(int(g.sum()) == 0 for g in got[1::2])


def test_on_network_labels(model):
    x = torch.from_numpy(np.stack([synth.make_input(60 + k, 512, 512) for k in range(2)])).to(DEV)
    labels, _ = model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)
    lab = labels.cpu().numpy()
    tgt = perturbed(61, lab, 0.001)
    got = model.match_zones(labels, torch.from_numpy(grey_of(tgt)).to(DEV), cap=4096, pair_cap=zones.PAIRS_MAX_CAP)
    torch.cuda.synchronize()
    want = zones.match_cpu(lab, tgt)
    assert totals(want, "matched") >= 1
    assert_equal_oracle([g.cpu().numpy() for g in got], want, 4096, zones.PAIRS_MAX_CAP, "network labels", sentinel=False)


# ---- the folder driver ---------------------------------------------------------------------------------------------------
SIZES = [(256, 256), (256, 256), (200, 256), (256, 256), (200, 256)]
KW = dict(precision="bf16", device_index=0, batch=2, target_size=256, calibrate=False)
FILES = ("zone_matches.csv", "zone_evaluation.csv")


@pytest.fixture(scope="module")
def labelled(built_lib, sd_np, tmp_path_factory):
    """A labelled folder whose samples are the frames a predict run fed the network and whose duals are that run's label PNGs,
    perturbed and spread over the grey bands.  Returns (root, checkpoint, {(wood, name): (labels, grey)})."""
    from PIL import Image
    from neuralbarkcalculator_amd.predict import predict_folder
    base = tmp_path_factory.mktemp("zone_match")
    ckpt = str(base / "ckpt.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    first = str(base / "first")
    wood = "epinette_gelee"
    os.makedirs(os.path.join(first, "samples", wood))
    for k, (h, w) in enumerate(SIZES):
        img = (synth.make_input(300 + k, h, w).transpose(1, 2, 0) * 60 + 128).clip(0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(first, "samples", wood, "z%02d.png" % k))
    predict_folder(first, ckpt, **KW)
    root = str(base / "labelled")
    os.makedirs(os.path.join(root, "samples", wood))
    os.makedirs(os.path.join(root, "duals", wood))
    truth = {}
    for k in range(len(SIZES)):
        name = "z%02d.png" % k
        shutil.copy(os.path.join(first, "processed", "samples", wood, name), os.path.join(root, "samples", wood, name))
        png = np.asarray(Image.open(os.path.join(first, "results", "outputs", wood, name)))
        lab = np.zeros(png.shape, np.uint8)
        lab[png == 127] = 1
        lab[png == 255] = 2
        grey = grey_of(perturbed(400 + k, lab, 0.002), seed=k)
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
        truth[(wood, name)] = lab
    return root, ckpt, truth


def _read(root, name):
    with open(os.path.join(root, "results", name), "rb") as f:
        return f.read()


def _table(root, name):
    return list(csv.reader(open(os.path.join(root, "results", name)), delimiter="\t"))


def _expected(root, truth, iou=0.5):
    """The two tables and the figures as match_cpu and the formatters give them on the label PNGs and the duals on disk."""
    from PIL import Image
    matches, evaluation, figures = [zones.MATCH_COLUMNS], [zones.EVALUATION_COLUMNS], []
    for (wood, name), lab in sorted(truth.items()):
        grey = np.array(Image.open(os.path.join(root, "duals", wood, name)).convert("L"))
        o, t, p = zones.match_cpu(lab, zones.target_classes(grey))[0]
        matches += zones.match_rows(name, wood, o, t, p, iou)
        figures.append(zones.match_figures(o, t, p, iou))
        evaluation += zones.evaluation_rows(name, wood, figures[-1])
    return matches, evaluation, figures


def test_folder_with_and_without_zones(labelled):
    from neuralbarkcalculator_amd import evaluate as ev
    root, ckpt, truth = labelled
    st = ev.evaluate_folder(root, ckpt, **KW)
    assert st["summary"]["images_evaluated"] == len(SIZES) and "zones" not in st["summary"] and "zones_host_fallbacks" not in st
    assert not any(os.path.exists(os.path.join(root, "results", n)) for n in FILES)
    plain_csv, plain_doc = _read(root, "evaluation_stats.csv"), json.load(open(os.path.join(root, ev.SUMMARY_JSON)))

    st = ev.evaluate_folder(root, ckpt, zones=True, **KW)
    assert _read(root, "evaluation_stats.csv") == plain_csv
    doc = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert {k: v for k, v in doc.items() if k != "zones"} == plain_doc and list(doc)[-1] == "zones"
    matches, evaluation, figures = _expected(root, truth)
    assert _table(root, "zone_matches.csv") == matches and _table(root, "zone_evaluation.csv") == evaluation
    assert st["zones_host_fallbacks"] == 0
    want = json.loads(json.dumps(zones.match_summary(figures, 0.5, 1024, 2048, 0)))
    assert doc["zones"] == want and want["Bark"]["matched"] + want["Node"]["matched"] >= 1
    assert len(matches) > 1 + len(SIZES)
    full = {n: _read(root, n) for n in FILES}

    st1 = ev.evaluate_folder(root, ckpt, zones=True, zones_cap=1, zone_pairs_cap=1, **KW)
    assert st1["zones_host_fallbacks"] > 0
    assert {n: _read(root, n) for n in FILES} == full and _read(root, "evaluation_stats.csv") == plain_csv
    doc1 = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))["zones"]
    assert doc1 == dict(want, zones_cap=1, zone_pairs_cap=1, host_fallbacks=st1["zones_host_fallbacks"])

    ev.evaluate_folder(root, ckpt, zones=True, match_iou=0.8, **KW)
    matches8, evaluation8, figures8 = _expected(root, truth, 0.8)
    assert _table(root, "zone_matches.csv") == matches8 and _table(root, "zone_evaluation.csv") == evaluation8
    assert json.load(open(os.path.join(root, ev.SUMMARY_JSON)))["zones"]["match_iou"] == 0.8


def test_folder_on_two_ranks(labelled, tmp_path):
    """Two gloo ranks sharing the GPU (as tests/test_gpu_zones.py sets them up): the ranks hold unequal numbers of rows, rank 0
    writes what match_cpu and the formatters give."""
    import subprocess
    import sys
    from neuralbarkcalculator_amd import evaluate as ev
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root, ckpt, truth = labelled
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import evaluate\n"
            "dist.init_process_group('gloo')\n"
            "st = evaluate.evaluate_folder(%r, %r, precision='bf16', device_index=0, batch=2, target_size=256, calibrate=False, "
            "zones=True)\n"
            "assert st['world'] == 2 and st['images_total'] == %d and st['zones_host_fallbacks'] == 0\n"
            "dist.destroy_process_group()\n" % (repo, root, ckpt, len(SIZES)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    for n in FILES:
        if os.path.exists(os.path.join(root, "results", n)):
            os.remove(os.path.join(root, "results", n))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29679", str(script)],
                       cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    matches, evaluation, figures = _expected(root, truth)
    assert _table(root, "zone_matches.csv") == matches and _table(root, "zone_evaluation.csv") == evaluation
    doc = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))["zones"]
    assert doc == json.loads(json.dumps(zones.match_summary(figures, 0.5, 1024, 2048, 0)))
