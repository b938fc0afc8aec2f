"""The training run's frame on the GPU: nbc_training_frame against training_frame.pad_resize_cpu byte for byte, and
`evaluate --frame training` against the same driver on a folder of frames made on the host -- an identity, so no tolerance."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd import training_frame as tf
from neuralbarkcalculator_amd.postprocess import remove_small_zones

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
GUARD = 64
# (H, W) -> (Ht, Wt): no resample, rows only, columns only, both, p = L - 1 exactly (9 -> 24), then the training's own size
SMALL = [((21, 32), (32, 32)), ((22, 32), (32, 32)), ((32, 21), (32, 32)), ((21, 23), (32, 32)), ((27, 32), (32, 32)),
         ((32, 32), (32, 32)), ((17, 17), (32, 32)), ((13, 24), (24, 24)), ((9, 24), (24, 24))]
LARGE = [((521, 1024), (1024, 1024)), ((733, 1001), (1024, 1024))]


def images_of(h, w, channels, n=3):
    rng = np.random.default_rng(977 * h + 31 * w + channels)
    if channels == 3:
        return rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    return rng.choice(np.array([0, 127, 255], dtype=np.uint8), size=(n, h, w))


_tables = {}


def table_dev(lt):
    """The device table of a resampled axis, from the C call, uploaded once per length."""
    if lt not in _tables:
        _tables[lt] = torch.from_numpy(tf.table_of(*mdl.bilinear_taps(lt + 1, lt))).to(DEV)
    return _tables[lt]


def frame_on_device(lib, imgs, dst, src_off=0, out_off=GUARD, stream=None):
    """nbc_training_frame on ``imgs`` placed ``src_off`` bytes into its buffer, the output ``out_off`` bytes into one filled with
    0xA5.  Returns (frames, the bytes before them, the bytes after them); synchronises unless a stream is given."""
    n, h, w = imgs.shape[:3]
    channels = 3 if imgs.ndim == 4 else 1
    ht, wt = dst
    src = torch.zeros(imgs.size + 8, dtype=torch.uint8, device=DEV)
    src[src_off: src_off + imgs.size] = torch.from_numpy(imgs.reshape(-1)).to(DEV)
    total = n * ht * wt * channels
    out = torch.full((out_off + total + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    rows = table_dev(ht) if tf.frame_geometry(h, ht)[1] != ht else None
    cols = table_dev(wt) if tf.frame_geometry(w, wt)[1] != wt else None
    s = torch.cuda.current_stream(DEV) if stream is None else stream
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(DEV))
    _lib.check(lib.nbc_training_frame(src.data_ptr() + src_off, channels, n, h, w, ht, wt, rows.data_ptr() if rows is not None else None,
                                      cols.data_ptr() if cols is not None else None, out.data_ptr() + out_off, s.cuda_stream),
               "nbc_training_frame")
    if stream is not None:
        return out, src, (out_off, total)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return got[out_off: out_off + total].reshape((n, ht, wt) + ((3,) if channels == 3 else ())), got[:out_off], got[out_off + total:]


def check_shape(lib, src, dst, channels, placements):
    imgs = images_of(*src, channels)
    want = np.stack([tf.pad_resize_cpu(im, *dst) for im in imgs])      # once for every placement
    for n in (1, 3):
        for src_off, out_off in placements:
            got, before, after = frame_on_device(lib, imgs[:n], dst, src_off, out_off)
            assert (before == 0xA5).all() and (after == 0xA5).all(), (n, src_off, out_off)
            np.testing.assert_array_equal(got, want[:n], err_msg=str((n, src_off, out_off)))


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("src,dst", SMALL)
def test_device_frame_is_pad_resize_cpu(built_lib, src, dst, channels):
    """Source at byte offsets 0 and 1, output at every residue of a dword (the lone bytes before and after the aligned dwords),
    guard bytes on both sides untouched."""
    check_shape(built_lib, src, dst, channels, [(0, GUARD), (1, GUARD), (0, GUARD + 1), (1, GUARD + 2), (1, GUARD + 3)])


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("src,dst", LARGE)
def test_device_frame_at_the_trainings_size(built_lib, src, dst, channels):
    check_shape(built_lib, src, dst, channels, [(0, GUARD), (1, GUARD + 3)])


@pytest.mark.parametrize("channels", [3, 1])
def test_an_images_bytes_do_not_depend_on_batch_or_stream(built_lib, channels):
    src, dst = (21, 23), (32, 32)
    imgs = images_of(*src, channels)
    alone = [frame_on_device(built_lib, imgs[i: i + 1], dst)[0][0] for i in range(3)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 1, 0]):
        got = frame_on_device(built_lib, imgs[order], dst)[0]
        for pos, i in enumerate(order):
            assert got[pos].tobytes() == alone[i].tobytes(), (order, pos)
    # two streams at once, each with its own batch
    big = images_of(521, 1024, channels)
    want = frame_on_device(built_lib, big, (1024, 1024))[0]
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    a = frame_on_device(built_lib, big[:2], (1024, 1024), stream=s1)
    b = frame_on_device(built_lib, big[1:], (1024, 1024), 1, GUARD + 1, stream=s2)
    torch.cuda.synchronize()
    for (out, _, (off, total)), ref in ((a, want[:2]), (b, want[1:])):
        assert out.cpu().numpy()[off: off + total].tobytes() == ref.tobytes()


@pytest.fixture(scope="module")
def model32(sd_np, built_lib):
    return mdl.FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)


def test_model_training_frame_caches_its_tables_and_validates(model32):
    m = model32
    rgb, grey = images_of(21, 23, 3), images_of(21, 23, 1)
    out = m.training_frame(torch.from_numpy(rgb).to(DEV), (32, 32))
    assert out.shape == (3, 32, 32, 3) and out.dtype == torch.uint8 and out.device == DEV
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([tf.pad_resize_cpu(im, 32, 32) for im in rgb]))
    assert sorted(m._frame_taps) == [32]
    ptr = m._frame_taps[32].data_ptr()
    out = m.training_frame(torch.from_numpy(grey).to(DEV), (32, 32))
    assert out.shape == (3, 32, 32)
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([tf.pad_resize_cpu(im, 32, 32) for im in grey]))
    assert sorted(m._frame_taps) == [32] and m._frame_taps[32].data_ptr() == ptr           # reused, not rebuilt
    out = m.training_frame(torch.from_numpy(images_of(13, 24, 3)).to(DEV), (24, 32))         # rows 13 -> 25 -> 24; columns 24 -> 32, a pure map
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([tf.pad_resize_cpu(im, 24, 32) for im in images_of(13, 24, 3)]))
    assert sorted(m._frame_taps) == [24, 32] and m._frame_taps[32].data_ptr() == ptr
    m.training_frame(torch.from_numpy(images_of(22, 32, 3)).to(DEV), (32, 32))               # no axis resampled: no table
    assert sorted(m._frame_taps) == [24, 32]
    # a view that is not contiguous is framed like its copy
    wide = torch.from_numpy(images_of(21, 32, 3)).to(DEV)
    np.testing.assert_array_equal(m.training_frame(wide[:, :, :23], (32, 32)).cpu().numpy(),
                                  m.training_frame(wide[:, :, :23].contiguous(), (32, 32)).cpu().numpy())
    x = torch.from_numpy(rgb).to(DEV)
    for bad in (x.float(), x.cpu(), x[0, 0], x[..., :2], x[:0], x.to(torch.int64)):
        with pytest.raises(ValueError, match="uint8"):
            m.training_frame(bad, (32, 32))
    for size in ((16, 32), (32, 72), (32,), "ab", (0, 32)):                                    # shrinks / p > L - 1 / no pair
        with pytest.raises(ValueError):
            m.training_frame(x, size)


# ---- end to end ------------------------------------------------------------------------------------------------------------
T = 160
# rows 96..159, columns 128..160, odd and even deficits on both axes; one scan whose pad one reflection does not reach
LAYOUT = [("epinette_gelee", "a01.png", 170, 96, 128), ("epinette_gelee", "a02.png", 171, 97, 129), ("epinette_gelee", "a03.png", 172, 159, 160),
          ("epinette_non_gelee", "n1.png", 173, 120, 145), ("sapin", "s0_small.png", 174, 40, 160), ("sapin", "s1.png", 175, 131, 160),
          ("sapin", "s2.png", 176, 158, 128)]
SMALL_SCAN = "sapin/s0_small.png"


def _dual(idx, h, w):
    """A blocky class map as grey levels over all three decode bands."""
    rng = np.random.default_rng(idx)
    cls = np.kron(rng.integers(0, 3, size=((h + 15) // 16, (w + 15) // 16)), np.ones((16, 16), dtype=np.int64))[:h, :w]
    grey = np.array([[0, 63], [64, 191], [192, 255]])[cls]
    return (grey[..., 0] + (rng.random((h, w)) * (grey[..., 1] - grey[..., 0] + 1)).astype(np.int64)).astype(np.uint8)


@pytest.fixture(scope="module")
def folders(tmp_path_factory, sd_np):
    """Folder A: the scans and their duals.  Folder A': pad_resize_cpu of every sample and dual of A that the frame serves, as
    PNG.  Returns (A, A', checkpoint, {(wood, name): (frame of the sample, frame of the dual)})."""
    a, b = str(tmp_path_factory.mktemp("scans")), str(tmp_path_factory.mktemp("frames"))
    framed = {}
    for wood, name, idx, h, w in LAYOUT:
        img, grey = synth.make_frame(idx, h, w), _dual(idx, h, w)
        for root in (a, b):
            os.makedirs(os.path.join(root, "samples", wood), exist_ok=True)
            os.makedirs(os.path.join(root, "duals", wood), exist_ok=True)
        Image.fromarray(img, mode="RGB").save(os.path.join(a, "samples", wood, name))
        Image.fromarray(grey, mode="L").save(os.path.join(a, "duals", wood, name))
        if wood + "/" + name == SMALL_SCAN:
            continue
        framed[(wood, name)] = (tf.pad_resize_cpu(img, T, T), tf.pad_resize_cpu(grey, T, T))
        Image.fromarray(framed[(wood, name)][0], mode="RGB").save(os.path.join(b, "samples", wood, name))
        Image.fromarray(framed[(wood, name)][1], mode="L").save(os.path.join(b, "duals", wood, name))
    ckpt = os.path.join(a, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    return a, b, ckpt, framed


def _csv_bytes(root):
    return open(os.path.join(root, ev.STATS_CSV), "rb").read()


def _summary(root):
    return json.load(open(os.path.join(root, ev.SUMMARY_JSON)))


def _identity(folders, precision, **kw):
    a, b, ckpt, framed = folders
    st = ev.evaluate_folder(a, ckpt, precision=precision, device_index=0, frame="training", frame_size=T, **kw)
    ev.evaluate_folder(b, ckpt, precision=precision, device_index=0, **kw)
    got, want = _csv_bytes(a), _csv_bytes(b)
    assert got == want and len(got.splitlines()) == 1 + len(framed)
    return st


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_evaluate_on_the_frame_is_evaluate_on_a_folder_of_frames(folders, precision):
    a, b, ckpt, framed = folders
    st = _identity(folders, precision, loss=True, ce=True)
    header = list(csv.reader(open(os.path.join(a, ev.STATS_CSV)), delimiter="\t"))[0]
    assert header == ev.csv_header(loss=True, ce=True)
    assert st["images_total"] == len(LAYOUT) and st["images_evaluated_this_rank"] == len(framed)
    summary = _summary(a)
    assert summary["skipped"] == {"no_dual": [], "shape_mismatch": [], "too_large": [], "too_small": [SMALL_SCAN]}
    fr = summary["frame"]
    # padded lengths of T + 1: rows of 97, 159, 131; columns of 129, 145
    assert (fr["kind"], fr["size"], fr["resampled_rows"], fr["resampled_cols"], fr["pool"]) == ("training", T, 3, 2, 8)
    ok = [r for r in st["rows"] if r[3] == ev.STATUS_OK]
    assert [(r[1], r[2]) for r in ok] == [(h, w) for wd, nm, _, h, w in LAYOUT if wd + "/" + nm != SMALL_SCAN]   # the scan's H, W
    assert all(sum(r[4:13]) == T * T and sum(r[13:22]) == T * T for r in ok)                                   # the frame's pixels
    whole = _summary(b)
    for key in ("pooled", "column_means", "lovasz_softmax", "cross_entropy", "images_evaluated"):
        assert summary[key] == whole[key], key
    assert "frame" not in whole and sorted(whole["skipped"]) == ["no_dual", "shape_mismatch", "too_large"]


def test_the_frame_comes_before_the_windows_and_the_flips(folders):
    _identity(folders, "f16x2", windows=64)
    assert _summary(folders[0])["windows"] == {"window": 64, "stride": 32, "blend": "tent"}
    _identity(folders, "f16x2", tta="flips")
    assert _summary(folders[0])["tta"]["views"] == _summary(folders[1])["tta"]["views"]


def test_pooled_figures_from_the_rows_from_the_labels_and_from_two_ranks(folders, sd_np, tmp_path):
    a, _, ckpt, framed = folders
    st = ev.evaluate_folder(a, ckpt, precision="f16x2", device_index=0, frame="training", frame_size=T, pool=4)
    fr = _summary(a)["frame"]
    ok = [r for r in st["rows"] if r[3] == ev.STATUS_OK]
    want = metrics.pooled_over_groups([r[4:13] for r in ok], [r[13:22] for r in ok], 4)
    assert [g["images"] for g in want["groups"]] == [4, 2]                                   # the last group is short
    assert {k: fr[k] for k in want} == json.loads(json.dumps(want))
    # the same figures from label maps: the model on the host's frames, counted on the host
    m = mdl.FCNResNet50("f16x2").load_state_dict(sd_np).to(DEV)
    raw, clean = [], []
    for wood, name, *_ in LAYOUT:
        if (wood, name) not in framed:
            continue
        frame, grey = framed[(wood, name)]
        lab = m.predict_labels(torch.from_numpy(frame[None]).to(DEV), labels_dtype=torch.uint8)[0][0].cpu().numpy()
        t = metrics.target_classes(grey)
        raw.append(metrics.confusion_numpy(lab, t))
        clean.append(metrics.confusion_numpy(remove_small_zones(lab), t))
    again = metrics.pooled_over_groups(raw, clean, 4)
    assert (again["miou"], again["pixelwise_f1"]) == (fr["miou"], fr["pixelwise_f1"]) and json.loads(json.dumps(again["groups"])) == fr["groups"]
    # two ranks (gloo) sharing the GPU: the same files
    one_csv, one_summary = _csv_bytes(a), _summary(a)
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import evaluate\n"
            "dist.init_process_group('gloo')\n"
            "st = evaluate.evaluate_folder(%r, %r, precision='f16x2', device_index=0, frame='training', frame_size=%d, pool=4)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, a, ckpt, T, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29689", str(script)], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _csv_bytes(a) == one_csv and _summary(a) == one_summary


def test_subset_orders_the_groups(folders, tmp_path):
    a, _, ckpt, framed = folders
    names = [wd + "/" + nm for wd, nm, *_ in LAYOUT]
    picked = [names[6], names[4], names[0], names[3]]                                          # one of them the too_small scan
    path = tmp_path / "split.txt"
    path.write_text("\n".join(picked) + "\n")
    st = ev.evaluate_folder(a, ckpt, precision="f16x2", device_index=0, frame="training", frame_size=T, pool=2, subset=str(path))
    rows = list(csv.reader(open(os.path.join(a, ev.STATS_CSV)), delimiter="\t"))[1:]
    assert [r[1] + "/" + r[0] for r in rows] == [picked[0], picked[2], picked[3]] and st["images_total"] == 4
    fr = _summary(a)["frame"]
    assert [g["images"] for g in fr["groups"]] == [2, 1] and _summary(a)["skipped"]["too_small"] == [SMALL_SCAN]
    ok = [r for r in st["rows"] if r[3] == ev.STATUS_OK]
    assert fr["groups"][0]["miou"] == metrics.pooled_miou([r[4:13] for r in ok[:2]])


def test_without_the_flag_nothing_changes(folders):
    """The flag's default against no flag at all, within the run: the same bytes in both files, no "frame" entry, the three
    reasons."""
    _, a, ckpt, framed = folders
    ev.evaluate_folder(a, ckpt, precision="f16x2", device_index=0, loss=True)
    plain = (_csv_bytes(a), open(os.path.join(a, ev.SUMMARY_JSON), "rb").read())
    ev.evaluate_folder(a, ckpt, precision="f16x2", device_index=0, loss=True, frame="scan", frame_size=None, pool=None, subset=None)
    assert (_csv_bytes(a), open(os.path.join(a, ev.SUMMARY_JSON), "rb").read()) == plain
    summary = _summary(a)
    assert "frame" not in summary and sorted(summary["skipped"]) == ["no_dual", "shape_mismatch", "too_large"]
    assert summary["images_evaluated"] == len(framed)
