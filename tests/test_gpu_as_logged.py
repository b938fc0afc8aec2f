"""`evaluate --frame training --pool B --as_logged` end to end on the GPU: the loss and the PixelWiseF1 of each group as one batch,
against the model-level calls on the group's frames; one rank against two; the files the run writes without the flag."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd import training_frame as tf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
T = 160
# as tests/test_gpu_training_frame.py lays its folder out: odd and even deficits on both axes, one scan the frame cannot serve
LAYOUT = [("epinette_gelee", "a01.png", 270, 96, 128), ("epinette_gelee", "a02.png", 271, 97, 129), ("epinette_gelee", "a03.png", 272, 159, 160),
          ("epinette_non_gelee", "n1.png", 273, 120, 145), ("sapin", "s0_small.png", 274, 40, 160), ("sapin", "s1.png", 275, 131, 160),
          ("sapin", "s2.png", 276, 158, 128)]
SMALL_SCAN = "sapin/s0_small.png"
NAMES = [wd + "/" + nm for wd, nm, *_ in LAYOUT]


def _dual(idx, h, w):
    """A blocky class map as grey levels over all three decode bands; Node only where idx is even."""
    rng = np.random.default_rng(idx)
    cls = np.kron(rng.integers(0, 3 if idx % 2 == 0 else 2, size=((h + 15) // 16, (w + 15) // 16)), np.ones((16, 16), dtype=np.int64))[:h, :w]
    grey = np.array([[0, 63], [64, 191], [192, 255]])[cls]
    return (grey[..., 0] + (rng.random((h, w)) * (grey[..., 1] - grey[..., 0] + 1)).astype(np.int64)).astype(np.uint8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory, sd_np):
    """The scans and their duals, the checkpoint, and {wood/name: (frame of the sample, frame of the dual)} made on the host."""
    root = str(tmp_path_factory.mktemp("as_logged"))
    framed = {}
    for wood, name, idx, h, w in LAYOUT:
        img, grey = synth.make_frame(idx, h, w), _dual(idx, h, w)
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
        if wood + "/" + name != SMALL_SCAN:
            framed[wood + "/" + name] = (tf.pad_resize_cpu(img, T, T), tf.pad_resize_cpu(grey, T, T))
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    return root, ckpt, framed


@pytest.fixture(scope="module")
def model(sd_np, built_lib):
    return mdl.FCNResNet50("f16x2").load_state_dict(sd_np).to(DEV)


def _summary(root):
    return json.load(open(os.path.join(root, ev.SUMMARY_JSON)))


def _files(root):
    return open(os.path.join(root, ev.STATS_CSV), "rb").read(), open(os.path.join(root, ev.SUMMARY_JSON), "rb").read()


def _run(folder, **kw):
    root, ckpt, _ = folder
    return ev.evaluate_folder(root, ckpt, precision="f16x2", device_index=0, frame="training", frame_size=T, **kw)


def from_the_model(m, framed, names, pool):
    """``metrics.as_logged_over_groups`` from the model-level calls on each group's frames, in the order of ``names``."""
    raw, clean, terms, counts, sizes = [], [], [], [], []
    for a in range(0, len(names), pool):
        part = names[a:a + pool]
        x = torch.from_numpy(np.stack([framed[k][0] for k in part])).to(DEV)
        tgt = torch.from_numpy(np.stack([framed[k][1] for k in part])).to(DEV)
        lg = torch.empty((len(part), 3, T, T), dtype=torch.float32, device=DEV)
        labels, _ = m.predict_labels(x, labels_dtype=torch.uint8, logits_full=lg)
        raw.append(m.confusion(labels, tgt).sum(dim=0).cpu().numpy())
        t, c = m.lovasz_softmax_groups(lg, tgt, len(part))
        m.remove_small_zones_groups(labels, len(part))
        clean.append(m.confusion(labels, tgt).sum(dim=0).cpu().numpy())
        terms.append(t[0].cpu().numpy()), counts.append(c[0].cpu().numpy()), sizes.append(len(part))
    return json.loads(json.dumps(metrics.as_logged_over_groups(raw, clean, terms, counts, sizes)))


def test_each_groups_figures_are_the_model_level_calls_on_its_frames(folder, model):
    root, _, framed = folder
    st = _run(folder, pool=4, as_logged=True)
    fr = _summary(root)["frame"]
    al = fr["as_logged"]
    names = [k for k in NAMES if k in framed]
    assert al == from_the_model(model, framed, names, 4)
    assert [g["images"] for g in al["groups"]] == [4, 2] and sorted(al) == ["groups", "loss", "miou", "pixelwise_f1"]
    assert al["miou"] == fr["miou"] and [g["miou"] for g in al["groups"]] == [g["miou"] for g in fr["groups"]]   # today's figure
    assert st["summary"]["frame"]["as_logged"] == al
    assert "as the training logged it" in ev.format_summary(_summary(root))
    assert all(0 < g["loss"] <= 1 for g in al["groups"])


def test_groups_of_one_are_the_per_image_figures(folder):
    root, _, framed = folder
    _run(folder, pool=1, as_logged=True, loss=True)
    summary = _summary(root)
    fr, al = summary["frame"], summary["frame"]["as_logged"]
    rows = list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))[1:]
    assert len(rows) == len(framed) == len(al["groups"])
    assert al["pixelwise_f1"] == fr["pixelwise_f1"] and [g["pixelwise_f1"] for g in al["groups"]] == [g["pixelwise_f1"] for g in fr["groups"]]
    assert [g["loss"] for g in al["groups"]] == [float(r[18]) for r in rows]                    # the cells of --loss, every bit
    assert [g["loss_terms"][k] for g in al["groups"] for k in range(3) if g["present"][k]] == \
        [float(r[15 + k]) for r in rows for k in range(3) if r[15 + k] != ""]
    assert al["loss"] == pytest.approx(summary["lovasz_softmax"]["mean_over_images"], abs=1e-15)


def test_two_ranks_give_the_summary_of_one(folder, tmp_path):
    root, ckpt, _ = folder
    _run(folder, pool=2, as_logged=True)
    one = _files(root)
    assert [g["images"] for g in _summary(root)["frame"]["as_logged"]["groups"]] == [2, 2, 2]
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import evaluate\n"
            "dist.init_process_group('gloo')\n"
            "st = evaluate.evaluate_folder(%r, %r, precision='f16x2', device_index=0, frame='training', frame_size=%d, pool=2, as_logged=True)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "assert 0 < st['images_evaluated_this_rank'] < 6 and st['images_evaluated_this_rank'] %% 2 == 0\n"
            "dist.destroy_process_group()\n" % (REPO, root, ckpt, T, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29697", str(script)], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _files(root) == one                                                                  # float for float: the same bytes


def test_subset_reorders_the_groups(folder, model, tmp_path):
    root, _, framed = folder
    picked = [NAMES[6], NAMES[4], NAMES[0], NAMES[3], NAMES[1]]                                 # one of them the too_small scan
    path = tmp_path / "split.txt"
    path.write_text("\n".join(picked) + "\n")
    _run(folder, pool=2, as_logged=True, subset=str(path))
    al = _summary(root)["frame"]["as_logged"]
    assert [g["images"] for g in al["groups"]] == [2, 2]
    assert al == from_the_model(model, framed, [k for k in picked if k in framed], 2)
    assert al != from_the_model(model, framed, sorted(k for k in picked if k in framed), 2)


def test_without_the_flag_the_files_are_what_they_were(folder):
    root = folder[0]
    _run(folder, pool=4, loss=True)
    plain = _files(root)
    _run(folder, pool=4, loss=True, as_logged=False)
    assert _files(root) == plain
    _run(folder, pool=4, loss=True, as_logged=True)
    csv_bytes, summary = _files(root)
    assert csv_bytes == plain[0]                                                                # the per-image rows are the per-image operation's
    summary, before = json.loads(summary), json.loads(plain[1])
    assert summary["frame"].pop("as_logged") and summary == before
    with pytest.raises(ValueError, match="--as_logged needs --frame training"):
        ev.evaluate_folder(root, folder[1], precision="f16x2", device_index=0, as_logged=True)


def test_a_dual_that_decodes_to_another_shape_fails_the_run_by_name(folder, monkeypatch):
    root = folder[0]
    decode = ev.decode_dual

    def short(path):                                                                            # one row less than its header promised
        grey = decode(path)
        return grey[:-1] if path.endswith(os.path.join("epinette_gelee", "a02.png")) else grey

    monkeypatch.setattr(ev, "decode_dual", short)
    with pytest.raises(RuntimeError, match=r"epinette_gelee/a02\.png passed the header checks .*shape_mismatch.*--subset"):
        _run(folder, pool=4, as_logged=True)
    st = _run(folder, pool=4)                                                                   # without the flag it is skipped, as before
    assert st["summary"]["skipped"]["shape_mismatch"] == ["epinette_gelee/a02.png"]


def test_a_shard_beyond_the_bound_is_refused_before_the_loop(folder, monkeypatch):
    monkeypatch.setattr(ev, "AS_LOGGED_MAX_BYTES", ev.as_logged_bytes(6, T, 4) - 1)
    with pytest.raises(ValueError, match="--as_logged would hold"):
        _run(folder, pool=4, as_logged=True)
    monkeypatch.setattr(ev, "AS_LOGGED_MAX_BYTES", ev.as_logged_bytes(6, T, 4))
    assert _run(folder, pool=4, as_logged=True)["summary"]["frame"]["as_logged"]["loss"] is not None


def test_every_architecture_has_the_two_methods():
    for make in mdl.MODELS.values():                                                            # constructing one touches no device
        m = make("fp32")
        assert callable(m.lovasz_softmax_groups) and callable(m.remove_small_zones_groups)
