"""Per-image BatchNorm statistics on the f16x2 pipe without a GPU: the raw-convolution array of the C ABI (powers of two,
their relation to the blob's row and tensor exponents and to the running statistics, strict keys), the launch plan of the
mode, the model's and the drivers' option checks, and the two-rank broadcast of the array over gloo."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from neuralbarkcalculator_amd import _lib, synth, topology
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import folder_run
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import (DeepLabV3ResNet50, FCNResNet50, _tensor_array, bn_raw_flags, broadcast_bn_raw,
                                            conv_tile_info, describe_plan, fcn_resnet50, pack_bn_raw, pack_state_dict)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from bn_image_f16x2 import blob_sections, misjudged_state_dict, raw_sections  # noqa: E402

DL = "deeplabv3_resnet50"


@pytest.fixture(scope="module")
def fcn_sd():
    return synth.make_state_dict("trained_like", seed=7)


def _bn_units():
    return [u for u in topology.conv_units() if u.bn is not None]


def _row_and_input_power(sd, blob):
    """{unit: 2^(k_o + a_in)} from the blob: its scale is gamma / sqrt(var + eps) (f32, as the packer forms it) times
    2^(a_out - k_o - a_in), and the trailer holds a_out."""
    sections, exps = blob_sections(blob)
    out = {}
    for u in _bn_units():
        inv = np.float32(1.0) / np.sqrt(sd[u.bn + ".running_var"] + np.float32(1e-5), dtype=np.float32)
        alpha = (sd[u.bn + ".weight"] * inv).astype(np.float64)
        scale = sections[u.name][1].astype(np.float64)
        assert (alpha != 0).all() and (scale != 0).all(), u.name
        out[u.name] = alpha * 2.0 ** exps[u.name] / scale
    return out, exps


def test_raw_array_length_and_powers_of_two(built_lib, fcn_sd):
    n = built_lib.nbc_arch_bn_raw_floats(0)
    assert n == 2 * sum(u.cout for u in _bn_units()) == built_lib.nbc_arch_bn_affine_floats(0)
    assert built_lib.nbc_arch_bn_raw_floats(7) == 0
    raw, flags = pack_bn_raw(fcn_sd)
    assert raw.dtype == np.float32 and raw.size == n and flags == 0 and bn_raw_flags(raw) == 0
    mant, _ = np.frexp(raw)
    assert (mant == 0.5).all()                                  # every entry a power of two


def test_raw_array_undoes_the_blobs_row_and_input_powers(built_lib, fcn_sd):
    raw = raw_sections(pack_bn_raw(fcn_sd)[0])
    powers, _ = _row_and_input_power(fcn_sd, pack_state_dict(fcn_sd, "f16x2"))
    for u in _bn_units():
        first, second = (v.astype(np.float64) for v in raw[u.name])
        np.testing.assert_array_equal(first * second * powers[u.name], np.ones(u.cout), err_msg=u.name)


def test_raw_array_normalises_by_the_running_statistics(built_lib, fcn_sd):
    raw = raw_sections(pack_bn_raw(fcn_sd)[0])
    seen = 0
    for u in _bn_units():
        mu = np.abs(fcn_sd[u.bn + ".running_mean"].astype(np.float64))
        sd3 = 3.0 * np.sqrt(np.maximum(fcn_sd[u.bn + ".running_var"].astype(np.float64), 0.0))
        est = mu + sd3
        v = est / raw[u.name][1].astype(np.float64)             # second = 2^-r_o, and 2^r_o brings the estimate into [2, 4)
        pos = est > 0
        assert ((v[pos] >= 2.0) & (v[pos] < 4.0)).all(), u.name
        assert (raw[u.name][1][~pos] == 1.0).all()
        seen += int(pos.sum())
    assert seen > 20000
    # a misjudged channel moves its own power and nothing else, and the blob's weights do not move at all
    a = misjudged_state_dict(fcn_sd, 40)
    raw_a = raw_sections(pack_bn_raw(a)[0])
    unit = [u for u in _bn_units() if u.bn == "backbone.layer2.1.bn2"][0]
    for u in _bn_units():
        if u.name != unit.name:
            np.testing.assert_array_equal(raw_a[u.name][0], raw[u.name][0])
            np.testing.assert_array_equal(raw_a[u.name][1], raw[u.name][1])
    v = 3.0 * np.sqrt(a[unit.bn + ".running_var"].astype(np.float64)) / raw_a[unit.name][1].astype(np.float64)
    assert ((v >= 2.0) & (v < 4.0)).all()
    assert (np.abs(np.log2(raw_a[unit.name][1] / raw[unit.name][1]) - 20) <= 1).all()     # 2^20 up to the mean's share
    w_a, w = blob_sections(pack_state_dict(a, "f16x2"))[0], blob_sections(pack_state_dict(fcn_sd, "f16x2"))[0]
    for u in _bn_units():
        np.testing.assert_array_equal(w_a[u.name][0], w[u.name][0], err_msg=u.name)


@pytest.mark.parametrize("where,log2_scale", [("internal", -16), ("all", -20), ("all", 12)])
def test_raw_array_takes_the_input_tensors_power_from_the_trailer(built_lib, fcn_sd, where, log2_scale):
    from conftest import rescale_activations
    sd = rescale_activations(fcn_sd, 2.0 ** log2_scale, where)
    # 2^k_o: the ordinary checkpoint stores every tensor with power 0, and its conv weights are the rescaled one's
    row, exps0 = _row_and_input_power(fcn_sd, pack_state_dict(fcn_sd, "f16x2"))
    assert not any(exps0.values())
    _, exps = blob_sections(pack_state_dict(sd, "f16x2"))
    raw, flags = pack_bn_raw(sd)
    assert flags == 0
    raw = raw_sections(raw)
    # the power of the tensor each unit reads, from the trailer: a block's conv1 and downsample.0 read the residual stream
    # in front of the block, conv2 and conv3 the unit before them, classifier.0 the last stream
    a_in, stream, block_in = {}, exps["backbone.conv1"], None
    for u in _bn_units():
        leaf = u.name.rsplit(".", 1)[-1]
        if u.name == "backbone.conv1":
            a_in[u.name] = 0                                    # the image
        elif leaf == "conv1":
            block_in = stream
            a_in[u.name] = block_in
        elif leaf == "conv2":
            a_in[u.name] = exps[u.name[:-1] + "1"]
        elif leaf == "0" and ".downsample." in u.name:
            a_in[u.name] = block_in
        elif leaf == "conv3":
            a_in[u.name] = exps[u.name[:-1] + "2"]
            stream = exps[u.name]
        else:
            assert u.name == "classifier.0"
            a_in[u.name] = stream
    moved = 0
    for u in _bn_units():
        first, second = (v.astype(np.float64) for v in raw[u.name])
        np.testing.assert_array_equal(first * second * row[u.name], np.full(u.cout, 2.0 ** -a_in[u.name]), err_msg=u.name)
        moved += a_in[u.name] != 0
    assert moved >= 32


def test_raw_array_refuses_bad_keys_with_the_pack_message(built_lib, fcn_sd):
    bad = dict(fcn_sd)
    del bad["backbone.layer2.1.bn2.weight"]
    with pytest.raises(RuntimeError) as e1:
        pack_bn_raw(bad)
    assert "Missing key(s) in state_dict" in str(e1.value) and "backbone.layer2.1.bn2.weight" in str(e1.value)
    with pytest.raises(RuntimeError) as e2:
        pack_state_dict(bad)
    assert str(e1.value) == str(e2.value)
    shaped = dict(fcn_sd)
    shaped["classifier.1.bias"] = np.zeros(511, np.float32)
    with pytest.raises(RuntimeError, match="size or dtype mismatch for:.*classifier.1.bias"):
        pack_bn_raw(shaped)
    arr, n, _keep = _tensor_array(fcn_sd)
    out = np.zeros(10, np.float32)
    assert built_lib.nbc_pack_bn_raw(arr, n, 0, out.ctypes.data, 10) == _lib.NBC_ERR_INVALID


def test_raw_array_flags_a_power_outside_f32(built_lib, fcn_sd):
    sd = dict(fcn_sd)
    sd["backbone.layer1.0.bn1.running_var"] = np.full_like(fcn_sd["backbone.layer1.0.bn1.running_var"], 3e38)
    sd["backbone.layer1.0.bn1.running_mean"] = np.zeros_like(fcn_sd["backbone.layer1.0.bn1.running_mean"])
    sd["backbone.layer1.0.conv1.weight"] = fcn_sd["backbone.layer1.0.conv1.weight"] * np.float32(2.0 ** -60)   # r - k < -126
    raw, flags = pack_bn_raw(sd)
    assert flags & _lib.PACK_SCALE_RANGE and bn_raw_flags(raw) == _lib.PACK_SCALE_RANGE
    m = FCNResNet50("f16x2").set_bn_statistics("image_f16x2").load_state_dict(sd)
    assert m.pack_flags & _lib.PACK_SCALE_RANGE


def _ops(text):
    out = []
    for line in text.splitlines():
        f = line.split()
        if f[0] == "op":
            out.append(dict(name=f[1], kernel=f[2], **dict(kv.split("=") for kv in f[3:])))
    return out


def test_plan_of_the_mode(built_lib):
    ops = _ops(describe_plan("fcn_resnet50", "f16x2", 2, 64, 1024, False, "image"))
    ref = _ops(describe_plan("fcn_resnet50", "fp32", 2, 64, 1024, False, "image"))
    assert [(o["name"], o["kernel"]) for o in ops] == [(o["name"], o["kernel"]) for o in ref]
    kinds = [o["kernel"] for o in ops]
    assert kinds.count("conv_dma") == 54 and kinds.count("bn_stats") == 54 and kinds.count("bn_apply") == 54
    assert all(o["launches"] == "2" for o in ops if o["kernel"] == "bn_stats")
    assert not any("ds" in o for o in ops)                      # no fused (downsample.0, conv3) pair
    assert any("ds" in o for o in _ops(describe_plan("fcn_resnet50", "f16x2", 2, 64, 1024, False, "running")))
    for i, o in enumerate(ops):
        if o["kernel"] == "conv_dma":
            bn = topology.conv_units()[[u.name for u in topology.conv_units()].index(o["name"])].bn
            assert [ops[i + 1]["name"], ops[i + 2]["name"]] == [bn + ".stats", bn + ".apply"]
            assert "res" not in o                               # the identity is the apply op's
    # the stride-1 3x3 convolutions of the 8 x 128 maps run raw on both kinds of the row-step kernel
    by_name = {u.name: u for u in topology.conv_units()}
    row_kinds = set()
    for o in ops:
        u = by_name.get(o["name"])
        if o["kernel"] == "conv_dma" and u.k == 3 and u.stride == 1 and not o["name"].startswith("backbone.layer1"):
            kind = conv_tile_info("f16x2", int(o["tile"]))[2]
            assert kind in (1, 2), (o["name"], o["tile"])
            row_kinds.add(kind)
    assert row_kinds == {1, 2}
    # keep mode plans the same ops
    kept = _ops(describe_plan("fcn_resnet50", "f16x2", 1, 96, 160, True, "image"))
    assert [o["kernel"] for o in kept].count("bn_apply") == 54


def test_plan_refusals(built_lib):
    with pytest.raises(RuntimeError, match="Expected more than 1 value per channel when training"):
        describe_plan("fcn_resnet50", "f16x2", 1, 8, 8, False, "image")
    with pytest.raises(RuntimeError, match="per-image BatchNorm statistics need"):
        describe_plan("fcn_resnet50", "bf16", 1, 64, 64, False, "image")
    with pytest.raises(RuntimeError, match="per-image BatchNorm statistics need"):
        describe_plan(DL, "f16x2", 1, 64, 64, False, "image")


def test_set_bn_statistics_validation(built_lib):
    m = FCNResNet50("f16x2")
    assert m.set_bn_statistics("image_f16x2") is m and m.bn_statistics == "image_f16x2"
    m.set_bn_statistics("running")
    for prec in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="f16x2"):
            FCNResNet50(prec).set_bn_statistics("image_f16x2")
    with pytest.raises(ValueError, match=r"\[1, 256, 1, 1\]"):
        DeepLabV3ResNet50("f16x2").set_bn_statistics("image_f16x2")
    assert fcn_resnet50(precision="f16x2", bn_statistics="image_f16x2").bn_statistics == "image_f16x2"
    with pytest.raises(ValueError, match="f16x2"):
        fcn_resnet50(precision="fp32", bn_statistics="image_f16x2")


def test_driver_options(capsys):
    assert drv.resolve_bn_stats("image_f16x2", "auto") == "auto"
    assert drv.resolve_bn_stats("image_f16x2", "f16x2") == "f16x2"
    for prec in ("fp32", "bf16"):
        with pytest.raises(ValueError, match="f16x2"):
            drv.resolve_bn_stats("image_f16x2", prec)
    assert "image_f16x2" in folder_run.BN_STATS
    drv.check_bn_stats_arch("image_f16x2", "fcn_resnet50")
    with pytest.raises(ValueError, match="deeplabv3_resnet50"):
        drv.check_bn_stats_arch("image_f16x2", DL)
    with pytest.raises(ValueError, match="fcn_efficientnet_b0"):
        drv.check_bn_stats_arch("image_f16x2", "fcn_efficientnet_b0")
    for main in (drv.main, ev.main):                            # refused at argument time, before any device is touched
        for prec in ("fp32", "bf16"):
            with pytest.raises(SystemExit) as e:
                main(["/nonexistent", "--bn_stats", "image_f16x2", "--precision", prec])
            assert e.value.code == 2
    assert "--bn_stats image_f16x2 runs in --precision f16x2" in capsys.readouterr().err


def test_auto_falls_back_to_image_in_fp32():
    seen = []

    def run(precision, **kw):
        seen.append((precision, kw))
        if precision == "f16x2":
            raise folder_run.NonFiniteLogits("range", 0, 1)
        return {"rank": 0}

    folder_run.run_precision("predict", run, "auto", "image_f16x2")
    assert seen == [("f16x2", {"precision_auto": True}), ("fp32", {"bn_stats": "image"})]
    seen.clear()
    folder_run.run_precision("predict", run, "auto")
    assert seen == [("f16x2", {"precision_auto": True}), ("fp32", {})]


def test_evaluation_summary_records_the_mode():
    items = [{"name": "a.png", "wood": "sapin"}]
    row = np.zeros((1, 22), np.int64)
    row[0, 4] = row[0, 13] = 5
    _, summary = ev.report(items, row, "f16x2", "m.pt", "image_f16x2")
    assert (summary["bn_statistics"], summary["precision"]) == ("image_f16x2", "f16x2")
    assert "per-image BatchNorm" in ev.format_summary(summary)


def _raw_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        raw = None
        if rank == 0:                                            # only rank 0 reads the checkpoint
            raw = pack_bn_raw(synth.make_state_dict("trained_like", seed=11))[0]
        np.save(os.path.join(out_dir, f"raw{rank}.npy"), broadcast_bn_raw(raw))
    finally:
        dist.destroy_process_group()


def test_raw_array_broadcast_over_gloo(tmp_path, built_lib):
    mp.spawn(_raw_worker, args=(2, 29683, str(tmp_path)), nprocs=2, join=True)
    want = pack_bn_raw(synth.make_state_dict("trained_like", seed=11))[0]
    for r in range(2):
        got = np.load(os.path.join(str(tmp_path), f"raw{r}.npy"))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
