"""Per-image BatchNorm statistics without a GPU: the affine array of the C ABI (length, content, strict keys), the model's
and the drivers' option checks, the two-rank broadcast of the affine array over gloo, and the CPU oracle of the mode
(tests/helpers/bn_image_oracle.py) against a float64 numpy restatement."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from neuralbarkcalculator_amd import _lib, synth, topology
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import (DeepLabV3ResNet50, FCNResNet50, broadcast_bn_affine, fcn_resnet50,
                                            pack_bn_affine)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bn_image_oracle  # noqa: E402

DL = "deeplabv3_resnet50"


@pytest.fixture(scope="module")
def fcn_sd():
    return synth.make_state_dict("trained_like", seed=7)


def _bn_units(arch):
    return [u for u in topology.conv_units(arch) if u.bn is not None]


@pytest.mark.parametrize("arch", ["fcn_resnet50", DL])
def test_affine_length_is_twice_the_batchnorm_channels(built_lib, arch):
    n = built_lib.nbc_arch_bn_affine_floats(topology.arch_index(arch))
    assert n == 2 * sum(u.cout for u in _bn_units(arch))
    assert built_lib.nbc_arch_bn_affine_floats(7) == 0


@pytest.mark.parametrize("arch", ["fcn_resnet50", DL])
def test_affine_is_gamma_then_beta_in_unit_order_bit_for_bit(built_lib, fcn_sd, arch):
    sd = fcn_sd if arch == "fcn_resnet50" else synth.make_state_dict("trained_like", seed=7, arch=DL)
    got = pack_bn_affine(sd, arch)
    want = np.concatenate([np.concatenate([sd[u.bn + ".weight"], sd[u.bn + ".bias"]]).astype(np.float32)
                           for u in _bn_units(arch)])
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_affine_refuses_bad_keys_with_the_pack_message(built_lib, fcn_sd):
    bad = dict(fcn_sd)
    del bad["backbone.layer2.1.bn2.weight"]
    with pytest.raises(RuntimeError) as e1:
        pack_bn_affine(bad)
    assert "Missing key(s) in state_dict" in str(e1.value) and "backbone.layer2.1.bn2.weight" in str(e1.value)
    assert "nbc error %d" % _lib.NBC_ERR_KEYS in str(e1.value)
    shaped = dict(fcn_sd)
    shaped["classifier.1.bias"] = np.zeros(511, np.float32)
    with pytest.raises(RuntimeError, match="size or dtype mismatch for:.*classifier.1.bias"):
        pack_bn_affine(shaped)
    # the same words as strict packing of the blob
    from neuralbarkcalculator_amd.model import pack_state_dict
    with pytest.raises(RuntimeError) as e2:
        pack_state_dict(bad)
    assert str(e1.value) == str(e2.value)
    # the C entry point itself: too small an output
    from neuralbarkcalculator_amd.model import _tensor_array
    arr, n, _keep = _tensor_array(fcn_sd)
    out = np.zeros(10, np.float32)
    assert built_lib.nbc_pack_bn_affine(arr, n, 0, out.ctypes.data, 10) == _lib.NBC_ERR_INVALID


def test_set_bn_statistics_validation(built_lib):
    m = FCNResNet50("fp32")
    assert m.bn_statistics == "running"
    assert m.set_bn_statistics("image") is m and m.bn_statistics == "image"
    m.set_bn_statistics("running")
    with pytest.raises(ValueError, match="bn_statistics must be one of"):
        m.set_bn_statistics("batch")
    for prec in ("f16x2", "bf16"):
        with pytest.raises(ValueError, match="fp32"):
            FCNResNet50(prec).set_bn_statistics("image")
        FCNResNet50(prec).set_bn_statistics("running")
    with pytest.raises(ValueError, match=r"\[1, 256, 1, 1\]"):
        DeepLabV3ResNet50("fp32").set_bn_statistics("image")
    assert fcn_resnet50(bn_statistics="image").bn_statistics == "image"
    with pytest.raises(ValueError):
        fcn_resnet50(precision="bf16", bn_statistics="image")
    with pytest.raises(RuntimeError):
        FCNResNet50("fp32").train(True)                         # not training: nothing is updated


def test_driver_bn_stats_options(capsys):
    assert drv.resolve_bn_stats("image", "auto") == "fp32"
    assert drv.resolve_bn_stats("image", "fp32") == "fp32"
    for prec in ("auto", "fp32", "f16x2", "bf16"):
        assert drv.resolve_bn_stats("running", prec) == prec
    for prec in ("f16x2", "bf16"):
        with pytest.raises(ValueError, match="fp32"):
            drv.resolve_bn_stats("image", prec)
    with pytest.raises(ValueError):
        drv.resolve_bn_stats("batch", "fp32")
    drv.check_bn_stats_arch("image", "fcn_resnet50")
    drv.check_bn_stats_arch("running", DL)
    with pytest.raises(ValueError, match="deeplabv3_resnet50"):
        drv.check_bn_stats_arch("image", DL)
    # refused at argument time, before any device is touched
    for main in (drv.main, ev.main):
        for prec in ("f16x2", "bf16"):
            with pytest.raises(SystemExit) as e:
                main(["/nonexistent", "--bn_stats", "image", "--precision", prec])
            assert e.value.code == 2
    assert "--bn_stats image runs in --precision fp32" in capsys.readouterr().err


def test_evaluation_summary_records_the_mode():
    items = [{"name": "a.png", "wood": "sapin"}]
    row = np.zeros((1, 22), np.int64)
    row[0, 3] = 0
    row[0, 4] = row[0, 13] = 5
    _, summary = ev.report(items, row, "fp32", "m.pt", "image")
    assert summary["bn_statistics"] == "image"
    assert ev.report(items, row, "fp32", "m.pt")[1]["bn_statistics"] == "running"
    assert "per-image BatchNorm" in ev.format_summary(summary)


def _affine_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        affine = None
        if rank == 0:                                            # only rank 0 reads the checkpoint
            affine = pack_bn_affine(synth.make_state_dict("trained_like", seed=11))
        got = broadcast_bn_affine(affine)
        np.save(os.path.join(out_dir, f"affine{rank}.npy"), got)
    finally:
        dist.destroy_process_group()


def test_affine_array_broadcast_over_gloo(tmp_path, built_lib):
    mp.spawn(_affine_worker, args=(2, 29671, str(tmp_path)), nprocs=2, join=True)
    want = pack_bn_affine(synth.make_state_dict("trained_like", seed=11))
    for r in range(2):
        got = np.load(os.path.join(str(tmp_path), f"affine{r}.npy"))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the oracle of the mode -------------------------------------------------------------------------------------------
def _bn_image_numpy(x, gamma, beta, eps=1e-5):
    """F.batch_norm(training=True) of one image restated in float64 numpy: x [C,H,W]."""
    x = x.astype(np.float64)
    mean = x.mean(axis=(1, 2))
    var = ((x - mean[:, None, None]) ** 2).mean(axis=(1, 2))      # biased
    return (x - mean[:, None, None]) / np.sqrt(var + eps)[:, None, None] * gamma[:, None, None] + beta[:, None, None]


@pytest.fixture(scope="module")
def small_oracle(fcn_sd):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    return bn_image_oracle.load(fcn_sd)


def test_oracle_is_per_image_batchnorm_of_one_bottleneck(fcn_sd, small_oracle):
    x = torch.from_numpy(np.stack([synth.make_input(i, 48, 40) for i in (1, 2)]))
    outs = bn_image_oracle.layer_outputs(small_oracle.double(), x.double())
    small_oracle.float()
    # backbone.layer2.0: conv1 (1x1) of the previous unit's output, then bn1 and ReLU, per image
    t = outs["backbone.layer1.2.conv3"].numpy()
    w = fcn_sd["backbone.layer2.0.conv1.weight"].astype(np.float64)[:, :, 0, 0]
    g, b = fcn_sd["backbone.layer2.0.bn1.weight"], fcn_sd["backbone.layer2.0.bn1.bias"]
    for n in range(2):
        conv = np.einsum("oc,chw->ohw", w, t[n])
        want = np.maximum(_bn_image_numpy(conv, g.astype(np.float64), b.astype(np.float64)), 0.0)
        np.testing.assert_allclose(outs["backbone.layer2.0.conv1"][n].numpy(), want, rtol=0, atol=1e-10 * np.abs(want).max())
    # the running buffers never move, and they are not what the mode uses
    assert torch.equal(small_oracle.backbone.layer2[0].bn1.running_mean,
                       torch.from_numpy(fcn_sd["backbone.layer2.0.bn1.running_mean"]))


def test_oracle_batch_of_two_equals_each_alone(small_oracle):
    x = torch.from_numpy(np.stack([synth.make_input(i, 40, 56) for i in (3, 4)]))
    both = bn_image_oracle.lowres_logits(small_oracle, x)
    for i in range(2):
        assert torch.equal(both[i:i + 1], bn_image_oracle.lowres_logits(small_oracle, x[i:i + 1]))
    # and it is not the eval-mode network
    from oracle.fcn_resnet50_oracle import OracleFCNResNet50
    ev_model = OracleFCNResNet50()
    ev_model.load_state_dict(small_oracle.state_dict())
    with torch.no_grad():
        assert float((ev_model.lowres_logits(x) - both).abs().max()) > 1e-3
