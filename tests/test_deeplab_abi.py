"""deeplabv3_resnet50 on the host side (CPU only): the 362-key topology through the C ABI, strict loading and architecture
detection, the packed blob (layout, f32 pooling branch, the trailer's architecture word, the one power of two the five
ASPP branches share in f16x2), FCN blobs unchanged, and the folder drivers' architecture broadcast over gloo."""
import hashlib
import os

import ctypes as C
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from neuralbarkcalculator_amd import _lib, synth, topology
from neuralbarkcalculator_amd.model import DeepLabV3ResNet50, FCNResNet50, arch_of_state_dict, pack_state_dict

DL = "deeplabv3_resnet50"

# DeepLabHead's 44 keys in state_dict() order (the prefix classifier.0. on the convs.* and project.* keys)
_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
HEAD_KEYS = (
    [k for i in range(4) for k in [f"classifier.0.convs.{i}.0.weight"] + [f"classifier.0.convs.{i}.1.{b}" for b in _BN]]
    + ["classifier.0.convs.4.1.weight"] + [f"classifier.0.convs.4.2.{b}" for b in _BN]
    + ["classifier.0.project.0.weight"] + [f"classifier.0.project.1.{b}" for b in _BN]
    + ["classifier.1.weight"] + [f"classifier.2.{b}" for b in _BN]
    + ["classifier.4.weight", "classifier.4.bias"])


@pytest.fixture(scope="module")
def dl_sd():
    return synth.make_state_dict("trained_like", seed=7, arch=DL)


@pytest.fixture(scope="module")
def fcn_sd():
    return synth.make_state_dict("trained_like", seed=7)


def test_state_keys_through_the_abi(built_lib):
    spec = topology.state_dict_spec(DL)
    assert len(spec) == 362 and built_lib.nbc_arch_num_state_keys(1) == 362
    assert [k for k, _, _ in spec[:318]] == [k for k, _, _ in topology.state_dict_spec()[:318]]   # the shared trunk
    assert all(k.startswith("backbone.") for k, _, _ in spec[:318])
    assert [k for k, _, _ in spec[318:]] == HEAD_KEYS
    name = C.c_char_p()
    shape = (C.c_int64 * 4)()
    nd, dt = C.c_int32(), C.c_int32()
    for i, (key, shp, dtype) in enumerate(spec):
        _lib.check(built_lib.nbc_arch_state_key(1, i, C.byref(name), C.byref(shape), C.byref(nd), C.byref(dt)))
        assert name.value.decode() == key and nd.value == len(shp) and tuple(shape[:nd.value]) == shp
        assert dt.value == (1 if dtype == "int64" else 0)
    shapes = dict((k, s) for k, s, _ in spec)
    assert shapes["classifier.0.convs.3.0.weight"] == (256, 2048, 3, 3)
    assert shapes["classifier.0.convs.4.1.weight"] == (256, 2048, 1, 1)
    assert shapes["classifier.0.project.0.weight"] == (256, 1280, 1, 1)
    assert shapes["classifier.1.weight"] == (256, 256, 3, 3) and shapes["classifier.4.weight"] == (3, 256, 1, 1)
    # the unsuffixed functions are architecture 0; an unknown architecture is an error
    assert built_lib.nbc_arch_num_state_keys(0) == built_lib.nbc_num_state_keys() == 326
    assert built_lib.nbc_arch_num_state_keys(2) == _lib.NBC_ERR_INVALID


def test_conv_units_through_the_abi(built_lib):
    units = topology.conv_units(DL)
    assert built_lib.nbc_arch_num_convs(1) == len(units) == 61 and built_lib.nbc_num_convs() == 55
    d = _lib.NbcConvDesc()
    for i, u in enumerate(units):
        _lib.check(built_lib.nbc_arch_conv_info(1, i, C.byref(d)))
        got = (d.name.decode(), d.bn.decode() or None, d.cin, d.cout, d.k, d.stride, d.pad, d.dil, bool(d.relu), bool(d.bias),
               bool(d.residual))
        assert got == (u.name, u.bn, u.cin, u.cout, u.k, u.stride, u.pad, u.dil, u.relu, u.bias, u.residual)
    assert [(u.pad, u.dil) for u in units[54:57]] == [(12, 12), (24, 24), (36, 36)]
    assert units[57].pooled and sum(u.pooled for u in units) == 1


def test_strict_loading_between_the_architectures(built_lib, dl_sd, fcn_sd):
    with pytest.raises(RuntimeError, match="Missing key.*classifier.0.convs.0.0.weight.*Unexpected key.*\"classifier.0.weight\""):
        pack_state_dict(fcn_sd, "fp32", DL)
    with pytest.raises(RuntimeError, match="for fcn_resnet50.*Unexpected key.*classifier.0.project.0.weight"):
        pack_state_dict(dl_sd, "fp32")
    with pytest.raises(RuntimeError, match="Unexpected key"):
        FCNResNet50("fp32").load_state_dict(dl_sd)             # what the reference's strict load would do
    with pytest.raises(RuntimeError, match="Missing key"):
        DeepLabV3ResNet50("fp32").load_state_dict(fcn_sd)
    bad = dict(dl_sd)
    bad["classifier.0.convs.2.0.weight"] = np.zeros((256, 2048, 1, 1), np.float32)
    with pytest.raises(RuntimeError, match="size or dtype mismatch for: \"classifier.0.convs.2.0.weight\""):
        pack_state_dict(bad, "fp32", DL)


def test_architecture_detection(built_lib, dl_sd, fcn_sd):
    assert arch_of_state_dict(fcn_sd) == "fcn_resnet50"
    assert arch_of_state_dict(dl_sd) == DL
    partial = {k: v for k, v in dl_sd.items() if k != "classifier.0.convs.4.2.running_var"}
    with pytest.raises(RuntimeError, match="Missing key"):
        arch_of_state_dict(partial)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        arch_of_state_dict(dict(fcn_sd, **{"aux_classifier.0.weight": np.zeros((1,), np.float32)}))


def _align(v):
    return (v + 255) // 256 * 256


def _layout_bytes(units, prec):
    eb = 2 if prec == 1 else 4
    off = 0
    for u in units:
        if u.pooled:
            off = _align(_align(_align(off + u.cout * u.cin * 4) + u.cout * 4) + u.cout * 4)
        elif u.bn is None:
            off = _align(_align(off + u.cout * u.cin * 4) + u.cout * 4)
        else:
            ksteps = 7 if u.cin == 3 else u.k * u.k * u.cin * eb // 128
            off = _align(_align(_align(off + u.cout * ksteps * 128) + u.cout * 4) + u.cout * 4)
    return _align(off + 1024)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16x2"])
def test_blob_size_and_trailer_architecture_word(built_lib, dl_sd, fcn_sd, precision):
    prec = {"fp32": 0, "bf16": 1, "f16x2": 2}[precision]
    blob = pack_state_dict(dl_sd, precision, DL)
    assert blob.nbytes == built_lib.nbc_arch_packed_weights_bytes(prec, 1) == _layout_bytes(topology.conv_units(DL), prec)
    meta = blob[-1024:].view(np.int32)                          # the trailer is the blob's last 1 KiB
    assert meta[0] == 0x4e424335 and meta[1] == 0 and meta[2] == 61 and meta[3] == 1
    assert built_lib.nbc_packed_weights_arch(blob.ctypes.data, blob.nbytes, prec) == 1
    assert built_lib.nbc_packed_weights_flags_arch(blob.ctypes.data, blob.nbytes, prec, 1) == 0
    assert built_lib.nbc_packed_weights_flags_arch(blob.ctypes.data, blob.nbytes, prec, 0) < 0   # not an FCN blob
    fcn = pack_state_dict(fcn_sd, precision)
    assert fcn[-1024:].view(np.int32)[3] == 0 and built_lib.nbc_packed_weights_arch(fcn.ctypes.data, fcn.nbytes, prec) == 0
    assert DeepLabV3ResNet50(precision).load_state_dict(dl_sd).pack_flags == 0


# sha256 of the FCN blobs nbc_pack_weights wrote before the trailer's word 3 named the architecture (parent revision
# d41d263): the architecture-aware packer and the unsuffixed entry point must keep writing exactly these bytes
FCN_BLOB_SHA256 = {
    ("trained_like", 7, "fp32"): "316c9e5515971eab5ef6a2255414df5f59cc436d42f0b31084dbc23ae91b0bdf",
    ("trained_like", 7, "bf16"): "4c8f3386996475897f3bca9176a13973ea3b459efe70d6325f41267b3ee18289",
    ("trained_like", 7, "f16x2"): "2a8184d4e82a713bb0d9aa6205bae5ab1eaf712d477f6f7230ad26c5f7d1269d",
    ("random_init", 3, "f16x2"): "6cf307f5632f2b92175d3d42ea8bc28e54ab63a05b02cce5cbb989308240fd81",
}


@pytest.mark.parametrize("kind,seed,precision", sorted(FCN_BLOB_SHA256))
def test_fcn_blobs_are_byte_identical_to_the_parents(built_lib, kind, seed, precision):
    sd = synth.make_state_dict(kind, seed=seed)
    prec = {"fp32": 0, "bf16": 1, "f16x2": 2}[precision]
    blob = pack_state_dict(sd, precision)                        # nbc_pack_weights_arch(..., 0, ...)
    assert hashlib.sha256(blob.tobytes()).hexdigest() == FCN_BLOB_SHA256[(kind, seed, precision)]
    # the unsuffixed entry point writes the same bytes
    arr = (_lib.NbcTensor * len(sd))()
    keep = []
    for i, (k, v) in enumerate(sd.items()):
        a = np.ascontiguousarray(v)
        keep.append((a, k.encode()))
        arr[i].name, arr[i].data, arr[i].ndim = keep[-1][1], a.ctypes.data, v.ndim
        arr[i].dtype = 1 if v.dtype == np.int64 else 0
        for j in range(4):
            arr[i].shape[j] = v.shape[j] if j < v.ndim else 1
    other = np.zeros(built_lib.nbc_packed_weights_bytes(prec), np.uint8)
    _lib.check(built_lib.nbc_pack_weights(arr, len(sd), prec, other.ctypes.data, other.nbytes))
    assert np.array_equal(other, blob)


def _estimate(sd, bn):
    var = sd[bn + ".running_var"].astype(np.float64)
    return float((np.abs(sd[bn + ".bias"]) + 3 * np.abs(sd[bn + ".weight"]) * np.sqrt(var / (var + 1e-5))).max())


def _power(e):
    return 0 if 2.0 ** -5 <= e <= 2.0 ** 7 else 1 - int(np.floor(np.log2(e)))


def _head_sections(blob, units):
    """{unit name: (weights bytes, scale f32, shift f32)} of the f16x2 / f32 blob of DeepLabV3 (element size 4)."""
    out, off = {}, 0
    for u in units:
        if u.pooled:
            n = u.cout * u.cin * 4
        elif u.bn is None:
            n = u.cout * u.cin * 4
        else:
            n = u.cout * (7 if u.cin == 3 else u.k * u.k * u.cin * 4 // 128) * 128
        w = blob[off: off + n]
        off = _align(off + n)
        if u.bn is None:
            out[u.name] = (w, None, blob[off: off + 4 * u.cout].view(np.float32))
            off = _align(off + 4 * u.cout)
            continue
        sc = blob[off: off + 4 * u.cout].view(np.float32)
        off = _align(off + 4 * u.cout)
        sh = blob[off: off + 4 * u.cout].view(np.float32)
        off = _align(off + 4 * u.cout)
        out[u.name] = (w, sc, sh)
    return out


def _row_exponent(rows):
    m = np.abs(rows).max(1).astype(np.float64)
    return np.where(m > 0, 14 - np.floor(np.log2(np.where(m > 0, m, 1.0))), 0.0).astype(int)


@pytest.mark.parametrize("log2_scale,which", [(-14, (1,)), (-14, (0, 1, 2, 3, 4)), (12, (4,)), (0, ())])
def test_f16x2_aspp_branches_share_one_power(built_lib, dl_sd, log2_scale, which):
    """The five ASPP branches write one tensor: their BatchNorms get ONE power of two, the largest of their five estimates
    placed in [2, 4), folded into each branch's (scale, shift) and, inverted, into the projection's scale -- exactly.  The
    pooling branch keeps its f32 weights as the checkpoint holds them; its scale also takes layer4's power off."""
    units = topology.conv_units(DL)
    names = ["classifier.0.convs.%d.1" % i for i in range(4)] + ["classifier.0.convs.4.2"]
    sd = dict(dl_sd)
    for b in which:                                              # rescale the BatchNorm output of some branches
        for leaf in ("weight", "bias"):
            sd[names[b] + "." + leaf] = (sd[names[b] + "." + leaf] * np.float32(2.0 ** log2_scale)).astype(np.float32)
    blob = pack_state_dict(sd, "f16x2", DL)
    assert built_lib.nbc_packed_weights_flags_arch(blob.ctypes.data, blob.nbytes, 2, 1) == 0
    exps = blob[-1024:].view(np.int32)[8:8 + len(units)]
    idx = {u.name: i for i, u in enumerate(units)}
    a_cat = _power(max(_estimate(sd, n) for n in names))
    branch_units = [u for u in units if u.bn in names]
    assert [int(exps[idx[u.name]]) for u in branch_units] == [a_cat] * 5
    a_l4 = int(exps[idx["backbone.layer4.2.conv3"]])
    proj = units[idx["classifier.0.project.0"]]
    a_proj = _power(_estimate(sd, proj.bn))
    assert exps[idx[proj.name]] == a_proj and exps[idx["classifier.4"]] == 0
    if which == ():
        assert a_cat == 0 and not exps.any()
    elif len(which) == 5 or log2_scale > 0:
        assert a_cat != 0                                        # the largest estimate moved: so does the shared power
    else:
        assert a_cat == 0                                        # one small branch among ordinary ones: they decide
    sec = _head_sections(blob, units)

    def fold(bn):
        g, b = sd[bn + ".weight"], sd[bn + ".bias"]
        mu, var = sd[bn + ".running_mean"], sd[bn + ".running_var"]
        alpha = g * (np.float32(1.0) / np.sqrt(var + np.float32(1e-5), dtype=np.float32))
        return alpha, b - mu * alpha

    for u in branch_units:
        w, sc, sh = sec[u.name]
        alpha, beta = fold(u.bn)
        if u.pooled:
            np.testing.assert_array_equal(w.view(np.float32), sd[u.name + ".weight"].reshape(-1))
            k = np.zeros(u.cout, int)
        else:
            wt = sd[u.name + ".weight"].transpose(0, 2, 3, 1).reshape(u.cout, -1)
            k = _row_exponent(wt)
        np.testing.assert_array_equal(sc, np.ldexp(alpha, -k + a_cat - a_l4).astype(np.float32), err_msg=u.name)
        np.testing.assert_array_equal(sh, np.ldexp(beta, a_cat).astype(np.float32), err_msg=u.name)
    w, sc, sh = sec[proj.name]
    alpha, beta = fold(proj.bn)
    k = _row_exponent(sd[proj.name + ".weight"].reshape(proj.cout, -1))
    np.testing.assert_array_equal(sc, np.ldexp(alpha, -k + a_proj - a_cat).astype(np.float32))
    np.testing.assert_array_equal(sh, np.ldexp(beta, a_proj).astype(np.float32))


def _arch_worker(rank, world, port, case, out_dir):
    from neuralbarkcalculator_amd import predict as drv
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sd = None
        if rank == 0:                                            # only rank 0 reads the checkpoint: keys and shapes matter
            spec = topology.state_dict_spec(DL if case != "fcn" else "fcn_resnet50")
            sd = {k: np.zeros(s, np.int64 if t == "int64" else np.float32) for k, s, t in spec}
            if case == "bad":
                del sd["classifier.1.weight"]
        try:
            got = drv.resolve_arch("auto", sd, dist)
        except RuntimeError as e:
            got = "error: " + str(e)[:40]
        with open(os.path.join(out_dir, f"arch{rank}.txt"), "w") as f:
            f.write(got)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case,port", [("deeplab", 29651), ("fcn", 29652), ("bad", 29653)])
def test_driver_broadcasts_the_architecture_over_gloo(tmp_path, case, port):
    mp.spawn(_arch_worker, args=(2, port, case, str(tmp_path)), nprocs=2, join=True)
    got = [open(os.path.join(str(tmp_path), f"arch{r}.txt")).read() for r in range(2)]
    if case == "bad":
        assert all(g.startswith("error") for g in got), got      # every rank leaves alike
    else:
        assert got == [DL if case == "deeplab" else "fcn_resnet50"] * 2


def test_driver_arch_options():
    from neuralbarkcalculator_amd import predict as drv
    assert drv.resolve_arch("deeplabv3_resnet50") == DL and drv.resolve_arch("fcn_resnet50") == "fcn_resnet50"
    with pytest.raises(ValueError):
        drv.resolve_arch("deeplabv3_resnet101")
