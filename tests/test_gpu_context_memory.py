"""The context's device memory (csrc/device_mem.hpp under nbc_ctx): buffers that grow with the margin, are re-used and come
back with a cached plan; the workspaces that appear lazily (per-image BatchNorm, the identity buffer of a two-launch
downsample pair, remove_small_zones); weights loaded, loaded again, attached over an owned blob, and a refused load; the
temporaries of keep mode; destroy.  Everything is bit equality with a fresh context on the same weights."""
import ctypes as C

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib, synth
from neuralbarkcalculator_amd.model import FCNResNet50, _tensor_array

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 24, 40), (2, 40, 56), (1, 64, 64), (1, 24, 40)]      # rise, rise, rise past the margin of some buffers, fall


def frames(n, h, w, first=90):
    return torch.from_numpy(np.stack([synth.make_input(first + i, h, w) for i in range(n)])).to(DEV)


def predict(m, x):
    labels, counts, lowres = m.predict_labels(x, return_lowres=True)
    torch.cuda.synchronize()
    return labels, counts, lowres.view(torch.int32)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("labels", "counts", "lowres bits")):
        assert torch.equal(g, w), "%s: %s differ from a fresh context's" % (what, name)


@pytest.fixture(scope="module")
def fp32(built_lib, sd_np):
    """The weights every fresh context of this module shares (clone_shared: a context and workspace of its own)."""
    return FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)


@pytest.mark.parametrize("bn_statistics", ["running", "image"])
def test_rising_and_falling_shapes_on_one_object(fp32, bn_statistics):
    """"image" also grows the per-image BatchNorm workspace and allocates the unit table on the first forward."""
    m = fp32.clone_shared().set_bn_statistics(bn_statistics)
    for n, h, w in SHAPES:
        x = frames(n, h, w)
        assert_same(predict(m, x), predict(fp32.clone_shared().set_bn_statistics(bn_statistics), x), "%s at %s" % (bn_statistics, (n, h, w)))


def test_two_launch_downsample_pair_allocates_and_grows_the_identity_buffer(built_lib, sd_np):
    fused = FCNResNet50("f16x2").load_state_dict(sd_np).to(DEV)
    split = fused.clone_shared()
    split.set_fuse_downsample(False)
    for h in (32, 48):
        x = frames(1, h, h)
        got, want = predict(split, x), predict(fused, x)
        assert split.fused_pairs() == 0
        assert_same(got, want, "two launches at %dx%d" % (h, h))


def test_reload_and_reattach_at_the_c_abi(built_lib, fp32, sd_np):
    lib = built_lib
    x = frames(1, 32, 32)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    sd8 = synth.make_state_dict("trained_like", seed=8)
    want7 = fp32.clone_shared().lowres_logits(x)
    want8 = FCNResNet50("fp32").load_state_dict(sd8).to(DEV).lowres_logits(x)
    assert not torch.equal(want7, want8)

    def lowres(ctx):
        out = torch.empty_like(want7)
        _lib.check(lib.nbc_forward(ctx, x.data_ptr(), _lib.IN_F32_NCHW, 1, 32, 32, out.data_ptr(), None, None, _lib.LABEL_U8, None, 0,
                                   stream), "nbc_forward")
        torch.cuda.synchronize()
        return out

    ctx = C.c_void_p()
    _lib.check(lib.nbc_create(C.byref(ctx), 0), "nbc_create")
    try:
        for sd, want in ((sd_np, want7), (sd8, want8)):              # the second load replaces the blob the first one left
            arr, n, _keep = _tensor_array(sd)
            _lib.check(lib.nbc_load_weights(ctx, arr, n, _lib.PREC_FP32), "nbc_load_weights")
            assert torch.equal(lowres(ctx), want)
        blob = fp32._blob_dev                                         # a caller-held blob over the owned one
        _lib.check(lib.nbc_attach_weights(ctx, blob.data_ptr(), blob.numel(), _lib.PREC_FP32), "nbc_attach_weights")
        assert torch.equal(lowres(ctx), want7)
        # a refused load leaves the context as it was
        short = {k: v for k, v in sd8.items() if k != "backbone.layer2.0.conv1.weight"}
        arr, n, _keep = _tensor_array(short)
        nbytes = lib.nbc_packed_weights_bytes(_lib.PREC_FP32)
        pack_rc = lib.nbc_pack_weights(arr, n, _lib.PREC_FP32, np.zeros(nbytes, dtype=np.uint8).ctypes.data, nbytes)
        assert pack_rc != _lib.NBC_OK
        assert lib.nbc_load_weights(ctx, arr, n, _lib.PREC_FP32) == pack_rc
        assert torch.equal(lowres(ctx), want7)
        # and so after an owned blob: load, refused load, forward
        arr8, n8, _keep8 = _tensor_array(sd8)
        _lib.check(lib.nbc_load_weights(ctx, arr8, n8, _lib.PREC_FP32), "nbc_load_weights")
        assert lib.nbc_load_weights(ctx, arr, n, _lib.PREC_FP32) == pack_rc
        assert torch.equal(lowres(ctx), want8)
    finally:
        lib.nbc_destroy(ctx)


def test_remove_small_zones_workspace_grows_and_is_reused(fp32):
    m = fp32.clone_shared()
    rng = np.random.RandomState(5)
    for n, h, w in ((1, 16, 16), (2, 40, 40), (1, 16, 16)):
        labels = torch.from_numpy(rng.randint(0, 3, size=(n, h, w)).astype(np.uint8)).to(DEV)
        got, got_counts = m.remove_small_zones(labels.clone(), min_pixels=6)
        want, want_counts = fp32.clone_shared().remove_small_zones(labels.clone(), min_pixels=6)
        torch.cuda.synchronize()
        assert not torch.equal(got, labels)                           # zones were removed: the workspace was used
        assert torch.equal(got, want) and torch.equal(got_counts, want_counts)


def test_keep_mode_temporaries(fp32):
    m = fp32.clone_shared()
    x = frames(1, 32, 32)
    peaks = [m.activation_peaks(x) for _ in range(3)]
    assert peaks[0] == peaks[1] == peaks[2] and all(np.isfinite(v) and v > 0 for v in peaks[0].values())
    m.set_keep_activations(True)
    try:
        m.lowres_logits(x)
        reads = [m.read_activation("backbone.layer1.0.conv1", 1 << 16) for _ in range(3)]
    finally:
        m.set_keep_activations(False)
    assert reads[0].shape == (1, 64, 8, 8) and np.abs(reads[0]).max() > 0
    assert np.array_equal(reads[0], reads[1]) and np.array_equal(reads[0], reads[2])


def test_destroy_then_a_fresh_object(fp32):
    x = frames(1, 32, 32)
    first = fp32.clone_shared()
    want = predict(first, x)
    first.remove_small_zones(torch.zeros((1, 16, 16), dtype=torch.uint8, device=DEV))    # every kind of member holds something
    first._destroy()
    del first
    assert_same(predict(fp32.clone_shared(), x), want, "after a destroy")
