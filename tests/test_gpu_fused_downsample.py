"""The dual-branch form of the f16x2 conv kernel (csrc/conv_igemm_dma.hip, kVarDualBranch): downsample.0 of a stage's first
bottleneck computed inside the launch of the conv3 that adds it, for layer1.0, layer2.0 and layer3.0.  The tensor between
the two goes through the same fma, split and join as when it is stored and read back, so everything here is bit equality:
fused against two launches, against a tile that has no fused form, against the keep-activations run (which never fuses and
is itself checked layer by layer against the oracle), and against itself on two streams."""
import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import synth
from neuralbarkcalculator_amd.model import FCNResNet50, conv_tile_info, describe_plan

pytestmark = pytest.mark.gpu

LAYER_RTOL_FP32 = 4e-6      # tests/test_gpu_parity.py: the f32-grade modes' layer tolerance
DEV = "cuda:0"


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def model(built_lib, sd_np):
    m = FCNResNet50("f16x2").load_state_dict(sd_np).to(DEV)
    yield m
    m.set_fuse_downsample(True)
    m.set_conv_tile(-1)
    m.set_keep_activations(False)


def run(m, x):
    labels, counts, lowres = m.predict_labels(x, return_lowres=True)
    torch.cuda.synchronize()
    return labels.clone(), counts.clone(), lowres.clone(), m.fused_pairs()


# (1, 40, 72): layer1 maps of 10x18 = one full 128-pixel tile and a tail, a stride-2 downsample onto an odd 5x9 map, a pixel
# tile with most lanes out of range; (2, 72, 136): an image boundary inside a pixel tile; (3, 24, 1024): 128-pixel-wide maps
@pytest.mark.parametrize("shape,nan_pixel", [((1, 128, 128), False), ((1, 128, 128), True), ((1, 40, 72), False), ((2, 72, 136), False),
                                             ((2, 72, 136), True), ((3, 24, 1024), False)])
def test_fused_equals_two_launches_bit_for_bit(model, shape, nan_pixel):
    n, h, w = shape
    x = frames(range(50, 50 + n), h, w)
    if nan_pixel:                                        # as in test_nan_propagates_like_the_oracle: NaNs take the same way through both forms
        x[0, 1, h // 3, w // 2] = float("nan")
    x = x.to(DEV)
    model.set_fuse_downsample(True)
    l1, c1, low1, pairs = run(model, x)
    assert pairs == 3
    model.set_fuse_downsample(False)
    try:
        l0, c0, low0, pairs0 = run(model, x)
    finally:
        model.set_fuse_downsample(True)
    assert pairs0 == 0
    assert bool(torch.isnan(low1).any()) == nan_pixel and (n == 1 and nan_pixel or torch.isfinite(low1).any())
    assert torch.equal(bits(low1), bits(low0)), "lowres logits differ between the fused and the two-launch form"
    assert torch.equal(l1, l0) and torch.equal(c1, c0)


@pytest.mark.parametrize("shape", [(2, 72, 136), (1, 520, 1024)])
def test_fused_at_the_full_size_tile(model, shape):
    """Tile 17 (the three layers' tile at 1024x1024) forced: fused and two-launch forms agree on a small batch and on an
    image with more blocks than the chip holds at once (layer1: 520 tiles), where a block finishes while others have not
    started -- the fused launch must not write where a later block still reads (the plan gives conv3 a buffer that is
    neither its own input nor the downsample's)."""
    n, h, w = shape
    x = frames(range(61, 61 + n), h, w).to(DEV)
    model.set_conv_tile(17)
    try:
        _, _, low1, pairs = run(model, x)
        model.set_fuse_downsample(False)
        _, _, low0, pairs0 = run(model, x)
    finally:
        model.set_fuse_downsample(True)
        model.set_conv_tile(-1)
    assert (pairs, pairs0) == (3, 0)
    assert torch.isfinite(low1).all()
    assert torch.equal(bits(low1), bits(low0))


def test_the_fusion_runs_where_it_should_and_only_there(built_lib, sd_np, model):
    x = frames([3], 128, 128).to(DEV)
    _, _, want, pairs = run(model, x)
    assert pairs == 3
    for mode in ("fp32", "bf16"):
        other = FCNResNet50(mode).load_state_dict(sd_np).to(DEV)
        other.lowres_logits(x)
        torch.cuda.synchronize()
        assert other.fused_pairs() == 0, mode
    try:
        model.set_keep_activations(True)
        assert run(model, x)[3] == 0
        model.set_keep_activations(False)
        model.set_fuse_downsample(False)
        assert run(model, x)[3] == 0
        model.set_fuse_downsample(True)
        model.set_conv_tile(7)                           # a tile without the fused form
        _, _, low7, pairs7 = run(model, x)
        assert pairs7 == 0
        assert torch.equal(bits(low7), bits(want)), "a forced tile changes the logits"
        model.set_conv_tile(-1)
        assert run(model, x)[3] == 3
    finally:
        model.set_keep_activations(False)
        model.set_fuse_downsample(True)
        model.set_conv_tile(-1)


def test_layer_by_layer_with_keep_activations(oracle_model, model):
    """Keep-activations runs the pair as two launches (the tensor between them is read back here): both against the oracle,
    and the logits of that run against the fused run's."""
    from oracle.fcn_resnet50_oracle import layer_outputs
    x = frames([3], 128, 128)
    ref = layer_outputs(oracle_model, x)
    _, _, fused, pairs = run(model, x.to(DEV))
    assert pairs == 3
    model.set_keep_activations(True)
    try:
        _, _, kept, pairs_kept = run(model, x.to(DEV))
        assert pairs_kept == 0
        for stage in (1, 2, 3):
            for unit in ("downsample.0", "conv3"):
                name = "backbone.layer%d.0.%s" % (stage, unit)
                want = ref[name].numpy()
                got = model.read_activation(name, want.size)
                assert got.shape == want.shape, name
                scale = float(np.abs(want).max())
                err = float(np.abs(got - want).max())
                assert err <= LAYER_RTOL_FP32 * scale, f"{name}: max err {err} vs scale {scale}"
    finally:
        model.set_keep_activations(False)
    assert torch.equal(bits(kept), bits(fused))


def test_two_fused_forwards_at_once_are_deterministic(model):
    dev = torch.device(DEV)
    xs = [frames([70 + k], 128, 128).to(dev) for k in range(2)]
    alone = [run(model, x)[:3] for x in xs]
    models = [model, model.clone_shared()]
    streams = [torch.cuda.current_stream(dev), torch.cuda.Stream(dev)]
    outs = [None] * 2
    for rep in range(2):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                outs[k] = models[k].predict_labels(xs[k], return_lowres=True)
    torch.cuda.synchronize()
    assert [m.fused_pairs() for m in models] == [3, 3]
    for k in range(2):
        labels, counts, lowres = outs[k]
        assert torch.equal(labels, alone[k][0]) and torch.equal(counts, alone[k][1])
        assert torch.equal(bits(lowres), bits(alone[k][2])), f"stream {k} differs from the same frame alone"


DUAL_TILES = (17, 8, 10)     # the tiles flagged kTileDual in the menu (csrc/conv_tiles.hpp), written out: the independent pin


def test_the_two_forms_alternate_across_shapes_and_the_plan_cache(model):
    """One context, three shapes, each in both forms and out of the plan cache in the other one; whatever form ran before,
    every result is that of a fresh context in the default form.  The identity buffer, which only the two-launch form uses,
    is first allocated in the second step (1.25 MB, enough for the next two two-launch steps) and has to grow in the last
    one (3 x 6 x 256 pixels x 256 channels: 4.7 MB)."""
    steps = [((1, 40, 72), True), ((2, 72, 136), False), ((1, 40, 72), False), ((1, 128, 128), True), ((2, 72, 136), True),
             ((1, 128, 128), False), ((3, 24, 1024), False)]
    xs = {shape: frames(range(80, 80 + shape[0]), *shape[1:]).to(DEV) for shape, _ in steps}
    want = {}
    for shape, x in xs.items():
        fresh = model.clone_shared()
        want[shape] = run(fresh, x)
        fresh._destroy()
        assert want[shape][3] == 3 and torch.isfinite(want[shape][2]).all()
    m = model.clone_shared()
    try:
        for shape, fuse in steps:
            m.set_fuse_downsample(fuse)
            labels, counts, lowres, pairs = run(m, xs[shape])
            assert pairs == (3 if fuse else 0), (shape, fuse)
            assert torch.equal(bits(lowres), bits(want[shape][2])), (shape, fuse)
            assert torch.equal(labels, want[shape][0]) and torch.equal(counts, want[shape][1]), (shape, fuse)
    finally:
        m._destroy()


def test_autotune_on_a_context_that_only_ran_fused_then_a_forward(model):
    """nbc_autotune times downsample.0 and conv3 one by one, so it is the first to need the identity buffer here; the forward
    on the tuned tiles fuses the pairs whose conv3 got a tile with the dual-branch form."""
    x = frames([3], 128, 128).to(DEV)
    m = model.clone_shared()
    try:
        _, _, want, pairs = run(m, x)
        assert pairs == 3
        tiles = m.autotune(x, reps=1)
        assert tiles == m.plan_tiles()
        convs = [line.split()[1] for line in describe_plan("fcn_resnet50", "f16x2", 1, 128, 128).splitlines() if " conv_dma " in line]
        assert len(convs) == len(tiles) == 54
        conv3 = [tiles[convs.index("backbone.layer%d.0.conv3" % s)] for s in (1, 2, 3)]
        _, _, tuned, pairs = run(m, x)
        assert sorted(DUAL_TILES) == [t for t in range(21) if (conv_tile_info("f16x2", t) or (0, 0, 0, 0))[3]]
        assert pairs == sum(t in DUAL_TILES for t in conv3), conv3
        assert torch.equal(bits(tuned), bits(want))
    finally:
        m._destroy()


def test_profiling_runs_the_pairs_as_two_timed_launches(model):
    x = frames([3], 128, 128).to(DEV)
    m = model.clone_shared()
    try:
        _, _, want, pairs = run(m, x)
        assert pairs == 3
        m.set_profiling(True)
        _, _, low, pairs = run(m, x)
        records = m.op_records()
        m.set_profiling(False)
        assert pairs == 0 and len(records) == 58
        assert all(r["ms"] > 0 for r in records), [r["name"] for r in records if not r["ms"] > 0]
        assert torch.equal(bits(low), bits(want))
        assert run(m, x)[3] == 3
    finally:
        m._destroy()
