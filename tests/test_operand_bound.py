"""The per-element bound of tests/helpers/operand_bound.py without a GPU: the kernel's arithmetic restated on the CPU stays
within it on every element, and each of four seeded faults -- a truncating store, a K-step left out, a neighbour's alpha, a
lost border tap -- leaves it, at shapes whose K spans the network's (128 to 4608).  Beside each fault the figure the suite's
older bf16 metric (largest error over largest magnitude, limit 4e-2) gives it.  tests/test_gpu_bf16_operands.py holds the
device's kernels to the same bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import operand_bound as ob  # noqa: E402

from neuralbarkcalculator_amd import topology  # noqa: E402
from neuralbarkcalculator_amd.model import pack_state_dict  # noqa: E402

LAYER_RTOL_BF16 = 4e-2      # tests/test_gpu_parity.py: the limit the older metric holds bf16 to
SHAPES = [(128, 64, 1), (256, 64, 3), (512, 512, 3), (2048, 512, 1)]        # (Cin, Cout, k)
N, H, W = 2, 13, 17


def unit(cin, cout, k):
    """A conv unit as the network has them: post-ReLU bf16 inputs whose channels' gains spread over an order of magnitude,
    Kaiming-sized weights, a BatchNorm with every statistic alive, a post-ReLU bf16 residual with the same spread."""
    rng = np.random.default_rng(1000 * cin + 10 * cout + k)
    gain = np.logspace(-0.5, 0.5, cin, dtype=np.float32)[rng.permutation(cin)]
    x = ob.bf16_round(np.maximum(rng.standard_normal((N, cin, H, W), dtype=np.float32), 0) * gain[None, :, None, None])
    w = rng.standard_normal((cout, cin, k, k), dtype=np.float32) / np.float32(np.sqrt(cin * k * k))
    alpha, beta = ob.bn_pair(rng.uniform(0.5, 1.5, cout), 0.3 * rng.standard_normal(cout), 0.2 * rng.standard_normal(cout),
                             rng.uniform(0.25, 1.0, cout))
    gain_res = np.logspace(-0.5, 0.5, cout, dtype=np.float32)[rng.permutation(cout)]
    res = ob.bf16_round(np.maximum(rng.standard_normal((N, cout, H, W), dtype=np.float32), 0) * gain_res[None, :, None, None])
    return dict(x=x, w=w, alpha=alpha, beta=beta, res=res, relu=True, stride=1, pad=k // 2, dil=1)


_CASES = {}


def case(shape):
    """The unit, its float64 reference and its bound: computed once, shared, never written to."""
    if shape not in _CASES:
        torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))
        u = unit(*shape)
        y_ref, mag = ob.conv_unit_reference(**u)
        cin, _, k = shape
        bound = ob.bf16_unit_bound(y_ref, mag, u["alpha"], u["beta"], u["res"], cin * k * k)
        for a in (y_ref, bound):
            a.setflags(write=False)
        _CASES[shape] = u, y_ref, bound
    return _CASES[shape]


def ratios(got, y_ref, bound):
    """(worst ratio to the bound, share of elements over it, the older metric: largest error over largest magnitude)"""
    err = np.abs(got.astype(np.float64) - y_ref)
    r = err / bound
    return float(r.max()), float((r > 1.0).mean()), float(err.max() / np.abs(y_ref).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_faithful_arithmetic_is_within_the_bound_on_every_element(shape):
    u, y_ref, bound = case(shape)
    got = ob.emulate_unit(**u)
    worst, over, old = ratios(got, y_ref, bound)
    print("faithful %s: worst %.3f of the bound, %d elements over; older metric %.2e (limit %.0e)" %
          (shape, worst, int(over * got.size), old, LAYER_RTOL_BF16), flush=True)
    assert np.isfinite(got).all() and float(np.abs(y_ref).max()) > 1.0 and (got > 0).mean() > 0.25    # a live tensor
    assert worst <= 1.0, (shape, worst)


# every fault at every shape where it applies: a 1x1 kernel has no tap to lose
FAULT_CASES = [(s, f) for f in ob.FAULTS for s in SHAPES if f != "tap" or s[2] == 3]


@pytest.mark.parametrize("shape,fault", FAULT_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_a_seeded_fault_leaves_the_bound(shape, fault):
    u, y_ref, bound = case(shape)
    got = ob.emulate_unit(fault=fault, **u)
    worst, over, old = ratios(got, y_ref, bound)
    print("%s %s: worst %.3g of the bound, %.2f %% of elements over; older metric %.2e (limit %.0e: %s)" %
          (fault, shape, worst, 100 * over, old, LAYER_RTOL_BF16, "caught" if old > LAYER_RTOL_BF16 else "passes"), flush=True)
    assert worst > 1.0, (shape, fault, worst)
    if fault == "truncate":
        # what the bound is for: a store that truncates is an order of magnitude under the older metric's limit
        assert old < LAYER_RTOL_BF16 / 4, old
        assert worst <= 2.0                             # one bf16 ulp is twice the rounding's half
    if fault == "tap":
        hit = np.abs(got.astype(np.float64) - y_ref) > bound
        assert hit[..., -1].any() and not hit[..., :-1].any()       # the last column and nothing else


def test_the_bound_s_bf16_rounding_is_torch_s():
    """ties to even in both directions, carries into the exponent, the largest finite values, infinities, subnormals, NaN"""
    rng = np.random.default_rng(0)
    bits = np.concatenate([
        rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32),
        (np.arange(0x3f7e, 0x3f84, dtype=np.uint32)[:, None] << 16 | np.array([0x7fff, 0x8000, 0x8001, 0xffff, 0], np.uint32)).ravel(),
        np.array([0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
                  0x7f800001, 0x7fffffff, 0, 0x80000000, 1, 0x00008000, 0x00018000, 0x007fffff, 0x80008000], np.uint32)])
    a = bits.view(np.float32)
    want = torch.from_numpy(a.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    got = ob.bf16_round(a)
    nan = np.isnan(a)
    assert nan.sum() >= 4 and np.isnan(got[nan]).all() and np.isnan(want[nan]).all()
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert (got[~nan].view(np.uint32) & 0xffff == 0).all()
    assert ob.bf16_round(np.float32([3.4028235e38]))[0] == np.inf and ob.bf16_round(bits[-18:-17].view(np.float32)).view(np.uint32)[0] == 0x7f7f0000
    # truncation: the same values, never away from zero, and within one bf16 ulp
    fin = np.isfinite(a) & np.isfinite(got)
    t = ob.bf16_truncate(a)
    assert (np.abs(t[fin]) <= np.abs(a[fin])).all() and (t.view(np.uint32) & 0xffff == 0).all()


def test_the_restated_pair_is_float32_throughout():
    rng = np.random.default_rng(3)
    g, b, mu, var = rng.uniform(0.5, 1.5, 64), rng.standard_normal(64), rng.standard_normal(64), rng.uniform(0.1, 2.0, 64)
    alpha, beta = ob.bn_pair(g, b, mu, var)
    a64 = g.astype(np.float32).astype(np.float64) / np.sqrt(var.astype(np.float32).astype(np.float64) + 1e-5)
    b64 = b.astype(np.float32).astype(np.float64) - mu.astype(np.float32).astype(np.float64) * a64
    assert alpha.dtype == beta.dtype == np.float32
    # at most PAIR_ROUNDINGS roundings of 2^-24 on the way to either value
    assert (np.abs(alpha - a64) <= ob.PAIR_ROUNDINGS * ob.U * np.abs(a64)).all()
    assert (np.abs(beta - b64) <= ob.PAIR_ROUNDINGS * ob.U * (np.abs(b) + np.abs(mu * a64))).all()


def test_the_restated_pair_is_the_packer_s_bit_for_bit(built_lib, sd_np):
    """The bf16 blob's (scale, shift) of every conv unit (the layout of include/nbc.h: K-major bf16 rows in whole 128-byte
    K-steps, then scale and shift, every section 256-byte aligned): the four roundings the bound grants the pair are slack."""
    blob = pack_state_dict(sd_np, "bf16")
    align = lambda v: (v + 255) // 256 * 256  # noqa: E731
    off, seen = 0, 0
    for u in topology.conv_units():
        if u.bn is None:
            break
        ksteps = 7 if u.cin == 3 else u.k * u.k * u.cin * 2 // 128
        s_off = align(off + u.cout * ksteps * 128)
        t_off = align(s_off + u.cout * 4)
        alpha, beta = ob.bn_pair(*(sd_np[u.bn + k] for k in (".weight", ".bias", ".running_mean", ".running_var")))
        assert np.array_equal(blob[s_off: s_off + u.cout * 4].view(np.uint32), alpha.view(np.uint32)), u.name
        assert np.array_equal(blob[t_off: t_off + u.cout * 4].view(np.uint32), beta.view(np.uint32)), u.name
        off = align(t_off + u.cout * 4)
        seen += 1
    assert seen == 54
