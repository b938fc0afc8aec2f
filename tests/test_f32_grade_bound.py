"""The per-element bound of tests/helpers/f32_grade_bound.py and the exact probe of tests/helpers/gather_probe.py without a
GPU.  The f16x2 kernel's arithmetic restated on the CPU (emulate_unit_f16x2) stays within the bound on every element for one
conv unit of each kind, and seven seeded faults are recorded per kind: which the bound rejects, and which only the probe's
bit-for-bit comparison sees.  Every fault is caught by one of the two; the bound alone misses a piece-level product lost in one
K-step from K of about 150 on (the stem, K = 147, and K = 64 reject it, K = 256 passes it at 0.48 of the bound: the allowance
c (3 K + 1) u A is measured against 2^-11 of ONE K-step's share of A, and that share shrinks as 32 / K) and a truncated low piece
everywhere (2^-22 of the element against an allowance of 2^-15 of A at K = 64), and the probe alone misses what it cannot hold: the weights' low piece
(Q = 0), a neighbour's alpha (every alpha of a probe unit is the same power of two) and a forgotten activation power (all 0).
Around that: the two figures of the store the bound relies on, against numpy's binary16, and the restated weight pieces against
the packed blob.  tests/test_gpu_f32_grade_operands.py and tests/test_gpu_gather_probe.py hold the device's kernels to both."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import f32_grade_bound as fb  # noqa: E402
import gather_probe as gp  # noqa: E402
import operand_bound as ob  # noqa: E402

from neuralbarkcalculator_amd import topology  # noqa: E402
from neuralbarkcalculator_amd.model import pack_state_dict  # noqa: E402

# kind: (Cin, Cout, k, stride, pad, dil, identity, a_in, a_out); the map is 9 x 11 (the stem's input 18 x 22), one image
KINDS = {
    "stem": (3, 64, 7, 2, 3, 1, False, 0, 2),
    "1x1": (256, 64, 1, 1, 0, 1, False, 4, -3),
    "3x3": (64, 64, 3, 1, 1, 1, False, -3, 0),
    "identity 1x1": (64, 128, 1, 1, 0, 1, True, 0, 5),
    "row-step 3x3": (512, 32, 3, 1, 1, 1, False, 4, 0),
    "projection": (1280, 32, 1, 1, 0, 1, False, 2, 2),
    "ASPP 3x3 dilation 3": (2048, 16, 3, 1, 3, 3, False, 1, 0),
}
H, W = 9, 11


def stored_f16x2(v):
    return fb.join16(*fb.split16(v))


def unit(kind):
    """A conv unit as the network has them (tests/test_operand_bound.py: unit), its tensors values the f16x2 store can hold"""
    cin, cout, k, stride, pad, dil, identity, a_in, a_out = KINDS[kind]
    rng = np.random.default_rng(1000 * cin + 10 * cout + k)
    h, w = (2 * H, 2 * W) if stride == 2 else (H, W)
    gain = np.logspace(-0.5, 0.5, cin, dtype=np.float32)[rng.permutation(cin)]
    x = rng.standard_normal((1, cin, h, w), dtype=np.float32)
    x = stored_f16x2((x if cin == 3 else np.maximum(x, 0)) * gain[None, :, None, None])
    wt = rng.standard_normal((cout, cin, k, k), dtype=np.float32) / np.float32(np.sqrt(cin * k * k))
    alpha, beta = ob.bn_pair(rng.uniform(0.5, 1.5, cout), 0.3 * rng.standard_normal(cout), 0.2 * rng.standard_normal(cout),
                             rng.uniform(0.25, 1.0, cout))
    res = None
    if identity:
        g = np.logspace(-0.5, 0.5, cout, dtype=np.float32)[rng.permutation(cout)]
        res = stored_f16x2(np.maximum(rng.standard_normal((1, cout, H, W), dtype=np.float32), 0) * g[None, :, None, None])
    return dict(x=x, w=wt, alpha=alpha, beta=beta, res=res, relu=True, stride=stride, pad=pad, dil=dil), a_in, a_out


_CASES = {}


def case(kind):
    """The unit, its float64 reference and its bound: computed once, shared, never written to."""
    if kind not in _CASES:
        torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))
        u, a_in, a_out = unit(kind)
        y_ref, mag, tiny = fb.conv_unit_reference(u["x"], u["w"], "f16x2", u["alpha"], u["beta"], u["res"], u["relu"], u["stride"],
                                                  u["pad"], u["dil"])
        K = u["w"][0].size
        bound = fb.f16x2_unit_bound(y_ref, mag, tiny, u["alpha"], u["beta"], u["res"], K, a_out)
        for a in (y_ref, bound):
            a.setflags(write=False)
        _CASES[kind] = u, a_in, a_out, y_ref, bound
    return _CASES[kind]


def worst(got, y_ref, bound):
    return float((np.abs(got.astype(np.float64) - y_ref) / bound).max())


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_faithful_arithmetic_is_within_the_bound_on_every_element(kind):
    u, a_in, a_out, y_ref, bound = case(kind)
    got = fb.emulate_unit_f16x2(a_in=a_in, a_out=a_out, **u)
    r = worst(got, y_ref, bound)
    print("faithful %-20s K %5d: worst %.3f of the bound" % (kind, u["w"][0].size, r), flush=True)
    assert np.isfinite(got).all() and float(np.abs(y_ref).max()) > 1.0 and (got > 0).mean() > 0.25    # a live tensor
    assert r <= 1.0, (kind, r)


def probe_unit(kind, r):
    """A unit of the gather probe: one-hot rows of round r, the probe's BatchNorm, inputs the f16x2 store can hold"""
    cin, cout, k, stride, pad, dil, identity = KINDS[kind][:7]
    u = topology.ConvUnit("probe", "probe.bn3" if identity else "probe.bn1", cin, cout, k, stride, pad, dil, True, residual=identity)
    rng = np.random.default_rng(77 + r)
    x = stored_f16x2(np.maximum(rng.standard_normal((1, cin, H, W), dtype=np.float32) + np.float32(0.3), 0))
    res = stored_f16x2(np.maximum(rng.standard_normal((1, cout, H, W), dtype=np.float32), 0)) if identity else None
    pos, sg = gp.positions(u, r), gp.signs("fcn_resnet50", 1, u, r)
    wt = np.zeros((cout, cin, k, k), np.float32)
    wt[np.arange(cout), pos % cin, pos // cin // k, pos // cin % k] = sg
    beta = gp.biases("fcn_resnet50", 1, u, r)
    alpha, beta2 = ob.bn_pair(np.full(cout, 2.0 ** gp.log2_gain(u), np.float32), beta, np.zeros(cout, np.float32), np.full(cout, gp.PROBE_VAR))
    assert (alpha == np.float32(2.0 ** gp.log2_gain(u))).all() and np.array_equal(beta2, beta)        # the pair is exact
    return u, pos, sg, beta, dict(x=x, w=wt, alpha=alpha, beta=beta, res=res, relu=True, stride=stride, pad=pad, dil=dil)


# round 3 of the 3x3 unit selects tap (1, 0) in every row (Cin = Cout = 64): the tap the "tap" fault loses; K-step 1 of the
# identity unit holds the positions of rows 32..63
PROBES = [("3x3", 3), ("identity 1x1", 0)]


def probe_verdicts():
    """{fault: the probe's comparison fails on some probe unit}; the faithful arithmetic equals the expected tensor bit for bit"""
    seen = {f: False for f in fb.FAULTS}
    for kind, r in PROBES:
        u, pos, sg, beta, args = probe_unit(kind, r)
        want = gp.expected_unit(args["x"], u, pos, sg, beta, args["res"], "f16x2")
        got = fb.emulate_unit_f16x2(**args)
        assert gp.first_difference(got, want, u, pos, -1) is None, gp.first_difference(got, want, u, pos, -1)
        assert gp.low_piece_share(args["x"]) >= 0.5 and (want != 0).mean() >= 0.25
        step = int(pos[0]) // fb.KSTEP                  # a K-step some row selects
        for f in fb.FAULTS:
            if f == "reader_power" or (f == "tap" and u.k != 3):
                continue                                # every activation power of the probe is 0; a 1x1 kernel has no tap to lose
            bad = fb.emulate_unit_f16x2(fault=f, fault_kstep=step, **args)
            msg = gp.first_difference(bad, want, u, pos, -1)
            seen[f] = seen[f] or msg is not None
            if msg is not None and not any(k == f for k, _ in _MESSAGES):
                _MESSAGES.append((f, msg))
    return seen


_MESSAGES = []


def test_every_seeded_fault_is_caught_by_the_bound_or_by_the_probe():
    table = {}
    for kind in KINDS:
        u, a_in, a_out, y_ref, bound = case(kind)
        for f in fb.FAULTS:
            if (f == "tap" and u["w"].shape[-1] != 3) or (f == "reader_power" and a_in == 0):
                continue
            got = fb.emulate_unit_f16x2(a_in=a_in, a_out=a_out, fault=f, **u)
            table[(f, kind)] = worst(got, y_ref, bound)
    probe = probe_verdicts()
    print("fault          " + "".join("%-22s" % k for k in KINDS) + "probe", flush=True)
    for f in fb.FAULTS:
        cells = "".join("%-22s" % ("-" if (f, k) not in table else "%.3g %s" % (table[(f, k)], "rejected" if table[(f, k)] > 1 else "passes"))
                        for k in KINDS)
        print("%-15s%s%s" % (f, cells, "differs" if probe[f] else "equal"), flush=True)
    for f, msg in _MESSAGES:
        print("probe, %s: %s" % (f, msg), flush=True)
    for f in fb.FAULTS:
        by_bound = [k for k in KINDS if table.get((f, k), 0.0) > 1.0]
        assert by_bound or probe[f], "%s passes the bound on every kind and the probe" % f
    # what each part is for
    for f in ("third", "qx0"):                          # a product of one K-step: the bound sees it up to K of about 150
        assert all(table[(f, k)] > 1.0 for k in ("stem", "identity 1x1")), (f, table)
        assert all(table[(f, k)] <= 1.0 for k in ("1x1", "3x3", "row-step 3x3", "projection")), (f, table)
    for f in ("kstep", "alpha"):
        assert all(table[(f, k)] > 1.0 for k in KINDS if KINDS[k][0] * KINDS[k][2] ** 2 <= 4608), (f, table)
    assert all(table[("reader_power", k)] > 1.0 for k in KINDS if ("reader_power", k) in table)
    assert all(table[("tap", k)] > 1.0 for k in KINDS if ("tap", k) in table)
    assert all(table[("truncate_h1", k)] <= 1.0 for k in KINDS) and probe["truncate_h1"]      # the probe alone sees the store
    assert table[("third", "ASPP 3x3 dilation 3")] <= 1.0 and table[("qx0", "ASPP 3x3 dilation 3")] <= 1.0 and probe["third"]
    assert not probe["qx0"] and not probe["alpha"]                                              # the probe's known limits
    assert probe["kstep"] and probe["tap"]


def test_the_store_holds_what_the_bound_grants_it():
    """split16 against numpy's binary16: 2^-23 relative for |v| >= 2^-12, an absolute 2^-36 below, and the join is exact in f32"""
    rng = np.random.default_rng(5)
    mags = np.exp2(rng.uniform(-30, 15.9, 2_000_000))
    v = (mags * np.where(rng.random(mags.size) < 0.5, -1, 1)).astype(np.float32)
    h0, h1 = fb.split16(v)
    exact = h0.astype(np.float64) + h1.astype(np.float64) * 2.0 ** -11
    joined = fb.join16(h0, h1)
    assert np.array_equal(joined.astype(np.float64), exact)                     # f32-representable, every one
    err = np.abs(exact - v.astype(np.float64))
    big = np.abs(v) >= 2.0 ** -12
    rel, small = float((err[big] / np.abs(v[big])).max()), float(err[~big].max())
    print("split16: worst 2^%.2f relative on |v| >= 2^-12, 2^%.2f absolute below" % (np.log2(rel), np.log2(small)), flush=True)
    assert big.sum() > 10 ** 6 and (~big).sum() > 10 ** 5
    assert rel <= fb.STORE_REL and small <= fb.STORE_ABS
    # truncation: never away from zero, within one f16 ulp
    t = fb.f16_toward_zero(v)
    assert (np.abs(t.astype(np.float32)) <= np.abs(v)).all() and (np.abs(t.astype(np.float64) - h0.astype(np.float64)) <= np.spacing(np.abs(h0)).astype(np.float64)).all()


def _join_f16x2(raw_u8, row_elems, group):
    h = raw_u8.view(np.float16).reshape(-1, row_elems // group, 2, group)
    return h[:, :, 0, :].reshape(-1, row_elems), h[:, :, 1, :].reshape(-1, row_elems)


def test_the_restated_weight_pieces_are_the_packer_s_bit_for_bit(built_lib, sd_np):
    """The f16x2 blob of every conv unit (the layout of include/nbc.h: K-major rows in whole 128-byte K-steps, groups of 32
    elements as [P x 32][Q x 32] -- the stem: taps of 4 --, then scale and shift, every section 256-byte aligned): P, Q and the
    row exponent of f16x2_pieces are the packer's, and the blob's scale is the restated alpha times 2^-k."""
    blob = pack_state_dict(sd_np, "f16x2")
    align = lambda v: (v + 255) // 256 * 256  # noqa: E731
    off, seen = 0, 0
    for u in topology.conv_units():
        if u.bn is None:
            break
        stem = u.cin == 3
        cin_pad, ksteps = (4, 7) if stem else (u.cin, u.k * u.k * u.cin * 4 // 128)
        row = ksteps * 32
        g0, g1 = _join_f16x2(blob[off: off + u.cout * ksteps * 128], row, 4 if stem else 32)
        p, q, k = fb.f16x2_pieces(sd_np[u.name + ".weight"])
        for got, piece in ((g0, p), (g1, q)):
            want = np.zeros((u.cout, row), np.float16)
            khkwci = piece.transpose(0, 2, 3, 1)
            for tap in range(u.k * u.k):
                slot = (tap // u.k) * 8 + tap % u.k if stem else tap
                want[:, slot * cin_pad: slot * cin_pad + u.cin] = khkwci[:, tap // u.k, tap % u.k, :]
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), u.name
        s_off = align(off + u.cout * ksteps * 128)
        t_off = align(s_off + u.cout * 4)
        alpha, beta = ob.bn_pair(*(sd_np[u.bn + key] for key in (".weight", ".bias", ".running_mean", ".running_var")))
        assert np.array_equal(blob[s_off: s_off + u.cout * 4].view(np.uint32), np.ldexp(alpha, (-k).astype(np.int32)).astype(np.float32).view(np.uint32)), u.name
        assert np.array_equal(blob[t_off: t_off + u.cout * 4].view(np.uint32), beta.view(np.uint32)), u.name
        wt, k2, _ = fb.f16x2_weights(sd_np[u.name + ".weight"])
        w64 = sd_np[u.name + ".weight"].astype(np.float64)
        assert np.array_equal(k, k2) and (np.abs(wt - w64).reshape(u.cout, -1).max(1) <= 2.0 ** -23 * np.abs(w64).reshape(u.cout, -1).max(1)).all()
        off = align(t_off + u.cout * 4)
        seen += 1
    assert seen == 54
