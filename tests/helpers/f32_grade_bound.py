"""An f32-grade kernel ("f16x2", "fp32") on the operands it read: the definition in float64 and a bound on every output element,
derived from the roundings the arithmetic performs and from nothing the code under test returned.  Host only (numpy, torch on
the CPU).  The bf16 counterpart is operand_bound.py, whose constants and functions this file uses unchanged.

The reference.  x~ (and the identity) are the tensors the unit's producers stored, as read_activation returns them: pieces
joined, activation power taken off -- exact in f32.  w~ are the weights as the packer holds them: fp32 the checkpoint's; f16x2
(P + Q) 2^-k with k = f16x2_row_exponent(row) (largest |w| 2^k in [2^14, 2^15)), P = f16(w 2^k), Q = f16(w 2^k - P)
(`f16x2_weights`; tests/test_f32_grade_bound.py pins it to the packed blob).  y_ref = act(z alpha + beta + res) with
z = sum w~ x~ in float64, A = sum |w~| |x~|, (alpha, beta) the BatchNorm pair of operand_bound.bn_pair.  The powers of two the
packer folds into the pair (-k + a_out - a_in, a_out) are exact, so the bound is stated on the tensors the network defines.

f16x2, u = 2^-24, a = |alpha| A:

    |y - y_ref| <= 2^-23 |y_ref| + 2^-36 2^-a_out + (1 + 2^-23) [ D + S + C + E ]

  D = 2^-22 (1 + 2^-9) a      the product w x is P X0 + Q X0 + (P 2^-11) X1; the dropped Q X1 2^-11 has |Q| <= 2^-11 |P| and
                              |X1 2^-11| <= 2^-11 |X0|, and |P| |X0| <= (1 + 2^-9) |w~ 2^k| |x~ 2^a_in| (both pieces may lie
                              2^-11 above the joined value: (1 + 2^-11)^2 (1 + 2^-22) < 1 + 2^-9);
  S = 2^-25 |alpha| 2^-k sum_{0 < |P| < 2^-3} |x~|
                              P 2^-11 is formed in f16: exact for |P| >= 2^-3, an f16 subnormal below (half a subnormal ulp:
                              2^-25), times |X1| <= |X0| <= (1 + 2^-11) |x~ 2^a_in| -- the (1 + 2^-11) rides in the slack of the
                              2^-9 above; P = 0 gives an exact 0.  "2^-39 of the row's largest weight" in include/nbc.h;
  C = c (3 K + ceil(K / 256)) u (1 + 2^-9) a
                              the three products of a term are exact in f32 (11 x 11 bits); 3 K additions into one chain
                              and one join of the chain into the running sum every eight 32-channel K-steps (x2_flush):
                              ceil(K / 256) more; the magnitudes summed are those of the pieces, hence (1 + 2^-9); c = 2 is
                              granted, not measured: the matrix pipe's internal rounding is not documented;
  E = 6 u (a + |beta| + |res|)
                              operand_bound.UNIT_ROUNDINGS: the fma, the residual add, four inside the pair;
  2^-23 |y_ref| + 2^-36 2^-a_out
                              the store (split16): the pieces hold a value v to 2^-23 |v| for |v| >= 2^-12 and to an absolute
                              2^-36 below, v = y 2^a_out; (1 + 2^-23) because the computed value is split, not y_ref.
                              tests/test_f32_grade_bound.py checks both figures against numpy's binary16.

fp32:  |y - y_ref| <= c gamma(K + 1 + 2) a + E: each product rounds once (1), K additions, in two levels (2); no store term.

classifier.4 and the ASPP pooling branch follow operand_bound.head_reference / pooled_reference with the precision's store in
place of the bf16 store (`pooled_reference`); classifier.4 writes f32 logits in every precision.

emulate_unit_f16x2 is the kernel's arithmetic on the CPU with seeded faults; tests/test_f32_grade_bound.py uses it to show what
the bound rejects and what only the exact probe (gather_probe.py) sees."""
import numpy as np
import torch
import torch.nn.functional as F

import operand_bound as ob

U = ob.U
ACCUMULATION_FACTOR = ob.ACCUMULATION_FACTOR
PIECE_SLACK = 1.0 + 2.0 ** -9           # |P| |X0| <= (1 + 2^-9) |w~ 2^k| |x~ 2^a_in|
DROPPED = 2.0 ** -22                    # |Q X1 2^-11| <= 2^-22 |P X0|
LOW_SUBNORMAL = 2.0 ** -25              # P 2^-11 below f16's normal range: half a subnormal ulp
STORE_REL = 2.0 ** -23                  # split16 on |v| >= 2^-12
STORE_ABS = 2.0 ** -36                  # and below
JOIN_EVERY = 256                        # channels between two joins of the chain: eight K-steps of 32
KSTEP = 32
FP32_LEVELS = 2
FAULTS = ("third", "qx0", "truncate_h1", "reader_power", "kstep", "alpha", "tap")


def f16x2_row_exponent(rows):
    """k per row of [Cout, K] f32: the largest finite |w| times 2^k lies in [2^14, 2^15); 0 for a row of zeros; clamped to
    [-66, 80] (f16x2_row_exponent of csrc/nbc_net.cpp)."""
    a = np.abs(np.asarray(rows, dtype=np.float32))
    m = np.where(np.isfinite(a), a, np.float32(0)).max(axis=1)
    k = np.where(m > 0, 15 - np.frexp(m)[1], 0)
    return np.clip(k, -66, 80).astype(np.int64)


def f16x2_pieces(w):
    """(P, Q, k) of checkpoint weights [Cout, ...]: float16 arrays of w's shape and int64 [Cout]."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows = w.reshape(w.shape[0], -1)
    k = f16x2_row_exponent(rows)
    s = np.ldexp(rows, k[:, None].astype(np.int32)).astype(np.float32)          # exact
    with np.errstate(over="ignore"):
        p = s.astype(np.float16)
        q = (s - p.astype(np.float32)).astype(np.float16)                       # the difference is exact in f32
    return p.reshape(w.shape), q.reshape(w.shape), k


def f16x2_weights(w):
    """(w~ float64 of w's shape, k, P): w~ = (P + Q) 2^-k."""
    p, q, k = f16x2_pieces(w)
    wt = np.ldexp((p.astype(np.float64) + q.astype(np.float64)).reshape(w.shape[0], -1), -k[:, None].astype(np.int32))
    return wt.reshape(w.shape), k, p


def held_weights(w, precision):
    """(w~ float64, k or None, P or None) as the packer of `precision` holds the checkpoint's weights."""
    if precision == "f16x2":
        return f16x2_weights(w)
    assert precision == "fp32", precision
    return np.asarray(w, dtype=np.float32).astype(np.float64), None, None


def split16(v):
    """float32 -> (h0, h1) float16: h0 = f16(v), h1 = f16((v - h0) 2^11), round to nearest even (split_f16x2)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h0 = v.astype(np.float16)
        h1 = ((v - h0.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return h0, h1


def join16(h0, h1):
    """h0 + h1 2^-11 in float32 (exact for pieces split16 made)."""
    return h0.astype(np.float32) + h1.astype(np.float32) * np.float32(2.0 ** -11)


def f16_toward_zero(v):
    """float32 -> float16 truncated (the fault: a conversion that drops bits instead of rounding)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def _per_channel(v):
    return np.asarray(v, dtype=np.float64).reshape(1, -1, 1, 1)


def conv_unit_reference(x, w, precision, alpha, beta, res, relu, stride, pad, dil, pads=None):
    """x, res: f32 arrays as read back; w: the checkpoint's f32 weights.  Returns y_ref, A = sum |w~| |x~| (both float64) and, for
    f16x2, T = 2^-k sum_{0 < |P| < 2^-3} |x~| (None where no weight is that small, and for fp32).  pads = (before, after): zero
    rows / columns before the top / left and after the bottom / right edge in place of `pad` on every side (the TF-"same" pads of
    the EfficientNet stem)."""
    wt, k, p = held_weights(w, precision)
    xh = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if pads is not None:
        xh, pad = F.pad(xh, (pads[0], pads[1], pads[0], pads[1])), 0
    kw = dict(stride=stride, padding=pad, dilation=dil)
    with torch.no_grad():
        z = F.conv2d(xh.double(), torch.from_numpy(wt), **kw).numpy()
        mag = F.conv2d(xh.abs().double(), torch.from_numpy(np.abs(wt)), **kw).numpy()          # float64, as z: derived, not approximate
        tiny = None
        if p is not None:
            small = (np.abs(p.astype(np.float32)) < 2.0 ** -3) & (p != 0)
            if small.any():
                sel = np.ldexp(small.reshape(small.shape[0], -1).astype(np.float64), -k[:, None].astype(np.int32)).reshape(small.shape)
                tiny = F.conv2d(xh.abs().double(), torch.from_numpy(sel), **kw).numpy()
    y = z * _per_channel(alpha) + _per_channel(beta)
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    return y, mag, tiny


def _epilogue(a, beta, res):
    r = 0.0 if res is None else np.abs(np.asarray(res, dtype=np.float64))
    return ob.UNIT_ROUNDINGS * U * (a + np.abs(_per_channel(beta)) + r)


def f16x2_store(y_ref, a_out):
    return STORE_REL * np.abs(y_ref) + STORE_ABS * 2.0 ** -a_out


def f16x2_unit_bound(y_ref, A, tiny, alpha, beta, res, K, a_out=0, c=ACCUMULATION_FACTOR):
    al = np.abs(_per_channel(alpha))
    a = al * np.asarray(A, dtype=np.float64)
    dropped = DROPPED * PIECE_SLACK * a
    sub = 0.0 if tiny is None else LOW_SUBNORMAL * al * tiny
    acc = c * (3 * K + -(-K // JOIN_EVERY)) * U * PIECE_SLACK * a
    return f16x2_store(y_ref, a_out) + (1.0 + STORE_REL) * (dropped + sub + acc + _epilogue(a, beta, res))


def fp32_unit_bound(y_ref, A, alpha, beta, res, K, c=ACCUMULATION_FACTOR):
    a = np.abs(_per_channel(alpha)) * np.asarray(A, dtype=np.float64)
    return c * ob.gamma(K + 1 + FP32_LEVELS) * a + _epilogue(a, beta, res)


def unit_bound(precision, y_ref, A, tiny, alpha, beta, res, K, a_out=0, c=ACCUMULATION_FACTOR):
    if precision == "f16x2":
        return f16x2_unit_bound(y_ref, A, tiny, alpha, beta, res, K, a_out, c)
    assert precision == "fp32", precision
    return fp32_unit_bound(y_ref, A, alpha, beta, res, K, c)


def pooled_reference(x, w, alpha, beta, precision, a_out=0):
    """operand_bound.pooled_reference with the precision's store: gamma(H W + K) |alpha| A before the pair, the pair's
    roundings, then the f16x2 store or none.  Returns (y_ref, bound), each [N, Cout, 1, 1]."""
    n, k, h, wd = x.shape
    w2 = np.asarray(w, dtype=np.float64).reshape(w.shape[0], k)
    x64 = np.asarray(x, dtype=np.float64)
    al, be = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    z = x64.mean(axis=(2, 3)) @ w2.T
    a = np.abs(x64).mean(axis=(2, 3)) @ np.abs(w2).T * np.abs(al)
    y = np.maximum(z * al + be, 0.0)
    inner = ob.gamma(h * wd + k) * a + (ob.UNIT_ROUNDINGS - ob.RESIDUAL_ROUNDINGS) * U * (a + np.abs(be))
    bound = f16x2_store(y, a_out) + (1.0 + STORE_REL) * inner if precision == "f16x2" else inner
    return y.reshape(n, -1, 1, 1), bound.reshape(n, -1, 1, 1)


def im2col(x, k, stride, pad, dil):
    """x [N, C, H, W] -> ([N, K, L] in the packer's (kh, kw, ci) order, (Ho, Wo))"""
    n, c, h, w = x.shape
    ho = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    cols = F.unfold(torch.from_numpy(np.ascontiguousarray(x)), k, dilation=dil, padding=pad, stride=stride).numpy()
    cols = cols.reshape(n, c, k * k, ho * wo).transpose(0, 2, 1, 3).reshape(n, k * k * c, ho * wo)
    return np.ascontiguousarray(cols), (ho, wo)


def emulate_unit_f16x2(x, w, alpha, beta, res, relu, stride, pad, dil, a_in=0, a_out=0, fault=None, fault_kstep=1):
    """The f16x2 kernel's arithmetic on the CPU, in numpy float32 operation by operation: the stored input 2^a_in x split into
    binary16 pieces, the packer's P and Q, per K-step of 32 channels the products P X0, Q X0, (P 2^-11) X1 -- each exact in f32 --
    added one by one into an f32 chain that joins an f32 running sum every eight K-steps, the f32 fma with the pair (powers of two
    folded in as the packer folds them), the f32 residual add on the stored identity, the ReLU, split16.  Returns the tensor as
    read_activation would: pieces joined, 2^a_out taken off.  Every addition rounds, in one of the orders the matrix pipe may
    take: 3 K + ceil(K / 256) roundings, the count of the bound.  fault (K-step `fault_kstep` where one is named):
      "third"         the product (P 2^-11) X1 left out of one K-step;
      "qx0"           the product Q X0 left out of one K-step;
      "truncate_h1"   the store truncates the low piece instead of rounding it;
      "reader_power"  the launch forgets the 2^-a_in of the tensor it reads (needs a_in != 0);
      "kstep"         one K-step left out (all three products);
      "alpha"         alpha is taken from the neighbouring channel;
      "tap"           pixels of the last column lose the left-hand tap of the middle row of a 3x3 kernel."""
    assert fault is None or fault in FAULTS, fault
    w = np.asarray(w, dtype=np.float32)
    cout, cin, k = w.shape[0], w.shape[1], w.shape[-1]
    p, q, kexp = f16x2_pieces(w)
    order = lambda t: np.ascontiguousarray(t.transpose(0, 2, 3, 1).reshape(cout, -1))  # noqa: E731  [Cout][kh][kw][ci]
    p32, q32 = order(p).astype(np.float32), order(q).astype(np.float32)
    pl32 = (order(p) * np.float16(2.0 ** -11)).astype(np.float32)       # formed in f16, as v_pk_mul_f16 forms it
    x0, x1 = split16(np.ldexp(np.asarray(x, dtype=np.float32), a_in))
    c0, (ho, wo) = im2col(x0.astype(np.float32), k, stride, pad, dil)
    c1, _ = im2col(x1.astype(np.float32), k, stride, pad, dil)
    n, kk, npix = c0.shape
    if fault == "tap":
        assert k == 3
        last = np.arange(npix) % wo == wo - 1
        for cols in (c0, c1):
            cols[:, 3 * cin: 4 * cin, last] = 0.0
    step = KSTEP if cin >= KSTEP else k * cin           # the stem: one kernel row per K-step (its zero pads add nothing)
    total = np.zeros((n, cout, npix), np.float32)
    chain = np.zeros((n, cout, npix), np.float32)
    for t, k0 in enumerate(range(0, kk, step)):
        if t > 0 and t % 8 == 0:
            total += chain
            chain[:] = 0.0
        if fault == "kstep" and t == fault_kstep:
            continue
        for wt_, cols, name in ((p32, c0, "px0"), (q32, c0, "qx0"), (pl32, c1, "third")):
            if fault == name and t == fault_kstep:
                continue
            for i in range(k0, min(k0 + step, kk)):
                chain += wt_[None, :, i, None] * cols[:, None, i, :]       # an exact product, one rounded addition
    total += chain
    assert total.dtype == np.float32
    al, be = np.asarray(alpha, dtype=np.float32), np.asarray(beta, dtype=np.float32)
    if fault == "alpha":
        al = np.roll(al, 1)
    e = -kexp + a_out - (0 if fault == "reader_power" else a_in)
    scale = np.ldexp(al, e.astype(np.int32)).astype(np.float32)
    shift = np.ldexp(be, a_out).astype(np.float32)
    # fma: the product of two f32 values is exact in float64; the sum is rounded to float64, then to f32
    v = (total.astype(np.float64) * scale.reshape(1, -1, 1) + shift.reshape(1, -1, 1)).astype(np.float32).reshape(n, cout, ho, wo)
    if res is not None:
        v = v + np.ldexp(np.asarray(res, dtype=np.float32), a_out)
    if relu:
        v = np.maximum(v, np.float32(0.0))
    assert v.dtype == np.float32
    h0, h1 = split16(v)
    if fault == "truncate_h1":
        h1 = f16_toward_zero((v - h0.astype(np.float32)) * np.float32(2048))
    return np.ldexp(join16(h0, h1), -a_out).astype(np.float32)
