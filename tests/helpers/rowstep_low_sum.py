"""The f16x2 arithmetic of the row-step 3x3 kernel (csrc/conv3x3_rows.hip, x2_products_low / x2_join_low of csrc/f16x2_mma.hpp) on
the CPU, in numpy float32 operation by operation.  Host only.

It differs from f32_grade_bound.emulate_unit_f16x2, the generic kernel's arithmetic, in two things:

  the K order   (channel block, kh, kw): K-step t = (cb 3 + kh) 3 + kw reads the 32 channels of block cb under tap (kh, kw); the
                generic kernel walks (kh, kw, channel block);
  the low sum   per K-step the products P X0 and Q X0 go into the chain, which joins the running sum in front of every eighth
                K-step; the third product is P X1 with P AS STORED, into a sum of its own that no flush touches and that joins
                once behind the K loop: sum = fma(low, 2^-11, sum), one rounding.  P 2^-11 is never formed, so a weight with
                0 < |P| < 2^-3 passes through no f16 subnormal.

Roundings per output: 2 K in the chain, ceil(K / 256) joins, K in `low` at 2^-11 of the chain's scale, one fma -- fewer than the
3 K + ceil(K / 256) the bound of f32_grade_bound.py counts at full scale.  Every product is exact in f32 (11 x 11 bits) and every
addition rounds, in one of the orders the matrix pipe may take."""
import numpy as np

import f32_grade_bound as fb

KSTEP = fb.KSTEP
LOW_SCALE = 2.0 ** -11


def kstep_indices(cin, k=3):
    """per K-step of the row-step order, the K positions (packer order: (kh k + kw) Cin + ci) of its 32 channels"""
    assert cin % KSTEP == 0
    return [(kh * k + kw) * cin + cb * KSTEP + np.arange(KSTEP) for cb in range(cin // KSTEP) for kh in range(k) for kw in range(k)]


def emulate_unit(x, w, alpha, beta, relu, dil, a_in=0, a_out=0):
    """A 3x3 stride-1 unit (pad = dil, no identity) as the row-step kernel computes it.  x: the stored input as read_activation
    returns it; w: the checkpoint's f32 weights [Cout, Cin, 3, 3].  Returns the tensor as read_activation would."""
    w = np.asarray(w, dtype=np.float32)
    cout, cin, k = w.shape[0], w.shape[1], w.shape[-1]
    assert k == 3
    p, q, kexp = fb.f16x2_pieces(w)
    order = lambda t: np.ascontiguousarray(t.transpose(0, 2, 3, 1).reshape(cout, -1))  # noqa: E731  [Cout][kh][kw][ci]
    p32, q32 = order(p).astype(np.float32), order(q).astype(np.float32)
    x0, x1 = fb.split16(np.ldexp(np.asarray(x, dtype=np.float32), a_in))
    c0, (ho, wo) = fb.im2col(x0.astype(np.float32), k, 1, dil, dil)
    c1, _ = fb.im2col(x1.astype(np.float32), k, 1, dil, dil)
    n, kk, npix = c0.shape
    total = np.zeros((n, cout, npix), np.float32)
    chain = np.zeros((n, cout, npix), np.float32)
    low = np.zeros((n, cout, npix), np.float32)
    for t, idx in enumerate(kstep_indices(cin, k)):
        if t > 0 and t % 8 == 0:                          # x2_flush: the chain alone
            total += chain
            chain[:] = 0.0
        for i in idx:
            chain += p32[None, :, i, None] * c0[:, None, i, :]
        for i in idx:
            chain += q32[None, :, i, None] * c0[:, None, i, :]
        for i in idx:
            low += p32[None, :, i, None] * c1[:, None, i, :]           # P as stored: the product is exact
    total += chain                                                       # x2_join<false>
    # x2_join_low: one fma.  low 2^-11 is exact in float64; the sum is rounded to float64, then to f32
    total = (low.astype(np.float64) * LOW_SCALE + total.astype(np.float64)).astype(np.float32)
    assert total.dtype == np.float32 and low.dtype == np.float32 and chain.dtype == np.float32
    al, be = np.asarray(alpha, dtype=np.float32), np.asarray(beta, dtype=np.float32)
    scale = np.ldexp(al, (-kexp + a_out - a_in).astype(np.int32)).astype(np.float32)
    shift = np.ldexp(be, a_out).astype(np.float32)
    v = (total.astype(np.float64) * scale.reshape(1, -1, 1) + shift.reshape(1, -1, 1)).astype(np.float32).reshape(n, cout, ho, wo)
    if relu:
        v = np.maximum(v, np.float32(0.0))
    assert v.dtype == np.float32
    return np.ldexp(fb.join16(*fb.split16(v)), -a_out).astype(np.float32)
