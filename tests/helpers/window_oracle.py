"""A numpy restatement of the crop windows (include/nbc.h: nbc_window_grid, nbc_window_views, nbc_window_merge; DESIGN.md
3.18), written from the definition alone: the grid of an axis, the reflection fill, the window-major stack, the tent weights and
the weighted f32 mean in ascending window order -- one multiply and one add per window, one division by the exact weight sum."""
import numpy as np

CELL = 8
TENT, UNIFORM = 0, 1


def check_rules(S, T):
    assert S % 8 == 0 and 32 <= S <= 2048, S
    assert T % 8 == 0 and 8 <= T <= S <= 8 * T, (S, T)


def grid(L, S, T):
    """One axis of length L >= 8: (L8, E, offsets)."""
    check_rules(S, T)
    assert L >= 8
    L8 = 8 * -(-L // 8)
    E = min(S, L8)
    if L8 <= S:
        return L8, E, [0]
    offsets, k = [], 0
    while k * T + S < L8:
        offsets.append(k * T)
        k += 1
    offsets.append(L8 - S)
    return L8, E, offsets


def reflect_index(i, L):
    """The source index of position i of the padded axis."""
    return i if i < L else 2 * (L - 1) - i


def fill(a, row_axis, col_axis):
    """The frame padded to multiples of 8 by reflection, index by index."""
    a = np.asarray(a)
    H, W = a.shape[row_axis], a.shape[col_axis]
    rows = [reflect_index(i, H) for i in range(8 * -(-H // 8))]
    cols = [reflect_index(i, W) for i in range(8 * -(-W // 8))]
    return np.take(np.take(a, rows, axis=row_axis), cols, axis=col_axis)


def stack(x, S, T):
    """x: uint8 [N,H,W,3] or float32 [N,3,H,W] -> the stack [K*N, ...] of E_y x E_x windows, entry k * N + i = window k of image
    i, k = r * n_x + c."""
    x = np.asarray(x)
    ra, ca = (1, 2) if x.dtype == np.uint8 else (2, 3)
    _, ey, oys = grid(x.shape[ra], S, T)
    _, ex, oxs = grid(x.shape[ca], S, T)
    p = fill(x, ra, ca)
    out = []
    for oy in oys:
        for ox in oxs:
            sl = [slice(None)] * 4
            sl[ra], sl[ca] = slice(oy, oy + ey), slice(ox, ox + ex)
            out.append(p[tuple(sl)])
    return np.ascontiguousarray(np.concatenate(out))


def axis_weights(L, S, T, k, blend=TENT):
    """The per-axis weights int64 [e] of window k of an axis."""
    L8, E, offsets = grid(L, S, T)
    e = E // 8
    if blend == UNIFORM:
        return np.ones(e, dtype=np.int64)
    cap = max(1, e // 2)
    w = np.full(e, cap, dtype=np.int64)
    j = np.arange(e)
    if offsets[k] > 0:
        w = np.minimum(w, j + 1)
    if offsets[k] + E < L8:
        w = np.minimum(w, e - j)
    return w


def merge(lowres_windows, n, H, W, S, T, blend=TENT, return_cover=False):
    """float32 [K*N,3,e_y,e_x] -> float32 [N,3,h,w]: the window's own bits where one window covers a cell, else acc = f32(w_0) *
    v_0, acc = acc + f32(w_k) * v_k in ascending k (each operation rounded to f32), m = acc / f32(sum of w_k)."""
    L8y, Ey, oys = grid(H, S, T)
    L8x, Ex, oxs = grid(W, S, T)
    h, w, ey, ex = L8y // 8, L8x // 8, Ey // 8, Ex // 8
    v = np.asarray(lowres_windows, dtype=np.float32).reshape(len(oys) * len(oxs), n, 3, ey, ex)
    acc = np.zeros((n, 3, h, w), dtype=np.float32)
    first = np.zeros((n, 3, h, w), dtype=np.float32)
    wsum = np.zeros((h, w), dtype=np.int64)
    cover = np.zeros((h, w), dtype=np.int64)
    with np.errstate(all="ignore"):                  # inf - inf and overflow are part of the definition: NaN and inf
        for r, oy in enumerate(oys):
            wy = axis_weights(H, S, T, r, blend)
            for c, ox in enumerate(oxs):
                wx = axis_weights(W, S, T, c, blend)
                w2 = wy[:, None] * wx[None, :]
                ys, xs = slice(oy // 8, oy // 8 + ey), slice(ox // 8, ox // 8 + ex)
                vk = v[r * len(oxs) + c]
                prod = (w2.astype(np.float32)[None, None] * vk).astype(np.float32)
                fresh = (cover[ys, xs] == 0)[None, None]
                acc[:, :, ys, xs] = np.where(fresh, prod, (acc[:, :, ys, xs] + prod).astype(np.float32))
                first[:, :, ys, xs] = np.where(fresh, vk, first[:, :, ys, xs])
                wsum[ys, xs] += w2
                cover[ys, xs] += 1
        assert cover.min() >= 1 and wsum.min() >= 1 and wsum.max() < 2 ** 24
        m = np.where((cover == 1)[None, None], first, (acc / wsum.astype(np.float32)[None, None]).astype(np.float32))
    m = np.ascontiguousarray(m.astype(np.float32))
    return (m, cover) if return_cover else m
