# -*- coding: utf-8 -*-
"""Restatements, in numpy, of the gradients of the decoder's glue (csrc/decoder_glue_bwd.hip): the adjoint of the x2 / x4 bilinear
upsample (align_corners=False) and the backward of the prediction head out = conv3x3_p1(relu(x), w) + bias.

Two of each: a literal float64 one (the truth of the tests) and a float32 one in the kernels' stated summation order, with
fma(a, b, c) = float32(float64(a) * float64(b) + float64(c)) -- the product is exact in float64, the sum is rounded twice, which differs
from a fused multiply-add in rare ties only; the float32 restatement is held to the bound, never compared bit for bit.

``fault=`` plants one named mistake; tests/test_decoder_glue_grad.py shows that each is caught.
"""

import numpy as np

UP_FAULTS = ('border_interior', 'no_fold_n1', 'no_fold_n2', 'swap_xy_x4')
HEAD_FAULTS = ('flip_tap', 'mask_ge', 'mask_from_g', 'dw_no_relu', 'drop_range')


# ------------------------------------------------------------------------------------------------ the upsample's adjoint
def adj_row(j, n, S, fault=None, w75=0.75):
    """[(fine index, weight)] of coarse ``j`` on an axis of coarse length ``n``, fine indices ascending: the fine d = S j - S/2 + t,
    t = 0 .. 2 S - 1, with (2 t + 1) / (2 S) for t < S and the mirror image behind; at j = 0 the taps before the map do not exist and
    the S/2 behind them weigh 1 (the clamp of src at 0 folds coarse -1 onto coarse 0); at j = n - 1 the mirror image of that."""
    row = []
    fold = not ((fault == 'no_fold_n1' and n == 1) or (fault == 'no_fold_n2' and n == 2) or fault == 'border_interior')
    for t in range(2 * S):
        d = S * j - S // 2 + t
        if d < 0 or d >= S * n:
            continue
        wt = (2 * t + 1 if t < S else 4 * S - 2 * t - 1) / (2.0 * S)
        if fold and ((j == 0 and t < S) or (j == n - 1 and t >= S)):
            wt = 1.0
        if wt == 0.75:
            wt = w75
        row.append((d, wt))
    return row


def adj_matrix(n, S, fault=None, w75=0.75):
    """[n, S n] float64: row j holds adj_row(j, n, S)."""
    A = np.zeros((n, S * n))
    for j in range(n):
        for d, wt in adj_row(j, n, S, fault, w75):
            A[j, d] = wt
    return A


def upsample64(x, S):
    """The forward by its own rule, float64: src = max((d + 0.5) / S - 0.5, 0), i0 = floor(src), i1 = i0 + (i0 < n - 1)."""
    def mat(n):
        M = np.zeros((S * n, n))
        for d in range(S * n):
            src = max((d + 0.5) / S - 0.5, 0.0)
            i0 = int(np.floor(src))
            i1 = i0 + (1 if i0 < n - 1 else 0)
            M[d, i0] += 1.0 - (src - i0)
            M[d, i1] += src - i0
        return M
    x = np.asarray(x, np.float64)
    return np.matmul(np.matmul(mat(x.shape[2]), x), mat(x.shape[3]).T)


def upsample_adjoint64(g, S, fault=None, w75=0.75):
    """out [N,C,h,w] float64 for g [N,C,S h,S w]: the outer product of the two 1-D rows."""
    g = np.asarray(g, np.float64)
    h, w = g.shape[2] // S, g.shape[3] // S
    Ay, Ax = adj_matrix(h, S, fault, w75), adj_matrix(w, S, fault, w75)
    if fault == 'swap_xy_x4' and S == 4:
        # the 8 x 8 table of a coarse pixel read transposed: tap (ty, tx) weighs row_i[tx] * row_j[ty]
        def by_t(j, n):
            wt = [0.0] * (2 * S)
            for d, v in adj_row(j, n, S):
                wt[d - (S * j - S // 2)] = v
            return wt
        out = np.zeros(g.shape[:2] + (h, w))
        for i in range(h):
            for j in range(w):
                wi, wj = by_t(i, h), by_t(j, w)
                for ty in range(2 * S):
                    for tx in range(2 * S):
                        r, c = S * i - S // 2 + ty, S * j - S // 2 + tx
                        if 0 <= r < S * h and 0 <= c < S * w:
                            out[:, :, i, j] += wi[tx] * wj[ty] * g[:, :, r, c]
        return out
    return np.matmul(np.matmul(Ay, g), Ax.T)                      # out[i][j] = sum_r sum_s Ay[i][r] g[r][s] Ax[j][s]


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def upsample_adjoint32(g, S, w75=0.75):
    """The kernels' order in float32: fine rows ascending; in a row s = fma(wx, g, s) over the fine columns ascending from s = 0; then
    acc = fma(wy, s, acc) from acc = 0."""
    g = np.asarray(g, np.float32)
    N, C, H, W = g.shape
    h, w = H // S, W // S
    out = np.zeros((N, C, h, w), np.float32)
    for i in range(h):
        for j in range(w):
            acc = np.zeros((N, C), np.float32)
            for r, wy in adj_row(i, h, S, w75=w75):
                s = np.zeros((N, C), np.float32)
                for c, wx in adj_row(j, w, S, w75=w75):
                    s = fma32(np.float32(wx), g[:, :, r, c], s)
                acc = fma32(np.float32(wy), s, acc)
            out[:, :, i, j] = acc
    return out


def upsample_bound(g, S):
    """(T + 2) 2^-24 sum w |g| per element, float64: T = 16 (x2) / 64 (x4) additions at most, one rounding each, and two products."""
    T = {2: 16, 4: 64}[S]
    return (T + 2) * 2.0 ** -24 * upsample_adjoint64(np.abs(np.asarray(g, np.float64)), S)


# ------------------------------------------------------------------------------------------------ the prediction head
def _taps(g):
    """G [n, 2, 3, 3, H, W] with G[:, k, ky, kx, y, x] = g[:, k, y - ky + 1, x - kx + 1], zero outside the map."""
    n, K, H, W = g.shape
    pad = np.zeros((n, K, H + 2, W + 2), g.dtype)
    pad[:, :, 1:-1, 1:-1] = g
    G = np.zeros((n, K, 3, 3, H, W), g.dtype)
    for ky in range(3):
        for kx in range(3):
            G[:, :, ky, kx] = pad[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
    return G


def head_grads64(x, w, g, fault=None):
    """(dx [n,C,H,W], dw [2,C,3,3], db [2]) in float64 of out = conv3x3_p1(relu(x), w) + bias for the output gradient g [n,2,H,W]:
    dx = [x > 0] sum_{k,ky,kx} w[k,c,ky,kx] G[k,ky,kx]; dw[k,c,ky,kx] = sum_p relu(x)[p,c] G[k,ky,kx](p); db[k] = sum_p g[k,p].
    A NaN in x: mask 0, and relu(x) = 0."""
    x, w, g = (np.asarray(t, np.float64) for t in (x, w, g))
    G = _taps(g)
    wd = w[:, :, ::-1, :] if fault == 'flip_tap' else w
    with np.errstate(invalid='ignore'):
        mask = (x >= 0) if fault == 'mask_ge' else (x > 0)
        relu = np.where(x > 0, x, 0.0)
    dx = np.einsum('kcab,nkabyx->ncyx', wd, G)
    if fault == 'mask_from_g':
        mask = np.broadcast_to(g[:, :1] > 0, x.shape)
    dx = np.where(mask, dx, 0.0)
    dw = np.einsum('ncyx,nkabyx->kcab', np.nan_to_num(x, nan=0.0) if fault == 'dw_no_relu' else relu, G)
    return dx, dw, g.sum(axis=(0, 2, 3))


def head_plan(pixels, C, ct=32, slots=32, range_min=256, max_ranges=128, target=1024):
    """csrc/decoder_glue_bwd.hip: ph_plan, restated: (channel tiles, ranges, pixels per range)."""
    nct = C // ct
    nr = max(1, min(target // nct, -(-pixels // range_min), max_ranges))
    rl = -(-(-(-pixels // nr)) // slots) * slots
    return nct, -(-pixels // rl), rl


def head_grads32(x, w, g, fault=None, slots=32):
    """The kernels' order in float32.  dx: fma(w, G, dx) from 0 over k, ky, kx.  dw / db: per pixel range (head_plan; pixels in
    linear n, y, x order) slot s walks the pixels begin + s, begin + s + 32, ... with acc = fma(relu(x), G, acc) (db: acc += g), the
    slots are added in slot order, the ranges in range order."""
    x, w, g = (np.asarray(t, np.float32) for t in (x, w, g))
    n, C, H, W = x.shape
    P = n * H * W
    G = _taps(g).transpose(0, 4, 5, 1, 2, 3).reshape(P, 18)                  # [pixel][k, ky, kx]
    X = x.transpose(0, 2, 3, 1).reshape(P, C)
    w18 = w.transpose(0, 2, 3, 1).reshape(18, C)                               # [k, ky, kx][c]
    dx = np.zeros((P, C), np.float32)
    for t in range(18):
        dx = fma32(w18[t][None, :], G[:, t][:, None], dx)
    with np.errstate(invalid='ignore'):
        dx = np.where(X > 0, dx, np.float32(0))
        R = np.where(X > 0, X, np.float32(0))
    _, nranges, RL = head_plan(P, C)
    dw = db = None
    for rg in range(nranges):
        if fault == 'drop_range' and rg == nranges - 1 and nranges > 1:
            continue
        begin, end = rg * RL, min(rg * RL + RL, P)
        acc = np.zeros((slots, 18, C), np.float32)
        accb = np.zeros((slots, 2), np.float32)
        for p0 in range(begin, end, slots):
            m = min(slots, end - p0)
            acc[:m] = fma32(R[p0:p0 + m, None, :], G[p0:p0 + m, :, None], acc[:m])
            accb[:m] = accb[:m] + G[p0:p0 + m][:, [4, 13]]
        part, partb = acc[0], accb[0]
        for s in range(1, slots):
            part = part + acc[s]
            partb = partb + accb[s]
        dw = part if dw is None else dw + part
        db = partb if db is None else db + partb
    dw = dw.reshape(2, 3, 3, C).transpose(0, 3, 1, 2)
    return dx.reshape(n, H, W, C).transpose(0, 3, 1, 2), dw, db


def head_bounds(x, w, g):
    """Per-element bounds in float64: dx 20 2^-24 sum |w| |g|; dw (P + 2) 2^-24 sum |g| relu(x); db (P + 1) 2^-24 sum |g|."""
    x, w, g = (np.asarray(t, np.float64) for t in (x, w, g))
    P = x.shape[0] * x.shape[2] * x.shape[3]
    bx, bw, bb = head_grads64(np.ones_like(x), np.abs(w), np.abs(g))
    _, bw, _ = head_grads64(np.where(x > 0, x, 0.0), np.abs(w), np.abs(g))
    u = 2.0 ** -24
    return 20 * u * bx, (P + 2) * u * bw, (P + 1) * u * bb
