# -*- coding: utf-8 -*-
"""The gradient of the training loss lovasz + nll (core/train.py:180) with respect to the probabilities, restated twice in numpy,
with the bounds and the cases that tests/test_loss_grad.py shares.  Pixel classes, errors, keys and histograms are those of
tests/val_loss_ref.py.

literal(...)     float64.  The reference's loss and autograd through it: per present class the errors e = |fg - p_c| sorted in
                 descending order (a stable sort: ties keep the pixel order), the Jaccard index J_i of the i largest, the steps
                 J_i - J_(i-1) as constants (the reference detaches the permutation and computes them from the labels), so
                 dL_c / dp = s * step with s = -1 (foreground), +1 (background), 0 where e == 0 (torch's abs); the mean over the
                 present classes; and -1 / (p_label * n_good) on the label's channel.  Ignored and bad pixels get 0.
table_grad(...)  the arithmetic of csrc/val_loss_bwd.hip, roundings included (include/rmnet_hip.h I2).  From hist[c][fg][k], with
                 G the foreground count, F> / B> the counts of the bins above k and F>= / B>= of the bins at or above k, in float64
                 and rounded once to float32:
                     g_fg = (1 / (G + B>) + 1 / (G + B>=)) / 2        g_bg = (G - (F> + F>=) / 2) / ((G + B>)(G + B>=))
                 (G + B, F> + F>= and its half are exact; each reciprocal, their sum, the product and the quotient round once); 0
                 for an absent class.  Then in fp32, one rounding per operation:
                     grad = (s * g[key]) * fl32(1.0 / n_present)      [+ fl32(-1.0 / (float64(p) * float64(n_good))) where c == label]
bracket(...)     for every element the interval [g_lo, g_hi] that holds the sort's weight under ANY order of the tied pixels (tied:
                 equal rank values, the errors themselves or their keys): the weights 1 / (G + B) and (G - F) / ((G + B)(G + B + 1))
                 fall as F and B grow, a foreground pixel has B> <= B <= B>=, a background one F> <= F <= F>= and
                 B> <= B <= B>= - 1 (itself is one of B>=):
                     foreground  g_hi = 1 / (G + B>),                          g_lo = 1 / (G + B>=)
                     background  g_hi = (G - F>) / ((G + B>)(G + B> + 1)),     g_lo = (G - F>=) / ((G + B>= - 1)(G + B>=))

Bounds (u = 2^-53, v = 2^-24)
-----------------------------
EPS = 64 u (val_loss_ref.py) covers a float64 weight: at most six roundings of quantities of at most 1.
table_bound, the fp32 gradient of table_grad against the same formulas in float64: the table entry rounds once (v |g|), the
product with fl32(1 / n_present) twice more (the reciprocal's rounding and the product's), the NLL term once, the sum once:
    3 v |w| + v |t| + v |w + t| <= 4 v (|w| + |t|)        with w the Lovasz part and t the NLL part of the element.
ref_grad_bound, the reference's fp32 backward against the float64 literal gradient.  Its cumsums of 0 / 1 are exact, a Jaccard
value has two fp32 roundings (2 v absolute, J <= 1) and the difference of two neighbours rounds once: a step is off by at most
5 v.  The backward of the mean gives fl32(1 / n), the backward of the dot multiplies: two more roundings, 2 v |step| / n <= 2 v / n.
The NLL part is fl32(fl32(-1 / n_good) / p): 2 v |t|.  The two parts meet in one fp32 add, v |w + t|.  torch_route_bound:
the route under test computes both parts in float64, autograd rounds each to fp32 where it re-enters the fp32 probabilities and
adds the two in fp32: v |w| + v |t| + v |w + t| <= 2 v (|w| + |t|), plus EPS for the float64 arithmetic.  Together:
    7 v / n_present + 2 v |t| + 3 v (|w| + |t|) + EPS.
"""

import numpy as np

import val_loss_ref as vr

U, V, EPS = vr.U, vr.V, vr.EPS

FAULTS = ('ge_for_gt_f', 'ge_for_gt_b', 'f_for_b', 'no_sign', 'sign_at_zero', 'mean_over_all', 'n_valid', 'nll_wrong_channel',
          'bad_not_zeroed', 'top_has_width')


def table_bound(w, t):
    t = np.where(np.isfinite(t), np.abs(t), 0.0)
    return 4 * V * (np.abs(w) + t)


def ref_grad_bound(w, t, n_present):
    t = np.where(np.isfinite(t), np.abs(t), 0.0)
    return 7 * V / max(n_present, 1) + 2 * V * t + 3 * V * (np.abs(w) + t) + EPS


def torch_route_bound(w, t):
    t = np.where(np.isfinite(t), np.abs(t), 0.0)
    return 2 * V * (np.abs(w) + t) + EPS


def _scatter(per_pixel, good, shape):
    """[P, K] over the good pixels -> [N,K,H,W], 0 elsewhere."""
    N, K, H, W = shape
    out = np.zeros((N, H, W, K), per_pixel.dtype)
    out[good] = per_pixel
    return np.ascontiguousarray(np.moveaxis(out, -1, 1))


def nll_term(probs, labels, good):
    """float64 [P, K] over the good pixels: -1 / (p_label * n_good) on the label's channel."""
    p = np.moveaxis(probs, 1, -1)[good].astype(np.float64)
    lab = labels[good].astype(np.int64)
    t = np.zeros(p.shape)
    rows = np.arange(lab.size)
    with np.errstate(divide='ignore'):
        t[rows, lab] = -1.0 / (p[rows, lab] * np.float64(lab.size))
    return t


# ------------------------------------------------------------------------------------------------ the literal restatement
def literal(probs, labels, ignore_index=255):
    """{'loss', 'lovasz', 'nll' float64; 'grad', 'w', 't' float64 [N,K,H,W] (grad = w + t); 'n_present', 'n_good'}."""
    good, _, _ = vr.pixel_classes(probs, labels, ignore_index)
    K, P = probs.shape[1], int(good.sum())
    weights = np.zeros((P, K))
    values = []
    for c, (fg, e) in enumerate(vr.errors(probs, labels, good)):
        G = float(fg.sum())
        if G == 0:
            continue
        e = e.astype(np.float64)
        order = np.argsort(-e, kind='stable')
        fs = fg[order].astype(np.float64)
        jac = 1.0 - (G - np.cumsum(fs)) / (G + np.cumsum(1.0 - fs))
        step = jac.copy()
        step[1:] = jac[1:] - jac[:-1]
        values.append(float(np.sum(e[order] * step)))
        sign = np.where(e[order] == 0, 0.0, np.where(fg[order], -1.0, 1.0))
        weights[order, c] = sign * step
    n_present = len(values)
    w = weights / max(n_present, 1)
    t = nll_term(probs, labels, good)
    lovasz = sum(values) / n_present if n_present else 0.0
    logs = vr.nll_logs(probs, labels, ignore_index)
    with np.errstate(divide='ignore', invalid='ignore'):
        nll = float(np.float64(-logs.sum() if logs.size else 0.0) / np.float64(P))
    return {'loss': lovasz + nll, 'lovasz': lovasz, 'nll': nll, 'grad': _scatter(w + t, good, probs.shape), 'w': _scatter(w, good, probs.shape),
            't': _scatter(t, good, probs.shape), 'n_present': n_present, 'n_good': P}


# ------------------------------------------------------------------------------------------------ the table restatement
def suffix_counts(h):
    """(over bins > k, over bins >= k) of one histogram row, float64 (exact integers)."""
    ge = np.cumsum(h[::-1])[::-1].astype(np.float64)
    return np.concatenate([ge[1:], [0.0]]), ge


def tables_of(hist, faults=()):
    """float64 [K,2,bins+1] (index 0 g_bg, 1 g_fg) and G [K]: the formulas of the head, every operation rounded once."""
    K = hist.shape[0]
    out = np.zeros(hist.shape, np.float64)
    Gs = np.zeros(K)
    for c in range(K):
        fgt, fge = suffix_counts(hist[c, 1])
        bgt, bge = suffix_counts(hist[c, 0])
        G = fge[0]
        Gs[c] = G
        if G == 0:
            continue
        if 'f_for_b' in faults:
            fgt, fge, bgt, bge = bgt, bge, fgt, fge
        if 'ge_for_gt_f' in faults:
            fgt = fge
        if 'ge_for_gt_b' in faults:
            bgt = bge
        a, b = G + bgt, G + bge
        out[c, 1] = (1.0 / a + 1.0 / b) * 0.5
        out[c, 0] = (G - (fgt + fge) * 0.5) / (a * b)
    return out, Gs


def table_grad(probs, labels, ignore_index=255, bins=16, faults=()):
    """{'tables' float32 [K,2,bins+1], 'tables64', 'grad' float32 [N,K,H,W] (the kernel's bits), 'w64', 't64' float64 [N,K,H,W]
    (the two parts before any fp32 rounding), 'keys' int64 [P,K], 'fg' bool [P,K], 'good', 'hist', 'n_present', 'n_good'}."""
    good, bad_label, bad_prob = vr.pixel_classes(probs, labels, ignore_index)
    key_faults = ('clamp_top',) if 'top_has_width' in faults else ()
    hist = vr.histograms(probs, labels, ignore_index, bins, key_faults)
    t64, Gs = tables_of(hist, faults)
    t32 = t64.astype(np.float32)
    K, P = probs.shape[1], int(good.sum())
    n_present = int((Gs > 0).sum())
    n_for_nll = int((good | bad_label | bad_prob).sum()) if 'n_valid' in faults else P
    inv = np.float32(1.0 / np.float64(K if 'mean_over_all' in faults else max(n_present, 1))) if n_present else np.float32(0)
    keys = np.zeros((P, K), np.int64)
    fgs = np.zeros((P, K), bool)
    w32 = np.zeros((P, K), np.float32)
    w64 = np.zeros((P, K))
    for c, (fg, e) in enumerate(vr.errors(probs, labels, good)):
        key = vr.keys_of(e, bins, key_faults)
        keys[:, c], fgs[:, c] = key, fg
        s = np.where(fg, -1.0, 1.0)
        if 'no_sign' in faults:
            s = np.ones(P)
        if 'sign_at_zero' not in faults:
            s = np.where(e == 0, 0.0, s)
        kind = fg.astype(np.int64)
        w32[:, c] = (s.astype(np.float32) * t32[c, kind, key]) * inv
        w64[:, c] = s * t64[c, kind, key] / max(n_present, 1)
    p = np.moveaxis(probs, 1, -1)[good]
    lab = labels[good].astype(np.int64)
    rows = np.arange(P)
    with np.errstate(divide='ignore', over='ignore'):
        term = (-1.0 / (p[rows, lab].astype(np.float64) * np.float64(n_for_nll))).astype(np.float32)
    grad = w32.copy()
    at = (lab + 1) % K if 'nll_wrong_channel' in faults else lab
    grad[rows, at] = w32[rows, at] + term
    out = _scatter(grad, good, probs.shape)
    if 'bad_not_zeroed' in faults:                          # a bad pixel keeps a Lovasz part in the channels that are not its label's
        bad = bad_label | bad_prob
        with np.errstate(invalid='ignore'):
            pb = np.nan_to_num(np.moveaxis(probs, 1, -1)[bad], nan=0.5).clip(0, 1)
        leak = np.zeros(pb.shape, np.float32)
        for c in range(K):
            leak[:, c] = t32[c, 0, vr.keys_of(pb[:, c], bins)] * inv
        tmp = np.moveaxis(out, 1, -1).copy()
        tmp[bad] = leak
        out = np.ascontiguousarray(np.moveaxis(tmp, -1, 1))
    return {'tables': t32, 'tables64': t64, 'grad': out, 'w64': _scatter(w64, good, probs.shape),
            't64': _scatter(nll_term(probs, labels, good), good, probs.shape), 'keys': keys, 'fg': fgs, 'good': good, 'hist': hist,
            'n_present': n_present, 'n_good': P}


# ------------------------------------------------------------------------------------------------ the bracket
def bracket(rank, fg):
    """rank [P] (errors or keys), fg bool [P] -> (g_lo, g_hi) float64 [P] of one present class, whatever the order of the ties."""
    rank = np.asarray(rank, np.float64)
    gt = rank[None, :] > rank[:, None]                      # [i, j]: pixel j ranks strictly before pixel i
    ge = rank[None, :] >= rank[:, None]
    f_gt, f_ge = (gt & fg[None, :]).sum(1).astype(np.float64), (ge & fg[None, :]).sum(1).astype(np.float64)
    b_gt, b_ge = (gt & ~fg[None, :]).sum(1).astype(np.float64), (ge & ~fg[None, :]).sum(1).astype(np.float64)
    G = float(fg.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        hi = np.where(fg, 1.0 / (G + b_gt), (G - f_gt) / ((G + b_gt) * (G + b_gt + 1)))
        lo = np.where(fg, 1.0 / (G + b_ge), (G - f_ge) / ((G + b_ge - 1) * (G + b_ge)))
    return lo, hi


def grad_bracket(probs, labels, ignore_index=255, bins=None):
    """(lo, hi) float64 [N,K,H,W] of the Lovasz part of the gradient, sign and 1 / n_present applied (lo <= hi), ties by equal
    errors (bins None) or by equal keys; 0 for absent classes, e == 0 and the pixels left out."""
    good, _, _ = vr.pixel_classes(probs, labels, ignore_index)
    K, P = probs.shape[1], int(good.sum())
    lo, hi = np.zeros((P, K)), np.zeros((P, K))
    n_present = 0
    for c, (fg, e) in enumerate(vr.errors(probs, labels, good)):
        if not fg.any():
            continue
        n_present += 1
        g_lo, g_hi = bracket(e if bins is None else vr.keys_of(e, bins), fg)
        zero = e == 0
        lo[:, c] = np.where(zero, 0.0, np.where(fg, -g_hi, g_lo))
        hi[:, c] = np.where(zero, 0.0, np.where(fg, -g_lo, g_hi))
    n = max(n_present, 1)
    return _scatter(lo / n, good, probs.shape), _scatter(hi / n, good, probs.shape)


# ------------------------------------------------------------------------------------------------ cases
def distinct_clip(rng, N, K, H, W, bins, ignore=0.0):
    """Errors constructed, not probabilities: per class the P errors are P different multiples m / bins (bins <= 2^20: m / bins and
    1 - m / bins are exact in fp32), so no bin of a class holds two pixels; p = 1 - e on the label's channel, e elsewhere.  0 and
    `bins` are among the multiples when P allows, so e == 0 and e == 1 occur."""
    P = N * H * W
    assert P <= bins + 1 and bins <= 1 << 20
    labels = rng.integers(0, K, (N, H, W)).astype(np.uint8)
    probs = np.zeros((N, K, H, W), np.float32)
    ends = np.zeros((N, H, W), bool)                        # the pixels that hold an error of 0 or 1 are never ignored
    for c in range(K):
        m = rng.permutation(bins + 1)[:P]
        if P >= 4:
            for slot, end in ((0, 0), (1, bins)):
                if end not in m:
                    m[slot] = end                           # (not among the others: still all different)
        m = rng.permutation(m).reshape(N, H, W)
        e = (m / bins).astype(np.float32)
        ends |= (m == 0) | (m == bins)
        probs[:, c] = np.where(labels == c, np.float32(1) - e, e)
    labels[(rng.random((N, H, W)) < ignore) & ~ends] = 255
    return probs, labels


def lds_window(K, bins):
    """(LB, HB) of csrc/val_loss_parts.h, lds_bins: the table entries [0, LB) and [bins + 1 - HB, bins] are staged in LDS."""
    s = 1
    while 2 * s * 2 * K <= 15872:
        s *= 2
    return (bins + 1, 0) if bins + 1 <= s else (s // 2, s // 2)
