# -*- coding: utf-8 -*-
"""The arithmetic of the validation loss (include/rmnet_hip.h I1, csrc/val_loss.hip, rmnet_amd/losses.py) restated in numpy,
its bounds, and the cases the tests share.

Arithmetic
----------
probs float32 [N,K,H,W], labels uint8 [N,H,W].  A pixel is valid when its label is not ``ignore_index`` (an index outside
0 .. 255 ignores nothing).  A valid pixel is bad when its label is >= K (checked first) or when any of its K probabilities is not
inside [0, 1] (NaN included); bad pixels are counted and left out.  For every other pixel and class c, in fp32:
    fg = (label == c);  e = |fg - p_c|;  key = (unsigned)(e * bins) in [0, bins]        (bin `bins` holds e == 1 alone)
    hist[c][fg][key] += 1;   nll_sum += -log(p_label)
and per class, in float64, with G the foreground count, Fge / Bge the suffix sums over bins >= k and Fgt / Bgt those over bins > k:
    hi = (1/bins) sum_{k<bins} 1 - (G - Fge(k)) / (G + Bge(k))          lo = the same with Fgt, Bgt
A class with G == 0 is skipped.  lovasz = mean over the present classes of (lo + hi) / 2 (0 when none), nll = nll_sum / good
pixels (NaN when none), loss = lovasz + nll.  ``sorted_values`` is the exact thing that lo and hi bracket: per class the float64
sum over the errors in descending order of e_(i) (J_i - J_(i-1)), J_i the Jaccard loss of the i largest errors.

Bounds (u = 2^-53, v = 2^-24)
-----------------------------
EPS, restatement against the float64 sort.  A term 1 - a / b has two roundings and lies in [0, 1]: error <= 2u.  np.sum adds
pairwise: blocks of 128 in 8 accumulators (16 adds deep, 3 to combine), then a binary tree, at most 19 + 13 levels for 2^20 terms
of at most 1, and the division by a power of two is exact: a bracket end is off by at most 34u.  The sorted value
sum_i e_i (J_i - J_(i-1)) = sum_i (e_i - e_(i+1)) J_i (Abel) moves by at most 2u e_1 <= 2u for the error of J, by u for the rounding
of the differences, by u for the products and by at most 22u for the pairwise sum of at most 2^10 terms: 26u.  The mean over at
most 4 classes adds 4u.  EPS = 64u = 7.1e-15 covers all of it.

eps_device(bins), kernel against restatement.  vl_scan gives every lane ceil(bins / 1024) terms to add one after the other, then 6
levels over the lanes and 16 waves one after the other; every partial sum is at most the number of terms added, so after the
division by bins the error is at most (max(bins / 1024, 1) + 22 + 2) u; the restatement's own 34u is added: 1.2e-13 at 2^20 bins.

ref_lovasz_bound(P), the reference's fp32 LovaszLoss against the float64 sort, P pixels per class.  The errors are the same fp32
numbers and sort alike.  Its cumsums of 0 / 1 are exact below 2^24 elements, so intersection and union are exact; J has two fp32
roundings (2v); by the Abel form above that moves the value by at most 2v; the differences J_i - J_(i-1) round once (v in all,
they add up to at most 1); and the fp32 dot of P products, whatever its order, is off by at most P v times the sum of the
products (at most 1) plus v for the products themselves: (P + 4) v per class, and v more for the fp32 mean over classes.
ref_nll_bound: torch's fp32 log (1 ulp allowed, 2v relative) and the fp32 sum of P terms in any order ((P - 1) v relative to the
sum of magnitudes), the division (v): (P + 2) v * mean |log p|.

nll_device_bound: the device's logf is off by at most L_ULP ulps (tests/glue_ref.py: twice the largest error measured on an
MI355X, profiles/r14_a_glue_tests.md), an ulp being at most 2^-23 |log p|; the float64 sum of P terms in any order adds at most
P u times the sum of magnitudes.
"""

import numpy as np

from glue_ref import L_ULP

U = 2.0 ** -53
V = 2.0 ** -24
EPS = 64 * U

FAULTS = ('ge_for_gt', 'clamp_top', 'count_ignored', 'mean_over_all', 'fg_shifted', 'keep_bad', 'drop_frame0')


def eps_device(bins):
    return (max(bins // 1024, 1) + 22 + 2 + 34) * U


def ref_lovasz_bound(P):
    return (P + 5) * V


def ref_nll_bound(P, mean_abs_log):
    return (P + 2) * V * mean_abs_log


def nll_device_bound(logs):
    """Bound on |device nll_sum - float64 nll_sum| for the float64 logs of the counted target probabilities."""
    mag = float(np.abs(logs).sum())
    return L_ULP * 2.0 ** -23 * mag + logs.size * U * mag


def pixel_classes(probs, labels, ignore_index=255, faults=()):
    """(good, bad by label, bad by probability), bool [N,H,W]."""
    K = probs.shape[1]
    lab = labels.astype(np.int64)
    valid = lab != ignore_index if 0 <= ignore_index <= 255 else np.ones(lab.shape, bool)
    if 'count_ignored' in faults:
        valid = np.ones(lab.shape, bool)
    bad_label = valid & (lab >= K)
    with np.errstate(invalid='ignore'):
        inside = ((probs >= 0) & (probs <= 1)).all(axis=1)
    bad_prob = valid & ~bad_label & ~inside
    good = valid & ~bad_label & inside
    if 'keep_bad' in faults:
        good = valid & (lab < K)
    if 'drop_frame0' in faults:
        good = good.copy()
        good[0] = False
    return good, bad_label, bad_prob


def errors(probs, labels, good, faults=()):
    """Per class c: (fg bool [P], e float32 [P]) over the good pixels, in pixel order."""
    K = probs.shape[1]
    p = np.moveaxis(probs, 1, -1)[good]                    # [P, K]
    lab = labels[good].astype(np.int64)
    out = []
    for c in range(K):
        fg = lab == (c + 1 if 'fg_shifted' in faults else c)
        out.append((fg, np.abs(fg.astype(np.float32) - p[:, c]).astype(np.float32)))
    return out


def keys_of(e, bins, faults=()):
    with np.errstate(invalid='ignore', over='ignore'):
        key = (e * np.float32(bins)).astype(np.int64)
    if 'keep_bad' in faults:
        key = np.clip(key, 0, bins)                        # (what a bad probability would be counted as does not matter)
    if 'clamp_top' in faults:
        key = np.minimum(key, bins - 1)
    return key


def histograms(probs, labels, ignore_index=255, bins=1 << 20, faults=()):
    """int64 [K,2,bins+1] (index 0 background, 1 foreground)."""
    good, _, _ = pixel_classes(probs, labels, ignore_index, faults)
    K = probs.shape[1]
    hist = np.zeros((K, 2, bins + 1), np.int64)
    for c, (fg, e) in enumerate(errors(probs, labels, good, faults)):
        key = keys_of(e, bins, faults)
        hist[c, 1] = np.bincount(key[fg], minlength=bins + 1)
        hist[c, 0] = np.bincount(key[~fg], minlength=bins + 1)
    return hist


def brackets(hist, bins, faults=()):
    """float64 [K,3]: G, lo, hi."""
    K = hist.shape[0]
    out = np.zeros((K, 3))
    for c in range(K):
        fge = np.cumsum(hist[c, 1][::-1])[::-1].astype(np.float64)        # over bins >= k, k = 0 .. bins
        bge = np.cumsum(hist[c, 0][::-1])[::-1].astype(np.float64)
        G = fge[0]
        if G == 0:
            continue
        hi = np.sum(1.0 - (G - fge[:bins]) / (G + bge[:bins])) / bins
        if 'ge_for_gt' in faults:
            lo = hi
        else:
            lo = np.sum(1.0 - (G - fge[1:]) / (G + bge[1:])) / bins
        out[c] = G, lo, hi
    return out


def nll_logs(probs, labels, ignore_index=255, faults=()):
    """float64 log of the target probability of every good pixel."""
    good, _, _ = pixel_classes(probs, labels, ignore_index, faults)
    p = np.moveaxis(probs, 1, -1)[good]
    lab = labels[good].astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.log(p[np.arange(lab.size), np.minimum(lab, probs.shape[1] - 1)].astype(np.float64))


def clip_loss(probs, labels, ignore_index=255, bins=1 << 20, faults=()):
    """Everything the C entry returns and what losses.py makes of it."""
    good, bad_label, bad_prob = pixel_classes(probs, labels, ignore_index, faults)
    hist = histograms(probs, labels, ignore_index, bins, faults)
    per_class = brackets(hist, bins, faults)
    present = per_class[:, 0] > 0
    mid = (per_class[:, 1] + per_class[:, 2]) / 2
    if 'mean_over_all' in faults:
        lovasz = float(mid.sum() / len(mid))
    else:
        lovasz = float(mid[present].sum() / present.sum()) if present.any() else 0.0
    logs = nll_logs(probs, labels, ignore_index, faults)
    nll_sum = float(-logs.sum()) if logs.size else 0.0
    n_good = int(good.sum())
    with np.errstate(divide='ignore', invalid='ignore'):
        nll = float(np.float64(nll_sum) / np.float64(n_good))
    return {'hist': hist, 'per_class': per_class, 'present': present, 'lovasz': lovasz, 'nll_sum': nll_sum, 'nll': nll,
            'loss': lovasz + nll, 'counts': np.array([n_good, int(bad_label.sum()), int(bad_prob.sum())], np.int64)}


def sorted_values(probs, labels, ignore_index=255, faults=()):
    """float64 [K,2]: G and the exact Lovasz extension of every class by the sort (0 for an absent class)."""
    good, _, _ = pixel_classes(probs, labels, ignore_index, faults)
    out = np.zeros((probs.shape[1], 2))
    for c, (fg, e) in enumerate(errors(probs, labels, good, faults)):
        G = float(fg.sum())
        if G == 0:
            continue
        order = np.argsort(-e.astype(np.float64), kind='stable')
        es, fs = e[order].astype(np.float64), fg[order].astype(np.float64)
        jac = 1.0 - (G - np.cumsum(fs)) / (G + np.cumsum(1.0 - fs))
        step = jac.copy()
        step[1:] = jac[1:] - jac[:-1]
        out[c] = G, np.sum(es * step)
    return out


def sorted_lovasz(probs, labels, ignore_index=255, faults=()):
    sv = sorted_values(probs, labels, ignore_index, faults)
    present = sv[:, 0] > 0
    if 'mean_over_all' in faults:
        return float(sv[:, 1].sum() / len(sv))
    return float(sv[present, 1].sum() / present.sum()) if present.any() else 0.0


# ------------------------------------------------------------------------------------------------ cases
def softmax_clip(rng, N, K, H, W, peak=4.0, ignore=0.0, n_labels=None):
    """A random clip: soft-max probabilities (``peak`` scales the logits: large = peaked, 0 = flat), labels 0 .. n_labels - 1
    biased towards the arg-max, a share ``ignore`` of the pixels set to 255."""
    z = (rng.standard_normal((N, K, H, W)) * peak).astype(np.float64)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    p = np.clip(p, 0.0, 1.0)
    n_labels = K if n_labels is None else n_labels
    labels = np.where(rng.random((N, H, W)) < 0.7, np.minimum(p.argmax(axis=1), n_labels - 1), rng.integers(0, n_labels, (N, H, W)))
    labels = labels.astype(np.uint8)
    labels[rng.random((N, H, W)) < ignore] = 255
    return p, labels


def grid_clip(rng, N, K, H, W, bins):
    """Every probability a multiple of 1 / bins (bins <= 2^20: exact in fp32, and so is 1 - p), 0 and 1 included."""
    m = rng.integers(0, bins + 1, (N, K, H, W))
    edge = rng.random((N, K, H, W))
    m = np.where(edge < 0.15, 0, np.where(edge > 0.85, bins, m))
    return (m / bins).astype(np.float32), rng.integers(0, K, (N, H, W)).astype(np.uint8)
