# -*- coding: utf-8 -*-
"""Plain numpy restatement of the reference's boundary measure F, line for line against utils/metrics.py (the reference's own file
needs ``np.bool`` and skimage and cannot be imported on a current stack).  No scipy: the dilation is a loop over the disk's offsets.

The ``fault`` arguments plant one deliberate error each; tests/test_boundary_f.py asserts that every one of them changes a count
on its cases, i.e. that the cases can tell the right statement from the wrong ones."""

import numpy as np

FAULTS = ('square', 'wrap', 'edge', 'mask', 'swap')


def seg2bmap(seg, fault=None):
    """utils/metrics.py:186-216 with width / height unset (so bmap = b, :215-216)."""
    seg = np.asarray(seg).astype(bool)                 # :186-187
    assert np.atleast_3d(seg).shape[2] == 1            # :189
    e = np.zeros_like(seg)                             # :202
    s = np.zeros_like(seg)                             # :203
    se = np.zeros_like(seg)                            # :204
    e[:, :-1] = seg[:, 1:]                             # :206
    s[:-1, :] = seg[1:, :]                             # :207
    se[:-1, :-1] = seg[1:, 1:]                         # :208
    b = seg ^ e | seg ^ s | seg ^ se                   # :210
    if fault == 'edge':                                # planted: the last row / column keep the zero padding's boundary
        return b
    b[-1, :] = seg[-1, :] ^ e[-1, :]                   # :211
    b[:, -1] = seg[:, -1] ^ s[:, -1]                   # :212
    b[-1, -1] = 0                                      # :213
    return b


def disk(radius):
    """skimage.morphology.disk: every offset with dx^2 + dy^2 <= radius^2, as a uint8 [2r+1, 2r+1] array."""
    radius = int(radius)
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=np.uint8)


def binary_dilation(b, footprint, fault=None):
    """skimage.morphology.binary_dilation = scipy.ndimage.binary_dilation(b, structure=footprint), border value 0: out[y, x] is set
    when b[y + dy, x + dx] is set for some offset of the (symmetric, centred) footprint; pixels outside the image are 0."""
    b = np.asarray(b).astype(bool)
    H, W = b.shape
    r = footprint.shape[0] // 2
    out = np.zeros_like(b)
    if not b.any():                                    # (nothing to spread: saves the loop for the objects a frame does not hold)
        return out
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if not footprint[dy + r, dx + r]:
                continue
            if fault == 'wrap':                        # planted: a row's end continues in the next row (and the last in the first)
                out |= np.roll(b.reshape(-1), -(dy * W + dx)).reshape(H, W)
                continue
            if abs(dy) >= H or abs(dx) >= W:
                continue
            # out[y, x] |= b[y + dy, x + dx] wherever both are inside
            out[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] |= b[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return out


def f_counts(foreground_mask, gt_mask, radius, fault=None):
    """(n_fg, n_gt, fg_match, gt_match) of utils/metrics.py:137-152 for one pair of binary masks."""
    fg_boundary = seg2bmap(foreground_mask, fault)     # :138
    gt_boundary = seg2bmap(gt_mask, fault)             # :139
    foot = disk(radius)
    if fault == 'square':                              # planted: the whole (2r+1)^2 square
        foot = np.ones_like(foot)
    fg_src, gt_src = fg_boundary, gt_boundary
    if fault == 'mask':                                # planted: the mask is dilated, not its boundary
        fg_src, gt_src = np.asarray(foreground_mask).astype(bool), np.asarray(gt_mask).astype(bool)
    fg_dil = binary_dilation(fg_src, foot, fault)      # :141-142
    gt_dil = binary_dilation(gt_src, foot, fault)      # :143-144
    gt_match = gt_boundary * fg_dil                    # :147
    fg_match = fg_boundary * gt_dil                    # :148
    n_fg = np.sum(fg_boundary)                         # :151
    n_gt = np.sum(gt_boundary)                         # :152
    if fault == 'swap':                                # planted: the two intersections change places
        fg_match, gt_match = gt_match, fg_match
    return int(n_fg), int(n_gt), int(np.sum(fg_match)), int(np.sum(gt_match))


def f_from_counts(n_fg, n_gt, fg_match, gt_match):
    """utils/metrics.py:155-169."""
    if n_fg == 0 and n_gt > 0:                         # :155-157
        precision = 1
        recall = 0
    elif n_fg > 0 and n_gt == 0:                       # :158-160
        precision = 0
        recall = 1
    elif n_fg == 0 and n_gt == 0:                      # :161-163
        precision = 1
        recall = 1
    else:
        precision = fg_match / float(n_fg)             # :165
        recall = gt_match / float(n_gt)                # :166
    return 2 * precision * recall / (precision + recall) if precision + recall != 0 else 0       # :169


def boundary_radius(shape, bound_th=0.008):
    """utils/metrics.py:134-135."""
    return bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(shape))


def f_score(foreground_mask, gt_mask, bound_th=0.008):
    """Metrics._get_f_score, utils/metrics.py:119-169."""
    assert np.atleast_3d(foreground_mask).shape[2] == 1          # :132
    return f_from_counts(*f_counts(foreground_mask, gt_mask, boundary_radius(np.shape(foreground_mask), bound_th)))


def counts_of_labels(pred, gt, n_objects, radius, fault=None):
    """int64 [N, n_objects, 4] over label maps [N, H, W]: object k = (label == k), k = 1 .. n_objects."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = np.zeros((pred.shape[0], n_objects, 4), dtype=np.int64)
    for n in range(pred.shape[0]):
        for k in range(1, n_objects + 1):
            out[n, k - 1] = f_counts(pred[n] == k, gt[n] == k, radius, fault)
    return out


def f_of_counts(counts):
    """float64 [N, K] from the counts [N, K, 4], through f_from_counts one pair at a time."""
    counts = np.asarray(counts)
    return np.array([[float(f_from_counts(*(int(v) for v in c))) for c in row] for row in counts], dtype=np.float64).reshape(counts.shape[:2])
