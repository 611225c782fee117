# -*- coding: utf-8 -*-
"""Multi-scale inference's resize and merge in numpy float32, written from the rules of include/rmnet_hip.h (H1), and the cases the
tests of tests/test_tta.py share.  Every product, sum and division below is one numpy operation on float32 operands, so each is
rounded on its own.  ``fault`` plants one named mistake (None: none); the tests show that their cases see each of them."""

import numpy as np

F32 = np.float32
FAULTS = ('i1_unclamped', 'no_half_offset', 'flip_wrong_side', 'reciprocal_mean', 'reversed_order', 'last_argmax', 'swapped_scales')


def scaled_size(h, w, fs):
    """floor(double(in) * double(fs)) per axis: the size F.interpolate(scale_factor=fs) returns."""
    return int(np.floor(float(h) * float(fs))), int(np.floor(float(w) * float(fs)))


def scale_for_factor(fs):
    """(float)(1.0 / fs): the source step per output pixel under F.interpolate(scale_factor=fs)."""
    return F32(1.0 / float(fs))


def scale_for_size(inp, out):
    """fl((float)in / (float)out): the source step per output pixel under F.interpolate(size=)."""
    return F32(inp) / F32(out)


def axis(out, inp, scale, fault=None):
    """(i0, i1, l0, l1) for d = 0 .. out - 1."""
    scale = F32(scale)
    d = np.arange(out, dtype=F32)
    if fault == 'no_half_offset':
        s = np.maximum(scale * d, F32(0))
    else:
        s = np.maximum(scale * (d + F32(0.5)) - F32(0.5), F32(0))
    i0 = np.minimum(s, F32(inp - 1)).astype(np.int64)
    i1 = i0 + 1 if fault == 'i1_unclamped' else np.minimum(i0 + 1, inp - 1)
    l1 = s - i0.astype(F32)
    l0 = F32(1) - l1
    assert s.dtype == l0.dtype == l1.dtype == F32
    return i0, i1, l0, l1


def resize(x, out_h, out_w, scale_h, scale_w, flip=False, fault=None):
    """x [..., Hs, Ws] float32 -> [..., out_h, out_w]; ``flip`` mirrors the written rows."""
    x = np.asarray(x)
    assert x.dtype == F32
    if fault == 'swapped_scales':
        scale_h, scale_w = scale_w, scale_h
    if fault == 'flip_wrong_side' and flip:            # the source is mirrored, not the result
        x, flip = x[..., ::-1], False
    Hs, Ws = x.shape[-2:]
    y0, y1, l0y, l1y = axis(out_h, Hs, scale_h, fault)
    x0, x1, l0x, l1x = axis(out_w, Ws, scale_w, fault)
    if fault == 'i1_unclamped':                        # what lies past the last row / column: zeros here
        x = np.concatenate([x, np.zeros(x.shape[:-2] + (1, Ws), F32)], axis=-2)
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (1,), F32)], axis=-1)
    top, bottom = x[..., y0, :], x[..., y1, :]
    a, b, c, d = top[..., x0], top[..., x1], bottom[..., x0], bottom[..., x1]
    l0y, l1y = l0y[:, None], l1y[:, None]
    out = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)
    assert out.dtype == F32
    return np.ascontiguousarray(out[..., ::-1] if flip else out)


def resize_factor(x, fs, flip=False, fault=None):
    """F.interpolate(x, scale_factor=fs, mode='bilinear', align_corners=False) (then torch.flip(dims=[-1]) with ``flip``)."""
    h, w = scaled_size(x.shape[-2], x.shape[-1], fs)
    return resize(x, h, w, scale_for_factor(fs), scale_for_factor(fs), flip, fault)


def argmax_first(mean, fault=None):
    K = mean.shape[1]
    if fault == 'last_argmax':
        return (K - 1 - np.argmax(mean[:, ::-1], axis=1)).astype(np.uint8)
    return np.argmax(mean, axis=1).astype(np.uint8)


def merge(sources, flipped, H, W, fault=None):
    """sources [N,K,h_e,w_e] float32, one flag each -> (mean [N,K,H,W] float32, labels [N,H,W] uint8)."""
    entries = list(zip(sources, flipped))
    if fault == 'reversed_order':
        entries.reverse()
    acc = None
    for s, f in entries:
        s = np.asarray(s)
        if fault == 'flip_wrong_side':                 # the resized entry is mirrored, not its source
            v = resize(s, H, W, scale_for_size(s.shape[2], H), scale_for_size(s.shape[3], W), bool(f), None)
        else:
            v = resize(s[..., ::-1] if f else s, H, W, scale_for_size(s.shape[2], H), scale_for_size(s.shape[3], W), False, fault)
        acc = v if acc is None else acc + v
    if fault == 'reciprocal_mean':
        mean = acc * (F32(1) / F32(len(entries)))
    else:
        mean = acc / F32(len(entries))
    assert mean.dtype == F32
    mean = np.ascontiguousarray(mean)
    return mean, argmax_first(mean, fault)


# ------------------------------------------------------------------------------------------------ the shared cases
def plane(seed, *shape):
    """N(0, 1) float32 without a negative zero (x1 resizing returns +0.0 for it, as torch does)."""
    x = np.random.RandomState(seed).standard_normal(shape).astype(F32)
    x[x == 0] = F32(0)
    return x


# (P, Hs, Ws, fs): the output widths 1, 3, 4, 5, 63, 64, 65 (a lane per column: below, at and above a wave), 260 (a second
# workgroup), one-row and one-column sources, a one-row result, and every scale factor of the comparison with torch
RESIZE_SHAPES = [(1, 2, 2, 0.5), (2, 3, 3, 1.0), (1, 3, 2, 2.0), (3, 5, 4, 1.25), (1, 6, 42, 1.5), (2, 5, 128, 0.5), (1, 4, 52, 1.25),
                 (1, 3, 50, 1.3), (3, 1, 7, 1.5), (2, 5, 1, 2.0), (1, 1, 1, 2.0), (1, 3, 200, 1.3), (2, 30, 53, 0.6), (1, 37, 66, 0.75),
                 (1, 7, 9, 4.0)]


def resize_cases():
    """(name, x [P,Hs,Ws], fs, flip): every shape unflipped and flipped (odd and even widths both occur)."""
    out = []
    for i, (P, Hs, Ws, fs) in enumerate(RESIZE_SHAPES):
        for flip in (False, True):
            out.append(('%dx%dx%d fs=%g flip=%d' % (P, Hs, Ws, fs, flip), plane(100 + i, P, Hs, Ws), fs, flip))
    return out


_SCALES = (1.0, 0.75, 1.25, 0.5, 1.5, 2.0, 0.6, 1.3)


def _entries(seed, N, K, H, W, E, sizes=None):
    rs = np.random.RandomState(seed)
    sources, flipped = [], []
    for e in range(E):
        h, w = sizes[e] if sizes else (max(1, int(H * _SCALES[e])), max(1, int(W * _SCALES[e])))
        s = rs.standard_normal((N, K, h, w)).astype(F32)
        s[s == 0] = F32(0)
        sources.append(s)
        flipped.append(bool(e % 2))
    return sources, flipped


def merge_cases():
    """(name, sources, flipped, H, W).  Output widths 1, 3, 4, 5, 63, 64, 65 (four columns per lane: lanes without a full group,
    row bases that are and are not 16-byte aligned, a second lane and a second workgroup column at 260), up and down scales and
    flips of odd and even widths in one merge, E = 1 .. 8, K in {1, 2, 11, 255}, N = 1 and 3, one-row / one-column sources, a
    one-row result, ties across K."""
    out = []
    for W in (1, 3, 4, 5, 63, 64, 65, 260):
        H = 3 if W < 100 else 2
        out.append(('W=%d' % W, *_entries(200 + W, 1, 2, H, W, 3), H, W))
    for E in range(1, 9):
        out.append(('E=%d' % E, *_entries(300 + E, 1, 2, 5, 9, E), 5, 9))
    for K, N in ((1, 1), (11, 3), (255, 1)):
        out.append(('K=%d N=%d' % (K, N), *_entries(400 + K, N, K, 6, 8, 2), 6, 8))
    out.append(('one-row and one-column sources', *_entries(500, 3, 2, 4, 7, 3, sizes=[(1, 1), (1, 5), (5, 1)]), 4, 7))
    out.append(('one-row result', *_entries(501, 1, 3, 1, 6, 2, sizes=[(1, 6), (2, 9)]), 1, 6))
    out.append(('rows beyond one workgroup', *_entries(502, 1, 2, 9, 5, 2), 9, 5))
    # ties: planes 0 and 2 equal and largest on the left half, planes 1 and 3 on the right half, everything equal in the last row
    t = np.zeros((1, 4, 4, 6), F32)
    t[:, (0, 2), :3, :3] = 5
    t[:, (1, 3), :3, 3:] = 7
    out.append(('ties', [t, t.copy()], [False, False], 4, 6))
    return out


def order_case():
    """Three same-size entries whose fp32 sum depends on the order: (2^24 + 1) + 1 = 2^24 (twice a tie to even), (1 + 1) + 2^24 =
    2^24 + 2."""
    big, one = np.full((1, 1, 2, 3), 2.0 ** 24, F32), np.ones((1, 1, 2, 3), F32)
    return [big, one, one.copy()], [False, False, False], 2, 3
