# -*- coding: utf-8 -*-
"""Clip I/O in numpy, written from the rules of include/rmnet_hip.h (F1), and the cases the clip I/O tests share.  The fixture
tests/golden/clip_io.npz (recorded from the reference's own functions) pins every function here; the kernels and the torch
fallbacks of rmnet_amd.clip_io are compared with these bit for bit.  numpy only."""

import numpy as np

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ODD_MEAN, ODD_STD = (0.31, 0.5, 0.77), (0.19, 0.33, 0.271)


def palette():
    """uint8 [256,3]: ids 0 .. 15 from their bits (bits 0, 1, 2 -> 128 in red, green, blue; bit 3 -> 64 more red, 128 + 64 kept as
    191), then grey."""
    p = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for o in range(16):
        red = 128 * (o & 1) + 64 * (o >> 3 & 1)
        p[o] = (191 if red == 192 else red, 128 * (o >> 1 & 1), 128 * (o >> 2 & 1))
    return p


def trunc_u8(v):
    """(uint8) of float64 values: towards zero inside (-1, 256), saturated outside."""
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def normalize(frames_u8, mean=MEAN, std=STD):
    """[N,H,W,3] uint8 -> [N,3,H,W] float32: one float32 division, then a float64 subtraction and division, one rounding each."""
    x = frames_u8.astype(np.float32) / np.float32(255.0)
    y = (x.astype(np.float64) - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.ascontiguousarray(y.astype(np.float32).transpose(0, 3, 1, 2))


def denormalize(frames, mean=MEAN, std=STD):
    """[N,3,H,W] float32 -> [N,H,W,3] uint8: three float64 operations, then truncation."""
    x = frames.astype(np.float64).transpose(0, 2, 3, 1)
    return trunc_u8((x * np.asarray(std, np.float64) + np.asarray(mean, np.float64)) * 255.0)


def reorganize_lut(labels, ignore_idx=255):
    """(uint8 [256] table, number of ids): the ids present without ignore_idx, ascending, -> 0, 1, 2, ...; everything else -> 0."""
    ids = [i for i in sorted(set(labels.reshape(-1).tolist())) if i != ignore_idx]
    lut = np.zeros(256, np.uint8)
    for rank, i in enumerate(ids):
        lut[i] = rank
    return lut, len(ids)


def onehot(labels, K, lut=None):
    """[N,H,W] uint8 -> [N,K,H,W] uint8, plane k = (lut[label] == k)."""
    m = labels if lut is None else lut[labels]
    return np.stack([(m == k).astype(np.uint8) for k in range(K)], axis=1)


def argmax_first(prob):
    """[N,K,H,W] -> uint8 [N,H,W]: the first index of the maximum."""
    best, idx = prob[:, 0].copy(), np.zeros(prob[:, 0].shape, np.uint8)
    for k in range(1, prob.shape[1]):
        better = prob[:, k] > best
        best[better], idx[better] = prob[:, k][better], k
    return idx


def grow4(m):
    """m or any of its 4-neighbours, nothing beyond the border."""
    g = m.copy()
    g[1:] |= m[:-1]
    g[:-1] |= m[1:]
    g[:, 1:] |= m[:, :-1]
    g[:, :-1] |= m[:, 1:]
    return g


def overlay(frames, labels, mean=MEAN, std=STD, ignore_idx=255, alpha=0.4):
    """[N,3,H,W] float32, [N,H,W] uint8 -> [N,H,W,3] uint8.  Per frame, over the labels present without the smallest one and
    without ignore_idx, ascending: blend the object's pixels with its colour, then blacken its contour."""
    out = denormalize(frames, mean, std)
    colours = palette().astype(np.float64)
    for n in range(labels.shape[0]):
        present = sorted(set(labels[n].reshape(-1).tolist()))
        for o in present[1:]:
            if o == ignore_idx:
                continue
            m = labels[n] == o
            out[n][m] = trunc_u8(out[n].astype(np.float64) * alpha + (1.0 - alpha) * colours[o])[m]
            out[n][grow4(m) & ~m] = 0
    return out


# ------------------------------------------------------------------------------------------------ shared cases
SHAPES = ((1, 1), (1, 3), (2, 2), (3, 5), (7, 1), (1, 64), (2, 65), (3, 63), (5, 256), (4, 257), (1, 1023))
FRAME_IDS = ((0, 1, 2, 17, 255), (1, 2, 3, 255), (2, 3, 17))       # frame n draws from FRAME_IDS[n]: another lowest label in each


def shape_case(N, H, W, seed=0):
    """uint8 frames [N,H,W,3] and labels [N,H,W] in short random runs, so that objects touch, reach every border and differ in
    their lowest label from frame to frame."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W + N)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    labels = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        ids = np.asarray(FRAME_IDS[n % 3], np.uint8)
        runs = np.repeat(rng.integers(0, len(ids), (H, W // 2 + 1)), 2, axis=1)[:, :W]
        labels[n] = ids[runs]
        if n % 3 == 0:
            labels[n, 0, 0] = 0
    return frames, labels


_ART = {'.': 0, 'a': 1, 'b': 2, 'c': 3, 'd': 4, 'e': 5, 'q': 17, 'x': 255, 'g': 7}


def _art(rows):
    return np.array([[_ART[ch] for ch in row] for row in rows], np.uint8)


def overlay_clip():
    """Four 9 x 12 frames: (0) objects in the four corners and on the four borders, pairs that touch horizontally and vertically
    with the lower id on either side; (1) no background pixel; (2) one label throughout; (3) ignored pixels next to objects and
    next to the background, and an object of label >= 16."""
    labels = np.stack([
        _art(['aa...cc...bb',
              'a..........b',
              '...ab..ba...',
              'd..ab..ba..e',
              'd...........',
              '..c..e......',
              '..e..c...qq.',
              'b...dd...qqa',
              'bb..dd....aa']),
        _art(['bbbbbbcccccc',
              'bbbbbbcccccc',
              'bbaabbccxxcc',
              'bbaabbccxxcc',
              'bbbbbbcccccc',
              'qqqqqqaaaaaa',
              'qqqqqqaaaaaa',
              'qqqxqqaaeeaa',
              'qqqqqqaaaaaa']),
        _art(['gggggggggggg'] * 9),
        _art(['x..........x',
              '.xaa....bbx.',
              '..aax..xbb..',
              '..aa....bb..',
              '............',
              '..xxxx..q...',
              '..xccx..qx..',
              '..xxxx..q...',
              'a..........x']),
    ])
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, labels.shape + (3,), dtype=np.uint8), labels


EXHAUSTIVE_IDS = (0, 1, 8, 9, 16, 100, 255)      # colour components 0, 64, 128, 191 and the greys 16, 100, 255
EXHAUSTIVE_IGNORE = 254                           # so that label 255 is an object here


def exhaustive_case(mean=MEAN, std=STD):
    """Two frames of width 256 in which column x holds byte x in every channel, in bands of three rows per label of EXHAUSTIVE_IDS
    (the middle row of a band has no other label around it: a blend of the denormalised value alone).  Returns (uint8 frames
    [1,H,256,3], float32 frames [2,3,H,256], labels [2,H,256]): float frame 0 is the normalised uint8 frame -- whose
    denormalisation loses some values -- and float frame 1 holds the centre of every byte's interval, ((x + 0.5) / 255 - mean) /
    std, so that every byte value is denormalised to in every channel and meets every colour component."""
    H = 3 * len(EXHAUSTIVE_IDS)
    ramp = np.arange(256, dtype=np.uint8)
    frames_u8 = np.broadcast_to(ramp[None, None, :, None], (1, H, 256, 3)).copy()
    centre = ((ramp.astype(np.float64)[None, :] + 0.5) / 255.0 - np.asarray(mean)[:, None]) / np.asarray(std)[:, None]      # [3,256]
    second = np.broadcast_to(centre.astype(np.float32)[:, None, :], (3, H, 256))
    frames = np.ascontiguousarray(np.stack([normalize(frames_u8, mean, std)[0], second]))
    band = np.repeat(np.asarray(EXHAUSTIVE_IDS, np.uint8), 3)
    labels = np.ascontiguousarray(np.broadcast_to(band[None, :, None], (2, H, 256)))
    return frames_u8, frames, labels


def argmax_case(N, K, H, W, seed=0):
    """Probabilities drawn from {0, 0.25, 0.5, 1} (ties are frequent), with a lone maximum planted in the first plane at one pixel
    and in the last plane at another."""
    rng = np.random.default_rng(seed + 31 * K + H * W)
    prob = rng.choice(np.asarray([0.0, 0.25, 0.5, 1.0], np.float32), (N, K, H, W))
    flat = prob.reshape(N, K, H * W)
    flat[:, :, 0] = 0.25
    flat[:, 0, 0] = 2.0
    flat[:, :, -1] = 0.25
    flat[:, K - 1, -1] = 2.0
    return prob
