# -*- coding: utf-8 -*-
"""A numpy restatement of the split activation form of include/rmnet_hip.h (csrc/conv_split.hip: split4, split_act), in float32,
expression for expression:

    v' = ReLU(v) when asked (v < 0 ? 0 : v: keeps NaN and -0.0);   y = v' * 64;   c = fminf(fmaxf(y, -65504), 65504);
    hi = (fp16)c;   lo = (fp16)(c - (float)hi);   counted when !(fabsf(y) <= 65504)

and the layout [M][C / 32][2][32]: per pixel and block of 32 channels the 32 hi halves, then the 32 lo halves.  Every step is one
correctly rounded float32 or float16 operation, so the restatement is exact, and the tests compare bits."""

import numpy as np

ACT_SCALE = np.float32(64.0)
F16_MAX = np.float32(65504.0)


def split_values(v, relu=False):
    """(c, hi, lo, counted) of a float32 array, element by element."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        if relu:
            v = np.where(v < 0, np.float32(0.0), v)
        y = (v * ACT_SCALE).astype(np.float32)
        counted = ~(np.abs(y) <= F16_MAX)
        c = np.fmin(np.fmax(y, -F16_MAX), F16_MAX).astype(np.float32)       # (fmaxf / fminf: a NaN operand loses)
        hi = c.astype(np.float16)
        lo = (c - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return c, hi, lo, counted


def split_form(x_nhwc, relu=False):
    """float32 [..., C] (channels last in memory) -> (float16 [..., C // 32, 2, 32], number of counted elements)."""
    x = np.ascontiguousarray(x_nhwc, dtype=np.float32)
    c = x.shape[-1]
    assert c % 32 == 0
    _, hi, lo, counted = split_values(x, relu)
    lead = x.shape[:-1]
    planes = np.stack([hi.reshape(lead + (c // 32, 32)), lo.reshape(lead + (c // 32, 32))], axis=-2)
    return np.ascontiguousarray(planes), int(counted.sum())


def bits(a):
    """The raw 16-bit patterns of a float16 array (NaN and -0.0 compare as what they are)."""
    return np.ascontiguousarray(a).view(np.int16)
