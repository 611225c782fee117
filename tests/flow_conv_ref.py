# -*- coding: utf-8 -*-
"""Float64 restatements for tests/test_flow_conv.py (csrc/flow_conv.hip, ops.flow_conv_pack / ops.flow_conv).  Plain functions:
nothing here is collected by pytest.  The arithmetic, the exactness arguments and the per-element bound are those of
tests/conv_ref.py; what is added here is the tap list: channel-padded packs, and ConvTranspose2d(4, stride 2, padding 1) as four
2x2-tap phases.

Phase (a, b) in {0, 1}^2 computes the output pixels (2i + a, 2j + b), (i, j) over the INPUT map, from the input pixels
(i + a - 1 + ty, j + b - 1 + tx), ty, tx in {0, 1}, with the 4x4 kernel's element ky = 3 - a - 2 ty, kx = 3 - b - 2 tx: from
y = 2 iy - 1 + ky (stride 2, padding 1), y = 2i + a and iy = i + a - 1 + ty give ky = 3 - a - 2 ty."""

import numpy as np
import torch
import torch.nn.functional as F

import conv_ref as R


def ceil32(c):
    return (c + 31) // 32 * 32


def unpack(wp, cout, cin, taps, phases=1):
    """(Wh, Wl) [P, Cout, Cp, taps] float64, still scaled, from the [phase][tap][Cp / 32][hi, lo][co][32] layout."""
    cp = ceil32(cin)
    p = wp.view(torch.float16).double().view(phases, taps, cp // 32, 2, cout, 32)
    return tuple(p[:, :, :, i].permute(0, 3, 2, 4, 1).reshape(phases, cout, cp, taps) for i in (0, 1))


def phase_taps(a, b):
    """[(ty, tx, ky, kx)] of phase (a, b), in the pack's tap order (tap = 2 ty + tx)."""
    return [(ty, tx, 3 - a - 2 * ty, 3 - b - 2 * tx) for ty in (0, 1) for tx in (0, 1)]


def phase_input(t, a, b):
    """The [.., H + 1, W + 1] window of the zero-padded map that a VALID 2x2 convolution turns into phase (a, b)'s [.., H, W]."""
    h, w = t.shape[-2:]
    return F.pad(t, (1, 1, 1, 1))[..., a:a + h + 1, b:b + w + 1]


def deconv_by_phases_numpy(x, w):
    """ConvTranspose2d(4, stride 2, padding 1) of x [N, Cin, H, W] with w [Cin, Cout, 4, 4] as four 2x2-tap convolutions, in
    float64 numpy, loops written out: the statement the kernel implements."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    out = np.zeros((n, cout, 2 * h, 2 * wd))
    for a in (0, 1):
        for b in (0, 1):
            for ty, tx, ky, kx in phase_taps(a, b):
                for i in range(h):
                    iy = i + a - 1 + ty
                    if not 0 <= iy < h:
                        continue
                    for j in range(wd):
                        ix = j + b - 1 + tx
                        if 0 <= ix < wd:
                            out[:, :, 2 * i + a, 2 * j + b] += x[:, :, iy, ix] @ w[:, :, ky, kx]
    return out


def reference(x, w, shift, ksize, stride, transposed):
    """The float64 convolution + shift (no activation)."""
    x, w = x.double(), w.double()
    b = None if shift is None else shift.double()
    return F.conv_transpose2d(x, w, b, 2, 1) if transposed else F.conv2d(x, w, b, stride, ksize // 2)


def activate(y64, act):
    """The kernel's activation on the fp32 value: ReLU selects; LeakyReLU(0.1) is y > 0 ? y : y * 0.1f, one fp32 product."""
    y = y64.float()
    if act == 'relu':
        return torch.where(y < 0, torch.zeros_like(y), y)
    if act == 'leaky':
        y = y.numpy()
        return torch.from_numpy(np.where(y > 0, y, (y * np.float32(0.1)).astype(np.float32)))
    return y


def per_phase(fn, x_like, transposed, ksize, stride):
    """Apply ``fn(conv)`` where ``conv(t, w)`` convolves a [N, C, H, W] tensor with per-phase weights: returns the assembled map.
    ``fn`` gets (phase index, conv) and returns that phase's [N, Cout, Hg, Wg] result."""
    if not transposed:
        return fn(0, lambda t, w: F.conv2d(t, w, None, stride, ksize // 2))
    n, _, h, wd = x_like.shape
    out = None
    for a in (0, 1):
        for b in (0, 1):
            r = fn(2 * a + b, lambda t, w, a=a, b=b: F.conv2d(phase_input(t, a, b), w))
            if out is None:
                out = r.new_zeros(n, r.shape[1], 2 * h, 2 * wd)
            out[:, :, a::2, b::2] = r
    return out


def restate(x, wp, wu, cout, cin, ksize, stride, transposed, shift=None):
    """(T, A, P) for every output element, from the PACK and the fp32 input: T the exact three-term value, A the sum of the
    magnitudes of its products (times unscale / 64), P what the kernel returns when both accumulators are exact (conv_ref.py
    section 1b: fp32(acc + accx), scaled, fp32(. + shift))."""
    taps, phases = (4, 4) if transposed else (ksize * ksize, 1)
    kk = 2 if transposed else ksize
    wh, wl = unpack(wp, cout, cin, taps, phases)
    wh = wh[:, :, :cin].reshape(phases, cout, cin, kk, kk)
    wl = wl[:, :, :cin].reshape(phases, cout, cin, kk, kk)
    h, l = R.split_act(x)
    us = (wu.double() / R.ACT_SCALE).view(1, -1, 1, 1)
    hh = per_phase(lambda p, conv: conv(h, wh[p]), x, transposed, ksize, stride)
    cross = per_phase(lambda p, conv: conv(h, wl[p]) + conv(l, wh[p]), x, transposed, ksize, stride)
    mag = per_phase(lambda p, conv: conv(h.abs(), wh[p].abs() + wl[p].abs()) + conv(l.abs(), wh[p].abs()), x, transposed, ksize, stride)
    t = (hh + cross) * us
    pred = (hh + cross).float().double() * us
    if shift is not None:
        t = t + shift.double().view(1, -1, 1, 1)
        pred = (pred + shift.double().view(1, -1, 1, 1)).float().double()
    return t, mag * us, pred
