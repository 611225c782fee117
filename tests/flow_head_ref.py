# -*- coding: utf-8 -*-
"""Float64 restatements and input families for tests/test_flow_head.py (csrc/flow_head.hip, ops.flow_head_pack / ops.flow_head /
ops.flow_up).  Plain functions: nothing here is collected by pytest.

The flow head
-------------
out[n][co][y][x] = bias[co] + sum over the taps (ky, kx) inside the map and c < Cin of x[n][y + ky - 1][x + kx - 1][c] *
w[co][c][ky][kx], for a channels-last buffer of x_ld >= Cin channels per pixel.  The kernel forms it from plain fp32 fused
multiply-adds and fp32 additions in a fixed order (32-channel slices, nine taps, slices); the tests use only what holds for ANY
order:
  * integer family (``head_case('int', ...)``): activations in [-15, 15], weights in [-8, 8] (drawn independently for both output
    channels), an integer bias.  Every partial sum is an integer below 9 * 800 * 15 * 8 + 8 < 2^24, so every fp32 operation is
    exact and the result must equal the float64 F.conv2d cast to fp32, bit for bit;
  * random family (``head_case('random', ...)``): x, w, bias uniform in [-1, 1].  Summing K = 9 Cin products and a bias in fp32 in
    any order, with or without FMA, errs by at most (K + 2) 2^-24 (sum|x||w| + |b|) to first order (conv_ref.py, the pred_head
    paragraph): ``head_bound``.
Both families fill the padding channels Cin .. x_ld - 1 with NON-ZERO values of the family's kind: a kernel that reads one is wrong
on every pixel.

The pack (ops.flow_head_pack, include/rmnet_hip.h): fp32 [ceil32(Cin)][9][2], w[co][c][ky][kx] at (c * 9 + 3 ky + kx) * 2 + co,
zero for c >= Cin.  ``unpack`` inverts it.

The flow upsampler
------------------
ConvTranspose2d(2, 2, 4, stride 2, padding 1, bias=False) in the four-phase form of flow_conv_ref.py: the output pixel
(2i + a, 2j + b) is the sum over ci, ty, tx of flow[ci][i + a - 1 + ty][j + b - 1 + tx] * w[ci][co][3 - a - 2 ty][3 - b - 2 tx],
taps outside the map skipped (``up_numpy``): 8 products, so any fp32 order is within (8 + 2) 2^-24 sum|f||w| (``up_bound``)."""

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SLICE = 32                # csrc/flow_head.hip kCS
TILE = 14                 # csrc/flow_head.hip kOH = kOW


def ceil32(c):
    return (c + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------------- the pack
def unpack(wpack, cin):
    """(weight [2, Cin, 3, 3], padding [ceil32(Cin) - Cin, 9, 2]) from the [ceil32(Cin)][9][2] layout."""
    p = wpack.view(ceil32(cin), 3, 3, 2)
    return p[:cin].permute(3, 0, 1, 2).contiguous(), p[cin:].reshape(-1, 9, 2)


# ------------------------------------------------------------------------------------------------------- the head's inputs
def head_case(family, n, h, w, cin, x_ld, seed):
    """(x [N, x_ld, H, W] NCHW-shaped CPU tensor, padding channels filled; weight [2, Cin, 3, 3]; bias [2])."""
    g = torch.Generator().manual_seed(seed)
    if family == 'int':
        x = torch.randint(-15, 16, (n, x_ld, h, w), generator=g).float()
        x[:, cin:] = torch.randint(1, 16, (n, x_ld - cin, h, w), generator=g).float()          # (never zero)
        wt = torch.randint(-8, 9, (2, cin, 3, 3), generator=g).float()
        b = torch.randint(-8, 9, (2,), generator=g).float()
    else:
        x = torch.rand(n, x_ld, h, w, generator=g) * 2 - 1
        x[:, cin:] = 0.5 + 0.5 * torch.rand(n, x_ld - cin, h, w, generator=g)                   # (never zero)
        wt = torch.rand(2, cin, 3, 3, generator=g) * 2 - 1
        b = torch.rand(2, generator=g) * 2 - 1
    return x, wt, b


def head_reference(x, wt, b, cin):
    """The float64 F.conv2d of the first ``cin`` channels."""
    return F.conv2d(x[:, :cin].double(), wt.double(), b.double(), 1, 1)


def head_bound(x, wt, b, cin):
    """(9 Cin + 2) 2^-24 (sum|x||w| + |b|) per element, the sum over the taps inside the map."""
    mag = F.conv2d(x[:, :cin].double().abs(), wt.double().abs(), b.double().abs(), 1, 1)
    return (9 * cin + 2) * U * mag


FAULTS = ('tap', 'last_channel', 'swap', 'padding')


def head_restate(x, wt, b, cin, fault=None):
    """The head written out tap by tap in float64 (no F.conv2d), optionally with one planted fault:
    'tap' -- the centre tap missing at the border pixel (image 0, last row, last column); 'last_channel' -- channel Cin - 1
    dropped; 'swap' -- the two output channels swapped; 'padding' -- channel Cin of the buffer (padding) read with channel
    Cin - 1's weights."""
    x, wt, b = x.double(), wt.double(), b.double()
    n, _, h, w = x.shape
    nc = cin
    if fault == 'last_channel':
        nc = cin - 1
    elif fault == 'padding':
        nc = cin + 1
        wt = torch.cat((wt, wt[:, cin - 1:cin]), 1)
    xp = F.pad(x[:, :nc], (1, 1, 1, 1))
    out = b.view(1, 2, 1, 1).expand(n, 2, h, w).clone()
    for ky in range(3):
        for kx in range(3):
            t = torch.einsum('nchw,oc->nohw', xp[:, :, ky:ky + h, kx:kx + w], wt[:, :nc, ky, kx])
            if fault == 'tap' and (ky, kx) == (1, 1):
                t[0, :, h - 1, w - 1] = 0.0
            out += t
    return out.flip(1) if fault == 'swap' else out


# ------------------------------------------------------------------------------------------------------- the upsampler
def up_case(family, n, h, w, seed):
    """(flow [N, 2, h, w], weight [2, 2, 4, 4]) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    if family == 'int':
        return torch.randint(-15, 16, (n, 2, h, w), generator=g).float(), torch.randint(-8, 9, (2, 2, 4, 4), generator=g).float()
    return torch.rand(n, 2, h, w, generator=g) * 2 - 1, torch.rand(2, 2, 4, 4, generator=g) * 2 - 1


def up_numpy(flow, wt):
    """The four-phase formula in float64 numpy, loops written out: the statement flow_up implements."""
    f, wt = np.asarray(flow, np.float64), np.asarray(wt, np.float64)
    n, _, h, w = f.shape
    out = np.zeros((n, 2, 2 * h, 2 * w))
    for i in range(h):
        for j in range(w):
            for a in (0, 1):
                for b in (0, 1):
                    for ci in (0, 1):
                        for ty in (0, 1):
                            for tx in (0, 1):
                                iy, ix = i + a - 1 + ty, j + b - 1 + tx
                                if 0 <= iy < h and 0 <= ix < w:
                                    out[:, :, 2 * i + a, 2 * j + b] += f[:, ci, iy, ix, None] * wt[ci, :, 3 - a - 2 * ty, 3 - b - 2 * tx]
    return out


def up_reference(flow, wt):
    return F.conv_transpose2d(flow.double(), wt.double(), None, 2, 1)


def up_bound(flow, wt):
    """10 2^-24 sum|f||w| per element (8 products)."""
    return 10 * U * F.conv_transpose2d(flow.double().abs(), wt.double().abs(), None, 2, 1)
