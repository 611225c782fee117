# -*- coding: utf-8 -*-
"""Float64 restatements of the gradients of the decoder's 3x3 / stride 1 / pad 1 convolutions (rmnet_amd.ops.conv3x3_split under
autograd, csrc/conv3x3_wgrad.hip) for tests/test_conv_grad.py.  Plain functions: no fixtures, nothing here is collected by pytest.

1. The gradients (``grads64``)
------------------------------
For out = act(conv(pre(x), W) + b + res), pre / act = ReLU under relu_in / relu_out, and an incoming gradient g:
    G        = g * [out > 0]   under relu_out, else g
    grad_res = G
    db[co]   = sum_{n,y,x} G[n,co,y,x]
    dW[co,ci,ky,kx] = sum_{n,y,x} G[n,co,y,x] * pre(x)[n,ci,y+ky-1,x+kx-1]                       (zero outside the map)
    dX[n,ci,y,x]    = [x > 0 under relu_in] * sum_{co,ky,kx} G[n,co,y-ky+1,x-kx+1] * W[co,ci,ky,kx]   (zero outside the map)
written tap by tap over zero-padded arrays -- not through autograd, which is what it is checked against.  ``fault`` plants one of
FAULTS; every one is caught by a named case of tests/test_conv_grad.py.

2. The kernels' arithmetic and its per-element bound (``wgrad_restate`` / ``dgrad_restate`` / ``acc_bound``)
--------------------------------------------------------------------------------------------------------------
Staging: s = 9 - e for amax in [2^(e-1), 2^e), gs = G 2^s (exact: a power of two), so max|gs| lies in [2^8, 2^9).
Weight gradient, per element (co, tap, ci), with (h, l) = split(pre(x)) and (gh, gl) = split(gs) as the forward's loader splits an
activation (c = clamp(64 v, +-65504), h = fp16(c), l = fp16(c - h)):
    T = (sum_p gh h + sum_p (gh l + gl h)) * 2^-12 / 2^s                     the sums over the pixels p whose tap lies in the map
which is what exact arithmetic gives.  What the kernel adds to T:
  * every product of two fp16 numbers is exact in fp32;
  * the pixel axis is cut into R ranges of at most Kr pixels (``ops.conv3x3_wgrad_plan``).  Inside a range the hi*hi accumulator sums
    at most Kr products in fp32 and the cross accumulator 2 Kr; summing n numbers in fp32 in any order errs by at most
    (n - 1) u sum|terms| to first order, u = 2^-24: (Kr - 1) u Ahh_r + (2 Kr - 1) u Ax_r;
  * acc + accx: one rounding per range, at most u (Ahh_r + Ax_r) to first order;
  * the merge adds the R partials in range order: R - 1 roundings, each of a partial sum no larger than Ahh + Ax to first order;
  * the products with 2^-12 and with the inverse staging scale are exact (powers of two; results in fp32's normal range);
  * second-order terms: every first-order factor above is at most (2 Kr + R) u, so a factor (1 + 2^-10) covers them while
    2 Kr + R <= 2^14 (the tests use Kr <= 4096, R <= 64).
With Ahh = sum_r Ahh_r and Ax likewise:
    |got - T| <= (1 + 2^-10) u ((Kr + R - 1) Ahh + (2 Kr + R) Ax) * 2^-12 / 2^s                                  (``acc_bound``)
nothing tuned.  The bias gradient is a plain fp32 sum: every range in 8 chunks of Kr / 8 pixels, pixel by pixel, then the merge
over the 8 R partials -- Kc = Kr / 8 and Rc = 8 R in:
    |got - sum gs / 2^s| <= (1 + 2^-10) u (Kc + Rc - 2) sum|gs| / 2^s.                                        (``bias_bound``)
The data gradient is the forward kernel on the staged gradient with the flipped pack: one range (R = 1), K = 9 * 256 terms per
accumulator: the same formula with Kr = K, R = 1 and unscale[ci] 2^-6 / 2^s in place of 2^-12 / 2^s (``dgrad_restate``).

How sharp it is: a dropped cross term is worth about sqrt(K) 2^-12.5 of a typical product, the bound about K^2 2^-24 of it.  At
K = 32 pixels the missing term is several times the bound (``test_a_dropped_cross_term_...``), from a few hundred pixels on it is
inside -- which is why the exact family (section 3) carries the structure tests.

Against the true float64 gradient the representation error is added (``wgrad_repr_bound``): h + l differs from c by at most
2^-22 |c| (2^-31 in x's unit where l is an fp16 subnormal), gh + gl likewise (2^-31 / 2^s in g's unit), and the dropped l * gl
term is at most 2^-22 |x g|:  3 * 2^-22 sum|pre(x)||G| + 2^-31 (sum|G| + sum|pre(x)| / 2^s) over the taps inside the map.

3. Why integer inputs come back bit for bit
-------------------------------------------
x integers with |x| <= 15 (conv_ref.int_acts): 64 x is an fp16 number, l = 0.  G = +-2^k, k in {e-3 .. e}, or 0 (``pow2_grads``):
amax = 2^e, s = 8 - e, 64 gs = +-2^(14 + k - e) is an fp16 number, gl = 0.  Both cross accumulators add zeros; the hi*hi one holds
2^(12 + 8 - 3) times a sum of integers x * 2^(k - e + 3) with |.| <= 15 * 8 per pixel, below 2^24 for fewer than 139810 pixels: every
fp32 addition is exact in any order, in the ranges and in the merge.  The unscaling is exact.  So dW, db (sum of +-2^k: exact) and,
with conv_ref.int_weights (|w| <= 8, exact packs), dX (below 2304 * 8 * 8 < 2^24) must equal integer arithmetic in every bit.
"""

import math

import torch
import torch.nn.functional as F

import conv_ref

U = 2.0 ** -24
FAULTS = ('unflipped_tap', 'untransposed_weight', 'no_out_mask', 'no_x_mask', 'res_dropped', 'db_wrong_mask', 'range_lost', 'no_zero_pad')


def _shift(t, dy, dx, wrap=False):
    """t[n, c, y + dy, x + dx], zero outside the map (``wrap``: the planted fault -- the map wraps around instead)."""
    if wrap:
        return torch.roll(t, shifts=(-dy, -dx), dims=(2, 3))
    h, w = t.shape[2:]
    p = F.pad(t, (1, 1, 1, 1))
    return p[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def forward64(x, w, b=None, res=None, relu_in=False, relu_out=False):
    pre = F.relu(x.double()) if relu_in else x.double()
    out = sum(torch.einsum('nchw,oc->nohw', _shift(pre, ky - 1, kx - 1), w.double()[:, :, ky, kx]) for ky in range(3) for kx in range(3))
    if b is not None:
        out = out + b.double().view(1, -1, 1, 1)
    if res is not None:
        out = out + res.double()
    return F.relu(out) if relu_out else out


def grads64(x, w, g, b=None, res=None, relu_in=False, relu_out=False, fault=None):
    """(dX, dW, db, grad_res) in float64 as in section 1; x [N,Cin,H,W], w [Cout,Cin,3,3], g [N,Cout,H,W]."""
    assert fault is None or fault in FAULTS
    x, w, g = x.double(), w.double(), g.double()
    pre = F.relu(x) if relu_in else x
    G = g
    if relu_out and fault != 'no_out_mask':
        G = g * (forward64(x, w, b, res, relu_in, relu_out) > 0)
    wrap = fault == 'no_zero_pad'
    dW = torch.zeros_like(w)
    dX = torch.zeros_like(x)
    wd = w.transpose(0, 1) if fault == 'untransposed_weight' else w          # (needs Cin == Cout)
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = torch.einsum('nohw,nchw->oc', G, _shift(pre, ky - 1, kx - 1, wrap))
            sy, sx = (ky - 1, kx - 1) if fault == 'unflipped_tap' else (1 - ky, 1 - kx)
            dX += torch.einsum('nohw,oc->nchw', _shift(G, sy, sx, wrap), wd[:, :, ky, kx])
    if relu_in and fault != 'no_x_mask':
        dX = dX * (x > 0)
    db = (g * (x > 0) if fault == 'db_wrong_mask' else G).sum(dim=(0, 2, 3))   # (the fault needs Cin == Cout)
    grad_res = torch.zeros_like(G) if fault == 'res_dropped' else G
    return dX, dW, db, grad_res


# ------------------------------------------------------------------------------------------------------- staging
def stage_exponent(amax):
    """s with 2^s amax in [2^8, 2^9); 0 for 0, NaN, Inf.  Python floats (float64 holds every fp32 number, subnormals included)."""
    a = float(amax)
    if not (a > 0.0) or math.isinf(a):
        return 0
    return 9 - math.frexp(a)[1]


def stage64(G):
    """(gs float64, s) of a float gradient tensor: the exact staging."""
    s = stage_exponent(float(G.abs().max()))
    return torch.ldexp(G.double(), torch.tensor(float(s), dtype=torch.float64)), s


# ------------------------------------------------------------------------------------------------------- the kernels restated
def _ranges(pixels, plan):
    nct, nr, rl = plan
    return [(r * rl, min(pixels, (r + 1) * rl)) for r in range(nr)]


def wgrad_restate(x, gs, s, plan, relu_in=False, drop=None, lose_range=None):
    """(T, Ahh, Ax, Tb, Ab) of section 2 for channels-first x [N,Cin,H,W] and the staged gradient gs [N,Cout,H,W] (float64, already
    times 2^s); T / Ahh / Ax are [Cout,Cin,3,3] in dW's unit, Tb / Ab [Cout].  The partials are formed range by range as the kernel
    forms them (``plan`` = ops.conv3x3_wgrad_plan(N*H*W, Cin)) and added in range order; in float64 that order changes nothing, but a
    LOST range (``lose_range``, the planted fault) does.  ``drop`` = 'hl' | 'lh' leaves a cross term out (the power test)."""
    h, l = conv_ref.split_act(x, relu_in)
    gh, gl = conv_ref.split_act(gs)
    n, cin, hh, ww = x.shape
    cout = gs.shape[1]
    pix = n * hh * ww
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(pix, -1)                   # [pixel][channel], linear NHW order
    T = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    Ahh, Ax = torch.zeros_like(T), torch.zeros_like(T)
    Tb, Ab = torch.zeros(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
    ghf, glf, gsf = flat(gh), flat(gl), flat(gs.double())
    for ri, (p0, p1) in enumerate(_ranges(pix, plan)):
        if ri == lose_range:
            continue
        Tb += gsf[p0:p1].sum(0)
        Ab += gsf[p0:p1].abs().sum(0)
        for ky in range(3):
            for kx in range(3):
                hs, ls = flat(_shift(h, ky - 1, kx - 1))[p0:p1], flat(_shift(l, ky - 1, kx - 1))[p0:p1]
                a, b = ghf[p0:p1], glf[p0:p1]
                t = a.t() @ hs
                ahh = a.abs().t() @ hs.abs()
                ax = torch.zeros_like(ahh)
                if drop != 'hl':
                    t = t + a.t() @ ls
                    ax = ax + a.abs().t() @ ls.abs()
                if drop != 'lh':
                    t = t + b.t() @ hs
                    ax = ax + b.abs().t() @ hs.abs()
                T[:, :, ky, kx] += t
                Ahh[:, :, ky, kx] += ahh
                Ax[:, :, ky, kx] += ax
    un = 2.0 ** (-12 - s)
    return T * un, Ahh * un, Ax * un, Tb * 2.0 ** -s, Ab * 2.0 ** -s


def acc_bound(kr, nranges, ahh, ax):
    """(1 + 2^-10) u ((Kr + R - 1) Ahh + (2 Kr + R) Ax): section 2."""
    assert 2 * kr + nranges <= 2 ** 14
    return (1 + 2.0 ** -10) * U * ((kr + nranges - 1) * ahh + (2 * kr + nranges) * ax)


def bias_bound(kr, nranges, ab):
    return (1 + 2.0 ** -10) * U * max(kr + nranges - 2, 0) * ab


def wgrad_repr_bound(x, G, s, relu_in=False):
    """3 * 2^-22 sum|pre(x)||G| + 2^-31 (sum|G| + sum|pre(x)| / 2^s) over the taps inside the map, [Cout,Cin,3,3]."""
    pre = (F.relu(x.double()) if relu_in else x.double()).abs()
    Ga = G.double().abs()
    out = torch.zeros(G.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
    one_x, one_g = torch.ones_like(pre), torch.ones_like(Ga)
    for ky in range(3):
        for kx in range(3):
            sh = _shift(pre, ky - 1, kx - 1)
            inside = _shift(one_x, ky - 1, kx - 1)
            out[:, :, ky, kx] = 3 * 2.0 ** -22 * torch.einsum('nohw,nchw->oc', Ga, sh) \
                + 2.0 ** -31 * (torch.einsum('nohw,nchw->oc', Ga, inside) + torch.einsum('nohw,nchw->oc', one_g, sh) * 2.0 ** -s)
    return out


def dgrad_restate(gs, s, packs, cin):
    """(T, Ahh, Ax) [N,Cin,H,W] of the data gradient before the x > 0 mask: the forward kernel's arithmetic (conv_ref section 2) on
    the staged gradient with the packs of ops.conv3x3_dgrad_pack and unscale / 2^s."""
    gh, gl = conv_ref.split_act(gs)
    conv = lambda a, b: F.conv2d(a, b, None, 1, 1)
    outs = []
    for wp, wu in packs:
        wh, wl = conv_ref.unpack_conv(wp.cpu(), 256, gs.shape[1], 3)
        us = (wu.cpu().double() * 2.0 ** (-6 - s)).view(1, -1, 1, 1)
        t = (conv(gh, wh) + conv(gh, wl) + conv(gl, wh)) * us
        ahh = conv(gh.abs(), wh.abs()) * us
        ax = (conv(gh.abs(), wl.abs()) + conv(gl.abs(), wh.abs())) * us
        outs.append((t, ahh, ax))
    assert 256 * len(outs) == cin
    return tuple(torch.cat([o[i] for o in outs], dim=1) for i in range(3))


# ------------------------------------------------------------------------------------------------------- exact inputs
def pow2_grads(shape, seed, e=0, zeros=True):
    """+-2^k with k in {e-3 .. e} (and zeros), one element exactly 2^e: section 3."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-3, 1, shape, generator=g).float() + e
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    v = sign * torch.ldexp(torch.ones(shape), k)
    if zeros:
        v = v * (torch.randint(0, 4, shape, generator=g) > 0)
    v.view(-1)[0] = 2.0 ** e
    return v
