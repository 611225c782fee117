# -*- coding: utf-8 -*-
"""Float64 restatement of the backward of the two key / value heads (rmnet_amd.ops._KeyValueFn, csrc/conv_wgrad_n.hip) for
tests/test_kv_grad.py.  Plain functions: no fixtures, nothing here is collected by pytest.

The heads are key = conv(x, Wk) + bk and value = conv(x, Wv) + bv (3x3 / stride 1 / pad 1) and, on the regional path, both are a
constant +0.0 outside image n's rectangle (cx0, cx1, cy0, cy1), inclusive, clamped to the map.  For incoming gradients gk, gv:
    Gk = select(inside, gk, 0)      (a select: what gk holds outside the rectangle is never looked at)      Gv likewise
    dWk, dbk = the weight / bias gradient of a convolution for (x, Gk)          dWv, dbv for (x, Gv)       (conv_grad_ref.grads64)
    dX = dgrad(Gk, Wk) + dgrad(Gv, Wv)
What arrives from the memory read may be a [:, :, t] slice of a [N, C, T, h, w] tensor: ``read_planes`` restates the address
n sn + c sc + y W + x.  The device stages each head with its own power of two 2^s (``staged``) and divides by it again; in float64
that changes nothing unless the wrong head's scale is used.  ``fault`` plants one of FAULTS; each is caught by a named case of
tests/test_kv_grad.py."""

import torch

import conv_grad_ref as cg

FAULTS = ('mask_product', 'rect_of_previous_image', 'upper_edge_dropped', 'key_scale_for_value', 'unflipped_tap', 'res_dropped',
          'tail_tile_lost', 'sc_is_hw')


def inside(rects, n, h, w, fault=None):
    """bool [N, 1, H, W]: cell (y, x) of image i lies inside rects[i] (None: everywhere)."""
    if rects is None:
        return torch.ones(n, 1, h, w, dtype=torch.bool)
    r = torch.as_tensor(rects, dtype=torch.int64).view(n, 4)
    if fault == 'rect_of_previous_image':
        r = torch.roll(r, 1, 0)
    ys, xs = torch.arange(h).view(1, h, 1), torch.arange(w).view(1, 1, w)
    x1 = r[:, 1].view(n, 1, 1) - (1 if fault == 'upper_edge_dropped' else 0)
    y1 = r[:, 3].view(n, 1, 1) - (1 if fault == 'upper_edge_dropped' else 0)
    m = (xs >= r[:, 0].view(n, 1, 1)) & (xs <= x1) & (ys >= r[:, 2].view(n, 1, 1)) & (ys <= y1)
    return m.view(n, 1, h, w)


def read_planes(src, offset, sn, sc, n, c, h, w, fault=None):
    """[N, C, H, W] gathered from the flat tensor ``src``: element (n, c, y, x) at offset + n sn + c sc + y W + x."""
    if fault == 'sc_is_hw':
        sc = h * w
    idx = offset + (torch.arange(n).view(n, 1, 1) * sn + torch.arange(c).view(1, c, 1) * sc + torch.arange(h * w).view(1, 1, -1))
    return src.reshape(-1)[idx.reshape(-1)].view(n, c, h, w)


def masked(g, rects, fault=None):
    m = inside(rects, g.shape[0], g.shape[2], g.shape[3], fault)
    g = g.double()
    return g * m if fault == 'mask_product' else torch.where(m, g, torch.zeros_like(g))


def staged(G):
    """(G 2^s, s): the head's own staging exponent, from the largest |element| BEFORE the mask would be the device's default; the
    restatement only needs some exponent per head, and takes the masked gradient's."""
    a = float(torch.nan_to_num(G, nan=0.0, posinf=0.0, neginf=0.0).abs().max())
    s = cg.stage_exponent(a)
    return G * 2.0 ** s, s


def kv_grads64(x, wk, wv, gk, gv, rects=None, fault=None):
    """dict(dX, dWk, dbk, dWv, dbv) in float64; a head given as None contributes nothing (its entries are None)."""
    assert fault is None or fault in FAULTS
    out = dict(dX=torch.zeros_like(x.double()), dWk=None, dbk=None, dWv=None, dbv=None)
    tap_fault = 'unflipped_tap' if fault == 'unflipped_tap' else None
    s_key = None
    for name, w, g in (('k', wk, gk), ('v', wv, gv)):
        if g is None:
            continue
        G = masked(g, rects, fault)
        Gs, s = staged(G)
        if name == 'k':
            s_key = s
        s_used = s_key if (fault == 'key_scale_for_value' and name == 'v' and s_key is not None) else s
        dX, dW, db, _ = cg.grads64(x, w, Gs, fault=tap_fault)
        dX, dW, db = dX * 2.0 ** -s_used, dW * 2.0 ** -s_used, db * 2.0 ** -s_used
        if fault == 'tail_tile_lost':
            t0 = (w.shape[0] - 1) // 256 * 256                       # the last tile of up to 256 output channels
            dW[t0:] = 0.0
            db[t0:] = 0.0
        out['dW' + name], out['db' + name] = dW, db
        if name == 'v' and fault == 'res_dropped':
            out['dX'] = dX                                           # (the key head's dX lost)
        else:
            out['dX'] = out['dX'] + dX
    return out
