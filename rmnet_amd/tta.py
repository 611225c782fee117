# -*- coding: utf-8 -*-
"""The arithmetic around the network passes of multi-scale and flipped inference (utils/helpers.py:44-78): the bilinear resize of
the frames and the merge of the per-entry probability clips into one mean and one label map.

``resize_bilinear`` is F.interpolate(x, scale_factor=fs, mode='bilinear', align_corners=False), optionally followed by
torch.flip(dims=[-1]); ``merge`` is, per entry, torch.flip of a flipped entry, F.interpolate(size=(H, W)), then torch.stack,
torch.mean and the driver's torch.argmax, without any of the intermediate tensors.  Both are written from the formula torch's
bilinear kernel is written from, in plain fp32 with every product and sum rounded on its own (include/rmnet_hip.h H1).

As in ``rmnet_amd.clip_io``: contiguous float32 tensors on the GPU go to the HIP kernels of csrc/tta.hip (``rmnet_amd.ops``) and
everything else -- CPU tensors, strided views -- to a torch restatement with one torch operation per rounded operation, which
returns the same bits.
"""

import math

import numpy as np
import torch

from . import clip_io
from . import ops

MAX_ENTRIES = ops.TTA_MAX_ENTRIES


def _on_kernel(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def _f32(v):
    """A Python number rounded to float32, as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float64).to(torch.float32))


def scaled_size(h, w, fs):
    """The size F.interpolate(scale_factor=fs) gives an (h, w) image: floor(double(in) * double(fs)) per axis."""
    return int(math.floor(float(h) * float(fs))), int(math.floor(float(w) * float(fs)))


def scale_for_factor(fs):
    """The source step per output pixel that F.interpolate(scale_factor=fs) hands its kernel: (float)(1.0 / fs)."""
    return _f32(1.0 / float(fs))


def nearest_index_for_scale(out, inp, scale):
    """The source index of every output index d = 0 .. out - 1 of an axis with ``inp`` elements, int64 numpy array:
    min(int(floorf(float(d) * scale)), inp - 1) with the product rounded to float32 (include/rmnet_hip.h I2).  Host only."""
    d = np.arange(int(out), dtype=np.float32)
    return np.minimum(np.floor(d * np.float32(scale)), np.float32(int(inp) - 1)).astype(np.int64)


def nearest_index(out, inp, fs):
    """``nearest_index_for_scale`` with the scale of F.interpolate(scale_factor=fs, mode='nearest'), (float)(1.0 / fs): torch's
    legacy nearest rule as a plain formula.  torch's CPU kernels copy an axis whose output size equals its input size or its
    double even when ``fs`` is neither 1 nor 2; this does not."""
    return nearest_index_for_scale(out, inp, scale_for_factor(fs))


def _axis(out, inp, scale, device):
    """axis(d, in, scale) of include/rmnet_hip.h H1 for d = 0 .. out - 1: (i0, i1 int64, l0, l1 float32).  ``scale`` is a 0-dim
    float32 tensor."""
    d = torch.arange(out, dtype=torch.float32, device=device)
    s = torch.clamp_min((d + 0.5) * scale - 0.5, 0.0)
    last = torch.full((), float(inp - 1), dtype=torch.float32, device=device)
    i0 = torch.minimum(s, last).to(torch.int64)
    i1 = torch.clamp_max(i0 + 1, inp - 1)
    l1 = s - i0.to(torch.float32)
    return i0, i1, 1.0 - l1, l1


def _resize_torch(x, out_h, out_w, scale_h, scale_w):
    """x [..., Hs, Ws] float32 -> [..., out_h, out_w]; the scales are 0-dim float32 tensors.  One torch operation per rounded one."""
    Hs, Ws = x.shape[-2:]
    y0, y1, l0y, l1y = _axis(out_h, Hs, scale_h, x.device)
    x0, x1, l0x, l1x = _axis(out_w, Ws, scale_w, x.device)
    top, bottom = x.index_select(-2, y0), x.index_select(-2, y1)
    a, b = top.index_select(-1, x0), top.index_select(-1, x1)
    c, d = bottom.index_select(-1, x0), bottom.index_select(-1, x1)
    l0y, l1y = l0y.unsqueeze(-1), l1y.unsqueeze(-1)
    return l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)


def resize_bilinear(x, fs, flip=False, out=None):
    """x [..., H, W] float32 -> [..., floor(H * fs), floor(W * fs)]: F.interpolate(x, scale_factor=fs, mode='bilinear',
    align_corners=False) in plain fp32; with ``flip`` every row is written mirrored (torch.flip(dims=[-1]) of the result, in the same
    pass).  ``out``: a contiguous tensor of the result's shape to write into."""
    if x.dim() < 2 or x.dtype != torch.float32:
        raise RuntimeError('x must be float32 [..., H, W]')
    if not (float(fs) > 0.0 and math.isfinite(float(fs))):
        raise RuntimeError('expected a finite scale factor > 0')
    h, w = scaled_size(x.shape[-2], x.shape[-1], fs)
    if h < 1 or w < 1:
        raise RuntimeError('the scale factor %g leaves no pixel of a %d x %d image' % (fs, x.shape[-2], x.shape[-1]))
    scale = scale_for_factor(fs)
    if _on_kernel(x) and (out is None or _on_kernel(out)):
        return ops.resize_bilinear(x, h, w, scale, scale, flip, out)
    sc = torch.full((), scale, dtype=torch.float32, device=x.device)
    y = _resize_torch(x, h, w, sc, sc)
    if flip:
        y = torch.flip(y, dims=[-1])
    if out is None:
        return y.contiguous()
    out.copy_(y)
    return out


def merge(sources, flipped, size, want_labels=True):
    """sources: 1 .. 8 float32 tensors [N, K, h_e, w_e] (the probabilities of one entry each), flipped: one flag per entry (the entry
    holds a mirrored clip), size = (H, W) -> (mean float32 [N, K, H, W], labels uint8 [N, H, W] or None).

    Per entry v_e = F.interpolate(torch.flip(source) if flipped else source, size=(H, W), mode='bilinear', align_corners=False) with
    torch's scales for size=, fl(float(h_e) / float(H)) and the same for the width; acc = v_0, acc = fl(acc + v_e) in entry order, mean =
    fl(acc / float(E)), a true division; labels = the first index of the maximum of the means over K."""
    sources, flipped = list(sources), [bool(f) for f in flipped]
    E = len(sources)
    if not 1 <= E <= MAX_ENTRIES or len(flipped) != E:
        raise RuntimeError('expected 1 .. %d sources and one flag for each' % MAX_ENTRIES)
    H, W = int(size[0]), int(size[1])
    N, K = sources[0].shape[:2]
    if H < 1 or W < 1 or not 1 <= K <= 255:
        raise RuntimeError('expected a size >= 1 x 1 and 1 <= K <= 255')
    for s in sources:
        if s.dim() != 4 or tuple(s.shape[:2]) != (N, K) or s.dtype != torch.float32 or s.device != sources[0].device:
            raise RuntimeError('the sources must be float32 [N, K, h, w] with the same N and K on one device')
    if _on_kernel(*sources):
        return ops.tta_merge(sources, flipped, H, W, want_labels)
    dev = sources[0].device
    f32 = lambda v: torch.full((), float(v), dtype=torch.float32, device=dev)
    acc = None
    for s, f in zip(sources, flipped):
        v = _resize_torch(torch.flip(s, dims=[-1]) if f else s, H, W, f32(s.shape[2]) / f32(H), f32(s.shape[3]) / f32(W))
        acc = v if acc is None else acc + v
    # (a tensor divisor: torch may turn a division by a Python number into a multiplication by its reciprocal)
    mean = (acc / f32(E)).contiguous()
    return mean, (clip_io.argmax_labels(mean) if want_labels else None)
