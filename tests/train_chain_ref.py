# -*- coding: utf-8 -*-
"""The training chain as one chain, for tests/test_train_chain.py: r4 leaves -> the key / value heads (memory and query) -> the
expansion over the objects of a clip -> the regional memory read -> the decoder -> the decoder tail -> prob, and one backward of
sum(prob * cotangent) into every leaf and every parameter.  Plain functions; pytest collects nothing here.

``chain`` runs it in one of two modes.  ``device_grad=True``: the modules on the device, channels-last, ``fuse_epilogues_``,
``Decoder.device_grad_(glue=True)``, ``KeyValue.device_grad_()`` on both heads and ``ops.memory_read`` for the read -- every block's
backward is then one of the project's kernels.  ``device_grad=False``: the same module graph on torch ops (the CPU, float32 or
float64), with the read as the masked restatement of tests/test_memory_read_backward.py (models/rmnet.py:147-165) per object.  The
float64 run of the second mode is the truth; its float32 run is the yardstick (what autograd through a float32 library costs).

The cotangent is FIXED: the gradient of ``losses.training_loss`` at the float64 chain's prob, rounded to float32
(``loss_cotangent``), handed to every run.  All runs then differentiate the same smooth function sum(prob * c); no sort order and no
arg-max of the loss enters the comparison, while c keeps the loss's real shape (its magnitudes span more than 2^30).

The two cases are the smallest at which every seam exists (h w below every tile; at most two objects per clip, so the expansion's
backward adds two numbers and has one summation order):
  multi   n_objects [2, 1], K 4 (one channel beyond the count), T 2, 3 x 5 cells, frame 41 x 70 padded to 48 x 80 (all four pads
          non-zero), proper sub-rectangles that differ per object and frame, ``index_select`` over ``batch_of_obj``.
  single  n_objects [1, 1], K 2, T 1, 2 x 3 cells, frame 32 x 48 (no pad): the "object i is clip i" branch of ``_segment_core``,
          the query heads given ``kv_rects``.
"""

import copy
import functools

import torch

FAULTS = ('key_frames_swapped', 'q_val_unmasked', 'r2_not_summed', 'pad_shifted', 'sqrt_is_De', 'dec_channels_swapped')

SHAPES = {
    # (x0, x1, y0, y1), both ends inclusive: mem_rects [no][T], qry_rects [no]
    'multi': dict(n_objects=[2, 1], K=4, T=2, h=3, w=5, frame=(41, 70),
                  mem_rects=[[(0, 3, 0, 1), (1, 4, 1, 2)], [(1, 3, 0, 2), (0, 2, 1, 2)], [(2, 4, 0, 1), (0, 4, 0, 1)]],
                  qry_rects=[(0, 3, 0, 2), (1, 4, 0, 1), (1, 3, 1, 2)]),
    'single': dict(n_objects=[1, 1], K=2, T=1, h=2, w=3, frame=(32, 48),
                   mem_rects=[[(0, 1, 0, 1)], [(1, 2, 0, 0)]], qry_rects=[(0, 1, 0, 1), (1, 2, 0, 1)]),
}


def make_case(name, seed):
    """The case's shapes, rectangles, labels and leaves (float32 values from ``seed``; every run starts from copies of them)."""
    from rmnet_amd import helpers
    s = SHAPES[name]
    n_objects, T, h, w = s['n_objects'], s['T'], s['h'], s['w']
    B, no = len(n_objects), sum(n_objects)
    H, W = s['frame']
    pad = helpers.pad_amounts(H, W, 16)
    assert (H + pad[2] + pad[3], W + pad[0] + pad[1]) == (16 * h, 16 * w)
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    leaves = {'r4m%d' % t: r(no, 1024, h, w) for t in range(T)}
    leaves.update(r4q=r(B, 1024, h, w), r3=r(B, 512, 2 * h, 2 * w), r2=r(B, 256, 4 * h, 4 * w))
    classes = 3 if name == 'multi' else 2
    labels = (torch.arange(B * H * W).view(B, H, W) % classes).to(torch.uint8)
    return dict(name=name, seed=seed, n_objects=n_objects, B=B, no=no, K=s['K'], T=T, h=h, w=w, H=H, W=W, pad=pad, leaves=leaves,
                labels=labels, batch_of_obj=[b for b, n in enumerate(n_objects) for _ in range(n)],
                mem_rects=torch.tensor(s['mem_rects'], dtype=torch.int32).view(no, T, 4),
                qry_rects=torch.tensor(s['qry_rects'], dtype=torch.int32).view(no, 4))


@functools.lru_cache(maxsize=None)
def _initial_modules():
    from rmnet_amd import networks
    mods = torch.nn.ModuleDict(dict(decoder=networks.Decoder(256), kv_memory=networks.KeyValue(1024, 128, 512),
                                    kv_query=networks.KeyValue(1024, 128, 512)))
    return networks.procedural_init_(mods)            # (the fill is a hash of the state-dict key: the two heads differ)


def build_modules(dtype, device, device_grad=False):
    """The three modules at their procedural weights, ready for ``chain`` (``modules=``): a test that takes optimiser steps keeps
    them from one call to the next."""
    from rmnet_amd import networks
    mods = copy.deepcopy(_initial_modules()).to(dtype)
    if device_grad:
        mods = mods.to(device).to(memory_format=torch.channels_last)
        networks.fuse_epilogues_(mods)
        mods['decoder'].device_grad_(glue=True)
        mods['kv_memory'].device_grad_()
        mods['kv_query'].device_grad_()
    else:
        mods = mods.to(device)
    return mods.train()


def param_names(mods):
    return [n for n, _ in mods.named_parameters()]


def inside(rect, h, w, dtype=torch.float64, device='cpu'):
    """The 0 / 1 map [h * w] of the cells inside ``rect`` = (x0, x1, y0, y1), by comparison (nothing is clamped)."""
    x0, x1, y0, y1 = (int(v) for v in rect)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    return ((xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)).reshape(-1).to(dtype).to(device)


def read(m_key, m_val, q_key, q_val, mem_rects, qry_rects, fault=None):
    """The masked torch restatement of the regional read, per object: m_key [no, De, T, h, w], m_val [no, Do, T, h, w], q_key
    [no, De, h, w], q_val [no, Do, h, w] -> [no, 2 Do, h, w]."""
    no, De, T, h, w = m_key.shape
    Do = m_val.shape[1]
    outs = []
    for o in range(no):
        mm = torch.cat([inside(mem_rects[o, t], h, w, m_key.dtype, m_key.device) for t in range(T)])
        qm = inside(qry_rects[o], h, w, m_key.dtype, m_key.device)
        km, vm = m_key[o].reshape(De, -1) * mm[None, :], m_val[o].reshape(Do, -1) * mm[None, :]
        qq, qv = q_key[o].reshape(De, -1) * qm[None, :], q_val[o].reshape(Do, -1)
        p = torch.softmax(km.t() @ qq / (float(De) if fault == 'sqrt_is_De' else De ** 0.5), dim=0)
        outs.append(torch.cat([vm @ p, qv if fault == 'q_val_unmasked' else qv * qm[None, :]], dim=0).view(2 * Do, h, w))
    return torch.stack(outs)


class _SelectLastWins(torch.autograd.Function):
    """``index_select`` over dim 0 whose backward keeps one object's gradient per clip instead of their sum (a planted fault)."""

    @staticmethod
    def forward(ctx, x, index):
        ctx.index, ctx.n = index, x.shape[0]
        return x.index_select(0, index)

    @staticmethod
    def backward(ctx, g):
        out = g.new_zeros((ctx.n,) + tuple(g.shape[1:]))
        for i, b in enumerate(ctx.index.tolist()):
            out[b] = g[i]
        return out, None


def loss_cotangent(prob, labels):
    """d training_loss / d prob at ``prob`` (float64, the CPU: the sort-based route), rounded to float32."""
    from rmnet_amd import losses
    p = prob.detach().double().cpu().requires_grad_(True)
    losses.training_loss(p, labels.cpu()).backward()
    return p.grad.float()


def heads(mods, case, leaves, device, device_grad, fault=None):
    """(m_key, m_val, q_key, q_val) as the read takes them: the memory heads per frame stacked on dim 2, the query heads expanded
    over the objects of each clip."""
    T, n_objects = case['T'], case['n_objects']
    mem_rects = case['mem_rects'].to(device)
    qry_rects = case['qry_rects'].to(device)
    kvs = [mods['kv_memory'](leaves['r4m%d' % t], mem_rects[:, t].contiguous()) for t in range(T)]
    keys = [k for k, _ in kvs]
    m_key = torch.stack(keys[::-1] if fault == 'key_frames_swapped' else keys, dim=2)
    m_val = torch.stack([v for _, v in kvs], dim=2)
    one_each = all(n == 1 for n in n_objects)
    q_key, q_val = mods['kv_query'](leaves['r4q'], qry_rects) if one_each else mods['kv_query'](leaves['r4q'])
    if not one_each:
        idx = torch.tensor(case['batch_of_obj'], dtype=torch.int64, device=device)
        q_key, q_val = q_key.index_select(0, idx), q_val.index_select(0, idx)
    return m_key, m_val, q_key, q_val


def chain(dtype, device, case, cotangent=None, labels=None, fault=None, device_grad=False, modules=None):
    """One forward and one backward of the chain.  ``cotangent``: a tensor like prob; None -- ``loss_cotangent`` of this run's own
    prob (the float64 CPU run does this once, every other run is given its result); 'loss' -- no cotangent at all:
    ``losses.training_loss(prob, labels).backward()``.  ``fault``: one of FAULTS, planted in this run.  ``modules``: those of
    ``build_modules`` (their gradients are cleared first); default: fresh ones.
    Returns (the decoder's logits, prob, {name: gradient}) as float64 CPU tensors: the T + 3 leaves and every parameter."""
    from rmnet_amd import losses, ops
    from rmnet_amd.rmnet import RMNet
    device = torch.device(device)
    assert fault is None or fault in FAULTS
    assert not device_grad or (device.type == 'cuda' and dtype == torch.float32)
    labels = case['labels'] if labels is None else labels
    mods = build_modules(dtype, device, device_grad) if modules is None else modules
    mods.zero_grad(set_to_none=True)
    leaves = {}
    for name, v in case['leaves'].items():
        v = v.detach().clone().to(device, dtype)          # (a copy: the case's own tensors never become leaves of a graph)
        if device_grad:
            v = v.contiguous(memory_format=torch.channels_last)
        leaves[name] = v.requires_grad_(True)
    n_objects, K, pad = case['n_objects'], case['K'], case['pad']
    m_key, m_val, q_key, q_val = heads(mods, case, leaves, device, device_grad, fault)
    r3e, r2e = leaves['r3'], leaves['r2']
    if not all(n == 1 for n in n_objects):
        idx = torch.tensor(case['batch_of_obj'], dtype=torch.int64, device=device)
        r3e = r3e.index_select(0, idx)
        r2e = _SelectLastWins.apply(r2e, idx) if fault == 'r2_not_summed' else r2e.index_select(0, idx)
    if device_grad:
        m4, _ = ops.memory_read(m_key.contiguous(), m_val.contiguous(), q_key.contiguous(), q_val.contiguous(),
                                case['mem_rects'].to(device), case['qry_rects'].to(device))
    else:
        m4 = read(m_key, m_val, q_key, q_val, case['mem_rects'], case['qry_rects'], fault)
    dec = mods['decoder'](m4, r3e, r2e)
    if fault == 'pad_shifted':
        pad = (pad[0] + 1, pad[1] - 1, pad[2], pad[3])
    tail = RMNet(None).train().decoder_tail
    _, prob = tail(dec.flip(1) if fault == 'dec_channels_swapped' else dec, n_objects, K, pad)
    if isinstance(cotangent, str):
        assert cotangent == 'loss'
        losses.training_loss(prob, labels.to(device)).backward()
    else:
        c = loss_cotangent(prob, labels) if cotangent is None else cotangent
        (prob * c.to(device, dtype)).sum().backward()
    grads = {name: v.grad for name, v in leaves.items()}
    grads.update({name: p.grad for name, p in mods.named_parameters()})
    assert all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]
    f64 = lambda t: t.detach().cpu().double().contiguous()
    return f64(dec), f64(prob), {k: f64(g) for k, g in grads.items()}


def errors(got, want):
    """{name: max|got - want| / max|want|}."""
    assert set(got) == set(want)
    return {k: float((got[k] - want[k]).abs().max() / want[k].abs().max()) for k in want}


def clip_rows(case, b):
    """{leaf: the rows of clip ``b``}: its own row of r4q / r3 / r2, its objects' rows of every r4m."""
    objs = [o for o, bb in enumerate(case['batch_of_obj']) if bb == b]
    rows = {'r4m%d' % t: objs for t in range(case['T'])}
    rows.update(r4q=[b], r3=[b], r2=[b])
    return rows


def clip_errors(case, got, want, b):
    """``errors`` over the rows of clip ``b`` alone, relative to that clip's own largest gradient."""
    rows = clip_rows(case, b)
    return {k: float((got[k][r] - want[k][r]).abs().max() / want[k][r].abs().max()) for k, r in rows.items()}


def sgd_step_(mods, lr):
    """Plain SGD in place on every parameter (each ``_version`` moves: the packs must follow)."""
    with torch.no_grad():
        for p in mods.parameters():
            p.add_(p.grad, alpha=-lr)
