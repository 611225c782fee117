# -*- coding: utf-8 -*-
"""The validation loss of the reference's test driver (core/test.py:97), evaluated where the probabilities live:

    loss = lovasz_loss(est_probs, masks) + nll_loss(torch.log(est_probs), masks)

on ``probs`` float32 [N, K, H, W] (what ``RMNet.forward`` returns per clip, what ``segment_video_tta`` returns as 'probs')
and ``labels`` uint8 [N, H, W]; no permute to the reference's [B, C, F, H, W] is made.

Two routes compute it.

* 'hip': ``ops.clip_loss`` (csrc/val_loss.hip).  One streaming pass builds two integer histograms of the errors per class, one
  small scan turns them into a bracket [lo, hi] of every class's Lovasz extension with hi - lo <= 1 / bins, and the value is the
  midpoint.  No sort, no permuted copy, no per-class temporaries, no host synchronisation; the same bits from call to call.
* 'torch': the sort, in this project's own words.  Per present class the errors |fg - p_c| are sorted in descending order, the
  Jaccard index J_i of the i largest errors is taken from two running counts, and the value is sum_i e_(i) (J_i - J_(i-1)).
  The errors are the fp32 values; counts, indices and the sum are float64, so lo == hi == the sorted value up to float64
  rounding.  It runs on CPU tensors and is the A/B yardstick on the device, where its masked selection synchronises.

``training_loss`` is the same loss, differentiable once with respect to ``probs`` (core/train.py:180): on 'hip' an
autograd.Function around ``ops.clip_loss_grad`` (csrc/val_loss_bwd.hip), whose one histogram pass gives value and gradient; on
'torch' autograd through the sort.  The three functions under ``torch.no_grad`` are unchanged by it.

Both leave the same pixels out: a pixel whose label is ``ignore_index``; and, counted in ``n_bad``, a pixel whose label is >= K
or that has a probability outside [0, 1] (NaN included) -- torch's NLLLoss would raise for the former, and a NaN that silently
turns finite has been met here before (profiles/r14_a_glue_tests.md).
"""

import torch

DEFAULT_BINS = 1 << 20

# The route that CUDA tensors take by default: 'hip' or 'torch'.  Measured on an MI355X on a 70-frame 480 x 854 clip at 2^20 bins
# (profiles/r31_a_val_loss.md; HIP events, calls back to back): 'hip' 2.07 ms against 'torch' 12.78 ms with K = 3 and 6.97 ms against
# 43.40 ms with K = 11 on synthetic peaked soft-maxes; 3.45 ms against 12.20 ms and 7.67 ms against 28.65 ms on the output of
# RMNet.forward with procedural weights (saturated: most errors are 0 or 1).  Peak memory above the inputs: 25 MB against 3.2 GB
# (K = 3) and 92 MB against 4.1 GB (K = 11).  'hip' is faster at both K, so no K is routed to 'torch'.
DEVICE_ROUTE = 'hip'


def _route(probs, route):
    if not probs.is_cuda:
        return 'torch'
    route = DEVICE_ROUTE if route is None else route
    if route not in ('hip', 'torch'):
        raise ValueError("route must be 'hip' or 'torch'")
    return route


def _check(probs, labels):
    if probs.dim() != 4 or labels.dim() != 3 or (probs.shape[0],) + tuple(probs.shape[2:]) != tuple(labels.shape):
        raise RuntimeError('expected probs [N, K, H, W] and labels [N, H, W]')
    if probs.dtype != torch.float32 or labels.dtype != torch.uint8:
        raise RuntimeError('expected float32 probabilities and uint8 labels')


def _pixel_classes(probs, labels, ignore_index):
    """(good, bad by label, bad by probability) as bool [N, H, W]."""
    K = probs.shape[1]
    lab = labels.long()
    valid = lab != int(ignore_index) if 0 <= int(ignore_index) <= 255 else torch.ones_like(lab, dtype=torch.bool)
    bad_label = valid & (lab >= K)
    inside = ((probs >= 0) & (probs <= 1)).all(dim=1)
    bad_prob = valid & ~bad_label & ~inside
    return valid & ~bad_label & inside, bad_label, bad_prob


def _torch_pieces(probs, labels, ignore_index):
    """The sort-based route: {'per_class' float64 [K, 3] (G, value, value), 'nll_sum', 'counts' int64 [3]}."""
    K = probs.shape[1]
    good, bad_label, bad_prob = _pixel_classes(probs, labels, ignore_index)
    p = probs.permute(0, 2, 3, 1)[good]                           # [P, K], the good pixels only
    lab = labels[good].long()
    per_class = torch.zeros(K, 3, dtype=torch.float64, device=probs.device)
    for c in range(K):
        fg = lab == c
        G = fg.sum().to(torch.float64)
        if float(G) == 0:
            continue
        e, order = torch.sort((fg.to(torch.float32) - p[:, c]).abs(), descending=True)
        fg_sorted = fg[order].to(torch.float64)
        f = fg_sorted.cumsum(0)                                   # foreground pixels among the i largest errors
        b = (1.0 - fg_sorted).cumsum(0)                           # background pixels among them
        jac = 1.0 - (G - f) / (G + b)
        step = jac.clone()
        step[1:] = jac[1:] - jac[:-1]
        value = (e.to(torch.float64) * step).sum()
        per_class[c, 0], per_class[c, 1], per_class[c, 2] = G, value, value
    p_label = p.gather(1, lab.view(-1, 1)).view(-1) if lab.numel() else p.new_zeros(0)
    nll_sum = -(p_label.to(torch.float64).log()).sum()
    counts = torch.stack([good.sum(), bad_label.sum(), bad_prob.sum()]).to(torch.int64)
    return {'per_class': per_class, 'nll_sum': nll_sum, 'counts': counts}


def _pieces(probs, labels, ignore_index, bins, route):
    _check(probs, labels)
    if _route(probs, route) == 'hip':
        from . import ops
        return ops.clip_loss(probs.contiguous(), labels.contiguous(), ignore_index, bins)
    return _torch_pieces(probs, labels, ignore_index)


def _lovasz_from(per_class):
    present = per_class[:, 0] > 0
    n = present.sum()
    lo = torch.where(present, per_class[:, 1], torch.zeros_like(per_class[:, 1]))
    hi = torch.where(present, per_class[:, 2], torch.zeros_like(per_class[:, 2]))
    value = ((lo + hi) / 2).sum() / n.clamp(min=1).to(torch.float64)      # 0 when no class is present
    return {'value': value, 'lo': lo, 'hi': hi, 'present': present}


def _nll_from(pieces):
    return pieces['nll_sum'] / pieces['counts'][0].to(torch.float64)      # 0 / 0 = NaN with no pixel, as NLLLoss gives


@torch.no_grad()
def lovasz_softmax(probs, labels, ignore_index=255, bins=DEFAULT_BINS, route=None):
    """Lovasz-softmax (models/lovasz_loss.py) of a clip: {'value' float64 0-d: the mean over the present classes of (lo + hi) / 2,
    0 when none is; 'lo', 'hi' float64 [K]: the bracket of every class (0 for an absent one); 'present' bool [K]}."""
    return _lovasz_from(_pieces(probs, labels, ignore_index, bins, route)['per_class'])


@torch.no_grad()
def nll(probs, labels, ignore_index=255, route=None):
    """torch.nn.NLLLoss(ignore_index)(log(probs), labels) with the mean reduction, float64 0-d: +inf when a target probability is
    0, NaN when no pixel counts."""
    return _nll_from(_pieces(probs, labels, ignore_index, 2, route))


@torch.no_grad()
def validation_loss(probs, labels, ignore_index=255, bins=DEFAULT_BINS, route=None):
    """The loss of core/test.py:97: {'loss', 'lovasz', 'nll' float64 0-d, 'n_bad' int64 0-d: the pixels left out for a label >= K
    or a probability outside [0, 1]}, on the device of ``probs``."""
    pieces = _pieces(probs, labels, ignore_index, bins, route)
    lovasz = _lovasz_from(pieces['per_class'])['value']
    nll_value = _nll_from(pieces)
    return {'loss': lovasz + nll_value, 'lovasz': lovasz, 'nll': nll_value, 'n_bad': pieces['counts'][1] + pieces['counts'][2]}


# ------------------------------------------------------------------------------------------------ the training loss
# The route that CUDA tensors take through ``training_loss`` by default, forward + backward.  Measured on an MI355X
# (profiles/r34_a_loss_grad.md; HIP events, 20 / 5 calls back to back, 'hip' against 'torch'), 70-frame 480 x 854 clip at 2^20 bins:
# 3.56 against 29.87 ms with K = 3 and 9.64 against 86.77 ms with K = 11 on synthetic peaked soft-maxes, 5.06 against 30.11 ms and 10.56
# against 58.40 ms on the saturated output of RMNet.forward with procedural weights; a training batch of the reference's config.py
# (12 x 4 x 465 x 465) 2.91 against 3.65 ms.  At 2^12 bins: 0.79 / 2.16 ms (synthetic), 21.69 / 36.26 ms (saturated: vl_hist's
# contended LDS adds) and 0.37 ms (batch), all below the sort's.  Peak memory above the inputs, K = 3 / K = 11: 0.69 / 2.53 GB (the
# saved gradient and its product with grad_output) against 3.99 / 9.50 GB.  'hip' is faster in every case, so no K is routed to 'torch'.
TRAIN_DEVICE_ROUTE = 'hip'


def _check_training(probs, labels, route):
    if probs.dim() != 4 or labels.dim() != 3 or (probs.shape[0],) + tuple(probs.shape[2:]) != tuple(labels.shape):
        raise RuntimeError('expected probs [N, K, H, W] and labels [N, H, W]')
    if labels.dtype != torch.uint8:
        raise RuntimeError('expected uint8 labels')
    if probs.dtype != torch.float32 and not (route == 'torch' and probs.dtype == torch.float64):
        raise RuntimeError("expected float32 probabilities (float64 too on the 'torch' route)")


def _torch_training_loss(probs, labels, ignore_index):
    """The sort, left differentiable: the permutation and the Jaccard steps carry no gradient (models/lovasz_loss.py detaches the
    permutation and computes the steps from the labels alone), abs has derivative 0 at 0, and the NLL is -log(p_label) / good
    pixels.  Steps and sums are float64."""
    K = probs.shape[1]
    good, _, _ = _pixel_classes(probs.detach(), labels, ignore_index)
    p = probs.permute(0, 2, 3, 1)[good]                           # [P, K], the good pixels only
    lab = labels[good].long()
    terms = []
    for c in range(K):
        fg = lab == c
        G = fg.sum().to(torch.float64)
        if float(G) == 0:
            continue
        e, order = torch.sort((fg.to(p.dtype) - p[:, c]).abs(), descending=True)
        fg_sorted = fg[order].to(torch.float64)
        f = fg_sorted.cumsum(0)
        b = (1.0 - fg_sorted).cumsum(0)
        jac = 1.0 - (G - f) / (G + b)
        step = jac.clone()
        step[1:] = jac[1:] - jac[:-1]
        terms.append((e.to(torch.float64) * step).sum())
    lovasz = torch.stack(terms).sum() / len(terms) if terms else p.to(torch.float64).sum() * 0.0
    p_label = p.gather(1, lab.view(-1, 1)).view(-1) if lab.numel() else p.new_zeros(0)
    nll_sum = -(p_label.to(torch.float64).log()).sum()
    return lovasz + nll_sum / good.sum().to(torch.float64)      # 0 / 0 = NaN with no pixel, as NLLLoss gives


class _TrainingLossHip(torch.autograd.Function):
    """Value and gradient from one call of ``ops.clip_loss_grad``: the histogram is built once."""

    @staticmethod
    def forward(ctx, probs, labels, ignore_index, bins):
        from . import ops
        out = ops.clip_loss_grad(probs.contiguous(), labels.contiguous(), ignore_index, bins)
        ctx.save_for_backward(out['grad'])
        return _lovasz_from(out['per_class'])['value'] + _nll_from(out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        grad, = ctx.saved_tensors
        return grad * grad_output.to(grad.dtype), None, None, None


def training_loss(probs, labels, ignore_index=255, bins=DEFAULT_BINS, route=None):
    """lovasz + nll of core/train.py:180 as a float64 0-d tensor on the device of ``probs``, differentiable once with respect to
    ``probs`` (the soft-max in front of them is the network's).  On 'hip' the gradient is the subgradient at the errors quantised
    to ``bins`` bins (csrc/val_loss_bwd.hip): that of the sort where no bin of a class holds two pixels, inside the span of the
    sort's tie orders elsewhere; ignored and bad pixels get 0.  When nothing asks for a gradient the forward entry runs alone."""
    if not probs.is_cuda:
        route = 'torch'
    else:
        route = TRAIN_DEVICE_ROUTE if route is None else route
        if route not in ('hip', 'torch'):
            raise ValueError("route must be 'hip' or 'torch'")
    _check_training(probs, labels, route)
    if route == 'torch':
        return _torch_training_loss(probs, labels, ignore_index)
    if probs.requires_grad and torch.is_grad_enabled():
        return _TrainingLossHip.apply(probs, labels, int(ignore_index), int(bins))
    from . import ops
    pieces = ops.clip_loss(probs.detach().contiguous(), labels.contiguous(), ignore_index, bins)
    return _lovasz_from(pieces['per_class'])['value'] + _nll_from(pieces)
