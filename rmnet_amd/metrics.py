# -*- coding: utf-8 -*-
"""Region similarity J (Jaccard index) and boundary measure F evaluated where the label maps live.

Restates ``utils/metrics.py:84-102`` of the reference (J = |seg & ann| / |seg | ann|, and 1 when both
are empty) with tensor ops that run on the GPU without a host synchronisation, so that a sharded
evaluation exchanges scalars over RCCL (``rmnet_amd.dist.sum_over_ranks``) instead of label maps.

F (``utils/metrics.py:119-226``) is four exact integer counts per (frame, object) -- the sizes of the two boundary maps and of
each one's part inside the other's dilation by a disk -- followed by a few float64 operations.  uint8 label maps on the GPU get
their counts from the HIP kernel (``ops.boundary_match``, csrc/boundary_f.hip); everything else takes the torch restatement below,
which returns the same integers.  J-Mean, F-Mean and JF-Mean are the reference's three scores (``utils/metrics.py:22-41``).
"""

import numpy as np
import torch
import torch.nn.functional as F


def jaccard_per_object(pred_labels, gt_labels, n_objects):
    """pred_labels, gt_labels: integer label maps [N, H, W] (0 = background) on any device.
    Returns J as float64 [N, n_objects] for objects 1..n_objects (device of the inputs, no sync)."""
    if pred_labels.shape != gt_labels.shape or pred_labels.dim() != 3:
        raise RuntimeError('expected two [N, H, W] label maps of the same shape')
    ids = torch.arange(1, n_objects + 1, device=pred_labels.device).view(1, -1, 1, 1)
    seg = pred_labels.unsqueeze(1) == ids
    ann = gt_labels.unsqueeze(1) == ids
    inter = (seg & ann).flatten(2).sum(2).to(torch.float64)
    union = (seg | ann).flatten(2).sum(2).to(torch.float64)
    return torch.where(union == 0, torch.ones_like(union), inter / union.clamp(min=1))


def mean_jaccard(pred_labels, gt_labels, n_objects, skip_first_and_last=True):
    """Mean J over objects and frames; DAVIS convention drops the first (given) and the last frame.

    The reference's own test loop differs in two ways (``utils/metrics.py:70-81``, ``core/test.py:104-141``): it drops frame 0
    only, and it takes ``n_objects`` as the clip's largest ground-truth label.  Pass ``skip_first_and_last=False`` with frames
    ``[1:]`` and that count to score a clip its way; the same holds for ``mean_boundary_f``."""
    j = jaccard_per_object(pred_labels, gt_labels, n_objects)
    if skip_first_and_last and j.shape[0] > 2:
        j = j[1:-1]
    return j.mean()


# ------------------------------------------------------------------------------------------------ boundary measure F
def boundary_radius(H, W, bound_th=0.008):
    """The disk's radius in pixels for an H x W frame (utils/metrics.py:134-135): ``bound_th`` itself when it is >= 1, else
    ceil(bound_th * |(H, W)|), computed on the host in float64 as the reference does.  8 at 480x854, 18 at 1080x1920."""
    if bound_th >= 1:
        return bound_th
    return int(np.ceil(bound_th * np.linalg.norm((H, W))))


def _disk(radius, device):
    """skimage.morphology.disk(radius) as a float32 [1, 1, 2r+1, 2r+1] convolution weight."""
    ax = torch.arange(-radius, radius + 1, device=device)
    return ((ax.view(-1, 1) ** 2 + ax.view(1, -1) ** 2) <= radius * radius).to(torch.float32).view(1, 1, 2 * radius + 1, 2 * radius + 1)


def _bmap(seg):
    """seg2bmap at the map's own size (utils/metrics.py:202-213) over the last two dimensions of a bool tensor."""
    e, s, se = torch.zeros_like(seg), torch.zeros_like(seg), torch.zeros_like(seg)
    e[..., :, :-1] = seg[..., :, 1:]
    s[..., :-1, :] = seg[..., 1:, :]
    se[..., :-1, :-1] = seg[..., 1:, 1:]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[..., -1, :] = seg[..., -1, :] ^ e[..., -1, :]
    b[..., :, -1] = seg[..., :, -1] ^ s[..., :, -1]
    b[..., -1, -1] = False
    return b


def _dilate(b, disk):
    """binary_dilation with zeros outside the image: a pixel is set when the disk centred on it covers a set pixel.  The sums are
    small integers in fp32, exact; the threshold sits between 0 and 1 so that a convolution algorithm that rounds (a transform-domain
    one on the GPU) cannot turn an empty neighbourhood into a set pixel."""
    r = disk.shape[-1] // 2
    return F.conv2d(b.flatten(0, 1).unsqueeze(1).to(torch.float32), disk, padding=r).view(b.shape) > 0.5


_TORCH_PATH_PIXELS = 1 << 24      # frames x objects x pixels per convolution of the torch restatement (memory, not results)


def _boundary_counts_torch(pred_labels, gt_labels, n_objects, radius):
    N, H, W = pred_labels.shape
    dev = pred_labels.device
    ids = torch.arange(1, n_objects + 1, device=dev).view(1, -1, 1, 1)
    disk = _disk(radius, dev)
    step = max(1, _TORCH_PATH_PIXELS // max(1, n_objects * H * W))
    out = []
    for n0 in range(0, N, step):
        fg = _bmap(pred_labels[n0:n0 + step].unsqueeze(1) == ids)
        gt = _bmap(gt_labels[n0:n0 + step].unsqueeze(1) == ids)
        fg_match = fg & _dilate(gt, disk)          # utils/metrics.py:143, 148
        gt_match = gt & _dilate(fg, disk)          # utils/metrics.py:141, 147
        out.append(torch.stack([m.flatten(2).sum(2) for m in (fg, gt, fg_match, gt_match)], dim=2))
    return torch.cat(out).to(torch.int32)


def boundary_counts(pred_labels, gt_labels, n_objects, radius):
    """pred_labels, gt_labels: integer label maps [N, H, W] (0 = background) on any device.  Returns int32 [N, n_objects, 4]:
    (n_fg, n_gt, fg_match, gt_match) for objects 1..n_objects -- |bmap(pred)|, |bmap(gt)|, |bmap(pred) & dilate(bmap(gt))| and
    |bmap(gt) & dilate(bmap(pred))| with the reference's seg2bmap and disk(radius) (utils/metrics.py:137-152).  Contiguous uint8
    maps on the GPU go to the HIP kernel; CPU tensors, other integer types and strided views take the torch restatement, which
    returns the same integers."""
    if pred_labels.shape != gt_labels.shape or pred_labels.dim() != 3:
        raise RuntimeError('expected two [N, H, W] label maps of the same shape')
    radius, n_objects = int(radius), int(n_objects)
    if radius < 0 or n_objects < 1:
        raise RuntimeError('expected radius >= 0 and n_objects >= 1')
    if all(t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() for t in (pred_labels, gt_labels)):
        from . import ops
        return ops.boundary_match(pred_labels, gt_labels, n_objects, radius)
    return _boundary_counts_torch(pred_labels, gt_labels, n_objects, radius)


def f_from_counts(counts):
    """counts [..., 4] = (n_fg, n_gt, fg_match, gt_match) -> F as float64 [...]: the four cases of utils/metrics.py:155-169 as
    tensor ops (no host sync).  An empty prediction against a non-empty truth has P = 1, R = 0; the reverse P = 0, R = 1; both
    empty P = R = 1; otherwise P = fg_match / n_fg and R = gt_match / n_gt.  F = 2 P R / (P + R), and 0 when P + R = 0."""
    n_fg, n_gt, fg_match, gt_match = counts.to(torch.float64).unbind(-1)
    one, zero = torch.ones_like(n_fg), torch.zeros_like(n_fg)
    precision = torch.where(n_fg == 0, one, torch.where(n_gt == 0, zero, fg_match / n_fg.clamp(min=1)))
    recall = torch.where(n_gt == 0, one, torch.where(n_fg == 0, zero, gt_match / n_gt.clamp(min=1)))
    total = precision + recall
    return torch.where(total == 0, zero, 2 * precision * recall / torch.where(total == 0, one, total))


def boundary_f_per_object(pred_labels, gt_labels, n_objects, bound_th=0.008):
    """F as float64 [N, n_objects] for objects 1..n_objects (device of the inputs, no sync): utils/metrics.py:119-169 per frame
    and object, the radius from the frame size by the reference's rule."""
    radius = boundary_radius(pred_labels.shape[-2], pred_labels.shape[-1], bound_th)
    return f_from_counts(boundary_counts(pred_labels, gt_labels, n_objects, radius))


def mean_boundary_f(pred_labels, gt_labels, n_objects, skip_first_and_last=True):
    """Mean F over objects and frames, with mean_jaccard's frame convention (see there for the reference's own)."""
    f = boundary_f_per_object(pred_labels, gt_labels, n_objects)
    if skip_first_and_last and f.shape[0] > 2:
        f = f[1:-1]
    return f.mean()


def jf_mean(j, f):
    """JF-Mean (utils/metrics.py:228-230)."""
    return (j + f) / 2
