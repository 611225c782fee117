# -*- coding: utf-8 -*-
"""The two ends of the reference's inference driver (core/inference.py:50-71) where the clip lives: uint8 frames and palette label
maps in, uint8 label maps and overlay frames out.

Input side: ``normalize_frames`` is Normalize + ToTensor (utils/data_transforms.py:41-50, 86-96 with img_normalize,
utils/helpers.py:133-135); ``reorganize_lut`` + ``onehot_labels`` are ReorganizeObjectID + ToOneHot without the shuffle
(utils/data_transforms.py:53-83 with to_onehot, utils/helpers.py:81-90).  Output side: ``argmax_labels`` is the driver's
torch.argmax, ``overlay`` is get_segmentation (utils/helpers.py:138-178) for every frame of a clip at once.

Every function sends contiguous tensors of the kernel's dtype on the GPU to the HIP kernels of csrc/clip_io.hip (``rmnet_amd.ops``)
and everything else -- CPU tensors, other dtypes, strided views -- to a torch restatement that returns the same bytes: each
floating-point operation of the reference's numpy arithmetic is one torch operation in the same precision, so nothing is fused
and nothing is reordered.
"""

import torch

from . import ops

# PALETTE of utils/helpers.py:139-157: the 16 DAVIS colours, then grey [i, i, i]
_DAVIS16 = [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128], [128, 128, 128],
            [64, 0, 0], [191, 0, 0], [64, 128, 0], [191, 128, 0], [64, 0, 128], [191, 0, 128], [64, 128, 128], [191, 128, 128]]
PALETTE = torch.arange(256, dtype=torch.uint8).view(256, 1).repeat(1, 3)
PALETTE[:16] = torch.tensor(_DAVIS16, dtype=torch.uint8)


def _on_kernel(*tensors_and_dtypes):
    """True when every (tensor, dtype) pair is a contiguous GPU tensor of that dtype: the kernels' calling convention."""
    return all(t.is_cuda and t.dtype == d and t.is_contiguous() for t, d in tensors_and_dtypes)


def _triple(v, device):
    return torch.tensor([float(x) for x in v], dtype=torch.float64, device=device)


def normalize_frames(frames, mean, std):
    """frames [N,H,W,3] uint8 -> float32 [N,3,H,W] on the same device:  x = fl32(u / 255.f), y = fl32((double(x) - mean[c]) / std[c]),
    which is img_normalize in numpy's types followed by the loader's astype(float32) and ToTensor's permute."""
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise RuntimeError('frames must be [N, H, W, 3]')
    if _on_kernel((frames, torch.uint8)):
        return ops.frames_normalize(frames, mean, std)
    # (a tensor divisor: torch may turn a division by a Python number into a multiplication by its reciprocal)
    x = frames.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32, device=frames.device)
    y =(x.to(torch.float64) - _triple(mean, frames.device)) / _triple(std, frames.device)
    return y.to(torch.float32).permute(0, 3, 1, 2).contiguous()


def reorganize_lut(labels, ignore_idx=255):
    """ReorganizeObjectID as a table: the ids present anywhere in ``labels`` (any shape, integer values 0 .. 255) without
    ``ignore_idx``, in ascending order, map to 0, 1, 2, ...; the ignore id and absent ids map to 0.  Returns ``(lut, n_ids)``: a
    uint8 [256] table and the number of ids as a 0-dim int64 tensor, both on the device of ``labels`` and computed there without a
    host synchronisation (a 256-bin presence vector, a cumulative sum, a mask)."""
    present = torch.zeros(256, dtype=torch.int64, device=labels.device)
    present.scatter_(0, labels.reshape(-1).to(torch.int64), 1)
    if 0 <= int(ignore_idx) < 256:
        present[int(ignore_idx)] = 0
    rank = torch.cumsum(present, 0) - 1
    lut = torch.where(present > 0, rank, torch.zeros_like(rank)).to(torch.uint8)
    return lut, present.sum()


def onehot_labels(labels, K, lut=None):
    """labels [N,H,W] integer -> uint8 [N,K,H,W], plane k = (lut[label] == k) (``lut``: a uint8 [256] table such as
    reorganize_lut's, None for the identity).  A remapped label >= K sets no plane, as in to_onehot."""
    if labels.dim() != 3:
        raise RuntimeError('labels must be [N, H, W]')
    K = int(K)
    if not 1 <= K <= 255:
        raise RuntimeError('expected 1 <= K <= 255')
    if _on_kernel((labels, torch.uint8)) and (lut is None or _on_kernel((lut, torch.uint8))):
        return ops.labels_onehot(labels, K, lut)
    m = labels.to(torch.int64)
    if lut is not None:
        m = lut.to(labels.device).to(torch.int64)[m]
    ids = torch.arange(K, device=labels.device).view(1, K, 1, 1)
    return (m.unsqueeze(1) == ids).to(torch.uint8)


def restore_ids(labels, ids):
    """labels [...] of plane indices (what ``argmax_labels`` returns) -> uint8 [...] in the clip's own ids: ``ids[labels]`` with
    ``ids`` the ascending raw ids (``reorganize_lut``'s inverse; ``ObjectPlan.ids``).  A plane beyond the ids (no object of the
    clip lives there) maps to 0, so no index leaves the table."""
    ids = torch.as_tensor(ids, dtype=torch.uint8, device=labels.device).reshape(-1)
    table = torch.zeros(256, dtype=torch.uint8, device=labels.device)
    table[:ids.numel()] = ids
    return table[labels.to(torch.uint8).to(torch.int64)]


def argmax_labels(prob):
    """prob [N,K,H,W] -> uint8 [N,H,W], the first index of the maximum over K (1 <= K <= 255)."""
    if prob.dim() != 4 or not 1 <= prob.shape[1] <= 255:
        raise RuntimeError('prob must be [N, K, H, W] with 1 <= K <= 255')
    if _on_kernel((prob, torch.float32)):
        return ops.argmax_labels(prob)
    return prob.argmax(dim=1).to(torch.uint8)


def _trunc_u8(v):
    """(uint8) of a float64 tensor as numpy casts values in (-1, 256): towards zero; saturated outside, NaN -> 0."""
    return torch.nan_to_num(v, nan=0.0).clamp(0.0, 255.0).to(torch.uint8)


def _overlay_torch(frames, labels, mean, std, ignore_idx, alpha):
    N, _, H, W = frames.shape
    dev = frames.device
    alpha = float(alpha)
    v = _trunc_u8((frames.to(torch.float64).permute(0, 2, 3, 1) * _triple(std, dev) + _triple(mean, dev)) * 255.0)      # [N,H,W,3]
    L = labels.to(torch.int16)
    lowest = L.flatten(1).min(dim=1).values.view(N, 1, 1)
    padded = torch.nn.functional.pad(L, (1, 1, 1, 1), value=-1)
    around = torch.stack([padded[:, 1:-1, :-2], padded[:, 1:-1, 2:], padded[:, :-2, 1:-1], padded[:, 2:, 1:-1]])
    event = (around >= 0) & (around != L) & (around != lowest) & (around != int(ignore_idx))
    highest = torch.where(event, around, torch.full_like(around, -1)).max(dim=0).values
    first = torch.where(event, around, torch.full_like(around, 256)).min(dim=0).values
    mine = (L != lowest) & (L != int(ignore_idx))
    zero = torch.where(mine, highest > L, highest >= 0)
    start = torch.where((mine & (first < L)).unsqueeze(-1), torch.zeros_like(v), v)
    colour = PALETTE.to(dev)[L.to(torch.int64)].to(torch.float64)
    blended = _trunc_u8(start.to(torch.float64) * alpha + (1.0 - alpha) * colour)
    out = torch.where(mine.unsqueeze(-1), blended, v)
    return torch.where(zero.unsqueeze(-1), torch.zeros_like(out), out).contiguous()


def overlay(frames, labels, mean, std, ignore_idx=255, alpha=0.4):
    """frames [N,3,H,W] float32 (normalised), labels [N,H,W] integer -> uint8 [N,H,W,3]: get_segmentation of every frame.

    Per pixel: v_c = (uint8) trunc((double(x_c) * std[c] + mean[c]) * 255.0).  S = the labels present in the frame minus the
    smallest one present (np.unique(mask)[1:]) minus ``ignore_idx``.  Of the pixel's own label and its 4-neighbours' labels
    inside the image, those in S act in ascending order: the own label o blends, v_c = (uint8) trunc(double(v_c) * alpha +
    (1.0 - alpha) * double(PALETTE[o][c])); another label blackens the pixel (it lies on that object's contour).  Every product
    and sum is rounded on its own."""
    if frames.dim() != 4 or frames.shape[1] != 3 or labels.dim() != 3 or labels.shape != frames.shape[:1] + frames.shape[2:]:
        raise RuntimeError('expected frames [N, 3, H, W] and labels [N, H, W]')
    if not 0.0 <= float(alpha) <= 1.0:
        raise RuntimeError('expected 0 <= alpha <= 1')
    if _on_kernel((frames, torch.float32), (labels, torch.uint8)):
        return ops.overlay(frames, labels, mean, std, ignore_idx, alpha)
    return _overlay_torch(frames, labels.to(frames.device), mean, std, ignore_idx, alpha)


def denormalize_frames(frames, mean, std):
    """frames [N,3,H,W] float32 -> uint8 [N,H,W,3], img_denormalize (utils/helpers.py:127-130) of every frame: the overlay of a
    label map that holds one label throughout, whose set S is empty."""
    labels = torch.zeros(frames.shape[:1] + frames.shape[2:], dtype=torch.uint8, device=frames.device)
    return overlay(frames, labels, mean, std)
