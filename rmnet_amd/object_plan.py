# -*- coding: utf-8 -*-
"""Objects that are first annotated in the middle of a clip (the YouTube-VOS protocol), planned once per clip.

The reference spreads this over three places: its loader counts the objects cumulatively, one count per frame
(utils/data_loaders.py:58-65), ReorganizeObjectID renumbers the ids over the whole clip (utils/data_transforms.py:53-68), and
RMNet.forward injects a new object's annotation into the logits at the frame where the count changes and pins the object's logit
to -16.1181 until then (models/rmnet.py:398-407, 436-450).  All of it follows from WHICH ids every frame holds, so here

  ``label_presence``    reduces the clip's label maps to a 256-bit set per frame on the device (csrc/late_objects.hip),
  ``appearance_plan``   downloads those N x 32 bytes -- the one host synchronisation -- and derives on the host the id table, the
                        per-frame counts, the frames with edits and a per-frame, per-channel action (0 keep, 1 absent, 2 inject),
  ``object_edit_softmax``  applies one frame's actions to the logits and writes their soft-max, in one launch.

Under multi-scale and flipped inference (utils/helpers.py:44-78) the reference nearest-resizes the one-hot masks of every frame and
hands them to the network with the loader's full-size counts.  Resizing one-hot planes by nearest neighbour and taking their argmax
equals applying the clip's table to the sampled label, so per scale only ``seen`` changes: ``label_presence_scaled`` gives the
presence of the sampled maps of all scales in one launch, ``appearance_plans`` one plan per scale from ONE download -- counts, ids
and fresh frames from the full-size presence, ``seen`` from the sampled one --, and ``object_edit_softmax(sampling=)`` reads the
injected plane at the sampled, possibly mirrored position of the full-size label map.  The mirrored pass uses the same plan.

``RMNet.forward(..., object_plan=(labels, [plan per clip]))`` consumes the plan: no one-hot masks of any frame but the first, no
torch.unique per frame.  Contiguous GPU tensors of the kernels' dtypes go to the kernels, everything else to a torch restatement
that returns the same words / the same logit bits.
"""

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from . import tta

ABSENT_LOGIT = -16.1181          # models/rmnet.py:448
NEW_OBJECT_SCALE = 32.0605       # models/rmnet.py:442
KEEP, ABSENT, INJECT = 0, 1, 2


class ObjectPlan(object):
    """What ``appearance_plan`` returns.  Host fields: ``K``, ``ids`` (ascending raw ids, numpy uint8), ``n_objects`` (list, one
    clamped cumulative count per frame), ``n_max``, ``fresh`` (set of frames whose count differs from the frame before),
    ``seen`` (list of sets of planes per frame), ``action_host`` (numpy uint8 [N,K]), ``edited`` (set of frames with a non-zero
    action).  Device fields: ``lut`` uint8 [256], ``ids_dev`` uint8 [len(ids)], ``action`` uint8 [N,K]."""

    def __init__(self, K, lut_host, ids, n_objects, fresh, seen, action_host, device):
        self.K = int(K)
        self.lut_host = lut_host
        self.ids = ids
        self.n_objects = [int(n) for n in n_objects]
        self.n_max = self.n_objects[-1]
        self.fresh = set(fresh)
        self.seen = seen
        self.action_host = action_host
        self.edited = {t for t in range(action_host.shape[0]) if action_host[t].any()}
        self.lut = torch.from_numpy(lut_host).to(device)
        self.ids_dev = torch.from_numpy(ids).to(device)
        self.action = torch.from_numpy(action_host).to(device)


def _presence_torch(labels):
    N = labels.shape[0]
    present = torch.zeros(N, 256, dtype=torch.int64, device=labels.device)
    present.scatter_(1, labels.reshape(N, -1).to(torch.int64), 1)
    words = (present.view(N, 8, 32) << torch.arange(32, device=labels.device)).sum(dim=2)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def label_presence(labels):
    """labels [N,H,W], integer values 0 .. 255 -> int32 [N,8] on the same device: bit ``v & 31`` of word ``v >> 5`` of row n is set
    exactly when value v occurs in frame n (uint32 words carried as int32).  No host synchronisation."""
    if labels.dim() != 3:
        raise RuntimeError('labels must be [N, H, W]')
    if labels.is_cuda and labels.dtype == torch.uint8 and labels.is_contiguous() and labels.numel() > 0:
        return ops.label_presence(labels)
    return _presence_torch(labels)


def presence_sets(presence):
    """int32 / uint32 [N,8] words (tensor or array) -> list of N ascending lists of the values present.  Downloads a tensor."""
    if isinstance(presence, torch.Tensor):
        presence = presence.detach().cpu().numpy()
    words = np.ascontiguousarray(presence).astype(np.int64) & 0xffffffff
    if words.ndim != 2 or words.shape[1] != 8:
        raise RuntimeError('presence must be [N, 8]')
    return [[v for v in range(256) if (int(row[v >> 5]) >> (v & 31)) & 1] for row in words]


def label_presence_scaled(labels, H, W, frame_scales):
    """labels [N,H,W], integer values 0 .. 255, and S scale factors -> int32 [S,N,8] on the same device: row (s, n) is
    ``label_presence`` of frame n nearest-resized by factor s -- to ``tta.scaled_size(H, W, fs)`` with ``tta.nearest_index`` per
    axis -- without the resized map.  One launch for all scales for contiguous uint8 GPU tensors, a torch restatement otherwise.
    No host synchronisation."""
    if labels.dim() != 3 or tuple(labels.shape[1:]) != (int(H), int(W)):
        raise RuntimeError('labels must be [N, H, W]')
    scales = [float(fs) for fs in frame_scales]
    if not 1 <= len(scales) <= tta.MAX_ENTRIES:
        raise RuntimeError('expected 1 .. %d scales' % tta.MAX_ENTRIES)
    sizes = [tta.scaled_size(H, W, fs) for fs in scales]
    if any(h < 1 or w < 1 for h, w in sizes):
        raise RuntimeError('a scale factor leaves no pixel of a %d x %d label map' % (H, W))
    if labels.is_cuda and labels.dtype == torch.uint8 and labels.is_contiguous() and labels.numel() > 0:
        steps = [tta.scale_for_factor(fs) for fs in scales]
        return ops.label_presence_nearest(labels, sizes, [(s, s) for s in steps])
    out = []
    for fs, (h, w) in zip(scales, sizes):
        iy = torch.from_numpy(tta.nearest_index(h, H, fs)).to(labels.device)
        ix = torch.from_numpy(tta.nearest_index(w, W, fs)).to(labels.device)
        out.append(_presence_torch(labels.index_select(1, iy).index_select(2, ix)))
    return torch.stack(out)


def _plan_from_sets(frames, sampled, n_max_objects, ignore_idx, dev):
    """``appearance_plan`` on the value lists of every frame: ``frames`` at full size, ``sampled`` what the network's masks hold."""
    N = len(frames)
    if N < 1 or len(sampled) != N:
        raise RuntimeError('the clip has no frame' if N < 1 else 'presence and sampled must hold the same frames')
    n_cap = int(n_max_objects)
    K = n_cap + 1
    if not 1 <= K <= 255:
        raise RuntimeError('expected 0 <= n_max_objects <= 254')
    ignore = int(ignore_idx)
    ids = sorted(set(v for f in frames for v in f if v != ignore))
    lut = np.zeros(256, np.uint8)
    for i, v in enumerate(ids):
        lut[v] = i
    so_far, n_objects = set(), []
    for f in frames:
        so_far.update(v for v in f if v != ignore)
        n_objects.append(min(len(so_far) - 1, n_cap))
    n_max = n_objects[-1]
    fresh = {t for t in range(1, N) if n_objects[t] != n_objects[t - 1]}
    seen = [set(int(lut[v]) if lut[v] < K else 0 for v in f) for f in sampled]
    action = np.zeros((N, K), np.uint8)
    existing = set(seen[0])
    for t in range(1, N):
        if t in fresh:
            for k in sorted(seen[t]):
                if k not in existing:
                    existing.add(k)
                    action[t, k] = INJECT
        for k in range(n_max + 1):
            if k not in existing:
                action[t, k] = ABSENT
    return ObjectPlan(K, lut, np.asarray(ids, np.uint8), n_objects, fresh, seen, action, dev)


def appearance_plan(presence, n_max_objects, ignore_idx=255, sampled=None):
    """The clip's plan from its per-frame presence words ([N,8], ``label_presence``); ``n_max_objects`` is the configuration's cap
    (K = n_max_objects + 1 planes).  Everything is derived on the host from one download:

    lut          ReorganizeObjectID's table (``clip_io.reorganize_lut``): the ids present anywhere in the clip without
                 ``ignore_idx``, ascending, map to 0, 1, 2, ...; every other id maps to 0.  ``ids`` is its inverse.
    n_objects[t] min(|ids seen in frames 0 .. t without ignore_idx| - 1, n_max_objects); n_max = n_objects[N - 1].
    fresh        frames t >= 1 whose count differs from frame t - 1's.  It follows the CLAMPED count, as the reference does: an id
                 that arrives once the count has reached n_max_objects changes nothing and its object stays absent.
    seen[t]      {lut[v] if lut[v] < K else 0 : v in frame t}: torch.unique(torch.argmax(one-hot masks of frame t, dim=0)); a
                 remapped id >= K has no plane and an ignored pixel falls on plane 0.
    action[t][k] with ``existing`` = seen[0], growing: at a fresh t every k of seen[t] outside ``existing`` is injected (2) and
                 joins it; then every k <= n_max outside ``existing`` is absent (1); everything else, and every k > n_max, is
                 kept (0).  Frame 0 has no action.  Background can be missing and can be injected.

    ``sampled``: the presence words [N,8] of the label maps as the network's masks hold them -- nearest-resized to a scale, one row
    of ``label_presence_scaled``.  ``seen`` (and with it ``existing`` and the actions) is then taken from them and everything else
    still from ``presence``: the reference counts at full size and looks at the resized masks (utils/helpers.py:44-78).  An
    object that the resize loses at a fresh frame is not injected there and stays absent until a later fresh frame shows it."""
    dev = presence.device if isinstance(presence, torch.Tensor) else torch.device('cpu')
    frames = presence_sets(presence)
    return _plan_from_sets(frames, frames if sampled is None else presence_sets(sampled), n_max_objects, ignore_idx, dev)


def appearance_plans(presence, sampled, n_max_objects, ignore_idx=255):
    """One plan per scale: ``presence`` [N,8] at full size, ``sampled`` [S,N,8] (``label_presence_scaled``) -> list of S plans,
    plan s = ``appearance_plan(presence, n_max_objects, ignore_idx, sampled[s])``, from ONE download of both tensors."""
    if not isinstance(presence, torch.Tensor):
        presence, sampled = torch.as_tensor(np.asarray(presence).view(np.int32)), torch.as_tensor(np.asarray(sampled).view(np.int32))
    if presence.dim() != 2 or sampled.dim() != 3 or tuple(sampled.shape[1:]) != tuple(presence.shape):
        raise RuntimeError('expected presence [N, 8] and sampled [S, N, 8]')
    dev = presence.device
    words = torch.cat([presence.unsqueeze(0), sampled.to(dev)]).cpu().numpy()            # (the one host synchronisation)
    frames = presence_sets(words[0])
    return [_plan_from_sets(frames, presence_sets(w), n_max_objects, ignore_idx, dev) for w in words[1:]]


def _edit_softmax_torch(logit, labels, lut, action, prob):
    f32 = lambda v: torch.full((), v, dtype=torch.float32, device=logit.device)
    act = action.detach().cpu().numpy()
    B, K = act.shape
    for b in range(B):
        for k in range(K):
            if act[b, k] == ABSENT:
                logit[b, k] = f32(ABSENT_LOGIT)
            elif act[b, k] == INJECT:
                if labels is None:
                    m = torch.zeros(logit.shape[2:], dtype=torch.float32, device=logit.device)
                else:
                    m = (lut[b].to(logit.device)[labels[b].to(logit.device).to(torch.int64)] == k).to(torch.float32)
                logit[b, k] = m * f32(NEW_OBJECT_SCALE) - f32(-ABSENT_LOGIT)          # two fp32 operations, two roundings
    prob.copy_(F.softmax(logit, dim=1))
    return prob


def _sample_labels(labels, H, W, sampling):
    """labels [B,Hs,Ws] -> [B,H,W]: the nearest-resized and, per slot, mirrored maps that ``sampling`` describes, materialised."""
    scale_h, scale_w, flips = sampling
    iy = torch.from_numpy(tta.nearest_index_for_scale(H, labels.shape[1], scale_h)).to(labels.device)
    ix = torch.from_numpy(tta.nearest_index_for_scale(W, labels.shape[2], scale_w)).to(labels.device)
    out = labels.index_select(1, iy).index_select(2, ix)
    return torch.stack([torch.flip(m, dims=[1]) if f else m for m, f in zip(out, flips)])


def object_edit_softmax(logit, labels, lut, action, prob, sampling=None):
    """``ops.object_edit_softmax`` for float32 GPU tensors, a torch restatement otherwise (it downloads ``action``): ``logit``
    [B,K,H,W] edited in place per ``action`` [B,K] with ``labels`` [B,H,W] (or None) and ``lut`` [B,256], its soft-max over K
    written to ``prob``.  The edited logits are the same bits on both routes; the restatement's soft-max is torch's.

    ``sampling = (scale_h, scale_w, flips)``: ``labels`` are full-size maps [B,Hs,Ws] and pixel (y, x) of slot b reads
    labels[b][src(y)][src(W - 1 - x if flips[b] else x)] by ``tta.nearest_index_for_scale``; the restatement samples, mirrors and
    then does what it does without."""
    if logit.dim() != 4 or prob.shape != logit.shape or not 1 <= logit.shape[1] <= 255:
        raise RuntimeError('logit and prob must be [B, K, H, W] with 1 <= K <= 255')
    if tuple(action.shape) != tuple(logit.shape[:2]) or tuple(lut.shape) != (logit.shape[0], 256):
        raise RuntimeError('expected action [B, K] and lut [B, 256]')
    if sampling is not None:
        sampling = (float(sampling[0]), float(sampling[1]), [bool(f) for f in sampling[2]])
        if len(sampling[2]) != logit.shape[0] or (labels is not None and (labels.dim() != 3 or labels.shape[0] != logit.shape[0])):
            raise RuntimeError('sampling needs one flip flag per batch slot and labels [B, Hs, Ws]')
    if logit.is_cuda and logit.dtype == torch.float32 and prob.dtype == torch.float32:
        return ops.object_edit_softmax(logit, labels, lut.contiguous(), action.contiguous(), prob, sampling)
    if sampling is not None and labels is not None:
        labels = _sample_labels(labels, logit.shape[2], logit.shape[3], sampling)
    return _edit_softmax_torch(logit, labels, lut, action, prob)
