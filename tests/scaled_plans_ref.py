# -*- coding: utf-8 -*-
"""numpy restatement of what the reference does with objects that are first annotated in the middle of a clip when the clip runs at
another scale, possibly mirrored (multi_scale_inference, utils/helpers.py:44-78, in front of models/rmnet.py:398-450).  No torch, no
GPU: tests/test_scaled_plans.py imports this on any machine, next to tests/late_objects_ref.py whose pieces it reuses.

Literal, in the reference's order:

  loader counts      utils/data_loaders.py:58-65 on the FULL-SIZE label maps (late_objects_ref.loader_counts): multi_scale_inference
                     hands the same n_objects to every pass
  one-hot masks      ReorganizeObjectID + ToOneHot of every full-size frame (late_objects_ref.reorganize / to_onehot)
  nearest resize     F.interpolate(masks.float(), scale_factor=fs, mode='nearest') of every PLANE: output size floor(in * fs) per
                     axis, source index min(int(floorf(float(d) * scale)), in - 1) with scale = float32(1.0 / fs) -- torch's legacy
                     nearest rule as a plain formula (``nearest_index``; tests/test_scaled_plans.py compares it with torch's CPU kernel)
  the mirrored pass  torch.flip(masks, dims=[4]) of the RESIZED planes
  the loop           models/rmnet.py:398-450 on those masks and the full-size counts, as late_objects_ref.reference_clip has it

``resize=(out_h, out_w, scale_h, scale_w)`` replaces the factor by an explicit size and scales, as the C entries take them.  With a
factor the clamp to in - 1 cannot be reached at any size a test can hold: d <= in * fs - 1 gives d / fs <= in - 1 / fs, and the
rounding of the scale and of the product adds at most in * 2^-23, so an index of ``in`` needs in > 2^23 / fs.  The planted fault that
drops the clamp is therefore caught by a case with an explicit size.

Mutants (``mutant=``), each caught by a named clip of the test:
  counts_from_sampled   the loader's counts taken from the resized label maps
  seen_from_full        torch.unique(torch.argmax(masks[t])) taken from the full-size masks at every frame
  existing_from_full    existing_objects seeded from the full-size frame 0, later frames from the resized masks
  round_to_nearest      the source index rounded to the nearest integer instead of floored
  scale_float64         the scale and the product kept in float64
  clamp_missing         no min(., in - 1): the index runs on (wrapped here, so that the restatement stays inside its array)
  mirror_plan           the mirrored pass planned on resize(flip(masks)) instead of flip(resize(masks))
"""

import math

import numpy as np

import late_objects_ref as base

F32 = np.float32
MUTANTS = ('counts_from_sampled', 'seen_from_full', 'existing_from_full', 'round_to_nearest', 'scale_float64', 'clamp_missing',
           'mirror_plan')


def scaled_size(h, w, fs):
    return int(math.floor(float(h) * float(fs))), int(math.floor(float(w) * float(fs)))


def nearest_index(out, inp, scale, mutant=None):
    """int64 [out]: the source index of every output index.  ``scale`` is the source step per output pixel."""
    if mutant == 'scale_float64':
        idx = np.floor(np.arange(out, dtype=np.float64) * float(scale))
    elif mutant == 'round_to_nearest':
        idx = np.rint(np.arange(out, dtype=F32) * F32(scale))
    else:
        idx = np.floor(np.arange(out, dtype=F32) * F32(scale))
    idx = idx.astype(np.int64)
    return idx % inp if mutant == 'clamp_missing' else np.minimum(idx, inp - 1)


def _resize_args(H, W, fs, resize, mutant):
    if resize is not None:
        return resize
    h, w = scaled_size(H, W, fs)
    scale = 1.0 / float(fs) if mutant == 'scale_float64' else F32(1.0 / float(fs))
    return h, w, scale, scale


def nearest_resize(planes, fs, resize=None, mutant=None):
    """[..., H, W] -> [..., h, w]: every plane resized by nearest neighbour."""
    H, W = planes.shape[-2:]
    h, w, scale_h, scale_w = _resize_args(H, W, fs, resize, mutant)
    iy, ix = nearest_index(h, H, scale_h, mutant), nearest_index(w, W, scale_w, mutant)
    return planes[..., iy, :][..., ix]


def sampled_maps(label_maps, fs, mirrored=False, resize=None):
    """The label maps as a materialised resize (and mirror) of the raw maps: what the device entries must behave as if they read."""
    out = nearest_resize(np.stack([np.asarray(m, np.uint8) for m in label_maps]), fs, resize)
    return np.ascontiguousarray(out[..., ::-1] if mirrored else out)


def reference_clip_scaled(label_maps, n_max_objects, fs, mirrored=False, ignore_idx=255, logits=None, resize=None, mutant=None):
    """The protocol on full-size uint8 label maps [N,H,W] for the pass at factor ``fs`` (mirrored or not).  Returns the fields of
    late_objects_ref.reference_clip; ``masks`` are the resized (mirrored) one-hot masks the network is handed, ``logits`` float32
    [N,K,h,w] (frame 0 unused) the edited copy."""
    label_maps = [np.asarray(m, np.uint8) for m in label_maps]
    N = len(label_maps)
    K = n_max_objects + 1
    maps, ids = base.reorganize(label_maps, ignore_idx)
    lut = np.zeros(256, np.uint8)
    for idx, mi in enumerate(ids):
        lut[int(mi)] = idx
    full = np.stack([base.to_onehot(m, K) for m in maps])                     # [N,K,H,W]
    if mirrored and mutant == 'mirror_plan':
        masks = nearest_resize(full[..., ::-1], fs, resize, mutant)
    else:
        masks = nearest_resize(full, fs, resize, mutant)
        if mirrored:
            masks = masks[..., ::-1]                                          # torch.flip(_masks, dims=[4])
    if mutant == 'counts_from_sampled':
        n_objects = base.loader_counts(list(nearest_resize(np.stack(label_maps), fs, resize)), n_max_objects, ignore_idx)
    else:
        n_objects = base.loader_counts(label_maps, n_max_objects, ignore_idx)

    n_max = max(n_objects)
    seen_in = full if mutant == 'seen_from_full' else masks
    arg_set = lambda t: [int(j) for j in np.unique(np.argmax(seen_in[t], axis=0))]
    existing_objects = [int(j) for j in np.unique(np.argmax(full[0], axis=0))] if mutant == 'existing_from_full' else arg_set(0)
    contains_new_objects = [j for j in range(1, N) if n_objects[j] != n_objects[j - 1]]

    action = np.zeros((N, K), np.uint8)
    out = None if logits is None else np.array(logits, F32)
    for t in range(1, N):
        if t in contains_new_objects:
            for j in arg_set(t):
                if j not in existing_objects:
                    existing_objects.append(j)
                    action[t, j] = 2
                    if out is not None:
                        out[t, j] = masks[t, j].astype(F32) * base.NEW_OBJECT_SCALE - base.NEW_OBJECT_SHIFT
        for j in range(n_max + 1):
            if j not in existing_objects:
                action[t, j] = 1
                if out is not None:
                    out[t, j] = base.ABSENT_LOGIT
    res = dict(ids=ids, lut=lut, n_objects=n_objects, n_max=n_max, fresh=set(contains_new_objects),
               seen=[set(arg_set(t)) for t in range(N)], action=action, edited={t for t in range(N) if action[t].any()},
               masks=np.ascontiguousarray(masks), K=K)
    if out is not None:
        res['logits'] = out
    return res
