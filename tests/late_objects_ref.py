# -*- coding: utf-8 -*-
"""numpy restatement of the reference's handling of objects that are first annotated in the middle of a clip (the YouTube-VOS
protocol), of the presence words of rmnet_amd/csrc/late_objects.hip, and the error bound of the edit kernel's soft-max.  No torch,
no GPU: tests/test_late_objects.py imports this on any machine.

The restatement is literal -- label maps in, one-hot masks, np.unique(np.argmax(...)), Python loops -- in the reference's order:

  loader_counts      utils/data_loaders.py:58-65: a set of ids that grows frame by frame, without the ignore id;
                     n_objects[t] = min(len(set) - 1, n_max_objects)
  reorganize         ReorganizeObjectID, utils/data_transforms.py:53-68: np.unique over the WHOLE clip without the ignore id, every
                     map renumbered through it into np.zeros (so the ignore id and nothing else falls on 0 besides the lowest id)
  to_onehot          utils/helpers.py:81-90: plane k = (mask == k) for k < K; a renumbered id >= K sets no plane
  reference_clip     models/rmnet.py:398-407 and 436-448 on those masks: existing_objects from frame 0's argmax,
                     contains_new_objects from the counts, and per frame the injection of every plane in the argmax set that is
                     not in existing_objects (at a frame whose count changed), then -16.1181 for every plane <= n_max_objects that
                     is not.  With ``logits`` it performs the writes in fp32 exactly as torch does (masks.float() * 32.0605 - 16.1181
                     is two fp32 operations) and records, besides, WHICH write reached every plane: action 0 none, 1 absent,
                     2 inject -- the table rmnet_amd.object_plan.appearance_plan must reproduce.

Mutants (``mutant=``), each one a plausible slip of a restatement that a named case of the test catches:
  count_per_frame       the count from frame t's ids alone instead of cumulatively
  table_per_frame       the renumbering table from every frame's own ids instead of the clip's
  clamp_dropped         n_objects without min(., n_max_objects)
  fresh_from_ids        contains_new_objects from the growth of the id set instead of from the clamped count
  ids_ge_K_to_last      a renumbered id >= K put on plane K - 1 instead of on none
  inject_from_argmax    the injected mask taken as (argmax == j) instead of the one-hot plane j (= lut[label] == j): they differ
                        where a pixel has no plane, which the argmax sends to plane 0
  existing_reset        existing_objects started again from frame 0's set at every frame
  absent_before_inject  the table of ONE action per plane filled with the absent marks first and the injection skipped where a mark
                        already stands.  (As literal logit writes the order would not matter, the later write wins; in a table it does.)

The soft-max bound
------------------
The kernel evaluates, per pixel, with l_k the fp32 logits after the edit:  mx = max_k l_k (exact: a maximum rounds nothing);
d_k = fl(l_k - mx);  e_k = expf(d_k);  s = e_0, s = fl(s + e_k) for k ascending;  p_k = fl(e_k / s).  u = 2^-24 is one fp32
rounding (relative), E the largest error of the device's expf in ulps on [-34, 0] (glue_ref.E_ULP: twice the measured 0.834, see
profiles/r14_a_glue_tests.md), one ulp being at most 2 u relative.  D = max_k |l_k - mx| of the pixel.
  1. d_k = (l_k - mx)(1 + a), |a| <= u: an absolute error of at most D u in the exponent, i.e. a relative error of at most D u in
     exp(d_k) to first order.  (For the maximum itself d_k = 0 exactly.)
  2. e_k = exp(d_k)(1 + b), |b| <= 2 E u.  So e_k = exp(l_k - mx)(1 + t_k) with |t_k| <= (D + 2 E) u =: T.
  3. s: K positive terms, K - 1 roundings, each term's relative error at most T, so s = S (1 + c) with |c| <= T + (K - 1) u
     whatever the order of the additions.
  4. p_k = (e_k / s)(1 + g), |g| <= u.
  Together  |p^_k - p_k| / p_k <= T + T + (K - 1) u + u = (4 E + 2 D + K) u  to first order, the count the issue gives.  The
  neglected products of two terms are below (4 E + 2 D + K) u ~ 330 u = 2e-5 of the bound at D = 34, K = 255; every bound is
  multiplied by the same 1 + 1e-3 that glue_ref uses for them.  The reference p_k is the float64 soft-max of the SAME fp32 logits,
  whose own error (~K 2^-53) is nothing at this scale.  E is only known on [-34, 0]: every case must keep D <= 34 (exp(-34) =
  1.7e-15 is a normal fp32 number, so nothing underflows either), which the test asserts.
  All channels absent: every l_k is the same number, d_k = 0, expf(0) = 1 exactly (the test checks it), s = K exactly (an integer
  below 2^24) and p_k = fl(1 / K): the correctly rounded quotient, bit for bit.
"""

import numpy as np

from glue_ref import E_ULP, SLACK, U

F32 = np.float32
ABSENT_LOGIT = F32(-16.1181)            # models/rmnet.py:448
NEW_OBJECT_SCALE = F32(32.0605)         # models/rmnet.py:442
NEW_OBJECT_SHIFT = F32(16.1181)
D_MAX = 34.0
MUTANTS = ('count_per_frame', 'table_per_frame', 'clamp_dropped', 'fresh_from_ids', 'ids_ge_K_to_last', 'inject_from_argmax',
           'existing_reset', 'absent_before_inject')


# ================================================================================================ presence words
def presence_words(label_maps):
    """uint32 [N,8]: bit v & 31 of word v >> 5 of row n set exactly when byte value v occurs in frame n."""
    out = np.zeros((len(label_maps), 8), np.uint32)
    for n, m in enumerate(label_maps):
        for v in np.unique(np.asarray(m)):
            out[n, int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    return out


# ================================================================================================ the reference, restated
def loader_counts(label_maps, n_max_objects, ignore_idx=255, mutant=None):
    mask_indexes = set()
    n_objects = []
    for m in label_maps:
        _mask_indexes = np.unique(m)
        _mask_indexes = _mask_indexes[_mask_indexes != ignore_idx]
        if mutant == 'count_per_frame':
            mask_indexes = set()
        mask_indexes.update(int(i) for i in _mask_indexes)
        _n_objects = len(mask_indexes) - 1 if mutant == 'clamp_dropped' else min(len(mask_indexes) - 1, n_max_objects)
        n_objects.append(_n_objects)
    return n_objects


def reorganize(label_maps, ignore_idx=255, mutant=None):
    """(renumbered maps, the clip's ids ascending)."""
    masks = [np.array(m) for m in label_maps]
    mask_indexes = np.unique(np.array(masks))
    mask_indexes = mask_indexes[mask_indexes != ignore_idx]
    out = []
    for m in masks:
        indexes = mask_indexes
        if mutant == 'table_per_frame':
            indexes = np.unique(m)
            indexes = indexes[indexes != ignore_idx]
        _m = np.zeros(m.shape)
        for idx, mi in enumerate(indexes):
            _m[m == mi] = idx
        out.append(_m.astype(np.uint8))
    return out, mask_indexes.astype(np.uint8)


def to_onehot(mask, k, mutant=None):
    h, w = mask.shape
    one_hot_masks = np.zeros((k, h, w), dtype=np.uint8)
    for k_idx in range(k):
        one_hot_masks[k_idx] = (mask == k_idx)
    if mutant == 'ids_ge_K_to_last':
        one_hot_masks[k - 1] |= (mask >= k).astype(np.uint8)
    return one_hot_masks


def onehot_clip(label_maps, n_max_objects, ignore_idx=255, mutant=None):
    """uint8 [N,K,H,W]: ReorganizeObjectID + ToOneHot of every frame."""
    maps, _ = reorganize(label_maps, ignore_idx, mutant)
    return np.stack([to_onehot(m, n_max_objects + 1, mutant) for m in maps])


def reference_clip(label_maps, n_max_objects, ignore_idx=255, logits=None, mutant=None):
    """The whole protocol on uint8 label maps [N,H,W].  Returns a dict: ids, lut (uint8 [256], the clip's table), n_objects,
    n_max, fresh (set), seen (list of sets: the argmax set of every frame), action (uint8 [N,K]), edited (set), masks
    (uint8 [N,K,H,W]) and, with ``logits`` float32 [N,K,H,W] (frame 0 unused), 'logits': the edited copy."""
    label_maps = [np.asarray(m, np.uint8) for m in label_maps]
    N = len(label_maps)
    K = n_max_objects + 1
    n_objects = loader_counts(label_maps, n_max_objects, ignore_idx, mutant)
    maps, ids = reorganize(label_maps, ignore_idx, mutant)
    lut = np.zeros(256, np.uint8)
    for idx, mi in enumerate(ids):
        lut[int(mi)] = idx
    masks = np.stack([to_onehot(m, K, mutant) for m in maps])

    n_max = max(n_objects)                                                   # torch.max(no).item()
    arg_set = lambda t: [int(j) for j in np.unique(np.argmax(masks[t], axis=0))]
    existing_objects = arg_set(0)
    if mutant == 'fresh_from_ids':
        sets, grown = set(), []
        for m in label_maps:
            before = len(sets)
            sets.update(int(v) for v in np.unique(m) if v != ignore_idx)
            grown.append(len(sets) != before)
        contains_new_objects = [j for j in range(1, N) if grown[j]]
    else:
        contains_new_objects = [j for j in range(1, N) if n_objects[j] != n_objects[j - 1]]

    action = np.zeros((N, K), np.uint8)
    out = None if logits is None else np.array(logits, F32)
    for t in range(1, N):
        if mutant == 'existing_reset':
            existing_objects = arg_set(0)
        if mutant == 'absent_before_inject':
            for j in range(n_max + 1):
                if j not in existing_objects and j < K:
                    action[t, j] = 1
        if t in contains_new_objects:
            for j in arg_set(t):
                if j not in existing_objects:
                    existing_objects.append(j)
                    if mutant == 'absent_before_inject' and action[t, j]:
                        continue
                    action[t, j] = 2
                    if out is not None:
                        m = (np.argmax(masks[t], axis=0) == j) if mutant == 'inject_from_argmax' else masks[t, j]
                        out[t, j] = m.astype(F32) * NEW_OBJECT_SCALE - NEW_OBJECT_SHIFT
        for j in range(n_max + 1):
            if j not in existing_objects and j < K:           # (j < K: only the clamp_dropped mutant can pass it)
                action[t, j] = 1
                if out is not None:
                    out[t, j] = ABSENT_LOGIT
    res = dict(ids=ids, lut=lut, n_objects=n_objects, n_max=n_max, fresh=set(contains_new_objects),
               seen=[set(arg_set(t)) for t in range(N)], action=action,
               edited={t for t in range(N) if action[t].any()}, masks=masks, K=K)
    if out is not None:
        res['logits'] = out
    return res


# ================================================================================================ one frame of the edit kernel
def edit_frame(logit, labels, lut, action):
    """float32 [K,H,W] logits edited as rmnet_object_edit_softmax_f32 does it (a copy): fp32, one rounding per operation."""
    out = np.array(logit, F32)
    K = out.shape[0]
    for k in range(K):
        if action[k] == 1:
            out[k] = ABSENT_LOGIT
        elif action[k] == 2:
            m = np.zeros(out.shape[1:], F32) if labels is None else (np.asarray(lut)[np.asarray(labels)] == k).astype(F32)
            out[k] = m * NEW_OBJECT_SCALE - NEW_OBJECT_SHIFT
    return out


def softmax_f64(logit):
    """float64 soft-max over axis 0 of fp32 logits [K, ...]."""
    l = np.asarray(logit, np.float64)
    e = np.exp(l - l.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def spread(logit):
    """D of every pixel: max_k |l_k - max_k l_k|."""
    l = np.asarray(logit, np.float64)
    return (l.max(axis=0) - l.min(axis=0))


def softmax_bound(logit, E=None):
    """(p64 [K,...], bound [K,...]) per the module docstring: p (4 E + 2 D + K) u (1 + 1e-3)."""
    E = E_ULP if E is None else E
    p = softmax_f64(logit)
    K = p.shape[0]
    return p, SLACK * p * (4.0 * E + 2.0 * spread(logit)[None] + K) * U
