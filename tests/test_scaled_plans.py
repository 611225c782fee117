# -*- coding: utf-8 -*-
"""Objects that appear mid-clip under multi-scale and flipped inference: tta.nearest_index, object_plan.label_presence_scaled /
appearance_plan(sampled=) / appearance_plans / object_edit_softmax(sampling=), the two kernels of include/rmnet_hip.h I2,
RMNet.forward(object_plan=(labels, plans, sampling)) and the drivers, against the literal numpy restatement of the reference in
tests/scaled_plans_ref.py.

Without a GPU: the index rule against torch's CPU kernel off the sizes where that kernel copies, the restatement pinned by
hand-written clips whose answers stand in this file, every planted fault caught by a named clip, the plans equal to the restatement
in every field, the torch routes, and the argument rules.  On the GPU: every word of the presence kernel and every logit and
probability bit of the edit kernel against the existing entries on materialised maps, and whole clips against
helpers.multi_scale_inference fed the one-hot masks of all frames."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_io_ref
import late_objects_ref as base
import scaled_plans_ref as ref

gpu = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4                                          # RMNET_E_INVALID_ARG, RMNET_E_UNSUPPORTED
FACTORS = (0.3, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0)
TWELVE = (0.3, 0.5, 0.6, 0.75, 0.9, 1.0, 1.01, 1.1, 1.25, 1.5, 1.7, 2.0)
ID_POOL = (0, 3, 5, 9, 31, 32, 63, 64, 200, 254, 255)


def dev():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    return torch.device('cuda', 0)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _clip(shape, *frames):
    """Label maps from per-frame lists of (value, rows, columns); rows / columns are ints or slices.  Unset pixels are 0."""
    out = []
    for spec in frames:
        m = np.zeros(shape, np.uint8)
        for v, r, c in spec:
            m[r, c] = v
        out.append(m)
    return out


S = slice
BLOCK5 = (5, S(0, 4), S(0, 4))
# the clip of the issue: 5 frames of 8 x 8; id 5 everywhere, id 38 as one pixel at (1, 5) in frame 2 and on [2:4, 4:6] afterwards, id 77 at
# (6, 6) in frame 4, one pixel of 255 in frame 1.  At 0.5 only even rows and columns are read.
HAND = _clip((8, 8), [BLOCK5], [BLOCK5, (255, 7, 7)], [BLOCK5, (38, 1, 5)], [BLOCK5, (38, S(2, 4), S(4, 6))],
             [BLOCK5, (38, S(2, 4), S(4, 6)), (77, 6, 6)])
EVEN = (S(0, 4, 2), S(0, 4, 2))
# name -> (label maps, cap, factor, the answers).  The plan of the mirrored pass must be the same one.
CASES = {
    'hand_1.0_cap3': (HAND, 3, 1.0, dict(n_objects=[1, 1, 2, 2, 3], action=[[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 2, 1], [0, 0, 0, 1], [0, 0, 0, 2]])),
    # the single pixel of frame 2 is lost: fresh but nothing injected; frame 3 shows the object but is not fresh; injected with 77 at frame 4
    'hand_0.5_cap3': (HAND, 3, 0.5, dict(n_objects=[1, 1, 2, 2, 3], action=[[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 2, 2]])),
    'hand_1.0_cap2': (HAND, 2, 1.0, dict(n_objects=[1, 1, 2, 2, 2], action=[[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 0], [0, 0, 0]])),
    # lost at the only fresh frame and never injected, because no later fresh frame comes
    'hand_0.5_cap2_never_injected': (HAND, 2, 0.5, dict(n_objects=[1, 1, 2, 2, 2], action=[[0, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]])),
    'hand_1.0_cap10': (HAND, 10, 1.0, dict(n_objects=[1, 1, 2, 2, 3], action=[r + [0] * 7 for r in
                                                                            [[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 2, 1], [0, 0, 0, 1], [0, 0, 0, 2]]])),
    'hand_0.5_cap10': (HAND, 10, 0.5, dict(n_objects=[1, 1, 2, 2, 3], action=[r + [0] * 7 for r in
                                                                            [[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 2, 2]]])),
    # 6 rows at 1.25 are read as 0, 0, 1, 2, 3, 4, 4: row 5 never, so an upscale loses the object too
    'lost_in_the_last_row_at_1.25': (_clip((6, 6), [(5, S(0, 2), S(0, 2))], [(5, S(0, 2), S(0, 2)), (9, 5, S(0, 3))]), 2, 1.25,
                                     dict(n_objects=[1, 2], action=[[0, 0, 0], [0, 0, 1]])),
    'seen_in_the_last_row_at_1.0': (_clip((6, 6), [(5, S(0, 2), S(0, 2))], [(5, S(0, 2), S(0, 2)), (9, 5, S(0, 3))]), 2, 1.0,
                                    dict(n_objects=[1, 2], action=[[0, 0, 0], [0, 0, 2]])),
    # lost in a column only: column 1 is not read at 0.5, but its mirror image, column 2, would be
    'lost_in_a_column_at_0.5': (_clip((4, 4), [(5, 0, 0)], [(5, 0, 0), (9, 0, 1)]), 2, 0.5, dict(n_objects=[1, 2], action=[[0, 0, 0], [0, 0, 1]])),
    'cap_swallows_an_id': (_clip((4, 4), [(5, 0, 0)], [(5, 0, 0), (9, 2, 2)]), 1, 0.5, dict(n_objects=[1, 1], action=[[0, 0], [0, 0]])),
    # frame 0 without background: a sampled 255 falls on plane 0 and makes the background exist; one that is not sampled does not
    'ignored_label_sampled': (_clip((4, 4), [(5, S(0, 4), S(0, 4)), (255, 2, 2)], [(5, S(0, 4), S(0, 4)), (255, 2, 2)],
                                    [(5, S(0, 4), S(0, 4)), (255, 2, 2), (0, 0, 0)]), 1, 0.5, dict(n_objects=[0, 0, 1], action=[[0, 0], [0, 0], [0, 0]])),
    'ignored_label_not_sampled': (_clip((4, 4), [(5, S(0, 4), S(0, 4)), (255, 1, 1)], [(5, S(0, 4), S(0, 4)), (255, 1, 1)],
                                        [(5, S(0, 4), S(0, 4)), (255, 1, 1), (0, 0, 0)]), 1, 0.5, dict(n_objects=[0, 0, 1], action=[[0, 0], [1, 0], [2, 0]])),
    # the full-size frame 0 has background, the sampled one has none: plane 0 is injected with the new object
    'background_missing_from_the_sampled_frame_0': (_clip((4, 4), [(5,) + EVEN], [(5, 0, 0), (9, 2, 2)]), 2, 0.5,
                                                    dict(n_objects=[1, 2], action=[[0, 0, 0], [2, 0, 2]])),
    'leaves_and_returns': (_clip((4, 4), [(5, 0, 0)], [(5, 0, 0), (9, 2, 2)], [(5, 0, 0)], [(5, 0, 0), (9, 2, 2), (31, 0, 2)]), 3, 0.5,
                           dict(n_objects=[1, 2, 2, 3], action=[[0, 0, 0, 0], [0, 0, 2, 1], [0, 0, 0, 1], [0, 0, 0, 2]])),
    # 31 columns at 1.3: output column 39 reads source column 30 in float32 (39 * 0.76923078f rounds to 30), 29 in float64
    'last_column_at_1.3': (_clip((1, 31), [(5, 0, 0)], [(5, 0, 0), (9, 0, 30)]), 2, 1.3, dict(n_objects=[1, 2], action=[[0, 0, 0], [0, 0, 2]])),
}
# planted fault -> (the clip that catches it, mirrored pass, explicit (out_h, out_w, scale_h, scale_w) or None)
CAUGHT_BY = {
    'counts_from_sampled': ('hand_0.5_cap3', False, None),
    'seen_from_full': ('hand_0.5_cap3', False, None),
    'existing_from_full': ('background_missing_from_the_sampled_frame_0', False, None),
    'round_to_nearest': ('lost_in_the_last_row_at_1.25', False, None),
    'scale_float64': ('last_column_at_1.3', False, None),
    'clamp_missing': ('seen_in_the_last_row_at_1.0', False, (7, 6, 1.0, 1.0)),       # one output row more than the scale covers
    'mirror_plan': ('lost_in_a_column_at_0.5', True, None),
}


def _fields(r):
    return dict(ids=[int(i) for i in r['ids']], lut=r['lut'].tolist(), n_objects=list(r['n_objects']), n_max=r['n_max'], fresh=set(r['fresh']),
                seen=[set(s) for s in r['seen']], action=r['action'].tolist(), edited=set(r['edited']))


def _plan_fields(p):
    return dict(ids=[int(i) for i in p.ids], lut=p.lut_host.tolist(), n_objects=list(p.n_objects), n_max=p.n_max, fresh=set(p.fresh),
                seen=[set(s) for s in p.seen], action=p.action_host.tolist(), edited=set(p.edited))


def _logits_for(n, K, h, w, seed=0):
    return (np.random.RandomState(seed).rand(n, K, h, w) * 31.9 - 16.0).astype(np.float32)


# ================================================================================================ CPU: the index rule
def test_nearest_index_literals():
    from rmnet_amd import tta
    assert tta.nearest_index(4, 8, 0.5).tolist() == [0, 2, 4, 6]
    assert tta.nearest_index(6, 8, 0.75).tolist() == [0, 1, 2, 4, 5, 6]
    assert tta.nearest_index(7, 6, 1.25).tolist() == [0, 0, 1, 2, 3, 4, 4]           # row 5 is never read
    assert tta.nearest_index(8, 4, 2.0).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert tta.nearest_index(5, 5, 1.0).tolist() == [0, 1, 2, 3, 4]
    assert tta.nearest_index_for_scale(7, 6, 1.0).tolist() == [0, 1, 2, 3, 4, 5, 5]  # the clamp
    assert tta.nearest_index(40, 31, 1.3)[39] == 30 and int(math.floor(39 * (1.0 / 1.3))) == 29
    for fs in TWELVE:
        for n in (1, 6, 31, 70):
            out = tta.scaled_size(n, n, fs)[0]
            assert np.array_equal(tta.nearest_index(out, n, fs), ref.nearest_index(out, n, np.float32(1.0 / fs)))
            assert tta.nearest_index(out, n, fs).dtype == np.int64


def _special(inp, fs):
    """torch's CPU kernels copy an axis whose output size equals its input size or its double while fs is neither 1 nor 2."""
    return fs not in (1.0, 2.0) and int(math.floor(inp * fs)) in (inp, 2 * inp)


def test_nearest_index_equals_torchs_cpu_kernel_off_the_sizes_where_it_copies():
    from rmnet_amd import tta
    widths = (1, 2, 3, 5, 17, 33, 64, 70)
    ran = skipped = 0
    for fs in TWELVE:
        for H in range(1, 71):
            for W in widths:
                h, w = tta.scaled_size(H, W, fs)
                if h < 1 or w < 1:
                    continue
                if _special(H, fs) or _special(W, fs):
                    skipped += 1
                    continue
                x = (torch.arange(H * W, dtype=torch.float32) % 251.0).view(1, 1, H, W)
                want = F.interpolate(x, scale_factor=fs, mode='nearest')[0, 0].numpy()
                got = x[0, 0].numpy()[tta.nearest_index(h, H, fs)][:, tta.nearest_index(w, W, fs)]
                assert np.array_equal(got, want), (fs, H, W)
                ran += 1
    print('cases compared %d, skipped at special sizes %d' % (ran, skipped))
    # the special sizes are a condition, not a tolerance: an axis of n elements is special at fs when floor(n * fs) is n or 2 n.  Among
    # these factors and n <= 70 that is every n at 1.01, n <= 9 at 1.1, n <= 3 at 1.25, n = 1 at 1.5 and 1.7, and none below 1
    special = {fs: [n for n in range(1, 71) if _special(n, fs)] for fs in TWELVE}
    assert special[1.01] == list(range(1, 71)) and special[1.1] == list(range(1, 10)) and special[1.25] == [1, 2, 3]
    assert special[1.5] == special[1.7] == [1] and not any(special[fs] for fs in TWELVE if fs <= 1.0 or fs == 2.0)
    # 1.01: 560; 1.1: 9 * 8 + 61 * 4 = 316; 1.25: 3 * 8 + 67 * 3 = 225; 1.5 and 1.7: 8 + 69 = 77 each
    assert skipped == 560 + 316 + 225 + 77 + 77 == 1255 and ran == 4932


# ================================================================================================ CPU: the restatement, pinned
@pytest.mark.parametrize('name', sorted(CASES))
def test_the_restatement_gives_the_hand_written_answers_mirrored_or_not(name):
    maps, cap, fs, want = CASES[name]
    plain = ref.reference_clip_scaled(maps, cap, fs)
    mirrored = ref.reference_clip_scaled(maps, cap, fs, mirrored=True)
    assert list(plain['n_objects']) == want['n_objects'] and plain['action'].tolist() == want['action'], name
    assert _fields(plain) == _fields(mirrored), name                      # one plan serves both passes
    assert np.array_equal(mirrored['masks'], plain['masks'][..., ::-1])
    assert plain['masks'].shape[-2:] == ref.scaled_size(*maps[0].shape, fs)
    # resizing one-hot planes and taking the argmax == the clip's table applied to the sampled label (no plane -> 0)
    sampled = ref.sampled_maps(maps, fs)
    remapped = plain['lut'][sampled]
    assert np.array_equal(np.argmax(plain['masks'], axis=1), np.where(remapped < cap + 1, remapped, 0))
    if fs == 1.0:                                                         # at factor 1 it is the protocol of tests/late_objects_ref.py
        assert _fields(plain) == _fields(base.reference_clip(maps, cap))


def test_the_counts_are_the_full_size_ones_at_every_factor():
    for fs in (0.5, 0.75, 1.0, 1.25):
        for cap in (2, 3, 10):
            r = ref.reference_clip_scaled(HAND, cap, fs)
            assert list(r['n_objects']) == [min(n, cap) for n in (1, 1, 2, 2, 3)] and [int(i) for i in r['ids']] == [0, 5, 38, 77]


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_every_planted_fault_is_caught_by_its_named_clip(mutant):
    name, mirrored, resize = CAUGHT_BY[mutant]
    maps, cap, fs, _ = CASES[name]
    h, w = resize[:2] if resize else ref.scaled_size(*maps[0].shape, fs)
    logits = _logits_for(len(maps), cap + 1, h, w)
    good = ref.reference_clip_scaled(maps, cap, fs, mirrored, logits=logits, resize=resize)
    bad = ref.reference_clip_scaled(maps, cap, fs, mirrored, logits=logits, resize=resize, mutant=mutant)
    assert _fields(good) != _fields(bad) or not _same_bits(good['logits'], bad['logits']), mutant
    assert set(CAUGHT_BY) == set(ref.MUTANTS)


# ================================================================================================ CPU: the plans
def _random_clip(rng):
    N, H, W = int(rng.randint(1, 7)), int(rng.randint(4, 10)), int(rng.randint(4, 10))
    maps = []
    for _ in range(N):
        ids = rng.choice(ID_POOL, size=int(rng.randint(1, 5)), replace=False)
        m = np.full((H, W), ids[0], np.uint8)
        for v in ids[1:]:                                 # small objects: single pixels and short runs, which a scale can lose
            y, x = int(rng.randint(0, H)), int(rng.randint(0, W))
            m[y, x:x + int(rng.randint(1, 3))] = v
        maps.append(m)
    return maps, int(rng.randint(1, 5))


def _sampled_words(maps, fs):
    return base.presence_words(list(ref.sampled_maps(maps, fs)))


def test_the_plans_equal_the_restatement_in_every_field():
    from rmnet_amd import object_plan
    rng = np.random.RandomState(30)
    clips = [(m, c) for m, c, _, _ in CASES.values()] + [_random_clip(rng) for _ in range(300)]
    lost = fresh = 0
    for maps, cap in clips:
        if base.reference_clip(maps, cap)['n_max'] < 0:
            continue
        factors = [fs for fs in FACTORS if min(ref.scaled_size(*maps[0].shape, fs)) >= 1]
        words = torch.from_numpy(base.presence_words(maps).view(np.int32))
        sampled = torch.from_numpy(np.stack([_sampled_words(maps, fs) for fs in factors]).view(np.int32))
        plans = object_plan.appearance_plans(words, sampled, cap)
        assert len(plans) == len(factors)
        for fs, plan, s in zip(factors, plans, sampled):
            want = ref.reference_clip_scaled(maps, cap, fs)
            assert _plan_fields(plan) == _fields(want), fs
            assert _plan_fields(object_plan.appearance_plan(words, cap, sampled=s)) == _fields(want)
            assert plan.K == cap + 1 and tuple(plan.action.shape) == (len(maps), cap + 1) and plan.action.dtype == torch.uint8
            lost += int(want['action'].tolist() != base.reference_clip(maps, cap)['action'].tolist())
            fresh += len(want['fresh'])
        # unchanged: without ``sampled``, and with the full-size presence as ``sampled``, it is the plan of before
        before = _fields(base.reference_clip(maps, cap))
        assert _plan_fields(object_plan.appearance_plan(words, cap)) == before
        assert _plan_fields(object_plan.appearance_plan(words, cap, sampled=words)) == before
        assert _plan_fields(object_plan.appearance_plans(words, words[None], cap)[0]) == before
    print('plans that differ from the full-size one %d, fresh frames %d' % (lost, fresh))
    assert lost > 50 and fresh > 300                      # (the random clips do lose objects at a scale)


# ================================================================================================ CPU: the torch routes
def test_the_torch_route_of_label_presence_scaled_equals_the_presence_of_the_sampled_maps():
    from rmnet_amd import object_plan
    rng = np.random.RandomState(4)
    for shape in ((1, 1, 1), (3, 6, 6), (2, 12, 13), (4, 9, 31)):
        maps = rng.randint(0, 256, size=shape).astype(np.uint8)
        factors = [fs for fs in FACTORS if min(ref.scaled_size(shape[1], shape[2], fs)) >= 1]
        want = np.stack([_sampled_words(maps, fs) for fs in factors])
        for t in (torch.from_numpy(maps), torch.from_numpy(maps).to(torch.int64)):
            got = object_plan.label_presence_scaled(t, shape[1], shape[2], factors)
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(factors), shape[0], 8)
            assert np.array_equal(got.numpy().view(np.uint32), want)
    with pytest.raises(RuntimeError, match=r'\[N, H, W\]'):
        object_plan.label_presence_scaled(torch.zeros(1, 4, 4, dtype=torch.uint8), 4, 5, (1.0,))
    with pytest.raises(RuntimeError, match='leaves no pixel'):
        object_plan.label_presence_scaled(torch.zeros(1, 1, 4, dtype=torch.uint8), 1, 4, (0.5,))
    with pytest.raises(RuntimeError, match='scales'):
        object_plan.label_presence_scaled(torch.zeros(1, 4, 4, dtype=torch.uint8), 4, 4, (1.0,) * 9)


def _edit_inputs(rng, B, K, Hs, Ws, h, w):
    """(logit [B,K,h,w], full-size labels [B,Hs,Ws], lut [B,256], action rows) with more ids than planes."""
    lut = np.zeros((B, 256), np.uint8)
    labels = np.zeros((B, Hs, Ws), np.uint8)
    n_ids = min(K + 3, 255)
    for b in range(B):
        ids = np.sort(rng.choice(np.arange(255), size=n_ids, replace=False))
        lut[b, ids] = np.arange(n_ids)
        labels[b] = ids[rng.randint(0, n_ids, size=(Hs, Ws))]
    logit = (rng.rand(B, K, h, w) * 31.9 - 16.0).astype(np.float32)
    mixed = rng.randint(0, 3, size=(B, K)).astype(np.uint8)
    mixed[0, K - 1] = 2
    inject_all = np.full((B, K), 2, np.uint8)
    return logit, labels, lut, (mixed, inject_all)


@pytest.mark.parametrize('K', [1, 3, 11])
def test_the_torch_route_of_the_sampling_edit_gives_the_bits_of_the_edit_on_the_materialised_map(K):
    from rmnet_amd import object_plan, tta
    rng = np.random.RandomState(300 + K)
    for fs in (0.5, 0.75, 1.25, 2.0):
        Hs, Ws = 6, 9
        h, w = ref.scaled_size(Hs, Ws, fs)
        step = tta.scale_for_factor(fs)
        for flips in ((False, False), (True, False), (False, True)):
            logit, labels, lut, actions = _edit_inputs(rng, 2, K, Hs, Ws, h, w)
            for action in actions:
                materialised = np.stack([ref.sampled_maps(labels[b:b + 1], fs, mirrored=flips[b])[0] for b in range(2)])
                got, prob = torch.from_numpy(logit.copy()), torch.full((2, K, h, w), 7.0)
                out = object_plan.object_edit_softmax(got, torch.from_numpy(labels), torch.from_numpy(lut), torch.from_numpy(action), prob,
                                                      sampling=(step, step, flips))
                want, want_prob = torch.from_numpy(logit.copy()), torch.empty(2, K, h, w)
                object_plan.object_edit_softmax(want, torch.from_numpy(materialised), torch.from_numpy(lut), torch.from_numpy(action), want_prob)
                assert out is prob and _same_bits(got.numpy(), want.numpy()) and _same_bits(prob.numpy(), want_prob.numpy())
                for b in range(2):
                    edited = base.edit_frame(logit[b], materialised[b], lut[b], action[b])
                    assert _same_bits(got[b].numpy(), edited) and float(base.spread(edited).max()) <= base.D_MAX
                    p64, bound = base.softmax_bound(edited)
                    assert (np.abs(prob[b].numpy().astype(np.float64) - p64) <= bound).all()


def test_whole_clip_edits_with_the_scaled_plans_equal_the_literal_writes_on_resized_masks():
    """Frame by frame with the scale's plan and the FULL-SIZE label maps, the sampling edit gives the logits that the reference's index
    writes on nearest-resized (and mirrored) one-hot masks give -- on every hand-written clip, for both passes."""
    from rmnet_amd import object_plan, tta
    for name, (maps, cap, fs, _) in CASES.items():
        h, w = ref.scaled_size(*maps[0].shape, fs)
        words = torch.from_numpy(base.presence_words(maps).view(np.int32))
        plan = object_plan.appearance_plans(words, torch.from_numpy(_sampled_words(maps, fs).view(np.int32))[None], cap)[0]
        step = tta.scale_for_factor(fs)
        for mirrored in (False, True):
            logits = _logits_for(len(maps), cap + 1, h, w, seed=5)
            want = ref.reference_clip_scaled(maps, cap, fs, mirrored, logits=logits)['logits']
            got = torch.from_numpy(logits.copy())
            for t in sorted(plan.edited):
                object_plan.object_edit_softmax(got[t:t + 1], torch.from_numpy(maps[t])[None], plan.lut[None], plan.action[t:t + 1],
                                                torch.empty_like(got[t:t + 1]), sampling=(step, step, (mirrored,)))
            assert _same_bits(got.numpy(), want), (name, mirrored)


# ================================================================================================ CPU: argument rules
def test_argument_rules_of_the_two_new_entries_need_no_gpu():
    """Every refusal of the C entries comes before the first call into the runtime, so made-up addresses do for pointers."""
    import ctypes
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    p, odd = 0x10000, 0x10002
    assert lib.rmnet_label_presence_nearest_rows() > 0

    def presence(labels=p, N=1, Hs=4, Ws=4, hd=(2,), wd=(2,), sh=(2.0,), sw=(2.0,), S=None, out=p, null=None):
        n = len(hd)
        arrays = dict(hd=(ctypes.c_int * n)(*hd), wd=(ctypes.c_int * n)(*wd), sh=(ctypes.c_float * n)(*sh), sw=(ctypes.c_float * n)(*sw))
        ptr = {k: (None if k == null else ctypes.cast(v, ctypes.c_void_p)) for k, v in arrays.items()}
        return lib.rmnet_label_presence_nearest_u8(labels, N, Hs, Ws, ptr['hd'], ptr['wd'], ptr['sh'], ptr['sw'], n if S is None else S, out, None)

    for bad in (dict(labels=None), dict(out=None), dict(null='hd'), dict(null='wd'), dict(null='sh'), dict(null='sw'), dict(N=0), dict(Hs=0),
                dict(Ws=-1), dict(hd=(0,)), dict(wd=(0,)), dict(S=0), dict(out=odd), dict(sh=(0.0,)), dict(sw=(-1.0,)),
                dict(sh=(float('inf'),)), dict(sw=(float('nan'),)),
                dict(hd=(2,) * 9, wd=(2,) * 9, sh=(1.0,) * 9, sw=(1.0,) * 9)):
        assert presence(**bad) == INVALID, bad
    side = (1 << 24) + 1
    for unsupported in (dict(Hs=side, Ws=1), dict(Hs=1, Ws=side), dict(hd=(side,)), dict(wd=(side,)), dict(N=2, Hs=1 << 15, Ws=1 << 15)):
        assert presence(**unsupported) == UNSUPPORTED, unsupported

    def edit(logit=p, lbs=8, labels=p, labs=16, Hs=4, Ws=4, sh=2.0, sw=2.0, flips=0, lut=p, action=p, prob=p, pbs=8, B=1, K=2, H=2, W=2):
        return lib.rmnet_object_edit_softmax_nearest_f32(logit, lbs, labels, labs, Hs, Ws, sh, sw, flips, lut, action, prob, pbs, B, K, H, W, None)

    for missing in ('logit', 'lut', 'action', 'prob'):
        assert edit(**{missing: None}) == INVALID
    for bad in (dict(K=0), dict(K=256, lbs=1024, pbs=1024), dict(B=0), dict(H=0), dict(W=-1), dict(Hs=0), dict(Ws=0), dict(logit=odd),
                dict(prob=odd), dict(lbs=7), dict(pbs=7), dict(labs=15), dict(labs=-16), dict(sh=0.0), dict(sw=float('nan')),
                dict(sh=float('inf'))):
        assert edit(**bad) == INVALID, bad
    big = 1 << 31
    for unsupported in (dict(B=65), dict(lbs=big), dict(pbs=big), dict(labs=big), dict(Hs=side, Ws=1, labs=side), dict(Ws=side, Hs=1, labs=side),
                        dict(H=side, W=1, lbs=4 * side, pbs=4 * side), dict(H=1 << 15, W=1 << 15, lbs=big << 2, pbs=big << 2),
                        dict(Hs=1 << 16, Ws=1 << 16, labs=1 << 32), dict(B=3, lbs=big - 8, pbs=8)):
        assert edit(**unsupported) == UNSUPPORTED, unsupported
    # the bindings
    z = torch.zeros
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.label_presence_nearest(z(1, 2, 2, dtype=torch.uint8), [(1, 1)], [(2.0, 2.0)])
    with pytest.raises(RuntimeError, match=r'\[N, H, W\]'):
        ops.label_presence_nearest(z(2, 2, dtype=torch.uint8), [(1, 1)], [(2.0, 2.0)])
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.object_edit_softmax(z(1, 2, 2, 2), None, z(1, 256, dtype=torch.uint8), z(1, 2, dtype=torch.uint8), z(1, 2, 2, 2),
                                sampling=(1.0, 1.0, (False,)))
    from rmnet_amd import object_plan
    with pytest.raises(RuntimeError, match='one flip flag'):
        object_plan.object_edit_softmax(z(1, 2, 2, 2), None, z(1, 256, dtype=torch.uint8), z(1, 2, dtype=torch.uint8), z(1, 2, 2, 2),
                                        sampling=(1.0, 1.0, (False, True)))


class _Params(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))


def test_python_argument_rules():
    from rmnet_amd import inference, object_plan
    from rmnet_amd.rmnet import RMNet
    frames = torch.zeros(3, 3, 4, 4)
    labels = torch.zeros(3, 4, 4, dtype=torch.uint8)
    stand_in = _Params()
    with pytest.raises(RuntimeError, match="video\\['labels'\\]"):
        inference.segment_video_tta(stand_in, None, {'frames': frames}, (0.5, 1.0), True, new_objects=True, n_max_objects=2)
    with pytest.raises(RuntimeError, match='n_max_objects'):
        inference.segment_video_tta(stand_in, None, {'frames': frames, 'labels': labels}, (0.5, 1.0), True, new_objects=True)
    with pytest.raises(RuntimeError, match=r'uint8 \[N, H, W\]'):
        inference.segment_video_tta(stand_in, None, {'frames': frames, 'labels': labels[:2]}, (1.0,), new_objects=True, n_max_objects=2)
    # unchanged: without scale_plans the combination is refused with the text of before
    u8 = torch.zeros(3, 4, 4, 3, dtype=torch.uint8)
    for kw in (dict(frame_scales=(0.75, 1.0)), dict(flip_lr=True), dict(frame_scales=(0.75, 1.0), scale_plans=False)):
        with pytest.raises(RuntimeError, match='frame_scales / flip_lr'):
            inference.segment_video_u8(None, None, u8, labels, 2, clip_io_ref.MEAN, clip_io_ref.STD, new_objects=True, **kw)
    # forward: a three-tuple whose sizes do not fit, refused before anything runs on a device
    net = RMNet(None).eval()
    words = torch.from_numpy(base.presence_words(labels.numpy()).view(np.int32))
    plan = object_plan.appearance_plan(words, 2)
    cpu = torch.device('cpu')
    call = lambda fr, lab, plans, sampling: net(fr, torch.zeros(1, 1, 3, *fr.shape[-2:]), torch.zeros(1, 3, 2, *fr.shape[-2:]), None, 5,
                                                device=cpu, object_plan=(lab, plans, sampling))
    full = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    for fr, lab, plans, sampling in ((torch.zeros(1, 3, 3, 4, 4), full, [plan], (0.75, (False,))),         # 8 * 0.75 = 6, not 4
                                     (torch.zeros(1, 3, 3, 4, 4), full, [plan], (0.5, (False, True))),     # two flags, one slot
                                     (torch.zeros(1, 3, 3, 4, 4), full[0], [plan], (0.5, (False,))),       # labels without a batch axis
                                     (torch.zeros(1, 3, 3, 4, 4), full[:, :2], [plan], (0.5, (False,)))):  # two frames of labels
        with pytest.raises(RuntimeError, match='sampling'):
            call(fr, lab, plans, sampling)
    with pytest.raises(RuntimeError, match='one plan of N frames and K planes per clip'):                 # right sizes, no plan for the slot
        call(torch.zeros(1, 3, 3, 4, 4), full, [], (0.5, (False,)))
    with pytest.raises(RuntimeError, match='one plan of N frames and K planes per clip'):                 # the two-tuple form, as before
        net(torch.zeros(1, 3, 3, 4, 4), torch.zeros(1, 1, 3, 4, 4), torch.zeros(1, 3, 2, 4, 4), None, 5, device=cpu, object_plan=(full, [plan]))


# ================================================================================================ GPU: the presence kernel
def _guarded_u8(n_bytes, offset, fill=0xA5):
    """(buffer, view of n_bytes that starts ``offset`` bytes past a 16-byte boundary, with at least 32 guard bytes on either side)."""
    buf = torch.full((32 + 16 + n_bytes + 32,), fill, dtype=torch.uint8, device=dev())
    start = 32 + ((-(buf.data_ptr() + 32)) % 16) + offset
    return buf, buf[start:start + n_bytes]


def _entries(H, W, factors):
    """(sizes, scales) of the kernel's entries for the factors; a factor that leaves no pixel is replaced by 1.0."""
    from rmnet_amd import tta
    factors = [fs if min(tta.scaled_size(H, W, fs)) >= 1 else 1.0 for fs in factors]
    return factors, [tta.scaled_size(H, W, fs) for fs in factors], [(tta.scale_for_factor(fs),) * 2 for fs in factors]


def _scaled_presence_of(maps, factors, offset=0):
    """The kernel's words [S,N,8] for uint8 [N,H,W] at a byte offset inside a guarded buffer, which must come back unchanged, and the
    restatement's words for the same factors."""
    from rmnet_amd import ops
    N, H, W = maps.shape
    factors, sizes, scales = _entries(H, W, factors)
    buf, view = _guarded_u8(maps.size, offset)
    view.copy_(torch.from_numpy(maps.reshape(-1)).to(dev()))
    t = view.view(N, H, W)
    assert t.data_ptr() % 16 == offset
    before = buf.clone()
    got = ops.label_presence_nearest(t, sizes, scales)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(factors), N, 8)
    return got.cpu().numpy().view(np.uint32), np.stack([_sampled_words(maps, fs) for fs in factors])


@gpu
def test_presence_kernel_is_exhaustive_over_the_index_rule():
    """Maps whose pixels hold distinct values: a word differs as soon as one source pixel is read that the rule does not read, or the
    reverse.  Each factor on its own and all seven in one launch."""
    for H, W in ((1, 1), (1, 7), (7, 1), (6, 6), (12, 13), (15, 17)):
        maps = np.arange(H * W, dtype=np.uint8).reshape(1, H, W)
        assert len(np.unique(maps)) == H * W
        for fs in FACTORS:
            got, want = _scaled_presence_of(maps, [fs])
            assert np.array_equal(got, want), (H, W, fs)
        got, want = _scaled_presence_of(maps, FACTORS)
        assert np.array_equal(got, want), (H, W)
    got, want = _scaled_presence_of(np.arange(36, dtype=np.uint8).reshape(1, 6, 6), [1.25])
    # row 5 (30 .. 35) and column 5 (5, 11, .. 29) are never read; (4, 4) = 28 is
    assert not (want[0, 0, 0] >> 30) & 1 and not (want[0, 0, 0] >> 29) & 1 and (want[0, 0, 0] >> 28) & 1 and np.array_equal(got, want)


@gpu
def test_presence_kernel_structure_widths_offsets_and_entry_counts():
    """Three frames of different content (a frame mix-up shows), source widths 1 .. 70 and 260 at heights 1 .. 3, every byte offset
    0 .. 15 and every entry count 1 .. 8, cycled over the sizes; guards untouched."""
    rng = np.random.RandomState(6)
    pool = FACTORS + (1.3,)
    offsets, counts = set(), set()
    case = 0
    for W in list(range(1, 71)) + [260]:
        for H in (1, 2, 3):
            maps = np.stack([np.asarray(ids, np.uint8)[rng.randint(0, 4, size=(H, W))] for ids in ((0, 5, 9, 200), (3, 31, 32, 64), (63, 254, 255, 1))])
            offset, S = case % 16, 1 + (case // 3) % 8
            factors = [pool[(case + i) % len(pool)] for i in range(S)]
            got, want = _scaled_presence_of(maps, factors, offset)
            assert np.array_equal(got, want), (H, W, offset, factors)
            offsets.add(offset)
            counts.add(S)
            case += 1
    assert offsets == set(range(16)) and counts == set(range(1, 9))


@gpu
def test_presence_kernel_beyond_one_workgroup_all_values_one_value_and_a_graph_replay():
    from rmnet_amd import ops, tta
    rows = ops.label_presence_nearest_rows()
    rng = np.random.RandomState(7)
    H, W = 2 * rows + 6, 70                               # three workgroups per frame at 1.0, two at 0.5, four at 1.25
    for fs in (0.5, 1.0, 1.25):
        h = tta.scaled_size(H, W, fs)[0]
        assert h > rows
        last = int(tta.nearest_index(h, H, fs)[-1])       # the last sampled source row
        maps = np.asarray([0, 5, 9], np.uint8)[rng.randint(0, 3, size=(2, H, W))]
        maps[1, last, 0] = 200                            # only in the last sampled row of frame 1, in a sampled column
        got, want = _scaled_presence_of(maps, [fs, 1.0], 3)
        assert np.array_equal(got, want) and (got[0, 1, 200 >> 5] >> (200 & 31)) & 1 and not (got[0, 0, 200 >> 5] >> (200 & 31)) & 1
    every = np.arange(256, dtype=np.uint8)[rng.permutation(256)].reshape(1, 16, 16)
    got, want = _scaled_presence_of(every, [1.0, 2.0, 0.5], 5)
    assert (got[:2] == np.uint32(0xffffffff)).all() and np.array_equal(got, want)
    for v in (0, 31, 32, 63, 64, 255):
        got, want = _scaled_presence_of(np.full((1, 7, 11), v, np.uint8), FACTORS, 9)
        one = np.zeros(8, np.uint32)
        one[v >> 5] = np.uint32(1) << np.uint32(v & 31)
        assert np.array_equal(got, want) and (got == one).all(), v
    # one capture, replayed on other label maps: the entry zeroes its output inside the graph
    first = rng.randint(0, 256, size=(2, 9, 31)).astype(np.uint8)
    second = np.asarray([3, 64], np.uint8)[rng.randint(0, 2, size=(2, 9, 31))]
    factors, sizes, scales = _entries(9, 31, (0.5, 1.25))
    labels = torch.from_numpy(first).to(dev())
    stream = torch.cuda.Stream(dev())
    stream.wait_stream(torch.cuda.current_stream(dev()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        ops.label_presence_nearest(labels, sizes, scales)
        with torch.cuda.graph(graph, stream=stream):
            out = ops.label_presence_nearest(labels, sizes, scales)
        labels.copy_(torch.from_numpy(second).to(dev()))
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(dev()).wait_stream(stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.stack([_sampled_words(second, fs) for fs in factors]))


@gpu
def test_label_presence_scaled_takes_the_kernel_and_equals_its_torch_route():
    from rmnet_amd import object_plan
    rng = np.random.RandomState(8)
    maps = np.asarray(ID_POOL, np.uint8)[rng.randint(0, len(ID_POOL), size=(4, 12, 13))]
    got = object_plan.label_presence_scaled(torch.from_numpy(maps).to(dev()), 12, 13, FACTORS)
    want = object_plan.label_presence_scaled(torch.from_numpy(maps), 12, 13, FACTORS)
    assert got.is_cuda and torch.equal(got.cpu(), want)


# ================================================================================================ GPU: the edit kernel
SENTINEL = 12345.0
FLIP_BITS = (0, 1, 2, 3, 5)


def _source_side(out, fs):
    return max(1, int(math.ceil(out / fs)))


def _run_both_edits(logit, labels, lut, action, step, flips, h, w):
    """The sampling entry on est[:, 1] / labels[:, 1] of guarded [B,3,...] tensors and the existing entry on the materialised
    (mirrored) maps; returns both (logit, prob) pairs as numpy arrays and asserts that nothing outside the slices changed."""
    from rmnet_amd import ops
    B, K = action.shape
    d = dev()
    lbuf = torch.full((B, 3, K, h, w), SENTINEL, device=d)
    pbuf = torch.full((B, 3, K, h, w), SENTINEL, device=d)
    lbuf[:, 1] = torch.from_numpy(logit).to(d)
    ubuf = None
    if labels is not None:
        ubuf = torch.full((B, 3) + labels.shape[1:], 77, dtype=torch.uint8, device=d)
        ubuf[:, 1] = torch.from_numpy(labels).to(d)
    t_lut, t_action = torch.from_numpy(lut).to(d), torch.from_numpy(action).to(d)
    out = ops.object_edit_softmax(lbuf[:, 1], None if ubuf is None else ubuf[:, 1], t_lut, t_action, pbuf[:, 1], sampling=(step, step, flips))
    torch.cuda.synchronize()
    assert out.data_ptr() == pbuf[:, 1].data_ptr()
    for buf in (lbuf, pbuf):
        assert bool((buf[:, 0] == SENTINEL).all()) and bool((buf[:, 2] == SENTINEL).all())
    if ubuf is not None:
        assert bool((ubuf[:, 0] == 77).all()) and bool((ubuf[:, 2] == 77).all()) and torch.equal(ubuf[:, 1].cpu(), torch.from_numpy(labels))
    materialised = None
    if labels is not None:
        materialised = np.stack([ref.sampled_maps(labels[b:b + 1], None, mirrored=flips[b], resize=(h, w, step, step))[0] for b in range(B)])
    want_logit = torch.from_numpy(logit).to(d)
    want_prob = torch.empty(B, K, h, w, device=d)
    ops.object_edit_softmax(want_logit, None if materialised is None else torch.from_numpy(materialised).to(d), t_lut, t_action, want_prob)
    return (lbuf[:, 1].cpu().numpy(), pbuf[:, 1].cpu().numpy()), (want_logit.cpu().numpy(), want_prob.cpu().numpy()), materialised


@gpu
@pytest.mark.parametrize('K', [1, 2, 3, 11, 255])
def test_sampling_edit_kernel_equals_the_existing_entry_on_the_materialised_map_in_every_bit(K):
    """Output widths 1 .. 9, 64, 65 at heights 1 .. 3: one-pixel lanes (H*W % 4 != 0), four-pixel lanes inside one row (W % 4 == 0),
    four-pixel lanes that cross a row end (H*W % 4 == 0 with W % 4 != 0: 2 x 2, 6 x 2) and rows longer than a wave; the factors 0.5,
    0.75, 1.25, 2.0; B = 1, 2, 3 with the flip bits 0, 1, 2, 3, 5 cycled over the sizes.  (W % 4 == 0 with H*W % 4 != 0 does not exist.)"""
    from rmnet_amd import tta
    rng = np.random.RandomState(400 + K)
    combos = [(B, bits) for B in (1, 2, 3) for bits in FLIP_BITS]
    seen, forms, case = set(), set(), 0
    for w in list(range(1, 10)) + [64, 65]:
        for h in (1, 2, 3):
            for fs in (0.5, 0.75, 1.25, 2.0):
                B, bits = combos[case % len(combos)]
                case += 1
                flips = tuple(bool((bits >> b) & 1) for b in range(B))
                step = tta.scale_for_factor(fs)
                logit, labels, lut, actions = _edit_inputs(rng, B, K, _source_side(h, fs), _source_side(w, fs), h, w)
                got, want, materialised = _run_both_edits(logit, labels, lut, actions[case % 2], step, flips, h, w)
                assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), (K, h, w, fs, B, bits)
                for b in range(B):
                    assert _same_bits(got[0][b], base.edit_frame(logit[b], materialised[b], lut[b], actions[case % 2][b]))
                seen.add((B, bits))
                forms.add(((h * w) % 4 == 0, w % 4 == 0))
    assert seen == set(combos) and forms == {(True, True), (True, False), (False, False)}


@gpu
def test_sampling_edit_kernel_without_labels_and_one_graph_replay():
    from rmnet_amd import ops, tta
    rng = np.random.RandomState(10)
    d = dev()
    step = tta.scale_for_factor(0.75)
    h, w = 6, 8
    logit, labels, lut, (mixed, inject_all) = _edit_inputs(rng, 2, 3, 8, 11, h, w)
    # no label map and an inject action: m = 0 everywhere, as the existing entry has it
    got, want, _ = _run_both_edits(logit, None, lut, inject_all, step, (False, True), h, w)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert (np.ascontiguousarray(got[0]).view(np.uint32) == np.float32(-16.1181).view(np.uint32)).all()
    # one capture, replayed on other logits and actions
    logit_b = (rng.rand(2, 3, h, w) * 31.9 - 16.0).astype(np.float32)
    t_logit, t_action = torch.from_numpy(logit).to(d), torch.from_numpy(mixed).to(d)
    t_labels, t_lut, t_prob = torch.from_numpy(labels).to(d), torch.from_numpy(lut).to(d), torch.empty(2, 3, h, w, device=d)
    stream = torch.cuda.Stream(d)
    stream.wait_stream(torch.cuda.current_stream(d))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        ops.object_edit_softmax(t_logit, t_labels, t_lut, t_action, t_prob, sampling=(step, step, (True, False)))
        with torch.cuda.graph(graph, stream=stream):
            ops.object_edit_softmax(t_logit, t_labels, t_lut, t_action, t_prob, sampling=(step, step, (True, False)))
        t_logit.copy_(torch.from_numpy(logit_b).to(d))
        t_action.copy_(torch.from_numpy(inject_all).to(d))
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(d).wait_stream(stream)
    got, want, _ = _run_both_edits(logit_b, labels, lut, inject_all, step, (True, False), h, w)
    assert _same_bits(t_logit.cpu().numpy(), want[0]) and _same_bits(t_prob.cpu().numpy(), want[1])


# ================================================================================================ GPU: torch's device nearest kernel
@gpu
def test_torchs_device_nearest_kernel_follows_the_formula_off_the_special_sizes():
    """F.interpolate(mode='nearest') on the device -- what helpers.multi_scale_inference resizes its masks with -- against
    ``nearest_index``; required equal wherever no axis is special.  At three special sizes the rule it follows is printed, not
    asserted (profiles/r30_a_scaled_plans.md records it)."""
    from rmnet_amd import tta
    d = dev()
    ran = 0
    for fs in TWELVE:
        for H in range(1, 71):
            for W in (1, 5, 33, 64):
                h, w = tta.scaled_size(H, W, fs)
                if h < 1 or w < 1 or _special(H, fs) or _special(W, fs):
                    continue
                x = (torch.arange(H * W, dtype=torch.float32, device=d) % 251.0).view(1, 1, H, W)
                want = F.interpolate(x, scale_factor=fs, mode='nearest')[0, 0]
                iy, ix = torch.from_numpy(tta.nearest_index(h, H, fs)).to(d), torch.from_numpy(tta.nearest_index(w, W, fs)).to(d)
                assert torch.equal(x[0, 0].index_select(0, iy).index_select(1, ix), want), (fs, H, W)
                ran += 1
    assert ran > 2000
    for H, W, fs in ((68, 33, 1.01), (68, 64, 1.01), (5, 5, 1.1)):
        x = torch.arange(H * W, dtype=torch.float32, device=d).view(1, 1, H, W)
        got = F.interpolate(x, scale_factor=fs, mode='nearest')[0, 0]
        h, w = tta.scaled_size(H, W, fs)
        iy, ix = torch.from_numpy(tta.nearest_index(h, H, fs)).to(d), torch.from_numpy(tta.nearest_index(w, W, fs)).to(d)
        formula = bool(torch.equal(x[0, 0].index_select(0, iy).index_select(1, ix), got))
        copy = bool(tuple(got.shape) == (H, W) and torch.equal(got, x[0, 0]))
        print('device nearest kernel at %d x %d, factor %g: formula %s, copy %s' % (H, W, fs, formula, copy))


# ================================================================================================ GPU: whole clips
class _Recorder:
    """Stands where the network stands in the drivers and keeps what went in and what came out."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, frames, masks, flows, n_objects, memorize_every, **kw):
        est = self.net(frames, masks, flows, n_objects, memorize_every, **kw)
        self.calls.append({'frames': frames, 'masks': masks, 'flows': flows, 'n_objects': n_objects, 'kw': kw, 'est': est})
        return est


H_CLIP, W_CLIP = 96, 160


def _flows_for(clip):
    """The supplied flows of the synthetic clip (a constant drift of (-3, -2) pixels at full size) at the clip's scale."""
    fl = torch.zeros(clip.shape[0], clip.shape[1], 2, clip.shape[3], clip.shape[4], device=clip.device)
    fl[:, :, 0] = -3.0 * clip.shape[4] / W_CLIP
    fl[:, :, 1] = -2.0 * clip.shape[3] / H_CLIP
    return fl


@pytest.fixture(scope='module')
def late_clip():
    """The late-object clip of tests/test_late_objects.py (5 frames, 96 x 160, ids 0, 5, 38, object 2 from frame 2), its variant with
    object 2's first annotation cut down to one pixel at an odd row and column, and the procedural weights."""
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    frames, masks, _, _ = synthetic_clip(5, 3, H_CLIP, W_CLIP, seed=11, size=1.3)
    planes = masks[0].argmax(dim=1).numpy()
    planes[:2][planes[:2] == 2] = 0
    labels = np.asarray([0, 5, 38], np.uint8)[planes]
    cut = labels.copy()
    ys, xs = np.nonzero((labels[2] == 38) & (np.arange(H_CLIP)[:, None] % 2 == 1) & (np.arange(W_CLIP)[None, :] % 2 == 1))
    cut[2][cut[2] == 38] = 0
    cut[2, ys[len(ys) // 2], xs[len(xs) // 2]] = 38
    assert int((cut[2] == 38).sum()) == 1
    mean, std = torch.tensor(clip_io_ref.MEAN).view(1, 3, 1, 1), torch.tensor(clip_io_ref.STD).view(1, 3, 1, 1)
    u8 = ((frames[0] * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    f32 = torch.from_numpy(clip_io_ref.normalize(u8.numpy())).unsqueeze(0)
    return dict(u8=u8, f32=f32, labels=labels, cut=cut, state=networks.procedural_init_(RMNet(None)).state_dict())


def _reproducible():
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _net(c):
    from rmnet_amd.rmnet import RMNet
    net = RMNet(None)
    net.load_state_dict(c['state'])
    return net.to(dev()).eval()


def _reference_route(net, c, labels, scales, flip, device):
    """helpers.multi_scale_inference on the same network, fed the one-hot masks of ALL frames and the per-frame counts."""
    from types import SimpleNamespace
    from rmnet_amd import helpers
    r = base.reference_clip(list(labels), 2)
    cfg = SimpleNamespace(TEST=SimpleNamespace(FRAME_SCALES=list(scales), FLIP_LR=flip, MEMORIZE_EVERY=2))
    masks_all = torch.from_numpy(r['masks']).unsqueeze(0)
    counts = torch.tensor([r['n_objects']], dtype=torch.long)
    with torch.no_grad():
        _, probs = helpers.multi_scale_inference(cfg, _flows_for, net, c['f32'].to(device), masks_all.to(device), counts)
    return probs[0].cpu(), r


def _meets_the_bars(what, probs, want):
    """The bars tests/test_tta.py uses against multi_scale_inference: atol 3e-3 on the probabilities, label agreement > 0.999."""
    diff = float((probs - want).abs().max())
    agree = float((probs.argmax(1) == want.argmax(1)).float().mean())
    print('%s: max |dp| %.3e, label agreement %.5f' % (what, diff, agree))
    assert diff < 3e-3 and agree > 0.999, what


@gpu
@pytest.mark.parametrize('pair_flips', [True, False])
def test_late_object_clip_at_three_scales_with_the_flip_against_multi_scale_inference(pair_flips, late_clip, monkeypatch):
    from rmnet_amd import inference
    c = late_clip
    net = _net(c)
    rec = _Recorder(net)
    monkeypatch.setattr(inference, 'PAIR_FLIPS', pair_flips)
    scales = (0.75, 1.0, 1.25)
    with _reproducible(), torch.no_grad():
        out = inference.segment_video_u8(rec, _flows_for, c['u8'], torch.from_numpy(c['labels']), 2, clip_io_ref.MEAN, clip_io_ref.STD,
                                         memorize_every=2, frame_scales=scales, flip_lr=True, new_objects=True, scale_plans=True)
        probs = inference.segment_video_tta(net, _flows_for, {'frames': c['f32'][0], 'labels': torch.from_numpy(c['labels'])}, scales, True, 2,
                                            pair_flips=pair_flips, new_objects=True, n_max_objects=2)
        want, r = _reference_route(net, c, c['labels'], scales, True, dev())
    assert len(rec.calls) == (3 if pair_flips else 6)
    from rmnet_amd import tta
    for i, call in enumerate(rec.calls):
        fs = scales[i if pair_flips else i // 2]
        h, w = tta.scaled_size(H_CLIP, W_CLIP, fs)
        B = 2 if pair_flips else 1
        assert tuple(call['masks'].shape) == (B, 1, 3, h, w) and call['n_objects'] is None and tuple(call['frames'].shape) == (B, 5, 3, h, w)
        labels, plans, sampling = call['kw']['object_plan']
        assert tuple(labels.shape) == (B, 5, H_CLIP, W_CLIP) and labels.dtype == torch.uint8 and torch.equal(labels[0].cpu(), torch.from_numpy(c['labels']))
        assert len(plans) == B and sampling[0] == fs and tuple(sampling[1]) == ((False, True) if pair_flips else (bool(i % 2),))
        assert plans[0].action_host.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 0], [0, 0, 0]]
    assert out['ids'].tolist() == [0, 5, 38] and out['n_objects_per_frame'] == [1, 1, 2, 2, 2] and out['n_objects'] == 2
    assert probs['ids'].tolist() == [0, 5, 38] and probs['n_objects_per_frame'] == r['n_objects']
    _meets_the_bars('driver against multi_scale_inference, pair_flips %s' % pair_flips, probs['probs'].cpu(), want)
    agree = float((out['labels'].cpu() == want.argmax(1)).float().mean())
    print('segment_video_u8 labels against multi_scale_inference %.5f' % agree)
    assert agree > 0.999 and out['overlay'] is not None
    pixels = [int((out['labels'][t] == 2).sum()) for t in range(5)]
    print('pixels of object 2 per frame', pixels)
    assert pixels[0] == 0 and pixels[1] == 0 and all(p > 0 for p in pixels[2:])


@gpu
def test_an_annotation_that_a_scale_loses_is_not_injected_there(late_clip):
    """Object 2's frame-2 annotation is one pixel at an odd row and column: the 0.5 scale never reads it, its plan injects nothing (and,
    the count never changing again, keeps the object absent), the 1.0 scale injects it; the driver still meets the bars."""
    from rmnet_amd import inference, object_plan
    c = late_clip
    cut = torch.from_numpy(c['cut']).to(dev())
    plans = object_plan.appearance_plans(object_plan.label_presence(cut), object_plan.label_presence_scaled(cut, H_CLIP, W_CLIP, (0.5, 1.0)), 2)
    assert plans[0].n_objects == plans[1].n_objects == [1, 1, 2, 2, 2] and plans[0].fresh == {2}
    assert plans[0].action_host.tolist() == [[0, 0, 0]] + [[0, 0, 1]] * 4 and not (plans[0].action_host == 2).any()
    assert plans[1].action_host.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 0], [0, 0, 0]]
    for p, fs in zip(plans, (0.5, 1.0)):
        assert _plan_fields(p) == _fields(ref.reference_clip_scaled(list(c['cut']), 2, fs))
    net = _net(c)
    with _reproducible(), torch.no_grad():
        got = inference.segment_video_tta(net, _flows_for, {'frames': c['f32'][0], 'labels': torch.from_numpy(c['cut'])}, (0.5, 1.0), True, 2,
                                          new_objects=True, n_max_objects=2)
        want, _ = _reference_route(net, c, c['cut'], (0.5, 1.0), True, dev())
    _meets_the_bars('cut-down annotation at (0.5, 1.0)', got['probs'].cpu(), want)


@gpu
def test_late_object_clip_against_the_oracles_cpu_path_through_multi_scale_inference(late_clip, oracle_mod):
    from rmnet_amd import inference
    c = late_clip
    oracle_net = oracle_mod.OracleRMNet()
    oracle_net.load_state_dict(c['state'])
    want, _ = _reference_route(oracle_net.eval(), c, c['labels'], (0.75, 1.0), True, torch.device('cpu'))
    with _reproducible(), torch.no_grad():
        got = inference.segment_video_tta(_net(c), _flows_for, {'frames': c['f32'][0], 'labels': torch.from_numpy(c['labels'])}, (0.75, 1.0), True, 2,
                                          new_objects=True, n_max_objects=2)
    _meets_the_bars('driver against the CPU path at (0.75, 1.0) with the flip', got['probs'].cpu(), want)


@gpu
def test_one_scale_without_flip_through_the_new_route_is_the_single_scale_protocol(late_clip):
    from rmnet_amd import inference
    c = late_clip
    net = _Recorder(_net(c))
    with _reproducible(), torch.no_grad():
        new = inference.segment_video_tta(net, _flows_for, {'frames': c['f32'][0], 'labels': torch.from_numpy(c['labels'])}, (1.0,), False, 2,
                                          new_objects=True, n_max_objects=2)
        old = inference.segment_video_u8(net, _flows_for, c['u8'], torch.from_numpy(c['labels']), 2, clip_io_ref.MEAN, clip_io_ref.STD,
                                         memorize_every=2, new_objects=True)
    mine, theirs = net.calls
    assert torch.equal(mine['frames'], theirs['frames']) and torch.equal(mine['masks'].float(), theirs['masks'].float())
    assert mine['kw']['object_plan'][1][0].action_host.tolist() == theirs['kw']['object_plan'][1][0].action_host.tolist()
    diff = float((mine['est'] - theirs['est']).abs().max())
    print('new route against segment_video_u8(new_objects=True): max |dp| %.3e' % diff)
    assert diff < 1e-3                                    # (two runs of one route already differ in late frames: tests/test_late_objects.py)
    assert torch.equal(new['labels'], old['labels']) and new['ids'].tolist() == old['ids'].tolist() == [0, 5, 38]
    assert new['n_objects_per_frame'] == old['n_objects_per_frame']


# ================================================================================================ CPU: the compiler's resources
def test_the_new_kernels_use_no_lds_and_no_scratch_and_the_existing_edit_keeps_its_registers(tmp_path):
    """From the metadata of a compile-only gfx950 build (tests/test_kernel_resources.py): the issue asks for no LDS and no scratch in
    the sampling presence kernel, and that factoring the walks out of lo_edit leaves that kernel's resources where they were (31 and
    17 VGPRs for the four-pixel and the one-pixel form, profiles/r29_a_late_objects.md)."""
    from test_kernel_resources import _compile, _kernels
    found = _kernels(_compile('late_objects.hip', str(tmp_path / 'late_objects.s')))
    one = lambda fragment: [k for n, k in found.items() if fragment in n]
    new = one('19lo_presence_nearestE') + one('15lo_edit_nearestILi4EE') + one('15lo_edit_nearestILi1EE')
    assert len(new) == 3 and len(found) == 6
    for k in found.values():
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
    (edit4,), (edit1,) = one('7lo_editILi4EE'), one('7lo_editILi1EE')
    assert edit4['vgpr_count'] == 31 and edit1['vgpr_count'] == 17
