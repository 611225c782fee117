# -*- coding: utf-8 -*-
"""Objects that are first annotated in the middle of a clip (the YouTube-VOS protocol): rmnet_amd.object_plan, the two kernels of
csrc/late_objects.hip, RMNet.forward(object_plan=) and inference.segment_video_u8(new_objects=True), against the literal numpy
restatement of the reference in tests/late_objects_ref.py.

Without a GPU: the restatement is pinned by hand-written clips whose answers stand in this file, every planted fault of the
restatement is caught by a named clip, ``appearance_plan`` equals the restatement in every field on those clips and on random
ones, and the torch routes of both operations return the restatement's words / logit bits and probabilities inside the derived
bound.  On the GPU: every word of the presence kernel and every logit bit / probability of the edit kernel over the sizes at which
their code takes another path, inside guarded buffers, and a whole clip against the oracle's CPU path."""

import numpy as np
import pytest
import torch

import clip_io_ref
import late_objects_ref as ref

gpu = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4                                          # RMNET_E_INVALID_ARG, RMNET_E_UNSUPPORTED
INJECT_HI = np.float32(np.float32(32.0605) - np.float32(16.1181))      # m = 1: fl(fl(1 * 32.0605f) - 16.1181f)
ABSENT = np.float32(-16.1181)                                          # m = 0: fl(0 - 16.1181f), and the absent logit
ID_POOL = (0, 3, 5, 9, 31, 32, 63, 64, 200, 254, 255)


def dev():
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    return torch.device('cuda', 0)


def frame(*ids):
    """A 2 x 3 label map that holds exactly ``ids`` (the first one fills what is left)."""
    return np.asarray((list(ids) + [ids[0]] * 6)[:6], np.uint8).reshape(2, 3)


# name -> (label maps, n_max_objects, the answers).  K = n_max_objects + 1 planes.
CASES = {
    # ids [0, 5, 9] -> planes 0, 1, 2; object 2 is absent at frame 1, injected at frame 2, and stays when id 5 has gone
    'appears_at_frame_2': ([frame(0, 5), frame(0, 5), frame(0, 5, 9), frame(0, 9)], 2, dict(
        ids=[0, 5, 9], n_objects=[1, 1, 2, 2], fresh={2}, seen=[{0, 1}, {0, 1}, {0, 1, 2}, {0, 2}],
        action=[[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 0]])),
    'two_at_once': ([frame(0, 3), frame(0, 3, 5, 9)], 3, dict(
        ids=[0, 3, 5, 9], n_objects=[1, 3], fresh={1}, seen=[{0, 1}, {0, 1, 2, 3}], action=[[0, 0, 0, 0], [0, 0, 2, 2]])),
    # the late id 3 is smaller than the early id 9: over the clip 9 is plane 2 from frame 0 on, and plane 1 is the late one
    'late_object_with_smaller_id': ([frame(0, 9), frame(0, 9), frame(0, 3, 9)], 2, dict(
        ids=[0, 3, 9], n_objects=[1, 1, 2], fresh={2}, seen=[{0, 2}, {0, 2}, {0, 1, 2}], action=[[0, 0, 0], [0, 1, 0], [0, 2, 0]])),
    # one object allowed: id 9 arrives when the count already stands at the cap, no frame is fresh, 9 has no plane (falls on 0)
    'clamp_swallows_a_new_id': ([frame(0, 5), frame(0, 5, 9)], 1, dict(
        ids=[0, 5, 9], n_objects=[1, 1], fresh=set(), seen=[{0, 1}, {0, 1}], action=[[0, 0], [0, 0]])),
    # ids 5 and 9 renumber to 2 and 3 >= K = 2: no plane, their pixels' argmax is plane 0
    'ids_beyond_the_planes': ([frame(0, 3), frame(0, 5, 9)], 1, dict(
        ids=[0, 3, 5, 9], n_objects=[1, 1], fresh=set(), seen=[{0, 1}, {0}], action=[[0, 0], [0, 0]])),
    # 255 is no id and its pixels fall on plane 0
    'ignored_label': ([frame(0, 5, 255), frame(255, 9)], 2, dict(
        ids=[0, 5, 9], n_objects=[1, 2], fresh={1}, seen=[{0, 1}, {0, 2}], action=[[0, 0, 0], [0, 0, 2]])),
    # frame 0 holds one object and no background: plane 0 is absent, then injected like any object
    'frame_0_without_background': ([frame(5), frame(5), frame(0, 5), frame(0, 5, 9)], 2, dict(
        ids=[0, 5, 9], n_objects=[0, 0, 1, 2], fresh={2, 3}, seen=[{1}, {1}, {0, 1}, {0, 1, 2}],
        action=[[0, 0, 0], [1, 0, 1], [2, 0, 1], [0, 0, 2]])),
    # background injected while id 9 (plane 2 >= K = 2) is in the frame: the injected mask is label == 0, not argmax == 0
    'background_injected_next_to_an_id_without_plane': ([frame(5), frame(0, 5, 9)], 1, dict(
        ids=[0, 5, 9], n_objects=[0, 1], fresh={1}, seen=[{1}, {0, 1}], action=[[0, 0], [2, 0]])),
    # id 9 appears, disappears and returns at a fresh frame: it is not injected a second time
    'disappears_and_returns': ([frame(0, 5), frame(0, 5, 9), frame(0, 5), frame(0, 5, 9, 31)], 3, dict(
        ids=[0, 5, 9, 31], n_objects=[1, 2, 2, 3], fresh={1, 3}, seen=[{0, 1}, {0, 1, 2}, {0, 1}, {0, 1, 2, 3}],
        action=[[0, 0, 0, 0], [0, 0, 2, 1], [0, 0, 0, 1], [0, 0, 0, 2]])),
}
# planted fault of the restatement -> the clip that catches it
CAUGHT_BY = {
    'count_per_frame': 'appears_at_frame_2',
    'table_per_frame': 'late_object_with_smaller_id',
    'clamp_dropped': 'clamp_swallows_a_new_id',
    'fresh_from_ids': 'clamp_swallows_a_new_id',
    'ids_ge_K_to_last': 'ids_beyond_the_planes',
    'inject_from_argmax': 'background_injected_next_to_an_id_without_plane',
    'existing_reset': 'disappears_and_returns',
    'absent_before_inject': 'frame_0_without_background',
}


def _logits_for(maps, K, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.rand(len(maps), K, *maps[0].shape) * 31.9 - 16.0).astype(np.float32)


def _fields(r):
    """The comparable fields of a restatement result."""
    return dict(ids=[int(i) for i in r['ids']], lut=r['lut'].tolist(), n_objects=list(r['n_objects']), n_max=r['n_max'], fresh=set(r['fresh']),
                seen=[set(s) for s in r['seen']], action=r['action'].tolist(), edited=set(r['edited']))


def _plan_fields(p):
    return dict(ids=[int(i) for i in p.ids], lut=p.lut_host.tolist(), n_objects=list(p.n_objects), n_max=p.n_max, fresh=set(p.fresh),
                seen=[set(s) for s in p.seen], action=p.action_host.tolist(), edited=set(p.edited))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ================================================================================================ CPU: the restatement, pinned
@pytest.mark.parametrize('name', sorted(CASES))
def test_the_restatement_gives_the_hand_written_answers(name):
    maps, n_cap, want = CASES[name]
    got = _fields(ref.reference_clip(maps, n_cap))
    lut = [0] * 256
    for i, v in enumerate(want['ids']):
        lut[v] = i
    want = dict(want, lut=lut, n_max=want['n_objects'][-1], edited={t for t, row in enumerate(want['action']) if any(row)})
    assert got == want


def test_the_injected_and_absent_logits_of_the_restatement_are_the_fp32_literals():
    """frame 1 of the case that injects the background: label 0 -> fl(fl(32.0605f) - 16.1181f), labels 5 and 9 -> -16.1181f; 9 has
    no plane, so an injection from the argmax set would have counted it as background.  Everything else keeps its bits."""
    maps, n_cap, _ = CASES['background_injected_next_to_an_id_without_plane']
    logits = _logits_for(maps, n_cap + 1)
    out = ref.reference_clip(maps, n_cap, logits=logits)['logits']
    assert float(INJECT_HI) == pytest.approx(15.9424, abs=1e-4) and ABSENT == np.float32(-16.1181)
    want = np.where(maps[1] == 0, INJECT_HI, ABSENT).astype(np.float32)
    assert _same_bits(out[1, 0], want) and _same_bits(out[1, 1], logits[1, 1]) and _same_bits(out[0], logits[0])
    # the literal writes and the one-frame form of the kernel (lut[label] == k) are the same thing
    r = ref.reference_clip(maps, n_cap)
    assert _same_bits(ref.edit_frame(logits[1], maps[1], r['lut'], r['action'][1]), out[1])


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_every_planted_fault_is_caught_by_its_named_case(mutant):
    maps, n_cap, _ = CASES[CAUGHT_BY[mutant]]
    logits = _logits_for(maps, n_cap + 1)
    good, bad = ref.reference_clip(maps, n_cap, logits=logits), ref.reference_clip(maps, n_cap, logits=logits, mutant=mutant)
    differs = _fields(good) != _fields(bad) or not np.array_equal(good['masks'], bad['masks']) or not _same_bits(good['logits'], bad['logits'])
    assert differs, mutant
    assert set(CAUGHT_BY) == set(ref.MUTANTS)


def _random_clip(rng):
    N = int(rng.randint(1, 9))
    maps = []
    for _ in range(N):
        ids = rng.choice(ID_POOL, size=int(rng.randint(1, 5)), replace=False)
        maps.append(ids[rng.randint(0, len(ids), size=(6, 7))].astype(np.uint8))
    return maps, int(rng.randint(1, 5))


def test_appearance_plan_equals_the_restatement_in_every_field():
    from rmnet_amd import clip_io, object_plan
    rng = np.random.RandomState(29)
    clips = [(m, c) for m, c, _ in CASES.values()] + [_random_clip(rng) for _ in range(300)]
    fresh_frames = 0
    for maps, n_cap in clips:
        want = ref.reference_clip(maps, n_cap)
        if want['n_max'] < 0:
            continue                                    # nothing but the ignored id: segment_video_u8 refuses such a clip
        words = ref.presence_words(maps)
        plan = object_plan.appearance_plan(torch.from_numpy(words.view(np.int32)), n_cap)
        assert _plan_fields(plan) == _fields(want)
        assert plan.K == n_cap + 1 and plan.action.dtype == torch.uint8 and tuple(plan.action.shape) == (len(maps), n_cap + 1)
        assert plan.lut.tolist() == want['lut'].tolist() and plan.ids_dev.tolist() == [int(i) for i in want['ids']]
        fresh_frames += len(want['fresh'])
    assert fresh_frames > 100                           # (the random clips do gain objects)
    # the table is clip_io.reorganize_lut's
    maps, n_cap = clips[-1]
    lut, n_ids = clip_io.reorganize_lut(torch.from_numpy(np.stack(maps)))
    plan = object_plan.appearance_plan(ref.presence_words(maps).view(np.int32), n_cap)
    assert lut.tolist() == plan.lut.tolist() and int(n_ids) == len(plan.ids)


# ================================================================================================ CPU: the torch routes
def test_the_torch_route_of_label_presence_returns_the_same_words():
    from rmnet_amd import object_plan
    rng = np.random.RandomState(3)
    every = np.arange(256, dtype=np.uint8)[rng.permutation(256)].reshape(1, 16, 16)
    clips = [every, np.full((2, 3, 5), 31, np.uint8), rng.randint(0, 256, size=(4, 9, 11)).astype(np.uint8),
             np.asarray(ID_POOL, np.uint8)[rng.randint(0, len(ID_POOL), size=(5, 6, 7))]]
    for maps in clips:
        want = ref.presence_words(maps)
        for t in (torch.from_numpy(maps), torch.from_numpy(maps).to(torch.int64), torch.from_numpy(maps).transpose(1, 2)):
            got = object_plan.label_presence(t)
            assert got.dtype == torch.int32 and np.array_equal(got.numpy().view(np.uint32), want)
        assert object_plan.presence_sets(torch.from_numpy(want.view(np.int32))) == [sorted(set(m.ravel().tolist())) for m in maps]
    for v in (0, 31, 32, 63, 64, 255):
        got = object_plan.label_presence(torch.full((1, 2, 2), v, dtype=torch.uint8)).numpy().view(np.uint32)
        want = np.zeros((1, 8), np.uint32)
        want[0, v >> 5] = np.uint32(1) << np.uint32(v & 31)
        assert np.array_equal(got, want)


def _edit_cases(rng, B, K, H, W):
    """(name, logit [B,K,H,W], labels [B,H,W] or None, lut [B,256], action [B,K]) for the action sets of the edit kernel."""
    lut = np.zeros((B, 256), np.uint8)
    labels = np.zeros((B, H, W), np.uint8)
    n_ids = min(K + 3, 255)
    for b in range(B):
        ids = np.sort(rng.choice(np.arange(255), size=n_ids, replace=False))      # more ids than planes: some remap to >= K
        lut[b, ids] = np.arange(n_ids)
        labels[b] = ids[rng.randint(0, n_ids, size=(H, W))]
    logit = lambda: (rng.rand(B, K, H, W) * 31.9 - 16.0).astype(np.float32)
    keep, absent = np.zeros((B, K), np.uint8), np.ones((B, K), np.uint8)
    inject0 = keep.copy()
    inject0[:, 0] = 2
    mixed = rng.randint(0, 3, size=(B, K)).astype(np.uint8)
    mixed[0, K - 1] = 2                                   # (the last plane injected next to ids beyond it)
    no_labels = rng.randint(0, 2, size=(B, K)).astype(np.uint8)
    return [('all_keep', logit(), labels, lut, keep), ('all_absent', logit(), labels, lut, absent), ('inject_0', logit(), labels, lut, inject0),
            ('mixed', logit(), labels, lut, mixed), ('no_labels', logit(), None, lut, no_labels)]


def _check_edit(name, logit_in, labels, lut, action, logit_out, prob):
    """The contract of the edit on numpy arrays: logit bits, the literals, kept channels, the probabilities' bound."""
    B, K = action.shape
    for b in range(B):
        want = ref.edit_frame(logit_in[b], None if labels is None else labels[b], lut[b], action[b])
        assert float(ref.spread(want).max()) <= ref.D_MAX               # E is known on [-34, 0] only
        assert _same_bits(logit_out[b], want), (name, b)
        for k in range(K):
            if action[b, k] == 0:
                assert _same_bits(logit_out[b, k], logit_in[b, k]), (name, b, k)
            elif action[b, k] == 1:
                assert (np.ascontiguousarray(logit_out[b, k]).view(np.uint32) == ABSENT.view(np.uint32)).all()
            else:
                m = np.zeros(logit_in.shape[2:], bool) if labels is None else lut[b][labels[b]] == k
                assert _same_bits(logit_out[b, k], np.where(m, INJECT_HI, ABSENT))
        p64, bound = ref.softmax_bound(want)
        err = np.abs(prob[b].astype(np.float64) - p64)
        assert (err <= bound).all(), (name, b, float((err / bound).max()))
        if name == 'all_absent':                          # d = 0, expf(0) = 1, the sum is K exactly: the correctly rounded 1 / K
            assert (np.ascontiguousarray(prob[b]).view(np.uint32) == (np.float32(1.0) / np.float32(K)).view(np.uint32)).all(), (name, K)


@pytest.mark.parametrize('K', [1, 2, 3, 11, 255])
def test_the_torch_route_of_the_edit_gives_the_restatements_bits_and_bounded_probabilities(K):
    from rmnet_amd import object_plan
    assert np.exp(np.float32(0.0)) == np.float32(1.0)
    rng = np.random.RandomState(100 + K)
    for name, logit, labels, lut, action in _edit_cases(rng, 2, K, 5, 7):
        t_logit = torch.from_numpy(logit.copy())
        prob = torch.full((2, K, 5, 7), 7.0)
        out = object_plan.object_edit_softmax(t_logit, None if labels is None else torch.from_numpy(labels), torch.from_numpy(lut),
                                              torch.from_numpy(action), prob)
        assert out is prob
        _check_edit(name, logit, labels, lut, action, t_logit.numpy(), prob.numpy())


def test_whole_clip_edits_of_the_torch_route_equal_the_literal_writes():
    """Frame by frame with the plan's actions and the raw label maps, the edit gives the logits that the reference's index writes on
    one-hot masks give -- on every hand-written clip."""
    from rmnet_amd import object_plan
    for name, (maps, n_cap, _) in CASES.items():
        logits = _logits_for(maps, n_cap + 1, seed=5)
        want = ref.reference_clip(maps, n_cap, logits=logits)['logits']
        plan = object_plan.appearance_plan(ref.presence_words(maps).view(np.int32), n_cap)
        got = torch.from_numpy(logits.copy())
        for t in sorted(plan.edited):
            object_plan.object_edit_softmax(got[t:t + 1], torch.from_numpy(maps[t])[None], plan.lut[None], plan.action[t:t + 1],
                                            torch.empty_like(got[t:t + 1]))
        assert _same_bits(got.numpy(), want), name


# ================================================================================================ CPU: argument rules
def test_argument_rules_of_the_two_entries_need_no_gpu():
    """Every refusal of the C entries comes before the first call into the runtime, so made-up addresses do for pointers."""
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    p, odd = 0x10000, 0x10002
    assert lib.rmnet_label_presence_chunk_bytes() > 0 and lib.rmnet_label_presence_chunk_bytes() % 16 == 0
    assert lib.rmnet_label_presence_u8(None, 1, 2, 2, p, None) == INVALID
    assert lib.rmnet_label_presence_u8(p, 1, 2, 2, None, None) == INVALID
    for n, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        assert lib.rmnet_label_presence_u8(p, n, h, w, p, None) == INVALID
    assert lib.rmnet_label_presence_u8(p, 1, 2, 2, odd, None) == INVALID
    assert lib.rmnet_label_presence_u8(p, 2, 1 << 15, 1 << 15, p, None) == UNSUPPORTED

    def edit(logit=p, lbs=8, labels=p, labs=4, lut=p, action=p, prob=p, pbs=8, B=1, K=2, H=2, W=2):
        return lib.rmnet_object_edit_softmax_f32(logit, lbs, labels, labs, lut, action, prob, pbs, B, K, H, W, None)

    for missing in ('logit', 'lut', 'action', 'prob'):
        assert edit(**{missing: None}) == INVALID
    for bad in (dict(K=0), dict(K=256, lbs=1024, pbs=1024), dict(B=0), dict(H=0), dict(W=-1), dict(logit=odd), dict(prob=odd),
                dict(lbs=7), dict(pbs=7), dict(labs=3)):
        assert edit(**bad) == INVALID, bad
    big = 1 << 31
    for unsupported in (dict(lbs=big), dict(pbs=big), dict(labs=big), dict(B=65536),
                        dict(H=1 << 15, W=1 << 15, lbs=big << 2, pbs=big << 2, labs=big), dict(B=3, lbs=big - 8, pbs=8)):
        assert edit(**unsupported) == UNSUPPORTED, unsupported
    # the bindings: shapes and dtypes before anything else, then CUDA tensors only
    z = torch.zeros
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.label_presence(z(1, 2, 2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r'\[N, H, W\]'):
        ops.label_presence(z(2, 2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='1 <= K <= 255'):
        ops.object_edit_softmax(z(1, 256, 1, 1), None, z(1, 256, dtype=torch.uint8), z(1, 256, dtype=torch.uint8), z(1, 256, 1, 1))
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.object_edit_softmax(z(1, 2, 2, 2), None, z(1, 256, dtype=torch.uint8), z(1, 2, dtype=torch.uint8), z(1, 2, 2, 2))
    with pytest.raises(RuntimeError, match='prob must be'):
        ops.object_edit_softmax(z(1, 2, 2, 2), None, z(1, 256, dtype=torch.uint8), z(1, 2, dtype=torch.uint8), z(1, 3, 2, 2))


def test_segment_video_u8_refuses_new_objects_with_scales_or_flip_and_single_label_maps():
    from rmnet_amd import inference
    u8 = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    labels = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for kw in (dict(frame_scales=(0.75, 1.0)), dict(flip_lr=True)):
        with pytest.raises(RuntimeError, match='frame_scales / flip_lr'):
            inference.segment_video_u8(None, None, u8, labels, 2, clip_io_ref.MEAN, clip_io_ref.STD, new_objects=True, **kw)
    with pytest.raises(RuntimeError, match=r'\[N, H, W\]'):
        inference.segment_video_u8(None, None, u8, labels[0], 2, clip_io_ref.MEAN, clip_io_ref.STD, new_objects=True)


def test_restore_ids_round_trip():
    from rmnet_amd import clip_io, object_plan
    rng = np.random.RandomState(8)
    raw = np.asarray([0, 5, 38, 200], np.uint8)[rng.randint(0, 4, size=(3, 6, 7))]
    plan = object_plan.appearance_plan(ref.presence_words(raw).view(np.int32), 4)
    planes = plan.lut[torch.from_numpy(raw).to(torch.int64)]
    assert torch.equal(clip_io.restore_ids(planes, plan.ids), torch.from_numpy(raw))
    assert clip_io.restore_ids(torch.tensor([4, 200]), plan.ids).tolist() == [0, 0]      # a plane without an id of the clip


# ================================================================================================ GPU: the presence kernel
def _guarded_u8(n_bytes, offset, fill=0xA5):
    """(buffer, view of n_bytes that starts ``offset`` bytes past a 16-byte boundary, with at least 32 guard bytes on either side)."""
    buf = torch.full((32 + 16 + n_bytes + 32,), fill, dtype=torch.uint8, device=dev())
    start = 32 + ((-(buf.data_ptr() + 32)) % 16) + offset
    return buf, buf[start:start + n_bytes]


def _presence_of(maps, offset):
    """The kernel's words for uint8 [N,H,W] placed at a byte offset inside a guarded buffer; asserts that the buffer is unchanged."""
    from rmnet_amd import ops
    N, H, W = maps.shape
    buf, view = _guarded_u8(maps.size, offset)
    view.copy_(torch.from_numpy(maps.reshape(-1)).to(dev()))
    t = view.view(N, H, W)
    assert t.data_ptr() % 16 == offset
    before = buf.clone()
    got = ops.label_presence(t)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                       # read-only: guards and payload unchanged
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, 8)
    return got.cpu().numpy().view(np.uint32)


@gpu
def test_presence_kernel_every_word_over_plane_sizes_and_byte_offsets():
    from rmnet_amd import ops
    chunk = ops.label_presence_chunk_bytes()
    rng = np.random.RandomState(1)
    for hw in (1, 15, 16, 17, 63, 64, 65):
        for offset in range(16):
            maps = np.asarray(ID_POOL, np.uint8)[rng.randint(0, len(ID_POOL), size=(3, 1, hw))]
            assert np.array_equal(_presence_of(maps, offset), ref.presence_words(maps)), (hw, offset)
    hw = 4 * chunk + 5                                    # five workgroups per frame, the last one nearly empty, a tail of 5 bytes
    for offset in (0, 1, 11, 15):
        maps = np.asarray([0, 5, 9], np.uint8)[rng.randint(0, 3, size=(2, 1, hw))]
        maps[0, 0, hw - 1] = 63                           # only in the last byte
        maps[1, 0, 0] = 64                                # only in the first byte
        maps[1, 0, 3 * chunk + 100] = 254                 # only in the fourth workgroup
        assert np.array_equal(_presence_of(maps, offset), ref.presence_words(maps)), offset
    for offset in (0, 7):                                 # 17 x 29: a plane shape that is no multiple of anything
        maps = rng.randint(0, 256, size=(2, 17, 29)).astype(np.uint8)
        assert np.array_equal(_presence_of(maps, offset), ref.presence_words(maps))


@gpu
def test_presence_kernel_keeps_neighbouring_frames_apart():
    """A value in the last byte of frame n only, and a value in the first byte of frame n + 1 only, for N = 1 .. 3, at plane sizes
    and offsets that put the frame boundary inside a 16-byte vector."""
    for N in (1, 2, 3):
        for hw in (17, 65, 256):
            for offset in (0, 3, 15):
                for n in range(N):
                    maps = np.full((N, 1, hw), 5, np.uint8)
                    maps[n, 0, hw - 1] = 200
                    if n + 1 < N:
                        maps[n + 1, 0, 0] = 32
                    got = _presence_of(maps, offset)
                    assert np.array_equal(got, ref.presence_words(maps)), (N, hw, offset, n)
                    assert [bool(got[i, 200 >> 5] >> (200 & 31) & 1) for i in range(N)] == [i == n for i in range(N)]
                    assert [bool(got[i, 32 >> 5] >> (32 & 31) & 1) for i in range(N)] == [i == n + 1 for i in range(N)]


@gpu
def test_presence_kernel_all_values_single_values_and_a_graph_replay():
    from rmnet_amd import ops
    rng = np.random.RandomState(2)
    every = np.arange(256, dtype=np.uint8)[rng.permutation(256)].reshape(1, 16, 16)
    assert (_presence_of(every, 5) == np.uint32(0xffffffff)).all()
    for v in (0, 31, 32, 63, 64, 255):
        want = np.zeros((1, 8), np.uint32)
        want[0, v >> 5] = np.uint32(1) << np.uint32(v & 31)
        assert np.array_equal(_presence_of(np.full((1, 7, 11), v, np.uint8), 9), want), v
    # one capture, replayed on other label maps: the entry zeroes its output inside the graph
    first = rng.randint(0, 256, size=(2, 9, 31)).astype(np.uint8)
    second = np.asarray([3, 64], np.uint8)[rng.randint(0, 2, size=(2, 9, 31))]
    labels = torch.from_numpy(first).to(dev())
    stream = torch.cuda.Stream(dev())
    stream.wait_stream(torch.cuda.current_stream(dev()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        ops.label_presence(labels)
        with torch.cuda.graph(graph, stream=stream):
            out = ops.label_presence(labels)
        labels.copy_(torch.from_numpy(second).to(dev()))
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(dev()).wait_stream(stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.presence_words(second))


# ================================================================================================ GPU: the edit kernel
SENTINEL = 12345.0


def _run_edit_on_gpu(logit, labels, lut, action):
    """The kernel on slices [:, 1] of guarded [B,3,...] buffers; returns (edited logits, probabilities) and asserts that nothing
    outside the slices changed."""
    from rmnet_amd import ops
    B, K, H, W = logit.shape
    d = dev()
    lbuf = torch.full((B, 3, K, H, W), SENTINEL, device=d)
    pbuf = torch.full((B, 3, K, H, W), SENTINEL, device=d)
    lbuf[:, 1] = torch.from_numpy(logit).to(d)
    ubuf = None
    if labels is not None:
        ubuf = torch.full((B, 3, H, W), 77, dtype=torch.uint8, device=d)
        ubuf[:, 1] = torch.from_numpy(labels).to(d)
    out = ops.object_edit_softmax(lbuf[:, 1], None if ubuf is None else ubuf[:, 1], torch.from_numpy(lut).to(d), torch.from_numpy(action).to(d),
                                  pbuf[:, 1])
    torch.cuda.synchronize()
    assert out.data_ptr() == pbuf[:, 1].data_ptr()
    for buf in (lbuf, pbuf):
        assert bool((buf[:, 0] == SENTINEL).all()) and bool((buf[:, 2] == SENTINEL).all())
    if ubuf is not None:
        assert bool((ubuf[:, 0] == 77).all()) and bool((ubuf[:, 2] == 77).all()) and torch.equal(ubuf[:, 1].cpu(), torch.from_numpy(labels))
    return lbuf[:, 1].cpu().numpy(), pbuf[:, 1].cpu().numpy()


@gpu
@pytest.mark.parametrize('K', [1, 2, 3, 11, 12, 255])
def test_edit_kernel_logit_bits_and_bounded_probabilities(K):
    """Plane sizes around the 4-pixel lanes (1, 3, 4, 5), around a wave (63 .. 65) and beyond one workgroup of one-pixel lanes (260),
    B = 2 with two tables and two action rows, every action set.  All-absent gives p = fl(1 / K) exactly: the differences are 0,
    expf(0) = 1 and the sum is the integer K -- expf(0) itself cannot be seen through a quotient, so the device library's exp of 0
    is also looked at directly."""
    assert float(torch.exp(torch.zeros(1, device=dev()))[0]) == 1.0
    rng = np.random.RandomState(200 + K)
    for hw in (1, 3, 4, 5, 63, 64, 65, 260):
        H, W = (1, hw) if hw != 260 else (13, 20)
        for name, logit, labels, lut, action in _edit_cases(rng, 2, K, H, W):
            got_logit, got_prob = _run_edit_on_gpu(logit, labels, lut, action)
            _check_edit(name, logit, labels, lut, action, got_logit, got_prob)


@gpu
def test_edit_kernel_graph_replay():
    from rmnet_amd import ops
    rng = np.random.RandomState(9)
    d = dev()
    cases = _edit_cases(rng, 2, 3, 6, 10)
    _, logit_a, labels, lut, action_a = cases[3]
    _, logit_b, _, _, action_b = cases[2]
    t_logit, t_action = torch.from_numpy(logit_a).to(d), torch.from_numpy(action_a).to(d)
    t_labels, t_lut, t_prob = torch.from_numpy(labels).to(d), torch.from_numpy(lut).to(d), torch.empty(2, 3, 6, 10, device=d)
    stream = torch.cuda.Stream(d)
    stream.wait_stream(torch.cuda.current_stream(d))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        ops.object_edit_softmax(t_logit, t_labels, t_lut, t_action, t_prob)
        with torch.cuda.graph(graph, stream=stream):
            ops.object_edit_softmax(t_logit, t_labels, t_lut, t_action, t_prob)
        t_logit.copy_(torch.from_numpy(logit_b).to(d))
        t_action.copy_(torch.from_numpy(action_b).to(d))
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(d).wait_stream(stream)
    _check_edit('replay', logit_b, labels, lut, action_b, t_logit.cpu().numpy(), t_prob.cpu().numpy())


# ================================================================================================ GPU: a whole clip
class _Recorder:
    """Stands where the network stands in segment_video_u8 and keeps what went in and what came out."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, frames, masks, flows, n_objects, memorize_every, **kw):
        est = self.net(frames, masks, flows, n_objects, memorize_every, **kw)
        self.calls.append({'frames': frames, 'masks': masks, 'flows': flows, 'n_objects': n_objects, 'kw': kw, 'est': est})
        return est


@pytest.fixture(scope='module')
def late_clip(oracle_mod):
    """The late-object clip of tests/test_gpu_parity.py (5 frames, 96 x 160, object 2 from frame 2) as a folder of images would hold
    it -- uint8 frames, label maps with the ids 0, 5, 38 -- and the oracle's CPU path on it, computed once: fed with the one-hot
    masks and per-frame counts that the restatement builds from the label maps."""
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    N, H, W = 5, 96, 160
    frames, masks, flows, _ = synthetic_clip(N, 3, H, W, seed=11, size=1.3)
    planes = masks[0].argmax(dim=1).numpy()
    planes[:2][planes[:2] == 2] = 0                       # object 2 is background in frames 0 and 1
    labels = np.asarray([0, 5, 38], np.uint8)[planes]
    mean, std = torch.tensor(clip_io_ref.MEAN).view(1, 3, 1, 1), torch.tensor(clip_io_ref.STD).view(1, 3, 1, 1)
    u8 = ((frames[0] * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    r = ref.reference_clip(list(labels), 2)
    assert r['n_objects'] == [1, 1, 2, 2, 2] and r['action'].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 0], [0, 0, 0]]
    prod = networks.procedural_init_(RMNet(None))
    oracle_net = oracle_mod.OracleRMNet()
    oracle_net.load_state_dict(prod.state_dict())
    f32 = torch.from_numpy(clip_io_ref.normalize(u8.numpy())).unsqueeze(0)           # the bits the driver's normalisation gives
    masks_all = torch.from_numpy(r['masks']).unsqueeze(0)
    counts = torch.tensor([r['n_objects']], dtype=torch.long)
    with torch.no_grad():
        est_cpu = oracle_net.eval()(f32, masks_all, flows, counts, 2)
    return dict(u8=u8, labels=torch.from_numpy(labels), flows=flows, f32=f32, masks_all=masks_all, counts=counts, est_cpu=est_cpu,
                state=prod.state_dict(), ref=r)


def _reproducible():
    """The library's convolutions with reproducible solvers (tests/test_clip_io.py): two runs of one clip then agree in every bit."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


@gpu
@pytest.mark.parametrize('fused', [False, True])
def test_late_object_clip_through_segment_video_u8(fused, late_clip):
    from rmnet_amd import clip_io, inference
    from rmnet_amd.rmnet import RMNet
    c = late_clip
    d = dev()
    net = RMNet(None)
    net.load_state_dict(c['state'])
    net = net.to(d).eval()
    if fused:
        net.fuse_epilogues()
    rec = _Recorder(net)
    flownet = lambda clip: c['flows'].to(d)
    with _reproducible(), torch.no_grad():
        out = inference.segment_video_u8(rec, flownet, c['u8'], c['labels'], 2, clip_io_ref.MEAN, clip_io_ref.STD, memorize_every=2,
                                         new_objects=True)
        call = rec.calls[0]
        est = call['est'][0].cpu()
        # the route that exists without the plan, on the same inputs: one-hot masks of all frames, per-frame counts
        plain, plain_logits = net(call['frames'], c['masks_all'], call['flows'], c['counts'], 2, device=d, return_logits=True)
        planned, planned_logits = net(call['frames'], c['masks_all'][:, :1], call['flows'], None, 2, device=d, return_logits=True,
                                      object_plan=call['kw']['object_plan'])
        old = inference.segment_video_u8(net, flownet, c['u8'], c['labels'], 2, clip_io_ref.MEAN, clip_io_ref.STD, memorize_every=2)
    assert tuple(call['masks'].shape) == (1, 1, 3, 96, 160) and call['n_objects'] is None         # frame 0 only, counts from the plan
    assert torch.equal(call['frames'].cpu(), c['f32'])
    assert out['n_objects'] == 2 and out['n_objects_per_frame'] == [1, 1, 2, 2, 2] and out['ids'].tolist() == [0, 5, 38]
    # against the oracle's CPU path: the bars of test_rmnet_new_object_and_batch_of_clips
    est_cpu = c['est_cpu'][0]
    print('max |dp| vs the CPU path %.3e' % float((est - est_cpu).abs().max()))
    assert float((est - est_cpu).abs().max()) < 1e-3
    agree = float((est.argmax(1) == est_cpu.argmax(1)).float().mean())
    print('label agreement %.5f' % agree)
    assert agree > 0.999
    assert torch.equal(out['labels'].cpu(), est.argmax(1).to(torch.uint8))
    # object 2: numerically nothing before it appears, pixels from then on
    assert float(est[1, 2].max()) < 1e-6
    pixels = [int((out['labels'][t] == 2).sum()) for t in range(5)]
    print('pixels of object 2 per frame', pixels)
    assert pixels[0] == 0 and pixels[1] == 0 and all(p > 0 for p in pixels[2:])
    # against forward without a plan: frame 0 is the same bits, the first edited frame (1) has the same logits and probabilities
    # inside the derived bound of their float64 soft-max, later frames the 1e-3 bar.  (Equal bits are not asked of later frames: two
    # runs of ONE route already differ in the last frame of this clip, by up to 4e-4 in the logits, whichever route it is.)
    plain, plain_logits, planned = plain[0].cpu(), plain_logits[0].cpu().numpy(), planned[0].cpu()
    first = min(c['ref']['edited'])
    assert torch.equal(planned[:first], plain[:first]) and torch.equal(est[:first], plain[:first])
    print('planned run against the driver\'s run, max |dp| %.3e' % float((planned - est).abs().max()))
    assert float((planned - est).abs().max()) < 1e-3
    assert first == 1 and _same_bits(planned_logits[0, first].cpu().numpy(), plain_logits[first])
    assert float(ref.spread(plain_logits[first]).max()) <= ref.D_MAX
    p64, bound = ref.softmax_bound(plain_logits[first])
    err = np.abs(planned[first].numpy().astype(np.float64) - p64)
    print('first edited frame: largest error / bound %.3f' % float((err / bound).max()))
    assert (err <= bound).all()
    assert float((planned[first + 1:] - plain[first + 1:]).abs().max()) < 1e-3
    # the gap this closes: without new_objects, object 2 is counted from frame 0, never exists and never gets a pixel
    assert int((old['labels'] == 2).sum()) == 0 and old['n_objects'] == 2
    # label maps in the clip's own ids
    restored = clip_io.restore_ids(out['labels'], out['ids'])
    assert set(restored.unique().tolist()) <= {0, 5, 38} and torch.equal(restored == 38, out['labels'] == 2)
    assert torch.equal(c['labels'][0], restored[0].cpu())             # frame 0 is the annotation itself
