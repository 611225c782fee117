# -*- coding: utf-8 -*-
"""The validation loss (Lovasz-softmax + NLL, core/test.py:97) without a sort: the numpy restatement of tests/val_loss_ref.py
pinned by hand, by the float64 sort and by the reference's recorded values; rmnet_amd.losses and inference.test_videos on the
CPU; and csrc/val_loss.hip on the GPU, every histogram count against the restatement.  The bounds are derived in val_loss_ref.py."""

import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch

import boundary_ref as br
import val_loss_ref as ref
from conftest import GOLDEN

INF = float('inf')


def f32(a):
    return np.asarray(a, np.float32)


def clip_of(pixels, K, N=1):
    """pixels: [(label, (p_0 .. p_{K-1})), ...] -> probs [N,K,1,n/N], labels [N,1,n/N]."""
    labels = np.asarray([p[0] for p in pixels], np.uint8).reshape(N, 1, -1)
    probs = f32([p[1] for p in pixels]).reshape(N, -1, K).transpose(0, 2, 1)[:, :, None, :]
    return np.ascontiguousarray(probs), labels


# name -> (probs, labels, bins, expected): every figure below is worked out by hand (tests/val_loss_ref.py has the formulas)
def hand_cases():
    L = math.log
    c = {}
    # one pixel (the reference's p > 1 branch is not taken): class 1 has G = 1, e = 0.25, J_1 = 1: value 0.25; key 4 of 16
    c['one_pixel'] = (*clip_of([(1, (0.25, 0.75))], 2), 16,
                      dict(G=[0, 1], lo=[0, 0.25], hi=[0, 5 / 16], sort=[0, 0.25], lovasz=(0.25 + 5 / 16) / 2, nll=-L(0.75), counts=[1, 0, 0]))
    c['one_pixel_2bins'] = (*clip_of([(1, (0.25, 0.75))], 2), 2,
                            dict(G=[0, 1], lo=[0, 0.0], hi=[0, 0.5], sort=[0, 0.25], lovasz=0.25, nll=-L(0.75), counts=[1, 0, 0]))
    c['all_ignored'] = (*clip_of([(255, (0.25, 0.75)), (255, (0.5, 0.5))], 2), 16,
                        dict(G=[0, 0], lo=[0, 0], hi=[0, 0], sort=[0, 0], lovasz=0.0, nll=float('nan'), counts=[0, 0, 0]))
    # class 2 absent.  class 0: errors 0.5 (fg), 0.25 (bg): J = 1, 1: 0.5.  class 1: errors 0.25 (bg), 0.25 (fg), a tie: 0.25
    # either way.  bins 16, class 0: keys 8 (fg), 4 (bg); hi = (9 terms of 1) / 16, lo = 8 / 16.  class 1: keys 4, 4: for
    # k <= 4, Fge = Bge = 1: 1 - 0 / 2 = 1, 5 terms: hi = 5 / 16; Fgt = Bgt = 1 for k < 4: lo = 4 / 16
    c['absent_class'] = (*clip_of([(0, (0.5, 0.25, 0.25)), (1, (0.25, 0.75, 0.0))], 3), 16,
                         dict(G=[1, 1, 0], lo=[0.5, 0.25, 0], hi=[9 / 16, 5 / 16, 0], sort=[0.5, 0.25, 0],
                              lovasz=((0.5 + 9 / 16) / 2 + (0.25 + 5 / 16) / 2) / 2, nll=(-L(0.5) - L(0.75)) / 2, counts=[2, 0, 0]))
    # one class present, two frames of one pixel: errors 0.5, 0.25, both fg, G = 2: J = 0.5, 1: 0.5 * 0.5 + 0.25 * 0.5 = 0.375
    # bins 16: keys 8, 4.  Fge = 2 for k <= 4 (5 terms of 1), 1 for k = 5 .. 8 (4 terms of 0.5): hi = 7 / 16.  Fgt = 2 for k < 4,
    # 1 for k = 4 .. 7: lo = 6 / 16.   bins 2: keys 1, 0.  hi = (1 + 0.5) / 2, lo = (0.5 + 0) / 2
    single = [(0, (0.5, 0.5)), (0, (0.75, 0.25))]
    c['single_class'] = (*clip_of(single, 2, N=2), 16,
                         dict(G=[2, 0], lo=[0.375, 0], hi=[7 / 16, 0], sort=[0.375, 0], lovasz=(0.375 + 7 / 16) / 2,
                              nll=(-L(0.5) - L(0.75)) / 2, counts=[2, 0, 0]))
    c['single_class_2bins'] = (*clip_of(single, 2, N=2), 2,
                               dict(G=[2, 0], lo=[0.25, 0], hi=[0.75, 0], sort=[0.375, 0], lovasz=0.5, nll=(-L(0.5) - L(0.75)) / 2,
                                    counts=[2, 0, 0]))
    # e == 1: the target class has probability 0.  class 0: G = 1, e = 1, key 16: Fge = Fgt = 1 for every k < 16: lo = hi = 1.
    # class 1: G = 0
    c['top_bin'] = (*clip_of([(0, (0.0, 1.0))], 2), 16,
                    dict(G=[1, 0], lo=[1.0, 0], hi=[1.0, 0], sort=[1.0, 0], lovasz=1.0, nll=INF, counts=[1, 0, 0]))
    # an ignored pixel next to the one pixel of 'one_pixel'
    c['ignored_pixel'] = (*clip_of([(1, (0.25, 0.75)), (255, (0.5, 0.5))], 2), 16, c['one_pixel'][3])
    # bad pixels next to it: a label >= K, a probability above 1, a NaN, a negative one, and a bad label with a bad probability
    c['bad_pixels'] = (*clip_of([(1, (0.25, 0.75)), (2, (0.5, 0.5)), (0, (1.5, 0.25)), (1, (float('nan'), 0.5)), (0, (0.5, -0.1)),
                                 (7, (2.0, 0.0)), (255, (float('nan'), 3.0))], 2), 16,
                       dict(c['one_pixel'][3], counts=[1, 2, 3]))
    return c


HAND = hand_cases()
# the planted fault -> the hand case that catches it
CAUGHT_BY = {'ge_for_gt': 'single_class', 'clamp_top': 'top_bin', 'count_ignored': 'ignored_pixel', 'mean_over_all': 'absent_class',
             'fg_shifted': 'one_pixel', 'keep_bad': 'bad_pixels', 'drop_frame0': 'single_class'}


def same(a, b, tol=ref.EPS):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((np.abs(a - b) <= tol) | (a == b) | (np.isnan(a) & np.isnan(b))))


def hand_ok(name, faults=()):
    probs, labels, bins, want = HAND[name]
    got = ref.clip_loss(probs, labels, 255, bins, faults)
    sv = ref.sorted_values(probs, labels, 255, faults)
    return (same(got['per_class'][:, 0], want['G'], 0) and same(got['per_class'][:, 1], want['lo']) and same(got['per_class'][:, 2], want['hi'])
            and same(sv[:, 1], want['sort']) and same(got['lovasz'], want['lovasz']) and same(got['nll'], want['nll'])
            and got['counts'].tolist() == want['counts'])


@pytest.mark.parametrize('name', sorted(HAND))
def test_restatement_gives_the_hand_written_answers(name):
    assert hand_ok(name)


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_every_planted_fault_is_caught_by_its_case(fault):
    assert set(CAUGHT_BY) == set(ref.FAULTS)
    assert hand_ok(CAUGHT_BY[fault]) and not hand_ok(CAUGHT_BY[fault], (fault,))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('name', sorted(HAND))
def test_losses_on_cpu_tensors_give_the_hand_written_answers(name):
    from rmnet_amd import losses
    probs, labels, bins, want = HAND[name]
    lv = losses.lovasz_softmax(t(probs), t(labels), bins=bins)
    assert lv['present'].tolist() == [g > 0 for g in want['G']]
    assert same(lv['lo'].numpy(), want['sort']) and same(lv['hi'].numpy(), want['sort'])          # the torch route: lo == hi == the sort
    present = [s for s, g in zip(want['sort'], want['G']) if g > 0]
    assert same(float(lv['value']), sum(present) / max(len(present), 1))
    assert same(float(losses.nll(t(probs), t(labels))), want['nll'])
    v = losses.validation_loss(t(probs), t(labels), bins=bins)
    assert set(v) == {'loss', 'lovasz', 'nll', 'n_bad'} and all(x.dim() == 0 for x in v.values())
    assert int(v['n_bad']) == want['counts'][1] + want['counts'][2]
    assert same(float(v['loss']), float(lv['value']) + want['nll'])


def random_cases():
    out = []
    for K in (1, 2, 3, 4):
        for peak, ignore in ((0.0, 0.0), (1.0, 0.2), (6.0, 0.0), (20.0, 0.3)):
            out.append((K, peak, ignore))
    return out


@pytest.mark.parametrize('bins', [2, 16, 1 << 10, 1 << 20])
def test_the_sorted_value_lies_inside_the_bracket(bins):
    """EPS (val_loss_ref.py) = 64 * 2^-53: the roundings of the two scans, of the float64 sort and of the mean."""
    rng = np.random.default_rng(bins)
    cases = random_cases() if bins < (1 << 20) else random_cases()[1::3]
    for K, peak, ignore in cases:
        probs, labels = ref.softmax_clip(rng, 2, K, 5, 7, peak=peak, ignore=ignore)
        got = ref.clip_loss(probs, labels, 255, bins)
        sv = ref.sorted_values(probs, labels)
        assert (got['per_class'][:, 0] == sv[:, 0]).all()
        lo, hi = got['per_class'][:, 1], got['per_class'][:, 2]
        assert (sv[:, 1] >= lo - ref.EPS).all() and (sv[:, 1] <= hi + ref.EPS).all(), (K, peak, ignore)
        assert (hi - lo <= 1.0 / bins + ref.EPS).all() and (hi >= lo).all()
        assert abs(got['lovasz'] - ref.sorted_lovasz(probs, labels)) <= 0.5 / bins + ref.EPS


@pytest.mark.parametrize('bins', [2, 16, 1 << 10, 1 << 20])
def test_lo_is_exact_when_every_probability_is_a_multiple_of_the_bin_width(bins):
    rng = np.random.default_rng(bins + 1)
    for K in (1, 2, 3):
        probs, labels = ref.grid_clip(rng, 2, K, 5, 7, bins)
        assert (probs == 0).any() and (probs == 1).any()
        got = ref.clip_loss(probs, labels, 255, bins)
        sv = ref.sorted_values(probs, labels)
        assert same(got['per_class'][:, 1], sv[:, 1]), (bins, K)
        assert got['hist'][:, :, bins].sum() > 0                      # e == 1 is there, in its own bin


def onehot_clip(rng, N, K, H, W):
    labels = rng.integers(0, K, (N, H, W)).astype(np.uint8)
    probs = (labels[:, None] == np.arange(K)[None, :, None, None]).astype(np.float32)
    return probs, labels


def test_nll_is_exactly_zero_for_sure_targets_and_infinite_for_an_impossible_one():
    from rmnet_amd import losses
    probs, labels = onehot_clip(np.random.default_rng(3), 2, 3, 5, 7)
    got = ref.clip_loss(probs, labels, 255, 16)
    assert got['nll'] == 0.0 and (got['per_class'][:, 1] == 0).all() and (got['per_class'][:, 2] == 1 / 16).all()      # every key is 0
    assert ref.sorted_lovasz(probs, labels) == 0.0 and float(losses.validation_loss(t(probs), t(labels))['loss']) == 0.0
    assert float(losses.nll(t(probs), t(labels))) == 0.0
    probs[1, :, 2, 3] = np.roll(probs[1, :, 2, 3], 1)                  # the target of one pixel gets probability 0
    assert ref.clip_loss(probs, labels, 255, 16)['nll'] == INF
    assert float(losses.nll(t(probs), t(labels))) == INF
    assert float(losses.validation_loss(t(probs), t(labels))['loss']) == INF


def test_the_recorded_values_of_the_reference_sit_inside_the_derived_bounds():
    """tests/golden/val_loss.npz holds what the reference's LovaszLoss and NLLLoss returned (fp32) on a dozen 2x5x7 clips; the
    float64 sort, the restatement at 2^20 bins and losses.* on CPU tensors agree with them within ref_lovasz_bound /
    ref_nll_bound (val_loss_ref.py)."""
    from rmnet_amd import losses
    d = np.load(os.path.join(GOLDEN, 'val_loss.npz'))
    names = [str(n) for n in d['names']]
    assert len(names) == 12
    assert (d['ignored_labels'] == 255).any() and not (d['missing_class_labels'] == 3).any() and d['missing_class_probs'].shape[1] == 4
    bins = 1 << 20
    for n in names:
        probs, labels, lovasz, nll = d[n + '_probs'], d[n + '_labels'], float(d[n + '_lovasz']), float(d[n + '_nll'])
        P = int((labels != 255).sum())
        lb = ref.ref_lovasz_bound(P)
        nb = ref.ref_nll_bound(P, float(np.abs(ref.nll_logs(probs, labels)).mean()))
        got = ref.clip_loss(probs, labels, 255, bins)
        print('%-14s lovasz: ref - sort %.2e (bound %.2e), ref - restated %.2e;  nll: %.2e (bound %.2e)'
              % (n, abs(lovasz - ref.sorted_lovasz(probs, labels)), lb, abs(lovasz - got['lovasz']), abs(nll - got['nll']), nb))
        assert abs(lovasz - ref.sorted_lovasz(probs, labels)) <= lb
        assert abs(lovasz - got['lovasz']) <= lb + 0.5 / bins + ref.EPS
        assert abs(nll - got['nll']) <= nb
        v = losses.validation_loss(t(probs), t(labels), bins=bins)
        assert abs(lovasz - float(v['lovasz'])) <= lb + ref.EPS and abs(nll - float(v['nll'])) <= nb + ref.EPS
        assert abs(lovasz + nll - float(v['loss'])) <= lb + nb + ref.EPS and int(v['n_bad']) == 0


# ------------------------------------------------------------------------------------------------ the driver
VIDEO_SHAPES = [(5, 1, 9, 12), (4, 2, 8, 11), (3, 1, 7, 9), (6, 3, 9, 13), (4, 1, 6, 10)]      # (N, objects, H, W)


def fake_videos():
    rng = np.random.default_rng(17)
    videos = []
    for v, (N, no, H, W) in enumerate(VIDEO_SHAPES):
        labels = np.repeat(np.repeat(rng.integers(0, no + 1, (N, (H + 2) // 3, (W + 2) // 3)), 3, axis=1), 3, axis=2)[:, :H, :W]
        videos.append({'frames': torch.zeros(N, 3, H, W), 'n_objects': no, 'labels': t(labels.astype(np.uint8)), 'id': v})
    return videos


def fake_probs(video):
    """A "network": the ground truth shifted by one pixel, every frame with another confidence."""
    labels = video['labels'].numpy()
    K = int(video['n_objects']) + 1
    shifted = np.roll(labels, 1, axis=2)
    onehot = (shifted[:, None] == np.arange(K)[None, :, None, None]).astype(np.float64)
    conf = (0.5 + 0.4 * (np.arange(labels.shape[0]) % 3) / 2).reshape(-1, 1, 1, 1)
    return t((conf * onehot + (1 - conf) / K).astype(np.float32))


def literal_test_loop(videos):
    """core/test.py:69-141 line by line on numpy arrays: the loss over all frames, the metrics over frames 1 .. N - 1 and objects
    1 .. n_objects, the loss averaged over clips and the metrics weighted by the object count."""
    loss_sum = n_clips = j_sum = f_sum = weight = 0.0
    for video in videos:
        probs, labels, no = fake_probs(video).numpy(), video['labels'].numpy(), int(video['n_objects'])
        r = ref.clip_loss(probs, labels, 255, 2)
        loss_sum += ref.sorted_lovasz(probs, labels) + r['nll']
        n_clips += 1
        pred = probs.argmax(axis=1)
        js, fs = [], []
        for i in range(1, labels.shape[0]):
            for k in range(1, no + 1):
                seg, ann = pred[i] == k, labels[i] == k
                js.append(1.0 if not seg.any() and not ann.any() else (seg & ann).sum() / (seg | ann).sum())
                fs.append(float(br.f_score(seg, ann)))
        j_sum += np.mean(js) * no
        f_sum += np.mean(fs) * no
        weight += no
    j, f = j_sum / weight, f_sum / weight
    return {'Loss': loss_sum / n_clips, 'J-Mean': j, 'F-Mean': f, 'JF-Mean': (j + f) / 2}


def _driver_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from rmnet_amd import inference
    seen = []

    def probs_fn(video):
        seen.append(video['id'])
        return fake_probs(video)
    result = inference.test_videos(fake_videos(), probs_fn)
    q.put((rank, sorted(seen), result))
    dist.destroy_process_group()


def test_the_driver_on_one_rank_follows_the_literal_loop():
    from rmnet_amd import inference
    want = literal_test_loop(fake_videos())
    got = inference.test_videos(fake_videos(), fake_probs, rank=0, world_size=1)
    assert set(got) == {'Loss', 'J-Mean', 'F-Mean', 'JF-Mean'} and all(isinstance(x, float) for x in got.values())
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    assert 0 < got['J-Mean'] < 1 and 0 < got['F-Mean'] < 1 and got['Loss'] > 0
    # the conventions that a slip would change: the DAVIS frames (last frame dropped too), an unweighted mean over clips
    assert abs(got['J-Mean'] - inference.evaluate_videos(fake_videos(), lambda v: fake_probs(v).argmax(dim=1).to(torch.uint8), 0, 1)) > 1e-6
    bad = fake_videos()
    bad[1]['labels'][0, 0, 0] = 9
    with pytest.raises(RuntimeError, match='label >= K'):
        inference.test_videos(bad, fake_probs, rank=0, world_size=1)


def test_the_driver_over_two_gloo_ranks():
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_driver_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    results = {o[0]: o[2] for o in out}
    seen = {o[0]: o[1] for o in out}
    assert sorted(seen[0] + seen[1]) == [0, 1, 2, 3, 4] and seen[0] and seen[1]
    want = literal_test_loop(fake_videos())
    assert results[0] == results[1]
    for k in want:
        assert abs(results[0][k] - want[k]) <= 1e-12, (k, results[0][k], want[k])


# ------------------------------------------------------------------------------------------------ the C entry's argument rules
def test_c_entry_argument_rules():
    from rmnet_amd import _lib
    lib = _lib.load()
    wsb = lib.rmnet_clip_loss_workspace_bytes
    assert wsb(3, 16) == 3 * 2 * 17 * 4 + 512 * 32
    assert wsb(1, 2) == 1 * 2 * 3 * 4 + 512 * 32
    assert wsb(11, 1 << 20) == (11 * 2 * ((1 << 20) + 1) * 4) + 512 * 32
    assert wsb(255, 1 << 22) == (255 * 2 * ((1 << 22) + 1) * 4 + 7) // 8 * 8 + 512 * 32
    for K, bins in ((0, 16), (256, 16), (-1, 16), (3, 0), (3, 1), (3, 3), (3, 24), (3, 1 << 23), (3, -16)):
        assert wsb(K, bins) == 0, (K, bins)
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    big = 1 << 20
    call = lib.rmnet_clip_loss_f32
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    for i in (0, 1, 8, 9, 10):                                     # probs, labels, per_class, nll_sum, counts
        args = [p, p, 2, 3, 5, 7, 255, 16, p, p, p, p, big, None]
        args[i] = None
        assert call(*args) == INVALID, i
    for K in (0, -1, 256):
        assert call(p, p, 2, K, 5, 7, 255, 16, p, p, p, p, big, None) == INVALID
    for bins in (0, 1, 3, 24, 1 << 23, -2):
        assert call(p, p, 2, 3, 5, 7, 255, bins, p, p, p, p, big, None) == INVALID
    for n, h, w in ((0, 5, 7), (2, 0, 7), (2, 5, 0), (-1, 5, 7)):
        assert call(p, p, n, 3, h, w, 255, 16, p, p, p, p, big, None) == INVALID
    assert call(p, p, 2, 3, 1 << 15, 1 << 15, 255, 16, p, p, p, p, big, None) == UNSUPPORTED       # N*H*W = 2^31
    assert call(p, p, 2, 3, 5, 7, 255, 16, p, p, p, None, big, None) == WORKSPACE
    assert call(p, p, 2, 3, 5, 7, 255, 16, p, p, p, p, wsb(3, 16) - 1, None) == WORKSPACE
    for i in (0, 8, 9, 10, 11):                                    # a misaligned probs / per_class / nll_sum / counts / workspace
        args = [p, p, 2, 3, 5, 7, 255, 16, p, p, p, p, big, None]
        args[i] = odd if i else ctypes.c_void_p(p.value + 2)
        assert call(*args) == INVALID, i


def test_ops_clip_loss_rejects_cpu_tensors():
    from rmnet_amd import ops
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.clip_loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the kernels
GUARD_P, GUARD_L = 7.0, 0          # a guard probability is a bad one and a guard label a counted one: a read past an end shows


def device_call(probs, labels, ignore=255, bins=16, off_p=0, off_l=0):
    """ops.clip_loss on copies of the arrays placed ``off_p`` elements / ``off_l`` bytes into guarded, pre-filled buffers."""
    from rmnet_amd import ops
    pb = torch.full((probs.size + 64,), GUARD_P, dtype=torch.float32, device='cuda')
    lb = torch.full((labels.size + 64,), GUARD_L, dtype=torch.uint8, device='cuda')
    at_p, at_l = 16 + off_p, 16 + off_l
    pb[at_p:at_p + probs.size] = t(probs).reshape(-1).cuda()
    lb[at_l:at_l + labels.size] = t(labels).reshape(-1).cuda()
    pv, lv = pb[at_p:at_p + probs.size].view(probs.shape), lb[at_l:at_l + labels.size].view(labels.shape)
    assert pv.data_ptr() % 16 == (4 * off_p) % 16 and lv.data_ptr() % 16 == off_l % 16
    out = ops.clip_loss(pv, lv, ignore, bins, want_hist=True)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert torch.equal(pv.cpu(), t(probs)) or np.isnan(probs).any()
    for buf, n, at, g in ((pb, probs.size, at_p, GUARD_P), (lb, labels.size, at_l, GUARD_L)):
        assert bool((buf[:at] == g).all()) and bool((buf[at + n:] == g).all())
    return got


def check_against_restatement(probs, labels, ignore=255, bins=16, off_p=0, off_l=0, tag=None):
    got = device_call(probs, labels, ignore, bins, off_p, off_l)
    want = ref.clip_loss(probs, labels, ignore, bins)
    tag = (tag, probs.shape, bins, off_p, off_l)
    assert got['hist'].shape == want['hist'].shape and (got['hist'].astype(np.int64) == want['hist']).all(), tag       # every integer
    assert got['counts'].tolist() == want['counts'].tolist(), tag
    assert (got['per_class'][:, 0] == want['per_class'][:, 0]).all(), tag
    eps = ref.eps_device(bins)
    assert (np.abs(got['per_class'][:, 1:] - want['per_class'][:, 1:]) <= eps).all(), (tag, np.abs(got['per_class'] - want['per_class']).max())
    logs = ref.nll_logs(probs, labels, ignore)
    if np.isfinite(logs).all():
        bound = ref.nll_device_bound(logs)
        assert abs(float(got['nll_sum']) - want['nll_sum']) <= bound, (tag, float(got['nll_sum']), want['nll_sum'], bound)
    else:
        assert float(got['nll_sum']) == INF, tag
    return got, want


def spoil(rng, probs, labels, K):
    """Ignored pixels, labels >= K and probabilities outside [0, 1] sprinkled over a clip (in place)."""
    N, _, H, W = probs.shape
    n = max(1, labels.size // 10)
    flat = labels.reshape(-1)
    flat[rng.integers(0, flat.size, n)] = 255
    if K < 255:
        flat[rng.integers(0, flat.size, n)] = rng.integers(K, 255, n)
    for bad in (np.nan, 1.5, -0.1, np.inf, -np.inf, np.float32(1) + np.float32(2.0 ** -23), -1e-30):
        for _ in range(max(1, n // 4)):
            probs[rng.integers(N), rng.integers(K), rng.integers(H), rng.integers(W)] = bad


@pytest.mark.gpu
def test_every_count_matches_at_every_plane_size_and_alignment():
    """Plane sizes 1 .. 65 and 255 .. 257 (with N > 1 the frame boundaries fall inside the 4-pixel groups), N = 1 .. 3, label
    offsets 0 .. 15 and probability offsets 0 .. 3 elements, K = 1, 2, 3, 11, bins 2 and 16 (the whole histogram in LDS at these K)."""
    rng = np.random.default_rng(41)
    for i, hw in enumerate(list(range(1, 66)) + [255, 256, 257]):
        N, K = 1 + i % 3, (1, 2, 3, 11)[(i // 3) % 4]
        H, W = (1, hw) if hw % 5 else (5, hw // 5)
        probs, labels = ref.softmax_clip(rng, N, K, H, W, peak=(0.0, 3.0, 12.0)[i % 3], ignore=0.1)
        if i % 4 == 3:
            spoil(rng, probs, labels, K)
        check_against_restatement(probs, labels, 255, (2, 16)[i % 2], off_p=i % 4, off_l=i % 16, tag=hw)


@pytest.mark.gpu
@pytest.mark.parametrize('K,bins', [(64, 16), (255, 16), (255, 2), (11, 1 << 20), (3, 1 << 20), (1, 1 << 20), (2, 1 << 10)])
def test_every_count_matches_at_every_class_count(K, bins):
    """K = 64 keeps the 17 bins of bins = 16 in LDS, K = 255 only bins 0 .. 7 and 9 .. 16 (bin 8 goes out as global atomics); 2^20
    bins take all three ways out: the aggregated keys 0 and `bins`, the lowest and highest bins in LDS and the global atomics in
    between.  More than one workgroup (P > 2048), odd planes."""
    rng = np.random.default_rng(K + bins)
    N, H, W = (2, 5, 13) if K >= 64 else (3, 37, 21)
    probs, labels = ref.softmax_clip(rng, N, K, H, W, peak=6.0, ignore=0.05)
    check_against_restatement(probs, labels, 255, bins, off_p=1, off_l=3)
    spoil(rng, probs, labels, K)
    got, want = check_against_restatement(probs, labels, 255, bins, off_p=2, off_l=5)
    assert want['counts'][2] > 0 and (K == 255 or want['counts'][1] > 0)
    check_against_restatement(probs, labels, 300, bins)                       # nothing is ignored: label 255 is a bad label or class 254
    probs, labels = ref.grid_clip(rng, N, K, H, W, min(bins, 1 << 20))      # every probability on a bin edge, 0 and 1 included
    got, want = check_against_restatement(probs, labels, 255, bins, off_p=3)
    assert want['hist'][:, :, bins].sum() > 0 and float(got['nll_sum']) == INF


@pytest.mark.gpu
def test_the_aggregated_and_the_atomic_path_each_alone():
    rng = np.random.default_rng(5)
    bins = 1 << 20
    probs, labels = onehot_clip(rng, 2, 3, 37, 21)                            # every key is 0
    got, want = check_against_restatement(probs, labels, 255, bins, off_p=1, off_l=1)
    assert want['hist'][:, :, 0].sum() == want['hist'].sum() == 3 * 2 * 37 * 21
    assert float(got['nll_sum']) == 0.0 and (got['per_class'][:, 1] == 0).all() and (got['per_class'][:, 2] == 1.0 / bins).all()
    P = 6001                                                                  # all keys distinct: e = i / bins, K = 1, all foreground
    probs = (1.0 - np.arange(P) / bins).astype(np.float32).reshape(1, 1, 1, P)
    got, want = check_against_restatement(probs, np.zeros((1, 1, P), np.uint8), 255, bins, off_p=3, off_l=7)
    assert want['hist'].max() == 1 and want['hist'][0, 1, :P].all()
    sv = ref.sorted_values(probs, np.zeros((1, 1, P), np.uint8))
    assert abs(got['per_class'][0, 1] - sv[0, 1]) <= ref.eps_device(bins) + ref.EPS           # multiples of 1 / bins: lo is exact


@pytest.mark.gpu
def test_a_workgroup_that_takes_more_than_one_step():
    """More than 512 x 512 groups of 4 pixels: every workgroup loops, and the last one ends inside its range."""
    rng = np.random.default_rng(6)
    N, K, H, W = 2, 2, 701, 751
    assert N * H * W > 4 * 512 * 512 and (H * W) % 4 == 3
    probs, labels = ref.softmax_clip(rng, N, K, H, W, peak=8.0, ignore=0.02)
    got, want = check_against_restatement(probs, labels, 255, 1 << 20, off_p=1, off_l=2)
    assert abs((got['per_class'][:, 1:].mean()) - ref.sorted_lovasz(probs, labels)) <= 0.5 / (1 << 20) + ref.eps_device(1 << 20) + ref.EPS


@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from rmnet_amd import ops
    rng = np.random.default_rng(8)
    probs, labels = ref.softmax_clip(rng, 3, 3, 37, 53, peak=5.0, ignore=0.1)
    spoil(rng, probs, labels, 3)
    pv, lv = t(probs).cuda(), t(labels).cuda()
    bits = lambda o: [o[k].cpu().numpy().tobytes() for k in ('per_class', 'nll_sum', 'counts', 'hist')]
    eager = bits(ops.clip_loss(pv, lv, bins=1 << 16, want_hist=True))
    assert bits(ops.clip_loss(pv, lv, bins=1 << 16, want_hist=True)) == eager
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.clip_loss(pv, lv, bins=1 << 16, want_hist=True)                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a single stream, no parallel branches
        out = ops.clip_loss(pv, lv, bins=1 << 16, want_hist=True)
    for v in out.values():
        v.fill_(3)                                                            # the replay clears and rewrites everything it returns
    graph.replay()
    torch.cuda.synchronize()
    assert bits(out) == eager


@pytest.mark.gpu
def test_validation_loss_on_the_device_against_the_torch_route():
    """The kernels' midpoint lies within 0.5 / bins of the sort; the torch route is the float64 sort (EPS), its NLL the float64
    log, from which the device's logf may differ by nll_device_bound."""
    from rmnet_amd import losses
    rng = np.random.default_rng(9)
    assert losses.DEVICE_ROUTE in ('hip', 'torch')
    for K, bins in ((3, 1 << 20), (2, 1 << 10), (4, 16)):
        probs, labels = ref.softmax_clip(rng, 3, K, 37, 53, peak=5.0, ignore=0.1)
        pv, lv = t(probs).cuda(), t(labels).cuda()
        a = losses.validation_loss(pv, lv, bins=bins, route='hip')
        b = losses.validation_loss(pv, lv, bins=bins, route='torch')
        assert all(x.is_cuda and x.dim() == 0 for x in list(a.values()) + list(b.values()))
        logs = ref.nll_logs(probs, labels)
        nb = ref.nll_device_bound(logs) / logs.size + ref.EPS
        lv_bound = 0.5 / bins + ref.eps_device(bins) + ref.EPS
        print('K %d bins %d: lovasz %.3e (bound %.3e)  nll %.3e (bound %.3e)' % (K, bins, abs(float(a['lovasz'] - b['lovasz'])), lv_bound,
                                                                            abs(float(a['nll'] - b['nll'])), nb))
        assert abs(float(a['lovasz'] - b['lovasz'])) <= lv_bound and abs(float(a['nll'] - b['nll'])) <= nb
        assert abs(float(a['loss'] - b['loss'])) <= lv_bound + nb and int(a['n_bad']) == int(b['n_bad']) == 0
        assert abs(float(b['lovasz']) - ref.sorted_lovasz(probs, labels)) <= ref.EPS
        lo_hi = losses.lovasz_softmax(pv, lv, bins=bins, route='hip')
        assert bool((lo_hi['hi'] - lo_hi['lo'] <= 1.0 / bins + ref.eps_device(bins)).all()) and lo_hi['present'].all()


@pytest.mark.gpu
def test_the_driver_on_a_real_clip_through_clip_probs():
    from rmnet_amd import inference, networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    N, H, W = 4, 96, 160
    frames, masks, flows, _ = synthetic_clip(N, 3, H, W, seed=11, size=1.3)
    net = networks.procedural_init_(RMNet(None)).cuda().eval()
    video = {'frames': frames[0], 'masks': masks[0], 'n_objects': 2, 'labels': masks[0].argmax(dim=1).to(torch.uint8)}
    probs = inference.clip_probs(net, lambda clip: flows.cuda(), video, memorize_every=2)
    assert tuple(probs.shape) == (N, 3, H, W) and probs.is_cuda and probs.dtype == torch.float32
    hip = inference.test_videos([video], lambda v: probs, rank=0, world_size=1, loss_route='hip')
    tor = inference.test_videos([video], lambda v: probs, rank=0, world_size=1, loss_route='torch')
    p_np, l_np = probs.cpu().numpy(), video['labels'].numpy()
    logs = ref.nll_logs(p_np, l_np)
    bound = 0.5 / (1 << 20) + ref.eps_device(1 << 20) + ref.EPS + ref.nll_device_bound(logs) / logs.size
    print('Loss hip %.9f torch %.9f (bound %.3e)' % (hip['Loss'], tor['Loss'], bound), hip)
    assert abs(hip['Loss'] - tor['Loss']) <= bound and math.isfinite(hip['Loss']) and hip['Loss'] > 0
    assert all(hip[k] == tor[k] for k in ('J-Mean', 'F-Mean', 'JF-Mean'))
    assert abs(tor['Loss'] - (ref.sorted_lovasz(p_np, l_np) + ref.clip_loss(p_np, l_np, 255, 2)['nll'])) <= 4 * ref.EPS
