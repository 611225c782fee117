# -*- coding: utf-8 -*-
"""Clip I/O (csrc/clip_io.hip, rmnet_amd.clip_io, include/rmnet_hip.h F1): uint8 frames and label maps in, label maps and overlay
frames out.  Every comparison is bit for bit; no tolerance appears in this file.

The chain of evidence: tests/golden/clip_io.npz, recorded from the reference's own img_normalize / to_onehot / ReorganizeObjectID /
get_segmentation, pins the numpy restatement tests/clip_io_ref.py; the restatement then judges the torch fallbacks (CPU tests) and
the four kernels (GPU tests) on the cases of clip_io_ref.py.  Copies of the restatement with one planted fault each must differ
from it on those cases, which shows that the cases can see the fault."""

import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import clip_io_ref as ref
from conftest import GOLDEN

gpu = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


def bits(a):
    """An array as raw integers, so that a comparison of floats is a comparison of bits (and -0.0 != 0.0)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def golden():
    d = np.load(os.path.join(GOLDEN, 'clip_io.npz'))
    return {name: {k.split('/', 1)[1]: d[k] for k in d.files if k.startswith(name + '/')} for name in d['names']}, d['palette'], int(d['K'])


# At alpha = 0.4 a fused multiply-add in the blend returns the same byte as the two separately rounded operations for every byte
# value and every colour component that occurs (0, 64, 128, 191, 16, 100, 255): no test at the default alpha can see a contraction
# of the blend.  At alpha = 0.7 nine (value, component) pairs differ, (96, 16) -> 71 against 72 among them, so the exhaustive
# frames are blended with both.
EXHAUSTIVE_ALPHAS = (0.4, 0.7)


def overlay_cases():
    """The overlay cases of the GPU tests: (name, uint8 frames, float32 frames, labels, mean, std, ignore_idx, alpha).  The uint8
    frames are the source of the first float frames (of all of them but for the exhaustive cases, whose second float frame holds the
    centres of the bytes' intervals)."""
    out = []
    u8, labels = ref.overlay_clip()
    for alpha in (0.0, 0.4, 1.0):
        out.append(('clip a=%g' % alpha, u8, ref.normalize(u8), labels, ref.MEAN, ref.STD, 255, alpha))
    out.append(('clip odd', u8, ref.normalize(u8, ref.ODD_MEAN, ref.ODD_STD), labels, ref.ODD_MEAN, ref.ODD_STD, 255, 0.4))
    for mean, std in ((ref.MEAN, ref.STD), (ref.ODD_MEAN, ref.ODD_STD)):
        ramp, frames, labels2 = ref.exhaustive_case(mean, std)      # (uint8 frames for float frame 0 only)
        for alpha in EXHAUSTIVE_ALPHAS:
            out.append(('exhaustive a=%g' % alpha, ramp, frames, labels2, mean, std, ref.EXHAUSTIVE_IGNORE, alpha))
    return out


# ================================================================================================ CPU
def test_the_restatement_equals_the_fixture_recorded_from_the_reference(golden):
    cases, pal, K = golden
    assert len(cases) == 7 and same(ref.palette(), pal)
    for name, c in cases.items():
        frames, labels, mean, std, alpha = c['frames'], c['labels'], c['mean'], c['std'], float(c['alpha'])
        normalized = ref.normalize(frames, mean, std)
        assert same(normalized, c['normalized']), name
        lut, n_ids = ref.reorganize_lut(labels)
        assert n_ids == int(c['n_ids']) and same(lut[labels], c['remapped']), name
        assert same(ref.onehot(labels, K, lut), c['onehot_remapped']) and same(ref.onehot(labels, K), c['onehot_plain']), name
        assert same(ref.denormalize(normalized, mean, std), c['denorm']), name
        assert same(ref.overlay(normalized, labels, mean, std, 255, alpha), c['overlay']), name
    # what the fixture covers: a frame without background, labels 255 and >= 16, touching objects, sparse ids, 1-row and 1-column maps
    assert cases['clip']['labels'][1].min() == 1 and (cases['clip']['labels'] == 255).any() and (cases['clip']['labels'] == 17).any()
    assert sorted(set(cases['sparse']['labels'].ravel().tolist())) == [3, 7, 200, 255] and int(cases['sparse']['n_ids']) == 3
    assert cases['one_row']['labels'].shape[1] == 1 and cases['one_col']['labels'].shape[2] == 1
    assert (cases['clip']['denorm'] != cases['clip']['frames']).any()          # the denormalised byte is not the source byte


def _check_all_against_the_restatement(device, contiguous):
    """Every function of rmnet_amd.clip_io on the shape cases, the overlay cases and an argmax case, against the restatement.
    ``contiguous`` False hands over strided views, which take the torch restatement on any device."""
    from rmnet_amd import clip_io

    def t(a):
        x = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        if contiguous:
            return x
        wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=x.dtype, device=device)
        wide[..., ::2] = x
        return wide[..., ::2]

    for (H, W) in ref.SHAPES:
        for N in (1, 3):
            u8, labels = ref.shape_case(N, H, W)
            normalized = ref.normalize(u8)
            assert same(to_np(clip_io.normalize_frames(t(u8), ref.MEAN, ref.STD)), normalized), (N, H, W)
            lut, n_ids = clip_io.reorganize_lut(t(labels))
            want_lut, want_n = ref.reorganize_lut(labels)
            assert same(to_np(lut), want_lut) and int(n_ids) == want_n, (N, H, W)
            for K in (2, 5):       # 2: smaller than the largest remapped id
                assert same(to_np(clip_io.onehot_labels(t(labels), K, lut)), ref.onehot(labels, K, want_lut)), (N, H, W, K)
            assert same(to_np(clip_io.onehot_labels(t(labels), 18)), ref.onehot(labels, 18)), (N, H, W)
            got = clip_io.overlay(t(normalized), t(labels), ref.MEAN, ref.STD)
            assert same(to_np(got), ref.overlay(normalized, labels)), (N, H, W)
            for K in (1, 2, 3, 11):
                prob = ref.argmax_case(N, K, H, W)
                assert same(to_np(clip_io.argmax_labels(t(prob))), ref.argmax_first(prob)), (N, K, H, W)
    for name, u8, frames, labels, mean, std, ignore_idx, alpha in overlay_cases():
        # normalise, denormalise and blend in a chain: the overlay is fed what normalize_frames itself returned.  For the exhaustive
        # cases that is every byte value in every channel through the normalisation, with both (mean, std) pairs
        normalized = to_np(clip_io.normalize_frames(t(u8), mean, std))
        assert same(normalized, frames[:len(u8)]), name
        chained = np.concatenate([normalized, frames[len(u8):]])
        got = clip_io.overlay(t(chained), t(labels), mean, std, ignore_idx, alpha)
        assert same(to_np(got), ref.overlay(frames, labels, mean, std, ignore_idx, alpha)), name
    all_ignored = np.full((2, 3, 4), 255, np.uint8)
    lut, n_ids = clip_io.reorganize_lut(t(all_ignored))
    assert int(n_ids) == 0 and not to_np(lut).any()
    assert same(to_np(clip_io.onehot_labels(t(all_ignored), 3, lut)), ref.onehot(all_ignored, 3, np.zeros(256, np.uint8)))
    assert not to_np(clip_io.onehot_labels(t(all_ignored), 3)).any()


def test_the_torch_fallbacks_equal_the_restatement_on_the_cpu():
    _check_all_against_the_restatement(torch.device('cpu'), contiguous=True)


def test_other_dtypes_take_the_fallback_and_give_the_same_bytes():
    from rmnet_amd import clip_io
    u8, labels = ref.overlay_clip()
    frames = ref.normalize(u8)
    got = clip_io.overlay(torch.from_numpy(frames), torch.from_numpy(labels.astype(np.int64)), ref.MEAN, ref.STD)
    assert same(to_np(got), ref.overlay(frames, labels))
    assert same(to_np(clip_io.onehot_labels(torch.from_numpy(labels.astype(np.int32)), 4)), ref.onehot(labels, 4))
    prob = ref.argmax_case(2, 3, 3, 5).astype(np.float64)
    assert same(to_np(clip_io.argmax_labels(torch.from_numpy(prob))), ref.argmax_first(prob))
    assert same(to_np(clip_io.PALETTE), ref.palette())
    assert same(to_np(clip_io.denormalize_frames(torch.from_numpy(frames), ref.MEAN, ref.STD)), ref.denormalize(frames))
    with pytest.raises(RuntimeError):
        clip_io.overlay(torch.from_numpy(frames), torch.from_numpy(labels), ref.MEAN, ref.STD, alpha=1.5)
    with pytest.raises(RuntimeError):
        clip_io.argmax_labels(torch.zeros(1, 256, 2, 2))


def test_helpers_mirror_the_reference_signatures(golden):
    from rmnet_amd import helpers
    cases, pal, K = golden
    c = cases['clip']
    mean, std = c['mean'].tolist(), c['std'].tolist()
    image = helpers.img_normalize(c['frames'][0], mean, std)
    assert isinstance(image, np.ndarray) and same(image.transpose(2, 0, 1), c['normalized'][0])
    assert same(helpers.img_normalize(c['frames'][0], mean, std, order='CHW'), c['normalized'][0])
    assert same(helpers.to_onehot(c['labels'][0], K), c['onehot_plain'][0])
    assert same(to_np(helpers.to_onehot(torch.from_numpy(c['labels'][0]), K)), c['onehot_plain'][0])
    assert same(helpers.img_denormalize(torch.from_numpy(c['normalized'][0]), mean, std), c['denorm'][0])
    params = {'mean': mean, 'std': std}
    for i in range(4):
        frame = torch.cat([torch.from_numpy(c['normalized'][i]), torch.zeros(1, 9, 12)])       # (frame[:3] is what is drawn)
        image = helpers.get_segmentation(frame, torch.from_numpy(c['labels'][i].astype(np.int64)), params)
        assert image.mode == 'RGB' and same(np.array(image), c['overlay'][i])
    image = helpers.get_segmentation(None, torch.from_numpy(c['labels'][0].astype(np.int64)), params)
    assert image.mode == 'P' and same(np.array(image), c['labels'][0])
    assert same(np.asarray(image.getpalette(), np.uint8).reshape(-1, 3), pal)


def test_png_files_round_trip(tmp_path, golden):
    from PIL import Image
    from rmnet_amd import inference
    cases, pal, _ = golden
    c = cases['clip']
    paths = inference.write_segmentations(str(tmp_path / 'labels' / 'clip'), torch.from_numpy(c['labels']))
    assert [os.path.basename(p) for p in paths] == ['%05d.png' % i for i in range(4)] == sorted(os.listdir(str(tmp_path / 'labels' / 'clip')))
    for i, p in enumerate(paths):
        image = Image.open(p)
        assert image.mode == 'P' and same(np.array(image), c['labels'][i])
        assert same(np.asarray(image.getpalette(), np.uint8).reshape(-1, 3)[:256], pal)
    paths = inference.write_segmentations(str(tmp_path / 'overlay'), torch.from_numpy(c['overlay']))
    assert [os.path.basename(p) for p in paths] == ['%05d.png' % i for i in range(4)]
    for i, p in enumerate(paths):
        image = Image.open(p)
        assert image.mode == 'RGB' and same(np.array(image), c['overlay'][i])
    with pytest.raises(RuntimeError):
        inference.write_segmentations(str(tmp_path / 'bad'), torch.zeros(2, 3, 4, 5, dtype=torch.uint8))


def test_the_argument_rules_of_the_c_entries_hold_without_a_launch():
    """Every call below is refused on the host (a return of -3 would mean that a launch was attempted).  The pointers are
    placeholders: an entry that is going to refuse never reads them."""
    from rmnet_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    p = ctypes.c_void_p(1 << 20)
    three = ctypes.c_double * 3
    mean, std, zero_std = three(*ref.MEAN), three(*ref.STD), three(0.229, 0.0, 0.225)
    big = (1 << 30, 1 << 10, 1 << 10)          # N, H, W: 2^30 frames x 1024 workgroups of four-pixel lanes
    # frames in
    assert lib.rmnet_frames_normalize_u8(None, 1, 2, 2, mean, std, p, None) == INVALID
    assert lib.rmnet_frames_normalize_u8(p, 1, 2, 2, mean, std, None, None) == INVALID
    assert lib.rmnet_frames_normalize_u8(p, 1, 2, 2, None, std, p, None) == INVALID
    for n, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        assert lib.rmnet_frames_normalize_u8(p, n, h, w, mean, std, p, None) == INVALID
    assert lib.rmnet_frames_normalize_u8(p, 1, 2, 2, mean, zero_std, p, None) == INVALID
    assert lib.rmnet_frames_normalize_u8(p, *big, mean, std, p, None) == UNSUPPORTED
    # label maps in
    assert lib.rmnet_labels_onehot_u8(None, None, 1, 2, 2, 2, p, None) == INVALID
    assert lib.rmnet_labels_onehot_u8(p, None, 1, 2, 2, 2, None, None) == INVALID
    assert lib.rmnet_labels_onehot_u8(p, None, 1, 0, 2, 2, p, None) == INVALID
    assert lib.rmnet_labels_onehot_u8(p, None, 1, 256, 2, 2, p, None) == UNSUPPORTED
    assert lib.rmnet_labels_onehot_u8(p, None, big[0], 2, big[1], big[2], p, None) == UNSUPPORTED
    # label maps out
    assert lib.rmnet_argmax_labels_f32(None, 1, 2, 2, 2, p, None) == INVALID
    assert lib.rmnet_argmax_labels_f32(p, 1, 2, 2, 2, None, None) == INVALID
    assert lib.rmnet_argmax_labels_f32(p, 1, 0, 2, 2, p, None) == INVALID
    assert lib.rmnet_argmax_labels_f32(p, 1, 256, 2, 2, p, None) == UNSUPPORTED
    assert lib.rmnet_argmax_labels_f32(p, big[0], 2, big[1], big[2], p, None) == UNSUPPORTED
    # overlay frames out
    ok = (mean, std, 0.4, 255)
    assert lib.rmnet_overlay_u8(None, p, 1, 2, 2, *ok, p, p, 4, None) == INVALID
    assert lib.rmnet_overlay_u8(p, None, 1, 2, 2, *ok, p, p, 4, None) == INVALID
    assert lib.rmnet_overlay_u8(p, p, 1, 2, 2, *ok, None, p, 4, None) == INVALID
    assert lib.rmnet_overlay_u8(p, p, 0, 2, 2, *ok, p, p, 4, None) == INVALID
    for alpha in (-0.01, 1.01, float('nan')):
        assert lib.rmnet_overlay_u8(p, p, 1, 2, 2, mean, std, alpha, 255, p, p, 4, None) == INVALID
    assert lib.rmnet_overlay_u8(p, p, 1, 2, 2, mean, zero_std, 0.4, 255, p, p, 4, None) == INVALID
    assert lib.rmnet_overlay_u8(p, p, 1, 2, 2, *ok, p, None, 4, None) == WORKSPACE
    assert lib.rmnet_overlay_u8(p, p, 3, 2, 2, *ok, p, p, 11, None) == WORKSPACE
    assert lib.rmnet_overlay_u8(p, p, *big, *ok, p, p, 4 << 30, None) == UNSUPPORTED


def test_segment_video_u8_refuses_label_maps_that_hold_only_the_ignored_id():
    from rmnet_amd import inference
    u8, labels = ref.shape_case(2, 3, 5)
    with pytest.raises(RuntimeError, match='nothing to segment'):
        inference.segment_video_u8(_PerPixelNet(), None, torch.from_numpy(u8), torch.full((3, 5), 255, dtype=torch.uint8), 4, ref.MEAN, ref.STD)


def test_the_bindings_reject_cpu_tensors():
    from rmnet_amd import ops
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.frames_normalize(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), ref.MEAN, ref.STD)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.labels_onehot(torch.zeros(1, 2, 2, dtype=torch.uint8), 2)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.argmax_labels(torch.zeros(1, 2, 2, 2))
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.overlay(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.uint8), ref.MEAN, ref.STD)


# ------------------------------------------------------------------------------------------------ planted faults
def _fused_blend(v, alpha, colour):
    """trunc(fma(v, alpha, (1 - alpha) * colour)) per channel: the exact sum of the exact product and the rounded second term,
    rounded once (float(Fraction) rounds to nearest even), as a fused multiply-add would give it."""
    out = np.empty_like(v)
    for c in range(3):
        second = Fraction((1.0 - alpha) * float(colour[c]))
        table = np.array([min(255, int(float(Fraction(b) * Fraction(alpha) + second))) for b in range(256)], np.uint8)
        out[..., c] = table[v[..., c]]
    return out


def _grow8(m):
    g = ref.grow4(m)
    g[1:, 1:] |= m[:-1, :-1]
    g[1:, :-1] |= m[:-1, 1:]
    g[:-1, 1:] |= m[1:, :-1]
    g[:-1, :-1] |= m[1:, 1:]
    return g


FAULTS = ('eight_neighbours', 'round_to_nearest', 'descending', 'lowest_is_0', 'lowest_of_clip', 'fused_blend', 'source_byte')


def _overlay_with(fault, u8, frames, labels, mean, std, ignore_idx, alpha):
    """A copy of clip_io_ref.overlay with one fault planted (None: none)."""
    assert fault is None or fault in FAULTS
    rnd = np.rint if fault == 'round_to_nearest' else np.trunc
    to8 = lambda v: np.clip(rnd(v), 0, 255).astype(np.uint8)
    x = frames.astype(np.float64).transpose(0, 2, 3, 1)
    out = to8((x * np.asarray(std, np.float64) + np.asarray(mean, np.float64)) * 255.0)
    if fault == 'source_byte':
        out[:len(u8)] = u8
    colours = ref.palette().astype(np.float64)
    for n in range(labels.shape[0]):
        present = sorted(set(labels[n].reshape(-1).tolist()))
        lowest = 0 if fault == 'lowest_is_0' else int(labels.min()) if fault == 'lowest_of_clip' else present[0]
        objects = [o for o in present if o != lowest and o != ignore_idx]
        if fault == 'descending':
            objects.reverse()
        for o in objects:
            m = labels[n] == o
            if fault == 'fused_blend':
                blended = _fused_blend(out[n], alpha, colours[o])
            else:
                blended = to8(out[n].astype(np.float64) * alpha + (1.0 - alpha) * colours[o])
            out[n][m] = blended[m]
            out[n][(_grow8(m) if fault == 'eight_neighbours' else ref.grow4(m)) & ~m] = 0
    return out


def test_each_planted_fault_changes_a_byte_on_the_cases_of_the_gpu_tests():
    cases = overlay_cases()
    for (H, W) in ref.SHAPES:
        u8, labels = ref.shape_case(3, H, W)
        cases.append(('shape %dx%d' % (H, W), u8, ref.normalize(u8), labels, ref.MEAN, ref.STD, 255, 0.4))
    seen = dict.fromkeys(FAULTS, 0)
    for name, u8, frames, labels, mean, std, ignore_idx, alpha in cases:
        want = ref.overlay(frames, labels, mean, std, ignore_idx, alpha)
        assert same(_overlay_with(None, u8, frames, labels, mean, std, ignore_idx, alpha), want), name       # the copy itself is faithful
        for fault in FAULTS:
            seen[fault] += int((_overlay_with(fault, u8, frames, labels, mean, std, ignore_idx, alpha) != want).sum())
    print('bytes changed by each planted fault:', seen)
    assert all(n > 0 for n in seen.values()), seen
    # the exhaustive case alone sees the three arithmetic faults, and reaches every byte value in every channel before the blend
    for mean, std in ((ref.MEAN, ref.STD), (ref.ODD_MEAN, ref.ODD_STD)):
        u8, frames, labels = ref.exhaustive_case(mean, std)
        den = ref.denormalize(frames, mean, std)
        assert same(den[1], u8[0]) and (den[0] != u8[0]).any()
        want = ref.overlay(frames, labels, mean, std, ref.EXHAUSTIVE_IGNORE, 0.4)
        assert (_overlay_with('round_to_nearest', u8, frames, labels, mean, std, ref.EXHAUSTIVE_IGNORE, 0.4) != want).any()
        assert same(_overlay_with('fused_blend', u8, frames, labels, mean, std, ref.EXHAUSTIVE_IGNORE, 0.4), want)      # (see EXHAUSTIVE_ALPHAS)
        want7 = ref.overlay(frames, labels, mean, std, ref.EXHAUSTIVE_IGNORE, 0.7)
        assert (_overlay_with('fused_blend', u8, frames, labels, mean, std, ref.EXHAUSTIVE_IGNORE, 0.7) != want7).any()
        assert (_overlay_with('source_byte', u8, frames, labels, mean, std, ref.EXHAUSTIVE_IGNORE, 0.4) != want).any()
        # the normalisation sees all 768 (byte, channel) pairs of this pair of (mean, std) in the one frame
        assert all(len(set(u8[0, :, :, c].ravel().tolist())) == 256 for c in range(3))
    # argmax: the last index on ties
    prob = ref.argmax_case(3, 11, 3, 5)
    last = (prob.shape[1] - 1 - np.argmax(prob[:, ::-1], axis=1)).astype(np.uint8)
    assert (last != ref.argmax_first(prob)).any() and same(ref.argmax_first(prob), np.argmax(prob, axis=1).astype(np.uint8))


# ================================================================================================ GPU
@gpu
def test_the_kernels_equal_the_restatement_on_every_shape_and_overlay_case():
    """Contiguous tensors on the GPU: the four kernels, on the shapes of clip_io_ref.SHAPES with N = 1 and 3 (H*W mod 4 = 0 .. 3
    and mod 16 = 0: the 16-, 4- and 1-pixel lanes, pixel tails, one-row and one-column maps, another lowest label in each frame),
    the structured overlay clip with alpha 0, 0.4 and 1 and the exhaustive arithmetic frames with two (mean, std) pairs."""
    _check_all_against_the_restatement(dev(), contiguous=True)


@gpu
def test_strided_views_on_the_gpu_take_the_fallback_and_give_the_same_bytes():
    _check_all_against_the_restatement(dev(), contiguous=False)


@gpu
def test_argmax_with_255_planes_and_a_misaligned_plane_base():
    from rmnet_amd import clip_io
    prob = ref.argmax_case(2, 255, 3, 8)
    assert same(to_np(clip_io.argmax_labels(torch.from_numpy(prob).to(dev()))), ref.argmax_first(prob))
    # a contiguous tensor that starts one float (one byte) into an allocation: H*W % 4 == 0, but no 16-byte (4-byte) alignment
    prob = ref.argmax_case(3, 11, 4, 8)
    store = torch.zeros(prob.size + 1, device=dev())
    view = store[1:].view(prob.shape)
    view.copy_(torch.from_numpy(prob))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert same(to_np(clip_io.argmax_labels(view)), ref.argmax_first(prob))
    u8, labels = ref.shape_case(3, 4, 8)
    store = torch.zeros(labels.size + 1, dtype=torch.uint8, device=dev())
    lab = store[1:].view(labels.shape)
    lab.copy_(torch.from_numpy(labels))
    assert lab.is_contiguous() and lab.data_ptr() % 4 == 1
    frames = ref.normalize(u8)
    assert same(to_np(clip_io.onehot_labels(lab, 5)), ref.onehot(labels, 5))
    assert same(to_np(clip_io.overlay(torch.from_numpy(frames).to(dev()), lab, ref.MEAN, ref.STD)), ref.overlay(frames, labels))


@gpu
def test_two_calls_give_equal_bytes_and_the_four_entries_replay_from_one_graph():
    from rmnet_amd import clip_io, ops
    u8, labels = ref.shape_case(3, 5, 256)
    prob = ref.argmax_case(3, 11, 5, 256)
    lut_np, _ = ref.reorganize_lut(labels)
    t_u8, t_labels, t_prob, t_lut = (torch.from_numpy(a).to(dev()) for a in (u8, labels, prob, lut_np))

    def run():
        frames = ops.frames_normalize(t_u8, ref.MEAN, ref.STD)
        return frames, ops.labels_onehot(t_labels, 4, t_lut), ops.argmax_labels(t_prob), ops.overlay(frames, t_labels, ref.MEAN, ref.STD)

    first = [to_np(x) for x in run()]
    second = [to_np(x) for x in run()]
    frames = ref.normalize(u8)
    want = [frames, ref.onehot(labels, 4, lut_np), ref.argmax_first(prob), ref.overlay(frames, labels)]
    for a, b, w in zip(first, second, want):
        assert same(a, b) and same(a, w)
    stream = torch.cuda.Stream(device=dev())
    stream.wait_stream(torch.cuda.current_stream(dev()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            outs = run()
        t_u8.copy_(255 - t_u8)                        # other inputs than the captured call saw
        t_labels.copy_(torch.flip(t_labels, dims=[0]))
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(dev()).wait_stream(stream)
    u8b, labels_b = 255 - u8, np.ascontiguousarray(labels[::-1])
    frames_b = ref.normalize(u8b)
    want = [frames_b, ref.onehot(labels_b, 4, lut_np), ref.argmax_first(prob), ref.overlay(frames_b, labels_b)]
    for got, w in zip(outs, want):
        assert same(to_np(got), w)


def _u8_clip():
    """A 3-frame 96 x 160 synthetic clip as a folder of images would hold it: uint8 RGB frames, palette label maps with sparse ids
    (0, 5, 38) and a few ignored pixels."""
    from rmnet_amd.synthetic import synthetic_clip
    frames, masks, _, _ = synthetic_clip(3, 3, 96, 160, seed=3, size=1.5)
    mean, std = torch.tensor(ref.MEAN).view(1, 3, 1, 1), torch.tensor(ref.STD).view(1, 3, 1, 1)
    u8 = ((frames[0] * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    labels = np.asarray([0, 5, 38], np.uint8)[masks[0].argmax(dim=1).numpy()]
    labels[:, :2, :2] = 255
    return u8, labels


class _Recorder:
    """Stands where the network stands in segment_video / segment_video_u8 and keeps what went in and what came out."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, frames, masks, flows, n_objects, memorize_every, **kw):
        est = self.net(frames, masks, flows, n_objects, memorize_every, **kw)
        self.calls.append({'frames': frames, 'masks': masks, 'n_objects': n_objects, 'memorize_every': memorize_every, 'est': est})
        return est


class _PerPixelNet(torch.nn.Module):
    """A stand-in network whose output is a fixed elementwise function of the frames and of the first frame's masks: the same bits
    for the same inputs, with many exact ties between the planes."""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def forward(self, frames, masks, flows, n_objects, memorize_every, device=None):
        K = masks.shape[2]
        first = masks.to(frames.device)[:, :1].float()
        planes = torch.arange(K, device=frames.device, dtype=torch.float32).view(1, 1, K, 1, 1)
        return torch.softmax(first + torch.floor(frames[:, :, :1] * 2.0) * torch.remainder(planes, 2.0), dim=2)


def _library_reproducible():
    """The library's convolutions with reproducible solvers, as tests/test_flow_conv.py asks for them: with the default solvers two
    runs of the same networks on the same clip differ in their last bits (measured on an MI355X on this clip: flows not equal,
    probabilities up to 7.1e-05 apart, label maps different at 2 to 3 of 46080 pixels)."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


@gpu
def test_segment_video_u8_equals_segment_video_on_the_restated_inputs():
    """The labels of segment_video_u8 equal those of segment_video fed with the restatement's normalised frames and one-hot masks,
    and its overlay equals the restatement applied to those labels: with a per-pixel stand-in network, and with RMNet + TinyFlowNet
    under the library's reproducible solvers.  With the real networks a recorder around the network also shows what the statement
    is made of: segment_video_u8 hands the network the same bits as segment_video does (frames, masks, object count) and its labels
    are the first-index argmax of the very probabilities the network returned to it."""
    from rmnet_amd import inference, networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.tiny_flownet import TinyFlowNet
    u8, labels = _u8_clip()
    lut, n_ids = ref.reorganize_lut(labels)
    assert n_ids == 3
    normalized = ref.normalize(u8)
    video = {'frames': torch.from_numpy(normalized), 'masks': torch.from_numpy(ref.onehot(labels, 5, lut)).to(dev()), 'n_objects': 2}
    t_u8, t_labels = torch.from_numpy(u8), torch.from_numpy(labels)

    net, no_flow = _PerPixelNet().to(dev()), lambda clip: torch.zeros(1, clip.shape[1], 2, clip.shape[3], clip.shape[4], device=clip.device)
    got = inference.segment_video_u8(net, no_flow, t_u8, t_labels, 4, ref.MEAN, ref.STD, memorize_every=2)
    want = to_np(inference.segment_video(net, no_flow, video, memorize_every=2))
    assert got['n_objects'] == 2 and got['labels'].is_cuda and got['overlay'].is_cuda and got['labels'].dtype == torch.uint8
    assert same(to_np(got['labels']), want) and len(set(want.ravel().tolist())) >= 3
    assert same(to_np(got['overlay']), ref.overlay(normalized, want))
    first_only = inference.segment_video_u8(net, no_flow, t_u8, t_labels[0], 4, ref.MEAN, ref.STD, memorize_every=2, overlay=False)
    assert first_only['overlay'] is None and same(to_np(first_only['labels']), want)

    net = _Recorder(networks.procedural_init_(RMNet(None)).to(dev()).eval())
    tfn = networks.procedural_init_(TinyFlowNet(None)).to(dev()).eval()
    with _library_reproducible():
        got = inference.segment_video_u8(net, tfn, t_u8, t_labels, 4, ref.MEAN, ref.STD, memorize_every=2)
        want = to_np(inference.segment_video(net, tfn, video, memorize_every=2))
        first_only = inference.segment_video_u8(net, tfn, t_u8, t_labels[0], 4, ref.MEAN, ref.STD, memorize_every=2, overlay=False)
    mine, theirs = net.calls[:2]
    assert same(to_np(mine['frames']), to_np(theirs['frames'])) and same(to_np(mine['frames'][0]), normalized)
    assert same(to_np(mine['masks']), to_np(theirs['masks'])) and same(to_np(mine['n_objects']), to_np(theirs['n_objects']))
    assert mine['memorize_every'] == theirs['memorize_every'] == 2 and got['n_objects'] == 2
    assert same(to_np(got['labels']), to_np(mine['est'][0].argmax(dim=1).to(torch.uint8)))
    assert same(want, to_np(theirs['est'][0].argmax(dim=1).to(torch.uint8)))
    print('probabilities of the two runs: equal bits %s, max difference %.3e' % (torch.equal(mine['est'], theirs['est']), float((mine['est'] - theirs['est']).abs().max())))
    assert same(to_np(got['labels']), want) and len(set(want.ravel().tolist())) >= 2
    assert same(to_np(got['overlay']), ref.overlay(normalized, want))
    assert first_only['overlay'] is None and same(to_np(first_only['labels']), want)
