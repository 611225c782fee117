# -*- coding: utf-8 -*-
"""Boundary measure F (utils/metrics.py:119-226): the numpy restatement tests/boundary_ref.py pinned by hand-checkable answers, the
torch restatement of rmnet_amd.metrics against it on the CPU, and the HIP kernel (csrc/boundary_f.hip) against it on the GPU.  Every
count is an integer and is compared exactly."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import boundary_ref as br

FAMILIES = [(3, 3, 37, 70), (2, 2, 64, 128), (1, 5, 50, 200), (2, 2, 5, 9)]      # (N, K, H, W)
RULE_RADIUS = {(37, 70): 1, (64, 128): 2, (50, 200): 2, (5, 9): 1}               # ceil(0.008 * |(H, W)|)


# ------------------------------------------------------------------------------------------------ inputs and the shared reference
@functools.lru_cache(maxsize=None)
def blob_maps(N, K, H, W, seed=0, extra_label=False):
    """gt: one filled ellipse per object and frame (later objects paint over earlier ones; centres anywhere in the frame, so some
    touch its edges); pred: gt rolled by (1, 2) with 1 % of the pixels cleared.  uint8 [N, H, W] each."""
    rng = np.random.default_rng(1000 * seed + 7 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        for k in range(1, K + 1 + int(extra_label)):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ay, ax = rng.uniform(0.15, 0.45) * H + 1, rng.uniform(0.15, 0.45) * W + 1
            gt[n][((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1] = k
    pred = np.roll(gt, (1, 2), axis=(1, 2)).copy()
    pred[rng.random(pred.shape) < 0.01] = 0
    gt.setflags(write=False)
    pred.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def family_ref(N, K, H, W, radius, fault=None):
    pred, gt = blob_maps(N, K, H, W)
    out = br.counts_of_labels(pred, gt, K, radius, fault)
    out.setflags(write=False)
    return out


def family_cases():
    return [(f, r) for f in FAMILIES for r in (RULE_RADIUS[f[2:]], 3)]


def t8(a, device='cpu'):
    return torch.from_numpy(np.array(a, dtype=np.uint8, order='C')).to(device)          # (a C-ordered copy: the cached maps are read-only)


# ------------------------------------------------------------------------------------------------ CPU: the restatement itself
def test_disk_sizes():
    assert [int(br.disk(r).sum()) for r in (0, 1, 2, 3, 4, 5, 8, 18, 36)] == [1, 5, 13, 29, 49, 81, 197, 1009, 4053]
    d = br.disk(5)
    assert d[5 + 3, 5 + 4] == 1 and d[5 + 4, 5 + 4] == 0 and d[5, 0] == 1 and d[4, 0] == 0      # 25 <= 25 in, 32 > 25 out
    from rmnet_amd import metrics
    for r in (0, 1, 2, 5, 8, 18, 40):                  # the torch restatement's convolution weight is the same disk
        assert (metrics._disk(r, 'cpu')[0, 0].numpy() == br.disk(r)).all()


def test_boundary_radius_follows_the_reference_rule():
    from rmnet_amd import metrics
    want = {(480, 854): 8, (480, 864): 8, (1080, 1920): 18, (2160, 3840): 36, (16, 16): 1, (64, 128): 2, (50, 200): 2,
            (75, 100): 1, (100, 75): 1}          # |(75, 100)| = 125 and 0.008 * 125 is 1.0 in float64: the ceil stays 1
    for (h, w), r in want.items():
        assert metrics.boundary_radius(h, w) == r == br.boundary_radius((h, w)), (h, w)
        assert isinstance(metrics.boundary_radius(h, w), int)
    assert metrics.boundary_radius(480, 854, bound_th=3) == 3 == br.boundary_radius((480, 854), 3)
    for f in FAMILIES:
        assert metrics.boundary_radius(*f[2:]) == RULE_RADIUS[f[2:]]


def _set(b):
    return {(int(y), int(x)) for y, x in zip(*np.nonzero(b))}


def test_bmap_by_hand():
    from rmnet_amd import metrics
    def both(seg):
        seg = np.asarray(seg, dtype=np.uint8)
        a = _set(br.seg2bmap(seg))
        assert a == _set(metrics._bmap(torch.from_numpy(seg).bool()).numpy())        # the torch restatement says the same
        return a
    one = np.zeros((5, 5))
    one[2, 2] = 1
    assert both(one) == {(1, 1), (1, 2), (2, 1), (2, 2)}
    corner = np.zeros((5, 5))
    corner[4, 4] = 1
    assert both(corner) == {(3, 3), (3, 4), (4, 3)}
    assert both(np.ones((5, 5))) == set() and both(np.ones((1, 1))) == set() and both(np.zeros((1, 1))) == set()
    assert both(np.array([[0, 1, 1, 0, 1]])) == {(0, 0), (0, 2), (0, 3)}             # 1 0 1 1 0
    assert both(np.array([[0, 1, 1, 0, 1]]).T) == {(0, 0), (2, 0), (3, 0)}
    origin = np.zeros((4, 4))
    origin[0, 0] = 1
    assert both(origin) == {(0, 0)}


def test_the_four_f_cases():
    from rmnet_amd import metrics
    blob = np.zeros((12, 12), dtype=np.uint8)
    blob[3:8, 4:9] = 1
    empty = np.zeros_like(blob)
    assert br.f_score(empty, blob) == 0 and br.f_score(blob, empty) == 0
    assert br.f_score(empty, empty) == 1 and br.f_score(blob, blob) == 1
    n = br.f_counts(blob, blob, 1)[0]
    assert n > 0
    c = torch.tensor([[0, n, 0, 0], [n, 0, 0, 0], [0, 0, 0, 0], [n, n, n, n], [n, n, 0, 0]])
    f = metrics.f_from_counts(c)
    assert f.dtype == torch.float64 and f.tolist() == [0.0, 0.0, 1.0, 1.0, 0.0]


def test_restatement_dilation_against_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(3)
    for r in range(0, 7):
        for shape in ((23, 31), (4, 40), (9, 3)):
            b = rng.random(shape) < 0.04
            want = ndi.binary_dilation(b, structure=br.disk(r))
            assert (br.binary_dilation(b, br.disk(r)) == want).all(), (r, shape)
            from rmnet_amd import metrics
            assert (metrics._dilate(torch.from_numpy(b)[None, None], metrics._disk(r, 'cpu'))[0, 0].numpy() == want).all(), (r, shape)


# ------------------------------------------------------------------------------------------------ CPU: rmnet_amd.metrics
@pytest.mark.parametrize('family,radius', family_cases())
def test_boundary_counts_on_cpu_tensors_equal_the_restatement(family, radius):
    from rmnet_amd import metrics
    N, K, H, W = family
    pred, gt = blob_maps(*family)
    got = metrics.boundary_counts(t8(pred), t8(gt), K, radius)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, K, 4)
    want = family_ref(*family, radius)
    assert want[..., :2].min() > 0                                   # every object has a boundary in both maps
    assert (got.numpy() == want).all(), (got.numpy(), want)
    got64 = metrics.boundary_counts(t8(pred).long(), t8(gt).long(), K, radius)       # another integer type, same integers
    assert (got64.numpy() == want).all()


def test_f_from_counts_is_the_restatement_bit_for_bit():
    from rmnet_amd import metrics
    for family, radius in family_cases():
        want = family_ref(*family, radius)
        got = metrics.f_from_counts(torch.from_numpy(np.array(want)))
        assert got.dtype == torch.float64
        assert (got.numpy().view(np.int64) == br.f_of_counts(want).view(np.int64)).all()
    edge = np.array([[[0, 5, 0, 0], [5, 0, 0, 0], [0, 0, 0, 0], [7, 3, 2, 1], [7, 3, 0, 0], [9, 9, 9, 9]]])
    assert (metrics.f_from_counts(torch.from_numpy(edge)).numpy().view(np.int64) == br.f_of_counts(edge).view(np.int64)).all()


def test_per_object_f_and_means_on_cpu():
    from rmnet_amd import metrics
    family = FAMILIES[0]
    N, K, H, W = family
    pred, gt = blob_maps(*family)
    f = metrics.boundary_f_per_object(t8(pred), t8(gt), K)
    want = br.f_of_counts(family_ref(*family, RULE_RADIUS[(H, W)]))
    assert (f.numpy().view(np.int64) == want.view(np.int64)).all()
    assert float(metrics.mean_boundary_f(t8(pred), t8(gt), K)) == pytest.approx(want[1:-1].mean(), abs=1e-15)
    assert float(metrics.mean_boundary_f(t8(pred), t8(gt), K, skip_first_and_last=False)) == pytest.approx(want.mean(), abs=1e-15)
    assert metrics.jf_mean(0.25, 0.75) == 0.5
    with pytest.raises(RuntimeError):
        metrics.boundary_counts(t8(pred), t8(gt)[:, :-1], K, 1)


@pytest.mark.parametrize('fault', br.FAULTS)
def test_planted_faults_change_a_count(fault):
    """Each wrong statement of the measure gives other integers on the random families: the cases can tell them apart."""
    from rmnet_amd import metrics
    changed = []
    for f, r in family_cases():
        got = metrics.boundary_counts(*(t8(a) for a in blob_maps(*f)), f[1], r).numpy()
        assert (got == family_ref(*f, r)).all()                      # what the project computes is the unaltered statement ...
        changed.append(bool((family_ref(*f, r, fault) != got).any()))      # ... and not this altered one
    assert any(changed), fault
    if fault == 'square':
        assert all(changed)


# ------------------------------------------------------------------------------------------------ CPU: the C entry and ops
def test_c_entry_argument_rules_need_no_gpu():
    from rmnet_amd import _lib
    lib = _lib.load()
    assert lib.rmnet_boundary_match_workspace_bytes(2, 3, 37, 70) == 2 * 3 * 2 * 37 * 2 * 8
    assert lib.rmnet_boundary_match_workspace_bytes(0, 3, 37, 70) == 0
    assert lib.rmnet_boundary_match_workspace_bytes(2, 3, 37, 0) == 0
    assert lib.rmnet_boundary_match_u8(None, None, 2, 3, 37, 70, 8, None, None, 0, None) == -1
    buf = ctypes.create_string_buffer(64)          # non-NULL pointers; every call below is refused before any launch
    p = ctypes.addressof(buf)
    assert lib.rmnet_boundary_match_u8(p, p, 0, 3, 37, 70, 8, p, p, 64, None) == -1
    assert lib.rmnet_boundary_match_u8(p, None, 2, 3, 37, 70, 8, p, p, 64, None) == -1
    assert lib.rmnet_boundary_match_u8(p, p, 2, 65, 37, 70, 8, p, p, 64, None) == -4
    assert lib.rmnet_boundary_match_u8(p, p, 2, 3, 37, 70, -1, p, p, 64, None) == -4
    assert lib.rmnet_boundary_match_u8(p, p, 2, 3, 37, 70, 41, p, p, 64, None) == -4
    assert lib.rmnet_boundary_match_u8(p, p, 2, 3, 37, 70, 8, p, None, 1 << 20, None) == -2
    assert lib.rmnet_boundary_match_u8(p, p, 2, 3, 37, 70, 8, p, p, 64, None) == -2      # short workspace


def test_ops_boundary_match_rejects_cpu_tensors():
    from rmnet_amd import ops
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.boundary_match(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), 1, 1)


# ------------------------------------------------------------------------------------------------ GPU
def gpu_counts(pred, gt, K, radius):
    from rmnet_amd import ops
    return ops.boundary_match(t8(pred, 'cuda'), t8(gt, 'cuda'), K, radius).cpu().numpy()


def check(pred, gt, K, radius):
    """Kernel == restatement, all four integers of every (frame, object).  Returns the counts."""
    pred, gt = np.asarray(pred, dtype=np.uint8), np.asarray(gt, dtype=np.uint8)
    want = br.counts_of_labels(pred, gt, K, radius)
    got = gpu_counts(pred, gt, K, radius)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert (got == want).all(), (pred.shape, K, radius, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('family,radius', family_cases())
def test_kernel_equals_the_restatement_on_the_random_families(family, radius):
    pred, gt = blob_maps(*family)
    got = gpu_counts(pred, gt, family[1], radius)
    want = family_ref(*family, radius)
    assert (got == want).all(), (np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])


@pytest.mark.gpu
@pytest.mark.parametrize('radius', [0, 1, 2, 5, 8, 40])
def test_kernel_over_the_word_layout(radius):
    """Widths around the 64-pixel word (one word, a word and a bit, two and three words and a bit), heights down to one row, radii up
    to the largest: the disk covers the whole frame where radius >= H or >= W, and at W = 200 a radius of 40 reaches into the
    neighbouring word from either side.  A label K + 1 is painted into both maps."""
    for H in (1, 2, 5, 37, 64):
        for W in (1, 9, 63, 64, 65, 70, 128, 130, 200):
            pred, gt = blob_maps(1, 2, H, W, seed=1, extra_label=True)
            check(pred, gt, 2, radius)


def _rect(N, H, W, boxes):
    m = np.zeros((N, H, W), dtype=np.uint8)
    for n, y0, y1, x0, x1, k in boxes:
        m[n, y0:y1, x0:x1] = k
    return m


@pytest.mark.gpu
def test_kernel_at_the_frame_edges_and_corners():
    H, W = 20, 70
    boxes = [(0, 0, 6, 20, 40, 1), (1, 14, 20, 20, 40, 1), (2, 5, 12, 0, 9, 1), (3, 5, 12, 60, 70, 1),          # top, bottom, left, right
             (4, 0, 5, 0, 7, 1), (5, 0, 5, 63, 70, 1), (6, 15, 20, 0, 7, 1), (7, 15, 20, 63, 70, 1)]           # the four corners
    gt = _rect(8, H, W, boxes)
    for shift in ((0, 0), (1, 2), (-2, -1)):
        pred = np.roll(gt, shift, axis=(1, 2))           # (the roll wraps an edge object to the opposite edge: more edge cases)
        for r in (1, 3):
            check(pred, gt, 1, r)
    last = np.zeros((2, 9, 70), dtype=np.uint8)           # objects in the last row and in the last column only
    last[0, 8, 10:30] = 1
    last[1, 2:7, 69] = 1
    other = np.zeros_like(last)
    other[0, 7, 12:33] = 1
    other[1, 1:6, 68] = 1
    for r in (0, 1, 2):
        check(last, other, 1, r)
        check(other, last, 1, r)
        check(last, last, 1, r)


@pytest.mark.gpu
def test_kernel_across_the_word_columns():
    H, W = 12, 200
    gt = _rect(4, H, W, [(0, 2, 9, 40, 64, 1), (1, 2, 9, 64, 100, 1), (2, 2, 9, 100, 128, 1), (3, 2, 9, 128, 190, 1),
                         (0, 3, 8, 120, 129, 2), (1, 3, 8, 127, 140, 2), (2, 3, 8, 60, 65, 2), (3, 3, 8, 63, 64, 2)])
    for dx in (0, 1, -1, 3):
        pred = np.roll(gt, dx, axis=2)
        for r in (0, 1, 2, 5):
            check(pred, gt, 2, r)


@pytest.mark.gpu
def test_kernel_distance_is_the_disk():
    """Half planes x <= c have a boundary of one pixel per row, in column c.  Two of them at horizontal distance exactly r match in
    every row, at r + 1 in none; the single boundary pixel of a mask at the origin against a mask whose nearest boundary pixel is
    at offset (3, 4) (25 <= 25: inside) and (4, 4) (32 > 25: outside)."""
    r, H, W = 5, 9, 200
    xs = np.arange(W)
    for c in (10, 58, 61, 63, 64, 120, 127):
        for d, hit in ((r, H), (r + 1, 0)):
            pred = np.broadcast_to((xs <= c).astype(np.uint8), (1, H, W))
            gt = np.broadcast_to((xs <= c + d).astype(np.uint8), (1, H, W))
            assert check(pred, gt, 1, r).tolist() == [[[H, H, hit, hit]]]
            assert check(gt, pred, 1, r).tolist() == [[[H, H, hit, hit]]]
    origin = np.zeros((1, 12, 12), dtype=np.uint8)
    origin[0, 0, 0] = 1
    near = np.zeros_like(origin)
    near[0, 4, 5] = 1                      # boundary {(3,4), (3,5), (4,4), (4,5)}
    far = np.zeros_like(origin)
    far[0, 5, 5] = 1                       # boundary {(4,4), (4,5), (5,4), (5,5)}
    assert check(origin, near, 1, r).tolist() == [[[1, 4, 1, 1]]]
    assert check(near, origin, 1, r).tolist() == [[[4, 1, 1, 1]]]
    assert check(origin, far, 1, r).tolist() == [[[1, 4, 0, 0]]]
    assert check(far, origin, 1, r).tolist() == [[[4, 1, 0, 0]]]


@pytest.mark.gpu
def test_kernel_objects_frames_and_empty_maps():
    pred, gt = blob_maps(3, 3, 37, 70)
    H, W = 37, 70
    # a label above K belongs to no object: K = 2 on maps that hold label 3, and the counts of objects 1, 2 are those of K = 3
    assert (check(pred, gt, 2, 2) == check(pred, gt, 3, 2)[:, :2]).all()
    # K = 1 and K = 64 with most objects absent: F = 1 for those
    from rmnet_amd import metrics
    sparse = np.where(np.isin(gt, (1, 3)), gt * 21, 0).astype(np.uint8)                 # labels 21 and 63
    sparse_pred = np.roll(sparse, 1, axis=2)
    c64 = check(sparse_pred, sparse, 64, 1)
    f = metrics.f_from_counts(torch.from_numpy(c64)).numpy()
    absent = [k for k in range(64) if k + 1 not in (21, 63)]
    assert (c64[:, absent] == 0).all() and (f[:, absent] == 1).all() and (c64[:, [20, 62], :2] > 0).all()
    check(pred, gt, 1, 1)
    # three different frames: nothing leaks from one frame or object into the next
    three = np.zeros((3, H, W), dtype=np.uint8)
    three[0, 5:20, 5:30] = 1
    three[1, 10:30, 40:66] = 2
    got = check(three, np.roll(three, 1, axis=1), 2, 2)
    assert (got[0, 1] == 0).all() and (got[1, 0] == 0).all() and (got[2] == 0).all() and got[0, 0].min() > 0 and got[1, 1].min() > 0
    # pred empty, gt empty, both empty
    zero = np.zeros_like(gt)
    assert (check(zero, gt, 3, 1)[..., [0, 2, 3]] == 0).all()
    assert (check(pred, zero, 3, 1)[..., [1, 2, 3]] == 0).all()
    assert (check(zero, zero, 3, 1) == 0).all()


@pytest.mark.gpu
def test_counts_are_fully_written_and_repeatable():
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    family = FAMILIES[0]
    N, K, H, W = family
    pred, gt = (t8(a, 'cuda') for a in blob_maps(*family))
    want = family_ref(*family, 3)
    outs = []
    for fill in (0x7F7F7F7F, -1):
        counts = torch.full((N, K, 4), fill, dtype=torch.int32, device='cuda')
        ws = torch.full((lib.rmnet_boundary_match_workspace_bytes(N, K, H, W),), 0xA5, dtype=torch.uint8, device='cuda')
        rc = lib.rmnet_boundary_match_u8(ops._ptr(pred), ops._ptr(gt), N, K, H, W, 3, ops._ptr(counts), ops._ptr(ws), ws.numel(),
                                         ops._stream(pred.device))
        assert rc == 0
        outs.append(counts.cpu())
    assert (outs[0].numpy() == want).all() and torch.equal(outs[0], outs[1])
    a, b = ops.boundary_match(pred, gt, K, 3), ops.boundary_match(pred, gt, K, 3)
    assert torch.equal(a, b) and torch.equal(a.cpu(), outs[0])
    with pytest.raises(RuntimeError):
        ops.boundary_match(pred, gt[:, :-1].contiguous(), K, 3)
    with pytest.raises(RuntimeError):
        ops.boundary_match(pred, gt, 65, 3)
    with pytest.raises(RuntimeError):
        ops.boundary_match(pred, gt, K, 41)


@pytest.mark.gpu
def test_metrics_on_cuda_maps_equal_the_cpu_path(monkeypatch):
    from rmnet_amd import metrics, ops
    family = FAMILIES[1]
    N, K, H, W = family
    pred, gt = blob_maps(*family)
    f_gpu = metrics.boundary_f_per_object(t8(pred, 'cuda'), t8(gt, 'cuda'), K)
    f_cpu = metrics.boundary_f_per_object(t8(pred), t8(gt), K)
    assert f_gpu.is_cuda and f_gpu.dtype == torch.float64
    assert (f_gpu.cpu().numpy().view(np.int64) == f_cpu.numpy().view(np.int64)).all()
    # the mean adds the same four float64 values in [0, 1] in the device's own order: three roundings of at most 2^-53 * 4 each
    assert abs(float(metrics.mean_boundary_f(t8(pred, 'cuda'), t8(gt, 'cuda'), K)) - float(metrics.mean_boundary_f(t8(pred), t8(gt), K))) <= 2e-15
    # an int64 map and a transposed view stay off the kernel and give the same counts
    want = family_ref(*family, 2)
    def no_kernel(*a, **k):
        raise AssertionError('the kernel was called')
    monkeypatch.setattr(ops, 'boundary_match', no_kernel)
    got = metrics.boundary_counts(t8(pred, 'cuda').long(), t8(gt, 'cuda').long(), K, 2)
    assert got.is_cuda and got.dtype == torch.int32 and (got.cpu().numpy() == want).all()
    pt, gtt = t8(pred.transpose(0, 2, 1), 'cuda').transpose(1, 2), t8(gt.transpose(0, 2, 1), 'cuda').transpose(1, 2)
    assert not pt.is_contiguous() and tuple(pt.shape) == (N, H, W)
    assert (metrics.boundary_counts(pt, gtt, K, 2).cpu().numpy() == want).all()


@pytest.mark.gpu
def test_graph_capture_and_replay():
    from rmnet_amd import ops
    family = FAMILIES[0]
    pred, gt = (t8(a, 'cuda') for a in blob_maps(*family))
    eager = ops.boundary_match(pred, gt, family[1], 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.boundary_match(pred, gt, family[1], 3)            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # a single stream, no parallel branches
        out = ops.boundary_match(pred, gt, family[1], 3)
    out.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    new_pred = torch.roll(pred, 3, dims=2)
    want = ops.boundary_match(new_pred, gt, family[1], 3)
    pred.copy_(new_pred)                                      # the graph reads its inputs in place
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and not torch.equal(out, eager)


@pytest.mark.gpu
def test_evaluate_videos_jf_on_one_rank():
    from rmnet_amd import inference
    shapes = [(5, 2, 37, 70), (4, 3, 50, 96), (6, 1, 24, 130)]
    videos = []
    for i, (N, K, H, W) in enumerate(shapes):
        _, gt = blob_maps(N, K, H, W, seed=2 + i)
        videos.append({'frames': torch.zeros(N, 3, H, W), 'labels': t8(gt), 'n_objects': K})
    segment_fn = lambda v: torch.roll(v['labels'].to('cuda'), 2, dims=2)
    got = inference.evaluate_videos_jf(videos, segment_fn, rank=0, world_size=1)
    assert set(got) == {'J-Mean', 'F-Mean', 'JF-Mean'}
    assert got['J-Mean'] == inference.evaluate_videos(videos, segment_fn, rank=0, world_size=1)
    fs = []
    for (N, K, H, W), v in zip(shapes, videos):
        gt = v['labels'].numpy()
        f = br.f_of_counts(br.counts_of_labels(np.roll(gt, 2, axis=2), gt, K, int(br.boundary_radius((H, W)))))
        fs.append(f[1:-1].reshape(-1))
    assert abs(got['F-Mean'] - np.concatenate(fs).mean()) <= 1e-12
    assert got['JF-Mean'] == (got['J-Mean'] + got['F-Mean']) / 2
    assert 0 < got['F-Mean'] < 1 and 0 < got['J-Mean'] < 1
