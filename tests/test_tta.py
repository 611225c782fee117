# -*- coding: utf-8 -*-
"""Multi-scale and flipped inference on the device (csrc/tta.hip, rmnet_amd.tta, inference.segment_video_tta; include/rmnet_hip.h H1).

The chain of evidence: hand-checkable exact cases and a per-element comparison with torch's own CPU bilinear kernel pin the numpy
restatement tests/tta_ref.py; the restatement then judges, bit for bit, the torch fallback of rmnet_amd.tta (CPU tests) and the two
kernels (GPU tests) on the cases of tta_ref.py.  Copies of the restatement with one planted fault each must differ from it on named
cases, which shows that the cases can see the fault.  The driver is checked against the outputs recorded from the reference's own
multi_scale_inference (tests/golden/multi_scale_inference.npz) and against the single-scale path."""

import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tta_ref as ref
from conftest import GOLDEN

gpu = pytest.mark.gpu
F32 = np.float32
FACTORS = (0.5, 0.6, 0.75, 1.0, 1.25, 1.3, 1.5, 2.0)


def dev():
    return torch.device('cuda', 0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def to_np(t):
    return t.detach().cpu().numpy()


# ================================================================================================ CPU: the restatement
def test_same_size_returns_the_input_bits():
    x = ref.plane(1, 2, 7, 9)
    assert same(ref.resize_factor(x, 1.0), x)
    assert same(ref.resize(x, 7, 9, ref.scale_for_size(7, 7), ref.scale_for_size(9, 9)), x)
    mean, labels = ref.merge([x[None]], [False], 7, 9)
    assert same(mean, x[None]) and same(labels, np.argmax(x[None], axis=1).astype(np.uint8))


def test_exact_resizes_of_small_integer_planes():
    """x2, x4 and x0.5 of small integers: every weight is a multiple of 1/8, every product and sum exact, so the expected arrays are
    the real-number bilinear values and are given literally."""
    x = np.array([[0, 8], [16, 40]], F32)
    want2 = np.array([[0, 2, 6, 8],
                      [4, 7, 13, 16],
                      [12, 17, 27, 32],
                      [16, 22, 34, 40]], F32)
    assert same(ref.resize_factor(x, 2.0), want2)
    assert same(ref.resize_factor(x, 2.0, flip=True), want2[:, ::-1])
    row = np.array([[0, 8]], F32)
    assert same(ref.resize_factor(row, 4.0), np.array([[0, 0, 1, 3, 5, 7, 8, 8]] * 4, F32))
    y = np.array([[1, 3, 5, 7], [9, 11, 13, 15], [2, 4, 6, 8], [10, 12, 14, 16]], F32)
    assert same(ref.resize_factor(y, 0.5), np.array([[6, 10], [7, 11]], F32))
    assert same(ref.resize_factor(y, 0.5, flip=True), np.array([[10, 6], [11, 7]], F32))
    # the two ends of an axis: the first and last output pixels of an upsampling clamp to the border pixel
    col = np.array([[0], [8]], F32)
    assert same(ref.resize_factor(col, 2.0), np.array([[0, 0], [2, 2], [6, 6], [8, 8]], F32))


def test_exact_means_of_integer_planes():
    for E in (2, 4, 8):
        planes = [np.full((1, 2, 2, 3), 0, F32) for _ in range(E)]
        for e, p in enumerate(planes):
            p[:, 0] = 8 * (e + 1)                       # sum 8 * E (E + 1) / 2, mean 4 (E + 1)
            p[:, 1, :, e % 3] = 8 * E                   # plane 1 wins in some columns
        mean, labels = ref.merge(planes, [False] * E, 2, 3)
        want = sum(p.astype(np.float64) for p in planes) / E
        assert same(mean, want.astype(F32)) and (want == np.round(want)).all() and float(mean[0, 0, 0, 0]) == 4 * (E + 1)
        assert same(labels, np.argmax(want, axis=1).astype(np.uint8))
    # a flipped entry is read mirrored
    a = np.arange(6, dtype=F32).reshape(1, 1, 2, 3)
    mean, _ = ref.merge([a, a], [False, True], 2, 3)
    assert same(mean, np.full((1, 1, 2, 3), 0, F32) + np.array([[1, 1, 1], [4, 4, 4]], F32))


def _window(x, i0, i1, axis_):
    """Per output index along one axis: the smallest and largest source value among the positions i0 - 1 .. i1 + 1 (clipped)."""
    n = x.shape[axis_]
    lo = np.take(x, np.clip(i0 - 1, 0, n - 1), axis=axis_)
    hi = lo.copy()
    for idx in (i0, i1, np.clip(i1 + 1, 0, n - 1)):
        v = np.take(x, idx, axis=axis_)
        lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return lo, hi


def torch_bound(x, out_h, out_w, scale_h, scale_w):
    """The per-element bound of the comparison with torch's CPU kernel, which forms its source coordinates with fused operations.

    Both sides compute s = scale * (d + 0.5) - 0.5 in fp32; one rounds the product and the difference, the other may round once, and
    torch may also have rounded its scale another way by an ulp.  The two coordinates of an output pixel therefore differ by a few
    ulp of the largest coordinate of the axis; 'a few' is taken as 4: u = 4 * spacing(fl32(in)).  l1 = s - i0 is exact on both sides.
    A change of the coordinate by u moves the interpolated value by at most u times the largest difference between neighbouring
    source pixels -- also when it moves s across an integer, where (i0, l1 ~ 0) and (i0 - 1, l1 ~ 1) describe nearly the same point;
    hence the window i0 - 1 .. i1 + 1 per axis, whose range (max - min) bounds every such difference.  That gives u_x * range +
    u_y * range.  The value itself is four levels of rounded operations on either side (product, sum, product, sum), each within
    2^-24 relative of a quantity no larger than the largest |neighbour|: at most 4 * 2^-24 per side, 4 * 2^-23 = 4 eps between them.
    Returns bound [..., out_h, out_w]."""
    Hs, Ws = x.shape[-2:]
    y0, y1, _, _ = ref.axis(out_h, Hs, scale_h)
    x0, x1, _, _ = ref.axis(out_w, Ws, scale_w)
    lo_y, hi_y = _window(x, y0, y1, -2)
    lo = _window(lo_y, x0, x1, -1)[0]
    hi = _window(hi_y, x0, x1, -1)[1]
    rng = (hi - lo).astype(np.float64)
    largest = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
    u_y, u_x = 4.0 * float(np.spacing(F32(Hs))), 4.0 * float(np.spacing(F32(Ws)))
    return (u_x + u_y) * rng + 4.0 * float(np.finfo(F32).eps) * largest


def test_the_restatement_against_torchs_cpu_kernel_within_a_derived_per_element_bound():
    """F.interpolate on the CPU with every scale factor, and with size= going back to the source's size.  No equal bits are asked
    for (see torch_bound); at fs = 1.0 the two are equal."""
    worst = 0.0
    for i, (H, W) in enumerate(((30, 53), (37, 66), (33, 64))):
        x = ref.plane(10 + i, 2, 3, H, W)
        for fs in FACTORS:
            mine = ref.resize_factor(x, fs)
            theirs = F.interpolate(torch.from_numpy(x), scale_factor=fs, mode='bilinear', align_corners=False).numpy()
            assert mine.shape == theirs.shape, (H, W, fs)
            sc = ref.scale_for_factor(fs)
            err = np.abs(mine.astype(np.float64) - theirs)
            bound = torch_bound(x, mine.shape[-2], mine.shape[-1], sc, sc)
            assert (err <= bound).all(), (H, W, fs, float(err.max()), float((err - bound).max()))
            if fs == 1.0:
                assert same(mine, theirs)
            back = ref.resize(mine, H, W, ref.scale_for_size(mine.shape[-2], H), ref.scale_for_size(mine.shape[-1], W))
            theirs_back = F.interpolate(torch.from_numpy(mine), size=(H, W), mode='bilinear', align_corners=False).numpy()
            err_b = np.abs(back.astype(np.float64) - theirs_back)
            bound_b = torch_bound(mine, H, W, ref.scale_for_size(mine.shape[-2], H), ref.scale_for_size(mine.shape[-1], W))
            assert (err_b <= bound_b).all(), (H, W, fs, float(err_b.max()))
            worst = max(worst, float(err.max()), float(err_b.max()))
    print('largest difference from torch: %.3e' % worst)


def test_output_sizes_equal_torchs_for_every_size_and_factor():
    from rmnet_amd import tta
    for fs in FACTORS:
        for h in range(1, 71):
            for w in range(1, 71):
                want = ref.scaled_size(h, w, fs)
                assert tta.scaled_size(h, w, fs) == want
                if min(want) < 1:
                    with pytest.raises(RuntimeError):
                        F.interpolate(torch.zeros(1, 1, h, w), scale_factor=fs, mode='nearest')
                    continue
                # (the size rule does not depend on the mode; nearest is the cheapest way to ask torch 39 200 times)
                assert tuple(F.interpolate(torch.zeros(1, 1, h, w), scale_factor=fs, mode='nearest').shape[-2:]) == want, (h, w, fs)
    for fs in FACTORS:      # and the bilinear mode itself on one size per factor
        assert tuple(F.interpolate(torch.zeros(1, 1, 37, 66), scale_factor=fs, mode='bilinear', align_corners=False).shape[-2:]) == \
            tta.scaled_size(37, 66, fs)
    with pytest.raises(RuntimeError):
        tta.resize_bilinear(torch.zeros(1, 1, 1), 0.5)


# ================================================================================================ CPU: the fallback
def _check_against_the_restatement(device, contiguous=True):
    from rmnet_amd import tta

    def t(a):
        x = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        if contiguous:
            return x
        wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=x.dtype, device=device)
        wide[..., ::2] = x
        return wide[..., ::2]

    for name, x, fs, flip in ref.resize_cases():
        got = tta.resize_bilinear(t(x), fs, flip)
        assert got.is_contiguous() and same(to_np(got), ref.resize_factor(x, fs, flip)), name
    for name, sources, flipped, H, W in ref.merge_cases() + [('order',) + ref.order_case()]:
        want_mean, want_labels = ref.merge(sources, flipped, H, W)
        mean, labels = tta.merge([t(s) for s in sources], flipped, (H, W))
        assert same(to_np(mean), want_mean), name
        assert same(to_np(labels), want_labels), name
        mean, labels = tta.merge([t(s) for s in sources], flipped, (H, W), want_labels=False)
        assert labels is None and same(to_np(mean), want_mean), name


def test_the_torch_fallback_equals_the_restatement_on_the_cpu():
    _check_against_the_restatement(torch.device('cpu'))
    _check_against_the_restatement(torch.device('cpu'), contiguous=False)


def test_the_python_entries_check_their_arguments():
    from rmnet_amd import ops, tta
    x = torch.zeros(1, 2, 4, 4)
    with pytest.raises(RuntimeError):
        tta.merge([x] * 9, [False] * 9, (4, 4))
    with pytest.raises(RuntimeError):
        tta.merge([x], [False, True], (4, 4))
    with pytest.raises(RuntimeError):
        tta.merge([x, torch.zeros(1, 3, 4, 4)], [False, False], (4, 4))
    with pytest.raises(RuntimeError):
        tta.merge([torch.zeros(1, 256, 2, 2)], [False], (2, 2))
    with pytest.raises(RuntimeError):
        tta.resize_bilinear(x, float('nan'))
    with pytest.raises(RuntimeError):
        tta.resize_bilinear(x, 0.0)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.resize_bilinear(x, 4, 4, 1.0, 1.0)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.tta_merge([x], [False], 4, 4)


# ================================================================================================ CPU: planted faults
def test_each_planted_fault_is_caught_by_a_named_case():
    def differs(case, fault):
        kind, args = case
        if kind == 'resize':
            return not same(ref.resize_factor(*args), ref.resize_factor(*args, fault=fault))
        got, want = ref.merge(*args, fault=fault), ref.merge(*args)
        return not (same(got[0], want[0]) and same(got[1], want[1]))

    resize = {name: ('resize', (x, fs, flip)) for name, x, fs, flip in ref.resize_cases()}
    merge = {name: ('merge', (s, f, H, W)) for name, s, f, H, W in ref.merge_cases()}
    merge['order'] = ('merge', ref.order_case())
    named = {
        'i1_unclamped': [resize['1x3x2 fs=2 flip=0'], merge['W=4']],                 # the last output pixels of an upsampling
        'no_half_offset': [resize['1x2x2 fs=0.5 flip=0'], merge['W=5']],
        'flip_wrong_side': [resize['2x30x53 fs=0.6 flip=1'], merge['W=65']],         # equal in real numbers, not in fp32
        'reciprocal_mean': [merge['W=63']],                                         # three entries: x * fl(1/3) != x / 3
        'reversed_order': [merge['order']],
        'last_argmax': [merge['ties']],
        'swapped_scales': [merge['one-row and one-column sources']],                 # (a resize by one factor has one scale)
    }
    assert sorted(named) == sorted(ref.FAULTS)
    for fault, cases in named.items():
        for case in cases:
            assert differs(case, fault), fault
    # no fault planted: the copy is the restatement
    for case in list(resize.values()) + list(merge.values()):
        assert not differs(case, None)
    # the order case is order-sensitive in fp32 itself
    s, f, H, W = ref.order_case()
    assert float(ref.merge(s, f, H, W)[0].ravel()[0]) * 3 != float(ref.merge(s[::-1], f, H, W)[0].ravel()[0]) * 3


# ================================================================================================ CPU: the C entries
def test_the_argument_rules_of_the_c_entries_hold_without_a_launch():
    """Every call below is refused on the host with RMNET_E_INVALID_ARG (a return of -3 would mean that a launch was attempted).  The
    device pointers are placeholders: an entry that is going to refuse never reads them."""
    from rmnet_amd import _lib
    lib = _lib.load()
    INVALID = -1
    p = ctypes.c_void_p(1 << 20)
    resize = lib.rmnet_resize_bilinear_f32
    assert resize(None, 1, 2, 2, 2, 2, 1.0, 1.0, 0, p, None) == INVALID
    assert resize(p, 1, 2, 2, 2, 2, 1.0, 1.0, 0, None, None) == INVALID
    for sizes in ((0, 2, 2, 2, 2), (1, 0, 2, 2, 2), (1, 2, 0, 2, 2), (1, 2, 2, 0, 2), (1, 2, 2, 2, -1)):
        assert resize(p, *sizes, 1.0, 1.0, 0, p, None) == INVALID, sizes
    for bad in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
        assert resize(p, 1, 2, 2, 2, 2, bad, 1.0, 0, p, None) == INVALID, bad
        assert resize(p, 1, 2, 2, 2, 2, 1.0, bad, 0, p, None) == INVALID, bad

    def merge(E=2, N=1, K=2, H=4, W=4, ptrs=None, hs=None, ws=None, mean=p, labels=p, tables=(True,) * 4):
        n = max(E, 1)
        a_p = (ctypes.c_void_p * n)(*(ptrs or [1 << 20] * n))
        a_h = (ctypes.c_int * n)(*(hs or [3] * n))
        a_w = (ctypes.c_int * n)(*(ws or [3] * n))
        a_f = (ctypes.c_int * n)(*([0, 1] * n)[:n])
        arrays = [ctypes.cast(a, ctypes.c_void_p) if keep else None for a, keep in zip((a_p, a_h, a_w, a_f), tables)]
        return lib.rmnet_tta_merge_f32(*arrays, E, N, K, H, W, mean, labels, None)

    for i in range(4):
        assert merge(tables=tuple(j != i for j in range(4))) == INVALID
    assert merge(mean=None) == INVALID
    assert merge(ptrs=[1 << 20, None]) == INVALID
    for kw in (dict(N=0), dict(H=0), dict(W=-3), dict(hs=[3, 0]), dict(ws=[0, 3]), dict(E=0), dict(E=-1), dict(E=9), dict(K=0),
               dict(K=256)):
        assert merge(**kw) == INVALID, kw


# ================================================================================================ GPU: the kernels
GUARD = 64                     # floats (bytes for the label buffer) on either side of a guarded slice
SENTINEL = -12345.0


def _guarded(n, dtype=torch.float32):
    """A pre-filled buffer and a contiguous slice of ``n`` elements that starts one element past a 16-byte boundary."""
    fill = SENTINEL if dtype == torch.float32 else 0xA5
    store = torch.full((n + 2 * GUARD + 1,), fill, dtype=dtype, device=dev())
    view = store[GUARD + 1:GUARD + 1 + n]
    assert view.data_ptr() % 16 == (4 if dtype == torch.float32 else 1)
    return store, view


def _guard_untouched(store, n):
    s = to_np(store)
    fill = s.dtype.type(SENTINEL if s.dtype == F32 else 0xA5)
    return bool((s[:GUARD + 1] == fill).all() and (s[GUARD + 1 + n:] == fill).all())


@gpu
def test_the_kernels_equal_the_restatement_on_every_case():
    """Contiguous float32 tensors on the GPU: both kernels on the cases of tta_ref (see resize_cases and merge_cases for the branches
    they reach), every bit; and strided views, which take the fallback on the device."""
    _check_against_the_restatement(dev())
    _check_against_the_restatement(dev(), contiguous=False)


@gpu
def test_misaligned_base_pointers_and_untouched_guards():
    """Sources and results as slices of guarded, pre-filled buffers that start one float (one byte for the labels) past a 16-byte
    boundary: the vector stores must not be taken, and nothing outside the slices may change."""
    from rmnet_amd import ops
    for name, x, fs, flip in ref.resize_cases():
        want = ref.resize_factor(x, fs, flip)
        s_store, s_view = _guarded(x.size)
        s_view.copy_(torch.from_numpy(x).reshape(-1))
        d_store, d_view = _guarded(want.size)
        sc = float(ref.scale_for_factor(fs))
        got = ops.resize_bilinear(s_view.view(x.shape), want.shape[-2], want.shape[-1], sc, sc, flip, out=d_view.view(want.shape))
        assert same(to_np(got), want), name
        assert _guard_untouched(d_store, want.size) and _guard_untouched(s_store, x.size), name
    for name, sources, flipped, H, W in ref.merge_cases():
        want_mean, want_labels = ref.merge(sources, flipped, H, W)
        held = []
        for s in sources:
            store, view = _guarded(s.size)
            view.copy_(torch.from_numpy(s).reshape(-1))
            held.append((store, view.view(s.shape)))
        m_store, m_view = _guarded(want_mean.size)
        l_store, l_view = _guarded(want_labels.size, torch.uint8)
        mean, labels = ops.tta_merge([v for _, v in held], flipped, H, W, True, m_view.view(want_mean.shape), l_view.view(want_labels.shape))
        assert same(to_np(mean), want_mean) and same(to_np(labels), want_labels), name
        assert _guard_untouched(m_store, want_mean.size) and _guard_untouched(l_store, want_labels.size), name
        assert all(_guard_untouched(store, v.numel()) for store, v in held), name
        # without labels the label buffer keeps every byte
        l_store.fill_(0xA5)
        m_store.fill_(SENTINEL)
        mean, none = ops.tta_merge([v for _, v in held], flipped, H, W, False, m_view.view(want_mean.shape), l_view.view(want_labels.shape))
        assert none is None and same(to_np(mean), want_mean), name
        assert bool((l_store == 0xA5).all()) and _guard_untouched(m_store, want_mean.size), name


@gpu
def test_the_labels_are_those_of_the_argmax_kernel_on_the_mean():
    from rmnet_amd import clip_io, tta
    for name, sources, flipped, H, W in ref.merge_cases():
        mean, labels = tta.merge([torch.from_numpy(s).to(dev()) for s in sources], flipped, (H, W))
        assert mean.is_cuda and labels.dtype == torch.uint8 and torch.equal(labels, clip_io.argmax_labels(mean)), name


@gpu
def test_one_graph_replay_of_each_entry_gives_the_same_bytes():
    from rmnet_amd import ops
    x = ref.plane(7, 3, 30, 53)
    sources, flipped = ref._entries(8, 2, 3, 12, 20, 4)
    t_x = torch.from_numpy(x).to(dev())
    t_src = [torch.from_numpy(s).to(dev()) for s in sources]
    sc = float(ref.scale_for_factor(1.3))
    h, w = ref.scaled_size(30, 53, 1.3)

    def run():
        return (ops.resize_bilinear(t_x, h, w, sc, sc, True),) + ops.tta_merge(t_src, flipped, 12, 20)

    first = [to_np(o) for o in run()]
    want = [ref.resize_factor(x, 1.3, True), *ref.merge(sources, flipped, 12, 20)]
    assert all(same(a, b) for a, b in zip(first, want))
    stream = torch.cuda.Stream(device=dev())
    stream.wait_stream(torch.cuda.current_stream(dev()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            outs = run()
        t_x.copy_(torch.flip(t_x, dims=[0]) * 0.5)        # other inputs than the captured call saw
        for s in t_src:
            s.neg_()
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(dev()).wait_stream(stream)
    x2 = np.ascontiguousarray(x[::-1]) * F32(0.5)
    want = [ref.resize_factor(x2, 1.3, True), *ref.merge([-s for s in sources], flipped, 12, 20)]
    assert all(same(to_np(a), b) for a, b in zip(outs, want))


# ================================================================================================ GPU: the driver
class _Recorder:
    """Stands where the network stands and keeps what went in and what came out."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, frames, masks, flows, n_objects, memorize_every, **kw):
        est = self.net(frames, masks, flows, n_objects, memorize_every, **kw)
        self.calls.append({'frames': frames, 'masks': masks, 'flows': flows, 'n_objects': n_objects, 'memorize_every': memorize_every,
                           'est': est})
        return est


class _PerPixelNet(torch.nn.Module):
    """A stand-in network whose output is a fixed elementwise function of the frames and of the first frame's masks: the same bits
    for the same inputs at any batch size, with many exact ties between the planes."""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def forward(self, frames, masks, flows, n_objects, memorize_every, device=None):
        K = masks.shape[2]
        first = masks.to(frames.device)[:, :1].float()
        planes = torch.arange(K, device=frames.device, dtype=torch.float32).view(1, 1, K, 1, 1)
        return torch.softmax(first + torch.floor(frames[:, :, :1] * 2.0) * torch.remainder(planes, 2.0), dim=2)


def _no_flow(clip):
    return torch.zeros(clip.shape[0], clip.shape[1], 2, clip.shape[3], clip.shape[4], device=clip.device)


def _library_reproducible():
    """The library's convolutions with reproducible solvers, as tests/test_clip_io.py asks for them."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _networks():
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.tiny_flownet import TinyFlowNet
    return (networks.procedural_init_(RMNet(None)).to(dev()).eval(), networks.procedural_init_(TinyFlowNet(None)).to(dev()).eval())


@gpu
@pytest.mark.parametrize('pair_flips', [True, False])
def test_the_driver_matches_the_recorded_outputs_of_the_reference(pair_flips):
    """The clip and weights of cases.MSI_CLIP against the reference's own multi_scale_inference (recorded, not regenerated), with the
    tolerances of test_multi_scale_inference_matches_the_reference, for the same reason: the networks' own arithmetic."""
    sys.path.insert(0, GOLDEN)
    import cases
    from rmnet_amd import inference
    from rmnet_amd.synthetic import synthetic_clip
    g = np.load(os.path.join(GOLDEN, 'multi_scale_inference.npz'))
    net, tfn = _networks()
    c = cases.MSI_CLIP
    frames, masks, _, n_objects = synthetic_clip(c['N'], c['K'], c['H'], c['W'], seed=c['seed'], size=c['size'])
    video = {'frames': frames[0], 'masks': masks[0], 'n_objects': int(n_objects.max())}
    assert len(cases.MSI_CASES) == 2
    for name, scales, flip in cases.MSI_CASES:
        out = inference.segment_video_tta(net, tfn, video, scales, flip, c['memorize_every'], pair_flips=pair_flips)
        probs, labels = to_np(out['probs']), to_np(out['labels'])
        assert probs.shape == (c['N'], c['K'], c['H'], c['W']) and labels.shape == (c['N'], c['H'], c['W']) and labels.dtype == np.uint8
        print(name, 'pair_flips', pair_flips, 'largest difference %.3e' % float(np.abs(probs - g[name + '.probs'][0].astype(F32)).max()),
              'argmax agreement %.5f' % float((labels == g[name + '.argmax'][0]).mean()))
        np.testing.assert_allclose(probs, g[name + '.probs'][0].astype(F32), atol=3e-3, err_msg=name)
        assert (labels == g[name + '.argmax'][0]).mean() > 0.999, name
        assert same(labels, np.argmax(probs, axis=1).astype(np.uint8))


def _u8_clip():
    """A 3-frame 96 x 160 synthetic clip as a folder of images would hold it (as in tests/test_clip_io.py)."""
    import clip_io_ref
    from rmnet_amd.synthetic import synthetic_clip
    frames, masks, _, _ = synthetic_clip(3, 3, 96, 160, seed=3, size=1.5)
    mean, std = torch.tensor(clip_io_ref.MEAN).view(1, 3, 1, 1), torch.tensor(clip_io_ref.STD).view(1, 3, 1, 1)
    u8 = ((frames[0] * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    labels = np.asarray([0, 5, 38], np.uint8)[masks[0].argmax(dim=1).numpy()]
    labels[:, :2, :2] = 255
    return u8, labels


@gpu
def test_one_scale_without_flip_is_the_single_scale_path():
    """segment_video_tta(frame_scales=(1.0,), flip_lr=False): the network is handed the bits segment_video hands it (frames, flows,
    first-frame masks, object counts), the probabilities returned are, bit for bit, what the network returned, and the labels are
    segment_video's.  With the per-pixel stand-in the whole statement is checked on the outputs; with RMNet + TinyFlowNet (reproducible
    solvers) a recorder shows the two halves, since two runs of the real networks need not agree in their last bits."""
    import clip_io_ref
    from rmnet_amd import inference
    u8, labels = _u8_clip()
    lut, _ = clip_io_ref.reorganize_lut(labels)
    video = {'frames': torch.from_numpy(clip_io_ref.normalize(u8)), 'masks': torch.from_numpy(clip_io_ref.onehot(labels, 5, lut)).to(dev()),
             'n_objects': 2}
    for net, tfn in ((_PerPixelNet().to(dev()), _no_flow), _networks()):
        net = _Recorder(net)
        with _library_reproducible():
            out = inference.segment_video_tta(net, tfn, video, (1.0,), False, memorize_every=2)
            want = inference.segment_video(net, tfn, video, memorize_every=2)
        mine, theirs = net.calls
        assert same(to_np(mine['frames']), to_np(theirs['frames'])) and same(to_np(mine['flows']), to_np(theirs['flows']))
        assert same(to_np(mine['masks'][:, 0].float()), to_np(theirs['masks'][:, 0].float()))
        assert same(to_np(mine['n_objects']), to_np(theirs['n_objects'])) and mine['memorize_every'] == theirs['memorize_every'] == 2
        assert same(to_np(out['probs']), to_np(mine['est'][0]))
        assert same(to_np(out['labels']), to_np(mine['est'][0].argmax(dim=1).to(torch.uint8)))
        assert same(to_np(out['labels']), to_np(want)) and len(set(to_np(want).ravel().tolist())) >= 2
        if isinstance(net.net, _PerPixelNet):
            assert same(to_np(out['probs']), to_np(theirs['est'][0]))


@gpu
def test_segment_video_u8_keeps_its_default_path_and_takes_the_scales_and_the_flip(monkeypatch):
    import clip_io_ref
    from rmnet_amd import inference
    u8, labels = _u8_clip()
    t_u8, t_labels = torch.from_numpy(u8), torch.from_numpy(labels)
    lut, _ = clip_io_ref.reorganize_lut(labels)
    normalized = clip_io_ref.normalize(u8)
    video = {'frames': torch.from_numpy(normalized), 'masks': torch.from_numpy(clip_io_ref.onehot(labels, 5, lut)).to(dev()), 'n_objects': 2}
    for net, tfn in ((_PerPixelNet().to(dev()), _no_flow), _networks()):
        with _library_reproducible():
            # the defaults: what the call returned before, and the new driver is not entered
            with monkeypatch.context() as m:
                m.setattr(inference, 'segment_video_tta', None)
                got = inference.segment_video_u8(net, tfn, t_u8, t_labels, 4, clip_io_ref.MEAN, clip_io_ref.STD, memorize_every=2)
            want = to_np(inference.segment_video(net, tfn, video, memorize_every=2))
            assert got['n_objects'] == 2 and same(to_np(got['labels']), want)
            assert same(to_np(got['overlay']), clip_io_ref.overlay(normalized, want))
            # scales and flip: the labels of segment_video_tta on the same clip
            got = inference.segment_video_u8(net, tfn, t_u8, t_labels, 4, clip_io_ref.MEAN, clip_io_ref.STD, memorize_every=2,
                                             frame_scales=(0.75, 1.0), flip_lr=True)
            want = to_np(inference.segment_video_tta(net, tfn, video, (0.75, 1.0), True, memorize_every=2)['labels'])
        assert same(to_np(got['labels']), want) and len(set(want.ravel().tolist())) >= 2
        assert same(to_np(got['overlay']), clip_io_ref.overlay(normalized, want))
