# -*- coding: utf-8 -*-
"""The gradients of the decoder's glue (csrc/decoder_glue_bwd.hip): the adjoint of the x2 / x4 bilinear upsample, the backward of the
prediction head, ``ops.upsample2x_add`` / ``ops.pred_head`` / ``ops.upsample4x`` under autograd and ``Decoder.device_grad_(glue=True)``.

CPU part: the float64 restatement (tests/decoder_glue_grad_ref.py) pinned by the literal tap rows, by float64 torch autograd and by
the inner-product identity; the float32 restatement in the kernels' order inside the per-element bounds, and the bounds' power; nine
planted faults; the C entries' refusals; the compiler's resources.
GPU part: exact families (every bit), random families (the per-element bounds), NaN / -0.0 / NULL outputs, determinism and graph
replay, autograd, and the module against float64 with the library route as yardstick, bit-equal from call to call."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decoder_glue_grad_ref as ref
from conftest import ROOT

# the kernels' constants, restated (csrc/decoder_glue_bwd.hip; exported by rmnet_amd.ops)
THREADS, UP_MAX_BLOCKS = 256, 1024
HEAD_CT, HEAD_SLOTS, HEAD_RANGE_MIN, HEAD_MAX_RANGES, HEAD_TARGET_WGS = 32, 32, 256, 128, 1024
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
NAN = float('nan')
MAPS = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 3), (1, 7), (7, 1), (4, 33)]
# the prediction head walks pixels in groups of HEAD_SLOTS = 32 and cuts one range per HEAD_RANGE_MIN = 256 pixels or part of them:
# its own edges are 32 / 33 pixels (one group, one group + 1) and 256 / 257 pixels (one range; two ranges of 160 and 97)
HEAD_MAPS = [(1, 1), (1, 5), (3, 1), (2, 3), (15, 31), (17, 33), (1, 32), (1, 33), (16, 16), (1, 257)]


def dev():
    return torch.device('cuda', 0)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def torch_adjoint64(g, S):
    """float64 torch autograd through F.interpolate."""
    g = torch.as_tensor(np.asarray(g, np.float64))
    x = torch.zeros(g.shape[0], g.shape[1], g.shape[2] // S, g.shape[3] // S, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=S, mode='bilinear', align_corners=False).backward(g)
    return x.grad.numpy()


def torch_head64(x, w, g):
    x, w = (torch.as_tensor(np.asarray(t, np.float64)).requires_grad_(True) for t in (x, w))
    b = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.relu(x), w, b, padding=1).backward(torch.as_tensor(np.asarray(g, np.float64)))
    return x.grad.numpy(), w.grad.numpy(), b.grad.numpy()


def rng(seed):
    return np.random.default_rng(seed)


def head_case(seed, n, C, H, W, integers=False):
    r = rng(seed)
    if integers:
        return (r.integers(-4, 5, (n, C, H, W)).astype(np.float32), r.integers(-2, 3, (2, C, 3, 3)).astype(np.float32),
                r.integers(-2, 3, (n, 2, H, W)).astype(np.float32))
    return (r.standard_normal((n, C, H, W)).astype(np.float32), (r.standard_normal((2, C, 3, 3)) * 0.1).astype(np.float32),
            (r.standard_normal((n, 2, H, W)) * 10.0 ** r.integers(-6, 1, (n, 2, H, W))).astype(np.float32))


# ================================================================================================ CPU 1: the restatement
def test_the_constants_are_the_ones_ops_exports_and_the_plan_is_what_it_says():
    from rmnet_amd import ops
    assert (ops.GLUE_THREADS, ops.UPSAMPLE_BWD_MAX_BLOCKS) == (THREADS, UP_MAX_BLOCKS)
    assert (ops.PRED_BWD_CT, ops.PRED_BWD_SLOTS, ops.PRED_BWD_RANGE_MIN, ops.PRED_BWD_MAX_RANGES, ops.PRED_BWD_TARGET_WGS) == \
        (HEAD_CT, HEAD_SLOTS, HEAD_RANGE_MIN, HEAD_MAX_RANGES, HEAD_TARGET_WGS)
    for pixels, C in ((1, 32), (32, 32), (33, 64), (256, 256), (257, 32), (465, 32), (465, 256), (73728, 256), (10 ** 6, 1024)):
        assert ops.pred_head_backward_plan(pixels, C) == ref.head_plan(pixels, C)
    assert ref.head_plan(465, 32) == (1, 2, 256)                  # two ranges, the last one ragged: 209 pixels
    assert ref.head_plan(257, 32) == (1, 2, 160) and ref.head_plan(256, 32) == (1, 1, 256)
    assert ref.head_plan(73728, 256) == (8, 128, 576)


def test_the_tap_rows_are_the_literal_ones():
    rows = lambda n, S: [ref.adj_row(j, n, S) for j in range(n)]
    assert rows(1, 2) == [[(0, 1.0), (1, 1.0)]]
    assert rows(2, 2) == [[(0, 1.0), (1, 0.75), (2, 0.25)], [(1, 0.25), (2, 0.75), (3, 1.0)]]
    assert rows(3, 2) == [[(0, 1.0), (1, 0.75), (2, 0.25)], [(1, 0.25), (2, 0.75), (3, 0.75), (4, 0.25)], [(3, 0.25), (4, 0.75), (5, 1.0)]]
    assert rows(4, 2)[1] == [(1, 0.25), (2, 0.75), (3, 0.75), (4, 0.25)] and rows(4, 2)[2] == [(3, 0.25), (4, 0.75), (5, 0.75), (6, 0.25)]
    assert rows(4, 2)[0] == rows(3, 2)[0] and rows(4, 2)[3] == [(5, 0.25), (6, 0.75), (7, 1.0)]
    inner = [0.125, 0.375, 0.625, 0.875, 0.875, 0.625, 0.375, 0.125]
    assert rows(1, 4) == [[(0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0)]]
    first = [(0, 1.0), (1, 1.0), (2, 0.875), (3, 0.625), (4, 0.375), (5, 0.125)]
    assert rows(2, 4) == [first, [(2, 0.125), (3, 0.375), (4, 0.625), (5, 0.875), (6, 1.0), (7, 1.0)]]
    assert rows(3, 4)[0] == first and rows(3, 4)[1] == list(zip(range(2, 10), inner))
    assert rows(3, 4)[2] == [(6, 0.125), (7, 0.375), (8, 0.625), (9, 0.875), (10, 1.0), (11, 1.0)]
    assert rows(4, 4)[2] == list(zip(range(6, 14), inner)) and rows(4, 4)[3] == [(d + 4, v) for d, v in rows(3, 4)[2]]
    for S in (2, 4):
        for n in (1, 2, 3, 4, 5):
            assert np.array_equal(ref.adj_matrix(n, S).sum(axis=1), np.full(n, float(S)))       # every weight sums to S per axis
            assert np.array_equal(ref.adj_matrix(n, S).sum(axis=0), np.ones(S * n))              # and every fine index is spent once


@pytest.mark.parametrize('S', [2, 4])
def test_the_adjoint_is_torch_autograd_in_float64_and_the_transpose_of_the_forward(S):
    for seed, (h, w) in enumerate(MAPS + [(3, 3), (5, 5)]):
        r = rng(seed)
        g = r.standard_normal((2, 3, S * h, S * w))
        got, want = ref.upsample_adjoint64(g, S), torch_adjoint64(g, S)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (h, w)
        x = r.standard_normal((2, 3, h, w))
        up = ref.upsample64(x, S)
        assert np.abs(up - F.interpolate(torch.as_tensor(x), scale_factor=S, mode='bilinear', align_corners=False).numpy()).max() <= 1e-12
        lhs, rhs = (up * g).sum(), (x * got).sum()                # <up(x), g> == <x, up^T g>
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), (np.abs(up) * np.abs(g)).sum())


def test_the_head_restatement_is_torch_autograd_in_float64_and_gives_the_hand_written_answers():
    for seed, (n, C, H, W) in enumerate([(1, 2, 1, 1), (2, 3, 1, 5), (1, 2, 3, 1), (2, 4, 4, 5), (1, 32, 3, 7)]):
        x, w, g = head_case(seed, n, C, H, W)
        for got, want, name in zip(ref.head_grads64(x, w, g), torch_head64(x, w, g), ('dx', 'dw', 'db')):
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (name, n, C, H, W)
    # one live pixel of g at (1, 2) of a 3 x 4 map, one channel, x = 1 everywhere but a -1 and a NaN
    x = np.ones((1, 1, 3, 4))
    x[0, 0, 0, 1], x[0, 0, 2, 3] = -1.0, NAN
    w = np.arange(1.0, 19.0).reshape(2, 1, 3, 3)
    g = np.zeros((1, 2, 3, 4))
    g[0, 0, 1, 2], g[0, 1, 1, 2] = 1.0, 10.0
    dx, dw, db = ref.head_grads64(x, w, g)
    # out[1][2] reads x[1 + ky - 1][2 + kx - 1] with w[ky][kx]: dx[y][x] = w[y][x - 1], both planes: 1 + 10 * 10 ...
    want = np.zeros((3, 4))
    for ky in range(3):
        for kx in range(3):
            want[ky, 1 + kx] = w[0, 0, ky, kx] + 10.0 * w[1, 0, ky, kx]
    want[0, 1] = want[2, 3] = 0.0                                 # the negative and the NaN: mask 0
    assert np.array_equal(dx[0, 0], want)
    relu = np.where(x > 0, x, 0.0)[0, 0]
    assert np.array_equal(dw[0, 0], relu[0:3, 1:4]) and np.array_equal(dw[1, 0], 10.0 * relu[0:3, 1:4])     # the NaN counted nowhere
    assert np.array_equal(db, [1.0, 10.0])


# ================================================================================================ CPU 2: planted faults
def _up_fault_case(fault):
    S, h, w = {'border_interior': (2, 3, 4), 'no_fold_n1': (2, 1, 1), 'no_fold_n2': (4, 2, 2), 'swap_xy_x4': (4, 3, 5)}[fault]
    g = rng(7).standard_normal((1, 2, S * h, S * w))
    return S, g


@pytest.mark.parametrize('fault', ref.UP_FAULTS)
def test_a_planted_fault_in_the_adjoint_is_caught(fault):
    S, g = _up_fault_case(fault)
    want = torch_adjoint64(g, S)
    assert np.abs(ref.upsample_adjoint64(g, S) - want).max() <= 1e-12 * np.abs(want).max()
    bad = ref.upsample_adjoint64(g, S, fault=fault)
    assert np.abs(bad - want).max() > 1e-2 * np.abs(want).max(), fault
    assert (np.abs(bad - want) > ref.upsample_bound(g, S)).any()


@pytest.mark.parametrize('fault', [f for f in ref.HEAD_FAULTS if f != 'drop_range'])
def test_a_planted_fault_in_the_head_gradients_is_caught(fault):
    x, w, g = head_case(11, 2, 32, 4, 5, integers=(fault == 'mask_ge'))         # (integers: x holds exact zeros)
    want = torch_head64(x, w, g)
    bad = ref.head_grads64(x, w, g, fault=fault)
    bounds = ref.head_bounds(x, w, g)
    which = 1 if fault == 'dw_no_relu' else 0
    assert (np.abs(bad[which] - want[which]) > bounds[which]).any(), fault
    assert np.abs(bad[which] - want[which]).max() > 1e-2 * np.abs(want[which]).max()
    for k in range(3):
        if k != which:
            assert np.abs(bad[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max()


def test_a_partial_range_dropped_from_the_merge_is_caught():
    x, w, g = head_case(12, 1, 32, 15, 31)
    assert ref.head_plan(15 * 31, 32)[1] == 2
    truth, bounds = ref.head_grads64(x, w, g), ref.head_bounds(x, w, g)
    good, bad = ref.head_grads32(x, w, g), ref.head_grads32(x, w, g, fault='drop_range')
    for k in (1, 2):
        assert (np.abs(good[k] - truth[k]) <= bounds[k]).all()
        assert (np.abs(bad[k] - truth[k]) > bounds[k]).any()
    assert np.array_equal(good[0], bad[0])


# ================================================================================================ CPU 3: the bounds and their power
def _up_random(seed, N, C, h, w, S):
    r = rng(seed)
    return (r.standard_normal((N, C, S * h, S * w)) * 10.0 ** r.integers(-6, 1, (N, C, S * h, S * w))).astype(np.float32)


@pytest.mark.parametrize('S', [2, 4])
def test_the_float32_adjoint_is_within_its_bound_and_the_bound_has_power(S):
    """The bound is (T + 2) 2^-24 sum w |g|: one rounding per addition on any path (T = 16 / 64) and two products.

    Its power.  The planted 0.75 -> 0.7499999 (float32: 0.75 - 2^-23) moves a weight by 2.7 units of 2^-24 relative; an element of the
    x2 adjoint holds at most two such factors, so the fault moves an element by at most 5.4 units of 2^-24 sum w |g| -- and the bound
    grants 18.  No rounding bound of this form can reject it (even the count of roundings on the kernel's own path, 8, is above 5.4):
    that fault is caught where the arithmetic is exact, by the integer family, which is asserted here on the restatement (measured on
    the map below: the fault moves an element by at most 3.92 units).  What the random family's bound does reject is shown with the same weight moved by
    2^-12: outside the bound for a gradient of one sign."""
    for seed, (h, w) in enumerate(MAPS):
        g = _up_random(seed, 2, 3, h, w, S)
        err = np.abs(ref.upsample_adjoint32(g, S).astype(np.float64) - ref.upsample_adjoint64(g, S))
        assert (err <= ref.upsample_bound(g, S)).all(), (h, w)
    if S != 2:
        return
    g = rng(3).integers(-8, 9, (1, 2, 10, 14)).astype(np.float32)
    want = ref.upsample_adjoint64(g, 2)
    assert np.array_equal(ref.upsample_adjoint32(g, 2), want)                                  # exact in float32, any order
    planted = ref.upsample_adjoint32(g, 2, w75=float(np.float32(0.7499999)))
    units = np.abs(planted - want) / np.maximum(ref.upsample_bound(g, 2) / 18, 1e-300)
    print('0.75 -> 0.7499999: at most %.2f units of 2^-24 sum w |g| (the bound: 18)' % units.max())
    assert not np.array_equal(planted, want) and units.max() <= 5.4
    g = np.abs(_up_random(5, 1, 2, 5, 7, 2))
    coarse = ref.upsample_adjoint32(g, 2, w75=0.75 * (1 - 2.0 ** -12))
    assert (np.abs(coarse - ref.upsample_adjoint64(g, 2)) > ref.upsample_bound(g, 2)).any()


def test_the_float32_head_gradients_are_within_their_bounds_and_the_bounds_have_power():
    """dx: 18 fused multiply-adds, bound 20 units; dw: at most P additions and a product on any path, (P + 2); db: (P + 1).
    Power: every weight moved by 2^-12 relative puts dx outside its bound; x moved by 2^-12 puts dw outside (data of one sign)."""
    for seed, (n, C, H, W) in enumerate([(1, 32, 1, 1), (2, 32, 3, 5), (1, 64, 15, 31), (3, 32, 2, 3)]):
        x, w, g = head_case(seed, n, C, H, W)
        truth, bounds = ref.head_grads64(x, w, g), ref.head_bounds(x, w, g)
        for got, want, b, name in zip(ref.head_grads32(x, w, g), truth, bounds, ('dx', 'dw', 'db')):
            assert (np.abs(got - want) <= b).all(), (name, n, C, H, W)
    x, w, g = (np.abs(t) for t in head_case(9, 1, 32, 6, 7))
    truth, bounds = ref.head_grads64(x, w, g), ref.head_bounds(x, w, g)
    moved = ref.head_grads32(x * np.float32(1 + 2.0 ** -12), w * np.float32(1 + 2.0 ** -12), g)
    assert (np.abs(moved[0] - truth[0]) > bounds[0]).any() and (np.abs(moved[1] - truth[1]) > bounds[1]).any()


# ================================================================================================ CPU 4: refusals, resources, CPU op
def _up_refusals(good):
    inv, uns = E_INVALID, E_UNSUPPORTED
    yield 'null g', dict(g=0), inv
    yield 'null out', dict(out=0), inv
    yield 'N = 0', dict(N=0), inv
    yield 'C < 0', dict(C=-4), inv
    yield 'h = 0', dict(h=0), inv
    yield 'w = 0', dict(w=0), inv
    yield 'factor 3', dict(factor=3), uns
    yield 'factor 1', dict(factor=1), uns
    yield 'factor 8', dict(factor=8), uns
    yield 'nhwc: g off a 16-byte boundary', dict(g=good['g'] + 4), inv
    yield 'nhwc: out off a 16-byte boundary', dict(out=good['out'] + 8), inv
    yield 'nchw: g off a 4-byte boundary', dict(nhwc=0, g=good['g'] + 2), inv
    yield 'nchw: out off a 4-byte boundary', dict(nhwc=0, out=good['out'] + 1), inv
    yield 'nhwc: C % 4', dict(C=6), inv
    yield 'out inside g', dict(out=good['g'] + 64), inv
    yield 'g begins inside out', dict(g=good['out'] + 16), inv
    yield '2^31 elements of g', dict(N=1 << 10, C=1 << 9, h=1 << 5, w=1 << 5), uns
    yield 'far more than 2^63', dict(N=1 << 40, C=1 << 20, h=1 << 20, w=1 << 20), uns


def _up_call(lib, a):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.rmnet_upsample_bwd_f32(p(a['g']), a['N'], a['C'], a['h'], a['w'], a['factor'], a['nhwc'], p(a['out']), None)


def _head_refusals(good):
    inv, uns, wsp = E_INVALID, E_UNSUPPORTED, E_WORKSPACE
    for k in ('x', 'w', 'g'):
        yield 'null ' + k, {k: 0}, inv
    yield 'n = 0', dict(n=0), inv
    yield 'Hq < 0', dict(Hq=-1), inv
    yield 'Wq = 0', dict(Wq=0), inv
    yield 'C = 0', dict(C=0), inv
    for k in ('x', 'w', 'dx', 'ws'):
        yield k + ' off a 16-byte boundary', {k: good[k] + 4}, inv
    for k in ('g', 'dw', 'db'):
        yield k + ' off a 4-byte boundary', {k: good[k] + 2}, inv
    yield 'dx overlaps x', dict(dx=good['x'] + 16), inv
    yield 'dx is x', dict(dx=good['x']), inv
    yield 'dw overlaps g', dict(dw=good['g'] + 4), inv
    yield 'dw overlaps w', dict(dw=good['w']), inv
    yield 'db overlaps dw', dict(db=good['dw'] + 8), inv
    yield 'workspace overlaps dx', dict(ws=good['dx'] + 32), inv
    yield 'workspace overlaps db', dict(db=good['ws'] + 4), inv
    yield 'C % 32', dict(C=48), uns
    yield '2^31 elements', dict(n=1 << 12, Hq=1 << 7, Wq=1 << 7, C=32), uns
    yield 'null workspace', dict(ws=0), wsp
    yield 'null workspace for db alone', dict(ws=0, dx=0, dw=0), wsp
    yield 'short workspace', dict(ws_bytes=good['ws_bytes'] - 1), wsp
    yield 'nothing asked for: nothing launched', dict(dx=0, dw=0, db=0, ws=0), 0


def _head_call(lib, a):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.rmnet_pred_head_bwd_f32(p(a['x']), p(a['w']), p(a['g']), a['n'], a['Hq'], a['Wq'], a['C'], p(a['dx']), p(a['dw']), p(a['db']),
                                       p(a['ws']), a['ws_bytes'], None)


def test_the_entries_refuse_malformed_calls_before_they_touch_the_device():
    """No GPU here: a call that got past the checks would fail to launch or fault on these made-up addresses."""
    from rmnet_amd import _lib
    lib = _lib.load()
    good = dict(g=0x100000, N=1, C=8, h=3, w=5, factor=2, nhwc=1, out=0x200000)
    for name, kw, code in _up_refusals(good):
        assert _up_call(lib, dict(good, **kw)) == code, name
    n, Hq, Wq, C = 1, 15, 31, 32
    nbytes = lib.rmnet_pred_head_bwd_workspace_bytes(n, Hq, Wq, C)
    assert nbytes == 2 * (18 * C + 2) * 4                          # two ranges
    assert lib.rmnet_pred_head_bwd_workspace_bytes(1, 16, 16, 256) == (18 * 256 + 2) * 4
    assert lib.rmnet_pred_head_bwd_workspace_bytes(1, 4, 4, 48) == 0 and lib.rmnet_pred_head_bwd_workspace_bytes(0, 4, 4, 32) == 0
    assert lib.rmnet_pred_head_bwd_workspace_bytes(1 << 12, 1 << 7, 1 << 7, 32) == 0
    base = 0x100000
    good = dict(x=base, w=base + 0x100000, g=base + 0x200000, n=n, Hq=Hq, Wq=Wq, C=C, dx=base + 0x300000, dw=base + 0x400000,
                db=base + 0x500000, ws=base + 0x600000, ws_bytes=nbytes)
    for name, kw, code in _head_refusals(good):
        assert _head_call(lib, dict(good, **kw)) == code, name


def test_the_new_kernels_use_no_scratch_no_spill_and_no_static_lds(tmp_path):
    """From a compile-only gfx950 build: sizes and counts of the metadata, no instruction is looked at."""
    from rmnet_amd import build
    out = str(tmp_path / 'glue.s')
    subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                    os.path.join(ROOT, 'rmnet_amd', 'csrc', 'decoder_glue_bwd.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', open(out).read(), flags=re.S).group(1)
    found = {}
    for entry in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]:
        get = lambda key: re.search(r'^    \.%s:\s+(\S+)' % key, '    ' + entry, flags=re.M)
        if get('name'):
            found[get('name').group(1)] = {k: int(get(k).group(1)) for k in ('group_segment_fixed_size', 'private_segment_fixed_size',
                                                                            'vgpr_count', 'vgpr_spill_count')}
    frags = ['13pred_head_bwdE', '19pred_head_bwd_mergeE', '17upsample_bwd_nhwcILi2EE', '17upsample_bwd_nhwcILi4EE'] + \
        ['17upsample_bwd_nchwILi%dELb%dEE' % (s, v) for s in (2, 4) for v in (0, 1)]
    for frag in frags:
        hits = [k for n, k in found.items() if frag in n]
        assert len(hits) == 1, (frag, sorted(found))
        print(frag, hits[0])
        k = hits[0]
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (frag, k)
    assert len(found) == len(frags), sorted(found)
    assert [k for n, k in found.items() if '13pred_head_bwdE' in n][0]['vgpr_count'] <= 256      # 256 threads: two workgroups per CU
    assert 'decoder_glue_bwd.hip' in build.SOURCES


def test_upsample4x_on_the_cpu_is_the_torch_op():
    from rmnet_amd import ops
    x = torch.randn(2, 2, 3, 5, generator=torch.Generator().manual_seed(0))
    want = F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=False)
    assert torch.equal(ops.upsample4x(x), want)
    xr = x.clone().requires_grad_(True)
    out = ops.upsample4x(xr)
    assert torch.equal(out, want) and 'Upsample4x' not in type(out.grad_fn).__name__
    out.backward(torch.ones_like(out))
    assert torch.allclose(xr.grad, torch.full_like(x, 16.0))


# ================================================================================================ GPU helpers
GUARD = 64


def _guarded(n, d):
    pool = torch.full((n + 2 * GUARD,), NAN, device=d)
    assert pool.data_ptr() % 16 == 0
    return pool, pool[GUARD:GUARD + n]


def _guards_intact(pool, n):
    return bool(torch.isnan(pool[:GUARD]).all()) and bool(torch.isnan(pool[GUARD + n:]).all()) and not bool(torch.isnan(pool[GUARD:GUARD + n]).any())


def _inside(values, d, lead=0):
    """``values`` as a slice of a larger NaN-filled buffer, ``lead`` floats behind a 16-byte boundary."""
    flat = values.contiguous().view(-1)
    pool = torch.full((flat.numel() + 2 * GUARD + 4,), NAN, device=d)
    view = pool[GUARD + lead:GUARD + lead + flat.numel()]
    view.copy_(flat)
    return pool, view


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _raw_up(g, S, nhwc, lead=0):
    """One call of the C entry: g a CPU [N,C,S h,S w] tensor, laid out NHWC or NCHW inside a guarded buffer; out in a NaN-filled guarded
    pool.  Returns the CPU [N,C,h,w] result."""
    from rmnet_amd import _lib
    lib = _lib.load()
    d = dev()
    N, C, H, W = g.shape
    h, w = H // S, W // S
    gpool, gv = _inside(g.permute(0, 2, 3, 1) if nhwc else g, d, lead)
    opool, ov = _guarded(N * C * h * w, d)
    with torch.cuda.device(d):
        rc = lib.rmnet_upsample_bwd_f32(_p(gv), N, C, h, w, S, 1 if nhwc else 0, _p(ov), ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert _guards_intact(opool, N * C * h * w), 'out: a guard was written or an element was not'
    out = ov.cpu()
    return (out.view(N, h, w, C).permute(0, 3, 1, 2) if nhwc else out.view(N, C, h, w)).numpy()


def _same_bits(got, want64):
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64), 'the expected values are no float32 numbers'
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32))


def _raw_head(x, w, g, need=(True, True, True)):
    """One call of the C entry: CPU x [n,C,H,W] (stored channels-last), w [2,C,3,3], g [n,2,H,W]; every output in a NaN-filled guarded
    pool.  Returns (dx [n,C,H,W], dw, db) as numpy arrays, None for a part that was not asked for (its pool must stay NaN)."""
    from rmnet_amd import _lib
    lib = _lib.load()
    d = dev()
    x, w, g = (torch.as_tensor(t) for t in (x, w, g))
    n, C, H, W = x.shape
    _, xv = _inside(x.permute(0, 2, 3, 1), d)
    _, wv = _inside(w, d)
    _, gv = _inside(g, d, lead=1)
    sizes = (n * C * H * W, 18 * C, 2)
    pools = [_guarded(s, d) for s in sizes]
    nbytes = lib.rmnet_pred_head_bwd_workspace_bytes(n, H, W, C)
    assert nbytes == ref.head_plan(n * H * W, C)[1] * (18 * C + 2) * 4
    ws_pool, ws = _guarded(nbytes // 4, d)
    with torch.cuda.device(d):
        rc = lib.rmnet_pred_head_bwd_f32(_p(xv), _p(wv), _p(gv), n, H, W, C, *[_p(v) if k else None for (_, v), k in zip(pools, need)],
                                         _p(ws), nbytes, ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isnan(ws_pool[:GUARD]).all()) and bool(torch.isnan(ws_pool[GUARD + nbytes // 4:]).all()), 'workspace guard'
    res = []
    for (pool, v), s, k, name in zip(pools, sizes, need, ('dx', 'dw', 'db')):
        if k:
            assert _guards_intact(pool, s), name + ': a guard was written or an element was not'
            res.append(v.cpu())
        else:
            assert bool(torch.isnan(pool).all()), name + ' was written although it was not asked for'
            res.append(None)
    dx = res[0].view(n, H, W, C).permute(0, 3, 1, 2).numpy() if need[0] else None
    return dx, res[1].view(2, C, 3, 3).numpy() if need[1] else None, res[2].numpy() if need[2] else None


# ================================================================================================ GPU 1: the upsample's adjoint
@pytest.mark.gpu
@pytest.mark.parametrize('S', [2, 4])
@pytest.mark.parametrize('layout', ['nchw', 'nchw+1', 'nhwc4', 'nhwc8', 'nhwc36'])
def test_the_adjoint_returns_integer_arithmetic_in_every_bit(S, layout):
    """g integers in [-8, 8]: every weight is dyadic and at most 64 terms meet, so every order is exact in float32.  'nchw+1': g one
    float behind a 16-byte boundary (the scalar loader); NCHW maps with S w % 4 != 0 take it as well."""
    nhwc = layout.startswith('nhwc')
    C = int(layout[4:]) if nhwc else 3
    for N in (1, 3):
        for seed, (h, w) in enumerate(MAPS):
            g = rng(100 * N + seed).integers(-8, 9, (N, C, S * h, S * w)).astype(np.float32)
            got = _raw_up(torch.from_numpy(g), S, nhwc, lead=1 if layout == 'nchw+1' else 0)
            assert _same_bits(got, ref.upsample_adjoint64(g, S)), (N, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize('S,nhwc,shape', [(2, True, (1, 8, 300, 450)), (4, False, (1, 2, 370, 370)), (2, False, (1, 2, 370, 742))])
def test_the_adjoint_walks_a_second_grid_stride_iteration(S, nhwc, shape):
    N, C, h, w = shape
    items = N * h * w * C // 4 if nhwc else N * C * h * -(-w // (4 // S))
    assert UP_MAX_BLOCKS * THREADS < items < 2 * UP_MAX_BLOCKS * THREADS
    g = rng(1).integers(-8, 9, (N, C, S * h, S * w)).astype(np.float32)
    assert _same_bits(_raw_up(torch.from_numpy(g), S, nhwc), ref.upsample_adjoint64(g, S))


@pytest.mark.gpu
@pytest.mark.parametrize('S', [2, 4])
@pytest.mark.parametrize('nhwc', [False, True])
def test_the_adjoint_is_within_the_bound_of_the_float64_restatement(S, nhwc):
    for seed, (h, w) in enumerate(MAPS + [(9, 12)]):
        g = _up_random(seed, 2, 8, h, w, S)
        got = _raw_up(torch.from_numpy(g), S, nhwc).astype(np.float64)
        want, bound = ref.upsample_adjoint64(g, S), ref.upsample_bound(g, S)
        err = np.abs(got - want)
        print('%dx%d: largest error / bound %.3f' % (h, w, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (h, w)                       # (an element whose taps are all zero: 0 <= 0)


# ================================================================================================ GPU 2: the prediction head
@pytest.mark.gpu
@pytest.mark.parametrize('C', [32, 64, 256])
def test_the_head_gradients_are_integer_arithmetic_in_every_bit(C):
    for n in (1, 3):
        for seed, (H, W) in enumerate(HEAD_MAPS):
            x, w, g = head_case(10 * n + seed, n, C, H, W, integers=True)
            assert n * H * W * 4 * 2 < 2 ** 24 and 18 * 2 * 2 < 2 ** 24 and n * H * W * 2 < 2 ** 24      # every sum is an exact float32
            if (n, H, W) == (1, 15, 31):
                assert ref.head_plan(n * H * W, C)[1:] == (2, 256)                                       # two ranges, 256 + 209 pixels
            got, want = _raw_head(x, w, g), ref.head_grads64(x, w, g)
            for a, b, name in zip(got, want, ('dx', 'dw', 'db')):
                assert _same_bits(a, b), (name, n, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize('n,C,H,W', [(1, 32, 1, 1), (2, 32, 3, 5), (1, 64, 15, 31), (3, 256, 17, 33), (1, 32, 40, 52)])
def test_the_head_gradients_are_within_the_bounds_of_the_float64_restatement(n, C, H, W):
    x, w, g = head_case(n + C + H, n, C, H, W)
    got, want, bounds = _raw_head(x, w, g), ref.head_grads64(x, w, g), ref.head_bounds(x, w, g)
    for a, b, bd, name in zip(got, want, bounds, ('dx', 'dw', 'db')):
        err = np.abs(a.astype(np.float64) - b)
        print('%s: largest error / bound %.3f' % (name, (err / np.maximum(bd, 1e-300)).max()))
        assert (err <= bd).all(), name


@pytest.mark.gpu
def test_a_nan_and_a_negative_zero_in_x_are_masked_and_counted_nowhere():
    x, w, g = head_case(5, 2, 32, 5, 6, integers=True)
    x[0, 3, 2, 2], x[1, 7, 0, 5], x[1, 31, 4, 0] = NAN, -0.0, NAN
    dx, dw, db = _raw_head(x, w, g)
    want = ref.head_grads64(x, w, g)
    assert dx[0, 3, 2, 2] == 0 and dx[1, 7, 0, 5] == 0 and dx[1, 31, 4, 0] == 0
    assert _same_bits(dx, want[0]) and _same_bits(dw, want[1]) and _same_bits(db, want[2])


@pytest.mark.gpu
@pytest.mark.parametrize('need', [(False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True)])
def test_each_output_of_the_head_backward_may_be_null(need):
    x, w, g = head_case(6, 1, 64, 15, 31, integers=True)
    got, want = _raw_head(x, w, g, need), ref.head_grads64(x, w, g)
    for a, b, k in zip(got, want, need):
        assert (a is None) == (not k) and (a is None or _same_bits(a, b))


# ================================================================================================ GPU 3: determinism
@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_return_the_same_bits():
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(4)
    g2 = cl(torch.randn(2, 64, 18, 30, generator=gen).to(d))
    g4 = torch.randn(2, 2, 36, 60, generator=gen).to(d)
    x = cl(torch.randn(2, 64, 9, 31, generator=gen).to(d))
    w = torch.randn(2, 64, 3, 3, generator=gen).to(d)
    gh = torch.randn(2, 2, 9, 31, generator=gen).to(d)

    def run():
        return (ops.upsample_backward(g2, 2), ops.upsample_backward(g2.contiguous(), 2), ops.upsample_backward(g4, 4),
                ops.upsample_backward(cl(g4.expand(2, 2, 36, 60).repeat(1, 2, 1, 1)), 4)) + ops.pred_head_backward(x, w, gh)

    first = [t.clone() for t in run()]
    second = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert torch.equal(first[0], first[1]) and first[0].is_contiguous(memory_format=torch.channels_last) and first[1].is_contiguous()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # a single stream, no parallel branches
        held = run()
    for t in held:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, held))


# ================================================================================================ GPU 4: autograd
def _within(got, want64, bound, name):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want64)
    assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.gpu
@pytest.mark.parametrize('leaf', [True, False])
@pytest.mark.parametrize('chlast', [True, False])
def test_upsample2x_add_under_autograd(leaf, chlast):
    from rmnet_amd import ops
    d = dev()
    fmt = cl if chlast else (lambda t: t.contiguous())
    gen = torch.Generator().manual_seed(21)
    x0, s0, g0 = torch.randn(2, 8, 5, 7, generator=gen), torch.randn(2, 8, 10, 14, generator=gen), torch.randn(2, 8, 10, 14, generator=gen)
    xl, sl = fmt(x0.to(d)).requires_grad_(True), fmt(s0.to(d)).requires_grad_(True)
    x, s = (xl, sl) if leaf else (xl * 1.0, sl + 0.0)
    out = ops.upsample2x_add(x, s)
    assert out.grad_fn is not None and 'Upsample2xAdd' in type(out.grad_fn).__name__
    plain = ops.upsample2x_add(xl.detach(), sl.detach())
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    g = fmt(g0.to(d))
    out.backward(g)
    assert torch.equal(sl.grad, g)
    _within(xl.grad, ref.upsample_adjoint64(g0.numpy(), 2), ref.upsample_bound(g0.numpy(), 2), 'x')
    first = xl.grad.clone()
    xl.grad = sl.grad = None
    x, s = (xl, sl) if leaf else (xl * 1.0, sl + 0.0)
    ops.upsample2x_add(x, s).backward(2 * g)                      # grad_output scaling: a power of two moves every result exactly
    assert torch.equal(xl.grad, 2 * first) and torch.equal(sl.grad, 2 * g)
    # a frozen skip gets no gradient; no skip at all; nothing requiring grad: no graph and the same bits
    xl.grad = None
    ops.upsample2x_add(xl, sl.detach()).backward(g)
    assert torch.equal(xl.grad, first)
    xl.grad = None
    ops.upsample2x_add(xl).backward(g)
    assert torch.equal(xl.grad, first)
    assert ops.upsample2x_add(xl.detach(), sl.detach()).grad_fn is None
    with torch.no_grad():
        assert ops.upsample2x_add(xl, sl).grad_fn is None
    with pytest.raises(RuntimeError, match='out must be None'):
        ops.upsample2x_add(xl, sl, out=torch.empty_like(plain))
    gx, = torch.autograd.grad((ops.upsample2x_add(xl, sl) ** 2).sum(), xl, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|twice'):
        gx.sum().backward()


@pytest.mark.gpu
@pytest.mark.parametrize('leaf', [True, False])
def test_upsample4x_under_autograd(leaf):
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(22)
    x0, g0 = torch.randn(3, 2, 5, 7, generator=gen), torch.randn(3, 2, 20, 28, generator=gen)
    xl = x0.to(d).requires_grad_(True)
    want = F.interpolate(xl.detach(), scale_factor=4, mode='bilinear', align_corners=False)
    out = ops.upsample4x(xl if leaf else xl * 1.0)
    assert 'Upsample4x' in type(out.grad_fn).__name__ and torch.equal(out.detach(), want)
    g = g0.to(d)
    out.backward(g)
    _within(xl.grad, ref.upsample_adjoint64(g0.numpy(), 4), ref.upsample_bound(g0.numpy(), 4), 'x')
    first = xl.grad.clone()
    xl.grad = None
    ops.upsample4x(xl if leaf else xl * 1.0).backward(cl(2 * g))  # (a channels-last grad_output becomes a plain tensor)
    assert torch.equal(xl.grad, 2 * first)
    plain = ops.upsample4x(xl.detach())
    assert plain.grad_fn is None and torch.equal(plain, want)
    with torch.no_grad():
        assert ops.upsample4x(xl).grad_fn is None
    gx, = torch.autograd.grad((ops.upsample4x(xl) ** 2).sum(), xl, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|twice'):
        gx.sum().backward()


@pytest.mark.gpu
@pytest.mark.parametrize('leaf', [True, False])
def test_pred_head_under_autograd(leaf):
    from rmnet_amd import ops
    d = dev()
    x0, w0, g0 = head_case(23, 2, 64, 9, 13)
    b0 = np.array([0.25, -0.5], np.float32)
    xl = cl(torch.from_numpy(x0).to(d)).requires_grad_(True)
    wl, bl = torch.from_numpy(w0).to(d).requires_grad_(True), torch.from_numpy(b0).to(d).requires_grad_(True)
    args = lambda: (xl, wl, bl) if leaf else (xl * 1.0, wl * 1.0, bl + 0.0)
    out = ops.pred_head(*args())
    assert 'PredHead' in type(out.grad_fn).__name__
    plain = ops.pred_head(xl.detach(), wl.detach(), bl.detach())
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    g = torch.from_numpy(g0).to(d)
    out.backward(g)
    want, bounds = ref.head_grads64(x0, w0, g0), ref.head_bounds(x0, w0, g0)
    for t, wt, bd, name in zip((xl, wl, bl), want, bounds, ('x', 'w', 'b')):
        _within(t.grad, wt, bd, name)
    first = [t.grad.clone() for t in (xl, wl, bl)]
    for t in (xl, wl, bl):
        t.grad = None
    ops.pred_head(*args()).backward(cl(g.expand(2, 2, 9, 13)) * 2)
    assert all(torch.equal(2 * a, t.grad) for a, t in zip(first, (xl, wl, bl)))
    # only what is needed: a frozen weight and bias
    xl.grad = None
    ops.pred_head(xl, wl.detach(), bl.detach()).backward(g)
    assert torch.equal(xl.grad, first[0])
    # a bias that requires grad next to a detached x and weight is the inference path's call: no graph
    assert ops.pred_head(xl.detach(), wl.detach(), bl).grad_fn is None
    with torch.no_grad():
        assert ops.pred_head(xl, wl, bl).grad_fn is None
    gx, = torch.autograd.grad((ops.pred_head(xl, wl, bl) ** 2).sum(), xl, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|twice'):
        gx.sum().backward()


# ================================================================================================ GPU 5: the module
def _decoder():
    from rmnet_amd import networks
    dec = networks.Decoder(256)
    networks.procedural_init_(dec)
    return dec.eval()


def _decoder_inputs(seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    return r(2, 1024, 2, 3), r(2, 512, 4, 6), r(2, 256, 8, 12), r(2, 2, 32, 48)


def _device_decoder(d, glue):
    from rmnet_amd import networks
    dec = _decoder().to(d).to(memory_format=torch.channels_last)
    networks.fuse_epilogues_(dec)
    return dec.device_grad_(glue=True) if glue else dec.device_grad_()


def _backward(dec, inputs, d, dtype=torch.float32):
    r4, r3, r2, go = (t.to(d, dtype) for t in inputs)
    if d.type == 'cuda':
        r4, r3, r2 = cl(r4), cl(r3), cl(r2)
    r4.requires_grad_(True)
    dec.zero_grad(set_to_none=True)
    out = dec(r4, r3, r2)
    (out * go).sum().backward()
    grads = {'r4': r4.grad}
    grads.update({n: p.grad for n, p in dec.named_parameters()})
    return out, {k: v.detach().cpu().double() for k, v in grads.items()}


def _count_glue_ops(monkeypatch):
    from rmnet_amd import ops
    calls = {'upsample2x_add': 0, 'pred_head': 0, 'upsample4x': 0}
    depth = [0]                                                   # (a recorded op calls its own plain path: the outer call counts)
    for name in calls:
        def wrap(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += depth[0] == 0
            depth[0] += 1
            try:
                return _f(*a, **kw)
            finally:
                depth[0] -= 1
        monkeypatch.setattr(ops, name, wrap)
    return calls


@pytest.mark.gpu
def test_the_decoder_with_glue_trains_as_precisely_as_the_library_route_and_repeats_its_bits(monkeypatch):
    """The project's bar (tests/test_conv_grad.py): the largest error relative to the largest gradient, against the same module in
    float64 on the CPU, at most 4x that of torch autograd through the fp32 library convolutions on the same inputs."""
    from rmnet_amd import ops
    d = dev()
    inputs = _decoder_inputs()
    dec = _device_decoder(d, glue=True)
    ops.conv_range_word(d).zero_()
    ops.conv_grad_range_word(d).zero_()
    calls = _count_glue_ops(monkeypatch)
    out, ours = _backward(dec, inputs, d)
    assert out.grad_fn is not None and 'Upsample4x' in type(out.grad_fn).__name__
    assert calls == {'upsample2x_add': 2, 'pred_head': 1, 'upsample4x': 1}
    out2, again = _backward(dec, inputs, d)
    assert torch.equal(out, out2) and set(again) == set(ours) and len(ours) == 1 + 2 * 14
    assert all(torch.equal(ours[k], again[k]) for k in ours), [k for k in ours if not torch.equal(ours[k], again[k])]
    assert int(ops.conv_range_word(d)) == 0 and int(ops.conv_grad_range_word(d)) == 0
    _, want = _backward(_decoder().double(), inputs, torch.device('cpu'), torch.float64)
    monkeypatch.setenv('RMNET_CONV', 'miopen')
    lib = _decoder().to(d).to(memory_format=torch.channels_last).train()
    _, theirs = _backward(lib, inputs, d)
    monkeypatch.delenv('RMNET_CONV')
    assert set(ours) == set(want) == set(theirs)
    rel = lambda got: max(((got[k] - want[k]).abs().max() / want[k].abs().max()).item() for k in want)
    e_ours, e_lib = rel(ours), rel(theirs)
    print('largest gradient error relative to the largest gradient: ours %.3e, library %.3e' % (e_ours, e_lib))
    assert e_ours <= 4 * e_lib


@pytest.mark.gpu
def test_device_grad_without_glue_calls_none_of_the_new_ops(monkeypatch):
    d = dev()
    inputs = _decoder_inputs(1)
    dec = _device_decoder(d, glue=False)
    calls = _count_glue_ops(monkeypatch)
    out, grads = _backward(dec, inputs, d)
    assert out.grad_fn is not None and calls == {'upsample2x_add': 0, 'pred_head': 0, 'upsample4x': 0}
    dec.device_grad_(glue=True)
    out_glue, grads_glue = _backward(dec, inputs, d)
    assert calls == {'upsample2x_add': 2, 'pred_head': 1, 'upsample4x': 1}
    assert (out - out_glue).abs().max() <= 1e-5 * out.abs().max()
    assert all((grads[k] - grads_glue[k]).abs().max() <= 1e-4 * grads[k].abs().max() for k in grads)
    dec.device_grad_()                                            # as called before this flag existed: the flag is off again
    _backward(dec, inputs, d)
    assert calls == {'upsample2x_add': 2, 'pred_head': 1, 'upsample4x': 1}
    dec.device_grad_(False, glue=True)                            # no device gradient, no glue
    assert not dec._glue_grad and not dec.RF2._glue_grad


@pytest.mark.gpu
def test_the_head_reads_the_live_weight_after_an_optimiser_step():
    d = dev()
    r4, r3, r2, _ = _decoder_inputs(2)
    dec = _device_decoder(d, glue=True)
    r4 = cl(r4.to(d)).requires_grad_(True)
    before = dec(r4, cl(r3.to(d)), cl(r2.to(d))).detach()
    bias = dec.pred2.bias.detach()
    assert float((before[:, 0] - bias[0]).abs().max()) > 1e-3
    with torch.no_grad():
        dec.pred2.weight.zero_()                                  # an in-place step: the flat copy the inference path keeps is stale now
    after = dec(r4, cl(r3.to(d)), cl(r2.to(d)))
    for k in range(2):
        assert float((after.detach()[:, k] - bias[k]).abs().max()) <= 1e-6 * max(1.0, float(bias[k].abs()))
    after.sum().backward()
    assert float(dec.pred2.weight.grad.abs().max()) > 0 and dec.pred2.weight.grad.shape == dec.pred2.weight.shape
