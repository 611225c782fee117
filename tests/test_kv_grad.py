# -*- coding: utf-8 -*-
"""The gradients of the key / value heads: the weight / bias gradient for any multiple of 128 output channels and the stage pass for
what the memory read hands back (csrc/conv_wgrad_n.hip), the data gradient (``ops.kv_dgrad``: ``conv_split`` on flipped packs),
``ops._KeyValueFn`` and ``KeyValue.device_grad_``.

CPU part: the plan's literals and invariants, the float64 restatement (tests/kv_grad_ref.py) pinned by hand and by torch autograd,
eight planted faults, the two C entries' refusals, the compiler's resources.
GPU part: an exact family (every bit), Cout = 256 against the decoder's entry, a random family (the derived per-element bound of
tests/conv_grad_ref.py / tests/conv_ref.py), the stage kernel against torch in every bit, the module against float64, launches and
paths, determinism and a graph replay, repacking, the range words, and the chain r4 -> heads -> memory read."""

import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as cg
import conv_ref
import kv_grad_ref as ref
from conftest import ROOT

CT, KT, MAX_W, BIAS_SPLIT = 16, 32, 448, 8
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
NAN, INF = float('nan'), float('inf')


def dev():
    return torch.device('cuda', 0)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def t64(v):
    return torch.tensor(v, dtype=torch.float64)


# ================================================================================================ CPU 1: the plan
def test_the_plan_without_cout_is_unchanged_and_the_new_widths_get_their_literals():
    from rmnet_amd import ops
    plan = ops.conv3x3_wgrad_plan
    # the literal triples of tests/test_conv_grad.py
    assert plan(1, 32) == (2, 1, 32) and plan(256, 32) == (2, 1, 256) and plan(257, 32) == (2, 2, 160)
    assert plan(2 * 129 * 128, 32) == (2, 61, 544)
    assert plan(12 * 120 * 120, 256) == (16, 48, 3616) and plan(12 * 900, 1024) == (64, 12, 928)
    for p in (1, 256, 257, 10800, 3600):
        for cin in (32, 1024):
            assert plan(p, cin, 256) == plan(p, cin) == plan(p, cin, 128)         # one tile of output channels: today's plan
            assert plan(p, cin, 384) == plan(p, cin, 512)                         # two tiles
    # Cin 32: 2 channel tiles, 768 // (2 tiles) ranges allowed -- the length caps decide
    for cout in (128, 384, 512, 640):
        assert plan(1, 32, cout) == (2, 1, 32) and plan(256, 32, cout) == (2, 1, 256) and plan(257, 32, cout) == (2, 2, 160)
        assert plan(10800, 32, cout) == (2, 43, 256) and plan(3600, 32, cout) == (2, 15, 256)
        assert plan(1, 1024, cout) == (64, 1, 32) and plan(256, 1024, cout) == (64, 1, 256)
    # Cin 1024: 64 channel tiles, 768 // (64 * tiles) = 12 / 6 / 6 / 4 ranges
    assert plan(257, 1024, 128) == (64, 2, 160) and plan(257, 1024, 384) == (64, 2, 160) and plan(257, 1024, 640) == (64, 2, 160)
    assert plan(10800, 1024, 128) == (64, 12, 928) and plan(3600, 1024, 128) == (64, 12, 320)
    assert plan(10800, 1024, 384) == (64, 6, 1824) == plan(10800, 1024, 512) and plan(3600, 1024, 384) == (64, 6, 608)
    assert plan(10800, 1024, 640) == (64, 4, 2720) and plan(3600, 1024, 640) == (64, 4, 928)
    for p in (1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 3600, 10800, 33024, 172800):
        for cin in (32, 64, 256, 512, 1024):
            for cout in (128, 256, 384, 512, 640, 1024):
                nct, nr, rl = plan(p, cin, cout)
                assert nct == cin // CT and 1 <= nr <= 64 and rl % KT == 0 and (nr - 1) * rl < p <= nr * rl


# ================================================================================================ CPU 2: the restatement
def test_the_restatement_gives_the_hand_written_answers():
    # a 1 x 1 map: only the centre taps see it
    wk = torch.arange(1.0, 10.0).view(1, 1, 3, 3)
    wv = -torch.arange(1.0, 19.0).view(2, 1, 3, 3)
    r = ref.kv_grads64(t64([[[[3.0]]]]), wk, wv, t64([[[[5.0]]]]), t64([[[[7.0]], [[-2.0]]]]), rects=[(0, 0, 0, 0)])
    want = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    want[0, 0, 1, 1] = 15.0
    assert torch.equal(r['dWk'], want) and torch.equal(r['dbk'], t64([5.0]))
    assert r['dWv'][0, 0, 1, 1] == 21.0 and r['dWv'][1, 0, 1, 1] == -6.0 and float(r['dWv'].abs().sum()) == 27.0
    assert torch.equal(r['dbv'], t64([7.0, -2.0]))
    assert torch.equal(r['dX'], t64([[[[5.0 * 5.0 + 7.0 * -5.0 + -2.0 * -14.0]]]]))
    # one live tap: x at (1 + ky, 2 + kx), g at (2, 3) -- only dW[ky, kx] is non-zero, and dX lands on the pixel that the tap read
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        x, g = torch.zeros(1, 1, 5, 7, dtype=torch.float64), torch.zeros(1, 1, 5, 7, dtype=torch.float64)
        x[0, 0, 1 + ky, 2 + kx], g[0, 0, 2, 3] = 3.0, 2.0
        w = torch.zeros(1, 1, 3, 3)
        w[0, 0, ky, kx] = 4.0
        r = ref.kv_grads64(x, w, w, g, None)
        want = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
        want[0, 0, ky, kx] = 6.0
        assert torch.equal(r['dWk'], want) and r['dWv'] is None and r['dbv'] is None
        wx = torch.zeros_like(x)
        wx[0, 0, 1 + ky, 2 + kx] = 8.0                               # out(2, 3) reads x(2 + ky - 1, 3 + kx - 1) through w[ky, kx]
        assert torch.equal(r['dX'], wx)
    # a single-cell rectangle in a gradient of ones: dW sees only that cell, and its eight neighbours get dX through the taps
    x = torch.arange(1.0, 10.0, dtype=torch.float64).view(1, 1, 3, 3)
    w = torch.arange(1.0, 10.0).view(1, 1, 3, 3)
    r = ref.kv_grads64(x, w, w, torch.ones(1, 1, 3, 3), None, rects=[(1, 1, 1, 1)])
    assert torch.equal(r['dWk'], x) and torch.equal(r['dbk'], t64([1.0]))       # dW[ky, kx] = x(1 + ky - 1, 1 + kx - 1)
    assert torch.equal(r['dX'], w.double())                                      # dX(y, x) = G(1, 1) w[y, x]: y - ky + 1 = 1
    bad = ref.kv_grads64(x, w, w, torch.ones(1, 1, 3, 3), None, rects=[(1, 1, 1, 1)], fault='unflipped_tap')
    assert torch.equal(bad['dX'], w.double().flip(2, 3))
    # a rectangle that reaches beyond the map is clamped; an empty one gives zeros everywhere
    r = ref.kv_grads64(x, w, w, torch.ones(1, 1, 3, 3), None, rects=[(2, 9, -4, 0)])
    # the one cell (y 0, x 2): dW[ky, kx] = x(ky - 1, 1 + kx), zero where that leaves the map
    assert torch.equal(r['dbk'], t64([1.0])) and torch.equal(r['dWk'], t64([[[[0.0, 0.0, 0.0], [2.0, 3.0, 0.0], [5.0, 6.0, 0.0]]]]))
    r = ref.kv_grads64(x, w, w, torch.full((1, 1, 3, 3), NAN), torch.ones(1, 1, 3, 3), rects=[(1, 0, 1, 0)])
    for k in ('dX', 'dWk', 'dbk', 'dWv', 'dbv'):
        assert float(r[k].abs().sum()) == 0.0, k


def _autograd64(x, wk, wv, gk, gv, rects):
    x = x.double().requires_grad_(True)
    wk, wv = wk.double().requires_grad_(True), wv.double().requires_grad_(True)
    bk = torch.zeros(wk.shape[0], dtype=torch.float64, requires_grad=True)
    bv = torch.zeros(wv.shape[0], dtype=torch.float64, requires_grad=True)
    m = ref.inside(rects, x.shape[0], x.shape[2], x.shape[3])
    key = torch.where(m, F.conv2d(x, wk, bk, 1, 1), torch.zeros((), dtype=torch.float64))
    val = torch.where(m, F.conv2d(x, wv, bv, 1, 1), torch.zeros((), dtype=torch.float64))
    ((key * gk.double()).sum() + (val * gv.double()).sum()).backward()
    return dict(dX=x.grad, dWk=wk.grad, dbk=bk.grad, dWv=wv.grad, dbv=bv.grad)


RECT_SETS = {
    'none': None, 'whole': [(0, 6, 0, 4), (0, 6, 0, 4)], 'cell': [(3, 3, 2, 2), (0, 0, 0, 0)], 'row': [(0, 6, 1, 1), (0, 6, 4, 4)],
    'column': [(5, 5, 0, 4), (6, 6, 0, 4)], 'empty': [(1, 0, 1, 0), (2, 4, 1, 3)], 'beyond': [(-3, 2, 3, 11), (5, 40, -1, 1)],
    'per image': [(1, 4, 0, 2), (2, 6, 3, 4)],
}


def _cpu_case(seed=0, n=2, cin=4, ck=4, cv=8, h=5, w=7):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return r(n, cin, h, w), r(ck, cin, 3, 3), r(cv, cin, 3, 3), r(n, ck, h, w), r(n, cv, h, w) * 2.0 ** -12


@pytest.mark.parametrize('rects', sorted(RECT_SETS))
def test_the_restatement_is_torch_autograd_in_float64(rects):
    x, wk, wv, gk, gv = _cpu_case()
    got = ref.kv_grads64(x, wk, wv, gk, gv, RECT_SETS[rects])
    want = _autograd64(x, wk, wv, gk, gv, RECT_SETS[rects])
    for k, v in want.items():
        assert (got[k] - v).abs().max() <= 1e-12 * max(1.0, float(v.abs().max())), k


def _differs(a, b):
    for k in a:
        if a[k] is None:
            continue
        bad = torch.isnan(a[k]) != torch.isnan(b[k])
        if bad.any() or (torch.nan_to_num(a[k]) - torch.nan_to_num(b[k])).abs().max() > 1e-9 * max(1.0, float(torch.nan_to_num(b[k]).abs().max())):
            return True
    return False


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_a_planted_fault_in_the_heads_backward_is_caught(fault):
    x, wk, wv, gk, gv = _cpu_case(1)
    rects = RECT_SETS['per image']
    if fault == 'mask_product':
        gk = gk.clone()
        gk[0, 1, 4, 6] = NAN                                            # outside image 0's rectangle: must not leak
        good = ref.kv_grads64(x, wk, wv, gk, gv, rects)
        assert not any(torch.isnan(v).any() for v in good.values())
        assert any(torch.isnan(v).any() for v in ref.kv_grads64(x, wk, wv, gk, gv, rects, fault=fault).values())
        return
    if fault == 'tail_tile_lost':                                       # 384 outputs: the tail tile of 128
        gen = torch.Generator().manual_seed(2)
        wv = torch.randn(384, 4, 3, 3, generator=gen, dtype=torch.float64)
        gv = torch.randn(2, 384, 5, 7, generator=gen, dtype=torch.float64)
    if fault == 'sc_is_hw':                                             # gk is frame t = 2 of a [N, C, 3, h, w] tensor
        gen = torch.Generator().manual_seed(3)
        src = torch.randn(2, 4, 3, 5, 7, generator=gen, dtype=torch.float64)
        read = lambda f: ref.read_planes(src, 2 * 35, 4 * 3 * 35, 3 * 35, 2, 4, 5, 7, fault=f)
        assert torch.equal(read(None), src[:, :, 2])
        good = ref.kv_grads64(x, wk, wv, read(None), gv, rects)
        assert _differs(ref.kv_grads64(x, wk, wv, read(fault), gv, rects), good)
        return
    good = ref.kv_grads64(x, wk, wv, gk, gv, rects)
    assert not _differs(ref.kv_grads64(x, wk, wv, gk, gv, rects), good)
    assert _differs(ref.kv_grads64(x, wk, wv, gk, gv, rects, fault=fault), good), fault


# ================================================================================================ CPU 3: refusals, resources
def _wgrad_n_refusals(good):
    inv, uns, wsp = E_INVALID, E_UNSUPPORTED, E_WORKSPACE
    for k in ('x', 'g', 'g_scale', 'dw'):
        yield 'null ' + k, {k: 0}, inv
    for k in ('N', 'W', 'Cin', 'Cout'):
        yield k + ' = 0', {k: 0}, inv
    yield 'H < 0', dict(H=-1), inv
    yield 'Cout < 0', dict(Cout=-128), inv
    yield 'relu_out is no flag here', dict(flags=2), inv
    yield 'unknown flag', dict(flags=4), inv
    for k in ('x', 'g', 'g_scale', 'dw', 'db', 'ws'):
        yield 'misaligned ' + k, {k: good[k] + 4}, inv
    yield 'misaligned range word', dict(rw=good['rw'] + 2), inv
    yield 'dw overlaps x', dict(dw=good['x'] + 16), inv
    yield 'dw overlaps g', dict(dw=good['g'] + 16), inv
    yield 'dw overlaps the last row of g', dict(dw=good['g'] + 20 * 384 * 4 - 16), inv
    yield 'db overlaps dw', dict(db=good['dw'] + 9 * 32 * 384 * 4 - 16), inv
    yield 'workspace overlaps dw', dict(ws=good['dw']), inv
    yield 'dw overlaps g_scale', dict(g_scale=good['dw'] + 32), inv
    yield 'workspace overlaps the range word', dict(rw=good['ws'] + 8), inv
    yield 'db overlaps g_scale', dict(g_scale=good['db'] + 384 * 4 - 16), inv
    yield 'Cin % 32', dict(Cin=48), uns
    yield 'Cout % 128', dict(Cout=320), uns
    yield 'Cout = 64', dict(Cout=64), uns
    yield 'W above the widest map', dict(W=MAX_W + 1), uns
    yield '2^31 elements of g', dict(N=1 << 12, H=1 << 7, W=1 << 3, Cout=512), uns
    yield '2^31 elements of dw', dict(Cin=1 << 14, Cout=1 << 14), uns
    yield 'null workspace', dict(ws=0), wsp
    yield 'short workspace', dict(ws_bytes=good['ws_bytes'] - 1), wsp


def _wgrad_n_call(lib, a):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.rmnet_conv3x3_wgrad_n_f32(p(a['x']), p(a['g']), p(a['g_scale']), a['flags'], a['N'], a['H'], a['W'], a['Cin'], a['Cout'],
                                         p(a['dw']), p(a['db']), p(a['ws']), a['ws_bytes'], p(a['rw']), None)


def _stage_rect_refusals(good):
    inv, uns = E_INVALID, E_UNSUPPORTED
    for k in ('g', 'amax', 'gs', 'g_scale'):
        yield 'null ' + k, {k: 0}, inv
    for k in ('N', 'C', 'H', 'W'):
        yield k + ' = 0', {k: 0}, inv
    yield 'layout 2', dict(layout=2), inv
    yield 'layout -1', dict(layout=-1), inv
    yield 'misaligned gs', dict(gs=good['gs'] + 4), inv
    yield 'misaligned g_scale', dict(g_scale=good['g_scale'] + 8), inv
    yield 'channels-last g off 16 bytes', dict(layout=0, g=good['g'] + 4), inv
    yield 'planes off 4 bytes', dict(g=good['g'] + 2), inv
    yield 'misaligned amax', dict(amax=good['amax'] + 1), inv
    yield 'misaligned rects', dict(rects=good['rects'] + 2), inv
    yield 'planes fold: sc < H W', dict(sc=19), inv
    yield 'planes fold: sn < (C - 1) sc + H W', dict(sn=7 * 60 + 19), inv
    yield 'gs overlaps g partly', dict(layout=0, gs=good['g'] + 16), inv
    yield 'planes staged in place', dict(gs=good['g']), inv
    yield 'gs overlaps the last plane of g', dict(gs=good['g'] + (2 * 480 + 7 * 60 + 19) * 4 - 12), inv
    yield 'gs overlaps amax', dict(amax=good['gs'] + 64), inv
    yield 'gs overlaps the rectangles', dict(rects=good['gs'] + 3 * 8 * 20 * 4 - 4), inv
    yield 'g_scale overlaps amax', dict(amax=good['g_scale'] + 4), inv
    yield 'g_scale overlaps g', dict(g_scale=good['g'] + 32), inv
    yield 'g_scale overlaps the rectangles', dict(g_scale=good['rects'] + 32), inv
    yield 'C % 4', dict(C=6), uns
    yield '2^31 elements', dict(N=1 << 10, C=1 << 10, H=1 << 6, W=1 << 5, sc=1 << 11, sn=1 << 21), uns
    yield 'planes spanning 2^31 floats', dict(sn=1 << 30), uns


def _stage_rect_call(lib, a):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.rmnet_conv_grad_stage_rect_f32(p(a['g']), a['layout'], a['sn'], a['sc'], p(a['rects']), p(a['amax']), a['N'], a['C'],
                                              a['H'], a['W'], p(a['gs']), p(a['g_scale']), None)


def test_the_new_entries_refuse_malformed_calls_before_they_touch_the_device():
    """No GPU here: a call that got past the checks would fail to launch or fault on these made-up addresses."""
    from rmnet_amd import _lib
    lib = _lib.load()
    ws_bytes = lib.rmnet_conv3x3_wgrad_n_workspace_bytes
    N, H, W, Cin, Cout = 1, 4, 5, 32, 384
    assert ws_bytes(N, H, W, Cin, Cout) == (9 * Cin * Cout + BIAS_SPLIT * Cout) * 4                                # one range
    assert ws_bytes(1, 1, 257, 32, 640) == 2 * (9 * 32 * 640 + BIAS_SPLIT * 640) * 4                               # two
    assert ws_bytes(12, 30, 30, 1024, 640) == 4 * (9 * 1024 * 640 + BIAS_SPLIT * 640) * 4                          # the training shape
    assert ws_bytes(12, 30, 30, 1024, 256) == lib.rmnet_conv3x3_wgrad_workspace_bytes(12, 30, 30, 1024) == 12 * (9 * 1024 * 256 + 8 * 256) * 4
    assert ws_bytes(1, 4, MAX_W + 1, 32, 128) == 0 and ws_bytes(0, 4, 4, 32, 128) == 0 and ws_bytes(1, 4, 4, 32, 192) == 0
    assert ws_bytes(1, 4, 4, 32, 0) == 0 and ws_bytes(1, 4, 4, 48, 128) == 0
    base = 0x100000
    good = dict(x=base, g=base + 0x10000, g_scale=base + 0x20000, flags=1, N=N, H=H, W=W, Cin=Cin, Cout=Cout, dw=base + 0x100000,
                db=base + 0x80000, ws=base + 0x200000, ws_bytes=ws_bytes(N, H, W, Cin, Cout), rw=base + 0x20100)
    for name, kw, code in _wgrad_n_refusals(good):
        assert _wgrad_n_call(lib, dict(good, **kw)) == code, name
    # three images of 8 channels of 4 x 5 planes, 60 floats from plane to plane and 480 from image to image
    good = dict(g=0x100000, layout=1, sn=480, sc=60, rects=0x300000, amax=0x300100, N=3, C=8, H=4, W=5, gs=0x400000, g_scale=0x300200)
    for name, kw, code in _stage_rect_refusals(good):
        assert _stage_rect_call(lib, dict(good, **kw)) == code, name


def test_the_new_kernels_use_no_scratch_no_spill_and_no_static_lds(tmp_path):
    """From a compile-only gfx950 build: sizes and counts of the metadata, no instruction is looked at."""
    from rmnet_amd import build
    assert 'conv_wgrad_n.hip' in build.SOURCES
    out = str(tmp_path / 'wgrad_n.s')
    subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                    os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv_wgrad_n.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', open(out).read(), flags=re.S).group(1)
    found = {}
    for entry in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]:
        get = lambda key: re.search(r'^    \.%s:\s+(\S+)' % key, '    ' + entry, flags=re.M)
        if get('name'):
            found[get('name').group(1)] = {k: int(get(k).group(1)) for k in ('group_segment_fixed_size', 'private_segment_fixed_size',
                                                                            'vgpr_count', 'vgpr_spill_count', 'max_flat_workgroup_size')}
    assert len(found) == 5, sorted(found)                              # the GEMM, the bias sum, the merge, the two stage instances
    for name, k in found.items():
        print(name, k)
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (name, k)
        assert k['vgpr_count'] <= (256 if k['max_flat_workgroup_size'] == 512 else 512), (name, k)   # 512 threads: two waves a SIMD
        for frag in ('13conv3x3_wgradE', '10wgrad_biasE', '11wgrad_mergeE', '15conv_grad_stageE'):  # (tests/test_conv_grad.py's)
            assert frag not in name
    assert sorted(k['max_flat_workgroup_size'] for k in found.values()) == [128, 256, 256, 256, 512]


# ================================================================================================ GPU helpers
GUARD = 64


def _guarded(n, d):
    pool = torch.full((n + 2 * GUARD,), NAN, device=d)
    assert pool.data_ptr() % 16 == 0
    return pool, pool[GUARD:GUARD + n]


def _guards_intact(pool, n, nan_inside=False):
    ok = bool(torch.isnan(pool[:GUARD]).all()) and bool(torch.isnan(pool[GUARD + n:]).all())
    return ok and (nan_inside or not bool(torch.isnan(pool[GUARD:GUARD + n]).any()))


def _raw_wgrad_n(x, gs, g_scale, want_bias=True, rw=None, old_entry=False):
    """One call of the C entry with dw / db / workspace inside NaN-filled guarded pools; x [N,Cin,H,W] and gs [N,Cout,H,W]
    channels-last on the device.  Returns (dW [Cout,Cin,3,3], db) on the CPU."""
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    d = x.device
    N, cin, H, W = x.shape
    cout = gs.shape[1]
    n_dw = 9 * cin * cout
    dw_pool, dw = _guarded(n_dw, d)
    db_pool, db = _guarded(cout, d)
    nbytes = lib.rmnet_conv3x3_wgrad_workspace_bytes(N, H, W, cin) if old_entry else lib.rmnet_conv3x3_wgrad_n_workspace_bytes(N, H, W, cin, cout)
    assert nbytes == ops.conv3x3_wgrad_plan(N * H * W, cin, cout)[1] * (n_dw + BIAS_SPLIT * cout) * 4
    ws_pool, ws = _guarded(nbytes // 4, d)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)
    with torch.cuda.device(d):
        if old_entry:
            rc = lib.rmnet_conv3x3_wgrad_f32(p(x), p(gs), p(g_scale), 0, N, H, W, cin, p(dw), p(db) if want_bias else None, p(ws), nbytes, p(rw), st)
        else:
            rc = lib.rmnet_conv3x3_wgrad_n_f32(p(x), p(gs), p(g_scale), 0, N, H, W, cin, cout, p(dw), p(db) if want_bias else None, p(ws),
                                               nbytes, p(rw), st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _guards_intact(dw_pool, n_dw), 'dw: a guard was written or an element was not'
    assert _guards_intact(ws_pool, nbytes // 4, nan_inside=True), 'workspace guard'
    if want_bias:
        assert _guards_intact(db_pool, cout), 'db'
    else:
        assert bool(torch.isnan(db_pool).all())
    return dw.view(cout, 3, 3, cin).permute(0, 3, 1, 2).cpu(), db.cpu() if want_bias else None


def _int_dw(x, g):
    _, dW, db, _ = cg.grads64(x, torch.zeros(g.shape[1], x.shape[1], 3, 3), g)
    return dW.float(), db.float()


# ================================================================================================ GPU 1: wgrad, the exact family
WGRAD_EXACT = [
    # (Cin, Cout, N, H, W)
    (32, 128, 1, 1, 1), (32, 128, 2, 1, 9), (32, 384, 1, 5, 7), (64, 640, 2, 5, 7),
    (32, 512, 1, 1, 257),                                         # two ranges
    (32, 384, 1, 3, 33),                                          # a row one pixel longer than a K step
    (32, 640, 2, 16, 16),
    (64, 128, 2, 129, 128),                                       # many ranges, each crossing an image
]


@pytest.mark.gpu
@pytest.mark.parametrize('e', [0, -30])
@pytest.mark.parametrize('cin,cout,n,h,w', WGRAD_EXACT)
def test_wgrad_n_returns_integer_arithmetic_in_every_bit(cin, cout, n, h, w, e):
    from rmnet_amd import ops
    d = dev()
    x = conv_ref.int_acts((n, cin, h, w), 100 + cin + h)
    g = cg.pow2_grads((n, cout, h, w), 7 + w, e)
    want_dw, want_db = _int_dw(x, g)
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    assert torch.equal(gs.cpu(), g * 2.0 ** (8 - e)) and float(g_scale[0] * g_scale[1]) == 2.0 ** (8 - e)
    rw = torch.zeros(1, dtype=torch.int32, device=d)
    dw, db = _raw_wgrad_n(cl(x.to(d)), gs, g_scale, rw=rw)
    assert torch.equal(dw, want_dw), 'dW: %d elements differ' % int((dw != want_dw).sum())
    assert torch.equal(db, want_db)
    assert int(rw) == 0
    dw2, none = _raw_wgrad_n(cl(x.to(d)), gs, g_scale, want_bias=False)
    assert none is None and torch.equal(dw2, dw)
    got_dw, got_db = ops.conv3x3_wgrad(cl(x.to(d)), gs, g_scale)                   # the wrapper picks this entry
    assert got_dw.shape == (cout, cin, 3, 3) and got_dw.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got_dw.cpu(), want_dw) and torch.equal(got_db.cpu(), want_db)


@pytest.mark.gpu
@pytest.mark.parametrize('tap', range(9))
def test_wgrad_n_with_one_live_tap(tap):
    """x at one pixel, g at its neighbour through ``tap``: the only non-zero dW is that tap's, in all three tiles of 384 channels."""
    from rmnet_amd import ops
    d = dev()
    ky, kx = tap // 3, tap % 3
    x, g = torch.zeros(1, 32, 5, 7), torch.zeros(1, 384, 5, 7)
    x[0, :, 1 + ky, 2 + kx] = conv_ref.int_acts((32,), tap, 1, 15)
    g[0, :, 2, 3] = cg.pow2_grads((384,), tap, zeros=False)
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    dw, db = _raw_wgrad_n(cl(x.to(d)), gs, g_scale)
    want = torch.zeros(384, 32, 3, 3)
    want[:, :, ky, kx] = g[0, :, 2, 3].view(-1, 1) * x[0, :, 1 + ky, 2 + kx].view(1, -1)
    assert torch.equal(dw, want) and torch.equal(db, g[0, :, 2, 3])


@pytest.mark.gpu
@pytest.mark.parametrize('cin,n,h,w', [(32, 1, 19, 27), (256, 2, 16, 16)])
def test_256_outputs_through_the_new_entry_are_the_bits_of_the_old_one(cin, n, h, w):
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(cin + w)
    x = torch.randn(n, cin, h, w, generator=gen) * 3
    g = torch.randn(n, 256, h, w, generator=gen) * 1e-3
    x[0, 3, 0, 0], g[0, 5, h - 1, w - 1], g[0, 200, 0, 1] = 5000.0, NAN, INF       # counted: one of x, two of g
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)), amax=torch.tensor(4e-3, device=d))
    # (dw holds NaN where the planted values reach it: the bit patterns are compared, without the guarded pools' NaN test)
    from rmnet_amd import _lib
    lib = _lib.load()
    outs = []
    for entry_old in (True, False):
        n_dw = 9 * cin * 256
        dw = torch.full((n_dw,), 7.0, device=d)
        db = torch.full((256,), 7.0, device=d)
        nbytes = lib.rmnet_conv3x3_wgrad_n_workspace_bytes(n, h, w, cin, 256)
        assert nbytes == lib.rmnet_conv3x3_wgrad_workspace_bytes(n, h, w, cin)
        ws = torch.empty(nbytes // 4, device=d)
        word = torch.zeros(1, dtype=torch.int32, device=d)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)
        xd = cl(x.to(d))
        with torch.cuda.device(d):
            if entry_old:
                rc = lib.rmnet_conv3x3_wgrad_f32(p(xd), p(gs), p(g_scale), 0, n, h, w, cin, p(dw), p(db), p(ws), nbytes, p(word), st)
            else:
                rc = lib.rmnet_conv3x3_wgrad_n_f32(p(xd), p(gs), p(g_scale), 0, n, h, w, cin, 256, p(dw), p(db), p(ws), nbytes, p(word), st)
        torch.cuda.synchronize()
        assert rc == 0
        outs.append((dw.view(torch.int32).cpu(), db.view(torch.int32).cpu(), int(word)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2] == 3


# ================================================================================================ GPU 2: wgrad, the random family
def _random_g(kind, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen)
    if kind == 'mixed':                                           # output channel c times 2^(-24 + c mod 20)
        return g * torch.ldexp(torch.ones(shape[1]), (torch.arange(shape[1]) % 20 - 24).float()).view(1, -1, 1, 1)
    return g * float(kind)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['1e-8', '1', 'mixed'])
@pytest.mark.parametrize('cout', [128, 640])
@pytest.mark.parametrize('cin,n,h,w', [(32, 1, 4, 8), (64, 2, 16, 16)])
def test_wgrad_n_is_within_the_derived_bound_of_its_restatement(kind, cout, cin, n, h, w):
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(cin + h)
    x = torch.randn(n, cin, h, w, generator=gen) * 2
    g = _random_g(kind, (n, cout, h, w), 31)
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    gs64, s = cg.stage64(g)
    assert torch.equal(gs.cpu().double(), gs64) and float(g_scale[0]) == 2.0 ** s and float(g_scale[1]) == 1.0
    plan = ops.conv3x3_wgrad_plan(n * h * w, cin, cout)
    T, ahh, ax, Tb, Ab = cg.wgrad_restate(x, gs64, s, plan)
    dw, db = _raw_wgrad_n(cl(x.to(d)), gs, g_scale)
    err, bound = (dw.double() - T).abs(), cg.acc_bound(plan[2], plan[1], ahh, ax)
    print('dW: largest error / bound %.3f' % (err / bound.clamp_min(1e-300)).max())
    assert (err <= bound).all()
    assert ((db.double() - Tb).abs() <= cg.bias_bound(plan[2] // BIAS_SPLIT, plan[1] * BIAS_SPLIT, Ab)).all()
    truth = cg.grads64(x, torch.zeros(cout, cin, 3, 3), g)[1]
    assert ((dw.double() - truth).abs() <= bound + cg.wgrad_repr_bound(x, g, s)).all()


# ================================================================================================ GPU 3: the stage kernel
def _same_bits(got, want, what=''):
    """Equal in every bit (the sign of a zero included) where ``want`` is a number, NaN where it is NaN."""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ': NaN pattern'
    a = torch.where(nan, torch.zeros_like(got), got).view(torch.int32)
    b = torch.where(nan, torch.zeros_like(want), want).view(torch.int32)
    assert torch.equal(a, b), '%s: %d elements differ' % (what, int((a != b).sum()))


def _stage_rect_guarded(g, rects, amax):
    """``ops.conv_grad_stage_rect`` with gs inside a guarded pool (the wrapper's checks, the entry called by hand)."""
    from rmnet_amd import _lib, ops
    d = g.device
    N, C, H, W = g.shape
    if g.is_contiguous(memory_format=torch.channels_last):
        layout, sn, sc = 0, 0, 0
    else:
        layout, (sn, sc) = 1, ops._planes_strides(g)
    pool, flat = _guarded(g.numel(), d)
    sc_pool, g_scale = _guarded(4, d)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(d):
        rc = _lib.load().rmnet_conv_grad_stage_rect_f32(p(g), layout, sn, sc, p(rects), p(amax), N, C, H, W, p(flat), p(g_scale),
                                                        ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert _guards_intact(pool, g.numel(), nan_inside=True) and bool(torch.isnan(sc_pool[:GUARD]).all()) and bool(torch.isnan(sc_pool[GUARD + 2:]).all())
    return flat.view(N, H, W, C).permute(0, 3, 1, 2), g_scale[:2]


def _stage_want(g, rects, s):
    """torch.where + ldexp on the CPU: the select and the exact scale."""
    g = g.cpu()
    m = ref.inside(None if rects is None else rects.cpu().tolist(), g.shape[0], g.shape[2], g.shape[3])
    return torch.where(m, torch.ldexp(g, torch.tensor(s)), torch.zeros((), dtype=torch.float32))


def _rect_cases(n, h, w):
    one = lambda r: [r] * n
    yield 'none', None
    yield 'whole', one((0, w - 1, 0, h - 1))
    yield 'cell', one((w // 2, w // 2, h // 2, h // 2))
    yield 'row', one((0, w - 1, h - 1, h - 1))
    yield 'column', one((0, 0, 0, h - 1))
    yield 'empty', one((1, 0, 1, 0))
    yield 'beyond', one((-5, w + 3, -1, h + 9))
    yield 'per image', [(i % w, w - 1, 0, max(0, h - 1 - i)) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['channels_last', 'nchw', 'slice0', 'slice2'])
@pytest.mark.parametrize('c,n,h,w', [(128, 1, 1, 1), (512, 2, 3, 5), (128, 3, 16, 16), (512, 3, 30, 30), (132, 2, 9, 13)])
def test_the_stage_kernel_is_the_select_and_the_scale_in_every_bit(layout, c, n, h, w):
    """Both layouts and a [:, :, t] slice of [N, C, 3, h, w]; C 132 and 9 x 13 pixels leave a partial channel tile and a partial
    pixel tile in the transpose; the rectangles of ``_rect_cases``; NaN and Inf planted just outside and just inside one."""
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(c + h)
    if layout.startswith('slice'):
        src = (torch.randn(n, c, 3, h, w, generator=gen) * 1e-5).to(d)
        g = src[:, :, int(layout[-1])]
    else:
        g = (torch.randn(n, c, h, w, generator=gen) * 1e-5).to(d)
        g = cl(g) if layout == 'channels_last' else g
    amax = torch.linalg.vector_norm(g, INF)
    s = cg.stage_exponent(float(amax))
    for name, rects in _rect_cases(n, h, w):
        r = None if rects is None else torch.tensor(rects, dtype=torch.int32, device=d)
        gs, sc = _stage_rect_guarded(g, r, amax)
        _same_bits(gs, _stage_want(g, r, s), name)
        assert float(sc[0]) == 2.0 ** s and float(sc[1]) == 1.0
        got, sc2 = ops.conv_grad_stage_rect(g, r)                                  # the wrapper: amax by its own reduction
        assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(sc2, sc)
        _same_bits(got, gs, name + ' (wrapper)')
    if h >= 3 and w >= 3:
        # NaN / Inf around the edges of (1, w - 2, 1, h - 2): outside they are not looked at, inside they come through
        r = torch.tensor([(1, w - 2, 1, h - 2)] * n, dtype=torch.int32, device=d)
        g2 = g.clone() if not layout.startswith('slice') else src.clone()[:, :, int(layout[-1])]
        g2[0, 0, 0, 1], g2[0, 1, 1, 0], g2[n - 1, c - 1, h - 1, w - 2], g2[0, 2, h - 2, w - 1] = NAN, INF, -INF, NAN     # outside
        g2[0, 4, 1, 1], g2[n - 1, 5, h - 2, w - 2] = NAN, INF                                                              # inside
        gs, _ = _stage_rect_guarded(g2, r, amax)
        want = _stage_want(g2, r, s)
        _same_bits(gs, want, 'planted')
        assert int(torch.isnan(gs).sum()) == 1 and int(torch.isinf(gs).sum()) == 1


@pytest.mark.gpu
@pytest.mark.parametrize('amax', [0.0, 2.0 ** -149, 1e-40, 2.0 ** -118, 1.0, 3.0e38, INF, NAN])
def test_the_stage_rect_kernel_computes_the_exponent_of_the_restatement(amax):
    from rmnet_amd import ops
    d = dev()
    a32 = float(np.float32(amax))
    g = torch.zeros(2, 128, 2, 3)
    g[0, 0, 0, 0] = a32
    g[0, 1, 0, 0] = -a32 / 2 if np.isfinite(a32) else 1.0
    g[1, 2, 1, 2] = a32 / 8 if np.isfinite(a32) else -2.0
    s = cg.stage_exponent(a32)
    assert s == int(ops.conv_grad_stage_exponent(torch.tensor(a32)))
    rects = torch.tensor([(0, 2, 0, 1), (0, 1, 0, 1)], dtype=torch.int32, device=d)         # (1, 2, 1, 2) lies outside image 1's
    for gd in (g.to(d), cl(g.to(d))):
        gs, sc = ops.conv_grad_stage_rect(gd, rects, torch.tensor(a32, device=d))
        assert float(sc[0]) == 2.0 ** min(s, 126) and float(sc[1]) == 2.0 ** (s - min(s, 126))
        want = torch.ldexp(g.double(), torch.tensor(float(s), dtype=torch.float64))
        want[1, 2, 1, 2] = 0.0
        _same_bits(gs.double(), want)
        if 0 < a32 < INF:
            assert 2.0 ** 8 <= float(gs.abs().max()) < 2.0 ** 9
    with pytest.raises(RuntimeError):
        ops.conv_grad_stage_rect(g.to(d)[:, :, :, ::2])                                      # no dense planes
    with pytest.raises(RuntimeError):
        ops.conv_grad_stage_rect(g.to(d)[:, :126])                                           # C % 4


# ================================================================================================ GPU 4: the data gradient
def _kv_packs(wk, wv, d):
    from rmnet_amd import ops
    return ops.conv_split_dgrad_pack(wk.to(d)), ops.conv_split_dgrad_pack(wv.to(d))


@pytest.mark.gpu
def test_the_dgrad_pack_is_the_pack_of_the_flipped_transposed_weight():
    from rmnet_amd import ops
    d = dev()
    w = conv_ref.int_weights(128, 64, 3, 9).to(d)
    before = ops.conv_grad_launches['pack']
    wp, wu = ops.conv_split_dgrad_pack(w)
    assert ops.conv_grad_launches['pack'] == before + 1
    wp2, wu2 = ops.conv_split_pack(w.transpose(0, 1).flip(2, 3))
    assert torch.equal(wp, wp2) and torch.equal(wu, wu2) and wu.numel() == 64
    back = conv_ref.unpack_conv_weights(wp.cpu(), wu.cpu(), 64, 128, 3)
    assert torch.equal(back, w.cpu().double().transpose(0, 1).flip(2, 3))
    for bad in (torch.zeros(128, 32, 3, 3), torch.zeros(16, 64, 3, 3), torch.zeros(128, 64, 1, 1)):
        with pytest.raises(RuntimeError):
            ops.conv_split_dgrad_pack(bad)


@pytest.mark.gpu
@pytest.mark.parametrize('n,h,w,ek,ev', [(1, 1, 1, 0, 0), (2, 5, 7, -3, -40), (1, 3, 129, -25, 4)])
def test_kv_dgrad_returns_integer_arithmetic_in_every_bit(n, h, w, ek, ev):
    """Cin 64, heads 128 + 512; the two heads' gradients at very different exponents, each staged with its own scale."""
    from rmnet_amd import ops
    d = dev()
    wk, wv = conv_ref.int_weights(128, 64, 3, 11), conv_ref.int_weights(512, 64, 3, 12)
    gk, gv = cg.pow2_grads((n, 128, h, w), 3 + h, ek), cg.pow2_grads((n, 512, h, w), 4 + h, ev)
    x0 = torch.zeros(n, 64, h, w)
    want_k, want_v = cg.grads64(x0, wk, gk)[0], cg.grads64(x0, wv, gv)[0]
    packs = _kv_packs(wk, wv, d)
    gsk, sk = ops.conv_grad_stage_rect(gk.to(d))
    gsv, sv = ops.conv_grad_stage_rect(cl(gv.to(d)))
    assert float(sk[0]) == 2.0 ** (8 - ek) and float(sv[0]) == 2.0 ** (8 - ev)
    rw = torch.zeros(1, dtype=torch.int32, device=d)
    before = ops.conv_grad_launches['dgrad']
    got = ops.kv_dgrad(gsk, sk, gsv, sv, packs, rw)
    assert ops.conv_grad_launches['dgrad'] == before + 2
    assert got.is_contiguous(memory_format=torch.channels_last) and int(rw) == 0
    # (the sum of two exact integers times different powers of two is rounded once, by the second call's epilogue)
    assert torch.equal(got.cpu().double(), (want_k.float().double() + want_v).float().double())
    assert torch.equal(ops.kv_dgrad(gsk, sk, None, None, packs).cpu().double(), want_k)
    assert torch.equal(ops.kv_dgrad(None, None, gsv, sv, packs).cpu().double(), want_v)
    with pytest.raises(RuntimeError):
        ops.kv_dgrad(None, None, None, None, packs)


def _dgrad_chain_restate(gk, gv, packs, cin):
    """(T, bound) of the chain of two conv_split calls on the staged gradients: conv_ref's restatement and kernel bound, the second
    call with the first one's result as ``res``."""
    total_t, total_b, res = None, None, None
    for g, (wp, wu) in ((gk, packs[0]), (gv, packs[1])):
        gs64, s = cg.stage64(g)
        h, l = conv_ref.split_act(gs64)
        cg_in = g.shape[1]
        wh, wl = conv_ref.unpack_conv(wp.cpu(), cin, cg_in, 3)
        us = wu.cpu().double() * 2.0 ** -s
        t, a = conv_ref.restate(h, l, wh, wl, us, 1, 1, res=res)
        b = conv_ref.kernel_bound(9 * cg_in, a, t, res=res)
        total_b = b if total_b is None else total_b * (1 + 2.0 ** -20) + b       # (the second call reads the first one's rounded result)
        total_t = res = t
    return total_t, total_b


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['1e-8', '1', 'mixed'])
def test_kv_dgrad_is_within_the_derived_bound_of_the_restated_chain(kind):
    from rmnet_amd import ops
    d = dev()
    n, h, w, cin = 1, 5, 7, 64
    wk, wv = conv_ref.uniform_weights(128, cin, 3, 8), conv_ref.uniform_weights(512, cin, 3, 9)
    gk, gv = _random_g(kind, (n, 128, h, w), 77), _random_g(kind, (n, 512, h, w), 78) * 2.0 ** -14
    packs = _kv_packs(wk, wv, d)
    gsk, sk = ops.conv_grad_stage_rect(gk.to(d))
    gsv, sv = ops.conv_grad_stage_rect(gv.to(d))
    got = ops.kv_dgrad(gsk, sk, gsv, sv, packs).cpu().double()
    T, bound = _dgrad_chain_restate(gk, gv, packs, cin)
    print('dX: largest error / bound %.3f' % ((got - T).abs() / bound.clamp_min(1e-300)).max())
    assert ((got - T).abs() <= bound).all()
    x0 = torch.zeros(n, cin, h, w)
    truth = cg.grads64(x0, wk, gk)[0] + cg.grads64(x0, wv, gv)[0]
    assert (got - truth).abs().max() <= 2.0 ** -18 * truth.abs().max()           # (wiring: the flipped packs against the plain formula)


# ================================================================================================ GPU 5: the module under autograd
def _kv_module(cin, d, seed=0, keydim=128, valdim=512):
    from rmnet_amd import networks
    kv = networks.KeyValue(cin, keydim, valdim)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in kv.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.05 if p.dim() == 1 else (2.0 / (9 * cin)) ** 0.5))
    kv = kv.to(d).eval()
    networks.fuse_epilogues_(kv)
    return kv.to(memory_format=torch.channels_last)


def _module_bounds(x, kv, gk, gv, rects, regional):
    """(truth, bound) per gradient: the float64 restatement and restated bound + representation bound of the kernels' arithmetic."""
    from rmnet_amd import ops
    wk, wv = kv.key_conv.weight.detach().cpu(), kv.value_conv.weight.detach().cpu()
    r = rects if regional else None
    truth = ref.kv_grads64(x, wk, wv, gk, gv, r)
    bounds = {}
    n, cin, h, w = x.shape
    for name, wt, g in (('k', wk, gk), ('v', wv, gv)):
        G = ref.masked(g, r)
        # the device stages with the largest |element| of the gradient as it arrives (before the mask)
        s = cg.stage_exponent(float(g.abs().max()))
        gs64 = G * 2.0 ** s
        plan = ops.conv3x3_wgrad_plan(n * h * w, cin, wt.shape[0])
        T, ahh, ax, Tb, Ab = cg.wgrad_restate(x, gs64, s, plan)
        bounds['dW' + name] = cg.acc_bound(plan[2], plan[1], ahh, ax) + cg.wgrad_repr_bound(x, G, s)
        bounds['db' + name] = cg.bias_bound(plan[2] // BIAS_SPLIT, plan[1] * BIAS_SPLIT, Ab) + 2.0 ** -40 * Ab
    # dX: the chain's bound on the packs of the weights + the representation error of the gradient's and the weights' split
    d = kv.key_conv.weight.device
    packs = _kv_packs(wk, wv, d)
    Gk, Gv = ref.masked(gk, r), ref.masked(gv, r)
    total_t, total_b, res = None, None, None
    rep = torch.zeros(n, cin, h, w, dtype=torch.float64)
    for g_raw, G, wt, (wp, wu) in ((gk, Gk, wk, packs[0]), (gv, Gv, wv, packs[1])):
        s = cg.stage_exponent(float(g_raw.abs().max()))
        hh, ll = conv_ref.split_act(G * 2.0 ** s)
        wh, wl = conv_ref.unpack_conv(wp.cpu(), cin, G.shape[1], 3)
        us = wu.cpu().double() * 2.0 ** -s
        t, a = conv_ref.restate(hh, ll, wh, wl, us, 1, 1, res=res)
        b = conv_ref.kernel_bound(9 * G.shape[1], a, t, res=res)
        total_b = b if total_b is None else total_b * (1 + 2.0 ** -20) + b
        total_t = res = t
        wflip = wt.double().transpose(0, 1).flip(2, 3)
        rep = rep + conv_ref.repr_bound(G * 2.0 ** s, wflip, 1, 1) * 2.0 ** -s
    bounds['dX'] = total_b + rep
    return truth, bounds


@pytest.mark.gpu
@pytest.mark.parametrize('leaf', [True, False])
@pytest.mark.parametrize('regional', [False, True])
@pytest.mark.parametrize('cin', [64, 1024])
def test_the_heads_under_autograd_give_the_float64_gradients(cin, regional, leaf):
    from rmnet_amd import ops
    d = dev()
    kv = _kv_module(cin, d, seed=cin).device_grad_()
    n, h, w = 2, 4, 6
    gen = torch.Generator().manual_seed(3 + cin)
    x = torch.randn(n, cin, h, w, generator=gen)
    ck, cv = torch.randn(n, 128, h, w, generator=gen), torch.randn(n, 512, h, w, generator=gen) * 2.0 ** -15
    rects_l = [(1, 4, 0, 2), (2, 3, 3, 3)]
    rects = torch.tensor(rects_l, dtype=torch.int32, device=d) if regional else None
    xd = cl(x.to(d)).requires_grad_(True)
    xin = xd if leaf else xd * 1.0
    for p in kv.parameters():
        p.grad = None
    ops.conv_grad_range_word(d).zero_()
    fwd_word = int(ops.conv_range_word(d))
    key, val = kv(xin, rects)
    assert key.grad_fn is not None and type(key.grad_fn).__name__ == '_KeyValueFnBackward'
    with torch.no_grad():
        k0, v0 = kv(xd.detach(), rects)
    _same_bits(key, k0, 'key')
    _same_bits(val, v0, 'value')
    (key * ck.to(d)).sum().add((val * cv.to(d)).sum()).backward()
    truth, bounds = _module_bounds(x, kv, ck, cv, rects_l, regional)
    got = dict(dX=xd.grad, dWk=kv.key_conv.weight.grad, dbk=kv.key_conv.bias.grad, dWv=kv.value_conv.weight.grad, dbv=kv.value_conv.bias.grad)
    for k, want in truth.items():
        err = (got[k].cpu().double() - want).abs()
        print('%s: largest error / bound %.3f' % (k, (err / bounds[k].clamp_min(1e-300)).max()))
        assert (err <= bounds[k]).all(), k
    assert int(ops.conv_grad_range_word(d)) == 0 and int(ops.conv_range_word(d)) == fwd_word
    if regional:
        # more than one cell outside the rectangle nothing arrives: exactly +0.0
        m = ref.inside([(c0 - 1, c1 + 1, r0 - 1, r1 + 1) for c0, c1, r0, r1 in rects_l], n, h, w).expand(n, cin, h, w)
        far = xd.grad.cpu()[~m]
        assert far.numel() > 0 and torch.equal(far.view(torch.int32), torch.zeros_like(far).view(torch.int32))


# ================================================================================================ GPU 6: launches and paths
def _reset():
    from rmnet_amd import ops
    for k in ops.conv_grad_launches:
        ops.conv_grad_launches[k] = 0
    return ops.conv_grad_launches


@pytest.mark.gpu
def test_only_what_is_needed_is_launched_and_nothing_requiring_grad_means_no_graph():
    from rmnet_amd import ops
    d = dev()
    kv = _kv_module(64, d)
    x = cl(torch.randn(2, 64, 4, 6, generator=torch.Generator().manual_seed(1)).to(d))
    rects = torch.tensor([(1, 4, 0, 2), (0, 5, 1, 3)], dtype=torch.int32, device=d)
    with torch.no_grad():
        k0, v0 = kv(x, rects)
    # without device_grad_(): today's path, nothing recorded by the device function
    key, val = kv(x.clone().requires_grad_(True), rects)
    assert key.grad_fn is None or type(key.grad_fn).__name__ != '_KeyValueFnBackward'
    kv.device_grad_()
    assert kv.device_grad_() is kv
    # nothing requires grad: no graph, the same bits
    for p in kv.parameters():
        p.requires_grad_(False)
    n = _reset()
    key, val = kv(x, rects)
    assert key.grad_fn is None and val.grad_fn is None and not key.requires_grad
    _same_bits(key, k0)
    _same_bits(val, v0)
    assert n == {'stage': 0, 'wgrad': 0, 'dgrad': 0, 'pack': 0}
    # x alone: two stage passes, two dgrad calls, the packs once
    xg = x.clone().requires_grad_(True)
    key, val = kv(xg, rects)
    _same_bits(key, k0)
    (key.sum() + val.sum()).backward()
    assert n == {'stage': 2, 'wgrad': 0, 'dgrad': 2, 'pack': 2} and xg.grad is not None
    # only value used downstream: no key-head launch
    _reset()
    xg = x.clone().requires_grad_(True)
    for p in kv.parameters():
        p.requires_grad_(True)
        p.grad = None
    key, val = kv(xg, rects)
    val.sum().backward()
    assert n == {'stage': 1, 'wgrad': 1, 'dgrad': 1, 'pack': 0}
    assert kv.key_conv.weight.grad is None and kv.key_conv.bias.grad is None and kv.value_conv.weight.grad is not None
    # a bias-only request runs no GEMM; frozen x: no dgrad, no pack
    _reset()
    for p in kv.parameters():
        p.grad = None
    kv.key_conv.weight.requires_grad_(False)
    kv.value_conv.weight.requires_grad_(False)
    key, val = kv(x, rects)
    (key * 2.0).sum().add(val.sum()).backward()
    assert n == {'stage': 2, 'wgrad': 0, 'dgrad': 0, 'pack': 0}
    with torch.no_grad():
        m = ref.inside(rects.cpu().tolist(), 2, 4, 6).to(d)
    assert torch.equal(kv.key_conv.bias.grad, torch.full((128,), 2.0 * float(m[0].sum() + m[1].sum()), device=d))
    assert torch.equal(kv.value_conv.bias.grad, torch.full((512,), float(m[0].sum() + m[1].sum()), device=d))
    # train() takes the same path (no BatchNorm here); the switch off: not recorded by the device function
    kv.train()
    key, _ = kv(x, rects)
    assert type(key.grad_fn).__name__ == '_KeyValueFnBackward'
    _same_bits(key, k0)
    kv.eval().device_grad_(False)
    key, _ = kv(x, rects)
    assert type(key.grad_fn).__name__ != '_KeyValueFnBackward'


@pytest.mark.gpu
def test_double_backward_is_refused():
    d = dev()
    kv = _kv_module(64, d).device_grad_()
    x = cl(torch.randn(1, 64, 3, 5, generator=torch.Generator().manual_seed(2)).to(d)).requires_grad_(True)
    key, val = kv(x)
    (gx,) = torch.autograd.grad(key.sum() + val.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


@pytest.mark.gpu
def test_two_backward_calls_and_a_graph_replay_return_the_same_bits():
    from rmnet_amd import ops
    d = dev()
    kv = _kv_module(64, d).device_grad_()
    gen = torch.Generator().manual_seed(4)
    x = cl(torch.randn(2, 64, 16, 16, generator=gen).to(d))
    ck, cv = torch.randn(2, 128, 16, 16, generator=gen).to(d), torch.randn(2, 512, 16, 16, generator=gen).to(d)
    rects = torch.tensor([(1, 9, 0, 12), (3, 15, 2, 15)], dtype=torch.int32, device=d)
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        for p in kv.parameters():
            p.grad = None
        key, val = kv(xg, rects)
        ((key * ck).sum() + (val * cv).sum()).backward()
        runs.append([xg.grad.clone()] + [p.grad.clone() for p in kv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # one captured-graph replay of the three backward entries (each ran eagerly above: the LDS attribute is set)
    packs = (ops.conv_split_dgrad_pack(kv.key_conv.weight), ops.conv_split_dgrad_pack(kv.value_conv.weight))
    grw = ops.conv_grad_range_word(d)
    gk, gv = (ck * ref.inside(rects.cpu().tolist(), 2, 16, 16).to(d)).contiguous(), cl(cv)
    amax_k, amax_v = torch.linalg.vector_norm(gk, INF), torch.linalg.vector_norm(gv, INF)

    def backward_entries():
        gsk, sk = ops.conv_grad_stage_rect(gk, rects, amax_k)
        gsv, sv = ops.conv_grad_stage_rect(gv, rects, amax_v)
        dwk, dbk = ops.conv3x3_wgrad(x, gsk, sk, range_word=grw)
        dwv, dbv = ops.conv3x3_wgrad(x, gsv, sv, range_word=grw)
        return [ops.kv_dgrad(gsk, sk, gsv, sv, packs, grw), dwk, dbk, dwv, dbv]

    eager = [t.clone() for t in backward_entries()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = backward_entries()
    torch.cuda.current_stream(d).wait_stream(side)
    for t in outs:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_the_packs_follow_an_in_place_weight_update_and_are_not_rebuilt_without_one():
    from rmnet_amd import networks, ops
    d = dev()
    kv = _kv_module(64, d).device_grad_()
    x = cl(torch.randn(1, 64, 3, 5, generator=torch.Generator().manual_seed(6)).to(d))

    def step():
        xg = x.clone().requires_grad_(True)
        key, val = kv(xg)
        (key.sum() + val.sum()).backward()
        return key.detach().clone(), val.detach().clone(), xg.grad.clone()

    n = _reset()
    k1, v1, g1 = step()
    first = n['pack']
    assert first == 2
    wp = kv._wp
    k2, v2, g2 = step()
    assert n['pack'] == first and kv._wp is wp                                     # cached
    _same_bits(k2, k1)
    _same_bits(g2, g1)
    with torch.no_grad():
        kv.value_conv.weight.mul_(2.0)                                             # an optimiser step on one head
        kv.key_conv.bias.add_(1.0)
    k3, v3, g3 = step()
    assert n['pack'] == first + 2 and kv._wp is not wp
    fresh = copy.deepcopy(kv)                                                      # the same parameters, packed from scratch
    networks.fuse_epilogues_(fresh)
    with torch.no_grad():
        kf, vf = fresh(x)
    _same_bits(k3, kf, 'key after the update')
    _same_bits(v3, vf, 'value after the update')
    k4, v4, g4 = step()
    assert n['pack'] == first + 2
    _same_bits(g4, g3)
    assert not torch.equal(g3, g1)


@pytest.mark.gpu
def test_bad_values_are_counted_in_the_backward_word_and_the_forward_word_is_left_alone():
    from rmnet_amd import ops
    d = dev()
    kv = _kv_module(64, d).device_grad_()
    gen = torch.Generator().manual_seed(8)
    x = cl(torch.randn(1, 64, 4, 6, generator=gen).to(d)).requires_grad_(True)
    grw, frw = ops.conv_grad_range_word(d), ops.conv_range_word(d)
    grw.zero_()
    key, val = kv(x)
    fwd = int(frw)
    (key.sum() + val.sum()).backward()
    assert int(grw) == 0 and int(frw) == fwd
    # a staged gradient pushed outside the window by a lying amax: 4 elements of the key head at 2^12 times the claimed maximum
    gk = torch.randn(1, 128, 4, 6, generator=gen).to(d) * 1e-3
    gk[0, 7, 1, 1], gk[0, 8, 1, 2], gk[0, 9, 0, 0], gk[0, 127, 3, 5] = 16.0, -16.0, NAN, INF
    gs, sc = ops.conv_grad_stage_rect(gk, None, torch.tensor(4e-3, device=d))
    assert int(grw) == 0                                                           # the stage pass counts nothing
    ops.conv3x3_wgrad(x.detach(), gs, sc, range_word=grw)
    assert int(grw) == 4 and int(frw) == fwd                                       # once per element, whatever the channel tiles
    grw.zero_()
    packs = _kv_packs(kv.key_conv.weight.detach().cpu(), kv.value_conv.weight.detach().cpu(), d)
    ops.kv_dgrad(gs, sc, None, None, packs, grw)
    assert int(grw) == 4 and int(frw) == fwd
    # a bad activation is counted once too, in the first output-channel tile only (640 outputs: three tiles)
    grw.zero_()
    xb = x.detach().clone()
    xb[0, 5, 2, 2] = 5000.0
    g640 = cl(torch.randn(1, 640, 4, 6, generator=gen).to(d))
    gs, sc = ops.conv_grad_stage_rect(g640)
    ops.conv3x3_wgrad(xb, gs, sc, range_word=grw)
    assert int(grw) == 1 and int(frw) == fwd
    grw.zero_()


# ================================================================================================ GPU 7: the chain
@pytest.mark.gpu
def test_one_backward_runs_from_the_memory_read_into_both_heads_and_both_r4():
    """r4 leaves -> kv_memory and kv_query -> ops.memory_read with rectangles -> sum(mem_val * c): every gradient is, in every
    bit, what memory_read_backward's four outputs give when fed by hand into the three backward entries."""
    from rmnet_amd import ops
    d = dev()
    no, T, h, w, cin = 2, 2, 4, 6, 64
    kvm, kvq = _kv_module(cin, d, 1).device_grad_(), _kv_module(cin, d, 2).device_grad_()
    gen = torch.Generator().manual_seed(10)
    r4m = [cl(torch.randn(no, cin, h, w, generator=gen).to(d)).requires_grad_(True) for _ in range(T)]
    r4q = cl(torch.randn(no, cin, h, w, generator=gen).to(d)).requires_grad_(True)
    c = torch.randn(no, 1024, h, w, generator=gen).to(d)
    mem_rects = torch.tensor([[(1, 4, 0, 2), (0, 3, 1, 3)], [(2, 5, 1, 3), (1, 5, 0, 3)]], dtype=torch.int32, device=d)   # [no, T, 4]
    qry_rects = torch.tensor([(0, 4, 0, 3), (1, 5, 1, 2)], dtype=torch.int32, device=d)
    for p in list(kvm.parameters()) + list(kvq.parameters()):
        p.grad = None
    kvs = [kvm(r4m[t], mem_rects[:, t].contiguous()) for t in range(T)]
    m_key = torch.stack([k for k, _ in kvs], dim=2)
    m_val = torch.stack([v for _, v in kvs], dim=2)
    q_key, q_val = kvq(r4q, qry_rects)
    mem_val, _ = ops.memory_read(m_key, m_val, q_key, q_val, mem_rects, qry_rects)
    (mem_val * c).sum().backward()
    got = [t.grad for t in r4m] + [r4q.grad] + [p.grad for p in kvm.parameters()] + [p.grad for p in kvq.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in got)
    assert all(float(g.abs().max()) > 0 for g in got)
    # by hand
    with torch.no_grad():
        d_mk, d_mv, d_qk, d_qv = ops.memory_read_backward(m_key.detach(), m_val.detach(), q_key.detach(), q_val.detach(), mem_val.detach(),
                                                          c.contiguous(), mem_rects, qry_rects)
        grw = ops.conv_grad_range_word(d)

        def head(kv, x, gk, gv, rects):
            gsk, sk = ops.conv_grad_stage_rect(gk, rects)
            gsv, sv = ops.conv_grad_stage_rect(gv, rects)
            dwk, dbk = ops.conv3x3_wgrad(x.detach(), gsk, sk, range_word=grw)
            dwv, dbv = ops.conv3x3_wgrad(x.detach(), gsv, sv, range_word=grw)
            packs = (ops.conv_split_dgrad_pack(kv.key_conv.weight), ops.conv_split_dgrad_pack(kv.value_conv.weight))
            return ops.kv_dgrad(gsk, sk, gsv, sv, packs, grw), [dwk, dbk, dwv, dbv]

        want_x, want_p = [], None
        for t in range(T):
            dx, dp = head(kvm, r4m[t], d_mk[:, :, t], d_mv[:, :, t], mem_rects[:, t].contiguous())
            want_x.append(dx)
            want_p = dp if want_p is None else [a + b for a, b in zip(want_p, dp)]     # (autograd adds the frames in this order)
        dxq, dpq = head(kvq, r4q, d_qk, d_qv, qry_rects)
    want = want_x + [dxq] + want_p + dpq
    names = ['r4 memory %d' % t for t in range(T)] + ['r4 query'] + ['memory ' + k for k in ('dWk', 'dbk', 'dWv', 'dbv')] + \
        ['query ' + k for k in ('dWk', 'dbk', 'dWv', 'dbv')]
    for name, a, b in zip(names, got, want):
        _same_bits(a, b, name)                   # (memory parameters: the sum of two frames, the same bits in either order)
