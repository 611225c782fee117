# -*- coding: utf-8 -*-
"""The gradients of the decoder's 3x3 convolutions: the data gradient (the forward kernel on flipped packs), the weight / bias gradient
(csrc/conv3x3_wgrad.hip), the stage pass, ``ops.conv3x3_split`` under autograd and ``Decoder.device_grad_``.

CPU part: the float64 restatement (tests/conv_grad_ref.py) pinned by hand and by torch autograd, the kernel arithmetic's bound and its
power, the dgrad pack, the staging exponent, eight planted faults, the C entries' refusals, the compiler's resources.
GPU part: an exact family (every bit), a random family (the derived per-element bound), determinism, the range word, autograd, the
module against float64 with the library route as yardstick, repacking, and the chain loss -> tail -> decoder."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as ref
import conv_ref
from conftest import ROOT

# the kernel's constants, restated (csrc/conv3x3_wgrad.hip; exported by rmnet_amd.ops)
CT, KT, SUB, MAX_W, RANGE_MIN, MAX_RANGES, TARGET_WGS = 16, 32, 512, 448, 256, 64, 768
BIAS_SPLIT = 8
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
NAN = float('nan')


def dev():
    return torch.device('cuda', 0)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def test_the_constants_are_the_ones_ops_exports_and_the_plan_is_what_it_says():
    from rmnet_amd import ops
    assert (ops.WGRAD_CT, ops.WGRAD_KT, ops.WGRAD_SUB, ops.WGRAD_MAX_W) == (CT, KT, SUB, MAX_W)
    assert (ops.WGRAD_RANGE_MIN, ops.WGRAD_MAX_RANGES, ops.WGRAD_TARGET_WGS, ops.WGRAD_BIAS_SPLIT) == (RANGE_MIN, MAX_RANGES, TARGET_WGS, BIAS_SPLIT)
    assert ops.conv3x3_wgrad_plan(1, 32) == (2, 1, 32)
    assert ops.conv3x3_wgrad_plan(256, 32) == (2, 1, 256) and ops.conv3x3_wgrad_plan(257, 32) == (2, 2, 160)
    assert ops.conv3x3_wgrad_plan(2 * 129 * 128, 32) == (2, 61, 544)            # ranges longer than one activation image
    assert ops.conv3x3_wgrad_plan(12 * 120 * 120, 256) == (16, 48, 3616) and ops.conv3x3_wgrad_plan(12 * 900, 1024) == (64, 12, 928)
    for pixels in (1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 33024, 172800):
        for cin in (32, 64, 256, 512, 1024):
            nct, nr, rl = ops.conv3x3_wgrad_plan(pixels, cin)
            assert nct == cin // CT and 1 <= nr <= MAX_RANGES and rl % KT == 0 and (nr - 1) * rl < pixels <= nr * rl


# ================================================================================================ CPU 1: the restatement
def test_the_restatement_gives_the_hand_written_answers():
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    # one pixel: only the centre tap sees it
    w = torch.arange(1.0, 10.0).view(1, 1, 3, 3)
    dX, dW, db, gr = ref.grads64(t([[[[3.0]]]]), w, t([[[[5.0]]]]))
    want = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    want[0, 0, 1, 1] = 15.0
    assert torch.equal(dW, want) and db.item() == 5.0 and dX.item() == 5.0 * 5.0 and gr.item() == 5.0
    # one live tap: x only at (0, 0), g only at (1, 1) of a 3 x 3 map: pixel (1, 1) sees (0, 0) through tap (0, 0)
    x = torch.zeros(1, 1, 3, 3)
    g = torch.zeros(1, 1, 3, 3)
    x[0, 0, 0, 0], g[0, 0, 1, 1] = 2.0, 7.0
    dX, dW, db, _ = ref.grads64(x, w, g)
    want = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    want[0, 0, 0, 0] = 14.0
    assert torch.equal(dW, want) and db.item() == 7.0
    assert torch.equal(dX[0, 0], 7.0 * w[0, 0].double())                         # pixel (1, 1) read (y, x) through tap (y, x)
    # a corner pixel: the taps that leave the map see zeros
    dX, dW, db, _ = ref.grads64(torch.ones(1, 1, 2, 2), w, t([[[[1.0, 0.0], [0.0, 0.0]]]]))
    assert torch.equal(dW[0, 0], t([[0.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 1.0, 1.0]]))
    assert torch.equal(dX[0, 0], t([[5.0, 6.0], [8.0, 9.0]]))
    # the masks: a dead output passes nothing, a dead input receives nothing
    x = t([[[[-1.0, 2.0]]]])
    dX, dW, db, gr = ref.grads64(x, w, t([[[[1.0, 1.0]]]]), b=t([-11.0]), relu_in=True, relu_out=True)
    # pre = (0, 2): out = relu(6 * 2 - 11, 5 * 2 - 11) = (1, 0): only pixel 0 is live, and it saw pre(x)[1] = 2 through tap (1, 2)
    assert torch.equal(gr, t([[[[1.0, 0.0]]]])) and db.item() == 1.0
    want = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    want[0, 0, 1, 2] = 2.0
    assert torch.equal(dW, want) and torch.equal(dX, t([[[[0.0, 6.0]]]]))


def _autograd64(x, w, g, b, res, relu_in, relu_out):
    x, w, b, res = (None if v is None else v.double().clone().requires_grad_(True) for v in (x, w, b, res))
    out = F.conv2d(F.relu(x) if relu_in else x, w, b, 1, 1)
    if res is not None:
        out = out + res
    if relu_out:
        out = F.relu(out)
    out.backward(g.double())
    return x.grad, w.grad, None if b is None else b.grad, None if res is None else res.grad


def _case(seed, n=2, cin=4, cout=4, h=5, w=6):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    return r(n, cin, h, w), r(cout, cin, 3, 3) * 0.3, r(n, cout, h, w), r(cout) * 0.2, r(n, cout, h, w)


@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('relu_out', [False, True])
@pytest.mark.parametrize('with_res', [False, True])
def test_the_restatement_is_torch_autograd_in_float64(relu_in, relu_out, with_res):
    x, w, g, b, res = _case(3, cin=4, cout=6)
    res = res if with_res else None
    want = _autograd64(x, w, g, b, res, relu_in, relu_out)
    dX, dW, db, gr = ref.grads64(x, w, g, b, res, relu_in, relu_out)
    for got, ex in ((dX, want[0]), (dW, want[1]), (db, want[2])) + (((gr, want[3]),) if with_res else ()):
        assert (got - ex).abs().max() <= 1e-12 * max(1.0, ex.abs().max().item())


# ================================================================================================ CPU 2: the planted faults
# fault -> (what makes it show, which output shows it)
FAULT_CASES = {
    'unflipped_tap': (dict(), 'dX'),
    'untransposed_weight': (dict(), 'dX'),
    'no_out_mask': (dict(relu_out=True), 'dW'),
    'no_x_mask': (dict(relu_in=True), 'dX'),
    'res_dropped': (dict(res=True), 'grad_res'),
    'db_wrong_mask': (dict(relu_out=True), 'db'),
    'no_zero_pad': (dict(), 'dW'),
}


@pytest.mark.parametrize('fault', sorted(FAULT_CASES))
def test_a_planted_fault_in_the_gradients_is_caught(fault):
    """Each fault moves the output it belongs to away from autograd's by an amount of order 1; the clean restatement agrees to 1e-12."""
    kw, where = FAULT_CASES[fault]
    x, w, g, b, res = _case(11)                                                  # Cin == Cout: the transposed weight has the right shape
    res = res if kw.get('res') else None
    args = (x, w, g, b, res, kw.get('relu_in', False), kw.get('relu_out', False))
    want = dict(zip(('dX', 'dW', 'db', 'grad_res'), _autograd64(*args)))
    clean = dict(zip(('dX', 'dW', 'db', 'grad_res'), ref.grads64(x, w, g, b, res, args[5], args[6])))
    bad = dict(zip(('dX', 'dW', 'db', 'grad_res'), ref.grads64(x, w, g, b, res, args[5], args[6], fault=fault)))
    assert (clean[where] - want[where]).abs().max() <= 1e-12 * want[where].abs().max()
    assert (bad[where] - want[where]).abs().max() >= 0.05 * want[where].abs().max(), fault


def test_a_lost_partial_range_is_caught():
    """range_lost: the merge skips one range's partial.  Two ranges of 160 + 97 pixels; the loss is far outside the bound."""
    from rmnet_amd import ops
    gen = torch.Generator().manual_seed(5)
    x, G = torch.randn(1, 32, 1, 257, generator=gen), torch.randn(1, 8, 1, 257, generator=gen)
    plan = ops.conv3x3_wgrad_plan(257, 32)
    assert plan == (2, 2, 160)
    gs, s = ref.stage64(G)
    T, ahh, ax, Tb, Ab = ref.wgrad_restate(x, gs, s, plan)
    bound = ref.acc_bound(plan[2], plan[1], ahh, ax)
    truth = ref.grads64(x, torch.zeros(8, 32, 3, 3), G)
    assert ((T - truth[1]).abs() <= bound + ref.wgrad_repr_bound(x, G, s)).all() and (Tb - truth[2]).abs().max() < 1e-9
    for lost in (0, 1):
        Tl, _, _, Tbl, _ = ref.wgrad_restate(x, gs, s, plan, lose_range=lost)
        assert ((Tl - T).abs() > bound)[:, :, 1, 1].float().mean() > 0.99 and ((Tbl - Tb).abs() > ref.bias_bound(160 // BIAS_SPLIT, 2 * BIAS_SPLIT, Ab)).all()


# ================================================================================================ CPU 3: the arithmetic's bound
@pytest.mark.parametrize('mag', [1e-8, 1.0])
def test_the_restated_arithmetic_is_within_its_representation_bound_of_the_truth(mag):
    gen = torch.Generator().manual_seed(9)
    x, G = torch.randn(2, 32, 6, 7, generator=gen) * 3, torch.randn(2, 8, 6, 7, generator=gen) * mag
    gs, s = ref.stage64(G)
    assert 2.0 ** 8 <= gs.abs().max() < 2.0 ** 9
    T, ahh, ax, Tb, Ab = ref.wgrad_restate(x, gs, s, (2, 1, 96), relu_in=True)
    truth = ref.grads64(x, torch.zeros(8, 32, 3, 3), G, relu_in=True)
    assert ((T - truth[1]).abs() <= ref.wgrad_repr_bound(x, G, s, relu_in=True)).all()
    assert ((T - truth[1]).abs().max() > 0) and (Tb - truth[2]).abs().max() <= 1e-12 * mag * 84


def test_a_dropped_cross_term_at_a_short_reduction_is_outside_the_bound():
    """Non-vacuity: 32 pixels, one range.  Without gh * l (or gl * h) most elements leave the bound; with all three terms T is T."""
    gen = torch.Generator().manual_seed(2)
    x, G = torch.randn(1, 32, 4, 8, generator=gen), torch.randn(1, 16, 4, 8, generator=gen)
    gs, s = ref.stage64(G)
    T, ahh, ax, _, _ = ref.wgrad_restate(x, gs, s, (2, 1, 32))
    bound = ref.acc_bound(32, 1, ahh, ax)
    for drop in ('hl', 'lh'):
        Td = ref.wgrad_restate(x, gs, s, (2, 1, 32), drop=drop)[0]
        outside = ((Td - T).abs() > bound)[:, :, 1, 1]                           # the centre tap: all 32 pixels inside the map
        print('dropped %s: %.1f %% of the centre-tap elements outside the bound' % (drop, 100 * outside.float().mean()))
        assert outside.float().mean() > 0.5


# ================================================================================================ CPU 4: packs and staging
@pytest.mark.parametrize('cin', [256, 512])
def test_the_dgrad_pack_is_the_flipped_transposed_weight(cin):
    from rmnet_amd import ops
    w = conv_ref.uniform_weights(256, cin, 3, 21)
    packs = ops.conv3x3_dgrad_pack(w)
    assert len(packs) == cin // 256
    want = w.double().transpose(0, 1).flip(2, 3)
    for s, (wp, wu) in enumerate(packs):
        got = conv_ref.unpack_conv_weights(wp, wu, 256, 256, 3)                  # [ci][co][ky][kx]: 256 outputs (ci), 256 inputs (co)
        ex = want[256 * s:256 * (s + 1)]
        assert ((got - ex).abs() <= 2.0 ** -21 * ex.abs().amax(dim=(1, 2, 3), keepdim=True)).all()   # hi + lo: 22 bits of the row's top
    with pytest.raises(RuntimeError):
        ops.conv3x3_dgrad_pack(torch.zeros(256, 64, 3, 3))


def test_the_staging_exponent_puts_amax_into_the_window():
    from rmnet_amd import ops
    sub = float(np.float32(1e-40))
    for amax in (0.0, sub, float(np.float32(1e-8)), 1.0, float(np.float32(1e30)), float(np.finfo(np.float32).tiny), 2.0 ** -149,
                 float(np.finfo(np.float32).max), 255.99, 256.0, 511.9, 512.0):
        s = int(ops.conv_grad_stage_exponent(torch.tensor(amax, dtype=torch.float32)))
        assert s == ref.stage_exponent(amax)
        if amax == 0.0:
            assert s == 0
        else:
            assert 2.0 ** 8 <= np.ldexp(np.float64(amax), s) < 2.0 ** 9, (amax, s)
    for bad in (float('inf'), NAN):
        assert int(ops.conv_grad_stage_exponent(torch.tensor(bad))) == 0 == ref.stage_exponent(bad)


# ================================================================================================ CPU 5: refusals, resources
def _wgrad_refusals(good):
    inv, uns, wsp = E_INVALID, E_UNSUPPORTED, E_WORKSPACE
    yield 'null x', dict(x=0), inv
    yield 'null g', dict(g=0), inv
    yield 'null g_scale', dict(g_scale=0), inv
    yield 'null dw', dict(dw=0), inv
    yield 'N = 0', dict(N=0), inv
    yield 'H < 0', dict(H=-1), inv
    yield 'W = 0', dict(W=0), inv
    yield 'Cin = 0', dict(Cin=0), inv
    yield 'relu_out is no flag here', dict(flags=2), inv
    yield 'unknown flag', dict(flags=4), inv
    for k in ('x', 'g', 'g_scale', 'dw', 'db', 'ws'):
        yield 'misaligned ' + k, {k: good[k] + 4}, inv
    yield 'misaligned range word', dict(rw=good['rw'] + 2), inv
    yield 'dw overlaps x', dict(dw=good['x'] + 16), inv
    yield 'dw overlaps g', dict(dw=good['g'] + 16), inv
    yield 'db overlaps dw', dict(db=good['dw'] + 16), inv
    yield 'workspace overlaps dw', dict(ws=good['dw']), inv
    yield 'dw overlaps g_scale', dict(g_scale=good['dw'] + 32), inv
    yield 'workspace overlaps the range word', dict(rw=good['ws'] + 8), inv
    yield 'db overlaps g_scale', dict(g_scale=good['db'] + 16), inv
    yield 'Cin % 32', dict(Cin=48), uns
    yield 'W above the widest map', dict(W=MAX_W + 1), uns
    yield '2^31 elements', dict(N=1 << 12, H=1 << 7, W=1 << 4), uns
    yield 'null workspace', dict(ws=0), wsp
    yield 'short workspace', dict(ws_bytes=good['ws_bytes'] - 1), wsp


def _wgrad_call(lib, a):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.rmnet_conv3x3_wgrad_f32(p(a['x']), p(a['g']), p(a['g_scale']), a['flags'], a['N'], a['H'], a['W'], a['Cin'], p(a['dw']), p(a['db']),
                                       p(a['ws']), a['ws_bytes'], p(a['rw']), None)


def _stage_refusals(good):
    yield 'null g', dict(g=0), E_INVALID
    yield 'null amax', dict(amax=0), E_INVALID
    yield 'null gs', dict(gs=0), E_INVALID
    yield 'null g_scale', dict(g_scale=0), E_INVALID
    yield 'n = 0', dict(n=0), E_INVALID
    yield 'n % 4', dict(n=1022), E_INVALID
    yield 'misaligned g', dict(g=good['g'] + 4), E_INVALID
    yield 'misaligned act', dict(act=good['act'] + 8), E_INVALID
    yield 'misaligned amax', dict(amax=good['amax'] + 1), E_INVALID
    yield 'gs overlaps g partly', dict(gs=good['g'] + 16), E_INVALID
    yield 'gs overlaps act', dict(gs=good['act']), E_INVALID
    yield 'gs overlaps amax', dict(amax=good['gs'] + 64), E_INVALID
    yield 'n >= 2^31', dict(n=1 << 31), E_UNSUPPORTED


def _stage_call(lib, a):
    p = lambda v: ctypes.c_void_p(v) if v else None
    return lib.rmnet_conv_grad_stage_f32(p(a['g']), p(a['act']), p(a['amax']), a['n'], p(a['gs']), p(a['g_scale']), None)


def _good_wgrad(base, lib):
    N, H, W, Cin = 1, 4, 5, 32
    nbytes = lib.rmnet_conv3x3_wgrad_workspace_bytes(N, H, W, Cin)
    assert nbytes == (9 * Cin * 256 + BIAS_SPLIT * 256) * 4                        # one range
    return dict(x=base, g=base + 0x10000, g_scale=base + 0x20000, flags=1, N=N, H=H, W=W, Cin=Cin, dw=base + 0x30000, db=base + 0x80000,
                ws=base + 0x90000, ws_bytes=nbytes, rw=base + 0x20100)


def test_the_entries_refuse_malformed_calls_before_they_touch_the_device():
    """No GPU here: a call that got past the checks would fail to launch or fault on these made-up addresses."""
    from rmnet_amd import _lib
    lib = _lib.load()
    good = _good_wgrad(0x100000, lib)
    for name, kw, code in _wgrad_refusals(good):
        assert _wgrad_call(lib, dict(good, **kw)) == code, name
    assert lib.rmnet_conv3x3_wgrad_workspace_bytes(1, 4, MAX_W + 1, 32) == 0 and lib.rmnet_conv3x3_wgrad_workspace_bytes(0, 4, 4, 32) == 0
    assert lib.rmnet_conv3x3_wgrad_workspace_bytes(1, 1, 257, 32) == 2 * (9 * 32 * 256 + BIAS_SPLIT * 256) * 4
    good = dict(g=0x100000, act=0x200000, amax=0x300000, n=1024, gs=0x400000, g_scale=0x300100)
    for name, kw, code in _stage_refusals(good):
        assert _stage_call(lib, dict(good, **kw)) == code, name


def test_the_new_kernels_use_no_scratch_no_spill_and_no_static_lds(tmp_path):
    """From a compile-only gfx950 build: sizes and counts of the metadata, no instruction is looked at."""
    from rmnet_amd import build
    out = str(tmp_path / 'wgrad.s')
    subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                    os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv3x3_wgrad.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', open(out).read(), flags=re.S).group(1)
    found = {}
    for entry in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]:
        get = lambda key: re.search(r'^    \.%s:\s+(\S+)' % key, '    ' + entry, flags=re.M)
        if get('name'):                                            # (the lists after the kernels -- the version -- split the same way)
            found[get('name').group(1)] = {k: int(get(k).group(1)) for k in ('group_segment_fixed_size', 'private_segment_fixed_size',
                                                                            'vgpr_count', 'vgpr_spill_count')}
    for frag in ('13conv3x3_wgradE', '10wgrad_biasE', '11wgrad_mergeE', '15conv_grad_stageE'):
        hits = [k for n, k in found.items() if frag in n]
        assert len(hits) == 1, (frag, sorted(found))
        k = hits[0]
        print(frag, k)
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (frag, k)
    assert [k for n, k in found.items() if '13conv3x3_wgradE' in n][0]['vgpr_count'] <= 256    # 512 threads: two waves per SIMD
    assert 'conv3x3_wgrad.hip' in build.SOURCES


# ================================================================================================ GPU helpers
GUARD = 64


def _guarded(n, d):
    pool = torch.full((n + 2 * GUARD,), NAN, device=d)
    assert pool.data_ptr() % 16 == 0
    return pool, pool[GUARD:GUARD + n]


def _guards_intact(pool, n):
    return bool(torch.isnan(pool[:GUARD]).all()) and bool(torch.isnan(pool[GUARD + n:]).all()) and not bool(torch.isnan(pool[GUARD:GUARD + n]).any())


def _raw_wgrad(x, gs, g_scale, relu_in, want_bias=True, rw=None):
    """One call of the C entry with dw / db inside NaN-filled guarded pools; x [N,Cin,H,W] and gs [N,256,H,W] channels-last on the
    device.  Returns (dW [256,Cin,3,3], db) on the CPU."""
    from rmnet_amd import _lib
    lib = _lib.load()
    d = x.device
    N, cin, H, W = x.shape
    n_dw = 9 * cin * 256
    dw_pool, dw = _guarded(n_dw, d)
    db_pool, db = _guarded(256, d)
    nbytes = lib.rmnet_conv3x3_wgrad_workspace_bytes(N, H, W, cin)
    nr = -(-N * H * W // _plan(N * H * W, cin)[2])
    assert nbytes == nr * (n_dw + BIAS_SPLIT * 256) * 4
    ws_pool, ws = _guarded(nbytes // 4, d)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(d):
        rc = lib.rmnet_conv3x3_wgrad_f32(p(x), p(gs), p(g_scale), 1 if relu_in else 0, N, H, W, cin, p(dw), p(db) if want_bias else None, p(ws),
                                         nbytes, p(rw), ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert _guards_intact(dw_pool, n_dw), 'dw: a guard was written or an element was not'
    assert bool(torch.isnan(ws_pool[:GUARD]).all()) and bool(torch.isnan(ws_pool[GUARD + nbytes // 4:]).all()), 'workspace guard'
    if want_bias:
        assert _guards_intact(db_pool, 256), 'db'
    else:
        assert bool(torch.isnan(db_pool).all())
    return dw.view(256, 3, 3, cin).permute(0, 3, 1, 2).cpu(), db.cpu() if want_bias else None


def _plan(pixels, cin):
    """csrc/conv3x3_wgrad.hip: wgrad_plan, restated."""
    nct = cin // CT
    nr = max(1, min(TARGET_WGS // nct, -(-pixels // RANGE_MIN), MAX_RANGES))
    rl = -(-(-(-pixels // nr)) // KT) * KT
    return nct, -(-pixels // rl), rl


def _int_dw(x, g, relu_in):
    """dW and db in integer-exact float64 numpy: x, g [N,C,H,W] on the CPU."""
    _, dW, db, _ = ref.grads64(x, torch.zeros(g.shape[1], x.shape[1], 3, 3), g, relu_in=relu_in)
    return dW.float(), db.float()


# ================================================================================================ GPU 1: the exact family
WGRAD_EXACT = [
    # (Cin, N, H, W, relu_in, exponent of the largest gradient)
    (32, 1, 1, 1, False, 0), (32, 2, 1, 1, True, 0), (32, 1, 1, 9, False, 0), (32, 2, 9, 1, True, -30), (64, 1, 5, 7, True, 0),
    (64, 2, 5, 7, False, 3), (256, 1, 5, 7, True, -20), (32, 2, 16, 16, False, 0), (256, 2, 16, 16, True, 0),
    (32, 1, 3, 33, True, 0),                                      # a row one pixel longer than a K step
    (32, 1, 15, 17, False, 0), (32, 1, 16, 16, True, 0), (32, 1, 1, 257, False, 0),        # 255, 256, 257 pixels: one range / two
    (32, 1, 7, 73, True, 0), (32, 1, 16, 32, False, -40), (32, 1, 19, 27, True, 0),        # 511, 512, 513: two ranges / three
    (32, 1, 3, 160, False, 0), (32, 1, 7, 23, True, 0),                                    # 480 = 3 ranges of exactly 160; 161
    (64, 2, 129, 128, True, 0),                                   # 61 ranges of 544 pixels: each walks two activation images
]


@pytest.mark.gpu
@pytest.mark.parametrize('cin,n,h,w,relu_in,e', WGRAD_EXACT)
def test_wgrad_returns_integer_arithmetic_in_every_bit(cin, n, h, w, relu_in, e):
    from rmnet_amd import ops
    d = dev()
    x = conv_ref.int_acts((n, cin, h, w), 100 + cin + h)
    g = ref.pow2_grads((n, 256, h, w), 7 + w, e)
    want_dw, want_db = _int_dw(x, g, relu_in)
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    assert torch.equal(gs.cpu(), g * 2.0 ** (8 - e)) and float(g_scale[0] * g_scale[1]) == 2.0 ** (8 - e)
    rw = torch.zeros(1, dtype=torch.int32, device=d)
    dw, db = _raw_wgrad(cl(x.to(d)), gs, g_scale, relu_in, rw=rw)
    assert torch.equal(dw, want_dw), 'dW: %d elements differ' % int((dw != want_dw).sum())
    assert torch.equal(db, want_db)
    assert int(rw) == 0
    dw2, none = _raw_wgrad(cl(x.to(d)), gs, g_scale, relu_in, want_bias=False)
    assert none is None and torch.equal(dw2, dw)


@pytest.mark.gpu
@pytest.mark.parametrize('tap', range(9))
def test_wgrad_with_one_live_tap(tap):
    """x at one pixel, g at its neighbour through ``tap``: the only non-zero dW is that tap's."""
    from rmnet_amd import ops
    d = dev()
    ky, kx = tap // 3, tap % 3
    x, g = torch.zeros(1, 32, 5, 7), torch.zeros(1, 256, 5, 7)
    x[0, :, 1 + ky, 2 + kx] = conv_ref.int_acts((32,), tap, 1, 15)
    g[0, :, 2, 3] = ref.pow2_grads((256,), tap, zeros=False)
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    dw, db = _raw_wgrad(cl(x.to(d)), gs, g_scale, False)
    want = torch.zeros(256, 32, 3, 3)
    want[:, :, ky, kx] = g[0, :, 2, 3].view(-1, 1) * x[0, :, 1 + ky, 2 + kx].view(1, -1)
    assert torch.equal(dw, want) and torch.equal(db, g[0, :, 2, 3])


DGRAD_EXACT = [(256, 1, 1, 1), (256, 2, 1, 9), (512, 1, 9, 1), (256, 1, 5, 7), (512, 2, 5, 7), (256, 2, 16, 16), (512, 1, 3, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize('cin,n,h,w', DGRAD_EXACT)
def test_dgrad_returns_integer_arithmetic_in_every_bit(cin, n, h, w):
    from rmnet_amd import ops
    d = dev()
    wt = conv_ref.int_weights(256, cin, 3, 5 + cin)
    g = ref.pow2_grads((n, 256, h, w), 3 + h, -25)
    want = ref.grads64(torch.zeros(n, cin, h, w), wt, g)[0].float()
    packs = ops.conv3x3_dgrad_pack(wt.to(d))
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    inv = g_scale.reciprocal()
    rw = torch.zeros(1, dtype=torch.int32, device=d)
    for s, (wp, wu) in enumerate(packs):
        pool, flat = _guarded(n * h * w * 256, d)
        out = flat.view(n, h, w, 256).permute(0, 3, 1, 2)
        ops.conv3x3_split(gs, wp, wu * inv[0] * inv[1], out=out, range_word=rw)
        torch.cuda.synchronize()
        assert _guards_intact(pool, flat.numel())
        assert torch.equal(out.cpu(), want[:, 256 * s:256 * (s + 1)]), 'slice %d' % s
    got = ops.conv3x3_dgrad(gs, g_scale, packs, range_word=rw)
    assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got.cpu(), want) and int(rw) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('tap', range(9))
def test_dgrad_with_one_live_tap(tap):
    from rmnet_amd import ops
    d = dev()
    wt = torch.zeros(256, 256, 3, 3)
    wt[:, :, tap // 3, tap % 3] = conv_ref.int_weights(256, 256, 1, tap)[:, :, 0, 0]
    g = ref.pow2_grads((1, 256, 5, 7), tap)
    want = ref.grads64(torch.zeros(1, 256, 5, 7), wt, g)[0].float()
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    got = ops.conv3x3_dgrad(gs, g_scale, ops.conv3x3_dgrad_pack(wt.to(d)))
    assert torch.equal(got.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize('amax', [0.0, 2.0 ** -149, 1e-40, 2.0 ** -118, 2.0 ** -117, 1e-8, 1.0, 300.0, 1e30, 3.0e38, float('inf'), NAN])
def test_the_stage_kernel_computes_the_exponent_of_the_restatement_on_the_device(amax):
    """What the CPU test says of ``conv_grad_stage_exponent`` holds for the kernel's own frexpf: subnormal amax, the two-factor scale
    above 2^126, 1e30, 0, Inf and NaN.  The staged values are exact products; ``act`` masks; ``out=g`` works in place."""
    from rmnet_amd import ops
    d = dev()
    a32 = float(np.float32(amax))
    g = torch.zeros(1, 256, 2, 3)
    g[0, 0, 0, 0] = a32
    g[0, 1, 0, 0] = -a32 / 2 if np.isfinite(a32) else 1.0
    g[0, 2, 1, 2] = a32 / 8 if np.isfinite(a32) else -2.0
    act = torch.ones_like(g)
    act[0, 2, 1, 2] = -1.0
    act[0, 3, 0, 0] = 0.0
    gd = cl(g.to(d))
    gs, sc = ops.conv_grad_stage(gd, cl(act.to(d)), torch.tensor(a32, device=d))
    s = ref.stage_exponent(a32)
    assert s == int(ops.conv_grad_stage_exponent(torch.tensor(a32)))
    assert float(sc[0]) == 2.0 ** min(s, 126) and float(sc[1]) == 2.0 ** (s - min(s, 126))
    want = torch.ldexp(g.double(), torch.tensor(float(s), dtype=torch.float64))
    want[0, 2, 1, 2] = 0.0
    assert torch.equal(gs.cpu().double(), want, ) or (np.isnan(a32) and torch.equal(torch.isnan(gs.cpu()), torch.isnan(want)))
    if 0 < a32 < float('inf'):
        assert 2.0 ** 8 <= float(gs.abs().max()) < 2.0 ** 9
    auto, sc2 = ops.conv_grad_stage(gd)                            # amax by the reduction, no mask
    assert torch.equal(sc2, sc) or np.isnan(a32)
    same, _ = ops.conv_grad_stage(gd, out=gd)
    assert same.data_ptr() == gd.data_ptr() and torch.equal(torch.nan_to_num(gd), torch.nan_to_num(auto))


# ================================================================================================ GPU 2: the random family
def _random_g(kind, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen)
    if kind == 'mixed':                                           # output channel c times 2^(-24 + c mod 20)
        return g * torch.ldexp(torch.ones(shape[1]), (torch.arange(shape[1]) % 20 - 24).float()).view(1, -1, 1, 1)
    return g * float(kind)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['1e-8', '1', 'mixed'])
@pytest.mark.parametrize('cin,n,h,w,relu_in', [(32, 1, 4, 8, False), (64, 2, 16, 16, True)])
def test_wgrad_is_within_the_derived_bound_of_its_restatement(kind, cin, n, h, w, relu_in):
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(cin + h)
    x = torch.randn(n, cin, h, w, generator=gen) * 2
    g = _random_g(kind, (n, 256, h, w), 31)
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    gs64, s = ref.stage64(g)
    assert torch.equal(gs.cpu().double(), gs64) and float(g_scale[0]) == 2.0 ** s and float(g_scale[1]) == 1.0
    plan = _plan(n * h * w, cin)
    T, ahh, ax, Tb, Ab = ref.wgrad_restate(x, gs64, s, plan, relu_in)
    dw, db = _raw_wgrad(cl(x.to(d)), gs, g_scale, relu_in)
    err, bound = (dw.double() - T).abs(), ref.acc_bound(plan[2], plan[1], ahh, ax)
    print('dW: largest error / bound %.3f' % (err / bound.clamp_min(1e-300)).max())
    assert (err <= bound).all()
    assert ((db.double() - Tb).abs() <= ref.bias_bound(plan[2] // BIAS_SPLIT, plan[1] * BIAS_SPLIT, Ab)).all()
    truth = ref.grads64(x, torch.zeros(256, cin, 3, 3), g, relu_in=relu_in)[1]
    assert ((dw.double() - truth).abs() <= bound + ref.wgrad_repr_bound(x, g, s, relu_in)).all()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['1e-8', '1', 'mixed'])
def test_dgrad_is_within_the_derived_bound_of_its_restatement(kind):
    from rmnet_amd import ops
    d = dev()
    cin, n, h, w = 512, 1, 5, 7
    wt = conv_ref.uniform_weights(256, cin, 3, 8)
    g = _random_g(kind, (n, 256, h, w), 77)
    packs = ops.conv3x3_dgrad_pack(wt.to(d))
    gs, g_scale = ops.conv_grad_stage(cl(g.to(d)))
    gs64, s = ref.stage64(g)
    T, ahh, ax = ref.dgrad_restate(gs64, s, packs, cin)
    got = ops.conv3x3_dgrad(gs, g_scale, packs).cpu().double()
    bound = ref.acc_bound(9 * 256, 1, ahh, ax)
    print('dX: largest error / bound %.3f' % ((got - T).abs() / bound.clamp_min(1e-300)).max())
    assert ((got - T).abs() <= bound).all()
    truth = ref.grads64(torch.zeros(n, cin, h, w), wt, g)[0]
    assert (got - truth).abs().max() <= 2.0 ** -18 * truth.abs().max()           # (wiring: the flipped pack against the plain formula)


# ================================================================================================ GPU 3: determinism, range word
@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_return_the_same_bits():
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(4)
    x = cl((torch.randn(2, 256, 9, 31, generator=gen)).to(d))
    g = cl((torch.randn(2, 256, 9, 31, generator=gen) * 1e-6).to(d))
    packs = ops.conv3x3_dgrad_pack(conv_ref.uniform_weights(256, 256, 3, 1).to(d))

    def run():
        gs, sc = ops.conv_grad_stage(g)
        dw, db = ops.conv3x3_wgrad(x, gs, sc, relu_in=True)
        return dw, db, ops.conv3x3_dgrad(gs, sc, packs)

    first = [t.clone() for t in run()]                            # eagerly, before the capture: the LDS attribute is set here
    second = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # a single stream, no parallel branches
        held = run()
    for t in held:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, held))


@pytest.mark.gpu
def test_bad_values_are_counted_in_the_backward_word_and_the_forward_word_is_left_alone():
    from rmnet_amd import ops
    d = dev()
    fwd = ops.conv_range_word(d)
    before = int(fwd)
    grw = ops.conv_grad_range_word(d)
    assert grw.data_ptr() != fwd.data_ptr()
    x = cl(conv_ref.int_acts((1, 64, 5, 7), 1).to(d))
    g = ref.pow2_grads((1, 256, 5, 7), 2)
    one = torch.ones(2, device=d)
    for name, plant, count in (('NaN', NAN, 1), ('Inf', float('inf'), 1)):
        gb = g.clone()
        gb[0, 17, 2, 3] = plant
        gs, sc = ops.conv_grad_stage(cl(gb.to(d)))
        assert float(sc[0]) == 1.0 and float(sc[1]) == 1.0        # amax NaN / Inf: s = 0
        grw.zero_()
        ops.conv3x3_wgrad(x, gs, sc, range_word=grw)
        assert int(grw) == count, name
    xb = x.clone()
    xb[0, 33, 4, 6] = 1024.0
    xb[0, 5, 0, 0] = -2000.0
    gs, sc = ops.conv_grad_stage(cl(g.to(d)))
    grw.zero_()
    ops.conv3x3_wgrad(xb, gs, sc, range_word=grw)
    assert int(grw) == 2
    grw.zero_()
    ops.conv3x3_wgrad(xb, gs, sc, relu_in=True, range_word=grw)   # the ReLU removes the negative one
    assert int(grw) == 1
    grw.zero_()
    ops.conv3x3_wgrad(x, g.to(d).contiguous(memory_format=torch.channels_last) * 1024.0, one, range_word=grw)   # unstaged and too large
    assert int(grw) == int((g.abs() * 1024.0 * 64 > 65504).sum())
    grw.zero_()
    assert int(fwd) == before


# ================================================================================================ GPU 4: autograd
def _layer(cin, d, seed=3):
    from rmnet_amd import ops
    w = conv_ref.uniform_weights(256, cin, 3, seed).to(d)
    b = (torch.arange(256.0) / 512 - 0.2).to(d)
    wp, wu = ops.conv3x3_pack(w)
    return w, b, wp, wu


@pytest.mark.gpu
@pytest.mark.parametrize('leaf', [True, False])
def test_conv3x3_split_under_autograd_gives_the_float64_gradients(leaf):
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(12)
    x0, res0, g = (torch.randn(2, 256, 5, 7, generator=gen) for _ in range(3))
    w, b, wp, wu = _layer(256, d)
    w.requires_grad_(True), b.requires_grad_(True)
    xl = cl(x0.to(d)).requires_grad_(True)
    rl = cl(res0.to(d)).requires_grad_(True)
    x = xl if leaf else xl * 1.0
    res = rl if leaf else rl + 0.0
    out = ops.conv3x3_split(x, wp, wu, b, res=res, relu_in=True, relu_out=True, weight=w)
    assert out.grad_fn is not None and out.requires_grad
    plain = ops.conv3x3_split(xl.detach(), wp, wu, b.detach(), res=rl.detach(), relu_in=True, relu_out=True)
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    out.backward(cl(g.to(d)) * 1e-5)
    want = ref.grads64(x0, w.detach().cpu(), g * 1e-5, b.detach().cpu(), res0, relu_in=True, relu_out=True)
    for name, got, ex in (('x', xl.grad, want[0]), ('w', w.grad, want[1]), ('b', b.grad, want[2]), ('res', rl.grad, want[3])):
        err = (got.cpu().double() - ex).abs().max() / ex.abs().max()
        print('%s: %.2e' % (name, err))
        assert err <= 2.0 ** -18, name
    # grad_output scaling: twice the gradient is twice every result, exactly (a power of two moves the staging exponent only)
    first = [t.grad.clone() for t in (xl, w, b, rl)]
    for t in (xl, w, b, rl):
        t.grad = None
    x = xl if leaf else xl * 1.0
    res = rl if leaf else rl + 0.0
    ops.conv3x3_split(x, wp, wu, b, res=res, relu_in=True, relu_out=True, weight=w).backward(cl(g.to(d)) * 2e-5)
    assert all(torch.equal(2 * a, t.grad) for a, t in zip(first, (xl, w, b, rl)))


@pytest.mark.gpu
def test_nothing_requiring_grad_means_no_graph_and_the_same_bits_and_only_what_is_needed_is_launched():
    from rmnet_amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(13)
    x = cl(torch.randn(1, 256, 5, 7, generator=gen).to(d))
    g = cl(torch.randn(1, 256, 5, 7, generator=gen).to(d))
    w, b, wp, wu = _layer(256, d)
    with torch.no_grad():
        want = ops.conv3x3_split(x, wp, wu, b)
    got = ops.conv3x3_split(x, wp, wu, b, weight=w)               # grad mode on, nothing requires grad
    assert got.grad_fn is None and not got.requires_grad and torch.equal(got, want)
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        assert ops.conv3x3_split(xr, wp, wu, b, weight=w).grad_fn is None
    count = ops.conv_grad_launches

    def launches(**req):
        for k in count:
            count[k] = 0
        xx = x.clone().requires_grad_(req.get('x', False))
        ww = w.detach().clone().requires_grad_(req.get('w', False))
        bb = b.detach().clone().requires_grad_(req.get('b', False))
        out = ops.conv3x3_split(xx, wp, wu, bb, relu_out=True, weight=ww)
        assert torch.equal(out.detach(), ops.conv3x3_split(x, wp, wu, b, relu_out=True))
        out.backward(g)
        return dict(count), xx.grad, ww.grad, bb.grad

    c, gx, gw, gb = launches(x=True)                              # a frozen layer: dgrad alone
    assert (c['stage'], c['wgrad'], c['dgrad']) == (1, 0, 1) and gx is not None and gw is None and gb is None
    c, gx, gw, gb = launches(w=True, b=True)                      # r3 / r2 of a frozen encoder: no dgrad (and no dgrad pack)
    assert (c['stage'], c['wgrad'], c['dgrad'], c['pack']) == (1, 1, 0, 0) and gx is None and gw is not None and gb is not None
    ref_gb = gb.clone()
    c, gx, gw, gb = launches(b=True)                              # a trainable bias alone: no GEMM at all
    assert (c['stage'], c['wgrad'], c['dgrad']) == (0, 0, 0) and gw is None
    assert (gb - ref_gb).abs().max() <= 1e-4 * ref_gb.abs().max()
    c, gx, gw, gb = launches(x=True, w=True, b=True)
    assert (c['stage'], c['wgrad'], c['dgrad']) == (1, 1, 1)


@pytest.mark.gpu
def test_double_backward_is_refused():
    from rmnet_amd import ops
    d = dev()
    x = cl(torch.randn(1, 256, 3, 4).to(d)).requires_grad_(True)
    w, b, wp, wu = _layer(256, d)
    out = ops.conv3x3_split(x, wp, wu, b, weight=w)
    gx, = torch.autograd.grad((out * out).sum(), x, create_graph=True)     # (the incoming gradient 2 out depends on x)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|twice'):
        gx.sum().backward()
    with pytest.raises(RuntimeError, match='out must be None'):
        ops.conv3x3_split(x, wp, wu, b, weight=w, out=torch.empty_like(out))


# ================================================================================================ GPU 5: the module
def _decoder(d):
    from rmnet_amd import networks
    dec = networks.Decoder(256)
    networks.procedural_init_(dec)
    return dec.eval()


def _decoder_inputs(seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    return r(2, 1024, 2, 3), r(2, 512, 4, 6), r(2, 256, 8, 12), r(2, 2, 32, 48)


def _device_decoder(d):
    from rmnet_amd import networks
    dec = _decoder(d).to(d).to(memory_format=torch.channels_last)
    networks.fuse_epilogues_(dec)
    return dec.device_grad_()


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


@pytest.mark.gpu
def test_the_decoder_trains_on_the_device_as_precisely_as_the_library_route(monkeypatch):
    """Wiring: faults here are of order 1.  The bar is measured: our largest error relative to the largest gradient, against the same
    module in float64 on the CPU, at most 4x that of torch autograd through the fp32 library convolutions on the same inputs.
    Measured on an MI355X (profiles/r36_a_decoder_backward.md): ours 9.47e-07 to 1.006e-06, the library 4.11e-07 to 4.56e-07 over five runs."""
    from rmnet_amd import ops
    d = dev()
    inputs = _decoder_inputs()
    dec = _device_decoder(d)
    ops.conv_range_word(d).zero_()
    ops.conv_grad_range_word(d).zero_()
    for k in ops.conv_grad_launches:
        ops.conv_grad_launches[k] = 0
    for mode in ('eval', 'train'):
        getattr(dec, mode)()
        out, ours = _backward(dec, inputs, d)
        assert out.grad_fn is not None, 'the fused decoder returned a tensor without a graph'
    assert ops.conv_grad_launches['wgrad'] == 2 * 13 and ops.conv_grad_launches['stage'] == 2 * 13
    assert ops.conv_grad_launches['dgrad'] == 2 * (4 + 10) and ops.conv_grad_launches['pack'] == 11   # convFM only; r3 / r2 need none
    assert int(ops.conv_range_word(d)) == 0 and int(ops.conv_grad_range_word(d)) == 0
    cpu = _decoder(d).double()
    _, want = _backward(cpu, inputs, torch.device('cpu'), torch.float64)
    monkeypatch.setenv('RMNET_CONV', 'miopen')
    lib = _decoder(d).to(d).to(memory_format=torch.channels_last).train()
    out_lib, theirs = _backward(lib, inputs, d)
    monkeypatch.delenv('RMNET_CONV')
    assert set(ours) == set(want) == set(theirs) and len(ours) == 1 + 2 * 14
    rel = lambda got: max(((got[k] - want[k]).abs().max() / want[k].abs().max()).item() for k in want)
    e_ours, e_lib = rel(ours), rel(theirs)
    print('largest gradient error relative to the largest gradient: ours %.3e, library %.3e' % (e_ours, e_lib))
    assert e_ours <= 4 * e_lib


@pytest.mark.gpu
def test_without_the_flag_or_without_grad_the_decoder_takes_the_paths_it_took():
    from rmnet_amd import networks
    d = dev()
    r4, r3, r2, _ = (cl(t.to(d)) if t.shape[1] != 2 else t for t in _decoder_inputs(1))
    dec = _device_decoder(d)
    with torch.no_grad():
        want = dec(r4, r3, r2)
    dec.device_grad_(False)
    with torch.no_grad():
        assert torch.equal(dec(r4, r3, r2), want)
    assert dec(r4, r3, r2).grad_fn is None                        # (the fused inference path builds no graph: the flag is what changes that)
    dec.device_grad_()
    for p in dec.parameters():
        p.requires_grad_(False)
    out = dec(r4, r3, r2)                                         # nothing requires grad: the inference path and its bits
    assert out.grad_fn is None and torch.equal(out, want)


@pytest.mark.gpu
def test_the_packs_follow_the_weights_and_are_not_rebuilt_without_a_change():
    from rmnet_amd import ops
    d = dev()
    inputs = _decoder_inputs(2)
    dec = _device_decoder(d)
    count = ops.conv_grad_launches
    _backward(dec, inputs, d)
    count['pack'] = 0
    wp_before = dec.ResMM._wp1.clone()
    out1, _ = _backward(dec, inputs, d)
    assert count['pack'] == 0 and torch.equal(dec.ResMM._wp1, wp_before)          # cached
    with torch.no_grad():
        dec.ResMM.conv1.weight.mul_(0.75)                         # an optimiser step in miniature (no power of two: the pack bits move)
    out2, g2 = _backward(dec, inputs, d)
    assert count['pack'] == 1 and not torch.equal(dec.ResMM._wp1, wp_before)
    assert not torch.equal(out1, out2)
    fresh = _decoder(d)
    with torch.no_grad():
        fresh.ResMM.conv1.weight.mul_(0.75)
    fresh = fresh.to(d).to(memory_format=torch.channels_last)
    from rmnet_amd import networks
    networks.fuse_epilogues_(fresh)
    out3, g3 = _backward(fresh.device_grad_(), inputs, d)
    # the refreshed packs are the packs of a decoder that was fused with the new weight (pred2 and the upsamples are library
    # kernels, whose bits may differ from call to call: the results are compared to a tolerance, the packs bit for bit)
    assert torch.equal(dec.ResMM._wp1, fresh.ResMM._wp1) and torch.equal(dec.ResMM._wu1, fresh.ResMM._wu1)
    for (wa, ua), (wb, ub) in zip(dec.ResMM._dgrad_packs['1'][2], fresh.ResMM._dgrad_packs['1'][2]):
        assert torch.equal(wa, wb) and torch.equal(ua, ub)
    assert (out2 - out3).abs().max() <= 1e-5 * out3.abs().max()
    assert all((g2[k] - g3[k]).abs().max() <= 1e-4 * g3[k].abs().max() for k in g2)


@pytest.mark.gpu
def test_one_backward_runs_from_the_loss_through_the_tail_into_r4():
    from rmnet_amd import losses, ops
    d = dev()
    r4, r3, r2, _ = _decoder_inputs(3)
    dec = _device_decoder(d)
    ops.conv_grad_range_word(d).zero_()
    r4 = cl(r4.to(d)).requires_grad_(True)
    logits = dec(r4, cl(r3.to(d)), cl(r2.to(d)))                  # [2, 2, 32, 48]: two objects of one clip
    begin = torch.tensor([0, 2], dtype=torch.int32, device=d)
    _, prob = ops.soft_aggregate(logits.contiguous(), begin, 3, (0, 0, 0, 0), want_prob=True)
    labels = (torch.arange(32 * 48, device=d).view(1, 32, 48) % 3).to(torch.uint8)
    loss = losses.training_loss(prob, labels)
    loss.backward()
    assert r4.grad is not None and bool(torch.isfinite(r4.grad).all()) and float(r4.grad.abs().max()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in dec.parameters())
    assert int(ops.conv_grad_range_word(d)) == 0
