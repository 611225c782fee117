# -*- coding: utf-8 -*-
"""conv3x3_rows (csrc/conv3x3_rows.hip), the Cin = 256 decoder convolution that stages a whole tap row of activations in LDS once,
against the two kernels of csrc/conv3x3.hip.  The K order per accumulator, the operand bits and the epilogue expressions are the
same, so the yardstick is the old kernels (rmnet_conv3x3_split_lds_f32, and rmnet_conv3x3_split_f32) on the same inputs and the
comparison is ``torch.equal`` on the output and ``==`` on the range word: no tolerance is involved.

What is new in the kernel is its addressing: a workgroup stages the 130 pixels m0 + dy*W - 1 .. m0 + dy*W + 128 of each tap row,
clamped into the tensor, and a lane picks per (pixel tile, tap) between the staged row and a row of zeros.  The shapes (N, H, W)
are the smallest maps at which each addressing case exists, all with Cin = 256:

  (1, 1, 1)    only the centre tap is live
  (2, 5, 7)    M = 70 < 128, one tile spans two images
  (2, 9, 15)   M = 270, a tile boundary falls inside image 1
  (1, 3, 130)  W > 128: a tile lies inside one row, its tap rows are disjoint from it; the last tile holds 6 pixels
  (1, 2, 128)  the tiles are exactly the rows: every halo row belongs to another tile or to nothing
  (3, 1, 43)   H = 1: dy = +-1 is never valid; M = 129
  (1, 43, 1)   W = 1: dx = +-1 is never valid, and its row is a real neighbour's

  * randn x 3 inputs with bias on / off, the residual absent / separate / ``out is res``, and all four ReLU combinations, into a
    buffer with sentinels in front of and behind the output; ``x`` is unchanged afterwards;
  * one live tap at a time: a one-hot weight per output channel and an input whose neighbouring pixels and channels hold
    different small integers -- the exact integers against numpy, for each of the 9 taps (a wrong row shift or a leaked wrap
    pixel is a wrong integer);
  * the range word: out-of-window values, NaN, +Inf and -Inf at tile, halo, row-wrap and image boundaries;
  * the switch, by the export that is called; the export refuses Cin 128 and writes nothing;
  * one call captured in a graph and replayed;
  * CPU: what the compiler gives the kernel."""

import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

CIN = 256
SHAPES = [(1, 1, 1), (2, 5, 7), (2, 9, 15), (1, 3, 130), (1, 2, 128), (3, 1, 43), (1, 43, 1)]
GUARD = 64                     # floats in front of and behind the output (a multiple of 4: out stays 16-byte aligned)
SENTINEL = -12345.5
TILE = 128                     # pixels per workgroup
E_UNSUPPORTED = -4             # include/rmnet_hip.h


def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _select(monkeypatch, kernel):
    """'rows': the switch on and no kernel named; 'lds' / 'wreg': that kernel, named."""
    if kernel == 'rows':
        monkeypatch.setenv('RMNET_CONV3X3_ROWS', '1')
        monkeypatch.delenv('RMNET_CONV3X3_KERNEL', raising=False)
    else:
        monkeypatch.delenv('RMNET_CONV3X3_ROWS', raising=False)
        monkeypatch.setenv('RMNET_CONV3X3_KERNEL', kernel)


@functools.lru_cache(maxsize=None)
def _weights():
    """(wpack, w_unscale, bias) of one random [256, 256, 3, 3] convolution, shared by every shape and never written."""
    from rmnet_amd import ops
    g = torch.Generator().manual_seed(2000)
    wt = torch.randn((256, CIN, 3, 3), generator=g)
    bias = torch.randn(256, generator=g)
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    return wp, wu, bias.to(dev())


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x channels-last, res channels-last) on the device; made once per shape and never written."""
    n, h, w = shape
    g = torch.Generator().manual_seed(3000 + 97 * n + 13 * h + w)
    x = torch.randn((n, CIN, h, w), generator=g) * 3
    res = torch.randn((n, 256, h, w), generator=g) * 3
    return _cl(x), _cl(res)


def _guarded_out(n, h, w, fill=None):
    """A channels-last [N, 256, H, W] view in the middle of a buffer of sentinels -> (buffer, view)."""
    m = n * h * w * 256
    buf = torch.full((m + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev())
    out = buf[GUARD:GUARD + m].view(n, h, w, 256).permute(0, 3, 1, 2)
    assert out.is_contiguous(memory_format=torch.channels_last) and out.data_ptr() % 16 == 0
    if fill is not None:
        out.copy_(fill)
    return buf, out


def _call(monkeypatch, kernel, x, wp, wu, bias, res_mode, res, relu_in, relu_out, range_word='own'):
    """One launch of ``kernel`` into a guarded buffer -> (out, range word or None); the guards and x are checked here."""
    from rmnet_amd import ops
    _select(monkeypatch, kernel)
    n, _, h, w = x.shape
    rw = torch.zeros(1, dtype=torch.int32, device=dev()) if range_word == 'own' else None
    buf, out = _guarded_out(n, h, w, res if res_mode == 'inplace' else None)
    r = {'none': None, 'res': res, 'inplace': out}[res_mode]
    before = x.clone()
    got = ops.conv3x3_split(x, wp, wu, bias, r, relu_in=relu_in, relu_out=relu_out, out=out, range_word=rw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), '%s wrote outside out' % kernel
    assert not bool((out == SENTINEL).any()), '%s left output elements unwritten' % kernel
    assert torch.equal(x.view(torch.int32), before.view(torch.int32)), '%s changed x' % kernel
    return out, (int(rw.item()) if rw is not None else None)


def _assert_same(new, old, what):
    """Equal, NaN equal to NaN (the range cases plant NaN on purpose), said with the first differing elements."""
    same = (new == old) | (new.isnan() & old.isnan())
    if bool(same.all()):
        return
    bad = (~same).nonzero()
    first = [(tuple(int(v) for v in i), float(new[tuple(i)]), float(old[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index [n, co, y, x], new, reference): %s' % (what, bad.shape[0], new.numel(), first))


def _assert_equal(new, old, what):
    if not torch.equal(new, old):
        _assert_same(new, old, what)
        pytest.fail('%s: NaN in the outputs' % what)


# ================================================================================================ randn: every flag combination
@pytest.mark.gpu
@pytest.mark.parametrize('res_mode', ['none', 'res', 'inplace'])
@pytest.mark.parametrize('shape', SHAPES)
def test_outputs_and_range_words_equal_the_old_kernels_bit_for_bit(monkeypatch, shape, res_mode):
    wp, wu, bias = _weights()
    x, res = _inputs(shape)
    assert x.numel() < 8192 or (int((x > 0).sum()) > 2000 and int((x < 0).sum()) > 2000)
    for use_bias in (False, True):
        for relu_in in (False, True):
            for relu_out in (False, True):
                args = (x, wp, wu, bias if use_bias else None, res_mode, res, relu_in, relu_out)
                new, bad_new = _call(monkeypatch, 'rows', *args)
                old, bad_old = _call(monkeypatch, 'lds', *args)
                wreg, bad_wreg = _call(monkeypatch, 'wreg', *args)
                assert bad_new == bad_old == bad_wreg == 0
                what = '%s bias %s %s relu_in %s relu_out %s' % (shape, use_bias, res_mode, relu_in, relu_out)
                _assert_equal(new, old, what + ' (against lds)')
                _assert_equal(new, wreg, what + ' (against wreg)')
                assert float(new.abs().max()) > 1.0          # (not a comparison of two empty results)


# ================================================================================================ integers: one live tap at a time
def _integer_case(shape, tap):
    """x: (flat NHWC index mod 2039) - 1019 (64 x is an fp16 number inside the window; neighbouring pixels and channels differ).
    Weight: output channel co has one live element, +-(1 .. 5), at input channel (7 co + 3) mod 256 of tap ``tap``.  Bias: a
    different integer per channel.  Every output is one product plus the bias, exact in fp32."""
    n, h, w = shape
    flat = np.arange(n * h * w * CIN, dtype=np.int64)
    x = ((flat % 2039) - 1019).astype(np.float32).reshape(n, h, w, CIN)
    co = np.arange(256)
    ci = (7 * co + 3) % CIN
    val = ((co % 5) + 1) * np.where(co % 2, -1, 1)
    bias = (co - 128).astype(np.float32)
    ky, kx = tap // 3, tap % 3
    wt = np.zeros((256, CIN, 3, 3), dtype=np.float32)
    wt[co, ci, ky, kx] = val
    xp = np.zeros((n, h + 2, w + 2, CIN), dtype=np.float32)
    xp[:, 1:-1, 1:-1] = x
    want = np.empty((n, 256, h, w), dtype=np.float32)
    for c in range(256):
        want[:, c] = val[c] * xp[:, ky:ky + h, kx:kx + w, ci[c]] + bias[c]
    return torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), torch.from_numpy(bias), torch.from_numpy(want)


@pytest.mark.gpu
@pytest.mark.parametrize('tap', range(9))
@pytest.mark.parametrize('shape', [(2, 5, 7), (1, 3, 130)])
def test_one_live_tap_returns_the_exact_integers(monkeypatch, shape, tap):
    from rmnet_amd import ops
    x, wt, bias, want = _integer_case(shape, tap)
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    args = (_cl(x), wp, wu, bias.to(dev()), 'none', None, False, False)
    new, bad_new = _call(monkeypatch, 'rows', *args)
    old, bad_old = _call(monkeypatch, 'lds', *args)
    assert bad_new == bad_old == 0
    want = want.to(dev())
    assert int((want != bias.to(dev()).view(1, -1, 1, 1)).sum()) > want.numel() // 4       # (many outputs read a live product)
    _assert_equal(new, want, '%s tap %d integers against numpy' % (shape, tap))
    _assert_equal(new, old, '%s tap %d integers' % (shape, tap))


# ================================================================================================ the range word
PLANT_VALUES = [2000.0, float('nan'), float('inf'), float('-inf'), -2000.0]


def _plant_pixels(shape):
    """Flat pixel indices: the first and last pixel of every tile, pixels that tile 0 and tile 1 stage only as halo (below and above
    their own), the row-wrap pixels (last of a row, first of the next), the first and last pixel of every image."""
    n, h, w = shape
    m = n * h * w
    px = set()
    for m0 in range(0, m, TILE):
        px.update((m0, min(m0 + TILE, m) - 1))
    px.update(p for p in (TILE + w - 1, TILE + w // 2, TILE - w // 2 - 1, TILE - w) if 0 <= p < m)
    px.update(p for p in (w - 1, w, m - w - 1, m - w) if 0 <= p < m)
    for i in range(n):
        px.update((i * h * w, (i + 1) * h * w - 1))
    return sorted(px)


def _planted_input(shape):
    """randn x 3 with every value of PLANT_VALUES at each pixel of _plant_pixels, in the first and in the last channel block
    -> (x, list of planted values)."""
    n, h, w = shape
    x = _inputs(shape)[0].clone()
    planted = []
    for p in _plant_pixels(shape):
        i, r = divmod(p, h * w)
        for c0 in (0, CIN - 32):
            for k, v in enumerate(PLANT_VALUES):
                x[i, c0 + 3 + 6 * k, r // w, r % w] = v
                planted.append(v)
    return x, planted


@pytest.mark.gpu
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('shape', [(2, 9, 15), (1, 3, 130), (1, 2, 128)])
def test_range_word_counts_each_planted_element_once_as_the_lds_kernel_does(monkeypatch, shape, relu_in):
    wp, wu, bias = _weights()
    x, planted = _planted_input(shape)
    expect = sum(1 for v in planted if not (relu_in and v < 0))
    assert expect >= 30
    args = (x, wp, wu, bias, 'none', None, relu_in, False)
    new, bad_new = _call(monkeypatch, 'rows', *args)
    old, bad_old = _call(monkeypatch, 'lds', *args)
    assert bad_old == expect, (bad_old, expect)
    assert bad_new == expect, (bad_new, expect)
    _assert_same(new, old, '%s planted values, relu_in %s' % (shape, relu_in))


@pytest.mark.gpu
def test_without_a_range_word_nothing_is_counted_and_the_output_is_the_same(monkeypatch):
    from rmnet_amd import ops
    shape = (2, 9, 15)
    wp, wu, bias = _weights()
    x, _ = _planted_input(shape)
    shared = ops.conv_range_word(dev())
    before = int(shared.item())
    args = (x, wp, wu, bias, 'none', None, False, False)
    new, word = _call(monkeypatch, 'rows', *args, range_word=None)
    assert word is None
    old, _ = _call(monkeypatch, 'lds', *args)
    _assert_same(new, old, 'planted values, no range word')
    assert int(shared.item()) == before


# ================================================================================================ the switch
def test_the_switch_takes_0_and_1_and_anything_else_raises(monkeypatch):
    from rmnet_amd import ops
    assert ops.CONV3X3_ROWS_DEFAULT in (False, True)
    monkeypatch.delenv('RMNET_CONV3X3_ROWS', raising=False)
    assert ops.conv3x3_rows_enabled() is ops.CONV3X3_ROWS_DEFAULT
    for value, on in (('0', False), ('1', True)):
        monkeypatch.setenv('RMNET_CONV3X3_ROWS', value)
        assert ops.conv3x3_rows_enabled() is on
    for value in ('yes', '', 'true', '2'):
        monkeypatch.setenv('RMNET_CONV3X3_ROWS', value)
        with pytest.raises(RuntimeError, match='RMNET_CONV3X3_ROWS'):
            ops.conv3x3_rows_enabled()


class _Spy(object):
    """The loaded library, recording the name of every export that is fetched from it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


@pytest.mark.gpu
def test_the_switch_reaches_the_export_it_should(monkeypatch):
    from rmnet_amd import _lib, ops
    wp, wu, bias = _weights()
    x256 = _inputs((2, 5, 7))[0]
    x32 = _cl(torch.randn((2, 32, 5, 7), generator=torch.Generator().manual_seed(5)))
    wp32, wu32 = ops.conv3x3_pack(torch.randn((256, 32, 3, 3), generator=torch.Generator().manual_seed(6)).to(dev()))
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    default = ops.CONV3X3_ENTRIES[ops.CONV3X3_KERNEL_DEFAULT]
    cases = [('1', None, x256, wp, wu, 'rmnet_conv3x3_rows_f32'), ('1', None, x32, wp32, wu32, default),
             ('1', 'wreg', x256, wp, wu, 'rmnet_conv3x3_split_f32'), ('1', 'lds', x256, wp, wu, 'rmnet_conv3x3_split_lds_f32'),
             ('0', None, x256, wp, wu, default)]
    for rows, kernel, x, p, u, entry in cases:
        monkeypatch.setenv('RMNET_CONV3X3_ROWS', rows)
        if kernel is None:
            monkeypatch.delenv('RMNET_CONV3X3_KERNEL', raising=False)
        else:
            monkeypatch.setenv('RMNET_CONV3X3_KERNEL', kernel)
        del spy.names[:]
        ops.conv3x3_split(x, p, u, bias)
        torch.cuda.synchronize()
        assert [n for n in spy.names if n.startswith('rmnet_conv3x3')] == [entry], (rows, kernel, tuple(x.shape), spy.names)
    monkeypatch.setenv('RMNET_CONV3X3_ROWS', 'yes')
    monkeypatch.delenv('RMNET_CONV3X3_KERNEL', raising=False)
    del spy.names[:]
    with pytest.raises(RuntimeError, match='RMNET_CONV3X3_ROWS'):
        ops.conv3x3_split(x256, wp, wu, bias)
    assert not spy.names


@pytest.mark.gpu
def test_the_export_refuses_cin_128_and_writes_nothing():
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    n, h, w, cin = 1, 4, 6, 128
    x = _cl(torch.randn((n, cin, h, w), generator=torch.Generator().manual_seed(7)))
    wp, wu = ops.conv3x3_pack(torch.randn((256, cin, 3, 3), generator=torch.Generator().manual_seed(8)).to(dev()))
    buf, out = _guarded_out(n, h, w)
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    p = lambda t: ops._ptr(t)
    with torch.cuda.device(dev()):
        rc = lib.rmnet_conv3x3_rows_f32(p(x), p(wp), p(wu), None, None, 0, n, h, w, cin, p(out), p(rw), ops._stream(dev()))
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    assert bool((buf == SENTINEL).all()) and int(rw.item()) == 0


# ================================================================================================ graph capture
@pytest.mark.gpu
def test_a_captured_call_replays_to_the_eager_result(monkeypatch):
    """The eager call comes first: it sets the kernel's dynamic-LDS attribute, which a capture must not."""
    from rmnet_amd import ops
    wp, wu, bias = _weights()
    x, res = _inputs((2, 9, 15))
    _select(monkeypatch, 'rows')
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    eager = ops.conv3x3_split(x, wp, wu, bias, res, relu_in=True, range_word=rw)
    torch.cuda.synchronize()
    out = torch.full_like(eager, SENTINEL)
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        ops.conv3x3_split(x, wp, wu, bias, res, relu_in=True, out=out, range_word=rw)
    torch.cuda.current_stream(dev()).wait_stream(side)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.conv3x3_split(x, wp, wu, bias, res, relu_in=True, out=out, range_word=rw)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _assert_equal(out, eager, 'graph replay')
    assert int(rw.item()) == 0


# ================================================================================================ CPU: what the compiler gives
def test_the_kernel_has_no_static_lds_no_scratch_no_spill_and_its_launch_size_is_the_row_image(tmp_path):
    """Compile-only, with tests/test_kernel_resources.py's compile step and metadata reader (the metadata alone: no instruction is
    looked at).  One kernel in the file; its LDS is dynamic, so the compile-time size is 0 and the launch constant is checked against
    the derivation: 8 channel blocks x (hi, lo) x (130 staged rows + 4 rows of zeros, one per 64-byte quarter of a bank row) x
    32 fp16."""
    import test_kernel_resources as KR
    found = KR._kernels(KR._compile('conv3x3_rows.hip', str(tmp_path / 'conv3x3_rows.s')))
    assert len(found) == 1, sorted(found)
    k = KR._one(found, '12conv3x3_rowsE')
    print('conv3x3_rows   LDS %6d  scratch %d  VGPRs %3d  spilled %d' % tuple(k[f] for f in KR.FIELDS))
    name = list(found)[0]
    assert 'conv3x3_split' not in name and 'conv3x3_wreg' not in name
    assert k['group_segment_fixed_size'] == 0
    assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
    assert k['vgpr_count'] <= 256, k
    derived = (CIN // 32) * 2 * (TILE + 2 + 4) * 32 * 2
    assert derived == 137216 <= 160 * 1024 == 163840
    src = open(os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv3x3_rows.hip')).read()
    m = re.search(r'static_assert\(kRowsLdsBytes == (\d+),', src)
    assert m and int(m.group(1)) == derived
    assert 'static_assert(kRowsLdsBytes <= kLdsBytesPerCU' in src
    assert len(re.findall(r'hipLaunchKernelGGL\(conv3x3_rows,[^;]*kRowsLdsBytes', src)) == 1
