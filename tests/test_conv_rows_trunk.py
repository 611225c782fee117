# -*- coding: utf-8 -*-
"""conv_rows<C> (csrc/conv_rows.hip), the trunks' stride-1 3x3 convolution with Cin = Cout = C in {64, 128, 256} on a split input,
which stages a whole tap row of activations in LDS once, against conv_split_pre (rmnet_conv_split_pre_f32) on the same inputs.  The
K order per accumulator, the operand bits and the epilogue expressions are the same, so the comparison is ``torch.equal`` on an
integer view of the output (NaNs compare as their bits) and ``==`` on the range word: no tolerance is involved anywhere.

What is new in the kernel is its addressing: a workgroup owns MT = 32768 / C consecutive pixels, stages the MT + 2 pixels
m0 + dy*W - 1 .. m0 + dy*W + MT of each tap row, clamped into the tensor, and a lane picks per (pixel tile, tap) between the staged
row and a row of zeros.  The shapes (N, H, W), per C: M < MT; degenerate rows and columns; M = MT exactly and MT + 1; a tile inside
one row; image borders inside a tile; and 5 x 9 x 13, where the tile edges at 128, 256 and 512 fall inside images and the halo
crosses images.

  * every combination of fp32 / split output, ReLU, shift and range word on inputs of mixed sign up to the window;
  * one live tap at a time, the exact integers against numpy (tests/presplit_ref.py makes the split input);
  * saturated, NaN and Inf bit patterns planted in the split input at tile, halo, row-wrap and image boundaries: a tap that reads
    through a border is a different bit pattern;
  * the range word of a split output that leaves the window, and 0 for an fp32 output;
  * sentinels around ``out``, ``x`` unchanged, a captured call replayed;
  * what the export refuses, the switch and the class tuple by the export that is called, a whole bottleneck either way;
  * CPU: what the compiler gives each instance."""

import functools
import itertools

import numpy as np
import pytest
import torch

import presplit_ref

CLASSES = (64, 128, 256)
MT = {64: 512, 128: 256, 256: 128}          # pixels per workgroup: 32768 / C
EXACT = {128: (1, 8, 16), 256: (1, 16, 16), 512: (2, 16, 16)}          # M = MT
PLUS1 = {128: (1, 3, 43), 256: (1, 1, 257), 512: (1, 19, 27)}           # M = MT + 1
E_UNSUPPORTED = -4             # include/rmnet_hip.h
X_SPLIT, OUT_SPLIT, RELU_OUT = 4, 8, 2
GUARD = 64                     # 4-byte words in front of and behind the output (a multiple of 4: out stays 16-byte aligned)
SENTINEL = 0x5A5A5A5A


def shapes(c):
    mt = MT[c]
    return [(1, 3, 5), (2, 1, 1), (1, 7, 1), (1, 1, 9), EXACT[mt], PLUS1[mt], (1, 2, mt + 2), (3, 5, 7), (5, 9, 13)]


CASES = [(c, s) for c in CLASSES for s in shapes(c)]


def test_the_shapes_are_what_they_are_meant_to_be():
    for c in CLASSES:
        mt = MT[c]
        assert mt * c == 32768
        n, h, w = EXACT[mt]
        assert n * h * w == mt
        n, h, w = PLUS1[mt]
        assert n * h * w == mt + 1
        assert 5 * 9 * 13 == 585 > 512


def dev():
    return torch.device('cuda', 0)


def _select(monkeypatch, rows):
    """rows: the switch on and every class enabled; else the switch off (conv_split_pre)."""
    from rmnet_amd import ops
    monkeypatch.setenv('RMNET_CONV_PRESPLIT', '1')
    monkeypatch.setenv('RMNET_TRUNK_ROWS', '1' if rows else '0')
    monkeypatch.setattr(ops, 'TRUNK_ROWS_CLASSES', ops.TRUNK_ROWS_ALL)


@functools.lru_cache(maxsize=None)
def _weights(c):
    """(wpack, w_unscale, shift) of one random [C, C, 3, 3] convolution, shared by every shape and never written.  The weights are
    scaled so that most outputs of an input that fills the window stay inside it, and some do not."""
    from rmnet_amd import ops
    g = torch.Generator().manual_seed(2100 + c)
    wt = torch.randn((c, c, 3, 3), generator=g) / (3.0 * c ** 0.5)
    shift = torch.randn(c, generator=g) * 50
    wp, wu = ops.conv_split_pack(wt.to(dev()))
    return wp, wu, shift.to(dev())


@functools.lru_cache(maxsize=None)
def _input(c, shape):
    """A split activation on the device: mixed sign, most elements small, one in eight spread up to the window (|x| < 1023.5); made
    once per (C, shape) and never written."""
    from rmnet_amd import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(3100 + 1009 * c + 97 * n + 13 * h + w)
    x = torch.randn((n, h, w, c), generator=g) * 3
    big = (torch.rand((n, h, w, c), generator=g) * 2 - 1) * 1023
    x = torch.where(torch.rand((n, h, w, c), generator=g) < 0.125, big, x)
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    xs = ops.split_act(x.permute(0, 3, 1, 2).to(dev()).contiguous(memory_format=torch.channels_last), range_word=rw)
    assert int(rw.item()) == 0 and tuple(xs.shape) == (n, h, w, c // 32, 2, 32)
    return xs


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _assert_bits(new, old, what):
    assert new.dtype == old.dtype and new.shape == old.shape, what
    a, b = _bits(new), _bits(old)
    if torch.equal(a, b):
        return
    bad = (a != b).nonzero()
    first = [(tuple(int(v) for v in i), int(a[tuple(i)]), int(b[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d words differ; first (index, new, reference): %s' % (what, bad.shape[0], a.numel(), first))


def _conv(monkeypatch, rows, xs, wp, wu, shift, relu_out, out_split, use_rw):
    """ops.conv_split on one side of the switch -> (out, range word or None); x is checked to be unchanged."""
    from rmnet_amd import ops
    _select(monkeypatch, rows)
    rw = torch.zeros(1, dtype=torch.int32, device=dev()) if use_rw else None
    before = xs.clone()
    out = ops.conv_split(xs, wp, wu, shift, ksize=3, stride=1, relu_out=relu_out, range_word=rw, out_presplit=out_split)
    torch.cuda.synchronize()
    assert torch.equal(_bits(xs), _bits(before)), 'x changed'
    return out, (int(rw.item()) if use_rw else None)


# ================================================================================================ every flag combination
@pytest.mark.gpu
@pytest.mark.parametrize('c,shape', CASES)
def test_outputs_and_range_words_equal_conv_split_pre_bit_for_bit(monkeypatch, c, shape):
    wp, wu, shift = _weights(c)
    xs = _input(c, shape)
    for out_split, relu_out, use_shift, use_rw in itertools.product((False, True), repeat=4):
        args = (xs, wp, wu, shift if use_shift else None, relu_out, out_split, use_rw)
        new, bad_new = _conv(monkeypatch, True, *args)
        old, bad_old = _conv(monkeypatch, False, *args)
        what = 'C %d %s split out %s relu %s shift %s range word %s' % (c, shape, out_split, relu_out, use_shift, use_rw)
        _assert_bits(new, old, what)
        assert bad_new == bad_old, (what, bad_new, bad_old)
        if use_rw and not out_split:
            assert bad_new == 0, what
        assert float(new.float().abs().max()) > 1.0          # (not a comparison of two empty results)


# ================================================================================================ integers: one live tap at a time
def _integer_case(c, shape, tap):
    """x: (flat NHWC index mod 2039) - 1019 (64 x is an fp16 number inside the window: lo = 0; neighbouring pixels and channels
    differ).  Weight: output channel co has one live element, +-(1 .. 5), at input channel (7 co + 3) mod C of tap ``tap``.  Shift: a
    different integer per channel.  Every output is one product plus the shift, exact in fp32."""
    n, h, w = shape
    flat = np.arange(n * h * w * c, dtype=np.int64)
    x = ((flat % 2039) - 1019).astype(np.float32).reshape(n, h, w, c)
    co = np.arange(c)
    ci = (7 * co + 3) % c
    val = ((co % 5) + 1) * np.where(co % 2, -1, 1)
    shift = (co - c // 2).astype(np.float32)
    ky, kx = tap // 3, tap % 3
    wt = np.zeros((c, c, 3, 3), dtype=np.float32)
    wt[co, ci, ky, kx] = val
    xp = np.zeros((n, h + 2, w + 2, c), dtype=np.float32)
    xp[:, 1:-1, 1:-1] = x
    want = np.empty((n, c, h, w), dtype=np.float32)
    for k in range(c):
        want[:, k] = val[k] * xp[:, ky:ky + h, kx:kx + w, ci[k]] + shift[k]
    xs, counted = presplit_ref.split_form(x)
    assert counted == 0
    return torch.from_numpy(xs), torch.from_numpy(wt), torch.from_numpy(shift), torch.from_numpy(want)


@pytest.mark.gpu
@pytest.mark.parametrize('tap', range(9))
@pytest.mark.parametrize('c,shape', [(c, s) for c in CLASSES for s in ((3, 5, 7), (1, 2, MT[c] + 2))])
def test_one_live_tap_returns_the_exact_integers(monkeypatch, c, shape, tap):
    from rmnet_amd import ops
    xs, wt, shift, want = _integer_case(c, shape, tap)
    wp, wu = ops.conv_split_pack(wt.to(dev()))
    args = (xs.to(dev()), wp, wu, shift.to(dev()), False, False, True)
    new, bad_new = _conv(monkeypatch, True, *args)
    old, bad_old = _conv(monkeypatch, False, *args)
    assert bad_new == bad_old == 0
    want = want.to(dev())
    assert int((want != shift.to(dev()).view(1, -1, 1, 1)).sum()) > want.numel() // 4       # (many outputs read a live product)
    assert new.shape == want.shape
    _assert_bits(new, want.contiguous(memory_format=torch.channels_last), 'C %d %s tap %d integers against numpy' % (c, shape, tap))
    _assert_bits(new, old, 'C %d %s tap %d integers' % (c, shape, tap))


# ================================================================================================ border leaks
PLANT_HI = [0x7BFF, -0x0401, 0x7E00, 0x7C00, -0x0400]          # int16 patterns: +65504, -65504 (0xFBFF), NaN, +Inf, -Inf (0xFC00)


def _plant_pixels(shape, mt):
    """Flat pixel indices: the first and last pixel of every tile, pixels that tile 0 and tile 1 stage only as halo (below and above
    their own), the row-wrap pixels (last of a row, first of the next), the first and last pixel of every image."""
    n, h, w = shape
    m = n * h * w
    px = set()
    for m0 in range(0, m, mt):
        px.update((m0, min(m0 + mt, m) - 1))
    px.update(p for p in (mt + w - 1, mt + w, mt + w // 2, mt - w // 2 - 1, mt - w, mt - w - 1) if 0 <= p < m)
    px.update(p for p in (w - 1, w, m - w - 1, m - w) if 0 <= p < m)
    for i in range(n):
        px.update((i * h * w, (i + 1) * h * w - 1))
    return sorted(px)


def _planted_input(c, shape):
    """_input with every pattern of PLANT_HI in the hi plane at each pixel of _plant_pixels, in the first and in the last channel
    block (a different channel per pattern); the lo halves stay what they were."""
    n, h, w = shape
    xs = _input(c, shape).clone()
    flat = xs.view(n * h * w, c // 32, 2, 32).view(torch.int16)
    pixels = _plant_pixels(shape, MT[c])
    for p in pixels:
        for blk in (0, c // 32 - 1):
            for k, v in enumerate(PLANT_HI):
                flat[p, blk, 0, 3 + 6 * k] = v
    return xs, len(pixels)


@pytest.mark.gpu
@pytest.mark.parametrize('out_split', [False, True])
@pytest.mark.parametrize('c,shape', [(c, s) for c in CLASSES for s in ((5, 9, 13), (1, 2, MT[c] + 2), PLUS1[MT[c]])])
def test_planted_saturated_nan_and_inf_patterns_do_not_leak_through_a_border(monkeypatch, c, shape, out_split):
    wp, wu, shift = _weights(c)
    xs, pixels = _planted_input(c, shape)
    assert pixels >= 4
    new, bad_new = _conv(monkeypatch, True, xs, wp, wu, shift, False, out_split, True)
    old, bad_old = _conv(monkeypatch, False, xs, wp, wu, shift, False, out_split, True)
    if not out_split:           # (some outputs see a plant, some none; a split output holds a counted NaN as -65504)
        assert int(old.isnan().sum()) > 0 and int((~old.isnan()).sum()) > 0
    _assert_bits(new, old, 'C %d %s planted patterns, split out %s' % (c, shape, out_split))
    assert bad_new == bad_old and (bad_new > 0) == out_split, (bad_new, bad_old)


# ================================================================================================ the range word of a split output
@pytest.mark.gpu
@pytest.mark.parametrize('c', CLASSES)
def test_the_range_word_counts_the_produced_elements_outside_the_window(monkeypatch, c):
    """A shift of +-3000 on four channels puts every output of those channels outside the window (4 x M elements at least), ReLU
    brings the negative two back to 0; a NaN in the input adds the outputs that read it."""
    shape = (5, 9, 13)
    m = 5 * 9 * 13
    wp, wu, shift = _weights(c)
    shift = shift.clone()
    shift[1], shift[c // 2] = 3000.0, -3000.0
    shift[33], shift[c - 1] = 5000.0, -5000.0
    xs = _input(c, shape).clone()
    xs.view(m, c // 32, 2, 32).view(torch.int16)[300, 1, 0, 5] = 0x7E00
    for relu_out in (False, True):
        new, bad_new = _conv(monkeypatch, True, xs, wp, wu, shift, relu_out, True, True)
        old, bad_old = _conv(monkeypatch, False, xs, wp, wu, shift, relu_out, True, True)
        _assert_bits(new, old, 'C %d pushed past the window, relu %s' % (c, relu_out))
        assert bad_new == bad_old, (bad_new, bad_old)
        assert bad_new >= (2 if relu_out else 4) * m + 9 * (c - 4), bad_new          # (pixel 300 is an interior pixel: nine readers)
        f32, bad_f32 = _conv(monkeypatch, True, xs, wp, wu, shift, relu_out, False, True)
        assert bad_f32 == 0
        assert int(f32.isnan().sum()) >= 9 * c


# ================================================================================================ memory safety and reuse
def _raw(entry, xs, wp, wu, shift, flags, n, h, w, cin, cout, ksize, stride, out, res=None, out2=None, out_split=0, rw=None):
    from rmnet_amd import _lib, ops
    p = ops._ptr
    with torch.cuda.device(dev()):
        rc = getattr(_lib.load(), entry)(p(xs), p(wp), p(wu), p(shift), p(res), flags, n, h, w, cin, cout, ksize, stride, p(out), p(out2),
                                         out_split, p(rw), ops._stream(dev()))
    torch.cuda.synchronize()
    return rc


def _guarded(words):
    buf = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    out = buf[GUARD:GUARD + words]
    assert out.data_ptr() % 16 == 0
    return buf, out


@pytest.mark.gpu
@pytest.mark.parametrize('out_split', [False, True])
@pytest.mark.parametrize('c', CLASSES)
def test_nothing_is_written_outside_out_and_x_is_left_alone(c, out_split):
    wp, wu, shift = _weights(c)
    for shape in ((1, 3, 5), PLUS1[MT[c]], (5, 9, 13)):
        n, h, w = shape
        xs = _input(c, shape)
        before = xs.clone()
        flags = X_SPLIT | RELU_OUT | (OUT_SPLIT if out_split else 0)
        outs = []
        for entry in ('rmnet_conv_rows_pre_f32', 'rmnet_conv_split_pre_f32'):
            buf, out = _guarded(n * h * w * c)
            assert _raw(entry, xs, wp, wu, shift, flags, n, h, w, c, c, 3, 1, out) == 0
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), '%s wrote outside out' % entry
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), (c, shape)
        assert torch.equal(_bits(xs), _bits(before))


@pytest.mark.gpu
@pytest.mark.parametrize('c', CLASSES)
def test_a_captured_call_replays_to_the_eager_result(monkeypatch, c):
    """The eager call comes first: it sets the instance's dynamic-LDS attribute, which a capture must not."""
    from rmnet_amd import ops
    wp, wu, shift = _weights(c)
    xs = _input(c, (5, 9, 13))
    _select(monkeypatch, True)
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    call = lambda: ops.conv_split(xs, wp, wu, shift, ksize=3, relu_out=True, range_word=rw, out_presplit=True)
    eager = call()
    torch.cuda.synchronize()
    count = int(rw.item())
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream(dev()).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    torch.cuda.synchronize()
    out.zero_()
    rw.zero_()
    g.replay()
    torch.cuda.synchronize()
    _assert_bits(out, eager, 'C %d graph replay' % c)
    assert int(rw.item()) == count


# ================================================================================================ refusals
@pytest.mark.gpu
def test_the_export_refuses_everything_outside_its_class_and_writes_nothing():
    from rmnet_amd import ops
    g = torch.Generator().manual_seed(9)
    n, h, w = 1, 4, 6
    m = n * h * w

    def pack(cout, cin, k):
        return ops.conv_split_pack(torch.randn((cout, cin, k, k), generator=g).to(dev()))

    def split_x(cin):
        return ops.split_act(torch.randn((n, cin, h, w), generator=g).to(dev()).contiguous(memory_format=torch.channels_last))

    cases = []          # (what, x, pack, flags, cin, cout, ksize, stride, res, out2, out_split)
    cases.append(('stride 2', split_x(64), pack(64, 64, 3), X_SPLIT, 64, 64, 3, 2, False, False, 0))
    cases.append(('ksize 1', split_x(64), pack(64, 64, 1), X_SPLIT, 64, 64, 1, 1, False, False, 0))
    cases.append(('Cin != Cout', split_x(64), pack(128, 64, 3), X_SPLIT, 64, 128, 3, 1, False, False, 0))
    cases.append(('C 32', split_x(32), pack(64, 32, 3), X_SPLIT, 32, 32, 3, 1, False, False, 0))
    cases.append(('C 512', split_x(512), pack(512, 512, 3), X_SPLIT, 512, 512, 3, 1, False, False, 0))
    x32 = torch.randn((n, h, w, 64), generator=g).to(dev())
    cases.append(('fp32 x', x32, pack(64, 64, 3), 0, 64, 64, 3, 1, False, False, 0))
    cases.append(('fp32 x, split out', x32, pack(64, 64, 3), OUT_SPLIT, 64, 64, 3, 1, False, False, 0))
    cases.append(('res', split_x(64), pack(64, 64, 3), X_SPLIT, 64, 64, 3, 1, True, False, 0))
    cases.append(('out2', split_x(64), pack(64, 64, 3), X_SPLIT, 64, 64, 3, 1, False, True, 32))
    for what, x, (wp, wu), flags, cin, cout, k, s, use_res, use_out2, osplit in cases:
        buf, out = _guarded(m * max(cout, 64))
        res = torch.zeros(m * cout, device=dev()) if use_res else None
        buf2, out2 = _guarded(m * cout) if use_out2 else (None, None)
        rw = torch.zeros(1, dtype=torch.int32, device=dev())
        rc = _raw('rmnet_conv_rows_pre_f32', x, wp, wu, None, flags, n, h, w, cin, cout, k, s, out, res=res, out2=out2, out_split=osplit,
                  rw=rw)
        assert rc == E_UNSUPPORTED, (what, rc)
        assert bool((buf == SENTINEL).all()) and int(rw.item()) == 0, what
        assert buf2 is None or bool((buf2 == SENTINEL).all()), what


# ================================================================================================ the switch
def test_the_switch_takes_0_and_1_and_anything_else_raises(monkeypatch):
    from rmnet_amd import ops
    assert ops.TRUNK_ROWS_DEFAULT in (False, True)
    assert ops.TRUNK_ROWS_ALL == CLASSES and set(ops.TRUNK_ROWS_CLASSES) <= set(CLASSES)
    monkeypatch.delenv('RMNET_TRUNK_ROWS', raising=False)
    assert ops.trunk_rows_enabled() is ops.TRUNK_ROWS_DEFAULT
    for value, on in (('0', False), ('1', True)):
        monkeypatch.setenv('RMNET_TRUNK_ROWS', value)
        assert ops.trunk_rows_enabled() is on
    for value in ('yes', '', 'true', '2'):
        monkeypatch.setenv('RMNET_TRUNK_ROWS', value)
        with pytest.raises(RuntimeError, match='RMNET_TRUNK_ROWS'):
            ops.trunk_rows_enabled()


class _Spy(object):
    """The loaded library, recording the name of every export that is fetched from it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


@pytest.mark.gpu
def test_the_switch_and_the_class_tuple_reach_the_export_they_should(monkeypatch):
    from rmnet_amd import _lib, ops
    shape = (1, 3, 5)
    n, h, w = shape
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    rows, pre, plain = 'rmnet_conv_rows_pre_f32', 'rmnet_conv_split_pre_f32', 'rmnet_conv_split_f32'
    g = torch.Generator().manual_seed(11)
    x32 = torch.randn((n, 64, h, w), generator=g).to(dev()).contiguous(memory_format=torch.channels_last)
    res = torch.randn((n, 64, h, w), generator=g).to(dev()).contiguous(memory_format=torch.channels_last)
    wp1, wu1 = ops.conv_split_pack(torch.randn((64, 64, 1, 1), generator=g).to(dev()))
    wpw, wuw = ops.conv_split_pack(torch.randn((128, 64, 3, 3), generator=g).to(dev()))

    def called(**kw):
        del spy.names[:]
        c = kw.pop('c', 64)
        x = kw.pop('x', None)
        p, u = kw.pop('pack', _weights(c)[:2])
        ops.conv_split(_input(c, shape) if x is None else x, p, u, **kw)
        torch.cuda.synchronize()
        return [k for k in spy.names if k.startswith('rmnet_conv')]

    monkeypatch.setenv('RMNET_TRUNK_ROWS', '1')
    monkeypatch.setattr(ops, 'TRUNK_ROWS_CLASSES', CLASSES)
    for c in CLASSES:
        assert called(c=c) == [rows] and called(c=c, out_presplit=True, relu_out=True) == [rows]
    assert called(stride=2) == [pre]
    assert called(ksize=1, pack=(wp1, wu1)) == [pre]
    assert called(pack=(wpw, wuw)) == [pre]                     # Cin != Cout
    assert called(res=res) == [pre]
    assert called(x=x32) == [plain]                             # fp32 input: where it has always been
    assert called(x=x32, out_presplit=True) == [pre]
    monkeypatch.setattr(ops, 'TRUNK_ROWS_CLASSES', (128,))
    assert called(c=64) == [pre] and called(c=128) == [rows] and called(c=256) == [pre]
    monkeypatch.setattr(ops, 'TRUNK_ROWS_CLASSES', ())
    assert called(c=128) == [pre]
    monkeypatch.setattr(ops, 'TRUNK_ROWS_CLASSES', CLASSES)
    monkeypatch.setenv('RMNET_TRUNK_ROWS', '0')
    for c in CLASSES:
        assert called(c=c) == [pre]
    monkeypatch.setenv('RMNET_TRUNK_ROWS', 'yes')
    del spy.names[:]
    with pytest.raises(RuntimeError, match='RMNET_TRUNK_ROWS'):
        ops.conv_split(_input(64, shape), *_weights(64)[:2])
    assert not spy.names


@pytest.mark.gpu
@pytest.mark.parametrize('width', [64, 256])
def test_a_whole_bottleneck_gives_equal_bits_either_way(monkeypatch, width):
    """An identity block (stride 1: its conv2 is in the class) on a 9 x 13 map; width 256 hands conv3 a split input as well."""
    from rmnet_amd import _lib, networks, ops
    torch.backends.cudnn.benchmark = False
    block = networks.procedural_init_(torch.nn.Sequential(networks._Bottleneck(4 * width, width, 1, False)))
    block = block.to(dev()).eval()
    networks.fuse_epilogues_(block)
    block = block.to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(23)
    x = torch.relu(torch.randn((2, 4 * width, 9, 13), generator=g)).to(dev()).contiguous(memory_format=torch.channels_last)
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    outs = []
    for rows in (False, True):
        _select(monkeypatch, rows)
        del spy.names[:]
        word = ops.conv_range_word(dev())
        word.zero_()
        with torch.no_grad():
            outs.append(block(x).clone())
        torch.cuda.synchronize()
        assert int(word.item()) == 0
        names = [k for k in spy.names if k.startswith('rmnet_conv')]
        assert names.count('rmnet_conv_rows_pre_f32') == (1 if rows else 0), names
        assert len(names) == 3, names
    _assert_bits(outs[1], outs[0], 'bottleneck width %d' % width)
    assert float(outs[0].abs().max()) > 0


# ================================================================================================ CPU: what the compiler gives
def test_every_instance_has_no_static_lds_no_scratch_no_spill_and_at_most_256_vgprs(tmp_path):
    """Compile-only, with tests/test_kernel_resources.py's compile step and metadata reader (the metadata alone: no instruction is
    looked at).  Six instances (C x output form); their LDS is dynamic, so the compile-time size is 0, and the launch sizes are
    checked against the derivation: C / 32 channel blocks x (hi, lo) x (MT + 2 staged rows + 4 rows of zeros) x 32 fp16."""
    import os
    import re

    import test_kernel_resources as KR
    from conftest import ROOT
    found = KR._kernels(KR._compile('conv_rows.hip', str(tmp_path / 'conv_rows.s')))
    assert len(found) == 6, sorted(found)
    for c in CLASSES:
        for os_ in (0, 1):
            k = KR._one(found, '9conv_rowsILi%dELb%dEE' % (c, os_))
            print('conv_rows<%3d, %d>  LDS %6d  scratch %d  VGPRs %3d  spilled %d' % ((c, os_) + tuple(k[f] for f in KR.FIELDS)))
            assert k['group_segment_fixed_size'] == 0
            assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
            assert k['vgpr_count'] <= 256, k
    derived = [(c // 32) * 2 * (MT[c] + 2 + 4) * 32 * 2 for c in (256, 128, 64)]
    assert derived == [137216, 134144, 132608] and max(derived) <= 160 * 1024
    src = open(os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv_rows.hip')).read()
    m = re.search(r'static_assert\(rows_lds_bytes\(256\) == (\d+) && rows_lds_bytes\(128\) == (\d+) && rows_lds_bytes\(64\) == (\d+),', src)
    assert m and [int(v) for v in m.groups()] == derived
    assert 'static_assert(rows_lds_bytes(256) <= kLdsBytesPerCU' in src
    assert len(re.findall(r'hipLaunchKernelGGL\(\(conv_rows<C, OS>\),[^;]*rows_lds_bytes\(C\)', src)) == 1
