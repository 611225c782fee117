# -*- coding: utf-8 -*-
"""conv3x3_wreg (csrc/conv3x3.hip), the decoder convolution whose waves load their weight fragments straight from the pack into
registers, against conv3x3_split, the kernel that stages the weights through LDS.  The two share arguments, arithmetic, the K
order per accumulator and the epilogue expressions, and the 16-aligned MFMA tiles are the same, so the reference is the old
kernel and the comparison is ``torch.equal`` on the output and ``==`` on the range word: no tolerance is involved.  Every GPU case
runs both entries (rmnet_conv3x3_split_f32 and rmnet_conv3x3_split_lds_f32, through ``ops.conv3x3_split`` and its
RMNET_CONV3X3_KERNEL switch) on the same inputs.

What differs between the kernels is who owns what -- wave w owns all 128 pixels x channels 32w .. 32w+31 instead of a 64 x 64
tile, and a lane fetches its own 16 bytes of each weight fragment -- so the shapes are those at which that mapping, the pixel tail
and the K walk can go wrong:

  (1,1,1,32)    one pixel, one step per tap, all eight border taps outside
  (2,5,7,32)    M = 70 < 128, taps crossing rows and the image boundary between the two images
  (1,9,15,96)   M = 135: one full workgroup and a 7-pixel one; odd number of channel blocks (the weight register sets change
                names once per tap)
  (2,8,8,160)   M = 128 exactly; odd number of channel blocks
  (1,12,11,64)  M = 132; even number of channel blocks (tap 0 then has an odd number of steps left after the prologue's)
  (1,3,50,256)  M = 150; the decoder's own Cin

  * randn x 3 inputs (lo planes not zero) with every combination of input ReLU, output ReLU, bias, and residual absent / present /
    ``out is res``, and sentinels in front of and behind the output buffer;
  * an integer family: a different small integer in every input element and ONE live weight per output channel, at a channel and
    a tap that differ per output channel -- the output is exact, and a wrong (wave, tile) -> channel mapping or a wrong fragment
    shows as a wrong integer; checked against numpy as well as against the old entry;
  * the range word: out-of-window values of either sign, NaN and Inf at a corner, an edge and an interior pixel, in the first and
    in the last channel block, with and without the input ReLU (which removes the negative ones); ``range_word=None``;
  * the switch, by the export that is called; an unknown value raises;
  * CPU: the compiler gives the new kernel the X-only double buffer it declares, no scratch, no spill, at most 256 VGPRs, and
    conv3x3_split still has its 98304 B."""

import functools

import numpy as np
import pytest
import torch

SHAPES = [(1, 1, 1, 32), (2, 5, 7, 32), (1, 9, 15, 96), (2, 8, 8, 160), (1, 12, 11, 64), (1, 3, 50, 256), (1, 2, 9, 1024)]
GUARD = 64                     # floats in front of and behind the output (a multiple of 4: out stays 16-byte aligned)
SENTINEL = -12345.5
K_PER_BARRIER = 32             # conv3x3_wreg: K per step and barrier


def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _rw():
    return torch.zeros(1, dtype=torch.int32, device=dev())


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x channels-last, wpack, w_unscale, bias, res channels-last) on the device; made once per shape and never written."""
    from rmnet_amd import ops
    n, h, w, cin = shape
    g = torch.Generator().manual_seed(1000 + n * h * w + cin)
    x = torch.randn((n, cin, h, w), generator=g) * 3
    wt = torch.randn((256, cin, 3, 3), generator=g)
    bias = torch.randn(256, generator=g)
    res = torch.randn((n, 256, h, w), generator=g) * 3
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    return _cl(x), wp, wu, bias.to(dev()), _cl(res)


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
    """One launch of the entry ``kernel`` into a guarded buffer -> (out, range word or None); the guards are checked here."""
    from rmnet_amd import ops
    monkeypatch.setenv('RMNET_CONV3X3_KERNEL', kernel)
    n, _, h, w = x.shape
    rw = _rw() if range_word == 'own' else None
    buf, out = _guarded_out(n, h, w, res if res_mode == 'inplace' else None)
    r = {'none': None, 'res': res, 'inplace': out}[res_mode]
    got = ops.conv3x3_split(x, wp, wu, bias, r, relu_in=relu_in, relu_out=relu_out, out=out, range_word=rw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), '%s wrote outside out' % kernel
    assert not bool((out == SENTINEL).any()), '%s left output elements unwritten' % kernel
    return out, (int(rw.item()) if rw is not None else None)


def _same(a, b):
    """torch.equal, with NaN equal to NaN (the range cases plant NaN on purpose)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _assert_equal(new, old, what):
    """torch.equal, said with the first differing elements."""
    if not torch.equal(new, old):
        _assert_same(new, old, what)
        pytest.fail('%s: NaN in the outputs' % what)


def _assert_same(new, old, what):
    if _same(new, old):
        return
    bad = ((new != old) & ~(new.isnan() & old.isnan())).nonzero()
    first = [(tuple(int(v) for v in i), float(new[tuple(i)]), float(old[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index [n, co, y, x], wreg, lds): %s' % (what, bad.shape[0], new.numel(), first))


# ================================================================================================ randn: every flag combination
@pytest.mark.gpu
@pytest.mark.parametrize('res_mode', ['none', 'res', 'inplace'])
@pytest.mark.parametrize('use_bias', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_outputs_and_range_words_equal_the_lds_kernels_bit_for_bit(monkeypatch, shape, use_bias, res_mode):
    x, wp, wu, bias, res = _inputs(shape)
    for relu_in in (False, True):
        for relu_out in (False, True):
            args = (x, wp, wu, bias if use_bias else None, res_mode, res, relu_in, relu_out)
            new, bad_new = _call(monkeypatch, 'wreg', *args)
            old, bad_old = _call(monkeypatch, 'lds', *args)
            assert bad_new == bad_old == 0
            _assert_equal(new, old, '%s bias %s %s relu_in %s relu_out %s' % (shape, use_bias, res_mode, relu_in, relu_out))
            assert float(new.abs().max()) > 1.0          # (not a comparison of two empty results)


# ================================================================================================ integers: one live weight per channel
def _integer_case(shape):
    """x: (flat NHWC index mod 2039) - 1019 (64 x is an fp16 number inside the window).  Weight: output channel co has one live
    element, +-(1 .. 5), at input channel (7 co + 3) mod Cin and tap (co + co // 9) mod 9: neighbours differ in both.  Bias: a
    different integer per channel.  Every output is one product plus the bias, exact in fp32."""
    n, h, w, cin = shape
    flat = np.arange(n * h * w * cin, dtype=np.int64)
    x = ((flat % 2039) - 1019).astype(np.float32).reshape(n, h, w, cin)
    co = np.arange(256)
    ci, tap = (7 * co + 3) % cin, (co + co // 9) % 9
    val = ((co % 5) + 1) * np.where(co % 2, -1, 1)
    bias = (co - 128).astype(np.float32)
    wt = np.zeros((256, cin, 3, 3), dtype=np.float32)
    wt[co, ci, tap // 3, tap % 3] = val
    xp = np.zeros((n, h + 2, w + 2, cin), dtype=np.float32)
    xp[:, 1:-1, 1:-1] = x
    want = np.empty((n, 256, h, w), dtype=np.float32)
    for c in range(256):
        ky, kx = tap[c] // 3, tap[c] % 3
        want[:, c] = val[c] * xp[:, ky:ky + h, kx:kx + w, ci[c]] + bias[c]
    return torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), torch.from_numpy(bias), torch.from_numpy(want)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 5, 7, 32), (1, 9, 15, 96)])
def test_one_live_weight_per_output_channel_returns_the_exact_integers(monkeypatch, shape):
    from rmnet_amd import ops
    x, wt, bias, want = _integer_case(shape)
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    args = (_cl(x), wp, wu, bias.to(dev()), 'none', None, False, False)
    new, bad_new = _call(monkeypatch, 'wreg', *args)
    old, bad_old = _call(monkeypatch, 'lds', *args)
    assert bad_new == bad_old == 0
    want = want.to(dev())
    assert int((want != bias.to(dev()).view(1, -1, 1, 1)).sum()) > want.numel() // 2       # (most outputs read a live product)
    _assert_equal(new, want, '%s integers against numpy' % (shape,))
    _assert_equal(new, old, '%s integers' % (shape,))


# ================================================================================================ the range word
RANGE_SHAPE = (1, 9, 15, 96)
PLANT_VALUES = [2000.0, float('nan'), float('inf'), -2000.0]


def _planted_input():
    """randn x 3 with every value of PLANT_VALUES at a corner, an edge and an interior pixel, in the first and in the last channel
    block -> (x, list of planted values)."""
    n, h, w, cin = RANGE_SHAPE
    x = _inputs(RANGE_SHAPE)[0].clone()
    planted = []
    for (py, px) in ((0, 0), (0, w // 2), (h // 2, w // 2)):
        for c0 in (0, cin - 32):
            for k, v in enumerate(PLANT_VALUES):
                x[0, c0 + 5 + 7 * k, py, px] = v
                planted.append(v)
    return x, planted


@pytest.mark.gpu
@pytest.mark.parametrize('relu_in', [False, True])
def test_range_word_counts_each_planted_element_once_as_the_lds_kernel_does(monkeypatch, relu_in):
    _, wp, wu, bias, res = _inputs(RANGE_SHAPE)
    x, planted = _planted_input()
    expect = sum(1 for v in planted if not (relu_in and v < 0))
    assert expect == (18 if relu_in else 24)
    args = (x, wp, wu, bias, 'none', None, relu_in, False)
    new, bad_new = _call(monkeypatch, 'wreg', *args)
    old, bad_old = _call(monkeypatch, 'lds', *args)
    assert bad_old == expect, (bad_old, expect)
    assert bad_new == expect, (bad_new, expect)
    _assert_same(new, old, 'planted values, relu_in %s' % relu_in)


@pytest.mark.gpu
def test_without_a_range_word_nothing_is_counted_and_the_output_is_the_same(monkeypatch):
    from rmnet_amd import ops
    _, wp, wu, bias, res = _inputs(RANGE_SHAPE)
    x, _ = _planted_input()
    shared = ops.conv_range_word(dev())
    before = int(shared.item())
    args = (x, wp, wu, bias, 'none', None, False, False)
    new, word = _call(monkeypatch, 'wreg', *args, range_word=None)
    assert word is None
    old, _ = _call(monkeypatch, 'lds', *args)
    _assert_same(new, old, 'planted values, no range word')
    assert int(shared.item()) == before


# ================================================================================================ the switch
def test_the_variable_names_the_export_and_an_unknown_value_raises(monkeypatch):
    from rmnet_amd import ops
    assert ops.CONV3X3_ENTRIES == {'wreg': 'rmnet_conv3x3_split_f32', 'lds': 'rmnet_conv3x3_split_lds_f32'}
    assert ops.CONV3X3_KERNEL_DEFAULT in ops.CONV3X3_ENTRIES
    monkeypatch.delenv('RMNET_CONV3X3_KERNEL', raising=False)
    assert ops.conv3x3_entry() == ops.CONV3X3_ENTRIES[ops.CONV3X3_KERNEL_DEFAULT]
    for value, entry in ops.CONV3X3_ENTRIES.items():
        monkeypatch.setenv('RMNET_CONV3X3_KERNEL', value)
        assert ops.conv3x3_entry() == entry
    for value in ('', 'LDS', 'split', '0'):
        monkeypatch.setenv('RMNET_CONV3X3_KERNEL', value)
        with pytest.raises(RuntimeError, match='RMNET_CONV3X3_KERNEL'):
            ops.conv3x3_entry()


class _Spy(object):
    """The loaded library, recording the name of every export that is fetched from it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


@pytest.mark.gpu
def test_the_variable_reaches_the_export_it_names(monkeypatch):
    from rmnet_amd import _lib, ops
    x, wp, wu, bias, res = _inputs((2, 5, 7, 32))
    spy = _Spy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: spy)
    for value, entry in (('lds', 'rmnet_conv3x3_split_lds_f32'), ('wreg', 'rmnet_conv3x3_split_f32'), (None, None)):
        if value is None:
            monkeypatch.delenv('RMNET_CONV3X3_KERNEL')
            entry = ops.CONV3X3_ENTRIES[ops.CONV3X3_KERNEL_DEFAULT]
        else:
            monkeypatch.setenv('RMNET_CONV3X3_KERNEL', value)
        del spy.names[:]
        ops.conv3x3_split(x, wp, wu, bias)
        torch.cuda.synchronize()
        assert [n for n in spy.names if n.startswith('rmnet_conv3x3')] == [entry], (value, spy.names)
    monkeypatch.setenv('RMNET_CONV3X3_KERNEL', 'fast')
    del spy.names[:]
    with pytest.raises(RuntimeError, match='RMNET_CONV3X3_KERNEL'):
        ops.conv3x3_split(x, wp, wu, bias)
    assert not spy.names


# ================================================================================================ CPU: what the compiler gives
def test_the_new_kernel_gets_its_x_only_lds_and_the_old_one_keeps_its_own(tmp_path):
    """Compile-only, with tests/test_kernel_resources.py's compile step and metadata reader.  conv3x3_wreg declares two buffers of
    X hi / lo [128][K per barrier] fp16 and nothing else; no scratch, no spilled register, at most 256 VGPRs (one workgroup of
    eight waves per CU).  conv3x3_split is still in the file with its 98304 B."""
    import test_kernel_resources as KR
    found = KR._kernels(KR._compile('conv3x3.hip', str(tmp_path / 'conv3x3.s')))
    new = KR._one(found, '12conv3x3_wregE')
    print('conv3x3_wreg   LDS %6d  scratch %d  VGPRs %3d  spilled %d' % tuple(new[f] for f in KR.FIELDS))
    assert new['group_segment_fixed_size'] == 2 * 2 * 128 * K_PER_BARRIER * 2 == 32768
    assert new['private_segment_fixed_size'] == 0 and new['vgpr_spill_count'] == 0, new
    assert new['vgpr_count'] <= 256, new
    old = KR._one(found, '13conv3x3_splitE')
    assert old['group_segment_fixed_size'] == KR._double_buffer_bytes(128, 256) == 98304
    assert len(found) == 2, sorted(found)
