# -*- coding: utf-8 -*-
"""The split-fp16 convolutions' prefetch loop and epilogue (csrc/conv_split.hip, conv3x3.hip) at the smallest shapes at which
they can go wrong, bit for bit against the float64 convolution on integer inputs (why that is exact: tests/conv_ref.py, section 1):
  * K-step counts 1, 2, 3 (1x1, Cin 32 / 64 / 96) and 9, 18 (3x3, Cin 32 / 64) on every tile: with one step only the prologue and the
    step outside the loop run, odd and even counts end on different LDS buffers;
  * the epilogue, which reads every residual value before its first store, with M = 128 + 17 (rows of the last pixel tile beyond
    M), with and without a residual, in place (out is res), with ReLU, with two outputs -- sentinels behind the last valid row;
  * the range word: one out-of-window input is counted exactly once on every tile."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

SENT = 12345.0
KSTEPS = [(1, 32), (1, 64), (1, 96), (3, 32), (3, 64)]          # (ksize, Cin): 1, 2, 3, 9, 18 K steps
SMALL_MAPS = [(1, 5, 7), (1, 9, 15)]
BIG_MAPS = [(1, 128, 128), (1, 127, 129)]                       # 16384 pixels: exactly 512 workgroups; 16383: the last pixel tile partial
TILE_COUT = {'Narrow': 64, 'Mid': 128, 'Big': 1024}
# M = 5 x 29 = 128 + 17 pixels.  Big needs 512 workgroups: 2 pixel tiles x 256 slices of Cout = 65536
EPI_COUT = {'Narrow': 64, 'Mid': 128, 'Big': 65536}
EPI_SPLIT = {'Narrow': 32, 'Mid': 64, 'Big': 65536 - 4}
EPI_MAP = (1, 5, 29)
VARIANTS = ['res', 'out_is_res', 'res_relu', 'two_outputs', 'no_res']


def dev():
    return torch.device('cuda', 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nhwc(t):
    """[N, C, H, W] -> its NHWC memory as a flat tensor."""
    return t.permute(0, 2, 3, 1).contiguous().view(-1)


def _nchw(flat, n, c, h, w):
    return flat[:n * h * w * c].view(n, h, w, c).permute(0, 3, 1, 2)


def _assert_equal(got, want64, what):
    want = want64.float()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index, got, want): %s' % (what, bad.shape[0], got.numel(), first))


def _inputs(n, cin, cout, h, w, k, with_scale=True):
    seed = cin + cout + 7 * h + w + k
    x = R.int_acts((n, cin, h, w), seed).to(dev())
    wt = R.int_weights(cout, cin, k, seed + 1).to(dev())
    bn = R.pow2_scale(cout).to(dev()) if with_scale else torch.ones(cout, device=dev())
    shift = R.int_acts((cout,), seed + 2, -20, 20).to(dev())
    res = R.int_acts((n, cout, h, w), seed + 3, -50, 50).to(dev())
    return x, wt, bn, shift, res


def _want(x, wt, bn, shift, res, k, relu_out=False):
    t = F.conv2d(x.double(), wt.double() * bn.double().view(-1, 1, 1, 1), None, 1, k // 2) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        t = t + res.double()
    return F.relu(t) if relu_out else t


def _run(kernel, x, wp, wu, shift, variant, res, cout, split=None):
    """One raw launch with every output in a buffer as long as the last pixel tile, sentinels behind row M.  Returns (got [N, Cout,
    H, W], the words behind the last valid row of every output buffer)."""
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    n, cin, h, w = x.shape
    m = n * h * w
    rows = (m + 127) // 128 * 128
    xb = _nhwc(x)
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    flags = ops.CONV_RELU_OUT if variant == 'res_relu' else 0
    widths = [cout] if variant != 'two_outputs' else [split, cout - split]
    outs = [torch.full((rows * c,), SENT, device=dev()) for c in widths]
    resb = None
    if variant in ('res', 'res_relu'):
        resb = _nhwc(res)
    elif variant == 'out_is_res':
        outs[0][:m * cout] = _nhwc(res)
        resb = outs[0]
    if kernel == 'conv3x3':
        rc = lib.rmnet_conv3x3_split_f32(_p(xb), _p(wp), _p(wu), _p(shift), _p(resb), flags, n, h, w, cin, _p(outs[0]), _p(rw), None)
    else:
        k = {cin * cout * 2: 1, 9 * cin * cout * 2: 3}[wp.numel()]
        rc = lib.rmnet_conv_split_f32(_p(xb), _p(wp), _p(wu), _p(shift), _p(resb), flags, n, h, w, cin, cout, k, 1, _p(outs[0]),
                                      _p(outs[1]) if len(outs) > 1 else None, split or 0, _p(rw), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = torch.cat([_nchw(o, n, c, h, w) for o, c in zip(outs, widths)], dim=1)
    tails = torch.cat([o[m * c:] for o, c in zip(outs, widths)])
    return got, tails, int(rw.item())


# ================================================================================================ K-step counts
def _ksteps_split(tile, n, h, w, k, cin):
    from rmnet_amd import ops
    cout = TILE_COUT[tile]
    assert R.tile_of(n, cout, h, w, k, 1) == tile
    x, wt, bn, shift, res = _inputs(n, cin, cout, h, w, k)
    wp, wu = ops.conv_split_pack(wt, bn)
    got, tails, bad = _run('conv_split', x, wp, wu, shift, 'res', res, cout)
    assert bad == 0 and bool((tails == SENT).all())
    _assert_equal(got, _want(x, wt, bn, shift, res, k), 'conv_split %s %s %dx%d Cin %d' % (tile, (n, h, w), k, k, cin))


@pytest.mark.gpu
@pytest.mark.parametrize('k,cin', KSTEPS)
@pytest.mark.parametrize('n,h,w', SMALL_MAPS)
@pytest.mark.parametrize('tile', ['Narrow', 'Mid'])
def test_conv_split_small_tiles_every_k_step_count_bit_for_bit(tile, n, h, w, k, cin):
    _ksteps_split(tile, n, h, w, k, cin)


@pytest.mark.gpu
@pytest.mark.parametrize('k,cin', KSTEPS)
@pytest.mark.parametrize('n,h,w', BIG_MAPS)
def test_conv_split_big_tile_every_k_step_count_bit_for_bit(n, h, w, k, cin):
    _ksteps_split('Big', n, h, w, k, cin)


@pytest.mark.gpu
@pytest.mark.parametrize('cin', [32, 64])
@pytest.mark.parametrize('n,h,w', [(1, 5, 7), (2, 9, 15)])       # 270 pixels: the third pixel tile is partial
def test_conv3x3_split_9_and_18_k_steps_bit_for_bit(n, h, w, cin):
    from rmnet_amd import ops
    x, wt, bn, bias, res = _inputs(n, cin, 256, h, w, 3, with_scale=False)
    wp, wu = ops.conv3x3_pack(wt)
    got, tails, bad = _run('conv3x3', x, wp, wu, bias, 'res', res, 256)
    assert bad == 0 and bool((tails == SENT).all())
    _assert_equal(got, _want(x, wt, bn, bias, res, 3), 'conv3x3_split %s Cin %d' % ((n, h, w), cin))


# ================================================================================================ the epilogue
def _epilogue_case(kernel, cout, split, variant):
    from rmnet_amd import ops
    n, h, w = EPI_MAP
    assert n * h * w == 128 + 17
    k = 3 if kernel == 'conv3x3' else 1
    x, wt, bn, shift, res = _inputs(n, 32, cout, h, w, k, with_scale=kernel != 'conv3x3')
    wp, wu = ops.conv3x3_pack(wt) if kernel == 'conv3x3' else ops.conv_split_pack(wt, bn)
    got, tails, bad = _run(kernel, x, wp, wu, shift, variant, res, cout, split)
    what = '%s Cout %d %s' % (kernel, cout, variant)
    assert bad == 0, what
    assert bool((tails == SENT).all()), '%s: %d words behind row M were written' % (what, int((tails != SENT).sum()))
    with_res = variant in ('res', 'out_is_res', 'res_relu')
    _assert_equal(got, _want(x, wt, bn, shift, res if with_res else None, k, relu_out=variant == 'res_relu'), what)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('tile', ['Narrow', 'Mid', 'Big'])
def test_conv_split_epilogue_variants_with_rows_beyond_m(tile, variant):
    n, h, w = EPI_MAP
    assert R.tile_of(n, EPI_COUT[tile], h, w, 1, 1) == tile
    _epilogue_case('conv_split', EPI_COUT[tile], EPI_SPLIT[tile], variant)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', [v for v in VARIANTS if v != 'two_outputs'])
def test_conv3x3_split_epilogue_variants_with_rows_beyond_m(variant):
    _epilogue_case('conv3x3', 256, None, variant)


# ================================================================================================ the range word
@pytest.mark.gpu
@pytest.mark.parametrize('kernel,cout,k', [('conv_split', 64, 1), ('conv_split', 128, 3), ('conv_split', 65536, 1), ('conv3x3', 256, 3)])
def test_one_out_of_window_input_is_counted_exactly_once(kernel, cout, k):
    """One activation of 2000 (the window ends at 1023.5) at pixel (2, 11), channel 5: the range word is 1 on every tile -- Big's 256
    Cout slices count it in one, a 3x3 kernel at its centre tap only -- and every output that does not read it is still exact."""
    from rmnet_amd import ops
    n, h, w = EPI_MAP
    if kernel == 'conv_split':
        assert R.tile_of(n, cout, h, w, k, 1) == {64: 'Narrow', 128: 'Mid', 65536: 'Big'}[cout]
    x, wt, bn, shift, res = _inputs(n, 32, cout, h, w, k, with_scale=kernel != 'conv3x3')
    x[0, 5, 2, 11] = 2000.0
    wp, wu = ops.conv3x3_pack(wt) if kernel == 'conv3x3' else ops.conv_split_pack(wt, bn)
    got, tails, bad = _run(kernel, x, wp, wu, shift, 'res', res, cout)
    assert bad == 1, bad
    assert bool((tails == SENT).all())
    want = _want(x, wt, bn, shift, res, k).float()
    r = k // 2
    clean = torch.ones(h, w, dtype=torch.bool, device=dev())
    clean[2 - r:2 + r + 1, 11 - r:11 + r + 1] = False
    assert torch.equal(got[:, :, clean], want[:, :, clean])
