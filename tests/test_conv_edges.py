# -*- coding: utf-8 -*-
"""Edge-shape, bit-exact and per-element tests of the four HIP convolutions (csrc/conv_split.hip, conv3x3.hip, stem.hip,
pred_head.hip), next to the whole-tensor accuracy tests of test_conv_split.py / test_conv3x3_split.py / test_stem_head.py:
  1. integer inputs that every kernel must return bit for bit (indexing, borders, partial tiles, tile choice, epilogues, splits);
  2. the three-term arithmetic restated in float64 and a derived error bound asserted for EVERY output element;
  3. the argument checks of the C entries, with a sentinel in the output buffers.
The arithmetic, the exactness argument and the derivation of the bounds are in tests/conv_ref.py."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R


def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _rw():
    return torch.zeros(1, dtype=torch.int32, device=dev())


def _assert_equal(got, want64, what):
    """torch.equal on the fp32 cast of the float64 reference; on a mismatch, says how many elements differ and where the first are."""
    want = want64.float()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index, got, want): %s' % (what, bad.shape[0], got.numel(), first))


def _assert_within(got, ref, bound, what):
    """|got - ref| <= bound for every element (a NaN fails); returns the largest error / bound."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        first = [(tuple(int(v) for v in i), float(err[tuple(i)]), float(bound[tuple(i)])) for i in bad[:4]]
        pytest.fail('%s: %d of %d elements outside the bound, largest error / bound %.3g; first (index, error, bound): %s'
                    % (what, bad.shape[0], err.numel(), ratio, first))
    return ratio


# ================================================================================================ CPU: the premises
@pytest.mark.parametrize('cout,cin,k', [(64, 32, 1), (128, 64, 3), (640, 96, 3), (1024, 64, 1)])
def test_the_integer_packs_have_an_all_zero_lo_plane(cout, cin, k):
    """conv_split_pack of the part-1 weights: lo plane zero, hi * unscale is w * bn_scale exactly, and the channels with maxima
    8 / 3 / 5 take three different scales (2^11 / 2^13 / 2^12), the all-zero channel none."""
    from rmnet_amd import ops
    w, bn = R.int_weights(cout, cin, k, seed=cout + k), R.pow2_scale(cout)
    assert [float(w[c].abs().max()) for c in range(4)] == [8.0, 0.0, 3.0, 5.0] and float(w.abs().max()) == 8.0
    wp, wu = ops.conv_split_pack(w, bn)
    wh, wl = R.unpack_conv(wp, cout, cin, k)
    assert float(wl.abs().max()) == 0.0
    assert torch.equal(wh * wu.double().view(-1, 1, 1, 1), w.double() * bn.double().view(-1, 1, 1, 1))
    assert torch.equal(R.unpack_conv_weights(wp, wu, cout, cin, k), w.double() * bn.double().view(-1, 1, 1, 1))
    scale = (bn.double() / wu.double())[:4]
    assert scale.tolist() == [2.0 ** 11, bn[1].item(), 2.0 ** 13, 2.0 ** 12]
    if cout == 640:                         # the decoder's and the stems' packers on the same kind of weights
        w3 = R.int_weights(256, cin, 3, seed=5)
        wp3, wu3 = ops.conv3x3_pack(w3)
        wh3, wl3 = R.unpack_conv(wp3, 256, cin, 3)
        assert float(wl3.abs().max()) == 0.0 and torch.equal(wh3 * wu3.double().view(-1, 1, 1, 1), w3.double())
        for c7 in (3, 5):
            w7, bn7 = R.int_weights(64, c7, 7, seed=c7), R.pow2_scale(64)
            wp7, wu7 = ops.stem_pack(w7, bn7)
            wh7, wl7, pad7 = R.unpack_stem(wp7, c7)
            assert float(wl7.abs().max()) == 0.0 and float(pad7.abs().max()) == 0.0
            assert torch.equal(wh7 * wu7.double().view(-1, 1, 1, 1), w7.double() * bn7.double().view(-1, 1, 1, 1))


def test_integer_activations_split_into_an_exact_hi_and_a_zero_lo():
    x = torch.arange(-15, 16).float().view(1, 31, 1, 1)
    h, l = R.split_act(x)
    assert torch.equal(h, x.double() * 64) and float(l.abs().max()) == 0.0
    h, l = R.split_act(x, relu=True)
    assert torch.equal(h, F.relu(x).double() * 64)


@pytest.mark.parametrize('cin', [32, 64])
def test_the_bound_catches_a_missing_term(cin):
    """The restatement alone, 1x1, K = Cin: with either cross term dropped (at 1x1, Wl dropped for a tap is h*Wl dropped), or l
    zeroed for the last 4 channels of a 32-channel block, T leaves the per-element bound in most elements (measured: 97 / 97 / 87 %
    at K = 32, 91 / 92 / 59 % at K = 64).  With 3x3 kernels the bound grows as K^2 and the faults as sqrt(K): see the next test
    for what the bound still does there, and the lo-exact cases below for what checks a single tap's lo plane."""
    from rmnet_amd import ops
    x = torch.randn(2, cin, 13, 20, generator=torch.Generator().manual_seed(1))
    w = R.uniform_weights(64, cin, 1, seed=3)
    wp, wu = ops.conv_split_pack(w)
    wh, wl = R.unpack_conv(wp, 64, cin, 1)
    h, l = R.split_act(x)
    t, a = R.restate(h, l, wh, wl, wu, 1, 0)
    bound = R.kernel_bound(cin, a, t)
    assert float((t - F.conv2d(x.double(), w.double())).abs().max()) <= float(R.repr_bound(x, w, 1, 0).max())
    l4 = l.clone()
    l4[:, 28:32] = 0.0
    for name, kw in (('h*Wl dropped', dict(hwl=False)), ('l*Wh dropped', dict(lwh=False)), ('l zeroed for 4 channels', dict(lwh=(l4, wh)))):
        tm, _ = R.restate(h, l, wh, wl, wu, 1, 0, **kw)
        frac = float(((tm - t).abs() > bound).double().mean())
        print('K %d, %s: outside the bound in %.0f %% of the elements' % (cin, name, 100 * frac))
        assert frac > 0.5, (name, frac)


P2_SMALL = [(2, 32, 64, 13, 20), (2, 64, 128, 12, 19)]


@pytest.mark.parametrize('kind', R.INPUTS)
@pytest.mark.parametrize('k,s', [(1, 1), (1, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize('n,cin,cout,h,w', P2_SMALL)
def test_a_kernel_without_a_cross_term_fails_the_every_element_check(n, cin, cout, h, w, k, s, kind):
    """The two small part-2 cases of conv_split with the restatement minus l*Wh standing in for the kernel: at 3x3 (K = 288, 576) the
    fault is inside the bound in most elements, but every element is asserted and some always leave, so each of these 32 cases would
    fail.  (A fault in ONE tap or K block at K = 576 can stay inside the bound everywhere: that is the lo-exact cases' job.)"""
    from rmnet_amd import ops
    seed = cin + cout + k + s
    x, wt = R.make_inputs(kind, (n, cin, h, w), R.uniform_weights(cout, cin, k, seed), seed + 1)
    wp, wu = ops.conv_split_pack(wt)
    wh, wl = R.unpack_conv(wp, cout, cin, k)
    hx, lx = R.split_act(x)
    t, a = R.restate(hx, lx, wh, wl, wu, s, k // 2)
    bad, _ = R.restate(hx, lx, wh, wl, wu, s, k // 2, lwh=False)
    outside = (bad - t).abs() > R.kernel_bound(k * k * cin, a, t)
    assert bool(outside.any()), float(outside.double().mean())


@pytest.mark.parametrize('cin,k', [(32, 1), (64, 3), (256, 3)])
def test_the_lo_exact_prediction_stands_on_exact_halves_and_sees_one_tap(cin, k):
    """Section 1b of conv_ref on the CPU: the activations split into h = 64 a and l = b / 256, the pack into Wh = p 2^11 and
    Wl = q / 4, all exact; both accumulators' absolute sums stay below 2^24 of their units; and the prediction changes in most
    elements when Wl is zeroed in one tap, or l in the last 4 channels of one 32-channel block -- faults the bound cannot see at
    K = 576 and 2304."""
    from rmnet_amd import ops
    x = R.lo_acts((2, cin, 7, 9), seed=cin)
    w = R.lo_weights(128, cin, k, seed=cin + 1)
    a = torch.round(x)
    p = torch.round(w)
    wp, wu = ops.conv_split_pack(w)
    wh, wl = R.unpack_conv(wp, 128, cin, k)
    h, l = R.split_act(x)
    assert bool((wu == 2.0 ** -11).all())
    assert torch.equal(h, a.double() * 64) and torch.equal(l, (x.double() - a.double()) * 64) and float(l.abs().max()) == 3 / 256
    assert torch.equal(wh, p.double() * 2 ** 11) and torch.equal(wl, (w.double() - p.double()) * 2 ** 11) and float(wl.abs().max()) == 0.25
    conv = lambda u, v: F.conv2d(u, v, None, 1, k // 2)
    assert float(conv(h.abs(), wh.abs()).max()) / 2 ** 17 < 2 ** 24
    assert float((conv(h.abs(), wl.abs()) + conv(l.abs(), wh.abs())).max()) < 2 ** 24
    want = R.predict(h, l, wh, wl, wu, 1, k // 2)
    wl_tap = wl.clone()
    wl_tap[:, :, k // 2, k // 2] = 0.0
    l4 = l.clone()
    l4[:, 28:32] = 0.0
    for name, other in (('Wl zeroed in the centre tap', R.predict(h, l, wh, wl_tap, wu, 1, k // 2)),
                        ('l zeroed for 4 channels', R.predict(h, l4, wh, wl, wu, 1, k // 2))):
        frac = float((other != want).double().mean())
        print('Cin %d %dx%d, %s: the prediction changes in %.0f %% of the elements' % (cin, k, k, name, 100 * frac))
        assert frac > 0.5, (name, frac)


# ================================================================================================ 1. bit-exact integer cases
KS = [(1, 1), (1, 2), (3, 1), (3, 2)]
# (N, Cin, Cout, H, W), run at every (k, stride) of KS.  Tile of each (shape, stride), asserted by test_the_cases_land_on_the_tiles_...:
SPLIT_SHAPES = [(1, 32, 64, 5, 7),                                              # Narrow: one partial tile
                (3, 64, 128, 13, 20), (3, 64, 128, 12, 19),                    # Mid: M no multiple of 128, images straddle tiles
                (2, 32, 128, 1, 1), (2, 32, 128, 1, 9), (2, 32, 128, 9, 1),    # Mid: degenerate maps
                (1, 96, 640, 9, 11),                                            # Mid: five Cout slices
                (1, 64, 1024, 128, 128),                                        # stride 1: M = 16384, exactly 512 workgroups -> Big;
                                                                                # stride 2: M = 4096 -> Mid
                (1, 64, 1024, 128, 127)]                                        # stride 1: 508 workgroups -> Mid (and Mid at stride 2)
# the Big tile at stride 2 needs M >= 16384 behind the stride: N = 4 (stride 2 only; at stride 1 it would be a 268 MB output)
BIG_S2 = (4, 64, 1024, 128, 128)
SPLIT_CASES = [sh + ks for sh in SPLIT_SHAPES for ks in KS] + [BIG_S2 + (1, 2), BIG_S2 + (3, 2)]
P2_CASES = [sh + ks for sh in P2_SMALL + [(1, 64, 1024, 128, 128)] for ks in KS] + [BIG_S2 + (1, 2), BIG_S2 + (3, 2)]


def test_the_cases_land_on_the_tiles_the_comments_name():
    """The host's tile rule restated (conv_ref.tile_of): Big runs 1x1 and 3x3 at stride 1 AND at stride 2, in the bit-exact and in
    the per-element cases; the 128 x 127 map is the Mid side of the same decision."""
    big = {c for c in SPLIT_CASES if R.tile_of(c[0], c[2], c[3], c[4], c[5], c[6]) == 'Big'}
    assert big == {(1, 64, 1024, 128, 128, 1, 1), (1, 64, 1024, 128, 128, 3, 1), BIG_S2 + (1, 2), BIG_S2 + (3, 2)}
    assert {c for c in P2_CASES if R.tile_of(c[0], c[2], c[3], c[4], c[5], c[6]) == 'Big'} == big
    assert all(R.tile_of(1, 1024, 128, 127, k, s) == 'Mid' for k, s in KS)
    assert all(R.tile_of(1, 1024, 128, 128, k, 2) == 'Mid' for k in (1, 3))
    assert {R.tile_of(c[0], c[2], c[3], c[4], c[5], c[6]) for c in SPLIT_CASES if c[2] == 64} == {'Narrow'}
    assert {R.tile_of(c[0], c[2], c[3], c[4], c[5], c[6]) for c in SPLIT_CASES if c[2] in (128, 640)} == {'Mid'}


def _split_exact(n, cin, cout, h, w, k, s, relu_in=False, relu_out=False, use_shift=True, use_res=True, inplace=False, split=None):
    """One integer case of conv_split: (got, float64 reference)."""
    from rmnet_amd import ops
    seed = cin + cout + 7 * h + w + k + s
    x = R.int_acts((n, cin, h, w), seed).to(dev())
    wt, bn = R.int_weights(cout, cin, k, seed + 1).to(dev()), R.pow2_scale(cout).to(dev())
    ho, wo = R.out_hw(h, w, k, s)
    shift = R.int_acts((cout,), seed + 2, -20, 20).to(dev()) if use_shift else None
    res = R.int_acts((n, cout, ho, wo), seed + 3, -50, 50).to(dev()) if use_res else None
    want = F.conv2d((F.relu(x) if relu_in else x).double(), wt.double() * bn.double().view(-1, 1, 1, 1), None, s, k // 2)
    if use_shift:
        want = want + shift.double().view(1, -1, 1, 1)
    if use_res:
        want = want + res.double()
    if relu_out:
        want = F.relu(want)
    wp, wu = ops.conv_split_pack(wt, bn)
    rw = _rw()
    rg = _cl(res) if use_res else None
    out = rg.clone() if inplace else None
    got = ops.conv_split(_cl(x), wp, wu, shift, out if inplace else rg, ksize=k, stride=s, relu_in=relu_in, relu_out=relu_out, out=out,
                         range_word=rw, split=split)
    if inplace:
        assert got.data_ptr() == out.data_ptr()
    assert int(rw.item()) == 0
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cout,h,w,k,s', SPLIT_CASES)
def test_conv_split_returns_integer_cases_bit_for_bit(n, cin, cout, h, w, k, s):
    got, want = _split_exact(n, cin, cout, h, w, k, s)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _assert_equal(got, want, 'conv_split %s %dx%d/s%d' % ((n, cin, cout, h, w), k, k, s))


EPILOGUES = {'relu_in': dict(relu_in=True), 'relu_out': dict(relu_out=True), 'relu_both': dict(relu_in=True, relu_out=True),
             'shift_only': dict(use_res=False), 'res_only': dict(use_shift=False), 'neither': dict(use_shift=False, use_res=False),
             'out_is_res': dict(inplace=True, relu_out=True)}


@pytest.mark.gpu
@pytest.mark.parametrize('k,s', [(1, 1), (3, 2)])
@pytest.mark.parametrize('name', sorted(EPILOGUES))
def test_conv_split_epilogues_bit_for_bit(name, k, s):
    got, want = _split_exact(2, 64, 128, 13, 20, k, s, **EPILOGUES[name])
    _assert_equal(got, want, 'conv_split %s %dx%d/s%d' % (name, k, k, s))


@pytest.mark.gpu
@pytest.mark.parametrize('k,s', [(1, 1), (3, 2)])
@pytest.mark.parametrize('shape,split', [((2, 64, 128, 13, 20), c) for c in (4, 60, 64, 124)]
                         + [((1, 96, 640, 9, 11), c) for c in (128, 132, 636)])
def test_conv_split_two_outputs_equal_the_unsplit_launch(shape, split, k, s):
    """``split`` inside a lane group's tile, inside a wave's, on and off a workgroup tile's edge: the two outputs, each
    channels-last with its own channel count, concatenated equal the unsplit launch (and the float64 reference) bit for bit."""
    n, cin, cout, h, w = shape
    whole, want = _split_exact(n, cin, cout, h, w, k, s, use_res=False)
    (a, b), _ = _split_exact(n, cin, cout, h, w, k, s, use_res=False, split=split)
    ho, wo = R.out_hw(h, w, k, s)
    assert a.shape == (n, split, ho, wo) and b.shape == (n, cout - split, ho, wo)
    assert a.is_contiguous(memory_format=torch.channels_last) and b.is_contiguous(memory_format=torch.channels_last)
    assert a.stride(1) == 1 and b.stride(1) == 1 and a.stride(3) == split and b.stride(3) == cout - split
    assert torch.equal(torch.cat((a, b), dim=1), whole)
    _assert_equal(whole, want, 'conv_split unsplit %s' % (shape,))


def _c3_exact(n, cin, h, w, relu_in=False, relu_out=False, use_bias=True, use_res=True, inplace=False):
    from rmnet_amd import ops
    seed = cin + 7 * h + w
    x = R.int_acts((n, cin, h, w), seed).to(dev())
    wt = R.int_weights(256, cin, 3, seed + 1).to(dev())
    bias = R.int_acts((256,), seed + 2, -20, 20).to(dev()) if use_bias else None
    res = R.int_acts((n, 256, h, w), seed + 3, -50, 50).to(dev()) if use_res else None
    want = F.conv2d((F.relu(x) if relu_in else x).double(), wt.double(), bias.double() if use_bias else None, 1, 1)
    if use_res:
        want = want + res.double()
    if relu_out:
        want = F.relu(want)
    wp, wu = ops.conv3x3_pack(wt)
    rw = _rw()
    rg = _cl(res) if use_res else None
    out = rg.clone() if inplace else None
    got = ops.conv3x3_split(_cl(x), wp, wu, bias, out if inplace else rg, relu_in=relu_in, relu_out=relu_out, out=out, range_word=rw)
    if inplace:
        assert got.data_ptr() == out.data_ptr()
    assert int(rw.item()) == 0
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,h,w', [(1, 32, 1, 1), (2, 64, 7, 9), (3, 256, 13, 20), (1, 1024, 9, 11)])
def test_conv3x3_split_returns_integer_cases_bit_for_bit(n, cin, h, w):
    got, want = _c3_exact(n, cin, h, w)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _assert_equal(got, want, 'conv3x3_split %s' % ((n, cin, h, w),))


@pytest.mark.gpu
@pytest.mark.parametrize('flags', list(range(16)) + ['out_is_res'])
def test_conv3x3_split_prologue_and_epilogue_flags_bit_for_bit(flags):
    kw = dict(inplace=True, relu_in=True) if flags == 'out_is_res' else \
        dict(relu_in=bool(flags & 1), relu_out=bool(flags & 2), use_bias=bool(flags & 4), use_res=bool(flags & 8))
    got, want = _c3_exact(2, 64, 7, 9, **kw)
    _assert_equal(got, want, 'conv3x3_split 7x9 %s' % (kw,))


def _stem_inputs(cin, x):
    frame = x[:, :3].contiguous()
    mask = x[:, 3].contiguous() if cin == 5 else None
    other = x[:, 4].contiguous() if cin == 5 else None
    return frame, mask, other


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['cin3', 'cin5', 'cin5_no_other'])
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (2, 5, 7), (2, 33, 31), (1, 34, 66), (2, 70, 130)])
def test_stem_split_returns_integer_cases_bit_for_bit(n, h, w, case):
    """Convolution, folded scale, shift, ReLU and the 3x3 / stride-2 max-pool, on maps on both sides of the 32-pixel core
    boundaries and with odd and even pooled sizes."""
    from rmnet_amd import ops
    cin = 3 if case == 'cin3' else 5
    seed = cin + 7 * h + w
    x = R.int_acts((n, cin, h, w), seed)
    if cin == 5:
        x[:, 3:] = R.int_acts((n, 2, h, w), seed + 4, 0, 1)
        if case == 'cin5_no_other':
            x[:, 4] = 0.0
    x = x.to(dev())
    wt, bn = R.int_weights(64, cin, 7, seed + 1).to(dev()), R.pow2_scale(64).to(dev())
    shift = R.int_acts((64,), seed + 2, -20, 20).to(dev())
    want = R.pool(F.relu(F.conv2d(x.double(), wt.double() * bn.double().view(-1, 1, 1, 1), None, 2, 3) + shift.double().view(1, -1, 1, 1)))
    wp, wu = ops.stem_pack(wt, bn)
    frame, mask, other = _stem_inputs(cin, x)
    rw = _rw()
    got = ops.stem_split(frame, mask, None if case == 'cin5_no_other' else other, wp, wu, shift, range_word=rw)
    assert int(rw.item()) == 0
    assert got.is_contiguous(memory_format=torch.channels_last)
    _assert_equal(got, want, 'stem_split %s %s' % (case, (n, h, w)))


HEAD_SHAPES = [(1, 1, 1), (3, 7, 9), (2, 33, 61)]


@pytest.mark.gpu
@pytest.mark.parametrize('c', [32, 64, 256])
@pytest.mark.parametrize('n,h,w', HEAD_SHAPES)
def test_pred_head_returns_integer_cases_bit_for_bit(n, h, w, c):
    from rmnet_amd import ops
    seed = c + 7 * h + w
    x = R.int_acts((n, c, h, w), seed).to(dev())
    wt = R.int_acts((2, c, 3, 3), seed + 1, -8, 8).to(dev())
    b = torch.tensor([7.0, -3.0], device=dev())
    want = F.conv2d(F.relu(x).double(), wt.double(), b.double(), 1, 1)
    got = ops.pred_head(_cl(x), wt, b)
    assert got.is_contiguous()
    _assert_equal(got, want, 'pred_head %s' % ((n, c, h, w),))


# ------------------------------------------------------------------------------------------------ 1b. non-zero lo planes, exact
@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,cout,h,w,k,s', [(1, 32, 64, 5, 7, 1, 1), (1, 32, 64, 5, 7, 3, 2)]
                         + [(2, 64, 128, 13, 20) + ks for ks in KS] + [(1, 64, 1024, 128, 128, 3, 1), BIG_S2 + (3, 2)])
def test_conv_split_returns_lo_exact_cases_bit_for_bit(n, cin, cout, h, w, k, s):
    """Activations and weights whose hi and lo halves are both exact and non-zero (conv_ref section 1b): every tap's h*Wl and l*Wh
    are live and the kernel must return the predicted roundings bit for bit, on every tile."""
    from rmnet_amd import ops
    seed = cin + cout + h + k + s
    x = R.lo_acts((n, cin, h, w), seed).to(dev())
    wt = R.lo_weights(cout, cin, k, seed + 1).to(dev())
    ho, wo = R.out_hw(h, w, k, s)
    shift = R.int_acts((cout,), seed + 2, -20, 20).to(dev())
    res = R.int_acts((n, cout, ho, wo), seed + 3, -50, 50).to(dev())
    wp, wu = ops.conv_split_pack(wt)
    wh, wl = R.unpack_conv(wp, cout, cin, k)
    hx, lx = R.split_act(x)
    assert float(lx.abs().max()) == 3 / 256 and float(wl.abs().max()) == 0.25
    want = R.predict(hx, lx, wh, wl, wu, s, k // 2, shift, res)
    rw = _rw()
    got = ops.conv_split(_cl(x), wp, wu, shift, _cl(res), ksize=k, stride=s, range_word=rw)
    assert int(rw.item()) == 0
    _assert_equal(got, want, 'conv_split lo-exact %s %dx%d/s%d' % ((n, cin, cout, h, w), k, k, s))


@pytest.mark.gpu
@pytest.mark.parametrize('n,cin,h,w', [(2, 64, 7, 9), (3, 256, 13, 20)])
def test_conv3x3_split_returns_lo_exact_cases_bit_for_bit(n, cin, h, w):
    from rmnet_amd import ops
    seed = cin + h
    x = R.lo_acts((n, cin, h, w), seed).to(dev())
    wt = R.lo_weights(256, cin, 3, seed + 1).to(dev())
    bias = R.int_acts((256,), seed + 2, -20, 20).to(dev())
    res = R.int_acts((n, 256, h, w), seed + 3, -50, 50).to(dev())
    wp, wu = ops.conv3x3_pack(wt)
    wh, wl = R.unpack_conv(wp, 256, cin, 3)
    hx, lx = R.split_act(x)
    assert float(lx.abs().max()) == 3 / 256 and float(wl.abs().max()) == 0.25
    want = R.predict(hx, lx, wh, wl, wu, 1, 1, bias, res)
    rw = _rw()
    got = ops.conv3x3_split(_cl(x), wp, wu, bias, _cl(res), range_word=rw)
    assert int(rw.item()) == 0
    _assert_equal(got, want, 'conv3x3_split lo-exact %s' % ((n, cin, h, w),))


@pytest.mark.gpu
@pytest.mark.parametrize('cin', [3, 5])
def test_stem_split_returns_lo_exact_cases_bit_for_bit(cin):
    from rmnet_amd import ops
    n, h, w = 2, 33, 31
    x = R.lo_acts((n, cin, h, w), cin).to(dev())
    wt = R.lo_weights(64, cin, 7, cin + 1).to(dev())
    shift = R.int_acts((64,), cin + 2, -20, 20).to(dev())
    wp, wu = ops.stem_pack(wt)
    wh, wl, _ = R.unpack_stem(wp, cin)
    hx, lx = R.split_act(x)
    assert float(lx.abs().max()) == 3 / 256 and float(wl.abs().max()) == 0.25
    want = R.pool(R.predict(hx, lx, wh, wl, wu, 2, 3, shift, relu_out=True))
    frame, mask, other = _stem_inputs(cin, x)
    rw = _rw()
    got = ops.stem_split(frame, mask, other, wp, wu, shift, range_word=rw)
    assert int(rw.item()) == 0
    _assert_equal(got, want, 'stem_split lo-exact cin %d' % cin)


# ================================================================================================ 2. per-element bounds
def _epilogue_terms(cout, out_shape, scale, seed):
    g = torch.Generator().manual_seed(seed)
    bn = (torch.rand(cout, generator=g) * 0.4 + 0.8).float()
    shift = ((torch.rand(cout, generator=g) * 2 - 1) * 0.05).float()
    res = torch.randn(out_shape, generator=g) * scale
    return bn.to(dev()), shift.to(dev()), res.to(dev())


def _kind_scale(kind):
    return 1.0 if kind == 'mixed' else float(kind)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', R.INPUTS)
@pytest.mark.parametrize('n,cin,cout,h,w,k,s', P2_CASES)
def test_conv_split_every_element_within_the_derived_bound(n, cin, cout, h, w, k, s, kind):
    """Folded scale, shift and residual: every output element within the summation bound of the float64 three-term restatement,
    and within that plus the representation term of the true float64 convolution."""
    from rmnet_amd import ops
    seed = cin + cout + k + s
    x, wt = R.make_inputs(kind, (n, cin, h, w), R.uniform_weights(cout, cin, k, seed), seed + 1)
    x, wt = x.to(dev()), wt.to(dev())
    ho, wo = R.out_hw(h, w, k, s)
    bn, shift, res = _epilogue_terms(cout, (n, cout, ho, wo), _kind_scale(kind), seed + 2)
    wp, wu = ops.conv_split_pack(wt, bn)
    rw = _rw()
    got = ops.conv_split(_cl(x), wp, wu, shift, _cl(res), ksize=k, stride=s, range_word=rw)
    assert int(rw.item()) == 0
    wh, wl = R.unpack_conv(wp, cout, cin, k)
    hx, lx = R.split_act(x)
    t, a = R.restate(hx, lx, wh, wl, wu, s, k // 2, shift, res)
    bound = R.kernel_bound(k * k * cin, a, t, shift, res)
    what = 'conv_split %s %dx%d/s%d %s' % ((n, cin, cout, h, w), k, k, s, kind)
    r1 = _assert_within(got, t, bound, what + ' against the restatement')
    w64 = wt.double() * bn.double().view(-1, 1, 1, 1)
    true = F.conv2d(x.double(), w64, None, s, k // 2) + shift.double().view(1, -1, 1, 1) + res.double()
    r2 = _assert_within(got, true, bound + R.repr_bound(x, w64, s, k // 2), what + ' against float64')
    print('EDGE %s: error / bound %.3f (restatement) %.3f (float64)' % (what, r1, r2))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', R.INPUTS)
@pytest.mark.parametrize('n,cin,h,w', [(2, 32, 7, 9), (2, 64, 13, 20)])
def test_conv3x3_split_every_element_within_the_derived_bound(n, cin, h, w, kind):
    from rmnet_amd import ops
    seed = cin + h
    x, wt = R.make_inputs(kind, (n, cin, h, w), R.uniform_weights(256, cin, 3, seed), seed + 1)
    x, wt = x.to(dev()), wt.to(dev())
    _, bias, res = _epilogue_terms(256, (n, 256, h, w), _kind_scale(kind), seed + 2)
    wp, wu = ops.conv3x3_pack(wt)
    rw = _rw()
    got = ops.conv3x3_split(_cl(x), wp, wu, bias, _cl(res), range_word=rw)
    assert int(rw.item()) == 0
    wh, wl = R.unpack_conv(wp, 256, cin, 3)
    hx, lx = R.split_act(x)
    t, a = R.restate(hx, lx, wh, wl, wu, 1, 1, bias, res)
    bound = R.kernel_bound(9 * cin, a, t, bias, res)
    what = 'conv3x3_split %s %s' % ((n, cin, h, w), kind)
    r1 = _assert_within(got, t, bound, what + ' against the restatement')
    true = F.conv2d(x.double(), wt.double(), bias.double(), 1, 1) + res.double()
    r2 = _assert_within(got, true, bound + R.repr_bound(x, wt, 1, 1), what + ' against float64')
    print('EDGE %s: error / bound %.3f (restatement) %.3f (float64)' % (what, r1, r2))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', R.INPUTS)
@pytest.mark.parametrize('cin', [3, 5])
def test_stem_split_every_element_within_the_derived_bound(cin, kind):
    """(2, 37, 53): the bound of the pre-pool values carried through ReLU (1-Lipschitz) and the max-pool (the maximum of the bounds
    over the window)."""
    from rmnet_amd import ops
    n, h, w = 2, 37, 53
    x, wt = R.make_inputs(kind, (n, cin, h, w), R.uniform_weights(64, cin, 7, cin), cin + 1)
    x, wt = x.to(dev()), wt.to(dev())
    bn, shift, _ = _epilogue_terms(64, (1,), 1.0, cin + 2)
    wp, wu = ops.stem_pack(wt, bn)
    frame, mask, other = _stem_inputs(cin, x)
    rw = _rw()
    got = ops.stem_split(frame, mask, other, wp, wu, shift, range_word=rw)
    assert int(rw.item()) == 0
    wh, wl, _ = R.unpack_stem(wp, cin)
    hx, lx = R.split_act(x)
    t, a = R.restate(hx, lx, wh, wl, wu, 2, 3, shift)
    bound = R.kernel_bound(49 * cin, a, t, shift)
    what = 'stem_split cin %d %s %s' % (cin, (n, h, w), kind)
    r1 = _assert_within(got, R.pool(F.relu(t)), R.pool(bound), what + ' against the restatement')
    w64 = wt.double() * bn.double().view(-1, 1, 1, 1)
    true = F.conv2d(x.double(), w64, None, 2, 3) + shift.double().view(1, -1, 1, 1)
    r2 = _assert_within(got, R.pool(F.relu(true)), R.pool(bound + R.repr_bound(x, w64, 2, 3)), what + ' against float64')
    print('EDGE %s: error / bound %.3f (restatement) %.3f (float64)' % (what, r1, r2))


@pytest.mark.gpu
@pytest.mark.parametrize('c', [32, 64, 256])
@pytest.mark.parametrize('n,h,w', HEAD_SHAPES)
def test_pred_head_every_element_within_the_fp32_summation_bound(n, h, w, c):
    """Plain fp32 FMA: |got - fp64| <= (K + 2) 2^-24 (sum |relu(x)||w| + |b|), K = 9 C, for every element."""
    from rmnet_amd import ops
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g).to(dev())
    wt = R.uniform_weights(2, c, 3, seed=c).to(dev())
    b = torch.tensor([0.03, -0.02], device=dev())
    got = ops.pred_head(_cl(x), wt, b)
    xr = F.relu(x).double()
    want = F.conv2d(xr, wt.double(), b.double(), 1, 1)
    bound = (9 * c + 2) * R.U * (F.conv2d(xr, wt.double().abs(), b.double().abs(), 1, 1))
    r = _assert_within(got, want, bound, 'pred_head %s' % ((n, c, h, w),))
    print('EDGE pred_head %s: error / bound %.3f' % ((n, c, h, w), r))


# ================================================================================================ 3. argument checks
SENT = 12345.0
E_INVALID, E_UNSUPPORTED = -1, -4          # include/rmnet_hip.h: RMNET_E_INVALID_ARG, RMNET_E_UNSUPPORTED


def _p(addr):
    return ctypes.c_void_p(addr) if addr else None


def _pool():
    """One allocation of sentinels that every pointer of a raw call is a view into."""
    return torch.full((1 << 17,), SENT, dtype=torch.float32, device=dev())


def _intact(pool):
    torch.cuda.synchronize()
    return bool((pool == SENT).all())


@pytest.mark.gpu
def test_conv_split_entry_rejects_bad_arguments_and_leaves_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    pool = _pool()
    base = pool.data_ptr()
    assert base % 256 == 0
    at = lambda floats: base + 4 * floats
    # 1x1 / stride 1, N 1, 8 x 8, Cin = Cout = 64: x and out have the same extent (4096 floats)
    good = dict(x=at(0), wp=at(32768), wu=at(49152), shift=at(50176), res=None, flags=0, N=1, H=8, W=8, cin=64, cout=64, k=1, s=1,
                out=at(8192), out2=None, split=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rmnet_conv_split_f32(_p(a['x']), _p(a['wp']), _p(a['wu']), _p(a['shift']), _p(a['res']), a['flags'], a['N'], a['H'],
                                        a['W'], a['cin'], a['cout'], a['k'], a['s'], _p(a['out']), _p(a['out2']), a['split'], None, None)

    two = dict(out2=at(16384), split=32)
    cases = [('out is x', dict(out=at(0)), E_INVALID),
             ('out2 overlaps out', dict(out2=at(8192 + 1024), split=32), E_INVALID),
             ('out2 overlaps x', dict(out2=at(256), split=32), E_INVALID),
             ('unknown flag bit', dict(flags=4), E_INVALID),
             ('unknown flag bit next to a known one', dict(flags=8 | 1), E_INVALID),
             ('out2 with res', dict(two, res=at(20480)), E_INVALID),
             ('out_split 0', dict(two, split=0), E_INVALID),
             ('out_split Cout', dict(two, split=64), E_INVALID),
             ('out_split 6', dict(two, split=6), E_INVALID),
             ('ksize 5', dict(k=5), E_UNSUPPORTED),
             ('stride 3', dict(s=3), E_UNSUPPORTED),
             ('Cin 48', dict(cin=48), E_UNSUPPORTED),
             ('Cout 96', dict(cout=96), E_UNSUPPORTED)]
    for name in ('x', 'wp', 'wu', 'shift', 'out'):
        cases.append(('%s misaligned by 4 bytes' % name, {name: good[name] + 4}, E_INVALID))
    cases.append(('res misaligned by 4 bytes', dict(res=at(20480) + 4), E_INVALID))
    cases.append(('out2 misaligned by 4 bytes', dict(two, out2=at(16384) + 4), E_INVALID))
    for name, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (name, rc, want)
        assert _intact(pool), name
    # the same arguments without the fault are accepted (and write): each rejection above is the one change's
    assert call() == 0 and call(**two) == 0 and call(res=at(20480)) == 0
    assert not _intact(pool)


@pytest.mark.gpu
def test_conv_split_wrapper_raises_on_what_it_does_not_implement():
    from rmnet_amd import ops
    x = torch.randn(1, 64, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev())
    wp, wu = ops.conv_split_pack(R.uniform_weights(64, 64, 1, seed=4).to(dev()))
    out = _cl(torch.full((1, 64, 8, 8), SENT))
    xg = _cl(x)
    res = _cl(torch.zeros(1, 64, 8, 8))
    for name, fn in (('NCHW x', lambda: ops.conv_split(x, wp, wu, ksize=1, out=out)),
                     ('float64 x', lambda: ops.conv_split(xg.double(), wp, wu, ksize=1, out=out)),
                     ('pack of another Cin', lambda: ops.conv_split(_cl(x[:, :32]), wp, wu, ksize=1, out=out)),
                     ('res of the wrong shape', lambda: ops.conv_split(xg, wp, wu, None, _cl(torch.zeros(1, 64, 4, 4)), ksize=1, out=out)),
                     ('split with res', lambda: ops.conv_split(xg, wp, wu, None, res, ksize=1, split=32)),
                     ('split with res and out', lambda: ops.conv_split(xg, wp, wu, None, res, ksize=1, out=out, split=32)),
                     ('out is x', lambda: ops.conv_split(out, wp, wu, ksize=1, out=out))):
        with pytest.raises(RuntimeError):
            fn()
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), name
    ok = ops.conv_split(xg, wp, wu, ksize=1, out=out)             # (and the same call without a fault runs)
    assert ok.data_ptr() == out.data_ptr() and not bool((out == SENT).any())


@pytest.mark.gpu
def test_stem_entry_rejects_bad_arguments_and_leaves_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    pool = _pool()
    base = pool.data_ptr()
    at = lambda floats: base + 4 * floats
    good = dict(frame=at(0), mask=at(1024), other=at(2048), wp=at(32768), wu=at(65536), shift=at(66560), N=1, H=8, W=8, out=at(4096))

    def call(**kw):
        a = dict(good, **kw)
        return lib.rmnet_stem_split_f32(_p(a['frame']), _p(a['mask']), _p(a['other']), _p(a['wp']), _p(a['wu']), _p(a['shift']), a['N'],
                                        a['H'], a['W'], _p(a['out']), None, None)

    cases = [('other without mask', dict(mask=None), E_INVALID), ('no frame', dict(frame=None), E_INVALID),
             ('no pack', dict(wp=None), E_INVALID), ('no unscale', dict(wu=None), E_INVALID), ('no out', dict(out=None), E_INVALID),
             ('N 0', dict(N=0), E_INVALID), ('H 0', dict(H=0), E_INVALID), ('W -1', dict(W=-1), E_INVALID)]
    for name in ('wp', 'wu', 'shift', 'out'):
        cases.append(('%s misaligned by 4 bytes' % name, {name: good[name] + 4}, E_INVALID))
    for name in ('frame', 'mask', 'other'):
        cases.append(('%s misaligned by 2 bytes' % name, {name: good[name] + 2}, E_INVALID))
    for name, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (name, rc, want)
        assert _intact(pool), name
    assert call() == 0 and call(mask=None, other=None) == 0 and call(other=None, shift=None) == 0
    assert not _intact(pool)


@pytest.mark.gpu
def test_pred_head_entry_rejects_bad_arguments_and_leaves_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    pool = _pool()
    base = pool.data_ptr()
    at = lambda floats: base + 4 * floats
    good = dict(x=at(0), w=at(8192), bias=at(16384), n=1, H=4, W=4, C=64, out=at(20480))

    def call(**kw):
        a = dict(good, **kw)
        return lib.rmnet_pred_head_f32(_p(a['x']), _p(a['w']), _p(a['bias']), a['n'], a['H'], a['W'], a['C'], _p(a['out']), None)

    cases = [('C 48', dict(C=48), E_UNSUPPORTED), ('x misaligned by 4 bytes', dict(x=at(0) + 4), E_INVALID),
             ('w misaligned by 2 bytes', dict(w=at(8192) + 2), E_INVALID), ('bias misaligned by 2 bytes', dict(bias=at(16384) + 2), E_INVALID),
             ('out misaligned by 2 bytes', dict(out=at(20480) + 2), E_INVALID), ('n 0', dict(n=0), E_INVALID),
             ('no x', dict(x=None), E_INVALID), ('no out', dict(out=None), E_INVALID), ('C 0', dict(C=0), E_INVALID),
             ('no w', dict(w=None), E_INVALID), ('no bias', dict(bias=None), E_INVALID), ('H 0', dict(H=0), E_INVALID),
             ('W 0', dict(W=0), E_INVALID), ('H -1', dict(H=-1), E_INVALID)]
    for name, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (name, rc, want)
        assert _intact(pool), name
    assert call() == 0
    assert not _intact(pool)


@pytest.mark.gpu
def test_stem_and_head_wrappers_raise_on_what_they_do_not_implement():
    """ops.stem_split and ops.pred_head allocate their own output, so there is no caller's buffer to hold a sentinel: the inputs are
    checked to be untouched instead, and the same calls without the fault run."""
    from rmnet_amd import ops
    frame = torch.full((1, 3, 8, 8), SENT, device=dev())
    plane = torch.full((1, 8, 8), SENT, device=dev())
    wp, wu = ops.stem_pack(R.uniform_weights(64, 5, 7, seed=1).to(dev()))
    wp3, wu3 = ops.stem_pack(R.uniform_weights(64, 3, 7, seed=1).to(dev()))
    x = _cl(torch.full((1, 64, 4, 4), SENT))
    wt, b = R.uniform_weights(2, 64, 3, seed=2).to(dev()), torch.zeros(2, device=dev())
    for name, fn in (('other without mask', lambda: ops.stem_split(frame, None, plane, wp, wu)),
                     ('the 3-channel pack with a mask', lambda: ops.stem_split(frame, plane, plane, wp3, wu3)),
                     ('the 5-channel pack without a mask', lambda: ops.stem_split(frame, wpack=wp, w_unscale=wu)),
                     ('a mask of another shape', lambda: ops.stem_split(frame, plane[:, :4].contiguous(), None, wp, wu)),
                     ('a float64 frame', lambda: ops.stem_split(frame.double(), plane, None, wp, wu)),
                     ('no pack', lambda: ops.stem_split(frame, plane)),
                     ('head: C 48', lambda: ops.pred_head(_cl(x[:, :48]), wt[:, :48].contiguous(), b)),
                     ('head: NCHW x', lambda: ops.pred_head(x.contiguous(), wt, b)),
                     ('head: float64 x', lambda: ops.pred_head(x.double(), wt, b)),
                     ('head: weight of another C', lambda: ops.pred_head(x, wt[:, :32].contiguous(), b)),
                     ('head: three biases', lambda: ops.pred_head(x, wt, torch.zeros(3, device=dev())))):
        with pytest.raises(RuntimeError):
            fn()
        torch.cuda.synchronize()
        assert bool((frame == SENT).all()) and bool((plane == SENT).all()) and bool((x == SENT).all()), name
    assert ops.stem_split(frame, plane, plane, wp, wu).shape == (1, 64, 2, 2)
    assert ops.stem_split(frame, wpack=wp3, w_unscale=wu3).shape == (1, 64, 2, 2)
    assert ops.pred_head(x, wt, b).shape == (1, 2, 4, 4)
