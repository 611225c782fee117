# -*- coding: utf-8 -*-
"""The split-fp16 convolutions' K walk (csrc/conv3x3.hip, csrc/conv_split.hip).  conv3x3_split walks K taps outside, channel blocks
inside, with the border test as a per-pixel tap mask and a branch-free load, the input ReLU and the range count hoisted to one loop
instance per (ReLU, counted tap), and the next step's activation split placed between the MFMAs of the current one; conv_split's
three tiles derive the tap from the step number and test the border per load.  Both must read the same elements and count the same
ones, so the same cases run on both.  Everything here is bit for bit against the
float64 convolution on integer-valued inputs (why that is exact: tests/conv_ref.py, section 1), except the randn cases, which are
held per element to conv_ref's derived bound (section 2) and guard the cross terms that integer inputs leave at zero.

  * one live tap at a time: nine packs, each zero outside one tap, on an input that holds (nearly) a different integer in every
    element -- x = (flat NHWC index mod 2039) - 1019, so that 64 x is an fp16 number inside the window and every element within
    21 pixels of another differs from it.  A tap that reads the wrong pixel, the wrong channel block, or a pixel across a row or an
    image border shows as a wrong integer.  Sums: Cin * 1019 * 8 < 2^20 in the common unit, exact in fp32 in any order;
  * Cin 32 and 96: the tap changes after 1 and after 3 channel blocks; maps 2x5x7 and 1x9x15: a 128-pixel tile spans rows and images;
  * the input ReLU on and off, on negative inputs;
  * the range word: an out-of-window value, a NaN and a negative out-of-window value, each at a border pixel -- where the taps of
    its neighbours that do not count read it as well -- and each once in the first and once in the second channel block.  The
    expected word follows from the rule alone: every element that the convolution reads is counted once, at its counted tap, if
    pre(x) is outside the window (the negative one is not, after the ReLU);
  * CPU: the kernels' registers, spills, scratch and LDS, against the limits tests/test_kernel_resources.py states."""

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

MAP_A, MAP_B, MAP_S2 = (2, 5, 7), (1, 9, 15), (2, 7, 9)
# Big needs 512 workgroups: one pixel tile x 512 slices of 256 channels, every slice with the same 256-channel pack.  That is a
# 131072-channel output per launch: 37 MB at the 70 pixels of MAP_A, and a 16 MB pack per K step.  It is affordable only because
# the maps are this small -- enlarge the maps and Big's cases stop being quick.
TILE_COUT = {'Narrow': 64, 'Mid': 128, 'Big': 512 * 256}
TILE_REAL = {'Narrow': 64, 'Mid': 128, 'Big': 256}
TILES = ['Narrow', 'Mid', 'Big']
PRIME = 2039


def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _rw():
    return torch.zeros(1, dtype=torch.int32, device=dev())


def _distinct_acts(n, cin, h, w):
    """[N, Cin, H, W]: element (n, c, y, x) holds (its flat NHWC index mod 2039) - 1019."""
    flat = torch.arange(n * h * w * cin, dtype=torch.int64)
    return ((flat % PRIME) - (PRIME // 2)).float().view(n, h, w, cin).permute(0, 3, 1, 2).contiguous()


def _one_tap(wt, tap):
    w1 = torch.zeros_like(wt)
    w1[:, :, tap // 3, tap % 3] = wt[:, :, tap // 3, tap % 3]
    return w1


def _assert_equal(got, want64, what):
    want = want64.float()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index, got, want): %s' % (what, bad.shape[0], got.numel(), first))


def _pack(kernel, tile, wt, bn):
    """(wpack, unscale, real Cout): Big's pack is the 256-channel pack repeated over 512 slices."""
    from rmnet_amd import ops
    if kernel == 'conv3x3':
        return ops.conv3x3_pack(wt) + (256,)
    wp, wu = ops.conv_split_pack(wt, bn)
    real = wt.shape[0]
    rep = TILE_COUT[tile] // real
    if rep > 1:
        k2, cin = wt.shape[2] * wt.shape[3], wt.shape[1]
        wp = wp.view(k2, cin // 32, 2, real, 32).repeat(1, 1, 1, rep, 1).contiguous().view(-1)
        wu = wu.repeat(rep)
    return wp, wu, real


def _launch(kernel, tile, x, wp, wu, shift, k, s, relu_in, real):
    """One launch -> (got [N, real Cout, Ho, Wo] after checking that every slice of Big returned the same, range word)."""
    from rmnet_amd import ops
    rw = _rw()
    if kernel == 'conv3x3':
        got = ops.conv3x3_split(_cl(x), wp, wu, shift, None, relu_in=relu_in, range_word=rw)
    else:
        n, _, h, w = x.shape
        assert R.tile_of(n, wu.numel(), h, w, k, s) == tile
        sh = shift.repeat(wu.numel() // real) if shift is not None else None
        got = ops.conv_split(_cl(x), wp, wu, sh, None, ksize=k, stride=s, relu_in=relu_in, range_word=rw)
        if wu.numel() != real:
            sl = got.unflatten(1, (wu.numel() // real, real))
            same = sl == sl[:, :1]
            same |= sl.isnan() & sl[:, :1].isnan()
            assert bool(same.all()), 'the Cout slices of one pack differ'
            got = sl[:, 0]
    torch.cuda.synchronize()
    return got, int(rw.item())


def _want(x, wt, bn, shift, k, s, relu_in):
    xd = F.relu(x.double()) if relu_in else x.double()
    w64 = wt.double() * (bn.double().view(-1, 1, 1, 1) if bn is not None else 1.0)
    return F.conv2d(xd, w64, None, s, k // 2) + shift.double().view(1, -1, 1, 1)


def _terms(kernel, tile, cin, k, seed):
    cout = 256 if kernel == 'conv3x3' else TILE_REAL[tile]
    wt = R.int_weights(cout, cin, k, seed).to(dev())
    bn = None if kernel == 'conv3x3' else R.pow2_scale(cout).to(dev())
    shift = R.int_acts((cout,), seed + 1, -20, 20).to(dev())
    return wt, bn, shift


# ================================================================================================ one live tap at a time
def _one_live_tap(kernel, tile, shape, cin, s):
    n, h, w = shape
    x = _distinct_acts(n, cin, h, w).to(dev())
    assert float(x.abs().max()) <= 1019 and bool((x[0, :, 0, 0] != x[0, :, 0, 1]).all()) and bool((x[0, :, 0, 0] != x[0, :, 1, 0]).all())
    wt, bn, shift = _terms(kernel, tile, cin, 3, 11 + cin)
    for tap in range(9):
        w1 = _one_tap(wt, tap)
        wp, wu, real = _pack(kernel, tile, w1, bn)
        got, bad = _launch(kernel, tile, x, wp, wu, shift, 3, s, False, real)
        assert bad == 0, (tap, bad)
        _assert_equal(got, _want(x, w1, bn, shift, 3, s, False), '%s %s %s Cin %d stride %d, tap %d alone' % (kernel, tile, shape, cin, s, tap))


@pytest.mark.gpu
@pytest.mark.parametrize('cin', [32, 96])
@pytest.mark.parametrize('shape', [MAP_A, MAP_B])
def test_conv3x3_split_one_live_tap_at_a_time(shape, cin):
    _one_live_tap('conv3x3', None, shape, cin, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('cin', [32, 96])
@pytest.mark.parametrize('tile', TILES)
def test_conv_split_3x3_one_live_tap_at_a_time(tile, cin):
    _one_live_tap('conv_split', tile, MAP_A, cin, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('tile', TILES)
def test_conv_split_3x3_stride_2_on_an_odd_map_one_live_tap_at_a_time(tile):
    _one_live_tap('conv_split', tile, MAP_S2, 32, 2)


# ================================================================================================ the input ReLU, on and off
KERNEL_TILES = [('conv3x3', None)] + [('conv_split', t) for t in TILES]


@pytest.mark.gpu
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('kernel,tile', KERNEL_TILES)
def test_input_relu_on_and_off_on_negative_inputs(kernel, tile, relu_in):
    n, h, w = MAP_A
    x = R.int_acts((n, 64, h, w), 5).to(dev())
    assert float(x.min()) == -15.0
    wt, bn, shift = _terms(kernel, tile, 64, 3, 21)
    wp, wu, real = _pack(kernel, tile, wt, bn)
    got, bad = _launch(kernel, tile, x, wp, wu, shift, 3, 1, relu_in, real)
    assert bad == 0
    want = _want(x, wt, bn, shift, 3, 1, relu_in)
    assert not torch.equal(want, _want(x, wt, bn, shift, 3, 1, not relu_in))
    _assert_equal(got, want, '%s %s relu_in %s' % (kernel, tile, relu_in))


# ================================================================================================ the range word
def _planted(n, h, w, s):
    """(image, channel, y, x, value) of the planted elements: three border pixels that the convolution reads at a counted tap (with
    stride 2 on an odd map every pixel is read by one: even rows / columns by the centre tap's, odd ones by the last tap's), each
    value once in channel block 0 and once in block 1."""
    big, nan, neg = 2000.0, float('nan'), -2000.0
    return [(0, 5, 0, 0, big), (0, 37, 0, w - 1, big),
            (n - 1, 9, h - 1, w - 1, nan), (n - 1, 41, h - 1, 0, nan),
            (0, 13, h - 1, w // 2, neg), (n - 1, 45, 0, w // 2 + 1, neg)]


def _range_case(kernel, tile, shape, k, s, relu_in):
    n, h, w = shape
    x = R.int_acts((n, 64, h, w), 9).to(dev())
    plants = _planted(n, h, w, s)
    assert len({(i, y, xx) for i, _, y, xx, _ in plants}) == 6          # six different pixels, all on the border
    for i, c, y, xx, v in plants:
        assert y in (0, h - 1) or xx in (0, w - 1)
        x[i, c, y, xx] = v
    wt, bn, shift = _terms(kernel, tile, 64, k, 31)
    wp, wu, real = _pack(kernel, tile, wt, bn)
    got, bad = _launch(kernel, tile, x, wp, wu, shift, k, s, relu_in, real)
    # the rule: once, at the counted tap, every element whose pre(x) is outside the window: 2000 and NaN always, -2000 only without ReLU
    expect = sum(1 for _, _, _, _, v in plants if not (relu_in and v < 0))
    assert expect == (4 if relu_in else 6)
    assert bad == expect, (bad, expect)
    # every output that reads no planted element is still exact
    xc = x.clone()
    dirty = torch.zeros(n, 1, h, w, dtype=torch.float64, device=dev())
    for i, c, y, xx, v in plants:
        xc[i, c, y, xx] = 0.0
        dirty[i, 0, y, xx] = 1.0
    clean = F.conv2d(dirty, torch.ones(1, 1, k, k, dtype=torch.float64, device=dev()), None, s, k // 2) == 0
    assert 0 < int(clean.sum()) < clean.numel()
    want = _want(xc, wt, bn, shift, k, s, relu_in).float()
    m = clean.expand_as(want)
    assert torch.equal(got[m], want[m]), '%s %s: outputs that read no planted element differ' % (kernel, tile)


@pytest.mark.gpu
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('kernel,tile', KERNEL_TILES)
def test_range_word_counts_each_planted_element_once_at_its_counted_tap(kernel, tile, relu_in):
    _range_case(kernel, tile, MAP_A, 3, 1, relu_in)


@pytest.mark.gpu
@pytest.mark.parametrize('tile', TILES)
def test_range_word_3x3_stride_2_on_an_odd_map(tile):
    _range_case('conv_split', tile, MAP_S2, 3, 2, True)


@pytest.mark.gpu
@pytest.mark.parametrize('tile', TILES)
def test_range_word_1x1_counts_in_the_first_and_in_later_channel_blocks(tile):
    """1x1: the only tap counts, so the first channel block is counted by the prologue's store and the second inside the loop."""
    _range_case('conv_split', tile, MAP_A, 1, 1, True)


# ================================================================================================ non-integer inputs
@pytest.mark.gpu
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('kernel,tile', KERNEL_TILES)
def test_randn_inputs_stay_inside_the_derived_bound_per_element(kernel, tile, relu_in):
    n, h, w = MAP_A
    cin, k = 64, 3
    g = torch.Generator().manual_seed(77)
    x = torch.randn((n, cin, h, w), generator=g).to(dev())
    cout = 256 if kernel == 'conv3x3' else TILE_REAL[tile]
    wt = R.uniform_weights(cout, cin, k, 78).to(dev())
    shift = torch.randn(cout, generator=g).to(dev())
    wp, wu, real = _pack(kernel, tile, wt, None)
    wp1, wu1 = wp.view(9, cin // 32, 2, -1, 32)[:, :, :, :real].contiguous().view(-1), wu[:real]
    got, bad = _launch(kernel, tile, x, wp, wu, shift, k, 1, relu_in, real)
    assert bad == 0
    wh, wl = R.unpack_conv(wp1, real, cin, k)
    hx, lx = R.split_act(x, relu=relu_in)
    t, a = R.restate(hx, lx, wh, wl, wu1, 1, 1, shift)
    bound = R.kernel_bound(k * k * cin, a, t, shift)
    err = (got.double() - t).abs()
    worst = float((err / bound).max())
    print('%s %s relu_in %s: largest error / bound %.3f' % (kernel, tile, relu_in, worst))
    assert bool((err <= bound).all()), worst
    # (and the restatement is the convolution: a dropped cross term is far outside what follows)
    true = _want(x, wt, None, shift, k, 1, relu_in)
    assert bool(((got.double() - true).abs() <= bound + R.repr_bound(x, wt.double(), 1, 1, relu=relu_in)).all())


# ================================================================================================ CPU: what the compiler gives
VGPR_LIMIT = {'conv3x3_split': 256, 'Big': 256, 'Mid': 128, 'Narrow': 128}      # one workgroup per CU: 256; two: 128


def test_the_two_files_kernels_keep_their_registers_lds_and_have_no_spill_or_scratch(tmp_path):
    """Compile-only, from the code objects' metadata, with tests/test_kernel_resources.py's own compile step, metadata reader and
    kernel table (its helpers, so that the two files cannot drift apart), against the limits that file states: LDS exactly the
    declared double buffer, no scratch, no spilled register, at most 256 VGPRs for the kernels that run one workgroup per CU and
    128 for those that run two."""
    import test_kernel_resources as KR
    found = {}
    for src in ('conv3x3.hip', 'conv_split.hip'):
        for name, res in KR._kernels(KR._compile(src, str(tmp_path / (src + '.s')))).items():
            found[name] = dict(res, src=src)
    conv = KR._conv_kernels(found)
    assert sorted(conv) == sorted(VGPR_LIMIT)
    for name, (k, mt, nt, vgprs) in conv.items():
        print('%-14s LDS %6d  scratch %d  VGPRs %3d  spilled %d' % (name, k['group_segment_fixed_size'], k['private_segment_fixed_size'],
                                                                   k['vgpr_count'], k['vgpr_spill_count']))
        assert vgprs == VGPR_LIMIT[name], (name, vgprs)
        assert k['group_segment_fixed_size'] == KR._double_buffer_bytes(mt, nt), (name, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (name, k)
        assert k['vgpr_count'] <= VGPR_LIMIT[name], (name, k)
