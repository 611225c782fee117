# -*- coding: utf-8 -*-
"""TinyFlowNet's wide convolutions on the split-fp16 tap-list kernel (csrc/flow_conv.hip): the packer, the phase decomposition of
the transposed convolution and the compiler's resources on the CPU; on the GPU integer inputs bit for bit, channel-strided outputs
against sentinels, the lo planes (exact family and per-element bound of tests/conv_ref.py), the range word, the C entry's argument
checks, and the whole network through the RMNET_FLOW_CONV switch."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import flow_conv_ref as FR


def dev():
    return torch.device('cuda', 0)


def _rw():
    return torch.zeros(1, dtype=torch.int32, device=dev())


def _buffer(x, ld, fill=0.0):
    """[N, C, H, W] -> a channels-last [N, ld, H, W] device buffer holding x in its first C channels and ``fill`` behind them."""
    n, c, h, w = x.shape
    b = torch.full((n, h, w, ld), fill, dtype=torch.float32)
    b[..., :c] = x.permute(0, 2, 3, 1)
    return b.to(dev()).permute(0, 3, 1, 2)


def _weights(kind, cout, cin, k, transposed, seed):
    """Conv2d [Cout, Cin, k, k] or, transposed, ConvTranspose2d [Cin, Cout, 4, 4] weights of one of conv_ref.py's families (their
    per-output-channel structure kept)."""
    w = {'int': R.int_weights, 'lo': R.lo_weights, 'uniform': R.uniform_weights}[kind](cout, cin, k, seed)
    return w.permute(1, 0, 2, 3).contiguous() if transposed else w


def _run(x, w, shift, ksize, stride, transposed, act, x_ld=None, out=None, coff=0, rw=None, fill=0.0):
    from rmnet_amd import ops
    wp, wu = ops.flow_conv_pack(w, transposed=transposed)
    cin = x.shape[1]
    xb = _buffer(x, x_ld or cin, fill)
    got = ops.flow_conv(xb, wp.to(dev()), wu.to(dev()), None if shift is None else shift.to(dev()), ksize=ksize, stride=stride,
                        transposed=transposed, act=act, cin=cin, out=out, out_coff=coff, range_word=rw)
    return got


def _assert_equal(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index, got, want): %s' % (what, bad.shape[0], got.numel(), first))


# ================================================================================================ CPU
def _roundtrip_weights(shape, seed):
    """Magnitudes in [0.1, 1] of a per-channel scale: no weight so far below its channel's largest that its lo half is an fp16
    subnormal (there the pack's error is 2^-25 absolute, not 2^-22 relative; conv_ref.py section 2)."""
    g = torch.Generator().manual_seed(seed)
    w = (0.1 + 0.9 * torch.rand(shape, generator=g)) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    return w


@pytest.mark.parametrize('cout,cin,k,transposed', [(64, 64, 3, False), (128, 194, 5, False), (64, 386, 4, True), (128, 32, 4, True)])
def test_the_pack_restores_every_weight_and_pads_with_zeros(cout, cin, k, transposed):
    """(hi + lo) * unscale is the weight within 2^-21 relative, forward and transposed (each 4x4 element appears in exactly one
    phase and tap); the channels Cin .. ceil32(Cin) - 1 are exactly zero in both planes; the scale is a power of two that puts the
    channel's largest magnitude in [2^14, 2^15)."""
    from rmnet_amd import ops
    shape = (cin, cout, 4, 4) if transposed else (cout, cin, k, k)
    w = _roundtrip_weights(shape, seed=cout + cin) * (2.0 ** (torch.arange(cout) % 7 - 3)).view((1, -1, 1, 1) if transposed else (-1, 1, 1, 1))
    wp, wu = ops.flow_conv_pack(w, transposed=transposed)
    cp = FR.ceil32(cin)
    taps, phases = (4, 4) if transposed else (k * k, 1)
    assert wp.dtype == torch.int16 and wp.numel() == phases * taps * cp * cout * 2 and wu.shape == (cout,)
    wh, wl = FR.unpack(wp, cout, cin, taps, phases)
    assert float(wh[:, :, cin:].abs().max() if cp > cin else 0.0) == 0.0 and float(wl[:, :, cin:].abs().max() if cp > cin else 0.0) == 0.0
    back = (wh + wl) * wu.double().view(1, -1, 1, 1)                      # [P, Cout, Cp, taps]
    m, e = torch.frexp(wu.double())
    assert torch.equal(m, torch.full_like(m, 0.5))                         # a power of two
    big = w.double().abs().amax(dim=(0, 2, 3) if transposed else (1, 2, 3)) / wu.double()       # (hi itself may round up to 2^15)
    assert bool(((big >= 2.0 ** 14) & (big < 2.0 ** 15)).all())
    if transposed:
        seen = torch.zeros(4, 4)
        for a in (0, 1):
            for b in (0, 1):
                for ty, tx, ky, kx in FR.phase_taps(a, b):
                    want = w[:, :, ky, kx].double().t()                    # [Cout, Cin]
                    got = back[2 * a + b, :, :cin, 2 * ty + tx]
                    assert bool(((got - want).abs() <= 2.0 ** -21 * want.abs()).all()), (a, b, ty, tx)
                    seen[ky, kx] += 1
        assert torch.equal(seen, torch.ones(4, 4))
    else:
        want = w.double().reshape(cout, cin, k * k)
        assert bool(((back[0, :, :cin] - want).abs() <= 2.0 ** -21 * want.abs()).all())


@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 7)])
def test_four_two_by_two_phases_are_the_transposed_convolution(h, w):
    """Integer inputs and weights, float64: the numpy restatement of 'four 2x2-tap convolutions in the pack's tap order' equals
    F.conv_transpose2d(4, stride 2, padding 1) exactly -- and so do the phase weights the packer itself builds."""
    from rmnet_amd import ops
    x = R.int_acts((2, 3, h, w), seed=h * 10 + w).double()
    wt = R.int_acts((3, 5, 4, 4), seed=7, lo=-8, hi=8).double()
    want = F.conv_transpose2d(x, wt, None, 2, 1)
    assert np.array_equal(FR.deconv_by_phases_numpy(x.numpy(), wt.numpy()), want.numpy())
    ph = ops.flow_conv_phase_weights(wt)                                   # [4, Cout, Cin, 2, 2]
    assert ph.shape == (4, 5, 3, 2, 2)
    got = FR.per_phase(lambda p, conv: conv(x, ph[p]), x, True, 4, 2)
    assert torch.equal(got, want)


def test_fuse_epilogues_leaves_the_state_dict_alone():
    from rmnet_amd import networks
    from rmnet_amd.tiny_flownet import FLOW_SPLIT_LAYERS, TinyFlowNet
    net = networks.procedural_init_(TinyFlowNet(None)).eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.fuse_epilogues()
    after = net.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(torch.equal(after[k], before[k]) for k in before)
    assert sorted(net._flow_packs) == sorted(FLOW_SPLIT_LAYERS) and len(FLOW_SPLIT_LAYERS) == 10
    assert not [n for n, _ in net.named_buffers()] and len(list(net.parameters())) == len(before)
    for name in FLOW_SPLIT_LAYERS:                  # a pack per layer, of the size its shape gives
        conv = getattr(net, name)[0]
        tr = isinstance(conv, torch.nn.ConvTranspose2d)
        taps = 16 if tr else conv.kernel_size[0] ** 2
        wp, wu = net._flow_packs[name]
        assert wu.numel() == conv.out_channels and wp.numel() == taps * FR.ceil32(conv.in_channels) * conv.out_channels * 2, name


def test_the_switch_has_the_measured_default_and_rejects_other_values(monkeypatch):
    """'split' since the bench rule was met (profiles/r13_a_flow_conv.md)."""
    from rmnet_amd import tiny_flownet
    monkeypatch.delenv('RMNET_FLOW_CONV', raising=False)
    assert tiny_flownet.flow_conv_backend() == tiny_flownet.FLOW_CONV_DEFAULT == 'split'
    monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
    assert tiny_flownet.flow_conv_backend() == 'split'
    monkeypatch.setenv('RMNET_FLOW_CONV', 'fast')
    with pytest.raises(RuntimeError):
        tiny_flownet.flow_conv_backend()


def test_the_kernel_gets_no_scratch_no_spill_and_no_static_lds(tmp_path):
    """Compile-only, from the metadata (sizes and register counts, as test_kernel_resources.py reads them): the kernel takes its
    LDS at launch (static 0), has no scratch and no spilled VGPR, and fits two workgroups per CU (<= 128 VGPRs)."""
    from rmnet_amd import build
    from test_kernel_resources import _compile, _kernels
    assert 'flow_conv.hip' in build.SOURCES
    ks = {n: k for n, k in _kernels(_compile('flow_conv.hip', str(tmp_path / 'flow_conv.s'))).items() if 'flow_taps' in n}
    assert len(ks) == 1, sorted(ks)
    for name, k in ks.items():
        print(name, k)
        assert 'conv_split' not in name and 'conv3x3_split' not in name
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (name, k)
        assert k['vgpr_count'] <= 128, (name, k)


# ================================================================================================ GPU: integers, bit for bit
FWD = {'k3s1': (3, 1, False), 'k3s2': (3, 2, False), 'k5s2': (5, 2, False), 'tr': (4, 2, True)}


# (layer, N, H, W, Cin, x_ld, Cout, act): every layer kind on every map, both N, every Cin / x_ld, every Cout (one, two and four
# 64-channel slices), every activation; 3 x 7 x 7 = 147 grid pixels cross a 128-pixel tile.  The two last cases have 130 and 32
# pixel tiles per slice and phase: more workgroups than CUs.
EXACT = [
    ('k3s1', 1, 1, 1, 32, 32, 64, 'leaky'), ('k3s1', 3, 5, 7, 64, 64, 128, 'relu'), ('k3s1', 1, 9, 11, 194, 224, 256, None),
    ('k3s1', 3, 7, 7, 386, 416, 64, 'leaky'), ('k3s1', 1, 5, 7, 770, 800, 128, 'leaky'),
    ('k3s2', 1, 1, 1, 64, 64, 128, None), ('k3s2', 3, 5, 7, 32, 32, 256, 'leaky'), ('k3s2', 3, 9, 11, 64, 64, 64, 'relu'),
    ('k3s2', 1, 9, 11, 386, 416, 128, 'leaky'), ('k3s2', 3, 14, 14, 32, 32, 64, None),
    ('k5s2', 1, 1, 1, 32, 32, 256, 'relu'), ('k5s2', 3, 5, 7, 194, 224, 64, 'leaky'), ('k5s2', 1, 9, 11, 64, 64, 128, 'leaky'),
    ('k5s2', 3, 14, 14, 64, 96, 128, None), ('k5s2', 1, 5, 7, 770, 800, 64, 'relu'),
    ('tr', 1, 1, 1, 32, 32, 64, None), ('tr', 3, 5, 7, 64, 64, 256, 'leaky'), ('tr', 1, 9, 11, 770, 800, 128, 'leaky'),
    ('tr', 3, 7, 7, 386, 416, 64, 'relu'), ('tr', 3, 9, 11, 194, 224, 128, None), ('tr', 1, 5, 7, 32, 64, 256, 'relu'),
    ('k3s2', 1, 255, 257, 32, 32, 256, 'leaky'), ('tr', 1, 63, 65, 32, 32, 256, 'leaky'),
]


def test_the_exact_cases_cover_what_the_issue_lists():
    for axis, values in ((0, set(FWD)), (1, {1, 3}), (4, {32, 64, 194, 386, 770}), (6, {64, 128, 256}), (7, {None, 'relu', 'leaky'})):
        assert {c[axis] for c in EXACT} == values, axis
    assert {(1, 1), (5, 7), (9, 11)} <= {(c[2], c[3]) for c in EXACT} and any(c[1] * c[2] * c[3] == 147 for c in EXACT)


@pytest.mark.gpu
@pytest.mark.parametrize('layer,n,h,w,cin,x_ld,cout,act', EXACT)
def test_integer_inputs_come_back_bit_for_bit(layer, n, h, w, cin, x_ld, cout, act):
    """Integer activations |x| <= 15 and weights |w| <= 8, an integer shift: lo planes zero and every partial sum below 2^24
    (K <= 25 * 770, K * 120 < 2^24), so the kernel must return the float64 convolution rounded once (conv_ref.py section 1); the
    LeakyReLU's negative outputs are one fp32 product y * 0.1f."""
    k, s, tr = FWD[layer]
    x = R.int_acts((n, cin, h, w), seed=n * 100 + h * 10 + cin)
    wt = _weights('int', cout, cin, k, tr, seed=cout + cin + k)
    shift = R.int_acts((cout,), seed=5, lo=-40, hi=40)
    want64 = FR.reference(x, wt, shift, k, s, tr)
    assert float(want64.abs().max()) < 2.0 ** 24
    want = FR.activate(want64, act)
    if act == 'leaky':
        assert bool((want64 < 0).any())
    rw = _rw()
    got = _run(x, wt, shift, k, s, tr, act, x_ld=x_ld, rw=rw)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _assert_equal(got, want, '%s N %d %dx%d Cin %d Cout %d %s' % (layer, n, h, w, cin, cout, act))
    assert int(rw.item()) == 0


# ================================================================================================ GPU: strided output
@pytest.mark.gpu
@pytest.mark.parametrize('layer,n,h,w,cin,cout', [('k3s1', 3, 7, 7, 64, 64), ('k5s2', 1, 9, 11, 32, 128), ('tr', 3, 5, 7, 64, 128),
                                                  ('tr', 1, 9, 11, 32, 64), ('tr', 1, 63, 65, 32, 256)])
@pytest.mark.parametrize('coff', [0, 128])
def test_a_strided_output_touches_only_its_channels(layer, n, h, w, cin, cout, coff):
    """``out`` is a sentinel-filled buffer of 416 channels per pixel inside a longer allocation: the channels outside
    [coff, coff + Cout) and everything behind the last pixel keep their bits, the channels inside are the exact result -- every
    output pixel written (a pixel no phase wrote would keep the sentinel), and the same from a second run into another fill."""
    from rmnet_amd import ops
    k, s, tr = FWD[layer]
    ld, slack = 416, 4096
    x = R.int_acts((n, cin, h, w), seed=17 + coff)
    wt = _weights('int', cout, cin, k, tr, seed=3)
    shift = R.int_acts((cout,), seed=6, lo=-9, hi=9)
    want = FR.activate(FR.reference(x, wt, shift, k, s, tr), 'leaky')
    ho, wo = ops.flow_conv_out_hw(h, w, k, s, tr)
    results = []
    for sentinel in (-12345.5, float('nan')):
        flat = torch.full((n * ho * wo * ld + slack,), sentinel, device=dev())
        before = flat.clone().view(torch.int32)
        out = flat[:n * ho * wo * ld].view(n, ho, wo, ld).permute(0, 3, 1, 2)
        ret = _run(x, wt, shift, k, s, tr, 'leaky', out=out, coff=coff)
        assert ret.data_ptr() == out.data_ptr()
        after = flat.view(torch.int32)
        assert torch.equal(after[n * ho * wo * ld:], before[n * ho * wo * ld:])
        px_after, px_before = after[:n * ho * wo * ld].view(-1, ld), before[:n * ho * wo * ld].view(-1, ld)
        assert torch.equal(px_after[:, :coff], px_before[:, :coff]) and torch.equal(px_after[:, coff + cout:], px_before[:, coff + cout:])
        got = out[:, coff:coff + cout]
        _assert_equal(got, want, '%s coff %d sentinel %r' % (layer, coff, sentinel))
        results.append(got.clone())
    assert torch.equal(results[0], results[1])


# ================================================================================================ GPU: the lo planes
@pytest.mark.gpu
@pytest.mark.parametrize('layer,n,h,w,cin,x_ld,cout', [('k3s1', 3, 7, 7, 64, 64, 128), ('k3s2', 1, 9, 11, 32, 32, 64),
                                                       ('k5s2', 3, 5, 7, 64, 64, 64), ('tr', 3, 7, 7, 64, 64, 64),
                                                       ('tr', 1, 5, 7, 194, 224, 128), ('k3s1', 1, 5, 7, 194, 224, 64),
                                                       ('tr', 1, 63, 65, 32, 32, 256)])
def test_the_lo_exact_family_comes_back_bit_for_bit(layer, n, h, w, cin, x_ld, cout):
    """conv_ref.py section 1b: x = a + b 2^-14 and w = p + q 2^-13 give live cross terms in every tap with both accumulators still
    exact (K * 432 < 2^24), so the kernel must return ``restate``'s prediction -- fp32(acc + accx), scaled, fp32(. + shift) -- bit
    for bit; a kernel that loses a lo plane in one tap or phase does not."""
    from rmnet_amd import ops
    k, s, tr = FWD[layer]
    x = R.lo_acts((n, cin, h, w), seed=cin + h)
    wt = _weights('lo', cout, cin, k, tr, seed=cout + k)
    shift = R.int_acts((cout,), seed=8, lo=-20, hi=20)
    wp, wu = ops.flow_conv_pack(wt, transposed=tr)
    taps, phases = (4, 4) if tr else (k * k, 1)
    wh, wl = FR.unpack(wp, cout, cin, taps, phases)
    assert float(wl.abs().max()) > 0.0 and float(R.split_act(x)[1].abs().max()) > 0.0
    assert torch.equal(((wh + wl) * wu.double().view(1, -1, 1, 1))[:, :, :cin].sum(0).sum(-1),
                       (wt.double().permute(1, 0, 2, 3) if tr else wt.double()).sum((2, 3)))            # the pack is exact
    assert taps * cin * 432 < 2 ** 24
    _, _, pred = FR.restate(x, wp, wu, cout, cin, k, s, tr, shift)
    got = _run(x, wt, shift, k, s, tr, None, x_ld=x_ld)
    _assert_equal(got, pred.float(), '%s lo-exact' % layer)


@pytest.mark.gpu
@pytest.mark.parametrize('scale', ['1e-3', '1', '1e2'])
@pytest.mark.parametrize('layer,n,h,w,cin,x_ld,cout', [('k3s1', 3, 7, 7, 32, 32, 64), ('k5s2', 1, 9, 11, 64, 64, 128),
                                                       ('tr', 3, 7, 7, 194, 224, 64)])
def test_every_element_is_within_the_three_term_bound(layer, n, h, w, cin, x_ld, cout, scale):
    """Random inputs at three scales against the float64 convolution, element by element: conv_ref.py's kernel bound
    (K + 4) 2^-24 A + 2^-23 (|shift| + |T|) with K = taps * Cin products per accumulator (<= 2050), plus its representation bound
    3 * 2^-22 sum|x||w| + 2^-31 sum|w|.  Nothing tuned."""
    from rmnet_amd import ops
    k, s, tr = FWD[layer]
    wt = _weights('uniform', cout, cin, k, tr, seed=cout + cin)
    x, _ = R.make_inputs(scale, (n, cin, h, w), wt, seed=int(float(scale) * 1000) + cin)
    shift = torch.randn(cout, generator=torch.Generator().manual_seed(2)) * float(scale)
    wp, wu = ops.flow_conv_pack(wt, transposed=tr)
    taps = 4 if tr else k * k
    assert taps * cin <= 2050
    t, a, _ = FR.restate(x, wp, wu, cout, cin, k, s, tr, shift)
    conv_abs = (lambda p, q: F.conv_transpose2d(p, q, None, 2, 1)) if tr else (lambda p, q: F.conv2d(p, q, None, s, k // 2))
    repr_b = 3 * 2.0 ** -22 * conv_abs(x.double().abs(), wt.double().abs()) + 2.0 ** -31 * conv_abs(torch.ones_like(x).double(), wt.double().abs())
    bound = R.kernel_bound(taps * cin, a, t, shift) + repr_b
    ref = FR.reference(x, wt, shift, k, s, tr)
    got = _run(x, wt, shift, k, s, tr, None, x_ld=x_ld).cpu().double()
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('%s scale %s: largest error / bound %.3g' % (layer, scale, ratio))
    assert bool((err <= bound).all()), (layer, scale, ratio, int((err > bound).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('layer,cin,x_ld', [('k3s1', 194, 224), ('tr', 770, 800), ('k5s2', 386, 416)])
def test_what_the_padding_channels_hold_does_not_matter(layer, cin, x_ld):
    """1e3 in the channels Cin .. x_ld - 1 of the input buffer instead of zero: the same output, bit for bit (the pack's weights
    there are zero), and the range word does not count them."""
    k, s, tr = FWD[layer]
    x = R.lo_acts((2, cin, 5, 7), seed=cin)
    wt = _weights('uniform', 64, cin, k, tr, seed=1)
    zeros = _run(x, wt, None, k, s, tr, 'leaky', x_ld=x_ld, fill=0.0)
    rw = _rw()
    filled = _run(x, wt, None, k, s, tr, 'leaky', x_ld=x_ld, fill=1e3, rw=rw)
    assert torch.equal(zeros, filled) and int(rw.item()) == 0
    rw = _rw()
    nan = _run(x, wt, None, k, s, tr, 'leaky', x_ld=x_ld, fill=float('nan'), rw=rw)
    assert torch.equal(zeros, nan) and int(rw.item()) == 0


# ================================================================================================ GPU: the range word
@pytest.mark.gpu
@pytest.mark.parametrize('layer', ['k3s1', 'k5s2', 'tr'])
def test_the_range_word_counts_what_leaves_the_window(layer):
    """Clean input: 0.  One planted 2000.0, NaN or Inf (|x| >= 1023.5 saturates): non-zero, whichever pixel and channel holds it --
    the last real channel of a padded buffer and the last pixel included."""
    k, s, tr = FWD[layer]
    cin, x_ld = 194, 224
    x = R.int_acts((3, cin, 7, 7), seed=4)
    wt = _weights('int', 64, cin, k, tr, seed=2)
    rw = _rw()
    _run(x, wt, None, k, s, tr, 'leaky', x_ld=x_ld, rw=rw)
    assert int(rw.item()) == 0
    x1 = x.clone()
    x1[0, 0, 0, 0] = 1023.0                         # 65472 after scaling: inside
    _run(x1, wt, None, k, s, tr, 'leaky', x_ld=x_ld, rw=rw)
    assert int(rw.item()) == 0
    for value, where in ((2000.0, (0, 0, 0, 0)), (float('nan'), (1, 100, 3, 4)), (float('inf'), (2, cin - 1, 6, 6)),
                         (-1024.0, (2, 193, 0, 6))):
        xb = x.clone()
        xb[where] = value
        rw = _rw()
        _run(xb, wt, None, k, s, tr, 'leaky', x_ld=x_ld, rw=rw)
        assert int(rw.item()) > 0, (value, where)


def _tfn(channels_last=True, fused=True):
    from rmnet_amd import networks
    from rmnet_amd.tiny_flownet import TinyFlowNet
    net = networks.procedural_init_(TinyFlowNet(None)).to(dev()).eval()
    if fused:
        net.fuse_epilogues()
    if channels_last:
        net = net.to(memory_format=torch.channels_last)
    return net


def _bits(t):
    return t.contiguous().view(torch.int32)


def _library_reproducible():
    """The library's convolutions in their deterministic mode.  With its default solvers two runs of the SAME network on the SAME clip
    differ in the last bits (measured on an MI355X: the output of two consecutive RMNET_FLOW_CONV=miopen runs was not torch.equal),
    so 'bit for bit what the library path returns' can only be asked with reproducible solvers on both sides."""
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


@pytest.mark.gpu
def test_a_clip_outside_the_window_is_redone_on_the_library(monkeypatch):
    """A frame with a 1e6 pixel drives conv1's output past 1023.5: ``forward`` sees the range word, recomputes the clip with the
    kernel off and returns bit for bit what RMNET_FLOW_CONV=miopen returns; ``last_clip`` says so.  A clean clip stays on the
    kernel."""
    net = _tfn()
    g = torch.Generator().manual_seed(3)
    frames = torch.rand(1, 3, 3, 64, 128, generator=g).to(dev())
    monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
    with torch.no_grad():
        net(frames)
    assert net.last_clip == {'flow_conv': 'split', 'range': 0}
    frames[0, 1, 1, 20, 30] = 1e6
    with torch.no_grad(), _library_reproducible():
        monkeypatch.setenv('RMNET_FLOW_CONV', 'miopen')
        first = net(frames)
        monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
        got = net(frames)
        assert net.last_clip['flow_conv'] == 'miopen' and net.last_clip['range'] > 0
        monkeypatch.setenv('RMNET_FLOW_CONV', 'miopen')
        want = net(frames)
        assert net.last_clip == {'flow_conv': 'miopen', 'range': 0}
    print('library run to run: first == second %s; largest |flow| %.3e' % (torch.equal(_bits(first), _bits(want)), float(want.abs().max())))
    assert torch.equal(_bits(got), _bits(want))


# ================================================================================================ GPU: the C entry
@pytest.mark.gpu
def test_the_c_entry_rejects_what_it_does_not_implement():
    """Every argument rule of rmnet_flow_conv_f32 with its code, the sentinel output untouched, and one positive control."""
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    INVALID, UNSUPPORTED = -1, -4
    n, h, w, cin, cout = 1, 5, 7, 64, 64
    x = _buffer(R.int_acts((n, cin, h, w), seed=1), 96)
    wt = R.int_weights(cout, cin, 3, seed=2)
    wp, wu = (t.to(dev()) for t in ops.flow_conv_pack(wt))
    wpt, wut = (t.to(dev()) for t in ops.flow_conv_pack(wt.permute(1, 0, 2, 3).contiguous().repeat(1, 1, 2, 2)[:, :, :4, :4], transposed=True))
    shift = torch.zeros(cout, device=dev())
    out = torch.full((n, 2 * h, 2 * w, 128), -7.25, device=dev())           # large enough for every case below
    rw = _rw()
    big = torch.empty(4 * 5 * 7 * 96 + 64, device=dev())                    # for the overlap cases

    def call(x_=x.data_ptr(), x_ld=96, wp_=wp.data_ptr(), wu_=wu.data_ptr(), sh=shift.data_ptr(), flags=ops.FLOW_LEAKY, N=n, H=h, W=w,
             Cin=cin, Cout=cout, k=3, s=1, out_=out.data_ptr(), out_ld=128, coff=0):
        return lib.rmnet_flow_conv_f32(x_, x_ld, wp_, wu_, sh, flags, N, H, W, Cin, Cout, k, s, out_, out_ld, coff, rw.data_ptr(),
                                       torch.cuda.current_stream(dev()).cuda_stream)

    cases = [
        ('null x', dict(x_=None), INVALID), ('null wpack', dict(wp_=None), INVALID), ('null w_unscale', dict(wu_=None), INVALID),
        ('null out', dict(out_=None), INVALID), ('N = 0', dict(N=0), INVALID), ('Cin = 0', dict(Cin=0), INVALID),
        ('x misaligned', dict(x_=x.data_ptr() + 4), INVALID), ('out misaligned', dict(out_=out.data_ptr() + 8), INVALID),
        ('shift misaligned', dict(sh=shift.data_ptr() + 4), INVALID), ('wpack misaligned', dict(wp_=wp.data_ptr() + 2), INVALID),
        ('unknown flag', dict(flags=8), INVALID), ('two activations', dict(flags=ops.FLOW_RELU | ops.FLOW_LEAKY), INVALID),
        ('ksize 1', dict(k=1), UNSUPPORTED), ('ksize 7', dict(k=7), UNSUPPORTED), ('ksize 4 forward', dict(k=4, s=2), UNSUPPORTED),
        ('stride 3', dict(s=3), UNSUPPORTED), ('stride 0', dict(s=0), UNSUPPORTED),
        ('transposed ksize 3', dict(flags=ops.FLOW_TRANSPOSED, k=3, s=2), UNSUPPORTED),
        ('transposed stride 1', dict(flags=ops.FLOW_TRANSPOSED, k=4, s=1), UNSUPPORTED),
        ('Cout 32', dict(Cout=32), UNSUPPORTED), ('Cout 96', dict(Cout=96), UNSUPPORTED),
        ('x_ld % 4', dict(x_ld=66), INVALID), ('x_ld < ceil32(Cin)', dict(Cin=70, x_ld=92), INVALID), ('x_ld < Cin', dict(x_ld=32), INVALID),
        ('out_ld % 4', dict(out_ld=126), INVALID), ('coff % 4', dict(coff=2), INVALID), ('coff < 0', dict(coff=-4), INVALID),
        ('coff + Cout > out_ld', dict(coff=68), INVALID),
        ('input index range', dict(N=8, H=4096, W=4096, x_ld=32, Cin=32), UNSUPPORTED),
        ('output index range', dict(flags=ops.FLOW_TRANSPOSED | ops.FLOW_LEAKY, k=4, s=2, N=4, H=1024, W=1024, x_ld=64, wp_=wpt.data_ptr(),
                                    wu_=wut.data_ptr()), UNSUPPORTED),
        ('out inside x', dict(x_=big.data_ptr(), N=4, out_=big.data_ptr() + 4 * 5 * 7 * 96 * 4 - 64), INVALID),
        ('x inside out', dict(x_=out.data_ptr() + 1024), INVALID),
    ]
    for name, kw, code in cases:
        assert call(**kw) == code, name
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and int(rw.item()) == 0
    # positive controls: the same arguments unchanged, forward and transposed
    assert call() == 0
    want = FR.activate(FR.reference(x[:, :cin].cpu(), wt, None, 3, 1, False), 'leaky')
    _assert_equal(out.view(-1)[:n * h * w * 128].view(n, h, w, 128)[..., :cout].permute(0, 3, 1, 2), want, 'positive control')
    assert call(flags=ops.FLOW_TRANSPOSED, k=4, s=2, wp_=wpt.data_ptr(), wu_=wut.data_ptr(), coff=64) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool((out[..., 64:] != -7.25).any())


def test_the_wrapper_rejects_what_the_kernel_would():
    """The Python-side checks, before any launch (CPU tensors are the first of them)."""
    from rmnet_amd import ops
    wp, wu = ops.flow_conv_pack(R.int_weights(64, 32, 3, seed=1))
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.flow_conv(torch.zeros(1, 32, 4, 4).contiguous(memory_format=torch.channels_last), wp, wu)
    with pytest.raises(RuntimeError):
        ops.flow_conv_pack(torch.zeros(64, 32, 7, 7))
    with pytest.raises(RuntimeError):
        ops.flow_conv_pack(torch.zeros(64, 32, 3, 3), transposed=True)
    with pytest.raises(RuntimeError):
        ops.flow_conv_pack(torch.zeros(32, 32, 3, 3))
    with pytest.raises(RuntimeError):
        ops.flow_conv_pack(torch.zeros(64, 32, 3, 3, dtype=torch.float64))


@pytest.mark.gpu
def test_the_wrapper_checks_shapes_before_it_launches():
    from rmnet_amd import ops
    wp, wu = (t.to(dev()) for t in ops.flow_conv_pack(R.int_weights(64, 64, 3, seed=1)))
    x = _buffer(R.int_acts((1, 64, 5, 7), seed=1), 64)
    for kw in (dict(ksize=1), dict(stride=3), dict(transposed=True), dict(act='gelu'), dict(cin=70), dict(cin=32),
               dict(out=torch.empty(1, 64, 5, 6, device=dev()).contiguous(memory_format=torch.channels_last)),
               dict(out=torch.empty(1, 96, 5, 7, device=dev()).contiguous(memory_format=torch.channels_last), out_coff=64),
               dict(out=torch.empty(1, 96, 5, 7, device=dev()), out_coff=0), dict(out_coff=4),
               dict(range_word=torch.zeros(1, device=dev()))):
        with pytest.raises(RuntimeError):
            ops.flow_conv(x, wp, wu, **dict(dict(ksize=3, stride=1), **kw))
    with pytest.raises(RuntimeError):
        ops.flow_conv(x.contiguous(), wp, wu, ksize=3)                    # NCHW
    assert ops.flow_conv(x, wp, wu, ksize=3).shape == (1, 64, 5, 7)


# ================================================================================================ GPU: the whole network
def _parent_forward(net, img0, img1):
    """TinyFlowNet._forward as it was before the kernel: the library's convolutions (with the fused bias + LeakyReLU pass of a
    fused network), three torch.cat."""
    from rmnet_amd.helpers import pad_divide_by
    (img0, img1), pad = pad_divide_by([img0, img1], 64, img0.shape[2:])
    pair = torch.cat((F.interpolate(img0, scale_factor=0.5, mode='bilinear'), F.interpolate(img1, scale_factor=0.5, mode='bilinear')), dim=1)
    run = net._fused_block if getattr(net, '_fused', False) and not net.training and pair.is_cuda else (lambda m, x: m(x))
    c2 = run(net.conv2, run(net.conv1, pair))
    c3 = run(net.conv3_1, run(net.conv3, c2))
    c4 = run(net.conv4_1, run(net.conv4, c3))
    c5 = run(net.conv5_1, run(net.conv5, c4))
    cat4 = torch.cat((c4, run(net.deconv4, c5), net.upsampled_flow5_to_4(net.predict_flow5(c5))), 1)
    cat3 = torch.cat((c3, run(net.deconv3, cat4), net.upsampled_flow4_to_3(net.predict_flow4(cat4))), 1)
    cat2 = torch.cat((c2, run(net.deconv2, cat3), net.upsampled_flow3_to_2(net.predict_flow3(cat3))), 1)
    flow = F.interpolate(net.predict_flow2(cat2), scale_factor=8, mode='bilinear')
    lw, uw, lh, uh = pad
    if lh + uh > 0:
        flow = flow[:, :, lh:flow.shape[2] - uh, :]
    if lw + uw > 0:
        flow = flow[:, :, :, lw:flow.shape[3] - uw]
    return flow


@pytest.fixture(scope='module')
def cpu_reference():
    """The same network on the CPU in float64, for the two clips of the whole-network test: computed once."""
    from rmnet_amd import networks
    from rmnet_amd.tiny_flownet import TinyFlowNet
    net = networks.procedural_init_(TinyFlowNet(None)).eval().double()
    out = {}
    for shape in ((2, 3, 3, 64, 128), (1, 2, 3, 70, 100)):
        frames = torch.rand(shape, generator=torch.Generator().manual_seed(shape[3]))
        with torch.no_grad():
            out[shape] = (frames, net(frames.double()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 3, 3, 64, 128), (1, 2, 3, 70, 100)])
def test_the_network_on_the_kernel_is_as_close_to_float64_as_on_the_library(shape, cpu_reference, monkeypatch):
    """Frames 2x3x64x128 (maps down to 1x2 at conv5) and 1x2x70x100 (padded to 128x128, un-padded again): both paths against the
    float64 CPU network; the split path's largest error may be at most 4x the library path's, on the same inputs (both are
    fp32-class with different summation orders).

    Measured on an MI355X (profiles/r13_a_flow_conv.md): split 2.429e-06 and 1.79e-06 - 1.84e-06 against the library's
    7.16e-07 - 7.48e-07 and 6.74e-07 (ratios 3.2 - 3.4 and 2.7).  The library's figure differs from run to run, its solvers are
    not reproducible.  With the hi*hi products summed in ONE accumulator level the kernel was at 3.216e-06 (ratio 3.7 - 4.3: over
    the bound in some runs); the two levels of csrc/flow_conv.hip are there for this test."""
    net = _tfn()
    frames, ref = cpu_reference[shape]
    errs = {}
    for mode in ('miopen', 'split'):
        monkeypatch.setenv('RMNET_FLOW_CONV', mode)
        with torch.no_grad():
            got = net(frames.to(dev()))
        assert net.last_clip == {'flow_conv': mode, 'range': 0}
        errs[mode] = float((got.cpu().double() - ref).abs().max())
    print('%s: max |flow - float64| miopen %.3e split %.3e (largest |flow| %.3e)' % (shape, errs['miopen'], errs['split'], float(ref.abs().max())))
    assert errs['split'] <= 4 * errs['miopen'], errs


@pytest.mark.gpu
def test_the_golden_flows_through_the_kernel(golden_dir, monkeypatch):
    """tests/golden/tiny_flownet.npz through the split path, at test_tiny_flownet_on_gpu's tolerances."""
    g = np.load(os.path.join(golden_dir, 'tiny_flownet.npz'))
    net = _tfn()
    monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
    with torch.no_grad():
        fl = net(torch.from_numpy(g['frames']).to(dev()))
    assert net.last_clip == {'flow_conv': 'split', 'range': 0}
    np.testing.assert_allclose(fl.cpu().numpy(), g['flows'], atol=2e-3, rtol=1e-3)


class _Calls:
    """Counts the F.conv2d / F.conv_transpose2d calls by output channels."""

    def __init__(self, monkeypatch):
        self.seen = []
        for name, co in (('conv2d', 0), ('conv_transpose2d', 1)):
            real = getattr(F, name)

            def wrapped(x, weight, *a, _real=real, _name=name, _co=co, **k):
                self.seen.append((_name, weight.shape[_co]))
                return _real(x, weight, *a, **k)
            monkeypatch.setattr(F, name, wrapped)

    def wide(self):
        return sorted(c for c in self.seen if c[1] >= 64)


@pytest.mark.gpu
def test_the_switch_selects_the_path(monkeypatch):
    """RMNET_FLOW_CONV=miopen, an NCHW network, a network that is not fused: bit for bit the path as it was (restated above; with
    the library's reproducible solvers on both sides, see ``_library_reproducible``).
    With split on a fused channels-last network the ten wide layers issue no F.conv2d / F.conv_transpose2d: what is left is
    conv1, the four flow heads and the three 2 -> 2 upsamplers."""
    g = torch.Generator().manual_seed(11)
    a, b = (torch.rand(2, 3, 64, 128, generator=g).to(dev()) for _ in range(2))
    net = _tfn()
    nchw = _tfn(channels_last=False)
    plain = _tfn(fused=False)
    with torch.no_grad(), _library_reproducible():
        monkeypatch.setenv('RMNET_FLOW_CONV', 'miopen')
        want = _parent_forward(net, a, b)
        assert torch.equal(_bits(net._forward(a, b)), _bits(want))
        monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
        for other in (nchw, plain):
            calls = _Calls(monkeypatch)
            got = other._forward(a, b)
            assert len(calls.wide()) == 11, calls.seen
            monkeypatch.undo()
            monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
            assert torch.equal(_bits(got), _bits(_parent_forward(other, a, b)))
        calls = _Calls(monkeypatch)
        got = net._forward(a, b)
        seen = list(calls.seen)
        monkeypatch.undo()
        assert [c for c in seen if c[1] >= 64] == [('conv2d', 64)], seen            # conv1 alone
        assert sorted(seen) == [('conv2d', 2)] * 4 + [('conv2d', 64)] + [('conv_transpose2d', 2)] * 3, seen
        net.train()
        monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
        calls = _Calls(monkeypatch)
        net._forward(a, b)
        assert len(calls.wide()) == 11                                              # (training mode: the module graph)
        monkeypatch.undo()
    assert float((got - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))


@pytest.mark.gpu
def test_the_split_path_is_captured_and_replayed(monkeypatch):
    """``_forward`` on the kernel has no host synchronisation and no frame-dependent argument: captured once into a HIP graph (one
    stream, as bench.py does it) and replayed on other frames, it returns what the eager call returns on those frames -- to the
    library's own run-to-run difference in conv1 and the flow heads, far below the 1e-4 asked here -- and the range word stays
    zero."""
    net = _tfn()
    monkeypatch.setenv('RMNET_FLOW_CONV', 'split')
    g = torch.Generator().manual_seed(5)
    clips = [torch.rand(2, 3, 64, 128, generator=g).to(dev()) for _ in range(4)]
    s_a, s_b = clips[0].clone(), clips[1].clone()
    net.flow_range_word(dev()).zero_()
    with torch.no_grad():
        side = torch.cuda.Stream(dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            for _ in range(2):
                net._forward(s_a, s_b)
        torch.cuda.current_stream(dev()).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s_out = net._forward(s_a, s_b)
        for a, b in ((clips[2], clips[3]), (clips[1], clips[0])):
            s_a.copy_(a)
            s_b.copy_(b)
            graph.replay()
            got = s_out.clone()
            want = net._forward(a, b)
            assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    assert net.flow_range_count() == 0
