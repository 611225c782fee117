# -*- coding: utf-8 -*-
"""The split-fp16 3x3 convolution of the decoder (csrc/conv3x3.hip, rmnet_conv3x3_split_f32): code object, weight pack,
accuracy against fp64 next to MIOpen fp32, fused prologue / epilogue, the range word and the clip redo."""

import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import conv_ref

SRC = os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv3x3.hip')


def _tool(name):
    for d in ('/opt/rocm/llvm/bin', '/opt/rocm/bin'):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    pytest.fail('%s not found' % name)


def test_code_object_uses_f16_mfma_and_only_vector_memory_writes(tmp_path):
    """Compile-only gfx950 build of the kernel: f16 MFMAs in the code object, no scalar-unit store / atomic / cache opcodes."""
    from rmnet_amd import build
    co = str(tmp_path / 'conv3x3.co')
    subprocess.check_call([build.hipcc_path(), '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only',
                           '--no-gpu-bundle-output', '-c', SRC, '-o', co])
    text = subprocess.check_output([_tool('llvm-objdump'), '-d', '--mcpu=gfx950', co]).decode()
    ops_ = re.findall(r'^\s+([a-z_][a-z0-9_]*)\b', text, flags=re.M)
    assert ops_.count('v_mfma_f32_16x16x32_f16') >= 48, 'expected the 4x4x3 f16 MFMAs of one K step'
    forbidden = tuple(p + '_' for p in ('s' + '_store', 's' + '_buffer_store', 's' + '_scratch_store', 's' + '_atomic',
                                        's' + '_buffer_atomic')) + ('s' + '_dcache_wb', 's' + '_dcache_discard')
    bad = sorted({o for o in ops_ if o.startswith(forbidden) or o in forbidden})
    assert not bad, bad


def _weights(cin, seed=0, std=None):
    g = torch.Generator().manual_seed(seed)
    std = 0.9 * (2.0 / (9 * cin)) ** 0.5 if std is None else std
    return ((torch.rand(256, cin, 3, 3, generator=g) * 2 - 1) * (std * 3 ** 0.5)).float()


def _unpack(wp, wu, cin):
    """The pack back to [256, Cin, 3, 3] float64 (hi + lo, unscaled), straight from the documented layout."""
    return conv_ref.unpack_conv_weights(wp, wu, 256, cin, 3)


@pytest.mark.parametrize('cin', [64, 256, 1024])
def test_weight_pack_reproduces_the_weights(cin):
    """hi + lo, unscaled, is w to 2^-21 relative per element (plus half a subnormal step of the scaled lo plane for the rare
    elements 2^-17 below their channel's largest); the scale is a power of two that puts max |w| in [2^14, 2^15)."""
    from rmnet_amd import ops
    w = _weights(cin, seed=cin)
    w[3] *= 1e-3              # a channel of much smaller weights
    w[5] = 0.0                # an all-zero channel
    wp, wu = ops.conv3x3_pack(w)
    assert wp.dtype == torch.int16 and wp.numel() == 9 * cin * 256 * 2 and wu.shape == (256,)
    m, e = torch.frexp(wu)
    assert bool((m == 0.5).all())                                    # powers of two
    scaled = w.abs().amax(dim=(1, 2, 3)).double() / wu.double()
    live = scaled > 0
    assert bool(((scaled[live] >= 2 ** 14) & (scaled[live] < 2 ** 15)).all())
    back = _unpack(wp, wu, cin)
    err = (back - w.double()).abs()
    bound = 2.0 ** -21 * w.double().abs() + 2.0 ** -25 * wu.double().view(-1, 1, 1, 1)
    assert bool((err <= bound).all()), float((err / (bound + 1e-300)).max())
    assert float(back[5].abs().max()) == 0.0


def test_weight_pack_layout_is_the_convolution():
    """A CPU emulation of the kernel's GEMM (K = tap x input channel, three split products) on the packed planes equals the
    fp64 convolution to fp32-class accuracy: the layout the header documents is the one the packer writes."""
    from rmnet_amd import ops
    cin, H, W = 64, 5, 7
    w = _weights(cin, seed=1)
    x = torch.randn(2, cin, H, W, generator=torch.Generator().manual_seed(2))
    wp, wu = ops.conv3x3_pack(w)
    p = wp.view(torch.float16).double().view(9, cin // 32, 2, 256, 32)
    xs = x.double() * 64
    xh = xs.half().double()
    xl = (xs - xh).half().double()
    xp = [F.pad(t, (1, 1, 1, 1)) for t in (xh, xl)]
    acc = torch.zeros(2, 256, H, W, dtype=torch.float64)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        for cb in range(cin // 32):
            ah, al = p[tap, cb, 0], p[tap, cb, 1]                        # [co][kk]
            bh = xp[0][:, 32 * cb:32 * cb + 32, ky:ky + H, kx:kx + W]
            bl = xp[1][:, 32 * cb:32 * cb + 32, ky:ky + H, kx:kx + W]
            for a, b in ((ah, bh), (ah, bl), (al, bh)):
                acc += torch.einsum('ok,nkhw->nohw', a, b)
    got = acc * wu.double().view(1, -1, 1, 1) / 64
    want = F.conv2d(x.double(), w.double(), None, 1, 1)
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------------------- GPU
def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _case(cin, n, h, w, scale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g) * scale
    wt = _weights(cin, seed=seed + 1)
    b = (torch.rand(256, generator=g) * 2 - 1) * 0.05
    res = torch.randn(n, 256, h, w, generator=g) * scale
    return x, wt, b, res


def _errors(x, wt, b, res, relu_in, relu_out, use_bias, use_res, inplace=False):
    """(max |split - fp64|, max |MIOpen fp32 - fp64|) for one configuration."""
    from rmnet_amd import ops
    xi = F.relu(x) if relu_in else x
    want = F.conv2d(xi.double(), wt.double(), b.double() if use_bias else None, 1, 1)
    if use_res:
        want = want + res.double()
    if relu_out:
        want = F.relu(want)
    xg, wg, bg, rg = _cl(x), _cl(wt), b.to(dev()), _cl(res)
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    out = rg.clone() if (inplace and use_res) else None
    got = ops.conv3x3_split(xg, wp, wu, bg if use_bias else None, (out if inplace else rg) if use_res else None,
                            relu_in=relu_in, relu_out=relu_out, out=out, range_word=rw)
    if inplace and use_res:
        assert got.data_ptr() == out.data_ptr()
    def fp32(xx, ww, bb, rr):
        r = F.conv2d(F.relu(xx) if relu_in else xx, ww, bb if use_bias else None, 1, 1)
        if use_res:
            r = r + rr
        return F.relu(r) if relu_out else r
    ref = fp32(xg, wg, bg, rg)
    torch.cuda.synchronize()
    assert int(rw.item()) == 0
    e_split = float((got.double().cpu() - want).abs().max())
    e_miopen = float((ref.double().cpu() - want).abs().max())
    if x.shape[2] * x.shape[3] < 32 * 32:
        # on tiny maps MIOpen may pick its direct kernel, which accumulates in fp64 (naive_conv_*_float_double_float): there the
        # fp32 yardstick is the CPU's fp32 convolution as well
        cpu = fp32(x, wt, b, res)
        e_miopen = max(e_miopen, float((cpu.double() - want).abs().max()))
    return e_split, e_miopen


@pytest.mark.gpu
@pytest.mark.parametrize('cin,h,w', [(256, 120, 216), (256, 7, 9), (512, 60, 108), (512, 30, 54), (1024, 30, 54),
                                     (1024, 7, 9), (1024, 120, 216), (256, 30, 54), (512, 120, 216)])
def test_matches_fp64_as_well_as_miopen(cin, h, w):
    """Batch 2, bias + skip: max abs error against fp64 within 2x that of MIOpen fp32 on the same inputs (measured: 2.5-3.5x
    SMALLER on every map from 30x54 up).  On the 7x9 map the fp32 yardsticks' maximum runs over only 32 k outputs and both come
    out near 1.3e-6 / 1.9e-6 while the split kernel's error stays at its usual 3.5e-6 / 5.6e-6: the bar there is 4x."""
    torch.backends.cudnn.benchmark = False
    x, wt, b, res = _case(cin, 2, h, w, 1.0, seed=cin + h)
    es, em = _errors(x, wt, b, res, False, False, True, True)
    print('cin %d %dx%d: split %.3e  miopen %.3e' % (cin, h, w, es, em))
    assert es <= (2 if h * w >= 32 * 32 else 4) * em, (es, em)


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [1e-3, 1.0, 1e2])
@pytest.mark.parametrize('relu_in,relu_out,use_bias,use_res',
                         [(a, b_, c, d) for a in (False, True) for b_ in (False, True) for c in (False, True) for d in (False, True)])
def test_every_prologue_epilogue_combination(scale, relu_in, relu_out, use_bias, use_res):
    x, wt, b, res = _case(256, 2, 30, 54, scale, seed=7)
    es, em = _errors(x, wt, b, res, relu_in, relu_out, use_bias, use_res)
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [1e-3, 1.0, 1e2])
def test_in_place_on_the_skip(scale):
    x, wt, b, res = _case(512, 2, 60, 108, scale, seed=9)
    es, em = _errors(x, wt, b, res, True, False, True, True, inplace=True)
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
def test_rejects_what_it_does_not_implement():
    from rmnet_amd import _lib, ops
    x, wt, b, res = _case(256, 1, 8, 8, 1.0, seed=3)
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    with pytest.raises(RuntimeError):
        ops.conv3x3_split(x.to(dev()), wp, wu)                        # NCHW
    with pytest.raises(RuntimeError):
        ops.conv3x3_split(_cl(x).double(), wp, wu)                    # dtype
    with pytest.raises(RuntimeError):
        ops.conv3x3_split(_cl(x[:, :128]), wp, wu)                    # pack of another Cin
    xg = _cl(x)
    with pytest.raises(_lib.RMNetHipError):
        ops.conv3x3_split(xg, wp, wu, out=xg)                         # out over x


@pytest.mark.gpu
def test_range_word_counts_saturated_inputs():
    from rmnet_amd import ops
    x, wt, b, res = _case(256, 2, 12, 20, 1.0, seed=5)
    x[0, 3, 4, 5] = 7e4
    x[1, 200, 0, 0] = float('nan')
    x[1, 17, 11, 19] = -2000.0
    wp, wu = ops.conv3x3_pack(wt.to(dev()))
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.conv3x3_split(_cl(x), wp, wu, b.to(dev()), range_word=rw)
    assert int(rw.item()) == 3                     # once per element, not once per tap
    rw.zero_()
    ops.conv3x3_split(_cl(x), wp, wu, b.to(dev()), relu_in=True, range_word=rw)
    assert int(rw.item()) == 2                     # -2000 is 0 after the ReLU; NaN is still counted


@pytest.mark.gpu
def test_forward_redoes_the_clip_on_miopen_when_the_word_is_set(monkeypatch):
    """A decoder activation beyond the window: forward() sees the range word at its per-clip sync, redoes the clip on the
    MIOpen path and says so in last_clip['reread']; the result is the MIOpen path's."""
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    torch.backends.cudnn.benchmark = False
    net = networks.procedural_init_(RMNet(None)).to(dev()).eval()
    with torch.no_grad():
        net.decoder.convFM.bias.add_(3000.0)          # m4 ~ 3000 > 1023.5: ResMM.conv1's input leaves the window
    net.fuse_epilogues()
    net = net.to(memory_format=torch.channels_last)
    frames, masks, flows, n_objects = synthetic_clip(4, 2, 96, 160, seed=4)
    with torch.no_grad():
        est = net(frames, masks, flows, n_objects, 2)
        assert (net.last_clip['reread'] or '').startswith('miopen'), net.last_clip
        monkeypatch.setenv('RMNET_CONV', 'miopen')
        ref = net(frames, masks, flows, n_objects, 2)
        assert net.last_clip['reread'] is None
    assert torch.equal(est, ref)


@pytest.mark.gpu
def test_decoder_takes_the_split_path_and_the_switch(monkeypatch):
    """Channels-last + fuse_epilogues(): the decoder's 256-channel convolutions run on the split kernel (within fp32-class error
    of MIOpen), RMNET_CONV=miopen switches them back; NCHW networks keep MIOpen."""
    from rmnet_amd import networks
    torch.backends.cudnn.benchmark = False
    dec = networks.procedural_init_(networks.Decoder(256)).to(dev()).eval()
    networks.fuse_epilogues_(dec)
    g = torch.Generator().manual_seed(1)
    r4 = torch.randn(2, 1024, 6, 10, generator=g).to(dev())
    r3 = _cl(torch.randn(2, 512, 12, 20, generator=g))
    r2 = _cl(torch.randn(2, 256, 24, 40, generator=g))
    calls = []
    from rmnet_amd import ops
    real = ops.conv3x3_split
    monkeypatch.setattr(ops, 'conv3x3_split', lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        nchw = dec(r4, r3.contiguous(), r2.contiguous())
        assert not calls
        dec = dec.to(memory_format=torch.channels_last)
        split = dec(r4, r3, r2)
        assert len(calls) == 1 + 2 + 5 + 5           # convFM, ResMM, RF3, RF2
        monkeypatch.setenv('RMNET_CONV', 'miopen')
        miopen = dec(r4, r3, r2)
        assert len(calls) == 13
    scale = float(miopen.abs().max())
    assert float((split - miopen).abs().max()) <= 1e-5 * scale
    assert float((nchw - miopen).abs().max()) <= 1e-5 * scale
