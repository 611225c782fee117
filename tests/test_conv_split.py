# -*- coding: utf-8 -*-
"""The general split-fp16 convolution of the trunks and key / value heads (csrc/conv_split.hip, rmnet_conv_split_f32): code object,
weight pack with folded BatchNorm, which convolutions take it, accuracy per shape class against fp64 next to MIOpen fp32, whole
bottleneck blocks and heads against a float64 restatement, the range word and the clip redo."""

import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import conv_ref

SRC = os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv_split.hip')


def _tool(name):
    for d in ('/opt/rocm/llvm/bin', '/opt/rocm/bin'):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    pytest.fail('%s not found' % name)


def test_code_object_uses_f16_mfma_and_only_vector_memory_writes(tmp_path):
    """Compile-only gfx950 build: the three tile shapes' f16 MFMAs in the code object, no scalar-unit store / atomic / cache opcodes."""
    from rmnet_amd import build
    co = str(tmp_path / 'conv_split.co')
    subprocess.check_call([build.hipcc_path(), '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only',
                           '--no-gpu-bundle-output', '-c', SRC, '-o', co])
    text = subprocess.check_output([_tool('llvm-objdump'), '-d', '--mcpu=gfx950', co]).decode()
    ops_ = re.findall(r'^\s+([a-z_][a-z0-9_]*)\b', text, flags=re.M)
    assert ops_.count('v_mfma_f32_16x16x32_f16') >= 48 + 24 + 12, 'expected one K step of each tile shape (4x4x3, 4x2x3, 2x2x3)'
    forbidden = tuple(p + '_' for p in ('s' + '_store', 's' + '_buffer_store', 's' + '_scratch_store', 's' + '_atomic',
                                        's' + '_buffer_atomic')) + ('s' + '_dcache_wb', 's' + '_dcache_discard')
    bad = sorted({o for o in ops_ if o.startswith(forbidden) or o in forbidden})
    assert not bad, bad


def _weights(cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    std = 0.9 * (2.0 / (k * k * cin)) ** 0.5
    return ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (std * 3 ** 0.5)).float()


def _unpack(wp, wu, cout, cin, k):
    """The pack back to [Cout, Cin, k, k] float64 (hi + lo, unscaled), straight from the documented layout."""
    return conv_ref.unpack_conv_weights(wp, wu, cout, cin, k)


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('cout', [64, 128, 256, 512, 1024])
def test_pack_reproduces_the_weights_times_the_bn_scale(k, cout):
    """hi + lo, unscaled, is w * bn_scale (the product in float64) to 2^-21 relative per element (plus half a subnormal step of the
    scaled lo plane); the scale is a power of two that puts max |w * bn_scale| in [2^14, 2^15)."""
    from rmnet_amd import ops
    cin = 64
    w = _weights(cout, cin, k, seed=cout + k)
    w[3] *= 1e-3
    w[5] = 0.0
    g = torch.Generator().manual_seed(cout)
    bn = (torch.rand(cout, generator=g) * 0.4 + 0.8).float()
    wp, wu = ops.conv_split_pack(w, bn)
    assert wp.dtype == torch.int16 and wp.numel() == k * k * cin * cout * 2 and wu.shape == (cout,) and wu.dtype == torch.float32
    m, _ = torch.frexp(wu)
    assert bool((m == 0.5).all())
    want = w.double() * bn.double().view(-1, 1, 1, 1)
    scaled = want.abs().amax(dim=(1, 2, 3)) / wu.double()
    live = scaled > 0
    assert bool(((scaled[live] >= 2 ** 14) & (scaled[live] < 2 ** 15)).all())
    back = _unpack(wp, wu, cout, cin, k)
    err = (back - want).abs()
    bound = 2.0 ** -21 * want.abs() + 2.0 ** -25 * wu.double().view(-1, 1, 1, 1)
    assert bool((err <= bound).all()), float((err / (bound + 1e-300)).max())
    assert float(back[5].abs().max()) == 0.0
    if k == 3 and cout == 256:              # without a scale: the decoder kernel's pack, bit for bit
        wp3, wu3 = ops.conv3x3_pack(w)
        wp0, wu0 = ops.conv_split_pack(w)
        assert torch.equal(wp0, wp3) and torch.equal(wu0, wu3)


def test_the_trunks_and_heads_take_the_split_kernel():
    """fuse_epilogues(): every bottleneck convolution of both trunks (conv1-3 and the projections) and both KeyValue heads carry a
    pack; the stems (Cin 3 / 5, 7x7) and the decoder stay off this kernel."""
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    net = networks.procedural_init_(RMNet(None)).eval()
    net.fuse_epilogues()
    blocks = [m for m in net.modules() if isinstance(m, networks._Bottleneck)]
    heads = [m for m in net.modules() if isinstance(m, networks.KeyValue)]
    assert len(blocks) == 2 * (3 + 4 + 6) and len(heads) == 2
    assert all(m._conv_split for m in blocks + heads)
    convs = sum(3 + (m.downsample is not None) for m in blocks)
    assert convs == 2 * (13 * 3 + 3)
    for m in blocks:
        for name, c in (('1', m.conv1), ('2', m.conv2), ('3', m.conv3)) + ((('d', m.downsample[0]),) if m.downsample is not None else ()):
            assert networks.split_eligible(c)
            assert getattr(m, '_wp' + name).numel() == c.weight.numel() * 2
    for kv in heads:
        assert kv._wu.numel() == 128 + 512 and kv._bkv.numel() == 640
    for enc in (net.encoder_memory, net.encoder_query):
        assert not networks.split_eligible(enc.conv1)
    assert not networks.split_eligible(net.decoder.pred2)
    prev = networks.set_split_conv_(net, False)
    assert not any(m._conv_split for m in blocks + heads)
    networks.restore_split_conv_(prev)
    assert all(m._conv_split for m in blocks + heads)
    x = torch.randn(1, 256, 8, 8)
    assert not networks._split_path_ok(blocks[3], x, blocks[3].conv1, ('split',))      # CPU input: the module graph


# ---------------------------------------------------------------------------------------------------------- GPU
def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


# (Cin, Cout, k, stride, N, H, W): one case per shape class and tile (Narrow 128 x 64, Mid 128 x 128, Big 128 x 256)
CASES = [(256, 64, 1, 1, 2, 60, 108), (64, 64, 3, 1, 2, 60, 108), (256, 512, 1, 2, 2, 60, 108), (128, 128, 3, 2, 2, 60, 108),
         (64, 1024, 1, 1, 2, 64, 128), (64, 256, 3, 2, 2, 128, 256), (1024, 640, 3, 1, 2, 30, 54)]


@pytest.mark.gpu
@pytest.mark.parametrize('cin,cout,k,s,n,h,w', CASES)
def test_matches_fp64_as_well_as_miopen(cin, cout, k, s, n, h, w):
    """Batch 2, folded scale + shift + skip + ReLU: max abs error against fp64 within 2x that of MIOpen fp32 on the same inputs."""
    from rmnet_amd import ops
    torch.backends.cudnn.benchmark = False
    g = torch.Generator().manual_seed(cin + cout + k + s)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = _weights(cout, cin, k, seed=cout)
    sc = (torch.rand(cout, generator=g) * 0.4 + 0.8).float()
    sh = ((torch.rand(cout, generator=g) * 2 - 1) * 0.05).float()
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    res = torch.randn(n, cout, ho, wo, generator=g)
    xg, rg = _cl(x), _cl(res)
    want = F.relu(F.conv2d(xg.double(), wt.double().to(dev()), None, s, k // 2) * sc.double().to(dev()).view(1, -1, 1, 1)
                  + sh.double().to(dev()).view(1, -1, 1, 1) + rg.double())
    wp, wu = ops.conv_split_pack(wt.to(dev()), sc.to(dev()))
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    got = ops.conv_split(xg, wp, wu, sh.to(dev()), rg, ksize=k, stride=s, relu_out=True, range_word=rw)
    ref = F.relu(F.conv2d(xg, _cl(wt), None, s, k // 2) * sc.to(dev()).view(1, -1, 1, 1) + sh.to(dev()).view(1, -1, 1, 1) + rg)
    assert int(rw.item()) == 0
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    es = float((got.double() - want).abs().max())
    em = float((ref.double() - want).abs().max())
    print('cin %d cout %d %dx%d/s%d %dx%d: split %.3e  miopen %.3e' % (cin, cout, k, k, s, h, w, es, em))
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
def test_range_word_counts_each_read_element_once():
    """3x3 / stride 2 on an odd and an even map: each out-of-window element counted once wherever it sits (even / odd rows and
    columns, the last row / column), also when Cout spans several workgroup tiles (640 = 5 Mid tiles, 1024 = 8); 1x1 / stride 2
    never reads the odd rows and columns, and does not count them."""
    from rmnet_amd import ops
    for h, w in ((13, 20), (12, 19)):
        x = torch.randn(2, 64, h, w, generator=torch.Generator().manual_seed(h))
        spots = [(0, 3, 0, 0), (0, 5, 1, 1), (1, 7, 2, 3), (1, 9, h - 1, w - 1), (0, 11, h - 2, w - 1), (1, 13, 5, 0)]
        for b, c, i, j in spots:
            x[b, c, i, j] = 5e3
        x[1, 17, 4, 6] = float('nan')
        xg = _cl(x)
        for k, s, cout, want in ((3, 2, 128, len(spots) + 1), (3, 1, 128, len(spots) + 1), (3, 1, 640, len(spots) + 1),
                                 (1, 1, 1024, len(spots) + 1), (1, 2, 64, sum(1 for _, _, i, j in spots if i % 2 == 0 and j % 2 == 0) + 1)):
            wp, wu = ops.conv_split_pack(_weights(cout, 64, k, seed=k).to(dev()))
            rw = torch.zeros(1, dtype=torch.int32, device=dev())
            ops.conv_split(xg, wp, wu, ksize=k, stride=s, range_word=rw)
            assert int(rw.item()) == want, (h, w, k, s, cout, int(rw.item()), want)


def _bn_(m, g):
    for bn in m.modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            bn.running_mean.copy_((torch.rand(bn.num_features, generator=g) - 0.5) * 0.2)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 0.45 + 0.8)
            bn.weight.data.copy_(torch.rand(bn.num_features, generator=g) * 0.4 + 0.8)
            bn.bias.data.copy_((torch.rand(bn.num_features, generator=g) - 0.5) * 0.2)


def _block64(sd, p, x, stride, project):
    """A bottleneck block restated in float64 from its state dict with plain F.conv2d / F.batch_norm."""
    def bn(t, q):
        return F.batch_norm(t, sd[q + '.running_mean'].double(), sd[q + '.running_var'].double(), sd[q + '.weight'].double(),
                            sd[q + '.bias'].double(), False, 0.0, 1e-5)
    t = F.relu(bn(F.conv2d(x, sd[p + 'conv1.weight'].double()), p + 'bn1'))
    t = F.relu(bn(F.conv2d(t, sd[p + 'conv2.weight'].double(), None, stride, 1), p + 'bn2'))
    t = bn(F.conv2d(t, sd[p + 'conv3.weight'].double()), p + 'bn3')
    skip = bn(F.conv2d(x, sd[p + 'downsample.0.weight'].double(), None, stride), p + 'downsample.1') if project else x
    return F.relu(t + skip)


@pytest.mark.gpu
@pytest.mark.parametrize('c_in,width,stride,project', [(256, 128, 2, True), (512, 128, 1, False), (64, 64, 1, True)])
def test_whole_bottleneck_blocks_match_a_float64_restatement(c_in, width, stride, project, monkeypatch):
    """Identity and projection blocks on the split path (channels-last, fused epilogues) against float64 F.conv2d / F.batch_norm of
    the state dict, within 2x the error of the same block on MIOpen (RMNET_CONV=decoder); every convolution went to the kernel."""
    from rmnet_amd import networks, ops
    torch.backends.cudnn.benchmark = False
    g = torch.Generator().manual_seed(c_in + width)
    blk = networks.procedural_init_(networks._Bottleneck(c_in, width, stride, project))
    with torch.no_grad():
        _bn_(blk, g)
    blk = blk.to(dev()).eval()
    networks.fuse_epilogues_(blk)
    blk = blk.to(memory_format=torch.channels_last)
    x = _cl(F.relu(torch.randn(2, c_in, 40, 72, generator=g)))
    sd = {k: v.to(dev()) for k, v in blk.state_dict().items()}
    want = _block64(sd, '', x.double(), stride, project)
    calls = []
    real = ops.conv_split
    monkeypatch.setattr(ops, 'conv_split', lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        got = blk(x)
        assert len(calls) == 3 + project
        monkeypatch.setenv('RMNET_CONV', 'decoder')
        ref = blk(x)
        assert len(calls) == 3 + project
    es, em = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
    print('block %d/%d/s%d: split %.3e  miopen %.3e' % (c_in, width, stride, es, em))
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
def test_key_value_heads_match_a_float64_restatement(monkeypatch):
    """Both heads in one launch, written as two dense tensors; they equal float64 F.conv2d within 2x MIOpen fp32's error."""
    from rmnet_amd import networks, ops
    torch.backends.cudnn.benchmark = False
    kv = networks.procedural_init_(networks.KeyValue(1024, 128, 512)).to(dev()).eval()
    networks.fuse_epilogues_(kv)
    kv = kv.to(memory_format=torch.channels_last)
    x = _cl(F.relu(torch.randn(2, 1024, 30, 54, generator=torch.Generator().manual_seed(5))))
    calls = []
    real = ops.conv_split
    monkeypatch.setattr(ops, 'conv_split', lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        k4, v4 = kv(x)
        assert len(calls) == 1 and k4.shape == (2, 128, 30, 54) and v4.shape == (2, 512, 30, 54)
        assert k4.is_contiguous(memory_format=torch.channels_last) and v4.is_contiguous(memory_format=torch.channels_last)
        monkeypatch.setenv('RMNET_CONV', 'decoder')
        rk, rv = kv(x)
        assert len(calls) == 1
    for got, ref, c in ((k4, rk, kv.key_conv), (v4, rv, kv.value_conv)):
        want = F.conv2d(x.double(), c.weight.double(), c.bias.double(), 1, 1)
        es, em = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
        assert es <= 2 * em, (es, em)


@pytest.mark.gpu
def test_forward_redoes_the_clip_on_miopen_when_an_encoder_activation_leaves_the_window(monkeypatch):
    """An activation beyond |x| < 1023.5 inside a trunk (the stem's BatchNorm shift + 3000 feeds layer1): forward() sees the range
    word, redoes the clip with every split convolution off, and returns what RMNET_CONV=miopen computes."""
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    torch.backends.cudnn.benchmark = False
    net = networks.procedural_init_(RMNet(None)).to(dev()).eval()
    with torch.no_grad():
        net.encoder_query.bn1.bias.add_(3000.0)
    net.fuse_epilogues()
    net = net.to(memory_format=torch.channels_last)
    frames, masks, flows, n_objects = synthetic_clip(3, 2, 96, 160, seed=4)
    with torch.no_grad():
        est = net(frames, masks, flows, n_objects, 2)
        assert (net.last_clip['reread'] or '').startswith('miopen'), net.last_clip
        monkeypatch.setenv('RMNET_CONV', 'miopen')
        ref = net(frames, masks, flows, n_objects, 2)
        assert not (net.last_clip['reread'] or '').startswith('miopen')      # (the bank's own exact re-read may follow: values are large)
    assert torch.equal(est, ref)
