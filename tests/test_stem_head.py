# -*- coding: utf-8 -*-
"""The fused encoder stem (csrc/stem.hip, rmnet_stem_split_f32) and the decoder's prediction head (csrc/pred_head.hip,
rmnet_pred_head_f32): weight pack, wiring and switches, code object, accuracy against float64 next to the MIOpen path, the range
word, whole encoders / decoder and a whole clip against RMNET_CONV=trunk (the stems and the head on MIOpen).  The two kernels are
not the default path yet (networks.STEM_DEFAULT / HEAD_DEFAULT: unmeasured), so the network tests select them with RMNET_CONV=full."""

import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import conv_ref

SRC = os.path.join(ROOT, 'rmnet_amd', 'csrc', 'stem.hip')


def _tool(name):
    for d in ('/opt/rocm/llvm/bin', '/opt/rocm/bin'):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    pytest.fail('%s not found' % name)


def _weights(cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    std = 0.9 * (2.0 / (k * k * cin)) ** 0.5
    return ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (std * 3 ** 0.5)).float()


def _unpack(wp, wu, cin):
    """The stem pack back to ([64, Cin, 7, 7] float64 (hi + lo, unscaled), the K padding's planes), from the documented layout."""
    return conv_ref.unpack_stem_weights(wp, wu, cin)


@pytest.mark.parametrize('cin', [3, 5])
def test_stem_pack_reproduces_the_weights_times_the_bn_scale(cin):
    """hi + lo, unscaled, is w * bn_scale (the product in float64) to 2^-21 relative per element plus 2^-25 of the channel's unscale; the
    scale is a power of two that puts max |w * bn_scale| in [2^14, 2^15); a zero channel stays zero; the K padding is zero."""
    from rmnet_amd import ops
    w = _weights(64, cin, 7, seed=cin)
    w[3] *= 1e-3
    w[5] = 0.0
    bn = (torch.rand(64, generator=torch.Generator().manual_seed(cin)) * 0.4 + 0.8).float()
    wp, wu = ops.stem_pack(w, bn)
    kp = {3: 160, 5: 256}[cin]
    assert wp.dtype == torch.int16 and wp.numel() == kp * 64 * 2 and wu.shape == (64,) and wu.dtype == torch.float32
    m, _ = torch.frexp(wu)
    assert bool((m == 0.5).all())
    want = w.double() * bn.double().view(-1, 1, 1, 1)
    scaled = want.abs().amax(dim=(1, 2, 3)) / wu.double()
    live = scaled > 0
    assert int(live.sum()) == 63
    assert bool(((scaled[live] >= 2 ** 14) & (scaled[live] < 2 ** 15)).all())
    back, pad = _unpack(wp, wu, cin)
    err = (back - want).abs()
    bound = 2.0 ** -21 * want.abs() + 2.0 ** -25 * wu.double().view(-1, 1, 1, 1)
    assert bool((err <= bound).all()), float((err / (bound + 1e-300)).max())
    assert float(back[5].abs().max()) == 0.0
    assert pad.numel() == 64 * 2 * (kp - 49 * cin) and float(pad.abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        ops.stem_pack(_weights(64, 4, 7, seed=1))


def test_the_stems_and_the_head_are_wired_and_switched(monkeypatch):
    """fuse_epilogues(): both encoders carry a stem pack of the documented size (the memory encoder's is the pack of the three stacked
    weights) next to _s1 / _b1 / _w5, the decoder a flat copy of pred2's weight; set_split_conv_ / restore_split_conv_ toggle them with
    everything else; RMNET_CONV=trunk is a value, anything unknown still raises; a CPU input keeps the module graph."""
    from rmnet_amd import networks, ops
    from rmnet_amd.rmnet import RMNet
    net = networks.procedural_init_(RMNet(None)).eval()
    with torch.no_grad():
        _bn_(net.encoder_memory.bn1, torch.Generator().manual_seed(1))
    net.fuse_epilogues()
    em, eq, dec = net.encoder_memory, net.encoder_query, net.decoder
    assert eq._wp.dtype == torch.int16 and eq._wp.numel() == 160 * 64 * 2 and eq._wu.numel() == 64
    assert em._wp.numel() == 256 * 64 * 2 and em._wu.numel() == 64
    assert em._w5.shape == (64, 5, 7, 7) and em._s1.numel() == 64 and em._b1.numel() == 64 and eq._s1.numel() == 64
    w5 = torch.cat((em.conv1.weight, em.conv1_m.weight, em.conv1_o.weight), dim=1)
    wp, wu = ops.stem_pack(w5, networks._bn_scale64(em.bn1))
    assert torch.equal(em._wp, wp) and torch.equal(em._wu, wu)
    assert torch.equal(dec._wpred.view(dec.pred2.weight.shape), dec.pred2.weight)
    assert em._conv_split and eq._conv_split and dec._conv_split
    prev = networks.set_split_conv_(net, False)
    assert not (em._conv_split or eq._conv_split or dec._conv_split)
    networks.restore_split_conv_(prev)
    assert em._conv_split and eq._conv_split and dec._conv_split
    for v in ('trunk', 'full'):
        monkeypatch.setenv('RMNET_CONV', v)
        assert networks.split_conv_backend() == v
    monkeypatch.setenv('RMNET_CONV', 'stems')
    with pytest.raises(RuntimeError):
        networks.split_conv_backend()
    monkeypatch.delenv('RMNET_CONV')
    net = net.to(memory_format=torch.channels_last)
    monkeypatch.setenv('RMNET_CONV', 'full')
    assert not networks._split_path_ok(eq, torch.randn(1, 3, 32, 32), eq.conv1, networks._stem_backends())      # CPU input: the module graph
    assert not networks._pred_head_ok(dec, torch.randn(1, 256, 8, 8))
    with torch.no_grad():
        r4 = eq(torch.randn(1, 3, 32, 32))[0]
    assert r4.shape == (1, 1024, 2, 2)
    # the default takes a new kernel only where the switch says it was measured to win
    monkeypatch.delenv('RMNET_CONV')
    assert ('split' in networks._stem_backends()) == networks.STEM_DEFAULT


def test_stem_code_object_uses_f16_mfma_and_does_not_spill(tmp_path):
    """Compile-only gfx950 build of the stem: f16 MFMAs in the code object (both Cin variants: 4 channel tiles x 3 terms each), and
    the resource-usage remarks report no scratch and no spilled registers for either."""
    from rmnet_amd import build
    co = str(tmp_path / 'stem.co')
    r = subprocess.run([build.hipcc_path(), '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '--no-gpu-bundle-output',
                        '-Rpass-analysis=kernel-resource-usage', '-c', SRC, '-o', co], stderr=subprocess.PIPE, check=True)
    text = subprocess.check_output([_tool('llvm-objdump'), '-d', '--mcpu=gfx950', co]).decode()
    assert len(re.findall(r'^\s+v_mfma_f32_16x16x32_f16\b', text, flags=re.M)) >= 2 * 12
    remarks = r.stderr.decode()
    assert len(re.findall(r'Function Name: \S*stem_split', remarks)) == 2, remarks
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', remarks)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', remarks)]
    assert scratch == [0, 0] and spills == [0, 0], remarks


# ---------------------------------------------------------------------------------------------------------- GPU
def dev():
    return torch.device('cuda', 0)


def _bn_(m, g):
    for bn in m.modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            bn.running_mean.copy_((torch.rand(bn.num_features, generator=g) - 0.5) * 0.2)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 0.45 + 0.8)
            bn.weight.data.copy_(torch.rand(bn.num_features, generator=g) * 0.4 + 0.8)
            bn.bias.data.copy_((torch.rand(bn.num_features, generator=g) - 0.5) * 0.2)


def _stem64(x, w, sc, sh):
    y = F.conv2d(x.double(), w.double(), None, 2, 3) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    return F.max_pool2d(F.relu(y), 3, 2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(37, 53), (64, 96), (70, 130)])
@pytest.mark.parametrize('case', ['cin3', 'cin5', 'cin5_no_other'])
def test_stem_matches_fp64_as_well_as_the_miopen_path(case, h, w):
    """Batch 2: max abs error against float64 within 2x that of the parent's path (fp32 F.conv2d, then affine_relu_maxpool) on the same
    inputs; channels-last output of the stated shape; range word 0; a missing others-mask equals an explicit zero plane bit for bit."""
    from rmnet_amd import ops
    torch.backends.cudnn.benchmark = False
    cin = 3 if case == 'cin3' else 5
    g = torch.Generator().manual_seed(h + w + cin)
    frame = torch.randn(2, 3, h, w, generator=g).to(dev())
    mask = torch.rand(2, h, w, generator=g).to(dev())
    other = torch.zeros(2, h, w, device=dev()) if case == 'cin5_no_other' else torch.rand(2, h, w, generator=g).to(dev())
    wt = _weights(64, cin, 7, seed=cin).to(dev())
    sc = (torch.rand(64, generator=g) * 0.4 + 0.8).float().to(dev())
    sh = ((torch.rand(64, generator=g) * 2 - 1) * 0.05).float().to(dev())
    x = frame if cin == 3 else torch.cat((frame, mask.unsqueeze(1), other.unsqueeze(1)), dim=1)
    want = _stem64(x, wt, sc, sh)
    wp, wu = ops.stem_pack(wt, sc)
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    if cin == 3:
        got = ops.stem_split(frame, wpack=wp, w_unscale=wu, shift=sh, range_word=rw)
    else:
        got = ops.stem_split(frame, mask, None if case == 'cin5_no_other' else other, wp, wu, sh, range_word=rw)
    ref = ops.affine_relu_maxpool(F.conv2d(x, wt, None, 2, 3), sc, sh)
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert int(rw.item()) == 0
    assert got.shape == (2, 64, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1) and got.shape == want.shape
    assert got.is_contiguous(memory_format=torch.channels_last)
    es = float((got.double() - want).abs().max())
    em = float((ref.double() - want).abs().max())
    print('stem %s %dx%d: split %.3e  miopen %.3e' % (case, h, w, es, em))
    if case == 'cin5_no_other':
        assert torch.equal(got, ops.stem_split(frame, mask, other, wp, wu, sh))
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
def test_stem_range_word_counts_each_input_element_once():
    """Seven out-of-window inputs (corners, an odd / odd pixel, a last-column pixel, one in each mask plane, a NaN) on an even / odd and an
    odd / even map: the word is exactly 7 although neighbouring tiles re-read their halo; the 3-channel stem counts the frame's only."""
    from rmnet_amd import ops
    for h, w in ((13, 20), (12, 19)):
        g = torch.Generator().manual_seed(h)
        frame = torch.randn(2, 3, h, w, generator=g)
        mask, other = torch.rand(2, h, w, generator=g), torch.rand(2, h, w, generator=g)
        for b, c, i, j in ((0, 0, 0, 0), (1, 2, h - 1, w - 1), (0, 1, 5, 7), (1, 0, 4, w - 1)):
            frame[b, c, i, j] = 5e3
        frame[1, 1, 6, 2] = float('nan')
        mask[0, 3, 4] = 5e3
        other[1, 8, 9] = 5e3
        frame, mask, other = frame.to(dev()), mask.to(dev()), other.to(dev())
        for cin, want in ((5, 7), (3, 5)):
            wp, wu = ops.stem_pack(_weights(64, cin, 7, seed=cin).to(dev()))
            rw = torch.zeros(1, dtype=torch.int32, device=dev())
            if cin == 5:
                ops.stem_split(frame, mask, other, wp, wu, range_word=rw)
            else:
                ops.stem_split(frame, wpack=wp, w_unscale=wu, range_word=rw)
            assert int(rw.item()) == want, (h, w, cin, int(rw.item()), want)
    # a map of 3 x 5 tiles (each owns a 32 x 32 input core and re-reads 5 / 2 pixels of halo around it): outliers on both sides of the
    # core boundaries at rows / columns 32 and 64, all inside some neighbour's halo, are still counted once each
    h, w = 70, 130
    g = torch.Generator().manual_seed(h)
    frame = torch.randn(2, 3, h, w, generator=g)
    mask, other = torch.rand(2, h, w, generator=g), torch.rand(2, h, w, generator=g)
    spots = [(0, 0, 27, 27), (0, 1, 31, 31), (0, 2, 32, 32), (1, 0, 33, 64), (1, 1, 36, 63), (1, 2, 63, 95), (0, 0, 64, 96), (1, 1, 66, 128),
             (0, 2, 31, 64), (1, 0, 29, 98)]
    for b, c, i, j in spots:
        frame[b, c, i, j] = 5e3
    mask[0, 31, 32] = 5e3
    mask[1, 64, 63] = float('inf')
    other[1, 32, 31] = float('nan')
    frame, mask, other = frame.to(dev()), mask.to(dev()), other.to(dev())
    for cin, want in ((5, len(spots) + 3), (3, len(spots))):
        wp, wu = ops.stem_pack(_weights(64, cin, 7, seed=cin).to(dev()))
        rw = torch.zeros(1, dtype=torch.int32, device=dev())
        if cin == 5:
            ops.stem_split(frame, mask, other, wp, wu, range_word=rw)
        else:
            ops.stem_split(frame, wpack=wp, w_unscale=wu, range_word=rw)
        assert int(rw.item()) == want, (h, w, cin, int(rw.item()), want)


@pytest.mark.gpu
@pytest.mark.parametrize('hq,wq', [(7, 9), (24, 40), (33, 61)])
def test_pred_head_matches_fp64_as_well_as_miopen(hq, wq):
    """n = 3, C = 256, inputs of both signs: max abs error against float64 conv(relu(x)) within 2x that of fp32 F.conv2d(F.relu(x));
    NCHW-contiguous output; C = 64 is accepted, C = 48 is an error."""
    from rmnet_amd import ops
    torch.backends.cudnn.benchmark = False
    g = torch.Generator().manual_seed(hq + wq)
    x = torch.randn(3, 256, hq, wq, generator=g).to(dev()).contiguous(memory_format=torch.channels_last)
    wt = _weights(2, 256, 3, seed=2).to(dev())
    b = torch.tensor([0.03, -0.02], device=dev())
    want = F.conv2d(F.relu(x.double()), wt.double(), b.double(), 1, 1)
    got = ops.pred_head(x, wt, b)
    ref = F.conv2d(F.relu(x), wt.contiguous(memory_format=torch.channels_last), b, 1, 1)
    assert got.shape == (3, 2, hq, wq) and got.is_contiguous()
    es = float((got.double() - want).abs().max())
    em = float((ref.double() - want).abs().max())
    print('head %dx%d: kernel %.3e  miopen %.3e' % (hq, wq, es, em))
    assert es <= 2 * em, (es, em)
    if (hq, wq) == (7, 9):
        x64 = x[:, :64].contiguous(memory_format=torch.channels_last)
        got64 = ops.pred_head(x64, wt[:, :64].contiguous(), b)
        want64 = F.conv2d(F.relu(x64.double()), wt[:, :64].double(), b.double(), 1, 1)
        assert float((got64.double() - want64).abs().max()) < 1e-4
        with pytest.raises(RuntimeError):
            ops.pred_head(x[:, :48].contiguous(memory_format=torch.channels_last), wt[:, :48].contiguous(), b)


def _count(monkeypatch, ops, name):
    calls = []
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def _pooled(enc):
    """Forward pre-hook that keeps the stem stage's output (what layer1 receives)."""
    kept = []
    h = enc.res2.register_forward_pre_hook(lambda m, a: kept.append(a[0]))
    return kept, h


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['query', 'memory'])
def test_whole_encoders_take_one_stem_launch_and_agree_with_the_trunk_path(which, monkeypatch):
    """Channels-last, fused, randomised BatchNorm statistics, 96 x 160: one stem launch per call and none under RMNET_CONV=trunk.  The
    stem stage is where the two runs differ, so it is compared where its float64 restatement is defined, at the input of layer1: the
    stem kernel's output against the trunk run's within 2x the trunk run's own error against float64 conv / BatchNorm / ReLU / pool;
    the trunks behind it run the same kernels in both runs and must return finite maps of the same shapes that agree within 1e-3
    of each map's largest value."""
    from rmnet_amd import networks, ops
    torch.backends.cudnn.benchmark = False
    g = torch.Generator().manual_seed(7)
    enc = networks.procedural_init_(networks.EncoderQuery() if which == 'query' else networks.EncoderMemory())
    with torch.no_grad():
        _bn_(enc, g)
    enc = enc.to(dev()).eval()
    networks.fuse_epilogues_(enc)
    enc = enc.to(memory_format=torch.channels_last)
    frame = torch.randn(2, 3, 96, 160, generator=g).to(dev())
    args = (frame,) if which == 'query' else (frame, torch.rand(2, 96, 160, generator=g).to(dev()), torch.rand(2, 96, 160, generator=g).to(dev()))
    calls = _count(monkeypatch, ops, 'stem_split')
    kept, hook = _pooled(enc)
    monkeypatch.setenv('RMNET_CONV', 'full')
    with torch.no_grad():
        got = enc(*args)
        assert len(calls) == 1
        monkeypatch.setenv('RMNET_CONV', 'trunk')
        ref = enc(*args)
        assert len(calls) == 1
    hook.remove()
    x = frame if which == 'query' else torch.cat((frame, args[1].unsqueeze(1), args[2].unsqueeze(1)), dim=1)
    w = enc.conv1.weight if which == 'query' else torch.cat((enc.conv1.weight, enc.conv1_m.weight, enc.conv1_o.weight), dim=1)
    bn = enc.bn1
    y = F.batch_norm(F.conv2d(x.double(), w.double(), None, 2, 3), bn.running_mean.double(), bn.running_var.double(), bn.weight.double(),
                     bn.bias.double(), False, 0.0, bn.eps)
    want = F.max_pool2d(F.relu(y), 3, 2, 1)
    es = float((kept[0].double() - kept[1].double()).abs().max())
    em = float((kept[1].double() - want).abs().max())
    print('encoder %s stem stage: split vs trunk %.3e  trunk vs fp64 %.3e' % (which, es, em))
    assert es <= 2 * em, (es, em)
    for a, b in zip(got[:3], ref[:3]):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        print('  output %s: max |split - trunk| %.3e of max %.3e' % (tuple(a.shape), float((a - b).abs().max()), float(b.abs().max())))
        # (loose, so that the test stands on its own: 1e-3 of the map's largest value is the project's bar for two fp32-class paths that
        #  differ in summation order, fuse_epilogues' docstring; the stem stage differs by ~1e-6 and 13 blocks follow it)
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())


@pytest.mark.gpu
def test_whole_decoder_takes_one_head_launch_and_agrees_with_the_trunk_path(monkeypatch):
    """Channels-last fused Decoder on the 1/16, 1/8 and 1/4 maps of a 96 x 160 input: one head launch per call, none under
    RMNET_CONV=trunk; the logits agree with the trunk run's within 2x the trunk run's own error against a float64 restatement of the
    head stage (ReLU, pred2, x4 bilinear) on the same m2."""
    from rmnet_amd import networks, ops
    torch.backends.cudnn.benchmark = False
    g = torch.Generator().manual_seed(11)
    dec = networks.procedural_init_(networks.Decoder(256)).to(dev()).eval()
    networks.fuse_epilogues_(dec)
    dec = dec.to(memory_format=torch.channels_last)
    cl = lambda t: t.to(dev()).contiguous(memory_format=torch.channels_last)
    r4, r3, r2 = cl(torch.randn(2, 1024, 6, 10, generator=g)), cl(torch.randn(2, 512, 12, 20, generator=g)), cl(torch.randn(2, 256, 24, 40, generator=g))
    calls = _count(monkeypatch, ops, 'pred_head')
    kept = []
    hook = dec.RF2.register_forward_hook(lambda m, a, o: kept.append(o))
    monkeypatch.setenv('RMNET_CONV', 'full')
    with torch.no_grad():
        got = dec(r4, r3, r2)
        assert len(calls) == 1
        monkeypatch.setenv('RMNET_CONV', 'trunk')
        ref = dec(r4, r3, r2)
        assert len(calls) == 1
    hook.remove()
    assert torch.equal(kept[0], kept[1])                  # (the same kernels in front of the head in both runs)
    p = dec.pred2
    want = F.interpolate(F.conv2d(F.relu(kept[1].double()), p.weight.double(), p.bias.double(), 1, 1), scale_factor=4, mode='bilinear',
                         align_corners=False)
    assert got.shape == ref.shape == (2, 2, 96, 160)
    es = float((got.double() - ref.double()).abs().max())
    em = float((ref.double() - want).abs().max())
    print('decoder head stage: kernel vs trunk %.3e  trunk vs fp64 %.3e' % (es, em))
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
def test_whole_clip_agrees_with_the_trunk_path_eagerly_and_under_a_graph(monkeypatch):
    """synthetic_clip(3, 2, 96, 160, seed=4) through RMNet.forward: the default path against RMNET_CONV=trunk within 1e-3 in
    probability (the per-clip bar of fuse_epilogues' docstring), nothing redone; graph=True equals the eager default run within the
    same bar."""
    from rmnet_amd import networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    torch.backends.cudnn.benchmark = False
    net = networks.procedural_init_(RMNet(None)).to(dev()).eval()
    net.fuse_epilogues()
    net = net.to(memory_format=torch.channels_last)
    frames, masks, flows, n_objects = synthetic_clip(3, 2, 96, 160, seed=4)
    monkeypatch.setenv('RMNET_CONV', 'full')
    with torch.no_grad():
        est = net(frames, masks, flows, n_objects, 2).cpu()
        assert net.last_clip['reread'] is None, net.last_clip
        est_g = net(frames, masks, flows, n_objects, 2, graph=True).cpu()
        assert net.last_clip['reread'] is None, net.last_clip
        monkeypatch.setenv('RMNET_CONV', 'trunk')
        ref = net(frames, masks, flows, n_objects, 2).cpu()
        assert net.last_clip['reread'] is None, net.last_clip
    d, dg = float((est - ref).abs().max()), float((est_g - est).abs().max())
    print('clip: max |dp| split vs trunk %.3e, graph vs eager %.3e' % (d, dg))
    assert d <= 1e-3, d
    assert dg <= 1e-3, dg
