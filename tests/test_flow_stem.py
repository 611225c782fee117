# -*- coding: utf-8 -*-
"""TinyFlowNet's fused front end (csrc/flow_stem.hip, rmnet_flow_stem_f32): zero-padding, bilinear halving, the 6-channel cat, conv1,
bias and LeakyReLU in one launch.  Weight pack, switch and wiring, code object; on the GPU: accuracy against a float64 restatement
next to the library path, one live tap at a time, the range word, sentinels, refusals, capture / replay and the whole network."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import conv_ref

SRC = os.path.join(ROOT, 'rmnet_amd', 'csrc', 'flow_stem.hip')
SENTINEL = -777.25


def _tool(name):
    for d in ('/opt/rocm/llvm/bin', '/opt/rocm/bin'):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    pytest.fail('%s not found' % name)


def _weights(seed, cin=6):
    g = torch.Generator().manual_seed(seed)
    std = 0.9 * (2.0 / (49 * cin)) ** 0.5
    return ((torch.rand(64, cin, 7, 7, generator=g) * 2 - 1) * (std * 3 ** 0.5)).float()


def _bias(seed):
    return ((torch.rand(64, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * 0.05).float()


# ---------------------------------------------------------------------------------------------------------- CPU
def test_flow_stem_pack_restores_the_weights_to_stem_packs_bound():
    """hi + lo, unscaled, is w to 2^-21 relative per element plus 2^-25 of the channel's unscale (stem_pack's bound); the scale is a
    power of two that puts max |w| in [2^14, 2^15); a zero channel stays zero; the K padding 294 .. 319 is zero; other shapes raise."""
    from rmnet_amd import ops
    w = _weights(6)
    w[3] *= 1e-3
    w[5] = 0.0
    wp, wu = ops.flow_stem_pack(w)
    assert wp.dtype == torch.int16 and wp.numel() == 320 * 64 * 2 and wu.shape == (64,) and wu.dtype == torch.float32
    m, _ = torch.frexp(wu)
    assert bool((m == 0.5).all())
    want = w.double()
    scaled = want.abs().amax(dim=(1, 2, 3)) / wu.double()
    live = scaled > 0
    assert int(live.sum()) == 63
    assert bool(((scaled[live] >= 2 ** 14) & (scaled[live] < 2 ** 15)).all())
    back, pad = conv_ref.unpack_stem_weights(wp, wu, 6)
    err = (back - want).abs()
    bound = 2.0 ** -21 * want.abs() + 2.0 ** -25 * wu.double().view(-1, 1, 1, 1)
    assert bool((err <= bound).all()), float((err / (bound + 1e-300)).max())
    assert float(back[5].abs().max()) == 0.0
    assert pad.numel() == 64 * 2 * (320 - 294) and float(pad.abs().max()) == 0.0
    for bad in (_weights(1, cin=5), _weights(1)[:32], _weights(1).double()):
        with pytest.raises(RuntimeError):
            ops.flow_stem_pack(bad)
    # stem_pack's documented layout, Cin 6: element k = (7 ky + kx) 6 + ci of channel co sits at [k / 32][plane][co][k % 32]
    planes = wp.view(torch.float16).view(10, 2, 64, 32)
    co, ci, ky, kx = 9, 4, 5, 2
    k = (7 * ky + kx) * 6 + ci
    hi, lo = float(planes[k // 32, 0, co, k % 32]), float(planes[k // 32, 1, co, k % 32])
    assert abs((hi + lo) * float(wu[co]) - float(w[co, ci, ky, kx])) <= float(bound[co, ci, ky, kx])


def test_the_switch_its_default_and_the_wiring(monkeypatch):
    """RMNET_FLOW_STEM is '0' or '1', read at every call, FLOW_STEM_DEFAULT when unset, anything else raises; fuse_epilogues() builds
    the pack of conv1's weight as a plain attribute and fuse_epilogues(False) drops it; a CPU frame pair keeps the module graph."""
    from rmnet_amd import networks, ops, tiny_flownet
    from rmnet_amd.tiny_flownet import TinyFlowNet
    monkeypatch.delenv('RMNET_FLOW_STEM', raising=False)
    assert isinstance(tiny_flownet.FLOW_STEM_DEFAULT, bool)
    assert tiny_flownet.flow_stem_enabled() == tiny_flownet.FLOW_STEM_DEFAULT
    for v, want in (('0', False), ('1', True), (' 1 ', True)):
        monkeypatch.setenv('RMNET_FLOW_STEM', v)
        assert tiny_flownet.flow_stem_enabled() is want
    for v in ('', 'on', '2'):
        monkeypatch.setenv('RMNET_FLOW_STEM', v)
        with pytest.raises(RuntimeError):
            tiny_flownet.flow_stem_enabled()
    monkeypatch.setenv('RMNET_FLOW_STEM', '1')
    net = networks.procedural_init_(TinyFlowNet(None)).eval()
    keys = sorted(net.state_dict())
    assert not hasattr(net, '_flow_stem_pack')
    net.fuse_epilogues()
    wp, wu = ops.flow_stem_pack(net.conv1[0].weight.detach())
    assert torch.equal(net._flow_stem_pack[0], wp) and torch.equal(net._flow_stem_pack[1], wu)
    assert sorted(net.state_dict()) == keys
    a = torch.rand(1, 3, 64, 128)
    assert not net._flow_stem_ok(a, a)
    with torch.no_grad():
        assert net._forward(a, a).shape == (1, 2, 64, 128)
    net.fuse_epilogues(False)
    assert not hasattr(net, '_flow_stem_pack')


def test_flow_stem_code_object_uses_f16_mfma_no_static_lds_and_does_not_spill(tmp_path):
    """Compile-only gfx950 build: one kernel, whose name does not contain 'stem_split'; f16 MFMAs (4 channel tiles x 3 terms);
    no scratch, no spilled register, 0 bytes of static LDS (the 115,296 B are dynamic)."""
    from rmnet_amd import build
    assert 'flow_stem.hip' in build.SOURCES
    co = str(tmp_path / 'flow_stem.co')
    r = subprocess.run([build.hipcc_path(), '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '--no-gpu-bundle-output',
                        '-Rpass-analysis=kernel-resource-usage', '-c', SRC, '-o', co], stderr=subprocess.PIPE, check=True)
    text = subprocess.check_output([_tool('llvm-objdump'), '-d', '--mcpu=gfx950', co]).decode()
    assert len(re.findall(r'^\s+v_mfma_f32_16x16x32_f16\b', text, flags=re.M)) >= 12
    remarks = r.stderr.decode()
    names = re.findall(r'Function Name: (\S+)', remarks)
    assert len(names) == 1 and 'flow_stem' in names[0] and 'stem_split' not in names[0], names
    for key in (r'ScratchSize \[bytes/lane\]', r'VGPRs Spill', r'SGPRs Spill', r'LDS Size \[bytes/block\]'):
        assert [int(v) for v in re.findall(key + r': (\d+)', remarks)] == [0], (key, remarks)


# ---------------------------------------------------------------------------------------------------------- GPU
def dev():
    return torch.device('cuda', 0)


def _frames(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g) * 2 - 0.5, torch.rand(n, 3, h, w, generator=g) * 2 - 0.5


def _pair64(img0, img1, pad):
    """The float64 pair: zero pad, 2x2 mean, cat."""
    lw, uw, lh, uh = pad
    return torch.cat([F.avg_pool2d(F.pad(x.double(), (lw, uw, lh, uh)), 2) for x in (img0, img1)], dim=1)


def _ref64(img0, img1, wt, b, pad):
    return F.leaky_relu(F.conv2d(_pair64(img0, img1, pad), wt.double(), b.double(), 2, 3), 0.1)


def _library(img0, img1, wt, b, pad):
    """What TinyFlowNet._forward does in front of conv2 without the kernel: F.pad, F.interpolate, torch.cat, fp32 convolution."""
    lw, uw, lh, uh = pad
    a, c = (F.interpolate(F.pad(x, (lw, uw, lh, uh)), scale_factor=0.5, mode='bilinear') for x in (img0, img1))
    return F.leaky_relu(F.conv2d(torch.cat((a, c), dim=1), wt, b, 2, 3), 0.1)


def _compare(h, w, pad, seed):
    from rmnet_amd import ops
    torch.backends.cudnn.benchmark = False
    img0, img1 = (t.to(dev()) for t in _frames(2, h, w, seed))
    wt, b = _weights(seed).to(dev()), _bias(seed).to(dev())
    wp, wu = ops.flow_stem_pack(wt)
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    keep0, keep1 = img0.clone(), img1.clone()
    got = ops.flow_stem(img0, img1, wp, wu, b, pad=pad, range_word=rw)
    want = _ref64(img0, img1, wt, b, pad)
    ref = _library(img0, img1, wt, b, pad)
    assert int(rw.item()) == 0
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(img0, keep0) and torch.equal(img1, keep1)
    es = float((got.double() - want).abs().max())
    em = float((ref.double() - want).abs().max())
    print('flow_stem %dx%d pad %s -> %s: kernel %.3e  library %.3e' % (h, w, pad, tuple(got.shape[2:]), es, em))
    assert torch.equal(got, ops.flow_stem(img0, img1, wp, wu, b, pad=pad))            # two calls: equal bits
    assert es <= 2 * em, (es, em)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(38, 86), (70, 130), (64, 128)])
def test_flow_stem_matches_fp64_as_well_as_the_library_path(h, w):
    """Batch 2, padded to a multiple of 64 as _forward pads: max abs error against float64 pad + 2x2 mean + conv + bias + LeakyReLU
    within 2x that of the library path on the same inputs.  38 x 86: lh 13 and lw 21 both odd (2x2 blocks straddle the pad edge), one
    row of two tiles; 70 x 130: 2 x 3 tiles, halos that cross tiles; 64 x 128: no padding."""
    from rmnet_amd.helpers import pad_amounts
    pad = pad_amounts(h, w, 64)
    if (h, w) == (38, 86):
        assert pad[2] == 13 and pad[0] == 21
    if (h, w) == (64, 128):
        assert tuple(pad) == (0, 0, 0, 0)
    _compare(h, w, tuple(pad), seed=h + w)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,pad', [(70, 90, (5, 7, 2, 2)), (40, 50, (3, 5, 1, 1))])
def test_flow_stem_partial_tiles_with_explicit_pads(h, w, pad):
    """Padded sizes whose half is odd: 74 x 102 -> pair 37 x 51 -> 19 x 26 conv pixels (2 x 2 tiles, the last row / column of each
    partial, the last pair row / column read by the last conv pixel only); 42 x 58 -> 21 x 29 -> 11 x 15: one partial tile."""
    _compare(h, w, pad, seed=h)


@pytest.mark.gpu
def test_flow_stem_one_live_tap_at_a_time():
    """49 launches at 38 x 86 (padded 64 x 128), batch 1, each with the weights of one tap (ky, kx) alive: every output element
    against numpy's float64 sum over the six channels of that tap.  Bound per element: the operands are carried to 2^-22 relative
    each (hi + lo), the dropped lo x lo term is 2^-22, the pair's own fp32 mean 2^-23 and the fp32 accumulation of 18 terms and the
    epilogue under 2^-21 -- together below 2^-19 of sum |w| |pair| + |bias|; asserted at 2^-18."""
    from rmnet_amd import ops
    from rmnet_amd.helpers import pad_amounts
    h, w = 38, 86
    pad = tuple(pad_amounts(h, w, 64))
    img0, img1 = _frames(1, h, w, seed=5)
    wt, b = _weights(5), _bias(5)
    pair = np.pad(_pair64(img0, img1, pad)[0].numpy(), ((0, 0), (3, 3), (3, 3)))           # [6][32 + 6][64 + 6]
    hc, wc = 16, 32
    d0, d1, bd = img0.to(dev()), img1.to(dev()), b.to(dev())
    for ky in range(7):
        for kx in range(7):
            one = torch.zeros_like(wt)
            one[:, :, ky, kx] = wt[:, :, ky, kx]
            wp, wu = ops.flow_stem_pack(one.to(dev()))
            got = ops.flow_stem(d0, d1, wp, wu, bd, pad=pad)[0].cpu().numpy().astype(np.float64)       # [64][hc][wc]
            x = pair[:, ky:ky + 2 * hc:2, kx:kx + 2 * wc:2]                                              # [6][hc][wc]
            wk = one[:, :, ky, kx].double().numpy()                                                      # [64][6]
            pre = np.einsum('oc,chw->ohw', wk, x) + b.double().numpy()[:, None, None]
            want = np.where(pre > 0, pre, 0.1 * pre)
            bound = 2.0 ** -18 * (np.einsum('oc,chw->ohw', np.abs(wk), np.abs(x)) + np.abs(b.double().numpy())[:, None, None])
            err = np.abs(got - want)
            assert (err <= bound).all(), (ky, kx, float((err / bound).max()))


@pytest.mark.gpu
def test_flow_stem_range_word_counts_each_pair_element_once():
    """70 x 130 (padded 128 x 192, lh 29, lw 31, 2 x 3 tiles whose 32 x 32 cores meet at pair rows 31 | 32 and columns 31 | 32 and
    63 | 64 = frame rows 33, 34 | 35, 36, columns 31, 32 | 33, 34 and 95, 96 | 97, 98): out-of-window values, a NaN and an Inf in
    both frames on both sides of every core boundary (all inside a neighbour's halo), in the pad-straddling first / last row and
    column and in the corners, every one in a 2x2 block of its own: the word is their number.  A value whose 2x2 mean stays inside
    the window is not counted; clean frames leave the word 0."""
    from rmnet_amd import ops
    from rmnet_amd.helpers import pad_amounts
    h, w = 70, 130
    pad = tuple(pad_amounts(h, w, 64))
    assert pad[2] == 29 and pad[0] == 31
    img0, img1 = _frames(2, h, w, seed=9)
    big, nan, inf = 1e4, float('nan'), float('inf')
    spots = [(0, 0, 0, 0, 0, big), (1, 1, 2, h - 1, w - 1, big), (0, 1, 1, 0, w - 1, big), (1, 0, 0, h - 1, 0, nan),         # corners
             (0, 0, 1, 33, 31, big), (0, 1, 2, 35, 33, big), (1, 0, 0, 34, 96, inf), (1, 1, 1, 36, 97, big),                 # core corners
             (0, 0, 2, 34, 60, big), (1, 1, 0, 35, 120, -big), (0, 1, 1, 10, 32, big), (1, 0, 2, 50, 33, big), (0, 0, 0, 60, 95, big),
             (1, 1, 2, 20, 98, nan),                                                                                        # core edges
             (0, 0, 1, 17, 0, big), (1, 1, 0, 44, w - 1, big), (0, 1, 2, 0, 71, -inf), (1, 0, 1, h - 1, 40, big)]            # pad-straddling
    blocks = set()
    for n, which, c, i, j, v in spots:
        (img0, img1)[which][n, c, i, j] = v
        blocks.add((n, which, c, (i + pad[2]) // 2, (j + pad[0]) // 2))
    assert len(blocks) == len(spots)
    img1[0, 0, 41, 77] = 4000.0                    # (2x2 mean ~1000: inside the window)
    wp, wu = ops.flow_stem_pack(_weights(9).to(dev()))
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.flow_stem(img0.to(dev()), img1.to(dev()), wp, wu, pad=pad, range_word=rw)
    assert int(rw.item()) == len(spots), (int(rw.item()), len(spots))
    rw.zero_()
    clean0, clean1 = (t.to(dev()) for t in _frames(2, h, w, seed=9))
    ops.flow_stem(clean0, clean1, wp, wu, pad=pad, range_word=rw)
    assert int(rw.item()) == 0


def _entry_args(h=38, w=86, n=2, pad=(21, 21, 13, 13), seed=3):
    from rmnet_amd import ops
    img0, img1 = (t.to(dev()) for t in _frames(n, h, w, seed))
    wp, wu = ops.flow_stem_pack(_weights(seed).to(dev()))
    hpad, wpad = h + pad[2] + pad[3], w + pad[0] + pad[1]
    hc, wc = (hpad // 2 - 1) // 2 + 1, (wpad // 2 - 1) // 2 + 1
    guard = 4096
    buf = torch.full((guard + n * hc * wc * 64 + guard,), SENTINEL, device=dev())
    rw = torch.zeros(1, dtype=torch.int32, device=dev())
    return dict(img0=img0, img1=img1, wp=wp, wu=wu, bias=_bias(seed).to(dev()), N=n, H=h, W=w, Hpad=hpad, Wpad=wpad, lh=pad[2], lw=pad[0],
                buf=buf, guard=guard, out_elems=n * hc * wc * 64, rw=rw, pad=pad)


def _call(a, **over):
    from rmnet_amd import _lib
    a = dict(a, **over)
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    out = over.get('out', a['buf'].data_ptr() + 4 * a['guard'])
    rc = _lib.load().rmnet_flow_stem_f32(p(a['img0']), p(a['img1']), a.get('bs0', 3 * a['H'] * a['W']), a.get('bs1', 3 * a['H'] * a['W']), p(a['wp']), p(a['wu']), p(a['bias']), a['N'], a['H'], a['W'], a['Hpad'],
                                         a['Wpad'], a['lh'], a['lw'], ctypes.c_void_p(out), p(a['rw']),
                                         ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
def test_flow_stem_writes_its_output_and_nothing_around_it():
    """The C entry on a caller's buffer with 16 KB of sentinels on either side: the output equals ops.flow_stem's bit for bit, the
    sentinels and both frames are untouched, the range word stays 0."""
    from rmnet_amd import ops
    a = _entry_args()
    keep0, keep1 = a['img0'].clone(), a['img1'].clone()
    ops.flow_stem(a['img0'], a['img1'], a['wp'], a['wu'], a['bias'], pad=a['pad'])             # (the first call on the device: eager)
    assert _call(a) == 0
    g, n = a['guard'], a['out_elems']
    want = ops.flow_stem(a['img0'], a['img1'], a['wp'], a['wu'], a['bias'], pad=a['pad'])
    assert torch.equal(a['buf'][g:g + n].view(2, 16, 32, 64), want.permute(0, 2, 3, 1))
    assert bool((a['buf'][:g] == SENTINEL).all()) and bool((a['buf'][g + n:] == SENTINEL).all())
    assert torch.equal(a['img0'], keep0) and torch.equal(a['img1'], keep1) and int(a['rw'].item()) == 0


@pytest.mark.gpu
def test_flow_stem_reads_the_frames_of_a_clip_in_place():
    """clip[:, t] and clip[:, t - 1] of a [2, 3, 3, 38, 86] clip (dense frames at a batch stride of three frames) give the bits of
    their contiguous copies, and the clip is unchanged; a channels-last frame pair is copied by the wrapper and gives them too."""
    from rmnet_amd import ops
    a = _entry_args()
    clip = torch.rand(2, 3, 3, 38, 86, generator=torch.Generator().manual_seed(8)).to(dev())
    keep = clip.clone()
    f0, f1 = clip[:, 2], clip[:, 1]
    assert not f0.is_contiguous()
    want = ops.flow_stem(f0.contiguous(), f1.contiguous(), a['wp'], a['wu'], a['bias'], pad=a['pad'])
    assert torch.equal(ops.flow_stem(f0, f1, a['wp'], a['wu'], a['bias'], pad=a['pad']), want)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    assert torch.equal(ops.flow_stem(cl(f0), cl(f1), a['wp'], a['wu'], a['bias'], pad=a['pad']), want)
    assert torch.equal(clip, keep)


@pytest.mark.gpu
def test_flow_stem_entry_refusals_write_nothing():
    """Null pointers, sizes, pads that do not hold the frame, batch strides below a frame, misaligned pointers, an output that overlaps a frame: RMNET_E_INVALID_ARG;
    an odd padded size, 2^31 input elements: RMNET_E_UNSUPPORTED; the output buffer keeps its sentinels and the range word its value.
    The wrapper refuses CPU tensors, other dtypes, shapes and packs before it launches."""
    from rmnet_amd import ops
    a = _entry_args()
    a['rw'].fill_(5)
    out = a['buf'].data_ptr() + 4 * a['guard']
    invalid = [dict(img0=None), dict(img1=None), dict(wp=None), dict(wu=None), dict(out=0), dict(N=0), dict(H=0), dict(W=-1), dict(Hpad=0),
               dict(lh=-1), dict(lw=-2), dict(bs0=3 * 38 * 86 - 1), dict(bs1=0), dict(lh=27), dict(lw=43), dict(Hpad=50, lh=13), dict(out=out + 4), dict(wu=a['wu'].data_ptr() + 4),
               dict(bias=a['bias'].data_ptr() + 8), dict(wp=a['wp'].data_ptr() + 2), dict(img0=a['img0'].data_ptr() + 2),
               dict(out=a['img0'].data_ptr()), dict(out=a['img1'].data_ptr() + 64)]
    unsupported = [dict(Hpad=65), dict(Wpad=129), dict(N=1 << 20, H=38, W=86)]
    frames = (a['img0'].clone(), a['img1'].clone())
    for over in invalid:
        assert _call(a, **over) == -1, over
    for over in unsupported:
        assert _call(a, **over) == -4, over
    assert bool((a['buf'] == SENTINEL).all()) and int(a['rw'].item()) == 5
    assert torch.equal(a['img0'], frames[0]) and torch.equal(a['img1'], frames[1])
    i0, i1, wp, wu, b = a['img0'], a['img1'], a['wp'], a['wu'], a['bias']
    for name, fn in (('CPU frames', lambda: ops.flow_stem(i0.cpu(), i1.cpu(), wp, wu, b)),
                     ('float64 frames', lambda: ops.flow_stem(i0.double(), i1.double(), wp, wu, b)),
                     ('two shapes', lambda: ops.flow_stem(i0, i1[:, :, :-2].contiguous(), wp, wu, b)),
                     ('four channels', lambda: ops.flow_stem(torch.cat((i0, i0[:, :1]), 1), torch.cat((i1, i1[:, :1]), 1), wp, wu, b)),
                     ('a stem pack of Cin 5', lambda: ops.flow_stem(i0, i1, ops.stem_pack(_weights(1, cin=5).to(dev()))[0], wu, b)),
                     ('32 biases', lambda: ops.flow_stem(i0, i1, wp, wu, b[:32].contiguous())),
                     ('a negative pad', lambda: ops.flow_stem(i0, i1, wp, wu, b, pad=(-1, 1, 0, 0))),
                     ('an odd padded size', lambda: ops.flow_stem(i0, i1, wp, wu, b, pad=(0, 1, 0, 0)))):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(name)


@pytest.mark.gpu
def test_flow_stem_is_captured_and_replayed():
    """After an eager call (the dynamic-LDS attribute is set outside a capture) the launch is captured into a HIP graph; replayed on
    other frames it returns the eager call's bits, and the range word stays 0."""
    from rmnet_amd import ops
    a = _entry_args(h=70, w=130, pad=(31, 31, 29, 29))
    s0, s1 = a['img0'].clone(), a['img1'].clone()
    with torch.no_grad():
        side = torch.cuda.Stream(dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.cuda.stream(side):
            ops.flow_stem(s0, s1, a['wp'], a['wu'], a['bias'], pad=a['pad'], range_word=a['rw'])
        torch.cuda.current_stream(dev()).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s_out = ops.flow_stem(s0, s1, a['wp'], a['wu'], a['bias'], pad=a['pad'], range_word=a['rw'])
        for seed in (11, 12):
            f0, f1 = (t.to(dev()) for t in _frames(2, 70, 130, seed))
            s0.copy_(f0)
            s1.copy_(f1)
            graph.replay()
            got = s_out.clone()
            assert torch.equal(got, ops.flow_stem(f0, f1, a['wp'], a['wu'], a['bias'], pad=a['pad']))
    assert int(a['rw'].item()) == 0


@pytest.mark.gpu
def test_whole_forward_with_the_kernel_is_as_close_to_float64_as_without(monkeypatch):
    """TinyFlowNet._forward at 96 x 160, batch 2, fused and channels-last: RMNET_FLOW_STEM=1 issues one flow_stem launch and no
    F.conv2d with 64 outputs, RMNET_FLOW_STEM=0 the other way round; the two flows differ by at most 2x the error of the switched-off
    path against the same network in float64 on the CPU; the range word stays 0."""
    from rmnet_amd import networks, ops
    from rmnet_amd.tiny_flownet import TinyFlowNet
    torch.backends.cudnn.benchmark = False
    img0, img1 = (t + 0.25 for t in _frames(2, 96, 160, seed=21))
    with torch.no_grad():
        want = networks.procedural_init_(TinyFlowNet(None)).eval().double()._forward(img0.double(), img1.double())
    net = networks.procedural_init_(TinyFlowNet(None)).to(dev()).eval()
    net.fuse_epilogues()
    net = net.to(memory_format=torch.channels_last)
    stem_calls, conv_calls = [], []
    real_stem, real_conv = ops.flow_stem, F.conv2d
    monkeypatch.setattr(ops, 'flow_stem', lambda *a, **k: stem_calls.append(1) or real_stem(*a, **k))
    monkeypatch.setattr(F, 'conv2d', lambda x, w, *a, **k: conv_calls.append(w.shape[0]) or real_conv(x, w, *a, **k))
    d0, d1 = img0.to(dev()), img1.to(dev())
    net.flow_range_word(dev()).zero_()
    with torch.no_grad():
        monkeypatch.setenv('RMNET_FLOW_STEM', '1')
        on = net._forward(d0, d1)
        assert len(stem_calls) == 1 and 64 not in conv_calls, (stem_calls, conv_calls)
        monkeypatch.setenv('RMNET_FLOW_STEM', '0')
        off = net._forward(d0, d1)
        assert len(stem_calls) == 1 and conv_calls.count(64) == 1, (stem_calls, conv_calls)
    assert net.flow_range_count() == 0
    assert on.shape == off.shape == (2, 2, 96, 160)
    es = float((on.double().cpu() - off.double().cpu()).abs().max())
    em = float((off.double().cpu() - want).abs().max())
    print('_forward 96x160: on vs off %.3e  off vs float64 %.3e  (largest |flow| %.3e)' % (es, em, float(want.abs().max())))
    assert es <= 2 * em, (es, em)
