# -*- coding: utf-8 -*-
"""Pre-split activations (include/rmnet_hip.h; csrc/conv_split.hip: conv_split<tile, XS, OS>, split_act): a tensor that only split-fp16
convolutions read is kept as fp16 hi / lo planes and split once, by its producer, instead of at every tap and Cout tile of its
reader.  The split depends on the element alone, so everything here is bit for bit:

  * rmnet_split_act_f32 against the numpy restatement (tests/presplit_ref.py), with an out-of-window value of either sign, NaN, Inf
    and -0.0 planted, with and without the ReLU; the range word is the restatement's count;
  * the consumer: conv_split on split(x) == rmnet_conv_split_f32 on x, for every tile (Big as 512 slices of one pack, as
    tests/test_conv_overlap.py selects it), maps of 70 and 135 pixels (the second crosses a pixel tile), Cin 32 and 96, 1x1, 3x3 and
    3x3 / stride 2, with and without res and the output ReLU, randn inputs (all three product terms live); the key / value form
    with two outputs; one live tap at a time on an input with a different integer in every element, where a tap's zeros in the
    wrong plane or chunk show;
  * the producer: the split output of either input form == restatement(the fp32 instance's output), range word == the count
    (a shift of +-3000 on two channels puts them outside the window).  The fp32 in / fp32 out instance and the split ones are
    instances of one kernel template that differ in the loader, the K loop's order of loads and the store; the fp32 instance's own
    bits are anchored against float64 in tests/test_conv_edges.py and tests/test_conv_split.py;
  * the argument rules of rmnet_conv_split_pre_f32 and rmnet_split_act_f32;
  * four bottlenecks and the key / value heads with RMNET_CONV_PRESPLIT on and off: equal outputs, and a range word that is
    non-zero in both settings when an intermediate leaves the window; one graph capture and replay of the stage;
  * CPU: the restatement's round trip, and the twelve instances' registers, spills, scratch and LDS from the code object's metadata."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import presplit_ref as P

MAP_A, MAP_B, MAP_S2 = (2, 5, 7), (1, 9, 15), (2, 7, 9)
TILE_COUT = {'Narrow': 64, 'Mid': 128, 'Big': 512 * 256}       # (Big: tests/test_conv_overlap.py says why it is affordable)
TILE_REAL = {'Narrow': 64, 'Mid': 128, 'Big': 256}
TILES = ['Narrow', 'Mid', 'Big']
INVALID, UNSUPPORTED = -1, -4


def dev():
    return torch.device('cuda', 0)


def _cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _rw():
    return torch.zeros(1, dtype=torch.int32, device=dev())


def _nhwc(t):
    """A channels-last [N, C, H, W] tensor as a numpy [N, H, W, C] array."""
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _split_t(x, relu=False):
    """The restatement's split form of a channels-last fp32 tensor, on the device, and its count."""
    planes, n = P.split_form(_nhwc(x), relu)
    return torch.from_numpy(planes).to(dev()), n


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    ib = torch.int32 if got.dtype == torch.float32 else torch.int16
    if torch.equal(got.contiguous().view(ib), want.contiguous().view(ib)):
        return
    bad = (got.contiguous().view(ib) != want.contiguous().view(ib)).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index, got, want): %s' % (what, bad.shape[0], got.numel(), first))


def _pack(tile, wt):
    from rmnet_amd import ops
    wp, wu = ops.conv_split_pack(wt)
    real = wt.shape[0]
    rep = TILE_COUT[tile] // real
    if rep > 1:
        k2, cin = wt.shape[2] * wt.shape[3], wt.shape[1]
        wp = wp.view(k2, cin // 32, 2, real, 32).repeat(1, 1, 1, rep, 1).contiguous().view(-1)
        wu = wu.repeat(rep)
    return wp, wu, rep


# ================================================================================================ CPU: the restatement
def test_the_restatement_round_trips_to_two_to_the_minus_22():
    """hi + lo == c to 2^-22 relative: hi keeps 11 bits of c, lo 11 bits of the rest.  Below that, lo's own grid: fp16's subnormal
    spacing is 2^-24, so half of it absolutely.  Specials: NaN and out-of-window values saturate and are counted, -0.0 stays -0.0."""
    g = np.random.RandomState(3)
    v = (g.randn(4096) * np.repeat(2.0 ** np.arange(-12, 4), 256)).astype(np.float32)
    c, hi, lo, counted = P.split_values(v)
    assert not counted.any() and np.array_equal(c, v * np.float32(64))
    err = np.abs(c.astype(np.float64) - (hi.astype(np.float64) + lo.astype(np.float64)))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(c.astype(np.float64)), 2.0 ** -25)).all(), float(err.max())
    sp = np.array([1023.6, -1023.6, 1023.5, np.nan, np.inf, -np.inf, -0.0, -3.0], np.float32)      # (1023.5 * 64 is fp16's largest)
    c, hi, lo, counted = P.split_values(sp)
    assert counted.tolist() == [True, True, False, True, True, True, False, False]
    assert c[:6].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, -65504.0]
    assert np.signbit(hi[6]) and hi[6] == 0 and lo[6] == 0 and not np.signbit(lo[6])
    c, hi, lo, counted = P.split_values(sp, relu=True)
    assert counted.tolist() == [True, False, False, True, True, False, False, False] and c[7] == 0 and np.signbit(hi[6])
    planes, n = P.split_form(np.arange(2 * 64, dtype=np.float32).reshape(2, 64))
    assert planes.shape == (2, 2, 2, 32) and n == 0 and planes[1, 1, 0, 5] == np.float16(64 * (64 + 32 + 5)) and not planes[:, :, 1].any()


# ================================================================================================ CPU: what the compiler gives
VGPR_LIMIT = {'Big': 256, 'Mid': 128, 'Narrow': 128}


def test_the_new_kernels_keep_their_registers_lds_and_have_no_spill_or_scratch(tmp_path):
    """Compile-only, with tests/test_kernel_resources.py's compile step and metadata reader: every instance of conv_split<tile, XS, OS>
    (all four pairs of input and output form x 3 tiles) has no spill and no scratch, at most 128 VGPRs for Mid and Narrow (two
    workgroups per CU) and 256 for Big, and static LDS exactly the declared double buffer (96 / 64 / 48 KB); these twelve are the
    file's only convolution kernels (no five-parameter conv_split, no conv_split_pre kernel is left); split_act has no LDS, scratch
    or spill."""
    import test_kernel_resources as KR
    found = KR._kernels(KR._compile('conv_split.hip', str(tmp_path / 'conv_split.s')))
    for xs, os_ in ((1, 1), (1, 0), (0, 1), (0, 0)):         # (the VGPR counts of record: profiles/r27_a_conv_split_fold.md)
        for tile, (wm, wn, ti, tj, wpe) in KR.TILES.items():
            k = KR._one(found, '10conv_splitILi%dELi%dELi%dELi%dELi%dELb%dELb%dEEE' % (wm, wn, ti, tj, wpe, xs, os_))
            print('%-6s x split %d out split %d  LDS %6d  scratch %d  VGPRs %3d  spilled %d'
                  % (tile, xs, os_, k['group_segment_fixed_size'], k['private_segment_fixed_size'], k['vgpr_count'],
                     k['vgpr_spill_count']))
            assert k['group_segment_fixed_size'] == KR._double_buffer_bytes(wm * ti * 16, wn * tj * 16), (tile, k)
            assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (tile, k)
            assert k['vgpr_count'] <= VGPR_LIMIT[tile], (tile, k)
    assert len([n for n in found if '10conv_splitI' in n]) == 12
    old = [n for n in found if '14conv_split_pre' in n or ('10conv_splitI' in n and 'ELb' not in n)]
    assert not old, old                                      # (a leftover copy: the old seven- or five-parameter kernel)
    k = KR._one(found, '9split_actE')
    assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k


# ================================================================================================ rmnet_split_act_f32
@pytest.mark.gpu
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,c', [((1, 3, 5), 32), ((2, 5, 7), 96)])
def test_split_act_equals_the_restatement_bit_for_bit(shape, c, relu):
    from rmnet_amd import ops
    n, h, w = shape
    x = torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(c + h)) * 40
    plants = [2000.0, -2000.0, float('nan'), float('inf'), float('-inf'), -0.0, 1023.5, -1023.4]
    for i, v in enumerate(plants):
        x[i % n, (11 * i + 3) % c, (i * 2) % h, (i * 3 + 1) % w] = v
    xc = _cl(x)
    want, count = P.split_form(_nhwc(xc), relu)
    assert count == (3 if relu else 5)                     # (2000, NaN, Inf; and -2000, -Inf without the ReLU; 1023.5 is inside)
    rw = _rw()
    got = ops.split_act(xc, relu=relu, range_word=rw)
    assert got.dtype == torch.float16 and tuple(got.shape) == (n, h, w, c // 32, 2, 32) and ops.is_split_act(got)
    assert np.array_equal(P.bits(got.cpu().numpy()), P.bits(want))
    assert int(rw.item()) == count


# ================================================================================================ consumer and producer, every tile
def _case(tile, shape, cin, k, s):
    """One shape on one tile, res and the output ReLU on and off: conv_split's three split forms against the fp32 in / fp32 out instance's output."""
    from rmnet_amd import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(100 * cin + 10 * k + s + h)
    x = _cl(torch.randn((n, cin, h, w), generator=g))
    real = TILE_REAL[tile]
    wt = R.uniform_weights(real, cin, k, 7 + cin).to(dev())
    wp, wu, rep = _pack(tile, wt)
    cout = wu.numel()
    assert R.tile_of(n, cout, h, w, k, s) == tile
    shift = torch.randn(real, generator=g)
    shift[1], shift[2] = 3000.0, -3000.0                   # two channels outside the window (the second: inside after a ReLU)
    shift = shift.repeat(rep).to(dev())
    ho, wo = R.out_hw(h, w, k, s)
    res_all = _cl(torch.randn((n, real, ho, wo), generator=g).repeat(1, rep, 1, 1))
    xs, x_count = _split_t(x)
    assert x_count == 0
    for use_res in (False, True):
        for relu_out in (False, True):
            what = '%s %s Cin %d %dx%d / %d res %s relu_out %s' % (tile, shape, cin, k, k, s, use_res, relu_out)
            kw = dict(shift=shift, res=res_all if use_res else None, ksize=k, stride=s, relu_out=relu_out)
            rw = _rw()
            want = ops.conv_split(x, wp, wu, range_word=rw, **kw)
            assert int(rw.item()) == 0
            # consumer: split in, fp32 out
            got = ops.conv_split(xs, wp, wu, range_word=rw, **kw)
            _same_bits(got, want, what + ': split in, fp32 out')
            assert int(rw.item()) == 0 and got.is_contiguous(memory_format=torch.channels_last)
            # producer, either input form
            planes, count = P.split_form(_nhwc(want))
            assert count == n * ho * wo * rep * (1 if relu_out else 2), (what, count)
            wantp = torch.from_numpy(planes).to(dev())
            for xin, form in ((xs, 'split'), (x, 'fp32')):
                rw = _rw()
                gotp = ops.conv_split(xin, wp, wu, range_word=rw, out_presplit=True, **kw)
                assert tuple(gotp.shape) == (n, ho, wo, cout // 32, 2, 32)
                _same_bits(gotp, wantp, what + ': %s in, split out' % form)
                assert int(rw.item()) == count, (what, form, int(rw.item()), count)
            if use_res:
                assert not torch.equal(res_all, want)           # (an fp32 out may still be res; a split one is a new tensor)


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('cin', [32, 96])
@pytest.mark.parametrize('shape', [MAP_A, MAP_B])
@pytest.mark.parametrize('tile', TILES)
def test_split_input_and_split_output_equal_the_fp32_kernel_bit_for_bit(tile, shape, cin, k):
    _case(tile, shape, cin, k, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('tile', TILES)
def test_split_input_and_split_output_3x3_stride_2_on_an_odd_map(tile):
    _case(tile, MAP_S2, 32, 3, 2)


@pytest.mark.gpu
def test_key_value_form_with_two_outputs_reads_a_split_input():
    from rmnet_amd import ops
    n, h, w = MAP_B
    g = torch.Generator().manual_seed(640)
    x = _cl(torch.randn((n, 64, h, w), generator=g))
    wt = R.uniform_weights(640, 64, 3, 641).to(dev())
    wp, wu = ops.conv_split_pack(wt)
    shift = torch.randn(640, generator=g).to(dev())
    k0, v0 = ops.conv_split(x, wp, wu, shift, ksize=3, split=128)
    rw = _rw()
    k1, v1 = ops.conv_split(_split_t(x)[0], wp, wu, shift, ksize=3, split=128, range_word=rw)
    assert tuple(k1.shape) == (n, 128, h, w) and tuple(v1.shape) == (n, 512, h, w) and int(rw.item()) == 0
    _same_bits(k1, k0, 'key')
    _same_bits(v1, v0, 'value')


@pytest.mark.gpu
def test_one_live_tap_at_a_time_on_a_split_input_with_a_different_integer_in_every_element():
    """x = (flat NHWC index mod 2039) - 1019: 64 x is an fp16 number, so the lo plane is all zero and the hi plane holds a different
    value in (nearly) every element.  A tap's zeros, or its values, in the wrong plane, chunk or pixel give a wrong integer: the result
    must be the fp32-input instance's AND the float64 convolution (exact: tests/conv_ref.py, section 1)."""
    from rmnet_amd import ops
    n, h, w = MAP_A
    cin, cout = 96, 128
    flat = torch.arange(n * h * w * cin, dtype=torch.int64)
    x = ((flat % 2039) - 1019).float().view(n, h, w, cin).permute(0, 3, 1, 2).contiguous()
    xc = _cl(x)
    xs, _ = _split_t(xc)
    assert not bool(xs[..., 1, :].any()) and bool(xs[..., 0, :].any())
    wt = R.int_weights(cout, cin, 3, 107).to(dev())
    shift = R.int_acts((cout,), 108, -20, 20).to(dev())
    for tap in range(9):
        w1 = torch.zeros_like(wt)
        w1[:, :, tap // 3, tap % 3] = wt[:, :, tap // 3, tap % 3]
        wp, wu = ops.conv_split_pack(w1)
        rw = _rw()
        got = ops.conv_split(xs, wp, wu, shift, ksize=3, range_word=rw)
        _same_bits(got, ops.conv_split(xc, wp, wu, shift, ksize=3), 'tap %d alone, against the fp32-input kernel' % tap)
        want = F.conv2d(xc.double(), w1.double(), None, 1, 1) + shift.double().view(1, -1, 1, 1)
        assert torch.equal(got, want.float()), 'tap %d alone, against float64' % tap
        assert int(rw.item()) == 0


# ================================================================================================ argument rules
@pytest.mark.gpu
def test_the_new_entries_refuse_what_they_document():
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    n, h, w, cin, cout = 1, 4, 6, 32, 64
    wt = R.uniform_weights(cout, cin, 1, 1).to(dev())
    wp, wu = ops.conv_split_pack(wt)
    buf = torch.zeros(4 * n * h * w * cout + 64, dtype=torch.float32, device=dev())      # x, out, res carved from one allocation
    x, out, res = buf[:768], buf[1024:1024 + 1536], buf[4096:4096 + 1536]
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    X, O = ops.CONV_X_SPLIT, ops.CONV_OUT_SPLIT

    def call(flags, x_=None, out_=None, res_=None, cin_=cin, out2=None, osplit=0):
        return lib.rmnet_conv_split_pre_f32(x_ or p(x), p(wp), p(wu), None, res_, flags, n, h, w, cin_, cout, 1, 1, out_ or p(out), out2,
                                            osplit, None, None)

    for flags in (X, O, X | O, X | ops.CONV_RELU_OUT, 0):
        assert call(flags) == 0, flags
    assert call(O, res_=p(res)) == 0
    for flags in (16, X | 16, 32 | O, -1):                                            # unknown flag bits
        assert call(flags) == INVALID, flags
    assert call(X | ops.CONV_RELU_IN) == INVALID                                      # the ReLU belongs to the producer
    for flags in (X, O, X | O):
        assert call(flags, x_=p(x, 4)) == INVALID and call(flags, out_=p(out, 8)) == INVALID      # misaligned
        assert call(flags, out_=p(x)) == INVALID and call(flags, out_=p(x, 16 * 4)) == INVALID    # out overlaps x
        assert call(flags, cin_=48) == UNSUPPORTED                                                # Cin % 32
    assert call(O, res_=p(res, 2)) == INVALID
    assert call(O, out_=p(res), res_=p(res)) == INVALID                               # a split out must not be res ...
    assert call(O, out_=p(res, 64), res_=p(res)) == INVALID and call(X | O, out_=p(res), res_=p(res)) == INVALID
    assert call(X, out_=p(res), res_=p(res)) == 0                                     # ... an fp32 one may
    assert call(O, out2=p(res), osplit=32) == INVALID                                 # no second output in split form
    assert lib.rmnet_conv_split_f32(p(x), p(wp), p(wu), None, None, X, n, h, w, cin, cout, 1, 1, p(out), None, 0, None, None) == INVALID
    assert lib.rmnet_conv_split_f32(p(x), p(wp), p(wu), None, None, O, n, h, w, cin, cout, 1, 1, p(out), None, 0, None, None) == INVALID

    act = lambda x_, out_, m=n * h * w, c=cin: lib.rmnet_split_act_f32(x_, m, c, 0, out_, None, None)
    assert act(p(x), p(out)) == 0
    assert act(None, p(out)) == INVALID and act(p(x), None) == INVALID and act(p(x), p(out), m=0) == INVALID
    assert act(p(x, 4), p(out)) == INVALID and act(p(x), p(out, 8)) == INVALID
    assert act(p(x), p(x)) == INVALID and act(p(x), p(x, 16 * 4)) == INVALID           # in place: an item's output is elsewhere
    assert act(p(x), p(out), c=48) == UNSUPPORTED
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='relu_in'):
        ops.conv_split(ops.split_act(_cl(torch.zeros(1, 32, 4, 6))), wp, wu, ksize=1, relu_in=True)
    with pytest.raises(RuntimeError, match='out_presplit'):
        ops.conv_split(_cl(torch.zeros(1, 32, 4, 6)), wp, wu, ksize=1, out_presplit=True, split=32)


# ================================================================================================ the modules and the switch
def _stage(plant):
    """Four bottlenecks (projection, identity, two projections / stride 2) from the 1/4 map of a 1x3x64x96 frame down to 1/16; the
    last one's conv3 has 256 input channels and reads a split input, the others' (64, 64, 128) read fp32
    (networks.PRESPLIT_MIN_CIN_1X1)."""
    from rmnet_amd import networks
    assert networks.PRESPLIT_MIN_CIN_1X1 == 256
    stage = torch.nn.Sequential(networks._Bottleneck(64, 64, 1, True), networks._Bottleneck(256, 64, 1, False),
                                networks._Bottleneck(256, 128, 2, True), networks._Bottleneck(512, 256, 2, True))
    stage = networks.procedural_init_(stage)
    if plant:
        with torch.no_grad():
            stage[1].bn1.bias[7] += 3000.0           # one channel of the second block's conv1 output leaves the window
    stage = stage.to(dev()).eval()
    networks.fuse_epilogues_(stage)
    return stage.to(memory_format=torch.channels_last)


def _run(module, x, presplit, monkeypatch):
    """(outputs, range word, [input was split, per conv_split call])."""
    from rmnet_amd import ops
    monkeypatch.setenv('RMNET_CONV_PRESPLIT', '1' if presplit else '0')
    seen = []
    real = ops.conv_split
    monkeypatch.setattr(ops, 'conv_split', lambda *a, **k: seen.append((ops.is_split_act(a[0]), bool(k.get('out_presplit')))) or real(*a, **k))
    word = ops.conv_range_word(dev())
    word.zero_()
    with torch.no_grad():
        out = module(x)
    monkeypatch.setattr(ops, 'conv_split', real)
    return out, int(word.item()), seen


@pytest.mark.gpu
@pytest.mark.parametrize('plant', [False, True])
def test_a_bottleneck_stage_gives_the_same_bits_with_the_switch_on_and_off(plant, monkeypatch):
    torch.backends.cudnn.benchmark = False
    stage = _stage(plant)
    x = _cl(F.relu(torch.randn(1, 64, 16, 24, generator=torch.Generator().manual_seed(17))))
    off, w_off, seen_off = _run(stage, x, False, monkeypatch)
    on, w_on, seen_on = _run(stage, x, True, monkeypatch)
    assert len(seen_off) == len(seen_on) == 4 + 3 + 4 + 4 and not any(a or b for a, b in seen_off)
    # (input split, output split) per block: conv1 fp32 -> split, conv2 split -> fp32 (the last block: -> split), the projection
    # fp32 -> fp32, conv3 fp32 -> fp32 (the last block: split -> fp32)
    narrow = [(False, True), (True, False), (False, False), (False, False)]
    assert seen_on == narrow + [narrow[0], narrow[1], narrow[3]] + narrow + [(False, True), (True, True), (False, False), (True, False)]
    assert tuple(on.shape) == (1, 1024, 4, 6) and on.dtype == torch.float32
    _same_bits(on, off, 'stage output')
    if plant:
        assert w_off > 0 and w_on > 0, (w_off, w_on)
    else:
        assert w_off == 0 and w_on == 0, (w_off, w_on)


@pytest.mark.gpu
@pytest.mark.parametrize('plant', [False, True])
def test_the_key_value_heads_give_the_same_bits_with_the_switch_on_and_off(plant, monkeypatch):
    from rmnet_amd import networks
    torch.backends.cudnn.benchmark = False
    kv = networks.procedural_init_(networks.KeyValue(1024, 128, 512)).to(dev()).eval()
    networks.fuse_epilogues_(kv)
    kv = kv.to(memory_format=torch.channels_last)
    x = F.relu(torch.randn(1, 1024, 4, 6, generator=torch.Generator().manual_seed(18)))
    if plant:
        x[0, 5, 1, 1] = 2000.0
    x = _cl(x)
    (k0, v0), w_off, seen_off = _run(kv, x, False, monkeypatch)
    (k1, v1), w_on, seen_on = _run(kv, x, True, monkeypatch)
    assert seen_off == [(False, False)] and seen_on == [(True, False)]
    _same_bits(k1, k0, 'key')
    _same_bits(v1, v0, 'value')
    assert (w_off, w_on) == ((1, 1) if plant else (0, 0))


@pytest.mark.gpu
def test_the_stage_replays_from_a_captured_graph_with_the_switch_on(monkeypatch):
    from rmnet_amd import ops
    torch.backends.cudnn.benchmark = False
    monkeypatch.setenv('RMNET_CONV_PRESPLIT', '1')
    stage = _stage(False)
    x = _cl(F.relu(torch.randn(1, 64, 16, 24, generator=torch.Generator().manual_seed(19))))
    ops.conv_range_word(dev())
    with torch.no_grad():
        eager = stage(x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            stage(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = stage(x)
        y.zero_()
        graph.replay()
    torch.cuda.synchronize()
    _same_bits(y, eager, 'replayed stage')
