# -*- coding: utf-8 -*-
"""The regional instance of conv_split (csrc/conv_split.hip: conv_split_region; include/rmnet_hip.h: rmnet_conv_split_region_f32):
the key / value heads computed only for the cells inside one rectangle per image, written NCHW.

  * GPU: against the dense ``ops.conv_split(xs, ..., split=)`` on the same split input, brought to NCHW.  The GEMM's rows are the
    compacted cells, so a cell's K order and operand bits are those of the dense kernel: EVERY element of both outputs is compared
    bit for bit with ``where(inside, dense, +0.0)``, on outputs that held NaN before the call.  Maps of 9 x 14 (126 cells: one
    128-row tile holds an object and part of the next) and 12 x 23 (276 cells: a rectangle crosses tile boundaries), batch 3,
    Cin 64, Cout 256 / split 128 (two channel slices, one per output) and Cout 128 / split 32 (one slice, both outputs).  The range
    word is what it was.
  * CPU: a table of refused calls with literal codes, in the manner of tests/test_conv3x3_rules.py, and the instance's registers,
    spills, scratch and LDS from the code object's metadata.

The rectangle of 128 + 1 cells: 129 = 3 x 43 has no rectangle inside either map.  What the case is for -- a second tile that holds
one row -- is built from a 128-cell box followed by a one-cell box, and the smallest area above 128 that a box of the 12 x 23 map
has, 130 = 13 x 10, is there too; the 9 x 14 map has 126 cells, so its interior boxes are smaller."""

import ctypes

import pytest
import torch

INVALID, UNSUPPORTED = -1, -4
X_SPLIT, OUT_SPLIT, RELU_IN, RELU_OUT = 4, 8, 1, 2
N, CIN = 3, 64
MAPS = {'9x14': (9, 14), '12x23': (12, 23)}
CHANNELS = {'256/128': (256, 128), '128/32': (128, 32)}


def rect_sets(H, W):
    """{name: three rectangles (cx0, cx1, cy0, cy1)}, mixed so that tiles span objects."""
    whole = (0, W - 1, 0, H - 1)
    empty = (5, 4, 2, 6)                                   # cx1 < cx0
    sets = {
        'whole | corner | row': [whole, (0, 0, 0, 0), (0, W - 1, H // 2, H // 2)],
        'column | left | right': [(W // 3, W // 3, 0, H - 1), (0, 3, 2, 5), (W - 4, W - 1, 2, 5)],
        'top | bottom | corner': [(3, 7, 0, 2), (3, 7, H - 3, H - 1), (W - 1, W - 1, H - 1, H - 1)],
        'empty | beyond every side | corner': [empty, (-3, W + 2, -2, H + 4), (W - 1, W - 1, 0, 0)],
        'half outside | whole | whole': [(-2, 3, -1, 2), whole, whole],
        'corner | empty rows | last row': [(0, 0, H - 1, H - 1), (2, 6, 4, 3), (0, W - 1, H - 1, H - 1)],      # cy1 < cy0
        'all empty': [empty, (1, 0, 1, 0), (W, W + 3, 0, H - 1)],                                               # the last: right of the map
    }
    if (H, W) == (12, 23):
        sets['128 cells | one cell | 130 cells'] = [(2, 17, 2, 9), (20, 20, 10, 10), (1, 13, 1, 10)]
        sets['192 cells | 128 cells | whole'] = [(2, 17, 0, 11), (1, 16, 2, 9), whole]
    else:
        sets['interior | interior | interior'] = [(2, 11, 2, 6), (1, 12, 1, 7), (3, 4, 3, 4)]
    return sets


def clamp(r, H, W):
    cx0, cx1, cy0, cy1 = max(r[0], 0), min(r[1], W - 1), max(r[2], 0), min(r[3], H - 1)
    return (cx0, cx1, cy0, cy1) if cx1 >= cx0 and cy1 >= cy0 else None


def area(r, H, W):
    c = clamp(r, H, W)
    return 0 if c is None else (c[1] - c[0] + 1) * (c[3] - c[2] + 1)


CASES = [(m, s) for m, hw in MAPS.items() for s in rect_sets(*hw)]


def test_the_cases_are_what_their_names_say():
    """The areas the cases are there for: a tile that holds an object and part of the next, rectangles that cross tile boundaries, a
    multiple of 128, 128 + 1 rows in all, nothing at all."""
    a = {(m, s): [area(r, *MAPS[m]) for r in rs] for m in MAPS for s, rs in rect_sets(*MAPS[m]).items()}
    assert a[('9x14', 'whole | corner | row')] == [126, 1, 14] and a[('12x23', 'whole | corner | row')] == [276, 1, 23]
    assert a[('12x23', '128 cells | one cell | 130 cells')] == [128, 1, 130]
    assert a[('12x23', '192 cells | 128 cells | whole')] == [192, 128, 276]      # (object 1 is 128 rows that straddle tiles 1 and 2)
    assert a[('9x14', 'empty | beyond every side | corner')] == [0, 126, 1] and a[('9x14', 'half outside | whole | whole')] == [12, 126, 126]
    assert a[('9x14', 'all empty')] == [0, 0, 0] and a[('12x23', 'all empty')] == [0, 0, 0]
    assert a[('12x23', 'corner | empty rows | last row')] == [1, 0, 23]
    assert len(CASES) == 8 + 9


# ================================================================================================ GPU: every element, bit for bit
def dev():
    return torch.device('cuda', 0)


_cache = {}


def _problem(map_name, ch_name):
    """The split input, the pack and the dense heads as NCHW tensors: computed once per (map, channels) and left unchanged."""
    key = (map_name, ch_name)
    if key not in _cache:
        from rmnet_amd import ops
        H, W = MAPS[map_name]
        cout, split = CHANNELS[ch_name]
        g = torch.Generator().manual_seed(33 + 7 * len(_cache))
        x = torch.randn(N, CIN, H, W, generator=g).to(dev()).contiguous(memory_format=torch.channels_last)
        wp, wu = ops.conv_split_pack(torch.randn(cout, CIN, 3, 3, generator=g) * 0.05)
        shift = torch.randn(cout, generator=g).to(dev())
        rw = torch.zeros(1, dtype=torch.int32, device=dev())
        xs = ops.split_act(x, range_word=rw)
        wp, wu = wp.to(dev()), wu.to(dev())
        k, v = ops.conv_split(xs, wp, wu, shift, ksize=3, range_word=rw, split=split)
        assert int(rw.item()) == 0 and not ops._is_cl(k.contiguous())
        _cache[key] = (xs, wp, wu, shift, k.contiguous(), v.contiguous())
        assert _cache[key][4].is_contiguous() and bool(torch.isfinite(_cache[key][4]).all()) and bool((_cache[key][5] != 0).any())
    return _cache[key]


def _inside(rects, H, W):
    m = torch.zeros(N, 1, H, W, dtype=torch.bool)
    for o, r in enumerate(rects):
        c = clamp(r, H, W)
        if c is not None:
            m[o, 0, c[2]:c[3] + 1, c[0]:c[1] + 1] = True
    return m.to(dev())


def _bits_equal(got, want, what):
    gi, wi = got.view(torch.int32), want.view(torch.int32)
    if torch.equal(gi, wi):
        return
    bad = (gi != wi).nonzero()
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]
    pytest.fail('%s: %d of %d elements differ; first (index, got, want): %s' % (what, bad.shape[0], got.numel(), first))


@pytest.mark.gpu
@pytest.mark.parametrize('ch_name', list(CHANNELS))
@pytest.mark.parametrize('map_name,set_name', CASES)
def test_inside_the_rectangles_the_dense_bits_and_plus_zero_everywhere_else(map_name, set_name, ch_name):
    from rmnet_amd import ops
    H, W = MAPS[map_name]
    cout, split = CHANNELS[ch_name]
    xs, wp, wu, shift, k_ref, v_ref = _problem(map_name, ch_name)
    rects = rect_sets(H, W)[set_name]
    rt = torch.tensor(rects, dtype=torch.int32, device=dev())
    rw = torch.full((1,), 7, dtype=torch.int32, device=dev())
    k = torch.full((N, split, H, W), float('nan'), device=dev())
    v = torch.full((N, cout - split, H, W), float('nan'), device=dev())
    got = ops.conv_split(xs, wp, wu, shift, ksize=3, range_word=rw, split=split, rects=rt, _out=(k, v))
    assert got[0] is k and got[1] is v
    inside = _inside(rects, H, W)
    zero = torch.zeros((), device=dev())
    for name, g, ref in (('key', k, k_ref), ('value', v, v_ref)):
        assert not bool(torch.isnan(g).any()), '%s: a cell was not written' % name
        assert bool((g.masked_select(~inside.expand_as(g)) == 0).all()), '%s: not zero outside the rectangles' % name
        _bits_equal(g, torch.where(inside, ref, zero), name)             # every element: the dense bits inside, +0.0 outside
    assert int(rw.item()) == 7
    assert torch.equal(rt.cpu(), torch.tensor(rects, dtype=torch.int32))


@pytest.mark.gpu
def test_the_call_allocates_nchw_outputs_and_python_refuses_what_the_kernel_does_not_serve():
    from rmnet_amd import ops
    H, W = MAPS['9x14']
    xs, wp, wu, shift, k_ref, v_ref = _problem('9x14', '256/128')
    rects = [(0, W - 1, 0, H - 1)] * N
    rt = torch.tensor(rects, dtype=torch.int32, device=dev())
    k, v = ops.conv_split(xs, wp, wu, shift, ksize=3, split=128, rects=rt, relu_out=True)
    assert k.is_contiguous() and v.is_contiguous() and tuple(k.shape) == (N, 128, H, W) and tuple(v.shape) == (N, 128, H, W)
    _bits_equal(k, torch.relu(k_ref), 'key, relu_out')
    _bits_equal(v, torch.relu(v_ref), 'value, relu_out')
    x32 = torch.zeros(N, CIN, H, W, device=dev()).contiguous(memory_format=torch.channels_last)
    for bad in (dict(x=x32), dict(split=None), dict(stride=2), dict(rects=rt[:2]), dict(rects=rt.long()), dict(rects=rt.cpu()),
                dict(out_presplit=True), dict(split=130)):
        kw = dict(x=xs, split=128, stride=1, rects=rt, out_presplit=False)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.conv_split(kw.pop('x'), wp, wu, shift, ksize=3, **kw)
    with pytest.raises(RuntimeError):
        ops.conv_split(xs, wp, wu, shift, ksize=3, split=128, _out=(k, v))


# ================================================================================================ CPU: the argument rules
POINTERS = ['x', 'wpack', 'w_unscale', 'shift', 'rects', 'out', 'out2']
_buf = ctypes.create_string_buffer(1 << 16)
P = (ctypes.addressof(_buf) + (1 << 15)) & ~255          # an aligned address in the middle of the buffer


def call(**changes):
    """A call that breaks no rule (N, H, W, Cin, Cout, split = 1, 2, 9, 64, 128, 32; rects in front of x, out and out2 behind it),
    with `changes` applied.  out / out2 / rects may be functions of the call's addresses and byte counts."""
    c = dict(x=P, wpack=P, w_unscale=P, shift=P, flags=X_SPLIT, N=1, H=2, W=9, Cin=64, Cout=128, ksize=3, stride=1, rects=P - 256,
             out=None, out2=None, out_split=32)
    c.update(changes)
    M = c['N'] * c['H'] * c['W']
    s = dict(x=c['x'], xb=M * c['Cin'] * 4, ob=M * c['out_split'] * 4, o2b=M * (c['Cout'] - c['out_split']) * 4, rects=c['rects'])
    if c['out'] is None:
        c['out'] = lambda s: s['x'] + s['xb']
    if callable(c['out']):
        c['out'] = c['out'](s)
    s['out'] = c['out']
    if c['out2'] is None:
        c['out2'] = lambda s: s['out'] + s['ob']
    if callable(c['out2']):
        c['out2'] = c['out2'](s)
    return c


TABLE = []
for name in ('x', 'wpack', 'w_unscale', 'out', 'rects', 'out2'):
    TABLE.append(('%s is null' % name, call(**{name: (lambda s: 0) if name in ('out', 'out2') else 0}), INVALID))
for name in ('N', 'H', 'W', 'Cin', 'Cout'):
    TABLE.append(('%s = 0' % name, call(**{name: 0}), INVALID))
TABLE.append(('fp32 input (no RMNET_CONV_X_SPLIT)', call(flags=0), INVALID))
TABLE.append(('fp32 input with the output ReLU', call(flags=RELU_OUT), INVALID))
TABLE.append(('a split output asked for', call(flags=X_SPLIT | OUT_SPLIT), INVALID))
TABLE.append(('the input ReLU asked for', call(flags=X_SPLIT | RELU_IN), INVALID))
TABLE.append(('an unknown flag bit', call(flags=X_SPLIT | 16), INVALID))
for name in POINTERS:
    mis = call()
    mis[name] += 4
    TABLE.append(('%s misaligned by 4 bytes' % name, mis, INVALID))
for sp in (0, 128, 30, -4):
    TABLE.append(('out_split = %d' % sp, call(out_split=sp), INVALID))
TABLE.append(('ksize = 1', call(ksize=1), UNSUPPORTED))
TABLE.append(('ksize = 5', call(ksize=5), UNSUPPORTED))
TABLE.append(('stride = 2', call(stride=2), UNSUPPORTED))
TABLE.append(('Cout = 64', call(Cout=64), UNSUPPORTED))
TABLE.append(('Cout = 192', call(Cout=192), UNSUPPORTED))
TABLE.append(('Cin = 48', call(Cin=48), UNSUPPORTED))
TABLE.append(('N = 65 (more than the tables hold)', call(N=65), UNSUPPORTED))
TABLE.append(('N*H*W*Cout = 2^31', call(H=4096, W=4096), UNSUPPORTED))
TABLE.append(('out on the last bytes of x', call(out=lambda s: s['x'] + s['xb'] - 16, out2=lambda s: s['x'] + s['xb'] + (1 << 12)), INVALID))
TABLE.append(('out is x', call(out=lambda s: s['x'], out2=lambda s: s['x'] + s['xb'] + (1 << 12)), INVALID))
TABLE.append(('out2 on the first bytes of x', call(out2=lambda s: s['x'] - s['o2b'] + 16, rects=P - (1 << 14)), INVALID))
TABLE.append(('out2 on the last bytes of out', call(out2=lambda s: s['out'] + s['ob'] - 16), INVALID))
XB, OB, O2B = 18 * 64 * 4, 18 * 32 * 4, 18 * 96 * 4       # the base call's bytes of x, out and out2 (out at P + XB, out2 behind it)
TABLE.append(('rects inside out', call(rects=P + XB + 16), INVALID))
TABLE.append(('rects on the last bytes of out2', call(rects=P + XB + OB + O2B - 16), INVALID))
# several rules broken at once: the earlier group's code
mis = call(ksize=1)
mis['shift'] += 4
TABLE.append(('a misaligned pointer and ksize = 1', mis, INVALID))
TABLE.append(('stride = 2 and out on x', call(stride=2, out=lambda s: s['x'], out2=lambda s: s['x'] + s['xb'] + (1 << 12)), UNSUPPORTED))
TABLE.append(('null rects and Cout = 64', call(rects=0, Cout=64), INVALID))


def refused(c):
    """The rules, restated: does the call break one?"""
    if not (c['x'] and c['wpack'] and c['w_unscale'] and c['out']) or min(c['N'], c['H'], c['W'], c['Cin'], c['Cout']) <= 0:
        return True
    if c['flags'] & ~(X_SPLIT | RELU_OUT) or not c['flags'] & X_SPLIT or not c['rects'] or not c['out2']:
        return True
    if any(c[p] & 15 for p in POINTERS) or not 0 < c['out_split'] < c['Cout'] or c['out_split'] % 4:
        return True
    if c['ksize'] != 3 or c['stride'] != 1 or c['Cin'] % 32 or c['Cout'] % 128 or c['N'] > 64:
        return True
    M = c['N'] * c['H'] * c['W']
    if M * max(c['Cin'], c['Cout']) >= 1 << 31:
        return True
    spans = [(c['x'], M * c['Cin'] * 4), (c['out'], M * c['out_split'] * 4), (c['out2'], M * (c['Cout'] - c['out_split']) * 4),
             (c['rects'], 16 * c['N'])]
    hit = lambda a, b: a[0] < b[0] + b[1] and b[0] < a[0] + a[1]
    return hit(spans[1], spans[0]) or hit(spans[2], spans[0]) or hit(spans[2], spans[1]) or hit(spans[1], spans[3]) or hit(spans[2], spans[3])


# the guard of this file, at import: the base call breaks no rule (it is never made), and no row is a call that the export accepts
assert not refused(call()) and not refused(call(flags=X_SPLIT | RELU_OUT)) and not refused(call(N=64))
assert len(TABLE) == 44 and all(refused(c) for _, c, _ in TABLE), [w for w, c, _ in TABLE if not refused(c)]


def test_every_bad_call_gets_the_code_of_its_first_broken_rule():
    """Everything is refused before any launch, so the pointers are addresses in and around a ctypes buffer that nobody reads."""
    from rmnet_amd import _lib
    lib = _lib.load()
    run = lambda c: lib.rmnet_conv_split_region_f32(c['x'], c['wpack'], c['w_unscale'], c['shift'], c['flags'], c['N'], c['H'], c['W'],
                                                    c['Cin'], c['Cout'], c['ksize'], c['stride'], c['rects'], c['out'], c['out2'],
                                                    c['out_split'], None, None)
    got = [(what, run(c), want) for what, c, want in TABLE]
    assert [g for g in got if g[1] != g[2]] == []


def test_the_switch_is_read_at_every_call_and_a_bad_value_raises(monkeypatch):
    from rmnet_amd import ops
    monkeypatch.delenv('RMNET_KV_REGION', raising=False)
    assert ops.kv_region_enabled() is ops.KV_REGION_DEFAULT
    monkeypatch.setenv('RMNET_KV_REGION', '0')
    assert ops.kv_region_enabled() is False
    monkeypatch.setenv('RMNET_KV_REGION', ' 1 ')
    assert ops.kv_region_enabled() is True
    for bad in ('', 'yes', '2'):
        monkeypatch.setenv('RMNET_KV_REGION', bad)
        with pytest.raises(RuntimeError):
            ops.kv_region_enabled()


# ================================================================================================ CPU: what the compiler gives
def test_the_regional_instance_keeps_two_workgroups_per_cu(tmp_path):
    """Compile-only, with tests/test_kernel_resources.py's compile step and metadata reader: no scratch, no spill, at most 128 VGPRs
    (4 waves per SIMD) and the Mid tile's 64 KB double buffer plus the row map's tables -- (64 + 1) prefix words and 64 rectangles
    -- inside 80 KB, so that two workgroups share a CU's 160 KB as the dense Mid instances do."""
    import test_kernel_resources as KR
    found = KR._kernels(KR._compile('conv_split.hip', str(tmp_path / 'conv_split.s')))
    k = KR._one(found, '17conv_split_regionE')
    print('conv_split_region  LDS %6d  scratch %d  VGPRs %3d  spilled %d'
          % (k['group_segment_fixed_size'], k['private_segment_fixed_size'], k['vgpr_count'], k['vgpr_spill_count']))
    assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
    assert k['vgpr_count'] <= 128, k
    assert k['group_segment_fixed_size'] == KR._double_buffer_bytes(128, 128) + (64 + 1) * 4 + 64 * 4 * 4, k
    assert k['group_segment_fixed_size'] <= 80 * 1024, k
