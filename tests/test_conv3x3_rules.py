# -*- coding: utf-8 -*-
"""The argument rules of the decoder's three 3x3 exports (csrc/conv3x3_parts.h: conv3x3_args), without a GPU.

rmnet_conv3x3_split_f32, rmnet_conv3x3_split_lds_f32 and rmnet_conv3x3_rows_f32 share one set of rules: everything that is
INVALID_ARG except the overlap first, then Cin % 32 and the 2^31 limit (UNSUPPORTED), then the overlap of out with x (INVALID_ARG);
the rows export then adds Cin == 256 (UNSUPPORTED).  Every call of the table is refused before any launch, so the pointers are
addresses in and around a ctypes buffer and are never dereferenced.  A call that all three rules accept must NOT appear here: it
would launch a kernel on these addresses.

The expected codes are literals.  They were filled by running this table against the library built from the commit before the
three entries shared their rules (three hand-kept copies), which gave the same code for every row from all three exports."""

import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -4
EXPORTS = ['rmnet_conv3x3_split_f32', 'rmnet_conv3x3_split_lds_f32', 'rmnet_conv3x3_rows_f32']
POINTERS = ['x', 'wpack', 'w_unscale', 'bias', 'res', 'out']

_buf = ctypes.create_string_buffer(1 << 16)
P = (ctypes.addressof(_buf) + (1 << 15)) & ~255          # an aligned address in the middle of the buffer


def call(**changes):
    """A call that breaks no rule (N, H, W, Cin = 1, 2, 9, 256; out right behind x), with `changes` applied.  `out` may be a
    function of the call's x and byte counts: out(x, x_bytes, out_bytes)."""
    c = dict(x=P, wpack=P, w_unscale=P, bias=P, res=P, flags=3, N=1, H=2, W=9, Cin=256, out=None)
    c.update(changes)
    M = c['N'] * c['H'] * c['W']
    xb, ob = M * c['Cin'] * 4, M * 256 * 4
    if c['out'] is None:
        c['out'] = lambda x, xb, ob: x + xb               # adjacent: no overlap
    if callable(c['out']):
        c['out'] = c['out'](c['x'], xb, ob)
    return c


first_byte = lambda x, xb, ob: x - ob + 16                # out's last 16 bytes are x's first 16
last_byte = lambda x, xb, ob: x + xb - 16                 # out's first 16 bytes are x's last 16

# (what is wrong, the call, the code)
TABLE = []
for name in ('x', 'wpack', 'w_unscale', 'out'):
    TABLE.append(('%s is null' % name, call(**{name: 0}), INVALID))
for name in ('N', 'H', 'W', 'Cin'):
    TABLE.append(('%s = 0' % name, call(**{name: 0}), INVALID))
    TABLE.append(('%s = -1' % name, call(**{name: -1}), INVALID))
TABLE.append(('an unknown flag bit', call(flags=4), INVALID))
TABLE.append(('an unknown flag bit next to the known ones', call(flags=7), INVALID))
for name in POINTERS:
    mis = call()
    mis[name] += 4
    TABLE.append(('%s misaligned by 4 bytes' % name, mis, INVALID))
TABLE.append(('Cin = 48', call(Cin=48), UNSUPPORTED))
# N*H*W*max(Cin, 256) at 2^31 is refused as UNSUPPORTED; just below it the call reaches the overlap test, which refuses it as
# INVALID_ARG (the same overlap is in the call AT the limit, where the earlier group's code wins)
TABLE.append(('M * 256 = 2^31 (Cin = 256)', call(H=2048, W=4096, out=last_byte), UNSUPPORTED))
TABLE.append(('M * 256 = 2^31 - 256 (Cin = 256), out on x', call(H=1, W=(1 << 23) - 1, out=last_byte), INVALID))
TABLE.append(('M * 256 = 2^31 (Cin = 32: the limit is on max(Cin, 256))', call(H=2048, W=4096, Cin=32, out=last_byte), UNSUPPORTED))
TABLE.append(('M * 256 = 2^31 - 256 (Cin = 32), out on x', call(H=1, W=(1 << 23) - 1, Cin=32, out=last_byte), INVALID))
TABLE.append(('M * 512 = 2^31 (Cin = 512)', call(H=1024, W=4096, Cin=512, out=last_byte), UNSUPPORTED))
TABLE.append(('M * 512 = 2^31 - 512 (Cin = 512), out on x', call(H=1, W=(1 << 22) - 1, Cin=512, out=last_byte), INVALID))
TABLE.append(('out overlaps the first bytes of x', call(out=first_byte), INVALID))
TABLE.append(('out overlaps the last bytes of x', call(out=last_byte), INVALID))
TABLE.append(('out is x', call(out=lambda x, xb, ob: x), INVALID))
# several rules broken at once: the earlier group's code
mis = call(Cin=48)
mis['res'] += 4
TABLE.append(('a misaligned pointer and Cin = 48', mis, INVALID))
TABLE.append(('Cin = 48 and out on x', call(Cin=48, out=first_byte), UNSUPPORTED))

# the rows export's own rule, everything else valid.  ONLY for that export: the other two accept these calls and would launch
ROWS_ONLY = [('Cin = 128', call(Cin=128), UNSUPPORTED), ('Cin = 512', call(Cin=512), UNSUPPORTED)]


def refused(c):
    """conv3x3_args, restated: does the call break a shared rule?"""
    if not (c['x'] and c['wpack'] and c['w_unscale'] and c['out']) or min(c['N'], c['H'], c['W'], c['Cin']) <= 0:
        return True
    if c['flags'] & ~3 or any(c[p] & 15 for p in POINTERS):
        return True
    M = c['N'] * c['H'] * c['W']
    if c['Cin'] % 32 or M * max(c['Cin'], 256) >= 1 << 31:
        return True
    return c['out'] < c['x'] + M * c['Cin'] * 4 and c['x'] < c['out'] + M * 256 * 4


# the guard of this file, at import: no row may be a call that its export accepts
assert len(TABLE) == 32 and all(refused(c) for _, c, _ in TABLE)
assert not any(refused(c) for _, c, _ in ROWS_ONLY) and all(c['Cin'] != 256 for _, c, _ in ROWS_ONLY)


def run(lib, export, c):
    return getattr(lib, export)(c['x'], c['wpack'], c['w_unscale'], c['bias'], c['res'], c['flags'], c['N'], c['H'], c['W'], c['Cin'],
                                c['out'], None, None)


@pytest.fixture(scope='module')
def lib():
    from rmnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('export', EXPORTS)
def test_every_bad_call_gets_the_code_of_its_first_broken_rule(lib, export):
    got = [(what, run(lib, export, c), want) for what, c, want in TABLE]
    assert [g for g in got if g[1] != g[2]] == []


def test_the_three_exports_agree_on_every_row(lib):
    codes = [[run(lib, e, c) for _, c, _ in TABLE] for e in EXPORTS]
    assert codes[0] == codes[1] == codes[2]


def test_the_rows_export_adds_its_cin_rule_after_the_shared_ones(lib):
    got = [(what, run(lib, 'rmnet_conv3x3_rows_f32', c), want) for what, c, want in ROWS_ONLY]
    assert [g for g in got if g[1] != g[2]] == []
