# -*- coding: utf-8 -*-
"""What every kernel of librmnet_hip.so is given by the compiler, read from the metadata of a compile-only gfx950 build (no GPU):
LDS bytes, scratch bytes, VGPRs and spilled VGPRs per kernel.

The LDS a kernel is allocated must be what its ``__shared__`` declarations add up to.  More than that means the compiler has moved
a private array into LDS: it does so with arrays of HIP's struct vector types (``uint4 wr[4]``), and that cost the split-fp16
convolutions 16-32 KB of LDS and their whole weight prefetch (profiles/r12_a_weight_prefetch.md).  The expected sizes are
computed here from the tile shapes and from the constants of the sources, restated next to the declarations they stand for;
sizes and register counts only -- no instruction is looked at."""

import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'rmnet_amd', 'csrc')
FIELDS = ('group_segment_fixed_size', 'private_segment_fixed_size', 'vgpr_count', 'vgpr_spill_count')


def _compile(src, out):
    from rmnet_amd import build
    subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                    os.path.join(CSRC, src), '-o', out], check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def _kernels(asm):
    """{mangled name: {field: int}} from the .amdgpu_metadata of one assembly file."""
    m = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', asm, flags=re.S)
    if not m or 'amdhsa.kernels:' not in m.group(1):
        return {}
    body = m.group(1).split('amdhsa.kernels:', 1)[1]
    out = {}
    for entry in re.split(r'\n  - ', body)[1:]:
        entry = '    ' + entry
        get = lambda key: re.search(r'^    \.%s:\s+(\S+)' % key, entry, flags=re.M)
        name = get('name')
        if not name:
            continue
        out[name.group(1)] = {k: int(get(k).group(1)) for k in FIELDS}
    return out


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from rmnet_amd import build
    tmp = tmp_path_factory.mktemp('resources')
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        texts = list(pool.map(lambda s: _compile(s, str(tmp / (s + '.s'))), build.SOURCES))
    found = {}
    for src, text in zip(build.SOURCES, texts):
        for name, res in _kernels(text).items():
            found[name] = dict(res, src=src)
    return found


def _one(kernels, fragment):
    hits = [n for n in kernels if fragment in n]
    assert len(hits) == 1, (fragment, hits)
    return kernels[hits[0]]


# ------------------------------------------------------------------------------------------------ the split-fp16 convolutions
KT = 32
# (WM, WN, TI, TJ, WPE) of conv_split's three tiles (csrc/conv_split.hip, launch_tile), and what WPE allows; each tile has four
# instances <..., XS, OS>: here the fp32 in / fp32 out one (Lb0ELb0), all twelve in tests/test_conv_presplit.py
TILES = {'Big': (2, 4, 4, 4, 2), 'Mid': (2, 4, 4, 2, 4), 'Narrow': (4, 2, 2, 2, 4)}


def _double_buffer_bytes(mt, nt):
    """Two buffers of X hi/lo [MT][32] + W hi/lo [NT][32] fp16."""
    return 2 * (2 * mt * KT + 2 * nt * KT) * 2


def _conv_kernels(kernels):
    out = {'conv3x3_split': (_one(kernels, '13conv3x3_splitE'), 128, 256, 256)}
    for tile, (wm, wn, ti, tj, wpe) in TILES.items():
        k = _one(kernels, '10conv_splitILi%dELi%dELi%dELi%dELi%dELb0ELb0EEE' % (wm, wn, ti, tj, wpe))
        out[tile] = (k, wm * ti * 16, wn * tj * 16, 256 if wpe == 2 else 128)
    return out


def test_the_split_convolutions_get_their_declared_lds_and_keep_their_prefetch_in_registers(kernels):
    """LDS exactly the declared double buffer (96 KB for the two one-workgroup kernels, 64 KB Mid, 48 KB Narrow): the weight
    prefetch array is not in LDS.  No scratch, no spill; at most 256 VGPRs for the kernels that run one workgroup per CU and 128 for
    Mid and Narrow, which run two."""
    conv = _conv_kernels(kernels)
    for name, (k, mt, nt, vgprs) in conv.items():
        print('%-14s LDS %6d  scratch %d  VGPRs %3d  spilled %d' % (name, k['group_segment_fixed_size'], k['private_segment_fixed_size'],
                                                                   k['vgpr_count'], k['vgpr_spill_count']))
    assert _double_buffer_bytes(128, 256) == 98304          # (the figure of the sources' comments)
    for name, (k, mt, nt, vgprs) in conv.items():
        assert k['group_segment_fixed_size'] == _double_buffer_bytes(mt, nt), (name, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (name, k)
        assert k['vgpr_count'] <= vgprs, (name, k)
    assert conv['Mid'][0]['group_segment_fixed_size'] == 65536 and conv['Narrow'][0]['group_segment_fixed_size'] == 49152


# ------------------------------------------------------------------------------------------------ every other kernel
def _declared_lds():
    """{name fragment: bytes}: the __shared__ declarations of every other kernel that has any, added up.  A declaration that an
    instance never reads is not allocated; those are named."""
    f = 4
    d = {}
    # bank.hip: kDe 128, kDo 512, kQT 64, kJT 32, kMaxT 2048, kMaxObj = kBankMaxObj 64
    de, qt, jt, max_t, max_obj = 128, 64, 32, 2048, 64
    d['9bk_appendE'] = jt * (de + 1) * f                                         # tile[kJT][kDe + 1]
    kbuf, pbuf = jt * de * 2, 4 * 2 * 64 * 16
    lds_bytes = 8 * kbuf + 3 * pbuf + 3 * qt * 4 + (max_t + 4) * 4 + max_t * 4 + 12 * 256        # kLdsBytes
    plan = 5 * max_obj * 4 + max_obj * 4 * 4 + 6 * 4 + max_obj * 4               # o_njt .. o_sb, o_rect, plan_n .. sgave, o_c
    for terms in (1, 2, 3):
        d['7bk_mainILi%dEE' % terms] = lds_bytes + plan - 4                       # (plan_c is written, never read)
    # memory_read.hip: kKS 48, kVS 34, kPS 80, kMaxSplits = kSplitMax 64, kThreads 256
    do, ks, vs, ps, splits, threads = 512, 48, 34, 80, 64, 256
    for regional in 'b1', 'b0':
        d['7mr_mainIL%sEE' % regional] = (de * ks + do * vs + jt * ps + qt + 4 + (max_t + 4)) * f          # lds[kLdsFloats]
        for ch in (16, 32):
            n = splits * qt + 4 * qt + ch * (qt + 1) + 4 * qt                    # Wt, red, Tt, red2
            if regional == 'b1':
                n += splits + ch + (threads // ch) * ch                          # Wm, Tm, tp: the mean slot, regional reads only
            d['10mr_combineIL%sELi%dEE' % (regional, ch)] = n * f
    # region_map.hip: red[kThreads / 64][5] ints, box[4] ints
    for frag in ('13region_reduceILb1EE', '13region_reduceILb0EE', '20region_reduce_warpedE'):
        d[frag] = (256 // 64) * 5 * 4
    d['11region_fillILb1EE'] = d['11region_fillILb0EE'] = 4 * 4
    # stem.hip: wlds[KP * 64 * 2] halves + the union of the conv tile [289][64 + 4] floats and the patch planes [39 * 39 * CIN] x 4 B
    for cin in (3, 5):
        kp = (49 * cin + 31) // 32 * 32
        d['10stem_splitILi%dEE' % cin] = kp * 64 * 2 * 2 + max(17 * 17 * (64 + 4) * 4, 39 * 39 * cin * 4)
    # pred_head.hip: lds[kThreads * (kCK + 4)] floats
    d['9pred_headE'] = 512 * (32 + 4) * f
    return d


def test_every_other_kernel_is_allocated_the_lds_it_declares(kernels):
    """Every kernel of build.SOURCES outside the two convolution files: LDS allocated == LDS declared (0 for the kernels without a
    __shared__ declaration; p_kernel's is dynamic).  The figures the library had when this test was written are checked against the
    derivation, so that a slip in the derivation itself shows."""
    declared = _declared_lds()
    assert declared['10stem_splitILi5EE'] == 144144 and declared['10stem_splitILi3EE'] == 119568 and declared['9pred_headE'] == 73728
    others = {n: k for n, k in kernels.items() if k['src'] not in ('conv3x3.hip', 'conv_split.hip')}
    assert len(others) >= 40, sorted(others)
    used = set()
    wrong = []
    for name, k in sorted(others.items()):
        frags = [f for f in declared if f in name]
        assert len(frags) <= 1, (name, frags)
        used.update(frags)
        want = declared[frags[0]] if frags else 0
        if k['group_segment_fixed_size'] != want:
            wrong.append((name, k['src'], k['group_segment_fixed_size'], want))
    assert not wrong, 'LDS allocated != declared (name, file, allocated, declared): %s' % wrong
    assert used == set(declared), sorted(set(declared) - used)
