# -*- coding: utf-8 -*-
"""Per-element and bit-exact tests of the exact-fp32 memory read: mr_main / mr_combine of rmnet_amd/csrc/memory_read.hip
(ops.memory_read(..., flags=ops.MR_EXACT_FP32), De = 128, Do = 512): the route of every clip whose bank reports out-of-window
values, and the reference of other tests.  The constructions, the exactness arguments and the derivation of the bound are in
tests/exact_read_ref.py.

Shapes (no, T, h, w), their rectangles and the branch each enters (confirmed from exact_read_ref.plan_of on the CPU, and on the GPU
from the plan record the read leaves in a caller-owned workspace):
  min          1, 1, 1, 1    dense    one cell; inline q_val (h w % 4 != 0)
  hw63/64/65   1, 1, 7x9 / 8x8 / 5x13  dense    an idle lane; a full query tile; a second tile of one lane; copy blocks at 64 only
  tail33       1, 3, 1, 11   dense    M % 32 == 1
  split5       1, 10, 8, 8   dense    njt = 20, nsplit = 5
  split17      1, 35, 8, 8   dense    njt = 70, nsplit = 17: the re-read loops of the merge, uneven split boundaries
  split64      1, 130, 8, 8  dense    njt = 260, nsplit = 64: the cap and its guard
  obj3_split17 3, 35, 8, 8   dense    nsplit = 17 under the 32-channel combine (its batches of four splits and its re-read loops)
  obj2 / obj3  2 / 3, 2, 6, 10  the ten sets of generic_ref.rect_sets    16- / 32-channel combine, per-object plan records and slots
  mean63       1, 2, 8, 16   query box of 63 cells    the mean slot in lane 63 of tile 0
  mean_alone   1, 2, 8, 16   query box of 64 cells    the mean slot alone in tile 1 (the n1 <= n0 return)
  q_empty      2, 2, 5, 13   object 0's query box empty    the fill blocks write every cell
  q_cover      1, 2, 5, 13   boxes beyond the grid on every side    a regional call with nothing masked, N_out = 0
  m_empty      2, 3, 6, 10   every memory box of object 1 empty    M = 0, nsplit = 0, read-out 0; object 0 normal
  gaps         1, 2, 9, 13   the ten sets (a column, a row, a box from cell 64 among them)   masked cells between box columns, rows above / below
  T70 / T130   1, 70 / 130, 5, 6   random boxes, ~30 % empty, empty across frames 63..65 and 127..129    prefix carry once / twice, zero-area frames
  tcap         2, 2, 5, 13   from tensors with Tcap = 4    channel stride != T h w
  misaligned   1, 2, 8, 8    dense and boxed, q_val or out 4 bytes off a 16-byte boundary (ctypes)    inline q_val although h w % 4 == 0
"""

import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_read_ref as X
import generic_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = X.MR_EXACT_FP32
FAMILIES = ('onehot', 'zero', 'orth', 'random', 'spike')
DENSE = ('min', 'hw63', 'hw64', 'hw65', 'tail33', 'split5', 'split17', 'split64', 'obj3_split17')
TEN_SETS = ('obj2', 'obj3', 'gaps')
SHAPES = {'min': (1, 1, 1, 1), 'hw63': (1, 1, 7, 9), 'hw64': (1, 1, 8, 8), 'hw65': (1, 1, 5, 13), 'tail33': (1, 3, 1, 11),
          'split5': (1, 10, 8, 8), 'split17': (1, 35, 8, 8), 'split64': (1, 130, 8, 8), 'obj3_split17': (3, 35, 8, 8), 'obj2': (2, 2, 6, 10), 'obj3': (3, 2, 6, 10),
          'mean63': (1, 2, 8, 16), 'mean_alone': (1, 2, 8, 16), 'q_empty': (2, 2, 5, 13), 'q_cover': (1, 2, 5, 13),
          'm_empty': (2, 3, 6, 10), 'gaps': (1, 2, 9, 13), 'T70': (1, 70, 5, 6), 'T130': (1, 130, 5, 6), 'tcap': (2, 2, 5, 13),
          'misaligned': (1, 2, 8, 8)}
TCAP = {'tcap': 4}
POISONED = ('split17', 'mean_alone', 'q_empty', 'm_empty', 'obj3')


def _long_rects(T, h, w):
    """Random boxes, about 30 % of them empty, empty runs across frames 63..65 and 127..129."""
    rng = np.random.RandomState(T)
    mr = np.zeros((1, T, 4), np.int32)
    for t in range(T):
        x0, y0 = rng.randint(0, w), rng.randint(0, h)
        mr[0, t] = (x0, rng.randint(x0, w), y0, rng.randint(y0, h))
        if rng.rand() < 0.3 or t in (63, 64, 65, 127, 128, 129):
            mr[0, t] = (1, 0, 1, 0)
    mr[0, 0] = (-1, w, 0, h - 2)
    return mr, np.array([[1, w - 2, 0, h - 1]], np.int32)


@functools.lru_cache(maxsize=None)
def variants(shape):
    """[(tag, (mem_rects, qry_rects) or None)] of a shape."""
    no, T, h, w = SHAPES[shape]
    k = G.rect_kinds(h, w)
    arr = lambda rows: np.array(rows, np.int32)
    if shape in DENSE:
        return [('dense', None)]
    if shape in TEN_SETS:
        return [(tag, (mr, qr)) for tag, mr, qr, _ in G.rect_sets(no, T, h, w)]
    if shape == 'mean63':
        return [('box', (arr([[k['full'], k['botright']]]), arr([(0, 8, 0, 6)])))]
    if shape == 'mean_alone':
        return [('box', (arr([[k['full'], k['botright']]]), arr([(4, 11, 0, 7)])))]
    if shape == 'q_empty':
        return [('box', (arr([[k['topleft'], k['full']], [k['row'], k['botright']]]), arr([k['empty'], k['topleft']])))]
    if shape == 'q_cover':
        return [('box', (arr([[k['beyond'], k['beyond']]]), arr([k['beyond']])))]
    if shape == 'm_empty':
        return [('box', (arr([[k['full'], k['cell'], k['topleft']], [k['empty'], (5, 2, 0, 3), (0, 3, 4, 1)]]), arr([k['botright'], k['topleft']])))]
    if shape in ('T70', 'T130'):
        return [('box', _long_rects(T, h, w))]
    if shape == 'tcap':
        s = G.rect_sets(no, T, h, w)[1]
        return [('dense', None), ('r1', (s[1], s[2]))]
    assert shape == 'misaligned'
    return [('dense', None), ('box', (arr([[k['topleft'], k['full']]]), arr([k['botright']])))]


def all_keys():
    return [(s, tag, f) for s in SHAPES for tag, _ in variants(s) for f in FAMILIES]


@functools.lru_cache(maxsize=None)
def get_case(shape, tag, family):
    rects = dict(variants(shape))[tag]
    seed = 0 if tag in ('dense', 'box') else int(tag[1:]) + 1
    name = '%s/%s/%s' % (shape, tag, family)
    args = (name, SHAPES[shape], rects, TCAP.get(shape), seed)
    if family == 'onehot':
        return X.onehot_case(*args)
    if family in ('zero', 'orth'):
        return X.equal_case(*args, variant=family)
    return X.random_case(*args) if family == 'random' else X.spike_case(*args)


@functools.lru_cache(maxsize=None)
def get_exp(shape, tag, family):
    return X.expectations(get_case(shape, tag, family))


# ================================================================================================ CPU: the plan
def test_every_shape_enters_its_named_branch():
    P = {(s, tag): X.plan_of(get_case(s, tag, 'zero')) for s in SHAPES for tag, _ in variants(s)}
    one = lambda s, tag='dense': P[(s, tag)]['objects'][0]
    assert one('min')['M'] == 1 and not P[('min', 'dense')]['copy_blocks']
    assert [one(s)['Mq'] for s in ('hw63', 'hw64', 'hw65')] == [63, 64, 65] and [one(s)['nqt'] for s in ('hw63', 'hw64', 'hw65')] == [1, 1, 2]
    assert [P[(s, 'dense')]['copy_blocks'] for s in ('hw63', 'hw64', 'hw65')] == [False, True, False]
    assert one('tail33')['M'] % 32 == 1 and one('tail33')['njt'] == 2
    assert (one('split5')['njt'], one('split5')['nsplit']) == (20, 5)
    assert (one('split17')['njt'], one('split17')['nsplit']) == (70, 17) and one('split17')['nsplit'] > X.ML_REG_SPLITS
    assert len(set(np.diff(one('split17')['bounds']))) > 1                                    # uneven splits
    assert (one('split64')['njt'], one('split64')['nsplit']) == (260, X.SPLIT_MAX)
    assert [po['nsplit'] for po in P[('obj3_split17', 'dense')]['objects']] == [17] * 3 and P[('obj3_split17', 'dense')]['comb'] == 32
    assert 256 // one('split64')['nqt'] > X.SPLIT_MAX and 260 // X.SPLIT_MIN_TILES > X.SPLIT_MAX   # the cap, nothing else, decides
    for tag, _ in variants('obj2'):
        assert P[('obj2', tag)]['comb'] == 16 and P[('obj3', tag)]['comb'] == 32
        assert [po['record'][8] for po in P[('obj3', tag)]['objects']] == [0, 86, 172] and P[('obj3', tag)]['slots'] == 86
    m63, mal = one('mean63', 'box'), one('mean_alone', 'box')
    assert m63['mean'] and (m63['Mq'], m63['mean_tile'], m63['mean_lane'], m63['nqt'], m63['mean_alone']) == (63, 0, 63, 1, False)
    assert mal['mean'] and (mal['Mq'], mal['mean_tile'], mal['mean_lane'], mal['nqt'], mal['mean_alone']) == (64, 1, 0, 2, True)
    assert mal['fill_rows'] == 0 and m63['fill_rows'] == 1
    qe = P[('q_empty', 'box')]['objects']
    assert qe[0]['Mq'] == 0 and qe[0]['mean'] and qe[0]['fill_rows'] == 5 and qe[0]['nqt'] == 1 and qe[1]['Mq'] > 0
    qc = one('q_cover', 'box')
    assert P[('q_cover', 'box')]['regional'] and not qc['mean'] and qc['n_out'] == 0 and qc['Mq'] == 65 and qc['fill_rows'] == 0
    me = P[('m_empty', 'box')]['objects']
    assert (me[1]['M'], me[1]['nsplit'], me[1]['njt']) == (0, 0, 0) and me[0]['M'] > 0 and me[0]['nsplit'] >= 1
    gq = {tuple(one('gaps', tag)['qr']) for tag, _ in variants('gaps')}
    assert (6, 6, 0, 8) in gq and (0, 12, 4, 4) in gq and (12, 12, 4, 8) in gq          # one column, one row, from cell 64 = (4, 12)
    assert any(0 < one('gaps', tag)['fill_rows'] and one('gaps', tag)['qr'][2] == 0 for tag, _ in variants('gaps'))      # rows below only
    assert any(0 < one('gaps', tag)['fill_rows'] and one('gaps', tag)['qr'][3] == 8 for tag, _ in variants('gaps'))      # rows above only
    for s, chunks in (('T70', 2), ('T130', 3)):
        po = one(s, 'box')
        assert P[(s, 'box')]['prefix_chunks'] == chunks
        frac = np.mean(np.array(po['areas']) == 0)
        assert 0.2 < frac < 0.45 and not any(po['areas'][63:66]) and (s == 'T70' or not any(po['areas'][127:130]))
        assert po['areas'][62] + po['areas'][66] > 0 and sum(po['areas'][64:]) > 0       # live cells beyond the first carry
    # (T130's frames 128 and 129 are empty: the second carry decides M = prefix[T] itself)
    assert get_case('tcap', 'dense', 'zero')['Tcap'] == 4 and get_case('tcap', 'dense', 'zero')['m_key'].shape[2] == 4
    mis = get_case('misaligned', 'box', 'zero')
    assert X.plan_of(mis)['copy_blocks'] and not X.plan_of(mis, aligned=False)['copy_blocks']
    nsp = sorted({po['nsplit'] for p in P.values() for po in p['objects']})
    print('EXACT plans: nsplit values over the set %s' % nsp)


def test_rectangle_kinds_are_spread_over_frames_and_objects():
    for shape in TEN_SETS:
        no, T, h, w = SHAPES[shape]
        sets = G.rect_sets(no, T, h, w)
        for o in range(no):
            assert {q[o] for _, _, _, (_, q) in sets} == set(G.KIND_NAMES), shape
            for t in range(T):
                assert {m[o][t] for _, _, _, (m, _) in sets} == set(G.KIND_NAMES), shape
        assert all(len({tuple(r) for r in mr.reshape(-1, 4)}) > 1 for _, mr, _, _ in sets), shape


def _plan_tuples():
    tuples = []
    for s in SHAPES:
        for tag, _ in variants(s):
            p = X.plan_of(get_case(s, tag, 'zero'))
            no, T, h, w = SHAPES[s]
            tuples += [(po['Mq'], h * w, po['njt'], no, p['slots']) for po in p['objects']]
    rng = np.random.RandomState(3)
    for _ in range(4000):
        no, hw = int(rng.randint(1, 70)), int(rng.randint(1, 2000))
        tuples.append((int(rng.randint(0, hw + 1)), hw, int(rng.randint(0, 2 ** rng.randint(1, 13))), no, X.slots_for(no, hw)))
    return tuples


def test_restated_bank_plan_equals_the_native_one(tmp_path):
    """tests/native/bank_plan_print.cpp prints common.h's bank_plan() for every shape of the set and a random sweep."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    exe = str(tmp_path / 'bank_plan_print')
    cc = subprocess.run([hipcc, '-O1', '-std=c++17', '-w', '--offload-arch=gfx950', os.path.join(ROOT, 'tests', 'native', 'bank_plan_print.cpp'),
                         '-o', exe], capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-2000:]
    tuples = _plan_tuples()
    run = subprocess.run([exe], input=''.join('%d %d %d %d %d\n' % t for t in tuples), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in run.stdout.split('\n') if line]
    assert got == [X.bank_plan(*t) for t in tuples]
    assert 'kSplitMax %d, kSplitMinTiles %d, kSplitTargetSlots %d, kPlanInts %d' % (X.SPLIT_MAX, X.SPLIT_MIN_TILES, X.SPLIT_TARGET, X.PLAN_INTS) in run.stderr


def test_workspace_layout_total_equals_the_librarys_count():
    """(rmnet_memory_read_workspace_bytes launches nothing: it runs without a GPU.)"""
    from rmnet_amd import _lib
    lib = _lib.load()
    shapes = list(SHAPES.values()) + [(8, 5, 30, 54), (64, 2, 3, 4), (65, 2, 3, 4), (130, 1, 9, 9), (1, 2048, 2, 2)]
    for no, T, h, w in shapes:
        lay = X.workspace_layout(no, h * w)
        assert lay['total'] == lib.rmnet_memory_read_workspace_bytes(no, 128, 512, T, h, w, EXACT), (no, T, h, w)
        assert lay['slots'] >= no * X.slots_for(no, h * w) and lay['ml'] % 256 == 0 and lay['plan'] % 256 == 0


def test_xcd_remap_is_a_bijection():
    for n in range(1, 4097):
        b = np.arange(n)
        q, r, x = n >> 3, n & 7, b & 7
        got = np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + (b >> 3)
        assert np.array_equal(np.sort(got), b), n
        assert n > 40 or [X.xcd_remap(i, n) for i in range(n)] == got.tolist()          # (the scalar restatement is the same map)


# ================================================================================================ CPU: the references
def test_case_premises():
    """One-hot: live targets at the named positions, logits 0 or about 362 in float32.  Spike: base spread <= 8 and the three rises
    where the family says; the +20 gives positive arguments without a rescale, the +45 rescales after a split's first tile."""
    named = dict(tile_first=False, tile_last=False, split_last_tile=False, last_split=False, split16=False, tail_last=False, after_empty=False)
    pos_arg = rescale = late = 0
    for s, tag, fam in all_keys():
        case = get_case(s, tag, fam)
        no, T, h, w = SHAPES[s]
        plan = X.plan_of(case)
        if fam == 'onehot':
            for o, po in enumerate(plan['objects']):
                mm, qm = G.live_masks(case, o)
                tg = case['targets'][o]
                assert np.array_equal(tg >= 0, qm & mm.any()) and mm[tg[tg >= 0]].all(), case['name']
                cells = X.compaction(case, o)[0]
                assert np.array_equal(np.sort(cells), np.flatnonzero(mm)), case['name']       # the compaction is the box, clamped
                pos = case['positions'][o]
                hit = {int(np.flatnonzero(cells == t)[0]) for t in set(tg[tg >= 0].tolist())}
                named['tile_first'] |= any(n % 32 == 0 and n > 0 for n in hit)
                named['tile_last'] |= any(n % 32 == 31 for n in hit)
                named['tail_last'] |= po['M'] % 32 != 0 and po['M'] - 1 in hit
                if po['nsplit'] > 1:
                    b = po['bounds']
                    named['split_last_tile'] |= any(n // 32 == b[1] - 1 for n in hit) and any(n // 32 == b[1] for n in hit)
                    named['last_split'] |= any(n // 32 >= b[-2] for n in hit)
                if po['nsplit'] > 16:
                    named['split16'] |= any(b[16] <= n // 32 < b[17] for n in hit) and any(b[15] <= n // 32 < b[16] for n in hit)
                pre = np.concatenate([[0], np.cumsum(po['areas'])])
                named['after_empty'] |= any(po['areas'][t] > 0 and po['areas'][t - 1] == 0 and int(pre[t]) in hit for t in range(1, T))
                k = np.where(mm, case['m_key'][o][:, :T].reshape(128, -1), 0)
                q = np.where(qm, case['q_key'][o].reshape(128, -1), 0)
                dot = k.T.astype(np.float32) @ q.astype(np.float32)
                assert set(np.unique(dot).tolist()) <= {0.0, 4096.0}, case['name']
                if (tg >= 0).any():
                    sel = np.flatnonzero(tg >= 0)
                    assert (dot[tg[sel], sel] == 4096.0).all() and (dot[:, sel] == 4096.0).sum() == sel.size, case['name']
        if fam == 'spike':
            for o, po in enumerate(plan['objects']):
                if po['M'] == 0:
                    continue
                cells, qcells, _ = X.compaction(case, o)
                if qcells.size == 0:
                    continue
                sl = G._logits64(case, o)[0][cells][:, qcells]
                x, nb, _ = X._walk64(sl, po['M'], po['bounds'], case['name'])
                pos_arg += int((x > 10.0).any())
                rescale += int(nb.max() > 0)
                if po['nsplit'] > 1:
                    late += 1
                    assert '+45late' in case['spikes'][o] and case['spikes'][o]['+45late'] // 32 >= po['bounds'][-2]
                if po['njt'] >= 3:                                       # the +20 rise: no rescale at its tile, arguments up to +28
                    n20 = case['spikes'][o]['+20']
                    assert 12.0 - 1e-3 <= float(x[n20].min()) and float(x[n20].max()) <= 28.0 + 1e-3, (case['name'], x[n20].min(), x[n20].max())
                    assert (nb[:32] > 0).all() and (nb[case['spikes'][o]['+45']] == 0).all(), case['name']
    assert all(named.values()), named
    assert pos_arg > 20 and rescale > 20 and late >= 3, (pos_arg, rescale, late)          # (split5, split17 and split64 at least)
    print('EXACT premises: one-hot positions %s; spike cases with positive arguments %d, with a rescale %d, with a late split %d' % (
        sorted(named), pos_arg, rescale, late))


@pytest.mark.parametrize('shape', list(SHAPES))
def test_read_f32_meets_read_f64_on_every_case(shape):
    """The fp32 restatement against the float64 semantics by the GPU tests' own comparison, with junk in the masked cells; bit for
    bit wherever the families say so.  The share of the __expf term A_REL in the bound stays below 1 % for every element."""
    worst = share = 0.0
    nbits = 0
    for s, tag, fam in all_keys():
        if s != shape:
            continue
        case, exp = get_case(s, tag, fam), get_exp(s, tag, fam)
        dirty = X.junked(case)
        out = X.read_f32(dirty)
        assert np.array_equal(_bits(out[:, 512:]), _bits(G.qval_half(dirty))), case['name']
        out[:, 512:] = exp['out_bits'][:, 512:]                              # (q_val's masked cells were junked: compared above)
        res = X.check(case, exp, out)
        assert res['ok'], res['why']
        worst, nbits = max(worst, res['ratio_out']), nbits + res['bits_out']
        b = exp['bound_out'][:, :512]
        if b.max() > 0:
            sh = float((exp['a_share'][:, :512][b > 0] / b[b > 0]).max())
            assert sh < 0.01, (case['name'], sh)
            share = max(share, sh)
        if fam == 'onehot':
            assert exp['out_exact'][:, :512].reshape(exp['onehot'].shape[0], 512, -1)[:, 0][exp['onehot']].all()
    assert worst < 1.0
    print('EXACT read_f32 %-10s largest error / bound %.3f, %d elements bit for bit, largest share of the A term %.2e' % (shape, worst, nbits, share))


# mutant -> the case of the GPU set that rejects it
MUTANT_CASE = {
    'acc_not_rescaled': ('split5', 'dense', 'spike'),
    'lsum_not_rescaled': ('split5', 'dense', 'spike'),
    'nout_dropped_query': ('obj2', 'r1', 'random'),
    'nout_dropped_mean': ('obj2', 'r1', 'zero'),
    'nout_unclamped': ('obj2', 'r0', 'random'),                    # memory boxes 'beyond' the grid
    'ref_not_raised': ('m_empty', 'box', 'random'),                # M = 0: expf(-inf - (-inf)) for the absent splits
    'splits_ge16_ignored': ('split17', 'dense', 'onehot'),
    'uneven_last_tile_dropped': ('split17', 'dense', 'onehot'),
    'tail_logit_zero': ('tail33', 'dense', 'zero'),
    'prefix_carry_dropped': ('T70', 'box', 'onehot'),
    'rects_unclamped': ('obj2', 'r0', 'random'),
    'mean_slot_tile0': ('mean_alone', 'box', 'random'),
    'between_columns_neighbour': ('mean_alone', 'box', 'random'),
    'fill_skipped_mq0': ('q_empty', 'box', 'random'),
    'qval_not_zeroed': ('gaps', 'r2', 'random'),
    'rects_of_object0': ('obj3', 'r1', 'onehot'),
    'stride_thw': ('tcap', 'dense', 'onehot'),
    'sqrt_is_De': ('hw65', 'dense', 'random'),
}


@pytest.mark.parametrize('mutant', X.MUTANTS)
def test_each_planted_fault_is_rejected_by_a_named_case(mutant):
    assert set(MUTANT_CASE) == set(X.MUTANTS)
    key = MUTANT_CASE[mutant]
    case, exp = get_case(*key), get_exp(*key)
    good = X.check(case, exp, X.read_f32(case))
    assert good['ok'], good['why']
    bad = X.check(case, exp, X.read_f32(case, mutant))
    assert not bad['ok'], '%s passes on %s' % (mutant, case['name'])
    print('EXACT mutant %-26s rejected by %s: %s' % (mutant, case['name'], bad['why'][:150]))


VACUITY_SHARE = 0.10       # of the read-out elements of the case must leave the bound


@functools.lru_cache(maxsize=None)
def _vacuity_case(mutant):
    """expf_16ulp: a random case of eight objects with two memory cells and one query each, the keys scaled by 2^-7 (the dot
    product's share of the bound, gamma_128 sum |k q|, then lies below expf's): 16 ulp is about 32 roundings, and a longer memory's
    counted roundings alone exceed that.  merge_weight_2m18: split5's spike case, whose splits without a rise have weights far below 1."""
    if mutant == 'merge_weight_2m18':
        return get_case('split5', 'dense', 'spike')
    case = X.random_case('vacuity/expf', (8, 2, 1, 1), None, None, 7)
    case['m_key'] *= np.float32(2.0 ** -7)
    return case


@pytest.mark.parametrize('mutant', X.VACUITY)
def test_the_bound_is_not_vacuous(mutant):
    """An expf that is 16 ulp off (the sign by the argument's lowest mantissa bit), or the merge weight of one split (a number in
    [0, 1]) off by 2^-18, leaves the bound in at least VACUITY_SHARE of the read-out elements of a case whose unmutated restatement
    is inside it."""
    case = _vacuity_case(mutant)
    exp = X.expectations(case)
    assert X.check(case, exp, X.read_f32(case))['ok']
    out = X.read_f32(case, mutant)
    err = np.abs(out[:, :512].astype(np.float64) - exp['out64'][:, :512])
    frac = float((err > exp['bound_out'][:, :512]).mean())
    print('EXACT vacuity %-18s %.1f %% of the elements of %s leave the bound' % (mutant, 100 * frac, case['name']))
    assert frac >= VACUITY_SHARE, (mutant, frac)


# ================================================================================================ GPU
def dev():
    import torch
    return torch.device('cuda', 0)


def cu(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _read(case, flags=EXACT):
    from rmnet_amd import ops
    out, _ = ops.memory_read(cu(case['m_key']), cu(case['m_val']), cu(case['q_key']), cu(case['q_val']), cu(case['mem_rects']),
                             cu(case['qry_rects']), flags=flags, T=case['T'])
    return out.cpu().numpy()


SENT = 12345.0
GUARD = 64                 # floats before and after out


def _read_c(case, poison=False, qv_off=0, out_off=0):
    """rmnet_memory_read_f32 through ctypes with a caller-owned workspace (0xFF bytes when ``poison``), out pre-filled with SENT inside
    guard bands, q_val / out shifted by ``qv_off`` / ``out_off`` floats off their 256-byte aligned allocation.  Returns (out, the plan
    records [no, 12], the guard bands)."""
    import torch
    from rmnet_amd import _lib
    lib = _lib.load()
    no, T, h, w = X.dims(case)
    mk, mv, qk = cu(case['m_key']), cu(case['m_val']), cu(case['q_key'])
    mr, qr = cu(case['mem_rects']), cu(case['qry_rects'])
    nqv, nout = no * 512 * h * w, no * 1024 * h * w
    qv_buf = torch.zeros(nqv + 8, dtype=torch.float32, device=dev())
    qv_buf[qv_off:qv_off + nqv] = cu(case['q_val']).reshape(-1)
    out_buf = torch.full((nout + 2 * GUARD + 8,), SENT, dtype=torch.float32, device=dev())
    lay = X.workspace_layout(no, h * w)
    nb = lib.rmnet_memory_read_workspace_bytes(no, 128, 512, T, h, w, EXACT)
    assert nb == lay['total']
    ws = torch.full((nb,), 0xFF if poison else 0, dtype=torch.uint8, device=dev())
    assert qv_buf.data_ptr() % 256 == 0 and out_buf.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
    p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)
    cs = case['Tcap'] * h * w
    torch.cuda.synchronize()
    rc = lib.rmnet_memory_read_f32(p(mk), p(mv), p(qk), p(qv_buf, qv_off), no, 128, 512, T, h, w, cs, cs * 128, cs, cs * 512,
                                   p(out_buf, GUARD + out_off), None, p(mr), p(qr), EXACT, p(ws), nb, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    host = out_buf.cpu().numpy()
    out = host[GUARD + out_off:GUARD + out_off + nout].reshape(no, 1024, h, w)
    guards = np.concatenate([host[:GUARD + out_off], host[GUARD + out_off + nout:]])
    rec = ws[lay['plan']:lay['plan'] + no * X.PLAN_INTS * 4].cpu().numpy().view(np.int32).reshape(no, X.PLAN_INTS)
    return out, rec, guards


def _assert_plan(case, rec, aligned=True):
    want = np.array([po['record'] for po in X.plan_of(case, aligned)['objects']], np.int32)
    assert np.array_equal(rec, want), (case['name'], rec.tolist(), want.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('shape,family', [(s, f) for s in SHAPES if s != 'misaligned' for f in FAMILIES])
def test_exact_read_per_element(shape, family):
    """Every element of every case of (shape, family): bit for bit or inside the bound (a NaN fails; the report counts the offenders
    and names the first).  The plan record read back from a caller-owned workspace equals plan_of; the call through the C entry gives
    the bits of ops.memory_read."""
    worst, nbits = 0.0, 0
    for tag, _ in variants(shape):
        case, exp = get_case(shape, tag, family), get_exp(shape, tag, family)
        out = _read(case)
        res = X.check(case, exp, out)
        print('EXACT %-24s largest error / bound %.3f, bit for bit %d of %d' % (case['name'], res['ratio_out'], res['bits_out'], out.size))
        assert res['ok'], res['why']
        out_c, rec, guards = _read_c(case)
        _assert_plan(case, rec)
        assert np.array_equal(_bits(out_c), _bits(out)) and (guards == SENT).all(), case['name']
        worst, nbits = max(worst, res['ratio_out']), nbits + res['bits_out']
    assert worst < 1.0
    print('EXACT SUMMARY %s %s: largest error / bound %.3f, %d elements bit for bit' % (shape, family, worst, nbits))


@pytest.mark.gpu
@pytest.mark.parametrize('tag,which', [('dense', 'q_val'), ('dense', 'out'), ('box', 'q_val'), ('box', 'out')])
def test_misaligned_q_val_or_out_takes_the_inline_path(tag, which):
    """q_val or out 4 bytes off a 16-byte boundary: no copy blocks although h w % 4 == 0; the same bits as the aligned call."""
    for family in FAMILIES:
        case, exp = get_case('misaligned', tag, family), get_exp('misaligned', tag, family)
        ref, rec0, _ = _read_c(case)
        out, rec, guards = _read_c(case, qv_off=1 if which == 'q_val' else 0, out_off=1 if which == 'out' else 0)
        res = X.check(case, exp, out)
        assert res['ok'], res['why']
        _assert_plan(case, rec, aligned=False)
        assert np.array_equal(_bits(out), _bits(ref)) and (guards == SENT).all(), case['name']


@pytest.mark.gpu
@pytest.mark.parametrize('shape', POISONED)
def test_poisoned_workspace(shape):
    """The workspace holds 0xFF bytes (NaN patterns) before the call, out a sentinel between guard bands: every output element is
    written, none is NaN, the guards are untouched, and the result has the bits of the call with a clean workspace."""
    for tag, _ in variants(shape):
        for family in ('random', 'zero'):
            case, exp = get_case(shape, tag, family), get_exp(shape, tag, family)
            out, rec, guards = _read_c(case, poison=True)
            assert (guards == SENT).all(), case['name']
            nan, unwritten = int(np.isnan(out).sum()), int((out == SENT).sum())
            assert nan == 0 and unwritten == 0, '%s: %d NaN, %d elements not written' % (case['name'], nan, unwritten)
            _assert_plan(case, rec)
            res = X.check(case, exp, out)
            assert res['ok'], res['why']
            assert np.array_equal(_bits(out), _bits(_read_c(case)[0])), case['name']


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ['obj2', 'obj3', 'gaps', 'q_empty', 'm_empty', 'mean63', 'mean_alone', 'T70', 'tcap'])
def test_garbage_outside_the_boxes_changes_nothing(shape):
    """Finite junk in every masked key and value cell, in the frames beyond T, and in q_key and q_val of the masked query cells: the
    read-out keeps its bits; the q_val half is the junked q_val inside the box and q_val * 0.0f (its sign kept) outside."""
    for tag, rects in variants(shape):
        if rects is None and shape != 'tcap':
            continue
        case = get_case(shape, tag, 'random')
        dirty = X.junked(case)
        clean, got = _read(case), _read(dirty)
        assert np.array_equal(_bits(got[:, :512]), _bits(clean[:, :512])), case['name']
        want = G.qval_half(dirty)
        assert np.array_equal(_bits(got[:, 512:]), _bits(want)), case['name']
        if rects is not None and any(po['mean'] for po in X.plan_of(case)['objects']):
            assert np.signbit(want[want == 0]).any() and not np.signbit(want[want == 0]).all()      # both zeros occur


@pytest.mark.gpu
@pytest.mark.parametrize('shape,tag', [('split5', 'dense'), ('obj3', 'r3')])
def test_two_calls_and_a_graph_replay_give_equal_bits(shape, tag):
    import torch
    from rmnet_amd import ops
    case = get_case(shape, tag, 'random')
    args = [cu(case[k]) for k in ('m_key', 'm_val', 'q_key', 'q_val', 'mem_rects', 'qry_rects')]
    a = ops.memory_read(*args, flags=EXACT)[0].cpu().numpy()
    b = ops.memory_read(*args, flags=EXACT)[0].cpu().numpy()
    assert np.array_equal(_bits(a), _bits(b))
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        ops.memory_read(*args, flags=EXACT)
    torch.cuda.current_stream(dev()).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.memory_read(*args, flags=EXACT)[0]
    torch.cuda.synchronize()
    out.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(a))


@pytest.mark.gpu
@pytest.mark.parametrize('shape,tag', [('obj3', 'r1'), ('T70', 'box')])
def test_tensor_bank_read_returns_the_bits_of_the_direct_call(shape, tag):
    from rmnet_amd import ops
    case = X.junked(get_case(shape, tag, 'random'))
    no, T, h, w = X.dims(case)
    tb = ops.TensorBank(no, T + 3, h, w, dev())
    tb.m_key.fill_(77.0)
    tb.m_val.fill_(-55.0)
    mk, mv, mr = cu(case['m_key']), cu(case['m_val']), cu(case['mem_rects'])
    for t in range(T):
        tb.append(t, mk[:, :, t].contiguous(), mv[:, :, t].contiguous(), mr[:, t].contiguous())
    out = tb.read(T, cu(case['q_key']), cu(case['q_val']), cu(case['qry_rects'])).cpu().numpy()
    assert np.array_equal(_bits(out), _bits(_read(case))), case['name']
    exp = get_exp(shape, tag, 'random')
    assert np.array_equal(_bits(out[:, 512:]), _bits(G.qval_half(case))), case['name']
    out[:, 512:] = exp['out_bits'][:, 512:]                                  # (q_val's masked cells were junked: compared above)
    res = X.check(case, exp, out)
    assert res['ok'], res['why']


@pytest.mark.gpu
def test_gated_fallback_returns_the_bits_of_the_exact_read():
    """Flags 0 with one key element at 5e3, outside the split-fp16 bank's window: the drop-in entry's transient bank reports it on the
    device and mr_main / mr_combine do the read.  Same inputs for both calls."""
    for tag in ('r1', 'r4'):
        case = dict(get_case('obj2', tag, 'random'))
        mk = case['m_key'].copy()
        cells = X.compaction(case, 0)[0]
        mk[0, 5].reshape(-1)[cells[0]] = np.float32(5e3)                     # a live cell of object 0
        case['m_key'] = mk
        gated, exact = _read(case, flags=0), _read(case, flags=EXACT)
        assert not np.isnan(exact).any() and np.array_equal(_bits(gated), _bits(exact)), case['name']
        clean = _read(get_case('obj2', tag, 'random'), flags=0)
        assert not np.array_equal(_bits(clean), _bits(_read(get_case('obj2', tag, 'random')))), 'the bank path was not taken on clean inputs'
