# -*- coding: utf-8 -*-
"""Per-element tests of the generic memory read (p_kernel / pv_kernel of rmnet_amd/csrc/memory_read.hip) and of the affinity
output p, next to the whole-tensor golden cases of tests/test_gpu_parity.py:
  1. one-hot cases that every element of p and of the read-out must return bit for bit (indexing: tiles, tails, strides, rectangles);
  2. equal-logit cases: p = fl(1 / (T h w)) bit for bit, the read-out bit for bit or inside the bound;
  3. random inputs inside a derived per-element bound;
  4. planted faults (CPU) that show each of the above rejects what it is there for;
  5. the fast shape's p, the TensorBank fallback beyond 2048 frames, the argument rules of the C entry.
The constructions, the exactness argument and the derivation of the bound are in tests/generic_ref.py.

Shapes (no, De, Do, T, h, w) and the branch each enters:
  min     (1, 2, 1, 1, 1, 1)       a soft-max over one cell; three of the four strided sequences are empty
  hw63    (1, 16, 32, 1, 7, 9)     h w = 63: one query tile with one idle lane
  hw64    (1, 3, 17, 2, 8, 8)      h w = 64: a full tile; odd De; pv_kernel's second blockIdx.y holds the one channel 16
  hw65    (2, 4, 5, 3, 5, 13)      h w = 65: a second query tile of one lane; T h w = 195 = 3 (mod 4); Do = 5 (d0 + u < Do); two objects
  tiles3  (3, 16, 16, 2, 3, 43)    h w = 129: three query tiles, three objects
  lds     (1, 224, 4, 1, 2, 5)     De at the LDS limit (57,344 + 1,024 bytes of dynamic LDS)
  tcap    (2, 4, 5, 2, 5, 13)      from tensors with Tcap = 4: channel stride != T h w, the T= argument
  fast    (2, 128, 512, 2, 6, 10)  RMNet's shape on the generic kernels (RMNET_MR_FORCE_GENERIC)
Each runs dense and with the ten rectangle sets of generic_ref.rect_sets (full, beyond the grid on every side, one cell, one row,
one column, empty, a box ending at cell 63, a box starting at cell 64, negative edges, edges >= w / >= h; different per frame and
object).  The one-hot family does not apply to tiles3 and fast: its builder's premise "worst-case fp32 logit error <= 16" fails
there (test_the_onehot_builder_refuses_shapes_beyond_its_premise)."""

import ctypes
import functools
import os

import numpy as np
import pytest

import generic_ref as G

MR_FORCE_GENERIC = 1
MR_ATOL, MR_RTOL = 3e-5, 2e-5           # tests/test_gpu_parity.py: the fp32-class bar of the fast path's default arithmetic

SHAPES = {'min': ((1, 2, 1, 1, 1, 1), None, 0),
          'hw63': ((1, 16, 32, 1, 7, 9), None, 0),
          'hw64': ((1, 3, 17, 2, 8, 8), None, 0),
          'hw65': ((2, 4, 5, 3, 5, 13), None, 0),
          'tiles3': ((3, 16, 16, 2, 3, 43), None, 0),
          'lds': ((1, 224, 4, 1, 2, 5), None, 0),
          'tcap': ((2, 4, 5, 2, 5, 13), 4, 0),
          'fast': ((2, 128, 512, 2, 6, 10), None, MR_FORCE_GENERIC)}
FAMILIES = ('onehot', 'zero', 'orth', 'random')
ONEHOT_BEYOND_PREMISE = ('tiles3', 'fast')
TAGS = ('dense',) + tuple('r%d' % s for s in range(10))


def applies(shape, family):
    return not (family == 'onehot' and shape in ONEHOT_BEYOND_PREMISE)


@functools.lru_cache(maxsize=None)
def get_case(shape, tag, family):
    """The case as built (masked cells hold whatever the builder put there)."""
    dims, tcap, _ = SHAPES[shape]
    no, De, Do, T, h, w = dims
    rects = None
    seed = 0
    if tag != 'dense':
        s = int(tag[1:])
        _, mr, qr, _ = G.rect_sets(no, T, h, w)[s]
        rects, seed = (mr, qr), s + 1
    name = '%s/%s/%s' % (shape, tag, family)
    if family == 'onehot':
        return G.onehot_case(name, dims, rects, tcap, seed)
    if family in ('zero', 'orth'):
        return G.equal_case(name, dims, rects, tcap, seed, variant=family)
    return G.random_case(name, dims, rects, tcap, seed)


@functools.lru_cache(maxsize=None)
def get_exp(shape, tag, family):
    return G.expectations(get_case(shape, tag, family))


def all_keys():
    return [(s, t, f) for s in SHAPES for t in TAGS for f in FAMILIES if applies(s, f)]


# ================================================================================================ CPU: the premises
def test_rectangle_sets_hold_every_kind_for_every_frame_and_object():
    for shape, (dims, _, _) in SHAPES.items():
        no, De, Do, T, h, w = dims
        sets = G.rect_sets(no, T, h, w)
        for o in range(no):
            assert {q[o] for _, _, _, (_, q) in sets} == set(G.KIND_NAMES), shape
            for t in range(T):
                assert {m[o][t] for _, _, _, (m, _) in sets} == set(G.KIND_NAMES), shape
        if no > 1 or T > 1:
            assert all(len({tuple(r) for r in mr.reshape(-1, 4)}) > 1 or no * T == 1 for _, mr, _, _ in sets), shape
        k = G.rect_kinds(h, w)
        assert k['beyond'][0] < 0 and k['beyond'][2] < 0 and k['beyond'][1] >= w and k['beyond'][3] >= h
        assert k['empty'] == (1, 0, 1, 0)
        if h * w > 64:                     # the boxes at the tile boundary: last live cell 63, first live cell 64
            c = dict(no=1, De=1, Do=1, T=1, h=h, w=w, mem_rects=np.array([[k['to63']]], np.int32), qry_rects=np.array([k['from64']], np.int32))
            mm, qm = G.live_masks(c, 0)
            assert np.flatnonzero(mm)[-1] == 63 and np.flatnonzero(qm)[0] == 64, shape


def test_onehot_premises_and_targets():
    """Every one-hot case of the GPU set: the builder's assertions (gap >= 256 in float64, worst-case fp32 logit error <= 16, live
    targets, dot products exact in float32), and the targets named in the issue, over the set."""
    seen = dict(first=False, last=False, box_first=False, box_last=False, res=set(), tiles=set())
    worst_gap, worst_err = np.inf, 0.0
    for shape, tag, family in all_keys():
        if family != 'onehot':
            continue
        case = get_case(shape, tag, family)
        prem = G.onehot_premises(case)
        assert prem['targets_live'] and prem['exact_dot'] and prem['gap'] >= 256.0 and prem['logit_err'] <= 16.0, (case['name'], prem)
        worst_gap, worst_err = min(worst_gap, prem['gap']), max(worst_err, prem['logit_err'])
        no, De, Do, T, h, w = G.dims(case)
        for o in range(no):
            tg = case['targets'][o]
            mm, qm = G.live_masks(case, o)
            assert np.array_equal(tg >= 0, qm & mm.any()), case['name']          # every live query has a target
            L = np.flatnonzero(mm)
            hit = set(int(j) for j in tg[tg >= 0])
            seen['res'] |= {j % 4 for j in hit}
            seen['tiles'] |= {int(i) // 64 for i in np.flatnonzero(tg >= 0)}
            if tag == 'dense':
                seen['first'] |= 0 in hit
                seen['last'] |= T * h * w - 1 in hit
            elif L.size and L.size < T * h * w:
                seen['box_first'] |= int(L[0]) in hit
                seen['box_last'] |= int(L[-1]) in hit
    assert seen['first'] and seen['last'] and seen['box_first'] and seen['box_last'] and seen['res'] == {0, 1, 2, 3}, seen
    assert seen['tiles'] >= {0, 1}, seen
    print('GENERIC onehot premises: smallest gap %.1f, largest worst-case fp32 logit error %.2f' % (worst_gap, worst_err))


def test_the_onehot_builder_refuses_shapes_beyond_its_premise():
    """tiles3 and fast: g^2 >= 512 sqrt(De) with T h w = 258 / 120 cells makes gamma_De sum |k q| / sqrt(De) exceed 16."""
    for shape in ONEHOT_BEYOND_PREMISE:
        with pytest.raises(AssertionError):
            G.onehot_case('x', SHAPES[shape][0])
    assert G.onehot_g(4) == 32 and G.onehot_g(16) == 64 and G.onehot_g(224) == 128


def test_the_issues_worked_example_of_the_onehot_family():
    """De = 4, T = 3, h = 5, w = 13, g = 32: smallest gap 256, exact logits, the right arg-max for every query (numpy float32)."""
    case = get_case('hw65', 'dense', 'onehot')
    assert case['g'] == 32 and G.onehot_premises(case)['gap'] == 256.0
    _, p = G.read_f32(case)
    for o in range(case['no']):
        assert np.array_equal(p[o].argmax(axis=0), case['targets'][o])
        assert np.array_equal(np.sort(p[o], axis=0)[-2:], np.stack([np.zeros(65, np.float32), np.ones(65, np.float32)]))


def test_random_and_equal_cases_keep_expf_inside_its_measured_interval():
    worst = 0.0
    for shape, tag, family in all_keys():
        if family == 'onehot':
            continue
        case = get_case(shape, tag, family)
        sp = max(float(G.spread(case, o).max()) for o in range(case['no']))
        assert sp <= (30.0 if family == 'random' else 0.0), (case['name'], sp)
        worst = max(worst, sp)
    assert worst > 8.0                       # (and the random cases are not flat)
    print('GENERIC largest logit spread of a random case: %.2f' % worst)


@pytest.mark.parametrize('shape', list(SHAPES))
def test_read_f32_meets_read_f64_inside_the_bound_on_every_case(shape):
    """The fp32 restatement against the float64 semantics with the GPU tests' own comparison, on every case of the GPU set, with
    garbage in the masked cells."""
    worst = [0.0, 0.0]
    for s, tag, family in all_keys():
        if s != shape:
            continue
        case = G.filled(get_case(s, tag, family), 'garbage')
        out, p = G.read_f32(case)
        res = G.check(case, get_exp(s, tag, family), out, p)
        assert res['ok'], res['why']
        worst = [max(worst[0], res['ratio_p']), max(worst[1], res['ratio_out'])]
    assert max(worst) < 1.0
    print('GENERIC read_f32 %s: largest error / bound p %.3f out %.3f' % (shape, worst[0], worst[1]))


# ================================================================================================ CPU: the planted faults
# mutant -> the case of the GPU set that rejects it (shape, rectangle set, family, fill) and what about the case does it
MUTANT_CASE = {
    'drop_tail': ('hw65', 'dense', 'zero', 'zero'),                 # T h w = 195: cells 192..194 get p = 0 instead of fl(1 / 195)
    'drop_cell_64': ('hw65', 'dense', 'onehot', 'zero'),            # query cell 64 must hold its target's value vector
    'drop_last_channel': ('hw65', 'dense', 'onehot', 'zero'),       # Do = 5: channel 4 is the tail of d0 + u < Do
    'rect_exclusive': ('hw65', 'r0', 'onehot', 'zero'),             # the last live cell of a box is a target
    'stride_thw': ('tcap', 'dense', 'onehot', 'zero'),              # Tcap = 4, T = 2
    'masked_neg_inf': ('hw65', 'r1', 'random', 'zero'),
    'masked_value_added': ('hw65', 'r1', 'random', 'garbage'),      # only garbage in the masked cells shows it
    'rects_of_object0': ('hw65', 'r1', 'onehot', 'zero'),
    'qval_not_zeroed': ('hw65', 'r1', 'random', 'zero'),
    'sqrt_is_De': ('hw65', 'dense', 'random', 'zero'),              # (the one-hot family cannot see it: the gap stays above 100)
}


@pytest.mark.parametrize('mutant', G.MUTANTS)
def test_each_planted_fault_is_rejected_by_a_named_case(mutant):
    assert set(MUTANT_CASE) == set(G.MUTANTS)
    shape, tag, family, fill = MUTANT_CASE[mutant]
    case = G.filled(get_case(shape, tag, family), fill)
    exp = get_exp(shape, tag, family)
    good = G.check(case, exp, *G.read_f32(case))
    assert good['ok'], good['why']
    bad = G.check(case, exp, *G.read_f32(case, mutant))
    assert not bad['ok'], '%s passes on %s' % (mutant, case['name'])
    print('GENERIC mutant %-18s rejected by %s (%s fill): %s' % (mutant, case['name'], fill, bad['why'][:160]))


def _golden_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, 'memory_reader.npz'))
    cases = []
    for name in ('dense', 'regional', 'allmasked_query', 'tiny_p', 'peaky'):
        mk, mv, qk, qv = (g['%s.%s' % (name, k)] for k in ('m_key', 'm_val', 'q_key', 'q_val'))
        no, De, T, h, w = mk.shape
        for rects in ((False, True) if name + '.mem_rects' in g.files else (False,)):
            c = dict(name='golden %s%s' % (name, ' + rects, dirty' if rects else ''), family='random', no=no, De=De, Do=mv.shape[1], T=T, Tcap=T,
                     h=h, w=w, int_vals=False, m_key=mk, m_val=mv, q_key=qk, q_val=qv,
                     mem_rects=g[name + '.mem_rects'].reshape(no, T, 4) if rects else None,
                     qry_rects=g[name + '.qry_rects'].reshape(no, 4) if rects else None)
            if rects:                       # as test_memory_read_golden_regional_fused_mask does: garbage wherever the masks are zero, q_val too
                c = dict(G.filled(c, 'garbage'), name=c['name'])
                qv2 = qv.copy()
                qv2[qv2 == 0] = np.random.RandomState(0).randn(int((qv2 == 0).sum())).astype(np.float32) * 3
                c['q_val'] = qv2
            cases.append((c, g[name + '.mem_val'], g[name + '.p'] if name + '.p' in g.files else None))
    return cases


def test_what_the_planted_faults_do_against_the_old_bars(golden_dir):
    """The golden cases' inputs (tests/test_gpu_parity.py reads them with flags=1 at MR_ATOL / MR_RTOL, tiny_p's p at 1e-6 / 1e-5)
    through read_f32 with each planted fault: which of them the whole-tensor bars accept.  A record (printed), and one assertion: three
    of the ten faults pass on EVERY golden case -- the golden shapes never enter the branch they break (h w <= 48, Do = 512 or 32,
    Tcap = T) -- each of which a named case above rejects."""
    accepted = {m: 0 for m in G.MUTANTS}
    cases = _golden_cases(golden_dir)
    for c, want, want_p in cases:
        base, _ = G.read_f32(c)
        assert np.allclose(base, want, atol=MR_ATOL, rtol=MR_RTOL), c['name']
        for m in G.MUTANTS:
            out, p = G.read_f32(c, m)
            with np.errstate(invalid='ignore'):
                ok = bool(np.allclose(out, want, atol=MR_ATOL, rtol=MR_RTOL))
                if want_p is not None:
                    ok &= bool(np.allclose(p, want_p, atol=1e-6, rtol=1e-5))
                err = float(np.nanmax(np.abs(out.astype(np.float64) - want)))
            changed = not np.array_equal(out, base)
            accepted[m] += ok
            print('GENERIC old bars, %-34s %-18s changes the read-out: %-5s max err %.2e: %s' % (
                c['name'], m, changed, err, 'ACCEPTED' if ok else 'rejected'))
    through = [m for m in G.MUTANTS if accepted[m] == len(cases)]
    print('GENERIC old bars accept on every golden case: %s' % ', '.join(through))
    assert set(through) == {'drop_cell_64', 'drop_last_channel', 'stride_thw'}


# ================================================================================================ GPU
def dev():
    import torch
    return torch.device('cuda', 0)


def cu(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _read(case, flags=0, want_p=True):
    from rmnet_amd import ops
    out, p = ops.memory_read(cu(case['m_key']), cu(case['m_val']), cu(case['q_key']), cu(case['q_val']), cu(case['mem_rects']),
                             cu(case['qry_rects']), want_p=want_p, flags=flags, T=case['T'])
    return out.cpu().numpy(), (None if p is None else p.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,family', [(s, f) for s in SHAPES for f in FAMILIES if applies(s, f)])
def test_generic_read_per_element(shape, family):
    """Every element of p and out of every case of (shape, family): bit for bit or inside the bound (generic_ref.check).  The same
    bits with zeros and with garbage in the masked cells and in the frames beyond T; the same bits of out with the affinity in the
    workspace (want_p=False) and in the caller's buffer."""
    flags = SHAPES[shape][2]
    worst_p = worst_o = 0.0
    nbits = ncases = 0
    for tag in TAGS:
        exp = get_exp(shape, tag, family)
        base = get_case(shape, tag, family)
        zero = G.filled(base, 'zero')
        out, p = _read(zero, flags, True)
        res = G.check(zero, exp, out, p)
        assert res['ok'], res['why']
        out_ws, none = _read(zero, flags, False)
        assert none is None and np.array_equal(_bits(out_ws), _bits(out)), '%s: out differs with the affinity in the workspace' % zero['name']
        if tag != 'dense' or base['Tcap'] > base['T']:
            out_g, p_g = _read(G.filled(base, 'garbage'), flags, True)
            assert np.array_equal(_bits(out_g), _bits(out)) and np.array_equal(_bits(p_g), _bits(p)), '%s: garbage in masked cells changes the result' % zero['name']
        worst_p, worst_o = max(worst_p, res['ratio_p']), max(worst_o, res['ratio_out'])
        nbits += res['bits_p'] + res['bits_out']
        ncases += 1
        print('GENERIC %-24s error / bound p %.3f out %.3f, bit for bit %d of %d' % (
            zero['name'], res['ratio_p'], res['ratio_out'], res['bits_p'] + res['bits_out'], out.size + p.size))
    assert worst_p < 1.0 and worst_o < 1.0
    print('GENERIC SUMMARY %s %s: %d cases, largest error / bound p %.3f out %.3f, %d elements bit for bit' % (
        shape, family, ncases, worst_p, worst_o, nbits))


def _fast_cases():
    dims = SHAPES['fast'][0]
    sets = G.rect_sets(*[dims[i] for i in (0, 3, 4, 5)])
    yield G.random_case('fastp/dense', dims, None, None, 21)
    for s in (1, 8):                                   # beyond / topleft / botright / cell / row / col / empty among their boxes
        yield G.random_case('fastp/r%d' % s, dims, (sets[s][1], sets[s][2]), None, 22 + s)


@pytest.mark.gpu
def test_fast_shape_affinity_per_element():
    """MemoryReader(return_affinity=True) at RMNet's shape without RMNET_MR_FORCE_GENERIC: the fast path writes out, p_kernel alone
    writes p.  out has the same bits with and without p; p is inside the generic bound per element; the float64 product V p of the
    DEVICE's p agrees with out[:, :Do] inside the sum of the two paths' bounds: sum_j |v_j| dp_j for p, and MR_ATOL + MR_RTOL |out|
    for the fast path -- its default arithmetic (split-fp16 operands) has no derived per-element bound on random inputs
    (bank_ref.tolerance covers the integer cases only), so the fp32-class bar of tests/test_gpu_parity.py stands in for it."""
    from rmnet_amd.rmnet import MemoryReader
    with_p, without = MemoryReader(return_affinity=True), MemoryReader()
    for case in _fast_cases():
        case = G.filled(case, 'garbage')
        exp = G.expectations(case)
        no, De, Do, T, h, w = G.dims(case)
        args = [cu(case[k]) for k in ('m_key', 'm_val', 'q_key', 'q_val', 'mem_rects', 'qry_rects')]
        out, p = with_p(*args)
        out0, none = without(*args)
        out, p, out0 = out.cpu().numpy(), p.cpu().numpy(), out0.cpu().numpy()
        assert none is None and np.array_equal(_bits(out), _bits(out0)), case['name']
        err = np.abs(p.astype(np.float64) - exp['p64'])
        ratio = float((err / exp['bound_p']).max())
        assert (err <= exp['bound_p']).all(), (case['name'], ratio)
        uni = np.broadcast_to(exp['p_exact'][:, None, :], p.shape)
        assert np.array_equal(_bits(p)[uni], _bits(exp['p_bits'])[uni]), case['name']
        assert np.array_equal(_bits(out[:, Do:]), _bits(exp['out_bits'][:, Do:])), case['name']
        worst = 0.0
        for o in range(no):
            mm, _ = G.live_masks(case, o)
            v = np.where(mm, case['m_val'][o][:, :T].reshape(Do, -1).astype(np.float64), 0.0)
            vp = v @ p[o].astype(np.float64)
            got = out[o, :Do].reshape(Do, -1).astype(np.float64)
            tol = np.abs(v) @ exp['bound_p'][o] + MR_ATOL + MR_RTOL * np.abs(got)
            assert (np.abs(vp - got) <= tol).all(), (case['name'], o, float((np.abs(vp - got) / tol).max()))
            worst = max(worst, float((np.abs(vp - got) / tol).max()))
        print('GENERIC %-12s fast path + p: p error / bound %.3f, |V p - out| / tolerance %.3f, %d elements of p bit for bit' % (
            case['name'], ratio, worst, int(uni.sum())))


@functools.lru_cache(maxsize=None)
def _long_cases():
    dims = (1, 128, 512, 2049, 3, 4)
    kinds = G.rect_kinds(3, 4)
    mr = np.array([[kinds[G.KIND_NAMES[(t * 7 + t // 10) % 10]] for t in range(2049)]], np.int32)
    mr[0, 2048] = kinds['topleft']                     # the frame beyond one launch is not empty
    qr = np.array([kinds['beyond']], np.int32)
    rnd = G.random_case('long/random', dims, (mr, qr), 2052, 31)
    eq = G.equal_case('long/zero', dims, (mr, np.array([kinds['botright']], np.int32)), 2052, 32, variant='zero')
    return rnd, eq


def test_long_memory_cases_on_the_cpu():
    """The 2049-frame cases' premises (spread, every rectangle kind among the frames) without the 24,588 x 12 x 512 fp32 restatement."""
    rnd, eq = _long_cases()
    assert float(G.spread(rnd, 0).max()) <= 30.0 and float(G.spread(eq, 0).max()) == 0.0
    assert len({tuple(r) for r in rnd['mem_rects'][0]}) == len(set(G.rect_kinds(3, 4).values()))
    assert G.live_masks(rnd, 0)[0][2048 * 12:].any()


@pytest.mark.gpu
def test_tensor_bank_beyond_one_launch_per_element():
    """ops.TensorBank with capacity 2052 on a 3 x 4 grid, 2049 frames appended with rectangles (some beyond the grid): the read
    warns, falls to the generic kernels with the bank's capacity strides (1.2 MB of workspace) and is inside the bound per element;
    the equal-logit case likewise (p stays in the workspace: out is all there is to compare)."""
    import torch
    from rmnet_amd import ops
    lib_ws = ops._lib.load().rmnet_memory_read_workspace_bytes(1, 128, 512, 2049, 3, 4, MR_FORCE_GENERIC)
    assert lib_ws == (4 * 2049 * 144 + 255) // 256 * 256 and lib_ws < 1.25e6
    for case in _long_cases():
        case = G.filled(case, 'garbage')
        exp = G.expectations(case)
        tb = ops.TensorBank(1, 2052, 3, 4, dev())
        mk, mv, mr = cu(case['m_key']), cu(case['m_val']), cu(case['mem_rects'])
        tb.m_key.fill_(77.0)                            # (what append does not write must not be read as zero)
        tb.m_val.fill_(-55.0)
        for t in range(2049):
            tb.append(t, mk[:, :, t].contiguous(), mv[:, :, t].contiguous(), mr[:, t].contiguous())
        with pytest.warns(UserWarning, match='falling back to the generic path'):
            out = tb.read(2049, cu(case['q_key']), cu(case['q_val']), cu(case['qry_rects']))
        torch.cuda.synchronize()
        res = G.check(case, exp, out.cpu().numpy())
        assert res['ok'], res['why']
        assert res['ratio_out'] < 1.0
        print('GENERIC %-12s TensorBank T = 2049: out error / bound %.3f, %d elements bit for bit' % (case['name'], res['ratio_out'], res['bits_out']))


SENT = 12345.0
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4      # include/rmnet_hip.h


@pytest.mark.gpu
def test_c_entry_argument_rules():
    """rmnet_memory_read_f32 through ctypes on views of one sentinel-filled allocation: every rejection leaves all of it alone, and the
    same call without the fault runs."""
    import torch
    from rmnet_amd import _lib
    lib = _lib.load()
    for no, De, Do, T, h, w in [d for d, _, _ in SHAPES.values()] + [(3, 7, 9, 5, 2, 3)]:
        flags = MR_FORCE_GENERIC if (De, Do) == (128, 512) else 0
        want = (4 * no * T * (h * w) ** 2 + 255) // 256 * 256
        assert lib.rmnet_memory_read_workspace_bytes(no, De, Do, T, h, w, flags) == want, (no, De, Do, T, h, w)
    pool = torch.full((1 << 16,), SENT, dtype=torch.float32, device=dev())
    base = pool.data_ptr()
    assert base % 256 == 0
    at = lambda floats: ctypes.c_void_p(base + 4 * floats)
    rects = torch.tensor([0, 3, 0, 2] * 3, dtype=torch.int32, device=dev())
    no, Do, T, h, w = 1, 8, 2, 3, 4
    thw, hw = T * h * w, h * w
    good = dict(De=16, cs_k=0, cs_v=0, p=None, mr=None, qr=None, ws=at(40960), ws_bytes=None)

    def call(**kw):
        a = dict(good, **kw)
        nb = lib.rmnet_memory_read_workspace_bytes(no, a['De'], Do, T, h, w, 0) if a['ws_bytes'] is None else a['ws_bytes']
        # m_key at 0 (225 * 24 floats at most), m_val at 8192, q_key at 16384, q_val at 24576, out at 28672, p at 32768
        return lib.rmnet_memory_read_f32(at(0), at(8192), at(16384), at(24576), no, a['De'], Do, T, h, w, a['cs_k'], 0, a['cs_v'], 0, at(28672),
                                         a['p'], a['mr'], a['qr'], 0, a['ws'], nb, None)

    need = lib.rmnet_memory_read_workspace_bytes(no, 16, Do, T, h, w, 0)
    r = ctypes.c_void_p(rects.data_ptr())
    cases = [('De = 225', dict(De=225), E_UNSUPPORTED),
             ('workspace one byte short', dict(ws_bytes=need - 1), E_WORKSPACE),
             ('no workspace and no p', dict(ws=None), E_WORKSPACE),
             ('mem_rects without qry_rects', dict(mr=r), E_INVALID),
             ('qry_rects without mem_rects', dict(qr=r), E_INVALID),
             ('key channel stride below T h w', dict(cs_k=thw - 1), E_INVALID),
             ('value channel stride below T h w', dict(cs_v=thw - 1), E_INVALID)]
    for name, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (name, rc, want)
        torch.cuda.synchronize()
        assert bool((pool == SENT).all()), name
    # the same arguments without the fault run: with the workspace; with a NULL workspace when p_out is given; at De = 224
    # (values 0, 1, 2, ... so that the read-out is not the sentinel: equal keys give the mean of each channel, 24 d + 11.5)
    pool[8192:8192 + Do * thw] = torch.arange(Do * thw, dtype=torch.float32, device=dev())
    assert call() == 0
    torch.cuda.synchronize()
    out = pool[28672:28672 + 2 * Do * hw].clone()
    mean = (torch.arange(Do, dtype=torch.float32, device=dev()) * thw + (thw - 1) / 2.0).view(Do, 1).expand(Do, hw)
    assert bool(((out[:Do * hw].view(Do, hw) - mean).abs() <= 1e-4 * mean).all()) and bool((out[Do * hw:] == SENT).all())
    uniform = float(np.float32(1.0) / np.float32(thw))
    assert bool((pool[40960:40960 + thw * hw] == uniform).all())                         # equal inputs: a uniform p, in the workspace
    pool[28672:28672 + 2 * Do * hw] = SENT
    assert call(ws=None, ws_bytes=0, p=at(32768)) == 0
    torch.cuda.synchronize()
    assert torch.equal(pool[28672:28672 + 2 * Do * hw], out)
    assert bool((pool[32768:32768 + thw * hw] == uniform).all()) and bool((pool[32768 + thw * hw:40960] == SENT).all())
    assert call(De=224, ws_bytes=need) == 0 and call(mr=r, qr=r) == 0
    torch.cuda.synchronize()
