# -*- coding: utf-8 -*-
"""Gradients of the memory read: rmnet_memory_read_backward_f32 (rmnet_amd/csrc/memory_read_bwd.hip), ops.memory_read_backward and the
autograd wiring of ops.memory_read / rmnet.MemoryReader.  The references, the exactness arguments and the derivation of the bound
are in tests/read_backward_ref.py; the cases come from tests/generic_ref.py.

Shapes (no, De, Do, T, h, w), Tcap, and the seam each reaches (the kernels' tiles: 32 memory cells x 32 queries, 64 queries in the
statistics pass, 64 value channels per stage, De padded to 4 / 16):
  min    (1, 4, 1, 1, 1, 1)         M = 1: a soft-max over one cell; Do = 1; one lane of every tile
  s35    (1, 20, 24, 2, 3, 5)   4   h w = 15 < a tile; De = 20 (padded to 32 as an output row); Tcap = T + 2
  s57    (3, 4, 1, 3, 5, 7)         h w = 35: a second query tile of 3; three objects; T = 3; M = 105
  s79    (1, 224, 40, 1, 7, 9)      De at the limit (14 output row tiles, 106 KB of LDS); h w = 63: one idle lane in the statistics
  s88    (1, 4, 1, 2, 8, 8)     4   h w = 64: full tiles everywhere, M = 128 a power of two (the exact equal-logit family); Tcap = T + 2
  s513   (3, 20, 24, 5, 5, 13)      h w = 65: a third query tile / a second statistics tile of one lane; T = 5; M = 325
  fast   (1, 128, 512, 2, 10, 13) 4 RMNet's channels: eight value stages, the > 64 KB LDS request; h w = 130; Tcap = T + 2
  fast3  (3, 128, 512, 1, 3, 5)     RMNet's channels with three objects
Every shape runs dense and with rectangle sets of generic_ref.rect_sets; `fast` runs all ten, so every rectangle kind (full, beyond
the grid, one cell, one row, one column, empty, ending at cell 63, starting at cell 64, negative edges, edges >= w / >= h) is a
query box and a memory box at the (128, 512) shape."""

import ctypes
import functools

import numpy as np
import pytest

import generic_ref as G
import read_backward_ref as B

SHAPES = {'min': ((1, 4, 1, 1, 1, 1), None),
          's35': ((1, 20, 24, 2, 3, 5), 4),
          's57': ((3, 4, 1, 3, 5, 7), None),
          's79': ((1, 224, 40, 1, 7, 9), None),
          's88': ((1, 4, 1, 2, 8, 8), 4),
          's513': ((3, 20, 24, 5, 5, 13), None),
          'fast': ((1, 128, 512, 2, 10, 13), 4),
          'fast3': ((3, 128, 512, 1, 3, 5), None)}
RECT_TAGS = {'min': ('r0', 'r5'), 's35': ('r0', 'r5'), 's57': ('r1', 'r6'), 's79': ('r2', 'r7'), 's88': ('r3', 'r8'), 's513': ('r4', 'r9'),
             'fast': tuple('r%d' % s for s in range(10)), 'fast3': ('r2',)}
# family: 'random' (bounded), 'm1' / 'zero' / 'orth' / 'onehot' with integer values and an integer gradient (bit for bit)
KEYS = [(s, t, 'random') for s in SHAPES for t in ('dense',) + RECT_TAGS[s]]
KEYS += [('min', t, 'm1') for t in ('dense', 'r0')]
KEYS += [('s88', t, f) for t in ('dense', 'r3', 'r8') for f in ('zero', 'orth')] + [('s513', 'r4', 'zero'), ('fast3', 'dense', 'zero')]
KEYS += [(s, t, 'onehot') for s, tags in (('s35', ('dense', 'r5')), ('s57', ('dense', 'r1')), ('s88', ('dense', 'r3', 'r8')))
         for t in tags]
EXACT_FAMILIES = ('m1', 'zero', 'orth', 'onehot')


def key_id(k):
    return '-'.join(k)


@functools.lru_cache(maxsize=None)
def get_case(shape, tag, family):
    dims, tcap = SHAPES[shape]
    no, De, Do, T, h, w = dims
    rects, seed = None, 0
    if tag != 'dense':
        s = int(tag[1:])
        _, mr, qr, _ = G.rect_sets(no, T, h, w)[s]
        rects, seed = (mr, qr), s + 1
    name = '%s/%s/%s' % (shape, tag, family)
    if family == 'onehot':
        return B.with_int_values(G.onehot_case(name, dims, rects, tcap, seed))
    if family in ('zero', 'orth'):
        return B.with_int_values(G.equal_case(name, dims, rects, tcap, seed, variant=family))
    case = G.random_case(name, dims, rects, tcap, seed)
    return B.with_int_values(case) if family == 'm1' else case


@functools.lru_cache(maxsize=None)
def get_gout(shape, tag, family):
    g = B.grad_out_for(get_case(shape, tag, family), seed=len(tag) + len(family), ints=family in EXACT_FAMILIES)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def get_mem_val(shape, tag, family):
    """The forward's output handed to the backward: the float64 read, rounded (shared, read-only)."""
    m = G.read_f64(get_case(shape, tag, family))[0].astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def get_exact(shape, tag, family):
    if family not in EXACT_FAMILIES:
        return None
    return B.exact_expectations(get_case(shape, tag, family), get_gout(shape, tag, family))[1]


def check_key(key, got, mem_val=None, names=B.NAMES):
    case = get_case(*key)
    return B.check(case, get_gout(*key), got, mem_val=get_mem_val(*key) if mem_val is None else mem_val, exact=get_exact(*key),
                   extreme=key[2] == 'onehot', names=names)


# ================================================================================================ CPU: grad_f64 by hand
def _tiny(no, De, Do, T, h, w, rects=None, seed=1):
    return G.random_case('tiny', (no, De, Do, T, h, w), rects, None, seed)


def test_grad_f64_m1_is_the_identity_on_values():
    """M = 1: P = 1, dK = dQ = 0, dV[d] = sum_n G[d, n]."""
    case = _tiny(1, 4, 3, 1, 1, 1)
    g = B.grad_out_for(case)
    r = B.grad_f64(case, g)
    assert np.array_equal(r['d_m_val'].ravel(), g[0, :3].ravel().astype(np.float64))
    assert not r['d_m_key'].any() and not r['d_q_key'].any()
    assert np.array_equal(r['d_q_val'], g[:, 3:].astype(np.float64))


def test_grad_f64_zero_keys_spread_the_gradient_evenly():
    """K = 0, M = 16: dV[d, m] = sum_n G[d, n] / 16, dQ = 0, dK[c, m] = sum_n Q[c, n] (v_m . G_n - mean_m' v_m' . G_n) / (16 sqrt(De))."""
    case = G.equal_case('k0', (1, 4, 3, 1, 4, 4), variant='zero')
    g = B.grad_out_for(case)
    r = B.grad_f64(case, g)
    G1 = g[0, :3].reshape(3, 16).astype(np.float64)
    V = case['m_val'][0].reshape(3, 16).astype(np.float64)
    Q = case['q_key'][0].reshape(4, 16).astype(np.float64)
    np.testing.assert_allclose(r['d_m_val'][0].reshape(3, 16), np.repeat(G1.sum(axis=1, keepdims=True) / 16, 16, axis=1), rtol=1e-14)
    assert not r['d_q_key'].any()
    vg = V.T @ G1                                                # [m, n]
    want = Q @ ((vg - vg.mean(axis=0)) / 16).T / 2.0             # sqrt(4) = 2
    np.testing.assert_allclose(r['d_m_key'][0].reshape(4, 16), want, rtol=1e-12, atol=1e-12)


def test_grad_f64_onehot_puts_dv_on_the_selected_cell():
    case = B.with_int_values(G.onehot_case('oh', (1, 4, 3, 2, 3, 5)))
    g = B.grad_out_for(case, ints=True)
    r = B.grad_f64(case, g)
    tg = case['targets'][0]
    want = np.zeros((3, 30))
    for n, t in enumerate(tg):
        want[:, t] += g[0, :3].reshape(3, 15)[:, n]
    np.testing.assert_allclose(r['d_m_val'][0].reshape(3, 30), want, atol=1e-60)
    assert np.abs(r['d_m_key']).max() < 1e-60 and np.abs(r['d_q_key']).max() < 1e-60


def test_grad_f64_empty_query_rectangle_leaves_the_rank_one_term():
    h, w, T = 3, 5, 2
    mr = np.array([[(0, w - 1, 0, h - 1)] * T], np.int32)
    qr = np.array([(1, 0, 1, 0)], np.int32)
    case = _tiny(1, 4, 3, T, h, w, (mr, qr))
    g = B.grad_out_for(case)
    r = B.grad_f64(case, g)
    want = g[0, :3].reshape(3, 15).astype(np.float64).sum(axis=1) / 30
    np.testing.assert_allclose(r['d_m_val'][0].reshape(3, 30), np.repeat(want[:, None], 30, axis=1), rtol=1e-14)
    assert not r['d_m_key'].any() and not r['d_q_key'].any() and not r['d_q_val'].any()


def test_grad_f64_all_memory_masked_leaves_only_d_q_val():
    h, w, T = 3, 5, 2
    mr = np.array([[(1, 0, 1, 0)] * T], np.int32)
    qr = np.array([(0, w - 1, 0, h - 1)], np.int32)
    case = _tiny(1, 4, 3, T, h, w, (mr, qr))
    g = B.grad_out_for(case)
    r = B.grad_f64(case, g)
    assert not r['d_m_key'].any() and not r['d_m_val'].any() and not r['d_q_key'].any()
    assert np.array_equal(r['d_q_val'], g[:, 3:].astype(np.float64))


def _torch_restatement(torch, mk, mv, qk, qv, mm, qm, De):
    """models/rmnet.py:147-165 with the masks as explicit multiplications: mk [De, M], mv [Do, M], qk [De, N], qv [Do, N]."""
    km, vm, qq = mk * mm[None, :], mv * mm[None, :], qk * qm[None, :]
    p = torch.softmax(km.t() @ qq / De ** 0.5, dim=0)
    return torch.cat([vm @ p, qv * qm[None, :]], dim=0)


def test_grad_f64_equals_torch_autograd_and_the_restatement_passes_gradcheck():
    import torch
    no, De, Do, T, h, w = 1, 4, 3, 2, 2, 3
    for tag in (None, 1, 4, 7):
        rects = None if tag is None else G.rect_sets(no, T, h, w)[tag][1:3]
        case = _tiny(no, De, Do, T, h, w, rects, seed=3)
        g = B.grad_out_for(case)
        mm, qm = G.live_masks(case, 0)
        t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
        mk, mv = t64(case['m_key'][0].reshape(De, -1)), t64(case['m_val'][0].reshape(Do, -1))
        qk, qv = t64(case['q_key'][0].reshape(De, -1)), t64(case['q_val'][0].reshape(Do, -1))
        tm, tq = torch.tensor(mm.astype(np.float64)), torch.tensor(qm.astype(np.float64))
        out = _torch_restatement(torch, mk, mv, qk, qv, tm, tq, De)
        out.backward(torch.tensor(g[0].reshape(2 * Do, -1).astype(np.float64)))
        r = B.grad_f64(case, g)
        for name, leaf in (('d_m_key', mk), ('d_m_val', mv), ('d_q_key', qk), ('d_q_val', qv)):
            np.testing.assert_allclose(r[name][0].reshape(leaf.shape), leaf.grad.numpy(), rtol=1e-11, atol=1e-13, err_msg=name)
        assert torch.autograd.gradcheck(lambda a, b, c, d: _torch_restatement(torch, a, b, c, d, tm, tq, De), (mk, mv, qk, qv))


# ================================================================================================ CPU: the emulation, the bound, the mutants
def test_exact_families_have_integer_inputs_and_name_what_is_exact():
    n_exact = 0
    for key in KEYS:
        if key[2] not in EXACT_FAMILIES:
            continue
        case, g = get_case(*key), get_gout(*key)
        assert np.array_equal(case['m_val'], np.round(case['m_val'])) and np.array_equal(g, np.round(g)), key
        ex = get_exact(*key)
        n_exact += int(ex['d_m_val'][1].sum())
        assert ex['d_q_val'][1].all()
    assert n_exact > 10000


@pytest.mark.parametrize('key', KEYS, ids=key_id)
def test_the_fp32_emulation_is_inside_the_bound(key):
    """grad_f32 on every GPU case: inside the bound, and bit for bit where the exact families say so."""
    res = check_key(key, B.grad_f32(get_case(*key), get_gout(*key), get_mem_val(*key)))
    print(key_id(key), 'error / bound', res['ratio'], 'bit-exact elements', res['bits'])
    assert res['ok'], res['why']
    assert all(r <= 1.0 for r in res['ratio'].values())


def _logit_case(level, rects):
    """Every live logit = level: K = level sqrt(De) on channel 0, Q = 1 on channel 0."""
    case = G.equal_case('level%+d' % level, (1, 4, 3, 2, 3, 5), rects, None, 2, variant='zero')
    case['m_key'][:, 0] = np.float32(level * 2.0)
    case['q_key'][:] = 0
    case['q_key'][:, 0] = 1
    return case


def _mutant_cases():
    k = G.rect_kinds(3, 5)
    rect = lambda m, q: (np.array([[k[m]] * 2], np.int32), np.array([k[q]], np.int32))
    plain = ('s35', 'dense', 'random')
    return {'no_delta': get_case(*plain),
            'dk_no_scale': get_case(*plain),
            'no_rank1': G.random_case('rank1', (1, 4, 3, 2, 3, 5), rect('full', 'cell'), None, 1),
            'masked_not_in_denominator': G.random_case('denominator', (1, 4, 3, 2, 3, 5), rect('row', 'full'), None, 1),
            'max_live_only': _logit_case(-200, rect('row', 'full')),
            'dk_not_masked': G.random_case('dk-mask', (1, 4, 3, 2, 3, 5), rect('row', 'full'), None, 1),
            'dqv_not_masked': G.random_case('dqv-mask', (1, 4, 3, 2, 3, 5), rect('full', 'cell'), None, 1),
            'drop_last_query_tile': get_case('s513', 'dense', 'random'),
            'drop_last_cell': get_case(*plain),
            'tcap_for_t': get_case(*plain),
            'rect_exclusive': G.random_case('exclusive', (1, 4, 3, 2, 3, 5), rect('full', 'full'), None, 1)}


def test_every_planted_fault_is_rejected_by_its_case():
    cases = _mutant_cases()
    assert set(cases) == set(B.MUTANTS)
    survivors = []
    for mutant, case in cases.items():
        g = B.grad_out_for(case, seed=5)
        extreme = mutant == 'max_live_only'
        clean = B.check(case, g, B.grad_f32(case, g), extreme=extreme)
        assert clean['ok'], (mutant, clean['why'])
        if B.check(case, g, B.grad_f32(case, g, mutant=mutant), extreme=extreme)['ok']:
            survivors.append(mutant)
    assert not survivors, survivors


def test_large_positive_logits_do_not_overflow():
    """Logits near +150 with masked cells: exp(S) alone would overflow; exp(S - max) does not, and the masked cells' exp(-150) is 0."""
    k = G.rect_kinds(3, 5)
    case = _logit_case(150, (np.array([[k['row']] * 2], np.int32), np.array([k['full']], np.int32)))
    g = B.grad_out_for(case, seed=6)
    got = B.grad_f32(case, g)
    assert all(np.isfinite(v).all() for v in got.values())
    res = B.check(case, g, got, extreme=True)
    assert res['ok'], res['why']


# ================================================================================================ CPU: the C entry's argument rules
def _lib():
    from rmnet_amd import _lib
    return _lib.load()


def test_workspace_is_linear_in_T_and_smaller_than_the_affinity():
    lib = _lib()
    q = lib.rmnet_memory_read_backward_workspace_bytes
    for no, De, Do, h, w in ((3, 128, 512, 30, 54), (1, 20, 24, 3, 5), (12, 128, 512, 30, 30)):
        a, b, c = (q(no, De, Do, T, h, w) for T in (4, 8, 12))
        assert a > 0 and b - a == c - b == 4 * no * h * w * 4, (a, b, c)
    no, T, h, w = 3, 5, 30, 54
    assert q(no, 128, 512, T, h, w) < no * (T * h * w) * (h * w) * 4 // 10         # (far below the affinity: it is linear in M + N)
    for bad in ((0, 4, 4, 1, 2, 2), (1, 0, 4, 1, 2, 2), (1, 4, 0, 1, 2, 2), (1, 4, 4, 0, 2, 2), (1, 4, 4, 1, 0, 2), (1, 4, 4, 1, 2, 0)):
        assert q(*bad) == 0


def test_argument_rules_of_the_c_entry():
    """Every refusal comes before a launch, so it needs no GPU: the pointers below are never dereferenced."""
    lib = _lib()
    f = lib.rmnet_memory_read_backward_f32
    P = ctypes.c_void_p(4096)
    need = lib.rmnet_memory_read_backward_workspace_bytes(1, 4, 3, 2, 2, 3)

    def call(mk=P, mv=P, qk=P, qv=P, dims=(1, 4, 3, 2, 2, 3), strides=(0, 0, 0, 0), out=P, gout=P, mr=None, qr=None, grads=(P, P, P, P),
             ws=P, nbytes=need):
        return f(mk, mv, qk, qv, *dims, *strides, out, gout, mr, qr, *grads, ws, nbytes, None)

    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    for name in ('mk', 'mv', 'qk', 'qv', 'out', 'gout'):
        assert call(**{name: None}) == INVALID, name
    assert call(grads=(None, None, None, None)) == INVALID                      # nothing to compute
    for i in range(6):
        d = [1, 4, 3, 2, 2, 3]
        d[i] = 0
        assert call(dims=tuple(d)) == INVALID, i
    assert call(mr=P) == INVALID and call(qr=P) == INVALID                       # one rectangle array without the other
    assert call(strides=(11, 0, 0, 0)) == INVALID and call(strides=(0, 0, 11, 0)) == INVALID     # a channel stride below T h w = 12
    assert call(dims=(1, 225, 3, 2, 2, 3), nbytes=1 << 30) == UNSUPPORTED          # De > 224
    assert call(ws=None) == WORKSPACE and call(nbytes=need - 1) == WORKSPACE


# ================================================================================================ GPU
def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a):
    torch = _torch()
    return None if a is None else torch.from_numpy(np.array(a)).cuda()            # (a copy: the shared references are read-only)


FILL = np.float32(-77.5)


def run_c(case, gout, mem_val, need=(True, True, True, True), fill=FILL):
    """One call of the C entry on buffers pre-filled with ``fill``; returns {name: numpy array or None}."""
    torch = _torch()
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    no, De, Do, T, h, w = G.dims(case)
    tc = case['Tcap']
    t = {n: _dev(case[n]) for n in ('m_key', 'm_val', 'q_key', 'q_val', 'mem_rects', 'qry_rects')}
    mv_, go_ = _dev(mem_val), _dev(gout)
    shapes = dict(d_m_key=(no, De, tc, h, w), d_m_val=(no, Do, tc, h, w), d_q_key=(no, De, h, w), d_q_val=(no, Do, h, w))
    bufs = {n: (torch.full(shapes[n], float(fill), dtype=torch.float32, device='cuda') if need[i] else None) for i, n in enumerate(B.NAMES)}
    nb = lib.rmnet_memory_read_backward_workspace_bytes(no, De, Do, T, h, w)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    cs = tc * h * w
    p = ops._ptr
    rc = lib.rmnet_memory_read_backward_f32(p(t['m_key']), p(t['m_val']), p(t['q_key']), p(t['q_val']), no, De, Do, T, h, w, cs, cs * De, cs,
                                            cs * Do, p(mv_), p(go_), p(t['mem_rects']), p(t['qry_rects']), *[p(bufs[n]) for n in B.NAMES],
                                            p(ws), nb, ops._stream(torch.device('cuda', 0)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {n: (None if b is None else b.cpu().numpy()) for n, b in bufs.items()}


def _split_tail(case, got):
    """(the gradients with frames >= T set to 0, True when those frames still hold the fill)."""
    T = case['T']
    kept, out = True, {}
    for n, a in got.items():
        if a is not None and n in ('d_m_key', 'd_m_val') and case['Tcap'] > T:
            kept &= bool((a[:, :, T:] == FILL).all())
            a = a.copy()
            a[:, :, T:] = 0
        out[n] = a
    return out, kept


@pytest.mark.gpu
@pytest.mark.parametrize('key', KEYS, ids=key_id)
def test_every_element_of_the_four_gradients(key):
    case = get_case(*key)
    got, kept = _split_tail(case, run_c(case, get_gout(*key), get_mem_val(*key)))
    assert kept, 'frames >= T were written'
    res = check_key(key, got)
    print(key_id(key), 'error / bound', res['ratio'], 'bit-exact elements', res['bits'])
    assert res['ok'], res['why']


@pytest.mark.gpu
def test_partial_requests_give_the_same_bits():
    key = ('s513', 'r4', 'random')
    case, g, mv = get_case(*key), get_gout(*key), get_mem_val(*key)
    full = run_c(case, g, mv)
    for bits in range(1, 15):
        need = tuple(bool(bits >> i & 1) for i in range(4))
        got = run_c(case, g, mv, need)
        for i, n in enumerate(B.NAMES):
            if need[i]:
                assert B.same_bits(got[n], full[n]).all(), (need, n)
            else:
                assert got[n] is None


@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_give_the_same_bits():
    torch = _torch()
    from rmnet_amd import ops
    key = ('fast', 'r4', 'random')
    case = get_case(*key)
    T = case['T']
    args = [_dev(case[n]) for n in ('m_key', 'm_val', 'q_key', 'q_val')] + [_dev(get_mem_val(*key)), _dev(get_gout(*key))]
    rects = (_dev(case['mem_rects']), _dev(case['qry_rects']))
    first = ops.memory_read_backward(*args, *rects, T=T)
    second = ops.memory_read_backward(*args, *rects, T=T)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert all(not a[:, :, T:].any() for a in first[:2])                         # frames >= T: zero-filled by the wrapper
    # capture once on stand-in inputs, replay on the real ones
    static = [torch.zeros_like(a) for a in args]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.memory_read_backward(*static, *rects, T=T)                           # (warm-up on the side stream)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.memory_read_backward(*static, *rects, T=T)
    for s, a in zip(static, args):
        s.copy_(a)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def _leaves(case):
    torch = _torch()
    return [_dev(case[n]).requires_grad_(True) for n in ('m_key', 'm_val', 'q_key', 'q_val')]


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['split', 'exact'])
def test_autograd_through_memory_reader(precision):
    """The output has a grad_fn and backward() fills .grad (fails without the feature); .grad equals ops.memory_read_backward bit for
    bit and is inside the bound of grad_f64; a second backward accumulates."""
    torch = _torch()
    from rmnet_amd import ops
    from rmnet_amd.rmnet import MemoryReader
    key = ('fast', 'r7', 'random')
    case, g = get_case(*key), get_gout(*key)
    T = case['T']
    rects = (_dev(case['mem_rects']), _dev(case['qry_rects']))
    leaves = _leaves(case)
    if precision == 'exact':
        fwd = lambda *a: ops.memory_read(*a, *rects, T=T, flags=ops.MR_EXACT_FP32)
    else:
        reader = MemoryReader(precision=precision).train()
        fwd = lambda *a: reader(*a, *rects, T=T)
    mem_val, p = fwd(*leaves)
    assert p is None and mem_val.grad_fn is not None and mem_val.requires_grad
    weight = _dev(g)
    (mem_val * weight).sum().backward()
    assert all(l.grad is not None for l in leaves)
    want = ops.memory_read_backward(*[l.detach() for l in leaves], mem_val.detach(), weight, *rects, T=T)
    for l, wnt in zip(leaves, want):
        assert torch.equal(l.grad, wnt)
    got = {n: l.grad.cpu().numpy() for n, l in zip(B.NAMES, leaves)}
    res = check_key(key, got, mem_val=mem_val.detach().cpu().numpy())
    print(precision, 'error / bound', res['ratio'])
    assert res['ok'], res['why']
    # .sum(): a gradient of ones; the second backward accumulates
    once = [l.grad.clone() for l in leaves]
    fwd(*leaves)[0].sum().backward()
    ones = ops.memory_read_backward(*[l.detach() for l in leaves], mem_val.detach(), torch.ones_like(mem_val), *rects, T=T)
    for l, a, b in zip(leaves, once, ones):
        assert torch.equal(l.grad, a + b)


@pytest.mark.gpu
def test_autograd_rules():
    torch = _torch()
    from rmnet_amd import ops
    from rmnet_amd.rmnet import MemoryReader
    key = ('s513', 'dense', 'random')
    case = get_case(*key)
    base = [_dev(case[n]) for n in ('m_key', 'm_val', 'q_key', 'q_val')]
    # inputs that are outputs of torch ops receive gradients
    leaves = [b.clone().requires_grad_(True) for b in base]
    out, _ = MemoryReader()(*[l * 1.0 for l in leaves])
    out.sum().backward()
    want = ops.memory_read_backward(*base, out.detach(), torch.ones_like(out))
    for l, wnt in zip(leaves, want):
        assert torch.equal(l.grad, wnt)
    # only the inputs that need one get a gradient
    qk = base[2].clone().requires_grad_(True)
    MemoryReader()(base[0], base[1], qk, base[3])[0].sum().backward()
    assert torch.equal(qk.grad, want[2])
    # p is returned, and is not differentiable
    out, p = MemoryReader(return_affinity=True)(*leaves)
    assert out.requires_grad and p is not None and not p.requires_grad
    # out= cannot be combined with a gradient
    with pytest.raises(RuntimeError):
        ops.memory_read(*leaves, out=torch.empty_like(out))
    # without grad mode: no grad_fn, and the bits of the plain call
    plain, _ = ops.memory_read(*base)
    with torch.no_grad():
        quiet, _ = MemoryReader()(*leaves)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)
    assert torch.equal(MemoryReader()(*leaves)[0].detach(), plain)
