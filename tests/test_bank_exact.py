# -*- coding: utf-8 -*-
"""Bit-exact integer-logit tests of the memory-bank read in every arithmetic (tests/bank_ref.py has the construction, the
exactness budget and the count of roundings), a derived per-element bound for the fp16-operand modes on random inputs, and CPU
tests that plant faults in a numpy restatement of the tile loop and require the same comparisons to fail.
Figures of the first MI355X run: profiles/r11_a_bank_exact_tests.md."""

import functools

import numpy as np
import pytest

import bank_ref as br

MR_ATOL, MR_RTOL = 3e-5, 2e-5           # tests/test_gpu_parity.py: the fp32-class bar of the natural-base kernels
E = (1, 0, 1, 0)                        # an empty box


def _box(n, wmax, x0=0, y0=0):
    """(x0, x1, y0, y1) of exactly n cells, at most wmax wide."""
    for rows in range(1, 65):
        if n % rows == 0 and n // rows <= wmax:
            return (x0, x0 + n // rows - 1, y0, y0 + rows - 1)
    raise AssertionError(n)


def _rand_rects(rng, no, T, h, w, p_empty=0.2):
    def rect():
        if rng.rand() < p_empty:
            return E
        x0, y0 = rng.randint(0, w), rng.randint(0, h)
        return (x0, rng.randint(x0, w), y0, rng.randint(y0, h))
    return [[rect() for _ in range(T)] for _ in range(no)], [rect() if o else (0, w - 1, 0, h - 1) for o in range(no)]


def _specs():
    s = {}

    def add(name, family, *a, **k):
        s[name] = (a, dict(k, family=family))
    # 1. all logits equal, dense, T h w a power of two: the mean of integers
    add('eq_1x4x8x8', 'equal', 1, 4, 8, 8, logits='equal', junk=True)
    add('eq_2x2x4x16', 'equal', 2, 2, 4, 16, logits='equal', vals='quarter')
    add('eq_1x1x4x8', 'equal', 1, 1, 4, 8, logits='equal', junk=True, vals='quarter')
    # 2. general integer logits, R <= 4; l forced to a power of two in the dense 'pow2' cases
    add('pow2_1x2x8x16', 'general', 1, 2, 8, 16, logits='pow2', junk=True)
    add('pow2_2x1x8x8', 'general', 2, 1, 8, 8, logits='pow2', vals='quarter')
    add('pow2_1x4x16x16', 'general', 1, 4, 16, 16, logits='pow2')
    rng = np.random.RandomState(11)
    mr, qr = _rand_rects(rng, 2, 3, 9, 13)
    add('gen_2x3x9x13', 'general', 2, 3, 9, 13, mr, qr, logits='general', vals='quarter', junk=True)
    mr, qr = _rand_rects(rng, 3, 2, 12, 20)
    add('gen_3x2x12x20', 'general', 3, 2, 12, 20, mr, qr, logits='general')
    # 3. box areas around the 32-cell tile and the 64-cell step, T = 1, 2, 3, mixed with empty boxes (grid 4 x 128 = 512 cells)
    areas = (1, 31, 32, 33, 63, 64, 65, 96, 97)
    full = (0, 127, 0, 3)
    add('area_T1', 'areas', 9, 1, 4, 128, [[_box(a, 128, x0=a % 7)] for a in areas],
        [full, (3, 90, 1, 2), full, (0, 62, 0, 0), full, (5, 127, 0, 3), full, (0, 63, 1, 1), full], logits='equal', junk=True)
    pairs = ((31, 33), (1, 97), (63, 0), (0, 65), (96, 64))
    add('area_T2', 'areas', 5, 2, 4, 128, [[_box(a, 128) if a else E for a in p] for p in pairs],
        [full, (2, 66, 0, 3), full, (0, 127, 2, 3), (64, 127, 0, 0)], logits='equal', vals='quarter')
    trip = ((33, 31, 65), (1, 0, 97), (32, 63, 0), (97, 96, 1))
    add('area_T3_general', 'areas', 4, 3, 4, 128, [[_box(a, 128, y0=0) if a else E for a in p] for p in trip],
        [full, (1, 99, 0, 3), full, (0, 64, 1, 1)], logits='general', junk=True)
    add('area_T3_equal', 'areas', 4, 3, 4, 128, [[_box(a, 128) if a else E for a in p] for p in trip],
        [full, full, (0, 30, 0, 0), full], logits='equal')
    # 4. query boxes of 1, 63, 64 and 65 cells, empty, full, sticking out of the grid (8 x 16, T = 2: 256 cells)
    qb = [(5, 5, 3, 3), _box(63, 16, 2, 0), _box(64, 16), (1, 13, 2, 6), E, (0, 15, 0, 7), (-3, 20, -2, 5)]
    mb = [[(0, 15, 0, 7), (2, 12, 1, 6)], [(0, 15, 0, 7), E], [(1, 9, 0, 7), (0, 15, 2, 3)], [(0, 15, 0, 7), (0, 15, 0, 7)],
          [(0, 15, 0, 7), (3, 8, 3, 4)], [E, (4, 11, 2, 5)], [(-2, 18, 5, 9), (0, 0, 0, 0)]]
    add('qbox_equal', 'query boxes', 7, 2, 8, 16, mb, qb, logits='equal', junk=True)
    add('qbox_general', 'query boxes', 7, 2, 8, 16, mb, qb, logits='general', vals='quarter')
    # 5. launch plans
    for no in (1, 5, 14, 70):
        mr, qr = _rand_rects(np.random.RandomState(no), no, 2, 4, 5)
        add('plan_no%d' % no, 'plans', no, 2, 4, 5, mr, qr, logits='general', vals='quarter')
    rs = np.random.RandomState(60)
    add('plan_rounds_60', 'plans', 60, 1, 16, 24,
        [[(int(x), int(x) + int(rs.randint(2, 9)), int(y), int(y) + int(rs.randint(2, 6)))] for x, y in
         zip(rs.randint(0, 14, 60), rs.randint(0, 10, 60))], [(0, 23, 0, 15)] * 60, logits='general')
    mr, qr = _rand_rects(np.random.RandomState(70), 1, 70, 5, 6)
    add('plan_T70', 'plans', 1, 70, 5, 6, mr, qr, logits='general', junk=True)
    # 6. late spike (logit 12 among zeros): in the first / second tile of an fp16 step, and in a later split
    add('spike_tile2', 'spike', 1, 4, 8, 16, logits='spike', vals='sign', spike=(0, 4, 0))
    add('spike_tile3', 'spike', 1, 4, 8, 16, logits='spike', vals='sign', spike=(0, 6, 5), junk=True)
    add('spike_late_split', 'spike', 1, 8, 16, 24, logits='spike', vals='sign', spike=(6, 9, 7))
    # 7. more frames than one launch takes: bk_chain, bk_ml_fill; in the 4100 case the third chunk has only empty boxes
    for T in (2049, 4100):
        rs = np.random.RandomState(T)
        mr = [[E if (t >= 4096 or rs.rand() < 0.3) else (int(rs.randint(0, 2)), int(rs.randint(2, 4)), int(rs.randint(0, 2)), 2)
               for t in range(T)]]
        add('chain_T%d' % T, 'chain', 1, T, 3, 4, mr, [(0, 3, 0, 2)], logits='general')
    return s


SPECS = _specs()
NAMES = list(SPECS)
FIRST_FIVE = [n for n in NAMES if SPECS[n][1]['family'] in ('equal', 'general', 'areas', 'query boxes', 'plans')]
SINGLE_LAUNCH = [n for n in NAMES if SPECS[n][1]['family'] != 'chain']
MODES = ('split', 'f16', 'qx')


@functools.lru_cache(maxsize=None)
def case_of(name):
    a, k = SPECS[name]
    return br.make_case(name, *a, **k)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return br.exact_read(case_of(name))


# ====================================================================================================== CPU tests
def test_scaled_queries_are_exact_for_every_allowed_a():
    for a in br.ALLOWED_A:
        for s in (1.0, -1.0):
            q = br.query_for(s * a)
            assert q.dtype == np.float32 and np.float32(q * br.QSCALE) == np.float32(64.0 * s * a)
            h = np.float16(np.float32(q * br.QSCALE))
            assert float(h) == 64.0 * s * a                       # the fp16 hi plane holds it: the lo plane is exactly zero
    assert float(br.query_for(1.0)) == 7.84206485748291 and float(br.query_for(3.0)) == 23.526195526123047


@pytest.mark.parametrize('name', NAMES)
def test_budget_holds_for_every_gpu_case(name):
    ref = ref_of(name)
    assert br.budget_ok(ref), (ref['budget'], ref['R'])
    fam = SPECS[name][1]['family']
    assert ref['R'] <= (12 if fam == 'spike' else 4)
    if fam == 'equal' or name.startswith('pow2') or name in ('area_T1', 'area_T2', 'qbox_equal'):
        assert ref['exact'].all(), name                           # compared bit for bit in full
    if fam == 'chain':
        assert ref['nchunk'] == (2 if case_of(name)['T'] == 2049 else 3) and not ref['exact'][:, :512].any()


def test_the_cases_land_on_the_plans_the_table_names():
    plan = {n: br.plan_of(case_of(n)) for n in NAMES if SPECS[n][1]['family'] == 'plans'}
    assert [g['plan'] for g in plan['plan_no1']] == ['fast'] and [g['plan'] for g in plan['plan_no5']] == ['fast']
    assert [g['plan'] for g in plan['plan_no14']] == ['lds']                       # more than 12 objects: LDS atomics
    assert [g['nobj'] for g in plan['plan_no70']] == [64, 6]                       # two launch groups
    assert [g['rounds'] for g in plan['plan_rounds_60']] == [True] and plan['plan_rounds_60'][0]['pairs'] == 360
    assert [g['plan'] for g in plan['plan_T70']] == ['lds']                        # more than 64 frames
    case = case_of('area_T3_general')                                               # an fp16 step whose tiles belong to two frames
    assert br.mutant_touches(case, 'skip_second_tile', 'f16')


def test_the_spikes_sit_where_the_table_names():
    """Tiles count from 0; an fp16 step is tiles (2 s, 2 s + 1).  'spike_tile2' has its spike in the first tile of the second
    step, 'spike_tile3' in the second tile of that step.  'spike_late_split' has it in tile 78 of 96, while the device's search for
    the chunk length starts at an even cut of 4 tiles (plan_of): the spike is in a later chunk than the first for every chunk length
    up to 78, nearly twenty times the even cut.  That the device stays below that is its own rule (the smallest candidate from the
    even cut upwards whose chunks fit the workgroups), which plan_of does not restate."""
    assert br.spike_tile(case_of('spike_tile2')) == (2, 16) and br.spike_tile(case_of('spike_tile3')) == (3, 16)
    late = case_of('spike_late_split')
    assert br.spike_tile(late) == (78, 96)
    (g,) = br.plan_of(late)
    assert g['plan'] == 'fast' and g['pairs'] == 6 and g['even_cut'] == 4 and 78 >= 16 * g['even_cut']
    for name in ('spike_tile2', 'spike_tile3', 'spike_late_split'):
        case, ref = case_of(name), ref_of(name)
        assert ref['R'] == 12 and ref['nmax'] == 12                                  # one cell at 12 among zeros
        sees = case['a'][0, br.CH_U] == 4.0
        assert sees.any() and not sees.all()
        if name != 'spike_late_split':                                               # (there T h w = 3072 is no power of two)
            assert ref['exact'][0, 0][~sees].all()                                   # queries that do not see it: bit for bit


def test_reference_agrees_with_fractions():
    for name in ('gen_2x3x9x13', 'qbox_general', 'area_T2'):
        case, ref = case_of(name), ref_of(name)
        rng = np.random.RandomState(3)
        for _ in range(12):
            o, d = rng.randint(case['no']), rng.randint(1024)
            y, x = rng.randint(case['h']), rng.randint(case['w'])
            fr = br.exact_read_fraction(case, o, d, y, x)
            assert abs(float(fr) - ref['out'][o, d, y, x]) <= 2.0 ** -52 * abs(float(fr)), (name, o, d, y, x)
            if ref['exact'][o, d, y, x]:
                assert fr == fr.__class__(float(np.float32(ref['out'][o, d, y, x]))), (name, o, d, y, x)


@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_reference(name):
    """The numpy tile loop returns the rational reference: bit for bit where l is a power of two (check_read asserts that), within
    the counted roundings elsewhere -- in all three arithmetics and for several cuts of the tile list into segments."""
    case, ref = case_of(name), ref_of(name)
    for mode, ct in (('split', None), ('f16', None), ('qx', 4), ('split', 3), ('f16', 2)):
        if case['T'] > br.MAX_T and ct == 3:
            continue
        br.check_read(br.tile_loop_read(case, mode, chunk_tiles=ct), ref, '%s %s %s' % (name, mode, ct))


@pytest.mark.parametrize('mutant', br.MUTANTS)
def test_a_planted_fault_fails_every_case_it_touches(mutant):
    """Each mutant of the restatement must fail the part-2 comparison on every case whose rows it touches (and, to keep the
    'touches' predicate honest, it must touch at least one case), in every arithmetic."""
    touched = 0
    for name in NAMES:
        case, ref = case_of(name), ref_of(name)
        for mode in MODES:
            if not br.mutant_touches(case, mutant, mode):
                continue
            touched += 1
            got = br.tile_loop_read(case, mode, mutant=mutant)
            with pytest.raises(AssertionError):
                br.check_read(got, ref, name)
    assert touched > 0, mutant


RANDOM_SHAPES = [(2, 3, 9, 13, True), (1, 5, 30, 54, True), (1, 7, 16, 24, False), (14, 2, 6, 9, True)]


def _random_case(no, T, h, w, regional, kscale, vscale):
    rng = np.random.RandomState(no * 1000 + T * 100 + h + int(kscale * 10))
    mk = (rng.randn(no, 128, T, h, w) * kscale).astype(np.float32)
    mv = (rng.randn(no, 512, T, h, w) * vscale).astype(np.float32)
    qk = (rng.randn(no, 128, h, w) * kscale).astype(np.float32)
    qv = rng.randn(no, 512, h, w).astype(np.float32)
    if regional:
        mr, qr = _rand_rects(rng, no, T, h, w, 0.15)
        qr[0] = _rand_rects(rng, 1, 1, h, w, 0.0)[0][0][0]
    else:
        mr, qr = [[(0, w - 1, 0, h - 1)] * T] * no, [(0, w - 1, 0, h - 1)] * no
    return mk, mv, qk, qv, np.asarray(mr, np.int32).reshape(no, T, 4), np.asarray(qr, np.int32).reshape(no, 4)


@pytest.mark.parametrize('no,T,h,w,regional', RANDOM_SHAPES)
def test_truncated_value_plane_leaves_the_part3_bound(no, T, h, w, regional):
    """V's hi plane truncated instead of rounded to nearest: the read-out evaluated on those operands leaves the per-element bound
    of the true operands on every shape, at the peaked key scale 3.0 (where a read-out follows single cells and the bound is the
    tightest).

    KNOWN BLIND SPOT, not a passing condition: at key scale 0.6 the bound does not see this fault (the fraction of elements that
    leave it is printed: 0 % on three shapes, 0.8 % on (14, 2, 6, 9)).  No tighter evaluation of the same bound would: a
    truncation moves each value by at most 2^-11 |v|, 2^-12 |v| on average and toward zero, so over the N cells a read-out
    averages the shifts of positive and negative values cancel to about 2^-12 |v| / sqrt(N), while the weight rounding the mode is
    entitled to is 2^-11 sum w_i |v~_i - o| / L, about 2^-11 |v| whatever N.  Flat soft-maxes need the integer cases of part 2, where
    any wrong value bit fails; they cannot plant a truncation (their values are exact in fp16)."""
    for kscale in (3.0, 0.6):
        mk, mv, qk, qv, mr, qr = _random_case(no, T, h, w, regional, kscale, 1.0)
        want, bound = br.f16_operand_read(mk, mv, qk, qv, mr, qr)
        bad, _ = br.f16_operand_read(mk, mv, qk, qv, mr, qr, trunc_v=True)
        over = np.abs(bad[:, :512] - want[:, :512]) > bound
        print('truncated V, %s key scale %.1f: %.2f %% of the elements leave the bound' % ((no, T, h, w), kscale, 100.0 * over.mean()))
        if kscale == 3.0:
            assert over.any()


F16_ATOL_REL = 2.0 ** -10               # tests/test_gpu_parity.py: _f16_bars


def _old_bars_accept(got, want, vmax, mode):
    """The whole-tensor bars of tests/test_gpu_parity.py: _f16_bars for the fp16 modes, MR_ATOL / MR_RTOL for 'split'."""
    if mode == 'split':
        return bool(np.allclose(got, want, atol=MR_ATOL, rtol=MR_RTOL))
    err = np.abs(got[:, :512] - want[:, :512])
    return bool(not np.isnan(got).any() and err.max() <= F16_ATOL_REL * vmax and err.mean() < 1e-4
                and np.array_equal(got[:, 512:], want[:, 512:]))


@pytest.mark.parametrize('no,T,h,w,seed', [(1, 5, 30, 54, 0), (1, 5, 30, 54, 1), (5, 5, 30, 54, 1)])
def test_what_the_whole_tensor_bars_accept_of_the_planted_faults(no, T, h, w, seed):
    """The record behind this file (table in profiles/r11_a_bank_exact_tests.md): the eight planted faults on the inputs of the
    existing tests at (1, 5, 30, 54) and (5, 5, 30, 54) (tests/test_gpu_parity.py's generator; seed + 1 is what the bank tests use,
    seed + 0 what test_memory_read_random_vs_oracle uses -- with + 1 the one object of (1, 5, 30, 54) draws an EMPTY query box, so
    those tests run no soft-max at that shape and no fault can show), through the numpy tile loop, against the bars those tests
    apply -- _f16_bars in 'f16', MR_ATOL / MR_RTOL in 'split' -- and, for 'f16', against the per-element bound of part 3.
    Printed, not fixed in advance; asserted is only that the bars and the bound accept the loop without a fault (else the table
    would say nothing)."""
    rng = np.random.RandomState(no * 1000 + T * 100 + h + seed)
    mk = (rng.randn(no, 128, T, h, w) * 0.6).astype(np.float32)
    mv = rng.randn(no, 512, T, h, w).astype(np.float32)
    qk = (rng.randn(no, 128, h, w) * 0.6).astype(np.float32)
    qv = rng.randn(no, 512, h, w).astype(np.float32)

    def rect():
        if rng.rand() < 0.15:
            return E
        x0, y0 = rng.randint(0, w), rng.randint(0, h)
        return (x0, rng.randint(x0, w), y0, rng.randint(y0, h))
    mr = np.array([[rect() for _ in range(T)] for _ in range(no)], np.int32)
    qr = np.array([rect() for _ in range(no)], np.int32)
    case = dict(no=no, T=T, h=h, w=w, m_key=mk, m_val=mv, q_key=qk, q_val=qv, mem_rects=mr, qry_rects=qr, random=True)
    want = br.float64_read(case)
    want16, bound = br.f16_operand_read(mk, mv, qk, qv, mr, qr)
    vmax = float(np.abs(mv).max())
    rows = {}
    for mutant in (None,) + br.ALL_MUTANTS:
        got16, got32 = br.tile_loop_read(case, 'f16', mutant=mutant), br.tile_loop_read(case, 'split', mutant=mutant)
        e16 = np.abs(got16[:, :512] - want[:, :512])
        inside = (np.abs(got16[:, :512].astype(np.float64) - want16[:, :512]) <= bound).all() and np.array_equal(got16[:, 512:], want16[:, 512:].astype(np.float32))
        changed = not np.array_equal(got16, rows[None][4]) if mutant else False
        rows[mutant] = (_old_bars_accept(got16, want, vmax, 'f16'), _old_bars_accept(got32, want, vmax, 'split'), bool(inside),
                        (float(e16.max()), float(e16.mean()), float(np.abs(got32 - want).max())), got16, changed)
    for mutant, (a16, a32, ins, (emax, emean, e32), _, changed) in rows.items():
        print('%s seed + %d %-16s changes the read-out: %-5s | f16 max err %.2e mean %.2e: _f16_bars %s, part-3 bound %s | split max err %.2e: MR_ATOL %s' % (
            (no, T, h, w), seed, mutant or 'no fault', changed, emax, emean, 'accepts' if a16 else 'REJECTS', 'accepts' if ins else 'REJECTS',
            e32, 'accepts' if a32 else 'REJECTS'))
    live = [m for m in br.ALL_MUTANTS if rows[m][5]]
    print('%s seed + %d: of %d faults that change the read-out, _f16_bars accepts %d, MR_ATOL accepts %d, the part-3 bound accepts %d' % (
        (no, T, h, w), seed, len(live), sum(rows[m][0] for m in live), sum(rows[m][1] for m in live), sum(rows[m][2] for m in live)))
    assert rows[None][0] and rows[None][1] and rows[None][2]


# ====================================================================================================== GPU tests
def dev():
    import torch
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    return torch.device('cuda', 0)


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


_BANKS = {}


def _bank_of(name, case=None, key=None):
    """The case's frames in a MemoryBank (built once per case; the bank is the same for every arithmetic)."""
    from rmnet_amd import ops
    key = key or name
    if key not in _BANKS:
        case = case or case_of(name)
        no, T, h, w = case['no'], case['T'], case['h'], case['w']
        bank = ops.MemoryBank(no, T, h, w, dev())
        mk, mv = cu(case['m_key']), cu(case['m_val'])
        mr = None if case['mem_rects'] is None else cu(case['mem_rects'])
        for t in range(T):
            bank.append(t, mk[:, :, t].contiguous(), mv[:, :, t].contiguous(), None if mr is None else mr[:, t].contiguous())
        _BANKS.clear()                                             # one bank alive at a time (the chained ones are 330 MB)
        _BANKS[key] = (bank, cu(case['q_key']), cu(case['q_val']), None if case['qry_rects'] is None else cu(case['qry_rects']))
    return _BANKS[key]


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_bank_read_returns_the_rational_reference(name):
    """MemoryBank.read in 'split', 'f16' and 'qx' on the same bank: np.float32 of the exact rational bit for bit wherever l (or
    T h w outside the query box) is a power of two, at most the counted roundings elsewhere (bank_ref: two per launch, the chain's
    on top), channels 512.. exact always; overflow and time-out words 0; the logit word equal to its prediction where it is
    determined, else within the documented 8 below the true maximum and never above it.


    This needs the kernels to split the ROUNDED product fl32(q * qscale) (bank.hip: mul_rounded); a product contracted into the
    lo plane's subtraction leaves a non-zero lo plane and fails most cases in 'split' and 'qx'."""
    case, ref = case_of(name), ref_of(name)
    bank, qk, qv, qr = _bank_of(name)
    for mode in MODES:
        bank.precision = mode
        got = bank.read(case['T'], qk, qv, qr).cpu().numpy()
        err = np.abs(got.astype(np.float64) - ref['out'])
        tol = br.tolerance(ref)
        print('%s %s: %d of %d elements required bit-exact; largest error / counted bound %.3f' % (
            name, mode, int(ref['exact'].sum()), ref['exact'].size, float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0))
        br.check_read(got, ref, '%s %s' % (name, mode))
    assert bank.overflow_count() == 0 and bank.timeout_count() == 0
    word, want, top = bank.logit_max(), br.expected_logit_word(case), br.true_logit_max(case)
    print('%s: logit word %.6f, predicted %s, true maximum %.6f' % (name, word, want, top))
    if want is not None:
        assert word == want
    assert top - 8.0 - 1e-6 <= word <= top + 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('name', FIRST_FIVE)
def test_dropin_memory_read_returns_the_rational_reference(name):
    """ops.memory_read with flags 0, MR_F16 and MR_QX (staging + read in one call), the same comparison."""
    from rmnet_amd import ops
    case, ref = case_of(name), ref_of(name)
    args = [cu(case[k]) for k in ('m_key', 'm_val', 'q_key', 'q_val')]
    rects = [] if case['mem_rects'] is None else [cu(case['mem_rects']), cu(case['qry_rects'])]
    for flags in (0, ops.MR_F16, ops.MR_QX):
        got, _ = ops.memory_read(*args, *rects, flags=flags)
        br.check_read(got.cpu().numpy(), ref, '%s flags %d' % (name, flags))


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in FIRST_FIVE if SPECS[n][0][1] <= 3])
def test_staged_read_returns_the_rational_reference(name):
    """MemoryBank.stage / commit for all frames but the last, which is staged only: read_staged (frame count from the device)."""
    from rmnet_amd import ops
    case, ref = case_of(name), ref_of(name)
    no, T, h, w = case['no'], case['T'], case['h'], case['w']
    for mode in MODES:
        bank = ops.MemoryBank(no, T, h, w, dev(), precision=mode)
        for t in range(T):
            bank.stage(cu(case['m_key'][:, :, t]), cu(case['m_val'][:, :, t]), None if case['mem_rects'] is None else cu(case['mem_rects'][:, t]))
            if t < T - 1:
                bank.commit()
        got = bank.read_staged(cu(case['q_key']), cu(case['q_val']), None if case['qry_rects'] is None else cu(case['qry_rects']))
        br.check_read(got.cpu().numpy(), ref, '%s staged %s' % (name, mode))
        assert bank.overflow_count() == 0 and bank.timeout_count() == 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', SINGLE_LAUNCH)
def test_natural_base_kernels_meet_the_same_answer(name):
    """The exact-fp32 kernel (MR_EXACT_FP32) and TensorBank work in natural-base arithmetic: nothing is exact there, they meet the
    rational reference at the fp32-class bar.  Three independent implementations, one exact answer."""
    from rmnet_amd import ops
    case, ref = case_of(name), ref_of(name)
    mr, qr = br.full_rects(case)
    got, _ = ops.memory_read(cu(case['m_key']), cu(case['m_val']), cu(case['q_key']), cu(case['q_val']), cu(mr), cu(qr), flags=ops.MR_EXACT_FP32)
    np.testing.assert_allclose(got.cpu().numpy(), ref['out'], atol=MR_ATOL, rtol=MR_RTOL)
    tb = ops.TensorBank(case['no'], case['T'], case['h'], case['w'], dev())
    for t in range(case['T']):
        tb.append(t, cu(case['m_key'][:, :, t]), cu(case['m_val'][:, :, t]), cu(mr[:, t]))
    np.testing.assert_allclose(tb.read(case['T'], cu(case['q_key']), cu(case['q_val']), cu(qr)).cpu().numpy(), ref['out'], atol=MR_ATOL, rtol=MR_RTOL)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['gen_2x3x9x13', 'area_T3_general', 'qbox_general', 'qbox_equal', 'plan_no14', 'plan_T70'])
def test_garbage_outside_the_boxes_changes_no_bit(name):
    """Non-integers in every masked key / value cell and in the keys of the query cells outside the box: the same bits as the clean
    run, in every arithmetic, through the bank and through the drop-in entry."""
    from rmnet_amd import ops
    clean, ref = case_of(name), ref_of(name)
    dirty = br.with_garbage(clean)
    assert not np.array_equal(dirty['m_val'], clean['m_val']) and not np.array_equal(dirty['m_key'], clean['m_key'])
    outs = []
    for case, key in ((clean, name), (dirty, name + '+garbage')):
        bank, qk, qv, qr = _bank_of(name, case, key)
        for mode in MODES:
            bank.precision = mode
            outs.append(bank.read(case['T'], qk, qv, qr).cpu().numpy())
        got, _ = ops.memory_read(cu(case['m_key']), cu(case['m_val']), cu(case['q_key']), cu(case['q_val']), cu(case['mem_rects']),
                                 cu(case['qry_rects']), flags=ops.MR_F16)
        outs.append(got.cpu().numpy())
        assert bank.overflow_count() == 0
    for a, b in zip(outs[:4], outs[4:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        br.check_read(b, ref, name + ' with garbage')


@pytest.mark.gpu
@pytest.mark.parametrize('kscale,vscale', [(k, v) for k in (0.6, 3.0) for v in (1.0, 1e-2, 1e2)])
@pytest.mark.parametrize('no,T,h,w,regional', RANDOM_SHAPES)
def test_f16_modes_stay_inside_the_derived_bound_on_every_element(no, T, h, w, regional, kscale, vscale):
    """Random inputs, 'f16' and 'qx': every read-out element within bank_ref.f16_operand_read's bound of the float64 read on the
    operands the mode multiplies (K, V and q rounded as the kernels round them).  Separates operand faults from the weight rounding
    the mode is entitled to.  Largest error / bound of the first run: profiles/r11_a_bank_exact_tests.md."""
    from rmnet_amd import ops
    mk, mv, qk, qv, mr, qr = _random_case(no, T, h, w, regional, kscale, vscale)
    bank = ops.MemoryBank(no, T, h, w, dev())
    for t in range(T):
        bank.append(t, cu(mk[:, :, t]), cu(mv[:, :, t]), cu(mr[:, t]))
    for mode in ('f16', 'qx'):
        want, bound = br.f16_operand_read(mk, mv, qk, qv, mr, qr, qx=mode == 'qx')
        bank.precision = mode
        got = bank.read(T, cu(qk), cu(qv), cu(qr)).cpu().numpy()
        err = np.abs(got[:, :512].astype(np.float64) - want[:, :512])
        nz = bound > 0
        print('%s k %.1f v %g %s: largest error / bound %.3f' % ((no, T, h, w), kscale, vscale, mode, float((err[nz] / bound[nz]).max())))
        assert np.array_equal(got[:, 512:], want[:, 512:].astype(np.float32))
        assert (err <= bound).all(), int((err > bound).sum())
    assert bank.overflow_count() == 0 and bank.timeout_count() == 0
