# -*- coding: utf-8 -*-
"""Integer-logit cases for the memory-bank read (rmnet_amd/csrc/bank.hip) and their exact reference.

The construction.  bk_main's soft-max is exp2(S_raw * 2^-12 - m): keys and values are stored times 2^6, the query is
multiplied ONCE in fp32 by qscale = log2(e) / sqrt(128) * 2^6, merges rescale by exp2(m_s - m_tot) and the masked memory cells
enter as n_out * exp2(-m_tot).  So with
  * keys that are small integers k in a few of the 128 channels,
  * queries q (float32) whose scaled image fl32(q * qscale) is EXACTLY 64 a  (``query_for``; asserted in float32),
  * values that are small integers, halves or quarters,
the log2 logit of (query, cell) is the integer n = sum_c k_c a_c, every weight is an exact power of two in all three arithmetics
(the lo planes of q and P are zero, an fp16 hi plane holds a power of two exactly) and the read-out is the rational
    o = sum_i 2^n_i v_i / (sum_i 2^n_i + n_out),
which ``exact_read`` evaluates without rounding.  (This needs the kernel to split fl32(q * qscale), the ROUNDED product:
bank.hip's mul_rounded.  A plain `q * qscale` is contracted into the lo plane's subtraction: profiles/r11_a_bank_exact_tests.md.)

Exactness budget (derived from the kernel's rules; ``budget_ok`` asserts it for every case).  Take one query; R = its logit range
(max - min over its cells, the masked cells' 0 included), q_v the value quantum (1, 1/2 or 1/4), V = max |v|, M = cells inside the
memory boxes, N = T h w.  Inside a segment the weights are P_i = 2^(n_i - mref): mref is an integer (a tile maximum), never above
the running maximum and -- a bump happens only when a tile maximum exceeds mref by MORE than 11.54 -- at most 11 below it.  Every
term P_i 64 v_i of an O accumulator is therefore a multiple of u = 2^(n_min - mref) 64 q_v and every partial sum, in any order, is
at most M V 64 2^(n_max - mref) = (M V / q_v) 2^R u.  A rescale by alpha = 2^(mref_old - mref_new) <= 1 and a merge weight
2^(m_s - m_tot) <= 1 move u and the sums together.  The same holds for l with u = 2^(n_min - mref) and the bound N 2^R u
(the masked term n_out 2^(-m_tot) is a multiple of that u because R counts the logit 0).  Hence
    max(N, M V / q_v) * 2^R <= 2^24
makes every partial sum of S, l and O exact in fp32 whatever the order and whatever mref the deferral rule picks.  (R enters
once: the 2^6 storage scale, the deferred reference and the merge factors multiply quantum and sum alike.)  For fp16's hi plane
P must be a normal or sub-normal power of two: 2^-24 <= 2^(n_i - mref) <= 2^11, i.e. R <= 24.  R <= 4, V = 8, q_v = 1/4 allows
N <= 32768 at M V / q_v; the chained cases (N = 49,200) use integer values and R <= 4: 49,200 * 8 * 16 < 2^24.

Roundings of the normalisation, counted from the code (each is one fp32 rounding, relative 2^-24):
  * cell inside the query box, one launch: iq = 2^-6 / l (one correctly rounded division), out = acc * iq (one multiply): TWO;
    none when l is a power of two (then the result is the exact rational, which fp32 holds: bit for bit).
  * cell outside the query box (or an object without a memory cell): mu = colsum * fl(1 / (T h w)): TWO; none when T h w is a
    power of two.
  * chained read of c chunks (bk_chain): each chunk's read-out carries its two; then inv = 1 / lsum (one), c products w_k out_k
    (one each), c - 1 additions, acc * inv (one).  Products and additions act on magnitudes up to A = sum_k w_k |out_k| / sum w_k,
    so the bound is 2^-24 * ((2 + 1 + (c - 1)) A + 2 |o|).
``tolerance`` turns these counts into an absolute bound per element (with a factor 1 + 2^-10 for second-order terms)."""

import functools

import numpy as np

KDE, KDO, KJT, KQT = 128, 512, 32, 64
MAX_T = 2048                              # frames per launch (bank.hip kMaxT)
K_SRAW = np.float32(1.0 / 4096.0)
K_DEFER_RAW = np.float32(11.5415603) * np.float32(4096.0)
QSCALE = np.float32(1.44269504088896341) / np.sqrt(np.float32(128.0)) * np.float32(64.0)   # as launch_bank_main evaluates it
LN2 = 0.6931471805599453
ALLOWED_A = (0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 16.0)
SPLIT_TARGET, MAX_OBJ_PER_LAUNCH = 256, 64  # common.h: kSplitTargetSlots, kBankMaxObj

# channels that carry the logit: two per 32-channel MFMA k-block; a = +-1 / mult, k = mult * {-1, 0, 1}
ACT = (3, 17, 40, 58, 70, 93, 101, 126)
MULT = (1, 2, 4, 1, 2, 1, 4, 1)
PAIRS = ((0, 3, (1, 2, 3, 4, 5, 6, 8, 16)), (5, 7, (1, 2, 3, 5, 8)), (1, 4, (1, 2, 4, 6)), (2, 6, (1, 2, 4, 8, 16)))
CH_U, CH_SHIFT = 9, 77                    # 'pow2' / 'spike': per-cell logit, per-query shift


@functools.lru_cache(maxsize=None)
def query_for(a):
    """float32 q with fl32(q * qscale) == 64 a exactly (a neighbour of 64 a / qscale)."""
    if a == 0.0:
        return np.float32(0.0)
    want = np.float32(64.0 * a)
    q = np.float32(float(want) / float(QSCALE))
    cands = [q]
    lo = hi = q
    for _ in range(8):
        lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
        hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
        cands += [lo, hi]
    for c in cands:
        if np.float32(c * QSCALE) == want:
            return np.float32(c)
    raise AssertionError('no float32 query for a = %r' % a)


def _rect_mask(r, h, w):
    m = np.zeros((h, w), bool)
    x0, x1, y0, y1 = (int(v) for v in r)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 <= x1 and y0 <= y1:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def _pow2_counts(n):
    """Counts c_0..c_4 (sum n, every c_i >= 1) with sum c_i 2^i a power of two."""
    p = 1
    while p <= n:
        p *= 2
    while True:
        r = p - n - 26                     # one cell each at logits 1..4 uses 1 + 3 + 7 + 15
        if r >= 0:
            c = [0, 1, 1, 1, 1]
            for i, g in ((4, 15), (3, 7), (2, 3), (1, 1)):
                c[i] += r // g
                r %= g
            if sum(c) <= n:
                c[0] = n - sum(c)
                if c[0] >= 1:
                    return c
        p *= 2


def make_case(name, no, T, h, w, mem_rects=None, qry_rects=None, logits='general', vals='int', junk=False, seed=0,
              spike=None, family=''):
    """One case.  logits: 'equal' (all 0, by cancelling channel pairs), 'general' (n in [-2, 2] per (query, cell)), 'pow2' (dense:
    per-cell logits 0..4 with counts that make l a power of two, plus a per-query shift), 'spike' ('equal' plus one cell at 12:
    spike = (frame, y, x)).  vals: 'int' (|v| <= 8), 'quarter' (multiples of 1/4), 'sign' ({-1, 0, 1}).  junk: the channels that carry
    no logit are non-zero -- even ones in the keys, odd ones in the queries, so every product is still 0."""
    rng = np.random.RandomState(seed + 7919 * no + 31 * T + h * w)
    kint = np.zeros((no, KDE, T, h, w), np.float32)
    aq = np.zeros((no, KDE, h, w), np.float64)
    sgn = lambda shape: rng.randint(0, 2, shape) * 2 - 1
    if logits == 'general':
        nz = rng.randint(1, 3, (no, T, h, w))                      # one or two live channels per cell
        c1 = rng.randint(0, 8, (no, T, h, w))
        c2 = (c1 + rng.randint(1, 8, (no, T, h, w))) % 8
        for ci, (ch, mu) in enumerate(zip(ACT, MULT)):
            live = (c1 == ci) | ((c2 == ci) & (nz == 2))
            kint[:, ch] = live * sgn((no, T, h, w)) * mu
            aq[:, ch] = sgn((no, h, w)) / float(mu)
    else:
        for ci, (ch, mu) in enumerate(zip(ACT, MULT)):
            kint[:, ch] = mu
        for i, j, bs in PAIRS:
            b = np.asarray(bs, np.float64)[rng.randint(0, len(bs), (no, h, w))] * sgn((no, h, w))
            aq[:, ACT[i]] = b / MULT[i]
            aq[:, ACT[j]] = -b / MULT[j]
        if logits == 'pow2':
            assert mem_rects is None
            for o in range(no):
                u = np.repeat(np.arange(5), _pow2_counts(T * h * w))
                kint[o, CH_U] = rng.permutation(u).reshape(T, h, w)
            aq[:, CH_U] = 1.0
            kint[:, CH_SHIFT] = 1
            aq[:, CH_SHIFT] = rng.randint(-2, 3, (no, h, w))
        elif logits == 'spike':
            t, y, x = spike
            kint[:, CH_U, t, y, x] = 3
            aq[:, CH_U] = np.where(rng.rand(no, h, w) < 0.5, 4.0, 0.0)     # half of the queries see the spike (12), half do not
            aq[:, CH_U, 0, 0] = 4.0
        else:
            assert logits == 'equal'
    if junk:
        used = set(ACT) | {CH_U, CH_SHIFT}
        for ch in range(KDE):
            if ch in used:
                continue
            if ch % 2 == 0:
                kint[:, ch] = rng.randint(-3, 4, (no, T, h, w))
            else:
                aq[:, ch] = np.asarray(ALLOWED_A)[rng.randint(0, len(ALLOWED_A), (no, h, w))] * sgn((no, h, w))
    q_key = np.zeros((no, KDE, h, w), np.float32)
    for a in np.unique(aq):
        q_key[aq == a] = query_for(float(a))
    assert np.array_equal(q_key * QSCALE, (64.0 * aq).astype(np.float32)), 'scaled queries must be exactly 64 a'
    assert (q_key * QSCALE).dtype == np.float32
    if vals == 'int':
        m_val, vq = rng.randint(-8, 9, (no, KDO, T, h, w)).astype(np.float32), 1.0
    elif vals == 'quarter':
        m_val, vq = (rng.randint(-32, 33, (no, KDO, T, h, w)) / 4.0).astype(np.float32), 0.25
    else:
        m_val, vq = rng.randint(-1, 2, (no, KDO, T, h, w)).astype(np.float32), 1.0
    q_val = rng.randint(-8, 9, (no, KDO, h, w)).astype(np.float32)
    case = dict(name=name, family=family, no=no, T=T, h=h, w=w, m_key=kint, m_val=m_val, q_key=q_key, q_val=q_val, a=aq, vq=vq,
                logits=logits, mem_rects=None if mem_rects is None else np.asarray(mem_rects, np.int32).reshape(no, T, 4),
                qry_rects=None if qry_rects is None else np.asarray(qry_rects, np.int32).reshape(no, 4))
    assert (case['mem_rects'] is None) == (case['qry_rects'] is None)
    return case


def full_rects(case):
    """(mem_rects, qry_rects) with whole-grid boxes for a dense case (the entries that want rectangles)."""
    no, T, h, w = case['no'], case['T'], case['h'], case['w']
    if case['mem_rects'] is not None:
        return case['mem_rects'], case['qry_rects']
    f = np.array([0, w - 1, 0, h - 1], np.int32)
    return np.tile(f, (no, T, 1)), np.tile(f, (no, 1))


def with_garbage(case, seed=99):
    """The same case with non-integers in every masked key / value cell and in the keys of the query cells outside the box."""
    mr, qr = full_rects(case)
    rng = np.random.RandomState(seed)
    g = dict(case)
    mk, mv, qk = case['m_key'].copy(), case['m_val'].copy(), case['q_key'].copy()
    for o in range(case['no']):
        for t in range(case['T']):
            out = ~_rect_mask(mr[o, t], case['h'], case['w'])
            n = int(out.sum())
            mk[o, :, t][:, out] = (rng.randn(KDE, n) * 3.3).astype(np.float32)
            mv[o, :, t][:, out] = (rng.randn(KDO, n) * 7.7).astype(np.float32)
        out = ~_rect_mask(qr[o], case['h'], case['w'])
        qk[o][:, out] = (rng.randn(KDE, int(out.sum())) * 2.1).astype(np.float32)
    g.update(m_key=mk, m_val=mv, q_key=qk)
    return g


# ------------------------------------------------------------------------------------------------ exact reference
def _is_pow2(x):
    m, _ = np.frexp(x)
    return m == 0.5


def _object_logits(case, o, t0, t1):
    """(memory mask [t, h, w], query mask [h, w], integer logits [cells, queries]) of frames [t0, t1)."""
    mr, qr = full_rects(case)
    h, w = case['h'], case['w']
    mm = np.stack([_rect_mask(mr[o, t], h, w) for t in range(t0, t1)])
    qm = _rect_mask(qr[o], h, w)
    k = case['m_key'][o][:, t0:t1][:, mm].astype(np.float64)          # [128, M]
    n = k.T @ case['a'][o][:, qm]                                     # exact: small integers and quarters
    assert np.array_equal(n, np.rint(n)), 'logits must be integers'
    return mm, qm, n


def exact_read(case, per_launch=MAX_T):
    """The read-out as an exact rational per element, evaluated in float64 on integers below 2^53 (so num and den are exact; the
    one division rounds to 2^-53, and not at all where den is a power of two).  Returns a dict:
      out     [no, 1024, h, w] float64
      exact   [no, 1024, h, w] bool: the kernel must return np.float32(out) bit for bit
      amag    [no, 1024, h, w] float64: A of the chained reads (= |out| for one launch)
      nchunk, R (largest logit range of a query), nmax (largest logit, the masked 0 included), budget (largest budget product)."""
    no, T, h, w, hw = case['no'], case['T'], case['h'], case['w'], case['h'] * case['w']
    chunks = [(t0, min(t0 + per_launch, T)) for t0 in range(0, T, per_launch)]
    out = np.zeros((no, 2 * KDO, h, w))
    exact = np.ones((no, 2 * KDO, h, w), bool)
    amag = np.zeros((no, 2 * KDO, h, w))
    _, qr = full_rects(case)
    inv_vq = 1.0 / case['vq']
    R = nmax = 0
    budget = 0.0
    for o in range(no):
        xs, ws, ex = [], [], []
        qm = _rect_mask(qr[o], h, w)
        nlo = nhi = None
        Mtot = 0
        for t0, t1 in chunks:
            mm, _, n = _object_logits(case, o, t0, t1)
            Tc, M = t1 - t0, int(mm.sum())
            Mtot += M
            v = case['m_val'][o][:, t0:t1][:, mm].astype(np.float64) * inv_vq      # integers
            x = np.zeros((KDO, h, w))
            wgt = np.full((h, w), float(Tc * hw))
            e = np.zeros((h, w), bool)
            x[:, ~qm] = (v.sum(axis=1) * case['vq'] / (Tc * hw))[:, None]           # the mean of the boxed values over ALL cells
            e[~qm] = _is_pow2(float(Tc * hw))
            if M > 0 and qm.any():
                n_out = Tc * hw - M
                lo = np.minimum(n.min(axis=0), 0.0) if n_out else n.min(axis=0)
                hi = np.maximum(n.max(axis=0), 0.0) if n_out else n.max(axis=0)
                nlo = lo if nlo is None else np.minimum(nlo, lo)
                nhi = hi if nhi is None else np.maximum(nhi, hi)
                W = np.exp2(n - lo)
                num, den = v @ W, W.sum(axis=0) + n_out * np.exp2(-lo)
                assert np.abs(num).max() < 2.0 ** 53 and den.max() < 2.0 ** 53
                x[:, qm] = num * case['vq'] / den
                wgt[qm] = den * np.exp2(lo)
                e[qm] = _is_pow2(den)
            else:
                e[qm] = True                                                        # no memory cell inside a box: the read-out is 0
                if Tc * hw - M:
                    z = np.zeros(int(qm.sum()))
                    nlo = z if nlo is None else np.minimum(nlo, z)
                    nhi = z if nhi is None else np.maximum(nhi, z)
            xs.append(x); ws.append(wgt); ex.append(e)
        if len(chunks) == 1:
            out[o, :KDO], exact[o, :KDO], amag[o, :KDO] = xs[0], ex[0][None], np.abs(xs[0])
        else:
            wsum = sum(ws)
            out[o, :KDO] = sum(wk * xk for wk, xk in zip(ws, xs)) / wsum
            amag[o, :KDO] = sum(wk * np.abs(xk) for wk, xk in zip(ws, xs)) / wsum
            exact[o, :KDO] = False
        out[o, KDO:] = case['q_val'][o] * qm
        if nlo is not None and nlo.size:
            r = int((nhi - nlo).max())
            R, nmax = max(R, r), max(nmax, int(nhi.max()))
            budget = max(budget, max(T * hw, Mtot * float(np.abs(case['m_val'][o]).max()) * inv_vq) * 2.0 ** r)
    return dict(out=out, exact=exact, amag=amag, nchunk=len(chunks), R=R, nmax=nmax, budget=budget)


def exact_read_fraction(case, o, d, y, x):
    """One element in fractions.Fraction, straight from the semantics in bank.hip's header (slow; cross-check of exact_read)."""
    from fractions import Fraction
    mr, qr = full_rects(case)
    T, h, w = case['T'], case['h'], case['w']
    if d >= KDO:
        return Fraction(float(case['q_val'][o, d - KDO, y, x])) * int(_rect_mask(qr[o], h, w)[y, x])
    num, den = Fraction(0), Fraction(0)
    inside = _rect_mask(qr[o], h, w)[y, x]
    for t in range(T):
        mm = _rect_mask(mr[o, t], h, w)
        for yy in range(h):
            for xx in range(w):
                if mm[yy, xx] and inside:
                    n = sum(Fraction(float(case['m_key'][o, c, t, yy, xx])) * Fraction(float(case['a'][o, c, y, x])) for c in range(KDE)
                            if case['m_key'][o, c, t, yy, xx] != 0)
                    assert n.denominator == 1
                    wgt = Fraction(2) ** int(n)
                    num += wgt * Fraction(float(case['m_val'][o, d, t, yy, xx]))
                    den += wgt
                else:
                    den += 1                                   # masked cell (or a query outside its box: every logit is 0) ...
                    if mm[yy, xx]:
                        num += Fraction(float(case['m_val'][o, d, t, yy, xx]))   # ... whose boxed value still counts in the mean
    return num / den


def budget_ok(ref):
    return ref['budget'] <= 2.0 ** 24 and ref['R'] <= 24


def tolerance(ref):
    """Absolute bound per element from the rounding counts in the module docstring (0 where the result must be bit-exact)."""
    u = 2.0 ** -24 * (1.0 + 2.0 ** -10)
    if ref['nchunk'] == 1:
        tol = 2.0 * u * np.abs(ref['out'])
    else:
        c = ref['nchunk']
        tol = u * ((2 + 1 + (c - 1)) * ref['amag'] + 2.0 * np.abs(ref['out']))
    tol = np.where(ref['exact'], 0.0, tol)
    tol[:, KDO:] = 0.0
    return tol


def check_read(got, ref, what=''):
    """The part-2 comparison: bit for bit (uint32 view) where the reference says so, the counted roundings elsewhere, channels
    512.. exact.  One exception to the uint32 view: +0 against -0 passes.  The sign of a zero is not part of the read's semantics --
    `q_val x box` is -0 for a negative q_val outside the box when evaluated as a product and +0 when the cell is written as a
    zero, and the sign of an exactly cancelling sum follows the order of its terms -- so the reference cannot name it."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and not np.isnan(got).any(), what
    want32 = ref['out'].astype(np.float32)
    ex = ref['exact']
    bad = (got.view(np.uint32) != want32.view(np.uint32)) & ex & ~((got == 0) & (want32 == 0))
    assert not bad.any(), '%s: %d of %d bit-exact elements differ, first at %s: got %r want %r' % (
        what, int(bad.sum()), int(ex.sum()), tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], want32[tuple(np.argwhere(bad)[0])])
    err = np.abs(got.astype(np.float64) - ref['out'])
    over = err > tolerance(ref)
    assert not over.any(), '%s: %d elements beyond the counted roundings, worst %.3g x the bound' % (
        what, int(over.sum()), float((err[over] / np.maximum(tolerance(ref)[over], 1e-300)).max()))


def expected_logit_word(case, mode='split'):
    """The bank's logit word (natural units, as MemoryBank.logit_max returns it) where it is determined: every object is a single
    step of the walk (one 32-cell tile; two in the fp16 modes), or the first tile of every object holds its maximum.  Else None."""
    step = KJT if mode == 'split' else 2 * KJT
    mr, _ = full_rects(case)
    word = 0.0
    for o in range(case['no']):
        mm, qm, n = _object_logits(case, o, 0, min(case['T'], MAX_T))
        if n.size == 0:
            continue
        areas = mm.reshape(mm.shape[0], -1).sum(axis=1)
        tiles = int(((areas + KJT - 1) // KJT).sum())
        first = int(areas[areas > 0][0]) if (areas > 0).any() else 0
        single = tiles * KJT <= step and (tiles == 1 or mode != 'split')
        top = n.max(axis=0)
        first_has_max = bool((n[:min(first, KJT)].max(axis=0) == top).all()) and case['T'] <= MAX_T
        if not (single or first_has_max):
            return None
        word = max(word, float(top.max()))
    return float(np.float32(word)) * LN2


def spike_tile(case):
    """(tile, tiles) of a dense 'spike' case: the index of the 32-cell tile that holds the spike in the object's tile list."""
    t, y, x = [int(i[0]) for i in np.nonzero(case['m_key'][0, CH_U])]
    per = (case['h'] * case['w'] + KJT - 1) // KJT
    return t * per + (y * case['w'] + x) // KJT, case['T'] * per


def true_logit_max(case):
    """Largest logit of the case in natural units (0 at least: the word starts at 0)."""
    top = 0.0
    for o in range(case['no']):
        for t0 in range(0, case['T'], MAX_T):
            _, _, n = _object_logits(case, o, t0, min(t0 + MAX_T, case['T']))
            if n.size:
                top = max(top, float(n.max()))
    return top * LN2


# ------------------------------------------------------------------------------------------------ launch plans (host rule restated)
def plan_of(case):
    """What bk_main's plan does with the case, as far as the tests name it: 'fast' / 'lds' (<= 12 objects and <= 64 frames: areas in
    registers, else LDS atomics), launch groups (64 objects each) and whether a group has more (object, query tile) pairs than
    workgroups (then it runs in rounds; kSplitTargetSlots is an upper bound of the target, so pairs > 256 is sufficient).
    'even_cut' is where the device's search for the chunk length (tiles per workgroup) starts: the launch's tile pairs spread
    evenly over the workgroups, at least bank_chunk_min().  The search itself (equalised blocks, remainder chunks, the workgroups set
    aside) is NOT restated: how far above the even cut the chunk length ends up is the device's decision."""
    mr, qr = full_rects(case)
    no, T, h, w = case['no'], min(case['T'], MAX_T), case['h'], case['w']
    groups = []
    for g0 in range(0, no, MAX_OBJ_PER_LAUNCH):
        ng = min(no - g0, MAX_OBJ_PER_LAUNCH)
        pairs = work = njt_max = 0
        for o in range(g0, g0 + ng):
            njt = sum((int(_rect_mask(mr[o, t], h, w).sum()) + KJT - 1) // KJT for t in range(T))
            nqt = (int(_rect_mask(qr[o], h, w).sum()) + KQT - 1) // KQT
            pairs += nqt if njt else 0
            work += nqt * njt
            njt_max = max(njt_max, njt)
        cmin = max((njt_max + 60) // 61, 4)                              # common.h: bank_chunk_min (kSplitMax 64, kSplitMinTiles 4)
        groups.append(dict(nobj=ng, plan='fast' if ng <= 12 and T <= 64 else 'lds', pairs=pairs, rounds=pairs > SPLIT_TARGET,
                           even_cut=max(-(-work // SPLIT_TARGET), cmin)))
    return groups


# ------------------------------------------------------------------------------------------------ the tile loop, restated in numpy
MUTANTS = ('drop_last_cell', 'pad_in_l', 'n_out_off', 'swap_kperm', 'skip_second_tile', 'no_rescale', 'drop_chunk')
ALL_MUTANTS = MUTANTS + ('trunc_v',)     # V's hi plane truncated: an operand fault, visible on non-integer values only (part 3)


def _to_f16(x, trunc=False):
    """float32 -> fp16 -> float32, to nearest; trunc: toward zero."""
    hf = x.astype(np.float16)
    if trunc:
        over = np.abs(hf.astype(np.float32)) > np.abs(x)
        hf[over] = np.nextafter(hf[over], np.float16(0))
    return hf.astype(np.float32)


def _frame_tiles(case, o, t0, t1, f16_operands=False, trunc_v=False):
    """Tile list of frames [t0, t1): (K64 [32, 128], V64 [512, 32], nvalid, last tile of its frame, tiles of its frame).
    f16_operands: K64 and V64 rounded to fp16, the hi planes the fp16 modes multiply (a no-op on the integer cases)."""
    mr, _ = full_rects(case)
    h, w = case['h'], case['w']
    tiles = []
    for t in range(t0, t1):
        mm = _rect_mask(mr[o, t], h, w)
        k = (case['m_key'][o, :, t][:, mm] * np.float32(64)).T           # compact order = row-major inside the box
        v = case['m_val'][o, :, t][:, mm] * np.float32(64)
        if f16_operands:
            k, v = _to_f16(k), _to_f16(v, trunc_v)
        area = k.shape[0]
        nt = (area + KJT - 1) // KJT
        for u in range(nt):
            kk = np.zeros((KJT, KDE), np.float32)
            vv = np.zeros((KDO, KJT), np.float32)
            nv = min(area - u * KJT, KJT)
            kk[:nv] = k[u * KJT:u * KJT + nv]
            vv[:, :nv] = v[:, u * KJT:u * KJT + nv]
            tiles.append((kk, vv, nv, u == nt - 1, nt))
    return tiles


def _walk(tiles, qs, mode, mutant):
    """One segment: the online soft-max over its tiles (one per step; two in the fp16 modes).  Returns (acc [512, Q], m [Q], l [Q])."""
    Q = qs.shape[1]
    mref = np.full(Q, -np.inf, np.float32)
    l = np.zeros(Q, np.float32)
    acc = np.zeros((KDO, Q), np.float32)
    per = 1 if mode == 'split' else 2
    for s0 in range(0, len(tiles), per):
        step = list(tiles[s0:s0 + per])
        if mutant == 'skip_second_tile' and len(step) == 2 and step[0][3] and step[0][4] % 2 == 1:
            step = step[:1]
        S, V, pad = [], [], []
        for kk, vv, nv, last, _ in step:
            if mutant == 'drop_last_cell' and last:
                nv -= 1
            if mutant == 'swap_kperm' and s0 == 0 and nv >= 2:
                vv = vv.copy()
                vv[:, [0, 1]] = vv[:, [1, 0]]
            s = kk @ qs                                                   # raw units: 4096 n (exact in fp32)
            s[nv:] = -np.inf
            S.append(s); V.append(vv); pad.append(np.arange(KJT) >= nv)
        S, V, pad = np.concatenate(S), np.concatenate(V, axis=1), np.concatenate(pad)
        with np.errstate(invalid='ignore', over='ignore'):
            tmax = S.max(axis=0)
            bump = tmax > mref + K_DEFER_RAW
            alpha = np.where(bump, np.exp2((mref - tmax) * K_SRAW), np.float32(1)).astype(np.float32)
            mref = np.where(bump, tmax, mref)
            P = np.exp2(S * K_SRAW - mref * K_SRAW).astype(np.float32)
        if mode != 'split':
            P = P.astype(np.float16).astype(np.float32)
        lp = P.sum(axis=0, dtype=np.float32)
        if mutant == 'pad_in_l':
            with np.errstate(invalid='ignore'):
                lp = lp + np.where(np.isfinite(mref), np.float32(pad.sum()) * np.exp2(-mref * K_SRAW), 0).astype(np.float32)
        l = l * alpha + lp
        if mutant != 'no_rescale':
            acc = acc * alpha
        acc = acc + V @ P
    return acc, mref * K_SRAW, l


def tile_loop_read(case, mode='split', chunk_tiles=None, mutant=None, per_launch=MAX_T):
    """bk_append / bk_main / bk_chain restated: 32-cell tiles with zero padding, steps of one tile (two in 'f16' / 'qx'), the
    deferred reference, segments of ``chunk_tiles`` tiles merged with 2^(m_s - m_tot) and the masked cells' n_out 2^(-m_tot),
    iq = 2^-6 / l, the column-sum mean outside the query box, the chain over launches of ``per_launch`` frames.  fp32 throughout.
    Structure only: no lane layout.  ``mutant`` plants one fault (ALL_MUTANTS).  In 'f16' and 'qx' the operands are the fp16
    planes the kernels multiply (K64, V64 and the scaled query to fp16; in 'qx' the query keeps its lo plane) -- the identity on
    the integer cases, the modes' own rounding on random inputs; 'split' multiplies hi + lo pairs, restated here as fp32."""
    f16_ops = mode != 'split'
    no, T, h, w, hw = case['no'], case['T'], case['h'], case['w'], case['h'] * case['w']
    _, qr = full_rects(case)
    chunks = [(t0, min(t0 + per_launch, T)) for t0 in range(0, T, per_launch)]
    out = np.zeros((no, 2 * KDO, h, w), np.float32)
    for o in range(no):
        qm = _rect_mask(qr[o], h, w)
        qs = case['q_key'][o][:, qm] * QSCALE                              # [128, Q] float32; the fragments' hi plane (lo is 0)
        if f16_ops:
            qs = _to_f16(qs) + (_to_f16(qs - _to_f16(qs)) if mode == 'qx' else np.float32(0))
        res, ms, ls = [], [], []
        for t0, t1 in chunks:
            Tc = t1 - t0
            tiles = _frame_tiles(case, o, t0, t1, f16_ops, mutant == 'trunc_v')
            mr, _ = full_rects(case)
            M = sum(int(_rect_mask(mr[o, t], h, w).sum()) for t in range(t0, t1))
            colsum = np.zeros(KDO, np.float32)                              # bk_append sums the fp32 values, not a plane
            for _, vv, _, _, _ in (_frame_tiles(case, o, t0, t1) if f16_ops and case.get('random') else tiles):
                colsum += vv.sum(axis=1, dtype=np.float32) / np.float32(64)
            x = np.zeros((KDO, h, w), np.float32)
            x[:] = (colsum * (np.float32(1) / (np.float32(Tc) * np.float32(hw))))[:, None, None]
            m_c = np.zeros((h, w), np.float32)
            l_c = np.full((h, w), np.float32(Tc * hw), np.float32)
            if tiles and qm.any():
                C = chunk_tiles or len(tiles)
                parts = [_walk(tiles[j:j + C], qs, mode, mutant) for j in range(0, len(tiles), C)]
                n_out = np.float32(Tc * hw - M + (1 if mutant == 'n_out_off' else 0))
                mtot = np.max([p[1] for p in parts], axis=0)
                if n_out > 0:
                    mtot = np.maximum(mtot, np.float32(0))
                wts = [np.exp2(p[1] - mtot).astype(np.float32) for p in parts]
                lt = sum(p[2] * wt for p, wt in zip(parts, wts))
                if n_out > 0:
                    lt = lt + n_out * np.exp2(-mtot)
                acc = sum(p[0] * wt for p, wt in zip(parts, wts))
                x[:, qm] = acc * (np.float32(1.0 / 64.0) / lt.astype(np.float32))
                m_c[qm], l_c[qm] = mtot, lt
            res.append(x); ms.append(m_c); ls.append(l_c)
        if len(chunks) == 1:
            out[o, :KDO] = res[0]
        else:
            mmax = np.max(ms, axis=0)
            wg = [(lc * np.exp2(mc - mmax)).astype(np.float32) for lc, mc in zip(ls, ms)]
            if mutant == 'drop_chunk':
                wg[-1] = np.zeros_like(wg[-1])
            inv = np.float32(1) / sum(wg)
            out[o, :KDO] = sum(wk * xk for wk, xk in zip(wg, res)) * inv
        out[o, KDO:] = case['q_val'][o] * qm
    return out


def mutant_touches(case, mutant, mode):
    """Does the planted fault change a row this case reads?  (A case it does not touch must still pass.)"""
    mr, qr = full_rects(case)
    no, T, h, w = case['no'], case['T'], case['h'], case['w']
    hit = False
    for o in range(no):
        if not _rect_mask(qr[o], h, w).any():
            continue
        areas = [int(_rect_mask(mr[o, t], h, w).sum()) for t in range(T)]
        live = [a for a in areas if a]
        if not live:
            continue
        if mutant in ('drop_last_cell', 'n_out_off'):
            hit = True
        elif mutant == 'pad_in_l':
            hit |= any(a % KJT for a in live)
        elif mutant == 'swap_kperm':
            if min(live[0], KJT) >= 2:     # (cells of equal weight can be swapped unseen: the two logits must differ for a query)
                _, _, n = _object_logits(case, o, 0, min(T, MAX_T))
                hit |= bool((n[0] != n[1]).any())
        elif mutant == 'skip_second_tile':
            if mode != 'split':
                for c0 in range(0, T, MAX_T):
                    j = 0
                    lv = [a for a in areas[c0:c0 + MAX_T] if a]
                    for i, a in enumerate(lv):
                        nt = (a + KJT - 1) // KJT
                        if nt % 2 == 1 and (j + nt - 1) % 2 == 0 and i + 1 < len(lv):
                            hit = True
                        j += nt
        elif mutant == 'no_rescale':
            hit |= case['logits'] == 'spike'
        elif mutant == 'drop_chunk':
            hit |= T > MAX_T and any(areas[(T - 1) // MAX_T * MAX_T:])
    return hit


# ------------------------------------------------------------------------------------------------ part 3: random inputs, fp16 operands
def float64_read(case):
    """The read of a case in float64 on its float32 inputs as they are (semantics of bank.hip's header): what the whole-tensor
    bars of tests/test_gpu_parity.py compare with."""
    mr, qr = full_rects(case)
    no, T, h, w = case['no'], case['T'], case['h'], case['w']
    out = np.zeros((no, 2 * KDO, h, w))
    for o in range(no):
        mm = np.stack([_rect_mask(mr[o, t], h, w) for t in range(T)])
        qm = _rect_mask(qr[o], h, w)
        v = case['m_val'][o][:, mm].astype(np.float64)
        out[o, :KDO] = (v.sum(axis=1) / (T * h * w))[:, None, None]
        out[o, KDO:] = case['q_val'][o] * qm
        if v.shape[1] and qm.any():
            s = case['m_key'][o][:, mm].astype(np.float64).T @ case['q_key'][o][:, qm].astype(np.float64) / np.sqrt(128.0)
            top = np.maximum(s.max(axis=0), 0.0)
            wgt = np.exp(s - top)
            out[o, :KDO][:, qm] = (v @ wgt) / (wgt.sum(axis=0) + (T * h * w - v.shape[1]) * np.exp(-top))
    return out


def f16_operand_read(mk, mv, qk, qv, mr, qr, qx=False, trunc_v=False):
    """The read in float64 on the operands the fp16 modes actually multiply, and a bound on every element of what the kernel may
    add to it.  Deterministic roundings, reproduced here: K~ = fp16(64 K), V~ = fp16(64 V) (bk_append's hi planes),
    q~ = fp16(fl32(q * qscale)) -- in 'qx' the pair hi + lo.  Log2 logits s_i = K~_i . q~ / 4096, weights w_i = 2^(s_i - smax) (so
    max w = 1; smax counts the masked cells' 0), L = sum w_i + n_out 2^-smax, o = sum w_i v~_i / L.

    What the kernel adds (first order, derived here):
      1. weight rounding.  P_i = fp16(exp2(...)) relative to a reference mref <= the running maximum, so the largest P is >= 1 and
         a weight is off by <= 2^-11 relative while P_i is normal in fp16, by <= 2^-25 absolute (in units where max w >= 1) below.
         The logit itself comes out of fp32 MFMA chains (4 per tile, 8 in 'qx'; one rounding each and as much again inside, all
         below 2^-24 sum_c |K~ q~|), the fma and v_exp_f32 (2^-23 |s - m| and one ulp): eps_i = 2^-11 + ln2 2^-24 (nm t_i +
         2 |s_i - smax| + 24) + 2^-22 with t_i = sum_c |K~_ic q~_c| / 4096 and nm = 8 (16 in 'qx').
         With o' = sum (w_i + d_i) v_i / (L + sum d_i):  |o' - o| <= sum |d_i| |v~_i - o| / L, |d_i| <= eps_i w_i + 2^-25, and the
         masked cells (v = 0, weight off by 2^-22 relative) add 2^-22 |o|.
      2. sub-normal term: 2^-25 sum_i |v~_i - o| / L  (already inside |d_i|).
      3. fp32 accumulation of O and l: one rounding per MFMA (2 per tile and accumulator, <= 2 njt), per merge and rescale (<= 64 + 8),
         each <= 2^-24 of the partial sum's magnitude: 2^-24 (2 njt + 72) (sum w_i |v~_i| / L + |o|), and the two roundings of the
         normalisation: 2^-23 |o|.
    The whole is multiplied by 1 + 2^-8 for the second-order terms.  As the issue states the form, the leading factor comes to
    about 2^-11 (one-sided: 2^-10 would allow the numerator and the denominator to move against each other, which the exact
    first-order expression above already contains in |v~_i - o|).
    Returns (out [no, 1024, h, w] float64, bound [no, 512, h, w]).  trunc_v: V's hi plane truncated toward zero instead of rounded
    (the operand fault of the CPU mutant test)."""
    no, _, T, h, w = mk.shape
    hw = h * w
    out = np.zeros((no, 2 * KDO, h, w))
    bound = np.zeros((no, KDO, h, w))
    f16 = lambda x: x.astype(np.float16).astype(np.float64)
    for o in range(no):
        mm = np.stack([_rect_mask(mr[o, t], h, w) for t in range(T)])
        qm = _rect_mask(qr[o], h, w)
        k = f16(mk[o][:, mm] * np.float32(64))
        v32 = mv[o][:, mm] * np.float32(64)
        v = _to_f16(v32, trunc_v).astype(np.float64) / 64.0
        M = k.shape[1]
        colsum = mv[o][:, mm].astype(np.float64).sum(axis=1)
        out[o, :KDO] = (colsum / (T * hw))[:, None, None]
        bound[o] = (np.abs(mv[o][:, mm]).astype(np.float64).sum(axis=1) * (hw * T + 4) * 2.0 ** -24 / (T * hw))[:, None, None]
        out[o, KDO:] = qv[o] * qm
        if M == 0 or not qm.any():
            continue
        qsc = qk[o][:, qm] * QSCALE                                       # float32
        qh = qsc.astype(np.float16)
        qt = qh.astype(np.float64)
        if qx:
            qt = qt + f16(qsc - qh.astype(np.float32))
        s = (k.T @ qt) / 4096.0                                           # [M, Q]
        t_abs = (np.abs(k).T @ np.abs(qt)) / 4096.0
        n_out = T * hw - M
        smax = np.maximum(s.max(axis=0), 0.0) if n_out else s.max(axis=0)
        wgt = np.exp2(s - smax)
        L = wgt.sum(axis=0) + n_out * np.exp2(-smax)
        oo = (v @ wgt) / L                                                # [512, Q]
        eps = 2.0 ** -11 + LN2 * 2.0 ** -24 * ((16 if qx else 8) * t_abs + 2 * np.abs(s - smax) + 24) + 2.0 ** -22
        d = eps * wgt + 2.0 ** -25                                        # [M, Q]
        njt = int(((mm.reshape(T, -1).sum(axis=1) + KJT - 1) // KJT).sum())
        # sum_i d_i |v_i - o| <= sqrt(sum d_i * sum d_i (v_i - o)^2)  (Cauchy-Schwarz: three matrix products instead of a
        # [512, M, Q] array; an upper bound of the sum, about 1.25x for Gaussian values)
        D = d.sum(axis=0)
        var = (v * v) @ d - 2.0 * oo * (v @ d) + oo * oo * D
        b = np.sqrt(D * np.maximum(var, 0.0)) / L + 2.0 ** -22 * np.abs(oo)
        b += 2.0 ** -24 * (2 * njt + 72) * ((np.abs(v) @ wgt) / L + np.abs(oo)) + 2.0 ** -23 * np.abs(oo)
        out[o, :KDO][:, qm] = oo
        bound[o][:, qm] = b * (1 + 2.0 ** -8)
    return out, bound
