# -*- coding: utf-8 -*-
"""Cases, references and the error bound for the GENERIC path of rmnet_memory_read_f32: p_kernel and pv_kernel at the end of
rmnet_amd/csrc/memory_read.hip (any De <= 224, any Do, strided memory tensors, rectangles compared and not clamped), and the
affinity output p that p_kernel alone produces after the fast path.  No torch, no GPU: tests/test_memory_read_generic.py imports
this on any machine.

Semantics (memory_read.hip's header).  K, V are multiplied by the 0/1 maps of the memory rectangles, q_key and q_val by the map of
the query rectangle; S = K^T Q / sqrt(De); p = soft-max of S over ALL T h w cells (a masked cell has logit 0, not -inf);
out = cat(V p, q_val x box).  A rectangle is (x0, x1, y0, y1), both ends inclusive, and may stick out of the grid or be empty.

  read_f64   the semantics in float64: what every comparison refers to.
  read_f32   what the two kernels do, in numpy float32, in their order (below).  It carries the planted faults (MUTANTS); it need not
             match the device bit for bit on general inputs (hipcc contracts a * b + c into one FMA, numpy rounds twice).
  bound      a per-element bound on |device - read_f64| for p and out, from the roundings counted below.

The kernels' order, per object and query cell i (p_kernel: 64 query cells x 4 strided memory sequences jj = 0..3 per workgroup):
  1. dot_j = sum_c k_cj q_ci for c = 0 .. De-1 in order, 0 for a masked memory cell or a masked query       (De fp32 operations)
  2. s_j = dot_j / fl(sqrt(De))                                                            (sqrtf once on the host, one division)
  3. mx = max_j s_j: four strided maxima j = jj, jj + 4, ..., merged                                                     (exact)
  4. e_j = expf(s_j - mx)                                                                      (one subtraction, one expf)
  5. sum = ((r_0 + r_1) + r_2) + r_3 with r_jj = e_jj + e_jj+4 + ... in order    (ceil(T h w / 4) - 1 additions each, then 3)
  6. p_j = e_j / sum                                                                                           (one division)
  pv_kernel:
  7. out_d = sum over the LIVE cells j in order of v_dj p_j (masked cells are skipped, not multiplied by 0)    (n operations)
  8. out_{Do + d} = q_val_d inside the query box, q_val_d * 0.0f outside (a zero of q_val's sign)                      (exact)

The bound (u = 2^-24 one rounding, eps = 2^-23 one ulp, gamma_n = n u / (1 - n u)), first order, times SLACK = 1 + 1e-3:
  1-2. |s^_j - s_j| <= gamma_De A_j / sqrt(De) + 2 u |s_j| =: ds_j  with A_j = sum_c |k_cj q_ci|   (dot product; sqrt and division)
  3-4. The soft-max does not change when the same constant is taken from every logit, so take the device's own mx^ (one of the s^_j,
       an fp32 number) as that constant in the reference too: the argument x^_j = fl(s^_j - mx^) is off by <= ds_j + u |x_j|
       (one rounding for s - max), and e^_j = exp(x^_j) (1 + E eps) with E = glue_ref.E_ULP ulps -- TWICE the largest error of the
       device's expf measured on [-34, 0] (profiles/r14_a_glue_tests.md).  So e^_j = e_j (1 + t_j), |t_j| <= r_j := ds_j + u |x_j| + E eps,
       valid while every x_j lies in [-34, 0]: ``bound`` asserts the logit spread of every query it bounds in float64.
  5.   all terms are positive: sum^ = sum (1 + sum_j p_j t_j) (1 + g), |g| <= gamma_{L + 3}, L = ceil(T h w / 4)  (the partial
       sums' lengths, plus 3 for the merge)
  6.   p^_j = p_j (1 + t_j - sum_i p_i t_i - g + one rounding):  |p^_j - p_j| <= p_j (r_j + sum_i p_i r_i + gamma_{L+3} + u) + TINY
       TINY = 2^-125 covers a quotient or an expf below fp32's normal range (flushed or rounded to a sub-normal).
  7.   |out^_d - out_d| <= gamma_n sum_j |v_dj| p_j + sum_j |v_dj| dp_j over the n live cells, dp_j the bound of step 6.
  8.   0.
No constant here comes from what the kernels return.

The case families (tests/test_memory_read_generic.py has the shapes and the rectangle sets):
  'onehot'  channels 0 and 1 hold the keys (x_j, -x_j^2 / 2), x_j = g (j + 1), j the cell's index in the T h w memory; a live query i
            holds (x_t, 1) for its target cell t = t(i).  Then S_j = (x_t^2 - (x_j - x_t)^2) / (2 sqrt(De)): the target wins by
            g^2 / (2 sqrt(De)) >= 256 over every live cell and by x_t^2 / (2 sqrt(De)) >= 256 over the masked cells' 0, g being the
            smallest power of two with g^2 >= 512 sqrt(De).  g^2 / 2 is a power of two and the dot product is g^2 / 2 times the
            integer 2 (j+1)(t+1) - (j+1)^2, below 2^24 in magnitude: exact in fp32 in any order, with or without FMA.  The other
            channels are zero on one side (keys in odd channels, queries in even ones) and arbitrary on the other: every product is
            a zero.  expf(0) = 1 and expf(x) = 0 for x <= -200 on this build (measured, profiles/r14_a_glue_tests.md), so while the
            fp32 logits are within 16 of the true ones the device's p is exactly 1 at the target and 0 elsewhere, and out[:, :Do] is
            the target's value vector bit for bit -- for random float values and whatever the order of the sum.
  'equal'   every logit is 0: zero keys ('zero') or keys in even and queries in odd channels ('orth').  p = fl(1 / (T h w)) bit
            for bit in every row (every e is 1, the four partial sums are integers, the division is correctly rounded); out[:, :Do]
            is bit for bit when T h w is a power of two and the values are integers with sum |v| < 2^24, inside the bound otherwise.
            The same holds for every masked query cell and every object without a live memory cell in ANY family.
  'random'  keys at two scales (halved until the logit spread of every query is <= 30, a power of two each time), values at scales
            1e-2, 1 and 1e2 by channel: every element of p and out inside the bound.
"""

import numpy as np

import glue_ref

F32 = np.float32
U = 2.0 ** -24
EPS = 2.0 ** -23
E_ULP = glue_ref.E_ULP
SLACK = 1.0 + 1e-3
TINY = 2.0 ** -125
SPREAD_MAX = 34.0
DE_MAX = 224                       # memory_read.hip: the query tile [De][64] + red[256] must fit 64 KB of LDS

MUTANTS = ('drop_tail', 'drop_cell_64', 'drop_last_channel', 'rect_exclusive', 'stride_thw', 'masked_neg_inf', 'masked_value_added',
           'rects_of_object0', 'qval_not_zeroed', 'sqrt_is_De')


def gamma(n):
    return n * U / (1.0 - n * U)


def dims(case):
    return case['no'], case['De'], case['Do'], case['T'], case['h'], case['w']


# ================================================================================================ rectangles
def live_masks(case, o, mutant=None):
    """(memory cells [T * h * w], query cells [h * w]) inside their rectangles, by the kernels' comparisons (nothing is clamped)."""
    no, De, Do, T, h, w = dims(case)
    if case['mem_rects'] is None:
        return np.ones(T * h * w, bool), np.ones(h * w, bool)
    if mutant == 'rects_of_object0':
        o = 0
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    hi = (lambda a, b: a < b) if mutant == 'rect_exclusive' else (lambda a, b: a <= b)

    def inside(r):
        x0, x1, y0, y1 = (int(v) for v in r)
        return ((xx >= x0) & hi(xx, x1) & (yy >= y0) & hi(yy, y1)).ravel()

    mm = np.concatenate([inside(case['mem_rects'][o, t]) for t in range(T)])
    return mm, inside(case['qry_rects'][o])


def rect_kinds(h, w):
    """The rectangles every shape is read with: name -> (x0, x1, y0, y1)."""
    hw = h * w
    last = (w - 1, w - 1, h - 1, h - 1)
    return dict(full=(0, w - 1, 0, h - 1),
                beyond=(-2, w + 1, -1, h + 3),                           # sticks out on every side
                cell=(w // 2, w // 2, h // 2, h // 2),
                row=(0, w - 1, h // 2, h // 2),
                col=(w // 2, w // 2, 0, h - 1),
                empty=(1, 0, 1, 0),
                to63=(0, 63 % w, 0, 63 // w) if hw >= 64 else last,      # a box whose last cell is cell 63 (the last lane of query tile 0)
                from64=(64 % w, w - 1, 64 // w, h - 1) if hw > 64 else last,   # a box whose first cell is cell 64
                topleft=(-3, w // 2, -2, h // 2),                        # negative edges
                botright=(w // 2, w + 5, h // 2, h + 2))                 # edges >= w and >= h


KIND_NAMES = ('full', 'beyond', 'cell', 'row', 'col', 'empty', 'to63', 'from64', 'topleft', 'botright')


def rect_sets(no, T, h, w):
    """Ten rectangle sets [(tag, mem_rects [no, T, 4], qry_rects [no, 4], (memory kinds, query kinds))]: set s gives object o the
    query box s + o and frame t the memory box 3 s + 1 + o T + t (mod 10), so over the ten sets every kind is every object's query
    box and every frame's memory box once, and the boxes differ per frame and per object."""
    kinds = rect_kinds(h, w)
    sets = []
    for s in range(len(KIND_NAMES)):
        mk = [[KIND_NAMES[(3 * s + 1 + o * T + t) % 10] for t in range(T)] for o in range(no)]
        qk = [KIND_NAMES[(s + o) % 10] for o in range(no)]
        mr = np.array([[kinds[n] for n in row] for row in mk], np.int32).reshape(no, T, 4)
        qr = np.array([kinds[n] for n in qk], np.int32).reshape(no, 4)
        sets.append(('r%d' % s, mr, qr, (mk, qk)))
    return sets


# ================================================================================================ case builders
def _empty_case(name, family, shape, rects, tcap):
    no, De, Do, T, h, w = shape
    tcap = T if tcap is None else tcap
    assert tcap >= T and 1 <= De <= DE_MAX
    mr, qr = (None, None) if rects is None else rects
    return dict(name=name, family=family, no=no, De=De, Do=Do, T=T, Tcap=tcap, h=h, w=w, int_vals=False,
                m_key=np.zeros((no, De, tcap, h, w), F32), m_val=np.zeros((no, Do, tcap, h, w), F32),
                q_key=np.zeros((no, De, h, w), F32), q_val=np.zeros((no, Do, h, w), F32),
                mem_rects=None if mr is None else np.asarray(mr, np.int32).reshape(no, T, 4),
                qry_rects=None if qr is None else np.asarray(qr, np.int32).reshape(no, 4))


def _values(rng, shape, ints):
    if ints:
        return rng.randint(-8, 9, shape).astype(F32)
    sc = np.array([1e-2, 1.0, 1e2])[np.arange(shape[1]) % 3].reshape((1, -1) + (1,) * (len(shape) - 2))
    return (rng.randn(*shape) * sc).astype(F32)


def _rng(shape, seed, salt):
    no, De, Do, T, h, w = shape
    return np.random.RandomState((seed * 1000003 + salt * 7919 + no * 131 + De * 17 + Do * 29 + T * 31 + h * 37 + w) % (2 ** 31))


def onehot_g(De):
    g = 1
    while g * g < 512.0 * np.sqrt(De):
        g *= 2
    return g


def onehot_targets(case):
    """t(i) per object and query cell (-1: no target -- the query is masked or the object has no live memory cell).  The live
    queries take, in raster order: the first and the last live cell of the memory, the first and the last live cell of every frame's
    box, the first live cell of each residue j % 4; the rest are spread over the live cells by a fixed stride."""
    no, De, Do, T, h, w = dims(case)
    hw = h * w
    tg = np.full((no, hw), -1, np.int64)
    for o in range(no):
        mm, qm = live_masks(case, o)
        L = np.flatnonzero(mm)
        qi = np.flatnonzero(qm)
        if L.size == 0 or qi.size == 0:
            continue
        want = [L[0], L[-1]]
        for t in range(T):
            Lt = L[(L >= t * hw) & (L < (t + 1) * hw)]
            if Lt.size:
                want += [Lt[0], Lt[-1]]
        for r in range(4):
            Lr = L[L % 4 == r]
            if Lr.size:
                want.append(Lr[0])
        want = list(dict.fromkeys(int(j) for j in want))
        step = max(1, (2 * L.size) // 3) | 1
        for n, i in enumerate(qi):
            tg[o, i] = want[n] if n < len(want) else L[(n * step + o) % L.size]
    return tg


def onehot_case(name, shape, rects=None, tcap=None, seed=0):
    """Family (A).  Asserts its premises (module docstring): exact keys and queries, a float64 gap >= 256, a worst-case fp32 logit
    error <= 16, live targets.  Raises AssertionError for a shape that does not meet them."""
    no, De, Do, T, h, w = shape
    assert De >= 2
    case = _empty_case(name, 'onehot', shape, rects, tcap)
    rng = _rng(shape, seed, 1)
    hw, thw = h * w, T * h * w
    g = onehot_g(De)
    assert thw * thw * 3 < 2 ** 24, 'the integers 2 (j+1)(t+1) - (j+1)^2 must stay below 2^24'
    x = (g * (np.arange(case['Tcap'] * hw, dtype=np.float64) + 1.0))
    assert np.array_equal(x.astype(F32).astype(np.float64), x) and np.array_equal((x * x / 2).astype(F32).astype(np.float64)[:thw], (x * x / 2)[:thw])
    case['m_key'][:, 0] = x.astype(F32).reshape(case['Tcap'], h, w)
    case['m_key'][:, 1] = (-x * x / 2).astype(F32).reshape(case['Tcap'], h, w)
    for c in range(2, De):                                   # a zero on one side, anything on the other
        if c % 2:
            case['m_key'][:, c] = (rng.randn(no, case['Tcap'], h, w) * 3).astype(F32)
        else:
            case['q_key'][:, c] = (rng.randn(no, h, w) * 3).astype(F32)
    tg = onehot_targets(case)
    case['targets'] = tg
    qk0 = np.where(tg >= 0, x[np.maximum(tg, 0)], 0.0)
    case['q_key'][:, 0] = qk0.astype(F32).reshape(no, h, w)
    case['q_key'][:, 1] = (tg >= 0).astype(F32).reshape(no, h, w)
    case['m_val'][:] = _values(rng, case['m_val'].shape, False)
    case['m_val'][case['m_val'] == 0] = F32(0.5)             # (a zero value could not tell its cell from a skipped one)
    case['q_val'][:] = _values(rng, case['q_val'].shape, False)
    case['g'] = g
    prem = onehot_premises(case)
    assert prem['targets_live'] and prem['gap'] >= 256.0 and prem['logit_err'] <= 16.0 and prem['exact_dot'], (name, prem)
    return case


def _logits64(case, o):
    """(s [thw, hw], A = sum_c |k q| [thw, hw], memory mask, query mask) of one object in float64."""
    no, De, Do, T, h, w = dims(case)
    mm, qm = live_masks(case, o)
    k = np.where(mm, case['m_key'][o][:, :T].reshape(De, -1).astype(np.float64), 0.0)
    q = np.where(qm, case['q_key'][o].reshape(De, -1).astype(np.float64), 0.0)
    return k.T @ q / np.sqrt(float(De)), np.abs(k).T @ np.abs(q), mm, qm


def onehot_premises(case):
    """gap: the smallest margin of a target's float64 logit over any other cell's (a masked cell's 0 included); logit_err: the
    worst-case fp32 error of a logit by the bound's steps 1-2; targets_live; exact_dot: the dot products evaluated in float32 in
    channel order equal the float64 ones."""
    no, De, Do, T, h, w = dims(case)
    gap, err, live, exact = np.inf, 0.0, True, True
    for o in range(no):
        s, A, mm, qm = _logits64(case, o)
        tg = case['targets'][o]
        sel = np.flatnonzero(tg >= 0)
        live &= bool(mm[tg[sel]].all() and qm[sel].all())
        if sel.size == 0:
            continue
        err = max(err, float((gamma(De) * A / np.sqrt(float(De)) + 2 * U * np.abs(s))[:, sel].max()))
        st = s[tg[sel], sel]
        other = s[:, sel].copy()
        other[tg[sel], np.arange(sel.size)] = -np.inf
        if other.shape[0] > 1:
            gap = min(gap, float((st - other.max(axis=0)).min()))
        k32 = np.where(mm, case['m_key'][o][:, :T].reshape(De, -1), F32(0))
        q32 = np.where(qm, case['q_key'][o].reshape(De, -1), F32(0))
        dot = np.zeros(s.shape, F32)
        for c in range(De):
            dot = dot + k32[c][:, None] * q32[c][None, :]
        exact &= bool(np.array_equal(dot.astype(np.float64) / np.sqrt(float(De)), s))
    return dict(gap=gap, logit_err=err, targets_live=live, exact_dot=exact)


def equal_case(name, shape, rects=None, tcap=None, seed=0, variant='zero'):
    """Family (B): 'zero' -- zero keys, random queries, integer values; 'orth' -- keys in even channels, queries in odd ones, float
    values at three scales."""
    no, De, Do, T, h, w = shape
    case = _empty_case(name, 'equal', shape, rects, tcap)
    rng = _rng(shape, seed, 2)
    case['q_key'][:] = (rng.randn(no, De, h, w) * 2).astype(F32)
    if variant == 'orth':
        case['m_key'][:] = (rng.randn(*case['m_key'].shape) * 2).astype(F32)
        case['m_key'][:, 1::2] = 0
        case['q_key'][:, 0::2] = 0
    else:
        assert variant == 'zero'
    case['int_vals'] = variant == 'zero'
    case['m_val'][:] = _values(rng, case['m_val'].shape, case['int_vals'])
    case['q_val'][:] = _values(rng, case['q_val'].shape, False)
    case['variant'] = variant
    return case


def spread(case, o):
    """Largest logit range (max - min over all T h w cells, the masked cells' 0 included) per query of object o, float64."""
    s = _logits64(case, o)[0]
    return s.max(axis=0) - s.min(axis=0)


def random_case(name, shape, rects=None, tcap=None, seed=0):
    """Family (C).  Keys N(0, 1) times 1 or 1/4 by cell, queries N(0, 1); the keys are halved until every query's logit spread is
    <= 30 (decided in float64 on the CPU, so the device's arguments of expf stay inside [-34, 0] with room for their error)."""
    no, De, Do, T, h, w = shape
    case = _empty_case(name, 'random', shape, rects, tcap)
    rng = _rng(shape, seed, 3)
    sc = np.where(rng.rand(no, 1, case['Tcap'], h, w) < 0.5, 1.0, 0.25)
    case['m_key'][:] = (rng.randn(*case['m_key'].shape) * sc).astype(F32)
    case['q_key'][:] = rng.randn(no, De, h, w).astype(F32)
    case['m_val'][:] = _values(rng, case['m_val'].shape, False)
    case['q_val'][:] = _values(rng, case['q_val'].shape, False)
    while max(float(spread(case, o).max()) for o in range(no)) > 30.0:
        case['m_key'] *= F32(0.5)
    return case


def filled(case, how, seed=5):
    """The case with its masked cells rewritten: memory cells outside their box (keys and values), frames T .. Tcap - 1, and the
    q_key of the query cells outside the box.  how = 'zero' or 'garbage' (finite, some of it large).  q_val is never touched: its
    masked cells are part of the result (a zero of their sign).  The semantics ignore all of these cells."""
    no, De, Do, T, h, w = dims(case)
    rng = np.random.RandomState(seed + 11 * no + T)
    c = dict(case)
    mk, mv, qk = case['m_key'].copy(), case['m_val'].copy(), case['q_key'].copy()

    def junk(shape):
        if how == 'zero':
            return np.zeros(shape, F32)
        a = (rng.randn(*shape) * 7.7).astype(F32)
        a[rng.rand(*shape) < 0.05] = F32(-3.0e4)
        return a

    for o in range(no):
        mm, qm = live_masks(case, o)
        dead = ~mm.reshape(T, h, w)
        mk[o][:, :T][:, dead] = junk((De, int(dead.sum())))
        mv[o][:, :T][:, dead] = junk((Do, int(dead.sum())))
        mk[o][:, T:] = junk(mk[o][:, T:].shape)
        mv[o][:, T:] = junk(mv[o][:, T:].shape)
        qk[o][:, ~qm.reshape(h, w)] = junk((De, int((~qm).sum())))
    c.update(m_key=mk, m_val=mv, q_key=qk, fill=how)
    return c


# ================================================================================================ the references
def read_f64(case):
    """(out [no, 2 Do, h, w], p [no, T h w, h w]) in float64."""
    no, De, Do, T, h, w = dims(case)
    out = np.zeros((no, 2 * Do, h * w))
    p = np.zeros((no, T * h * w, h * w))
    for o in range(no):
        s, _, mm, qm = _logits64(case, o)
        e = np.exp(s - s.max(axis=0))
        p[o] = e / e.sum(axis=0)
        v = np.where(mm, case['m_val'][o][:, :T].reshape(Do, -1).astype(np.float64), 0.0)
        out[o, :Do] = v @ p[o]
        out[o, Do:] = case['q_val'][o].reshape(Do, -1) * qm
    return out.reshape(no, 2 * Do, h, w), p


def qval_half(case):
    """out[:, Do:] as float32 bits: q_val inside the query box, q_val * 0.0f outside."""
    no, De, Do, T, h, w = dims(case)
    qv = case['q_val'].reshape(no, Do, h * w)
    qm = np.stack([live_masks(case, o)[1] for o in range(no)])[:, None, :]
    return np.where(qm, qv, qv * F32(0)).reshape(no, Do, h, w)


def _flat(t, C, T, thw, wrong_stride):
    """[C, T h w] view of one object's [C, Tcap, h, w] tensor; wrong_stride: read with a channel stride of T h w."""
    if not wrong_stride:
        return t[:, :T].reshape(C, thw)
    flat = t.reshape(-1)
    return np.stack([flat[c * thw:(c + 1) * thw] for c in range(C)])


def read_f32(case, mutant=None):
    """(out, p) in float32 in the kernels' order (module docstring); ``mutant`` plants one fault of MUTANTS.  expf is the correctly
    rounded one (float64 exp, rounded), so the result does not depend on the host's libm."""
    assert mutant is None or mutant in MUTANTS
    no, De, Do, T, h, w = dims(case)
    hw, thw = h * w, T * h * w
    out = np.zeros((no, 2 * Do, hw), F32)
    p_all = np.zeros((no, thw, hw), F32)
    div = F32(De) if mutant == 'sqrt_is_De' else np.sqrt(F32(De))
    with np.errstate(all='ignore'):
        for o in range(no):
            mm, qm = live_masks(case, o, mutant)
            wrong = mutant == 'stride_thw'
            k = _flat(case['m_key'][o], De, T, thw, wrong)
            v = _flat(case['m_val'][o], Do, T, thw, wrong)
            q = np.where(qm, case['q_key'][o].reshape(De, hw), F32(0))
            dot = np.zeros((thw, hw), F32)
            for c in range(De):
                dot = dot + k[c][:, None] * q[c][None, :]
            dot[~mm] = F32(0)
            sc = dot / div
            if mutant == 'masked_neg_inf':
                sc[~mm] = -np.inf
            n = thw - thw % 4 if mutant == 'drop_tail' else thw
            p = np.zeros((thw, hw), F32)
            if n:
                mx = np.full(hw, -np.inf, F32)
                for jj in range(4):
                    if sc[jj:n:4].shape[0]:
                        mx = np.maximum(mx, sc[jj:n:4].max(axis=0))
                e = np.exp((sc[:n] - mx).astype(np.float64)).astype(F32)
                parts = [np.cumsum(e[jj::4], axis=0, dtype=F32)[-1] if e[jj::4].shape[0] else np.zeros(hw, F32) for jj in range(4)]
                tot = ((parts[0] + parts[1]) + parts[2]) + parts[3]
                p[:n] = e / tot
            live = np.flatnonzero(np.ones(thw, bool) if mutant == 'masked_value_added' else mm)
            if live.size:
                blk = max(1, (1 << 23) // (live.size * hw))
                for d0 in range(0, Do, blk):
                    prod = v[d0:d0 + blk][:, live, None] * p[None, live, :]
                    out[o, d0:min(d0 + blk, Do)] = np.cumsum(prod, axis=1, dtype=F32)[:, -1]
            qv = case['q_val'][o].reshape(Do, hw)
            out[o, Do:] = qv if mutant == 'qval_not_zeroed' else np.where(qm, qv, qv * F32(0))
            if mutant == 'drop_cell_64' and hw > 64:
                p[:, 64] = 0
                out[o, :, 64] = 0
            if mutant == 'drop_last_channel' and Do % 4:
                out[o, Do - 1] = 0
                out[o, 2 * Do - 1] = 0
            p_all[o] = p
    return out.reshape(no, 2 * Do, h, w), p_all


def bound(case, skip=None):
    """(out64, p64, bound_out [no, 2 Do, h, w], bound_p [no, T h w, h w]): the module docstring's derivation.  ``skip`` [no, h w]
    bool marks queries whose logits are outside the bound's premise (the one-hot queries, compared bit for bit instead): every other
    query's logit spread is asserted to be <= 34 here."""
    no, De, Do, T, h, w = dims(case)
    hw, thw = h * w, T * h * w
    out64, p64 = read_f64(case)
    bo = np.zeros((no, 2 * Do, hw))
    bp = np.zeros((no, thw, hw))
    L = -(-thw // 4)
    for o in range(no):
        s, A, mm, qm = _logits64(case, o)
        x = s - s.max(axis=0)
        checked = np.ones(hw, bool) if skip is None else ~skip[o]
        assert float(-x[:, checked].min(initial=0.0)) <= SPREAD_MAX, (case['name'], 'logit spread beyond expf\'s measured interval')
        ds = gamma(De) * A / np.sqrt(float(De)) + 2 * U * np.abs(s)
        r = ds + U * np.abs(x) + E_ULP * EPS
        p = p64[o]
        bp[o] = SLACK * (p * (r + (p * r).sum(axis=0) + gamma(L + 3) + U) + TINY)
        v = np.abs(np.where(mm, case['m_val'][o][:, :T].reshape(Do, -1).astype(np.float64), 0.0))
        bo[o, :Do] = SLACK * (gamma(int(mm.sum())) * (v @ p) + v @ bp[o])
    return out64, p64, bo.reshape(no, 2 * Do, h, w), bp


# ================================================================================================ what a result must be
def _is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def expectations(case):
    """Everything a result of the case is compared with:
      out64, p64, bound_out, bound_p                      (``bound``)
      out_bits [no, 2 Do, h, w] f32, out_exact bool       where out must be these 32 bits
      p_bits [no, T h w, h w] f32, p_exact [no, h w] bool the queries (columns of p) that must be these bits in every row
    Bit for bit: the q_val half everywhere; the one-hot queries (p and the read-out); p of every query whose logits are all 0 (masked,
    or an object without a live memory cell, or the 'equal' family); the read-out of such a query when it is 0 (no live cell) or when
    T h w is a power of two and the values are integers with sum |v| < 2^24."""
    no, De, Do, T, h, w = dims(case)
    hw, thw = h * w, T * h * w
    onehot = np.zeros((no, hw), bool)
    if case['family'] == 'onehot':
        onehot = case['targets'] >= 0
    out64, p64, bo, bp = bound(case, skip=onehot)
    out_bits = out64.astype(F32)
    out_exact = np.zeros((no, 2 * Do, hw), bool)
    p_bits = p64.astype(F32)
    p_exact = np.zeros((no, hw), bool)
    out_bits = out_bits.reshape(no, 2 * Do, hw)
    out_bits[:, Do:] = qval_half(case).reshape(no, Do, hw)
    out_exact[:, Do:] = True
    for o in range(no):
        mm, qm = live_masks(case, o)
        uniform = ~qm | (not mm.any()) | (case['family'] == 'equal')
        uniform &= ~onehot[o]
        p_exact[o] = uniform | onehot[o]
        p_bits[o][:, uniform] = F32(1.0) / F32(thw)
        v = np.where(mm, case['m_val'][o][:, :T].reshape(Do, -1), F32(0))
        if not mm.any():
            out_exact[o, :Do] = True
            out_bits[o, :Do] = F32(0)
        elif case['int_vals'] and _is_pow2(thw) and float(np.abs(v).sum(axis=1).max()) < 2.0 ** 24:
            out_exact[o, :Do] |= uniform[None, :]
        sel = np.flatnonzero(onehot[o])
        if sel.size:
            tg = case['targets'][o][sel]
            p_bits[o][:, sel] = 0
            p_bits[o][tg, sel] = 1
            out_bits[o, :Do][:, sel] = v[:, tg]
            out_exact[o, :Do][:, sel] = True
    return dict(out64=out64, p64=p64, bound_out=bo, bound_p=bp, out_bits=out_bits.reshape(no, 2 * Do, h, w),
                out_exact=out_exact.reshape(no, 2 * Do, h, w), p_bits=p_bits, p_exact=p_exact, onehot=onehot)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.view(np.uint32) == b.view(np.uint32)


def check(case, exp, out, p=None):
    """Compares EVERY element of out (and of p when given): bit for bit where ``expectations`` says so, inside the bound elsewhere
    (a NaN fails).  Returns dict(ok, why, ratio_out, ratio_p, bits_out, bits_p): the largest error / bound of the bounded elements
    and how many elements were compared bit for bit."""
    res = dict(ok=True, why='', ratio_out=0.0, ratio_p=0.0, bits_out=0, bits_p=0)

    def one(what, got, bits, exact, ref, bnd):
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
        bad = exact & ~same_bits(got, bits)
        err = np.abs(got.astype(np.float64) - ref)
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(exact, 0.0, np.where(err <= bnd, err / np.maximum(bnd, 1e-300), np.inf))
        ratio[~exact & ~(err <= bnd)] = np.inf                     # (NaN included)
        res['ratio_' + what] = float(ratio.max(initial=0.0))
        res['bits_' + what] = int(exact.sum())
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            res['ok'] = False
            res['why'] += '%s %s: %d of %d bit-exact elements differ, first at %s: got %r want %r; ' % (
                case['name'], what, int(bad.sum()), int(exact.sum()), i, got[i], bits[i])
        over = ~np.isfinite(ratio)
        if over.any():
            i = tuple(np.argwhere(over)[0])
            res['ok'] = False
            res['why'] += '%s %s: %d elements outside the bound, first at %s: got %r want %r bound %.3g; ' % (
                case['name'], what, int(over.sum()), i, got[i], ref[i], bnd[i])

    one('out', out, exp['out_bits'], exp['out_exact'], exp['out64'], exp['bound_out'])
    if p is not None:
        pe = np.broadcast_to(exp['p_exact'][:, None, :], exp['p64'].shape)
        one('p', p, exp['p_bits'], pe, exp['p64'], exp['bound_p'])
    return res
