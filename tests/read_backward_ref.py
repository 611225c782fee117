# -*- coding: utf-8 -*-
"""References and the error bound for the gradients of the memory read (rmnet_amd/csrc/memory_read_bwd.hip,
rmnet_memory_read_backward_f32).  No torch, no GPU: tests/test_memory_read_backward.py imports this on any machine.  The cases
are those of tests/generic_ref.py (onehot_case, equal_case, random_case, rect_sets); nothing there is changed.

Semantics, per object (M = T h w memory cells, N = h w queries; mm [M], qm [N] the 0/1 maps of the rectangles, both ends
inclusive, all ones in the dense form; Km = K mm, Vm = V mm, Qm = Q qm):
    S = Km^T Qm / sqrt(De)      P = soft-max of S over the M cells (a masked cell has logit 0)      R = Vm P
    mem_val = cat(R, q_val qm)
and with G = d mem_val[:Do], G2 = d mem_val[Do:]:
    d q_val = G2 qm       delta_n = sum_d G[d, n] R[d, n]       dP = Vm^T G       dS = P o (dP - delta)
    d V = (G P^T) mm      d K = (Qm dS^T / sqrt(De)) mm          d Q = (Km dS / sqrt(De)) qm

  grad_f64   the seven formulas in float64: what every comparison refers to.
  grad_f32   what the kernels do, in numpy float32 and in their order (below), with the masked cells handled analytically as the
             kernels handle them.  It carries the planted faults (MUTANTS).  fmaf is emulated through float64 (the product of two
             floats is exact there) and expf is the correctly rounded one, so it need not match the device bit for bit.
  bound      a per-element bound on |device - grad_f64| for each of the four gradients.

The kernels' order, per object, over the Ml live memory cells and the Nl live queries (raster order), c = M - Ml masked cells:
  1. dot_mn = fmaf chain over the channels c = 0 .. De-1 of k_cm q_cn                                        (De roundings)
  2. s_mn = dot_mn / fl(sqrt(De))                                                    (sqrtf once on the host, one division)
  3. mx_n = max_m s_mn, and max(mx_n, 0) when c > 0                                                                 (exact)
  4. e_mn = expf(s_mn - mx_n); sum_n = the e_mn of eight contiguous ranges of the memory tiles (32 cells each), every range added
     in four interleaved sequences of 8 terms per tile and merged by two additions; the eight ranges added in order; + c *
     expf(-mx_n) when c > 0                                          (<= L + 11 roundings, L = 8 ceil(ceil(Ml / 32) / 8))
  5. P_mn = e_mn / sum_n                                                                                     (one division)
  6. delta_n = four strided fmaf chains over d of G_dn R_dn, merged by three additions              (ceil(Do/4) + 3 roundings)
  7. dP_mn = fmaf chain over d = 0 .. Do-1 of v_dm G_dn                                                       (Do roundings)
  8. dS_mn = P_mn * (dP_mn - delta_n)                                                                      (two roundings)
  9. dV_dm = fmaf chain over the live queries of G_dn P_mn, + rank_d                                      (Nl + 1 roundings)
     rank_d = (sum over the masked queries of G_dn) / M: 64 strided sequences, a six-level butterfly, one division
 10. dK_cm = (fmaf chain over the live queries of q_cn dS_mn) / fl(sqrt(De))                              (Nl + 2 roundings)
 11. dQ_cn = (fmaf chains over up to eight contiguous ranges of the live memory cells of k_cm dS_mn, added in order)
             / fl(sqrt(De))                                                                         (<= Ml + 8 + 2 roundings)
 12. d q_val = G2 inside the query box, 0 outside; every masked cell of dK, dV, dQ is 0                             (exact)
Zero padding (De to 4 or 16, Do to 64, the tiles to 32) adds fmaf(0, x, acc) = acc: no rounding.

The bound (u = 2^-24, eps = 2^-23, gamma_n = n u / (1 - n u), E = glue_ref.E_ULP: twice the measured error of the device's expf
on [-34, 0]; first order; times SLACK = 1 + 1e-3; TINY = 2^-125 for a result below the normal range):
  1-2.  |s^ - s| <= ds := gamma_De A / sqrt(De) + 2 u |s|,  A_mn = sum_c |k_cm q_cn|
  3-4.  soft-max is shift invariant: take the device's own mx^ as the shift in the reference too.  x^ = fl(s^ - mx^) is off by
        <= ds + u |x|, so e^ = e (1 + t), |t| <= r := ds + u |x| + E eps; the masked cells' term c expf(-mx^) has t <= r0 := E eps + u.
        All terms positive: sum^ = sum (1 + sum_j p_j t_j) (1 + g), |g| <= gamma_{L+11}, L = 8 ceil(ceil(Ml / 32) / 8).
        Valid while x >= -34 (``bound`` asserts it unless told the case is a CPU-only extreme one, where expf is the exact one and
        an e below the normal range is within TINY of the truth).
  5.    |P^ - P| <= dPr := P (r + rbar + gamma_{L+11} + u) + TINY,  rbar_n = sum_m P_mn r_mn + (c e0 / sum) r0
  6.    |delta^ - delta| <= ddl := gamma_{ceil(Do/4)+3} sum_d |G R^| + sum_d |G| |R^ - R|   (R^ = the mem_val handed to the call: its
        own error is measured against R in float64, not assumed)
  7.    |dP^ - dP| <= ddP := gamma_Do sum_d |v G|
  8.    t = dP - delta: |t^ - t| <= ddP + ddl + u |t|;  |dS^ - dS| <= ddS := dPr |t| + P (ddP + ddl + u |t|) + u |dS|
  9.    |dV^ - dV| <= gamma_Nl sum_n |G| P + sum_n |G| dPr + gamma_{ceil(N/64)+7} sum_{n masked} |G| / M + u |dV|
 10.    |dK^ - dK| <= (gamma_Nl sum_n |q dS| + sum_n |q| ddS) / sqrt(De) + 2 u |dK|
 11.    |dQ^ - dQ| <= (gamma_{Ml+8} sum_m |k dS| + sum_m |k| ddS) / sqrt(De) + 2 u |dQ|
 12.    0
Every term is a constant times a float64 sum of absolute values of the element's own chain; no constant comes from what the
kernels return.

Bit for bit (``exact_expectations``): with integer V and G of small magnitude every chain of steps 6, 7, 9 is a sum of integers
below 2^24, and
  M = 1       P = 1: dS = 1 * (dP - delta) = 0 exactly (both are the same integer), dK = dQ = 0, dV = G (+ rank)
  equal       every logit 0, M a power of two: P = 2^-k exactly, dV = 2^-k (integer sums); dS = 2^-k (integer - delta) with delta
              = sum_d G R, R = 2^-k (integer): exact; K = 0 gives dQ = 0 and dK = (sum_n q dS) / sqrt(De), compared inside the bound
  one-hot     P is exactly 1 at the target and 0 elsewhere (generic_ref's premise), dP_tn - delta_n = 0: dK = dQ = 0 and dV lands on
              the target cells only, as integer sums
so dV and d q_val (and dK, dQ where they are 0) are compared bit for bit there."""

import numpy as np

import generic_ref as G

F32 = np.float32
U, EPS, E_ULP, SLACK, TINY = G.U, G.EPS, G.E_ULP, G.SLACK, G.TINY
SPREAD_MAX = G.SPREAD_MAX
gamma = G.gamma
TILE = 32                          # memory_read_bwd.hip kBM = kBN

MUTANTS = ('no_delta', 'dk_no_scale', 'no_rank1', 'masked_not_in_denominator', 'max_live_only', 'dk_not_masked', 'dqv_not_masked',
           'drop_last_query_tile', 'drop_last_cell', 'tcap_for_t', 'rect_exclusive')
# 'max_live_only': the maximum is taken over the live cells and the masked cells are counted as c * exp(0), without the shift --
# right only while the live maximum is 0.  (Shifting their term too, c * exp(-max), is the same soft-max whatever the shift: with
# live logits near -200 it overflows to inf and gives P = 0 where the true P is below 1e-86, which no comparison of values can see.)
NAMES = ('d_m_key', 'd_m_val', 'd_q_key', 'd_q_val')


def grad_out_for(case, seed=0, ints=False):
    """A gradient [no, 2 Do, h, w] f32 to send back: integers in [-4, 4] or floats at two scales by channel."""
    no, De, Do, T, h, w = G.dims(case)
    rng = np.random.RandomState(977 * seed + 13 * no + De + 3 * Do + 7 * T + h * w)
    if ints:
        return rng.randint(-4, 5, (no, 2 * Do, h, w)).astype(F32)
    sc = np.array([1.0, 30.0])[np.arange(2 * Do) % 2].reshape(1, -1, 1, 1)
    return (rng.randn(no, 2 * Do, h, w) * sc).astype(F32)


def with_int_values(case):
    """The case with integer values in [-8, 8] (no zero: a zero could not tell its cell from a skipped one)."""
    c = dict(case)
    rng = np.random.RandomState(4243 + case['m_val'].size)
    v = rng.randint(1, 9, case['m_val'].shape) * rng.choice([-1, 1], case['m_val'].shape)
    c['m_val'] = v.astype(F32)
    c['int_vals'] = True
    return c


def _obj64(case, o, mutant=None):
    no, De, Do, T, h, w = G.dims(case)
    mm, qm = G.live_masks(case, o, 'rect_exclusive' if mutant == 'rect_exclusive' else None)
    k = np.where(mm, case['m_key'][o][:, :T].reshape(De, -1).astype(np.float64), 0.0)
    v = np.where(mm, case['m_val'][o][:, :T].reshape(Do, -1).astype(np.float64), 0.0)
    q = np.where(qm, case['q_key'][o].reshape(De, -1).astype(np.float64), 0.0)
    return k, v, q, mm, qm


def _empty_grads(case, dtype):
    no, De, Do, T, h, w = G.dims(case)
    tc = case['Tcap']
    return dict(d_m_key=np.zeros((no, De, tc, h, w), dtype), d_m_val=np.zeros((no, Do, tc, h, w), dtype),
                d_q_key=np.zeros((no, De, h, w), dtype), d_q_val=np.zeros((no, Do, h, w), dtype))


def grad_f64(case, grad_out):
    """The four gradients in float64 (frames >= T of d_m_key / d_m_val are 0)."""
    no, De, Do, T, h, w = G.dims(case)
    hw = h * w
    out = _empty_grads(case, np.float64)
    for o in range(no):
        k, v, q, mm, qm = _obj64(case, o)
        s = k.T @ q / np.sqrt(float(De))
        e = np.exp(s - s.max(axis=0))
        p = e / e.sum(axis=0)
        g = grad_out[o, :Do].reshape(Do, hw).astype(np.float64)
        g2 = grad_out[o, Do:].reshape(Do, hw).astype(np.float64)
        r = v @ p
        delta = (g * r).sum(axis=0)
        dp = v.T @ g
        ds = p * (dp - delta)
        out['d_m_val'][o][:, :T] = ((g @ p.T) * mm).reshape(Do, T, h, w)
        out['d_m_key'][o][:, :T] = ((q @ ds.T) / np.sqrt(float(De)) * mm).reshape(De, T, h, w)
        out['d_q_key'][o] = ((k @ ds) / np.sqrt(float(De)) * qm).reshape(De, h, w)
        out['d_q_val'][o] = (g2 * qm).reshape(Do, h, w)
    return out


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _chain(a, b):
    """sum_k a[i, k] b[j, k] as a k-ordered fmaf chain -> [i, j] float32."""
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k in range(a.shape[1]):
        acc = _fma(a[:, k][:, None], b[:, k][None, :], acc)
    return acc


def grad_f32(case, grad_out, mem_val=None, mutant=None):
    """The four gradients in float32 in the kernels' order; ``mem_val`` defaults to the float64 read rounded to float32."""
    assert mutant is None or mutant in MUTANTS
    no, De, Do, T, h, w = G.dims(case)
    hw, thw = h * w, T * h * w
    if mem_val is None:
        mem_val = G.read_f64(case)[0].astype(F32)
    out = _empty_grads(case, F32)
    rt = np.sqrt(F32(De))
    with np.errstate(all='ignore'):
        for o in range(no):
            mm, qm = G.live_masks(case, o, 'rect_exclusive' if mutant == 'rect_exclusive' else None)
            L, Q = np.flatnonzero(mm), np.flatnonzero(qm)
            m_tot = case['Tcap'] * hw if mutant == 'tcap_for_t' else thw
            c_masked = m_tot - L.size
            k = case['m_key'][o][:, :T].reshape(De, thw)[:, L]
            v = case['m_val'][o][:, :T].reshape(Do, thw)[:, L]
            q = case['q_key'][o].reshape(De, hw)[:, Q]
            g_all = grad_out[o, :Do].reshape(Do, hw)
            g = g_all[:, Q]
            r = mem_val[o, :Do].reshape(Do, hw)[:, Q]
            g2 = grad_out[o, Do:].reshape(Do, hw)
            out['d_q_val'][o] = (g2 if mutant == 'dqv_not_masked' else np.where(qm, g2, F32(0))).reshape(Do, h, w)
            dv = np.zeros((Do, thw), F32)
            dk = np.zeros((De, thw), F32)
            dq = np.zeros((De, hw), F32)
            rank = np.zeros(Do, F32)
            if (~qm).any() and mutant != 'no_rank1':
                rank = np.cumsum(g_all[:, ~qm], axis=1, dtype=F32)[:, -1] / F32(m_tot)
            if L.size and Q.size:
                s = _chain(k.T, q.T) / rt                                            # [Ml, Nl]
                mx = s.max(axis=0)
                if c_masked > 0 and mutant != 'max_live_only':
                    mx = np.maximum(mx, F32(0))
                e = np.exp((s - mx).astype(np.float64)).astype(F32)
                tot = np.cumsum(e, axis=0, dtype=F32)[-1]
                e0 = np.exp(-mx.astype(np.float64)).astype(F32)
                if mutant == 'max_live_only':
                    e0 = np.ones_like(e0)                                            # (see MUTANTS below the imports)
                if c_masked > 0 and mutant != 'masked_not_in_denominator':
                    tot = tot + F32(c_masked) * e0
                p = e / tot
                delta = np.zeros(Q.size, F32)
                for d in range(Do):
                    delta = _fma(g[d], r[d], delta)
                dp = _chain(v.T, g.T)
                ds = p * dp if mutant == 'no_delta' else p * (dp - delta)
                nq = Q.size - ((Q.size - 1) % TILE + 1) if mutant == 'drop_last_query_tile' else Q.size
                nm = L.size - 1 if mutant == 'drop_last_cell' else L.size
                dv[:, L[:nm]] = _chain(g[:, :nq], p[:nm, :nq]) + rank[:, None]
                dkl = _chain(q[:, :nq], ds[:nm, :nq])
                dk[:, L[:nm]] = dkl if mutant == 'dk_no_scale' else dkl / rt
                dq[:, Q[:nq]] = _chain(k[:, :nm], ds[:nm, :nq].T) / rt
                if mutant == 'dk_not_masked' and c_masked > 0:
                    ds0 = (e0 / tot) * (F32(0) - delta)                              # a masked cell's row of dS
                    dk[:, np.flatnonzero(~mm)] = ((q * ds0[None, :]).sum(axis=1) / rt)[:, None]
            elif L.size:
                dv[:, L] = rank[:, None]
            out['d_m_val'][o][:, :T] = dv.reshape(Do, T, h, w)
            out['d_m_key'][o][:, :T] = dk.reshape(De, T, h, w)
            out['d_q_key'][o] = dq.reshape(De, h, w)
    return out


def bound(case, grad_out, mem_val=None, extreme=False):
    """(grad64, bounds): dicts of the four gradients in float64 and of the per-element bounds on |device - grad64| (module
    docstring).  ``mem_val``: the forward output handed to the call (default: the float64 read rounded to float32)."""
    no, De, Do, T, h, w = G.dims(case)
    hw = h * w
    ref = grad_f64(case, grad_out)
    read64 = G.read_f64(case)[0]
    if mem_val is None:
        mem_val = read64.astype(F32)
    bnd = _empty_grads(case, np.float64)
    rt = np.sqrt(float(De))
    for o in range(no):
        k, v, q, mm, qm = _obj64(case, o)
        ml, nl, c = int(mm.sum()), int(qm.sum()), int((~mm).sum())
        g = grad_out[o, :Do].reshape(Do, hw).astype(np.float64)
        s = k.T @ q / rt
        A = np.abs(k).T @ np.abs(q)
        mx = s.max(axis=0)                                   # (masked cells' logit 0 is among the s)
        x = s - mx
        if not extreme:
            assert float(-x[:, qm].min(initial=0.0)) <= SPREAD_MAX, (case['name'], 'logit spread beyond expf\'s measured interval')
        e = np.exp(x)
        tot = e.sum(axis=0)
        p = e / tot
        ds_ = gamma(De) * A / rt + 2 * U * np.abs(s)
        r = np.where(mm[:, None], ds_ + U * np.abs(x) + E_ULP * EPS, E_ULP * EPS + U)          # masked rows: r0
        L = 8 * -(-(-(-ml // TILE)) // 8)
        rbar = (p * r).sum(axis=0)
        dpr = p * (r + rbar + gamma(L + 11) + U) + TINY
        r64 = read64[o, :Do].reshape(Do, hw)
        rhat = mem_val[o, :Do].reshape(Do, hw).astype(np.float64)
        ddl = gamma(-(-Do // 4) + 3) * (np.abs(g) * np.abs(rhat)).sum(axis=0) + (np.abs(g) * np.abs(rhat - r64)).sum(axis=0)
        delta = (g * r64).sum(axis=0)
        dp = v.T @ g
        ddp = gamma(Do) * (np.abs(v).T @ np.abs(g))
        t = dp - delta
        dS = p * t
        dds = dpr * np.abs(t) + p * (ddp + ddl + U * np.abs(t)) + U * np.abs(dS)
        live = mm[:, None] & qm[None, :]
        dds = np.where(live, dds, 0.0)
        dS = np.where(live, dS, 0.0)
        gl = np.where(qm, np.abs(g), 0.0)                    # |G| over the live queries
        gm = np.where(qm, 0.0, np.abs(g))                    # ... over the masked ones
        bv = gamma(nl) * (gl @ p.T) + gl @ np.where(live, dpr, 0.0).T + gamma(-(-hw // 64) + 7) * gm.sum(axis=1)[:, None] / (T * hw) \
            + U * np.abs(ref['d_m_val'][o][:, :T].reshape(Do, -1))
        bk = (gamma(nl) * (np.abs(q) @ np.abs(dS).T) + np.abs(q) @ dds.T) / rt + 2 * U * np.abs(ref['d_m_key'][o][:, :T].reshape(De, -1))
        bq = (gamma(ml + 8) * (np.abs(k) @ np.abs(dS)) + np.abs(k) @ dds) / rt + 2 * U * np.abs(ref['d_q_key'][o].reshape(De, -1))
        bnd['d_m_val'][o][:, :T] = (SLACK * bv * mm).reshape(Do, T, h, w)
        bnd['d_m_key'][o][:, :T] = (SLACK * bk * mm).reshape(De, T, h, w)
        bnd['d_q_key'][o] = (SLACK * bq * qm).reshape(De, h, w)
    return ref, bnd


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.view(np.uint32) == b.view(np.uint32)


def exact_expectations(case, grad_out):
    """{name: (bits float32, mask)}: the elements that must come back bit for bit (module docstring), for a case of an exact
    family with integer values and an integer gradient.  Everything outside a rectangle, frames >= T and d q_val are always exact."""
    no, De, Do, T, h, w = G.dims(case)
    hw, thw = h * w, T * h * w
    ref = grad_f64(case, grad_out)
    exp = {n: (ref[n].astype(F32) + F32(0), np.zeros(ref[n].shape, bool)) for n in NAMES}      # (+ 0: a zero is +0, also one rounded from -1e-200)
    exp['d_q_val'][1][:] = True
    ints = bool(case.get('int_vals')) and bool(np.array_equal(grad_out, np.round(grad_out)))
    for o in range(no):
        mm, qm = G.live_masks(case, o)
        dead = ~mm.reshape(T, h, w)
        for n in ('d_m_key', 'd_m_val'):
            exp[n][1][o][:, :T][:, dead] = True
            exp[n][1][o][:, T:] = True
        exp['d_q_key'][1][o][:, ~qm.reshape(h, w)] = True
        if not mm.any():
            exp['d_q_key'][1][o][:] = True
            continue
        if not ints:
            continue
        fam = case['family']
        pow2 = G._is_pow2(thw)
        if thw == 1 or fam == 'onehot':
            # (one-hot: queries without a live target do not exist -- every live query has one; masked queries add the rank-one
            #  term, an integer sum over M, exact only when M is a power of two)
            if fam == 'onehot' and not (qm.all() or pow2):
                continue
            for n in NAMES:
                exp[n][1][o][:] = True
        elif fam == 'equal' and pow2:
            exp['d_m_val'][1][o][:] = True
            if case.get('variant') == 'zero':
                exp['d_q_key'][1][o][:] = True
    return ref, exp


def check(case, grad_out, got, mem_val=None, exact=None, extreme=False, names=NAMES):
    """Compares EVERY element of the gradients in ``got`` ({name: float32 array}): bit for bit where ``exact`` (from
    exact_expectations) says so, inside the bound elsewhere (a NaN fails).  Returns dict(ok, why, ratio={name: largest error /
    bound}, bits={name: elements compared bit for bit})."""
    ref, bnd = bound(case, grad_out, mem_val, extreme)
    res = dict(ok=True, why='', ratio={}, bits={})
    for n in names:
        a = np.asarray(got[n])
        assert a.dtype == np.float32 and a.shape == ref[n].shape, (n, a.dtype, a.shape, ref[n].shape)
        ex = np.zeros(a.shape, bool) if exact is None else exact[n][1]
        if exact is not None:
            bad = ex & ~same_bits(a, exact[n][0])
            if bad.any():
                i = tuple(np.argwhere(bad)[0])
                res['ok'] = False
                res['why'] += '%s %s: %d of %d bit-exact elements differ, first at %s: got %r want %r; ' % (
                    case['name'], n, int(bad.sum()), int(ex.sum()), i, a[i], exact[n][0][i])
        err = np.abs(a.astype(np.float64) - ref[n])
        inside = err <= bnd[n]                                                   # (False for a NaN)
        over = ~ex & ~inside
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(ex | (bnd[n] == 0), 0.0, err / np.maximum(bnd[n], 1e-300))
        res['ratio'][n] = float(np.nanmax(ratio, initial=0.0)) if not over.any() else float('inf')
        res['bits'][n] = int(ex.sum())
        if over.any():
            i = tuple(np.argwhere(over)[0])
            res['ok'] = False
            res['why'] += '%s %s: %d elements outside the bound, first at %s: got %r want %r bound %.3g; ' % (
                case['name'], n, int(over.sum()), i, a[i], ref[n][i], bnd[n][i])
    return res
