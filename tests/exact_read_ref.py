# -*- coding: utf-8 -*-
"""Plan, references, error bound and case families for the EXACT-FP32 memory read: mr_main and mr_combine of
rmnet_amd/csrc/memory_read.hip, selected by RMNET_MR_EXACT_FP32, at De = 128, Do = 512.  numpy only (no torch, no GPU):
tests/test_memory_read_exact.py imports this on any machine.  The semantics, the rectangles and the 'equal' / 'random' builders are
those of tests/generic_ref.py (a masked memory cell has logit 0 and value 0, out = cat(V p, q_val x box)).

  plan_of    the launch plan restated: slots_for, mr_slots, bank_plan, the clamped areas, comb_channels, the workspace layout.
  read_f64   generic_ref.read_f64 (float64 semantics): what every comparison refers to.
  read_f32   what the two kernels do, in numpy float32, in their order (below), with the planted faults (MUTANTS).  Not bit for bit
             the device on general inputs (MFMA accumulation order, FMA contraction).
  bound      a per-element bound on |device - read_f64| for out[:, :512] from the roundings counted below.

The kernels' order, per object.  Rectangles are CLAMPED to the grid; frame t contributes area_t cells in raster order of its box,
prefix sums over chunks of 64 frames with a carry give the compacted index n -> (t, cy, cx) by binary search.  Compacted cells are
walked in tiles of 32, the njt = ceil(M / 32) tiles are cut into nsplit splits [s njt / nsplit, (s + 1) njt / nsplit).  Per split
and query i (the Mq compacted query cells and, when Mq < h w, one zero-key MEAN SLOT at compacted position Mq):
  1. s_j = dot_j / fl(sqrt(128)), dot_j by 32 MFMA steps of 4 channels in fp32; cells n >= M of the last tile: -inf
  2. tmax = max of the tile; if tmax > mref + kDefer (kDefer = 30; mref = -inf before the first tile): alpha = __expf(mref - tmax),
     mref = tmax; else alpha = 1                                            (the DEFERRED reference: x = s - mref may be up to +30)
  3. p_j = expf(fl(s_j - mref));  lsum = lsum * alpha + (sum of the tile's 32 p);  acc_d = acc_d * alpha + sum_j v_dj p_j (MFMA)
  4. the partial (acc, mref, lsum) of the split goes to the workspace.
  mr_combine, per query:  mtot = max_s mref_s, raised to 0 when N_out = T h w - M > 0;  w_s = expf(fl(mref_s - mtot));
  5. l = sum_s lsum_s w_s (four interleaved groups, then three additions) + N_out expf(-mtot);   inv = 1 / l
  6. out_d = (sum_s w_s acc_ds) * inv.   The mean slot: W_s = w_s / l, mean_d = sum_s W_s acc_ds (interleaved groups).
  7. write-out: a query cell gets its out_d, every masked query cell the mean vector; out[512 + d] = q_val inside the box and
     q_val * 0.0f outside (exact).

The bound (u = 2^-24, eps = 2^-23, gamma_n = n u / (1 - n u)), first order, times SLACK, plus TINY.  The soft-max does not change
when one constant is taken from every logit, so the reference takes the device's own fp32 references.  ``bound`` walks the tiles in
float64 to know, per query and split, where the reference is raised (it asserts that no decision tmax > mref + 30 is closer than
MARGIN to its threshold, so that the device decides alike) and hence every argument x_j of expf and how many rescales nb_j follow
cell j inside its split.  With A_j = sum_c |k_cj q_ci|:
  1.   |s^_j - s_j| <= gamma_128 A_j / sqrt(128) + 2 u |s_j| =: ds_j                 (dot product in any order; sqrtf and division)
  2-3. p^_j = e^(s_j - mref) (1 + t_j), |t_j| <= ds_j + u |x_j| + E eps, E = 2 E_MEASURED_WIDE ulps of expf, measured on
       [-64, 32] (tools/ubench/math_ulp.hip, profiles/r31_a_exact_read_tests.md): ``bound`` asserts -64 <= x_j <= 30 + MARGIN.
       Each rescale multiplies the earlier mass by alpha^ = alpha (1 + a), |a| <= A_REL + u |arg| + u (the argument's rounding and
       the product's): nb_j r_a with r_a = A_REL + u 64 + u.  A_REL = 2^-16 is four times the largest relative error of __expf
       measured on [-160, -30]; the tests assert that this term is below 1 % of every bound (A_REL is immaterial).
  5-6. w_s = expf(fl(mref_s - mtot)) carries u |mref_s - mtot| + E eps; N_out expf(-mtot): E eps + 2 u.
  p^_j, alpha^ and w^_s enter the numerator sum_j v_dj p_j and the denominator alike, so to first order their errors c_j =
  t_j + nb_j r_a + u |mref_s - mtot| + E eps move out_d by sum_j (v_dj - out_d) p_j c_j (and the closed-form term's by out_d p_out
  (E eps + 2 u), its value being 0).  The roundings of the two sums themselves are not shared:
       numerator    cell j's term passes the additions of acc from its MFMA to the end of its split, rem_j <= (cells left) + 4, and
                    nb_j products; then the merge (nsplit products and additions, gamma_{2 nsplit + 1}) and the product with inv (u);
       denominator  lsum: a chain of at most nt + 10 + nb additions and products (nt tiles of the longest split, 7 + 2 + 1 inside a
                    tile), the merge gamma_{nsplit + 5}, and 1 / l (u): one division and one product, the generic path has one division.
                    The mean slot divides per split and multiplies: the same count.
  With p_j the float64 soft-max:
       |out^_d - out_d| <= sum_j |v_dj - out_d| p_j c_j + |out_d| p_out (E eps + 2 u) + sum_j |v_dj| p_j (gamma_{rem_j} + nb_j u)
                           + (sum_j |v_dj| p_j) (gamma_{2 nsplit + 1} + u) + |out_d| (gamma_{nt + 10 + nb} + gamma_{nsplit + 5} + u)
  TINY = 2^-125 covers results below fp32's normal range.  No constant here comes from what the kernels return.

Case families:
  'onehot'  per object at most 128 candidate memory cells; candidate c holds the key G e_c (G = 64, e_c the unit vector of channel
            c), every other live cell a zero key; a live query with target c holds G e_c.  Every product is 0 or G^2 = 4096, so the
            target's logit is fl(4096 / fl(sqrt(128))), about 362, and every other logit -- masked cells included -- is exactly 0, in
            any order of the dot product.  expf(0) = 1 and expf(x) = 0 for x <= -200 on this build (profiles/r14_a_glue_tests.md),
            so out[:, :512] is the target's value vector BIT FOR BIT for random float values, whichever tile or split holds the
            target: its tile raises the reference (alpha = __expf(-362) = 0 wipes the tiles before it, or the accumulators are still
            0), p = expf(0) = 1 at the target and expf(-362) = 0 elsewhere, lsum = 1; later tiles add v * 0; splits without the target
            get the merge weight expf(0 - 362) = 0, the closed-form term is N_out expf(-362) = 0, l = 1, inv = 1.  Candidates sit at
            the first and last cell of a tile, the first and last tile of a split, the first and last split (and splits 15..17),
            the last compacted cell and the first cell of a box that follows empty boxes.  Masked query cells get the mean vector
            (inside the bound).
  'equal'   generic_ref.equal_case ('zero', 'orth'): every logit 0.  Integer values with sum |v| < 2^24 and T h w a power of two:
            every read-out element bit for bit (masked query cells and an object with M = 0 included); inside the bound otherwise.
  'random'  generic_ref.random_case: logit spread <= 30, no rescale after a split's first tile.
  'spike'   a random case with base spread <= 8 and rises planted through channel 0 (queries hold 1 there, spike cells
            rise * sqrt(128)): +20 (no rescale, expf at positive arguments), +45 after the first tile of a split (rescale), +45 in a
            later split only.
"""

import numpy as np

import generic_ref as G

F32 = np.float32
U, EPS = G.U, G.EPS
SLACK, TINY = G.SLACK, G.TINY
gamma = G.gamma
DE, DO = 128, 512
KQT, KJT = 64, 32
KDEFER = 30.0
SPLIT_TARGET, SPLIT_MAX, SPLIT_MIN_TILES = 256, 64, 4
PLAN_INTS = 12
BANK_MAX_OBJ = 64
ML_REG_SPLITS = 16                  # kMl = 4 times 4 thread groups: the splits mr_combine holds in registers
PREFIX_CHUNK = 64
MR_EXACT_FP32 = 2
ONEHOT_G = 64.0

E_MEASURED_WIDE = 0.840             # ulps, expf on [-64, 32] (profiles/r31_a_exact_read_tests.md)
E_WIDE = 2.0 * E_MEASURED_WIDE
A_MEASURED = 3.853e-6               # relative error of __expf on [-160, -30] (same file)
A_REL = 2.0 ** -16
X_LO, X_HI, MARGIN = -64.0, KDEFER, 1e-2

MUTANTS = ('acc_not_rescaled', 'lsum_not_rescaled', 'nout_dropped_query', 'nout_dropped_mean', 'nout_unclamped', 'ref_not_raised',
           'splits_ge16_ignored', 'uneven_last_tile_dropped', 'tail_logit_zero', 'prefix_carry_dropped', 'rects_unclamped',
           'mean_slot_tile0', 'between_columns_neighbour', 'fill_skipped_mq0', 'qval_not_zeroed', 'rects_of_object0', 'stride_thw',
           'sqrt_is_De')
VACUITY = ('expf_16ulp', 'merge_weight_2m18')


def dims(case):
    return case['no'], case['T'], case['h'], case['w']


# ================================================================================================ the plan
def slots_for(no, hw):
    nqt_max = (hw + 1 + KQT - 1) // KQT
    per_obj = (SPLIT_TARGET + no - 1) // no
    return max(nqt_max, per_obj)


def bank_total_slots(no, hw):
    nq = (hw + 63) // 64
    group0 = lambda obj0: (obj0 // BANK_MAX_OBJ) * (SPLIT_TARGET + BANK_MAX_OBJ * nq)
    rem = no % BANK_MAX_OBJ
    return group0(no - rem) + (SPLIT_TARGET + rem * nq if rem else 0)


def mr_slots(no, hw):
    return max(no * slots_for(no, hw), bank_total_slots(no, hw))


def bank_plan(Mq, hw, njt, no, slots):
    nqt = max(1, (Mq + (1 if Mq < hw else 0) + 63) // 64)
    ns = min(SPLIT_TARGET // (nqt * no), slots // nqt, SPLIT_MAX, njt // SPLIT_MIN_TILES)
    ns = min(max(ns, 1), njt)
    return nqt, ns


def comb_channels(no):
    return 16 if no <= 2 else 32


def align256(x):
    return (x + 255) // 256 * 256


def workspace_layout(no, hw):
    """Byte offsets (partial area, (m, l) area, plan records) and the total of the EXACT_FP32 workspace."""
    slots = mr_slots(no, hw)
    ml = align256(slots * DO * KQT * 4)
    plan = ml + align256(slots * 2 * KQT * 4)
    return dict(partials=0, ml=ml, plan=plan, total=plan + align256(no * PLAN_INTS * 4), slots=slots)


def clamp_rect(r, h, w):
    return max(int(r[0]), 0), min(int(r[1]), w - 1), max(int(r[2]), 0), min(int(r[3]), h - 1)


def rect_area(r):
    return max(r[1] - r[0] + 1, 0) * max(r[3] - r[2] + 1, 0)


def xcd_remap(b, n):
    q, r, x = n >> 3, n & 7, b & 7
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (b >> 3)


def plan_of(case, aligned=True):
    """Per object: Mq, nqt, M, njt, nsplit, the split boundaries in tiles, the clamped query box, the mean slot (exists, tile, lane,
    alone in its tile), n_out, the rows the fill blocks write, the plan record; per call: slots, copy blocks or inline q_val, the
    combine width, the prefix chunks, the workspace layout."""
    no, T, h, w = dims(case)
    hw = h * w
    regional = case['mem_rects'] is not None
    slots = slots_for(no, hw)
    objs = []
    for o in range(no):
        if regional:
            areas = [rect_area(clamp_rect(case['mem_rects'][o, t], h, w)) for t in range(T)]
            qr = clamp_rect(case['qry_rects'][o], h, w)
            Mq = rect_area(qr)
        else:
            areas, qr, Mq = [hw] * T, (0, w - 1, 0, h - 1), hw
        M = int(sum(areas))
        njt = (M + KJT - 1) // KJT
        nqt, nsplit = bank_plan(Mq, hw, njt, no, slots)
        masked = regional and Mq < hw
        rows_in = range(qr[2], qr[3] + 1) if Mq > 0 else range(0)
        objs.append(dict(Mq=Mq, nqt=nqt, M=M, njt=njt, nsplit=nsplit, areas=areas, qr=qr,
                         bounds=[s * njt // nsplit for s in range(nsplit + 1)] if nsplit else [0],
                         mean=masked, mean_tile=Mq >> 6, mean_lane=Mq & 63, mean_alone=masked and Mq % 64 == 0,
                         n_out=T * hw - M, fill_rows=(h - len(rows_in)) if masked else 0,
                         record=[Mq, nqt, nsplit, M, qr[0], qr[1], qr[2], qr[3], o * slots, 0, 0, 0]))
    return dict(objects=objs, slots=slots, regional=regional, copy_blocks=hw % 4 == 0 and aligned, comb=comb_channels(no),
                prefix_chunks=(T + PREFIX_CHUNK - 1) // PREFIX_CHUNK if regional else 0, layout=workspace_layout(no, hw))


# ================================================================================================ compaction
def _rects_for(case, o, mutant):
    """(memory rectangles [T][4], query rectangle) as the kernel would use them (clamped unless the fault says otherwise)."""
    no, T, h, w = dims(case)
    if case['mem_rects'] is None:
        return [(0, w - 1, 0, h - 1)] * T, (0, w - 1, 0, h - 1)
    oo = 0 if mutant == 'rects_of_object0' else o
    cl = (lambda r: tuple(int(v) for v in r)) if mutant == 'rects_unclamped' else (lambda r: clamp_rect(r, h, w))
    return [cl(case['mem_rects'][oo, t]) for t in range(T)], cl(case['qry_rects'][oo])


def _prefix(areas, mutant):
    pre = [0]
    carry = 0
    for base in range(0, len(areas), PREFIX_CHUNK):
        s = 0
        for a in areas[base:base + PREFIX_CHUNK]:
            s += a
            pre.append(carry + s)
        if mutant != 'prefix_carry_dropped':
            carry += s
    return np.array(pre, np.int64)


def _mem_cells(rects, prefix, T, h, w):
    """mem_index() of the kernel for n = 0 .. prefix[T] - 1: its binary search, then the raster position inside the box."""
    M = int(prefix[T])
    n = np.arange(max(M, 0), dtype=np.int64)
    lo, hi = np.zeros(n.size, np.int64), np.full(n.size, T, np.int64)
    while (hi - lo > 1).any():
        mid = (lo + hi) >> 1
        act, le = hi - lo > 1, prefix[mid] <= n
        lo, hi = np.where(act & le, mid, lo), np.where(act & ~le, mid, hi)
    r = np.array(rects, np.int64).reshape(T, 4)[lo]
    rw = np.maximum(r[:, 1] - r[:, 0] + 1, 1)                # (a fault can land in an empty box: the device would divide by 0)
    rem = n - prefix[lo]
    ry = rem // rw
    return (lo * h * w + (r[:, 2] + ry) * w + r[:, 0] + (rem - ry * rw)) % (T * h * w)


def compaction(case, o, mutant=None):
    """(memory cells in compacted order [M], query cells in compacted order [Mq]) as indices into T h w / h w."""
    no, T, h, w = dims(case)
    mr, qr = _rects_for(case, o, mutant)
    prefix = _prefix([rect_area(r) for r in mr], mutant)
    cells = _mem_cells(mr, prefix, T, h, w)
    rw = max(qr[1] - qr[0] + 1, 0)
    nq = np.arange(rect_area(qr), dtype=np.int64)
    qcells = ((qr[2] + nq // max(rw, 1)) * w + qr[0] + nq % max(rw, 1)) % (h * w)
    return cells, qcells, qr


# ================================================================================================ references
def read_f64(case):
    return G.read_f64(case)[0]


def _exp32(x, mutant=None):
    """The correctly rounded expf; 'expf_16ulp': 16 ulp off, the sign by the argument's low mantissa bit."""
    with np.errstate(all='ignore'):
        e = np.exp(np.asarray(x, np.float64)).astype(F32)
    if mutant == 'expf_16ulp':
        sign = np.where(np.asarray(x, F32).view(np.uint32) & 1, 1.0, -1.0)
        e = (e.astype(np.float64) * (1.0 + sign * 16 * EPS)).astype(F32)
    return e


def read_f32(case, mutant=None):
    """out [no, 1024, h, w] float32 in the kernels' order; cells no block writes stay NaN.  ``mutant`` plants one fault."""
    assert mutant is None or mutant in MUTANTS + VACUITY
    no, T, h, w = dims(case)
    hw, thw = h * w, T * h * w
    out = np.full((no, 2 * DO, hw), np.nan, F32)
    div = F32(DE) if mutant == 'sqrt_is_De' else np.sqrt(F32(DE))
    plan = plan_of(case)
    regional = plan['regional']
    kparts = 256 // plan['comb']
    fm = mutant if mutant in VACUITY else None
    with np.errstate(all='ignore'):
        for o in range(no):
            cells, qcells, qr = compaction(case, o, mutant)
            M, Mq = cells.size, qcells.size
            masked = regional and Mq < hw
            njt = (M + KJT - 1) // KJT
            nqt, nsplit = bank_plan(Mq, hw, njt, no, plan['slots'])
            n_out = F32(thw - (sum(rect_area(tuple(int(v) for v in r)) for r in case['mem_rects'][o])
                               if mutant == 'nout_unclamped' and regional else M))
            wrong = mutant == 'stride_thw'
            k = G._flat(case['m_key'][o], DE, T, thw, wrong)[:, cells]
            v = G._flat(case['m_val'][o], DO, T, thw, wrong)[:, cells]
            q = np.zeros((DE, Mq + 1), F32)                                   # the last column: the mean slot (zero key)
            q[:, :Mq] = case['q_key'][o].reshape(DE, hw)[:, qcells]
            nq = Mq + 1
            dot = np.zeros((M, nq), F32)
            for c in range(DE):
                dot = dot + k[c][:, None] * q[c][None, :]
            sc = dot / div
            parts = []
            for s in range(nsplit):
                jt0, jt1 = s * njt // nsplit, (s + 1) * njt // nsplit
                if mutant == 'uneven_last_tile_dropped':
                    jt1 = min(jt1, jt0 + njt // nsplit)
                mref, lsum, acc = np.full(nq, -np.inf, F32), np.zeros(nq, F32), np.zeros((DO, nq), F32)
                for jt in range(jt0, jt1):
                    a, b = jt * KJT, min(jt * KJT + KJT, M)
                    sv = np.full((KJT, nq), 0.0 if mutant == 'tail_logit_zero' else -np.inf, F32)
                    sv[:b - a] = sc[a:b]
                    tmax = sv.max(axis=0)
                    bump = tmax > mref + F32(KDEFER)
                    alpha = np.where(bump, _exp32(mref - tmax), F32(1))
                    mref = np.where(bump, tmax, mref)
                    p = _exp32(sv - mref, fm)
                    rs = p.sum(axis=0, dtype=F32)
                    lsum = (lsum if mutant == 'lsum_not_rescaled' else lsum * alpha) + rs
                    if mutant != 'acc_not_rescaled':
                        acc = acc * alpha
                    acc = acc + v[:, a:b] @ p[:b - a]
                parts.append((mref, lsum, acc))
            use = [s for s in range(nsplit) if not (mutant == 'splits_ge16_ignored' and s >= ML_REG_SPLITS)]
            mtot = np.full(nq, -np.inf, F32)
            for s in use:
                mtot = np.maximum(mtot, parts[s][0])
            if n_out > 0 and mutant != 'ref_not_raised':
                mtot = np.maximum(mtot, F32(0))
            wts = {s: _exp32(parts[s][0] - mtot) for s in use}
            if mutant == 'merge_weight_2m18' and len(use) > 1:                # split 1's weight (in [0, 1]) off by 2^-18
                wts[1] = wts[1] + F32(2.0 ** -18)
            closed = n_out * _exp32(-mtot) if n_out > 0 else np.zeros(nq, F32)
            # real queries: four interleaved groups, the closed-form term in group 0
            grp = [np.zeros(nq, F32) for _ in range(4)]
            for s in use:
                grp[s % 4] = grp[s % 4] + parts[s][1] * wts[s]
            if nsplit < ML_REG_SPLITS:                                        # a register slot without a split: l = 0, m = -inf
                grp[0] = grp[0] + F32(0) * _exp32(F32(-np.inf) - mtot)            # (NaN when mtot itself is -inf)
            if mutant != 'nout_dropped_query':
                grp[0] = grp[0] + closed
            inv = F32(1) / (((grp[0] + grp[1]) + grp[2]) + grp[3])
            accq = np.zeros((DO, nq), F32)
            for s in use:
                accq = accq + wts[s] * parts[s][2]
            res = accq * inv
            # the mean slot: weights divided by l, channels summed over interleaved groups of the splits
            lt = np.zeros(nq, F32)
            for s in use:
                lt = lt + parts[s][1] * wts[s]
            if mutant != 'nout_dropped_mean':
                lt = lt + closed
            tp = [np.zeros(DO, F32) for _ in range(kparts)]
            for s in use:
                tp[s % kparts] = tp[s % kparts] + (wts[s][Mq] / lt[Mq]) * parts[s][2][:, Mq]
            mean = np.zeros(DO, F32)
            for t in tp:
                mean = mean + t
            if mutant == 'mean_slot_tile0' and Mq >= KQT:
                mean = res[:, Mq & 63]
            # write-out
            inside = np.zeros(hw, bool)
            inside[qcells] = True
            cy = np.arange(hw) // w
            box_rows = (cy >= qr[2]) & (cy <= qr[3]) if Mq > 0 else np.zeros(hw, bool)
            if masked:
                if not (mutant == 'fill_skipped_mq0' and Mq == 0):
                    out[o, :DO][:, ~box_rows] = mean[:, None]
                out[o, :DO][:, box_rows & ~inside] = mean[:, None]
            out[o, :DO][:, qcells] = res[:, :Mq]
            if mutant == 'between_columns_neighbour' and masked and Mq > 0:
                for cell in np.flatnonzero(box_rows & ~inside):
                    prev = np.flatnonzero(qcells < cell)
                    n0 = (prev[-1] if prev.size else 0) // KQT * KQT          # the first query of the tile that writes the cell
                    out[o, :DO, cell] = res[:, n0]
            qv = case['q_val'][o].reshape(DO, hw)
            out[o, DO:] = qv if mutant == 'qval_not_zeroed' else np.where(inside, qv, qv * F32(0))
            if masked and mutant == 'fill_skipped_mq0' and Mq == 0:
                out[o, DO:] = np.nan
    return out.reshape(no, 2 * DO, h, w)


# ================================================================================================ the bound
def _walk64(s, M, bounds, name):
    """The deferred reference in float64 over the compacted logits s [M, nq]: per cell and query the argument x of expf and the number
    of rescales that follow the cell's tile inside its split; per query and split the final reference.  Asserts that no decision is
    within MARGIN of its threshold."""
    nq = s.shape[1]
    x = np.zeros_like(s)
    nb = np.zeros(s.shape, np.int32)
    mrefs = []
    for si in range(len(bounds) - 1):
        mref = np.full(nq, -np.inf)
        tiles = []
        for jt in range(bounds[si], bounds[si + 1]):
            a, b = jt * KJT, min(jt * KJT + KJT, M)
            tmax = s[a:b].max(axis=0)
            with np.errstate(invalid='ignore'):
                gap = tmax - (mref + KDEFER)
            assert not (np.abs(gap[np.isfinite(gap)]) < MARGIN).any(), (name, 'a raise of the reference is decided within the margin')
            bump = ~np.isfinite(gap) | (gap > 0)
            later = bump & np.isfinite(mref)
            for (pa, pb) in tiles:
                nb[pa:pb] += later[None, :]
            mref = np.where(bump, tmax, mref)
            x[a:b] = s[a:b] - mref
            tiles.append((a, b))
        mrefs.append(mref)
    return x, nb, mrefs


def bound(case, skip=None, parts=False):
    """(out64 [no, 1024, h, w], bound [no, 1024, h, w]; with ``parts`` also the share of the A_REL term).  The q_val half's bound
    is 0.  ``skip`` [no, h w] marks query cells outside the premise (the one-hot queries, compared bit for bit).  Asserts its
    validity range: every argument of expf in [X_LO, X_HI + MARGIN], every decision of the deferred reference clear of its threshold."""
    no, T, h, w = dims(case)
    hw, thw = h * w, T * h * w
    out64 = read_f64(case)
    bo = np.zeros((no, 2 * DO, hw))
    ashare = np.zeros((no, 2 * DO, hw))
    plan = plan_of(case)
    r_a = A_REL + U * 64 + U
    for o in range(no):
        po = plan['objects'][o]
        cells, qcells, qr = compaction(case, o)
        M, Mq, nsplit, n_out = po['M'], po['Mq'], po['nsplit'], po['n_out']
        if M == 0:
            continue                                                       # the read-out is exactly 0
        use = np.ones(Mq + 1, bool)
        if skip is not None:
            use[:Mq] = ~skip[o][qcells]
        sel = np.flatnonzero(use)
        if sel.size == 0:
            continue
        k = case['m_key'][o][:, :T].reshape(DE, thw)[:, cells].astype(np.float64)
        v = np.abs(case['m_val'][o][:, :T].reshape(DO, thw)[:, cells].astype(np.float64))
        q = np.zeros((DE, Mq + 1))
        q[:, :Mq] = case['q_key'][o].reshape(DE, hw)[:, qcells]
        q = q[:, sel]
        s = k.T @ q / np.sqrt(float(DE))
        A = np.abs(k).T @ np.abs(q)
        x, nb, mrefs = _walk64(s, M, po['bounds'], case['name'])
        mtot = np.max(np.stack(mrefs), axis=0)
        if n_out > 0:
            mtot = np.maximum(mtot, 0.0)
        xm = np.stack(mrefs) - mtot
        lo = min(float(x.min()), float(xm.min()), float((-mtot).min()) if n_out > 0 else 0.0)
        assert lo >= X_LO and float(x.max()) <= X_HI + MARGIN, (case['name'], lo, float(x.max()), 'expf outside its measured interval')
        e = np.exp(s - mtot)
        z = e.sum(axis=0) + n_out * np.exp(-mtot)
        p = e / z
        p_out = n_out * np.exp(-mtot) / z
        vs = case['m_val'][o][:, :T].reshape(DO, thw)[:, cells].astype(np.float64)
        o64 = vs @ p                                                        # [DO, queries]: the float64 read-out
        nt = max(po['bounds'][i + 1] - po['bounds'][i] for i in range(nsplit))
        split_of = np.searchsorted(np.array(po['bounds'][1:]) * KJT, np.arange(M), side='right')
        rem = np.minimum(np.array(po['bounds'][1:])[split_of] * KJT, M) - np.arange(M) + 4      # roundings of acc that cell j's term passes
        nbm = int(nb.max())
        ds = gamma(DE) * A / np.sqrt(float(DE)) + 2 * U * np.abs(s)
        c0 = ds + U * np.abs(x) + E_WIDE * EPS + U * np.abs(xm)[split_of] + E_WIDE * EPS         # shared by numerator and denominator
        c = c0 + nb * r_a
        c_out = E_WIDE * EPS + 2 * U
        own = gamma(rem)[:, None] + nb * U                                  # the numerator's own roundings
        g_num, g_den = gamma(2 * nsplit + 1) + U, gamma(nt + 10 + nbm) + gamma(nsplit + 5) + U
        vp = v @ p
        b = np.zeros((DO, sel.size))
        a_part = np.zeros((DO, sel.size))
        pc, pa = p * c, p * nb * r_a
        for n in range(sel.size):                                           # sum_j |v_dj - out_d| p_j c_j per query
            dv = np.abs(vs - o64[:, n][:, None])
            b[:, n] = dv @ pc[:, n]
            a_part[:, n] = dv @ pa[:, n]
        b = SLACK * (b + np.abs(o64) * p_out * c_out + v @ (p * own) + vp * g_num + np.abs(o64) * g_den) + TINY
        a_part = SLACK * a_part
        col = {int(i): n for n, i in enumerate(sel)}
        if Mq in col:                                                        # the mean slot's bound: every masked query cell
            inside = np.zeros(hw, bool)
            inside[qcells] = True
            bo[o, :DO][:, ~inside] = b[:, col[Mq]][:, None]
        live = sel[sel < Mq]
        bo[o, :DO][:, qcells[live]] = b[:, [col[int(i)] for i in live]]
        ashare[o, :DO][:, qcells[live]] = a_part[:, [col[int(i)] for i in live]]
    bo, ashare = bo.reshape(no, 2 * DO, h, w), ashare.reshape(no, 2 * DO, h, w)
    return (out64, bo, ashare) if parts else (out64, bo)


# ================================================================================================ case families
def _base(name, family, shape, rects, tcap):
    no, T, h, w = shape
    return G._empty_case(name, family, (no, DE, DO, T, h, w), rects, tcap)


def equal_case(name, shape, rects=None, tcap=None, seed=0, variant='zero'):
    no, T, h, w = shape
    return dict(G.equal_case(name, (no, DE, DO, T, h, w), rects, tcap, seed, variant), family=variant)


def random_case(name, shape, rects=None, tcap=None, seed=0):
    no, T, h, w = shape
    return G.random_case(name, (no, DE, DO, T, h, w), rects, tcap, seed)


def onehot_positions(po):
    """Compacted positions of the candidates of one object (at most 128), the named ones first."""
    M, njt, nsplit, bounds = po['M'], po['njt'], po['nsplit'], po['bounds']
    if M == 0:
        return []
    want = [0, min(KJT - 1, M - 1), min(KJT, M - 1), M - 1, (M - 1) // KJT * KJT]
    pre = np.concatenate([[0], np.cumsum(po['areas'])])
    want += [int(pre[t]) for t in range(1, len(po['areas'])) if po['areas'][t] > 0 and po['areas'][t - 1] == 0]
    for s in dict.fromkeys([0, nsplit - 1, 1, nsplit - 2, 15, 16, 17, nsplit // 2]):
        if 0 <= s < nsplit:
            jt0, jt1 = bounds[s], bounds[s + 1]
            want += [jt0 * KJT, min(jt0 * KJT + KJT - 1, M - 1), (jt1 - 1) * KJT, min(jt1 * KJT, M) - 1]
    want += [int(pre[t]) for t in range(len(po['areas'])) if po['areas'][t] > 0]
    want += [int(n) for n in np.linspace(0, M - 1, 24).astype(int)]
    return list(dict.fromkeys(want))[:DE]


def onehot_case(name, shape, rects=None, tcap=None, seed=0):
    no, T, h, w = shape
    case = _base(name, 'onehot', shape, rects, tcap)
    rng = G._rng((no, DE, DO, T, h, w), seed, 4)
    hw = h * w
    case['m_val'][:] = G._values(rng, case['m_val'].shape, False)
    case['m_val'][case['m_val'] == 0] = F32(0.5)
    case['q_val'][:] = G._values(rng, case['q_val'].shape, False)
    plan = plan_of(case)
    tg = np.full((no, hw), -1, np.int64)
    case['positions'] = []
    for o in range(no):
        cells, qcells, _ = compaction(case, o)
        pos = onehot_positions(plan['objects'][o])
        case['positions'].append(pos)
        if not pos or not qcells.size:
            continue
        mk = case['m_key'][o].reshape(DE, -1)                                # (a view: Tcap h w cells, the first T h w are read)
        for c, n in enumerate(pos):
            mk[c, cells[n]] = F32(ONEHOT_G)
        qk = case['q_key'][o].reshape(DE, hw)
        for i, cell in enumerate(qcells):
            c = (i + o) % len(pos)
            qk[c, cell] = F32(ONEHOT_G)
            tg[o, cell] = cells[pos[c]]
    case['targets'] = tg
    return case


SPIKES = (('+20', 20.0), ('+45', 45.0), ('+45late', 45.0))


def spike_positions(po):
    """Compacted positions of the three rises: +20 and +45 in tiles after the first of split 0 (the +45 after the +20), the late +45
    in the last split (after its first tile when it has more than one)."""
    M, njt, nsplit, bounds = po['M'], po['njt'], po['nsplit'], po['bounds']
    if M == 0:
        return {}
    t1 = bounds[1] if nsplit > 1 else njt
    pos = {'+20': min((1 if t1 > 1 else 0) * KJT + 5, M - 1)}
    pos['+45'] = min((2 if t1 > 2 else t1 - 1) * KJT + 17, M - 1)
    if nsplit > 1:
        lt0 = bounds[nsplit - 1]
        pos['+45late'] = min((lt0 + 1 if njt - lt0 > 1 else lt0) * KJT + 9, M - 1)
    return pos


def spike_case(name, shape, rects=None, tcap=None, seed=0):
    no, T, h, w = shape
    case = dict(random_case(name, shape, rects, tcap, seed + 100), family='spike')
    case['m_key'][:, 0] = 0
    case['q_key'][:, 0] = 1
    while max(float(G.spread(case, o).max()) for o in range(no)) > 8.0:
        case['m_key'] *= F32(0.5)
    plan = plan_of(case)
    case['spikes'] = []
    for o in range(no):
        cells = compaction(case, o)[0]
        pos = spike_positions(plan['objects'][o])
        case['spikes'].append(pos)
        mk0 = case['m_key'][o, 0].reshape(-1)
        done = set()
        for tag, rise in reversed(SPIKES):                                   # (a tiny memory: positions that coincide get one rise)
            if tag in pos and pos[tag] not in done:
                done.add(pos[tag])
                mk0[cells[pos[tag]]] += F32(rise * np.sqrt(float(DE)))
    return case


# ================================================================================================ what a result must be
def expectations(case):
    """out64, bound, out_bits, out_exact [no, 1024, h, w]: bit for bit the q_val half; the one-hot queries; an object without a live
    memory cell (0); the 'zero' family when T h w is a power of two and sum |v| < 2^24 (every cell, masked ones included)."""
    no, T, h, w = dims(case)
    hw, thw = h * w, T * h * w
    onehot = case['targets'] >= 0 if case['family'] == 'onehot' else np.zeros((no, hw), bool)
    out64, bo, ashare = bound(case, skip=onehot, parts=True)
    out_bits = out64.astype(F32).reshape(no, 2 * DO, hw)
    exact = np.zeros((no, 2 * DO, hw), bool)
    out_bits[:, DO:] = G.qval_half(case).reshape(no, DO, hw)
    exact[:, DO:] = True
    for o in range(no):
        mm, qm = G.live_masks(case, o)
        v = np.where(mm, case['m_val'][o][:, :T].reshape(DO, -1), F32(0))
        if not mm.any():
            exact[o, :DO] = True
            out_bits[o, :DO] = F32(0)
        elif case['int_vals'] and G._is_pow2(thw) and float(np.abs(v).sum(axis=1).max()) < 2.0 ** 24:
            exact[o, :DO] = True                                             # (out64 is an integer / 2^k: its fp32 rounding is exact)
        sel = np.flatnonzero(onehot[o])
        if sel.size:
            out_bits[o, :DO][:, sel] = v[:, case['targets'][o][sel]]
            exact[o, :DO][:, sel] = True
    sh = (no, 2 * DO, h, w)
    return dict(out64=out64, bound_out=bo, a_share=ashare, out_bits=out_bits.reshape(sh), out_exact=exact.reshape(sh),
                p64=None, bound_p=None, p_bits=None, p_exact=None, onehot=onehot)


def check(case, exp, out):
    """generic_ref.check on the read-out: every element bit for bit or inside the bound, a NaN fails; the report names the count and
    the first offender (index, got, want, bound)."""
    return G.check(case, exp, out)


def junked(case, seed=9):
    """The case with finite junk in every masked key and value cell, in the frames beyond T, and in q_key AND q_val of the masked query
    cells (q_val's masked cells are part of the result: a zero of their sign)."""
    c = G.filled(dict(case, De=DE, Do=DO), 'garbage', seed)
    no, T, h, w = dims(case)
    rng = np.random.RandomState(seed + 1)
    qv = case['q_val'].copy()
    for o in range(no):
        qm = G.live_masks(case, o)[1].reshape(h, w)
        qv[o][:, ~qm] = (rng.randn(DO, int((~qm).sum())) * 5).astype(F32)
    c['q_val'] = qv
    return c
