# -*- coding: utf-8 -*-
"""numpy restatements of the elementwise glue kernels of rmnet_amd/csrc/epilogue.hip (channel_affine, upsample2x_add,
affine_relu_maxpool, each in an NCHW and a channels-last form, and soft_aggregate), of their launchers' decisions, and the error
bound of soft_aggregate.  No torch, no GPU: tests/test_glue_edges.py imports this on any machine.

Every restatement takes and returns LOGICAL [N, C, H, W] arrays; the memory layout is the caller's business (both layouts of a
kernel evaluate the same expression on the same values, so one restatement serves both).

*_f32: every operation rounded to fp32 in the kernel's order (numpy float32 arithmetic is IEEE, one rounding per operation, and
       epilogue.hip is compiled with fp contract(off)).  For channel_affine, upsample2x_add and affine_relu_maxpool the kernels use
       nothing but +, -, *, comparisons and int <-> float conversions, so these are bit-for-bit oracles: every non-NaN output must
       have the same 32 bits, signed zeros included, and a NaN must be a NaN (payloads and signs of NaNs are not compared: the
       host and the device pick different default NaNs).  Details that follow from "the kernel's order":
         - an absent scale / shift is a multiplication by 1.0f / an addition of 0.0f, so -0.0 becomes +0.0 where shift is absent;
         - relu is y < 0 ? 0 : y (keeps -0.0 and NaN), LeakyReLU is y > 0 ? y : y * 0.1f;
         - the pool walks its window dy-major, dx-minor with best = t > best ? t : best from -inf, so among equal zeros the FIRST
           one's sign survives; padding is -inf (never wins, never a NaN), a NaN in the window gives NaN;
         - tap2x: src = 0.5f * (d + 0.5f) - 0.5f clamped at 0, i0 = (int)src, i1 = i0 + (i0 < n - 1), l1 = src - i0, l0 = 1 - l1;
           out = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11), then skip + out.
*_f64: the same mathematics in float64.  For upsample2x_add on inputs that are integer multiples of 4 with |x| <= 2^18 the
       weights {0, 1/4, 3/4, 1} make every inner product an integer, every outer product a multiple of 1/4 below 2^20, and the
       sums stay below 2^21: each fp32 step is exact, the float64 result is representable, and the kernel must return it exactly.
NaN:   soft_aggregate clamps with comparisons (em < lo ? lo : em), which keep a NaN, as torch.clamp does in the module graph: a NaN
       in one object's decoder logits is a NaN in that object's channel and in the background of that pixel (and, through the
       soft-max, in every probability of that pixel), and nowhere else.

soft_aggregate: the bound
-------------------------
u = 2^-24 (one fp32 rounding, relative), eps = 2^-23 (one ulp, relative, at worst).  E and L are the largest errors of the
device's expf and logf in ulps (E_ULP, L_ULP below: measured, see profiles/r14_a_glue_tests.md; the bound uses twice the measured
maxima).  Lines 147-195 of epilogue.hip, per object o and pixel, with d = |z1 - z0|:
  1. a = z - max(z0, z1): one of the two is exactly 0, the other -d (1 + t), |t| <= u          (argument subtraction: 1 rounding)
  2. e = expf(a): the larger is expf(0) (1 + E eps), the smaller exp(-d) with relative error <= d u + E eps    (two expf)
  3. s = e0 + e1: relative error <= that of its worse term + u                                                   (the sum)
  4. p = e1 / s: p = e1 / (e0 + e1) moves by (1 - p)(t1 - t0) under relative changes t of e, so
       rel(p) <= 2 E eps + d u + 2 u =: r_p                                                                 (the quotient)
  5. em = clamp(p): clamping is monotone and non-expansive, so |em^ - em| <= |p^ - p| = p r_p =: a_p with em the clamp of the
     TRUE p at the same fp32 constants (what soft_aggregate_f64 evaluates)
  6. q = 1 - em: rel(q) <= a_p / (1 - em) + u                                                                  (1 - em)
  7. r = em / q: rel(r) <= a_p / em + a_p / (1 - em) + 2 u                                                     (the quotient)
  8. l = logf(r): |l^ - l| <= rel(r) + L eps |l|                                                                (logf)
  so for a foreground logit, with em = p inside the clamp,  |l^ - l| <= r_p / (1 - p) + (2 + 2 L |l|) u:  the issue's
  (c_p + d) u / (1 - p) + (c_l + L' |l|) u  with c_p = 4 E + 2, c_l = 2, L' = 2 L (ulps to u).
  Background: bg = prod_o (1 - p_o), each factor with rel <= a_p,o / (1 - p_o) + u (step 6 without the clamp) and one more rounding
  per product, so rel(bg) <= sum_o (a_p,o / (1 - p_o) + 2 u); steps 5-8 with a_bg = bg rel(bg) in the place of a_p give
  rel(bg) / (1 - bg) + ... : the factors' relative errors summed and divided by 1 - bg.
  An absent channel is em_logit(0): steps 6-8 on an exact em, (2 + 2 L |l|) u.  The same holds for EVERY logit whose p (or bg) is
  exact in fp32, which is what the structural family is made of: its bound is this "logf term" alone.
  Soft-max over the K channels (lines 184-195), logits with errors g_k and true probabilities P_k, A = max_k |l_k - max l|:
  the subtraction l_k - mx (1 rounding of a value <= A), expf, a sum of K terms (K - 1 roundings), the quotient; P_k moves by
  P_k (t_k - sum_j P_j t_j) under changes t of the exponents, so
       |P^_k - P_k| <= P_k (g_k + sum_j P_j g_j + 2 A u + 2 E eps + K u).
  First-order terms only; the neglected products of two of them are below 1e-3 of the bound for d <= 6 (the largest single term
  is r_p / (1 - p) <= 30 u * 400 < 1e-3), and every bound is multiplied by 1 + 1e-3 for them.
  Roundings counted: 1 + 2 + 1 + 1 per object probability, 2 per background factor, 3 per logit, K + 2 per soft-max output.
"""

import numpy as np

F32 = np.float32
U = 2.0 ** -24
EPS = 2.0 ** -23
# expf and logf of the device library on gfx950, largest error found against float64 over the arguments the cases produce
# (tools/ubench/math_ulp.hip on an MI355X, 2^22 points each; profiles/r14_a_glue_tests.md has the run): expf 0.834 ulp on [-34, 0],
# logf 2.313 ulp on [1e-8, 1e8].  The bound allows twice that.
E_MEASURED, L_MEASURED = 0.834, 2.313
E_ULP, L_ULP = 2.0 * E_MEASURED, 2.0 * L_MEASURED
SLACK = 1.0 + 1e-3

K_THREADS, K_UNROLL = 256, 4            # epilogue.hip kThreads, kUnroll
MAX_GRID_Y = 65535


# ================================================================================================ the launchers, restated
def _ceil_div(a, b):
    return -(-a // b)


def plan_of(entry, shape, alignments=None, res=False):
    """What the launcher of ``entry`` does with an activation ``x`` of logical shape (N, C, H, W).
    alignments: {'x' | 'res' | 'skip' | 'out': address % 16} (absent = 0); ``res``: a residual / skip operand is passed.
    Returns dict(kernel=the template instance, grid=(x, y), iters=grid-stride iterations of workgroup (0, 0) (the busiest),
    passes=plane-loop passes of the busiest workgroup, slots=unroll slots that hold data in the LAST iteration of the busiest
    workgroup of the unrolled kernels)."""
    al = dict(alignments or {})
    N, C, H, W = shape
    mis = lambda *names: any(al.get(n, 0) % 16 for n in names)
    planes = N * C
    gy = min(planes, MAX_GRID_Y)
    passes = _ceil_div(planes, gy)
    if entry == 'channel_affine':
        HW = H * W
        vec = HW % 4 == 0 and not mis('x', 'out', 'res')
        per_block = K_THREADS * (4 * K_UNROLL if vec else 1)
        gx = min(_ceil_div(HW, per_block), 64)
        n = HW // 4 if vec else HW
        step = gx * K_THREADS * (K_UNROLL if vec else 1)
        return dict(kernel='channel_affine<%s,%s>' % ('VEC4' if vec else 'scalar', 'RES' if res else 'noRES'), vec=vec, grid=(gx, gy),
                    iters=_ceil_div(n, step), passes=passes)
    if entry == 'channel_affine_nhwc':
        assert C % 4 == 0 and not mis('x', 'out', 'res')
        C4 = C // 4
        n4 = N * H * W * C4
        gx = max(min(_ceil_div(n4, K_THREADS * K_UNROLL), 8192), 1)
        fixed = K_THREADS % C4 == 0
        step = gx * K_THREADS * K_UNROLL
        iters = _ceil_div(n4, step)
        last = n4 - (iters - 1) * step                      # float4 left for the last sweep; workgroup 0 takes the first 1024 of them
        return dict(kernel='channel_affine_nhwc<%s,%s>' % ('RES' if res else 'noRES', 'FIXED' if fixed else 'perElement'), fixed=fixed,
                    grid=(gx, 1), iters=iters, passes=1, slots=min(_ceil_div(min(last, K_THREADS * K_UNROLL), K_THREADS), K_UNROLL),
                    capped=_ceil_div(n4, K_THREADS * K_UNROLL) > 8192)
    if entry == 'upsample2x_add':
        vec = W % 2 == 0 and not mis('out', 'skip')
        items = 2 * H * ((2 * W) // 4 if vec else 2 * W)
        chunks = _ceil_div(items, K_THREADS)
        gx = min(chunks, 256)
        return dict(kernel='upsample2x_add<%s,%s>' % ('VEC4' if vec else 'scalar', 'ADD' if res else 'noADD'), vec=vec, grid=(gx, gy),
                    iters=_ceil_div(items, gx * K_THREADS), passes=passes, capped=chunks > 256, per_row=(2 * W) // 4 if vec else 2 * W)
    if entry == 'upsample2x_add_nhwc':
        assert C % 4 == 0 and not mis('x', 'out', 'skip')
        items = N * 4 * H * W * (C // 4)
        chunks = _ceil_div(items, K_THREADS)
        gx = max(min(chunks, 8192), 1)
        return dict(kernel='upsample2x_add_nhwc<%s>' % ('ADD' if res else 'noADD'), grid=(gx, 1), iters=_ceil_div(items, gx * K_THREADS),
                    passes=1, capped=chunks > 8192)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if entry == 'affine_relu_maxpool':
        vec = W == 2 * Wo and Wo % 4 == 0 and not mis('x', 'out')
        items = Ho * (Wo // 4 if vec else Wo)
        chunks = _ceil_div(items, K_THREADS)
        gx = min(chunks, 128)
        return dict(kernel='affine_relu_maxpool<%s>' % ('VEC4' if vec else 'scalar'), vec=vec, grid=(gx, gy),
                    iters=_ceil_div(items, gx * K_THREADS), passes=passes, capped=chunks > 128, per_row=Wo // 4 if vec else Wo)
    if entry == 'affine_relu_maxpool_nhwc':
        assert C % 4 == 0 and not mis('x', 'out')
        items = N * Ho * Wo * (C // 4)
        chunks = _ceil_div(items, K_THREADS)
        gx = max(min(chunks, 8192), 1)
        return dict(kernel='affine_relu_maxpool_nhwc', grid=(gx, 1), iters=_ceil_div(items, gx * K_THREADS), passes=1, capped=chunks > 8192)
    raise KeyError(entry)


# ================================================================================================ channel_affine
def _per_channel(t, C, default, dtype):
    if t is None:
        return np.full((1, C, 1, 1), default, dtype)
    return np.asarray(t, dtype).reshape(1, C, 1, 1)


def _channel_affine(x, scale, shift, res, rscale, rshift, relu, dtype, mutant=None):
    x = np.asarray(x, dtype)
    C = x.shape[1]
    sc, sh = _per_channel(scale, C, 1.0, dtype), _per_channel(shift, C, 0.0, dtype)
    leaky = lambda y: np.where(y > 0, y, y * dtype(F32(0.1)))
    with np.errstate(all='ignore'):
        y = x * sc + sh
        if res is not None:
            rs, rh = _per_channel(rscale, C, 1.0, dtype), _per_channel(rshift, C, 0.0, dtype)
            r = np.asarray(res, dtype)
            term = (r + rh) * rs if mutant == 'rshift_before_rscale' else r * rs + rh
            if mutant == 'leaky_before_res' and relu == 'leaky':
                return (leaky(y) + term).astype(dtype)
            y = y + term
        if relu == 'leaky':
            y = leaky(y)
        elif relu:
            y = np.where(y < 0, dtype(0.0), y)
    return y.astype(dtype)


def channel_affine_f32(x, scale=None, shift=None, res=None, rscale=None, rshift=None, relu=False, mutant=None):
    return _channel_affine(x, scale, shift, res, rscale, rshift, relu, F32, mutant)


def channel_affine_f64(x, scale=None, shift=None, res=None, rscale=None, rshift=None, relu=False):
    return _channel_affine(x, scale, shift, res, rscale, rshift, relu, np.float64)


# ================================================================================================ upsample2x_add
def tap2x(n, dtype=F32, mutant=None):
    """i0, i1, l0, l1 of the 2n outputs along one axis (epilogue.hip tap2x), in ``dtype`` arithmetic."""
    d = np.arange(2 * n).astype(dtype)
    src = dtype(0.5) * (d + dtype(0.5)) - dtype(0.5)
    src = np.where(src < 0, dtype(0.0), src)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < (n if mutant == 'i1_clamped_at_n' else n - 1))
    l1 = src - i0.astype(dtype)
    l0 = dtype(1.0) - l1
    if mutant == 'weights_swapped':
        l0, l1 = l1, l0
    return i0, i1, l0, l1


def _upsample(x, skip, dtype, mutant=None):
    x = np.asarray(x, dtype)
    N, C, h, w = x.shape
    if mutant == 'i1_clamped_at_n':       # the read one past the row / the plane: a zero stands for whatever lies there
        x = np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 1)))
    y0, y1, ly0, ly1 = tap2x(h, dtype, mutant)
    x0, x1, lx0, lx1 = tap2x(w, dtype, mutant)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    with np.errstate(all='ignore'):
        r0, r1 = x[:, :, y0, :], x[:, :, y1, :]
        o = ly0 * (lx0 * r0[..., x0] + lx1 * r0[..., x1]) + ly1 * (lx0 * r1[..., x0] + lx1 * r1[..., x1])
        if skip is not None:
            o = np.asarray(skip, dtype) + o
    return o.astype(dtype)


def upsample_f32(x, skip=None, mutant=None):
    return _upsample(x, skip, F32, mutant)


def upsample_f64(x, skip=None):
    return _upsample(x, skip, np.float64)


# ================================================================================================ affine_relu_maxpool
def _maxpool(x, scale, shift, dtype, mutant=None):
    x = np.asarray(x, dtype)
    N, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    sc, sh = _per_channel(scale, C, 1.0, dtype), _per_channel(shift, C, 0.0, dtype)
    with np.errstate(all='ignore'):
        v = x * sc + sh
        isnan = v != v
        a = np.where(v < 0, dtype(0.0), v)
        pad = ((0, 0), (0, 0), (1, 2), (1, 2))
        a = np.pad(a, pad, constant_values=-np.inf)
        isnan = np.pad(isnan, pad, constant_values=False)
        best = np.full((N, C, Ho, Wo), -np.inf, dtype)
        nan = np.zeros((N, C, Ho, Wo), bool)
        quad = (np.arange(Wo) % 4 == 0) & (np.arange(Wo) > 0)       # outputs whose left column is the vector kernel's scalar load
        for dy in range(3):
            for dx in range(3):
                t = a[:, :, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
                tn = isnan[:, :, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
                if mutant == 'left_column_dropped' and dx == 0:
                    t, tn = np.where(quad, dtype(-np.inf), t), tn & ~quad
                best = np.where(t > best, t, best)
                nan |= tn
        if mutant != 'nan_not_propagated':
            best = np.where(nan, dtype(np.nan), best)
    return best.astype(dtype)


def maxpool_f32(x, scale=None, shift=None, mutant=None):
    return _maxpool(x, scale, shift, F32, mutant)


def maxpool_f64(x, scale=None, shift=None):
    return _maxpool(x, scale, shift, np.float64)


# ================================================================================================ soft_aggregate
CLAMP_LO = F32(1e-7)
CLAMP_HI = F32(1.0) - F32(1e-7)


def _soft_aggregate(dec, obj_begin, K, pad_l, pad_t, H, W, dtype, want_prob=True, mutant=None, detail=False):
    """logit, prob [B, K, H, W] (prob None unless asked) in ``dtype`` arithmetic, in the kernel's order of operations.
    detail: also the per-clip lists of p, d = |z1 - z0| and bg (for the bound)."""
    dec = np.asarray(dec, dtype)
    Hp, Wp = dec.shape[2:]
    B = len(obj_begin) - 1
    lo = dtype(F32(1e-6)) if mutant == 'clamp_1e-6' else dtype(CLAMP_LO)
    hi = dtype(F32(1.0) - F32(1e-6)) if mutant == 'clamp_1e-6' else dtype(CLAMP_HI)
    if mutant == 'pads_swapped':
        pad_l, pad_t = pad_t, pad_l
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    pix = ((yy + pad_t) * Wp + (xx + pad_l)).ravel()
    one = dtype(1.0)

    def em_logit(em):
        em = np.minimum(np.maximum(em, lo), hi)
        return np.log(em / (one - em)).astype(dtype)

    logit = np.empty((B, K, H, W), dtype)
    prob = np.empty((B, K, H, W), dtype) if want_prob else None
    det = []
    with np.errstate(all='ignore'):
        labs = em_logit(np.zeros(H * W, dtype))
        for b in range(B):
            o0 = int(obj_begin[b])
            cnt = int(obj_begin[b + 1]) - o0
            n = cnt if mutant == 'min_dropped' else min(cnt, K - 1)
            bg = np.ones(H * W, dtype)
            ls, ps, ds = [], [], []
            for o in range(n):
                z0 = np.take(dec[o0 + o, 0].ravel(), pix, mode='wrap')
                z1 = np.take(dec[o0 + o, 1].ravel(), pix, mode='wrap')
                m = np.maximum(z0, z1)
                e0, e1 = np.exp(z0 - m).astype(dtype), np.exp(z1 - m).astype(dtype)
                p = e1 / (e0 + e1)
                bg = bg * (one - p)
                ls.append(em_logit(p))
                ps.append(p)
                ds.append(np.abs(z1.astype(np.float64) - z0.astype(np.float64)))
            l0 = em_logit(bg)
            chans = [l0] + ls[:K - 1] + [labs] * max(K - 1 - n, 0)
            for k in range(K):
                logit[b, k] = chans[k].reshape(H, W)
            if want_prob:
                full = [l0] + ls + [labs] * max(K - 1 - n, 0)
                mx = full[0]
                for l in full[1:]:
                    mx = np.maximum(mx, l)
                ex = [np.exp(l - mx).astype(dtype) for l in full]
                s = ex[0].copy()
                for e in ex[n + 1:]:
                    s = s + e
                for e in ex[1:n + 1]:
                    s = s + e
                for k in range(K):
                    prob[b, k] = (ex[k] / s).reshape(H, W)
            det.append(dict(p=ps, d=ds, bg=bg, n=n))
    return (logit, prob, det) if detail else (logit, prob)


def soft_aggregate_f32(dec, obj_begin, K, pad_l, pad_t, H, W, want_prob=True, mutant=None):
    return _soft_aggregate(dec, obj_begin, K, pad_l, pad_t, H, W, F32, want_prob, mutant)


def soft_aggregate_f64(dec, obj_begin, K, pad_l, pad_t, H, W, want_prob=True):
    return _soft_aggregate(dec, obj_begin, K, pad_l, pad_t, H, W, np.float64, want_prob)


def logf_term(l, L=None):
    """Steps 6-8 on an exact em: |l^ - l| <= (2 + 2 L |l|) u."""
    L = L_ULP if L is None else L
    return SLACK * (2.0 * U + L * EPS * np.abs(l))


def soft_aggregate_bound(dec, obj_begin, K, pad_l, pad_t, H, W, E=None, L=None):
    """(logit64, prob64, bound on the logits, bound on the probabilities) for every element: the module docstring's derivation."""
    E = E_ULP if E is None else E
    L = L_ULP if L is None else L
    logit, prob, det = _soft_aggregate(dec, obj_begin, K, pad_l, pad_t, H, W, np.float64, True, None, detail=True)
    lo, hi = float(CLAMP_LO), float(CLAMP_HI)
    bl = np.empty_like(logit)

    def from_abs(a_em, em_true, l):          # steps 5-8
        em = np.clip(em_true, lo, hi)
        return a_em / em + a_em / (1.0 - em) + 2.0 * U + L * EPS * np.abs(l)

    for b, d in enumerate(det):
        n = d['n']
        rel_bg = np.zeros(H * W)
        for o in range(n):
            p = d['p'][o]
            a_p = p * (2.0 * E * EPS + d['d'][o] * U + 2.0 * U)
            bl[b, o + 1] = from_abs(a_p, p, logit[b, o + 1].ravel()).reshape(H, W)
            rel_bg += a_p / np.maximum(1.0 - p, 1e-300) + 2.0 * U
        bl[b, 0] = from_abs(d['bg'] * rel_bg, d['bg'], logit[b, 0].ravel()).reshape(H, W)
        for k in range(n + 1, K):
            bl[b, k] = 2.0 * U + L * EPS * np.abs(logit[b, k])
    bl *= SLACK
    A = (logit.max(axis=1, keepdims=True) - logit).max(axis=1, keepdims=True)
    bp = SLACK * prob * (bl + (prob * bl).sum(axis=1, keepdims=True) + 2.0 * (A + 1.0) * U + 2.0 * E * EPS + K * U)
    return logit, prob, bl, bp


# ------------------------------------------------------------------------------------------------ the structural family
def _hash(a):
    """A fixed 32-bit mix (xorshift-multiply) of an integer array."""
    a = np.asarray(a, np.uint64)
    a = (a ^ (a >> np.uint64(16))) * np.uint64(0x45d9f3b) & np.uint64(0xffffffff)
    a = (a ^ (a >> np.uint64(16))) * np.uint64(0x45d9f3b) & np.uint64(0xffffffff)
    return a ^ (a >> np.uint64(16))


def structural_dec(n_tot, Hp, Wp, seed=0):
    """Decoder logits [n_tot, 2, Hp, Wp] with z1 - z0 drawn per (object, padded pixel) from {0, +200, -200} and z0 a small integer:
    all exact in fp32, z - max(z0, z1) exact, p in {1/2, 1, 0}."""
    idx = np.arange(n_tot * Hp * Wp).reshape(n_tot, Hp, Wp) + 7919 * seed
    hsh = _hash(idx)
    delta = np.array([0.0, 200.0, -200.0], np.float32)[(hsh % np.uint64(3)).astype(np.int64)]
    z0 = ((hsh >> np.uint64(8)) % np.uint64(7)).astype(np.float32) - 3.0
    return np.stack([z0, z0 + delta], axis=1).astype(np.float32)


def structural_choice(dec, pad_l, pad_t, H, W):
    """z1 - z0 of the un-padded window, [n_tot, H, W]."""
    return (dec[:, 1] - dec[:, 0])[:, pad_t:pad_t + H, pad_l:pad_l + W]


MUTANTS = ('i1_clamped_at_n', 'weights_swapped', 'left_column_dropped', 'nan_not_propagated', 'rshift_before_rscale', 'leaky_before_res',
           'min_dropped', 'pads_swapped', 'clamp_1e-6')


def bits_equal(a, b):
    """Same 32 bits wherever neither is a NaN, NaN exactly where the other is; returns (ok, flat index of the first difference)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    ai = np.where(a != a, np.int32(0x7fc00000), a.view(np.int32))
    bi = np.where(b != b, np.int32(0x7fc00000), b.view(np.int32))
    bad = np.flatnonzero(ai.ravel() != bi.ravel())
    return bad.size == 0, (int(bad[0]) if bad.size else -1), int(bad.size)
