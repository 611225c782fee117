# -*- coding: utf-8 -*-
"""numpy restatements of the gradient of the decoder tail (rmnet_amd/csrc/soft_aggregate_bwd.hip, include/rmnet_hip.h:
rmnet_soft_aggregate_bwd_f32), the error bound of its fp32 arithmetic, and the cases tests/test_tail_backward.py shares between its
CPU and GPU halves.  No torch, no GPU.

The steps (per clip b with n = min(count, K - 1) objects, per output pixel; P the saved probabilities, g = d loss / d P, q = d loss /
d logit, either may be absent):
    s    = sum_k P_k g_k        over all K channels, in channel order (s = P_0 g_0, then s = s + P_k g_k)
    dl_k = P_k (g_k - s) + q_k  (q_k alone without g)
    live_k = k <= n and action[b][k] == 0;  pass(e) = lo <= e <= hi, lo = fl32(1e-7), hi = fl32(1 - lo); false for a NaN
    a0   = live_0 and pass(bg) ? dl_0 / (1 - bg) : 0        with bg = ((1 (1 - p_0)) (1 - p_1)) ...
    dz_o = (live_{o+1} and pass(p_o) ? dl_{o+1} : 0) - a0 p_o
    grad_dec[o, 1] = dz_o, grad_dec[o, 0] = -dz_o;  +0.0 in the padding and for the objects o >= n of the clip
tail_backward(dtype=float64) is this, literally; tail_backward(dtype=float32) rounds every operation once, in the kernel's order
(the kernel is compiled with fp contract(off)), and takes p_o as an input (``p_in``) where the caller has the device's: the only
thing the host cannot reproduce is the device's expf.

The bound (tail_backward_bound)
-------------------------------
u = 2^-24, eps = 2^-23, E = glue_ref.E_ULP: twice the largest error of the device's expf measured on the arguments these cases
produce (tools/ubench/math_ulp.hip, profiles/r14_a_glue_tests.md).  P, g, q and dec are the kernel's inputs: exact.  With d =
|z1 - z0|, from glue_ref's derivation (steps 1-4 there):
  p.  rel(p_o) <= r_o = 2 E eps + d u + 2 u;   a_o = p_o r_o its absolute error
  bg. every factor 1 - p_o has relative error a_o / (1 - p_o) + u and every product rounds once more:
      rel(bg) <= R = sum_o (a_o / (1 - p_o) + 2 u)
  s.  K products (one rounding each) and K - 1 additions:  |s^ - s| <= e_s = K u sum_k |P_k g_k|
  dl. t1 = g_k - s^: e_s + u |g_k - s|;  t2 = P_k t1: P_k e_s + 2 u P_k |g_k - s|;  + q_k: one more rounding, u |dl_k|
      e_k = P_k e_s + 2 u P_k |g_k - s| + u |dl_k|          (0 without g: dl_k = q_k is a copy)
  a0. 1 - bg^ has absolute error bg R + u (1 - bg); the quotient rounds once:
      e_a = e_0 / (1 - bg) + |a0| (bg R / (1 - bg) + 2 u)
  dz. the product a0 p_o: e_a p_o + |a0| p_o (r_o + u);  the difference: u |dz_o|
      |dz^_o - dz_o| <= m_{o+1} e_{o+1} + m_0 (e_a p_o + |a0| p_o (r_o + u)) + u |dz_o|
with m the masks.  First-order terms only; every bound is multiplied by glue_ref.SLACK = 1 + 1e-3 for the products of two of
them.  The masks of the fp32 and the float64 evaluation are the same wherever no em lies at a clamp edge, which the cases
guarantee and ``clamp_margin_ok`` checks: 0 pixels are excused.  1 - bg is a cancellation when every p_o is small (d = 12: p_o =
6e-6, bg R / (1 - bg) reaches 2 n u / 6e-6 = 0.02 n), so the bound on a0 is wide there; a0 only enters multiplied by p_o <= 1 - bg.
"""

import numpy as np

import glue_ref as G

F32 = np.float32
U, EPS, SLACK = G.U, G.EPS, G.SLACK
CLAMP_LO, CLAMP_HI = G.CLAMP_LO, G.CLAMP_HI
K_THREADS, MAX_CHUNKS = 256, 1024            # soft_aggregate_bwd.hip: kThreads, kMaxChunks

MUTANTS = ('s_live_only', 'edited_passed', 'obj_mask_ignored', 'bg_mask_ignored', 'z0_sign', 'pads_swapped', 'next_clip_begin',
           'cap_ignored', 'p1p_extra', 'padding_unwritten', 'stride_ignored')


def begin_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def window(pad, Hp, Wp):
    lw, uw, lh, uh = pad
    return lw, lh, Hp - lh - uh, Wp - lw - uw


def fg_prob(dec, dtype):
    """p [n_tot, Hp, Wp] in ``dtype`` arithmetic: the forward's fg_prob (epilogue.hip) on every padded pixel."""
    z = np.asarray(dec, dtype)
    with np.errstate(all='ignore'):
        m = np.maximum(z[:, 0], z[:, 1])
        e0, e1 = np.exp(z[:, 0] - m).astype(dtype), np.exp(z[:, 1] - m).astype(dtype)
        return e1 / (e0 + e1)


def _ignore_stride(view):
    """What a kernel that took the batch stride for K*H*W would read as clip b of ``view`` = x[:, t] of a [B,N,K,H,W] buffer."""
    B = view.shape[0]
    inner = view[0].size * view.itemsize
    return np.lib.stride_tricks.as_strided(view[0], shape=view.shape, strides=(inner,) + view[0].strides, writeable=False) if B > 1 else view


def tail_backward(dec, obj_begin, K, pad_l, pad_t, H, W, prob, grad_prob=None, grad_logit=None, action=None, dtype=np.float64, p_in=None,
                  mutant=None, out=None, detail=False):
    """grad_dec [n_tot, 2, Hp, Wp] in ``dtype`` arithmetic.  ``out``: the buffer to write into (so that a caller can show which
    elements are written); default zeros.  detail: also the per-clip intermediates the bound needs."""
    assert grad_prob is not None or grad_logit is not None
    dec = np.asarray(dec)
    n_tot, _, Hp, Wp = dec.shape
    B = len(obj_begin) - 1
    lo, hi, one, zero = dtype(CLAMP_LO), dtype(CLAMP_HI), dtype(1.0), dtype(0.0)
    p_all = fg_prob(dec, dtype) if p_in is None else np.asarray(p_in, dtype)
    if out is None:
        out = np.zeros((n_tot, 2, Hp, Wp), dtype)
    if mutant == 'pads_swapped':
        pad_l, pad_t = pad_t, pad_l
    if mutant == 'stride_ignored':
        prob = _ignore_stride(prob)
        grad_prob = None if grad_prob is None else _ignore_stride(grad_prob)
        grad_logit = None if grad_logit is None else _ignore_stride(grad_logit)
    ys, xs = slice(pad_t, pad_t + H), slice(pad_l, pad_l + W)
    passes = lambda e: (e >= lo) & (e <= hi)
    det = []
    with np.errstate(all='ignore'):
        for b in range(B):
            o0, cnt = int(obj_begin[b]), int(obj_begin[b + 1]) - int(obj_begin[b])
            n = cnt if mutant == 'cap_ignored' else min(cnt, K - 1)
            if mutant != 'padding_unwritten':
                out[o0:o0 + cnt] = zero
            r0 = int(obj_begin[b + 1]) % max(n_tot, 1) if mutant == 'next_clip_begin' else o0
            P = np.asarray(prob[b], dtype)
            g = None if grad_prob is None else np.asarray(grad_prob[b], dtype)
            q = None if grad_logit is None else np.asarray(grad_logit[b], dtype)
            act = np.zeros(K, np.uint8) if action is None else np.asarray(action[b])
            live = [k <= n and (mutant == 'edited_passed' or act[k] == 0) for k in range(K)] + [False] * max(n + 1 - K, 0)
            s = np.zeros((H, W), dtype)
            if g is not None:
                for k in range(K):
                    if mutant == 's_live_only' and not live[k]:
                        continue
                    s = P[k] * g[k] if k == 0 else s + P[k] * g[k]

            def dl(k):
                if k >= K:
                    return np.zeros((H, W), dtype)
                if g is None:
                    return q[k]
                t = P[k] * (g[k] - s)
                return t if q is None else t + q[k]

            ps = [p_all[(r0 + o) % n_tot][ys, xs] for o in range(n)]
            bg = np.ones((H, W), dtype)
            for p in ps:
                bg = bg * (one - p)
            m0 = (passes(bg) | (mutant == 'bg_mask_ignored')) & live[0]
            dl0 = dl(0)
            a0 = np.where(m0, dl0 / (one - bg), zero)
            dzs, ms, dls = [], [], []
            for o, p in enumerate(ps):
                mk = (passes(p) | (mutant == 'obj_mask_ignored')) & live[o + 1]
                dlk = dl(o + 1)
                dz = np.where(mk, dlk, zero) - a0 * p
                if mutant == 'p1p_extra':
                    dz = dz * (p * (one - p))
                out[o0 + o, 1][ys, xs] = dz
                out[o0 + o, 0][ys, xs] = dz if mutant == 'z0_sign' else -dz
                dzs.append(dz), ms.append(mk), dls.append(dlk)
            det.append(dict(n=n, o0=o0, p=ps, bg=bg, s=s, a0=a0, m0=m0, dl0=dl0, dz=dzs, m=ms, dl=dls, P=P, g=g, q=q))
    return (out, det) if detail else out


def tail_backward_f32(dec, obj_begin, K, pad_l, pad_t, H, W, prob, grad_prob=None, grad_logit=None, action=None, p_in=None, mutant=None,
                      out=None):
    return tail_backward(dec, obj_begin, K, pad_l, pad_t, H, W, prob, grad_prob, grad_logit, action, F32, p_in, mutant, out)


def tail_backward_bound(dec, obj_begin, K, pad_l, pad_t, H, W, prob, grad_prob=None, grad_logit=None, action=None, E=None):
    """(grad_dec in float64, bound) for every element of [n_tot, 2, Hp, Wp]: the module docstring's derivation.  The bound of an
    element that must be an exact +0.0 (padding, beyond the cap) is 0."""
    E = G.E_ULP if E is None else E
    ref, det = tail_backward(dec, obj_begin, K, pad_l, pad_t, H, W, prob, grad_prob, grad_logit, action, np.float64, detail=True)
    bound = np.zeros_like(ref)
    ys, xs = slice(pad_t, pad_t + H), slice(pad_l, pad_l + W)
    d_all = np.abs(np.asarray(dec, np.float64)[:, 1] - np.asarray(dec, np.float64)[:, 0])
    for d in det:
        n, o0, P, g, q, s = d['n'], d['o0'], d['P'], d['g'], d['q'], d['s']
        if g is not None:
            e_s = K * U * np.abs(P * g).sum(axis=0)

            def e_dl(k, dlk):
                return P[k] * e_s + 2 * U * P[k] * np.abs(g[k] - s) + (U * np.abs(dlk) if q is not None else 0.0)
        else:
            def e_dl(k, dlk):
                return np.zeros_like(dlk)
        r = [2 * E * EPS + d_all[o0 + o][ys, xs] * U + 2 * U for o in range(n)]
        with np.errstate(all='ignore'):
            R = sum((p * ro / (1.0 - p) + 2 * U for p, ro in zip(d['p'], r)), np.zeros_like(d['bg']))
            one_bg = 1.0 - d['bg']
            e_a = np.where(d['m0'], e_dl(0, d['dl0']) / one_bg + np.abs(d['a0']) * (d['bg'] * R / one_bg + 2 * U), 0.0)
        for o in range(n):
            p = d['p'][o]
            e = np.where(d['m'][o], e_dl(o + 1, d['dl'][o]), 0.0) + e_a * p + np.abs(d['a0']) * p * (r[o] + U) + U * np.abs(d['dz'][o])
            bound[o0 + o, 0][ys, xs] = bound[o0 + o, 1][ys, xs] = SLACK * e
    return ref, bound


def clamp_margin_ok(dec, obj_begin, K, pad_l, pad_t, H, W, rel=1e-3):
    """(ok, number of offending values): in float64, no em of the case -- an object's p or a clip's bg, inside the window -- lies
    within a relative ``rel`` of a clamp edge: |em - 1e-7| > rel * 1e-7 and |(1 - em) - 1e-7| > rel * 1e-7 (the upper edge is
    measured where the logit is, on 1 - em).  NaNs are not at an edge."""
    p_all = fg_prob(dec, np.float64)
    ys, xs = slice(pad_t, pad_t + H), slice(pad_l, pad_l + W)
    edge = float(CLAMP_LO)
    bad = 0
    for b in range(len(obj_begin) - 1):
        o0, n = int(obj_begin[b]), min(int(obj_begin[b + 1]) - int(obj_begin[b]), K - 1)
        ems = [p_all[o0 + o][ys, xs] for o in range(n)]
        bg = np.ones((H, W))
        for p in ems:
            bg = bg * (1.0 - p)
        for em in ems + [bg]:
            with np.errstate(invalid='ignore'):
                bad += int(((np.abs(em - edge) <= rel * edge) | (np.abs((1.0 - em) - (1.0 - float(CLAMP_HI))) <= rel * edge)).sum())
    return bad == 0, bad


# ------------------------------------------------------------------------------------------------ inputs
def random_dec(counts, Hp, Wp, seed, far=0.15, span=12.0):
    """Decoder logits [n_tot,2,Hp,Wp]: |z1 - z0| <= span, and on a share ``far`` of the (object, pixel) pairs 20 <= |z1 - z0| <= 30
    (clamped high or low with a wide margin).  A pixel whose bg would come near a clamp edge gets z1 = z0 in all its objects."""
    rng = np.random.default_rng(seed)
    n = int(sum(counts))
    z0 = (rng.standard_normal((n, Hp, Wp)) * 3.0).astype(F32)
    d = rng.uniform(-span, span, (n, Hp, Wp))
    big = rng.random((n, Hp, Wp)) < far
    d = np.where(big, np.sign(d) * rng.uniform(20.0, 30.0, (n, Hp, Wp)), d).astype(F32)
    dec = np.stack([z0, z0 + d], axis=1).astype(F32)
    begin = begin_of(counts)
    for b, c in enumerate(counts):
        o0 = int(begin[b])
        if c == 0:
            continue
        p = fg_prob(dec[o0:o0 + c], np.float64)
        bg = np.prod(1.0 - p, axis=0)
        near = (np.abs(bg - 1e-7) <= 1e-2 * 1e-7) | (np.abs((1.0 - bg) - 1e-7) <= 1e-2 * 1e-7)
        dec[o0:o0 + c, 1] = np.where(near[None], dec[o0:o0 + c, 0], dec[o0:o0 + c, 1])
    return dec


def random_probs(rng, B, K, H, W):
    """A soft-max of random logits, fp32: what a forward could have saved."""
    l = rng.standard_normal((B, K, H, W)) * 3.0
    e = np.exp(l - l.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F32)


def exact_inputs(counts, K, Hp, Wp, pad, seed):
    """The exact family: z1 - z0 in {0, +200, -200} (glue_ref.structural_dec: p in {1/2, 1, 0} exactly, on the host and on the
    device), P multiples of 1/16 in [0, 1], g and q multiples of 1/4 with |.| <= 2: every product, sum and difference of the steps
    up to dl_k is exact in fp32; the quotient dl_0 / (1 - bg) (1 - bg = 3/4, 7/8, ...) and the difference that follows it can round, each
    once and IEEE-correctly on both sides: the fp32 restatement is a bit-for-bit oracle for this family."""
    rng = np.random.default_rng(seed)
    lw, lh, H, W = window(pad, Hp, Wp)
    B = len(counts)
    dec = G.structural_dec(int(sum(counts)), Hp, Wp, seed=seed)
    P = (rng.integers(0, 17, (B, K, H, W)) / 16.0).astype(F32)
    g = (rng.integers(-8, 9, (B, K, H, W)) / 4.0).astype(F32)
    q = (rng.integers(-8, 9, (B, K, H, W)) / 4.0).astype(F32)
    return dec, P, g, q


def plan_of(Hp, Wp, W, pad_l, aligned16=True, p_aligned16=True, strides=(0,)):
    """(V, PV, chunks): the launcher's lane form and grid for a padded plane (soft_aggregate_bwd.hip)."""
    vec = Wp % 4 == 0 and aligned16
    pvec = vec and W % 4 == 0 and pad_l % 4 == 0 and p_aligned16 and all(s % 4 == 0 for s in strides)
    per_block = K_THREADS * (4 if vec else 1)
    return (4 if vec else 1), pvec, min(-(-(Hp * Wp) // per_block), MAX_CHUNKS)
