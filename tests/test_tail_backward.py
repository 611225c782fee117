# -*- coding: utf-8 -*-
"""The gradient of the decoder tail (csrc/soft_aggregate_bwd.hip, ops.soft_aggregate under autograd, RMNet.decoder_tail).

CPU: the float64 restatement of tests/tail_backward_ref.py against hand-written pixels, torch autograd through the module graph and
gradcheck; the fp32 restatement inside the derived bound; the clamp margin of every case the GPU tests use; planted faults; the C
entry's refusals.  GPU: exact families bit for bit, the random family inside the bound, autograd, the loss head end to end, the
refusals with guarded buffers, the compiler's resources."""

import ctypes
import math

import numpy as np
import pytest
import torch

import glue_ref as G
import tail_backward_ref as R

gpu = pytest.mark.gpu
F32 = np.float32
NAN = float('nan')
SENT = 12345.0
E_INVALID, E_UNSUPPORTED = -1, -4


def dev():
    return torch.device('cuda', torch.cuda.current_device())


# ================================================================================================ cases
# name -> (objects per clip, K, Hp, Wp, (lw, uw, lh, uh), action rows | None, strided)
EXACT_CASES = {
    'no pad, one object, K 2': ([1], 2, 16, 16, (0, 0, 0, 0), None, False),
    'pads 1 2 3 0, clips of 2 / 0 / 3 objects, K 4, every action': ([2, 0, 3], 4, 16, 32, (1, 2, 3, 0), [[0, 1, 0, 0], [2, 0, 1, 0], [0, 0, 2, 1]], False),
    'over the cap: 4 and 1 objects, K 3, pads 0 3 0 1': ([4, 1], 3, 16, 16, (0, 3, 0, 1), [[0, 0, 1], [0, 0, 0]], False),
    'batch-strided slices, clips of 1 / 2 objects, K 3': ([1, 2], 3, 16, 16, (0, 0, 0, 0), None, True),
    'edited background, pads 1 2 3 0, 16 x 16': ([2], 3, 16, 16, (1, 2, 3, 0), [[2, 0, 0]], False),
}
# name -> (objects per clip, K, Hp, Wp, pad, action rows | None, which gradients, strided, dec offset in floats)
RANDOM_CASES = {
    '1 object, K 2, 16 x 16, no pad, both': ([1], 2, 16, 16, (0, 0, 0, 0), None, 'both', False, 0),
    '2 objects, K 4, 16 x 32, pads 1 2 3 0, grad_prob': ([2], 4, 16, 32, (1, 2, 3, 0), None, 'prob', False, 0),
    'clips of 0 / 5 / 2 objects, K 6, pads 0 3 0 1, grad_logit, actions': ([0, 5, 2], 6, 16, 16, (0, 3, 0, 1), [[0] * 6, [0, 0, 1, 0, 2, 0], [1, 0, 0, 0, 0, 0]], 'logit', False, 0),
    'over the cap: 3 and 1 objects, K 3, 16 x 32, both': ([3, 1], 3, 16, 32, (1, 2, 3, 0), None, 'both', False, 0),
    'clips of 1 / 1 objects, K 4 (n + 3), grad_prob': ([1, 1], 4, 16, 16, (0, 0, 0, 0), None, 'prob', False, 0),
    'K 255, 2 objects, pads 0 3 0 1, grad_prob': ([2], 255, 16, 16, (0, 3, 0, 1), None, 'prob', False, 0),
    'batch-strided slices 4 bytes off, clips of 2 / 1 / 1, K 3, both': ([2, 1, 1], 3, 16, 16, (0, 0, 0, 0), None, 'both', True, 0),
    'dec 4 bytes off a 16-byte boundary (one-pixel lanes), K 3, both': ([2], 3, 16, 16, (1, 2, 3, 0), None, 'both', False, 1),
    'second grid-stride iteration of one-pixel lanes': ([1], 2, 520, 513, (1, 0, 7, 0), None, 'prob', False, 0),
}
E2E = dict(counts=[2], K=3, H=16, W=32, frames=3, seed=77)


def _inputs(name, family):
    """(dec, begin, K, (lw, lh, H, W), P, g, q, action, strided, dec_off) of a case; g / q None where the case gives none."""
    if family == 'exact':
        counts, K, Hp, Wp, pad, action, strided = EXACT_CASES[name]
        mode, off = 'both', 0
        seed = 1 + list(EXACT_CASES).index(name)
        dec, P, g, q = R.exact_inputs(counts, K, Hp, Wp, pad, seed)
    else:
        counts, K, Hp, Wp, pad, action, mode, strided, off = RANDOM_CASES[name]
        seed = 100 + list(RANDOM_CASES).index(name)
        lw, lh, H, W = R.window(pad, Hp, Wp)
        rng = np.random.default_rng(seed)
        dec = R.random_dec(counts, Hp, Wp, seed)
        P = R.random_probs(rng, len(counts), K, H, W)
        g = rng.standard_normal(P.shape).astype(F32)
        q = rng.standard_normal(P.shape).astype(F32)
    act = None if action is None else np.array(action, np.uint8)
    return dec, R.begin_of(counts), K, R.window(pad, Hp, Wp), P, (g if mode != 'logit' else None), (q if mode != 'prob' else None), act, strided, off


def _strided(x):
    """x [B,K,H,W] as the slice [:, 1] of a [B,3,K,H,W] array whose other slices hold the sentinel."""
    buf = np.full((x.shape[0], 3) + x.shape[1:], SENT, x.dtype)
    buf[:, 1] = x
    return buf[:, 1]


def _within(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err == 0, 0.0, np.inf))
    return not bool(bad.any()), float(np.nanmax(ratio)) if ratio.size else 0.0, int(bad.sum())


def _assert_bits(got, want, what):
    ok, first, count = G.bits_equal(got, want)
    assert ok, '%s: %d elements differ, first at flat index %d: got %r, want %r' % (what, count, first, got.ravel()[first], want.ravel()[first])


# ================================================================================================ CPU 1: the float64 restatement
def _pixel(z, K, P, g, counts=None, action=None, q=None):
    """grad_dec of clips of 1 x 1 pixels: z [n_tot][2], P / g [B][K] -> float64 [n_tot, 2]."""
    counts = [len(z)] if counts is None else counts
    B = len(counts)
    dec = np.array(z, np.float64).reshape(len(z), 2, 1, 1)
    arr = lambda v: None if v is None else np.array(v, np.float64).reshape(B, K, 1, 1)
    act = None if action is None else np.array(action, np.uint8).reshape(B, K)
    return R.tail_backward(dec, R.begin_of(counts), K, 0, 0, 1, 1, arr(P), arr(g), arr(q), act)[:, :, 0, 0]


def test_the_float64_restatement_on_hand_written_pixels():
    ln3 = math.log(3.0)                                   # p = 3/4, bg = 1/4
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-15)
    # one object, unclamped: logit_1 = d and logit_0 = -d with d = z1 - z0, so dz = dl_1 - dl_0 = -3/16 - 3/16
    assert close(_pixel([[0, ln3]], 2, [[0.25, 0.75]], [[1, 0]]), [[0.375, -0.375]])
    # clamped high: p = 1 - 1.4e-11 and bg = 1.4e-11 both fail the clamp
    assert np.array_equal(_pixel([[0, 25]], 2, [[0.25, 0.75]], [[1, 0]]), [[0, 0]])
    # clamped low: p = 1.4e-11, bg = 1 - 1.4e-11
    assert np.array_equal(_pixel([[0, -25]], 2, [[0.25, 0.75]], [[1, 0]]), [[0, 0]])
    # two objects, bg = (4.5e-5)^2 clamped, the objects pass: s = 2.3, dz = (dl_1, dl_2) = (0.3 (2 - 2.3), 0.5 (3 - 2.3))
    assert close(_pixel([[0, 10], [0, 10]], 3, [[0.2, 0.3, 0.5]], [[1, 2, 3]])[:, 1], [-0.09, 0.35])
    # n = 0: an empty clip in front of the first case changes nothing and owns nothing
    assert close(_pixel([[0, ln3]], 2, [[0.5, 0.5], [0.25, 0.75]], [[7, 9], [1, 0]], counts=[0, 1]), [[0.375, -0.375]])
    # an absent channel takes part in s: s = 2.3, dl_0 = 0.2 (1 - 2.3), dl_1 = -0.09, dz = dl_1 - dl_0
    assert close(_pixel([[0, ln3]], 3, [[0.2, 0.3, 0.5]], [[1, 2, 3]])[:, 1], [0.17])
    # action 1 on the object's channel: only the background path is left, dz = -dl_0
    assert close(_pixel([[0, ln3]], 3, [[0.2, 0.3, 0.5]], [[1, 2, 3]], action=[[0, 1, 0]])[:, 1], [0.26])
    # action 2 on the background: only the object's own path is left, dz = dl_1
    assert close(_pixel([[0, ln3]], 3, [[0.2, 0.3, 0.5]], [[1, 2, 3]], action=[[2, 0, 0]])[:, 1], [-0.09])
    # over the cap: K = 2 keeps one object of two; the second gets exactly 0 and does not enter bg
    got = _pixel([[0, ln3], [0, 5]], 2, [[0.25, 0.75]], [[1, 0]])
    assert close(got[0], [0.375, -0.375]) and np.array_equal(got[1], [0, 0]) and not np.signbit(got[1]).any()
    # grad_logit alone is passed on: dz = q_1 - q_0
    assert close(_pixel([[0, ln3]], 2, [[0.25, 0.75]], None, q=[[0.5, 2.0]])[:, 1], [1.5])


def _module_graph(dec, counts, K, pad, action, g, q, dtype=torch.float64):
    """grad of sum(prob * g) + sum(logit * q) through RMNet.decoder_tail on the CPU: the literal module graph."""
    from rmnet_amd.rmnet import RMNet
    net = RMNet(None).train()
    d = torch.tensor(np.asarray(dec), dtype=dtype, requires_grad=True)
    edit = None
    if action is not None:
        B = len(counts)
        edit = (None, torch.zeros(B, 256, dtype=torch.uint8), torch.from_numpy(np.asarray(action, np.uint8)))
    logit, prob = net.decoder_tail(d, counts, K, pad, edit)
    loss = (prob * torch.tensor(g, dtype=dtype)).sum() + (logit * torch.tensor(q, dtype=dtype)).sum()
    loss.backward()
    return d.grad.numpy(), prob.detach().numpy(), logit.detach().numpy()


@pytest.mark.parametrize('counts,K,pad,action', [([2], 3, (1, 2, 3, 0), None), ([1, 0, 3], 5, (0, 3, 0, 1), [[0, 1, 0, 0, 0], [0, 0, 0, 0, 0], [2, 0, 1, 0, 2]]),
                                                   ([2, 1], 3, (0, 0, 0, 0), [[2, 0, 0], [0, 2, 0]])])
def test_the_float64_restatement_is_torch_autograd_through_the_module_graph(counts, K, pad, action):
    Hp, Wp = 10, 12
    lw, lh, H, W = R.window(pad, Hp, Wp)
    rng = np.random.default_rng(K)
    dec = R.random_dec(counts, Hp, Wp, seed=K)
    g, q = rng.standard_normal((len(counts), K, H, W)), rng.standard_normal((len(counts), K, H, W))
    want, prob, _ = _module_graph(dec, counts, K, pad, action, g, q)
    assert R.clamp_margin_ok(dec, R.begin_of(counts), K, lw, lh, H, W)[0]
    got = R.tail_backward(dec, R.begin_of(counts), K, lw, lh, H, W, prob, g, q, None if action is None else np.array(action, np.uint8))
    assert np.abs(want).max() > 0.1 and (want == 0).any()               # live gradients, and zeros (padding, clamped pixels)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)


def test_gradcheck_of_the_module_graph_away_from_the_clamp_edges():
    from rmnet_amd.rmnet import RMNet
    net = RMNet(None).train()
    rng = np.random.default_rng(5)
    z = torch.tensor(rng.uniform(-2.0, 2.0, (3, 2, 4, 5)), dtype=torch.float64, requires_grad=True)

    def f(d):
        logit, prob = net.decoder_tail(d, [2, 1], 3, (1, 0, 0, 1))
        return logit, prob
    assert torch.autograd.gradcheck(f, (z,), eps=1e-6, atol=1e-7)


def test_a_nan_in_dec_is_what_torch_makes_of_it():
    """One NaN in one object of a two-object clip: torch's autograd through the module graph gives a NaN to BOTH objects at that
    pixel (the soft-max over K spreads it) and leaves every other pixel alone; so does the restatement, and with it the kernel."""
    counts, K, pad, Hp, Wp = [2], 3, (1, 0, 0, 1), 6, 7
    lw, lh, H, W = R.window(pad, Hp, Wp)
    rng = np.random.default_rng(3)
    dec = R.random_dec(counts, Hp, Wp, seed=3, far=0.0)
    dec[1, 0, 2, 4] = NAN
    g, q = rng.standard_normal((1, K, H, W)), np.zeros((1, K, H, W))
    want, prob, _ = _module_graph(dec, counts, K, pad, None, g, q)
    got = R.tail_backward(dec, R.begin_of(counts), K, lw, lh, H, W, prob, g, None, None)
    nan = np.zeros_like(want, bool)
    nan[:, :, 2, 4] = True
    assert np.array_equal(np.isnan(want), nan) and np.array_equal(np.isnan(got), nan)
    np.testing.assert_allclose(got[~nan], want[~nan], rtol=1e-9, atol=1e-12)
    got32 = R.tail_backward_f32(dec, R.begin_of(counts), K, lw, lh, H, W, prob.astype(F32), g.astype(F32))
    assert np.array_equal(np.isnan(got32), nan)


# ================================================================================================ CPU 2: the fp32 restatement and the bound
@pytest.mark.parametrize('name', [n for n in RANDOM_CASES if 'grid-stride' not in n])
def test_the_fp32_restatement_is_inside_the_bound_around_float64(name):
    dec, begin, K, (lw, lh, H, W), P, g, q, act, _, _ = _inputs(name, 'random')
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, P, g, q, act)
    got = R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act)
    ok, ratio, bad = _within(got, ref, bound)
    print('TAIL cpu %-70s largest error / bound %.3f, largest bound %.3g, largest |grad| %.3g' % (name, ratio, bound.max(), np.abs(ref).max()))
    assert ok, (name, ratio, bad)
    assert ratio > 0.02 and np.abs(ref).max() > 0.1          # (the restatement uses a real share of the bound)


def test_the_bound_is_not_vacuous():
    """A p that is 64 u off, a division replaced by one that is 16 ulp off, or an s that drops one channel leave the bound."""
    name = '2 objects, K 4, 16 x 32, pads 1 2 3 0, grad_prob'
    dec, begin, K, (lw, lh, H, W), P, g, q, act, _, _ = _inputs(name, 'random')
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, P, g, q, act)
    p32 = R.fg_prob(dec, F32)
    assert _within(R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act, p_in=p32), ref, bound)[0]
    off = R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act, p_in=p32 * F32(1 + 64 * G.U))
    assert not _within(off, ref, bound)[0]
    good = R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act)
    assert not _within(good * F32(1 + 16 * G.EPS), ref, bound)[0]
    assert not _within(R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act, mutant='s_live_only'), ref, bound)[0]
    assert float(np.median(bound[bound > 0] / np.abs(ref[bound > 0]).clip(1e-30))) < 1e-5     # a few 1e-7 of the values, not a tolerance


# ================================================================================================ CPU 3: away from the clamp edges
def _e2e_inputs():
    rng = np.random.default_rng(E2E['seed'])
    decs = [R.random_dec(E2E['counts'], E2E['H'], E2E['W'], E2E['seed'] + t, far=0.0, span=6.0) for t in range(E2E['frames'])]
    labels = rng.integers(0, E2E['K'], (E2E['frames'], E2E['H'], E2E['W'])).astype(np.uint8)
    return decs, labels


def test_no_case_of_the_gpu_tests_has_an_em_at_a_clamp_edge():
    """0 pixels are excused for a clamp mask that differs between fp32 and float64: no em within a relative 1e-3 of an edge."""
    for name in RANDOM_CASES:
        dec, begin, K, (lw, lh, H, W), *_ = _inputs(name, 'random')
        d = np.abs(dec[:, 1].astype(np.float64) - dec[:, 0])
        assert ((d <= 12.0 + 1e-5) | (d >= 20.0 - 1e-5)).all(), name
        assert R.clamp_margin_ok(dec, begin, K, lw, lh, H, W) == (True, 0), name
    for name in EXACT_CASES:
        dec, begin, K, (lw, lh, H, W), *_ = _inputs(name, 'exact')
        assert R.clamp_margin_ok(dec, begin, K, lw, lh, H, W) == (True, 0), name
    for dec in _e2e_inputs()[0]:
        assert R.clamp_margin_ok(dec, R.begin_of(E2E['counts']), E2E['K'], 0, 0, E2E['H'], E2E['W']) == (True, 0)


# ================================================================================================ CPU 4: planted faults
def _fails(name, family, mutant):
    """Does the comparison the GPU test of this case makes reject the fp32 restatement with this fault?"""
    dec, begin, K, (lw, lh, H, W), P, g, q, act, strided, _ = _inputs(name, family)
    if strided:
        P, g, q = _strided(P), (None if g is None else _strided(g)), (None if q is None else _strided(q))
    out = np.full(dec.shape, NAN, F32)
    got = R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act, mutant=mutant, out=out)
    if family == 'exact':
        return not G.bits_equal(got, R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act))[0]
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, P, g, q, act)
    return not _within(got, ref, bound)[0]


def test_every_planted_fault_fails_a_named_case():
    missed = []
    for m in R.MUTANTS:
        hit = [(f, n) for f, cases in (('exact', EXACT_CASES), ('random', RANDOM_CASES)) for n in cases if 'grid-stride' not in n and _fails(n, f, m)]
        print('MUTANT %-20s %s' % (m, 'caught by %d cases, first: %s "%s"' % (len(hit), hit[0][0], hit[0][1]) if hit else 'MISSED'))
        if not hit:
            missed.append(m)
        assert not any(_fails(n, f, None) for f, n in hit[:1])            # (the unmutated restatement passes the same comparison)
    assert not missed, missed


# ================================================================================================ CPU 5 / GPU 5: the entry's refusals
ORDER = ['dec', 'begin', 'B', 'K', 'Hp', 'Wp', 'pad_l', 'pad_t', 'H', 'W', 'prob', 'prob_bs', 'gp', 'gp_bs', 'gl', 'gl_bs', 'action', 'grad_dec']


def _refusals(good):
    khw = good['K'] * good['H'] * good['W']
    big = 1 << 31
    cases = [('no %s' % n, {n: None}, E_INVALID) for n in ('dec', 'begin', 'prob', 'grad_dec')]
    cases += [('both gradients NULL', dict(gp=None, gl=None), E_INVALID)]
    cases += [('%s 2 bytes off' % n, {n: good[n] + 2}, E_INVALID) for n in ('dec', 'begin', 'prob', 'gp', 'gl', 'grad_dec')]
    cases += [('%s %d' % (n, v), {n: v}, E_INVALID) for n in ('B', 'K', 'H', 'W') for v in (0, -1)]
    cases += [('K 256', dict(K=256, prob_bs=256 * khw, gp_bs=256 * khw, gl_bs=256 * khw), E_INVALID),
              ('pad_l -1', dict(pad_l=-1), E_INVALID), ('pad_t -1', dict(pad_t=-1), E_INVALID),
              ('pad_l + W = Wp + 1', dict(pad_l=good['Wp'] - good['W'] + 1), E_INVALID),
              ('pad_t + H = Hp + 1', dict(pad_t=good['Hp'] - good['H'] + 1), E_INVALID),
              ('W = Wp + 1 without padding', dict(pad_l=0, W=good['Wp'] + 1, prob_bs=big - 1, gp_bs=big - 1, gl_bs=big - 1), E_INVALID),
              ('prob stride K*H*W - 1', dict(prob_bs=khw - 1), E_INVALID), ('grad_prob stride K*H*W - 1', dict(gp_bs=khw - 1), E_INVALID),
              ('grad_logit stride K*H*W - 1', dict(gl_bs=khw - 1), E_INVALID),
              ('B 65536', dict(B=65536), E_UNSUPPORTED), ('prob stride 2^31', dict(prob_bs=big), E_UNSUPPORTED),
              ('grad_prob stride 2^31', dict(gp_bs=big), E_UNSUPPORTED), ('grad_logit stride 2^31', dict(gl_bs=big), E_UNSUPPORTED),
              ('(B - 1) stride + K*H*W = 2^31', dict(prob_bs=(big - khw) // (good['B'] - 1) + 1), E_UNSUPPORTED),
              ('2 Hp Wp = 2^31', dict(Hp=1 << 15, Wp=1 << 15), E_UNSUPPORTED)]
    return cases


def _call(lib, args):
    p = lambda v: ctypes.c_void_p(v) if v else None
    ptrs = ('dec', 'begin', 'prob', 'gp', 'gl', 'action', 'grad_dec')
    return lib.rmnet_soft_aggregate_bwd_f32(*([p(args[k]) if k in ptrs else args[k] for k in ORDER] + [None]))


def test_the_entry_refuses_malformed_calls_before_it_touches_the_device():
    """No GPU here: a call that got past the checks would fail to launch (RMNET_E_LAUNCH) or fault on these made-up addresses."""
    from rmnet_amd import _lib
    lib = _lib.load()
    good = dict(dec=0x10000, begin=0x20000, B=2, K=3, Hp=8, Wp=12, pad_l=2, pad_t=1, H=6, W=7, prob=0x30000, prob_bs=3 * 42 + 5, gp=0x40000,
                gp_bs=3 * 42, gl=0x50000, gl_bs=3 * 42 + 1, action=0x60000, grad_dec=0x70000)
    for name, kw, code in _refusals(good):
        assert _call(lib, dict(good, **kw)) == code, name


# ================================================================================================ GPU helpers
def _run_entry(dec, begin, K, win, P, g, q, act, strided=False, dec_off=0):
    """One call of the C entry with grad_dec pre-filled with NaN inside a sentinel pool; P / g / q as slices [:, 1] of [B,3,K,H,W]
    buffers that start 4 bytes off a 16-byte boundary when ``strided``.  Returns grad_dec; asserts that nothing else was written."""
    from rmnet_amd import _lib
    lib = _lib.load()
    d = dev()
    lw, lh, H, W = win
    B = len(begin) - 1
    n = dec.size
    Hp, Wp = dec.shape[2:]
    dec_pool = torch.full((n + 16,), SENT, device=d)
    out_pool = torch.full((n + 16,), SENT, device=d)
    lo = 4 + dec_off
    dec_pool[lo:lo + n] = torch.from_numpy(dec).to(d).flatten()
    out_pool[lo:lo + n] = NAN
    assert dec_pool.data_ptr() % 16 == 0 and out_pool.data_ptr() % 16 == 0
    t_begin = torch.from_numpy(begin).to(d)
    keep, ptr, bs = [], {}, {}
    for key, x in (('prob', P), ('gp', g), ('gl', q)):
        if x is None:
            ptr[key], bs[key] = None, 0
        elif strided:
            buf = torch.full((x.size * 3 + 16,), SENT, device=d)
            v = buf[5:5 + 3 * x.size].view(B, 3, *x.shape[1:])
            v[:, 1] = torch.from_numpy(x).to(d)
            keep.append((buf, v, torch.from_numpy(x)))
            ptr[key], bs[key] = v[:, 1].data_ptr(), v.stride(0)
            assert ptr[key] % 16 != 0
        else:
            t = torch.from_numpy(x).to(d)
            keep.append((t, None, None))
            ptr[key], bs[key] = t.data_ptr(), x[0].size
    t_act = None if act is None else torch.from_numpy(act).to(d)
    p = lambda v: ctypes.c_void_p(v) if v else None
    with torch.cuda.device(d):
        rc = lib.rmnet_soft_aggregate_bwd_f32(p(dec_pool.data_ptr() + 4 * lo), p(t_begin.data_ptr()), B, K, Hp, Wp, lw, lh, H, W, p(ptr['prob']), bs['prob'],
                                              p(ptr['gp']), bs['gp'], p(ptr['gl']), bs['gl'], p(t_act.data_ptr()) if act is not None else None,
                                              p(out_pool.data_ptr() + 4 * lo), ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    host = out_pool.cpu().numpy()
    assert (host[:lo] == SENT).all() and (host[lo + n:] == SENT).all(), 'grad_dec: a guard was written'
    assert (dec_pool.cpu().numpy()[lo:lo + n] == dec.ravel()).all() or np.isnan(dec).any()
    for buf, v, x in keep:
        if v is not None:                                 # the inputs and their neighbours are as they were
            assert bool((v[:, 0] == SENT).all()) and bool((v[:, 2] == SENT).all()) and np.array_equal(v[:, 1].cpu().numpy(), x.numpy(), equal_nan=True)
    return host[lo:lo + n].reshape(dec.shape)


# ================================================================================================ GPU 1: exact families
def _plus_zero(shape, begin, K, win):
    """The elements that must be an exact +0.0, sign included: the padding and the objects at or beyond the cap."""
    lw, lh, H, W = win
    pad = np.ones(shape, bool)
    pad[:, :, lh:lh + H, lw:lw + W] = False
    for b in range(len(begin) - 1):
        pad[int(begin[b]) + min(int(begin[b + 1] - begin[b]), K - 1):int(begin[b + 1])] = True
    return pad


@gpu
@pytest.mark.parametrize('mode', ['both', 'prob', 'logit'])
@pytest.mark.parametrize('name', list(EXACT_CASES))
def test_exact_family_every_bit_of_grad_dec(name, mode):
    dec, begin, K, win, P, g, q, act, strided, _ = _inputs(name, 'exact')
    g, q = (g if mode != 'logit' else None), (q if mode != 'prob' else None)
    lw, lh, H, W = win
    ch = G.structural_choice(dec, lw, lh, H, W)
    assert all(int((ch == v).sum()) > 0 for v in (0.0, 200.0, -200.0))
    want = R.tail_backward_f32(dec, begin, K, lw, lh, H, W, P, g, q, act)
    got = _run_entry(dec, begin, K, win, P, g, q, act, strided)
    _assert_bits(got, want, 'exact "%s", %s' % (name, mode))
    pad = _plus_zero(dec.shape, begin, K, win)
    assert (got[pad] == 0).all() and not np.signbit(got[pad]).any()
    assert (got != 0).any() and (got[~pad] == 0).any()


# ================================================================================================ GPU 2: the random family
@gpu
@pytest.mark.parametrize('name', list(RANDOM_CASES))
def test_random_family_every_element_inside_the_derived_bound(name):
    dec, begin, K, win, P, g, q, act, strided, off = _inputs(name, 'random')
    lw, lh, H, W = win
    Hp, Wp = dec.shape[2:]
    if 'grid-stride' in name:
        assert R.plan_of(Hp, Wp, W, lw) == (1, False, R.MAX_CHUNKS) and Hp * Wp > R.MAX_CHUNKS * R.K_THREADS
    if off or strided:
        assert R.plan_of(Hp, Wp, W, lw, aligned16=not off, p_aligned16=not strided)[:2] == ((1, False) if off else (4, False))
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, P, g, q, act)
    got = _run_entry(dec, begin, K, win, P, g, q, act, strided, off)
    ok, ratio, bad = _within(got, ref, bound)
    print('TAIL gpu %-70s largest error / bound %.3f' % (name, ratio))
    assert ok, (name, ratio, bad)
    pad = _plus_zero(dec.shape, begin, K, win)
    assert (bound[pad] == 0).all() and (got[pad] == 0).all() and not np.signbit(got[pad]).any()


@gpu
def test_a_nan_in_dec_gives_nan_at_its_pixel_and_nothing_anywhere_else():
    """The CPU case pinned against torch, on the device and through all three lane forms: a NaN in one object's logits at a window
    pixel makes both objects' gradients NaN there (never a finite value), a NaN in the padding changes nothing, every other element
    stays inside the bound."""
    counts, K, Hp, Wp, pad = [2], 3, 16, 16, (4, 0, 3, 0)
    lw, lh, H, W = R.window(pad, Hp, Wp)
    begin = R.begin_of(counts)
    rng = np.random.default_rng(12)
    dec = R.random_dec(counts, Hp, Wp, seed=12, far=0.0)
    dec[1, 0, lh + 2, lw + 5] = NAN
    dec[0, 1, 1, 1] = NAN                                 # padding
    _, P = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W)
    assert np.isnan(P[0, :, 2, 5]).all() and np.isnan(P).sum() == K
    g = rng.standard_normal(P.shape).astype(F32)
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, P, g)
    nan = np.zeros(dec.shape, bool)
    nan[:, :, lh + 2, lw + 5] = True
    assert np.array_equal(np.isnan(ref), nan)
    for strided, off in ((False, 0), (True, 0), (False, 1)):          # <4, true>, <4, false>, <1, false>
        assert R.plan_of(Hp, Wp, W, lw, aligned16=not off, p_aligned16=not strided)[:2] == ((1, False) if off else (4, not strided))
        got = _run_entry(dec, begin, K, (lw, lh, H, W), P, g, None, None, strided, off)
        assert np.array_equal(np.isnan(got), nan), (strided, off)
        assert _within(got[~nan], ref[~nan], bound[~nan])[0], (strided, off)


# ================================================================================================ GPU 3: autograd
def _edit_args(B, K, H, W, rng, d):
    labels = torch.from_numpy(rng.integers(0, K, (B, H, W)).astype(np.uint8)).to(d)
    lut = torch.arange(256, dtype=torch.uint8).repeat(B, 1).to(d)
    return labels, lut


@gpu
def test_autograd_through_ops_soft_aggregate():
    from rmnet_amd import ops
    d = dev()
    name = 'over the cap: 3 and 1 objects, K 3, 16 x 32, both'
    dec, begin, K, (lw, lh, H, W), P, g, q, _, _, _ = _inputs(name, 'random')
    pad = RANDOM_CASES[name][4]
    t_begin, tg, tq = torch.from_numpy(begin).to(d), torch.from_numpy(g).to(d), torch.from_numpy(q).to(d)
    plain = torch.from_numpy(dec).to(d)
    logit0, prob0 = ops.soft_aggregate(plain, t_begin, K, pad, want_prob=True)
    assert logit0.grad_fn is None and prob0.grad_fn is None and not logit0.requires_grad            # no graph without requires_grad
    leaf = plain.clone().requires_grad_(True)
    with torch.no_grad():
        l_ng, p_ng = ops.soft_aggregate(leaf, t_begin, K, pad, want_prob=True)
    assert l_ng.grad_fn is None and torch.equal(l_ng, logit0) and torch.equal(p_ng, prob0)
    logit, prob = ops.soft_aggregate(leaf, t_begin, K, pad, want_prob=True)
    assert torch.equal(logit, logit0) and torch.equal(prob, prob0)                                 # today's bits
    ((prob * tg).sum() + (logit * tq).sum()).backward()
    want = ops.soft_aggregate_backward(plain, t_begin, K, pad, prob0, tg, tq)
    assert torch.equal(leaf.grad, want) and bool((want != 0).any())
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, prob0.cpu().numpy(), g, q)
    assert _within(leaf.grad.cpu().numpy(), ref, bound)[0]
    # a non-leaf, and grad_output scaling (by a power of two: every product stays exact, the bits are 4 x the leaf's)
    leaf2 = plain.clone().requires_grad_(True)
    logit2, prob2 = ops.soft_aggregate(leaf2 * 1.0, t_begin, K, pad, want_prob=True)
    (4.0 * ((prob2 * tg).sum() + (logit2 * tq).sum())).backward()
    assert torch.equal(leaf2.grad, 4.0 * want)
    # logits only: the probabilities are computed inside, only grad_logit arrives
    leaf3 = plain.clone().requires_grad_(True)
    logit3, none = ops.soft_aggregate(leaf3, t_begin, K, pad)
    assert none is None and torch.equal(logit3, logit0)
    (logit3 * tq).sum().backward()
    assert torch.equal(leaf3.grad, ops.soft_aggregate_backward(plain, t_begin, K, pad, prob0, None, tq))
    # double backward is refused
    leaf4 = plain.clone().requires_grad_(True)
    _, prob4 = ops.soft_aggregate(leaf4, t_begin, K, pad, want_prob=True)
    first, = torch.autograd.grad((prob4 * tg).sum(), leaf4, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()


@gpu
def test_autograd_with_both_edit_actions():
    from rmnet_amd import ops
    d = dev()
    counts, K, Hp, Wp, pad = [2, 1], 4, 16, 32, (1, 2, 3, 0)
    lw, lh, H, W = R.window(pad, Hp, Wp)
    rng = np.random.default_rng(41)
    dec, begin = R.random_dec(counts, Hp, Wp, seed=41), R.begin_of(counts)
    action = np.array([[0, 0, 0, 2], [1, 0, 2, 0]], np.uint8)
    labels, lut = _edit_args(2, K, H, W, rng, d)
    g = rng.standard_normal((2, K, H, W)).astype(F32)
    t_begin, t_action, tg = torch.from_numpy(begin).to(d), torch.from_numpy(action).to(d), torch.from_numpy(g).to(d)
    leaf = torch.from_numpy(dec).to(d).requires_grad_(True)
    logit, prob = ops.soft_aggregate(leaf, t_begin, K, pad, want_prob=True, edit=(labels, lut, t_action))
    l0, p0 = ops.soft_aggregate(leaf.detach(), t_begin, K, pad, want_prob=True, edit=(labels, lut, t_action))
    assert torch.equal(logit, l0) and torch.equal(prob, p0) and l0.grad_fn is None
    inj = (labels[0] == 3).float() * 32.0605 - 16.1181
    assert torch.equal(logit[0, 3], inj) and bool((logit[1, 0] == -16.1181).all())
    (prob * tg).sum().backward()
    ref, bound = R.tail_backward_bound(dec, begin, K, lw, lh, H, W, prob.detach().cpu().numpy(), g, None, action)
    ok, ratio, bad = _within(leaf.grad.cpu().numpy(), ref, bound)
    assert ok, (ratio, bad)
    assert bool((leaf.grad[2] != 0).any())                # clip 1's object: its background is edited, its own channel is live


@gpu
def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from rmnet_amd import ops
    d = dev()
    name = 'clips of 0 / 5 / 2 objects, K 6, pads 0 3 0 1, grad_logit, actions'
    dec, begin, K, win, P, _, q, act, _, _ = _inputs(name, 'random')
    pad = RANDOM_CASES[name][4]
    g = np.random.default_rng(8).standard_normal(P.shape).astype(F32)
    args = [torch.from_numpy(a).to(d) for a in (dec, begin, P, g, q, act)]
    call = lambda: ops.soft_aggregate_backward(args[0], args[1], K, pad, args[2], args[3], args[4], args[5])
    a, b = call(), call()
    assert torch.equal(a, b)
    stream = torch.cuda.Stream(d)
    stream.wait_stream(torch.cuda.current_stream(d))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call()
        with torch.cuda.graph(graph, stream=stream):
            out = call()
        out.fill_(NAN)
        graph.replay()
    stream.synchronize()
    torch.cuda.current_stream(d).wait_stream(stream)
    assert torch.equal(out, a)


# ================================================================================================ GPU 4: the loss head end to end
@gpu
def test_the_loss_head_end_to_end_against_float64_torch():
    """dec (a leaf per frame) -> RMNet.decoder_tail -> est[:, t] -> losses.training_loss -> backward, against the same chain in
    float64 torch on the CPU.  With F the tail's backward (linear in g), P^ / g^ the device's probabilities and loss gradient:
        |F^(P^, g^) - F(P, g)| <= |F^ - F|(P^, g^) + |F(P^, g^) - F(P, g)|
    the first term is tail_backward_bound at (P^, g^); the second is bounded to first order from |P^ - P| <= the forward's bound
    (glue_ref.soft_aggregate_bound) and |g^ - g| <= the width of the loss gradient's bin bracket (loss_grad_ref.grad_bracket at
    P^, widened to hold the float64 sort's weight where P^ and P order two pixels differently) + loss_grad_ref.table_bound + the
    NLL term's move with P:
        ds <= sum_k (P_k dg_k + |g_k| dP_k);  ddl_k <= P_k (dg_k + ds) + dP_k |g_k - s|;  ddz_o <= m_{o+1} ddl_{o+1} + m_0 ddl_0 p_o / (1 - bg)"""
    import loss_grad_ref as LG
    from rmnet_amd import losses
    from rmnet_amd.rmnet import RMNet
    d = dev()
    counts, K, H, W, T = E2E['counts'], E2E['K'], E2E['H'], E2E['W'], E2E['frames']
    decs, labels = _e2e_inputs()
    begin = R.begin_of(counts)
    net = RMNet(None).train()
    bins = losses.DEFAULT_BINS

    def chain(device, dtype):
        leaves = [torch.tensor(x, dtype=dtype, device=device, requires_grad=True) for x in decs]
        est = torch.zeros(1, T, K, H, W, dtype=dtype, device=device)
        for t, leaf in enumerate(leaves):
            est[:, t] = net.decoder_tail(leaf, counts, K, (0, 0, 0, 0))[1]
        est.retain_grad()
        loss = losses.training_loss(est[0], torch.from_numpy(labels).to(device), bins=bins)
        loss.backward()
        return [x.grad.cpu().numpy() for x in leaves], est.detach()[0].cpu().numpy(), est.grad[0].cpu().numpy(), float(loss.detach())

    got, P_hat, g_hat, loss_hat = chain(d, torch.float32)
    want, P64, g64, loss64 = chain(torch.device('cpu'), torch.float64)
    lit = LG.literal(P64, labels)
    t64, w64 = lit['t'], g64 - lit['t']
    lo, hi = LG.grad_bracket(P_hat, labels, bins=bins)
    lo, hi = np.minimum(lo, w64), np.maximum(hi, w64)
    worst = 0.0
    for t in range(T):
        _, p64, _, bp = G.soft_aggregate_bound(decs[t], begin, K, 0, 0, H, W)
        assert _within(P_hat[t:t + 1], p64, bp)[0]
        dP = bp[0]
        tt = np.abs(t64[t])
        dg = (hi[t] - lo[t]) + LG.table_bound(np.maximum(np.abs(lo[t]), np.abs(hi[t])), tt) + tt * (G.SLACK * dP / p64[0] + 4 * LG.V) + LG.EPS
        ref, bound = R.tail_backward_bound(decs[t], begin, K, 0, 0, H, W, P_hat[t:t + 1], g_hat[t:t + 1])
        _, det = R.tail_backward(decs[t], begin, K, 0, 0, H, W, P_hat[t:t + 1], g_hat[t:t + 1], detail=True)
        c = det[0]
        P, g = c['P'], c['g']
        ds = (P * dg + np.abs(g) * dP).sum(axis=0)
        ddl = P * (dg + ds) + dP * np.abs(g - c['s'])
        with np.errstate(all='ignore'):
            da0 = np.where(c['m0'], ddl[0] / (1.0 - c['bg']), 0.0)
        for o in range(c['n']):
            move = G.SLACK * (np.where(c['m'][o], ddl[o + 1], 0.0) + da0 * c['p'][o])
            total = bound[o, 1] + move
            for plane in (0, 1):
                ok, ratio, bad = _within(got[t][o, plane], want[t][o, plane], total)
                worst = max(worst, ratio)
                assert ok, (t, o, plane, ratio, bad)
    print('TAIL gpu end to end: largest error / bound %.3f, loss %.9g (float64 %.9g)' % (worst, loss_hat, loss64))
    assert max(float(np.abs(w).max()) for w in want) > 1e-5


# ================================================================================================ GPU 5: refused calls leave the buffers alone
@gpu
def test_the_entry_refuses_malformed_calls_and_leaves_guarded_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    d = dev()
    pool = torch.full((1 << 14,), SENT, device=d)
    base = pool.data_ptr()
    begin = torch.tensor([0, 1, 2], dtype=torch.int32, device=d)
    action = torch.zeros(2, 3, dtype=torch.uint8, device=d)
    at = lambda floats: base + 4 * floats
    good = dict(dec=at(0), begin=begin.data_ptr(), B=2, K=3, Hp=8, Wp=12, pad_l=2, pad_t=1, H=6, W=7, prob=at(1024), prob_bs=3 * 42 + 5,
                gp=at(2048), gp_bs=3 * 42, gl=at(3072), gl_bs=3 * 42 + 1, action=action.data_ptr(), grad_dec=at(4096))
    for name, kw, code in _refusals(good):
        assert _call(lib, dict(good, **kw)) == code, name
        torch.cuda.synchronize()
        assert bool((pool == SENT).all()), name
    for kw in (dict(), dict(gp=None), dict(gl=None), dict(action=None), dict(pad_l=5, pad_t=2), dict(prob=at(1025), gp=at(2049))):
        assert _call(lib, dict(good, **kw)) == 0, kw
        torch.cuda.synchronize()
        host = pool.cpu().numpy()
        out = host[4096:4096 + 2 * 2 * 8 * 12]
        assert not (out == SENT).any() and (np.delete(host, np.s_[4096:4096 + 2 * 2 * 8 * 12]) == SENT).all(), kw
        pool.fill_(SENT)


# ================================================================================================ 6: the compiler's resources
def test_the_new_kernels_use_no_lds_and_no_scratch(tmp_path):
    """The three instances of soft_aggregate_bwd, from a compile-only gfx950 build: no static __shared__, no scratch, no spill."""
    import test_kernel_resources as tkr
    from rmnet_amd import build
    assert 'soft_aggregate_bwd.hip' in build.SOURCES
    kernels = tkr._kernels(tkr._compile('soft_aggregate_bwd.hip', str(tmp_path / 'soft_aggregate_bwd.s')))
    assert len(kernels) == 3
    for frag in ('18soft_aggregate_bwdILi4ELb1EE', '18soft_aggregate_bwdILi4ELb0EE', '18soft_aggregate_bwdILi1ELb0EE'):
        k = tkr._one(kernels, frag)
        print(frag, k)
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (frag, k)
