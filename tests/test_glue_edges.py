# -*- coding: utf-8 -*-
"""Per-element, every-branch tests of the elementwise glue kernels (rmnet_amd/csrc/epilogue.hip), next to the whole-tensor
comparisons with torch's own kernels in test_gpu_parity.py:
  1. channel_affine, upsample2x_add and affine_relu_maxpool, both layouts, bit for bit against an fp32 numpy restatement that no
     torch GPU kernel takes part in, at the smallest shapes that enter every branch of the launchers (tests/glue_ref.plan_of
     confirms the branch of every case on the CPU);
  2. soft_aggregate on a structural family (indexing; every output within the logf term) and a random family (every output within
     a derived bound of a float64 restatement), NaN propagation;
  3. the C entries' argument checks with sentinels in the buffers, and the wrappers' layout rules;
  4. planted faults of the restatements (CPU): each must fail the comparison of a named case.
The restatements, the launch plans and the derivation of the bound are in tests/glue_ref.py."""

import ctypes

import numpy as np
import pytest
import torch

import glue_ref as G


def dev():
    return torch.device('cuda', 0)


def _rng(seed):
    return np.random.default_rng(seed)


def _randn(rng, shape):
    return rng.standard_normal(shape, dtype=np.float32)


# ================================================================================================ the cases and their branches
# name -> (entry, logical shape of x, operands, what plan_of must say).  'big': compared once, one configuration.
SHAPE_CASES = {
    'ca vec second iteration, ragged tail': ('channel_affine', (1, 2, 514, 512), dict(res=True), dict(vec=True, iters=2, passes=1, grid=(64, 2))),
    'ca scalar second iteration': ('channel_affine', (1, 2, 129, 129), dict(res=False), dict(vec=False, iters=2, passes=1, grid=(64, 2))),
    'ca vec plane loop': ('channel_affine', (1, 65540, 2, 2), dict(res=True), dict(vec=True, iters=1, passes=2, grid=(1, 65535))),
    'ca scalar plane loop': ('channel_affine', (3, 21846, 1, 1), dict(res=False), dict(vec=False, iters=1, passes=2, grid=(1, 65535))),
    'ca nhwc per-element, 9 workgroups, 4 slots': ('channel_affine_nhwc', (1, 12, 50, 60), dict(res=True),
                                                   dict(fixed=False, grid=(9, 1), iters=1, slots=4, capped=False)),
    'ca nhwc C 2048': ('channel_affine_nhwc', (1, 2048, 2, 3), dict(res=False), dict(fixed=False, grid=(3, 1), iters=1, capped=False)),
    'ca nhwc FIXED above the cap': ('channel_affine_nhwc', (1, 4, 2049, 4095), dict(res=True, big=True),
                                    dict(fixed=True, grid=(8192, 1), iters=2, slots=4, capped=True)),
    'ca nhwc per-element above the cap': ('channel_affine_nhwc', (1, 12, 1367, 2047), dict(res=False, big=True),
                                          dict(fixed=False, grid=(8192, 1), iters=2, slots=4, capped=True)),
    'up vec above 256 chunks': ('upsample2x_add', (1, 1, 258, 258), {}, dict(vec=True, capped=True, iters=2, passes=1)),
    'up scalar above 256 chunks': ('upsample2x_add', (1, 1, 129, 129), {}, dict(vec=False, capped=True, iters=2, passes=1)),
    'up scalar plane loop': ('upsample2x_add', (1, 65537, 1, 1), {}, dict(vec=False, passes=2, grid=(1, 65535))),
    'up vec plane loop': ('upsample2x_add', (1, 65538, 1, 2), {}, dict(vec=True, passes=2, per_row=1, grid=(1, 65535))),
    'up h 1': ('upsample2x_add', (2, 3, 1, 6), {}, dict(vec=True, iters=1)),
    'up w 1': ('upsample2x_add', (2, 3, 6, 1), {}, dict(vec=False, iters=1)),
    'up w 2, one item per row': ('upsample2x_add', (1, 2, 5, 2), {}, dict(vec=True, per_row=1)),
    'up nhwc above the cap': ('upsample2x_add_nhwc', (1, 4, 1024, 1025), dict(big=True), dict(capped=True, iters=3, grid=(8192, 1))),
    'up nhwc h 1': ('upsample2x_add_nhwc', (2, 4, 1, 5), {}, dict(capped=False, iters=1)),
    'up nhwc w 1': ('upsample2x_add_nhwc', (2, 8, 6, 1), {}, dict(capped=False, iters=1)),
    'mp scalar above 128 chunks': ('affine_relu_maxpool', (1, 1, 363, 363), {}, dict(vec=False, capped=True, iters=2)),
    'mp vec above 128 chunks, odd H': ('affine_relu_maxpool', (1, 1, 513, 1024), {}, dict(vec=True, capped=True, iters=2)),
    'mp plane loop': ('affine_relu_maxpool', (1, 65537, 3, 3), {}, dict(vec=False, passes=2, grid=(1, 65535))),
    'mp vec W 8, only xq 0': ('affine_relu_maxpool', (2, 3, 5, 8), {}, dict(vec=True, per_row=1)),
    'mp vec W 16, xq 0 and 1': ('affine_relu_maxpool', (2, 3, 6, 16), {}, dict(vec=True, per_row=2)),
    'mp nhwc above the cap, odd H and W': ('affine_relu_maxpool_nhwc', (1, 4, 2899, 2897), dict(big=True), dict(capped=True, iters=2)),
    'mp nhwc odd H and W': ('affine_relu_maxpool_nhwc', (2, 8, 7, 9), {}, dict(capped=False, iters=1)),
}
# a vectorisable shape with ONE pointer 4 bytes off: the launcher must take the scalar kernel
MISALIGNED = [('channel_affine', (2, 3, 4, 6), 'x'), ('channel_affine', (2, 3, 4, 6), 'res'), ('channel_affine', (2, 3, 4, 6), 'out'),
              ('upsample2x_add', (2, 3, 4, 6), 'skip'), ('upsample2x_add', (2, 3, 4, 6), 'out'), ('affine_relu_maxpool', (2, 3, 6, 16), 'x')]
# the families' small shapes: (NCHW path they take, channels-last instance)
CA_FAMILY = [((2, 8, 5, 6), False, True), ((2, 12, 4, 6), True, False)]       # shape, NCHW vec, NHWC FIXED


def test_plan_of_confirms_the_branch_of_every_gpu_case():
    for name, (entry, shape, opts, want) in SHAPE_CASES.items():
        plan = G.plan_of(entry, shape, res=bool(opts.get('res')) or entry.startswith('upsample'))
        for k, v in want.items():
            assert plan[k] == v, (name, k, plan)
        print('PLAN %-45s %-28s %-18s %s' % (name, entry, shape, plan))
    for entry, shape, which in MISALIGNED:
        assert G.plan_of(entry, shape, res=True)['vec'], (entry, shape)
        plan = G.plan_of(entry, shape, {which: 4}, res=True)
        assert not plan['vec'], (entry, shape, which)
        print('PLAN %-45s %-28s %-18s %s' % ('%s misaligned' % which, entry, shape, plan))
    for shape, vec, fixed in CA_FAMILY:
        assert G.plan_of('channel_affine', shape)['vec'] == vec and G.plan_of('channel_affine_nhwc', shape)['fixed'] == fixed
    # the caps themselves: one item below each, the cap does not bind
    assert G.plan_of('channel_affine', (1, 1, 512, 512))['iters'] == 1 and G.plan_of('channel_affine', (1, 1, 128, 128), {'x': 4})['iters'] == 1
    assert not G.plan_of('channel_affine_nhwc', (1, 4, 2048, 4096))['capped']
    assert not G.plan_of('upsample2x_add_nhwc', (1, 4, 512, 1024))['capped']


# ================================================================================================ CPU: the restatements themselves
def test_the_restatements_are_the_torch_expressions_on_the_cpu():
    """The fp32 restatements against torch's CPU operators evaluated op by op (channel_affine, the pool: bit for bit; the
    upsample: torch's CPU kernel orders its products differently, so within 2 ulp of the largest term)."""
    import torch.nn.functional as F
    rng = _rng(1)
    x, r = _randn(rng, (2, 5, 7, 9)), _randn(rng, (2, 5, 7, 9))
    sc, sh, rs, rh = [_randn(rng, 5) for _ in range(4)]
    t = torch.from_numpy
    v = lambda a: t(a).view(1, 5, 1, 1)
    want = torch.relu((t(x) * v(sc) + v(sh)) + (t(r) * v(rs) + v(rh)))
    assert G.bits_equal(G.channel_affine_f32(x, sc, sh, r, rs, rh, True), want.numpy())[0]
    want = F.leaky_relu(t(x) * v(sc) + v(sh), 0.1)
    assert float(np.abs(G.channel_affine_f32(x, sc, sh, relu='leaky') - want.numpy()).max()) <= 2.0 ** -23 * 8
    want = F.max_pool2d(torch.relu(t(x) * v(sc) + v(sh)), 3, stride=2, padding=1)
    assert G.bits_equal(G.maxpool_f32(x, sc, sh), want.numpy())[0]
    want = F.interpolate(t(x), scale_factor=2, mode='bilinear', align_corners=False)
    assert float(np.abs(G.upsample_f32(x) - want.numpy()).max()) <= 2.0 ** -22 * float(np.abs(x).max())
    assert float(np.abs(G.upsample_f64(x) - G.upsample_f32(x)).max()) <= 4 * 2.0 ** -24 * float(np.abs(x).max())
    assert float(np.abs(G.channel_affine_f64(x, sc, sh, r, rs, rh, 'leaky') - G.channel_affine_f32(x, sc, sh, r, rs, rh, 'leaky')).max()) < 1e-5
    assert float(np.abs(G.maxpool_f64(x, sc, sh) - G.maxpool_f32(x, sc, sh)).max()) < 1e-5


def _int4(rng, shape):
    """Integer multiples of 4, |x| <= 2^18, with the extremes present."""
    x = (4 * rng.integers(-2 ** 16, 2 ** 16 + 1, shape)).astype(np.float32)
    x.flat[0], x.flat[-1] = 2.0 ** 18, -2.0 ** 18
    return x


UP_SMALL = [s for (e, s, o, _) in SHAPE_CASES.values() if e.startswith('upsample') and not o.get('big')] + [(2, 3, 4, 6), (2, 4, 3, 5)]


@pytest.mark.parametrize('shape', UP_SMALL)
def test_the_integer_upsample_family_is_exact(shape):
    """Inputs that are multiples of 4: the float64 result is representable and the fp32 restatement returns it exactly."""
    rng = _rng(sum(shape))
    N, C, h, w = shape
    x, s = _int4(rng, shape), _int4(rng, (N, C, 2 * h, 2 * w))
    for skip in (None, s):
        w64 = G.upsample_f64(x, skip)
        assert np.array_equal(w64.astype(np.float32).astype(np.float64), w64)
        ok, first, n = G.bits_equal(G.upsample_f32(x, skip), w64.astype(np.float32))
        assert ok, (shape, first, n)


# ------------------------------------------------------------------------------------------------ soft_aggregate cases
# name -> (object counts per clip, K, Hp, Wp, (lw, uw, lh, uh))
STRUCT_CASES = {
    'four different pads, empty clips between full ones, absent channels': ([2, 0, 3, 0, 1], 4, 23, 29, (3, 5, 2, 4)),
    'more objects than K - 1': ([4, 1], 3, 17, 21, (1, 2, 3, 0)),
    'K 1': ([2, 0], 1, 9, 12, (2, 1, 0, 3)),
    'second grid-stride iteration': ([1], 2, 520, 513, (1, 0, 7, 0)),
}
RANDOM_CASES = {'1 object': ([1], 2, 37, 53, (0, 0, 0, 0)), '3 objects': ([3], 4, 37, 53, (2, 1, 3, 0)), '5 objects': ([5], 6, 37, 53, (0, 3, 1, 2)),
                'mixed clips': ([3, 1, 5], 6, 19, 23, (1, 2, 3, 4))}


def _soft_args(counts, K, Hp, Wp, pad):
    lw, uw, lh, uh = pad
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return begin, lw, lh, Hp - lh - uh, Wp - lw - uw


def _random_dec(counts, Hp, Wp, seed):
    rng = _rng(seed)
    n = sum(counts)
    z0 = _randn(rng, (n, Hp, Wp)) * np.float32(3.0)
    z1 = z0 + rng.uniform(-6.0, 6.0, (n, Hp, Wp)).astype(np.float32)
    return np.stack([z0, z1], axis=1)


def _within(got, ref, bound):
    """(all inside, largest error / bound, flat index of the worst) -- a NaN counts as outside."""
    err = np.abs(got.astype(np.float64) - ref)
    ratio = err / np.maximum(bound, 1e-300)
    bad = ~(err <= bound)
    worst = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    return not bool(bad.any()), float(np.nanmax(ratio)), worst, int(bad.sum())


def _struct_bounds(dec, begin, K, lw, lh, H, W):
    l64, p64, _, _ = G.soft_aggregate_bound(dec, begin, K, lw, lh, H, W)
    bl = G.logf_term(l64)
    A = (l64.max(axis=1, keepdims=True) - l64).max(axis=1, keepdims=True)
    bp = G.SLACK * p64 * (bl + (p64 * bl).sum(axis=1, keepdims=True) + 2.0 * (A + 1.0) * G.U + 2.0 * G.E_ULP * G.EPS + K * G.U)
    return l64, p64, bl, bp


@pytest.mark.parametrize('name', list(RANDOM_CASES))
def test_the_fp32_restatement_of_soft_aggregate_is_inside_the_bound(name):
    counts, K, Hp, Wp, pad = RANDOM_CASES[name]
    begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
    dec = _random_dec(counts, Hp, Wp, seed=K)
    l64, p64, bl, bp = G.soft_aggregate_bound(dec, begin, K, lw, lh, H, W)
    l32, p32 = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W)
    okl, rl, _, nl = _within(l32, l64, bl)
    okp, rp, _, npb = _within(p32, p64, bp)
    print('SOFT cpu random %-12s largest error / bound: logits %.3f, probabilities %.3f (largest bound %.3g)' % (name, rl, rp, bl.max()))
    assert okl and okp, (name, rl, rp, nl, npb)
    assert rl > 0.02            # (not vacuous: the restatement uses a real share of it)


@pytest.mark.parametrize('name', list(STRUCT_CASES))
def test_the_fp32_restatement_of_the_structural_family_is_inside_the_logf_term(name):
    counts, K, Hp, Wp, pad = STRUCT_CASES[name]
    begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
    dec = G.structural_dec(sum(counts), Hp, Wp, seed=K)
    ch = G.structural_choice(dec, lw, lh, H, W)
    assert all(int((ch == v).sum()) > 0 for v in (0.0, 200.0, -200.0))
    l64, p64, bl, bp = _struct_bounds(dec, begin, K, lw, lh, H, W)
    l32, p32 = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W)
    assert _within(l32, l64, bl)[0] and _within(p32, p64, bp)[0]
    assert len(np.unique(l64)) <= max(counts) + 5             # 0, the two clamp logits and those of 2^-k: nothing else


# ================================================================================================ CPU: planted faults
def _existing_generator_inputs():
    """The inputs of the test_gpu_parity.py cases of these kernels (same generators and seeds), as numpy arrays."""
    out = dict(ca=[], up=[], mp=[], sa=[])
    for N, C, H, W in [(2, 5, 7, 9), (3, 16, 30, 54), (1, 3, 1, 1), (1, 64, 240, 432)]:
        g = torch.Generator().manual_seed(N * 100 + C)
        x, r = torch.randn(N, C, H, W, generator=g).numpy(), torch.randn(N, C, H, W, generator=g).numpy()
        sc, sh, rs, rh = [torch.randn(C, generator=g).numpy() for _ in range(4)]
        out['ca'] += [(x, sc, sh, None, None, None, False), (x, sc, sh, None, None, None, True), (x, None, sh, r, None, None, False),
                      (x, sc, sh, r, rs, rh, True), (x, sc, None, r, None, rh, False), (x, None, None, r, None, None, True)]
    for N, C, H, W in [(2, 8, 5, 6), (3, 4, 7, 9), (1, 12, 6, 5), (1, 64, 30, 54), (2, 256, 12, 20)]:      # the channels-last test's calls
        g = torch.Generator().manual_seed(N * 100 + C)
        x, r = torch.randn(N, C, H, W, generator=g).numpy(), torch.randn(N, C, H, W, generator=g).numpy()
        sc, sh = (torch.rand(C, generator=g) + 0.5).numpy(), torch.randn(C, generator=g).numpy()
        rs, rh = (torch.rand(C, generator=g) + 0.5).numpy(), torch.randn(C, generator=g).numpy()
        out['ca'] += [(x, sc, sh, None, None, None, True), (x, sc, sh, None, None, None, False), (x, sc, sh, None, None, None, 'leaky'),
                      (x, sc, sh, r, None, None, True), (x, sc, sh, r, rs, rh, True)]
    for N, C, h, w in [(1, 1, 1, 1), (2, 3, 5, 6), (1, 2, 7, 9), (1, 8, 30, 54), (4, 16, 60, 108)]:
        g = torch.Generator().manual_seed(h * 100 + w)
        out['up'].append(torch.randn(N, C, h, w, generator=g).numpy())
    for N, C, H, W in [(1, 2, 1, 1), (2, 3, 7, 9), (3, 5, 16, 10), (2, 4, 9, 16), (1, 64, 240, 432)]:
        g = torch.Generator().manual_seed(H * 10 + W)
        x = torch.randn(N, C, H, W, generator=g).numpy()
        out['mp'].append((x, torch.randn(C, generator=g).numpy(), torch.randn(C, generator=g).numpy()))
    for counts, K, Hp, Wp, pad in [([1], 2, 32, 48, (0, 0, 0, 0)), ([0, 2], 4, 16, 16, (1, 0, 0, 1)), ([2, 1, 3], 5, 48, 64, (5, 5, 3, 2)),
                                   ([1, 1, 1, 1], 2, 480, 864, (5, 5, 0, 0))]:
        g = torch.Generator().manual_seed(sum(counts) * 10 + K)
        n = sum(counts)
        dec = (torch.randn(max(n, 1), 2, Hp, Wp, generator=g) * 4).numpy()[:n]
        out['sa'].append((dec,) + _soft_args(counts, K, Hp, Wp, pad) + (K,))
    return out


def _existing_tests_catch(mutant, inp):
    """Would the comparisons of test_gpu_parity.py (torch.equal; the 4e-7 whole-tensor bar of the upsample; rtol = atol = 2e-5 for
    soft_aggregate) reject a kernel with this fault, on their own inputs?  The unmutated restatement stands for torch's result."""
    if mutant in ('rshift_before_rscale', 'leaky_before_res'):
        return any(not G.bits_equal(G.channel_affine_f32(*a, mutant=mutant), G.channel_affine_f32(*a))[0] for a in inp['ca'])
    if mutant in ('i1_clamped_at_n', 'weights_swapped'):
        return any(float(np.abs(G.upsample_f32(x, mutant=mutant) - G.upsample_f32(x)).max()) > 4e-7 * max(1.0, float(np.abs(x).max()))
                   for x in inp['up'])
    if mutant == 'left_column_dropped':
        return any(not G.bits_equal(G.maxpool_f32(*a, mutant=mutant), G.maxpool_f32(*a))[0] for a in inp['mp'])
    if mutant == 'nan_not_propagated':                  # the one assertion there is: NaN at [0, 0, 0, 0] gives NaN at [0, 0, 0, 0]
        x, sc, sh = inp['mp'][1]
        x = x.copy()
        x[0, 0, 0, 0] = np.nan
        return not np.isnan(G.maxpool_f32(x, sc, sh, mutant=mutant)[0, 0, 0, 0])
    for dec, begin, lw, lh, H, W, K in inp['sa']:
        a, _ = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W, want_prob=False, mutant=mutant)
        b, _ = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W, want_prob=False)
        if not np.allclose(a, b, rtol=2e-5, atol=2e-5):
            return True
    return False


def _new_tests_catch(mutant):
    """The named case of this file on which the fault fails the new comparison, or None."""
    if mutant in ('i1_clamped_at_n', 'weights_swapped'):
        for name in ('up w 2, one item per row', 'up h 1', 'up w 1'):
            shape = SHAPE_CASES[name][1]
            x = _int4(_rng(sum(shape)), shape)
            if not G.bits_equal(G.upsample_f32(x, mutant=mutant), G.upsample_f64(x).astype(np.float32))[0]:
                return name
    if mutant == 'left_column_dropped':
        name = 'mp vec W 16, xq 0 and 1'
        x, sc, sh = _mp_inputs(SHAPE_CASES[name][1], 5)
        return name if not G.bits_equal(G.maxpool_f32(x, sc, sh, mutant=mutant), G.maxpool_f32(x, sc, sh))[0] else None
    if mutant == 'nan_not_propagated':
        x, sc, sh = _nan_window_inputs(7, 7, 4)
        return 'NaN in each window position' if not G.bits_equal(G.maxpool_f32(x, sc, sh, mutant=mutant), G.maxpool_f32(x, sc, sh))[0] else None
    if mutant in ('rshift_before_rscale', 'leaky_before_res'):
        x, r, par = _ca_inputs(CA_FAMILY[0][0], 3, special=True)
        a = (x, par[0], par[1], r, par[2], par[3], 'leaky')
        return 'res + res_scale + res_shift, leaky' if not G.bits_equal(G.channel_affine_f32(*a, mutant=mutant), G.channel_affine_f32(*a))[0] else None
    for name, (counts, K, Hp, Wp, pad) in STRUCT_CASES.items():
        begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
        dec = G.structural_dec(sum(counts), Hp, Wp, seed=K)
        l64, p64, bl, bp = _struct_bounds(dec, begin, K, lw, lh, H, W)
        l32, p32 = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W, mutant=mutant)
        if not (_within(l32, l64, bl)[0] and _within(p32, p64, bp)[0]):
            return name
    return None


def test_every_planted_fault_fails_a_named_case():
    """Nine mutants of the fp32 restatements.  Each must fail the NEW comparison on a named case; the table says which of them the
    inputs of the older tests would catch too.  (Padding as 0 instead of -inf is not planted: after the ReLU every window value is
    >= 0, so a 0 pad can never win where a -inf pad would not -- invisible by construction, for these tests and for any other.)"""
    inp = _existing_generator_inputs()
    missed = []
    for m in G.MUTANTS:
        new = _new_tests_catch(m)
        old = _existing_tests_catch(m, inp)
        print('MUTANT %-22s new tests: %-70s test_gpu_parity inputs: %s' % (m, 'caught by "%s"' % new if new else 'MISSED', 'caught' if old else 'not caught'))
        if new is None:
            missed.append(m)
    assert not missed, missed


def test_the_soft_aggregate_bound_is_not_vacuous():
    """On the random family, a logf that is 16 ulp off, or an expf argument moved by 32 u, leaves the bound."""
    counts, K, Hp, Wp, pad = RANDOM_CASES['3 objects']
    begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
    dec = _random_dec(counts, Hp, Wp, seed=K)
    l64, p64, bl, bp = G.soft_aggregate_bound(dec, begin, K, lw, lh, H, W)
    l32, _ = G.soft_aggregate_f32(dec, begin, K, lw, lh, H, W)
    assert _within(l32, l64, bl)[0]
    assert not _within(l32 * np.float32(1 + 16 * G.EPS), l64, bl)[0]                    # logf 16 ulp off
    dec2 = dec.copy()
    dec2[:, 1] += np.float32(32 * G.U) * np.maximum(np.abs(dec2[:, 1]), np.float32(1.0))   # the argument of an expf moved by 32 u
    l32b, _ = G.soft_aggregate_f32(dec2, begin, K, lw, lh, H, W)
    assert not _within(l32b, l64, bl)[0]


# ================================================================================================ inputs shared by CPU and GPU tests
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38], np.float32)


def _ca_inputs(shape, seed, special=False):
    rng = _rng(seed)
    x, r = _randn(rng, shape), _randn(rng, shape)
    par = [_randn(rng, shape[1]) for _ in range(4)]
    if special:
        n = x.size
        x.flat[np.arange(len(SPECIALS)) * 7 % n] = SPECIALS
        r.flat[(np.arange(len(SPECIALS)) * 11 + 3) % n] = SPECIALS[::-1]
    return x, r, par


def _mp_inputs(shape, seed, special=True):
    rng = _rng(seed)
    x = _randn(rng, shape)
    C = shape[1]
    sc, sh = _randn(rng, C), _randn(rng, C)            # (negative scales among them)
    if special and x.size >= 64:
        x.reshape(-1)[:: max(x.size // 13, 1)][:6] = [-np.inf, np.inf, -np.inf, -0.0, 0.0, -np.inf]
    if special:
        sc[0], sh[0] = -1.0, -100.0 if C > 1 else 0.25     # channel 0: every window negative before the ReLU (C > 1)
        if C > 1:
            x[:, 0] = np.abs(x[:, 0])
    return x, sc, sh


def _nan_window_inputs(H, W, C):
    """18 images: a NaN at each of the nine window positions of output (0, 0) (a border: the positions in the padding hold none)
    and of output (1, 1) (interior)."""
    rng = _rng(9)
    x = _randn(rng, (18, C, H, W))
    for i in range(18):
        yo = xo = i // 9
        dy, dx = (i % 9) // 3 - 1, (i % 9) % 3 - 1
        y, xx = 2 * yo + dy, 2 * xo + dx
        if 0 <= y < H and 0 <= xx < W:
            x[i, i % C, y, xx] = np.nan
    return x, _randn(rng, C), _randn(rng, C)


# ================================================================================================ GPU helpers
NAN_BITS = 0x7fc00000


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _off4(t):
    """A contiguous copy of t that starts 4 bytes past a 16-byte boundary (a view one float into a larger buffer)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32).masked_fill(t != t, NAN_BITS)


def _assert_bits(got, want, what):
    """Every element the same 32 bits (a NaN: a NaN), compared on the device; a failure names the first differing element."""
    if isinstance(want, np.ndarray):
        want = _t(want.astype(np.float32, copy=False))
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    gi, wi = _bits(got), _bits(want)
    if torch.equal(gi, wi):
        return
    bad = (gi != wi).flatten().nonzero().flatten()
    i = int(bad[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(want.shape)))
    pytest.fail('%s: %d of %d elements differ; first at %s: got %r (0x%08x), want %r (0x%08x)' % (
        what, bad.numel(), want.numel(), idx, float(got.contiguous().flatten()[i]), int(gi.flatten()[i]) & 0xffffffff,
        float(want.flatten()[i]), int(wi.flatten()[i]) & 0xffffffff))


def _place(a, cl=False, off=False):
    t = _t(a)
    if cl:
        t = _cl(t)
    return _off4(t) if off else t


# ================================================================================================ GPU: channel_affine
def _run_channel_affine(x, r, par, cl, scale=True, shift=True, res=False, rs=False, rh=False, relu=False, inplace=None, off=()):
    from rmnet_amd import ops
    sc, sh, rsc, rsh = par
    args = (sc if scale else None, sh if shift else None, r if res else None, rsc if rs else None, rsh if rh else None)
    want = G.channel_affine_f32(x, *args, relu=relu)
    d = lambda a: _t(a) if a is not None else None
    xd = _place(x, cl, 'x' in off)
    rd = _place(r, cl, 'res' in off) if res else None
    out = xd if inplace == 'x' else rd if inplace == 'res' else None
    if 'out' in off:
        out = _off4(torch.empty_like(xd))
    got = ops.channel_affine(xd, d(args[0]), d(args[1]), rd, d(args[3]), d(args[4]), relu=relu, out=out)
    if out is not None:
        assert got is out
    assert got.is_contiguous(memory_format=torch.channels_last) if cl else got.is_contiguous()
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize('cl', [False, True], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('shape,vec,fixed', CA_FAMILY)
def test_channel_affine_every_operand_combination_bit_for_bit(shape, vec, fixed, cl):
    """Every combination of the optional operands x relu in {False, True, 'leaky'}, NaN / +-inf / signed zeros / extremes among the
    inputs, in place on x and on res: the same 32 bits as channel_affine_f32 in every element."""
    x, r, par = _ca_inputs(shape, seed=shape[1], special=True)
    n = 0
    for relu in (False, True, 'leaky'):
        for scale in (False, True):
            for shift in (False, True):
                for res, rs, rh in ((False, False, False), (True, False, False), (True, True, False), (True, False, True), (True, True, True)):
                    kw = dict(scale=scale, shift=shift, res=res, rs=rs, rh=rh, relu=relu)
                    got, want = _run_channel_affine(x, r, par, cl, **kw)
                    _assert_bits(got, want, 'channel_affine %s %s %s' % (shape, 'nhwc' if cl else 'nchw', kw))
                    n += 1
        for inplace in ('x', 'res'):
            kw = dict(res=True, rs=True, rh=True, relu=relu, inplace=inplace)
            got, want = _run_channel_affine(x, r, par, cl, **kw)
            _assert_bits(got, want, 'channel_affine %s %s %s' % (shape, 'nhwc' if cl else 'nchw', kw))
    assert n == 60


def _shape_case(name):
    entry, shape, opts, _ = SHAPE_CASES[name]
    return entry, shape, opts


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n, c in SHAPE_CASES.items() if c[0].startswith('channel_affine')])
def test_channel_affine_branches_bit_for_bit(name):
    entry, shape, opts = _shape_case(name)
    cl = entry.endswith('nhwc')
    x, r, par = _ca_inputs(shape, seed=len(name), special=True)
    res = bool(opts.get('res'))
    configs = [dict(res=res, rs=res, rh=res, relu='leaky')]
    if not opts.get('big'):
        configs += [dict(res=res, relu=True, scale=False), dict(res=res, rs=res, relu=False, shift=False, inplace='x')]
    for kw in configs:
        got, want = _run_channel_affine(x, r, par, cl, **kw)
        _assert_bits(got, want, '%s %s' % (name, kw))


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['x', 'res', 'out'])
def test_channel_affine_with_one_misaligned_pointer_takes_the_scalar_kernel_and_the_same_bits(which):
    shape = (2, 3, 4, 6)
    x, r, par = _ca_inputs(shape, seed=2, special=True)
    kw = dict(res=True, rs=True, rh=True, relu='leaky')
    aligned, want = _run_channel_affine(x, r, par, False, **kw)
    got, _ = _run_channel_affine(x, r, par, False, off=(which,), **kw)
    _assert_bits(got, want, 'channel_affine, %s misaligned' % which)
    _assert_bits(got, aligned, 'channel_affine, %s misaligned, against the aligned run' % which)


# ================================================================================================ GPU: upsample2x_add
def _run_upsample(x, s, cl, skip=True, inplace=False, off=()):
    from rmnet_amd import ops
    xd = _place(x, cl)
    sd = _place(s, cl, 'skip' in off) if skip else None
    out = sd if inplace else None
    if 'out' in off:
        out = _off4(torch.empty(s.shape, device=dev()))
    got = ops.upsample2x_add(xd, sd, out=out)
    if out is not None:
        assert got is out
    assert got.is_contiguous(memory_format=torch.channels_last) if cl else got.is_contiguous()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n, c in SHAPE_CASES.items() if c[0].startswith('upsample')])
def test_upsample2x_add_bit_for_bit_random_and_exact_integer_families(name):
    """Random fp32 inputs against upsample_f32, and multiples of 4 against the float64 result itself; with and without the skip
    and in place on it.  (The cases above the caps run the in-place skip configuration of each family only.)"""
    entry, shape, opts = _shape_case(name)
    cl = entry.endswith('nhwc')
    N, C, h, w = shape
    rng = _rng(len(name))
    for family in ('random', 'integer'):
        if family == 'random':
            x, s = _randn(rng, shape), _randn(rng, (N, C, 2 * h, 2 * w))
            ref = lambda sk: G.upsample_f32(x, sk)
        else:
            x, s = _int4(rng, shape), _int4(rng, (N, C, 2 * h, 2 * w))
            ref = lambda sk: G.upsample_f64(x, sk).astype(np.float32)
        if not opts.get('big'):
            _assert_bits(_run_upsample(x, s, cl, skip=False), ref(None), '%s, %s, no skip' % (name, family))
            _assert_bits(_run_upsample(x, s, cl), ref(s), '%s, %s, skip' % (name, family))
        if not opts.get('big') or family == 'random':
            _assert_bits(_run_upsample(x, s, cl, inplace=True), ref(s), '%s, %s, in place on the skip' % (name, family))
        else:
            _assert_bits(_run_upsample(x, s, cl, skip=False), ref(None), '%s, %s, no skip' % (name, family))


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['skip', 'out'])
def test_upsample2x_add_with_one_misaligned_pointer_takes_the_scalar_kernel_and_the_same_bits(which):
    shape = (2, 3, 4, 6)
    rng = _rng(4)
    x, s = _randn(rng, shape), _randn(rng, (2, 3, 8, 12))
    want = G.upsample_f32(x, s)
    got = _run_upsample(x, s, False, off=(which,))
    _assert_bits(got, want, 'upsample2x_add, %s misaligned' % which)
    _assert_bits(got, _run_upsample(x, s, False), 'upsample2x_add, %s misaligned, against the aligned run' % which)


# ================================================================================================ GPU: affine_relu_maxpool
def _run_maxpool(x, sc, sh, cl, off=False):
    from rmnet_amd import ops
    got = ops.affine_relu_maxpool(_place(x, cl, off), _t(sc) if sc is not None else None, _t(sh) if sh is not None else None)
    assert got.is_contiguous(memory_format=torch.channels_last) if cl else got.is_contiguous()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n, c in SHAPE_CASES.items() if c[0].startswith('affine_relu_maxpool')])
def test_affine_relu_maxpool_branches_bit_for_bit(name):
    """Negative scales, a channel whose every window is negative before the ReLU, +-inf and signed zeros among the inputs."""
    entry, shape, opts = _shape_case(name)
    cl = entry.endswith('nhwc')
    x, sc, sh = _mp_inputs(shape, seed=len(name))
    _assert_bits(_run_maxpool(x, sc, sh, cl), G.maxpool_f32(x, sc, sh), name)
    if not opts.get('big'):
        _assert_bits(_run_maxpool(x, None, None, cl), G.maxpool_f32(x), name + ', no scale, no shift')
        _assert_bits(_run_maxpool(-np.abs(x), None, sh * 0, cl), G.maxpool_f32(-np.abs(x), None, sh * 0), name + ', nothing positive anywhere')


@pytest.mark.gpu
@pytest.mark.parametrize('kind,H,W,C', [('scalar', 7, 7, 3), ('VEC4', 6, 16, 3), ('nhwc', 7, 7, 4)])
def test_affine_relu_maxpool_a_nan_in_each_window_position(kind, H, W, C):
    """A NaN at each of the nine window positions of a border output and of an interior output (one image each): NaN in exactly the
    outputs whose window holds it."""
    x, sc, sh = _nan_window_inputs(H, W, C)
    plan = G.plan_of('affine_relu_maxpool', x.shape)
    assert plan['vec'] == (kind == 'VEC4')
    want = G.maxpool_f32(x, sc, sh)
    assert int(np.isnan(want).sum()) >= 13             # (four in-bounds positions of the border output, nine of the interior one)
    _assert_bits(_run_maxpool(x, sc, sh, kind == 'nhwc'), want, 'NaN windows, ' + kind)


@pytest.mark.gpu
def test_affine_relu_maxpool_with_a_misaligned_x_takes_the_scalar_kernel_and_the_same_bits():
    x, sc, sh = _mp_inputs((2, 3, 6, 16), seed=6)
    want = G.maxpool_f32(x, sc, sh)
    got = _run_maxpool(x, sc, sh, False, off=True)
    _assert_bits(got, want, 'affine_relu_maxpool, x misaligned')
    _assert_bits(got, _run_maxpool(x, sc, sh, False), 'affine_relu_maxpool, x misaligned, against the aligned run')


# ================================================================================================ GPU: soft_aggregate
def _run_soft(dec, begin, K, pad, want_prob=True):
    from rmnet_amd import ops
    logit, prob = ops.soft_aggregate(_t(dec), _t(begin), K, pad, want_prob=want_prob)
    return logit, prob


def _assert_inside(got, ref, bound, what):
    ok, ratio, worst, nbad = _within(got, ref, bound)
    if not ok:
        idx = tuple(int(v) for v in np.unravel_index(worst, ref.shape))
        pytest.fail('%s: %d of %d elements outside the bound, largest error / bound %.3g at %s: got %r, reference %r, bound %.3g' % (
            what, nbad, ref.size, ratio, idx, float(got[idx]), float(ref[idx]), float(bound[idx])))
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(STRUCT_CASES))
def test_soft_aggregate_structural_family_every_element_within_the_logf_term(name):
    """z1 - z0 in {0, +200, -200} per (object, pixel): p is exactly 1/2, 1 or 0, every em is exact, and every logit is within
    (2 + 2 L |l|) u of the float64 reference at the fp32 clamp constants; the foreground logit of a '0' cell is logf(1) = 0.0
    exactly (profiles/r14_a_glue_tests.md: expf(0) = 1 and logf(1) = 0 on gfx950).  Carries the indexing: four different pads,
    obj_begin with empty clips, more objects than K - 1, K = 1, absent channels, a second grid-stride iteration."""
    counts, K, Hp, Wp, pad = STRUCT_CASES[name]
    begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
    dec = G.structural_dec(sum(counts), Hp, Wp, seed=K)
    l64, p64, bl, bp = _struct_bounds(dec, begin, K, lw, lh, H, W)
    assert name != 'second grid-stride iteration' or H * W > 1024 * 256        # (launch_soft_aggregate: at most 1024 workgroups per clip)
    logit, prob = _run_soft(dec, begin, K, pad)
    assert tuple(logit.shape) == l64.shape == tuple(prob.shape)
    gl, gp = logit.cpu().numpy(), prob.cpu().numpy()
    rl = _assert_inside(gl, l64, bl, 'soft_aggregate structural "%s", logits' % name)
    rp = _assert_inside(gp, p64, bp, 'soft_aggregate structural "%s", probabilities' % name)
    ch = G.structural_choice(dec, lw, lh, H, W)
    zeros = total = 0
    for b, cnt in enumerate(counts):
        for o in range(min(cnt, K - 1)):
            cell = ch[begin[b] + o] == 0.0
            total += int(cell.sum())
            zeros += int((gl[b, o + 1][cell] == 0.0).sum())
    print('SOFT gpu structural %-70s error / logf term: logits %.3f, probabilities %.3f; logf(1) cells exactly 0.0: %d of %d' % (
        name, rl, rp, zeros, total))
    assert zeros == total
    only, none = _run_soft(dec, begin, K, pad, want_prob=False)
    assert none is None
    _assert_bits(only, logit, 'soft_aggregate structural "%s", want_prob=False' % name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(RANDOM_CASES))
def test_soft_aggregate_random_family_every_element_within_the_derived_bound(name):
    """|z1 - z0| <= 6, 1 / 3 / 5 objects: every logit and every probability against soft_aggregate_f64 and the bound of
    glue_ref.py's docstring, none left out."""
    counts, K, Hp, Wp, pad = RANDOM_CASES[name]
    begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
    dec = _random_dec(counts, Hp, Wp, seed=K)
    l64, p64, bl, bp = G.soft_aggregate_bound(dec, begin, K, lw, lh, H, W)
    logit, prob = _run_soft(dec, begin, K, pad)
    rl = _assert_inside(logit.cpu().numpy(), l64, bl, 'soft_aggregate random "%s", logits' % name)
    rp = _assert_inside(prob.cpu().numpy(), p64, bp, 'soft_aggregate random "%s", probabilities' % name)
    print('SOFT gpu random %-12s largest error / bound: logits %.3f, probabilities %.3f' % (name, rl, rp))
    only, _ = _run_soft(dec, begin, K, pad, want_prob=False)
    _assert_bits(only, logit, 'soft_aggregate random "%s", want_prob=False' % name)


@pytest.mark.gpu
def test_soft_aggregate_a_nan_stays_in_its_object_its_background_and_its_pixel():
    counts, K, Hp, Wp, pad = [3, 2], 4, 13, 17, (2, 1, 1, 3)
    begin, lw, lh, H, W = _soft_args(counts, K, Hp, Wp, pad)
    dec = _random_dec(counts, Hp, Wp, seed=8)
    clean_l, clean_p = _run_soft(dec, begin, K, pad)
    bad = dec.copy()
    spots = [(1, 0, 4, 5), (1, 1, 7, 2), (3, 1, 0, 0)]                 # (object, z0 / z1, y, x) in the un-padded window
    for o, z, y, x in spots:
        bad[o, z, y + lh, x + lw] = np.nan
    bad[0, 0, 0, 0] = np.nan                                           # (in the padding: read by nobody)
    logit, prob = _run_soft(bad, begin, K, pad)
    want_l, want_p = clean_l.clone(), clean_p.clone()
    for o, z, y, x in spots:
        b = 0 if o < 3 else 1
        k = o - int(begin[b]) + 1
        want_l[b, k, y, x] = float('nan')
        want_l[b, 0, y, x] = float('nan')
        want_p[b, :, y, x] = float('nan')
    _assert_bits(logit, want_l, 'soft_aggregate with NaN inputs, logits')
    _assert_bits(prob, want_p, 'soft_aggregate with NaN inputs, probabilities')


# ================================================================================================ GPU: the C entries
SENT = 12345.0
E_INVALID, E_UNSUPPORTED = -1, -4          # include/rmnet_hip.h: RMNET_E_INVALID_ARG, RMNET_E_UNSUPPORTED


def _p(addr):
    return ctypes.c_void_p(addr) if addr else None


def _entry_check(fn, order, good, cases, accepted):
    """``good``: argument name -> value; a pointer is '@<float offset into the sentinel pool>' with an optional '+4' (bytes), a raw
    address as ('raw', address), or None.  Each case changes ``good`` in one respect: the entry must return the code and leave
    every buffer alone.  Then the good call and its ``accepted`` variants run (and write)."""
    pool = torch.full((1 << 16,), SENT, dtype=torch.float32, device=dev())
    base = pool.data_ptr()
    assert base % 256 == 0

    def value(v):
        if isinstance(v, tuple):
            return _p(v[1])
        if isinstance(v, str):
            return _p(base + 4 * int(v[1:].split('+')[0]) + (4 if v.endswith('+4') else 0))
        return v

    def call(**kw):
        a = dict(good, **kw)
        return fn(*([value(a[k]) for k in order] + [None]))

    def intact():
        torch.cuda.synchronize()
        return bool((pool == SENT).all())

    for name, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (name, rc, want)
        assert intact(), name
    for i, kw in enumerate(accepted):
        assert call(**kw) == 0, kw
        assert i > 0 or not intact()          # (the good call writes; a later variant may well restore the sentinel, as an upsample of a constant does)


def _nulls(names):
    return [('no %s' % n, {n: None}, E_INVALID) for n in names]


def _nonpos(names):
    return [('%s %d' % (n, v), {n: v}, E_INVALID) for n in names for v in (0, -1)]


def _off(names, good):
    return [('%s misaligned by 4 bytes' % n, {n: good[n] + '+4'}, E_INVALID) for n in names]


@pytest.mark.gpu
def test_channel_affine_entries_reject_bad_arguments_and_leave_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    ptr = dict(x='@0', scale='@4096', shift='@4160', res='@1024', rscale='@4224', rshift='@4288', out='@2048')
    order = ['x', 'scale', 'shift', 'res', 'rscale', 'rshift', 'relu', 'N', 'C', 'HW', 'out']
    good = dict(ptr, relu=1, N=2, C=4, HW=16)
    r_without = [('rscale without res', dict(res=None, rshift=None), E_INVALID), ('rshift without res', dict(res=None, rscale=None), E_INVALID)]
    _entry_check(lib.rmnet_channel_affine_f32, order, good, _nulls(['x', 'out']) + _nonpos(['N', 'C', 'HW']) + r_without,
                 [dict(), dict(res=None, rscale=None, rshift=None), dict(x='@0+4')])
    order = ['x', 'scale', 'shift', 'res', 'rscale', 'rshift', 'relu', 'rows', 'C', 'out']
    good = dict(ptr, relu=1, rows=32, C=4)
    cases = (_nulls(['x', 'out']) + _nonpos(['rows', 'C']) + r_without + [('C %d' % c, dict(C=c), E_INVALID) for c in (1, 2, 3, 6)] +
             _off(['x', 'scale', 'shift', 'res', 'rscale', 'rshift', 'out'], good))
    _entry_check(lib.rmnet_channel_affine_nhwc_f32, order, good, cases, [dict(), dict(res=None, rscale=None, rshift=None), dict(scale=None, shift=None)])


@pytest.mark.gpu
def test_upsample2x_add_entries_reject_bad_arguments_and_leave_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    order = ['x', 'skip', 'N', 'C', 'h', 'w', 'out']
    good = dict(x='@0', skip='@1024', out='@2048', N=1, C=4, h=4, w=4)
    _entry_check(lib.rmnet_upsample2x_add_f32, order, good, _nulls(['x', 'out']) + _nonpos(['N', 'C', 'h', 'w']), [dict(), dict(skip=None), dict(out='@2048+4')])
    cases = (_nulls(['x', 'out']) + _nonpos(['N', 'C', 'h', 'w']) + [('C %d' % c, dict(C=c), E_INVALID) for c in (1, 2, 3, 6)] +
             _off(['x', 'skip', 'out'], good))
    _entry_check(lib.rmnet_upsample2x_add_nhwc_f32, order, good, cases, [dict(), dict(skip=None)])


@pytest.mark.gpu
def test_affine_relu_maxpool_entries_reject_bad_arguments_and_leave_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    order = ['x', 'scale', 'shift', 'N', 'C', 'H', 'W', 'out']
    good = dict(x='@0', scale='@4096', shift='@4160', out='@2048', N=1, C=4, H=8, W=8)
    _entry_check(lib.rmnet_affine_relu_maxpool_f32, order, good, _nulls(['x', 'out']) + _nonpos(['N', 'C', 'H', 'W']),
                 [dict(), dict(scale=None, shift=None), dict(x='@0+4')])
    cases = (_nulls(['x', 'out']) + _nonpos(['N', 'C', 'H', 'W']) + [('C %d' % c, dict(C=c), E_INVALID) for c in (1, 2, 3, 6)] +
             _off(['x', 'scale', 'shift', 'out'], good))
    _entry_check(lib.rmnet_affine_relu_maxpool_nhwc_f32, order, good, cases, [dict(), dict(scale=None, shift=None)])


@pytest.mark.gpu
def test_soft_aggregate_entry_rejects_bad_arguments_and_leaves_the_buffers_alone():
    from rmnet_amd import _lib
    lib = _lib.load()
    begin = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev())
    order = ['dec', 'begin', 'B', 'K', 'Hp', 'Wp', 'pad_l', 'pad_t', 'H', 'W', 'logit', 'prob']
    good = dict(dec='@0', begin=('raw', begin.data_ptr()), B=2, K=3, Hp=8, Wp=10, pad_l=2, pad_t=1, H=6, W=7, logit='@4096', prob='@8192')
    cases = (_nulls(['dec', 'begin', 'logit']) + _nonpos(['B', 'K', 'H', 'W']) +
             [('pad_l -1', dict(pad_l=-1), E_INVALID), ('pad_t -1', dict(pad_t=-1), E_INVALID),
              ('pad_l + W = Wp + 1', dict(pad_l=4), E_INVALID), ('pad_t + H = Hp + 1', dict(pad_t=3), E_INVALID),
              ('W = Wp + 1 without padding', dict(pad_l=0, W=11), E_INVALID), ('H = Hp + 1 without padding', dict(pad_t=0, H=9), E_INVALID),
              ('B 65536', dict(B=65536), E_UNSUPPORTED)])
    # the padding arithmetic's other side: pad + size == padded size is accepted
    _entry_check(lib.rmnet_soft_aggregate_f32, order, good, cases,
                 [dict(), dict(prob=None), dict(pad_l=3), dict(pad_t=2), dict(pad_l=0, pad_t=0, H=8, W=10)])


# ================================================================================================ GPU: the wrappers
@pytest.mark.gpu
def test_upsample2x_add_wrapper_refuses_an_out_of_the_other_layout():
    """NCHW operands with a channels-last ``out`` used to pass the checks and run the NCHW kernel on out's storage: right values,
    wrong places.  The first half shows that layout through the C entry, the second that the wrapper now raises and writes nothing;
    the lenient direction (channels-last operands, NCHW out: a NEW tensor is returned, out untouched) stays."""
    from rmnet_amd import _lib, ops
    rng = _rng(12)
    x, s = _randn(rng, (2, 8, 3, 5)), _randn(rng, (2, 8, 6, 10))
    want = G.upsample_f32(x, s)
    xd, sd = _t(x), _t(s)
    o = _cl(torch.full((2, 8, 6, 10), SENT, device=dev()))
    rc = _lib.load().rmnet_upsample2x_add_f32(_p(xd.data_ptr()), _p(sd.data_ptr()), 2, 8, 3, 5, _p(o.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
    storage = o.permute(0, 2, 3, 1).contiguous().flatten()              # o's memory, in order
    _assert_bits(storage.view(2, 8, 6, 10), want, 'the NCHW kernel on a channels-last tensor: its STORAGE holds the NCHW result')
    assert not torch.equal(o, _t(want))                                 # ... so the tensor itself does not
    o.fill_(SENT)
    with pytest.raises(RuntimeError, match='memory format'):
        ops.upsample2x_add(xd, sd, out=o)
    with pytest.raises(RuntimeError, match='memory format'):
        ops.upsample2x_add(xd, None, out=o)
    torch.cuda.synchronize()
    assert bool((o == SENT).all())
    # lenient: channels-last operands, NCHW out -> a new channels-last tensor; out is not written
    o2 = torch.full((2, 8, 6, 10), SENT, device=dev())
    got = ops.upsample2x_add(_cl(xd), _cl(sd), out=o2)
    assert got is not o2 and got.is_contiguous(memory_format=torch.channels_last) and bool((o2 == SENT).all())
    _assert_bits(got, want, 'channels-last operands, NCHW out')
    sk = sd.clone()                                                     # networks.Refine's call: out = skip, skip NCHW, x channels-last
    got = ops.upsample2x_add(_cl(xd), sk, out=sk)
    assert got is not sk and torch.equal(sk, sd)
    _assert_bits(got, want, 'channels-last x, NCHW skip passed as out')
    o3 = _cl(torch.empty(2, 8, 6, 10, device=dev()))                    # and the matching layouts still write in place
    assert ops.upsample2x_add(_cl(xd), _cl(sd), out=o3) is o3
    _assert_bits(o3, want, 'channels-last operands and out')


@pytest.mark.gpu
def test_glue_wrappers_layout_rules():
    from rmnet_amd import ops
    rng = _rng(13)
    x6, r6 = _randn(rng, (2, 6, 5, 7)), _randn(rng, (2, 6, 5, 7))
    sc, sh = _randn(rng, 6), _randn(rng, 6)
    with pytest.raises(RuntimeError, match='C % 4'):                   # channels-last channel_affine needs C % 4 == 0
        ops.channel_affine(_cl(_t(x6)), _t(sc), _t(sh))
    got = ops.affine_relu_maxpool(_cl(_t(x6)), _t(sc), _t(sh))         # the pool falls back to the NCHW kernel and result
    assert got.is_contiguous()
    _assert_bits(got, G.maxpool_f32(x6, sc, sh), 'channels-last pool with C % 4 != 0')
    x, r = _randn(rng, (2, 8, 5, 7)), _randn(rng, (2, 8, 5, 7))
    par = [_randn(rng, 8) for _ in range(4)]
    want = G.channel_affine_f32(x, par[0], par[1], r, par[2], par[3], 'leaky')
    for xcl in (False, True):                                           # res in the OTHER layout is converted, not misread
        xd, rd = (_cl(_t(x)), _t(r)) if xcl else (_t(x), _cl(_t(r)))
        got = ops.channel_affine(xd, _t(par[0]), _t(par[1]), rd, _t(par[2]), _t(par[3]), relu='leaky')
        assert got.is_contiguous(memory_format=torch.channels_last) if xcl else got.is_contiguous()
        _assert_bits(got, want, 'channel_affine, res in the other layout (x channels-last: %s)' % xcl)
    s = _randn(rng, (2, 8, 10, 14))
    wantu = G.upsample_f32(x, s)
    for xcl in (False, True):                                           # skip in the other layout: the channels-last kernel either way
        xd, sd = (_cl(_t(x)), _t(s)) if xcl else (_t(x), _cl(_t(s)))
        got = ops.upsample2x_add(xd, sd)
        assert got.is_contiguous(memory_format=torch.channels_last)
        _assert_bits(got, wantu, 'upsample2x_add, skip in the other layout (x channels-last: %s)' % xcl)
    with pytest.raises(RuntimeError):                                   # out of the other layout: channel_affine refuses both directions
        ops.channel_affine(_t(x), out=_cl(torch.empty(2, 8, 5, 7, device=dev())))
    with pytest.raises(RuntimeError):
        ops.channel_affine(_cl(_t(x)), out=torch.empty(2, 8, 5, 7, device=dev()))
