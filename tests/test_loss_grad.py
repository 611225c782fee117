# -*- coding: utf-8 -*-
"""The gradient of the training loss (Lovasz-softmax + NLL, core/train.py:180) without a sort: the two numpy restatements of
tests/loss_grad_ref.py pinned by hand, by torch autograd and by the reference's recorded gradients; rmnet_amd.losses.training_loss
on the CPU; and csrc/val_loss_bwd.hip on the GPU, every bit of the gradient and of the tables against the restatement.  The bounds
are derived in loss_grad_ref.py.

One departure from the reference is deliberate and checked below: where a probability that is NOT the label's is exactly 0, the
reference's gradient is NaN (torch.log's backward divides the zero gradient of a non-target channel by p: 0 / 0); here that element
is the Lovasz part alone, as the formula [c == label] * (-1 / (p_label * n_good)) says."""

import ctypes
import os

import numpy as np
import pytest
import torch

import loss_grad_ref as ref
import val_loss_ref as vr
from conftest import GOLDEN

INF = float('inf')
NAN = float('nan')


def f32(a):
    return np.asarray(a, np.float32)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def clip_of(pixels, K):
    """pixels: [(label, (p_0 .. p_{K-1})), ...] -> probs [1,K,1,n], labels [1,1,n]."""
    labels = np.asarray([p[0] for p in pixels], np.uint8).reshape(1, 1, -1)
    probs = f32([p[1] for p in pixels]).reshape(1, -1, K).transpose(0, 2, 1)[:, :, None, :]
    return np.ascontiguousarray(probs), labels


def per_pixel(grad):
    """[1,K,1,n] -> [n][K]"""
    return np.asarray(grad)[0, :, 0, :].T


# name -> (probs, labels, K, expected gradient [pixel][class], literal too?): every figure is worked out by hand from
# w_fg = 1 / (G + B), w_bg = (G - F) / ((G + B)(G + B + 1)) over the sorted errors, or the table formulas where a bin ties; bins = 16
def hand_cases():
    c = {}
    # one foreground pixel only: class 0 absent, class 1 has G = 1, weight 1: -1 / 1 - 1 / (0.75 * 1)
    c['one_foreground_pixel'] = (*clip_of([(1, (0.25, 0.75))], 2), 2, [[0, -7 / 3]], True)
    # class 2 absent.  class 0: px0 fg e 0.5 -> 1; px1 bg e 0.25, F = 1 -> 0.  class 1: px1 fg e 0.375 -> 1; px0 bg e 0.25 -> 0.
    # n_present 2, n_good 2: px0 -1/2 - 1/(0.5 * 2); px1 -1/2 - 1/(0.625 * 2)
    c['class_absent'] = (*clip_of([(0, (0.5, 0.25, 0.25)), (1, (0.25, 0.625, 0.125))], 3), 3, [[-1.5, 0, 0], [0, -1.3, 0]], True)
    # class 0 (G = 2: px0, px3), by error: px2 bg .875 -> 2/(2*3) = 1/3; px0 fg .75, B = 1 -> 1/3; px1 bg .5, F = 1, B = 1 -> 1/12;
    # px3 fg .0625, B = 2 -> 1/4.  class 1 (G = 2: px1, px2): px2 fg .875 -> 1/2; px0 bg .75, F = 1 -> 1/6; px1 fg .5, B = 1 -> 1/3;
    # px3 bg, F = 2 -> 0.  n_present 2, n_good 4
    four = [(0, (0.25, 0.75)), (1, (0.5, 0.5)), (1, (0.875, 0.125)), (0, (0.9375, 0.0625))]
    g4 = [[-1 / 6 - 1, 1 / 12], [1 / 24, -1 / 6 - 1 / 2], [1 / 6, -1 / 4 - 2], [-1 / 8 - 4 / 15, 0]]
    c['four_pixels'] = (*clip_of(four, 2), 2, g4, True)
    # one bin holds a foreground and a background pixel of each class (key 8): F> 0, F>= 1, B> 0, B>= 1:
    # g_fg = (1/1 + 1/2) / 2 = 3/4, g_bg = (1 - 1/2) / (1 * 2) = 1/4.  (The sort gives 1 and 0 in one order, 1/2 and 1/2 in the other.)
    c['a_tie_in_one_bin'] = (*clip_of([(0, (0.5, 0.5)), (1, (0.5, 0.5))], 2), 2, [[-3 / 8 - 1, 1 / 8], [1 / 8, -3 / 8 - 1]], False)
    # e == 0 on a foreground pixel (px0 class 0, px2 class 1) and on a background pixel (px2 class 0, px0 class 1): no Lovasz part,
    # although bin 0 of class 0 has g_fg = (1/2 + 1/3) / 2 and g_bg = (1 - 1/2) / (2 * 3).  class 0: px1 bg e .25 -> 1/2.
    # class 1 (G = 2): px1 fg e .25 -> 1/2.  n_present 2, n_good 3
    c['zero_error'] = (*clip_of([(0, (1.0, 0.0)), (1, (0.25, 0.75)), (1, (0.0, 1.0))], 2), 2,
                       [[-1 / 3, 0], [1 / 4, -1 / 4 - 4 / 9], [0, -1 / 3]], True)
    c['ignored_pixel'] = (*clip_of(four + [(255, (0.5, 0.5))], 2), 2, g4 + [[0, 0]], True)
    c['label_beyond_k'] = (*clip_of(four + [(2, (0.5, 0.5))], 2), 2, g4 + [[0, 0]], True)
    c['nan_probability'] = (*clip_of(four + [(0, (NAN, 0.5))], 2), 2, g4 + [[0, 0]], True)
    # p_label == 0 (px0): -inf.  class 0 (G = 1): px0 fg e 1 -> 1; px2 bg e .9375 and px1 bg, F = 1 -> 0.  class 1 (G = 2: px1, px2):
    # px0 bg e 1 -> 2/(2*3) = 1/3; px2 fg e .9375, B = 1 -> 1/3; px1 fg e .25, B = 1 -> 1/3.  n_present 2, n_good 3
    c['zero_target_probability'] = (*clip_of([(0, (0.0, 1.0)), (1, (0.25, 0.75)), (1, (0.9375, 0.0625))], 2), 2,
                                    [[-INF, 1 / 6], [0, -1 / 6 - 4 / 9], [0, -1 / 6 - 16 / 3]], True)
    return c


HAND = hand_cases()
# the planted fault -> the hand case that catches it
CAUGHT_BY = {'ge_for_gt_f': 'a_tie_in_one_bin', 'ge_for_gt_b': 'four_pixels', 'f_for_b': 'four_pixels', 'no_sign': 'four_pixels',
             'sign_at_zero': 'zero_error', 'mean_over_all': 'class_absent', 'n_valid': 'label_beyond_k', 'nll_wrong_channel': 'four_pixels',
             'bad_not_zeroed': 'nan_probability', 'top_has_width': 'zero_target_probability'}


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid='ignore'):                                       # (-inf against -inf: equal)
        return bool(np.all((np.abs(got - want) <= tol) | (got == want)))


def table_ok(name, faults=()):
    probs, labels, K, want, _ = HAND[name]
    got = per_pixel(ref.table_grad(probs, labels, 255, 16, faults)['grad'])
    return close(got, want, 4 * ref.V * np.maximum(np.abs(np.nan_to_num(np.asarray(want, np.float64), neginf=0.0)), 1.0))


@pytest.mark.parametrize('name', sorted(HAND))
def test_restatements_give_the_hand_written_answers(name):
    probs, labels, K, want, literal_too = HAND[name]
    assert table_ok(name)
    lit = per_pixel(ref.literal(probs, labels)['grad'])
    if literal_too:
        assert close(lit, want, 4 * ref.EPS), (lit, want)
    else:
        assert not close(lit, want, 1e-3)                                     # one order of the tie, not the mean of the two


@pytest.mark.parametrize('fault', ref.FAULTS)
def test_every_planted_fault_is_caught_by_its_case(fault):
    assert set(CAUGHT_BY) == set(ref.FAULTS)
    assert table_ok(CAUGHT_BY[fault]) and not table_ok(CAUGHT_BY[fault], (fault,))


def torch_reference_style(probs, labels, dtype=torch.float64):
    """Autograd through the loss written the way the reference writes it (sort, detached permutation, cumsums, dot, mean; NLL as
    -log p_label / n), on the good pixels that tests/val_loss_ref.py selects: the pin of ``literal`` by torch."""
    good, _, _ = vr.pixel_classes(probs, labels)
    x = t(probs).to(dtype).requires_grad_(True)
    p = x.permute(0, 2, 3, 1)[t(good)]
    lab = t(labels)[t(good)].long()
    losses = []
    for c in range(probs.shape[1]):
        fg = (lab == c).to(dtype)
        if fg.sum() == 0:
            continue
        errors = (fg - p[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        gs = fg[perm.detach()]
        jac = 1.0 - (gs.sum() - gs.cumsum(0)) / (gs.sum() + (1 - gs).cumsum(0))
        if len(gs) > 1:
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(errors_sorted, jac))
    loss = sum(losses) / max(len(losses), 1) + (-(p.gather(1, lab.view(-1, 1)).log()).sum() / max(lab.numel(), 1))
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize('name', sorted(HAND))
def test_literal_restatement_is_what_torch_autograd_gives(name):
    probs, labels, K, want, _ = HAND[name]
    lit = ref.literal(probs, labels)
    loss, grad = torch_reference_style(probs, labels)                         # (a pixel that is left out never enters the graph: 0)
    assert not np.isnan(grad).any()
    assert close(lit['grad'], grad, 4 * ref.EPS * np.maximum(np.abs(np.nan_to_num(grad, neginf=0.0)), 1.0))
    # (the literal restatement takes the errors in fp32, as the reference does: v relative to the Lovasz value)
    assert close(lit['loss'], loss, ref.V * lit['lovasz'] + 8 * ref.EPS * max(abs(loss), 1.0) if np.isfinite(loss) else 0)


def test_literal_restatement_against_torch_autograd_on_random_clips():
    rng = np.random.default_rng(2)
    for K, peak in ((1, 1.0), (2, 3.0), (3, 0.5), (4, 6.0)):
        probs, labels = vr.softmax_clip(rng, 2, K, 5, 7, peak=peak, ignore=0.2)
        loss, grad = torch_reference_style(probs, labels)
        lit = ref.literal(probs, labels)
        assert close(lit['grad'], grad, 4 * ref.EPS * np.maximum(np.abs(grad), 1.0)) and close(lit['loss'], loss, ref.V * lit['lovasz'] + 8 * ref.EPS * max(loss, 1.0))


# ------------------------------------------------------------------------------------------------ table against literal
def finite_close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid='ignore'):                                       # (-inf against -inf: equal)
        return bool(np.all((np.abs(got - want) <= tol) | (got == want)))


@pytest.mark.parametrize('K,bins', [(1, 128), (2, 1 << 10), (3, 1 << 10), (3, 1 << 20), (11, 1 << 10)])
def test_table_equals_the_sort_where_no_bin_holds_two_pixels(K, bins):
    rng = np.random.default_rng(K * 7 + bins)
    probs, labels = ref.distinct_clip(rng, 2, K, 5, 7, bins, ignore=0.1)
    tab, lit = ref.table_grad(probs, labels, 255, bins), ref.literal(probs, labels)
    assert tab['hist'].max() == 1
    assert tab['hist'][:, :, 0].sum() > 0 and tab['hist'][:, :, bins].sum() > 0          # e == 0 and e == 1 are there
    assert finite_close(tab['w64'], lit['w'], ref.EPS)                        # up to float64 rounding
    assert finite_close(tab['t64'], lit['t'], 0)
    assert finite_close(tab['grad'], lit['grad'], ref.table_bound(lit['w'], lit['t']))
    assert np.array_equal(np.isneginf(tab['grad']), np.isneginf(lit['grad']))


@pytest.mark.parametrize('bins', [2, 16, 1 << 10])
def test_table_and_sort_lie_inside_the_bracket_of_the_tie_orders(bins):
    rng = np.random.default_rng(bins + 3)
    for K in (1, 2, 3, 4):
        for peak, ignore in ((0.0, 0.0), (1.0, 0.2), (6.0, 0.0), (20.0, 0.3)):
            probs, labels = vr.softmax_clip(rng, 2, K, 5, 7, peak=peak, ignore=ignore)
            tab, lit = ref.table_grad(probs, labels, 255, bins), ref.literal(probs, labels)
            lo, hi = ref.grad_bracket(probs, labels, 255, bins)
            assert (lo <= hi).all()
            for name, w in (('table', tab['w64']), ('sort', lit['w'])):
                assert (w >= lo - ref.EPS).all() and (w <= hi + ref.EPS).all(), (name, K, peak, bins)
            fine_lo, fine_hi = ref.grad_bracket(probs, labels)                 # ties by equal errors: inside the bins' bracket
            assert (fine_lo >= lo - ref.EPS).all() and (fine_hi <= hi + ref.EPS).all()


@pytest.mark.parametrize('bins', [2, 16, 1 << 10])
def test_weights_of_a_class_add_up_to_one_and_of_a_bin_to_its_jaccard_step(bins):
    rng = np.random.default_rng(bins + 5)
    for K in (1, 3, 4):
        probs, labels = vr.softmax_clip(rng, 2, K, 5, 7, peak=2.0, ignore=0.1, n_labels=max(K - 1, 1))
        tab = ref.table_grad(probs, labels, 255, bins)
        hist, t64 = tab['hist'].astype(np.float64), tab['tables64']
        for c in range(K):
            mass = hist[c, 0] * t64[c, 0] + hist[c, 1] * t64[c, 1]            # what the pixels of each bin carry together
            G = hist[c, 1].sum()
            if G == 0:
                assert (t64[c] == 0).all()
                continue
            fgt, fge = ref.suffix_counts(tab['hist'][c, 1])
            bgt, bge = ref.suffix_counts(tab['hist'][c, 0])
            step = (1.0 - (G - fge) / (G + bge)) - (1.0 - (G - fgt) / (G + bgt))
            assert np.abs(mass - step).max() <= ref.EPS, (K, c, bins)
            assert abs(mass.sum() - 1.0) <= (bins + 1) * ref.U + ref.EPS
        assert tab['n_present'] == max(K - 1, 1) or K == 1


# ------------------------------------------------------------------------------------------------ the reference's recorded gradients
def fixture():
    d = np.load(os.path.join(GOLDEN, 'loss_grad.npz'))
    return [(str(n), bool(tied), d[str(n) + '_probs'], d[str(n) + '_labels'], float(d[str(n) + '_loss']), d[str(n) + '_grad'])
            for n, tied in zip(d['names'], d['tied'])]


def reference_nan_mask(probs, labels):
    """Where the reference's gradient is NaN: a probability of exactly 0 on a channel that is not the label's, on a counted pixel."""
    K = probs.shape[1]
    onehot = labels[:, None] == np.arange(K)[None, :, None, None]
    return (probs == 0) & ~onehot & (labels != 255)[:, None]


def test_the_torch_route_reproduces_the_recorded_gradients_of_the_reference():
    """tests/golden/loss_grad.npz: the reference's LovaszLoss + NLLLoss and backward() (fp32) on nine 70-pixel clips with K = 2, 3,
    11.  Where every class's errors differ the sort has one order and route='torch' equals the record within ref_grad_bound; on the
    tied clips the record is one of the tie orders and lies in the bracket, widened by the same bound."""
    from rmnet_amd import losses
    cases = fixture()
    assert len(cases) == 9 and sum(c[1] for c in cases) == 4 and {c[2].shape[1] for c in cases} == {2, 3, 11}
    for name, tied, probs, labels, loss, grad in cases:
        nan = reference_nan_mask(probs, labels)
        assert np.array_equal(np.isnan(grad), nan), name                       # the one departure, exactly where it is expected
        x = t(probs).requires_grad_(True)
        out = losses.training_loss(x, t(labels), route='torch')
        out.backward()
        got = x.grad.numpy()
        lit = ref.literal(probs, labels)
        assert got.dtype == np.float32 and (tied or finite_close(got, lit['grad'], ref.torch_route_bound(lit['w'], lit['t'])))
        bound = ref.ref_grad_bound(lit['w'], lit['t'], lit['n_present'])
        loss_bound = vr.ref_lovasz_bound(lit['n_good']) + (vr.ref_nll_bound(lit['n_good'], abs(lit['nll'])) if np.isfinite(lit['nll']) else 0)
        value = float(out.detach())
        assert value == loss or abs(value - loss) <= loss_bound + ref.V * abs(loss), name
        keep = ~nan
        assert np.array_equal(np.isneginf(got), np.isneginf(np.where(keep, grad, 0))), name
        fin = keep & np.isfinite(grad)
        with np.errstate(invalid='ignore'):
            err = np.abs(got.astype(np.float64) - grad)[fin]
        print('%-20s %s  largest |torch route - reference| / bound %.3f' % (name, 'tied' if tied else 'distinct', (err / bound[fin]).max() if not tied else NAN))
        if not tied:
            assert (err <= bound[fin]).all(), name
        lo, hi = ref.grad_bracket(probs, labels)
        if name.startswith('tied_k'):                                         # (a real bracket; on 'tied_flat' only pixels of one
            assert (hi - lo).max() > 100 * bound.max()                         # kind tie, after all foregrounds: every order agrees)
        lo, hi = lo + lit['t'], hi + lit['t']
        for which, g in (('reference', grad), ('torch route', got)):
            g = g.astype(np.float64)
            assert ((g >= lo - bound) & (g <= hi + bound))[fin].all(), (name, which)


def test_training_loss_on_cpu_tensors():
    from rmnet_amd import losses
    for name in sorted(HAND):
        probs, labels, K, want, literal_too = HAND[name]
        x = t(probs).requires_grad_(True)
        out = losses.training_loss(x, t(labels), bins=16)                     # CPU tensors: the sort, whatever the route
        assert out.dim() == 0 and out.dtype == torch.float64 and out.requires_grad
        out.backward()
        lit = ref.literal(probs, labels)
        assert close(x.grad.numpy(), lit['grad'], ref.torch_route_bound(lit['w'], lit['t'])), name
        value = float(out.detach())
        assert value == lit['loss'] or abs(value - lit['loss']) <= 8 * ref.EPS * max(abs(lit['loss']), 1.0)
        with torch.no_grad():
            assert not losses.training_loss(t(probs), t(labels)).requires_grad
        same = losses.training_loss(x, t(labels), route='hip')                # a CPU tensor never takes the device route
        assert float(same.detach()) == value
    # the value is the validation loss's
    rng = np.random.default_rng(4)
    probs, labels = vr.softmax_clip(rng, 2, 3, 5, 7, peak=3.0, ignore=0.2)
    assert abs(float(losses.training_loss(t(probs), t(labels))) - float(losses.validation_loss(t(probs), t(labels))['loss'])) <= 4 * ref.EPS
    # all pixels ignored: no class is present and the NLL is 0 / 0
    out = losses.training_loss(t(probs).requires_grad_(True), t(np.full_like(labels, 255)))
    assert np.isnan(float(out.detach()))


def test_training_loss_argument_errors():
    from rmnet_amd import losses, ops
    p, l = torch.rand(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='expected probs'):
        losses.training_loss(p[0], l)
    with pytest.raises(RuntimeError, match='expected probs'):
        losses.training_loss(p, l[:, :3])
    with pytest.raises(RuntimeError, match='uint8'):
        losses.training_loss(p, l.long())
    with pytest.raises(RuntimeError, match='float32'):
        losses.training_loss(p.half(), l)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.clip_loss_grad(p, l)
    assert losses.TRAIN_DEVICE_ROUTE in ('hip', 'torch')


def test_gradcheck_of_the_torch_route_where_the_errors_differ():
    """float64, at points whose per-class errors are pairwise different and away from 0 and 1 (the loss is differentiable there)."""
    from rmnet_amd import losses
    rng = np.random.default_rng(6)
    for K in (2, 3):
        probs, labels = ref.distinct_clip(rng, 1, K, 2, 3, 64)
        probs = np.clip(probs, 1 / 64, 63 / 64) + f32(rng.permutation(probs.size).reshape(probs.shape)) / 8192      # apart by >= 2^-13
        x = t(probs).double().requires_grad_(True)
        lab = t(labels)
        assert torch.autograd.gradcheck(lambda q: losses.training_loss(q, lab, route='torch'), (x,), eps=1e-7, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ the C entry's argument rules
def test_c_entry_argument_rules():
    from rmnet_amd import _lib
    lib = _lib.load()
    wsb = lib.rmnet_clip_loss_grad_workspace_bytes
    for K, bins in ((3, 16), (1, 2), (11, 1 << 20), (255, 1 << 22)):
        assert wsb(K, bins) == lib.rmnet_clip_loss_workspace_bytes(K, bins) > 0
    for K, bins in ((0, 16), (256, 16), (-1, 16), (3, 0), (3, 1), (3, 3), (3, 24), (3, 1 << 23), (3, -16)):
        assert wsb(K, bins) == 0, (K, bins)
    buf, gbuf = (ctypes.c_double * 4096)(), (ctypes.c_double * 4096)()
    p, g = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(gbuf, ctypes.c_void_p)
    big = 1 << 20
    call = lib.rmnet_clip_loss_grad_f32
    INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -4
    base = lambda: [p, p, 2, 3, 5, 7, 255, 16, g, p, p, p, p, big, None]
    for i in (0, 1, 8, 9, 10, 11):                                 # probs, labels, grad, per_class, nll_sum, counts
        args = base()
        args[i] = None
        assert call(*args) == INVALID, i
    for i, values in ((3, (0, -1, 256)), (7, (0, 1, 3, 24, 1 << 23, -2)), (2, (0, -1)), (4, (0,)), (5, (0,))):
        for v in values:
            args = base()
            args[i] = v
            assert call(*args) == INVALID, (i, v)
    args = base()
    args[4], args[5] = 1 << 15, 1 << 15                            # N*H*W = 2^31
    assert call(*args) == UNSUPPORTED
    args = base()
    args[12] = None
    assert call(*args) == WORKSPACE
    args = base()
    args[13] = wsb(3, 16) - 1
    assert call(*args) == WORKSPACE
    for i in (0, 8, 9, 10, 11, 12):                                # a misaligned probs / grad / per_class / nll_sum / counts / workspace
        args = base()
        args[i] = ctypes.c_void_p(args[i].value + (2 if i in (0, 8) else 4))
        assert call(*args) == INVALID, i
    n_bytes = 2 * 3 * 5 * 7 * 4
    for shift in (0, 4, n_bytes - 4, -4, 4 - n_bytes):             # grad overlaps probs
        args = base()
        args[0] = ctypes.c_void_p(p.value + 1024)
        args[8] = ctypes.c_void_p(p.value + 1024 + shift)
        assert call(*args) == INVALID, shift


def test_the_new_kernels_are_allocated_the_lds_they_declare_and_no_scratch(tmp_path):
    """tests/test_kernel_resources.py's rule for vl_grad_table and vl_grad_apply: no static __shared__ declaration (their LDS is
    dynamic, sized at launch), so 0 bytes of fixed LDS; no scratch and no spill.  Read from a compile-only gfx950 build."""
    import test_kernel_resources as tkr
    from rmnet_amd import build
    assert 'val_loss_bwd.hip' in build.SOURCES
    kernels = tkr._kernels(tkr._compile('val_loss_bwd.hip', str(tmp_path / 'val_loss_bwd.s')))
    assert len(kernels) == 2
    for frag in ('13vl_grad_tableE', '13vl_grad_applyE'):
        k = tkr._one(kernels, frag)
        print(frag, k)
        assert k['group_segment_fixed_size'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (frag, k)


# ------------------------------------------------------------------------------------------------ the kernels
GUARD_P, GUARD_L = 7.0, 0          # a guard probability is a bad one and a guard label a counted one: a read past an end shows


def spoil(rng, probs, labels, K):
    """Ignored pixels, labels >= K and probabilities outside [0, 1] sprinkled over a clip (in place): the recipe of
    tests/test_val_loss.py."""
    N, _, H, W = probs.shape
    n = max(1, labels.size // 10)
    flat = labels.reshape(-1)
    flat[rng.integers(0, flat.size, n)] = 255
    if K < 255:
        flat[rng.integers(0, flat.size, n)] = rng.integers(K, 255, n)
    for bad in (np.nan, 1.5, -0.1, np.inf, -np.inf, np.float32(1) + np.float32(2.0 ** -23), -1e-30):
        for _ in range(max(1, n // 4)):
            probs[rng.integers(N), rng.integers(K), rng.integers(H), rng.integers(W)] = bad


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_call(probs, labels, ignore=255, bins=16, off_p=0, off_l=0, off_g=0):
    """ops.clip_loss_grad on copies of the arrays placed ``off_p`` / ``off_g`` elements and ``off_l`` bytes into guarded buffers; the
    gradient goes into a buffer pre-filled with NaN, whose guards must stay NaN."""
    from rmnet_amd import _lib, ops
    lib = _lib.load()
    pb = torch.full((probs.size + 64,), GUARD_P, dtype=torch.float32, device='cuda')
    lb = torch.full((labels.size + 64,), GUARD_L, dtype=torch.uint8, device='cuda')
    gb = torch.full((probs.size + 64,), NAN, dtype=torch.float32, device='cuda')
    at_p, at_l, at_g = 16 + off_p, 16 + off_l, 16 + off_g
    pb[at_p:at_p + probs.size] = t(probs).reshape(-1).cuda()
    lb[at_l:at_l + labels.size] = t(labels).reshape(-1).cuda()
    pv, lv = pb[at_p:at_p + probs.size].view(probs.shape), lb[at_l:at_l + labels.size].view(labels.shape)
    gv = gb[at_g:at_g + probs.size].view(probs.shape)
    assert pv.data_ptr() % 16 == (4 * off_p) % 16 and lv.data_ptr() % 16 == off_l % 16 and gv.data_ptr() % 16 == (4 * off_g) % 16
    N, K, H, W = probs.shape
    per_class = torch.empty(K, 3, dtype=torch.float64, device='cuda')
    nll_sum = torch.empty((), dtype=torch.float64, device='cuda')
    counts = torch.empty(3, dtype=torch.int64, device='cuda')
    ws = torch.empty(lib.rmnet_clip_loss_grad_workspace_bytes(K, bins), dtype=torch.uint8, device='cuda')
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib.rmnet_clip_loss_grad_f32(ptr(pv), ptr(lv), N, K, H, W, ignore, bins, ptr(gv), ptr(per_class), ptr(nll_sum), ptr(counts),
                                      ptr(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    tables = ws[:K * 2 * (bins + 1) * 4].view(torch.float32).view(K, 2, bins + 1)
    got = {'grad': gv.cpu().numpy(), 'tables': tables.cpu().numpy(), 'per_class': per_class.cpu().numpy(), 'nll_sum': nll_sum.cpu().numpy(),
           'counts': counts.cpu().numpy()}
    for buf, n, at, g in ((pb, probs.size, at_p, GUARD_P), (lb, labels.size, at_l, GUARD_L)):
        assert bool((buf[:at] == g).all()) and bool((buf[at + n:] == g).all())
    assert bool(torch.isnan(gb[:at_g]).all()) and bool(torch.isnan(gb[at_g + probs.size:]).all())
    assert bits(pv.cpu().numpy()).tobytes() == bits(probs).tobytes()            # the inputs are untouched
    fwd = ops.clip_loss(pv, lv, ignore, bins)
    for k in ('per_class', 'nll_sum', 'counts'):                              # the forward entry's outputs, in every bit
        assert fwd[k].cpu().numpy().tobytes() == got[k].tobytes(), k
    return got


def check_against_restatement(probs, labels, ignore=255, bins=16, off_p=0, off_l=0, off_g=0, tag=None):
    got = device_call(probs, labels, ignore, bins, off_p, off_l, off_g)
    want = ref.table_grad(probs, labels, ignore, bins)
    tag = (tag, probs.shape, bins, off_p, off_l, off_g)
    assert not np.isnan(got['grad']).any(), tag                               # every element was written
    bad_t = bits(got['tables']) != bits(want['tables'])
    assert not bad_t.any(), (tag, 'tables', int(bad_t.sum()), np.argwhere(bad_t)[:4].tolist())
    bad_g = bits(got['grad']) != bits(want['grad'])
    assert not bad_g.any(), (tag, 'grad', int(bad_g.sum()), np.argwhere(bad_g)[:4].tolist(), got['grad'][bad_g][:4], want['grad'][bad_g][:4])
    assert got['counts'][0] == want['n_good']
    return got, want


@pytest.mark.gpu
def test_every_bit_matches_at_every_plane_size_and_alignment():
    """Plane sizes 1 .. 65 and 255 .. 257 (with N > 1 the frame boundaries fall inside the 4-pixel groups), N = 1 .. 3, label offsets
    0 .. 15 bytes, probability and gradient offsets 0 .. 3 elements in all sixteen pairs, K = 1, 2, 3, 11, bins 2 and 16 (the whole
    table in LDS at these K), every fourth clip spoilt."""
    rng = np.random.default_rng(43)
    pairs = set()
    for i, hw in enumerate(list(range(1, 66)) + [255, 256, 257]):
        N, K = 1 + i % 3, (1, 2, 3, 11)[(i // 3) % 4]
        H, W = (1, hw) if hw % 5 else (5, hw // 5)
        bins = (2, 16)[i % 2]
        assert ref.lds_window(K, bins) == (bins + 1, 0)
        probs, labels = vr.softmax_clip(rng, N, K, H, W, peak=(0.0, 3.0, 12.0)[i % 3], ignore=0.1)
        if i % 4 == 3:
            spoil(rng, probs, labels, K)
        pairs.add((i % 4, (i // 4) % 4))
        check_against_restatement(probs, labels, 255, bins, off_p=i % 4, off_l=i % 16, off_g=(i // 4) % 4, tag=hw)
    assert len(pairs) == 16


WINDOW_CASES = [(255, 16), (255, 2), (11, 1 << 10), (3, 1 << 12), (2, 1 << 12), (1, 1 << 13), (3, 1 << 20)]


def window_clip(K, bins):
    """(rng, probs, labels) of one case: more than one workgroup (P > 2048) unless K == 255, odd planes.  K == 1 takes uniform
    probabilities (a soft-max over one class is 1 everywhere)."""
    rng = np.random.default_rng(K + bins)
    N, H, W = (2, 5, 13) if K == 255 else (3, 37, 21)
    probs, labels = vr.softmax_clip(rng, N, K, H, W, peak=2.0 if K == 255 else 3.0, ignore=0.05)
    if K == 1:
        probs = rng.random(probs.shape).astype(np.float32)
    return rng, probs, labels


@pytest.mark.parametrize('K,bins', WINDOW_CASES)
def test_the_window_cases_reach_the_staged_and_the_gathered_entries(K, bins):
    """lds_bins' rule restated (loss_grad_ref.lds_window): except for (255, 2) the table does not fit the LDS window of its K, and
    the keys of the clip reach the staged low entries, the staged high entries and the entries in between."""
    LB, HB = ref.lds_window(K, bins)
    assert ref.lds_window(3, 16) == (17, 0) and ref.lds_window(3, 1 << 12) == (1024, 1024) and ref.lds_window(255, 16) == (8, 8)
    _, probs, labels = window_clip(K, bins)
    keys = ref.table_grad(probs, labels, 255, bins)['keys']
    if (K, bins) == (255, 2):
        assert (LB, HB) == (3, 0)
    else:
        assert HB > 0 and LB + HB < bins + 1
        assert (keys < LB).any() and (keys >= bins + 1 - HB).any() and ((keys >= LB) & (keys < bins + 1 - HB)).any()


@pytest.mark.gpu
@pytest.mark.parametrize('K,bins', WINDOW_CASES)
def test_every_bit_matches_at_every_class_count_and_beyond_the_lds_window(K, bins):
    """The cases of the test above: a clean clip, a spoilt one, one on which nothing is ignored, and one on the bin edges."""
    rng, probs, labels = window_clip(K, bins)
    N, _, H, W = probs.shape
    got, want = check_against_restatement(probs, labels, 255, bins, off_p=1, off_l=3, off_g=2)
    spoil(rng, probs, labels, K)
    got, want = check_against_restatement(probs, labels, 255, bins, off_p=2, off_l=5, off_g=1)
    assert want['n_good'] < (labels != 255).sum() and (got['grad'] == 0).any()
    check_against_restatement(probs, labels, 300, bins, off_g=3)              # nothing is ignored: label 255 is a bad label or class 254
    probs, labels = vr.grid_clip(rng, N, K, H, W, min(bins, 1 << 20))         # every probability on a bin edge, 0 and 1 included
    got, want = check_against_restatement(probs, labels, 255, bins, off_p=3)
    assert np.isneginf(got['grad']).any() and (want['hist'][:, :, bins].sum() > 0) and (want['hist'][:, :, 0].sum() > 0)


@pytest.mark.gpu
def test_distinct_errors_on_the_device_give_the_gradient_of_the_sort():
    rng = np.random.default_rng(12)
    for K, bins in ((2, 1 << 12), (3, 1 << 20)):
        probs, labels = ref.distinct_clip(rng, 3, K, 13, 21, bins, ignore=0.1)
        got, want = check_against_restatement(probs, labels, 255, bins, off_p=1, off_g=3)
        lit = ref.literal(probs, labels)
        assert want['hist'].max() == 1
        assert finite_close(got['grad'], lit['grad'], ref.table_bound(lit['w'], lit['t']) + ref.EPS)
        assert np.array_equal(np.isneginf(got['grad']), np.isneginf(lit['grad']))


@pytest.mark.gpu
def test_a_workgroup_that_takes_more_than_one_step():
    """More than 512 x 512 groups of 4 pixels: every workgroup of vl_grad_apply loops, and the last one ends inside its range."""
    rng = np.random.default_rng(6)
    N, K, H, W = 2, 2, 701, 751
    assert N * H * W > 4 * 512 * 512 and (H * W) % 4 == 3
    probs, labels = vr.softmax_clip(rng, N, K, H, W, peak=8.0, ignore=0.02)
    check_against_restatement(probs, labels, 255, 1 << 20, off_p=1, off_l=2, off_g=3)


@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from rmnet_amd import ops
    rng = np.random.default_rng(8)
    probs, labels = vr.softmax_clip(rng, 3, 3, 37, 53, peak=5.0, ignore=0.1)
    spoil(rng, probs, labels, 3)
    pv, lv = t(probs).cuda(), t(labels).cuda()
    every = lambda o: [o[k].cpu().numpy().tobytes() for k in ('per_class', 'nll_sum', 'counts', 'grad', 'tables')]
    eager = every(ops.clip_loss_grad(pv, lv, bins=1 << 16, want_tables=True))
    assert every(ops.clip_loss_grad(pv, lv, bins=1 << 16, want_tables=True)) == eager
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.clip_loss_grad(pv, lv, bins=1 << 16, want_tables=True)            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a single stream, no parallel branches
        out = ops.clip_loss_grad(pv, lv, bins=1 << 16, want_tables=True)
    for v in out.values():
        v.fill_(3)                                                            # the replay clears and rewrites everything it returns
    graph.replay()
    torch.cuda.synchronize()
    assert every(out) == eager


def _device_pair(probs, labels, bins, **kw):
    """(loss, grad) of training_loss(...).backward() on the device by both routes."""
    from rmnet_amd import losses
    out = {}
    for route in ('hip', 'torch'):
        x = t(probs).cuda().requires_grad_(True)
        loss = losses.training_loss(x, t(labels).cuda(), bins=bins, route=route, **kw)
        assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float64
        loss.backward()
        out[route] = (float(loss.detach()), x.grad.cpu().numpy())
    return out


@pytest.mark.gpu
def test_training_loss_backward_on_the_device_against_the_torch_route():
    """Distinct errors: both routes hold the sort's gradient, 'hip' with the roundings of table_bound, 'torch' with one fp32 rounding
    of its float64 sum.  Tied errors: both lie in the bracket of the tie orders of the bins."""
    rng = np.random.default_rng(14)
    for K, bins in ((2, 1 << 12), (3, 1 << 20), (11, 1 << 12)):
        probs, labels = ref.distinct_clip(rng, 2, K, 9, 13, bins, ignore=0.1)
        out = _device_pair(probs, labels, bins)
        lit = ref.literal(probs, labels)
        assert finite_close(out['torch'][1], lit['grad'], ref.torch_route_bound(lit['w'], lit['t']))
        assert finite_close(out['hip'][1], out['torch'][1], ref.table_bound(lit['w'], lit['t']) + ref.torch_route_bound(lit['w'], lit['t'])), (K, bins)
        assert np.array_equal(np.isneginf(out['hip'][1]), np.isneginf(out['torch'][1]))
        if np.isfinite(out['torch'][0]):
            logs = vr.nll_logs(probs, labels)
            assert abs(out['hip'][0] - out['torch'][0]) <= 0.5 / bins + vr.eps_device(bins) + vr.EPS + vr.nll_device_bound(logs) / logs.size
    for K, bins in ((3, 16), (2, 1 << 10)):
        probs, labels = vr.softmax_clip(rng, 2, K, 9, 13, peak=3.0, ignore=0.1)
        out = _device_pair(probs, labels, bins)
        lit = ref.literal(probs, labels)
        lo, hi = ref.grad_bracket(probs, labels, 255, bins)
        slack = ref.table_bound(lit['w'], lit['t']) + ref.torch_route_bound(lit['w'], lit['t'])
        for route in ('hip', 'torch'):
            g = out[route][1].astype(np.float64)
            assert ((g >= lo + lit['t'] - slack) & (g <= hi + lit['t'] + slack)).all(), (route, K, bins)
        assert (hi - lo).max() > 1e-4


@pytest.mark.gpu
def test_autograd_plumbing_on_the_device(monkeypatch):
    from rmnet_amd import losses, ops
    rng = np.random.default_rng(15)
    probs, labels = vr.softmax_clip(rng, 2, 3, 9, 13, peak=3.0, ignore=0.1)
    lv = t(labels).cuda()
    calls = {'grad': 0, 'value': 0}
    real_grad, real_value = ops.clip_loss_grad, ops.clip_loss
    monkeypatch.setattr(ops, 'clip_loss_grad', lambda *a, **k: (calls.__setitem__('grad', calls['grad'] + 1), real_grad(*a, **k))[1])
    monkeypatch.setattr(ops, 'clip_loss', lambda *a, **k: (calls.__setitem__('value', calls['value'] + 1), real_value(*a, **k))[1])
    x = t(probs).cuda().requires_grad_(True)
    loss = losses.training_loss(x, lv, bins=1 << 10, route='hip')
    assert calls == {'grad': 1, 'value': 0} and loss.requires_grad          # one call builds the histogram once, for value and gradient
    loss.backward()
    base = x.grad.clone()
    assert calls == {'grad': 1, 'value': 0}
    want = ref.table_grad(probs, labels, 255, 1 << 10)['grad']
    assert bits(base.cpu().numpy()).tobytes() == bits(want).tobytes()         # grad_output == 1 leaves the kernel's bits
    # grad_output != 1 scales the gradient
    x.grad = None
    (losses.training_loss(x, lv, bins=1 << 10, route='hip') * 0.25).backward()
    assert torch.equal(x.grad, base * 0.25)
    # a non-leaf: the soft-max of a leaf gets its gradient through torch's soft-max backward
    z = torch.randn(2, 3, 9, 13, device='cuda', dtype=torch.float64).mul_(2).float().requires_grad_(True)
    p = torch.softmax(z, dim=1)
    p.retain_grad()
    losses.training_loss(p, lv, bins=1 << 10, route='hip').backward()
    assert z.grad is not None and bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
    manual = p.detach() * (p.grad - (p.grad * p.detach()).sum(dim=1, keepdim=True))
    assert float((z.grad - manual).abs().max()) <= 1e-5 * float(p.grad.abs().max())
    # nothing asks for a gradient: the forward entry alone, and the same value
    calls.update(grad=0, value=0)
    with torch.no_grad():
        a = losses.training_loss(x, lv, bins=1 << 10, route='hip')
    b = losses.training_loss(x.detach(), lv, bins=1 << 10, route='hip')
    assert calls == {'grad': 0, 'value': 2} and not a.requires_grad and not b.requires_grad
    assert float(a) == float(b) == float(loss)
    # double backward raises
    y = t(probs).cuda().requires_grad_(True)
    g, = torch.autograd.grad(losses.training_loss(y, lv, bins=1 << 10, route='hip'), y, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
