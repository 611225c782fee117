# -*- coding: utf-8 -*-
"""Float64 restatements of the four HIP convolutions (csrc/conv_split.hip, conv3x3.hip, stem.hip, pred_head.hip) for the
per-element tests of tests/test_conv_edges.py.  Plain functions: no fixtures, nothing here is collected by pytest.

1. Why integer inputs come back bit for bit (``int_weights`` / ``int_acts``)
---------------------------------------------------------------------------
Activations are integers with |x| <= 15 (masks: 0 / 1), weights integers with |w| <= 8, the folded BatchNorm scale a power of
two, shift and residual integers.
  * The loader forms c = 64 x: an integer below 2^10, an fp16 number.  hi = c, lo = 0.
  * The packer scales w * bn_scale by the power of two that puts the channel's largest magnitude in [2^14, 2^15): an integer of at
    most 4 significant bits times a power of two, an fp16 number.  hi = w * bn_scale * 2^e, lo = 0 (``test_the_integer_packs_...``
    asserts this on the CPU).  Channels whose largest weight is 3, 5 and 8 take three different e, the all-zero channel e = 0.
  * So both cross-term MFMAs add zeros, and the hi * hi accumulator holds 64 * 2^e * bn_scale times a partial sum of integers
    x * w.  Every partial sum is below K * 15 * 8 <= 9216 * 120 < 2^24 in that common unit, so every fp32 addition is exact in
    whatever order the MFMAs and the K loop perform them.
  * The epilogue multiplies by unscale / 64 = 2^-e / 64 (exact), adds the integer shift and the integer residual.  With
    bn_scale in {1/4 .. 4} all values are multiples of min(1, bn_scale) and below 2^24 of that unit: exact again.
  * ReLU and the stem's 3x3 / stride-2 max-pool select values, they do not round.
Hence the kernel must equal the float64 F.conv2d expression cast to fp32, and the tests use torch.equal.  pred_head is plain
fp32 FMA over integers below 2^24: exact for the same reason.

1b. Non-zero lo planes, still bit for bit (``lo_weights`` / ``lo_acts`` / ``predict``)
----------------------------------------------------------------------------------
The integer cases leave the lo planes zero, and the bound of section 2 is wider than a lo-plane fault in one tap of a 3x3
convolution.  So a second exact family gives every tap live cross terms:
  * activations x = a + b 2^-14 with 1 <= |a| <= 15, |b| <= 3.  c = 64 a + b / 256, and |b| / 256 < 2^-6 is below half an fp16 step
    on either side of 64 a (the finest step next to 64 is 2^-5), so h = 64 a and l = b / 256, both exact;
  * weights w = p + q 2^-13 with integer |p| <= 8, q in {-1, 0, 1}, q = 0 where p = 0, and one exact 8 in every output channel, so
    every channel's scale is 2^11: ws = p 2^11 + q / 4, and 1/4 is below half an fp16 step next to any p 2^11 (the finest is 1 below
    2^11), so Wh = p 2^11 and Wl = q / 4, both exact.
Then the hi * hi accumulator holds 2^17 times a sum of integers a p (below K * 120 < 2^24: exact), the cross accumulator a sum of
the integers 16 a q and 8 b p (below K * 432 < 2^24 for K <= 2304: exact), both in any order.  What remains is the epilogue's own
roundings, which are fixed by the source: fp32(acc + accx), times unscale / 64 (exact), fp32(. + shift), fp32(. + res).
``predict`` performs exactly these, each sum formed without error in float64 and rounded to fp32 once, so the kernel must return
it bit for bit -- and a kernel that loses Wl or l anywhere in one tap does not (``test_the_lo_exact_prediction_...``).

2. The three-term arithmetic and its per-element bound (``restate`` / ``kernel_bound`` / ``repr_bound``)
-------------------------------------------------------------------------------------------------------
The kernels compute, for every output element,
    c = clamp(64 * relu?(x), +-65504),  h = fp16(c),  l = fp16(c - h)                      (``split_act``)
    Wh, Wl, unscale read from the pack                                                        (``unpack_conv`` / ``unpack_stem``)
    T = (sum h*Wh + sum (h*Wl + l*Wh)) * unscale / 64 + shift + res                           (``restate``)
where T is what exact arithmetic gives.  What the kernel adds to T:
  * every product of two fp16 numbers has 22 significant bits and is exact in fp32;
  * the hi * hi accumulator sums K such products in fp32, the cross accumulator 2 K.  Summing n numbers in fp32 in ANY order
    (the order inside one MFMA included) errs by at most (n - 1) u sum|terms| to first order, u = 2^-24.  Written with one
    factor for all three sums, (K - 1) u Ahh + (2 K - 1) u Ax <= (K + 1) u (Ahh + Ax) as long as (K - 2) Ax <= 2 Ahh; since
    |l| <= 2^-11 |h| and |Wl| <= 2^-11 |Wh| give Ax <= 2^-10 Ahh this holds for K <= 2050 (the tests use K <= 576);
  * acc + accx: one rounding, at most u (Ahh + Ax) (1 + K u); the product with unscale / 64 is exact (a power of two); the
    remaining 2 of the K + 4 cover the second-order terms (K u)^2 for K <= 2050;
  * + shift and + res: one rounding each, of a partial result no larger than |T| + |shift| + |res| (+ the error so far): at most
    2 u (|shift| + |res| + |T|) in all, written 2^-23.
So    |got - T| <= (K + 4) 2^-24 (sum|h Wh| + sum|h Wl| + sum|l Wh|) unscale / 64 + 2^-23 (|shift| + |res| + |T|)
for every element, with nothing tuned.  ReLU at the output is 1-Lipschitz and keeps the bound; a max-pool keeps it as the maximum
of the bounds over its window (the maximum of values that are within their bounds is within the maximum of the bounds).

How sharp it is: a dropped cross term is worth about sqrt(K) 2^-12.5 of a typical product, the bound (K + 4) K 2^-24 of it.  At
K = 32 the missing term is ~10x the bound, at K = 64 ~4x, from K = 288 on it is inside the bound -- which is why the power test
(``test_the_bound_catches_...``) and the sharpest GPU cases use 1x1 kernels with Cin 32 / 64.

Against the true float64 convolution of x with w * bn_scale the representation error is added (``repr_bound``):
  * h + l differs from c by at most 2^-22 |c| (fp16 rounding of l), or by 2^-25 where l is an fp16 subnormal: 2^-31 in x's unit;
  * Wh + Wl differs from the scaled weight by at most 2^-22 of it;
  * the dropped l * Wl term is at most 2^-22 |x w|;
giving 3 * 2^-22 sum|x||w scale| + 2^-31 sum|w scale| over the taps inside the map.

pred_head: C fused multiply-adds per tap, then bias + 9 partials in fp32: at most (C + 9) u (sum|relu(x)||w| + |b|) to first
order; the tests require (K + 2) u of it with K = 9 C, as the plain summation bound for K products and a bias.
"""

import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_SCALE = 64.0
F16_MAX = 65504.0


# ------------------------------------------------------------------------------------------------------- pack layouts
def unpack_conv(wp, cout, cin, k):
    """(Wh, Wl) [Cout, Cin, k, k] float64, still scaled, from the [tap][Cin / 32][hi, lo][co][Cin % 32] layout of conv_split_pack /
    conv3x3_pack (include/rmnet_hip.h)."""
    p = wp.view(torch.float16).double().view(k * k, cin // 32, 2, cout, 32)                 # [tap][cb][plane][co][kk]
    return tuple(p[:, :, i].permute(2, 1, 3, 0).reshape(cout, cin, k, k) for i in (0, 1))


def unpack_conv_weights(wp, wu, cout, cin, k):
    """The pack back to [Cout, Cin, k, k] float64: (hi + lo) * unscale."""
    wh, wl = unpack_conv(wp, cout, cin, k)
    return (wh + wl) * wu.double().view(-1, 1, 1, 1)


def unpack_stem(wp, cin):
    """(Wh, Wl) [64, Cin, 7, 7] float64, still scaled, and the K padding's planes [64, 2, Kp - 49 Cin], from the
    [k / 32][hi, lo][co][k % 32] layout of stem_pack, k = (7 ky + kx) Cin + ci."""
    kp = (49 * cin + 31) // 32 * 32
    p = wp.view(torch.float16).double().view(kp // 32, 2, 64, 32)
    flat = p.permute(2, 1, 0, 3).reshape(64, 2, kp)                                           # [co][plane][k]
    planes = tuple(flat[:, i, :49 * cin].reshape(64, 7, 7, cin).permute(0, 3, 1, 2) for i in (0, 1))
    return planes[0], planes[1], flat[:, :, 49 * cin:]


def unpack_stem_weights(wp, wu, cin):
    wh, wl, pad = unpack_stem(wp, cin)
    return (wh + wl) * wu.double().view(-1, 1, 1, 1), pad


# ------------------------------------------------------------------------------------------------------- integer inputs
def int_weights(cout, cin, k, seed):
    """Integer weights |w| <= 8 [Cout, Cin, k, k] fp32: channel 0 holds an 8, channel 1 is all zero, channels 2 and 3 have the
    maxima 3 and 5 (different packer scales)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-8, 9, (cout, cin, k, k), generator=g).float()
    w[0, 0, 0, 0] = 8.0
    w[1] = 0.0
    w[2] = w[2].clamp(-3, 3)
    w[2, 1, k - 1, 0] = 3.0
    w[3] = w[3].clamp(-5, 5)
    w[3, cin - 1, 0, k - 1] = -5.0
    return w


def int_acts(shape, seed, lo=-15, hi=15):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def pow2_scale(cout):
    """bn_scale in {1/4, 1/2, 1, 2, 4}, cycling over the channels."""
    return torch.ldexp(torch.ones(cout), (torch.arange(cout) % 5 - 2).float())


def lo_weights(cout, cin, k, seed):
    """w = p + q 2^-13 (section 1b) [Cout, Cin, k, k] fp32: an exact 8 in every output channel, q = 0 where p = 0."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(-8, 9, (cout, cin, k, k), generator=g).float()
    q = torch.randint(-1, 2, (cout, cin, k, k), generator=g).float()
    q[p == 0] = 0.0
    p[:, 0, 0, 0] = 8.0
    q[:, 0, 0, 0] = 0.0
    return p + q * 2.0 ** -13


def lo_acts(shape, seed):
    """x = a + b 2^-14 with 1 <= |a| <= 15, |b| <= 3 (section 1b)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(1, 16, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    b = torch.randint(-3, 4, shape, generator=g).float()
    return a + b * 2.0 ** -14


def tile_of(n, cout, h, w, k, s):
    """The tile rmnet_conv_split_f32 picks (csrc/conv_split.hip, the end of the entry): restated so that the tests can say, and check,
    which kernel instance a case runs."""
    ho, wo = out_hw(h, w, k, s)
    m = n * ho * wo
    if cout % 256 == 0 and (m + 127) // 128 * (cout // 256) >= 512:
        return 'Big'
    return 'Mid' if cout % 128 == 0 else 'Narrow'


def out_hw(h, w, k, s):
    p = k // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------------- the restatement
def split_act(x, relu=False):
    """(h, l) of the loaders, float64 in the 2^6-scaled unit."""
    x = x.double()
    if relu:
        x = F.relu(x)
    c = (x * ACT_SCALE).clamp(-F16_MAX, F16_MAX)
    h = c.half().double()
    l = (c - h).half().double()
    return h, l


def restate(h, l, wh, wl, wu, stride, pad, shift=None, res=None, hwl=None, lwh=None):
    """(T, A): T as in the module docstring, A = (sum|h Wh| + sum|h Wl| + sum|l Wh|) unscale / 64.  ``hwl`` / ``lwh`` replace the operands of the two cross terms (the power test's faults): pairs (h', Wl') and
    (l', Wh'), or False to drop the term."""
    us = (wu.double() / ACT_SCALE).view(1, -1, 1, 1)
    conv = lambda a, b: F.conv2d(a, b, None, stride, pad)
    s = conv(h, wh)
    if hwl is not False:
        a, b = (h, wl) if hwl is None else hwl
        s = s + conv(a, b)
    if lwh is not False:
        a, b = (l, wh) if lwh is None else lwh
        s = s + conv(a, b)
    t = s * us
    if shift is not None:
        t = t + shift.double().view(1, -1, 1, 1)
    if res is not None:
        t = t + res.double()
    a = (conv(h.abs(), wh.abs() + wl.abs()) + conv(l.abs(), wh.abs())) * us
    return t, a


def predict(h, l, wh, wl, wu, stride, pad, shift=None, res=None, relu_out=False):
    """The kernels' result where both accumulators are exact (section 1b): the epilogue's roundings, one at a time."""
    conv = lambda a, b: F.conv2d(a, b, None, stride, pad)
    r32 = lambda t: t.float().double()
    v = r32(conv(h, wh) + (conv(h, wl) + conv(l, wh))) * (wu.double() / ACT_SCALE).view(1, -1, 1, 1)
    if shift is not None:
        v = r32(v + shift.double().view(1, -1, 1, 1))
    if res is not None:
        v = r32(v + res.double())
    return F.relu(v) if relu_out else v


def kernel_bound(kred, a, t, shift=None, res=None):
    """(K + 4) 2^-24 A + 2^-23 (|shift| + |res| + |T|), per element."""
    tail = t.abs()
    if shift is not None:
        tail = tail + shift.double().abs().view(1, -1, 1, 1)
    if res is not None:
        tail = tail + res.double().abs()
    return (kred + 4) * U * a + 2.0 ** -23 * tail


def repr_bound(x, w, stride, pad, relu=False):
    """3 * 2^-22 sum|x||w| + 2^-31 sum|w| over the taps inside the map; ``w`` is w * bn_scale in float64."""
    x = x.double()
    if relu:
        x = F.relu(x)
    wa = w.double().abs()
    return 3 * 2.0 ** -22 * F.conv2d(x.abs(), wa, None, stride, pad) + 2.0 ** -31 * F.conv2d(torch.ones_like(x), wa, None, stride, pad)


def pool(t):
    return F.max_pool2d(t, 3, 2, 1)


# ------------------------------------------------------------------------------------------------------- part 2 inputs
def uniform_weights(cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    std = 0.9 * (2.0 / (k * k * cin)) ** 0.5
    return ((torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * (std * 3 ** 0.5)).float()


INPUTS = ('1e-3', '1', '1e2', 'mixed')


def large_channels(cin):
    """The input channels the mixed case calls large: scale 2^(-10 + c mod 14) with c mod 14 in the upper half of what occurs."""
    c = torch.arange(cin) % 14
    return c >= min(7, cin // 2)


def make_inputs(kind, shape, w, seed):
    """(x, w) for one of INPUTS: Gaussian x at a scale, or the mixed case -- input channel c times 2^(-10 + c mod 14), and the
    weights of the odd output channels zero on the large input channels, so that those outputs see only small activations (lo halves
    in fp16's subnormals)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind != 'mixed':
        return x * float(kind), w
    cin = shape[1]
    x = x * torch.ldexp(torch.ones(cin), (torch.arange(cin) % 14 - 10).float()).view(1, -1, 1, 1)
    w = w.clone()
    big = large_channels(cin).nonzero().flatten()
    odd = torch.arange(1, w.shape[0], 2)
    w[odd.view(-1, 1), big.view(1, -1)] = 0.0
    return x, w
