# -*- coding: utf-8 -*-
"""Plain numpy restatements of the kernels of rmnet_amd/csrc/region_map.hip and rmnet_amd/csrc/flow_affine.hip, the launch plan
of the region reduction, the shared case builders of tests/test_region_edges.py and the planted faults.  Nothing here is collected
by pytest and nothing here imports torch.

  region_map(mask, thr, n_pts, loose)      reg_att_map_generator.cu:15-93: sentinels (32767, 0, 32767, 0), ``>=`` in fp32, the
                                           point-count fallback, the four clamp expressions; channel 0 is zeros
  cell_rect / cell_rects                   the rule of include/rmnet_hip.h: the cells that survive F.interpolate(padded box map,
                                           scale_factor=1/stride); (1,0,1,0) for an empty rectangle and, with k_per_batch, channel 0
  rect_mask(x, rects)                      x * m in fp32 with m the 0/1 rectangle map (numpy gives NaN and -0.0 as the multiply does)
  flow_affine(flow, m1, m2)                flow_affine_transformation.cpp:63-83 in np.float32, one rounding per operation, left to
                                           right, y1 from the updated x1; std::round as copysign(floor(|x| + 0.5), x) in float64,
                                           which is exact for every fp32 x and is not the kernel's trunc form
  plan(B, K, H, W)                         (chunks, rows_per_chunk, vec): chunks_for of region_map.hip restated

Every restatement takes ``fault=``: one of MUTANTS, a deliberately wrong variant that some named case of the tests must expose.

Faults that are NOT planted, because no output can show them:
  * padding lanes counting when thr <= 0 (the reduction loads 0.0 for lanes past the row end): such a lane would add to n and to
    x_max only.  With thr <= 0 every real pixel of a finite non-negative mask counts as well, so the box is the full frame with
    or without the padding hits, clamped or fallen back.  (The kernel guards the lanes with ``x < W`` all the same.)
  * ``x0 < loose`` for ``x0 <= loose`` (and the same for y0): at x0 == loose both forms give 0 (x0 - loose), and they agree
    everywhere else, so the two expressions are the same function of the integers; test_region_edges.py proves that by
    enumeration (EQUIVALENT_MUTANTS) instead of pretending a case could tell them apart."""

import hashlib

import numpy as np

F32 = np.float32
SENTINEL = (32767, 0, 32767, 0)
EMPTY_RECT = (1, 0, 1, 0)

REGION_MUTANTS = ['gt_for_ge', 'float4_last_lane_ignored', 'second_base_pass_ignored', 'band_last_row_skipped', 'band_rows_past_4_skipped',
                  'trailing_band_folded_twice', 'n_le_npts', 'x1_gt_for_ge', 'y1_gt_for_ge', 'att_channel0_unwritten']
CELL_MUTANTS = ['cx0_floor', 'no_clamp_to_cw', 'empty_not_normalised']
RECT_MUTANTS = ['plus_zero_outside', 't_o_swapped']
FLOW_MUTANTS = ['round_trunc_fp32', 'round_half_even', 'y1_from_old_x1', 'one_fma', 'clamp_gt_for_ge', 'rows_from_4096_unwritten']
MUTANTS = REGION_MUTANTS + CELL_MUTANTS + RECT_MUTANTS + FLOW_MUTANTS
EQUIVALENT_MUTANTS = ['x0_lt_for_le', 'y0_lt_for_le']        # see the docstring: identical functions, proven by enumeration


# ================================================================================================ launch plan
def plan(B, K, H, W):
    """(chunks, rows_per_chunk, vec) of launch_region_map for buffers the caller aligned to 16 bytes."""
    planes = B * (K - 1 if K > 1 else 1)
    chunks = (1024 + planes - 1) // planes
    chunks = min(chunks, 256)
    chunks = min(chunks, (H + 3) // 4)
    chunks = max(chunks, 1)
    rows = (H + chunks - 1) // chunks
    return chunks, rows, W % 4 == 0


def workspace_bytes(B, K, H, W):
    return B * K * plan(B, K, H, W)[0] * 32


# ================================================================================================ region map
def loosen(n, box, H, W, n_pts, loose, fault=None):
    """.cu:55-77 on one channel's count and tight box."""
    x0, x1, y0, y1 = (int(v) for v in box)
    below = n <= n_pts if fault == 'n_le_npts' else n < n_pts
    if below:
        return (0, W - 1, 0, H - 1)
    lo = lambda v, f: 0 if (v < loose if fault == f else v <= loose) else v - loose
    hi = lambda v, n_, f: n_ - 1 if (v + loose > n_ if fault == f else v + loose >= n_) else v + loose
    return (lo(x0, 'x0_lt_for_le'), hi(x1, W, 'x1_gt_for_ge'), lo(y0, 'y0_lt_for_le'), hi(y1, H, 'y1_gt_for_ge'))


def region_map(mask, thr, n_pts, loose, fault=None, prefill=np.nan):
    """mask [B,K,H,W] f32 -> (att [B,K,H,W] f32, bboxes [B,K,4] int32).  ``prefill``: what an element nobody writes holds."""
    mask = np.asarray(mask, F32)
    B, K, H, W = mask.shape
    thr = F32(thr)
    chunks, rows, vec = plan(B, K, H, W)
    with np.errstate(invalid='ignore'):
        hit = (mask > thr) if fault == 'gt_for_ge' else (mask >= thr)
    hit = hit.copy()
    hit[:, 0] = False                                   # channel 0 is never inspected (.cu:31, 37)
    xs, ys = np.arange(W), np.arange(H)
    r0 = (ys // rows) * rows
    r1 = np.minimum(H, r0 + rows)
    if fault == 'float4_last_lane_ignored' and vec:
        hit[..., xs % 4 == 3] = False
    if fault == 'second_base_pass_ignored':
        hit[..., xs >= (1024 if vec else 512)] = False
    if fault == 'band_last_row_skipped':
        hit[:, :, ys == r1 - 1, :] = False
    if fault == 'band_rows_past_4_skipped':
        hit[:, :, ys - r0 >= 4, :] = False
    n = hit.sum(axis=(2, 3)).astype(np.int64)
    if fault == 'trailing_band_folded_twice':
        n = n + hit[:, :, ys // rows == chunks - 1, :].sum(axis=(2, 3))
    anyx, anyy = hit.any(axis=2), hit.any(axis=3)        # [B,K,W], [B,K,H]
    bboxes = np.zeros((B, K, 4), np.int32)
    att = np.zeros((B, K, H, W), F32)
    if fault == 'att_channel0_unwritten':
        att[:, 0] = prefill
    for b in range(B):
        for k in range(1, K):
            box = SENTINEL
            if anyx[b, k].any():
                cx, cy = np.flatnonzero(anyx[b, k]), np.flatnonzero(anyy[b, k])
                box = (cx[0], cx[-1], cy[0], cy[-1])
            x0, x1, y0, y1 = loosen(int(n[b, k]), box, H, W, n_pts, loose, fault)
            bboxes[b, k] = (x0, x1, y0, y1)
            inx = (xs >= x0) & (xs <= x1)
            iny = (ys >= y0) & (ys <= y1)
            att[b, k] = (iny[:, None] & inx[None, :]).astype(F32)      # .cu:81-92, inclusive
    return att, bboxes


# ================================================================================================ cell rectangles
def cell_rect(box, pad_l, pad_t, stride, ch, cw, fault=None):
    """(x0, x1, y0, y1) in pixels of the un-padded frame -> (cx0, cx1, cy0, cy1) inclusive on the ch x cw grid: cell (cy, cx)
    survives when pixel (stride * cy, stride * cx) of the map padded by (pad_l, pad_t) lies in the box."""
    x0, x1, y0, y1 = (int(v) for v in box)
    ax0, ax1, ay0, ay1 = x0 + pad_l, x1 + pad_l, y0 + pad_t, y1 + pad_t
    up = (lambda a: max(a, 0) // stride) if fault == 'cx0_floor' else (lambda a: 0 if a <= 0 else -(-a // stride))
    cx0, cy0 = up(ax0), up(ay0)
    cx1 = ax1 // stride if ax1 >= 0 else -1
    cy1 = ay1 // stride if ay1 >= 0 else -1
    if fault != 'no_clamp_to_cw':
        cx1, cy1 = min(cx1, cw - 1), min(cy1, ch - 1)
    if (cx1 < cx0 or cy1 < cy0) and fault != 'empty_not_normalised':
        return EMPTY_RECT
    return (cx0, cx1, cy0, cy1)


def cell_rects(boxes, k_per_batch, pad_l, pad_t, stride, ch, cw, fault=None):
    """boxes [..., 4] -> rects, same shape, with rmnet_boxes_to_cell_rects_i32's rule: k_per_batch > 0 makes every box whose flat
    index is a multiple of it (channel 0) the empty rectangle, whatever it holds."""
    boxes = np.asarray(boxes, np.int32)
    flat = boxes.reshape(-1, 4)
    out = np.empty_like(flat)
    for i, bx in enumerate(flat):
        out[i] = EMPTY_RECT if (k_per_batch > 0 and i % k_per_batch == 0) else cell_rect(bx, pad_l, pad_t, stride, ch, cw, fault)
    return out.reshape(boxes.shape)


def cell_grid_of(H, W, stride=16):
    """(pad_l, pad_t, stride, ch, cw) of pad_divide_by(16): the frame centred in the next multiple of 16."""
    dh, dw = (stride - H % stride) % stride, (stride - W % stride) % stride
    return (dw // 2, dh // 2, stride, (H + dh) // stride, (W + dw) // stride)


CELL_ENUM_W = [1, 5, 16, 17, 31, 33, 47, 48]


def cell_enum_pads(W):
    return sorted({0, 1, 7, 8, 15, ((16 - W % 16) % 16) // 2})


def cell_enum_boxes(W):
    """Every 0 <= x0 <= x1 < W."""
    return [(a, b) for a in range(W) for b in range(a, W)]


# ================================================================================================ rectangle mask
def rect_mask(x, rects, fault=None):
    """x [n,C,T,h,w] f32, rects [n,T,4] int32 (cx0, cx1, cy0, cy1) inclusive -> x * m, m = 1 inside the rectangle."""
    x = np.asarray(x, F32)
    n, C, T, h, w = x.shape
    r = np.asarray(rects, np.int64).reshape(n, T, 4)
    if fault == 't_o_swapped':
        flat = r.reshape(-1, 4)
        r = np.stack([np.stack([flat[(t * n + o) % (n * T)] for t in range(T)]) for o in range(n)])
    cx, cy = np.arange(w)[None, None, None, :], np.arange(h)[None, None, :, None]
    g = lambda i: r[:, :, i][:, :, None, None]
    m = (cx >= g(0)) & (cx <= g(1)) & (cy >= g(2)) & (cy <= g(3))          # [n,T,h,w]
    m = m[:, None]
    if fault == 'plus_zero_outside':
        return np.where(m, x, F32(0.0)).astype(F32)
    with np.errstate(invalid='ignore'):
        return x * m.astype(F32)


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def rect_kinds(h, w):
    """The rectangle kinds of the rect_mask cases, name -> (cx0, cx1, cy0, cy1)."""
    return {'whole grid': (0, w - 1, 0, h - 1), 'empty (1,0,1,0)': EMPTY_RECT, 'first cell': (0, 0, 0, 0),
            'last cell': (w - 1, w - 1, h - 1, h - 1), 'sticking out': (-3, w + 2, -3, h + 2),
            'inverted in x only': (w - 1, 0, 0, h - 1), 'inverted in y only': (0, w - 1, h - 1, 0),
            'INT32_MIN .. INT32_MAX': (INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX),
            'INT32_MAX .. INT32_MIN': (INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN),
            'interior': (w // 3, w - 1 - w // 4, h // 4, h - 1 - h // 3)}


RECT_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 17, 19), (1, 2, 3, 30, 54)]
RECT_SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, -3e38, 1e-45, -1e-45, -1e-40, 2.5], F32)


def rect_case(shape, rot=0):
    """(x, rects, kind names [n][T]): every (n, t) pair gets a different kind (rotated by ``rot``), and the specials are planted
    on a stride that is coprime to the plane size, so that they fall inside and outside the rectangles."""
    n, C, T, h, w = shape
    rng = np.random.default_rng(1000 + h * w + rot)
    x = rng.standard_normal(shape, dtype=F32)
    flat = x.reshape(-1)
    step = 7 if (h * w) % 7 else 11
    idx = (np.arange(flat.size // step + 1) * step)[: max(flat.size // step, 1)]
    idx = idx[idx < flat.size]
    flat[idx] = RECT_SPECIALS[np.arange(idx.size) % RECT_SPECIALS.size]
    kinds = rect_kinds(h, w)
    names = list(kinds)
    pick = [[names[(o * T + t + rot) % len(names)] for t in range(T)] for o in range(n)]
    rects = np.array([[kinds[k] for k in row] for row in pick], np.int64).astype(np.int32)
    return x, rects, pick


# ================================================================================================ flow affine
def _round_half_away(x):
    x64 = x.astype(np.float64)
    return np.copysign(np.floor(np.abs(x64) + 0.5), x64).astype(F32)


def _round(x, fault):
    if fault == 'round_trunc_fp32':                     # trunc(x + copysign(0.5, x)) with the add rounded to fp32
        return np.trunc(x + np.copysign(F32(0.5), x)).astype(F32)
    if fault == 'round_half_even':
        return np.rint(x).astype(F32)
    return _round_half_away(x)


def flow_affine(flow, m1, m2, fault=None, prefill=np.nan):
    """flow [H,W,2] f32, m1 / m2 [2,3] f32 -> [H,W,2] f32."""
    flow = np.asarray(flow, F32)
    a, b = np.asarray(m1, F32).reshape(6), np.asarray(m2, F32).reshape(6)
    H, W = flow.shape[:2]
    j = np.arange(W, dtype=F32)[None, :] + np.zeros((H, 1), F32)
    i = np.arange(H, dtype=F32)[:, None] + np.zeros((1, W), F32)
    with np.errstate(invalid='ignore', over='ignore'):
        x2 = _round(b[0] * j + b[1] * i + b[2], fault)
        y2 = _round(b[3] * j + b[4] * i + b[5], fault)
        x1 = j + flow[..., 0]
        y1 = i + flow[..., 1]

        def line(c0, c1, c2, u, v):
            if fault == 'one_fma':                      # fma(c1, v, fl(c0 * u)): the product c1 * v is not rounded on its own
                p = (c0 * u).astype(np.float64)
                s = (p + np.float64(c1) * v.astype(np.float64)).astype(F32)
                return s + c2
            return c0 * u + c1 * v + c2

        x1n = _round(line(a[0], a[1], a[2], x1, y1), fault)
        y1n = _round(line(a[3], a[4], a[5], x1 if fault == 'y1_from_old_x1' else x1n, y1), fault)

        def clamp(v, n):
            over = (v > F32(n)) if fault == 'clamp_gt_for_ge' else (v >= F32(n))
            return np.where(v < 0, F32(0.0), np.where(over, F32(n - 1), v)).astype(F32)

        out = np.stack([clamp(x1n, W) - clamp(x2, W), clamp(y1n, H) - clamp(y2, H)], axis=-1).astype(F32)
    if fault == 'rows_from_4096_unwritten':
        out[4096:] = prefill
    return out


def _halves_grid(H, W):
    """Flows on multiples of 0.5 of both signs, every residue against the pixel index."""
    y, x = np.mgrid[0:H, 0:W]
    fx = (((x * 3 + y * 5) % 25) - 12) * 0.5
    fy = (((x * 7 + y * 2) % 21) - 10) * 0.5
    return np.stack([fx, fy], axis=-1).astype(F32)


IDENTITY = np.array([[1, 0, 0], [0, 1, 0]], F32)
BELOW_HALF = np.nextafter(F32(0.5), F32(0.0))            # 0.49999997: trunc(x + 0.5) in fp32 rounds it to 1


def _near_halves(axis):
    """Row r of [3, 16] (axis 0: in x, pixel column j; axis 1: transposed, in y): j + flow is exactly j + 0.5 (r = 0), its fp32
    neighbour towards zero (r = 1: 0.49999997, 1.4999999, 2.4999998, 3.4999998, ...) and the one away from it (r = 2)."""
    H, W = 3, 16
    flow = np.zeros((H, W, 2), F32)
    for jx in range(13):
        half = F32(jx + 0.5)
        for r, t in enumerate((half, np.nextafter(half, F32(0.0)), np.nextafter(half, F32(np.inf)))):
            f = F32(t - F32(jx))
            assert F32(jx) + f == t                      # (the sum the kernel forms is exactly the target)
            flow[r, jx, 0] = f
    flow[..., 1] = 0.25
    if axis == 1:
        flow = np.ascontiguousarray(flow.transpose(1, 0, 2)[..., ::-1])
    return flow


def _edge_targets(H, W):
    """Identity matrices and integer flows: x1 lands exactly on -1, 0, W-1, W (y1 on -1, 0, H-1, H), every pairing."""
    tx, ty = [-1, 0, W - 1, W, -0.0, 1], [-1, 0, H - 1, H, -0.0, 2]
    y, x = np.mgrid[0:H, 0:W]
    fx = np.array(tx, F32)[(x + y) % 6] - x.astype(F32)
    fy = np.array(ty, F32)[(x * 2 + y) % 6] - y.astype(F32)
    return np.stack([fx, fy], axis=-1).astype(F32)


def _random_flow_case(H, W, seed):
    rng = np.random.RandomState(seed)
    flow = ((rng.rand(H, W, 2) - 0.5) * 40).astype(F32)
    flow[::3, ::2] = np.round(flow[::3, ::2] * 2) / 2     # a share of exact halves
    m1 = (np.eye(2, 3) + (rng.rand(2, 3) - 0.5) * 0.2).astype(F32)
    m2 = (np.eye(2, 3) + (rng.rand(2, 3) - 0.5) * 0.2).astype(F32)
    return flow, m1, m2


FLOW_TALL = ('tall 4099 x 3', 4099, 3, 4099)             # name, H, W, seed: stored as a seed and a digest, not as arrays


def flow_cases():
    """name -> (flow, m1, m2): the cases of tests/golden/flow_affine_edges.npz and of the GPU tests, in one place."""
    c = {}
    c['halves, identity 9 x 11'] = (_halves_grid(9, 11), IDENTITY, IDENTITY)
    y, x = np.mgrid[0:5, 0:7]
    sign = np.where((x + y) % 2 == 0, 1.0, -1.0).astype(F32)
    c['every flow +-0.49999997'] = (np.stack([sign * BELOW_HALF, -sign * BELOW_HALF], axis=-1).astype(F32), IDENTITY, IDENTITY)
    c['fp32 neighbours of the halves in x (3.4999998)'] = (_near_halves(0), IDENTITY, IDENTITY)
    c['fp32 neighbours of the halves in y'] = (_near_halves(1), IDENTITY, IDENTITY)
    d1 = np.array([[0.5, -0.25, 0.25], [0.25, 0.5, -0.5]], F32)
    d2 = np.array([[-0.5, 0.5, 0.5], [0.25, -0.25, 0.25]], F32)
    c['dyadic matrices on the halves grid 9 x 11'] = (_halves_grid(9, 11), d1, d2)
    c['dyadic matrices, swapped'] = (_halves_grid(9, 11), d2 + F32(2.0) * IDENTITY, d1)
    t1 = np.array([[1.0 / 3.0, 0.7, 0.1], [-0.3, 1.1, 0.9]], F32)
    t2 = np.array([[0.9, 0.1, -0.2], [0.2, 1.0 / 3.0, 0.3]], F32)
    c['inexact products (thirds and tenths) 9 x 11'] = (_halves_grid(9, 11) * F32(1.1), t1, t2)
    c['results on -1, 0, W-1, W 6 x 8'] = (_edge_targets(6, 8), IDENTITY, IDENTITY)
    c['shape 1 x 1'] = _random_flow_case(1, 1, 11)
    c['shape 2 x 257'] = _random_flow_case(2, 257, 2257)
    bad = _halves_grid(5, 6)
    bad.reshape(-1)[[0, 5, 9, 14, 22, 31, 40, 47, 58]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    c['NaN and +-Inf flows 5 x 6'] = (bad, d1 + IDENTITY, IDENTITY)
    return c


def flow_tall_case():
    _, H, W, seed = FLOW_TALL
    return _random_flow_case(H, W, seed)


def digest(a):
    """sha256 of an array's bytes with every NaN made the one quiet NaN."""
    a = np.ascontiguousarray(a, F32).copy()
    a[np.isnan(a)] = np.nan
    return hashlib.sha256(a.view(np.uint32).tobytes()).hexdigest()


def bits_equal(got, want):
    """(equal, index of the first difference, number of differences): the same 32 bits everywhere, a NaN matching any NaN."""
    g, w = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if g.shape != w.shape:
        return False, None, -1
    gi = np.where(np.isnan(g), np.uint32(0x7fc00000), g.view(np.uint32))
    wi = np.where(np.isnan(w), np.uint32(0x7fc00000), w.view(np.uint32))
    bad = np.flatnonzero(gi.reshape(-1) != wi.reshape(-1))
    if bad.size == 0:
        return True, None, 0
    return False, tuple(int(v) for v in np.unravel_index(int(bad[0]), w.shape)), int(bad.size)


# ================================================================================================ region cases (shared CPU / GPU)
# (B, K, H, W) with K - 1 live channels -> what the shape reaches, and the plan it must land on
REGION_SHAPES = {
    (1, 2, 1, 1): ('one pixel', (1, 1, False)),
    (1, 2, 1, 5): ('one row', (1, 1, False)),
    (1, 2, 5, 1): ('one column', (2, 3, False)),
    (1, 3, 9, 67): ('scalar path, second slot part filled', (3, 3, False)),
    (1, 2, 6, 515): ('scalar path, second base pass', (2, 3, False)),
    (2, 3, 13, 260): ('VEC4, w4 = 65; 4 bands of 4 rows, the last with one row', (4, 4, True)),
    (1, 2, 8, 1028): ('VEC4, second base pass with one float4', (2, 4, True)),
    (4, 16, 100, 8): ('60 planes: 18 bands of 6 rows, the last band empty', (18, 6, True)),
    (3, 400, 5, 8): ('more than 1024 planes: one band, wave 0 owns rows 0 and 4', (1, 5, True)),
    (1, 2, 32767, 1): ('256 bands of 128 rows; a hit at y = 32766 next to the sentinel', (256, 128, False)),
    (1, 2, 1, 32767): ('a hit at x = 32766 next to the sentinel, scalar', (1, 1, False)),
    (1, 2, 1, 32764): ('the widest VEC4 row', (1, 1, True)),
}
THR = F32(0.5)


def probe_xs(W):
    s = set(range(0, 6)) | set(range(62, 66)) | set(range(252, 260)) | set(range(511, 514)) | set(range(1020, 1028)) | set(range(W - 5, W))
    return sorted(v for v in s if 0 <= v < W)


def probe_ys(B, K, H, W):
    rows = plan(B, K, H, W)[1]
    s = set(range(0, 5)) | {rows - 1, rows, rows + 1, H - 2, H - 1}
    return sorted(v for v in s if 0 <= v < H)


def probes(B, K, H, W):
    """Every (x, y) of the two seam sets (their cross product; the three 32767-long shapes: it is one of the sets anyway)."""
    return [(x, y) for y in probe_ys(B, K, H, W) for x in probe_xs(W)]


def probe_masks(shape, pairs=False):
    """Yields (mask, points per plane) with one probe (or, ``pairs``, two probes in different bands and waves) per live plane,
    each pixel exactly THR on a background of the fp32 number just below it; a plane that is left over stays empty."""
    B, K, H, W = shape
    pts = probes(B, K, H, W)
    if pairs:                                           # (x_min, y_max) and (x_max, y_min) from two different partial records
        lo = [(x, y) for (x, y) in pts]
        pts = [((x, y), (x2, y2)) for (x, y), (x2, y2) in zip(lo, lo[::-1]) if x < x2 and y > y2]
    else:
        pts = [(p,) for p in pts]
    live = [(b, k) for b in range(B) for k in range(1, K)]
    below = np.nextafter(THR, F32(0.0))
    for at in range(0, len(pts), len(live)):
        mask = np.full(shape, below, F32)
        mask[:, 0] = 1.0                                # channel 0 above the threshold everywhere: it must not matter
        placed = {}
        for (b, k), group in zip(live, pts[at:at + len(live)]):
            for (x, y) in group:
                mask[b, k, y, x] = THR
            placed[(b, k)] = group
        yield mask, placed


def count_case(shape):
    """A checkerboard of hits two pixels or more inside the frame (the box loosened by COUNT_LOOSE = 1 is not the full frame) that spans several bands and both unroll slots -> (mask, n)."""
    B, K, H, W = shape
    rows = plan(*shape)[1]
    xs = [v for v in (2, 3, 5, 62, 63, 64, 65, 130, 254, 255, 256, 257, W - 4, W - 3) if 2 <= v <= W - 3]
    ys = [v for v in (2, 3, rows - 1, rows, rows + 1, 2 * rows, H - 4, H - 3) if 2 <= v <= H - 3]
    xs, ys = sorted(set(xs)), sorted(set(ys))
    rng = np.random.default_rng(B * 100 + W)
    mask = (rng.random(shape, dtype=F32) * F32(0.49)).astype(F32)
    n = 0
    for iy, y in enumerate(ys):
        for ix, x in enumerate(xs):
            if (ix + iy) % 2 == 0:
                mask[:, 1:, y, x] = THR if (ix % 3) else F32(0.75)
                n += 1
    return mask, n


COUNT_SHAPES = [(2, 3, 13, 260), (1, 3, 9, 67)]
COUNT_LOOSE = 1


def count_probe_masks(shape):
    """The count case with one extra hit per live plane at a probe position that is not a hit already."""
    B, K, H, W = shape
    base, n = count_case(shape)
    pts = [(x, y) for (x, y) in probes(*shape) if base[0, 1, y, x] < THR]
    live = [(b, k) for b in range(B) for k in range(1, K)]
    for at in range(0, len(pts), len(live)):
        mask = base.copy()
        for (b, k), (x, y) in zip(live, pts[at:at + len(live)]):
            mask[b, k, y, x] = THR
        if len(pts) - at < len(live):                  # the planes left over: the probe of the first plane once more
            for (b, k) in live[len(pts) - at:]:
                x, y = pts[at]
                mask[b, k, y, x] = THR
        yield mask, n


THRESHOLD_VALUES = {
    0.5: [0.5, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0)), np.nan, np.inf, -np.inf, 1e-45, -0.0],
    0.0: [0.0, -0.0, 1e-45, -1e-45, np.nan, np.inf, -np.inf, np.nextafter(F32(0.5), F32(0))],
    np.inf: [np.inf, 3.4028235e38, np.nan, -np.inf, 0.5, 0.0, -0.0, 1e-45],
}


def threshold_case(thr, W):
    """One channel per value: the value at pixel (1, c % W) of channel c + 1 on a background of -1, [1, 9, 3, W]; with
    n_pts = 1 and loose = 0 a channel whose value counts gives the one-pixel box and any other the full frame."""
    vals = np.array(THRESHOLD_VALUES[thr], F32)
    mask = np.full((1, 1 + len(vals), 3, W), -1.0, F32)
    for c, v in enumerate(vals):
        mask[0, c + 1, 1, (5 * c + 3) % W] = v
    return mask


def everything_counts_case(W):
    rng = np.random.default_rng(W)
    m = rng.random((2, 3, 7, W), dtype=F32)
    m[0, 1, 0, 0] = 0.0
    m[1, 2, 6, W - 1] = -0.0
    return m


SEAM_SHAPES = [(2, 3, 13, 260), (1, 3, 9, 67)]
SEAM_LOOSE = [0, 1, 3, 64]


def seam_masks(shape, loose):
    """Two corner pixels per live plane: the loosened box starts at x % 4 == r and ends at x % 4 == (r + 1) % 4 .. for r = 0 .. 3,
    on the first row of a band and on the last row of one.  Yields (mask, n_pts)."""
    B, K, H, W = shape
    rows = plan(*shape)[1]
    live = [(b, k) for b in range(B) for k in range(1, K)]
    for at in range(0, 4, len(live)):
        mask = np.zeros(shape, F32)
        for (b, k), r in zip(live, range(at, 4)):
            x0 = min(W - 1, 8 + r + loose)              # loosened: 8 + r (when it fits)
            x1 = max(x0, min(W - 1, 40 + 2 * r + (r + 1) % 4))
            y0 = min(H - 1, rows + loose)               # loosened: the first row of band 1 (when it fits)
            y1 = min(H - 1, max(y0, 2 * rows - 1 - loose))
            mask[b, k, y0, x0] = 0.5
            mask[b, k, y1, x1] = 1.0
        yield mask, 2


ALIGN_SHAPES = [(2, 3, 13, 260), (1, 2, 5, 8)]


def align_case(shape):
    rng = np.random.default_rng(shape[3])
    m = rng.random(shape, dtype=F32) * F32(0.49)
    B, K, H, W = shape
    m[:, 1:, H // 3:H // 2 + 2, 3:W - 2] = 0.9
    return m.astype(F32)


# ================================================================================================ warped cases
WARP_SHAPES = [(1, 2, 1, 7), (1, 2, 7, 1), (1, 3, 5, 257), (2, 2, 9, 300)]
WARP_BORDER_D = [2e-5, 5e-5, 1e-4, 2e-4, 1e-3]


def warp_flows(shape):
    """name -> flow [B,2,H,W] f32.  The border family lands the sample on -d, 0, W-1 and W-1+d (H-1 likewise in y): the
    validity sum of the bilinear footprint is 1 - d there, on both sides of 0.9999."""
    B, K, H, W = shape
    out = {'zero': np.zeros((B, 2, H, W), F32)}
    for name, (sx, sy) in {'shift +1': (1, 1), 'shift -1': (-1, -1), 'shift +(W-1)': (W - 1, H - 1), 'shift -(W-1)': (1 - W, 1 - H)}.items():
        f = np.zeros((B, 2, H, W), F32)
        f[:, 0], f[:, 1] = sx, sy
        out[name] = f
    xs, ys = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    for d in WARP_BORDER_D:
        tx = np.array([-d, 0.0, W - 1.0, W - 1.0 + d])
        ty = np.array([-d, 0.0, H - 1.0, H - 1.0 + d])
        yy, xx = np.mgrid[0:H, 0:W]
        f = np.zeros((B, 2, H, W), F32)
        f[:, 0] = (tx[(xx + yy) % 4] - xs).astype(F32)
        f[:, 1] = (ty[(xx // 2 + yy) % 4] - ys).astype(F32)
        out['border d = %g' % d] = f
    return out
