# -*- coding: utf-8 -*-
"""Every-branch tests of the oldest kernels, rmnet_amd/csrc/region_map.hip (region_reduce<VEC4>, region_reduce_warped,
region_fill<VEC4>, boxes_to_rects, rect_mask_kernel) and rmnet_amd/csrc/flow_affine.hip, next to the random-rectangle comparisons of
test_gpu_parity.py:
  1. CPU: the numpy restatements of tests/region_ref.py reproduce the committed fixtures and the oracle's C on every case of this
     file; cell_rect is pinned by enumeration against F.interpolate(padded map, scale_factor=1/16); flow_affine is pinned by
     tests/golden/flow_affine_edges.npz, recorded from the reference's own compiled C++; plan() against hand-worked values;
  2. GPU, through the C entries with caller-owned, pre-filled and guarded buffers, every comparison exact: a probe pixel on every
     seam of the reduction (float4 lanes, unroll slots, base passes, band ends, the waves' row stride, 1-row and 1-column shapes,
     the sentinel's neighbour), the count pinned to the unit, the threshold compare on NaN / Inf / neighbours / -0.0, the alignment
     branches, loosen and fill at the seams, the fused cell rectangles, the argument rules;
  3. GPU: the flow-warped region map against RMNet.warp on new shapes and on flows that land on the frame's border;
  4. GPU: rect_mask (sign of zero, NaN, the second loop pass, extreme rectangles) and flow_affine (halves, neighbours, clamp
     equalities, the row loop past 4096, the alignment rule);
  5. CPU: every planted fault of region_ref.MUTANTS fails a named case."""

import ctypes
import json
import os
import time

import numpy as np
import pytest
import torch

import region_ref as R

NAN_BITS = 0x7fc00000
INT_FILL = 0x7f7f7f7f
GUARD = 64                     # words behind every output
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4      # include/rmnet_hip.h


def dev():
    return torch.device('cuda', 0)


# ================================================================================================ CPU: plan and restatement pins
def test_plan_lands_every_shape_on_its_named_geometry():
    """chunks_for restated, against values worked by hand from region_map.hip (planes = B * (K - 1); chunks = ceil(1024 / planes)
    capped at 256 and at ceil(H / 4); rows = ceil(H / chunks))."""
    for shape, (what, want) in R.REGION_SHAPES.items():
        assert R.plan(*shape) == want, (shape, what, R.plan(*shape))
        print('PLAN %-20s chunks %3d rows %3d vec %-5s %s' % (shape, want[0], want[1], want[2], what))
    B, K, H, W = 2, 3, 13, 260
    chunks, rows, _ = R.plan(B, K, H, W)
    assert [min(H, (c + 1) * rows) - c * rows for c in range(chunks)] == [4, 4, 4, 1]       # the last band holds one row
    chunks, rows, _ = R.plan(4, 16, 100, 8)
    assert (chunks - 1) * rows >= 100 and (chunks - 2) * rows < 100                          # the trailing band is empty
    assert R.plan(1, 1, 7, 8) == (2, 4, True)                                                # K = 1: planes counts as 1
    assert R.workspace_bytes(2, 3, 13, 260) == 2 * 3 * 4 * 32


def _kat_mask(c):
    m = np.zeros((c['B'], c['K'], c['H'], c['W']), np.float32)
    for f in c['fills']:
        m[f['b'], f['k'], f['y0']:f['y1'] + 1, f['x0']:f['x1'] + 1] = f['v']
    return m


def _same_region(a, b):
    return R.bits_equal(a[0], b[0])[0] and np.array_equal(a[1], b[1])


def test_region_map_restatement_reproduces_the_fixtures(golden_dir, oracle_mod):
    """region_map_kat.json, region_boxes.npz and region_fuzz.npz (through cases.boxes_after_loosen): the same boxes, and the map
    and boxes of the oracle's C on each."""
    import sys
    sys.path.insert(0, golden_dir)
    import cases
    kat = json.load(open(os.path.join(golden_dir, 'region_map_kat.json')))
    for c in kat['cases']:
        got = R.region_map(_kat_mask(c), c['thr'], c['npts'], c['loose'])
        assert np.array_equal(got[1], np.array(c['bboxes'], np.int32)), c['name']
        assert _same_region(got, oracle_mod.region_map(_kat_mask(c), c['thr'], c['npts'], c['loose'])), c['name']
    g = np.load(os.path.join(golden_dir, 'region_boxes.npz'))
    for i, (B, K, H, W) in enumerate(cases.REGION_BOX_SHAPES):
        m = cases.region_box_case(i)
        want = cases.boxes_from_reference_tight(g['case%02d.tight' % i], K, H, W).reshape(B, K, 4)
        got = R.region_map(m, 0.5, 1, 0)
        assert np.array_equal(got[1], want), i
        assert _same_region(got, oracle_mod.region_map(m, 0.5, 1, 0)), i
    g = np.load(os.path.join(golden_dir, 'region_fuzz.npz'))
    for i, (B, K, H, W) in enumerate(cases.REGION_FUZZ_SHAPES[:16]):          # (the 8 shapes twice; the other 24 repeat them)
        m = cases.region_fuzz_case(i)
        for L in cases.REGION_FUZZ_LOOSE:
            for npt in cases.REGION_FUZZ_NPTS:
                want = cases.boxes_after_loosen(g['case%02d.tight' % i], g['case%02d.npts' % i], K, H, W, npt, L).reshape(B, K, 4)
                assert np.array_equal(R.region_map(m, 0.5, npt, L)[1], want), (i, L, npt)


def _region_named_cases():
    """(name, mask, thr, n_pts, loose) of every region-map case the GPU tests run, cheapest families first."""
    for shape in R.REGION_SHAPES:
        for i, (mask, _) in enumerate(R.probe_masks(shape)):
            yield 'probe %s call %d' % (shape, i), mask, R.THR, 1, 0
    for shape in R.REGION_SHAPES:
        for i, (mask, _) in enumerate(R.probe_masks(shape, pairs=True)):
            yield 'probe pair %s call %d' % (shape, i), mask, R.THR, 1, 0
    for thr in R.THRESHOLD_VALUES:
        for W in (12, 13):
            yield 'threshold %r W %d' % (thr, W), R.threshold_case(thr, W), thr, 1, 0
            yield 'threshold %r W %d, n_pts 0' % (thr, W), R.threshold_case(thr, W), thr, 0, 2
    for W in (12, 13):
        for thr in (-1.0, 0.0):
            yield 'everything counts, thr %r W %d' % (thr, W), R.everything_counts_case(W), thr, 10, 1
    for shape in R.SEAM_SHAPES:
        for L in R.SEAM_LOOSE:
            for i, (mask, npt) in enumerate(_seam_masks(shape, L)):
                yield 'seam %s loose %d call %d' % (shape, L, i), mask, 0.5, npt, L
    for shape in R.COUNT_SHAPES:
        mask, n = R.count_case(shape)
        yield 'count %s n_pts = n' % (shape,), mask, R.THR, n, R.COUNT_LOOSE
        yield 'count %s n_pts = n + 1' % (shape,), mask, R.THR, n + 1, R.COUNT_LOOSE
        for i, (pm, n) in enumerate(R.count_probe_masks(shape)):
            yield 'count %s + probe, call %d, n_pts = n + 1' % (shape, i), pm, R.THR, n + 1, R.COUNT_LOOSE
            yield 'count %s + probe, call %d, n_pts = n + 2' % (shape, i), pm, R.THR, n + 2, R.COUNT_LOOSE
    for shape in R.ALIGN_SHAPES:
        yield 'alignment %s' % (shape,), R.align_case(shape), 0.5, 10, 3


def _seam_masks(shape, L):
    """region_ref.seam_masks plus, for loose > 0, the clamp equalities x1 + loose == W and y1 + loose == H (x0 == y0 == loose)."""
    for mask, npt in R.seam_masks(shape, L):
        yield mask, npt
    B, K, H, W = shape
    if L > 0:
        mask = np.zeros(shape, np.float32)
        x1, y1 = W - L, (H - L if H - L >= 0 else H - 1)
        mask[:, 1:, min(L, y1), min(L, x1)] = 0.5
        mask[:, 1:, y1, x1] = 0.5
        yield mask, 2


def test_region_map_restatement_equals_the_oracle_on_the_cases_of_this_file(oracle_mod):
    """One call of every family and shape (the first of each name group) through rmnet_oracle.c: same map, same boxes; the probe
    family's closed form on the restatement itself."""
    seen = set()
    n = 0
    for name, mask, thr, npt, L in _region_named_cases():
        group = name.split(' call ')[0]
        if group in seen:
            continue
        seen.add(group)
        assert _same_region(R.region_map(mask, thr, npt, L), oracle_mod.region_map(mask, thr, npt, L)), name
        n += 1
    assert n >= 45
    for shape in R.REGION_SHAPES:
        for pairs in (False, True):
            for mask, placed in R.probe_masks(shape, pairs=pairs):
                att, bb = R.region_map(mask, R.THR, 1, 0)
                B, K, H, W = shape
                for b in range(B):
                    for k in range(1, K):
                        pts = placed.get((b, k))
                        if pts is None:
                            assert tuple(bb[b, k]) == (0, W - 1, 0, H - 1)
                        elif not pairs:
                            (x, y), = pts
                            assert tuple(bb[b, k]) == (x, x, y, y) and att[b, k].sum() == 1 and att[b, k, y, x] == 1
                        else:
                            (x, y), (x2, y2) = pts
                            assert tuple(bb[b, k]) == (x, x2, y2, y)
                break                                                    # (the first call of each: the others differ in the points only)


def test_count_family_is_pinned_to_the_unit():
    """n_pts == n gives the tight box loosened, n_pts == n + 1 the full frame -- in the restatement, where the count is a plain sum."""
    for shape in R.COUNT_SHAPES:
        B, K, H, W = shape
        mask, n = R.count_case(shape)
        chunks, rows, _ = R.plan(*shape)
        hit = mask[0, 1] >= R.THR
        assert int(hit.sum()) == n and n >= 12
        ys, xs = np.nonzero(hit)
        assert len(set(ys // rows)) >= 3 and xs.min() < 64 <= xs.max()           # several bands, both unroll slots
        assert xs.min() >= 2 and xs.max() <= W - 3 and ys.min() >= 2 and ys.max() <= H - 3
        _, tight = R.region_map(mask, R.THR, n, R.COUNT_LOOSE)
        _, full = R.region_map(mask, R.THR, n + 1, R.COUNT_LOOSE)
        assert tuple(tight[0, 1]) == (xs.min() - 1, xs.max() + 1, ys.min() - 1, ys.max() + 1)
        assert tuple(full[0, 1]) == (0, W - 1, 0, H - 1) and tuple(tight[0, 1]) != tuple(full[0, 1])


def test_lt_for_le_in_the_lower_clamps_is_the_same_function():
    """``v < L ? 0 : v - L`` and ``v <= L ? 0 : v - L`` agree on every integer (at v == L both give 0), so these two 'faults' of the
    issue's list cannot be planted: no output differs.  Enumerated instead of argued."""
    for m in R.EQUIVALENT_MUTANTS:
        for L in range(-3, 70):
            for v in list(range(-3, 140)) + [32767]:
                box = (v, v + 5, v, v + 5)
                assert R.loosen(5, box, 200, 200, 1, L, fault=m) == R.loosen(5, box, 200, 200, 1, L), (m, L, v)


def test_cell_rect_is_the_interpolated_box_map_by_enumeration(oracle_mod):
    """Every 0 <= x0 <= x1 < W for W in {1, 5, 16, 17, 31, 33, 47, 48} x pad_l in {0, 1, 7, 8, 15, the centring pad}: the cells of
    region_ref.cell_rect are exactly the non-zero cells of F.interpolate(padded box map, scale_factor=1/16), one axis at a time (the
    rule is separable: the other axis holds the whole frame); and oracle_cell_rects_i32 says the same."""
    import torch.nn.functional as F
    total = 0
    for W in R.CELL_ENUM_W:
        boxes = R.cell_enum_boxes(W)
        for pad in R.cell_enum_pads(W):
            Wp = -(-(W + pad) // 16) * 16
            cw = Wp // 16
            m = torch.zeros(len(boxes), 1, 16, Wp)
            for i, (a, b) in enumerate(boxes):
                m[i, 0, :, pad + a:pad + b + 1] = 1
            small = F.interpolate(m, scale_factor=1 / 16)
            assert tuple(small.shape) == (len(boxes), 1, 1, cw)
            small = small[:, 0, 0].numpy()
            full = np.array([(a, b, 0, 15) for a, b in boxes], np.int32)
            for axis in (0, 1):                                          # the same enumeration on x and on y
                bx = full if axis == 0 else full[:, [2, 3, 0, 1]]
                args = (pad, 0, 16, 1, cw) if axis == 0 else (0, pad, 16, cw, 1)
                got = R.cell_rects(bx, 0, *args)
                orc = oracle_mod.cell_rects(np.concatenate([bx[:1], bx])[None], args[0], args[1], args[3], args[4])[0, 1:]
                assert np.array_equal(got, orc), (W, pad, axis)
                for i in range(len(boxes)):
                    c0, c1, o0, o1 = got[i] if axis == 0 else got[i][[2, 3, 0, 1]]
                    cells = np.flatnonzero(small[i])
                    if cells.size == 0:
                        assert tuple(got[i]) == R.EMPTY_RECT, (W, pad, boxes[i])
                    else:
                        assert (c0, c1, o0, o1) == (cells[0], cells[-1], 0, 0) and cells.size == c1 - c0 + 1, (W, pad, boxes[i])
            total += len(boxes)
    assert total == 18345
    # the k_per_batch rule of rmnet_boxes_to_cell_rects_i32 and the empty box
    bx = np.array([[0, 47, 0, 15]] * 7, np.int32)
    assert [tuple(r) for r in R.cell_rects(bx, 3, 0, 0, 16, 1, 3)] == [R.EMPTY_RECT, (0, 2, 0, 0), (0, 2, 0, 0)] * 2 + [R.EMPTY_RECT]
    assert all(tuple(r) == (0, 2, 0, 0) for r in R.cell_rects(bx, 0, 0, 0, 16, 1, 3))
    assert R.cell_rect((0, 47, 0, 15), 0, 0, 16, 1, 2) == (0, 1, 0, 0)                       # clamped to cw - 1
    assert R.cell_rect(R.SENTINEL, 0, 0, 16, 4, 4) == R.EMPTY_RECT


def test_flow_affine_restatement_reproduces_the_reference_fixtures(golden_dir, oracle_mod):
    """tests/golden/flow_affine_edges.npz (the reference's compiled C++ on the cases of region_ref.flow_cases, recorded by
    make_flow_affine_edges_golden.py) and the older flow_affine.npz: the same bits, NaN at the same positions; the fixture's inputs
    are the ones region_ref builds today; rmnet_oracle.c agrees as well.  Also what the cases are there for: -0.0 outputs exist,
    NaN outputs exist, and 0.49999997 is the input that trunc(x + 0.5) in fp32 gets wrong (3.4999998 is not)."""
    g = np.load(os.path.join(golden_dir, 'flow_affine_edges.npz'))
    cases = R.flow_cases()
    assert list(g['names']) == list(cases)
    neg_zero = nans = 0
    for i, (name, (flow, m1, m2)) in enumerate(cases.items()):
        for key, value in (('flow', flow), ('m1', m1), ('m2', m2)):
            assert R.bits_equal(g['case%02d.%s' % (i, key)], value)[0], (name, key)
        want = g['case%02d.out' % i]
        ok, first, n = R.bits_equal(R.flow_affine(flow, m1, m2), want)
        assert ok, (name, first, n)
        assert R.bits_equal(oracle_mod.flow_affine(flow, m1, m2), want)[0], name
        neg_zero += int((np.signbit(want) & (want == 0)).sum())
        nans += int(np.isnan(want).sum())
    assert neg_zero >= 6 and nans >= 5
    name, H, W, seed = R.FLOW_TALL
    assert str(g['tall.name']) == name and int(g['tall.seed']) == seed and list(g['tall.shape']) == [H, W]
    tall = R.flow_affine(*R.flow_tall_case())
    assert R.digest(tall) == str(g['tall.digest'])
    assert R.bits_equal(tall[:2], g['tall.first_rows'])[0] and R.bits_equal(tall[-3:], g['tall.last_rows'])[0]
    old = np.load(os.path.join(golden_dir, 'flow_affine.npz'))
    for n in sorted({k.split('.')[0] for k in old.files}):
        assert R.bits_equal(R.flow_affine(old[n + '.flow'], old[n + '.m1'], old[n + '.m2']), old[n + '.out'])[0], n
    x = np.array([R.BELOW_HALF, 3.4999998], np.float32)
    assert list(np.trunc(x + np.float32(0.5))) == [1.0, 3.0] and list(R._round_half_away(x)) == [0.0, 3.0]


def test_rect_mask_restatement_equals_the_oracle_and_keeps_signs_and_nans(oracle_mod):
    for shape in R.RECT_SHAPES:
        x, rects, pick = R.rect_case(shape)
        want = R.rect_mask(x, rects)
        assert R.bits_equal(want, oracle_mod.rect_mask(x, rects))[0], shape
        if x.size > 1:
            assert len({k for row in pick for k in row}) == shape[0] * shape[2]          # every (n, t) pair its own kind
            outside = want != x
            assert (np.signbit(want) & (want == 0) & outside).any() and (np.isnan(want) & ~np.isnan(x)).any()   # -0.0 and inf * 0
            assert np.isnan(want[np.isnan(x)]).all()


# ================================================================================================ CPU: planted faults
def _flow_fault_case(m):
    for name, (flow, m1, m2) in list(R.flow_cases().items()) + [(R.FLOW_TALL[0], R.flow_tall_case())]:
        if not R.bits_equal(R.flow_affine(flow, m1, m2, fault=m), R.flow_affine(flow, m1, m2))[0]:
            return name
    return None


def _cell_named_cases():
    """(name, boxes, k_per_batch, grid arguments) of the stand-alone boxes_to_cell_rects launches."""
    for W in R.CELL_ENUM_W:
        xb = np.array(R.cell_enum_boxes(W), np.int32)
        yb = xb[np.random.default_rng(W).permutation(len(xb))]
        boxes = np.concatenate([xb, yb], axis=1)
        for pi, pad in enumerate(R.cell_enum_pads(W)):
            cw = -(-(W + pad) // 16)
            yield 'enumeration W %d pad %d' % (W, pad), boxes, (0, 1, 3)[pi % 3], (pad, pad, 16, cw, cw)
        if W in (33, 48):
            cw = -(-W // 16) - 1
            yield 'enumeration W %d on a grid one cell short' % W, boxes, 0, (0, 0, 16, cw, cw)


def _fault_case(m):
    if m in R.FLOW_MUTANTS:
        return _flow_fault_case(m)
    if m in R.RECT_MUTANTS:
        for shape in R.RECT_SHAPES:
            x, rects, _ = R.rect_case(shape)
            if not R.bits_equal(R.rect_mask(x, rects, fault=m), R.rect_mask(x, rects))[0]:
                return 'rect_mask %s' % (shape,)
        return None
    if m in R.CELL_MUTANTS:
        for name, boxes, kpb, grid in _cell_named_cases():
            if not np.array_equal(R.cell_rects(boxes, kpb, *grid, fault=m), R.cell_rects(boxes, kpb, *grid)):
                return name
        return None
    for name, mask, thr, npt, L in _region_named_cases():
        if not _same_region(R.region_map(mask, thr, npt, L, fault=m), R.region_map(mask, thr, npt, L)):
            return name
    return None


def test_each_planted_fault_fails_a_named_case():
    """For every entry of region_ref.MUTANTS the restatement with that fault differs from the clean one on a named GPU case, so
    a kernel with the fault fails that case's exact comparison.  (Not planted, with the reasons in region_ref.py: padding lanes
    counting when thr <= 0, and ``<`` for ``<=`` in the two lower clamps, which is the same function.)"""
    missed = []
    for m in R.MUTANTS:
        t0 = time.time()
        name = _fault_case(m)
        print('MUTANT %-28s %s  (%.1f s)' % (m, 'caught by "%s"' % name if name else 'MISSED', time.time() - t0))
        if name is None:
            missed.append(m)
    assert not missed, missed
    assert len(R.MUTANTS) == 21


# ================================================================================================ GPU helpers
def _p(addr):
    return ctypes.c_void_p(int(addr)) if addr else None


def _lib():
    from rmnet_amd import _lib
    return _lib.load()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _ibits(t):
    """int32 view of a float tensor with every NaN made the one quiet NaN."""
    t = t.contiguous()
    return t.view(torch.int32).masked_fill(t != t, NAN_BITS)


def _assert_same(got, want, what):
    """Exact: int32 tensors as they are, float tensors by their bits (a NaN matching a NaN); names the first difference."""
    if isinstance(want, np.ndarray):
        want = _t(want)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    gi = _ibits(got) if got.dtype == torch.float32 else got
    wi = _ibits(want) if want.dtype == torch.float32 else want
    if torch.equal(gi, wi):
        return
    bad = (gi != wi).flatten().nonzero().flatten()
    i = int(bad[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(want.shape)))
    pytest.fail('%s: %d of %d elements differ; first at %s: got %r, want %r' % (
        what, bad.numel(), want.numel(), idx, got.flatten()[i].item(), want.flatten()[i].item()))


class _RegionBuffers(object):
    """Caller-owned buffers of one shape: every output pre-filled (NaN bits / 0x7f7f7f7f), 64 guard words behind each, the
    workspace exactly rmnet_region_map_workspace_bytes long inside a guarded buffer, room for byte offsets in front of mask and att."""

    def __init__(self, shape):
        B, K, H, W = shape
        self.shape, self.n = shape, B * K * H * W
        self.lib = _lib()
        self.nws = int(self.lib.rmnet_region_map_workspace_bytes(B, K, H, W))
        assert self.nws == R.workspace_bytes(B, K, H, W), (shape, self.nws)          # plan() is the library's plan
        d = dev()
        self.mask = torch.zeros(self.n + 4, dtype=torch.float32, device=d)
        self.att = torch.empty(self.n + GUARD + 4, dtype=torch.int32, device=d)
        self.warped = torch.empty(self.n + GUARD, dtype=torch.int32, device=d)
        self.bb = torch.empty(B * K * 4 + GUARD, dtype=torch.int32, device=d)
        self.cr = torch.empty(B * K * 4 + GUARD, dtype=torch.int32, device=d)
        self.cr2 = torch.empty(B * K * 4 + GUARD, dtype=torch.int32, device=d)
        self.ws = torch.empty(self.nws + 4 * GUARD, dtype=torch.uint8, device=d)
        for t in (self.mask, self.att, self.bb, self.cr, self.ws):
            assert t.data_ptr() % 16 == 0
        assert self.n * 4 < 64 << 20

    def run(self, mask, thr, n_pts, loose, grid, att=True, rects=True, mask_off=0, att_off=0, ws_fill=0x7f, flow=None, warped=False):
        """One call of rmnet_region_map_f32 (or, with ``flow``, rmnet_region_map_warped_f32); checks the return code, the guards and
        the words in front of a shifted att; returns (att | None, bboxes, cell_rects | None[, warped]) as views."""
        B, K, H, W = self.shape
        n, nb = self.n, B * K * 4
        mo, ao = mask_off // 4, att_off // 4
        mv = self.mask[mo:mo + n]
        mv.copy_(mask.reshape(-1) if isinstance(mask, torch.Tensor) else _t(mask).reshape(-1))
        self.att.fill_(NAN_BITS)
        self.warped.fill_(NAN_BITS)
        self.bb.fill_(INT_FILL)
        self.cr.fill_(INT_FILL)
        self.ws.fill_(ws_fill)
        pl, pt, st, ch, cw = grid
        a_ptr = self.att.data_ptr() + att_off if att else 0
        tail = [_p(self.bb.data_ptr()), _p(self.cr.data_ptr() if rects else 0), pl, pt, st, ch, cw]
        if flow is None:
            rc = self.lib.rmnet_region_map_f32(_p(mv.data_ptr()), B, K, H, W, float(thr), int(n_pts), int(loose), _p(a_ptr), *tail,
                                               _p(self.ws.data_ptr()), self.nws, None)
        else:
            rc = self.lib.rmnet_region_map_warped_f32(_p(mv.data_ptr()), _p(flow.data_ptr()), B, K, H, W, float(thr), int(n_pts),
                                                      int(loose), _p(a_ptr), *tail, _p(self.warped.data_ptr() if warped else 0),
                                                      _p(self.ws.data_ptr()), self.nws, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((self.att[ao + n:] == NAN_BITS).all()) and bool((self.att[:ao] == NAN_BITS).all()), 'att guard'
        assert bool((self.bb[nb:] == INT_FILL).all()) and bool((self.cr[nb:] == INT_FILL).all()), 'bboxes / cell_rects guard'
        assert bool((self.ws[self.nws:] == ws_fill).all()), 'workspace guard'
        assert bool((self.warped[n:] == NAN_BITS).all()), 'warped guard'
        if not att:
            assert bool((self.att == NAN_BITS).all()), 'att written although NULL was passed'
        if not rects:
            assert bool((self.cr == INT_FILL).all())
        out = (self.att[ao:ao + n].view(torch.float32).view(B, K, H, W) if att else None, self.bb[:nb].view(B, K, 4),
               self.cr[:nb].view(B, K, 4) if rects else None)
        return out + (self.warped[:n].view(torch.float32).view(B, K, H, W),) if warped else out

    def rects_of(self, boxes, grid):
        """rmnet_boxes_to_cell_rects_i32 on device boxes [B,K,4] with k_per_batch = K."""
        B, K = self.shape[:2]
        self.cr2.fill_(INT_FILL)
        rc = self.lib.rmnet_boxes_to_cell_rects_i32(_p(boxes.data_ptr()), B * K, K, *grid, _p(self.cr2.data_ptr()), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((self.cr2[B * K * 4:] == INT_FILL).all())
        return self.cr2[:B * K * 4].view(B, K, 4)

    def check(self, mask, thr, n_pts, loose, what, **kw):
        """The call twice (the second time on a workspace pre-filled with other garbage): both the restatement's bits in every
        word of att, bboxes and cell_rects; cell_rects also what rmnet_boxes_to_cell_rects_i32 makes of the returned boxes."""
        B, K, H, W = self.shape
        grid = R.cell_grid_of(H, W)
        w_att, w_bb = R.region_map(mask, thr, n_pts, loose)
        w_cr = R.cell_rects(w_bb, K, *grid)
        w_att, w_bb, w_cr = _t(w_att), _t(w_bb), _t(w_cr)
        md = _t(mask)
        for run, fill in enumerate((0x7f, 0xff)):
            att, bb, cr = self.run(md, thr, n_pts, loose, grid, ws_fill=fill, **kw)
            tag = '%s, run %d' % (what, run)
            _assert_same(bb, w_bb, tag + ', bboxes')
            if cr is not None:
                _assert_same(cr, w_cr, tag + ', cell_rects')
                _assert_same(self.rects_of(bb, grid), w_cr, tag + ', rmnet_boxes_to_cell_rects_i32 of the boxes')
            if att is not None:
                _assert_same(att, w_att, tag + ', att')
        return w_bb


# ================================================================================================ GPU: region map
@pytest.mark.gpu
def test_the_exact_comparison_rejects_one_wrong_word():
    """The comparison every GPU test of this file uses, on a real output: it accepts the restatement, and it fails on one flipped
    pixel, on the sign of one zero, on a box that is off by one and on the expectation of a planted fault."""
    shape = (1, 3, 9, 67)
    buf = _RegionBuffers(shape)
    mask, _ = next(iter(R.probe_masks(shape)))
    att, bb, cr = buf.run(_t(mask), R.THR, 1, 0, R.cell_grid_of(9, 67))
    w_att, w_bb = R.region_map(mask, R.THR, 1, 0)
    _assert_same(att, w_att, 'att')
    _assert_same(bb, w_bb, 'bboxes')
    flipped, signed, off = w_att.copy(), w_att.copy(), w_bb.copy()
    flipped[0, 1, 8, 66] = 1.0 - flipped[0, 1, 8, 66]
    signed[0, 0, 0, 0] = -0.0
    off[0, 2, 1] += 1
    f_att, f_bb = R.region_map(mask, R.THR, 1, 0, fault='gt_for_ge')
    for got, wrong in ((att, flipped), (att, signed), (bb, off), (att, f_att), (bb, f_bb)):
        with pytest.raises(pytest.fail.Exception):
            _assert_same(got, wrong, 'must differ')


@pytest.mark.gpu
@pytest.mark.parametrize('shape', list(R.REGION_SHAPES), ids=lambda s: 'x'.join(map(str, s)))
def test_region_map_probe_pixel_on_every_seam(shape):
    """n_pts = 1, loose = 0, one pixel exactly at the threshold per live plane on a background of the fp32 number below it, channel
    0 all ones: the box is (x, x, y, y) and att a single 1 (asserted on the restatement by the CPU test above; here the kernel
    against the restatement, every word).  x over {0..5, 62..65, 252..259, 511..513, 1020..1027, W-5..W-1}, y over {0..4, rows-1,
    rows, rows+1, H-2, H-1}; then two probes per plane, so that (x_min, y_max) and (x_max, y_min) come from different records."""
    assert R.plan(*shape) == R.REGION_SHAPES[shape][1]
    buf = _RegionBuffers(shape)
    t0 = time.time()
    calls = 0
    for pairs in (False, True):
        for i, (mask, placed) in enumerate(R.probe_masks(shape, pairs=pairs)):
            buf.check(mask, R.THR, 1, 0, 'probe%s %s call %d' % (' pair' if pairs else '', shape, i))
            calls += 1
    print('REGION probe %-20s plan %s: %d probes, %d calls x 2 runs, %.2f s' % (shape, R.plan(*shape), len(R.probes(*shape)), calls, time.time() - t0))


@pytest.mark.gpu
def test_region_map_k_1_writes_channel_0_only():
    """K = 1: no reduce launch at all; att all zeros, box (0,0,0,0), rect (1,0,1,0), whatever the workspace holds."""
    for shape in [(1, 1, 7, 8), (3, 1, 5, 9)]:
        buf = _RegionBuffers(shape)
        bb = buf.check(np.ones(shape, np.float32), 0.5, 1, 0, 'K = 1 %s' % (shape,))
        assert int(bb.abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('shape', R.COUNT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_region_map_count_is_exact_to_the_unit(shape):
    """A checkerboard of n hits over several bands and both unroll slots: n_pts = n gives the tight box loosened, n_pts = n + 1 the
    full frame; then one extra hit at every probe position with n + 1 and n + 2.  A pixel dropped or counted twice anywhere flips
    one of the two."""
    buf = _RegionBuffers(shape)
    mask, n = R.count_case(shape)
    t0 = time.time()
    tight = buf.check(mask, R.THR, n, R.COUNT_LOOSE, 'count %s n_pts = n' % (shape,))
    full = buf.check(mask, R.THR, n + 1, R.COUNT_LOOSE, 'count %s n_pts = n + 1' % (shape,))
    assert not torch.equal(tight[:, 1:], full[:, 1:])
    calls = 0
    for i, (pm, n) in enumerate(R.count_probe_masks(shape)):
        buf.check(pm, R.THR, n + 1, R.COUNT_LOOSE, 'count %s + probe call %d, n_pts = n + 1' % (shape, i))
        buf.check(pm, R.THR, n + 2, R.COUNT_LOOSE, 'count %s + probe call %d, n_pts = n + 2' % (shape, i))
        calls += 2
    print('REGION count %-20s n = %d, %d calls x 2 runs, %.2f s' % (shape, n, calls + 2, time.time() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize('W', [12, 13])
def test_region_map_threshold_compare(W):
    """``>=`` in fp32 on thr, its two neighbours, NaN, +-Inf, a subnormal and -0.0 (thr = 0.5, 0.0 and +Inf), one value per
    channel; n_pts = 0 on the same masks (an empty channel then keeps the sentinels through the clamps); thr = -1 and 0 on a
    non-negative mask: everything counts."""
    for thr in R.THRESHOLD_VALUES:
        mask = R.threshold_case(thr, W)
        buf = _RegionBuffers(mask.shape)
        bb = buf.check(mask, thr, 1, 0, 'threshold %r W %d' % (thr, W)).cpu().numpy()
        with np.errstate(invalid='ignore'):
            counts = np.array(R.THRESHOLD_VALUES[thr], np.float32) >= np.float32(thr)
        for c, yes in enumerate(counts):                                 # (closed form: the one-pixel box, or the full frame)
            assert tuple(bb[0, c + 1]) == (((5 * c + 3) % W,) * 2 + (1, 1) if yes else (0, W - 1, 0, 2)), (thr, c)
        assert counts.any() and not counts.all()
        buf.check(mask, thr, 0, 2, 'threshold %r W %d, n_pts 0' % (thr, W))
    mask = R.everything_counts_case(W)
    buf = _RegionBuffers(mask.shape)
    for thr in (-1.0, 0.0):
        bb = buf.check(mask, thr, 10, 1, 'everything counts, thr %r W %d' % (thr, W)).cpu().numpy()
        assert all(tuple(bb[b, k]) == (0, W - 1, 0, 6) for b in range(2) for k in (1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', R.ALIGN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_region_map_alignment_branches_give_the_same_bits(shape):
    """W % 4 == 0 with mask, then att, 4, 8 and 12 bytes past a 16-byte boundary (the launcher must take the scalar kernels):
    the bits of the aligned call; att = NULL with and without cell_rects."""
    assert R.plan(*shape)[2]
    buf = _RegionBuffers(shape)
    mask = R.align_case(shape)
    buf.check(mask, 0.5, 10, 3, 'aligned %s' % (shape,))
    for off in (4, 8, 12):
        buf.check(mask, 0.5, 10, 3, 'mask + %d bytes %s' % (off, shape), mask_off=off)
        buf.check(mask, 0.5, 10, 3, 'att + %d bytes %s' % (off, shape), att_off=off)
        buf.check(mask, 0.5, 10, 3, 'mask and att + %d bytes %s' % (off, shape), mask_off=off, att_off=off)
    buf.check(mask, 0.5, 10, 3, 'att NULL %s' % (shape,), att=False)
    buf.check(mask, 0.5, 10, 3, 'att NULL, cell_rects NULL %s' % (shape,), att=False, rects=False)
    buf.check(mask, 0.5, 10, 3, 'cell_rects NULL %s' % (shape,), rects=False)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', R.SEAM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_region_map_loosen_and_fill_at_the_seams(shape):
    """loose in {0, 1, 3, 64}: filled rectangles that start and end at x % 4 = 0, 1, 2, 3, on the first and the last row of a band,
    and the clamp equalities x1 + loose == W, y1 + loose == H, x0 == y0 == loose."""
    buf = _RegionBuffers(shape)
    starts = set()
    for L in R.SEAM_LOOSE:
        for i, (mask, npt) in enumerate(_seam_masks(shape, L)):
            bb = buf.check(mask, 0.5, npt, L, 'seam %s loose %d call %d' % (shape, L, i)).cpu().numpy()
            starts |= {(int(b[0]) % 4, int(b[1]) % 4) for b in bb[:, 1:].reshape(-1, 4)}
    assert {s for s, _ in starts} == {0, 1, 2, 3} and {e for _, e in starts} == {0, 1, 2, 3}


@pytest.mark.gpu
def test_boxes_to_cell_rects_on_the_whole_enumeration():
    """rmnet_boxes_to_cell_rects_i32 alone, one launch per (W, pad) on every 0 <= x0 <= x1 < W paired with a permutation of the
    same boxes in y; k_per_batch in {0, 1, 3}; n_boxes is no multiple of 256; and two grids one cell short (the cw - 1 clamp)."""
    lib = _lib()
    launches = total = 0
    for name, boxes, kpb, grid in _cell_named_cases():
        n = len(boxes)
        assert n == 1 or n % 256 != 0
        want = R.cell_rects(boxes, kpb, *grid)
        bd = _t(boxes)
        out = torch.full((n * 4 + GUARD,), INT_FILL, dtype=torch.int32, device=dev())
        rc = lib.rmnet_boxes_to_cell_rects_i32(_p(bd.data_ptr()), n, kpb, *grid, _p(out.data_ptr()), None)
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        assert bool((out[n * 4:] == INT_FILL).all()), name
        _assert_same(out[:n * 4].view(n, 4), want, name + ', k_per_batch %d' % kpb)
        launches += 1
        total += n
    print('CELL %d launches, %d boxes' % (launches, total))


def _pool_check(fn, order, good, cases, pool, accepted=()):
    """Every case changes the good call in one respect: the entry returns the code and leaves the pool alone."""
    def call(**kw):
        a = dict(good, **kw)
        return fn(*[(_p(a[k]) if k in good['_ptrs'] else a[k]) for k in order])

    ref = pool.clone()
    for name, kw, want in cases:
        rc = call(**kw)
        assert rc == want, (name, rc, want)
        torch.cuda.synchronize()
        assert torch.equal(pool, ref), name
    for kw in accepted + ({},):
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()
    assert not torch.equal(pool, ref)                   # (the good call writes)


@pytest.mark.gpu
def test_region_entries_reject_bad_arguments_and_leave_the_buffers_alone():
    """rmnet_region_map_f32, _warped_f32, rmnet_boxes_to_cell_rects_i32, rmnet_rect_mask_f32: each NULL, each non-positive size,
    H or W = 32768, a workspace one byte short, warped without flow, cell_rects with a non-positive stride or grid -- the code of
    include/rmnet_hip.h, and not a word of any buffer changed."""
    lib = _lib()
    pool = torch.full((1 << 14,), INT_FILL, dtype=torch.int32, device=dev())
    base = pool.data_ptr()
    at = lambda words: base + 4 * words
    B, K, H, W = 2, 3, 5, 8
    nws = int(lib.rmnet_region_map_workspace_bytes(B, K, H, W))
    assert nws == R.workspace_bytes(B, K, H, W) and lib.rmnet_region_map_workspace_bytes(0, K, H, W) == 0
    pool[:B * K * H * W] = 0                            # the mask: finite
    ref_ptrs = {'mask', 'flow', 'att', 'bb', 'cr', 'warped', 'ws', 'stream'}
    good = dict(_ptrs=ref_ptrs, mask=at(0), flow=at(8192), B=B, K=K, H=H, W=W, thr=0.5, n_pts=1, loose=1, att=at(1024), bb=at(2048), cr=at(2304),
                pad_l=4, pad_t=5, stride=16, ch=1, cw=1, warped=at(3072), ws=at(4096), ws_bytes=nws, stream=0)
    pool[8192:8192 + B * 2 * H * W] = 0                 # the flow: zeros
    order = ['mask', 'B', 'K', 'H', 'W', 'thr', 'n_pts', 'loose', 'att', 'bb', 'cr', 'pad_l', 'pad_t', 'stride', 'ch', 'cw', 'ws', 'ws_bytes', 'stream']
    cases = ([('no %s' % n, {n: 0}, E_INVALID) for n in ('mask', 'bb')] + [('no workspace', dict(ws=0), E_WORKSPACE)] +
             [('%s = %d' % (n, v), {n: v}, E_INVALID) for n in ('B', 'K', 'H', 'W') for v in (0, -1)] +
             [('%s = 32768' % n, {n: 32768}, E_INVALID) for n in ('H', 'W')] +
             [('%s = 65536' % n, {n: 65536}, E_UNSUPPORTED) for n in ('B', 'K')] +
             [('workspace one byte short', dict(ws_bytes=nws - 1), E_WORKSPACE)] +
             [('cell_rects with %s = %d' % (n, v), {n: v}, E_INVALID) for n in ('stride', 'ch', 'cw') for v in (0, -1)])
    accepted = (dict(att=0), dict(cr=0, stride=0, ch=0, cw=0), dict(att=0, cr=0))
    _pool_check(lib.rmnet_region_map_f32, order, good, cases, pool, accepted)
    pool[1024:8192] = INT_FILL
    order_w = ['mask', 'flow'] + order[1:16] + ['warped', 'ws', 'ws_bytes', 'stream']
    no_flow = [('warped without flow', dict(flow=0), E_INVALID), ('no flow (this entry wants one, with or without warped)', dict(flow=0, warped=0), E_INVALID)]
    _pool_check(lib.rmnet_region_map_warped_f32, order_w, good, cases + no_flow, pool, accepted + (dict(warped=0),))
    pool[1024:8192] = INT_FILL
    pool[:64] = torch.arange(64, dtype=torch.int32, device=dev())
    good = dict(_ptrs={'bb', 'cr', 'stream'}, bb=at(0), n=16, kpb=3, pad_l=1, pad_t=2, stride=16, ch=4, cw=4, cr=at(1024), stream=0)
    order = ['bb', 'n', 'kpb', 'pad_l', 'pad_t', 'stride', 'ch', 'cw', 'cr', 'stream']
    cases = ([('no %s' % n, {n: 0}, E_INVALID) for n in ('bb', 'cr')] +
             [('%s = %d' % (n, v), {n: v}, E_INVALID) for n in ('n', 'stride', 'ch', 'cw') for v in (0, -1)])
    _pool_check(lib.rmnet_boxes_to_cell_rects_i32, order, good, cases, pool, (dict(kpb=0), dict(kpb=-1)))
    pool[1024:8192] = INT_FILL
    pool[:64] = 0
    good = dict(_ptrs={'x', 'rects', 'y', 'stream'}, x=at(2048), n=1, C=2, T=2, h=3, w=4, rects=at(0), y=at(1024), stream=0)
    order = ['x', 'n', 'C', 'T', 'h', 'w', 'rects', 'y', 'stream']
    cases = ([('no %s' % n, {n: 0}, E_INVALID) for n in ('x', 'rects', 'y')] +
             [('%s = %d' % (n, v), {n: v}, E_INVALID) for n in ('n', 'C', 'T', 'h', 'w') for v in (0, -1)])
    _pool_check(lib.rmnet_rect_mask_f32, order, good, cases, pool)


# ================================================================================================ GPU: flow-warped region map
@pytest.mark.gpu
@pytest.mark.parametrize('shape', R.WARP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_region_map_of_the_warped_mask_on_border_flows(shape):
    """rmnet_region_map_warped_f32 against RMNet.warp on the same GPU (the contract is the bits PyTorch-ROCm produces), torch.equal
    on the warped mask, boxes, rects and map: a 1-row and a 1-column frame, a second base pass of one pixel (W = 257), W = 300;
    zero flow, integer shifts of +-1 and +-(W-1), and samples that land on -d, 0, W-1 and W-1+d for d from 2e-5 to 1e-3, which puts
    the validity sum on both sides of 0.9999 (asserted on the torch result).  Non-finite flows are out of scope: the conversion of
    a NaN coordinate to an integer is undefined in both implementations."""
    from rmnet_amd.rmnet import RMNet
    net = RMNet(None)
    B, K, H, W = shape
    buf = _RegionBuffers(shape)
    grid = R.cell_grid_of(H, W)
    g = torch.Generator().manual_seed(H * 1000 + W)
    m = torch.rand(B, K, H, W, generator=g).to(dev())
    yy, xx = np.mgrid[0:H, 0:W]
    off_frame = torch.from_numpy((((xx + yy) % 4) % 3 == 0) & (W > 1) | (((xx // 2 + yy) % 4) % 3 == 0) & (H > 1)).to(dev())
    seen = set()
    for name, flow in R.warp_flows(shape).items():
        f = _t(flow)
        want, valid = net.warp(m, f)
        want = want.contiguous()
        if name.startswith('border'):
            seen |= {float(v) for v in valid[:, 0][off_frame.expand(B, H, W)].unique()}
        att0, bb0, rc0 = [t.clone() for t in buf.run(want, 0.5, 3, 2, grid)]
        for run, fill in enumerate((0x7f, 0xff)):
            att1, bb1, rc1, got = buf.run(m, 0.5, 3, 2, grid, flow=f, warped=True, ws_fill=fill)
            tag = 'warped %s, %s, run %d' % (shape, name, run)
            assert bool((got.view(torch.int32)[:, 0] == NAN_BITS).all()), tag + ': channel 0 of warped is not to be touched'
            assert torch.equal(got[:, 1:], want[:, 1:]), tag + ', warped mask'
            assert torch.equal(bb1, bb0) and torch.equal(rc1, rc0) and torch.equal(att1, att0), tag
        _, bb2, _ = buf.run(m, 0.5, 3, 2, grid, flow=f, att=False, rects=False)
        assert torch.equal(bb2, bb0), 'warped %s, %s, boxes only' % (shape, name)
    assert seen == {0.0, 1.0}, seen                     # both validity outcomes occur among the samples that leave the frame


# ================================================================================================ GPU: rect_mask
@pytest.mark.gpu
@pytest.mark.parametrize('shape', R.RECT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rect_mask_keeps_the_multiply_semantics(shape):
    """x * 0 outside the rectangle: NaN and +-Inf give NaN, negative values -0.0 (bits compared, NaN by position); 323 cells reach
    the kernel's second loop pass with a ragged tail; every (n, t) pair has a different kind of rectangle (whole grid, empty, first
    and last cell, sticking out, inverted in one axis, INT32_MIN / INT32_MAX), in two rotations."""
    lib = _lib()
    n, C, T, h, w = shape
    for rot in (0, 3):
        x, rects, pick = R.rect_case(shape, rot)
        want = R.rect_mask(x, rects)
        xd, rd = _t(x), _t(rects)
        y = torch.full((x.size + GUARD,), NAN_BITS, dtype=torch.int32, device=dev())
        for run in range(2):
            rc = lib.rmnet_rect_mask_f32(_p(xd.data_ptr()), n, C, T, h, w, _p(rd.data_ptr()), _p(y.data_ptr()), None)
            assert rc == 0
            torch.cuda.synchronize()
            assert bool((y[x.size:] == NAN_BITS).all())
            _assert_same(y[:x.size].view(torch.float32).view(shape), want, 'rect_mask %s rotation %d (%s)' % (shape, rot, pick))
        assert bool((_ibits(xd) == _ibits(_t(x))).all())                    # x is not written


# ================================================================================================ GPU: flow affine
def _flow_all_cases():
    return list(R.flow_cases().items()) + [(R.FLOW_TALL[0], R.flow_tall_case())]


@pytest.mark.gpu
def test_flow_affine_edges_bit_for_bit_through_every_entry():
    """The cases of tests/golden/flow_affine_edges.npz (pinned to the reference's C++ by the CPU test above) through
    rmnet_flow_affine_f32 on guarded buffers, rmnet_flow_affine_f32_host and update_optical_flow: the restatement's bits, -0.0
    included, NaN at the same positions; 4099 rows reach the row loop behind gridDim.y = 4096."""
    from rmnet_amd import flow_affine_transformation as fat
    lib = _lib()
    for name, (flow, m1, m2) in _flow_all_cases():
        H, W = flow.shape[:2]
        want = R.flow_affine(flow, m1, m2)
        t0 = time.time()
        fd, ad, bd = _t(flow), _t(m1), _t(m2)
        out = torch.full((H * W * 2 + GUARD,), NAN_BITS, dtype=torch.int32, device=dev())
        for run in range(2):
            rc = lib.rmnet_flow_affine_f32(_p(fd.data_ptr()), _p(ad.data_ptr()), _p(bd.data_ptr()), H, W, _p(out.data_ptr()), None)
            assert rc == 0, (name, rc)
            torch.cuda.synchronize()
            assert bool((out[H * W * 2:] == NAN_BITS).all()), name
            _assert_same(out[:H * W * 2].view(torch.float32).view(H, W, 2), want, 'rmnet_flow_affine_f32, %s' % name)
        nws = int(lib.rmnet_flow_affine_workspace_bytes(H, W))
        ws = torch.full((nws + 4 * GUARD,), 0x7f, dtype=torch.uint8, device=dev())
        host = np.full((H, W, 2), np.nan, np.float32)
        fl, a, b = (np.ascontiguousarray(v, np.float32) for v in (flow, m1, m2))
        rc = lib.rmnet_flow_affine_f32_host(fl.ctypes.data, a.ctypes.data, b.ctypes.data, H, W, host.ctypes.data, _p(ws.data_ptr()), nws, None)
        assert rc == 0 and bool((ws[nws:] == 0x7f).all()), name
        ok, first, nbad = R.bits_equal(host, want)
        assert ok, ('rmnet_flow_affine_f32_host', name, first, nbad)
        ok, first, nbad = R.bits_equal(fat.update_optical_flow(flow, m1, m2), want)
        assert ok, ('update_optical_flow', name, first, nbad)
        print('FLOW %-50s %4d x %3d  %.3f s' % (name, H, W, time.time() - t0))


@pytest.mark.gpu
def test_flow_affine_alignment_rule_is_enforced_before_any_launch():
    """flow and out are accessed as float2: 8-byte alignment for both, 4 for the matrices, RMNET_E_INVALID_ARG otherwise with every
    buffer untouched (the kernel is never launched on such a pointer).  The _host entry's staging pointers are workspace,
    workspace + 256 and workspace + 256 + 8*H*W: an 8-byte aligned workspace satisfies the rule, any other is refused."""
    lib = _lib()
    pool = torch.full((4096,), INT_FILL, dtype=torch.int32, device=dev())
    base = pool.data_ptr()
    assert base % 256 == 0
    H, W = 3, 5
    pool[:H * W * 2 + 64] = 0
    pool[1024:1036] = torch.tensor([1, 0, 0, 0, 1, 0] * 2, dtype=torch.float32).view(torch.int32).to(dev())
    good = dict(_ptrs={'flow', 'm1', 'm2', 'out', 'stream'}, flow=base, m1=base + 4096, m2=base + 4096 + 24, H=H, W=W, out=base + 8192, stream=0)
    order = ['flow', 'm1', 'm2', 'H', 'W', 'out', 'stream']
    cases = ([('no %s' % n, {n: 0}, E_INVALID) for n in ('flow', 'm1', 'm2', 'out')] +
             [('%s = %d' % (n, v), {n: v}, E_INVALID) for n in ('H', 'W') for v in (0, -1)] +
             [('%s + 4 bytes' % n, {n: good[n] + 4}, E_INVALID) for n in ('flow', 'out')] +
             [('%s + %d bytes' % (n, d), {n: good[n] + d}, E_INVALID) for n in ('m1', 'm2') for d in (1, 2, 3)] +
             [('%s = 2^24' % n, {n: 1 << 24}, E_UNSUPPORTED) for n in ('H', 'W')])
    accepted = (dict(flow=base + 8, out=base + 8192 + 8), dict(m1=base + 4096 + 4, m2=base + 4096 + 28))
    _pool_check(lib.rmnet_flow_affine_f32, order, good, cases, pool, accepted)
    # the _host entry
    pool.fill_(INT_FILL)
    nws = int(lib.rmnet_flow_affine_workspace_bytes(H, W))
    assert nws == H * W * 16 + 256 and (256 + H * W * 8) % 8 == 0 and lib.rmnet_flow_affine_workspace_bytes(0, W) == 0
    flow = np.zeros((H, W, 2), np.float32)
    m = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    out = np.full((H, W, 2), 7.0, np.float32)
    call = lambda ws, nbytes, f=flow.ctypes.data, o=out.ctypes.data: lib.rmnet_flow_affine_f32_host(f, m.ctypes.data, m.ctypes.data, H, W, o, _p(ws), nbytes, None)
    ref = pool.clone()
    for what, rc, want in (('no flow', call(base, nws, f=None), E_INVALID), ('no out', call(base, nws, o=None), E_INVALID),
                           ('no workspace', call(0, nws), E_WORKSPACE), ('workspace one byte short', call(base, nws - 1), E_WORKSPACE),
                           ('workspace + 4 bytes', call(base + 4, nws), E_INVALID)):
        assert rc == want, (what, rc, want)
        torch.cuda.synchronize()
        assert torch.equal(pool, ref) and bool((out == 7.0).all()), what
    assert call(base + 8, nws) == 0 and bool((out == 0.0).all())                # 8-byte aligned is enough
    assert torch.empty(256, dtype=torch.uint8, device=dev()).data_ptr() % 8 == 0  # what ops._ws hands to the entry
