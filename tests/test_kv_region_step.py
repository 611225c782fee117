# -*- coding: utf-8 -*-
"""The key / value heads on the cells inside the boxes (RMNET_KV_REGION; csrc/conv_split.hip: conv_split_region) in the frame step,
and what their two consumers do with a cell outside the box.

  * The consumers (csrc/bank.hip).  bk_append builds its cell index from the rectangle and loads nothing else, so NaN outside the
    rectangles of the memory head's outputs changes no bit of the bank: ``stage`` + ``read_staged`` return the same bits as with
    zeros there, and the overflow word stays 0.  bk_main gathers the query key by compacted cell (NaN outside the query box
    changes no bit of the read-out, though it reaches the bank's logit word through the padding lanes of a query tile) but
    MULTIPLIES the query value by the box: NaN outside the box comes out as NaN in the second half of the read-out.  That is why
    the regional kernel writes +0.0 to every cell it does not compute.
  * The whole step at 96 x 160 over 3 frames, RMNET_KV_REGION=0 against 1: 2 clips of one object (both heads regional) and 1 clip
    of 2 objects (the query head is per clip and stays dense, the memory head is per object and regional) -- equal logits and
    probabilities (torch.equal), equal bank status and data bytes, equal range word; and the third step once from a captured graph.
    These reads see one or two memorised frames.  With three, the read merges partial results in arrival order and its bits
    change from run to run whatever the heads do (see the test): there the bank and the read's inputs are compared."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda', 0)


# ================================================================================================ the consumers
def _consumer_case():
    g = torch.Generator().manual_seed(41)
    no, h, w = 3, 9, 14
    k4 = torch.randn(no, 128, h, w, generator=g) * 0.6
    v4 = torch.randn(no, 512, h, w, generator=g)
    qk = torch.randn(no, 128, h, w, generator=g) * 0.6
    qv = torch.randn(no, 512, h, w, generator=g)
    mem = [(2, 11, 1, 6), (0, 13, 0, 8), (5, 5, 3, 3)]          # a box, the whole map, one cell
    qry = [(1, 9, 2, 7), (3, 13, 0, 4), (0, 13, 0, 8)]
    return no, h, w, k4, v4, qk, qv, mem, qry


def _outside(rects, no, h, w):
    m = torch.ones(no, 1, h, w, dtype=torch.bool)
    for o, (cx0, cx1, cy0, cy1) in enumerate(rects):
        m[o, 0, cy0:cy1 + 1, cx0:cx1 + 1] = False
    return m


def _read(no, h, w, k4, v4, qk, qv, mem, qry, precision):
    from rmnet_amd import ops
    bank = ops.MemoryBank(no, 2, h, w, dev(), precision=precision)
    t = lambda a: a.to(dev()).contiguous()
    mr = torch.tensor(mem, dtype=torch.int32, device=dev())
    qr = torch.tensor(qry, dtype=torch.int32, device=dev())
    bank.stage(t(k4), t(v4), mr)
    out = bank.read_staged(t(qk), t(qv), qr)
    torch.cuda.synchronize()
    return out, bank.status(), bank.areas().cpu().clone()


@pytest.mark.parametrize('precision', ['split', 'f16'])
def test_nan_outside_the_boxes_reaches_the_read_out_only_through_the_query_value(precision):
    no, h, w, k4, v4, qk, qv, mem, qry = _consumer_case()
    nan = torch.full((), float('nan'))
    m_out, q_out = _outside(mem, no, h, w), _outside(qry, no, h, w)
    assert bool(m_out[0].any()) and not bool(m_out[1].any()) and bool(q_out[0].any()) and not bool(q_out[2].any())
    zero = torch.zeros(())
    base = _read(no, h, w, torch.where(m_out, zero, k4), torch.where(m_out, zero, v4), torch.where(q_out, zero, qk),
                 torch.where(q_out, zero, qv), mem, qry, precision)
    assert base[1][0] == 0 and bool(torch.isfinite(base[0]).all())
    # the memory head's outputs: no cell outside the rectangle is loaded
    got = _read(no, h, w, torch.where(m_out, nan, k4), torch.where(m_out, nan, v4), torch.where(q_out, zero, qk),
                torch.where(q_out, zero, qv), mem, qry, precision)
    assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32))
    assert got[1] == base[1] and torch.equal(got[2], base[2])
    # the query key: gathered by compacted cell
    got = _read(no, h, w, torch.where(m_out, zero, k4), torch.where(m_out, zero, v4), torch.where(q_out, nan, qk),
                torch.where(q_out, zero, qv), mem, qry, precision)
    # (the bank's logit word is not compared here: a query tile's padding lanes load cell (0, 0) and multiply it by 0.0, which a
    # NaN survives -- measured in 'split': the word reads 26761.6 instead of 1.35.  Zero or any finite value there gives 0.)
    assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)) and got[1][:2] == base[1][:2]
    # the query value: multiplied by the box, so NaN outside it comes out -- in the second half of the read-out, outside the box, only
    got = _read(no, h, w, torch.where(m_out, zero, k4), torch.where(m_out, zero, v4), torch.where(q_out, zero, qk),
                torch.where(q_out, nan, qv), mem, qry, precision)
    assert torch.equal(got[0][:, :512].view(torch.int32), base[0][:, :512].view(torch.int32))
    second = got[0][:, 512:].cpu()
    assert torch.equal(torch.isnan(second), q_out.expand_as(second))
    assert torch.equal(torch.where(q_out, zero, second).view(torch.int32), base[0][:, 512:].cpu().view(torch.int32))


# ================================================================================================ the whole step
_net = []


def _network():
    if not _net:
        from rmnet_amd import networks
        from rmnet_amd.rmnet import RMNet
        torch.backends.cudnn.benchmark = False
        net = networks.procedural_init_(RMNet(None)).to(dev()).eval()
        net.fuse_epilogues()
        _net.append(net.to(memory_format=torch.channels_last))
    return _net[0]


CLIPS = {'2 clips of 1 object': (2, 2, [1, 1]), '1 clip of 2 objects': (1, 3, [2])}


def _clip(B, K):
    from rmnet_amd.synthetic import synthetic_clip
    clips = [synthetic_clip(4, K, 96, 160, seed=11 + c, size=1.5) for c in range(B)]
    frames = torch.cat([c[0] for c in clips]).to(dev())
    masks = torch.cat([c[1] for c in clips]).to(dev()).float()
    flows = torch.cat([c[2] for c in clips]).to(dev())
    return frames, masks, flows


def _steps(which, switch, monkeypatch, commits, graph=False):
    """Three frame steps with RMNET_KV_REGION = switch, step i committed when commits[i]: every step's (logits, probabilities), the
    bank's status, areas and bytes, the range word, how many heads got rectangles and what every read was given.  ``graph``: the
    third step is captured and replayed."""
    from rmnet_amd import _lib, ops
    B, K, n_max = CLIPS[which]
    net = _network()
    frames, masks, flows = _clip(B, K)
    monkeypatch.undo()              # (an earlier run's wrappers)
    monkeypatch.setenv('RMNET_KV_REGION', switch)
    heads, reads = [], []
    conv, read = ops.conv_split, ops.MemoryBank.read_staged
    monkeypatch.setattr(ops, 'conv_split', lambda *a, **kw: (heads.append(kw.get('rects') is not None), conv(*a, **kw))[1])

    def read_staged(self, q_key, q_val, qry_rects=None, **kw):
        if not torch.cuda.is_current_stream_capturing():
            reads.append((q_key.clone(), q_val.clone(), qry_rects.clone()))
        return read(self, q_key, q_val, qry_rects, **kw)
    monkeypatch.setattr(ops.MemoryBank, 'read_staged', read_staged)
    rw = ops.conv_range_word(dev())
    rw.zero_()
    ctx = net._ClipContext(net, B, K, 96, 160, n_max, dev())
    bank = net.new_bank(ctx, 4)
    outs = []
    step = lambda t: net.frame_step(ctx, bank, frames[:, t - 1], masks[:, t - 1], frames[:, t], flows[:, t], commit=commits[t - 1])
    with torch.no_grad():
        for t in (1, 2):
            outs.append(tuple(o.clone() for o in step(t)))
        if graph:
            assert not commits[2]
            side = torch.cuda.Stream(dev())
            side.wait_stream(torch.cuda.current_stream(dev()))
            with torch.cuda.stream(side):
                step(3)
            torch.cuda.current_stream(dev()).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = step(3)
            for o in out:
                o.fill_(float('nan'))
            g.replay()
            outs.append(tuple(o.clone() for o in out))
        else:
            outs.append(tuple(o.clone() for o in step(3)))
    torch.cuda.synchronize()
    # the bank's data: everything in front of its control block (whose queue words and counters belong to the read's workgroups)
    data = bank.blob[:_lib.load().rmnet_bank_overflow_offset(bank.no, bank.capacity, bank.h, bank.w)].clone()
    return dict(outs=outs, status=bank.status(), areas=bank.areas().cpu().clone(), data=data, range=int(rw.item()),
                heads=sum(heads), reads=reads)


def _same_outputs(off, on, steps):
    for t in steps:
        a, b = off['outs'][t], on['outs'][t]
        assert len(a) == len(b) == 2
        assert torch.equal(a[0], b[0]), 'logits of step %d' % t
        assert torch.equal(a[1], b[1]), 'probabilities of step %d' % t
        assert bool(torch.isfinite(b[1]).all())


def _same_bank(off, on, slots):
    assert off['status'] == on['status'] and off['status'][0] == 0
    assert torch.equal(off['areas'], on['areas']) and int(on['areas'][:, :slots].min()) > 0
    differ = (off['data'] != on['data']).nonzero()                # every byte: keys, values, tile and column sums, areas
    assert differ.numel() == 0, '%d of %d bytes of the bank differ, the first at %d' % (differ.shape[0], off['data'].numel(), int(differ[0]))
    assert off['range'] == on['range'] == 0


ONE = '2 clips of 1 object'


@pytest.mark.parametrize('which', list(CLIPS))
def test_the_step_computes_the_same_bits_with_the_heads_on_the_boxes(which, monkeypatch):
    """Three frames, the first memorised for good and the next two tentatively: reads of one and two memorised frames."""
    commits = (True, False, False)
    off = _steps(which, '0', monkeypatch, commits)
    on = _steps(which, '1', monkeypatch, commits)
    # the memory head in every step, the query head when every clip has one object
    assert off['heads'] == 0 and on['heads'] == (6 if which == ONE else 3)
    _same_outputs(off, on, (0, 1, 2))
    _same_bank(off, on, 2)


@pytest.mark.parametrize('which', list(CLIPS))
def test_three_memorised_frames_give_the_same_bank_and_the_same_read_inputs(which, monkeypatch):
    """With three memorised frames the read cuts an object's tiles into two chunks and merges their partial results in the order
    in which the workgroups arrive, so the third step's logits are not the same bits from run to run -- with the dense heads
    too, and on the commit before this kernel: there 2862 to 5858 of the 61440 logits of '2 clips of 1 object' differed between
    two runs of one process, by at most 7.2e-5 (measured on MI355X).  What is compared here is therefore what that read is GIVEN:
    every byte of the bank's data after the third stage, and the query key / value / rectangles of every read -- the dense bits inside
    the query box and +0.0 outside it (nothing but the dense bits when the query head stays dense)."""
    commits = (True, True, False)
    off = _steps(which, '0', monkeypatch, commits)
    on = _steps(which, '1', monkeypatch, commits)
    _same_outputs(off, on, (0, 1))
    _same_bank(off, on, 3)
    assert len(off['reads']) == len(on['reads']) == 3
    zero = torch.zeros((), device=dev())
    for (qk0, qv0, qr0), (qk1, qv1, qr1) in zip(off['reads'], on['reads']):
        assert torch.equal(qr0, qr1)
        inside = torch.ones(qk0.shape[0], 1, *qk0.shape[2:], dtype=torch.bool)
        if which == ONE:
            inside = ~_outside([tuple(r) for r in qr1.cpu().tolist()], *inside.shape[::2], inside.shape[3])
            assert bool(inside.any()) and not bool(inside.all())
        inside = inside.to(dev())
        assert torch.equal(qk1.view(torch.int32), torch.where(inside, qk0, zero).view(torch.int32))
        assert torch.equal(qv1.view(torch.int32), torch.where(inside, qv0, zero).view(torch.int32))


def test_the_regional_step_replays_from_a_captured_graph(monkeypatch):
    commits = (True, False, False)
    off = _steps(ONE, '0', monkeypatch, commits)
    on = _steps(ONE, '1', monkeypatch, commits, graph=True)
    assert on['heads'] == 8                  # (two eager steps, the warm-up of the capture and the capture)
    _same_outputs(off, on, (0, 1, 2))
    _same_bank(off, on, 2)
