# -*- coding: utf-8 -*-
"""Forward + backward of the memory read through rmnet.MemoryReader (csrc/memory_read_bwd.hip) next to autograd through a torch
restatement of the reference's bmm / soft-max formula (models/rmnet.py:147-165), on the same GPU, in the same process, alternated.

Two shapes: the reference's training shape (no = 12, T = 2, 30 x 30 cells: a 465 crop padded to 480, TRAIN.BATCH_SIZE x
N_MAX_OBJECTS, N_MAX_FRAMES = 3) and a 480p inference shape (no = 3, T = 5, 30 x 54), De = 128, Do = 512, dense.
Per shape and route: the median, minimum and maximum of CALLS timed calls (device events around one forward + backward, one
synchronise per call) after WARMUP calls of each route, the two routes taking turns call by call; the peak of
torch.cuda.max_memory_allocated above the inputs in a forward + backward; for our route the time of the backward alone
(ops.memory_read_backward between events) and its share of the fp32 matrix peak from the FLOPs counted below; the largest
difference between the two routes' gradients, relative to the largest gradient.  Also the per-element error / bound figures of the
tests' cases when run with --ratios (tests/read_backward_ref.py, on the GPU).

Writes profiles/r32_a_read_backward.md.  Needs the GPU; fails without one.

    python tools/read_backward_times.py [--calls 30] [--warmup 5] [--out profiles/r32_a_read_backward.md]"""

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX = 157.3e12          # MI355X: 256 CUs x 4 SIMDs x 64 FLOP / clk x 2.4 GHz (v_mfma_f32_16x16x4_f32)
SHAPES = (('training', 12, 2, 30, 30), ('inference 480p', 3, 5, 30, 54))
DE, DO = 128, 512


def backward_flops(no, T, h, w):
    """FLOPs of the backward kernels as they are written, dense: S three times (statistics twice over the memory -- maximum,
    then sum -- counted once per sweep: 2 sweeps, + once in each gradient pass = 4), dP twice, dV, dK, dQ once; 2 M N per channel."""
    M, N = T * h * w, h * w
    return no * 2.0 * M * N * (4 * DE + 2 * DO + DO + DE + DE)


def needed_flops(no, T, h, w):
    """The products the gradient needs at least once: S, dP, dV, dK, dQ."""
    M, N = T * h * w, h * w
    return no * 2.0 * M * N * (DE + DO + DO + DE + DE)


def torch_read(m_key, m_val, q_key, q_val):
    """models/rmnet.py:147-165, dense."""
    import math
    import torch
    B, De, T, H, W = m_key.shape
    Do = m_val.shape[1]
    mi = m_key.view(B, De, T * H * W).transpose(1, 2)
    qi = q_key.view(B, De, H * W)
    p = torch.bmm(mi, qi) / math.sqrt(De)
    p = torch.softmax(p, dim=1)
    mem = torch.bmm(m_val.view(B, Do, T * H * W), p).view(B, Do, H, W)
    return torch.cat([mem, q_val], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r32_a_read_backward.md'))
    ap.add_argument('--ratios', default='', help='file with the error / bound lines of the GPU tests to quote')
    args = ap.parse_args()
    assert args.calls >= 20
    import torch
    assert torch.cuda.is_available(), 'needs the GPU'
    from rmnet_amd import ops
    from rmnet_amd.rmnet import MemoryReader
    dev = torch.device('cuda', 0)
    reader = MemoryReader().train()
    lines = ['# Memory read: forward + backward, ours next to torch autograd', '',
             'Written by `tools/read_backward_times.py` (%d timed calls per route after %d warm-up calls, the routes alternating call by '
             'call, device events around each forward + backward).  %s, torch %s.' % (args.calls, args.warmup, torch.cuda.get_device_name(0),
                                                                                  torch.__version__), '']
    for name, no, T, h, w in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        mk = (torch.randn(no, DE, T, h, w, device=dev, generator=g) * 0.6).requires_grad_(True)
        mv = torch.randn(no, DO, T, h, w, device=dev, generator=g).requires_grad_(True)
        qk = (torch.randn(no, DE, h, w, device=dev, generator=g) * 0.6).requires_grad_(True)
        qv = torch.randn(no, DO, h, w, device=dev, generator=g).requires_grad_(True)
        wgt = torch.randn(no, 2 * DO, h, w, device=dev, generator=g)
        leaves = (mk, mv, qk, qv)

        def ours():
            out, _ = reader(*leaves)
            out.backward(wgt)

        def theirs():
            torch_read(*leaves).backward(wgt)

        routes = (('ours', ours), ('torch', theirs))
        grads, peak, times = {}, {}, {n: [] for n, _ in routes}
        for n, fn in routes:
            for _ in range(args.warmup):
                for l in leaves:
                    l.grad = None
                fn()
            torch.cuda.synchronize()
            grads[n] = [l.grad.clone() for l in leaves]
            for l in leaves:
                l.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[n] = torch.cuda.max_memory_allocated() - base
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2 * args.calls)]
        for i in range(args.calls):
            for k, (n, fn) in enumerate(routes):
                for l in leaves:
                    l.grad = None
                a, b = ev[2 * i + k]
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[n].append(a.elapsed_time(b) * 1e3)
        # the backward alone
        with torch.no_grad():
            out, _ = reader(*leaves)
        det = [l.detach() for l in leaves]
        bt = []
        for i in range(args.warmup + args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.memory_read_backward(*det, out, wgt)
            b.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                bt.append(a.elapsed_time(b) * 1e3)
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads['ours'], grads['torch']))
        M, N = T * h * w, h * w
        med = {n: statistics.median(t) for n, t in times.items()}
        bmed = statistics.median(bt)
        lines += ['## %s: no = %d, T = %d, %d x %d cells (M = %d, N = %d), De = %d, Do = %d' % (name, no, T, h, w, M, N, DE, DO), '',
                  '| route | forward + backward, median us | min | max | peak memory above the inputs, MiB |', '|---|---|---|---|---|']
        for n, _ in routes:
            lines.append('| %s | %.1f | %.1f | %.1f | %.1f |' % (n, med[n], min(times[n]), max(times[n]), peak[n] / 2.0 ** 20))
        lines += ['', 'ours / torch = %.2f (medians).  Largest gradient difference between the routes, relative to the largest gradient: %.2e.'
                  % (med['ours'] / med['torch'], diff), '',
                  'Backward alone (`ops.memory_read_backward`, all its launches): median %.1f us (min %.1f, max %.1f).  FLOPs as the kernels are '
                  'written (S four times, dP twice): %.2f G = %.1f TFLOP/s = %.1f %% of the fp32 matrix peak (%.1f TF); counting each needed '
                  'product once (%.2f G): %.1f %%.  The affinity the torch route keeps is no M N 4 = %.1f MiB per copy.'
                  % (bmed, min(bt), max(bt), backward_flops(no, T, h, w) / 1e9, backward_flops(no, T, h, w) / bmed / 1e6,
                     100 * backward_flops(no, T, h, w) / (bmed * 1e-6) / PEAK_F32_MATRIX, PEAK_F32_MATRIX / 1e12,
                     needed_flops(no, T, h, w) / 1e9, 100 * needed_flops(no, T, h, w) / (bmed * 1e-6) / PEAK_F32_MATRIX,
                     no * M * N * 4 / 2.0 ** 20), '']
        print('\n'.join(lines[-9:]))
    if args.ratios and os.path.exists(args.ratios):
        lines += ['## Error / bound', '', open(args.ratios).read().rstrip(), '']
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
