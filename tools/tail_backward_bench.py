# -*- coding: utf-8 -*-
"""The decoder tail (2-class soft-max, soft aggregation, un-pad, soft-max over K) forward + backward, two ways on one GPU:

  fused   RMNet.decoder_tail on a CUDA tensor: ops.soft_aggregate under autograd, rmnet_soft_aggregate_f32 forward and
          rmnet_soft_aggregate_bwd_f32 (csrc/soft_aggregate_bwd.hip) backward, one launch each;
  graph   the module graph (F.softmax -> RMNet.soft_aggregation -> slicing -> F.softmax) under torch autograd on the same GPU: the
          yardstick, never the code under test.

Shapes: the reference's training batch (config.py TRAIN: 4 x 3 crops of 465 x 465, padded to 480 x 480; every crop a clip of its
own with 1 or 3 objects) and one 480 x 854 frame padded to 480 x 864 with 1, 3 and 10 objects (K = objects + 1).  The loss is
sum(prob * g) with a fixed random g, so that the backward gets a dense grad_prob as from the training loss.  For each: the backward
kernel alone, forward + backward of both routes -- HIP events around calls issued back to back, median / min / max over rounds --,
torch.cuda.max_memory_allocated above what the inputs take, and the kernel's bytes per second over the bytes it must move
(2n floats of dec read, 2n of grad_dec written, 2K of prob and grad_prob read per pixel), next to the 6.3 TB/s of a float4 copy.

    python tools/tail_backward_bench.py                 # every shape in a child process of its own, under `timeout -k 10`

The driver stops at the first step that does not return 0: nothing is started on the GPU after a step that failed there.
"""

import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> (clips, objects per clip, H, W)
SHAPES = {'train1': (12, 1, 465, 465), 'train3': (12, 3, 465, 465), 'frame1': (1, 1, 480, 854), 'frame3': (1, 3, 480, 854), 'frame10': (1, 10, 480, 854)}
LIMIT = 240


def timed(fn, rounds=7, calls=10):
    """ms per call: `calls` calls back to back between two HIP events, `rounds` times, after a warm-up."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return ms


def peak_above_inputs(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def step_shape(step):
    import torch
    import torch.nn.functional as F
    from rmnet_amd import ops
    from rmnet_amd.helpers import pad_amounts
    from rmnet_amd.rmnet import RMNet
    assert torch.cuda.is_available(), 'this step needs a GPU'
    B, n, H, W = SHAPES[step]
    K = n + 1
    pad = pad_amounts(H, W, 16)
    lw, uw, lh, uh = pad
    Hp, Wp = H + lh + uh, W + lw + uw
    gen = torch.Generator(device='cuda').manual_seed(n)
    dec = (torch.randn(B * n, 2, Hp, Wp, generator=gen, device='cuda') * 3.0).requires_grad_(True)
    g = torch.randn(B, K, H, W, generator=gen, device='cuda')
    counts = [n] * B
    begin = torch.arange(0, B * n + 1, n, dtype=torch.int32, device='cuda')
    net = RMNet(None).train()
    print('%s: %d clips of %d objects, %d x %d padded to %d x %d, K %d (dec %.1f MB, prob %.1f MB)'
          % (step, B, n, H, W, Hp, Wp, K, dec.numel() * 4 / 1e6, g.numel() * 4 / 1e6))

    def fused():
        dec.grad = None
        _, prob = net.decoder_tail(dec, counts, K, pad)
        (prob * g).sum().backward()
        return dec.grad

    def graph():
        dec.grad = None
        ps = F.softmax(dec, dim=1)[:, 1]
        logit = net.soft_aggregation(ps, K, counts)
        logit = logit[:, :, lh:logit.shape[2] - uh, lw:logit.shape[3] - uw]
        (F.softmax(logit, dim=1) * g).sum().backward()
        return dec.grad

    def loss_only():                                     # what both routes share: the product with g, its sum and their backward
        p = prob0.detach().requires_grad_(True)
        (p * g).sum().backward()

    with torch.no_grad():
        _, prob0 = ops.soft_aggregate(dec.detach(), begin, K, pad, want_prob=True)
    def graph64():                                       # the module graph in float64: what both fp32 routes are measured against
        d64 = dec.detach().double().requires_grad_(True)
        logit = net.soft_aggregation(F.softmax(d64, dim=1)[:, 1], K, counts)
        logit = logit[:, :, lh:logit.shape[2] - uh, lw:logit.shape[3] - uw]
        (F.softmax(logit, dim=1) * g.double()).sum().backward()
        return d64.grad

    a, b, c = fused().clone(), graph().clone(), graph64()
    da, db = (a.double() - c).abs(), (b.double() - c).abs()
    print('  against the module graph in float64 (largest |grad| %.3e): fused max %.3e, %d elements above 1e-5;  fp32 graph max %.3e, %d elements above 1e-5'
          % (float(c.abs().max()), float(da.max()), int((da > 1e-5).sum()), float(db.max()), int((db > 1e-5).sum())))
    del a, b, c, da, db
    torch.cuda.empty_cache()
    bwd = timed(lambda: ops.soft_aggregate_backward(dec.detach(), begin, K, pad, prob0, g, None, None))
    bytes_moved = (2 * n + 2 * n) * Hp * Wp * 4 * B + 2 * K * H * W * 4 * B
    print('  backward kernel alone: median %.4f ms (min %.4f, max %.4f); %.1f MB to move: %.2f TB/s (float4 copy: 6.3 TB/s)'
          % (statistics.median(bwd), min(bwd), max(bwd), bytes_moved / 1e6, bytes_moved / statistics.median(bwd) / 1e9))
    for name, fn in (('fused', fused), ('graph', graph), ('the loss sum(prob * g) and its backward alone', loss_only)):
        ms = timed(fn)
        print('  forward + backward, %-45s median %.4f ms (min %.4f, max %.4f)' % (name + ':', statistics.median(ms), min(ms), max(ms)))
    dec.grad = None
    for name, fn in (('fused', fused), ('graph', graph)):
        print('  peak memory above the inputs, %s: %.1f MB' % (name, peak_above_inputs(fn)))
        dec.grad = None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=list(SHAPES))
    args = ap.parse_args()
    if args.step:
        step_shape(args.step)
        return 0
    for step in SHAPES:
        print('--- step %s' % step, flush=True)
        rc = subprocess.run(['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__), '--step', step]).returncode
        if rc != 0:
            print('step %s ended with status %d: stopping here' % (step, rc))
            return rc if rc > 0 else 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
