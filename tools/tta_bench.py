# -*- coding: utf-8 -*-
"""Multi-scale and flipped inference (csrc/tta.hip, inference.segment_video_tta) on a 70-frame 854 x 480 clip, scales (0.75, 1.0, 1.25)
plus the left-right flip, i.e. six entries:

  kernels  the two kernels alone between device events, on K = 11 probability clips and on the frames: 5 warm-up calls, then the
           median of 20 calls, the bytes each has to move (every source read once + every output written once, from the shapes)
           over that time, against the 6.3 TB/s that a float4 copy reaches on an MI355X; and the torch sequence that ``tta_merge``
           replaces (flip, interpolate, stack, mean, argmax) the same way.  torch.cuda.max_memory_allocated above what is live
           before the call, for both.  The two means are compared (they need not be equal in the last bits: torch's GPU kernel
           fuses) and the label maps counted.
  call     the whole call on a one-object and on a three-object clip, RMNet + TinyFlowNet with the procedural weights: paired
           (a scale's two clips as one batch of two), unpaired, and through helpers.multi_scale_inference followed by argmax.
           One warm-up call each, then three timed calls each, alternating the three, host clock around a device synchronise.

    python tools/tta_bench.py            # every step in a child process of its own, under a time limit

The driver stops at the first step that does not return 0: nothing is started on the GPU after a step that failed there.
"""

import argparse
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, K, H, W = 70, 11, 480, 854
SCALES, FLIP = (0.75, 1.0, 1.25), True
HBM_COPY_TBS = 6.3                   # what a float4 copy reaches on an MI355X (8 TB/s on paper)
STEPS = (('kernels', 420), ('call', 900))      # (step, time limit in seconds)
RUNS = 3


def _median_ms(torch, fn, warm=5, calls=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    q = statistics.quantiles(times, n=10)
    return statistics.median(times), q[0], q[-1]


def _peak_mb(torch, fn):
    """Peak of the allocator during one call, above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak / 1e6


def torch_merge(torch, sources, flipped, size):
    """What multi_scale_inference and the driver do with the entries' probabilities."""
    F = torch.nn.functional
    resized = [F.interpolate(torch.flip(s, dims=[3]) if f else s, size=size, mode='bilinear', align_corners=False) for s, f in zip(sources, flipped)]
    mean = torch.mean(torch.stack(resized), dim=0)
    return mean, torch.argmax(mean, dim=1)


def step_kernels():
    import torch
    from rmnet_amd import ops, tta
    assert torch.cuda.is_available(), 'this step needs a GPU'
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    sources, flipped = [], []
    for fs in SCALES:
        h, w = tta.scaled_size(H, W, fs)
        for f in ((False, True) if FLIP else (False,)):
            sources.append(torch.softmax(3.0 * torch.randn(N, K, h, w, device=dev, generator=gen), dim=1))
            flipped.append(f)
    frames = torch.randn(N, 3, H, W, device=dev, generator=gen)
    src_bytes = sum(s.numel() * 4 for s in sources)
    out_bytes = N * K * H * W * 4 + N * H * W
    print('%d frames of %d x %d, K = %d, %d entries %s%s; median of 20 calls between device events (10 %% .. 90 %%)'
          % (N, W, H, K, len(sources), SCALES, ' + flip' if FLIP else ''))
    print('| step | ms per call | 10 %% .. 90 %% | MB moved | TB/s | share of %.1f TB/s | peak MB above the inputs |' % HBM_COPY_TBS)
    print('|---|---|---|---|---|---|---|')
    rows = [('rmnet_tta_merge_f32 (mean + labels)', lambda: ops.tta_merge(sources, flipped, H, W), src_bytes + out_bytes),
            ('  torch: flip, interpolate, stack, mean, argmax', lambda: torch_merge(torch, sources, flipped, (H, W)), src_bytes + out_bytes)]
    for fs in SCALES:
        h, w = tta.scaled_size(H, W, fs)
        sc = tta.scale_for_factor(fs)
        rows.append(('rmnet_resize_bilinear_f32 frames x%g, mirrored' % fs, lambda h=h, w=w, sc=sc: ops.resize_bilinear(frames, h, w, sc, sc, True),
                     frames.numel() * 4 + N * 3 * h * w * 4))
    rows.append(('  torch: flip(interpolate(frames, x1.25))',
                 lambda: torch.flip(torch.nn.functional.interpolate(frames, scale_factor=1.25, mode='bilinear', align_corners=False), dims=[3]),
                 frames.numel() * 4 + N * 3 * 600 * 1067 * 4))
    for name, fn, nbytes in rows:
        med, lo, hi = _median_ms(torch, fn)
        tbs = nbytes / (med * 1e-3) / 1e12
        print('| %s | %.3f | %.3f .. %.3f | %.0f | %.2f | %.0f %% | %.0f |' % (name, med, lo, hi, nbytes / 1e6, tbs, 100 * tbs / HBM_COPY_TBS, _peak_mb(torch, fn)))
    mean, labels = ops.tta_merge(sources, flipped, H, W)
    t_mean, t_labels = torch_merge(torch, sources, flipped, (H, W))
    print('kernel against the torch sequence: largest difference of the means %.3e, label maps equal at %.6f of the pixels'
          % (float((mean - t_mean).abs().max()), float((labels.long() == t_labels).float().mean())))
    torch.cuda.synchronize()


def step_call():
    import torch
    from rmnet_amd import helpers, inference, networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    from rmnet_amd.tiny_flownet import TinyFlowNet
    assert torch.cuda.is_available(), 'this step needs a GPU'
    dev = torch.device('cuda', 0)
    net = networks.procedural_init_(RMNet(None)).to(dev).eval()
    tfn = networks.procedural_init_(TinyFlowNet(None)).to(dev).eval()
    cfg = SimpleNamespace(TEST=SimpleNamespace(FRAME_SCALES=list(SCALES), FLIP_LR=FLIP, MEMORIZE_EVERY=5))
    print('%d frames of %d x %d, scales %s%s; seconds per call, host clock around a device synchronise, %d timed calls each after one warm-up '
          'call each, the three variants alternating' % (N, W, H, SCALES, ' + flip' if FLIP else '', RUNS))
    print('| clip | variant | seconds per call (each run) | median | peak MB above the inputs |')
    print('|---|---|---|---|---|')
    for n_obj in (1, 3):
        frames, masks, _, n_objects = synthetic_clip(N, n_obj + 1, H, W, seed=5, size=1.5)
        frames, masks = frames.to(dev), masks.to(dev)
        video = {'frames': frames[0], 'masks': masks[0], 'n_objects': n_obj}

        def mirror():
            with torch.no_grad():
                _, probs = helpers.multi_scale_inference(cfg, tfn, net, frames, masks, n_objects)
                return probs, probs[0].argmax(dim=1).to(torch.uint8)

        variants = (('segment_video_tta, paired', lambda: inference.segment_video_tta(net, tfn, video, SCALES, FLIP, 5, pair_flips=True)),
                    ('segment_video_tta, unpaired', lambda: inference.segment_video_tta(net, tfn, video, SCALES, FLIP, 5, pair_flips=False)),
                    ('helpers.multi_scale_inference + argmax', mirror))
        times = {name: [] for name, _ in variants}
        peaks = {}
        results = {}
        for name, fn in variants:                      # warm-up: every shape of the timed calls
            peaks[name] = _peak_mb(torch, fn)
        for _ in range(RUNS):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
                results[name] = out['labels'] if isinstance(out, dict) else out[1]
                del out
        for name, _ in variants:
            print('| %d object%s | %s | %s | %.3f | %.0f |' % (n_obj, 's' if n_obj > 1 else '', name, ', '.join('%.3f' % t for t in times[name]),
                                                            statistics.median(times[name]), peaks[name]))
        base = results['helpers.multi_scale_inference + argmax']
        for name in list(times)[:2]:
            print('  %s: label maps equal to the mirror\'s at %.6f of the pixels' % (name, float((results[name] == base).float().mean())))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        {'kernels': step_kernels, 'call': step_call}[args.step]()
        return 0
    for step, limit in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print('step %s ended with status %d: stopping here' % (step, rc))
            return rc if rc > 0 else 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
