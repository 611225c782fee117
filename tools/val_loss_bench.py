# -*- coding: utf-8 -*-
"""The validation loss (Lovasz-softmax + NLL, core/test.py:97) of one 70-frame 480 x 854 clip with K = 3 and K = 11 classes, two
ways on one GPU:

  hip    ops.clip_loss (csrc/val_loss.hip: one histogram pass, one scan) + the few tensor operations of losses.validation_loss;
  torch  the sort-based route of rmnet_amd/losses.py on the same device tensors (the reference's formula: a sort of all pixels
         per class, float64 running counts).

For each: HIP events around calls issued back to back, the median wall time of calls that each sit between two stream
synchronisations, torch.cuda.max_memory_allocated above what the inputs take, the value, and for 'hip' the bracket width, the
share of (pixel, class) elements whose key left the workgroup as an individual global atomic (a key outside the bins kept in
LDS), the share aggregated over the wave (keys 0 and `bins`), and the per-kernel split from torch.profiler when it gives one.  The probabilities are synthetic
peaked soft-maxes ('synth') and the output of RMNet.forward with procedural weights on a synthetic clip ('real').

    python tools/val_loss_bench.py            # every step in a child process of its own, under `timeout -k 10`

The driver stops at the first step that does not return 0: nothing is started on the GPU after a step that failed there.
"""

import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 70, 480, 854
BINS = 1 << 20
# (step, time limit in seconds)
STEPS = (('resources', 300), ('synth3', 300), ('synth11', 420), ('real3', 420), ('real11', 600))


def lds_bins(K, bins):
    """(LB, HB): the lowest and the highest bins that vl_hist keeps in LDS (csrc/val_loss.hip, lds_bins)."""
    s = 1
    while 2 * s * 2 * K <= 15872:
        s *= 2
    return (bins + 1, 0) if bins + 1 <= s else (s // 2, s // 2)


def step_resources(_):
    from rmnet_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'val_loss.s')
        subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                        os.path.join(build.CSRC, 'val_loss.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', asm, flags=re.S).group(1)
    for entry in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]:
        if '.vgpr_count:' not in entry:
            continue
        get = lambda key: re.search(r'^\s*\.%s:\s+(\S+)' % key, entry, flags=re.M).group(1)
        print('%-60s VGPRs %s (spilled %s)  SGPRs %s  scratch %s B  static LDS %s B' % (
            get('name'), get('vgpr_count'), get('vgpr_spill_count'), get('sgpr_count'), get('private_segment_fixed_size'),
            get('group_segment_fixed_size')))


def synthetic(K):
    """Blocky label maps and a peaked soft-max that favours the label map shifted by two pixels."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(K)
    coarse = torch.randint(0, K, (N, H // 32, (W + 31) // 32), generator=g, device='cuda')
    labels = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].to(torch.uint8).contiguous()
    target = torch.roll(labels, 2, dims=2).long()
    logits = torch.randn(N, K, H, W, generator=g, device='cuda') * 2.0
    logits.scatter_add_(1, target.unsqueeze(1), torch.full((N, 1, H, W), 12.0, device='cuda'))
    return torch.softmax(logits, dim=1).clamp_(0.0, 1.0).contiguous(), labels


def real(K):
    """RMNet.forward (procedural weights, given flows) on a synthetic clip with K - 1 objects."""
    import torch
    from rmnet_amd import inference, networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.synthetic import synthetic_clip
    frames, masks, flows, _ = synthetic_clip(N, K, H, W, seed=3, size=2.1 if K == 3 else 0.8)
    net = networks.procedural_init_(RMNet(None)).cuda().eval()
    video = {'frames': frames[0], 'masks': masks[0], 'n_objects': K - 1}
    probs = inference.clip_probs(net, lambda clip: flows.cuda(), video).contiguous()
    labels = masks[0].argmax(dim=1).to(torch.uint8).cuda().contiguous()
    del net
    torch.cuda.empty_cache()
    return probs, labels


def measure(name, fn, calls):
    import torch
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print('  %-6s HIP events over %d calls back to back: %.3f ms per call;  synchronised calls: median %.3f ms (min %.3f, max %.3f);  '
          'peak memory above the inputs %.1f MB' % (name, calls, a.elapsed_time(b) / calls, 1e3 * statistics.median(times),
                                                    1e3 * min(times), 1e3 * max(times), peak / 1e6))
    return out


def kernel_split(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        rows = [(e.key, getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0), e.count) for e in prof.key_averages()]
        rows = [r for r in rows if r[1] > 0]
        for key, total, count in sorted(rows, key=lambda r: -r[1])[:6]:
            print('    kernel %-70s %.3f ms per call (%d launches)' % (key[:70], total / 1e3 / 10, count))
    except Exception as ex:                                       # the split is a nicety: the timings above stand without it
        print('    per-kernel split not measured: %s' % ex)


def step_clip(K, source):
    import torch
    from rmnet_amd import losses, ops
    assert torch.cuda.is_available(), 'this step needs a GPU'
    probs, labels = (synthetic if source == 'synth' else real)(K)
    torch.cuda.synchronize()
    print('%s probabilities, %d x %d x %d x %d, %d bins (inputs %.1f MB)' % (source, N, K, H, W, BINS, (probs.numel() * 4 + labels.numel()) / 1e6))
    hip = measure('hip', lambda: losses.validation_loss(probs, labels, bins=BINS, route='hip'), 20)
    kernel_split(lambda: ops.clip_loss(probs, labels, bins=BINS))
    tor = measure('torch', lambda: losses.validation_loss(probs, labels, bins=BINS, route='torch'), 5)
    lv = losses.lovasz_softmax(probs, labels, bins=BINS, route='hip')
    out = ops.clip_loss(probs, labels, bins=BINS, want_hist=True)
    hist = out['hist'].long()
    total, (lb, hb) = int(hist.sum()), lds_bins(K, BINS)
    ends, far = int(hist[:, :, 0].sum() + hist[:, :, BINS].sum()), int(hist[:, :, lb:BINS + 1 - hb].sum())
    print('  hip    loss %.9f = lovasz %.9f + nll %.9f;  widest class bracket %.3e;  n_bad %d' % (
        float(hip['loss']), float(hip['lovasz']), float(hip['nll']), float((lv['hi'] - lv['lo']).max()), int(hip['n_bad'])))
    print('  torch  loss %.9f = lovasz %.9f + nll %.9f;  hip - torch: lovasz %.3e, nll %.3e' % (
        float(tor['loss']), float(tor['lovasz']), float(tor['nll']), float(hip['lovasz'] - tor['lovasz']), float(hip['nll'] - tor['nll'])))
    print('  of %d (pixel, class) elements: %.2f %% had key 0 or %d (aggregated over the wave), %.2f %% another key in the %d lowest or '
          'the %d highest bins (LDS), %.2f %% went out as single global atomics'
          % (total, 100.0 * ends / total, BINS, 100.0 * (total - ends - far) / total, lb, hb, 100.0 * far / total))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step == 'resources':
        step_resources(None)
        return 0
    if args.step:
        step_clip(int(args.step[5:] if args.step.startswith('synth') else args.step[4:]), 'synth' if args.step.startswith('synth') else 'real')
        return 0
    for step, limit in STEPS:
        print('--- step %s' % step, flush=True)
        rc = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step]).returncode
        if rc != 0:
            print('step %s ended with status %d: stopping here' % (step, rc))
            return rc if rc > 0 else 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
