# -*- coding: utf-8 -*-
"""Boundary measure F of one synthetic clip (70 frames, 3 objects, 480 x 854, radius 8 by the 0.008 rule), three ways on one machine:

  (a) metrics.boundary_f_per_object on uint8 maps on the GPU (csrc/boundary_f.hip + the float64 epilogue): median wall time of
      repeated calls, each between two stream synchronisations, after warm-up; and ops.boundary_match alone by HIP events;
  (b) the torch restatement of rmnet_amd.metrics on CPU tensors;
  (c) numpy boundary maps + scipy.ndimage.binary_dilation per frame and object, which is what the reference's
      skimage.morphology.binary_dilation calls (utils/metrics.py:141-144) -- when scipy imports.

All three must return the same counts.  Also prints VGPRs, scratch and LDS of the two kernels from the compiler's metadata.

    python tools/boundary_f_bench.py            # every step in a child process of its own, under a time limit

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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, K, H, W = 70, 3, 480, 854
STEPS = (('resources', 300), ('gpu', 300), ('cpu', 900))      # (step, time limit in seconds)


def clip():
    """gt: three filled ellipses that drift and breathe over the clip; pred: gt rolled by (1, 2) with 1 % of the pixels cleared."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((N, H, W), dtype=np.uint8)
    c = rng.uniform(0.25, 0.75, (K, 2)) * (H, W)
    v = rng.uniform(-2.0, 2.0, (K, 2))
    a = rng.uniform(0.08, 0.25, (K, 2)) * (H, W)
    for n in range(N):
        for k in range(K):
            cy, cx = c[k] + n * v[k]
            ay, ax = a[k] * (1 + 0.2 * np.sin(0.2 * n + k))
            gt[n][((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1] = k + 1
    pred = np.roll(gt, (1, 2), axis=(1, 2)).copy()
    pred[rng.random(pred.shape) < 0.01] = 0
    return pred, gt


def step_resources(_):
    from rmnet_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'boundary_f.s')
        subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                        os.path.join(build.CSRC, 'boundary_f.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', asm, flags=re.S).group(1)
    for entry in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]:
        if '.vgpr_count:' not in entry:          # (the metadata's version list follows the kernels)
            continue
        get = lambda key: re.search(r'^\s*\.%s:\s+(\S+)' % key, entry, flags=re.M).group(1)
        print('%-48s VGPRs %s (spilled %s)  SGPRs %s  scratch %s B  LDS %s B' % (
            get('name'), get('vgpr_count'), get('vgpr_spill_count'), get('sgpr_count'), get('private_segment_fixed_size'),
            get('group_segment_fixed_size')))


def step_gpu(workdir):
    import torch
    from rmnet_amd import metrics, ops
    assert torch.cuda.is_available(), 'the GPU step needs a GPU'
    pred, gt = (torch.from_numpy(a).cuda() for a in clip())
    radius = metrics.boundary_radius(H, W)
    counts = ops.boundary_match(pred, gt, K, radius)
    np.save(os.path.join(workdir, 'counts_gpu.npy'), counts.cpu().numpy())
    for _ in range(5):
        metrics.boundary_f_per_object(pred, gt, K)
    torch.cuda.synchronize()
    times = []
    for _ in range(50):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = metrics.boundary_f_per_object(pred, gt, K)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(50):
        ops.boundary_match(pred, gt, K, radius)
    b.record()
    torch.cuda.synchronize()
    q = statistics.quantiles(times, n=10)
    print('(a) GPU  metrics.boundary_f_per_object, %d x %d x %dx%d, radius %d: median %.3f ms (10 %% .. 90 %%: %.3f .. %.3f, 50 calls)'
          % (N, K, H, W, radius, 1e3 * statistics.median(times), 1e3 * q[0], 1e3 * q[-1]))
    print('    GPU  ops.boundary_match alone, HIP events over 50 calls back to back: %.3f ms per call' % (a.elapsed_time(b) / 50))
    print('    mean F of the clip %.6f' % float(f.mean()))


def step_cpu(workdir):
    import torch
    from rmnet_amd import metrics
    pred, gt = clip()
    radius = metrics.boundary_radius(H, W)
    tp, tg = torch.from_numpy(pred), torch.from_numpy(gt)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        counts = metrics.boundary_counts(tp, tg, K, radius)
        f = metrics.f_from_counts(counts)
        times.append(time.perf_counter() - t0)
    print('(b) CPU  torch restatement (%d threads): median %.1f ms of 3 calls (%s)'
          % (torch.get_num_threads(), 1e3 * statistics.median(times), ', '.join('%.1f' % (1e3 * t) for t in times)))
    counts = counts.numpy()
    path = os.path.join(workdir, 'counts_gpu.npy')
    if os.path.exists(path):
        assert (np.load(path) == counts).all(), 'the GPU counts differ from the torch restatement on the CPU'
        print('    GPU counts == CPU counts, all %d integers' % counts.size)
    try:
        import scipy.ndimage as ndi
    except ImportError:
        print('(c) scipy does not import: not measured')
        return
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import boundary_ref as br
    foot = br.disk(radius)
    t0 = time.perf_counter()
    ref = np.zeros((N, K, 4), dtype=np.int64)
    for n in range(N):
        for k in range(1, K + 1):
            fb, gb = br.seg2bmap(pred[n] == k), br.seg2bmap(gt[n] == k)
            fd, gd = ndi.binary_dilation(fb, structure=foot), ndi.binary_dilation(gb, structure=foot)
            ref[n, k - 1] = fb.sum(), gb.sum(), (fb & gd).sum(), (gb & fd).sum()
    fs = br.f_of_counts(ref)
    t1 = time.perf_counter()
    print('(c) CPU  numpy + scipy.ndimage.binary_dilation per frame and object, one thread: %.1f ms, one pass' % (1e3 * (t1 - t0)))
    assert (ref == counts).all(), 'the scipy statement differs from the torch restatement'
    assert (fs.view(np.int64) == f.numpy().view(np.int64)).all()
    print('    scipy counts == torch counts, F bit for bit; mean F %.6f' % fs.mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=[s for s, _ in STEPS])
    ap.add_argument('--dir')
    args = ap.parse_args()
    if args.step:
        {'resources': step_resources, 'gpu': step_gpu, 'cpu': step_cpu}[args.step](args.dir)
        return 0
    with tempfile.TemporaryDirectory() as workdir:
        for step, limit in STEPS:
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--dir', workdir], timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('step %s ended with status %d: stopping here' % (step, rc))
                return rc if rc > 0 else 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
