# -*- coding: utf-8 -*-
"""The four clip I/O entries (csrc/clip_io.hip) on one 70-frame 854 x 480 clip with K = 11, on the GPU and on the host of the same
machine:

  (a) each entry alone between two device events: 5 warm-up calls, then the median of 30 calls, with the bytes the entry has to
      move (inputs read once + outputs written once, from the shapes) over that time and against the 6.3 TB/s that a float4 copy
      reaches on an MI355X (8 TB/s on paper);
  (b) for the argmax, ``prob.argmax(1).to(torch.uint8)`` on the device, the two dispatches that inference.segment_video uses;
  (c) the numpy restatement tests/clip_io_ref.py on the host, one thread, on the first frames of the clip, per frame.

The GPU results of those first frames must equal the restatement's byte for byte.

    python tools/clip_io_bench.py            # every step in a child process of its own, under a time limit

The driver stops at the first step that does not return 0: nothing is started on the GPU after a step that failed there.
"""

import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, K, H, W = 70, 11, 480, 854
HOST_FRAMES = 4                      # frames of the clip that the host restatement runs (and that are compared)
HBM_COPY_TBS = 6.3                   # what a float4 copy reaches on an MI355X (8 TB/s on paper)
STEPS = (('gpu', 420), ('cpu', 600))      # (step, time limit in seconds)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def clip():
    """uint8 frames [N,H,W,3] of seeded noise over a gradient, label maps [N,H,W] with ten ellipses (ids 1 .. 10) that drift over
    the clip, and probabilities [N,K,H,W] float32 whose maximum is the label's plane, with ties elsewhere."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = (rng.integers(0, 64, (N, H, W, 3)) + (xx[None, :, :, None] * 191 // W)).astype(np.uint8)
    labels = np.zeros((N, H, W), dtype=np.uint8)
    c = rng.uniform(0.15, 0.85, (K - 1, 2)) * (H, W)
    v = rng.uniform(-1.5, 1.5, (K - 1, 2))
    a = rng.uniform(0.05, 0.15, (K - 1, 2)) * (H, W)
    for n in range(N):
        for k in range(K - 1):
            cy, cx = c[k] + n * v[k]
            labels[n][((yy - cy) / a[k][0]) ** 2 + ((xx - cx) / a[k][1]) ** 2 <= 1] = k + 1
    return frames, labels


def probabilities(labels, torch, dev):
    lab = torch.from_numpy(labels).to(dev)
    prob = torch.full((N, K, H, W), 0.05, device=dev)
    prob.scatter_(1, lab.long().unsqueeze(1), 0.5)
    return prob


def _median_ms(torch, fn, warm=5, calls=30):
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


def step_gpu(workdir):
    import torch
    from rmnet_amd import clip_io, ops
    assert torch.cuda.is_available(), 'the GPU step needs a GPU'
    dev = torch.device('cuda', 0)
    frames_np, labels_np = clip()
    u8, labels = torch.from_numpy(frames_np).to(dev), torch.from_numpy(labels_np).to(dev)
    prob = probabilities(labels_np, torch, dev)
    lut, n_ids = clip_io.reorganize_lut(labels)
    frames = ops.frames_normalize(u8, MEAN, STD)
    px = N * H * W
    rows = (('rmnet_frames_normalize_u8', lambda: ops.frames_normalize(u8, MEAN, STD), px * (3 + 12)),
            ('rmnet_labels_onehot_u8 (K = %d, table)' % K, lambda: ops.labels_onehot(labels, K, lut), px * (1 + K)),
            ('rmnet_argmax_labels_f32 (K = %d)' % K, lambda: ops.argmax_labels(prob), px * (4 * K + 1)),
            ('  torch: prob.argmax(1).to(uint8)', lambda: prob.argmax(1).to(torch.uint8), px * (4 * K + 1)),
            ('rmnet_overlay_u8 (three launches)', lambda: ops.overlay(frames, labels, MEAN, STD), px * (12 + 1 + 3)),
            ('  clip_io.reorganize_lut (torch ops)', lambda: clip_io.reorganize_lut(labels), px))
    print('%d frames of %d x %d, K = %d, %d ids in the label maps; median of 30 calls between device events (10 %% .. 90 %%)' % (N, W, H, K, int(n_ids)))
    print('| entry | ms per call | 10 %% .. 90 %% | MB moved | TB/s | share of %.1f TB/s |' % HBM_COPY_TBS)
    print('|---|---|---|---|---|---|')
    for name, fn, nbytes in rows:
        med, lo, hi = _median_ms(torch, fn)
        tbs = nbytes / (med * 1e-3) / 1e12
        print('| %s | %.3f | %.3f .. %.3f | %.0f | %.2f | %.0f %% |' % (name, med, lo, hi, nbytes / 1e6, tbs, 100 * tbs / HBM_COPY_TBS))
    assert torch.equal(ops.argmax_labels(prob), prob.argmax(1).to(torch.uint8)), 'the argmax kernel differs from torch.argmax'
    h = HOST_FRAMES
    np.savez(os.path.join(workdir, 'gpu.npz'), normalized=frames[:h].cpu().numpy(), onehot=ops.labels_onehot(labels[:h], K, lut).cpu().numpy(),
             argmax=ops.argmax_labels(prob[:h].contiguous()).cpu().numpy(), overlay=ops.overlay(frames[:h].contiguous(), labels[:h], MEAN, STD).cpu().numpy(),
             prob=prob[:h].cpu().numpy(), lut=lut.cpu().numpy())
    torch.cuda.synchronize()


def step_cpu(workdir):
    import clip_io_ref as ref
    frames_np, labels_np = clip()
    h = HOST_FRAMES
    u8, labels = frames_np[:h], labels_np[:h]
    path = os.path.join(workdir, 'gpu.npz')
    gpu = np.load(path) if os.path.exists(path) else None
    lut, _ = ref.reorganize_lut(labels_np)
    t = [time.perf_counter()]
    normalized = ref.normalize(u8, MEAN, STD)
    t.append(time.perf_counter())
    onehot = ref.onehot(labels, K, lut)
    t.append(time.perf_counter())
    over = ref.overlay(normalized, labels, MEAN, STD)
    t.append(time.perf_counter())
    print('numpy restatement on the host, one thread, %d frames, ms per frame: normalize %.1f, one-hot %.1f, overlay %.1f'
          % (h, *(1e3 * (t[i + 1] - t[i]) / h for i in range(3))))
    if gpu is None:
        print('no GPU results to compare with')
        return
    t0 = time.perf_counter()
    am = ref.argmax_first(gpu['prob'])
    print('                                                              argmax (K = %d) %.1f' % (K, 1e3 * (time.perf_counter() - t0) / h))
    assert np.array_equal(lut, gpu['lut'])
    assert np.array_equal(normalized.view(np.int32), gpu['normalized'].view(np.int32)) and np.array_equal(onehot, gpu['onehot'])
    assert np.array_equal(am, gpu['argmax']) and np.array_equal(over, gpu['overlay'])
    print('GPU results == restatement on those frames, byte for byte: normalized frames, one-hot masks, label maps, overlays')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=[s for s, _ in STEPS])
    ap.add_argument('--dir')
    args = ap.parse_args()
    if args.step:
        {'gpu': step_gpu, 'cpu': step_cpu}[args.step](args.dir)
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
