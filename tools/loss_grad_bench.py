# -*- coding: utf-8 -*-
"""The training loss (Lovasz-softmax + NLL, core/train.py:180), value and gradient with respect to the probabilities, two ways on
one GPU:

  hip    losses.training_loss(route='hip') + backward(): ops.clip_loss_grad (csrc/val_loss_bwd.hip: the histogram pass of the
         validation loss, one scan that also writes the two weight tables, one streaming pass that writes the gradient);
  torch  losses.training_loss(route='torch') + backward(): torch autograd through the sort (the reference's formulation: a permuted
         copy, a sort of all pixels per class, two cumsums, an index-scatter backward).  The yardstick, never the code under test.

Cases: the 70-frame 480 x 854 clip of tools/val_loss_bench.py with K = 3 and K = 11, synthetic peaked soft-maxes ('synth') and the
saturated output of RMNet.forward with procedural weights ('real'); and a training batch of the reference's config.py TRAIN section
('train': BATCH_SIZE 4 x N_MAX_FRAMES 3 frames of CROP 465 x 465, N_MAX_OBJECTS 3 + background = 4 classes).  Each at 2^20 and at
2^12 bins.  For each: HIP events around calls issued back to back, the median / min / max wall time of calls that each sit between
two stream synchronisations, torch.cuda.max_memory_allocated above what the inputs take, and the per-kernel split of
torch.profiler when it gives one.

vl_grad_apply's table gather is measured both ways in the same process, alternating: the library as built (RMNET_VL_GRAD_STAGE 1:
the lowest and highest table entries of every class staged in LDS) against a variant built with -DRMNET_VL_GRAD_STAGE=0 (plain
cached gathers), the C entry alone on preallocated buffers.

    python tools/loss_grad_bench.py --step variant     # where hipcc is: builds build/variants/librmnet_hip_plain_gather.so (no GPU)
    python tools/loss_grad_bench.py                    # every GPU step in a child process of its own, under `timeout -k 10`

The driver stops at the first step that does not return 0: nothing is started on the GPU after a step that failed there.
"""

import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import val_loss_bench as vb  # noqa: E402

VARIANT = os.path.join(ROOT, 'build', 'variants', 'librmnet_hip_plain_gather.so')
BINS = (1 << 20, 1 << 12)
# (step, time limit in seconds)
STEPS = (('resources', 300), ('train4', 300), ('synth3', 420), ('synth11', 600), ('real3', 600), ('real11', 780))


def step_variant():
    from rmnet_amd import build
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    cmd = [build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '-shared', '-fPIC', '-DRMNET_VL_GRAD_STAGE=0',
           '-o', VARIANT] + [os.path.join(build.CSRC, s) for s in build.SOURCES]
    subprocess.check_call(cmd, cwd=build.CSRC)
    print('built', VARIANT)


def step_resources():
    vb.step_resources(None)                                                   # val_loss.hip, as before
    import re
    import tempfile
    from rmnet_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'val_loss_bwd.s')
        subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                        os.path.join(build.CSRC, 'val_loss_bwd.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', asm, flags=re.S).group(1)
    for entry in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]:
        if '.vgpr_count:' not in entry:
            continue
        get = lambda key: re.search(r'^\s*\.%s:\s+(\S+)' % key, entry, flags=re.M).group(1)
        print('%-60s VGPRs %s (spilled %s)  SGPRs %s  scratch %s B  static LDS %s B' % (
            get('name'), get('vgpr_count'), get('vgpr_spill_count'), get('sgpr_count'), get('private_segment_fixed_size'),
            get('group_segment_fixed_size')))


def train_batch(K):
    """BATCH_SIZE x N_MAX_FRAMES frames of CROP_HSIZE x CROP_WSIZE as one [N, K, H, W] clip (the loss flattens them alike)."""
    import torch
    N, H, W = 4 * 3, 465, 465
    g = torch.Generator(device='cuda').manual_seed(K)
    coarse = torch.randint(0, K, (N, (H + 31) // 32, (W + 31) // 32), generator=g, device='cuda')
    labels = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].to(torch.uint8).contiguous()
    labels[:, :7] = 255                                                       # the fill colour of the augmentation's affine warp
    target = torch.roll(labels, 2, dims=2).clamp(max=K - 1).long()
    logits = torch.randn(N, K, H, W, generator=g, device='cuda') * 2.0
    logits.scatter_add_(1, target.unsqueeze(1), torch.full((N, 1, H, W), 6.0, device='cuda'))
    return torch.softmax(logits, dim=1).clamp_(0.0, 1.0).contiguous(), labels


class Buffers:
    """The outputs and the workspace of rmnet_clip_loss_grad_f32, allocated once: the variants write the same addresses."""

    def __init__(self, probs, bins):
        import torch
        from rmnet_amd import _lib
        K, dev = probs.shape[1], probs.device
        self.grad = torch.empty_like(probs)
        self.per_class = torch.empty(K, 3, dtype=torch.float64, device=dev)
        self.nll = torch.empty((), dtype=torch.float64, device=dev)
        self.counts = torch.empty(3, dtype=torch.int64, device=dev)
        self.ws = torch.empty(_lib.load().rmnet_clip_loss_grad_workspace_bytes(K, bins), dtype=torch.uint8, device=dev)


class Entry:
    """rmnet_clip_loss_grad_f32 of one library on the shared buffers."""

    def __init__(self, path, probs, labels, bins, buf):
        from rmnet_amd import _lib
        self.lib = ctypes.CDLL(path)
        fn = self.lib.rmnet_clip_loss_grad_f32
        fn.restype, fn.argtypes = _lib.SIGNATURES['rmnet_clip_loss_grad_f32']
        N, K, H, W = probs.shape
        self.buf = buf
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        self.args = (p(probs), p(labels), N, K, H, W, 255, bins, p(buf.grad), p(buf.per_class), p(buf.nll), p(buf.counts), p(buf.ws),
                     buf.ws.numel())

    def __call__(self):
        import torch
        rc = self.lib.rmnet_clip_loss_grad_f32(*self.args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc


def alternate(entries, rounds=7, calls=10):
    """{name: [ms per call of every round]}: the variants take turns, `calls` calls back to back between two HIP events."""
    import torch
    for e in entries.values():
        e()
    torch.cuda.synchronize()
    out = {k: [] for k in entries}
    for _ in range(rounds):
        for name, e in entries.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                e()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / calls)
    return out


def step_clip(step):
    import torch
    from rmnet_amd import _lib, losses, ops
    assert torch.cuda.is_available(), 'this step needs a GPU'
    source = step.rstrip('0123456789')
    K = int(step[len(source):])
    probs, labels = {'synth': vb.synthetic, 'real': vb.real, 'train': train_batch}[source](K)
    torch.cuda.synchronize()
    print('%s probabilities, %s (inputs %.1f MB; the gradient alone %.1f MB)' % (source, ' x '.join(str(s) for s in probs.shape),
                                                                                (probs.numel() * 4 + labels.numel()) / 1e6, probs.numel() * 4 / 1e6))
    leaf = probs.clone().requires_grad_(True)

    def both(route, bins):
        leaf.grad = None
        loss = losses.training_loss(leaf, labels, bins=bins, route=route)
        loss.backward()
        return loss.detach(), leaf.grad

    for bins in BINS:
        print(' bins %d' % bins)
        hip = vb.measure('hip', lambda: both('hip', bins), 20)
        vb.kernel_split(lambda: ops.clip_loss_grad(probs, labels, bins=bins))
        tor = vb.measure('torch', lambda: both('torch', bins), 5)
        fwd = vb.measure('value', lambda: ops.clip_loss(probs, labels, bins=bins), 20)
        del fwd
        d = (hip[1].double() - tor[1].double()).abs()
        fin = torch.isfinite(d)
        print('  loss hip %.9f torch %.9f;  |grad hip - grad torch|: max %.3e, mean %.3e over %d finite elements (%d not finite in both)'
              % (float(hip[0]), float(tor[0]), float(d[fin].max()), float(d[fin].mean()), int(fin.sum()), int((~fin).sum())))
        del hip, tor, d, fin
        leaf.grad = None
        torch.cuda.empty_cache()
        buf = Buffers(probs, bins)
        entries = {'staged': Entry(_lib.LIB_PATH, probs, labels, bins, buf)}
        if os.path.exists(VARIANT):
            entries['plain'] = Entry(VARIANT, probs, labels, bins, buf)
        else:
            print('  (no %s: the plain-gather variant is not measured)' % os.path.relpath(VARIANT, ROOT))
        for name, ms in alternate(entries).items():
            print('  entry alone, %-6s gather: median %.3f ms per call over %d alternating rounds of 10 calls (min %.3f, max %.3f)'
                  % (name, statistics.median(ms), len(ms), min(ms), max(ms)))
        if 'plain' in entries:
            entries['staged']()
            staged = buf.grad.view(torch.int32).clone()
            entries['plain']()
            assert torch.equal(staged, buf.grad.view(torch.int32)), 'the variants differ'
            del staged
            print('    per-kernel split of the plain-gather variant:')
            vb.kernel_split(entries['plain'])
        del entries, buf
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=['variant'] + [s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step == 'variant':
        step_variant()
        return 0
    if args.step == 'resources':
        step_resources()
        return 0
    if args.step:
        step_clip(args.step)
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
