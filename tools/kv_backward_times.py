# -*- coding: utf-8 -*-
"""Forward + backward of the key / value heads (``kv_memory`` / ``kv_query``: 3x3 convolutions 1024 -> 128 and 1024 -> 512), two ways
on one GPU:

  ours     KeyValue after fuse_epilogues() / channels-last with device_grad_(): the regional forward (split_act +
           conv_split_region), then per head conv_grad_stage_rect + conv3x3_wgrad (csrc/conv_wgrad_n.hip) and the data gradient as
           two conv_split launches on flipped packs (ops.kv_dgrad);
  library  the same weights as a plain module under torch autograd with both convolutions on the library (RMNET_CONV=miopen, train
           mode): the only route there was before, and the yardstick.  It computes the dense heads; the cotangents are zero outside
           the rectangles, so both routes compute the same gradients.

Shapes: the reference's training batch (4 crops x 3 objects: the memory head sees 12 x 1024 x 30 x 30, the query head 4 x 1024 x 30 x
30) and one 480 x 854 frame with 3 objects (3 x 1024 x 30 x 54); one rectangle per image from a plausible box (about a third of the
map's width and half its height, shifted from image to image).  x requires grad (the encoder's r4), every head parameter is trained;
the loss is sum(key * ck) + sum(value * cv) with fixed random cotangents, the value head's 2^-12 times the key head's.  The two
routes alternate call by call, each call between two device events, 5 warm-up and 30 timed calls per route, once in the order ours,
library and once library, ours; median / min / max per order, and torch.cuda.max_memory_allocated above what the inputs and weights
take.  A second child per shape runs our route alone under `rocprofv3 --kernel-trace --stats` (a run of its own: no counters, no
other tracing) for the per-kernel times, split into stage / wgrad / bias / merge / dgrad; the packs are torch ops that run once per
weight version and are timed by events on their own.

    python tools/kv_backward_times.py [--out profiles/r38_a_kv_backward.md] [--no-trace]

The output replaces what lies between the two marker comments of the profile; the hand-written sections around them stay.

Every child runs under `timeout -k 10`; the driver stops at the first step that does not return 0: nothing is started on the GPU after
a step that failed there.
"""

import argparse
import copy
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('PYTORCH_MIOPEN_SUGGEST_NHWC', '1')

# step -> (images, h, w of r4)
SHAPES = {'train_memory': (12, 30, 30), 'train_query': (4, 30, 30), 'frame': (3, 30, 54)}
CIN, KEYDIM, VALDIM = 1024, 128, 512
WARMUP, CALLS, LIMIT = 5, 30, 420
F16_PEAK = 2.5e15            # dense f16 MFMA FLOP/s of an MI355X; the three-term arithmetic can reach a third of it
# trace rows: label -> kernel name (whole word)
KERNELS = (('stage', 'grad_stage_rect'), ('wgrad', 'conv_wgrad_n'), ('bias', 'bias_grad_n'), ('merge', 'merge_grad_n'),
           ('dgrad', 'conv_split'), ('forward', 'conv_split_region'))


def boxes(n, h, w):
    """One cell rectangle (cx0, cx1, cy0, cy1) per image: a third of the width, half the height, shifted from image to image."""
    bw, bh = max(1, w // 3), max(1, h // 2)
    return [((3 * i) % (w - bw), (3 * i) % (w - bw) + bw - 1, (2 * i) % (h - bh), (2 * i) % (h - bh) + bh - 1) for i in range(n)]


def make(step):
    import torch
    from rmnet_amd import networks
    n, h, w = SHAPES[step]
    d = torch.device('cuda', 0)
    plain = networks.procedural_init_(networks.KeyValue(CIN, KEYDIM, VALDIM)).to(d).to(memory_format=torch.channels_last)
    ours = copy.deepcopy(plain).eval()
    networks.fuse_epilogues_(ours)
    ours.device_grad_()
    gen = torch.Generator(device='cuda').manual_seed(n)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x = cl(torch.relu(torch.randn(n, CIN, h, w, generator=gen, device=d))).requires_grad_(True)
    rl = boxes(n, h, w)
    rects = torch.tensor(rl, dtype=torch.int32, device=d)
    mask = torch.zeros(n, 1, h, w, device=d)
    for i, (x0, x1, y0, y1) in enumerate(rl):
        mask[i, :, y0:y1 + 1, x0:x1 + 1] = 1.0
    ck = torch.randn(n, KEYDIM, h, w, generator=gen, device=d) * 1e-3 * mask
    cv = torch.randn(n, VALDIM, h, w, generator=gen, device=d) * (1e-3 * 2.0 ** -12) * mask

    def run(kv, conv, r):
        os.environ['RMNET_CONV'] = conv
        x.grad = None
        kv.zero_grad(set_to_none=True)
        key, val = kv(x, r)
        ((key * ck).sum() + (val * cv).sum()).backward()

    inside = sum((x1 - x0 + 1) * (y1 - y0 + 1) for x0, x1, y0, y1 in rl) / float(n * h * w)
    return (lambda: run(ours, 'split', rects)), (lambda: run(plain.train(), 'miopen', None)), ours, plain, x, inside


def timed(fns, order):
    import torch
    ms = {name: [] for name in order}
    for i in range(WARMUP + CALLS):
        for name in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fns[name]()
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[name].append(a.elapsed_time(b))
    return ms


def step_shape(step, trace_calls=0):
    import torch
    from rmnet_amd import ops
    assert torch.cuda.is_available(), 'this step needs a GPU'
    ours, library, kv_o, kv_l, x, inside = make(step)
    n, h, w = SHAPES[step]
    if trace_calls:
        ours()                                            # (the packs are made here, outside the counted calls' steady state)
        for _ in range(trace_calls):
            ours()
        torch.cuda.synchronize()
        return
    print('%s: %d x %d x %d x %d, %.0f %% of the cells inside the rectangles' % (step, n, CIN, h, w, 100 * inside))
    ours()
    ga = {k: p.grad.clone() for k, p in kv_o.named_parameters()}
    ga['x'] = x.grad.clone()
    library()
    gb = {k: p.grad.clone() for k, p in kv_l.named_parameters()}
    gb['x'] = x.grad.clone()
    worst, name = max((float((ga[k] - gb[k]).abs().max() / gb[k].abs().max()), k) for k in ga)
    l2, name2 = max((float((ga[k] - gb[k]).double().norm() / gb[k].double().norm()), k) for k in ga)
    print('  the two routes differ by at most %.2e of the largest gradient element (%s) and %.2e in relative L2 norm (%s), the largest over x '
          'and the 4 parameters; range words: forward %d, backward %d'
          % (worst, name, l2, name2, int(ops.conv_range_word(x.device)), int(ops.conv_grad_range_word(x.device))))
    del ga, gb
    fns = {'ours': ours, 'library': library}
    for order in (('ours', 'library'), ('library', 'ours')):
        ms = timed(fns, order)
        print('  order %s, %s:' % order)
        for name in ('ours', 'library'):
            v = ms[name]
            print('    forward + backward, %-8s median %.3f ms (min %.3f, max %.3f)' % (name + ':', statistics.median(v), min(v), max(v)))
        print('    ours / library (medians): %.2f' % (statistics.median(ms['ours']) / statistics.median(ms['library'])))
    for name in ('ours', 'library'):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fns[name]()
        torch.cuda.synchronize()
        print('  peak memory above inputs and weights, %-8s %.0f MB' % (name + ':', (torch.cuda.max_memory_allocated() - base) / 1e6))
    # the packs: once per weight version
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.conv_split_dgrad_pack(kv_o.key_conv.weight)
    torch.cuda.synchronize()
    a.record()
    ops.conv_split_dgrad_pack(kv_o.key_conv.weight)
    ops.conv_split_dgrad_pack(kv_o.value_conv.weight)
    ops.conv_split_pack(torch.cat((kv_o.key_conv.weight, kv_o.value_conv.weight)))
    b.record()
    torch.cuda.synchronize()
    print('  pack (torch ops; after an optimiser step only): the forward pack and the two dgrad packs %.3f ms' % a.elapsed_time(b))


def trace(step, lines):
    """Our route alone under rocprofv3 --kernel-trace --stats: per-kernel time per forward + backward."""
    calls = 4
    n, h, w = SHAPES[step]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['timeout', '-k', '10', str(LIMIT), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'kv', '--',
               sys.executable, os.path.abspath(__file__), '--step', step, '--trace-calls', str(calls)]
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
        if rc != 0:
            return rc
        files = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        if not files:
            lines.append('  (no kernel_stats.csv was written)')
            return 0
        rows = list(csv.DictReader(open(files[0])))
    if rows and not {'Name', 'Calls', 'TotalDurationNs'} <= set(rows[0]):
        lines.append('  (kernel_stats.csv has the columns %s: not the ones this script reads)' % sorted(rows[0]))
        return 0
    # (calls + 1 forward + backward passes ran in the child: the first one also made the packs)
    runs = calls + 1
    lines.append('  per kernel, one forward + backward of our route (`--kernel-trace --stats`, %d calls, a run of its own):' % runs)
    lines.append('')
    lines.append('  | part | kernel | launches per call | us per call | us per launch |')
    lines.append('  |---|---|---|---|---|')
    total, listed_us = 0.0, 0.0
    per = {}
    for r in rows:
        name = r.get('Name', '')
        us = float(r.get('TotalDurationNs', 0)) / 1e3 / runs
        total += us
        for label, k in KERNELS:
            if re.search(r'\b%s\b' % k, name):
                e = per.setdefault(label, [0.0, 0.0])
                e[0] += float(r.get('Calls', 0)) / runs
                e[1] += us
                listed_us += us
    for label, k in KERNELS:
        if label in per:
            lines.append('  | %s | %s | %.1f | %.1f | %.1f |' % (label, k, per[label][0], per[label][1], per[label][1] / max(per[label][0], 1e-9)))
    lines.append('  | every other kernel (the split of x, torch: amax reductions, reciprocals, the loss; the packs of the first call) | | | %.1f | |'
                 % (total - listed_us))
    lines.append('  | every kernel of the call | | | %.1f | |' % total)
    lines.append('')
    if 'wgrad' in per:
        lines.append('  (the two heads share the conv_wgrad_n row; per head: "wgrad by head" below)')
        flops = 2.0 * (KEYDIM + VALDIM) * 9 * CIN * n * h * w
        lines.append('  conv_wgrad_n, both heads: %.3f TFLOP of useful work per call in %.1f us = %.1f %% of the f16 matrix peak / 3'
                     % (flops / 1e12, per['wgrad'][1], 100 * flops / (per['wgrad'][1] * 1e-6) / (F16_PEAK / 3)))
    return 0


def wgrad_by_head(step):
    """Device-event times of ``ops.conv3x3_wgrad`` alone (GEMM + bias + merge) at Cout 128 and 512: the fraction of the f16 matrix
    peak / 3."""
    import torch
    from rmnet_amd import ops
    n, h, w = SHAPES[step]
    d = torch.device('cuda', 0)
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = torch.relu(torch.randn(n, CIN, h, w, generator=gen, device=d)).contiguous(memory_format=torch.channels_last)
    print('%s: ops.conv3x3_wgrad alone (GEMM, bias and merge launches), %d calls between two events' % (step, CALLS))
    for cout in (KEYDIM, VALDIM):
        g = torch.randn(n, cout, h, w, generator=gen, device=d).contiguous(memory_format=torch.channels_last)
        gs, sc = ops.conv_grad_stage_rect(g)
        ms = []
        for i in range(WARMUP + CALLS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.conv3x3_wgrad(x, gs, sc)
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        flops = 2.0 * cout * 9 * CIN * n * h * w
        med = statistics.median(ms)
        print('  Cout %3d: plan %s, median %.3f ms (min %.3f, max %.3f): %.3f TFLOP = %.1f %% of the f16 matrix peak / 3'
              % (cout, ops.conv3x3_wgrad_plan(n * h * w, CIN, cout), med, min(ms), max(ms), flops / 1e12, 100 * flops / (med * 1e-3) / (F16_PEAK / 3)))


def resources():
    """Registers and LDS of the new kernels from a compile-only build (metadata; no instruction is looked at)."""
    from rmnet_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'w.s')
        subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                        os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv_wgrad_n.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', text, flags=re.S).group(1)
    entries = ['    ' + e for e in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]]
    lines = []
    for name in ('conv_wgrad_n', 'bias_grad_n', 'merge_grad_n', 'grad_stage_rectILb0E', 'grad_stage_rectILb1E'):
        blk = [e for e in entries if re.search(r'^    \.name:\s+\S*\d+%sE' % name, e, flags=re.M)][0]
        get = lambda key: re.search(r'^    \.%s:\s+(\d+)' % key, blk, flags=re.M).group(1)
        lines.append('  %-22s VGPRs %s, SGPRs %s, static LDS %s B, scratch %s B, spilled VGPRs %s' % (
            name, get('vgpr_count'), get('sgpr_count'), get('group_segment_fixed_size'), get('private_segment_fixed_size'), get('vgpr_spill_count')))
    lines.append('  conv_wgrad_n asks for 69632 + 64 (512 + 2 (W + 1) + 1) B of dynamic LDS: 106432 B at W = 30, 109504 B at W = 54;')
    lines.append('  grad_stage_rect<planes> for 8320 B')
    return lines


BEGIN, END = '<!-- kv_backward_times.py: begin -->', '<!-- kv_backward_times.py: end -->'


def write_section(path, lines):
    """Replace what lies between the two markers of ``path`` (a new file gets a title and the markers): the sections written by hand
    around them stay."""
    body = '\n'.join([BEGIN, ''] + lines + [END])
    text = open(path).read() if os.path.exists(path) else ''
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + body + text[text.index(END) + len(END):]
    else:
        text = (text or '# Key / value heads, forward + backward: device gradients against the library route\n\n') + body + '\n'
    open(path, 'w').write(text)


def child(extra):
    return ['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__)] + extra


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=list(SHAPES))
    ap.add_argument('--trace-calls', type=int, default=0)
    ap.add_argument('--wgrad-alone', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r38_a_kv_backward.md'))
    ap.add_argument('--no-trace', action='store_true')
    args = ap.parse_args()
    if args.step:
        if args.wgrad_alone:
            wgrad_by_head(args.step)
        else:
            step_shape(args.step, args.trace_calls)
        return 0
    lines = []
    for step in SHAPES:
        print('--- step %s' % step, flush=True)
        p = subprocess.run(child(['--step', step]), stdout=subprocess.PIPE, text=True)
        print(p.stdout, flush=True)
        lines += ['```', p.stdout.rstrip(), '```', '']
        rc = p.returncode
        if rc == 0 and not args.no_trace:
            rc = trace(step, lines)
            lines.append('')
        if rc == 0:
            p = subprocess.run(child(['--step', step, '--wgrad-alone']), stdout=subprocess.PIPE, text=True)
            print(p.stdout, flush=True)
            lines += ['wgrad by head:', '', '```', p.stdout.rstrip(), '```', '']
            rc = p.returncode
        if rc != 0:
            print('step %s ended with status %d: stopping here' % (step, rc))
            lines.append('step %s ended with status %d: the run stopped here' % (step, rc))
            write_section(args.out, lines)
            return rc if rc > 0 else 1
    lines += ['### The new kernels, as compiled', ''] + ['```'] + resources() + ['```', '']
    write_section(args.out, lines)
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
