# -*- coding: utf-8 -*-
"""Forward + backward of the decoder, two ways on one GPU:

  ours     Decoder after fuse_epilogues() / channels-last with device_grad_(): the thirteen 256-output 3x3 convolutions on the
           split-fp16 kernels forward, conv_grad_stage + conv3x3_wgrad (csrc/conv3x3_wgrad.hip) + the forward kernel on flipped packs
           backward; upsamples and the prediction head are torch ops;
  library  the same weights as a plain module under torch autograd with every convolution on the library (RMNET_CONV=miopen, train
           mode): the only route there was before, and the yardstick.

Shapes: the reference's training batch (4 crops x 3 objects = 12 decoder inputs, 465 padded to 480: maps 30^2 / 60^2 / 120^2) and one
480 x 854 frame with 3 objects (maps 30 x 54 / 60 x 108 / 120 x 216).  r4 requires grad (the memory read's backward continues from
it), r3 / r2 come from a frozen encoder, every decoder parameter is trained; the loss is sum(out * g) with a fixed random g.  The two
routes alternate call by call, each call between two device events, 5 warm-up and 30 timed calls per route; median / min / max and
torch.cuda.max_memory_allocated above what the inputs and weights take.  A second child per shape runs our route alone under
`rocprofv3 --kernel-trace --stats` (a run of its own: no counters, no other tracing) for the per-kernel times.

    python tools/decoder_backward_times.py [--out profiles/r36_a_decoder_backward.md] [--no-trace]

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

# step -> (decoder inputs, h, w of r4)
SHAPES = {'train': (12, 30, 30), 'frame': (3, 30, 54)}
WARMUP, CALLS, LIMIT = 5, 30, 420
F16_PEAK = 2.5e15            # dense f16 MFMA FLOP/s of an MI355X; the three-term arithmetic can reach a third of it
CONVS = ((1024, 1), (256, 1), (256, 1), (512, 2), (256, 2), (256, 2), (256, 2), (256, 2), (256, 4), (256, 4), (256, 4), (256, 4), (256, 4))
KERNELS = ('conv3x3_wgrad', 'wgrad_merge', 'wgrad_bias', 'conv_grad_stage', 'conv3x3_rows', 'conv3x3_wreg')


def make(step):
    import torch
    from rmnet_amd import networks
    n, h, w = SHAPES[step]
    d = torch.device('cuda', 0)
    plain = networks.procedural_init_(networks.Decoder(256)).to(d).to(memory_format=torch.channels_last)
    ours = copy.deepcopy(plain).eval()
    networks.fuse_epilogues_(ours)
    ours.device_grad_()
    gen = torch.Generator(device='cuda').manual_seed(n)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    r4 = cl(torch.randn(n, 1024, h, w, generator=gen, device=d)).requires_grad_(True)
    r3 = cl(torch.randn(n, 512, 2 * h, 2 * w, generator=gen, device=d))
    r2 = cl(torch.randn(n, 256, 4 * h, 4 * w, generator=gen, device=d))
    g = torch.randn(n, 2, 16 * h, 16 * w, generator=gen, device=d) * 1e-6

    def run(dec, conv):
        os.environ['RMNET_CONV'] = conv
        r4.grad = None
        dec.zero_grad(set_to_none=True)
        (dec(r4, r3, r2) * g).sum().backward()

    return (lambda: run(ours, 'split')), (lambda: run(plain.train(), 'miopen')), ours, plain, r4


def step_shape(step, trace_calls=0):
    import torch
    from rmnet_amd import ops
    assert torch.cuda.is_available(), 'this step needs a GPU'
    ours, library, dec_o, dec_l, r4 = make(step)
    n, h, w = SHAPES[step]
    if trace_calls:
        for _ in range(trace_calls):
            ours()
        torch.cuda.synchronize()
        return
    print('%s: %d decoder inputs, maps %d x %d / %d x %d / %d x %d' % (step, n, h, w, 2 * h, 2 * w, 4 * h, 4 * w))
    ours()
    ga = {k: p.grad.clone() for k, p in dec_o.named_parameters()}
    ga['r4'] = r4.grad.clone()
    library()
    gb = {k: p.grad.clone() for k, p in dec_l.named_parameters()}
    gb['r4'] = r4.grad.clone()
    worst, name = max((float((ga[k] - gb[k]).abs().max() / gb[k].abs().max()), k) for k in ga)
    l2, name2 = max((float((ga[k] - gb[k]).double().norm() / gb[k].double().norm()), k) for k in ga)
    print('  the two routes differ by at most %.2e of the largest gradient element (%s) and %.2e in relative L2 norm (%s), the largest over r4 '
          'and the 28 parameters; range words: forward %d, backward %d'
          % (worst, name, l2, name2, int(ops.conv_range_word(r4.device)), int(ops.conv_grad_range_word(r4.device))))
    del ga, gb
    ms = {'ours': [], 'library': []}
    for i in range(WARMUP + CALLS):
        for name, fn in (('ours', ours), ('library', library)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[name].append(a.elapsed_time(b))
    for name, fn in (('ours', ours), ('library', library)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        v = ms[name]
        print('  forward + backward, %-8s median %.3f ms (min %.3f, max %.3f); peak memory above inputs and weights %.0f MB'
              % (name + ':', statistics.median(v), min(v), max(v), (torch.cuda.max_memory_allocated() - base) / 1e6))
    print('  ours / library (medians): %.2f' % (statistics.median(ms['ours']) / statistics.median(ms['library'])))


def trace(step, lines):
    """Our route alone under rocprofv3 --kernel-trace --stats: per-kernel time per forward + backward."""
    calls = 4
    n, h, w = SHAPES[step]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['timeout', '-k', '10', str(LIMIT), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'dec', '--',
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
    lines.append('  per kernel, one forward + backward of our route (`--kernel-trace --stats`, %d calls, a run of its own):' % calls)
    lines.append('')
    lines.append('  | kernel | launches per call | us per call | us per launch |')
    lines.append('  |---|---|---|---|')
    total = 0.0
    per = {}
    for r in rows:
        name = r.get('Name', '')
        us = float(r.get('TotalDurationNs', 0)) / 1e3 / calls
        total += us
        for k in KERNELS:
            if re.search(r'\b%s\b' % k, name) or (k + '(') in name or ('::' + k) in name:
                e = per.setdefault(k, [0.0, 0.0])
                e[0] += float(r.get('Calls', 0)) / calls
                e[1] += us
    for k in KERNELS:
        if k in per:
            lines.append('  | %s | %.1f | %.1f | %.1f |' % (k, per[k][0], per[k][1], per[k][1] / max(per[k][0], 1e-9)))
    lines.append('  | every kernel of the call | | %.1f | |' % total)
    lines.append('')
    lines.append('  (conv3x3_rows / conv3x3_wreg rows hold the forward launches AND the data-gradient launches: the same kernels.)')
    if 'conv3x3_wgrad' in per:
        flops = sum(2.0 * 256 * 9 * cin * n * h * w * s * s for cin, s in CONVS)
        lines.append('  conv3x3_wgrad: %.2f TFLOP of useful work per call in %.1f us = %.1f %% of the f16 matrix peak / 3'
                     % (flops / 1e12, per['conv3x3_wgrad'][1], 100 * flops / (per['conv3x3_wgrad'][1] * 1e-6) / (F16_PEAK / 3)))
    return 0


def resources():
    """Registers and LDS of the new kernels from a compile-only build (metadata; no instruction is looked at)."""
    from rmnet_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'w.s')
        subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                        os.path.join(ROOT, 'rmnet_amd', 'csrc', 'conv3x3_wgrad.hip'), '-o', out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', text, flags=re.S).group(1)
    entries = ['    ' + e for e in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]]
    lines = []
    for name in ('conv3x3_wgrad', 'wgrad_bias', 'wgrad_merge', 'conv_grad_stage'):
        blk = [e for e in entries if re.search(r'^    \.name:\s+\S*\d+%sE' % name, e, flags=re.M)][0]
        get = lambda key: re.search(r'^    \.%s:\s+(\d+)' % key, blk, flags=re.M).group(1)
        lines.append('  %-16s VGPRs %s, SGPRs %s, static LDS %s B, scratch %s B, spilled VGPRs %s' % (
            name, get('vgpr_count'), get('sgpr_count'), get('group_segment_fixed_size'), get('private_segment_fixed_size'), get('vgpr_spill_count')))
    lines.append('  conv3x3_wgrad asks for 69632 + 64 (512 + 2 (W + 1) + 1) B of dynamic LDS: 101504 B at W = 120, 113536 B at W = 216')
    return lines


BEGIN, END = '<!-- decoder_backward_times.py: begin -->', '<!-- decoder_backward_times.py: end -->'


def write_section(path, lines):
    """Replace what lies between the two markers of ``path`` (a new file gets a title and the markers): the sections written by hand
    around them -- design notes, the module test's error values, the bench lines -- stay."""
    body = '\n'.join([BEGIN, ''] + lines + [END])
    text = open(path).read() if os.path.exists(path) else ''
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + body + text[text.index(END) + len(END):]
    else:
        text = (text or '# Decoder forward + backward: device gradients against the library route\n\n') + body + '\n'
    open(path, 'w').write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=list(SHAPES))
    ap.add_argument('--trace-calls', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r36_a_decoder_backward.md'))
    ap.add_argument('--no-trace', action='store_true')
    args = ap.parse_args()
    if args.step:
        step_shape(args.step, args.trace_calls)
        return 0
    lines = []
    for step in SHAPES:
        print('--- step %s' % step, flush=True)
        p = subprocess.run(['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__), '--step', step], stdout=subprocess.PIPE, text=True)
        print(p.stdout, flush=True)
        lines += ['```', p.stdout.rstrip(), '```', '']
        rc = p.returncode
        if rc == 0 and not args.no_trace:
            rc = trace(step, lines)
            lines.append('')
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
