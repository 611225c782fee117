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

`--glue on` measures `device_grad_(glue=True)` instead: the two routes that alternate are then our route as above ("glue off") and the
same decoder with the x2 upsample + add, the prediction head and the x4 upsample as recorded ops with the backward kernels of
csrc/decoder_glue_bwd.hip ("glue on"); both are traced, each in a run of its own, with the kernels outside the table's list by name,
and the streaming kernels' GB/s against their algorithmic bytes.  It writes to profiles/r37_a_decoder_glue_backward.md unless --out
says otherwise.

    python tools/decoder_backward_times.py --glue on [--out FILE] [--no-trace]

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
GLUE_KERNELS = ('upsample2x_add_nhwc', 'upsample_bwd_nhwc', 'pred_head', 'pred_head_bwd', 'pred_head_bwd_merge', 'upsample_bwd_nchw')
OTHERS_SHOWN = 14            # --glue on: that many of the kernels outside the lists, by time


def make(step, glue=False):
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

    if glue:                     # the same weights with the glue as recorded ops, in place of the library route
        plain = copy.deepcopy(ours).device_grad_(glue=True)
        return (lambda: run(ours, 'split')), (lambda: run(plain, 'split')), ours, plain, r4
    return (lambda: run(ours, 'split')), (lambda: run(plain.train(), 'miopen')), ours, plain, r4


def step_shape(step, trace_calls=0, glue=False, trace_second=False):
    import torch
    from rmnet_amd import ops
    assert torch.cuda.is_available(), 'this step needs a GPU'
    ours, library, dec_o, dec_l, r4 = make(step, glue)
    first, second = ('glue off', 'glue on') if glue else ('ours', 'library')
    n, h, w = SHAPES[step]
    if trace_calls:
        for _ in range(trace_calls):
            (library if trace_second else ours)()
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
    ms = {first: [], second: []}
    for i in range(WARMUP + CALLS):
        for name, fn in ((first, ours), (second, library)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[name].append(a.elapsed_time(b))
    for name, fn in ((first, ours), (second, library)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        v = ms[name]
        print('  forward + backward, %-8s median %.3f ms (min %.3f, max %.3f); peak memory above inputs and weights %.0f MB'
              % (name + ':', statistics.median(v), min(v), max(v), (torch.cuda.max_memory_allocated() - base) / 1e6))
    print('  %s / %s (medians): %.2f' % (first, second, statistics.median(ms[first]) / statistics.median(ms[second])))
    if glue:
        print('  every "glue on" call is faster than every "glue off" call: %s (slowest on %.3f ms, fastest off %.3f ms)'
              % (max(ms[second]) < min(ms[first]), max(ms[second]), min(ms[first])))


def trace(step, lines, glue=None):
    """Our route alone under rocprofv3 --kernel-trace --stats: per-kernel time per forward + backward.  ``glue``: 'off' / 'on', the
    route of a --glue on run."""
    calls = 4
    n, h, w = SHAPES[step]
    kernels = KERNELS + (GLUE_KERNELS if glue else ())
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['timeout', '-k', '10', str(LIMIT), 'rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'dec', '--',
               sys.executable, os.path.abspath(__file__), '--step', step, '--trace-calls', str(calls)]
        if glue:
            cmd += ['--glue', 'on'] + (['--trace-second'] if glue == 'on' else [])
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
    lines.append('  per kernel, one forward + backward of our route%s (`--kernel-trace --stats`, %d calls, a run of its own):'
                 % (' with glue ' + glue if glue else '', calls))
    lines.append('')
    lines.append('  | kernel | launches per call | us per call | us per launch |')
    lines.append('  |---|---|---|---|')
    total = 0.0
    per = {}
    others = []
    for r in rows:
        name = r.get('Name', '')
        us = float(r.get('TotalDurationNs', 0)) / 1e3 / calls
        total += us
        listed = False
        for k in kernels:
            # (the glue kernels' names are prefixes of one another: pred_head, pred_head_bwd, pred_head_bwd_merge -- whole words only)
            if re.search(r'\b%s\b' % k, name) or (k not in GLUE_KERNELS and ((k + '(') in name or ('::' + k) in name)):
                e = per.setdefault(k, [0.0, 0.0])
                e[0] += float(r.get('Calls', 0)) / calls
                e[1] += us
                listed = True
        if not listed:
            others.append((us, float(r.get('Calls', 0)) / calls, name))
    for k in kernels:
        if k in per:
            lines.append('  | %s | %.1f | %.1f | %.1f |' % (k, per[k][0], per[k][1], per[k][1] / max(per[k][0], 1e-9)))
    if glue:
        for us, cnt, name in sorted(others, reverse=True)[:OTHERS_SHOWN]:
            short = re.sub(r'\s+', ' ', name)
            lines.append('  | `%s` | %.1f | %.1f | %.1f |' % (short if len(short) <= 90 else short[:87] + '...', cnt, us, us / max(cnt, 1e-9)))
        rest = sorted(others, reverse=True)[OTHERS_SHOWN:]
        lines.append('  | %d more kernels | %.1f | %.1f | |' % (len(rest), sum(o[1] for o in rest), sum(o[0] for o in rest)))
    lines.append('  | every kernel of the call | | %.1f | |' % total)
    lines.append('')
    lines.append('  (conv3x3_rows / conv3x3_wreg rows hold the forward launches AND the data-gradient launches: the same kernels.)')
    if glue == 'on':
        # algorithmic bytes: the adjoint reads the fine gradient and writes the coarse one, 5 floats per coarse element (RF3's coarse map
        # is h x w, RF2's 2h x 2w; 256 channels); the head's backward reads x and g and writes dx (the partials are 18 KB per range)
        up = 4.0 * n * 256 * (h * w + 4 * h * w) * 5
        head = 4.0 * n * 16 * h * w * (2 * 256 + 2)
        for k, nbytes in (('upsample_bwd_nhwc', up), ('pred_head_bwd', head)):
            if k in per:
                lines.append('  %s: %.1f MB of algorithmic traffic per call in %.1f us = %.0f GB/s' % (k, nbytes / 1e6, per[k][1], nbytes / per[k][1] / 1e3))
    if 'conv3x3_wgrad' in per:
        flops = sum(2.0 * 256 * 9 * cin * n * h * w * s * s for cin, s in CONVS)
        lines.append('  conv3x3_wgrad: %.2f TFLOP of useful work per call in %.1f us = %.1f %% of the f16 matrix peak / 3'
                     % (flops / 1e12, per['conv3x3_wgrad'][1], 100 * flops / (per['conv3x3_wgrad'][1] * 1e-6) / (F16_PEAK / 3)))
    return 0


def resources(glue=False):
    """Registers and LDS of the new kernels from a compile-only build (metadata; no instruction is looked at)."""
    from rmnet_amd import build
    source = 'decoder_glue_bwd.hip' if glue else 'conv3x3_wgrad.hip'
    names = ('pred_head_bwd', 'pred_head_bwd_merge', 'upsample_bwd_nhwcILi2E', 'upsample_bwd_nhwcILi4E', 'upsample_bwd_nchwILi2ELb1E',
             'upsample_bwd_nchwILi2ELb0E', 'upsample_bwd_nchwILi4ELb1E', 'upsample_bwd_nchwILi4ELb0E') if glue \
        else ('conv3x3_wgrad', 'wgrad_bias', 'wgrad_merge', 'conv_grad_stage')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'w.s')
        subprocess.run([build.hipcc_path(), '--offload-arch=' + build.ARCH, '-O3', '-std=c++17', '--cuda-device-only', '-S',
                        os.path.join(ROOT, 'rmnet_amd', 'csrc', source), '-o', out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = re.search(r'\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata', text, flags=re.S).group(1)
    entries = ['    ' + e for e in re.split(r'\n  - ', meta.split('amdhsa.kernels:', 1)[1])[1:]]
    lines = []
    for name in names:
        blk = [e for e in entries if re.search(r'^    \.name:\s+\S*\d+%sE' % name, e, flags=re.M)][0]
        get = lambda key: re.search(r'^    \.%s:\s+(\d+)' % key, blk, flags=re.M).group(1)
        lines.append('  %-16s VGPRs %s, SGPRs %s, static LDS %s B, scratch %s B, spilled VGPRs %s' % (
            name, get('vgpr_count'), get('sgpr_count'), get('group_segment_fixed_size'), get('private_segment_fixed_size'), get('vgpr_spill_count')))
    if glue:
        lines.append('  pred_head_bwd asks for 36864 B of dynamic LDS')
        return lines
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
    ap.add_argument('--out', default=None, help='profiles/r36_a_decoder_backward.md, or profiles/r37_a_decoder_glue_backward.md under --glue on')
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--glue', choices=['off', 'on'], default='off')
    ap.add_argument('--trace-second', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    glue = args.glue == 'on'
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'r37_a_decoder_glue_backward.md' if glue else 'r36_a_decoder_backward.md')
    if args.step:
        step_shape(args.step, args.trace_calls, glue, args.trace_second)
        return 0
    lines = []
    for step in SHAPES:
        print('--- step %s' % step, flush=True)
        p = subprocess.run(['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__), '--step', step, '--glue', args.glue],
                           stdout=subprocess.PIPE, text=True)
        print(p.stdout, flush=True)
        lines += ['```', p.stdout.rstrip(), '```', '']
        rc = p.returncode
        if rc == 0 and not args.no_trace:
            for route in (('off', 'on') if glue else (None,)):
                if rc == 0:
                    rc = trace(step, lines, route)
                    lines.append('')
        if rc != 0:
            print('step %s ended with status %d: stopping here' % (step, rc))
            lines.append('step %s ended with status %d: the run stopped here' % (step, rc))
            write_section(args.out, lines)
            return rc if rc > 0 else 1
    lines += ['### The new kernels, as compiled', ''] + ['```'] + resources(glue) + ['```', '']
    write_section(args.out, lines)
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
