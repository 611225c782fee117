# -*- coding: utf-8 -*-
"""Event-timed loops for csrc/flow_head.hip at the bench shapes (16 frame pairs of 480 x 854): every flow head next to the library's
convolution of the same buffer with the zero-padded weight, every flow upsampler next to conv-transpose + copy + zero fill, and
TinyFlowNet._forward under RMNET_FLOW_CONV=split and full.  10 calls after 3 warm-up calls, one process.

    python tools/flow_head_bench.py            # prints one table row per line
"""

import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('PYTORCH_MIOPEN_SUGGEST_NHWC', '1')

from rmnet_amd import networks, ops                      # noqa: E402
from rmnet_amd.tiny_flownet import TinyFlowNet           # noqa: E402

COPY_RATE = 6.3e12        # bytes/s, the copy rate the project quotes for the MI355X
N = 16
# level: (H, W, Cin, x_ld) of the head's input
HEADS = {5: (8, 14, 512, 512), 4: (16, 28, 770, 800), 3: (32, 56, 386, 416), 2: (64, 112, 194, 224)}


def timed(fn, calls=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    dev = torch.device('cuda', 0)
    net = networks.procedural_init_(TinyFlowNet(None)).to(dev).eval().fuse_epilogues().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        print('| head | map | Cin / x_ld | kernel ms | GB/s | of 6.3 TB/s | library ms | kernel / library |')
        for level, (h, w, cin, ld) in HEADS.items():
            x = torch.randn(N, h, w, ld, generator=g).to(dev).permute(0, 3, 1, 2)
            x[:, cin:] = 0.0
            head = getattr(net, 'predict_flow%d' % level)
            pack = net._flow_head_packs[level]
            wlib = net._flow_head_w[level] if level in net._flow_head_w else head.weight
            got = ops.flow_head(x, pack, head.bias, cin=cin)
            want = F.conv2d(x, wlib, head.bias, 1, 1)
            diff = float((got - want).abs().max())
            tk = timed(lambda: ops.flow_head(x, pack, head.bias, cin=cin))
            tl = timed(lambda: F.conv2d(x, wlib, head.bias, 1, 1))
            rate = N * h * w * ld * 4 / (tk * 1e-3)
            print('| predict_flow%d | %dx%d | %d / %d | %.4f | %.0f | %.3f | %.4f | %.2f | (max diff %.2e)'
                  % (level, h, w, cin, ld, tk, rate / 1e9, rate / COPY_RATE, tl, tk / tl, diff))
        print('| upsampler | flow map | out_ld, coff | kernel ms | library + copy + zero ms | kernel / library |')
        for level, (h, w, cin, ld) in ((4, HEADS[4]), (3, HEADS[3]), (2, HEADS[2])):
            up = getattr(net, 'upsampled_flow%d_to_%d' % (level + 1, level))
            flow = torch.randn(N, 2, h // 2, w // 2, generator=g).to(dev)
            cat = torch.zeros(N, h, w, ld, device=dev).permute(0, 3, 1, 2)
            wk = net._flow_up_w[level]

            def lib():
                cat[:, cin - 2:cin].copy_(up(flow))
                cat[:, cin:].zero_()
            tk = timed(lambda: ops.flow_up(flow, wk, cat, cin - 2))
            tl = timed(lib)
            print('| upsampled_flow%d_to_%d | %dx%d | %d, %d | %.4f | %.4f | %.2f |' % (level + 1, level, h // 2, w // 2, ld, cin - 2, tk, tl, tk / tl))
        a, b = (torch.rand(N, 3, 480, 854, generator=g).to(dev) for _ in range(2))
        outs = {}
        for mode in ('split', 'full', 'split', 'full'):
            os.environ['RMNET_FLOW_CONV'] = mode
            net.flow_range_word(dev).zero_()
            t = timed(lambda: net._forward(a, b))
            outs[mode] = net._forward(a, b)
            print('_forward on %d frame pairs, RMNET_FLOW_CONV=%s: %.4f ms (range word %d)' % (N, mode, t, net.flow_range_count()))
        print('max |flow(full) - flow(split)| %.3e on a largest |flow| of %.3e'
              % (float((outs['full'] - outs['split']).abs().max()), float(outs['split'].abs().max())))


if __name__ == '__main__':
    main()
