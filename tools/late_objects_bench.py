# -*- coding: utf-8 -*-
"""Objects that appear mid-clip (csrc/late_objects.hip, rmnet_amd/object_plan.py, inference.segment_video_u8(new_objects=True)) on a
70-frame 854 x 480 clip with n_max_objects = 10 (K = 11 planes), two objects, the second one first annotated at frame 20:

  kernels  the two kernels alone between device events, 5 warm-up calls, then the median of 20 calls with the 10 % and 90 %
           quantiles, next to the torch sequences they replace: a scatter into a per-frame 256-bin presence vector (what
           clip_io.reorganize_lut does for the clip, per frame) against rmnet_label_presence_u8; the index writes of
           RMNet.forward followed by F.softmax against rmnet_object_edit_softmax_f32, on the [1,11,480,854] logits of the frame
           at which the second object is injected.  The results are compared.
  call     the whole call two ways, RMNet + TinyFlowNet with the procedural weights, plain and after fuse_epilogues():
           segment_video_u8(new_objects=True), and the route that needs no plan: the per-frame counts from a per-frame scatter and a
           download, one-hot masks of ALL frames, forward with the per-frame counts, argmax_labels.  One warm-up call each, then
           three timed calls each, alternating, host clock around a device synchronise; torch.cuda.max_memory_allocated above what
           is live before the call.  The label maps of the two routes are compared.

  --scales the same clip under multi-scale and flipped inference, scales (0.75, 1.0, 1.25) + flip (include/rmnet_hip.h I2):
           scaled_kernels  rmnet_label_presence_nearest_u8 over the three scales in one launch against rmnet_label_presence_u8 on
                           three materialised nearest-resized clips (the resizes are timed apart), and
                           rmnet_object_edit_softmax_nearest_f32 against rmnet_object_edit_softmax_f32 on a materialised, mirrored
                           map, at the 0.75 scale; the results are compared.
           scaled_call     segment_video_tta(new_objects=True), paired and unpaired, against helpers.multi_scale_inference fed the
                           one-hot masks of all frames and the per-frame counts, followed by argmax_labels; for scale,
                           segment_video_tta without late objects on the same frames.  Timed and compared as in ``call``.

    python tools/late_objects_bench.py            # every step in a child process of its own, under a time limit
    python tools/late_objects_bench.py --scales

The driver stops at the first step that does not return 0: nothing is started on the GPU after a step that failed there.
"""

import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 70, 480, 854
N_MAX_OBJECTS = 10
APPEARS_AT = 20
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STEPS = (('kernels', 300), ('call', 900))      # (step, time limit in seconds)
SCALED_STEPS = (('scaled_kernels', 300), ('scaled_call', 1100))
SCALES = (0.75, 1.0, 1.25)
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
    """(peak of the allocator during one call above what was allocated before it, the call's result)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6, out


def _clip(torch):
    """uint8 frames [N,H,W,3] and label maps [N,H,W] with the ids 0, 5, 38; id 38 is background before frame APPEARS_AT."""
    from rmnet_amd.synthetic import synthetic_clip
    frames, masks, _, _ = synthetic_clip(N, 3, H, W, seed=5, size=1.5)
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    u8 = ((frames[0] * std + mean).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    planes = masks[0].argmax(dim=1)
    planes[:APPEARS_AT][planes[:APPEARS_AT] == 2] = 0
    return u8, torch.tensor([0, 5, 38], dtype=torch.uint8)[planes]


def scatter_presence(torch, labels):
    """[N,256] presence of every frame by a scatter: the torch form of the presence kernel."""
    present = torch.zeros(labels.shape[0], 256, dtype=torch.int64, device=labels.device)
    present.scatter_(1, labels.reshape(labels.shape[0], -1).to(torch.int64), 1)
    return present


def step_kernels():
    import torch
    import torch.nn.functional as F
    from rmnet_amd import object_plan, ops
    assert torch.cuda.is_available(), 'this step needs a GPU'
    dev = torch.device('cuda', 0)
    _, labels = _clip(torch)
    labels = labels.to(dev)
    K = N_MAX_OBJECTS + 1
    plan = object_plan.appearance_plan(ops.label_presence(labels), N_MAX_OBJECTS)
    t = APPEARS_AT
    gen = torch.Generator(device=dev).manual_seed(0)
    logit0 = torch.randn(1, K, H, W, device=dev, generator=gen) * 4.0
    masks_t = ops.labels_onehot(labels[t:t + 1], K, plan.lut)[0]
    action = plan.action[t:t + 1].contiguous()
    rows = plan.action_host[t]
    prob = torch.empty(1, K, H, W, device=dev)
    logit = logit0.clone()

    def torch_edit():
        lg = logit0.clone()
        for k in range(K):
            if rows[k] == 2:
                lg[0, k] = masks_t[k].float() * 32.0605 - 16.1181
        missing = [k for k in range(K) if rows[k] == 1]
        if missing:
            lg[0, missing] = -16.1181
        return lg, F.softmax(lg, dim=1)

    def kernel_edit():
        logit.copy_(logit0)
        return ops.object_edit_softmax(logit, labels[t:t + 1], plan.lut[None], action, prob)

    print('%d label maps of %d x %d; one frame of K = %d logits with actions %s; median of 20 calls between device events (10 %% .. 90 %%)'
          % (N, W, H, K, rows.tolist()))
    print('| step | ms per call | 10 % .. 90 % |')
    print('|---|---|---|')
    for name, fn in (('rmnet_label_presence_u8, %d frames' % N, lambda: ops.label_presence(labels)),
                     ('  torch: scatter into [N,256]', lambda: scatter_presence(torch, labels)),
                     ('rmnet_object_edit_softmax_f32 (+ the copy that restores the logits)', kernel_edit),
                     ('  torch: clone, index writes, F.softmax', torch_edit),
                     ('  (the clone / copy alone)', lambda: logit.copy_(logit0))):
        med, lo, hi = _median_ms(torch, fn)
        print('| %s | %.3f | %.3f .. %.3f |' % (name, med, lo, hi))
    words = object_plan.presence_sets(ops.label_presence(labels))
    sets = [torch.nonzero(r).flatten().tolist() for r in scatter_presence(torch, labels).cpu()]
    lg, pr = torch_edit()
    kernel_edit()
    print('presence: kernel and scatter agree on every frame: %s; edit: logits equal in every bit: %s, largest difference of the '
          'probabilities %.3e' % (words == sets, bool(torch.equal(lg.view(torch.int32), logit.view(torch.int32))), float((pr - prob).abs().max())))
    torch.cuda.synchronize()


def step_call():
    import torch
    from rmnet_amd import clip_io, inference, networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.tiny_flownet import TinyFlowNet
    assert torch.cuda.is_available(), 'this step needs a GPU'
    dev = torch.device('cuda', 0)
    u8, labels = _clip(torch)
    u8, labels = u8.to(dev), labels.to(dev)
    K = N_MAX_OBJECTS + 1

    def planned(net, tfn):
        return inference.segment_video_u8(net, tfn, u8, labels, N_MAX_OBJECTS, MEAN, STD, overlay=False, new_objects=True)['labels']

    def unplanned(net, tfn):
        frames = clip_io.normalize_frames(u8, MEAN, STD)
        present = scatter_presence(torch, labels).cpu()                     # the per-frame counts of utils/data_loaders.py:58-65
        present[:, 255] = 0
        counts = (torch.cummax(present, dim=0).values.sum(dim=1) - 1).clamp(max=N_MAX_OBJECTS)
        lut, _ = clip_io.reorganize_lut(labels)
        masks = clip_io.onehot_labels(labels, K, lut)
        clip = frames.unsqueeze(0)
        est = net(clip, masks.unsqueeze(0), tfn(clip), counts.view(1, N), 5, device=dev)
        return clip_io.argmax_labels(est[0].contiguous())

    print('%d frames of %d x %d, n_max_objects = %d, object 2 from frame %d; seconds per call, host clock around a device synchronise, '
          '%d timed calls each after one warm-up call each, alternating' % (N, W, H, N_MAX_OBJECTS, APPEARS_AT, RUNS))
    print('| network | route | seconds per call (each run) | median | peak MB above the inputs |')
    print('|---|---|---|---|---|')
    for fused in (False, True):
        net = networks.procedural_init_(RMNet(None)).to(dev).eval()
        tfn = networks.procedural_init_(TinyFlowNet(None)).to(dev).eval()
        if fused:
            net.fuse_epilogues()
        variants = (('segment_video_u8(new_objects=True)', planned), ('one-hot masks of all frames + per-frame counts + argmax_labels', unplanned))
        times, peaks, results = {n: [] for n, _ in variants}, {}, {}
        with torch.no_grad():
            for name, fn in variants:
                peaks[name], out = _peak_mb(torch, lambda: fn(net, tfn))
                del out
            for _ in range(RUNS):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(net, tfn)
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
                    results[name] = out
                    del out
        for name, _ in variants:
            print('| %s | %s | %s | %.3f | %.0f |' % ('fuse_epilogues()' if fused else 'module graph', name, ', '.join('%.3f' % t for t in times[name]),
                                                   statistics.median(times[name]), peaks[name]))
        a, b = results[variants[0][0]], results[variants[1][0]]
        print('  label maps of the two routes equal at %.6f of the pixels; pixels of object 2 before / from frame %d: %d / %d'
              % (float((a == b).float().mean()), APPEARS_AT, int((a[:APPEARS_AT] == 2).sum()), int((a[APPEARS_AT:] == 2).sum())))
    torch.cuda.synchronize()


def _resized_labels(torch, tta, labels, fs):
    """The label maps nearest-resized by ``fs`` with the rule of the kernels, materialised."""
    h, w = tta.scaled_size(H, W, fs)
    iy = torch.from_numpy(tta.nearest_index(h, H, fs)).to(labels.device)
    ix = torch.from_numpy(tta.nearest_index(w, W, fs)).to(labels.device)
    return labels.index_select(1, iy).index_select(2, ix).contiguous()


def step_scaled_kernels():
    import torch
    from rmnet_amd import object_plan, ops, tta
    assert torch.cuda.is_available(), 'this step needs a GPU'
    dev = torch.device('cuda', 0)
    _, labels = _clip(torch)
    labels = labels.to(dev)
    K = N_MAX_OBJECTS + 1
    sizes = [tta.scaled_size(H, W, fs) for fs in SCALES]
    steps = [(tta.scale_for_factor(fs),) * 2 for fs in SCALES]
    resized = [_resized_labels(torch, tta, labels, fs) for fs in SCALES]
    plans = object_plan.appearance_plans(ops.label_presence(labels), ops.label_presence_nearest(labels, sizes, steps), N_MAX_OBJECTS)
    fs, (h, w), step, plan, t = SCALES[0], sizes[0], steps[0][0], plans[0], APPEARS_AT
    gen = torch.Generator(device=dev).manual_seed(0)
    logit0 = torch.randn(2, K, h, w, device=dev, generator=gen) * 4.0
    action = plan.action[t:t + 1].expand(2, -1).contiguous()
    lut = plan.lut[None].expand(2, -1).contiguous()
    full = labels[t:t + 1].expand(2, -1, -1)
    small = torch.stack([resized[0][t], torch.flip(resized[0][t], dims=[1])])
    logit, prob, prob_m = logit0.clone(), torch.empty(2, K, h, w, device=dev), torch.empty(2, K, h, w, device=dev)

    def sampling_edit():
        logit.copy_(logit0)
        return ops.object_edit_softmax(logit, full, lut, action, prob, sampling=(step, step, (False, True)))

    def materialised_edit():
        logit.copy_(logit0)
        return ops.object_edit_softmax(logit, small, lut, action, prob_m)

    print('%d label maps of %d x %d at the scales %s; a pair of frames (one mirrored) of K = %d logits at %d x %d with actions %s; median of '
          '20 calls between device events (10 %% .. 90 %%)' % (N, W, H, SCALES, K, w, h, plan.action_host[t].tolist()))
    print('| step | ms per call | 10 % .. 90 % |')
    print('|---|---|---|')
    for name, fn in (('rmnet_label_presence_nearest_u8, %d frames x 3 scales, one launch' % N, lambda: ops.label_presence_nearest(labels, sizes, steps)),
                     ('  rmnet_label_presence_u8 on three materialised resized clips', lambda: [ops.label_presence(r) for r in resized]),
                     ('  (materialising the three resized clips with torch indexing)', lambda: [_resized_labels(torch, tta, labels, f) for f in SCALES]),
                     ('rmnet_object_edit_softmax_nearest_f32, B = 2 (+ the copy that restores the logits)', sampling_edit),
                     ('  rmnet_object_edit_softmax_f32 on the materialised, mirrored maps (+ the copy)', materialised_edit),
                     ('  (the copy alone)', lambda: logit.copy_(logit0))):
        med, lo, hi = _median_ms(torch, fn)
        print('| %s | %.3f | %.3f .. %.3f |' % (name, med, lo, hi))
    same_words = all(torch.equal(a, ops.label_presence(r)) for a, r in zip(ops.label_presence_nearest(labels, sizes, steps), resized))
    sampling_edit()
    lg = logit.clone()
    materialised_edit()
    print('presence: every word equal to that of the materialised clips: %s; edit: logits equal in every bit: %s, probabilities equal in '
          'every bit: %s' % (same_words, bool(torch.equal(lg.view(torch.int32), logit.view(torch.int32))),
                             bool(torch.equal(prob.view(torch.int32), prob_m.view(torch.int32)))))
    torch.cuda.synchronize()


def step_scaled_call():
    from types import SimpleNamespace
    import torch
    from rmnet_amd import clip_io, helpers, inference, networks
    from rmnet_amd.rmnet import RMNet
    from rmnet_amd.tiny_flownet import TinyFlowNet
    assert torch.cuda.is_available(), 'this step needs a GPU'
    dev = torch.device('cuda', 0)
    u8, labels = _clip(torch)
    u8, labels = u8.to(dev), labels.to(dev)
    K = N_MAX_OBJECTS + 1
    frames = clip_io.normalize_frames(u8, MEAN, STD)
    cfg = SimpleNamespace(TEST=SimpleNamespace(FRAME_SCALES=list(SCALES), FLIP_LR=True, MEMORIZE_EVERY=5))

    def planned(pair):
        return lambda net, tfn: inference.segment_video_tta(net, tfn, {'frames': frames, 'labels': labels}, SCALES, True, 5, pair_flips=pair,
                                                            new_objects=True, n_max_objects=N_MAX_OBJECTS)['labels']

    def unplanned(net, tfn):
        present = scatter_presence(torch, labels).cpu()                     # the per-frame counts of utils/data_loaders.py:58-65
        present[:, 255] = 0
        counts = (torch.cummax(present, dim=0).values.sum(dim=1) - 1).clamp(max=N_MAX_OBJECTS)
        lut, _ = clip_io.reorganize_lut(labels)
        masks = clip_io.onehot_labels(labels, K, lut)
        _, probs = helpers.multi_scale_inference(cfg, tfn, net, frames.unsqueeze(0), masks.unsqueeze(0), counts.view(1, N))
        return clip_io.argmax_labels(probs[0].contiguous())

    def no_late_objects(net, tfn):
        lut, _ = clip_io.reorganize_lut(labels)
        masks = clip_io.onehot_labels(labels[:1], K, lut).expand(N, -1, -1, -1)
        return inference.segment_video_tta(net, tfn, {'frames': frames, 'masks': masks, 'n_objects': 2}, SCALES, True, 5)['labels']

    print('%d frames of %d x %d, n_max_objects = %d, object 2 from frame %d, scales %s + flip; seconds per call, host clock around a device '
          'synchronise, %d timed calls each after one warm-up call each, alternating' % (N, W, H, N_MAX_OBJECTS, APPEARS_AT, SCALES, RUNS))
    print('| network | route | seconds per call (each run) | median | peak MB above the inputs |')
    print('|---|---|---|---|---|')
    for fused in (False, True):
        net = networks.procedural_init_(RMNet(None)).to(dev).eval()
        tfn = networks.procedural_init_(TinyFlowNet(None)).to(dev).eval()
        if fused:
            net.fuse_epilogues()
        variants = (('segment_video_tta(new_objects=True), paired flips', planned(True)),
                    ('segment_video_tta(new_objects=True), unpaired', planned(False)),
                    ('helpers.multi_scale_inference, one-hot masks of all frames + per-frame counts + argmax_labels', unplanned),
                    ('(segment_video_tta without late objects: object 2 counted from frame 0)', no_late_objects))
        times, peaks, results = {n: [] for n, _ in variants}, {}, {}
        with torch.no_grad():
            for name, fn in variants:
                peaks[name], out = _peak_mb(torch, lambda: fn(net, tfn))
                del out
            for _ in range(RUNS):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(net, tfn)
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
                    results[name] = out
                    del out
        for name, _ in variants:
            print('| %s | %s | %s | %.3f | %.0f |' % ('fuse_epilogues()' if fused else 'module graph', name, ', '.join('%.3f' % t for t in times[name]),
                                                   statistics.median(times[name]), peaks[name]))
        want = results[variants[2][0]]
        for name in (variants[0][0], variants[1][0]):
            a = results[name]
            print('  %s: label maps equal to multi_scale_inference\'s at %.6f of the pixels; pixels of object 2 before / from frame %d: %d / %d'
                  % (name, float((a == want).float().mean()), APPEARS_AT, int((a[:APPEARS_AT] == 2).sum()), int((a[APPEARS_AT:] == 2).sum())))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--step', choices=[s for s, _ in STEPS + SCALED_STEPS])
    ap.add_argument('--scales', action='store_true', help='the steps under multi-scale and flipped inference')
    args = ap.parse_args()
    if args.step:
        {'kernels': step_kernels, 'call': step_call, 'scaled_kernels': step_scaled_kernels, 'scaled_call': step_scaled_call}[args.step]()
        return 0
    for step, limit in (SCALED_STEPS if args.scales else STEPS):
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
