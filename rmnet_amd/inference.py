# -*- coding: utf-8 -*-
"""Sharded per-video inference (BASELINE configs[3]).

The reference segments its test set one clip at a time on one GPU (core/inference.py:49-75: flows from
TinyFlowNet, RMNet.forward, argmax, save).  Clips are independent, so here every rank takes the clips
``rmnet_amd.dist.assign_videos`` gives it (longest-first greedy by frames x objects), runs the
device-resident frame loop on them, and only the uint8 label maps -- or, with ground truth, the J (and F)
scalars -- cross RCCL at the end.  No communication while a clip runs.
"""

import os

import torch

from . import clip_io
from . import dist as rd
from . import metrics


def video_costs(videos):
    """Cost of a clip ~ frames x objects (what the frame loop's time is proportional to)."""
    return [int(v['frames'].shape[0]) * max(int(v['n_objects']), 1) for v in videos]


@torch.no_grad()
def segment_video(net, flownet, video, memorize_every=5):
    """One clip: ``video`` = {'frames' [N,3,H,W] f32 normalised, 'masks' [N,K,H,W] one-hot (only frame 0
    is read), 'n_objects' int}.  Returns the label maps uint8 [N,H,W] on the model's device
    (core/inference.py:52-63 without the file output)."""
    frames = video['frames'].unsqueeze(0)
    masks = video['masks'].unsqueeze(0)
    N = frames.shape[1]
    n_objects = torch.full((1, N), int(video['n_objects']), dtype=torch.long)
    dev = next(net.parameters()).device
    frames = frames.to(dev, non_blocking=True)
    flows = flownet(frames)
    est = net(frames, masks, flows, n_objects, memorize_every, device=dev)
    return est[0].argmax(dim=1).to(torch.uint8)


@torch.no_grad()
def clip_probs(net, flownet, video, memorize_every=5):
    """``segment_video`` without the argmax: the probabilities float32 [N,K,H,W] of one clip on the model's device, what the
    validation loss (``losses.validation_loss``) is taken on."""
    frames = video['frames'].unsqueeze(0)
    masks = video['masks'].unsqueeze(0)
    N = frames.shape[1]
    n_objects = torch.full((1, N), int(video['n_objects']), dtype=torch.long)
    dev = next(net.parameters()).device
    frames = frames.to(dev, non_blocking=True)
    flows = flownet(frames)
    est = net(frames, masks, flows, n_objects, memorize_every, device=dev)
    return est[0]


# Whether segment_video_tta runs a scale's unflipped and flipped clips as one batch of two.  Measured on an MI355X on 70-frame 480p
# clips, scales (0.75, 1.0, 1.25) + flip (profiles/r28_a_tta.md): paired 2.51 s against 2.99 s with one object, 5.50 s against 5.83 s with
# three, the runs of a variant within 0.05 s of each other.
PAIR_FLIPS = True


@torch.no_grad()
def segment_video_tta(net, flownet, video, frame_scales=(1.0,), flip_lr=False, memorize_every=5, pair_flips=None, new_objects=False,
                      n_max_objects=None):
    """One clip at several scales, optionally also mirrored left-right, merged on the device: multi_scale_inference
    (utils/helpers.py:44-78) followed by the driver's argmax.  ``video`` as for ``segment_video``.  Returns {'probs': float32
    [N,K,H,W], 'labels': uint8 [N,H,W]} on the model's device.

    Per scale: the frames are resized by ``tta.resize_bilinear``, the first frame's masks by nearest neighbour, TinyFlowNet runs once
    on the unflipped frames, and the flipped twin takes the mirrored flow with its x channel negated, as the reference does.  With
    ``pair_flips`` the two clips of a scale go through ONE ``net`` call as a batch of two (slot 1 holds the mirrored frames, written
    by the resize itself); otherwise through two calls.  The entries -- per scale the unflipped, then the flipped one -- are merged by
    one ``tta.merge``: no resized probability clip, stack or mean tensor is ever built.

    ``new_objects=True`` is the YouTube-VOS protocol under the scales and the flip: ``video`` = {'frames', 'labels' uint8 [N,H,W] at
    full size} and ``n_max_objects`` is the configuration's cap.  The reference resizes the one-hot masks of every frame by nearest
    neighbour and counts the objects at full size; here one ``object_plan.label_presence``, one ``label_presence_scaled`` over all
    scales and one ``appearance_plans`` -- the call's one host synchronisation for its bookkeeping -- give a plan per scale, which
    serves the unflipped and the flipped pass alike.  Per scale the first frame's masks are the one-hot planes of frame 0 indexed
    by ``tta.nearest_index`` (the plain formula, the rule the plans and the edits follow), and the network reads the full-size label
    maps at the sampled, mirrored position where it injects an object.  The result also holds 'ids' and 'n_objects_per_frame'."""
    from torch.nn.functional import interpolate
    from . import tta
    if new_objects:
        return _segment_video_tta_new_objects(net, flownet, video, frame_scales, flip_lr, memorize_every, pair_flips, n_max_objects)
    scales = [float(s) for s in frame_scales]
    entries = len(scales) * (2 if flip_lr else 1)
    if not 1 <= entries <= tta.MAX_ENTRIES:
        raise RuntimeError('expected 1 .. %d entries (scales, doubled by the flip), got %d' % (tta.MAX_ENTRIES, entries))
    pair = bool(PAIR_FLIPS if pair_flips is None else pair_flips) and bool(flip_lr)
    dev = next(net.parameters()).device
    frames = video['frames'].to(dev, non_blocking=True).float().contiguous()
    first = video['masks'][:1].to(dev, non_blocking=True).float()          # [1,K,H,W]: the only masks the network reads
    N, _, H, W = frames.shape
    n_objects = int(video['n_objects'])
    sources, flipped = [], []
    for fs in scales:
        h, w = tta.scaled_size(H, W, fs)
        clip = torch.empty(2 if pair else 1, N, 3, h, w, dtype=torch.float32, device=dev)
        tta.resize_bilinear(frames, fs, out=clip[0])
        mask = interpolate(first, scale_factor=fs, mode='nearest').int()
        flow = flownet(clip[:1])
        runs = [(clip[:1], mask, flow)]
        if flip_lr:
            mirrored = clip[1:] if pair else torch.empty_like(clip)
            tta.resize_bilinear(frames, fs, flip=True, out=mirrored[0])
            flow_m = torch.flip(flow, dims=[4])
            flow_m[:, :, 0].neg_()
            runs.append((mirrored, torch.flip(mask, dims=[3]), flow_m))
        if pair:
            runs = [(clip, torch.cat([runs[0][1], runs[1][1]]), torch.cat([runs[0][2], runs[1][2]]))]
        for fr, mk, fl in runs:
            B = fr.shape[0]
            est = net(fr, mk.unsqueeze(1).expand(-1, N, -1, -1, -1), fl, torch.full((B, N), n_objects, dtype=torch.long), memorize_every,
                      device=dev)
            sources.extend(est[b] for b in range(B))
        flipped.extend([False, True] if flip_lr else [False])
    probs, labels = tta.merge([s.contiguous() for s in sources], flipped, (H, W))
    return {'probs': probs, 'labels': labels}


def _segment_video_tta_new_objects(net, flownet, video, frame_scales, flip_lr, memorize_every, pair_flips, n_max_objects):
    from . import object_plan, tta
    if 'labels' not in video:
        raise RuntimeError('new_objects needs video[\'labels\']: the uint8 label maps of every frame, [N, H, W]')
    if n_max_objects is None:
        raise RuntimeError('new_objects needs n_max_objects, the cap on the number of objects')
    scales = [float(s) for s in frame_scales]
    entries = len(scales) * (2 if flip_lr else 1)
    if not 1 <= entries <= tta.MAX_ENTRIES:
        raise RuntimeError('expected 1 .. %d entries (scales, doubled by the flip), got %d' % (tta.MAX_ENTRIES, entries))
    pair = bool(PAIR_FLIPS if pair_flips is None else pair_flips) and bool(flip_lr)
    dev = next(net.parameters()).device
    frames = video['frames'].to(dev, non_blocking=True).float().contiguous()
    labels = video['labels'].to(dev, non_blocking=True).contiguous()
    N, _, H, W = frames.shape
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (N, H, W):
        raise RuntimeError('new_objects needs the label maps of every frame, uint8 [N, H, W]')
    plans = object_plan.appearance_plans(object_plan.label_presence(labels), object_plan.label_presence_scaled(labels, H, W, scales),
                                         n_max_objects)                                             # (the host synchronisation)
    if plans[0].n_max < 0:
        raise RuntimeError('the label maps hold no id but the ignored one: there is nothing to segment')
    first = clip_io.onehot_labels(labels[:1], plans[0].K, plans[0].lut)                             # [1,K,H,W], full size
    sources, flipped = [], []
    for fs, plan in zip(scales, plans):
        h, w = tta.scaled_size(H, W, fs)
        clip = torch.empty(2 if pair else 1, N, 3, h, w, dtype=torch.float32, device=dev)
        tta.resize_bilinear(frames, fs, out=clip[0])
        iy = torch.from_numpy(tta.nearest_index(h, H, fs)).to(dev)
        ix = torch.from_numpy(tta.nearest_index(w, W, fs)).to(dev)
        mask = first.index_select(2, iy).index_select(3, ix)                                        # [1,K,h,w]
        flow = flownet(clip[:1])
        runs = [(clip[:1], mask, flow, (False,))]
        if flip_lr:
            mirrored = clip[1:] if pair else torch.empty_like(clip)
            tta.resize_bilinear(frames, fs, flip=True, out=mirrored[0])
            flow_m = torch.flip(flow, dims=[4])
            flow_m[:, :, 0].neg_()
            runs.append((mirrored, torch.flip(mask, dims=[3]), flow_m, (True,)))
        if pair:
            runs = [(clip, torch.cat([runs[0][1], runs[1][1]]), torch.cat([runs[0][2], runs[1][2]]), (False, True))]
        for fr, mk, fl, flips in runs:
            B = fr.shape[0]
            est = net(fr, mk.unsqueeze(1), fl, None, memorize_every, device=dev,
                      object_plan=(labels.unsqueeze(0).expand(B, -1, -1, -1), [plan] * B, (fs, flips)))
            sources.extend(est[b] for b in range(B))
        flipped.extend([False, True] if flip_lr else [False])
    probs, out = tta.merge([s.contiguous() for s in sources], flipped, (H, W))
    return {'probs': probs, 'labels': out, 'ids': plans[0].ids_dev, 'n_objects_per_frame': list(plans[0].n_objects)}


@torch.no_grad()
def segment_video_u8(net, flownet, frames_u8, labels_u8, n_max_objects, mean, std, memorize_every=5, overlay=True,
                     frame_scales=(1.0,), flip_lr=False, new_objects=False, scale_plans=False):
    """One clip from what a folder of images holds to what the reference's driver writes (core/inference.py:50-71 with the test
    loader in front of it, utils/data_loaders.py:40-71), without leaving the device: ``frames_u8`` uint8 [N,H,W,3] RGB,
    ``labels_u8`` uint8 palette label maps [N,H,W] or the first frame's [H,W] (only frame 0 is read by the network; the object ids
    are reorganised over whatever is given, as ReorganizeObjectID does over the clip).  Returns {'labels': uint8 [N,H,W],
    'overlay': uint8 [N,H,W,3] or None, 'n_objects': int} with the tensors on the model's device.  ``n_objects`` =
    min(ids in the label maps - 1, n_max_objects) (utils/data_loaders.py:64) costs the one host synchronisation of the call.
    With other ``frame_scales`` than (1.0,) or with ``flip_lr`` the labels come from ``segment_video_tta`` (TEST.FRAME_SCALES and
    TEST.FLIP_LR of the reference's configuration); with the defaults that path is not entered.

    ``new_objects=True`` is the YouTube-VOS protocol: an object may first be annotated several frames into the clip.  ``labels_u8``
    must then be [N,H,W] (frames without an annotation hold the ids of whatever is annotated there, e.g. all background: the
    count is cumulative).  ``object_plan.label_presence`` and ``appearance_plan`` replace ``reorganize_lut``'s count -- their one
    download is the call's host synchronisation --, only frame 0 is turned into one-hot masks, and the network injects every new
    object at the frame where the clamped cumulative count changes and keeps it absent until then (models/rmnet.py:436-450).
    The result also holds 'ids' (uint8, the clip's raw ids ascending: ``clip_io.restore_ids(labels, ids)`` gives the label maps in
    the clip's own ids, as a submission wants them) and 'n_objects_per_frame' (list); 'n_objects' is the last frame's count.
    A nearest-resized label map can lose a small object and with it an injection, so under other ``frame_scales`` than (1.0,) or
    ``flip_lr`` every scale needs a plan of its own: ``scale_plans=True`` makes them (``segment_video_tta(new_objects=True)``, one
    host synchronisation as before) and mirrors what the reference's multi_scale_inference does with the masks of every frame.
    ``scale_plans`` defaults to False, and the combination is then refused with a RuntimeError, as it was before the plans per
    scale existed."""
    if new_objects:
        return _segment_video_u8_new_objects(net, flownet, frames_u8, labels_u8, n_max_objects, mean, std, memorize_every, overlay,
                                             frame_scales, flip_lr, scale_plans)
    dev = next(net.parameters()).device
    frames_u8 = frames_u8.to(dev, non_blocking=True).contiguous()
    labels_u8 = labels_u8.to(dev, non_blocking=True)
    if labels_u8.dim() == 2:
        labels_u8 = labels_u8.unsqueeze(0)
    labels_u8 = labels_u8.contiguous()
    N = frames_u8.shape[0]
    frames = clip_io.normalize_frames(frames_u8, mean, std)
    lut, n_ids = clip_io.reorganize_lut(labels_u8)
    masks = clip_io.onehot_labels(labels_u8, int(n_max_objects) + 1, lut)
    if masks.shape[0] != N:
        masks = masks[:1].expand(N, -1, -1, -1)                      # frame 0 is the only one the network reads
    n_objects = min(int(n_ids) - 1, int(n_max_objects))
    if n_objects < 0:
        raise RuntimeError('the label maps hold no id but the ignored one: there is nothing to segment')
    if tuple(float(s) for s in frame_scales) != (1.0,) or flip_lr:
        labels = segment_video_tta(net, flownet, {'frames': frames, 'masks': masks, 'n_objects': n_objects}, frame_scales, flip_lr,
                                   memorize_every)['labels']
        return {'labels': labels, 'overlay': clip_io.overlay(frames, labels, mean, std) if overlay else None, 'n_objects': n_objects}
    clip = frames.unsqueeze(0)
    flows = flownet(clip)
    est = net(clip, masks.unsqueeze(0), flows, torch.full((1, N), n_objects, dtype=torch.long), memorize_every, device=dev)
    labels = clip_io.argmax_labels(est[0].contiguous())
    return {'labels': labels, 'overlay': clip_io.overlay(frames, labels, mean, std) if overlay else None, 'n_objects': n_objects}


def _segment_video_u8_new_objects(net, flownet, frames_u8, labels_u8, n_max_objects, mean, std, memorize_every, overlay, frame_scales,
                                  flip_lr, scale_plans=False):
    from . import object_plan
    scaled = tuple(float(s) for s in frame_scales) != (1.0,) or bool(flip_lr)
    if scaled and not scale_plans:
        raise RuntimeError('new_objects cannot be combined with frame_scales / flip_lr: every scale would need its own plan')
    if labels_u8.dim() != 3 or labels_u8.shape[0] != frames_u8.shape[0]:
        raise RuntimeError('new_objects needs the label maps of every frame, [N, H, W]')
    dev = next(net.parameters()).device
    frames_u8 = frames_u8.to(dev, non_blocking=True).contiguous()
    labels_u8 = labels_u8.to(dev, non_blocking=True).contiguous()
    frames = clip_io.normalize_frames(frames_u8, mean, std)
    if scaled:
        r = segment_video_tta(net, flownet, {'frames': frames, 'labels': labels_u8}, frame_scales, flip_lr, memorize_every, new_objects=True,
                              n_max_objects=n_max_objects)
        return {'labels': r['labels'], 'overlay': clip_io.overlay(frames, r['labels'], mean, std) if overlay else None,
                'n_objects': r['n_objects_per_frame'][-1], 'ids': r['ids'], 'n_objects_per_frame': r['n_objects_per_frame']}
    plan = object_plan.appearance_plan(object_plan.label_presence(labels_u8), n_max_objects)       # (the host synchronisation)
    if plan.n_max < 0:
        raise RuntimeError('the label maps hold no id but the ignored one: there is nothing to segment')
    first = clip_io.onehot_labels(labels_u8[:1], plan.K, plan.lut)                                  # [1,K,H,W]
    clip = frames.unsqueeze(0)
    flows = flownet(clip)
    est = net(clip, first.unsqueeze(0), flows, None, memorize_every, device=dev, object_plan=(labels_u8.unsqueeze(0), [plan]))
    labels = clip_io.argmax_labels(est[0].contiguous())
    return {'labels': labels, 'overlay': clip_io.overlay(frames, labels, mean, std) if overlay else None, 'n_objects': plan.n_max,
            'ids': plan.ids_dev, 'n_objects_per_frame': list(plan.n_objects)}


def write_segmentations(folder, images):
    """Write ``images`` as ``%05d.png`` into ``folder`` (created when missing), like core/inference.py:56-71: uint8 label maps
    [N,H,W] as P-mode images with the DAVIS palette, uint8 overlays [N,H,W,3] as RGB.  Returns the paths."""
    from PIL import Image
    images = images.detach().to('cpu', torch.uint8).numpy()
    if images.ndim not in (3, 4) or (images.ndim == 4 and images.shape[3] != 3):
        raise RuntimeError('expected label maps [N, H, W] or overlays [N, H, W, 3]')
    os.makedirs(folder, exist_ok=True)
    palette = clip_io.PALETTE.reshape(-1).tolist()
    paths = []
    for i, array in enumerate(images):
        image = Image.fromarray(array)
        if array.ndim == 2:
            image.putpalette(palette)
        paths.append(os.path.join(folder, '%05d.png' % i))
        image.save(paths[-1])
    return paths


def segment_videos(videos, segment_fn, rank=None, world_size=None, gather=True, dst=0):
    """Run ``segment_fn(video) -> uint8 [N,H,W]`` on this rank's share of ``videos`` (a list, identical
    on every rank) and gather the label maps on rank ``dst``.  Returns {video index: label maps} on
    ``dst`` (every rank's own share when ``gather`` is False or no process group exists)."""
    if rank is None or world_size is None:
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        world_size = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    mine = rd.my_videos(video_costs(videos), rank, world_size)
    results = {v: segment_fn(videos[v]) for v in mine}
    if not gather:
        return results
    return rd.gather_label_maps(results, len(videos), dst=dst)


def evaluate_videos(videos, segment_fn, rank=None, world_size=None):
    """Mean region similarity J over all clips and objects (utils/metrics.py:84-102; first and last
    frame of a clip skipped as in DAVIS) with ground truth ``video['labels']`` uint8 [N,H,W]: every
    rank scores its own clips on its device and two scalars are all-reduced.  Returns a float on every
    rank."""
    if rank is None or world_size is None:
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        world_size = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    mine = rd.my_videos(video_costs(videos), rank, world_size)
    total, count = 0.0, 0.0
    for v in mine:
        pred = segment_fn(videos[v])
        gt = videos[v]['labels'].to(pred.device)
        j = metrics.jaccard_per_object(pred.long(), gt.long(), int(videos[v]['n_objects']))
        if j.shape[0] > 2:
            j = j[1:-1]
        total += float(j.sum())
        count += float(j.numel())
    total = rd.sum_over_ranks(total)
    count = rd.sum_over_ranks(count)
    return total / max(count, 1.0)


def evaluate_videos_jf(videos, segment_fn, rank=None, world_size=None):
    """The reference's three scores (utils/metrics.py:22-41) with ground truth ``video['labels']`` uint8 [N,H,W]: mean region
    similarity J, mean boundary measure F (utils/metrics.py:119-169) and their mean, over all clips and objects, with the
    sharding and the frame convention of ``evaluate_videos`` (first and last frame of a clip skipped).  Every rank scores its own
    clips on its device -- one ``metrics.boundary_counts`` and one ``metrics.jaccard_per_object`` call per clip -- and three
    scalars are all-reduced.  Returns {'J-Mean', 'F-Mean', 'JF-Mean'} as floats on every rank."""
    if rank is None or world_size is None:
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        world_size = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    mine = rd.my_videos(video_costs(videos), rank, world_size)
    j_total, f_total, count = 0.0, 0.0, 0.0
    for v in mine:
        pred = segment_fn(videos[v])
        gt = videos[v]['labels'].to(pred.device)
        n_objects = int(videos[v]['n_objects'])
        j = metrics.jaccard_per_object(pred.long(), gt.long(), n_objects)
        radius = metrics.boundary_radius(pred.shape[-2], pred.shape[-1])
        f = metrics.f_from_counts(metrics.boundary_counts(pred, gt, n_objects, radius))
        if j.shape[0] > 2:
            j, f = j[1:-1], f[1:-1]
        j_total += float(j.sum())
        f_total += float(f.sum())
        count += float(j.numel())
    j_total = rd.sum_over_ranks(j_total)
    f_total = rd.sum_over_ranks(f_total)
    count = max(rd.sum_over_ranks(count), 1.0)
    return {'J-Mean': j_total / count, 'F-Mean': f_total / count, 'JF-Mean': metrics.jf_mean(j_total / count, f_total / count)}


def test_videos(videos, probs_fn, rank=None, world_size=None, loss_route=None):
    """The reference's test driver (core/test.py:69-141) over ``videos`` with ``probs_fn(video) -> float32 [N,K,H,W]`` and ground
    truth ``video['labels']`` uint8 [N,H,W].  Per clip: the loss of core/test.py:97 (``losses.validation_loss``) over all N
    frames, frame 0 included; and J and F by the reference's own convention (utils/metrics.py:70-81, 105-116): frame 0 dropped,
    the last frame kept, objects 1 .. ``video['n_objects']``, the prediction being the argmax of the probabilities.  Across clips
    as its AverageMeter does: the loss a plain mean over clips, the metrics weighted by the clip's object count, JF-Mean from
    ``metrics.jf_mean``.  Clips are sharded as in ``evaluate_videos`` and five sums are all-reduced.  Returns {'Loss', 'J-Mean',
    'F-Mean', 'JF-Mean'} as floats on every rank.  A clip with a label >= K or a probability outside [0, 1] raises RuntimeError;
    reading that count is the clip's one host synchronisation (the reference's ``loss.item()`` is one too)."""
    from . import losses
    if rank is None or world_size is None:
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        world_size = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    mine = rd.my_videos(video_costs(videos), rank, world_size)
    loss_total, clips, j_total, f_total, weight = 0.0, 0.0, 0.0, 0.0, 0.0
    for v in mine:
        probs = probs_fn(videos[v]).contiguous()
        gt = videos[v]['labels'].to(probs.device).contiguous()
        n_objects = int(videos[v]['n_objects'])
        loss = losses.validation_loss(probs, gt, route=loss_route)
        pred = probs.argmax(dim=1).to(torch.uint8)
        j = metrics.jaccard_per_object(pred[1:].long(), gt[1:].long(), n_objects)
        radius = metrics.boundary_radius(pred.shape[-2], pred.shape[-1])
        f = metrics.f_from_counts(metrics.boundary_counts(pred[1:].contiguous(), gt[1:].contiguous(), n_objects, radius))
        n_bad = int(loss['n_bad'])                                                           # (the host synchronisation)
        if n_bad:
            raise RuntimeError('clip %d: %d pixels have a label >= K or a probability outside [0, 1]' % (v, n_bad))
        loss_total += float(loss['loss'])
        clips += 1.0
        j_total += float(j.mean()) * n_objects
        f_total += float(f.mean()) * n_objects
        weight += float(n_objects)
    loss_total, clips, j_total, f_total, weight = (rd.sum_over_ranks(x) for x in (loss_total, clips, j_total, f_total, weight))
    j_mean, f_mean = j_total / max(weight, 1.0), f_total / max(weight, 1.0)
    return {'Loss': loss_total / max(clips, 1.0), 'J-Mean': j_mean, 'F-Mean': f_mean, 'JF-Mean': metrics.jf_mean(j_mean, f_mean)}
