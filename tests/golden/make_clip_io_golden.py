# -*- coding: utf-8 -*-
"""Generate tests/golden/clip_io.npz by running the REFERENCE's own loader transforms and get_segmentation on small clips.

Like make_golden.py this runs only where the reference is checked out (REF below); nothing of the reference is copied: its
modules are imported in place, fed the cases of tests/clip_io_ref.py and their outputs are stored as data.  utils/data_transforms.py
imports three modules that do not exist here and that none of the transforms used below touches (cv2, torchvision.transforms, the
compiled flow_affine_transformation); empty stand-ins are put into ``sys.modules`` for them.  No test runs this script.

    python tests/golden/make_clip_io_golden.py
"""

import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.dirname(HERE))

import clip_io_ref as ref  # noqa: E402

K = 4          # planes of the one-hot outputs: smaller than some remapped ids on purpose


def _reference():
    for name in ('cv2', 'torchvision', 'torchvision.transforms', 'flow_affine_transformation'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.path.insert(0, REF)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import utils.data_transforms as transforms
        import utils.helpers as helpers
    return transforms, helpers


def _sparse_clip():
    """Ids 3, 7, 200 and the ignore id, no 0: the remap has gaps to close and a lowest id that is not the background."""
    rng = np.random.default_rng(11)
    labels = np.asarray([3, 7, 200, 255], np.uint8)[np.repeat(rng.integers(0, 4, (3, 4, 5)), 2, axis=2)[:, :, :9]]
    labels[2][labels[2] == 200] = 7               # a frame that lacks one of the clip's ids
    return rng.integers(0, 256, labels.shape + (3,), dtype=np.uint8), labels


def cases():
    """(name, uint8 frames, labels, mean, std, alpha)"""
    out = [('clip', *ref.overlay_clip(), ref.MEAN, ref.STD, 0.4),
           ('odd', *ref.overlay_clip(), ref.ODD_MEAN, ref.ODD_STD, 0.7),
           ('rows3x5', *ref.shape_case(3, 3, 5), ref.MEAN, ref.STD, 0.4),
           ('one_row', *ref.shape_case(3, 1, 64), ref.MEAN, ref.STD, 0.4),
           ('one_col', *ref.shape_case(3, 7, 1), ref.MEAN, ref.STD, 0.4),
           ('wide', *ref.shape_case(1, 5, 70), ref.MEAN, ref.STD, 0.0),
           ('sparse', *_sparse_clip(), ref.MEAN, ref.STD, 1.0)]
    return out


def main():
    transforms, helpers = _reference()
    data = {'names': np.array([c[0] for c in cases()]), 'K': np.int64(K)}
    for name, frames, labels, mean, std, alpha in cases():
        mean, std = list(mean), list(std)
        # Normalize + ToTensor (utils/data_transforms.py:41-50, 86-96)
        normalized = [helpers.img_normalize(f, mean, std).astype(np.float32) for f in frames]
        tensor = torch.from_numpy(np.array(normalized)).float().permute(0, 3, 1, 2).contiguous()
        # ReorganizeObjectID + ToOneHot without the shuffle (:53-83)
        _, masks, _ = transforms.ReorganizeObjectID({'ignore_idx': 255})(None, [m.copy() for m in labels], None)
        ids = np.unique(labels)
        n_ids = len(ids[ids != 255])
        remapped = np.stack(masks)
        onehot_remapped = np.stack([helpers.to_onehot(m, K) for m in masks])
        onehot_plain = np.stack([helpers.to_onehot(m, K) for m in labels])
        # get_segmentation of every frame (utils/helpers.py:138-178) on the normalised frames, as the driver calls it
        params = {'mean': mean, 'std': std}
        overlay = np.stack([np.array(helpers.get_segmentation(tensor[i], torch.from_numpy(labels[i].astype(np.int64)), params,
                                                              ignore_idx=255, alpha=alpha)) for i in range(len(frames))])
        denorm = np.stack([helpers.img_denormalize(tensor[i], mean, std) for i in range(len(frames))])
        paletted = helpers.get_segmentation(None, torch.from_numpy(labels[0].astype(np.int64)), params)
        for key, value in (('frames', frames), ('labels', labels), ('mean', np.asarray(mean)), ('std', np.asarray(std)),
                           ('alpha', np.float64(alpha)), ('normalized', tensor.numpy()), ('remapped', remapped.astype(np.uint8)),
                           ('n_ids', np.int64(n_ids)), ('onehot_remapped', onehot_remapped), ('onehot_plain', onehot_plain),
                           ('overlay', overlay), ('denorm', denorm)):
            data['%s/%s' % (name, key)] = value
        data['palette'] = np.asarray(paletted.getpalette(), np.uint8).reshape(-1, 3)
        assert paletted.mode == 'P' and np.array_equal(np.array(paletted), labels[0])
    path = os.path.join(HERE, 'clip_io.npz')
    np.savez_compressed(path, **data)
    print('%s: %d arrays, %d bytes' % (path, len(data), os.path.getsize(path)))


if __name__ == '__main__':
    main()
