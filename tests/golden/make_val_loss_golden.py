# -*- coding: utf-8 -*-
"""Generate tests/golden/val_loss.npz by running the REFERENCE's own LovaszLoss (models/lovasz_loss.py) and torch.nn.NLLLoss, as
core/test.py:61-62, 97 sets them up, on a dozen small clips.

Like make_clip_io_golden.py this runs only where the reference is checked out (REF below); nothing of the reference is copied: its
module is imported in place, fed the clips of tests/val_loss_ref.py and its outputs are stored as data.  No test runs this script.

    python tests/golden/make_val_loss_golden.py
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.dirname(HERE))

import val_loss_ref as ref  # noqa: E402

IGNORE = 255


def cases():
    """(name, probs [N,K,H,W] float32, labels [N,H,W] uint8)"""
    rng = np.random.default_rng(31)
    out = []
    for i, (K, peak) in enumerate([(1, 2.0), (2, 4.0), (2, 0.0), (3, 4.0), (3, 1.0), (4, 6.0), (4, 0.5), (3, 8.0), (2, 1.0), (4, 3.0)]):
        out.append(('random%d' % i, *ref.softmax_clip(rng, 2, K, 5, 7, peak=peak)))
    out.append(('ignored', *ref.softmax_clip(rng, 2, 3, 5, 7, peak=3.0, ignore=0.3)))
    out.append(('missing_class', *ref.softmax_clip(rng, 2, 4, 5, 7, peak=3.0, n_labels=3)))
    assert (out[-2][2] == IGNORE).any() and not (out[-1][2] == 3).any()
    return out


def main():
    sys.path.insert(0, REF)
    from models.lovasz_loss import LovaszLoss
    lovasz_loss = LovaszLoss(ignore_index=IGNORE)
    nll_loss = torch.nn.NLLLoss(ignore_index=IGNORE)
    data = {'names': np.array([c[0] for c in cases()])}
    for name, probs, labels in cases():
        est = torch.from_numpy(probs).permute(1, 0, 2, 3).unsqueeze(0)            # [B, C, F, H, W], as core/test.py:90 leaves it
        masks = torch.from_numpy(labels.astype(np.int64)).unsqueeze(0)
        lovasz = lovasz_loss(est, masks)
        nll = nll_loss(torch.log(est), masks)
        assert lovasz.dtype == torch.float32 and nll.dtype == torch.float32
        data[name + '_probs'], data[name + '_labels'] = probs, labels
        data[name + '_lovasz'], data[name + '_nll'] = np.float32(lovasz.item()), np.float32(nll.item())
        print('%-14s lovasz %.7f  nll %.7f' % (name, lovasz.item(), nll.item()))
    np.savez_compressed(os.path.join(HERE, 'val_loss.npz'), **data)


if __name__ == '__main__':
    main()
