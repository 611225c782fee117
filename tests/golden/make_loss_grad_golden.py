# -*- coding: utf-8 -*-
"""Generate tests/golden/loss_grad.npz by running the REFERENCE's own LovaszLoss (models/lovasz_loss.py) and torch.nn.NLLLoss, as
core/train.py sets them up and adds them (line 180), and ``backward()``, on a handful of small clips.

Like make_val_loss_golden.py this runs only where the reference is checked out (REF below); nothing of the reference is copied: its
module is imported in place, fed the clips of tests/loss_grad_ref.py and tests/val_loss_ref.py, and the loss and the gradient it
returns are stored as data.  No test runs this script.

    python tests/golden/make_loss_grad_golden.py
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.dirname(HERE))

import loss_grad_ref as ref  # noqa: E402
import val_loss_ref as vr  # noqa: E402

IGNORE = 255


def cases():
    """(name, tied, probs [N,K,H,W] float32, labels [N,H,W] uint8): 'distinct*' have per class pairwise different errors, so the
    sort has one order; 'tied*' are on a grid of 8 steps (many equal errors, 0 and 1 among them) or flat soft-maxes."""
    rng = np.random.default_rng(34)
    out = []
    for K in (2, 3, 11):
        out.append(('distinct_k%d' % K, False, *ref.distinct_clip(rng, 2, K, 5, 7, 1 << 10)))
    out.append(('distinct_ignored', False, *ref.distinct_clip(rng, 2, 3, 5, 7, 1 << 12, ignore=0.3)))
    out.append(('distinct_one_frame', False, *ref.distinct_clip(rng, 1, 2, 3, 5, 1 << 8)))
    for K in (2, 3, 11):
        out.append(('tied_k%d' % K, True, *vr.grid_clip(rng, 2, K, 5, 7, 8)))
    p, l = vr.softmax_clip(rng, 2, 3, 5, 7, peak=0.0, ignore=0.2)                 # every probability 1 / 3: all errors tie per kind
    out.append(('tied_flat', True, p, l))
    return out


def main():
    sys.path.insert(0, REF)
    from models.lovasz_loss import LovaszLoss
    lovasz_loss = LovaszLoss(ignore_index=IGNORE)
    nll_loss = torch.nn.NLLLoss(ignore_index=IGNORE)
    data = {'names': np.array([c[0] for c in cases()]), 'tied': np.array([c[1] for c in cases()])}
    for name, tied, probs, labels in cases():
        est = torch.from_numpy(probs).permute(1, 0, 2, 3).unsqueeze(0).clone().requires_grad_(True)     # [B, C, F, H, W]
        masks = torch.from_numpy(labels.astype(np.int64)).unsqueeze(0)
        loss = lovasz_loss(est, masks) + nll_loss(torch.log(est), masks)
        loss.backward()
        grad = est.grad.squeeze(0).permute(1, 0, 2, 3).contiguous().numpy()
        assert loss.dtype == torch.float32 and grad.dtype == np.float32 and grad.shape == probs.shape
        data[name + '_probs'], data[name + '_labels'] = probs, labels
        data[name + '_loss'], data[name + '_grad'] = np.float32(loss.item()), grad
        print('%-20s loss %.7f  |grad| max %.4g  non-finite %d' % (name, loss.item(), np.abs(grad[np.isfinite(grad)]).max(),
                                                                  int((~np.isfinite(grad)).sum())))
    np.savez_compressed(os.path.join(HERE, 'loss_grad.npz'), **data)


if __name__ == '__main__':
    main()
