# -*- coding: utf-8 -*-
"""Convolutional sub-networks of RMNet, kept on stock PyTorch-ROCm (MIOpen).

SURVEY.md section 8 row C1: these stacks are *not* part of the hand-written hot path; they
are declared here only so that (a) the host-side mirror in ``rmnet_amd.rmnet`` has something
to feed the HIP kernels with and (b) public RMNet checkpoints load unchanged.  Every module
and parameter name below therefore matches the reference's state-dict keys:

    reference                                       here
    models/rmnet.py:24-48   ResBlock                ResBlock        (downsample/conv1/conv2)
    models/rmnet.py:51-80   EncoderMemory           EncoderMemory   (conv1_m/conv1_o/conv1/bn1/res2-4)
    models/rmnet.py:83-104  EncoderQuery            EncoderQuery    (conv1/bn1/res2-4)
    models/rmnet.py:107-120 Refine                  Refine          (convFS/ResFS/ResMM)
    models/rmnet.py:123-140 Decoder                 Decoder         (convFM/ResMM/RF3/RF2/pred2)
    models/rmnet.py:168-176 KeyValue                KeyValue        (key_conv/value_conv)

The reference takes its trunk from ``torchvision.models.resnet50`` (models/rmnet.py:57,86);
torchvision is not available in this image, so the ResNet-50 stem and stages 1-3 are declared
here with torchvision's parameter names (``conv1/bn1/conv2/bn2/conv3/bn3/downsample.{0,1}``),
stride on the 3x3 convolution (the "v1.5" variant torchvision ships).
"""

import torch
import torch.nn.functional as F
from torch import nn


class _Bottleneck(nn.Module):
    """ResNet-50 bottleneck: 1x1 reduce, 3x3 (carries the stride), 1x1 expand (x4)."""

    def __init__(self, c_in, width, stride, project):
        super().__init__()
        c_out = width * 4
        self.conv1 = nn.Conv2d(c_in, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, c_out, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(c_out)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(c_in, c_out, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(c_out))

    def forward(self, x):
        if getattr(self, '_fused', False) and not self.training and x.is_cuda:
            return self._forward_fused(x)
        skip = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return self.relu(y + skip)

    def _forward_fused(self, x):
        """Same block with BatchNorm(eval) / skip add / ReLU fused into one pass per convolution
        (rmnet_channel_affine_f32): 3 elementwise kernels instead of 7-8.  On a channels-last run every convolution runs on the
        split-fp16 kernel (csrc/conv_split.hip) instead, BatchNorm folded into its pack, shift / skip / ReLU in its epilogue."""
        from . import ops
        if _split_path_ok(self, x, self.conv1, ('full', 'split', 'trunk')):
            x = x.contiguous(memory_format=torch.channels_last)
            rw = ops.conv_range_word(x.device)
            # RMNET_CONV_PRESPLIT: t is read by exactly one later convolution each time, so it exists in split form only
            # (include/rmnet_hip.h): split and counted once, by the epilogue that produces it, not at every tap and Cout tile of its reader
            # The 3x3 classes gained as measured; a 1x1 reader only from PRESPLIT_MIN_CIN_1X1 input channels on (conv3 of layer3).
            # Below that its call is two or four K steps and measured no gain (supposed, not measured: its time is in writing its
            # output), so conv2 hands it fp32 as before
            pre = conv_presplit()
            # (conv1 of a stride-2 block is itself 10 % slower with a split output; with its 3x3 / stride 2 reader the pair is not:
            #  the bench line with those two conv1 on fp32 output was the same, profiles/r17_a_presplit.md)
            t = ops.conv_split(x, self._wp1, self._wu1, self._b1, ksize=1, relu_out=True, range_word=rw, out_presplit=pre)
            t = ops.conv_split(t, self._wp2, self._wu2, self._b2, ksize=3, stride=self.conv2.stride[0], relu_out=True, range_word=rw,
                               out_presplit=pre and self.conv3.in_channels >= PRESPLIT_MIN_CIN_1X1)
            if self.downsample is None:
                return ops.conv_split(t, self._wp3, self._wu3, self._b3, res=x, ksize=1, relu_out=True, range_word=rw)
            d = ops.conv_split(x, self._wpd, self._wud, self._bd, ksize=1, stride=self.downsample[0].stride[0], range_word=rw)
            return ops.conv_split(t, self._wp3, self._wu3, self._b3, res=d, ksize=1, relu_out=True, out=d, range_word=rw)
        t = self.conv1(x)
        ops.channel_affine(t, self._s1, self._b1, relu=True, out=t)
        t = self.conv2(t)
        ops.channel_affine(t, self._s2, self._b2, relu=True, out=t)
        t = self.conv3(t)
        if self.downsample is None:
            return ops.channel_affine(t, self._s3, self._b3, res=x, relu=True, out=t)
        d = self.downsample[0](x)
        return ops.channel_affine(t, self._s3, self._b3, res=d, res_scale=self._sd, res_shift=self._bd,
                                  relu=True, out=t)


def _stage(c_in, width, n_blocks, stride):
    blocks = [_Bottleneck(c_in, width, stride, project=True)]
    blocks += [_Bottleneck(width * 4, width, 1, project=False) for _ in range(n_blocks - 1)]
    return nn.Sequential(*blocks)


class ResNet50Trunk(nn.Module):
    """Stem + layer1..layer3 of ResNet-50 with torchvision attribute names."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = _stage(64, 64, 3, 1)      # 1/4,  256 ch
        self.layer2 = _stage(256, 128, 4, 2)    # 1/8,  512 ch
        self.layer3 = _stage(512, 256, 6, 2)    # 1/16, 1024 ch


def resnet50(pretrained=False):
    """Stand-in for ``torchvision.models.resnet50``; ``pretrained`` is ignored (no network)."""
    return ResNet50Trunk()


class ResBlock(nn.Module):
    """Pre-activation two-conv residual block (models/rmnet.py:24-48)."""

    def __init__(self, indim, outdim=None, stride=1):
        super().__init__()
        outdim = indim if outdim is None else outdim
        self.downsample = None
        if not (indim == outdim and stride == 1):
            self.downsample = nn.Conv2d(indim, outdim, 3, padding=1, stride=stride)
        self.conv1 = nn.Conv2d(indim, outdim, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(outdim, outdim, 3, padding=1)

    def forward(self, x):
        if getattr(self, '_fused', False) and not self.training and x.is_cuda:
            return self._forward_fused(x)
        r = self.conv2(F.relu(self.conv1(F.relu(x))))
        return (x if self.downsample is None else self.downsample(x)) + r

    def _forward_grad(self, x):
        """The block on the differentiable split-fp16 convolutions (``Decoder.device_grad_``): the two launches of the fused path,
        each recorded with its backward.  The skip is read by conv2's epilogue and never written in place."""
        t = _grad_conv(self, '1', self.conv1, x, relu_in=True, relu_out=True)
        return _grad_conv(self, '2', self.conv2, t, res=x)

    def _forward_fused(self, x):
        """Same arithmetic: the convolutions run without bias and one pass adds the bias with the
        ReLU (conv1) or with the skip (conv2) -- 3 elementwise kernels instead of 5.  (Not always
        bit-identical: MIOpen may choose another solver for the bias-free convolution.)"""
        from . import ops
        c1, c2 = self.conv1, self.conv2
        if self.downsample is None and _split_conv_ok(self, x, c1) and _split_conv_ok(self, x, c2):
            # both convolutions on the split-fp16 kernel, pre-activation ReLU / bias / ReLU / skip inside it
            x = x.contiguous(memory_format=torch.channels_last)
            rw = ops.conv_range_word(x.device)
            t = ops.conv3x3_split(x, self._wp1, self._wu1, c1.bias, relu_in=True, relu_out=True, range_word=rw)
            return ops.conv3x3_split(t, self._wp2, self._wu2, c2.bias, res=x, range_word=rw)
        t = F.conv2d(F.relu(x), c1.weight, None, c1.stride, c1.padding)
        ops.channel_affine(t, None, c1.bias, relu=True, out=t)
        r = F.conv2d(t, c2.weight, None, c2.stride, c2.padding)
        if self.downsample is None:
            return ops.channel_affine(r, None, c2.bias, res=x, out=r)
        ds = self.downsample
        d = F.conv2d(x, ds.weight, None, ds.stride, ds.padding)
        return ops.channel_affine(r, None, c2.bias, res=d, res_shift=ds.bias, out=r)


class EncoderMemory(nn.Module):
    """Frame + object mask + other-objects mask -> r4 (models/rmnet.py:51-80)."""

    def __init__(self, trunk_factory=resnet50):
        super().__init__()
        self.conv1_m = nn.Conv2d(1, 64, 7, stride=2, padding=3, bias=False)
        self.conv1_o = nn.Conv2d(1, 64, 7, stride=2, padding=3, bias=False)
        trunk = trunk_factory(pretrained=True)
        self.conv1, self.bn1, self.relu, self.maxpool = trunk.conv1, trunk.bn1, trunk.relu, trunk.maxpool
        self.res2, self.res3, self.res4 = trunk.layer1, trunk.layer2, trunk.layer3

    def forward(self, in_f, in_m, in_o):
        if _split_path_ok(self, in_f, self.conv1, _stem_backends()):
            # the whole stem in one launch of the split-fp16 kernel (csrc/stem.hip): the three sources are read in place (no 5-channel
            # cat), a missing others-mask is an all-zero plane, and the un-pooled activation is never written
            from . import ops
            pooled = ops.stem_split(in_f.contiguous(), in_m.float().contiguous(), None if in_o is None else in_o.float().contiguous(),
                                    self._wp, self._wu, self._b1, range_word=ops.conv_range_word(in_f.device))
            r2 = self.res2(pooled)
            r3 = self.res3(r2)
            return self.res4(r3), r3, r2, None, in_f
        m = in_m.unsqueeze(1).float()
        o = torch.zeros_like(m) if in_o is None else in_o.unsqueeze(1).float()
        if getattr(self, '_fused', False) and not self.training and in_f.is_cuda:
            # conv1(f) + conv1_m(m) + conv1_o(o) is ONE 7x7 convolution over the 5 stacked input
            # channels with the three weights stacked the same way: two convolutions and two
            # full-resolution adds fewer, same sum up to fp32 summation order.
            from . import ops
            c = self.conv1
            t = F.conv2d(torch.cat((in_f, m, o), dim=1), self._w5, None, c.stride, c.padding)
            # bn1 -> relu -> maxpool in one pass; the stem activation c1 itself is not materialised
            # (nothing downstream of the encoders reads it) and is returned as None
            c1, pooled = None, ops.affine_relu_maxpool(t, self._s1, self._b1)
        else:
            c1 = self.relu(self.bn1(self.conv1(in_f) + self.conv1_m(m) + self.conv1_o(o)))
            pooled = self.maxpool(c1)
        r2 = self.res2(pooled)
        r3 = self.res3(r2)
        r4 = self.res4(r3)
        return r4, r3, r2, c1, in_f


class EncoderQuery(nn.Module):
    """Frame -> (r4, r3, r2) (models/rmnet.py:83-104)."""

    def __init__(self, trunk_factory=resnet50):
        super().__init__()
        trunk = trunk_factory(pretrained=True)
        self.conv1, self.bn1, self.relu, self.maxpool = trunk.conv1, trunk.bn1, trunk.relu, trunk.maxpool
        self.res2, self.res3, self.res4 = trunk.layer1, trunk.layer2, trunk.layer3

    def forward(self, in_f):
        if _split_path_ok(self, in_f, self.conv1, _stem_backends()):
            from . import ops
            c1, pooled = None, ops.stem_split(in_f.contiguous(), wpack=self._wp, w_unscale=self._wu, shift=self._b1,
                                              range_word=ops.conv_range_word(in_f.device))      # (csrc/stem.hip: the whole stem)
        elif getattr(self, '_fused', False) and not self.training and in_f.is_cuda:
            from . import ops
            t = self.conv1(in_f)
            c1, pooled = None, ops.affine_relu_maxpool(t, self._s1, self._b1)   # (c1 not materialised)
        else:
            c1 = self.relu(self.bn1(self.conv1(in_f)))
            pooled = self.maxpool(c1)
        r2 = self.res2(pooled)
        r3 = self.res3(r2)
        r4 = self.res4(r3)
        return r4, r3, r2, c1, in_f


class Refine(nn.Module):
    """Skip-feature fusion + x2 bilinear upsample of the coarser map (models/rmnet.py:107-120)."""

    def __init__(self, inplanes, planes, scale_factor=2):
        super().__init__()
        self.convFS = nn.Conv2d(inplanes, planes, 3, padding=1)
        self.ResFS = ResBlock(planes, planes)
        self.ResMM = ResBlock(planes, planes)
        self.scale_factor = scale_factor

    def forward(self, f, pm):
        if _split_conv_ok(self, f, self.convFS):
            from . import ops
            f = f.contiguous(memory_format=torch.channels_last)
            s = ops.conv3x3_split(f, self._wp, self._wu, self.convFS.bias, range_word=ops.conv_range_word(f.device))
            s = self.ResFS(s)
        else:
            s = self.ResFS(self.convFS(f))
        if getattr(self, '_fused', False) and not self.training and s.is_cuda and self.scale_factor == 2:
            from . import ops
            return self.ResMM(ops.upsample2x_add(pm, s, out=s))     # s + up in one pass
        up = F.interpolate(pm, scale_factor=self.scale_factor, mode='bilinear', align_corners=False)
        return self.ResMM(s + up)

    def _forward_grad(self, f, pm):
        """``forward`` under ``Decoder.device_grad_``: the five convolutions differentiable on the device; the x2 upsample and the
        add as plain torch ops, or, with ``glue=True`` and ``scale_factor == 2``, as the recorded ``ops.upsample2x_add`` (one launch
        forward, a gather backward)."""
        s = self.ResFS._forward_grad(_grad_conv(self, '', self.convFS, f))
        if getattr(self, '_glue_grad', False) and self.scale_factor == 2:
            from . import ops
            return self.ResMM._forward_grad(ops.upsample2x_add(pm, s))
        up = F.interpolate(pm, scale_factor=self.scale_factor, mode='bilinear', align_corners=False)
        return self.ResMM._forward_grad(s + up)


class Decoder(nn.Module):
    """[mem | q_val] (1024 ch) + r3 + r2 -> 2-class logits at full resolution
    (models/rmnet.py:123-140)."""

    def __init__(self, mdim):
        super().__init__()
        self.convFM = nn.Conv2d(1024, mdim, 3, padding=1)
        self.ResMM = ResBlock(mdim, mdim)
        self.RF3 = Refine(512, mdim)
        self.RF2 = Refine(256, mdim)
        self.pred2 = nn.Conv2d(mdim, 2, 3, padding=1)

    def device_grad_(self, enable=True, glue=False):
        """Opt in to (or out of) the decoder's gradient on the device.  With the flag set, a call that autograd has to record --
        grad mode on and an input or a decoder parameter requiring grad -- runs the thirteen 256-output 3x3 convolutions through
        the differentiable ``ops.conv3x3_split`` (forward: the split-fp16 kernels; backward: csrc/conv3x3_wgrad.hip and the same
        forward kernel on flipped packs) in ``.train()`` and ``.eval()`` alike (the decoder holds no BatchNorm), provided the packs
        are there (``fuse_epilogues()``), the run is channels-last CUDA fp32 and RMNET_CONV allows the decoder kernels.  The x2
        upsample + add, ``pred2(relu(m2))`` and the x4 upsample are plain torch ops there, unless ``glue=True``: then they are the
        recorded ``ops.upsample2x_add`` (both ``Refine`` modules with ``scale_factor == 2``), ``ops.pred_head`` on the LIVE
        ``pred2.weight`` (a biased 3x3 / stride 1 / pad 1 convolution with two outputs and Cin % 32 == 0; any other ``pred2`` stays
        torch's) and ``ops.upsample4x``, whose backwards are the gathers and the one-pass kernel of csrc/decoder_glue_bwd.hip: the
        decoder is then differentiable on the device end to end, without an atomic add, and two ``backward()`` calls give the same
        bits in every gradient.  ``device_grad_()`` without the flag is what it was.  A convolution's packs follow its
        weight: they are rebuilt when ``weight._version`` has moved (an optimiser step) and cached otherwise -- on this path only:
        before inference with weights that were updated in place, call ``fuse_epilogues()`` again, as ever.  Every other call takes
        the path it took before.  Returns ``self``."""
        for m in self.modules():
            if isinstance(m, (Decoder, Refine, ResBlock)):
                m._device_grad = bool(enable)
                m._glue_grad = bool(enable) and bool(glue)
        return self

    def _grad_path_ok(self, r4, r3, r2):
        if not getattr(self, '_device_grad', False) or not torch.is_grad_enabled():
            return False
        mods = [m for m in self.modules() if isinstance(m, (Decoder, Refine, ResBlock))]
        if not all(getattr(m, '_fused', False) and getattr(m, '_conv_split', False) and getattr(m, '_device_grad', False) for m in mods):
            return False
        if any(isinstance(m, ResBlock) and m.downsample is not None for m in mods):
            return False
        cl = lambda t: t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
        for t, c in ((r4, self.convFM), (r3, self.RF3.convFS), (r2, self.RF2.convFS)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == c.in_channels and (cl(t) or cl(c.weight))):
                return False
        if split_conv_backend() not in ('full', 'split', 'trunk', 'decoder'):
            return False
        from . import ops
        if max(r4.shape[3], r3.shape[3], r2.shape[3]) > ops.WGRAD_MAX_W:      # (the weight gradient's widest map: such inputs keep the old path)
            return False
        return any(t.requires_grad for t in (r4, r3, r2)) or any(p.requires_grad for p in self.parameters())

    def forward(self, r4, r3, r2):
        if self._grad_path_ok(r4, r3, r2):
            m4 = self.ResMM._forward_grad(_grad_conv(self, '', self.convFM, r4))
            m2 = self.RF2._forward_grad(r2, self.RF3._forward_grad(r3, m4))
            if getattr(self, '_glue_grad', False):
                from . import ops
                if _pred_head_shape_ok(self.pred2) and self.pred2.weight.dtype == torch.float32:
                    # (the live weight, not the _wpred copy, which an optimiser step leaves stale; its gradient comes back as a plain
                    #  [2, C, 3, 3] tensor and autograd carries it through contiguous() to the channels-last parameter)
                    p2 = ops.pred_head(m2.contiguous(memory_format=torch.channels_last), self.pred2.weight.contiguous(), self.pred2.bias)
                else:
                    p2 = self.pred2(F.relu(m2)).contiguous()
                return ops.upsample4x(p2)
            p2 = self.pred2(F.relu(m2))
            return F.interpolate(p2.contiguous(), scale_factor=4, mode='bilinear', align_corners=False)
        if _split_conv_ok(self, r4, self.convFM):
            from . import ops
            r4 = r4.contiguous(memory_format=torch.channels_last)      # (the memory read's output is NCHW)
            m4 = self.ResMM(ops.conv3x3_split(r4, self._wp, self._wu, self.convFM.bias, range_word=ops.conv_range_word(r4.device)))
        else:
            m4 = self.ResMM(self.convFM(r4))
        m3 = self.RF3(r3, m4)
        m2 = self.RF2(r2, m3)
        if _pred_head_ok(self, m2):
            # ReLU, the two-channel convolution and the NCHW layout of the tail in one kernel (csrc/pred_head.hip)
            from . import ops
            p2 = ops.pred_head(m2.contiguous(memory_format=torch.channels_last), self._wpred.view(self.pred2.weight.shape), self.pred2.bias)
            return F.interpolate(p2, scale_factor=4, mode='bilinear', align_corners=False)
        p2 = self.pred2(F.relu(m2))
        # (channels-last runs: back to NCHW HERE, on the 2-channel quarter-resolution map -- the decoder tail kernel reads NCHW planes, and
        #  converting after the x4 upsample would move 16x the bytes; a no-op for NCHW tensors)
        return F.interpolate(p2.contiguous(), scale_factor=4, mode='bilinear', align_corners=False)


def _grad_packs(m, suffix, conv, need_x):
    """(wpack, w_unscale, dgrad packs) of ``conv`` (packs ``m._wp<suffix>`` / ``m._wu<suffix>``) for the weight as it is now: the
    forward pack is rebuilt when ``weight._version`` is not the version it was packed from, the dgrad packs (only when the input
    needs a gradient: ``need_x``; Cin % 256 == 0: every decoder convolution) likewise; both are cached otherwise.  ``conv3x3_pack``
    is device-side torch: no synchronisation."""
    from . import ops
    w = conv.weight
    ver = w._version
    if getattr(m, '_wver' + suffix, None) != ver:
        with torch.no_grad():
            wp, wu = ops.conv3x3_pack(w)
        m._buffers['_wp' + suffix], m._buffers['_wu' + suffix] = wp, wu
        setattr(m, '_wver' + suffix, ver)
    if not need_x:
        return getattr(m, '_wp' + suffix), getattr(m, '_wu' + suffix), None
    cache = m.__dict__.setdefault('_dgrad_packs', {})
    ent = cache.get(suffix)
    if ent is None or ent[0] != ver or ent[1] is not w:
        ent = cache[suffix] = (ver, w, ops.conv3x3_dgrad_pack(w))
    return getattr(m, '_wp' + suffix), getattr(m, '_wu' + suffix), ent[2]


def _grad_conv(m, suffix, conv, x, res=None, relu_in=False, relu_out=False):
    """One decoder convolution on the differentiable ``ops.conv3x3_split`` with the packs of ``_grad_packs``."""
    from . import ops
    wp, wu, dp = _grad_packs(m, suffix, conv, x.requires_grad)
    x = x.contiguous(memory_format=torch.channels_last)
    if res is not None:
        res = res.contiguous(memory_format=torch.channels_last)
    return ops.conv3x3_split(x, wp, wu, conv.bias, res=res, relu_in=relu_in, relu_out=relu_out,
                             range_word=ops.conv_range_word(x.device), weight=conv.weight, dgrad_packs=dp)


# The stem and prediction-head kernels become part of the default path ('split') only on a measured win: per-step time in a kernel
# trace below the dispatches they replace, and the bench line not below RMNET_CONV=trunk (profiles/r09_a_stem_head.md).  Measured
# in profiles/r23_a_front_ends.md, per frame step of the bench: the two stem launches 0.61 ms against 1.31 ms for the cat, the two
# library convolutions and the two pool passes; the head 0.15 ms against 0.70 ms for the ReLU, pred2 and the layout copy; every
# bench run with both above every run without.  RMNET_CONV=trunk switches both off.
STEM_DEFAULT = True
HEAD_DEFAULT = True


def _stem_backends():
    return ('full', 'split') if STEM_DEFAULT else ('full',)


def split_conv_backend():
    """RMNET_CONV (A/B switch, read at every call): 'full' -- every convolution of the fused path runs on a HIP kernel: the stems
    (csrc/stem.hip), the trunks, key / value heads and the decoder's 256-channel convolutions on the split-fp16 kernels
    (csrc/conv_split.hip, csrc/conv3x3.hip) and the prediction head (csrc/pred_head.hip); 'trunk' -- all but the stems and the
    prediction head, which stay on MIOpen; 'split' (default) -- 'trunk' plus whichever of the stem / head kernels STEM_DEFAULT /
    HEAD_DEFAULT name; 'decoder' -- only the decoder's 256-channel convolutions; 'miopen' -- none of them."""
    import os
    v = os.environ.get('RMNET_CONV', 'split').lower()
    if v not in ('full', 'split', 'trunk', 'decoder', 'miopen'):
        raise RuntimeError('RMNET_CONV must be full, split, trunk, decoder or miopen, got %r' % v)
    return v


# Whether the trunks' bottlenecks and the key / value heads keep their convolution-to-convolution activations in split form
# (csrc/conv_split.hip: conv_split_pre, split_act) when RMNET_CONV_PRESPLIT is not set.  The rule: on only if every bench run with
# it is above every run without it (profiles/r17_a_presplit.md).
PRESPLIT_DEFAULT = True
# The fewest input channels at which a 1x1 convolution is given its input in split form.  Measured per class (one kernel trace per
# tree, noise +-2 %): Cin 256 (Cout 1024 at 1/16) -5 %; Cin 128 (Cout 512 at 1/8) -2 % and Cin 64 (Cout 256 at 1/4) 0 %, both inside
# the noise, so they keep their fp32 input.
PRESPLIT_MIN_CIN_1X1 = 256


def conv_presplit():
    """RMNET_CONV_PRESPLIT (A/B switch, read at every call): '0' -- every split-fp16 convolution of the trunks and key / value heads
    reads and writes fp32 (the call sequence before the split activation form existed); anything else -- a bottleneck's conv1 output,
    and its conv2 output where conv3 gains from it (PRESPLIT_MIN_CIN_1X1), exist in split form only and KeyValue splits r4 once
    (rmnet_split_act_f32).  Unset: PRESPLIT_DEFAULT.  Same
    results and the same zero / non-zero range word either way."""
    import os
    v = os.environ.get('RMNET_CONV_PRESPLIT')
    return PRESPLIT_DEFAULT if v is None else v.strip() != '0'


def _split_path_ok(m, x, conv, backends, any_mode=False):
    """Module ``m`` may run its convolutions on a split-fp16 kernel for input ``x``: fused epilogues on, packs present and allowed
    (``m._conv_split``), eval (``any_mode``: or training -- for a module without BatchNorm), a CUDA fp32 4-D input with ``conv``'s
    channels in a channels-last run (the input or the network's weights channels-last), and RMNET_CONV one of ``backends``.
    Everything else keeps the MIOpen path."""
    if not (getattr(m, '_fused', False) and getattr(m, '_conv_split', False)) or (m.training and not any_mode):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == conv.in_channels):
        return False
    if not (x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
            or conv.weight.is_contiguous(memory_format=torch.channels_last) and not conv.weight.is_contiguous()):
        return False
    return split_conv_backend() in backends


def _split_conv_ok(m, x, conv):
    """The decoder's split-fp16 convolution (csrc/conv3x3.hip) serves ``conv`` of module ``m`` on input ``x``: ``_split_path_ok``,
    3x3 / stride 1 / pad 1, 256 outputs, Cin % 32 == 0."""
    if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1:
        return False
    return conv.out_channels == 256 and conv.in_channels % 32 == 0 and _split_path_ok(m, x, conv, ('full', 'split', 'trunk', 'decoder'))


def _pred_head_shape_ok(c):
    """``c`` is a convolution the prediction-head kernels implement: 3x3 / stride 1 / pad 1, two biased outputs, Cin % 32 == 0."""
    if c.bias is None or c.out_channels != 2 or c.in_channels % 32:
        return False
    return c.kernel_size == (3, 3) and c.stride == (1, 1) and c.padding == (1, 1) and c.dilation == (1, 1) and c.groups == 1


def _pred_head_ok(m, x):
    """The prediction-head kernel (csrc/pred_head.hip) serves ``m.pred2`` of Decoder ``m`` on input ``x``: ``_split_path_ok`` under
    RMNET_CONV=full (and =split once HEAD_DEFAULT is set), a flat copy of the weight present, 3x3 / stride 1 / pad 1, two biased outputs, Cin % 32 == 0."""
    c = m.pred2
    if getattr(m, '_wpred', None) is None or not _pred_head_shape_ok(c):
        return False
    return _split_path_ok(m, x, c, ('full', 'split') if HEAD_DEFAULT else ('full',))


def split_eligible(conv):
    """``conv`` (an nn.Conv2d) is a shape rmnet_conv_split_f32 implements: fp32, kernel 1x1 or 3x3 with padding k // 2, stride 1 or
    2, no dilation or groups, Cin % 32 == 0, Cout % 64 == 0."""
    k = conv.kernel_size
    return (isinstance(conv, nn.Conv2d) and conv.weight.dtype == torch.float32 and k in ((1, 1), (3, 3))
            and conv.padding == (k[0] // 2, k[0] // 2) and conv.stride in ((1, 1), (2, 2)) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.in_channels % 32 == 0 and conv.out_channels % 64 == 0)


def set_split_conv_(module, enable):
    """Allow (True) or forbid (False) the HIP convolutions (stems, trunks, key / value heads, decoder, prediction head) in
    ``module``'s fused path; returns the previous state of every module touched, for ``restore_split_conv_``."""
    prev = {}
    for m in module.modules():
        if isinstance(m, (_Bottleneck, KeyValue, ResBlock, Refine, Decoder, EncoderMemory, EncoderQuery)):
            # (one flag per module: an encoder's covers its stem (_wp / _wu), a Decoder's covers convFM (_wp / _wu) AND the prediction
            #  head, which has no pack -- _pred_head_ok additionally asks for the flat weight copy _wpred)
            prev[m] = getattr(m, '_conv_split', False)
            m._conv_split = bool(enable) and getattr(m, '_wu', getattr(m, '_wu1', None)) is not None
    return prev


def restore_split_conv_(prev):
    for m, v in prev.items():
        m._conv_split = v


class KeyValue(nn.Module):
    """Two 3x3 heads on r4 (models/rmnet.py:168-176)."""

    def __init__(self, indim, keydim, valdim):
        super().__init__()
        self.key_conv = nn.Conv2d(indim, keydim, 3, padding=1)
        self.value_conv = nn.Conv2d(indim, valdim, 3, padding=1)

    def device_grad_(self, enable=True):
        """Opt in to (or out of) the heads' gradient on the device.  With the flag set, a call that autograd has to record -- grad
        mode on and ``x`` or a head parameter requiring grad -- runs as ``ops._KeyValueFn`` in ``.train()`` and ``.eval()`` alike
        (the module holds no BatchNorm): the forward is the launch of the fused path (dense or regional, the same bits), the
        backward stages each head's gradient with its own scale (``ops.conv_grad_stage_rect``, masked by the rectangles on the
        regional path), takes the weight / bias gradients from ``ops.conv3x3_wgrad`` and the data gradient from ``ops.kv_dgrad`` --
        no atomics, the same bits from two ``backward()`` calls.  Provided the packs are there (``fuse_epilogues()``), the run is
        channels-last CUDA fp32, RMNET_CONV allows the trunk kernels, both heads have a multiple of 128 outputs, Cin % 64 == 0
        and the map is no wider than ``ops.WGRAD_MAX_W``.  The forward pack and the dgrad packs follow ``weight._version`` /
        ``bias._version`` of both convolutions: rebuilt after an optimiser step, cached otherwise -- on this path only: before
        inference with parameters that were updated in place, call ``fuse_epilogues()`` again, as ever.  Every other call takes the
        path it took before.  Returns ``self``."""
        self._device_grad = bool(enable)
        return self

    def _grad_path_ok(self, x):
        if not getattr(self, '_device_grad', False) or not torch.is_grad_enabled():
            return False
        kc, vc = self.key_conv, self.value_conv
        if not _split_path_ok(self, x, kc, ('full', 'split', 'trunk'), any_mode=True):
            return False
        from . import ops
        if kc.out_channels % 128 or vc.out_channels % 128 or kc.in_channels % 64 or x.shape[3] > ops.WGRAD_MAX_W:
            return False
        return x.requires_grad or any(p.requires_grad for p in self.parameters())

    def _grad_packs(self, need_x):
        """(wpack, w_unscale, bias pair, dgrad packs) for the parameters as they are now (see ``device_grad_``)."""
        from . import ops
        kc, vc = self.key_conv, self.value_conv
        params = (kc.weight, vc.weight, kc.bias, vc.bias)
        now = tuple((p, p._version) for p in params)
        same = lambda a, b: a is not None and len(a) == len(b) and all(p is q and v == u for (p, v), (q, u) in zip(a, b))
        if not same(getattr(self, '_kv_ver', None), now):
            with torch.no_grad():
                wp, wu = ops.conv_split_pack(torch.cat((kc.weight, vc.weight)))
                bkv = torch.cat((kc.bias, vc.bias)).contiguous()
            self._buffers['_wp'], self._buffers['_wu'], self._buffers['_bkv'] = wp, wu, bkv
            self._kv_ver = now
        if not need_x:
            return self._wp, self._wu, self._bkv, None
        ent = self.__dict__.get('_kv_dgrad')
        if ent is None or not same(ent[0], now[:2]):
            ent = self.__dict__['_kv_dgrad'] = (now[:2], (ops.conv_split_dgrad_pack(kc.weight), ops.conv_split_dgrad_pack(vc.weight)))
        return self._wp, self._wu, self._bkv, ent[1]

    def forward(self, x, rects=None):
        """(key, value), channels-last.  ``rects`` (int32 [N, 4] on the device, one cell rectangle per image): on the split-fp16 path
        with pre-split activations the heads are computed only inside the rectangles (``ops.conv_split(..., rects=)``) and come back
        NCHW-contiguous, +0.0 outside; on every other path, and for more images than the kernel's tables hold, ``rects`` is not
        looked at and the call is the one without it."""
        if self._grad_path_ok(x):
            from . import ops
            wp, wu, bkv, dp = self._grad_packs(x.requires_grad)
            kc, vc = self.key_conv, self.value_conv
            return ops._KeyValueFn.apply(x.contiguous(memory_format=torch.channels_last), kc.weight, kc.bias, vc.weight, vc.bias,
                                         (wp, wu, bkv, kc.out_channels, dp, conv_presplit()), rects)
        if _split_path_ok(self, x, self.key_conv, ('full', 'split', 'trunk')):
            # both heads in ONE launch of the split-fp16 kernel over the concatenated [key | value] pack, written as two tensors;
            # r4 comes from another kernel: one pass splits it (and counts), instead of 9 taps x 5 Cout tiles doing so
            from . import ops
            return ops.kv_heads(x.contiguous(memory_format=torch.channels_last), self._wp, self._wu, self._bkv,
                                self.key_conv.out_channels, rects, conv_presplit())
        return self.key_conv(x), self.value_conv(x)


def _hash_uniform(n, seed):
    """Exact integer hash (murmur3 finaliser on idx*2654435761 + seed) -> float64 in [-1, 1).
    Pure int64 tensor arithmetic: bit-identical on every torch version / platform."""
    m32 = 0xFFFFFFFF
    x = (torch.arange(n, dtype=torch.int64) * 2654435761 + seed * 40503 + 0x9E3779B9) & m32
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & m32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & m32
    x = x ^ (x >> 16)
    return x.to(torch.float64) * (2.0 / 4294967296.0) - 1.0


def procedural_init_(module, gain=0.9):
    """Deterministic, RNG-free weight fill used for fixtures and benchmarks (no checkpoint is
    reachable offline).  Every tensor is filled from an integer hash of (flat index, state-dict
    key); convolution weights get He scaling x ``gain``, the last conv of every residual branch
    is damped so activations stay O(1) through ResNet-50 with identity BatchNorm statistics."""
    import math
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith('num_batches_tracked'):
                continue
            seed = sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 1000003
            n = t.numel()
            noise = _hash_uniform(n, seed)
            if name.endswith('running_var'):
                val = torch.ones(n, dtype=torch.float64)
            elif name.endswith('running_mean'):
                val = torch.zeros(n, dtype=torch.float64)
            elif t.dim() == 1 and name.endswith('weight'):      # BN gamma
                val = 1.0 + 0.05 * noise
            elif name.endswith('bias'):
                val = 0.05 * noise
            elif t.dim() == 4:
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                if module_is_transposed(module, name):
                    fan_in = t.shape[0] * t.shape[2] * t.shape[3] // 4
                std = gain * math.sqrt(2.0 / max(fan_in, 1))
                if name.endswith('conv3.weight') or name.endswith('conv2.weight') and '.Res' in name:
                    std *= 0.5          # residual-branch output: keep the running sum from doubling
                val = noise * (std * math.sqrt(3.0))
            else:
                val = 0.05 * noise
            t.copy_(val.reshape(t.shape).to(t.dtype))
    return module


def module_is_transposed(module, key):
    mod = module
    for part in key.split('.')[:-1]:
        mod = getattr(mod, part) if not part.isdigit() else mod[int(part)]
    return isinstance(mod, nn.ConvTranspose2d)


# ----------------------------------------------------------------------------------------------
# Inference-time BatchNorm folding (eval mode only).  The reference keeps conv -> BN -> ReLU as three
# kernels (torchvision ResNet-50, models/rmnet.py:66-80, 96-103); in eval mode BN is the affine map
# y = (x - mean) * gamma / sqrt(var + eps) + beta, which folds into the preceding convolution's
# weights and bias.  Mathematically identical, differs only by fp32 rounding (covered by the
# end-to-end parity tests); removes ~2500 BatchNorm launches per 39 frames (6 % of GPU time).
# ----------------------------------------------------------------------------------------------
class _Identity(nn.Module):
    def forward(self, x):
        return x


def _bn_scale_shift(bn):
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def _bn_scale64(bn):
    """The eval BatchNorm's per-channel scale in float64 (what conv_split_pack folds into the weights)."""
    return bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)


def _fold(conv, bn):
    scale, shift = _bn_scale_shift(bn)
    fused = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                      conv.dilation, conv.groups, bias=True).to(conv.weight.device, conv.weight.dtype)
    fused.weight.copy_(conv.weight * scale.view(-1, 1, 1, 1))
    fused.bias.copy_(shift if conv.bias is None else conv.bias * scale + shift)
    return fused


@torch.no_grad()
def fold_batchnorm_(module):
    """Fold every conv->BN pair of the ResNet-50 trunks of ``module`` (an ``RMNet`` or one of its
    encoders) in place.  Call after loading weights, in eval mode.  The state dict of the folded
    module no longer matches the reference's (keep an un-folded copy if you need to save it)."""
    for m in module.modules():
        if isinstance(m, _Bottleneck):
            m.conv1, m.bn1 = _fold(m.conv1, m.bn1), _Identity()
            m.conv2, m.bn2 = _fold(m.conv2, m.bn2), _Identity()
            m.conv3, m.bn3 = _fold(m.conv3, m.bn3), _Identity()
            if m.downsample is not None:
                m.downsample = nn.Sequential(_fold(m.downsample[0], m.downsample[1]), _Identity())
        elif isinstance(m, EncoderQuery) and isinstance(m.bn1, nn.BatchNorm2d):
            m.conv1, m.bn1 = _fold(m.conv1, m.bn1), _Identity()
        elif isinstance(m, EncoderMemory) and isinstance(m.bn1, nn.BatchNorm2d):
            # bn1(conv1(f) + conv1_m(m) + conv1_o(o)): scale all three, shift once
            scale, shift = _bn_scale_shift(m.bn1)
            fused = _fold(m.conv1, m.bn1)
            m.conv1_m.weight.mul_(scale.view(-1, 1, 1, 1))
            m.conv1_o.weight.mul_(scale.view(-1, 1, 1, 1))
            m.conv1, m.bn1 = fused, _Identity()
    return module


# ----------------------------------------------------------------------------------------------
# Fused elementwise epilogues (eval mode, GPU only).  Unlike fold_batchnorm_ this keeps every
# parameter and the state dict untouched: the BatchNorm statistics are only re-expressed as a
# per-channel (scale, shift) pair held in non-persistent buffers, and the forward passes of
# _Bottleneck / ResBlock / the encoder stems call rmnet_channel_affine_f32 once per convolution
# instead of BatchNorm -> add -> ReLU (or bias -> ReLU / bias -> add) as separate kernels.
# ----------------------------------------------------------------------------------------------
@torch.no_grad()
def fuse_epilogues_(module, enable=True):
    """Switch ``module`` (an ``RMNet`` or any sub-module) to the fused elementwise path; call after
    loading weights, in eval mode.  ``enable=False`` switches back."""
    def put(m, name, t):
        if name in m._buffers:
            m._buffers[name] = t
        else:
            m.register_buffer(name, t, persistent=False)

    if enable and any(isinstance(m, _Identity) for m in module.modules()):
        raise RuntimeError('fuse_epilogues() after fuse_for_inference(): the BatchNorms are already folded into '
                           'the convolutions -- use one or the other')
    def snapshot(m):
        """(Re)compute the (scale, shift) pairs / the stacked stem of ONE module from its current parameters."""
        if isinstance(m, _Bottleneck):
            for i, bn in ((1, m.bn1), (2, m.bn2), (3, m.bn3)):
                sc, sh = _bn_scale_shift(bn)
                put(m, '_s%d' % i, sc.contiguous())
                put(m, '_b%d' % i, sh.contiguous())
            if m.downsample is not None:
                sc, sh = _bn_scale_shift(m.downsample[1])
                put(m, '_sd', sc.contiguous())
                put(m, '_bd', sh.contiguous())
            # packed split-fp16 weights with the BatchNorm scale folded in (csrc/conv_split.hip); 1-D, so .to(memory_format=...)
            # leaves them.  The shifts are the _b* above.
            from . import ops
            convs = [('1', m.conv1, m.bn1), ('2', m.conv2, m.bn2), ('3', m.conv3, m.bn3)]
            if m.downsample is not None:
                convs.append(('d', m.downsample[0], m.downsample[1]))
            ok = all(split_eligible(c) for _, c, _ in convs)
            for suffix, c, bn in convs:
                wp, wu = ops.conv_split_pack(c.weight, _bn_scale64(bn)) if ok else (None, None)
                put(m, '_wp' + suffix, wp)
                put(m, '_wu' + suffix, wu)
            m._conv_split = ok and enable
        elif isinstance(m, KeyValue):
            from . import ops
            kc, vc = m.key_conv, m.value_conv
            ok = (split_eligible(kc) and split_eligible(vc) and kc.kernel_size == vc.kernel_size == (3, 3)
                  and kc.stride == vc.stride == (1, 1) and kc.in_channels == vc.in_channels
                  and kc.bias is not None and vc.bias is not None)
            wp = wu = bkv = None
            if ok:
                wp, wu = ops.conv_split_pack(torch.cat((kc.weight, vc.weight)))
                bkv = torch.cat((kc.bias, vc.bias)).contiguous()
            put(m, '_wp', wp)
            put(m, '_wu', wu)
            put(m, '_bkv', bkv)
            # (KeyValue.device_grad_: the packs follow the parameters)
            m._kv_ver = tuple((p, p._version) for p in (kc.weight, vc.weight, kc.bias, vc.bias)) if ok else None
            m._conv_split = ok and enable
        elif isinstance(m, (EncoderMemory, EncoderQuery)):
            sc, sh = _bn_scale_shift(m.bn1)
            put(m, '_s1', sc.contiguous())
            put(m, '_b1', sh.contiguous())
            if isinstance(m, EncoderMemory):
                put(m, '_w5', torch.cat((m.conv1.weight, m.conv1_m.weight, m.conv1_o.weight), dim=1).contiguous())
            # packed split-fp16 stem (csrc/stem.hip), the BatchNorm scale folded in; the shift is _b1.  _w5 / _s1 stay for the MIOpen path
            from . import ops
            w = m._w5 if isinstance(m, EncoderMemory) else m.conv1.weight
            ok = w.dtype == torch.float32 and tuple(w.shape) in ((64, 3, 7, 7), (64, 5, 7, 7)) and m.conv1.stride == (2, 2) \
                and m.conv1.padding == (3, 3) and isinstance(m.bn1, nn.BatchNorm2d)
            wp, wu = ops.stem_pack(w, _bn_scale64(m.bn1)) if ok else (None, None)
            put(m, '_wp', wp)
            put(m, '_wu', wu)
            m._conv_split = ok and enable
        elif isinstance(m, (ResBlock, Refine, Decoder)):
            # packed split-fp16 weights of the 256-channel 3x3 convolutions (csrc/conv3x3.hip); 1-D, so .to(memory_format=...) leaves them
            from . import ops
            convs = {ResBlock: (('1', 'conv1'), ('2', 'conv2')), Refine: (('', 'convFS'),), Decoder: (('', 'convFM'),)}[type(m)]
            ok = True
            for suffix, name in convs:
                c = getattr(m, name)
                if c.out_channels == 256 and c.in_channels % 32 == 0 and c.kernel_size == (3, 3) \
                        and c.weight.dtype == torch.float32:
                    wp, wu = ops.conv3x3_pack(c.weight)
                else:
                    wp, wu, ok = None, None, False
                put(m, '_wp' + suffix, wp)
                put(m, '_wu' + suffix, wu)
                setattr(m, '_wver' + suffix, c.weight._version)      # (Decoder.device_grad_: the packs follow the weight)
            if isinstance(m, Decoder):
                # the prediction head (csrc/pred_head.hip) reads the plain fp32 weight: a flat NCHW copy, which .to(memory_format=...) leaves
                put(m, '_wpred', m.pred2.weight.detach().contiguous().view(-1).clone() if m.pred2.weight.dtype == torch.float32 else None)
            m._conv_split = ok and enable

    def _refresh(mod, incompatible):
        # load_state_dict() runs the post hooks of EVERY module it descends into, so a hook on each snapshot owner
        # covers net.load_state_dict(...) as well as net.encoder_query.load_state_dict(...) or a single block's.
        # (Editing a parameter in place is not observable: call fuse_epilogues() again after doing that.)
        if getattr(mod, '_fused', False):
            with torch.no_grad():
                snapshot(mod)

    for m in module.modules():
        if isinstance(m, (_Bottleneck, KeyValue, EncoderMemory, EncoderQuery, ResBlock, Refine, Decoder)):
            m._fused = bool(enable)
            snapshot(m)
            handle = getattr(m, '_fuse_hook', None)
            if enable and handle is None:
                m._fuse_hook = m.register_load_state_dict_post_hook(_refresh)
            elif not enable and handle is not None:
                handle.remove()
                m._fuse_hook = None
            m._fused = bool(enable)
    return module
