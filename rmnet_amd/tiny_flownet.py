# -*- coding: utf-8 -*-
"""TinyFlowNet on stock PyTorch-ROCm; on a fused channels-last network its ten wide convolutions run
on a HIP kernel (csrc/flow_conv.hip, ``RMNET_FLOW_CONV``: see ``TinyFlowNet._forward``), and with ``RMNET_FLOW_CONV=full`` its four
flow heads and three flow upsamplers as well (csrc/flow_head.hip); with ``RMNET_FLOW_STEM=1`` conv1 and the passes that build its
input run as one launch of csrc/flow_stem.hip.

Mirrors ``models/tiny_flownet.py`` of the reference: same constructor signature, same
``forward(frames) -> [B, N, 2, H, W]`` contract and the same state-dict keys
(``conv1.0.weight`` ... ``upsampled_flow3_to_2.weight``, reference lines 20-82) so that the
``'tflownet'`` entry of a public checkpoint loads unchanged.  The only behavioural change is
that the output buffer is allocated on the input's device (the reference allocates it on the
host and copies every frame back, lines 121-132) -- values are identical.
"""

import os

import torch
import torch.nn.functional as F
from torch import nn

from .helpers import pad_amounts, pad_divide_by


def _conv(c_in, c_out, k, stride=1):
    return nn.Sequential(nn.Conv2d(c_in, c_out, k, stride=stride, padding=k // 2),
                         nn.LeakyReLU(0.1, inplace=True))


def _deconv(c_in, c_out):
    return nn.Sequential(nn.ConvTranspose2d(c_in, c_out, 4, stride=2, padding=1, bias=True),
                         nn.LeakyReLU(0.1, inplace=True))


def _flow_head(c_in):
    return nn.Conv2d(c_in, 2, 3, padding=1, bias=True)


def _flow_up():
    return nn.ConvTranspose2d(2, 2, 4, stride=2, padding=1, bias=False)


# The default follows the bench line: three alternating runs per setting, every 'split' run above every 'miopen' run
# (540.6 - 541.8 against 522.8 - 523.6 frames/s, profiles/r13_a_flow_conv.md).
FLOW_CONV_DEFAULT = 'split'

# The ten layers with 64 or more output channels (93 % of the network's FLOPs)
FLOW_SPLIT_LAYERS = ('conv2', 'conv3', 'conv3_1', 'conv4', 'conv4_1', 'conv5', 'conv5_1', 'deconv4', 'deconv3', 'deconv2')
# channels per pixel of cat4 / cat3 / cat2: 770 / 386 / 194 rounded up to a multiple of 32 (the kernel reads whole 32-channel steps)
_CAT_LD = {4: 800, 3: 416, 2: 224}


def flow_conv_backend():
    """RMNET_FLOW_CONV (A/B switch, read at every call): 'split' (default) -- the ten wide convolutions of a fused, channels-last
    TinyFlowNet run on the split-fp16 HIP kernel; 'full' -- so do they, and the four flow heads and the three flow upsamplers run on
    csrc/flow_head.hip, which leaves conv1 as the network's only library convolution; 'miopen' -- none does."""
    v = os.environ.get('RMNET_FLOW_CONV', FLOW_CONV_DEFAULT).lower()
    if v not in ('split', 'full', 'miopen'):
        raise RuntimeError('RMNET_FLOW_CONV must be split, full or miopen, got %r' % v)
    return v


# conv1 with everything in front of it (two pads, two halvings, the 6-channel cat) and its bias + LeakyReLU in one launch of
# csrc/flow_stem.hip with RMNET_FLOW_STEM=1.  The rule for the default is networks.STEM_DEFAULT's: per-step time in a kernel trace
# below the dispatches it replaces, and every bench run above every run of the parent.  profiles/r23_a_front_ends.md has both
# measurements; the default is still off because tests/test_flow_conv.py::test_the_switch_selects_the_path and
# tests/test_flow_head.py::test_full_leaves_conv1_as_the_only_library_convolution pin conv1 as a library call on the default path
# (as they pin FLOW_CONV_DEFAULT): switching it on goes together with a change of those two tests.
FLOW_STEM_DEFAULT = False


def flow_stem_enabled():
    """RMNET_FLOW_STEM ('0' or '1', read at every call; unset: FLOW_STEM_DEFAULT).  Any other value is a RuntimeError."""
    v = os.environ.get('RMNET_FLOW_STEM')
    if v is None:
        return FLOW_STEM_DEFAULT
    if v.strip() not in ('0', '1'):
        raise RuntimeError("RMNET_FLOW_STEM must be '0' or '1', got %r" % v)
    return v.strip() == '1'


class TinyFlowNet(nn.Module):
    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = cfg
        self.conv1 = _conv(6, 64, 7, 2)
        self.conv2 = _conv(64, 128, 5, 2)
        self.conv3 = _conv(128, 256, 5, 2)
        self.conv3_1 = _conv(256, 256, 3)
        self.conv4 = _conv(256, 512, 3, 2)
        self.conv4_1 = _conv(512, 512, 3)
        self.conv5 = _conv(512, 512, 3, 2)
        self.conv5_1 = _conv(512, 512, 3)
        self.deconv4 = _deconv(512, 256)
        self.deconv3 = _deconv(770, 128)
        self.deconv2 = _deconv(386, 64)
        self.predict_flow5 = _flow_head(512)
        self.predict_flow4 = _flow_head(770)
        self.predict_flow3 = _flow_head(386)
        self.predict_flow2 = _flow_head(194)
        self.upsampled_flow5_to_4 = _flow_up()
        self.upsampled_flow4_to_3 = _flow_up()
        self.upsampled_flow3_to_2 = _flow_up()

    def _forward(self, img0, img1):
        """Flow for one frame pair (reference lines 84-119): pad to /64, halve, encode,
        three refinement levels, x8 bilinear upsample, un-pad.

        After ``fuse_epilogues()``, in eval mode, on CUDA fp32 frames of a channels-last run (the frames or the weights channels-last)
        and unless ``RMNET_FLOW_CONV=miopen``, the ten convolutions of ``FLOW_SPLIT_LAYERS`` run on the split-fp16 kernel
        (csrc/flow_conv.hip) with bias + LeakyReLU in its epilogue, writing straight into the concatenation buffers.  That kernel
        saturates activations outside |x| < 1023.5 and counts them in ``flow_range_word(device)``.  There is no host
        synchronisation here (the call can be captured into a HIP graph): ``forward`` zeroes and checks the word once per clip, a
        streaming caller of ``_forward`` checks ``flow_range_count()`` itself and, when it is non-zero, zeroes the word and redoes
        the frames since its last check with ``RMNET_FLOW_CONV=miopen``.  ``RMNET_FLOW_CONV=full`` runs the flow heads and the flow
        upsamplers on csrc/flow_head.hip as well (plain fp32, no window): conv1 is then the only library convolution.
        Under the same conditions ``RMNET_FLOW_STEM=1`` runs conv1 on csrc/flow_stem.hip, which reads the two frames in place: the
        pads, the halvings, the cat and the bias + LeakyReLU pass are not issued, and the elements of the frame pair outside the
        window are counted in the same word.  Its first call on a device must not come from a capturing stream."""
        if self._flow_stem_ok(img0, img1):
            from . import ops
            pad = pad_amounts(int(img0.shape[2]), int(img0.shape[3]), 64)
            wp, wu = self._flow_stem_pack
            c1 = ops.flow_stem(img0, img1, wp, wu, self.conv1[0].bias, pad=pad,
                               range_word=self.flow_range_word(img0.device))
            return self._unpad(self._refine_split(c1, full=flow_conv_backend() == 'full'), pad)
        (img0, img1), pad = pad_divide_by([img0, img1], 64, img0.shape[2:])
        pair = torch.cat((F.interpolate(img0, scale_factor=0.5, mode='bilinear'),
                          F.interpolate(img1, scale_factor=0.5, mode='bilinear')), dim=1)
        run = self._fused_block if getattr(self, '_fused', False) and not self.training and pair.is_cuda else (lambda m, x: m(x))
        backend = self._flow_split_ok(pair)
        if backend:
            flow2 = self._refine_split(run(self.conv1, pair), full=backend == 'full')
        else:
            c2 = run(self.conv2, run(self.conv1, pair))
            c3 = run(self.conv3_1, run(self.conv3, c2))
            c4 = run(self.conv4_1, run(self.conv4, c3))
            c5 = run(self.conv5_1, run(self.conv5, c4))

            cat4 = torch.cat((c4, run(self.deconv4, c5), self.upsampled_flow5_to_4(self.predict_flow5(c5))), 1)
            cat3 = torch.cat((c3, run(self.deconv3, cat4), self.upsampled_flow4_to_3(self.predict_flow4(cat4))), 1)
            cat2 = torch.cat((c2, run(self.deconv2, cat3), self.upsampled_flow3_to_2(self.predict_flow3(cat3))), 1)
            flow2 = self.predict_flow2(cat2)
        return self._unpad(flow2, pad)

    @staticmethod
    def _unpad(flow2, pad):
        """The x8 bilinear upsample of the 1/8-resolution flow and the crop back to the frame."""
        flow = F.interpolate(flow2, scale_factor=8, mode='bilinear')
        lw, uw, lh, uh = pad
        if lh + uh > 0:
            flow = flow[:, :, lh:flow.shape[2] - uh, :]
        if lw + uw > 0:
            flow = flow[:, :, :, lw:flow.shape[3] - uw]
        return flow

    # ------------------------------------------------------------------------------------------ the split-fp16 path
    def _flow_split_ok(self, pair):
        """'split' or 'full' when the ten wide convolutions run on csrc/flow_conv.hip for this input (the value of RMNET_FLOW_CONV),
        else False: fused with packs on the input's device, eval, CUDA fp32, a channels-last run, RMNET_FLOW_CONV not miopen, and
        not the MIOpen re-run of a clip that left the window."""
        if not getattr(self, '_fused', False) or self.training or getattr(self, '_flow_off', False):
            return False
        packs = getattr(self, '_flow_packs', None)
        if not packs or not (pair.is_cuda and pair.dtype == torch.float32 and packs['conv2'][0].device == pair.device):
            return False
        from .ops import _is_cl
        if not (_is_cl(pair) or _is_cl(self.conv2[0].weight)):
            return False
        backend = flow_conv_backend()
        return backend if backend in ('split', 'full') else False

    def _flow_stem_ok(self, img0, img1):
        """True when conv1 and the passes in front of it run on csrc/flow_stem.hip for this frame pair: RMNET_FLOW_STEM on, the
        conditions of ``_flow_split_ok`` (the ten wide convolutions take the kernel's output), two frames of one shape and a
        biased conv1 with its pack on the frames' device."""
        if not flow_stem_enabled() or img0.dim() != 4 or img0.shape[1] != 3 or img1.shape != img0.shape or img1.dtype != img0.dtype:
            return False
        pack = getattr(self, '_flow_stem_pack', None)
        if pack is None or pack[0].device != img0.device or img1.device != img0.device or self.conv1[0].bias is None:
            return False
        return bool(self._flow_split_ok(img0))

    def _refine_split(self, c1, full=False):
        """conv2 .. predict_flow2 on ``c1`` = conv1's output, the ten wide layers on the HIP kernel.  cat4 / cat3 / cat2 are ONE
        channels-last buffer each (800 / 416 / 224 channels per pixel): conv4_1 / conv3_1 / conv2 write the channels from 0, the
        deconvolutions theirs from 512 / 256 / 128, torch copies the two upsampled-flow channels behind them, and the padding up to
        the next multiple of 32 is zeroed -- so no torch.cat is left.  The flow heads of the three buffers convolve the WHOLE buffer
        with a zero-padded copy of their weight (``fuse_epilogues``): a channel-sliced view would be copied into a dense tensor
        by the library first.  Every buffer is a fresh stream-ordered allocation: nothing is kept between calls, and nothing
        depends on the frame, so the call can be captured.
        ``full``: the flow heads run on csrc/flow_head.hip, which reads the first 512 / 770 / 386 / 194 channels of c5 / cat4 / cat3 /
        cat2 with the heads' own weights (packed), and the upsamplers on its flow_up, which writes the two flow channels at 768 / 384 /
        192 of the next buffer and zeroes the padding behind them: no library call, no copy and no zero fill is left."""
        from . import ops
        word = self.flow_range_word(c1.device)
        self.__dict__['_flow_used'] = 'full' if full else 'split'            # (for ``forward``: a host flag, no synchronisation)

        def fc(name, x, cin=None, out=None, coff=0):
            conv = getattr(self, name)[0]
            wp, wu = self._flow_packs[name]
            tr = isinstance(conv, nn.ConvTranspose2d)
            return ops.flow_conv(x, wp, wu, conv.bias, ksize=conv.kernel_size[0], stride=conv.stride[0], transposed=tr, act='leaky',
                                 cin=cin, out=out, out_coff=coff, range_word=word)

        def buf(level, src):          # the buffer of a level: half the map of the level above (k 5 / pad 2 and k 3 / pad 1, stride 2)
            n, _, h, w = src.shape
            return torch.empty((n, _CAT_LD[level], (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=src.dtype, device=src.device,
                               memory_format=torch.channels_last)

        def tail(cat, real, up):
            cat[:, real - 2:real].copy_(up)           # the upsampled flow, behind the deconvolution's channels
            cat[:, real:].zero_()                     # the padding: finite for the kernel (zero weights), ZERO for the flow head

        def head(level, x, cin):
            return ops.flow_head(x, self._flow_head_packs[level], getattr(self, 'predict_flow%d' % level).bias, cin=cin)

        def up(level, flow, cat, real):               # flow_up writes the two channels and the zero padding behind them
            ops.flow_up(flow, self._flow_up_w[level], cat, real - 2)

        c1 = c1.contiguous(memory_format=torch.channels_last)      # (no copy in a channels-last run)
        cat2 = buf(2, c1)
        fc('conv2', c1, out=cat2)
        cat3 = buf(3, cat2)
        fc('conv3_1', fc('conv3', cat2, cin=128), out=cat3)
        cat4 = buf(4, cat3)
        fc('conv4_1', fc('conv4', cat3, cin=256), out=cat4)
        c5 = fc('conv5_1', fc('conv5', cat4, cin=512))

        if full:
            fc('deconv4', c5, out=cat4, coff=512)
            up(4, head(5, c5, 512), cat4, 770)
            fc('deconv3', cat4, cin=770, out=cat3, coff=256)
            up(3, head(4, cat4, 770), cat3, 386)
            fc('deconv2', cat3, cin=386, out=cat2, coff=128)
            up(2, head(3, cat3, 386), cat2, 194)
            return head(2, cat2, 194)
        fc('deconv4', c5, out=cat4, coff=512)
        tail(cat4, 770, self.upsampled_flow5_to_4(self.predict_flow5(c5)))
        fc('deconv3', cat4, cin=770, out=cat3, coff=256)
        tail(cat3, 386, self.upsampled_flow4_to_3(self._flow_head(4, cat4)))
        fc('deconv2', cat3, cin=386, out=cat2, coff=128)
        tail(cat2, 194, self.upsampled_flow3_to_2(self._flow_head(3, cat3)))
        return self._flow_head(2, cat2)

    def _flow_head(self, level, cat):
        head = getattr(self, 'predict_flow%d' % level)
        return F.conv2d(cat, self._flow_head_w[level], head.bias, 1, 1)

    def flow_range_word(self, device):
        """This network's int32 range word on ``device`` (created on first use: ``fuse_epilogues`` does that for the weights'
        device, outside any graph capture)."""
        words = self.__dict__.setdefault('_flow_range', {})
        idx = torch.device(device).index
        idx = torch.cuda.current_device() if idx is None else idx
        w = words.get(idx)
        if w is None:
            w = words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device('cuda', idx))
        return w

    def flow_range_count(self, device=None):
        """How often the split-fp16 kernel met an activation outside its window since the word was last zeroed (host sync)."""
        device = self.conv1[0].weight.device if device is None else device
        return int(self.flow_range_word(device).item())

    @torch.no_grad()
    def _build_flow_packs(self):
        """The ten weight packs, conv1's pack for csrc/flow_stem.hip, the zero-padded flow-head weights, the four flow-head packs and NCHW-contiguous upsampler weights
        of csrc/flow_head.hip, and the range word: plain attributes (not parameters or buffers, so ``state_dict()`` is untouched),
        rebuilt whenever the parameters move (``_apply``) or are loaded."""
        from . import ops
        packs = {}
        for name in FLOW_SPLIT_LAYERS:
            conv = getattr(self, name)[0]
            packs[name] = ops.flow_conv_pack(conv.weight.detach().float(), transposed=isinstance(conv, nn.ConvTranspose2d))
        heads = {}
        for level, ld in _CAT_LD.items():
            w = getattr(self, 'predict_flow%d' % level).weight.detach()
            heads[level] = F.pad(w, (0, 0, 0, 0, 0, ld - w.shape[1])).contiguous(memory_format=torch.channels_last)
        self.__dict__['_flow_packs'] = packs
        self.__dict__['_flow_stem_pack'] = ops.flow_stem_pack(self.conv1[0].weight.detach().float())
        self.__dict__['_flow_head_w'] = heads
        self.__dict__['_flow_head_packs'] = {level: ops.flow_head_pack(getattr(self, 'predict_flow%d' % level).weight.detach().float())
                                             for level in (5, 4, 3, 2)}
        self.__dict__['_flow_up_w'] = {level: getattr(self, 'upsampled_flow%d_to_%d' % (level + 1, level)).weight.detach().float()
                                       .contiguous().clone() for level in (4, 3, 2)}
        if self.conv1[0].weight.is_cuda:
            self.flow_range_word(self.conv1[0].weight.device)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if getattr(self, '_fused', False):
            self._build_flow_packs()           # (the packs are no buffers: they follow the parameters this way)
        return out

    def load_reference_state_dict(self, state_dict, strict=True):
        """Accepts the reference's checkpoints with or without DataParallel's ``module.`` prefix
        (core/inference.py:33-44)."""
        clean = {(k[7:] if k.startswith('module.') else k): v for k, v in state_dict.items()}
        return self.load_state_dict(clean, strict=strict)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        if getattr(self, '_fused', False):
            self._build_flow_packs()
        return out

    @staticmethod
    def _fused_block(block, x):
        """conv / deconv (+bias) -> LeakyReLU(0.1) with the bias and the activation in ONE pass
        (rmnet_channel_affine_f32, act 2) instead of two elementwise kernels."""
        from . import ops
        conv = block[0]
        if isinstance(conv, nn.ConvTranspose2d):
            t = F.conv_transpose2d(x, conv.weight, None, conv.stride, conv.padding)
        else:
            t = F.conv2d(x, conv.weight, None, conv.stride, conv.padding)
        return ops.channel_affine(t, None, conv.bias, relu='leaky', out=t)

    def fuse_epilogues(self, enable=True):
        """Bias + LeakyReLU of every block as one kernel (parameters untouched), and the weight packs of the ten wide convolutions
        for the split-fp16 kernel and of the flow heads and upsamplers for csrc/flow_head.hip (plain attributes: ``state_dict()`` is
        unchanged; ``RMNET_FLOW_CONV=miopen`` leaves them unused)."""
        self.eval()
        self._fused = bool(enable)
        if self._fused:
            self._build_flow_packs()
        else:
            self.__dict__.pop('_flow_packs', None)
            self.__dict__.pop('_flow_stem_pack', None)
            self.__dict__.pop('_flow_head_w', None)
            self.__dict__.pop('_flow_head_packs', None)
            self.__dict__.pop('_flow_up_w', None)
        return self

    def forward(self, frames, device=None):
        """Flow of every frame of a clip against its predecessor.  With the split-fp16 path on, the range word is zeroed before the
        loop and read once after it; a clip that left the kernel's window is computed again with the kernel off.  ``last_clip`` says
        which path the returned flows come from and what the word held."""
        # (the reference's DataParallel wrapper moves host frames to the GPU, core/inference.py:35-37)
        frames = frames.to(self.conv1[0].weight.device, non_blocking=True)
        if frames.is_cuda:
            self.flow_range_word(frames.device).zero_()
        self.__dict__['_flow_used'] = False
        flows = self._clip(frames)
        split = self.__dict__['_flow_used']          # some frame pair took the split-fp16 path: 'split' or 'full'
        count = self.flow_range_count(frames.device) if split else 0
        if count:
            self.__dict__['_flow_off'] = True
            try:
                flows = self._clip(frames)
            finally:
                self.__dict__['_flow_off'] = False
        self.__dict__['last_clip'] = {'flow_conv': split if split and not count else 'miopen', 'range': count}
        return flows

    def _clip(self, frames):
        b, n, _, h, w = frames.shape
        flows = frames.new_zeros(b, n, 2, h, w)
        for t in range(1, n):
            flows[:, t] = self._forward(frames[:, t], frames[:, t - 1])
        return flows
