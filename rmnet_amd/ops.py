# -*- coding: utf-8 -*-
"""Torch-facing wrappers over the C ABI.  PyTorch is plumbing here (device memory, current stream,
current device); all arithmetic happens in librmnet_hip.so.

Input validation mirrors the reference's pybind layer
(extensions/reg_att_map_generator/reg_att_map_generator_cuda.cpp:14-19: CUDA + contiguous, else
RuntimeError) and additionally checks dtype, which the reference only assumes.
"""

import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib


MR_FORCE_GENERIC = 1     # include/rmnet_hip.h RMNET_MR_*
MR_EXACT_FP32 = 2
BANK_MAX_SLOTS = 2048    # csrc/bank.hip, csrc/memory_read.hip kMaxT: frames per LAUNCH (longer banks are read in chunks)


def _check(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor' % name)      # CHECK_CUDA
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)          # CHECK_CONTIGUOUS
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))


def _is_cl(t):
    """True for a 4-D tensor that is channels-last in memory ([N,H,W,C]) and NOT also plain-contiguous (C == 1 or H == W == 1 are both)."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def _check_act(t, name):
    """An activation of the glue kernels: fp32, CUDA, NCHW-contiguous or channels-last."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor' % name)
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be torch.float32, got %s' % (name, t.dtype))
    if not (t.is_contiguous() or _is_cl(t)):
        raise RuntimeError('%s must be contiguous (NCHW) or channels-last' % name)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ws(nbytes, dev):
    # the caching allocator makes this a pointer bump; stream-ordered like any torch temporary
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def region_map(mask, prob_threshold=0.5, n_pts_threshold=10, n_bbox_loose_pixels=64,
               want_map=True, cell_grid=None, flow=None, want_warped=False):
    """mask [B,K,H,W] f32 cuda -> (att_map [B,K,H,W] f32 | None, bboxes [B,K,4] i32, rects | None).

    ``cell_grid = (pad_l, pad_t, stride, cells_h, cells_w)`` additionally returns the boxes as cell
    rectangles on the 1/stride feature grid (see include/rmnet_hip.h).
    ``flow`` [B,2,H,W]: the boxes are those of the flow-warped mask (RMNet.get_att_map with a flow,
    models/rmnet.py:252-287), computed without materialising it; with ``want_warped`` the warped mask
    (channels 1..K-1; channel 0 is zero) is returned as a fourth value."""
    _check(mask, 'mask')
    if mask.dim() != 4:
        raise RuntimeError('mask must be [B, K, H, W]')
    if flow is not None:
        return _region_map_warped(mask, flow, prob_threshold, n_pts_threshold, n_bbox_loose_pixels,
                                  want_map, cell_grid, want_warped)
    if want_warped:
        raise RuntimeError('want_warped needs a flow')
    lib = _lib.load()
    B, K, H, W = mask.shape
    dev = mask.device
    with torch.cuda.device(dev):
        att = torch.empty_like(mask) if want_map else None
        bboxes = torch.empty(B, K, 4, dtype=torch.int32, device=dev)
        rects = torch.empty(B, K, 4, dtype=torch.int32, device=dev) if cell_grid is not None else None
        pl, pt, st, ch, cw = cell_grid if cell_grid is not None else (0, 0, 16, 1, 1)
        nb = lib.rmnet_region_map_workspace_bytes(B, K, H, W)
        ws = _ws(nb, dev)
        rc = lib.rmnet_region_map_f32(_ptr(mask), B, K, H, W, float(prob_threshold),
                                      int(n_pts_threshold), int(n_bbox_loose_pixels), _ptr(att),
                                      _ptr(bboxes), _ptr(rects), int(pl), int(pt), int(st), int(ch),
                                      int(cw), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, 'rmnet_region_map_f32')
    return att, bboxes, rects


def _region_map_warped(mask, flow, prob_threshold, n_pts_threshold, n_bbox_loose_pixels, want_map,
                       cell_grid, want_warped):
    _check(flow, 'flow')
    B, K, H, W = mask.shape
    if tuple(flow.shape) != (B, 2, H, W):
        raise RuntimeError('flow must be [B, 2, H, W]')
    lib = _lib.load()
    dev = mask.device
    with torch.cuda.device(dev):
        att = torch.empty_like(mask) if want_map else None
        bboxes = torch.empty(B, K, 4, dtype=torch.int32, device=dev)
        rects = torch.empty(B, K, 4, dtype=torch.int32, device=dev) if cell_grid is not None else None
        warped = torch.zeros_like(mask) if want_warped else None
        pl, pt, st, ch, cw = cell_grid if cell_grid is not None else (0, 0, 16, 1, 1)
        nb = lib.rmnet_region_map_workspace_bytes(B, K, H, W)
        ws = _ws(nb, dev)
        rc = lib.rmnet_region_map_warped_f32(_ptr(mask), _ptr(flow), B, K, H, W, float(prob_threshold),
                                             int(n_pts_threshold), int(n_bbox_loose_pixels), _ptr(att),
                                             _ptr(bboxes), _ptr(rects), int(pl), int(pt), int(st),
                                             int(ch), int(cw), _ptr(warped), _ptr(ws), ws.numel(),
                                             _stream(dev))
    _lib.check(rc, 'rmnet_region_map_warped_f32')
    return (att, bboxes, rects, warped) if want_warped else (att, bboxes, rects)


def boxes_to_cell_rects(bboxes, pad_l, pad_t, stride, cells_h, cells_w, k_per_batch=0):
    """bboxes [..., 4] i32 cuda -> cell rectangles, same shape.  ``k_per_batch`` > 0 marks every
    k-th box (channel 0) as empty."""
    _check(bboxes, 'bboxes', torch.int32)
    lib = _lib.load()
    dev = bboxes.device
    out = torch.empty_like(bboxes)
    with torch.cuda.device(dev):
        rc = lib.rmnet_boxes_to_cell_rects_i32(_ptr(bboxes), bboxes.numel() // 4, int(k_per_batch),
                                               int(pad_l), int(pad_t), int(stride), int(cells_h),
                                               int(cells_w), _ptr(out), _stream(dev))
    _lib.check(rc, 'rmnet_boxes_to_cell_rects_i32')
    return out


def _check_read_args(m_key, m_val, q_key, q_val, mem_rects, qry_rects, T):
    """The argument rules shared by memory_read and memory_read_backward; returns (no, De, Do, Tcap, T, h, w)."""
    for t, n in ((m_key, 'm_key'), (m_val, 'm_val'), (q_key, 'q_key'), (q_val, 'q_val')):
        _check(t, n)
    if m_key.dim() != 5 or m_val.dim() != 5 or q_key.dim() != 4 or q_val.dim() != 4:
        raise RuntimeError('expected m_key/m_val [no,C,T,h,w] and q_key/q_val [no,C,h,w]')
    no, De, Tcap, h, w = m_key.shape
    Do = m_val.shape[1]
    if (m_val.shape[0], m_val.shape[2], m_val.shape[3], m_val.shape[4]) != (no, Tcap, h, w) or \
            tuple(q_key.shape) != (no, De, h, w) or tuple(q_val.shape) != (no, Do, h, w):
        raise RuntimeError('memory/query shapes do not agree')
    T = Tcap if T is None else int(T)
    if not 1 <= T <= Tcap:
        raise RuntimeError('T must be in [1, %d]' % Tcap)
    if (mem_rects is None) != (qry_rects is None):
        raise RuntimeError('mem_rects and qry_rects must be given together')
    if mem_rects is not None:
        _check(mem_rects, 'mem_rects', torch.int32)
        _check(qry_rects, 'qry_rects', torch.int32)
        if mem_rects.numel() != no * T * 4 or qry_rects.numel() != no * 4:
            raise RuntimeError('mem_rects must be [no,T,4] and qry_rects [no,4]')
    return no, De, Do, Tcap, T, h, w


def memory_read_backward(m_key, m_val, q_key, q_val, mem_val, grad_mem_val, mem_rects=None, qry_rects=None, T=None,
                         need=(True, True, True, True)):
    """Gradients of ``memory_read`` (csrc/memory_read_bwd.hip): fp32 MFMA kernels that recompute the soft-max from per-query
    statistics, so the result is the gradient of the exact function whatever arithmetic produced ``mem_val``.

    The first four arguments, the rectangles and ``T`` are the forward's; ``mem_val`` is its output and ``grad_mem_val`` the
    gradient that arrives, both [no,2*Do,h,w].  ``need`` = which of (d m_key, d m_val, d q_key, d q_val) to compute; the others
    come back as None.  With fewer frames read than the memory holds (T < Tcap) the frames beyond T get a zero gradient.
    Deterministic: no atomics, equal bits from call to call."""
    no, De, Do, Tcap, T, h, w = _check_read_args(m_key, m_val, q_key, q_val, mem_rects, qry_rects, T)
    for t, n in ((mem_val, 'mem_val'), (grad_mem_val, 'grad_mem_val')):
        _check(t, n)
        if tuple(t.shape) != (no, 2 * Do, h, w):
            raise RuntimeError('%s must be [no, 2*Do, h, w]' % n)
    need = tuple(bool(x) for x in need)
    if len(need) != 4 or not any(need):
        raise RuntimeError('need must name at least one of the four gradients')
    lib = _lib.load()
    dev = m_key.device
    with torch.cuda.device(dev):
        new = torch.empty_like if T == Tcap else torch.zeros_like       # (frames >= T are not written by the kernels)
        d_mk = new(m_key) if need[0] else None
        d_mv = new(m_val) if need[1] else None
        d_qk = torch.empty_like(q_key) if need[2] else None
        d_qv = torch.empty_like(q_val) if need[3] else None
        ws = _ws(lib.rmnet_memory_read_backward_workspace_bytes(no, De, Do, T, h, w), dev)
        cs = Tcap * h * w
        rc = lib.rmnet_memory_read_backward_f32(_ptr(m_key), _ptr(m_val), _ptr(q_key), _ptr(q_val), no, De, Do, T, h, w,
                                                cs, cs * De, cs, cs * Do, _ptr(mem_val), _ptr(grad_mem_val), _ptr(mem_rects),
                                                _ptr(qry_rects), _ptr(d_mk), _ptr(d_mv), _ptr(d_qk), _ptr(d_qv), _ptr(ws), ws.numel(),
                                                _stream(dev))
    _lib.check(rc, 'rmnet_memory_read_backward_f32')
    return d_mk, d_mv, d_qk, d_qv


class _MemoryReadFn(torch.autograd.Function):
    """memory_read under autograd: the forward is the call every other caller makes, the backward is memory_read_backward."""

    @staticmethod
    def forward(ctx, m_key, m_val, q_key, q_val, mem_rects, qry_rects, want_p, flags, T, events):
        mem_val, p = memory_read(m_key.detach(), m_val.detach(), q_key.detach(), q_val.detach(), mem_rects, qry_rects, want_p, flags, T,
                                 None, events)
        ctx.save_for_backward(m_key, m_val, q_key, q_val, mem_val)
        ctx.rects = (mem_rects, qry_rects)
        ctx.T = T
        if p is None:
            return mem_val, None
        ctx.mark_non_differentiable(p)
        return mem_val, p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_mem_val, _grad_p):
        m_key, m_val, q_key, q_val, mem_val = ctx.saved_tensors
        grads = memory_read_backward(m_key, m_val, q_key, q_val, mem_val, grad_mem_val.contiguous(), ctx.rects[0], ctx.rects[1], ctx.T,
                                     need=ctx.needs_input_grad[:4])
        return grads + (None,) * 6


def memory_read(m_key, m_val, q_key, q_val, mem_rects=None, qry_rects=None, want_p=False, flags=0,
                T=None, out=None, events=None):
    """Fused (regional) memory read.

    m_key [no,De,Tcap,h,w], m_val [no,Do,Tcap,h,w] (only the first ``T`` frames are read; default
    all), q_key [no,De,h,w], q_val [no,Do,h,w]; optional mem_rects [no,T,4] / qry_rects [no,4] i32.
    ``events`` = (ev_start, ev_mid, ev_end) raw hipEvent_t handles (ints) recorded around the two
    kernels of the fast path (profiling only).
    Returns (mem_val [no,2*Do,h,w], p [no,T*h*w,h*w] | None).

    Differentiable in its four float inputs: when grad mode is on and one of them requires grad, the call is recorded as one
    ``torch.autograd.Function`` whose backward is ``memory_read_backward`` -- the gradient of the exact function, whatever
    ``flags`` the forward ran with.  ``p`` is not differentiable, there is no double backward, and ``out=`` cannot be combined
    with a gradient.  Every other call takes the plain path."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (m_key, m_val, q_key, q_val)):
        if out is not None:
            raise RuntimeError('memory_read: out= cannot be used when a gradient is needed')
        _check_read_args(m_key, m_val, q_key, q_val, mem_rects, qry_rects, T)
        return _MemoryReadFn.apply(m_key, m_val, q_key, q_val, mem_rects, qry_rects, want_p, flags, T, events)
    no, De, Do, Tcap, T, h, w = _check_read_args(m_key, m_val, q_key, q_val, mem_rects, qry_rects, T)
    lib = _lib.load()
    dev = m_key.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(no, 2 * Do, h, w, dtype=torch.float32, device=dev)
        else:
            _check(out, 'out')
        p = torch.empty(no, T * h * w, h * w, dtype=torch.float32, device=dev) if want_p else None
        nb = lib.rmnet_memory_read_workspace_bytes(no, De, Do, T, h, w, int(flags))
        ws = _ws(nb, dev)
        cs = Tcap * h * w
        ev = [ctypes.c_void_p(e) if e else None for e in (events or (None, None, None))]
        rc = lib.rmnet_memory_read_f32_ev(_ptr(m_key), _ptr(m_val), _ptr(q_key), _ptr(q_val), no, De, Do,
                                          T, h, w, cs, cs * De, cs, cs * Do, _ptr(out), _ptr(p),
                                          _ptr(mem_rects), _ptr(qry_rects), int(flags), _ptr(ws),
                                          ws.numel(), _stream(dev), ev[0], ev[1], ev[2])
    _lib.check(rc, 'rmnet_memory_read_f32')
    return out, p


BANK_F16 = 4                      # include/rmnet_hip.h: RMNET_BANK_F16 (== RMNET_MR_F16)
MR_F16 = 4
BANK_QX = 8                       # RMNET_BANK_QX (== RMNET_MR_QX)
MR_QX = 8
_PRECISION_FLAGS = {'split': 0, 'f16': BANK_F16, 'qx': BANK_QX}


def _precision(p):
    """'split': K, V, q and P enter the MFMAs as fp16 hi/lo pairs, three terms, fp32-class accuracy (default).
    'f16': hi planes only -- fp16 operands, fp32 accumulate, about 2^-11 relative (include/rmnet_hip.h).
    'qx': 'f16' with the query as a hi/lo pair (its rounding is the logit error that does not average out)."""
    if p not in _PRECISION_FLAGS:
        raise ValueError("precision must be 'split', 'qx' or 'f16'")
    return p


def _loop_precision(p):
    """Arithmetic of the frame loop's bank read: 'auto' (default), 'split', 'qx' or 'f16' -- see RMNet.__init__ and
    profiles/r05_iou_calibration.md for what 'auto' picks and why."""
    if p not in ('auto', 'split', 'qx', 'f16'):
        raise ValueError("read_precision must be 'auto', 'split', 'qx' or 'f16'")
    return p


class MemoryBank:
    """Device-resident regional memory of one clip: ``no`` objects x ``capacity`` frame slots on an
    h x w feature grid (csrc/bank.hip).  ``append`` writes a slot from the un-masked KeyValue outputs
    and the frame's cell rectangles; ``read`` runs the fused regional read over the first T slots."""

    def __init__(self, no, capacity, h, w, device, precision='split'):
        lib = _lib.load()
        self.no, self.capacity, self.h, self.w = int(no), int(capacity), int(h), int(w)
        self.device = torch.device(device)
        self.precision = _precision(precision)        # arithmetic of ``read``: 'split' (fp32-class, default), 'qx' or 'f16'
        nb = lib.rmnet_bank_bytes(self.no, self.capacity, self.h, self.w)
        if nb == 0:
            raise RuntimeError('invalid bank geometry')
        with torch.cuda.device(self.device):
            self.blob = torch.zeros(nb, dtype=torch.uint8, device=self.device)
            # device-resident copy of `committed`: stage() / read_staged() hand it to the kernels, so a captured HIP graph
            # of the frame step stays valid while the memory grows (rmnet_bank_*_at in include/rmnet_hip.h)
            self.n_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.committed = 0

    def append(self, slot, k4, v4, rects=None):
        _check(k4, 'k4')
        _check(v4, 'v4')
        if tuple(k4.shape) != (self.no, 128, self.h, self.w) or tuple(v4.shape) != (self.no, 512, self.h, self.w):
            raise RuntimeError('k4/v4 must be [no,128,h,w] / [no,512,h,w]')
        if rects is not None:
            _check(rects, 'rects', torch.int32)
            if rects.numel() != self.no * 4:
                raise RuntimeError('rects must be [no,4]')
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.rmnet_bank_append_f32(_ptr(self.blob), self.no, self.capacity, self.h, self.w, int(slot),
                                           _ptr(k4), _ptr(v4), _ptr(rects), _stream(self.device))
        _lib.check(rc, 'rmnet_bank_append_f32')

    def areas(self):
        """[no, capacity] int32 view of the per-slot cell counts kept in the blob (debug / accounting only)."""
        off = _lib.load().rmnet_bank_area_offset(self.no, self.capacity, self.h, self.w)
        return self.blob[off:off + self.no * self.capacity * 4].view(torch.int32).view(self.no, self.capacity)

    def overflow_count(self):
        """Number of 16-byte groups appended so far that held an element outside the bank's fp16
        window (|x| >= 1023.5, NaN, Inf; include/rmnet_hip.h).  Synchronises the stream -- call it once
        per clip, not per frame.  Non-zero = the read-outs of this bank are not trustworthy."""
        off = _lib.load().rmnet_bank_overflow_offset(self.no, self.capacity, self.h, self.w)
        return int(self.blob[off:off + 4].view(torch.int32).item())

    def timeout_count(self):
        """Merges of a read that gave up waiting for another workgroup's partial (the int32 behind the overflow word).  Always 0
        on a healthy device; a non-zero value also sets a sticky bit in the overflow word.  Synchronises the stream."""
        off = _lib.load().rmnet_bank_overflow_offset(self.no, self.capacity, self.h, self.w)
        return int(self.blob[off + 4:off + 8].view(torch.int32).item())

    def status(self):
        """(overflow word, merge time-outs, largest logit so far) in ONE device-to-host copy -- what the frame loop checks once per clip."""
        off = _lib.load().rmnet_bank_overflow_offset(self.no, self.capacity, self.h, self.w)
        w = self.blob[off:off + 12].cpu()
        return int(w[0:4].view(torch.int32).item()), int(w[4:8].view(torch.int32).item()), float(w[8:12].view(torch.float32).item()) * 0.6931471805599453

    def logit_max(self):
        """Largest affinity logit (natural units, S = k . q / sqrt(128): models/rmnet.py:155-157) any read of this bank has used as a
        soft-max reference so far -- the kernel's deferred reference, i.e. a lower bound within 8 of the true maximum (include/rmnet_hip.h,
        "logit word").  Synchronises the stream: once per clip."""
        off = _lib.load().rmnet_bank_overflow_offset(self.no, self.capacity, self.h, self.w)
        return float(self.blob[off + 8:off + 12].view(torch.float32).item()) * 0.6931471805599453

    def assert_synced(self):
        """Debug aid: the host mirror ``committed`` and the device counter ``n_dev`` agree (they only move together in
        ``commit``; a captured ``frame_step(commit=True)`` or a foreign write to either would desynchronise them silently --
        the kernels flag an out-of-range slot in the overflow word, an in-range wrong slot only this check finds).  Synchronises."""
        n = int(self.n_dev.item())
        if n != self.committed:
            raise RuntimeError('MemoryBank: device frame counter %d != host counter %d' % (n, self.committed))

    def stage(self, k4, v4, rects):
        """Write one frame into the first free slot without committing it (the tentative previous
        frame of models/rmnet.py:416-426).  Returns the number of frames visible to ``read``.  The slot index
        travels as the device counter ``n_dev`` (graph-replayable); ``committed`` mirrors it on the host."""
        if self.committed >= self.capacity:
            raise RuntimeError('memory bank overflow (%d slots)' % self.capacity)
        _check(k4, 'k4')
        _check(v4, 'v4')
        if tuple(k4.shape) != (self.no, 128, self.h, self.w) or tuple(v4.shape) != (self.no, 512, self.h, self.w):
            raise RuntimeError('k4/v4 must be [no,128,h,w] / [no,512,h,w]')
        if rects is not None:
            _check(rects, 'rects', torch.int32)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.rmnet_bank_append_f32_at(_ptr(self.blob), self.no, self.capacity, self.h, self.w, 0, _ptr(self.n_dev),
                                              _ptr(k4), _ptr(v4), _ptr(rects), _stream(self.device))
        _lib.check(rc, 'rmnet_bank_append_f32_at')
        return self.committed + 1

    def commit(self):
        """Keep the staged frame: one-element add on the device counter (after the read that used it as tentative).  Not inside
        a graph capture: the host mirror would advance once, the device counter on every replay."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('MemoryBank.commit() inside a HIP graph capture: commit between replays (RMNet.forward does)')
        self.committed += 1
        self.n_dev += 1

    def read_staged(self, q_key, q_val, qry_rects=None, out=None, events=None, ws=None):
        """``read(committed + 1, ...)`` with the frame count taken from the device counter (committed frames + the
        staged one): the call a captured graph replays.  A bank of more than 2048 slots is read in chunks planned on the
        host (csrc/memory_read.hip: launch_bank_read), so there the host's own count is used."""
        if self.capacity > BANK_MAX_SLOTS:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('MemoryBank.read_staged() of a bank of more than %d slots inside a HIP graph capture: the chunked '
                                   'read is planned on the host, a replay would keep reading the frame count of the capture' % BANK_MAX_SLOTS)
            return self.read(self.committed + 1, q_key, q_val, qry_rects, out=out, events=events, ws=ws)
        return self.read(1, q_key, q_val, qry_rects, out=out, events=events, ws=ws, _t_dev=self.n_dev)

    def read(self, T, q_key, q_val, qry_rects=None, out=None, events=None, ws=None, _t_dev=None):
        _check(q_key, 'q_key')
        _check(q_val, 'q_val')
        if tuple(q_key.shape) != (self.no, 128, self.h, self.w) or tuple(q_val.shape) != (self.no, 512, self.h, self.w):
            raise RuntimeError('q_key/q_val must be [no,128,h,w] / [no,512,h,w]')
        if qry_rects is not None:
            _check(qry_rects, 'qry_rects', torch.int32)
        if not 1 <= int(T) <= self.capacity:
            raise RuntimeError('T out of range')
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(self.no, 1024, self.h, self.w, dtype=torch.float32, device=self.device)
            if ws is None:
                ws = _ws(lib.rmnet_bank_read_workspace_bytes_for(self.no, self.h, self.w, int(T)), self.device)
            ev = [ctypes.c_void_p(e) if e else None for e in (events or (None, None, None))]
            rc = lib.rmnet_bank_read_f32_at(_ptr(self.blob), self.no, self.capacity, self.h, self.w, int(T), _ptr(_t_dev),
                                            _PRECISION_FLAGS[self.precision], _ptr(q_key), _ptr(q_val), _ptr(qry_rects), _ptr(out), _ptr(ws),
                                            ws.numel(), _stream(self.device), ev[0], ev[1], ev[2])
        _lib.check(rc, 'rmnet_bank_read_f32_at')
        return out


class TensorBank:
    """Same interface as ``MemoryBank`` on plain fp32 tensors in the reference's layout
    ([no,C,Tcap,h,w] + cell rectangles), read with the exact-fp32 kernel: no limit on the value range, about
    4x slower.  The frame loop switches to it when a ``MemoryBank`` reported out-of-window values (beyond 2048
    memorised frames it falls to the generic kernels, with a warning: the exact fused kernel takes one launch's frames)."""

    def __init__(self, no, capacity, h, w, device):
        self.no, self.capacity, self.h, self.w = int(no), int(capacity), int(h), int(w)
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.m_key = torch.zeros(self.no, 128, self.capacity, self.h, self.w, device=self.device)
            self.m_val = torch.zeros(self.no, 512, self.capacity, self.h, self.w, device=self.device)
            self.rects = torch.zeros(self.no, self.capacity, 4, dtype=torch.int32, device=self.device)
            # the whole-grid rectangle, built ONCE (a torch.tensor([...], device=...) per call is a blocking host-to-device copy
            # in the middle of the frame loop: this is the overflow fallback of every clip)
            self._full = torch.tensor([[0, self.w - 1, 0, self.h - 1]] * self.no, dtype=torch.int32, device=self.device)
        self.committed = 0

    def append(self, slot, k4, v4, rects=None):
        _check(k4, 'k4')
        _check(v4, 'v4')
        self.m_key[:, :, slot] = k4
        self.m_val[:, :, slot] = v4
        self.rects[:, slot] = self._full if rects is None else rects.view(self.no, 4)

    def overflow_count(self):
        return 0

    def logit_max(self):
        """(MemoryBank's interface: the exact-fp32 kernels have no arithmetic whose error grows with the logits.)"""
        return 0.0

    def status(self):
        return 0, 0, 0.0

    def timeout_count(self):
        """(MemoryBank's interface: the exact-fp32 kernels have no cross-workgroup merge that could time out.)"""
        return 0

    def assert_synced(self):
        """(MemoryBank's interface: there is no device-resident frame counter here.)"""

    def stage(self, k4, v4, rects):
        if self.committed >= self.capacity:
            raise RuntimeError('memory bank overflow (%d slots)' % self.capacity)
        self.append(self.committed, k4, v4, rects)
        return self.committed + 1

    def commit(self):
        self.committed += 1

    def read_staged(self, q_key, q_val, qry_rects=None, out=None, events=None, ws=None):
        return self.read(self.committed + 1, q_key, q_val, qry_rects, out=out, events=events, ws=ws)

    def read(self, T, q_key, q_val, qry_rects=None, out=None, events=None, ws=None):
        if qry_rects is None:
            qry_rects = self._full
        out, _ = memory_read(self.m_key, self.m_val, q_key, q_val, self.rects[:, :T].contiguous(),
                             qry_rects.contiguous(), T=T, out=out, events=events,
                             flags=MR_EXACT_FP32 if T <= BANK_MAX_SLOTS else self._generic_flags(T))
        return out

    def _generic_flags(self, T):
        import warnings
        nbytes = self.no * T * (self.h * self.w) ** 2 * 4
        warnings.warn('rmnet_amd: %d memorised frames exceed the fused kernels (%d): falling back to the generic path, which '
                      'materialises the affinity (%.1f GB of workspace)' % (T, BANK_MAX_SLOTS, nbytes / 1e9))
        return MR_FORCE_GENERIC


def rect_mask(x, rects):
    """x [n,C,T,h,w] * 0/1 cell rectangles [n,T,4] (models/rmnet.py:247-248, 357-358)."""
    _check(x, 'x')
    _check(rects, 'rects', torch.int32)
    n, C, T, h, w = x.shape
    if rects.numel() != n * T * 4:
        raise RuntimeError('rects must be [n,T,4]')
    lib = _lib.load()
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        rc = lib.rmnet_rect_mask_f32(_ptr(x), n, C, T, h, w, _ptr(rects), _ptr(y), _stream(x.device))
    _lib.check(rc, 'rmnet_rect_mask_f32')
    return y


def channel_affine(x, scale=None, shift=None, res=None, res_scale=None, res_shift=None, relu=False,
                   out=None):
    """out = act(x * scale[c] + shift[c] + (res * res_scale[c] + res_shift[c])) for NCHW fp32 ``x`` in
    one pass (csrc/epilogue.hip); ``relu``: False, True, or 'leaky' (= LeakyReLU(0.1)).  ``out`` may be
    ``x`` or ``res`` (in place); default: a new tensor.
    Replaces BatchNorm2d(eval) / conv bias / skip add / ReLU sequences around the convolutions."""
    _check_act(x, 'x')
    if x.dim() != 4:
        raise RuntimeError('x must be [N,C,H,W]')
    N, C, H, W = x.shape
    cl = _is_cl(x)                  # channels-last activations: the NHWC kernel (same arithmetic; csrc/epilogue.hip)
    for t, n in ((scale, 'scale'), (shift, 'shift'), (res_scale, 'res_scale'), (res_shift, 'res_shift')):
        if t is not None:
            _check(t, n)
            if t.numel() != C:
                raise RuntimeError('%s must have C = %d elements' % (n, C))
    if res is not None:
        _check_act(res, 'res')
        if res.shape != x.shape:
            raise RuntimeError('res must have the shape of x')
        if cl and not res.is_contiguous(memory_format=torch.channels_last):
            res = res.contiguous(memory_format=torch.channels_last)      # (a skip in the other layout: one conversion)
        elif not cl and not res.is_contiguous():
            res = res.contiguous()
    elif res_scale is not None or res_shift is not None:
        raise RuntimeError('res_scale / res_shift without res')
    if out is None:
        out = torch.empty_like(x)       # (preserves the memory format)
    else:
        _check_act(out, 'out')
        if out.shape != x.shape or not (out.is_contiguous(memory_format=torch.channels_last) if cl else out.is_contiguous()):
            raise RuntimeError('out must have the shape and memory format of x')
    lib = _lib.load()
    with torch.cuda.device(x.device):
        if cl and C % 4 == 0:
            rc = lib.rmnet_channel_affine_nhwc_f32(_ptr(x), _ptr(scale), _ptr(shift), _ptr(res), _ptr(res_scale), _ptr(res_shift),
                                                   2 if relu == 'leaky' else (1 if relu else 0), N * H * W, C, _ptr(out), _stream(x.device))
            _lib.check(rc, 'rmnet_channel_affine_nhwc_f32')
            return out
        if cl:
            raise RuntimeError('channels-last channel_affine needs C % 4 == 0')
        rc = lib.rmnet_channel_affine_f32(_ptr(x), _ptr(scale), _ptr(shift), _ptr(res), _ptr(res_scale),
                                          _ptr(res_shift), 2 if relu == 'leaky' else (1 if relu else 0), N, C, H * W, _ptr(out),
                                          _stream(x.device))
    _lib.check(rc, 'rmnet_channel_affine_f32')
    return out


def upsample2x_add(x, skip=None, out=None):
    """skip + F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False) in one pass
    (csrc/epilogue.hip); ``skip`` None = plain upsample; ``out`` may be ``skip`` (in place).
    The kernel is chosen by the operands: channels-last if ``x`` or ``skip`` is (the other one is converted), NCHW otherwise, and
    the result has that memory format.  An NCHW ``out`` next to channels-last operands is NOT written: a new channels-last tensor
    is returned instead (networks.Refine passes out=s whatever the layouts are and uses the returned value).  The other mismatch,
    a channels-last ``out`` next to NCHW operands, raises: the NCHW kernel would fill its storage in the wrong order.

    Differentiable in ``x`` and ``skip``: when grad mode is on and one of them requires grad, the call is recorded as one
    ``torch.autograd.Function`` that saves nothing.  The forward is the same launch into a new tensor (``out`` must be None); the
    backward hands the incoming gradient to ``skip`` as it is and ``upsample_backward(g, 2)`` to ``x``.  No double backward.
    Every other call takes the plain path."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, skip)):
        if out is not None:
            raise RuntimeError('upsample2x_add under autograd allocates its own output: out must be None')
        return _Upsample2xAddFn.apply(x, skip)
    _check_act(x, 'x')
    if x.dim() != 4:
        raise RuntimeError('x must be [N,C,h,w]')
    N, C, h, w = x.shape
    shape = (N, C, 2 * h, 2 * w)
    cl = _is_cl(x) or (skip is not None and _is_cl(skip))
    fmt = torch.channels_last if cl else torch.contiguous_format
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)      # (no copy when it already is)
    if skip is not None:
        _check_act(skip, 'skip')
        if tuple(skip.shape) != shape:
            raise RuntimeError('skip must be [N,C,2h,2w]')
        if cl and not _is_cl(skip):
            skip = skip.contiguous(memory_format=torch.channels_last)
    if out is None or (cl and not _is_cl(out)):
        out = torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=fmt)
    else:
        _check_act(out, 'out')
        if tuple(out.shape) != shape:
            raise RuntimeError('out must be [N,C,2h,2w]')
        if not cl and not out.is_contiguous():
            raise RuntimeError('out must have the memory format of x and skip (NCHW here, out is channels-last)')
    lib = _lib.load()
    with torch.cuda.device(x.device):
        if cl:
            rc = lib.rmnet_upsample2x_add_nhwc_f32(_ptr(x), _ptr(skip), N, C, h, w, _ptr(out), _stream(x.device))
            _lib.check(rc, 'rmnet_upsample2x_add_nhwc_f32')
            return out
        rc = lib.rmnet_upsample2x_add_f32(_ptr(x), _ptr(skip), N, C, h, w, _ptr(out), _stream(x.device))
    _lib.check(rc, 'rmnet_upsample2x_add_f32')
    return out


# ---- gradients of the decoder's glue (csrc/decoder_glue_bwd.hip) ----------------------------------------------------------------
# The kernels' constants, restated by tests/test_decoder_glue_grad.py: threads per workgroup, the upsample adjoint's largest grid,
# and the prediction head's channels per workgroup, pixel slots and range plan.
GLUE_THREADS, UPSAMPLE_BWD_MAX_BLOCKS = 256, 1024
PRED_BWD_CT, PRED_BWD_SLOTS = 32, 32
PRED_BWD_RANGE_MIN, PRED_BWD_MAX_RANGES, PRED_BWD_TARGET_WGS = 256, 128, 1024


def pred_head_backward_plan(pixels, C):
    """(channel tiles, ranges, pixels per range) of ``pred_head_backward`` for n*Hq*Wq = ``pixels``: csrc/decoder_glue_bwd.hip, ph_plan."""
    nct = C // PRED_BWD_CT
    nr = max(1, min(PRED_BWD_TARGET_WGS // nct, -(-pixels // PRED_BWD_RANGE_MIN), PRED_BWD_MAX_RANGES))
    rl = -(-(-(-pixels // nr)) // PRED_BWD_SLOTS) * PRED_BWD_SLOTS
    return nct, -(-pixels // rl), rl


def upsample_backward(g, factor, out=None):
    """The adjoint of ``F.interpolate(x, scale_factor=factor, mode='bilinear', align_corners=False)`` for ``factor`` 2 or 4
    (csrc/decoder_glue_bwd.hip, include/rmnet_hip.h: rmnet_upsample_bwd_f32): ``g`` [N,C,factor*h,factor*w] fp32, the gradient of
    the fine map, -> the gradient [N,C,h,w] of the coarse one.  Channels-last if ``g`` is (C % 4 == 0), NCHW otherwise, and the
    result (``out``, when given, must have it) has that memory format.  A gather with constant weights: no atomics, every element
    written once, the same bits on every call.  No fall-back: anything else is a RuntimeError."""
    _check_act(g, 'g')
    factor = int(factor)
    if factor not in (2, 4):
        raise RuntimeError('upsample_backward serves factor 2 and 4, got %d' % factor)
    if g.dim() != 4 or g.shape[2] % factor or g.shape[3] % factor or g.numel() == 0:
        raise RuntimeError('g must be a non-empty [N,C,%d h,%d w] tensor, got %s' % (factor, factor, tuple(g.shape)))
    N, C, H, W = g.shape
    h, w = H // factor, W // factor
    cl = _is_cl(g)
    if cl and C % 4:
        raise RuntimeError('a channels-last g needs C %% 4 == 0, got %d' % C)
    shape = (N, C, h, w)
    if out is None:
        out = torch.empty(shape, dtype=g.dtype, device=g.device, memory_format=torch.channels_last if cl else torch.contiguous_format)
    else:
        _check_act(out, 'out')
        if tuple(out.shape) != shape or out.device != g.device:
            raise RuntimeError('out must be [N,C,h,w] on the device of g')
        if not out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format):
            raise RuntimeError('out must have the memory format of g')
    lib = _lib.load()
    with torch.cuda.device(g.device):
        rc = lib.rmnet_upsample_bwd_f32(_ptr(g), N, C, h, w, factor, 1 if cl else 0, _ptr(out), _stream(g.device))
    _lib.check(rc, 'rmnet_upsample_bwd_f32')
    return out


def _glue_grad_input(g):
    """An incoming gradient as a tensor ``upsample_backward`` takes: itself when dense (NCHW, or channels-last with C % 4 == 0),
    else an NCHW copy (an expanded or sliced grad_output)."""
    if g.is_contiguous() or (_is_cl(g) and g.shape[1] % 4 == 0):
        return g
    return g.contiguous()


class _Upsample2xAddFn(torch.autograd.Function):
    """upsample2x_add under autograd.  Saves nothing: both maps are linear."""

    @staticmethod
    def forward(ctx, x, skip):
        ctx.set_materialize_grads(False)
        return upsample2x_add(x.detach(), None if skip is None else skip.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None
        gx = upsample_backward(_glue_grad_input(g), 2) if ctx.needs_input_grad[0] else None
        return gx, (g if ctx.needs_input_grad[1] else None)


class _Upsample4xFn(torch.autograd.Function):
    """upsample4x under autograd: torch's forward, the gather of upsample_backward instead of torch's atomic scatter behind it."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        return F.interpolate(x.detach(), scale_factor=4, mode='bilinear', align_corners=False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return None if g is None else upsample_backward(g.contiguous(), 4)


def upsample4x(x):
    """``F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=False)``: the decoder's last step.  The forward is that
    call; on a CUDA fp32 ``x`` that requires grad (grad mode on) it is recorded as one ``torch.autograd.Function`` whose backward is
    ``upsample_backward(g.contiguous(), 4)`` -- deterministic, where torch's own backward adds with atomics.  No double backward.
    On the CPU, and for every call that needs no gradient, it is the plain torch op."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.requires_grad and torch.is_grad_enabled():
        return _Upsample4xFn.apply(x)
    return F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=False)


def pred_head_backward(x, weight, g, need=(True, True, True)):
    """The gradients of ``pred_head`` (csrc/decoder_glue_bwd.hip, include/rmnet_hip.h: rmnet_pred_head_bwd_f32) for a channels-last
    fp32 ``x`` [n, C, Hq, Wq] (the forward's input, C % 32 == 0), ``weight`` [2, C, 3, 3] and the NCHW-contiguous gradient ``g``
    [n, 2, Hq, Wq] of the output.  Returns ``(dx, dw, db)`` -- dx channels-last like x, masked by ``x > 0`` (a NaN in x: 0), dw
    [2, C, 3, 3], db [2] -- with None for the parts ``need`` does not ask for.  One pass over x, per-range partials merged in range
    order: no atomics, the same bits on every call.  No fall-back: anything else is a RuntimeError."""
    _check_act(x, 'x')
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last) or x.numel() == 0:
        raise RuntimeError('x must be a non-empty channels-last [n, C, Hq, Wq] tensor')
    n, C, H, W = x.shape
    if C % 32:
        raise RuntimeError('pred_head_backward needs C %% 32 == 0, got %d' % C)
    _check(weight, 'weight')
    _check(g, 'g')
    if tuple(weight.shape) != (2, C, 3, 3) or tuple(g.shape) != (n, 2, H, W):
        raise RuntimeError('pred_head_backward needs weight [2, %d, 3, 3] and g [%d, 2, %d, %d], got %s / %s'
                           % (C, n, H, W, tuple(weight.shape), tuple(g.shape)))
    if weight.device != x.device or g.device != x.device:
        raise RuntimeError('pred_head_backward: every tensor must be on %s' % x.device)
    need_x, need_w, need_b = (bool(v) for v in need)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last) if need_x else None
    dw = torch.empty((2, C, 3, 3), dtype=x.dtype, device=x.device) if need_w else None
    db = torch.empty(2, dtype=x.dtype, device=x.device) if need_b else None
    if not (need_x or need_w or need_b):
        return dx, dw, db
    lib = _lib.load()
    ws = _ws(lib.rmnet_pred_head_bwd_workspace_bytes(n, H, W, C), x.device) if need_w or need_b else None
    with torch.cuda.device(x.device):
        rc = lib.rmnet_pred_head_bwd_f32(_ptr(x), _ptr(weight), _ptr(g), n, H, W, C, _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws),
                                         ws.numel() if ws is not None else 0, _stream(x.device))
    _lib.check(rc, 'rmnet_pred_head_bwd_f32')
    return dx, dw, db


class _PredHeadFn(torch.autograd.Function):
    """pred_head under autograd: saves x and the weight."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, weight)
        return pred_head(x.detach(), weight.detach(), bias.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None
        x, weight = ctx.saved_tensors
        return pred_head_backward(x.detach(), weight.detach(), g.contiguous(), ctx.needs_input_grad[:3])


def soft_aggregate_backward(dec, obj_begin, K, pad, prob, grad_prob=None, grad_logit=None, action=None):
    """The gradient of the decoder tail with respect to ``dec`` [n_tot,2,Hp,Wp], in one launch (csrc/soft_aggregate_bwd.hip,
    include/rmnet_hip.h: rmnet_soft_aggregate_bwd_f32).  ``prob`` [B,K,H,W] are the probabilities the forward saved (after the
    edits on an edited frame), ``grad_prob`` / ``grad_logit`` the gradients with respect to them / to the (edited) logits -- at
    least one --, ``action`` uint8 [B,K] the frame's edits (``object_edit_softmax``) or None.  prob and the two gradients may be
    batch-strided views whose slices are contiguous (``est[:, t]``).  Returns ``grad_dec`` like ``dec``, every element written."""
    _check(dec, 'dec')
    _check(obj_begin, 'obj_begin', torch.int32)
    if dec.dim() != 4 or dec.shape[1] != 2:
        raise RuntimeError('dec must be [n,2,Hp,Wp]')
    if grad_prob is None and grad_logit is None:
        raise RuntimeError('soft_aggregate_backward needs grad_prob or grad_logit')
    B = obj_begin.numel() - 1
    K = int(K)
    if B < 1 or not 1 <= K <= 255:
        raise RuntimeError('expected obj_begin [B+1] with B >= 1 and 1 <= K <= 255')
    Hp, Wp = dec.shape[2:]
    lw, uw, lh, uh = pad
    H, W = Hp - lh - uh, Wp - lw - uw
    strides = []
    for t, name in ((prob, 'prob'), (grad_prob, 'grad_prob'), (grad_logit, 'grad_logit')):
        if t is None:
            strides.append(0)
            continue
        strides.append(_batch_slices(t, name, (K, H, W), torch.float32))
        if t.shape[0] != B or t.device != dec.device:
            raise RuntimeError('%s must be [B, K, H, W] on the device of dec' % name)
    if action is not None:
        _check(action, 'action', dtype=torch.uint8)
        if tuple(action.shape) != (B, K) or action.device != dec.device:
            raise RuntimeError('action must be uint8 [B, K] on the device of dec')
    grad_dec = torch.empty_like(dec)
    if dec.numel() == 0:
        return grad_dec
    lib = _lib.load()
    with torch.cuda.device(dec.device):
        rc = lib.rmnet_soft_aggregate_bwd_f32(_ptr(dec), _ptr(obj_begin), B, K, Hp, Wp, lw, lh, H, W, _ptr(prob), strides[0],
                                              _ptr(grad_prob), strides[1], _ptr(grad_logit), strides[2], _ptr(action), _ptr(grad_dec),
                                              _stream(dec.device))
    _lib.check(rc, 'rmnet_soft_aggregate_bwd_f32')
    return grad_dec


class _SoftAggregateFn(torch.autograd.Function):
    """soft_aggregate (+ object_edit_softmax on an edited frame) under autograd: the forward is the two launches every other caller
    makes, the backward is soft_aggregate_backward.  It returns (logit, prob) and both are differentiable."""

    @staticmethod
    def forward(ctx, dec, obj_begin, K, pad, edit):
        d = dec.detach()
        logit, prob = soft_aggregate(d, obj_begin, K, pad, want_prob=True)
        action = None
        if edit is not None:
            labels, lut, action = edit[:3]
            object_edit_softmax(logit, labels, lut, action, prob, edit[3] if len(edit) > 3 else None)
        ctx.save_for_backward(dec, obj_begin, prob, *(() if action is None else (action,)))
        ctx.K, ctx.pad = K, tuple(pad)
        ctx.set_materialize_grads(False)
        return logit, prob

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logit, grad_prob):
        saved = ctx.saved_tensors
        dec, obj_begin, prob = saved[:3]
        if grad_logit is None and grad_prob is None:
            return None, None, None, None, None
        same = lambda g: None if g is None else g.contiguous()         # (an expanded or sliced grad_output becomes a plain tensor)
        grad = soft_aggregate_backward(dec.detach(), obj_begin, ctx.K, ctx.pad, prob, same(grad_prob), same(grad_logit),
                                       saved[3] if len(saved) > 3 else None)
        return grad, None, None, None, None


def soft_aggregate(dec, obj_begin, K, pad, want_prob=False, edit=None):
    """Decoder logits [n_tot,2,Hp,Wp] -> (logit [B,K,H,W], prob [B,K,H,W] | None): 2-class soft-max,
    soft aggregation (models/rmnet.py:289-302), un-pad by ``pad = (lw, uw, lh, uh)`` and, when asked,
    the soft-max over the K channels, in one kernel.  ``obj_begin`` int32 [B+1] on the device.

    ``edit = (labels, lut, action[, sampling])``: the frame's late-object edits (models/rmnet.py:436-448) follow in a second
    launch -- the arguments of ``object_edit_softmax`` -- so the returned logits are the edited ones and ``prob`` their soft-max.

    Differentiable in ``dec``: when grad mode is on and ``dec`` requires grad, the call is recorded as one
    ``torch.autograd.Function`` whose backward is ``soft_aggregate_backward`` (one launch).  The probabilities are then computed
    whether or not they are asked for -- the backward reads them --, and there is no double backward.  Every other call takes
    the plain path."""
    if isinstance(dec, torch.Tensor) and dec.requires_grad and torch.is_grad_enabled():
        _check(dec, 'dec')
        logit, prob = _SoftAggregateFn.apply(dec, obj_begin, K, pad, edit)
        return logit, (prob if want_prob else None)
    if edit is not None:
        logit, prob = soft_aggregate(dec, obj_begin, K, pad, want_prob=True)
        object_edit_softmax(logit, edit[0], edit[1], edit[2], prob, edit[3] if len(edit) > 3 else None)
        return logit, (prob if want_prob else None)
    _check(dec, 'dec')
    _check(obj_begin, 'obj_begin', torch.int32)
    if dec.dim() != 4 or dec.shape[1] != 2:
        raise RuntimeError('dec must be [n,2,Hp,Wp]')
    B = obj_begin.numel() - 1
    Hp, Wp = dec.shape[2:]
    lw, uw, lh, uh = pad
    H, W = Hp - lh - uh, Wp - lw - uw
    logit = torch.empty(B, K, H, W, dtype=dec.dtype, device=dec.device)
    prob = torch.empty_like(logit) if want_prob else None
    lib = _lib.load()
    with torch.cuda.device(dec.device):
        rc = lib.rmnet_soft_aggregate_f32(_ptr(dec), _ptr(obj_begin), B, K, Hp, Wp, lw, lh, H, W,
                                          _ptr(logit), _ptr(prob), _stream(dec.device))
    _lib.check(rc, 'rmnet_soft_aggregate_f32')
    return logit, prob


CONV_COUT = 256                   # csrc/conv3x3.hip: output channels of the split-fp16 convolution
CONV_RELU_IN, CONV_RELU_OUT = 1, 2  # RMNET_CONV_*


@torch.no_grad()
def conv3x3_pack(weight):
    """[256, Cin, 3, 3] fp32 weight -> (wpack [9 * Cin * 256 * 2] fp16 bits as int16, w_unscale fp32 [256]) in the layout of
    include/rmnet_hip.h (rmnet_conv3x3_split_f32): per output channel a power-of-two scale 2^e puts max |w| in
    [2^14, 2^15), the scaled weights are split into fp16 hi = rne(ws), lo = rne(ws - hi) and laid out as
    [tap][Cin / 32][hi, lo][co][Cin % 32].  Exact up to fp16 rounding of lo (2^-22 relative)."""
    if weight.dim() != 4 or weight.shape[0] != CONV_COUT or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] % 32:
        raise RuntimeError('conv3x3_pack needs a [256, Cin, 3, 3] weight with Cin % 32 == 0, got %s' % (tuple(weight.shape),))
    if weight.dtype != torch.float32:
        raise RuntimeError('conv3x3_pack needs fp32 weights, got %s' % weight.dtype)
    w = weight.detach().contiguous()
    cin = w.shape[1]
    amax = w.abs().amax(dim=(1, 2, 3))
    _, ex = torch.frexp(amax)                              # amax in [2^(ex-1), 2^ex)
    e = torch.where(amax > 0, 15 - ex, torch.zeros_like(ex))
    ws = torch.ldexp(w, e.view(-1, 1, 1, 1).to(w.dtype))   # exact: power-of-two scaling
    hi = ws.half()
    lo = (ws - hi.float()).half()
    planes = torch.stack([p.reshape(CONV_COUT, cin // 32, 32, 9).permute(3, 1, 0, 2) for p in (hi, lo)], dim=2)
    unscale = torch.ldexp(torch.ones_like(amax), (-e).to(amax.dtype))
    return planes.contiguous().view(-1).view(torch.int16), unscale.contiguous()      # (fp16 bits held as int16: .float() leaves them)


_range_words = {}


def conv_range_word(device):
    """The device's int32 range word of the split-fp16 convolutions (created on first use: call it once outside graph capture).
    One per device, shared by every network on it: ``RMNet.forward`` zeroes it at the start of a clip and reads it at the end."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    w = _range_words.get(idx)
    if w is None:
        w = _range_words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device('cuda', idx))
    return w


# The kernel behind conv3x3_split when RMNET_CONV3X3_KERNEL is not set: 'wreg' -- conv3x3_wreg, weight fragments loaded straight
# into registers (rmnet_conv3x3_split_f32); 'lds' -- conv3x3_split, weights staged through LDS (rmnet_conv3x3_split_lds_f32).
# Both return the same bits.  The rule: 'wreg' only if every bench run with it is above every run with 'lds'
# (profiles/r19_a_conv3x3_wreg.md).
CONV3X3_KERNEL_DEFAULT = 'wreg'
CONV3X3_ENTRIES = {'wreg': 'rmnet_conv3x3_split_f32', 'lds': 'rmnet_conv3x3_split_lds_f32'}


def conv3x3_entry():
    """The export that ``conv3x3_split`` calls: RMNET_CONV3X3_KERNEL ('wreg' or 'lds', read at every call; unset:
    CONV3X3_KERNEL_DEFAULT).  Any other value is a RuntimeError."""
    v = os.environ.get('RMNET_CONV3X3_KERNEL')
    v = CONV3X3_KERNEL_DEFAULT if v is None else v.strip()
    if v not in CONV3X3_ENTRIES:
        raise RuntimeError('RMNET_CONV3X3_KERNEL must be one of %s, got %r' % (sorted(CONV3X3_ENTRIES), v))
    return CONV3X3_ENTRIES[v]


# The Cin = 256 convolutions on conv3x3_rows (csrc/conv3x3_rows.hip: a tap row's activations staged in LDS once; the same bits)
# when RMNET_CONV3X3_ROWS is not set.  The rule: True only if every bench run with it is above every run of the parent commit and
# above every run of the same tree with the switch off (profiles/r20_a_conv3x3_rows.md).
CONV3X3_ROWS_DEFAULT = True
CONV3X3_ROWS_ENTRY = 'rmnet_conv3x3_rows_f32'
CONV3X3_ROWS_CIN = 256


def conv3x3_rows_enabled():
    """RMNET_CONV3X3_ROWS ('0' or '1', read at every call; unset: CONV3X3_ROWS_DEFAULT).  Any other value is a RuntimeError."""
    v = os.environ.get('RMNET_CONV3X3_ROWS')
    if v is None:
        return CONV3X3_ROWS_DEFAULT
    if v.strip() not in ('0', '1'):
        raise RuntimeError("RMNET_CONV3X3_ROWS must be '0' or '1', got %r" % v)
    return v.strip() == '1'


def conv3x3_split(x, wpack, w_unscale, bias=None, res=None, relu_in=False, relu_out=False, out=None, range_word=None, weight=None,
                  dgrad_packs=None):
    """act(conv3x3(pre(x), w) + bias + res) for a channels-last fp32 ``x`` [N, Cin, H, W] and 256 output channels, stride 1,
    padding 1, on the split-fp16 MFMA kernel (csrc/conv3x3.hip); ``pre`` / ``act`` = ReLU when ``relu_in`` / ``relu_out``.
    ``wpack, w_unscale`` come from ``conv3x3_pack``.  ``out`` (channels-last, may be ``res``, must not be ``x``) defaults to a
    new tensor.  ``range_word`` (int32 [1] on the device): activations with |pre(x)| >= 1023.5, NaN or Inf are saturated
    and counted there -- check it before trusting the result.  No fall-back: anything else is a RuntimeError.

    Differentiable in ``x``, ``weight``, ``bias`` and ``res`` for a caller that passes ``weight`` (the [256, Cin, 3, 3] tensor the
    pack was made from; the pack itself carries no gradient) or ``dgrad_packs``: when grad mode is on and one of the four requires
    grad, the call is recorded as one ``torch.autograd.Function``.  The forward is the same launch; the backward stages the incoming gradient (``conv_grad_stage``), takes
    the weight / bias gradient from ``conv3x3_wgrad`` and the data gradient from this kernel on ``dgrad_packs``
    (``conv3x3_dgrad_pack(weight)``, built on the spot when not given; Cin % 256 == 0).  Only what ``needs_input_grad`` asks for is
    computed, ``out`` must be left to the call, and there is no double backward.  Every other call takes the plain path: the bits
    and the graph-free result of before."""
    if (weight is not None or dgrad_packs is not None) and torch.is_grad_enabled() \
            and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, weight, bias, res)):
        if out is not None:
            raise RuntimeError('conv3x3_split under autograd allocates its own output: out must be None')
        return _Conv3x3SplitFn.apply(x, weight, bias, res, wpack, w_unscale, dgrad_packs, bool(relu_in), bool(relu_out), range_word)
    _check_act(x, 'x')
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('x must be a channels-last [N, Cin, H, W] tensor')
    N, cin, H, W = x.shape
    if cin % 32:
        raise RuntimeError('conv3x3_split needs Cin % 32 == 0, got %d' % cin)
    _check(wpack, 'wpack', torch.int16)
    if wpack.numel() != 9 * cin * CONV_COUT * 2:
        raise RuntimeError('wpack has %d elements, a Cin = %d pack has %d' % (wpack.numel(), cin, 9 * cin * CONV_COUT * 2))
    _check(w_unscale, 'w_unscale')
    shape = (N, CONV_COUT, H, W)
    for t, n in ((bias, 'bias'),):
        if t is not None:
            _check(t, n)
            if t.numel() != CONV_COUT:
                raise RuntimeError('%s must have 256 elements' % n)
    if w_unscale.numel() != CONV_COUT:
        raise RuntimeError('w_unscale must have 256 elements')
    if res is not None:
        _check_act(res, 'res')
        if tuple(res.shape) != shape or not res.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError('res must be a channels-last [N, 256, H, W] tensor')
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    else:
        _check_act(out, 'out')
        if tuple(out.shape) != shape or not out.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError('out must be a channels-last [N, 256, H, W] tensor')
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
    for t in (wpack, w_unscale, bias, res, out, range_word):
        if t is not None and t.device != x.device:
            raise RuntimeError('conv3x3_split: every tensor must be on %s' % x.device)
    flags = (CONV_RELU_IN if relu_in else 0) | (CONV_RELU_OUT if relu_out else 0)
    entry = conv3x3_entry()
    # conv3x3_rows: the switch on, no kernel named explicitly (RMNET_CONV3X3_KERNEL=wreg|lds always gets that kernel), Cin = 256
    if conv3x3_rows_enabled() and os.environ.get('RMNET_CONV3X3_KERNEL') is None and cin == CONV3X3_ROWS_CIN:
        entry = CONV3X3_ROWS_ENTRY
    lib = _lib.load()
    with torch.cuda.device(x.device):
        rc = getattr(lib, entry)(_ptr(x), _ptr(wpack), _ptr(w_unscale), _ptr(bias), _ptr(res), flags, N, H, W, cin,
                                 _ptr(out), _ptr(range_word), _stream(x.device))
    _lib.check(rc, entry)
    return out


# ---- gradients of conv3x3_split (csrc/conv3x3_wgrad.hip) ------------------------------------------------------------------------
# The weight-gradient kernel's constants, restated by tests/test_conv_grad.py: input channels per workgroup, pixels per K step,
# pixels per activation image (a range longer than that is walked in several images), the widest map, and the range plan's three.
WGRAD_CT, WGRAD_KT, WGRAD_SUB, WGRAD_MAX_W = 16, 32, 512, 448
WGRAD_RANGE_MIN, WGRAD_MAX_RANGES, WGRAD_TARGET_WGS = 256, 64, 768
WGRAD_BIAS_SPLIT = 8              # the bias gradient sums a range in that many chunks
GRAD_TOP_EXP = 9                  # a staged gradient's largest element lies in [2^8, 2^9)

# Launches made by the gradient path, counted on the Python side ('pack' counts conv3x3_dgrad_pack and conv_split_dgrad_pack calls); tests reset and read it.
conv_grad_launches = {'stage': 0, 'wgrad': 0, 'dgrad': 0, 'pack': 0}


def conv3x3_wgrad_plan(pixels, cin, cout=256):
    """(channel tiles, ranges, pixels per range) of ``conv3x3_wgrad`` for N*H*W = ``pixels`` and ``cout`` output channels, which are
    walked in ceil(cout / 256) tiles that share the ranges: csrc/conv3x3_wgrad_parts.h, wgrad_plan."""
    nct = cin // WGRAD_CT
    nr = max(1, min(WGRAD_TARGET_WGS // (nct * -(-cout // CONV_COUT)), -(-pixels // WGRAD_RANGE_MIN), WGRAD_MAX_RANGES))
    rl = -(-(-(-pixels // nr)) // WGRAD_KT) * WGRAD_KT
    return nct, -(-pixels // rl), rl


_grad_range_words = {}


def conv_grad_range_word(device):
    """The device's int32 range word of the convolutions' BACKWARD (created on first use: call it once outside graph capture):
    staged gradients and saved activations outside the fp16 window, NaN and Inf are counted here, never in ``conv_range_word``,
    which stays what the forward left in it."""
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    w = _grad_range_words.get(idx)
    if w is None:
        w = _grad_range_words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device('cuda', idx))
    return w


@torch.no_grad()
def conv3x3_dgrad_pack(weight):
    """The packs of the data gradient of a [256, Cin, 3, 3] convolution, Cin % 256 == 0: for stride 1 / pad 1,
    dX = conv3x3(G, W transposed and flipped), a convolution with 256 inputs and Cin outputs, i.e. Cin / 256 calls of
    ``conv3x3_split``.  Returns the list of ``conv3x3_pack(weight.transpose(0, 1).flip(2, 3)[256 s : 256 (s + 1)])``."""
    if weight.dim() != 4 or weight.shape[0] != CONV_COUT or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] % CONV_COUT:
        raise RuntimeError('conv3x3_dgrad_pack needs a [256, Cin, 3, 3] weight with Cin %% 256 == 0, got %s' % (tuple(weight.shape),))
    conv_grad_launches['pack'] += 1
    wt = weight.detach().transpose(0, 1).flip(2, 3)
    return [conv3x3_pack(wt[s * CONV_COUT:(s + 1) * CONV_COUT]) for s in range(weight.shape[1] // CONV_COUT)]


def conv_grad_stage_exponent(amax):
    """s (an int32 tensor like ``amax``, any device) with 2^s * amax in [2^8, 2^9): 9 - e for amax in [2^(e-1), 2^e), subnormals
    included; 0 for amax = 0, NaN or Inf.  What csrc/conv3x3_wgrad.hip: conv_grad_stage computes on the device."""
    a = amax.detach().to(torch.float32)
    _, ex = torch.frexp(a)
    return torch.where((a > 0) & torch.isfinite(a), GRAD_TOP_EXP - ex, torch.zeros_like(ex))


def conv_grad_stage(g, act=None, amax=None, out=None):
    """The stage pass of a convolution's backward, one kernel and no host synchronisation: ``gs = [act > 0] * g * 2^s`` with
    ``s = conv_grad_stage_exponent(amax)``.  ``g`` (fp32, dense; ``act`` of the same shape and strides, or None) is the incoming
    gradient, ``amax`` a 0-dim fp32 upper bound of |g| on the device, taken before the mask (default: the largest |element|, one
    reduction).  Returns ``(gs, g_scale)``: ``gs`` like ``g`` (``out`` may be ``g`` itself) and ``g_scale`` fp32 [2], two powers
    of two whose product is 2^s (the second is 1 unless amax < 2^-118)."""
    _check_act(g, 'g')
    if amax is None:
        amax = torch.linalg.vector_norm(g, float('inf'))
    _check(amax, 'amax')
    if amax.numel() != 1:
        raise RuntimeError('amax must hold one element')
    if act is not None:
        _check_act(act, 'act')
        if act.shape != g.shape or act.stride() != g.stride():
            raise RuntimeError('act must have the shape and strides of g')
    if g.numel() == 0 or g.numel() % 4:
        raise RuntimeError('conv_grad_stage needs a non-empty g with a multiple of 4 elements')
    gs = torch.empty_like(g) if out is None else out
    if gs.shape != g.shape or gs.stride() != g.stride() or gs.dtype != g.dtype:
        raise RuntimeError('out must have the shape, strides and dtype of g')
    g_scale = torch.empty(4, dtype=torch.float32, device=g.device)[:2]
    for t in (act, amax, gs):
        if t is not None and t.device != g.device:
            raise RuntimeError('conv_grad_stage: every tensor must be on %s' % g.device)
    lib = _lib.load()
    with torch.cuda.device(g.device):
        rc = lib.rmnet_conv_grad_stage_f32(_ptr(g), _ptr(act), _ptr(amax), g.numel(), _ptr(gs), _ptr(g_scale), _stream(g.device))
    _lib.check(rc, 'rmnet_conv_grad_stage_f32')
    conv_grad_launches['stage'] += 1
    return gs, g_scale


def conv3x3_wgrad(x, g, g_scale, relu_in=False, want_bias=True, range_word=None):
    """The weight and bias gradient of ``conv3x3_split`` (csrc/conv3x3_wgrad.hip, include/rmnet_hip.h: rmnet_conv3x3_wgrad_f32):
    ``dW[co, ci, ky, kx] = sum g[n, co, y, x] * pre(x)[n, ci, y + ky - 1, x + kx - 1] / (g_scale[0] * g_scale[1])`` and
    ``db[co] = sum g[n, co, y, x] / (g_scale[0] * g_scale[1])`` for channels-last fp32 ``x`` [N, Cin, H, W] (the forward's input,
    ``pre`` = ReLU under ``relu_in``) and ``g`` [N, Cout, H, W], Cout % 128 == 0 (the STAGED gradient of ``conv_grad_stage`` or
    ``conv_grad_stage_rect`` with its ``g_scale``; ``torch.ones(2)`` for a gradient that is already inside |g| < 1023.5).  Returns
    ``(dW, db)``: dW a channels-last [Cout, Cin, 3, 3] tensor, db [Cout] or None.  Deterministic: no atomics, the same bits on
    every call.  Cout = 256 runs rmnet_conv3x3_wgrad_f32, every other width rmnet_conv3x3_wgrad_n_f32 (csrc/conv_wgrad_n.hip: the
    same arithmetic over tiles of output channels).  ``range_word``: the backward's (``conv_grad_range_word``)."""
    for t, n in ((x, 'x'), (g, 'g')):
        _check_act(t, n)
        if t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError('%s must be a channels-last 4-D tensor' % n)
    N, cin, H, W = x.shape
    cout = g.shape[1]
    if tuple(g.shape) != (N, cout, H, W) or cout % 128 or cout == 0:
        raise RuntimeError('g must be [N, Cout, H, W] with Cout %% 128 == 0 for x [N, Cin, H, W], got %s and %s'
                           % (tuple(g.shape), tuple(x.shape)))
    if cin % 32:
        raise RuntimeError('conv3x3_wgrad needs Cin % 32 == 0, got %d' % cin)
    _check(g_scale, 'g_scale')
    if g_scale.numel() != 2:
        raise RuntimeError('g_scale must hold two floats')
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
    for t in (g, g_scale, range_word):
        if t is not None and t.device != x.device:
            raise RuntimeError('conv3x3_wgrad: every tensor must be on %s' % x.device)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    db = torch.empty(cout, dtype=torch.float32, device=x.device) if want_bias else None
    lib = _lib.load()
    flags = CONV_RELU_IN if relu_in else 0
    if cout == CONV_COUT:
        what = 'rmnet_conv3x3_wgrad_f32'
        ws = _ws(lib.rmnet_conv3x3_wgrad_workspace_bytes(N, H, W, cin), x.device)
        with torch.cuda.device(x.device):
            rc = lib.rmnet_conv3x3_wgrad_f32(_ptr(x), _ptr(g), _ptr(g_scale), flags, N, H, W, cin, _ptr(dw), _ptr(db), _ptr(ws),
                                             ws.numel(), _ptr(range_word), _stream(x.device))
    else:
        what = 'rmnet_conv3x3_wgrad_n_f32'
        ws = _ws(lib.rmnet_conv3x3_wgrad_n_workspace_bytes(N, H, W, cin, cout), x.device)
        with torch.cuda.device(x.device):
            rc = lib.rmnet_conv3x3_wgrad_n_f32(_ptr(x), _ptr(g), _ptr(g_scale), flags, N, H, W, cin, cout, _ptr(dw), _ptr(db), _ptr(ws),
                                               ws.numel(), _ptr(range_word), _stream(x.device))
    _lib.check(rc, what)
    conv_grad_launches['wgrad'] += 1
    return dw, db


def conv3x3_dgrad(gs, g_scale, dgrad_packs, range_word=None):
    """The data gradient of ``conv3x3_split`` from the staged gradient ``gs`` [N, 256, H, W] (``conv_grad_stage``): one
    ``conv3x3_split`` per 256 input channels on the packs of ``conv3x3_dgrad_pack``, with ``w_unscale / (g_scale[0] * g_scale[1])``
    in place of ``w_unscale`` (exact: powers of two); the slices are concatenated in channels-last.  No mask is applied here."""
    inv = g_scale.reciprocal()
    parts = []
    for wp, wu in dgrad_packs:
        parts.append(conv3x3_split(gs, wp, wu * inv[0] * inv[1], range_word=range_word))
        conv_grad_launches['dgrad'] += 1
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


class _Conv3x3SplitFn(torch.autograd.Function):
    """conv3x3_split under autograd: out = act(conv(pre(x)) + bias + res).  Saves x and, under relu_out, out -- nothing else."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, wpack, w_unscale, dgrad_packs, relu_in, relu_out, range_word):
        det = lambda t: None if t is None else t.detach()
        out = conv3x3_split(det(x), wpack, w_unscale, det(bias), det(res), relu_in, relu_out, range_word=range_word)
        need_x = ctx.needs_input_grad[0]
        if need_x and dgrad_packs is None and weight is None:
            raise RuntimeError('conv3x3_split: the gradient with respect to x needs weight or dgrad_packs')
        if need_x and x.shape[1] % CONV_COUT:
            raise RuntimeError('conv3x3_split: the gradient with respect to x needs Cin %% 256 == 0, got %d' % x.shape[1])
        if weight is not None and weight.requires_grad and tuple(weight.shape) != (CONV_COUT, x.shape[1], 3, 3):
            raise RuntimeError('weight must be [256, Cin, 3, 3]')
        # (the packs are made from the weight as it is NOW: an optimiser step between forward and backward must not change the gradient)
        ctx.dgrad_packs = (dgrad_packs if dgrad_packs is not None else conv3x3_dgrad_pack(weight)) if need_x else None
        ctx.relu_in, ctx.relu_out = relu_in, relu_out
        ctx.save_for_backward(x, *((out,) if relu_out else ()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        x = saved[0].detach()
        out = saved[1] if ctx.relu_out else None
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        g = grad_out.contiguous(memory_format=torch.channels_last)          # (an expanded or NCHW grad_output becomes a plain tensor)
        gx = gw = gb = gr = None
        if need_r:
            gr = g if out is None else torch.ops.aten.threshold_backward(g, out, 0)
        if need_x or need_w:
            grw = conv_grad_range_word(x.device)
            gs, g_scale = conv_grad_stage(g, out)
            if need_w:
                gw, gb = conv3x3_wgrad(x, gs, g_scale, ctx.relu_in, want_bias=need_b, range_word=grw)
            if need_x:
                gx = conv3x3_dgrad(gs, g_scale, ctx.dgrad_packs, range_word=grw)
                if ctx.relu_in:
                    gx = torch.ops.aten.threshold_backward(gx, x, 0)
        if need_b and gb is None:                                           # (a trainable bias on frozen weights: no GEMM)
            gm = g if out is None else (gr if gr is not None else torch.ops.aten.threshold_backward(g, out, 0))
            gb = gm.sum(dim=(0, 2, 3))
        return gx, gw, gb, gr, None, None, None, None, None, None


# ---- gradients of the key / value heads (csrc/conv_wgrad_n.hip; the data gradient is conv_split on flipped packs) -----------------
GRAD_LAYOUT_NHWC, GRAD_LAYOUT_PLANES = 0, 1   # RMNET_GRAD_LAYOUT_*


def _planes_strides(g):
    """(sn, sc) when 4-D ``g`` is made of H x W planes that are dense in themselves and do not fold onto each other, else None."""
    N, C, H, W = g.shape
    st = g.stride()
    if (W > 1 and st[3] != 1) or (H > 1 and st[2] != W):
        return None
    sc = st[1] if C > 1 else H * W
    sn = st[0] if N > 1 else (C - 1) * sc + H * W
    return (sn, sc) if sc >= H * W and sn >= (C - 1) * sc + H * W else None


def conv_grad_stage_rect(g, rects=None, amax=None):
    """The stage pass for the gradients the memory read hands back (csrc/conv_wgrad_n.hip: grad_stage_rect), one kernel and no host
    synchronisation: ``gs`` = a new dense channels-last [N, C, H, W] tensor with ``gs[n, c, y, x] = g[n, c, y, x] * 2^s`` where
    (x, y) lies inside ``rects[n]`` = (cx0, cx1, cy0, cy1) (int32 [N, 4] on the device, inclusive, clamped to the map: the
    convention of ``conv_split(..., rects=)``) and +0.0 elsewhere -- a select: NaN or Inf outside a rectangle does not reach
    ``gs``.  Without ``rects`` it is a layout + scale pass.  ``g`` (fp32, C % 4 == 0) is channels-last dense, or made of planes:
    element (n, c, y, x) at ``n * sn + c * sc + y * W + x`` (an NCHW tensor, one of the regional pair, a ``[:, :, t]`` slice of
    [no, C, Tcap, h, w]).  ``s = conv_grad_stage_exponent(amax)``; ``amax`` is a 0-dim upper bound of |g| on the device, taken
    before the mask (default: the largest |element| of ``g`` as given, one reduction).  Returns ``(gs, g_scale)`` as
    ``conv_grad_stage`` does."""
    if not isinstance(g, torch.Tensor) or not g.is_cuda or g.dtype != torch.float32:
        raise RuntimeError('g must be a CUDA torch.float32 tensor')
    if g.dim() != 4 or g.numel() == 0 or g.shape[1] % 4:
        raise RuntimeError('conv_grad_stage_rect needs a non-empty [N, C, H, W] g with C %% 4 == 0, got %s' % (tuple(g.shape),))
    N, C, H, W = g.shape
    if g.is_contiguous(memory_format=torch.channels_last):
        layout, sn, sc = GRAD_LAYOUT_NHWC, 0, 0
    else:
        st = _planes_strides(g)
        if st is None:
            raise RuntimeError('conv_grad_stage_rect: g must be channels-last dense or made of dense H x W planes, got strides %s'
                               % (g.stride(),))
        layout, (sn, sc) = GRAD_LAYOUT_PLANES, st
    if amax is None:
        amax = torch.linalg.vector_norm(g, float('inf'))
    _check(amax, 'amax')
    if amax.numel() != 1:
        raise RuntimeError('amax must hold one element')
    if rects is not None:
        _check(rects, 'rects', torch.int32)
        if tuple(rects.shape) != (N, 4) or not rects.is_contiguous():
            raise RuntimeError('rects must be a contiguous [N, 4] = %s tensor, got %s' % ((N, 4), tuple(rects.shape)))
    for t in (amax, rects):
        if t is not None and t.device != g.device:
            raise RuntimeError('conv_grad_stage_rect: every tensor must be on %s' % g.device)
    gs = torch.empty((N, C, H, W), dtype=torch.float32, device=g.device, memory_format=torch.channels_last)
    g_scale = torch.empty(4, dtype=torch.float32, device=g.device)[:2]
    with torch.cuda.device(g.device):
        rc = _lib.load().rmnet_conv_grad_stage_rect_f32(_ptr(g), layout, sn, sc, _ptr(rects), _ptr(amax), N, C, H, W, _ptr(gs),
                                                        _ptr(g_scale), _stream(g.device))
    _lib.check(rc, 'rmnet_conv_grad_stage_rect_f32')
    conv_grad_launches['stage'] += 1
    return gs, g_scale


@torch.no_grad()
def conv_split_dgrad_pack(weight):
    """The pack of the data gradient of a [Cout, Cin, 3, 3] stride 1 / pad 1 convolution on ``conv_split``, Cout % 32 == 0 and
    Cin % 64 == 0: dX = conv(G, W transposed and flipped), a convolution with Cout inputs and Cin outputs.  Returns
    ``conv_split_pack(weight.transpose(0, 1).flip(2, 3))``."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] % 32 or weight.shape[1] % 64:
        raise RuntimeError('conv_split_dgrad_pack needs a [Cout, Cin, 3, 3] weight with Cout %% 32 == 0 and Cin %% 64 == 0, got %s'
                           % (tuple(weight.shape),))
    conv_grad_launches['pack'] += 1
    return conv_split_pack(weight.detach().transpose(0, 1).flip(2, 3))


def kv_dgrad(gs_key, scale_key, gs_val, scale_val, packs, range_word=None):
    """The data gradient of the two key / value heads from their staged gradients (``conv_grad_stage_rect``; fp32 channels-last
    [N, keydim, H, W] and [N, valdim, H, W], each with its OWN staging scale): ``packs`` = the two ``conv_split_dgrad_pack``
    results, key head first.  Two ``conv_split`` calls (ksize 3, stride 1): the first writes dX of the key head, the second takes
    it as ``res`` and ``out``; each uses ``w_unscale / (g_scale[0] * g_scale[1])`` of its own head (exact: powers of two).  A head
    given as None launches nothing.  ``range_word``: the backward's (``conv_grad_range_word``)."""
    dx = None
    for gs, sc, (wp, wu) in ((gs_key, scale_key, packs[0]), (gs_val, scale_val, packs[1])):
        if gs is None:
            continue
        inv = sc.reciprocal()
        dx = conv_split(gs, wp, wu * inv[0] * inv[1], res=dx, ksize=3, out=dx, range_word=range_word)
        conv_grad_launches['dgrad'] += 1
    if dx is None:
        raise RuntimeError('kv_dgrad: at least one head must have a gradient')
    return dx


def kv_heads(x, wpack, w_unscale, bias, split, rects=None, presplit=True):
    """The two key / value heads in one launch over their concatenated pack: (key, value) for a channels-last fp32 ``x``.  With
    ``presplit`` x is split once (``split_act``); with ``rects`` as well (and no more images than KV_REGION_MAX_OBJECTS) the
    heads are computed only inside the rectangles and come back NCHW-contiguous (``conv_split(..., rects=)``)."""
    rw = conv_range_word(x.device)
    if presplit:
        x = split_act(x, range_word=rw)
        if kv_regional(x.shape[0], rects, presplit):
            return conv_split(x, wpack, w_unscale, bias, ksize=3, range_word=rw, split=split, rects=rects)
    return conv_split(x, wpack, w_unscale, bias, ksize=3, range_word=rw, split=split)


def kv_regional(n, rects, presplit):
    """Whether ``kv_heads`` runs the regional kernel for ``n`` images."""
    return bool(presplit) and rects is not None and n <= KV_REGION_MAX_OBJECTS


class _KeyValueFn(torch.autograd.Function):
    """The key / value heads under autograd (``KeyValue.device_grad_``): the forward is ``kv_heads``; saves x and the rectangles,
    nothing else.  ``pack`` = (wpack, w_unscale, bias of both heads, split, dgrad packs or None, presplit)."""

    @staticmethod
    def forward(ctx, x, w_key, b_key, w_val, b_val, pack, rects):
        wp, wu, bkv, split, dgrad_packs, presplit = pack
        if ctx.needs_input_grad[0] and dgrad_packs is None:
            raise RuntimeError('_KeyValueFn: the gradient with respect to x needs the dgrad packs')
        key, value = kv_heads(x.detach(), wp, wu, bkv, split, rects, presplit)
        ctx.regional = kv_regional(x.shape[0], rects, presplit)
        ctx.dgrad_packs = dgrad_packs if ctx.needs_input_grad[0] else None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, *((rects,) if ctx.regional else ()))
        return key, value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_key, g_val):
        saved = ctx.saved_tensors
        x = saved[0].detach()
        rects = saved[1] if ctx.regional else None
        need_x = ctx.needs_input_grad[0]
        grw = conv_grad_range_word(x.device)
        staged, grads = [], []
        for g, need_w, need_b in ((g_key, ctx.needs_input_grad[1], ctx.needs_input_grad[2]),
                                  (g_val, ctx.needs_input_grad[3], ctx.needs_input_grad[4])):
            gs = sc = gw = gb = None
            if g is not None and (need_x or need_w or need_b):
                if not g.is_contiguous(memory_format=torch.channels_last) and _planes_strides(g) is None:
                    g = g.contiguous()                                      # (an expanded grad_output becomes a plain tensor)
                gs, sc = conv_grad_stage_rect(g, rects)
                if need_w:
                    gw, gb = conv3x3_wgrad(x, gs, sc, want_bias=need_b, range_word=grw)
                elif need_b:                                                # (a trainable bias on frozen weights: no GEMM)
                    inv = sc.reciprocal()
                    gb = gs.sum(dim=(0, 2, 3)) * inv[0] * inv[1]
            staged += [gs, sc]
            grads += [gw, gb]
        gx = None
        if need_x and (staged[0] is not None or staged[2] is not None):
            gx = kv_dgrad(staged[0], staged[1], staged[2], staged[3], ctx.dgrad_packs, range_word=grw)
        return (gx,) + tuple(grads) + (None, None)


@torch.no_grad()
def conv_split_pack(weight, bn_scale=None):
    """[Cout, Cin, k, k] fp32 weight (k = 1 or 3, Cin % 32 == 0, Cout % 64 == 0), optionally times a per-output-channel
    ``bn_scale`` (a folded BatchNorm: the product is formed in float64) -> (wpack [k*k * Cin * Cout * 2] fp16 bits as int16,
    w_unscale fp32 [Cout]) in the layout of include/rmnet_hip.h (rmnet_conv_split_f32): per output channel a power-of-two scale
    2^e puts max |w * bn_scale| in [2^14, 2^15), the scaled product is split into fp16 hi = rne(ws), lo = rne(ws - hi) and laid
    out as [tap][Cin / 32][hi, lo][co][Cin % 32].  hi + lo, unscaled, is w * bn_scale to ~2^-22 relative."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3) or weight.shape[1] % 32 \
            or weight.shape[0] % 64:
        raise RuntimeError('conv_split_pack needs a [Cout, Cin, k, k] weight with k in (1, 3), Cin % 32 == 0 and Cout % 64 == 0, '
                           'got %s' % (tuple(weight.shape),))
    if weight.dtype != torch.float32:
        raise RuntimeError('conv_split_pack needs fp32 weights, got %s' % weight.dtype)
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    w = weight.detach().double()
    if bn_scale is not None:
        if bn_scale.numel() != cout:
            raise RuntimeError('bn_scale must have Cout = %d elements' % cout)
        w = w * bn_scale.detach().to(w.device, torch.float64).view(-1, 1, 1, 1)
    amax = w.abs().amax(dim=(1, 2, 3))
    _, ex = torch.frexp(amax)                              # amax in [2^(ex-1), 2^ex)
    e = torch.where(amax > 0, 15 - ex, torch.zeros_like(ex))
    ws = torch.ldexp(w, e.view(-1, 1, 1, 1).to(w.dtype))   # exact: power-of-two scaling
    hi = ws.half()
    lo = (ws - hi.double()).half()
    planes = torch.stack([p.reshape(cout, cin // 32, 32, k * k).permute(3, 1, 0, 2) for p in (hi, lo)], dim=2)
    unscale = torch.ldexp(torch.ones_like(amax), (-e).to(amax.dtype)).float()
    return planes.contiguous().view(-1).view(torch.int16), unscale.contiguous()


CONV_X_SPLIT, CONV_OUT_SPLIT = 4, 8  # RMNET_CONV_X_SPLIT / RMNET_CONV_OUT_SPLIT


def is_split_act(t):
    """``t`` is an activation in the split form of include/rmnet_hip.h: torch.float16 [N, H, W, C // 32, 2, 32], contiguous."""
    return isinstance(t, torch.Tensor) and t.dtype == torch.float16 and t.dim() == 6 and tuple(t.shape[4:]) == (2, 32)


def _check_split_act(t, name):
    if not is_split_act(t):
        raise RuntimeError('%s must be a split activation: torch.float16 [N, H, W, C // 32, 2, 32]' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor' % name)
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)


def split_act(x, relu=False, range_word=None):
    """Channels-last fp32 ``x`` [N, C, H, W], C % 32 == 0 -> its split form, torch.float16 [N, H, W, C // 32, 2, 32]
    (include/rmnet_hip.h; csrc/conv_split.hip: split_act), after a ReLU when ``relu``.  Elements outside the window are saturated
    and counted in ``range_word`` here, once each; ``conv_split`` on the result counts nothing.  For tensors that another kernel
    produced: ``conv_split(..., out_presplit=True)`` writes the form itself."""
    _check_act(x, 'x')
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('x must be a channels-last [N, C, H, W] tensor')
    N, C, H, W = x.shape
    if C % 32 or x.numel() == 0:
        raise RuntimeError('split_act needs C % 32 == 0 and a non-empty tensor, got %s' % (tuple(x.shape),))
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
        if range_word.device != x.device:
            raise RuntimeError('split_act: every tensor must be on %s' % x.device)
    out = torch.empty((N, H, W, C // 32, 2, 32), dtype=torch.float16, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        rc = lib.rmnet_split_act_f32(_ptr(x), N * H * W, C, 1 if relu else 0, _ptr(out), _ptr(range_word), _stream(x.device))
    _lib.check(rc, 'rmnet_split_act_f32')
    return out


# The trunks' stride-1 3x3 bottleneck convolutions (split input, Cin == Cout, no residual) on conv_rows (csrc/conv_rows.hip: a tap
# row's activations staged in LDS once; the same bits) when RMNET_TRUNK_ROWS is not set, for the channel counts of
# TRUNK_ROWS_CLASSES.  The rules (profiles/r21_a_trunk_rows.md): the default is True only if every bench run with it is above every
# run of the parent commit; a class is listed only if its per-call time in a kernel trace falls by more than the classes whose code
# did not change move.  TRUNK_ROWS_ALL is what the export implements; the 64-channel class (layer1, 1/4 maps) measured the same
# time on either kernel (-1.0 % in the trace, inside the -0.2 to +1.3 % of the unchanged classes) and stays on conv_split_pre.
TRUNK_ROWS_DEFAULT = True
TRUNK_ROWS_ENTRY = 'rmnet_conv_rows_pre_f32'
TRUNK_ROWS_ALL = (64, 128, 256)
TRUNK_ROWS_CLASSES = (128, 256)


def trunk_rows_enabled():
    """RMNET_TRUNK_ROWS ('0' or '1', read at every call; unset: TRUNK_ROWS_DEFAULT).  Any other value is a RuntimeError."""
    v = os.environ.get('RMNET_TRUNK_ROWS')
    if v is None:
        return TRUNK_ROWS_DEFAULT
    if v.strip() not in ('0', '1'):
        raise RuntimeError("RMNET_TRUNK_ROWS must be '0' or '1', got %r" % v)
    return v.strip() == '1'


# The key / value heads of ``RMNet.frame_step`` on the regional kernel (csrc/conv_split.hip: conv_split_region -- only the cells
# inside the boxes are computed, the outputs are NCHW; the same bits inside the boxes) when RMNET_KV_REGION is not set.  The rule:
# True only if every bench run with it is above every run of the parent commit (profiles/r33_a_kv_region.md).
KV_REGION_DEFAULT = True
KV_REGION_ENTRY = 'rmnet_conv_split_region_f32'
KV_REGION_MAX_OBJECTS = 64       # csrc/conv_split.hip kRegionMaxObjects: more images per call go to the dense head


def kv_region_enabled():
    """RMNET_KV_REGION ('0' or '1', read at every call; unset: KV_REGION_DEFAULT).  Any other value is a RuntimeError."""
    v = os.environ.get('RMNET_KV_REGION')
    if v is None:
        return KV_REGION_DEFAULT
    if v.strip() not in ('0', '1'):
        raise RuntimeError("RMNET_KV_REGION must be '0' or '1', got %r" % v)
    return v.strip() == '1'


def conv_split(x, wpack, w_unscale, shift=None, res=None, ksize=3, stride=1, relu_in=False, relu_out=False, out=None,
               range_word=None, split=None, out_presplit=False, rects=None, _out=None):
    """act(conv(pre(x), w) + shift + res) for a channels-last fp32 ``x`` [N, Cin, H, W], kernel ``ksize`` (1 or 3, padding
    ksize // 2), ``stride`` (1 or 2) and Cout = ``w_unscale.numel()`` (a multiple of 64) on the split-fp16 MFMA kernel
    (csrc/conv_split.hip); ``pre`` / ``act`` = ReLU when ``relu_in`` / ``relu_out``.  ``wpack, w_unscale`` come from
    ``conv_split_pack``.  ``out`` (channels-last, may be ``res``, must not be ``x``) defaults to a new tensor.  ``range_word``: as
    for ``conv3x3_split``.  ``split`` (a multiple of 4 inside (0, Cout), no ``res`` / ``out``): the output channels [0, split) and
    [split, Cout) are written to two new channels-last tensors, returned as a pair.

    Pre-split activations (include/rmnet_hip.h): ``x`` may be a split activation (torch.float16 [N, H, W, Cin // 32, 2, 32], from
    ``split_act`` or from ``out_presplit``); ``relu_in`` is then refused and nothing is counted for the input.  With
    ``out_presplit`` the result is returned in that form instead of fp32 (no ``out``, no ``split``) and its elements outside the
    window are counted in ``range_word``.  Same arithmetic and same bits either way.  No fall-back: anything else is a
    RuntimeError.

    ``rects`` (int32 [N, 4] on the device: one cell rectangle (cx0, cx1, cy0, cy1) per image, inclusive, clamped to the map by the
    kernel): the regional form, for a split-activation ``x``, ``ksize=3``, ``stride=1``, ``split=`` and Cout % 128 == 0.  The pair
    is returned NCHW-contiguous; a cell inside its image's rectangle holds the bits of the call without ``rects``, every other
    cell is +0.0.  Only the cells inside the rectangles are computed.  (``_out``: the pair to write, for the tests.)"""
    x_split = is_split_act(x)
    if x_split:
        _check_split_act(x, 'x')
        N, H, W = x.shape[:3]
        cin = x.shape[3] * 32
        if relu_in:
            raise RuntimeError('conv_split: relu_in cannot be applied to a split activation (its producer applies it)')
    else:
        _check_act(x, 'x')
        if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError('x must be a channels-last [N, Cin, H, W] tensor')
        N, cin, H, W = x.shape
    if ksize not in (1, 3) or stride not in (1, 2):
        raise RuntimeError('conv_split implements ksize 1 / 3 and stride 1 / 2, got %r / %r' % (ksize, stride))
    _check(w_unscale, 'w_unscale')
    cout = w_unscale.numel()
    if cin % 32 or cout % 64 or cout == 0:
        raise RuntimeError('conv_split needs Cin % 32 == 0 and Cout % 64 == 0, got %d, %d' % (cin, cout))
    _check(wpack, 'wpack', torch.int16)
    if wpack.numel() != ksize * ksize * cin * cout * 2:
        raise RuntimeError('wpack has %d elements, a %dx%d Cin = %d Cout = %d pack has %d'
                           % (wpack.numel(), ksize, ksize, cin, cout, ksize * ksize * cin * cout * 2))
    pad = ksize // 2
    shape = (N, cout, (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1)
    if shift is not None:
        _check(shift, 'shift')
        if shift.numel() != cout:
            raise RuntimeError('shift must have Cout = %d elements' % cout)
    if res is not None:
        _check_act(res, 'res')
        if tuple(res.shape) != shape or not res.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError('res must be a channels-last %s tensor' % (shape,))
    out2 = None
    if rects is not None:
        if not x_split or ksize != 3 or stride != 1 or split is None or res is not None or out is not None or out_presplit \
                or relu_in or cout % 128 or not 0 < split < cout or split % 4:
            raise RuntimeError('conv_split: rects needs a split-activation x, ksize 3, stride 1, split= (a multiple of 4 in (0, Cout)) '
                               'and Cout % 128 == 0, without res / out / out_presplit')
        _check(rects, 'rects', torch.int32)
        if tuple(rects.shape) != (N, 4):
            raise RuntimeError('rects must be [N, 4] = %s, got %s' % ((N, 4), tuple(rects.shape)))
        if _out is None:
            out = torch.empty((N, split) + shape[2:], dtype=torch.float32, device=x.device)
            out2 = torch.empty((N, cout - split) + shape[2:], dtype=torch.float32, device=x.device)
        else:
            out, out2 = _out
            for t, c in ((out, split), (out2, cout - split)):
                _check(t, '_out')
                if tuple(t.shape) != (N, c) + shape[2:]:
                    raise RuntimeError('_out must be the NCHW pair %s / %s' % ((N, split) + shape[2:], (N, cout - split) + shape[2:]))
    elif _out is not None:
        raise RuntimeError('conv_split: _out goes with rects')
    elif out_presplit:
        if split is not None or out is not None:
            raise RuntimeError('conv_split: out_presplit returns one new split activation, without split / out')
        out = torch.empty((N, shape[2], shape[3], cout // 32, 2, 32), dtype=torch.float16, device=x.device)
    elif split is not None:
        if res is not None or out is not None or not 0 < split < cout or split % 4:
            raise RuntimeError('conv_split: split must be a multiple of 4 in (0, %d), without res / out' % cout)
        out = torch.empty((N, split) + shape[2:], dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        out2 = torch.empty((N, cout - split) + shape[2:], dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    elif out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    else:
        _check_act(out, 'out')
        if tuple(out.shape) != shape or not out.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError('out must be a channels-last %s tensor' % (shape,))
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
    for t in (wpack, w_unscale, shift, res, out, out2, range_word, rects):
        if t is not None and t.device != x.device:
            raise RuntimeError('conv_split: every tensor must be on %s' % x.device)
    flags = (CONV_RELU_IN if relu_in else 0) | (CONV_RELU_OUT if relu_out else 0)
    if rects is not None:
        with torch.cuda.device(x.device):
            rc = _lib.load().rmnet_conv_split_region_f32(_ptr(x), _ptr(wpack), _ptr(w_unscale), _ptr(shift), flags | CONV_X_SPLIT, N, H, W,
                                                         cin, cout, ksize, stride, _ptr(rects), _ptr(out), _ptr(out2), split,
                                                         _ptr(range_word), _stream(x.device))
        _lib.check(rc, KV_REGION_ENTRY)
        return out, out2
    # conv_rows: the switch on (read at every call, so a bad value raises whatever the shape), and the class it serves
    rows = trunk_rows_enabled() and x_split and ksize == 3 and stride == 1 and cin == cout and cin in TRUNK_ROWS_CLASSES \
        and res is None and split is None
    lib = _lib.load()
    with torch.cuda.device(x.device):
        if x_split or out_presplit:
            flags |= (CONV_X_SPLIT if x_split else 0) | (CONV_OUT_SPLIT if out_presplit else 0)
            what = TRUNK_ROWS_ENTRY if rows else 'rmnet_conv_split_pre_f32'
            rc = getattr(lib, what)(_ptr(x), _ptr(wpack), _ptr(w_unscale), _ptr(shift), _ptr(res), flags, N, H, W, cin,
                                    cout, ksize, stride, _ptr(out), _ptr(out2), split or 0, _ptr(range_word),
                                    _stream(x.device))
        else:
            what = 'rmnet_conv_split_f32'
            rc = lib.rmnet_conv_split_f32(_ptr(x), _ptr(wpack), _ptr(w_unscale), _ptr(shift), _ptr(res), flags, N, H, W, cin, cout,
                                          ksize, stride, _ptr(out), _ptr(out2), split or 0, _ptr(range_word), _stream(x.device))
    _lib.check(rc, what)
    return out if out2 is None else (out, out2)


FLOW_RELU, FLOW_LEAKY, FLOW_TRANSPOSED = 1, 2, 4   # RMNET_FLOW_*
_FLOW_ACT = {None: 0, False: 0, 'none': 0, True: FLOW_RELU, 'relu': FLOW_RELU, 'leaky': FLOW_LEAKY}


def flow_conv_phase_weights(weight):
    """ConvTranspose2d(4, stride 2, padding 1) weight [Cin, Cout, 4, 4] -> [4, Cout, Cin, 2, 2]: the four 2x2-tap forward kernels of
    the output parities.  Phase 2a + b computes the output pixels (2i + a, 2j + b) from the input pixels (i + a - 1 + ty,
    j + b - 1 + tx), ty, tx in {0, 1}, with the weight of ky = 3 - a - 2 ty, kx = 3 - b - 2 tx (from y = 2 iy - 1 + ky)."""
    w = weight.permute(1, 0, 2, 3)
    phases = []
    for a in (0, 1):
        for b in (0, 1):
            ky = torch.tensor([3 - a, 1 - a], device=w.device)
            kx = torch.tensor([3 - b, 1 - b], device=w.device)
            phases.append(w.index_select(2, ky).index_select(3, kx))
    return torch.stack(phases, 0)


@torch.no_grad()
def flow_conv_pack(weight, transposed=False):
    """fp32 weight -> (wpack fp16 bits as int16, w_unscale fp32 [Cout]) in the layout of include/rmnet_hip.h (rmnet_flow_conv_f32):
    ``conv_split_pack``'s scheme -- per output channel a power-of-two scale 2^e puts max |w| in [2^14, 2^15), hi = rne(ws),
    lo = rne(ws - hi), [tap][Cin_p / 32][hi, lo][co][32] -- with the input channels zero-padded to Cin_p = ceil32(Cin).
    ``transposed=False``: a [Cout, Cin, k, k] Conv2d weight, k = 3 or 5, one pack.  ``transposed=True``: a [Cin, Cout, 4, 4]
    ConvTranspose2d(4, stride 2, padding 1) weight, rearranged into the four 2x2-tap phase packs (``flow_conv_phase_weights``), one
    after the other, under one scale per output channel.  Cout % 64 == 0."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in ((4,) if transposed else (3, 5)):
        raise RuntimeError('flow_conv_pack needs a [Cout, Cin, k, k] weight with k in (3, 5), or transposed a [Cin, Cout, 4, 4] one, '
                           'got %s' % (tuple(weight.shape),))
    if weight.dtype != torch.float32:
        raise RuntimeError('flow_conv_pack needs fp32 weights, got %s' % weight.dtype)
    w = weight.detach().double()
    w = flow_conv_phase_weights(w) if transposed else w.unsqueeze(0)          # [P, Cout, Cin, KH, KW]
    P, cout, cin, kh, kw = w.shape
    if cout % 64:
        raise RuntimeError('flow_conv_pack needs Cout % 64 == 0, got ' + str(cout))
    cp = (cin + 31) // 32 * 32
    amax = w.abs().amax(dim=(0, 2, 3, 4))
    _, ex = torch.frexp(amax)                              # amax in [2^(ex-1), 2^ex)
    e = torch.where(amax > 0, 15 - ex, torch.zeros_like(ex))
    ws = torch.ldexp(w, e.view(1, -1, 1, 1, 1).to(w.dtype))   # exact: power-of-two scaling
    hi = ws.half()
    lo = (ws - hi.double()).half()
    pad = lambda p: torch.nn.functional.pad(p, (0, 0, 0, 0, 0, cp - cin))
    planes = torch.stack([pad(p).reshape(P, cout, cp // 32, 32, kh * kw).permute(0, 4, 2, 1, 3) for p in (hi, lo)], dim=3)
    unscale = torch.ldexp(torch.ones_like(amax), (-e).to(amax.dtype)).float()
    return planes.contiguous().view(-1).view(torch.int16), unscale.contiguous()


def flow_conv_out_hw(H, W, ksize, stride, transposed):
    if transposed:
        return 2 * H, 2 * W
    pad = ksize // 2
    return (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1


def flow_conv(x, wpack, w_unscale, shift=None, *, ksize=3, stride=1, transposed=False, act=None, cin=None, out=None, out_coff=0,
              range_word=None):
    """act(conv(x[:, :cin], w) + shift) on the split-fp16 tap-list kernel (csrc/flow_conv.hip): a forward convolution with ``ksize``
    3 or 5 (padding ksize // 2) and ``stride`` 1 or 2, or, ``transposed``, ConvTranspose2d(4, stride 2, padding 1) (``ksize=4,
    stride=2``).  ``wpack, w_unscale`` come from ``flow_conv_pack``; Cout = ``w_unscale.numel()``.  ``act``: None, 'relu' or
    'leaky' (LeakyReLU(0.1), the expression of ``channel_affine``).
    ``x`` is a channels-last fp32 [N, x_ld, H, W] tensor of which the first ``cin`` channels (default: all) are the input: a
    channel-padded buffer, x_ld % 4 == 0 and x_ld >= ceil32(cin); what the channels cin .. ceil32(cin) - 1 hold does not matter.
    ``out``: None for a new channels-last [N, Cout, Ho, Wo] tensor, or a channels-last [N, out_ld, Ho, Wo] buffer of which only the
    channels ``out_coff .. out_coff + Cout - 1`` are written (both multiples of 4); it must not share memory with ``x``.  Returns
    ``out``.  ``range_word`` (int32 [1]): as for ``conv3x3_split``, but an element may be counted more than once.  No fall-back:
    anything else is a RuntimeError."""
    _check_act(x, 'x')
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('x must be a channels-last [N, C, H, W] tensor')
    if transposed:
        if ksize != 4 or stride != 2:
            raise RuntimeError('flow_conv implements the transposed convolution for ksize 4 / stride 2, got %r / %r' % (ksize, stride))
    elif ksize not in (3, 5) or stride not in (1, 2):
        raise RuntimeError('flow_conv implements ksize 3 / 5 and stride 1 / 2, got %r / %r' % (ksize, stride))
    if act not in _FLOW_ACT:
        raise RuntimeError("act must be None, 'relu' or 'leaky', got %r" % (act,))
    N, x_ld, H, W = x.shape
    cin = x_ld if cin is None else int(cin)
    cp = (cin + 31) // 32 * 32
    if cin <= 0 or x_ld % 4 or x_ld < cp:
        raise RuntimeError('flow_conv needs x_ld %% 4 == 0 and x_ld >= ceil32(cin): x has %d channels for cin = %d' % (x_ld, cin))
    _check(w_unscale, 'w_unscale')
    cout = w_unscale.numel()
    if cout % 64 or cout == 0:
        raise RuntimeError('flow_conv needs Cout % 64 == 0, got ' + str(cout))
    _check(wpack, 'wpack', torch.int16)
    want = (16 if transposed else ksize * ksize) * cp * cout * 2
    if wpack.numel() != want:
        raise RuntimeError('wpack has %d elements, a %dx%d%s cin = %d Cout = %d pack has %d'
                           % (wpack.numel(), ksize, ksize, ' transposed' if transposed else '', cin, cout, want))
    if shift is not None:
        _check(shift, 'shift')
        if shift.numel() != cout:
            raise RuntimeError('shift must have Cout = %d elements' % cout)
    Ho, Wo = flow_conv_out_hw(H, W, ksize, stride, transposed)
    if out is None:
        if out_coff:
            raise RuntimeError('out_coff without out')
        out = torch.empty((N, cout, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    else:
        _check_act(out, 'out')
        if out.dim() != 4 or not out.is_contiguous(memory_format=torch.channels_last) or \
                (out.shape[0], out.shape[2], out.shape[3]) != (N, Ho, Wo):
            raise RuntimeError('out must be a channels-last [%d, out_ld, %d, %d] tensor' % (N, Ho, Wo))
        if out.shape[1] % 4 or out_coff % 4 or out_coff < 0 or out_coff + cout > out.shape[1]:
            raise RuntimeError('flow_conv needs out_ld %% 4 == 0, out_coff %% 4 == 0 and out_coff + Cout <= out_ld, got %d, %d, %d'
                               % (out.shape[1], out_coff, cout))
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
    for t in (wpack, w_unscale, shift, out, range_word):
        if t is not None and t.device != x.device:
            raise RuntimeError('flow_conv: every tensor must be on %s' % x.device)
    flags = _FLOW_ACT[act] | (FLOW_TRANSPOSED if transposed else 0)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        rc = lib.rmnet_flow_conv_f32(_ptr(x), x_ld, _ptr(wpack), _ptr(w_unscale), _ptr(shift), flags, N, H, W, cin, cout, ksize, stride,
                                     _ptr(out), out.shape[1], out_coff, _ptr(range_word), _stream(x.device))
    _lib.check(rc, 'rmnet_flow_conv_f32')
    return out


FLOW_HEAD_SLICE = 32              # csrc/flow_head.hip kCS: input channels per workgroup; the pack is padded to a multiple of it


@torch.no_grad()
def flow_head_pack(weight):
    """[2, Cin, 3, 3] fp32 flow-head weight (any memory format) -> wpack fp32 [ceil32(Cin) * 9 * 2] in the layout of
    include/rmnet_hip.h (rmnet_flow_head_f32): weight[co][c][ky][kx], unrounded, at (c * 9 + 3 * ky + kx) * 2 + co, zero for
    c >= Cin."""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or weight.shape[0] != 2 or tuple(weight.shape[2:]) != (3, 3) \
            or weight.shape[1] < 1:
        raise RuntimeError('flow_head_pack needs a [2, Cin, 3, 3] weight, got %s' % (tuple(getattr(weight, 'shape', ())),))
    if weight.dtype != torch.float32:
        raise RuntimeError('flow_head_pack needs fp32 weights, got %s' % weight.dtype)
    cin = weight.shape[1]
    cp = (cin + FLOW_HEAD_SLICE - 1) // FLOW_HEAD_SLICE * FLOW_HEAD_SLICE
    pack = torch.zeros(cp, 9, 2, dtype=torch.float32, device=weight.device)
    pack[:cin] = weight.detach().permute(1, 2, 3, 0).reshape(cin, 9, 2)
    return pack.view(-1)


def flow_head(x, wpack, bias, cin=None):
    """conv3x3_p1(x[:, :cin], w) + bias with two output channels in plain fp32 FMA (csrc/flow_head.hip) -> NCHW-contiguous
    [N, 2, H, W].  ``x`` is a channels-last fp32 [N, x_ld, H, W] tensor of which the first ``cin`` channels (default: all) are the
    input, x_ld % 4 == 0; what the channels cin .. x_ld - 1 hold does not matter (NaN included).  ``wpack`` comes from
    ``flow_head_pack`` of a [2, cin, 3, 3] weight, ``bias`` is fp32 [2].  The result has a fixed order of summation: the same bits
    from call to call and for any N.  No fall-back: anything else is a RuntimeError."""
    _check_act(x, 'x')
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('x must be a channels-last [N, C, H, W] tensor')
    N, x_ld, H, W = x.shape
    cin = x_ld if cin is None else int(cin)
    if cin <= 0 or x_ld % 4 or x_ld < cin:
        raise RuntimeError('flow_head needs x_ld %% 4 == 0 and x_ld >= cin >= 1: x has %d channels for cin = %d' % (x_ld, cin))
    _check(wpack, 'wpack')
    want = (cin + FLOW_HEAD_SLICE - 1) // FLOW_HEAD_SLICE * FLOW_HEAD_SLICE * 18
    if wpack.numel() != want:
        raise RuntimeError('wpack has %d elements, a cin = %d flow-head pack has %d' % (wpack.numel(), cin, want))
    _check(bias, 'bias')
    if bias.numel() != 2:
        raise RuntimeError('bias must have 2 elements')
    if wpack.device != x.device or bias.device != x.device:
        raise RuntimeError('flow_head: every tensor must be on %s' % x.device)
    if N == 0 or H == 0 or W == 0:
        raise RuntimeError('flow_head needs a non-empty x, got %s' % (tuple(x.shape),))
    out = torch.empty((N, 2, H, W), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        nb = lib.rmnet_flow_head_workspace_bytes(N, H, W, cin)
        ws = _ws(nb, x.device)
        rc = lib.rmnet_flow_head_f32(_ptr(x), x_ld, _ptr(wpack), _ptr(bias), N, H, W, cin, _ptr(out), _ptr(ws), nb, _stream(x.device))
    _lib.check(rc, 'rmnet_flow_head_f32')
    return out


def flow_up(flow, weight, out, coff):
    """ConvTranspose2d(2, 2, 4, stride 2, padding 1, bias=False) of ``flow`` [N, 2, h, w] (NCHW fp32, a flow head's output) with
    ``weight`` [2, 2, 4, 4] (NCHW-contiguous), written into the channels ``coff, coff + 1`` of the channels-last fp32 buffer ``out``
    [N, out_ld, 2h, 2w]; the channels ``coff + 2 .. out_ld - 1`` are set to +0.0 and nothing else is written (csrc/flow_head.hip).
    out_ld % 4 == 0, coff % 4 == 0, coff + 2 <= out_ld.  Returns ``out``.  No fall-back: anything else is a RuntimeError."""
    _check(flow, 'flow')
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise RuntimeError('flow must be [N, 2, h, w]')
    N, _, h, w = flow.shape
    if N == 0 or h == 0 or w == 0:
        raise RuntimeError('flow_up needs a non-empty flow, got %s' % (tuple(flow.shape),))
    _check(weight, 'weight')
    if tuple(weight.shape) != (2, 2, 4, 4):
        raise RuntimeError('flow_up needs a [2, 2, 4, 4] weight, got %s' % (tuple(weight.shape),))
    _check_act(out, 'out')
    if out.dim() != 4 or not out.is_contiguous(memory_format=torch.channels_last) or \
            (out.shape[0], out.shape[2], out.shape[3]) != (N, 2 * h, 2 * w):
        raise RuntimeError('out must be a channels-last [%d, out_ld, %d, %d] tensor' % (N, 2 * h, 2 * w))
    coff = int(coff)
    if out.shape[1] % 4 or coff % 4 or coff < 0 or coff + 2 > out.shape[1]:
        raise RuntimeError('flow_up needs out_ld %% 4 == 0, coff %% 4 == 0 and coff + 2 <= out_ld, got %d, %d' % (out.shape[1], coff))
    if weight.device != flow.device or out.device != flow.device:
        raise RuntimeError('flow_up: every tensor must be on %s' % flow.device)
    lib = _lib.load()
    with torch.cuda.device(flow.device):
        rc = lib.rmnet_flow_up_f32(_ptr(flow), _ptr(weight), N, h, w, _ptr(out), out.shape[1], coff, _stream(flow.device))
    _lib.check(rc, 'rmnet_flow_up_f32')
    return out


STEM_COUT = 64                    # csrc/stem.hip: output channels of the encoder stems


def stem_kp(cin):
    """Padded K of the stem pack: 49 * Cin rounded up to a multiple of 32 (147 -> 160, 245 -> 256)."""
    return (49 * cin + 31) // 32 * 32


@torch.no_grad()
def stem_pack(weight, bn_scale=None):
    """[64, Cin, 7, 7] fp32 stem weight (Cin 3, or 5 = conv1 | conv1_m | conv1_o stacked), optionally times a per-output-channel
    ``bn_scale`` (the folded BatchNorm: the product is formed in float64) -> (wpack [Kp * 64 * 2] fp16 bits as int16, w_unscale
    fp32 [64]) in the layout of include/rmnet_hip.h (rmnet_stem_split_f32): scale and hi / lo split as ``conv_split_pack``,
    K index k = (7 * ky + kx) * Cin + ci zero-padded to Kp = 160 / 256, laid out as [k / 32][hi, lo][co][k % 32]."""
    if weight.dim() != 4 or weight.shape[0] != STEM_COUT or weight.shape[1] not in (3, 5) or tuple(weight.shape[2:]) != (7, 7):
        raise RuntimeError('stem_pack needs a [64, Cin, 7, 7] weight with Cin 3 or 5, got %s' % (tuple(weight.shape),))
    if weight.dtype != torch.float32:
        raise RuntimeError('stem_pack needs fp32 weights, got %s' % weight.dtype)
    cin = weight.shape[1]
    w = weight.detach().double()
    if bn_scale is not None:
        if bn_scale.numel() != STEM_COUT:
            raise RuntimeError('bn_scale must have 64 elements')
        w = w * bn_scale.detach().to(w.device, torch.float64).view(-1, 1, 1, 1)
    amax = w.abs().amax(dim=(1, 2, 3))
    _, ex = torch.frexp(amax)                              # amax in [2^(ex-1), 2^ex)
    e = torch.where(amax > 0, 15 - ex, torch.zeros_like(ex))
    ws = torch.ldexp(w, e.view(-1, 1, 1, 1).to(w.dtype))   # exact: power-of-two scaling
    kp = stem_kp(cin)
    wk = torch.zeros(STEM_COUT, kp, dtype=torch.float64, device=w.device)
    wk[:, :49 * cin] = ws.permute(0, 2, 3, 1).reshape(STEM_COUT, 49 * cin)
    hi = wk.half()
    lo = (wk - hi.double()).half()
    planes = torch.stack([p.reshape(STEM_COUT, kp // 32, 32).permute(1, 0, 2) for p in (hi, lo)], dim=1)
    unscale = torch.ldexp(torch.ones_like(amax), (-e).to(amax.dtype)).float()
    return planes.contiguous().view(-1).view(torch.int16), unscale.contiguous()


def stem_split(frame, mask=None, other=None, wpack=None, w_unscale=None, shift=None, range_word=None):
    """max_pool2d(relu(conv7x7_s2_p3(x) * g + shift), 3, stride 2, padding 1) in one launch of the split-fp16 stem kernel
    (csrc/stem.hip) -> channels-last fp32 [N, 64, Hp, Wp].  ``frame`` [N, 3, H, W] NCHW; ``mask`` / ``other`` [N, H, W] (both None:
    the 3-channel query stem; ``mask`` given: the 5-channel memory stem, ``other`` None = an all-zero plane).  ``wpack, w_unscale``
    come from ``stem_pack`` (which folds g); ``range_word``: as for ``conv3x3_split``, counted per input element.  No fall-back:
    anything else is a RuntimeError."""
    _check(frame, 'frame')
    if frame.dim() != 4 or frame.shape[1] != 3:
        raise RuntimeError('frame must be [N, 3, H, W]')
    N, _, H, W = frame.shape
    if other is not None and mask is None:
        raise RuntimeError('stem_split: other without mask')
    for t, n in ((mask, 'mask'), (other, 'other')):
        if t is not None:
            _check(t, n)
            if tuple(t.shape) != (N, H, W):
                raise RuntimeError('%s must be [N, H, W] = %s' % (n, (N, H, W)))
    if wpack is None or w_unscale is None:
        raise RuntimeError('stem_split needs wpack and w_unscale (ops.stem_pack)')
    cin = 3 if mask is None else 5
    _check(wpack, 'wpack', torch.int16)
    if wpack.numel() != stem_kp(cin) * STEM_COUT * 2:
        raise RuntimeError('wpack has %d elements, a Cin = %d stem pack has %d' % (wpack.numel(), cin, stem_kp(cin) * STEM_COUT * 2))
    _check(w_unscale, 'w_unscale')
    if w_unscale.numel() != STEM_COUT:
        raise RuntimeError('w_unscale must have 64 elements')
    if shift is not None:
        _check(shift, 'shift')
        if shift.numel() != STEM_COUT:
            raise RuntimeError('shift must have 64 elements')
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
    for t in (mask, other, wpack, w_unscale, shift, range_word):
        if t is not None and t.device != frame.device:
            raise RuntimeError('stem_split: every tensor must be on %s' % frame.device)
    hc, wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, STEM_COUT, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1), dtype=frame.dtype, device=frame.device,
                      memory_format=torch.channels_last)
    lib = _lib.load()
    with torch.cuda.device(frame.device):
        rc = lib.rmnet_stem_split_f32(_ptr(frame), _ptr(mask), _ptr(other), _ptr(wpack), _ptr(w_unscale), _ptr(shift), N, H, W,
                                      _ptr(out), _ptr(range_word), _stream(frame.device))
    _lib.check(rc, 'rmnet_stem_split_f32')
    return out


FLOW_STEM_CIN = 6                 # csrc/flow_stem.hip: the frame pair's channels
FLOW_STEM_KP = 320                # 49 * 6 = 294 rounded up to a multiple of 32


@torch.no_grad()
def flow_stem_pack(weight):
    """[64, 6, 7, 7] fp32 weight of TinyFlowNet's conv1 -> (wpack [320 * 64 * 2] fp16 bits as int16, w_unscale fp32 [64]) in
    ``stem_pack``'s layout with Cin 6 (include/rmnet_hip.h, rmnet_flow_stem_f32): per-channel power-of-two scale, hi / lo split,
    K index k = (7 * ky + kx) * 6 + ci zero-padded from 294 to 320, laid out as [k / 32][hi, lo][co][k % 32]."""
    if tuple(weight.shape) != (STEM_COUT, FLOW_STEM_CIN, 7, 7):
        raise RuntimeError('flow_stem_pack needs a [64, 6, 7, 7] weight, got %s' % (tuple(weight.shape),))
    if weight.dtype != torch.float32:
        raise RuntimeError('flow_stem_pack needs fp32 weights, got %s' % weight.dtype)
    w = weight.detach().double()
    amax = w.abs().amax(dim=(1, 2, 3))
    _, ex = torch.frexp(amax)                              # amax in [2^(ex-1), 2^ex)
    e = torch.where(amax > 0, 15 - ex, torch.zeros_like(ex))
    ws = torch.ldexp(w, e.view(-1, 1, 1, 1).to(w.dtype))   # exact: power-of-two scaling
    wk = torch.zeros(STEM_COUT, FLOW_STEM_KP, dtype=torch.float64, device=w.device)
    wk[:, :49 * FLOW_STEM_CIN] = ws.permute(0, 2, 3, 1).reshape(STEM_COUT, 49 * FLOW_STEM_CIN)
    hi = wk.half()
    lo = (wk - hi.double()).half()
    planes = torch.stack([p.reshape(STEM_COUT, FLOW_STEM_KP // 32, 32).permute(1, 0, 2) for p in (hi, lo)], dim=1)
    unscale = torch.ldexp(torch.ones_like(amax), (-e).to(amax.dtype)).float()
    return planes.contiguous().view(-1).view(torch.int16), unscale.contiguous()


def flow_stem(img0, img1, wpack, w_unscale, bias=None, pad=(0, 0, 0, 0), range_word=None):
    """leaky_relu(conv7x7_s2_p3(pair) + bias, 0.1) in one launch of csrc/flow_stem.hip -> channels-last fp32 [N, 64, Hc, Wc], where
    ``pair`` = cat(halve(zero_pad(img0)), halve(zero_pad(img1))) is never built: ``img0, img1`` [N, 3, H, W] are read in place (every
    frame a dense [3, H, W] block at any batch stride, e.g. ``clip[:, t]`` of a [N, T, 3, H, W] clip; other layouts are copied),
    ``pad`` = (lw, uw, lh, uh) as ``helpers.pad_amounts`` returns it (the padded size must be even), the halving is
    F.interpolate(scale_factor=0.5, 'bilinear') = a 2x2 mean.  ``wpack, w_unscale`` come from ``flow_stem_pack``; ``range_word``: as
    for ``stem_split``, counted per element of the pair.  The first call on a device must not come from a capturing stream.  No
    fall-back: anything else is a RuntimeError."""
    for t, n in ((img0, 'img0'), (img1, 'img1')):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError('%s must be a CUDA float32 tensor' % n)
    if img0.dim() != 4 or img0.shape[1] != 3 or img1.shape != img0.shape:
        raise RuntimeError('img0 and img1 must be [N, 3, H, W] of one shape')
    N, _, H, W = img0.shape

    def frames(t):       # dense [3, H, W] frames at a batch stride the kernel can step over, else a contiguous copy
        ok = tuple(t.stride()[1:]) == (H * W, W, 1) and (N == 1 or t.stride(0) >= 3 * H * W)
        return t if ok else t.contiguous()
    img0, img1 = frames(img0), frames(img1)
    bs0, bs1 = (max(int(t.stride(0)), 3 * H * W) if N > 1 else 3 * H * W for t in (img0, img1))
    lw, uw, lh, uh = (int(p) for p in pad)
    if min(lw, uw, lh, uh) < 0:
        raise RuntimeError('flow_stem: negative pad %s' % (pad,))
    hpad, wpad = H + lh + uh, W + lw + uw
    _check(wpack, 'wpack', torch.int16)
    if wpack.numel() != FLOW_STEM_KP * STEM_COUT * 2:
        raise RuntimeError('wpack has %d elements, a flow stem pack has %d' % (wpack.numel(), FLOW_STEM_KP * STEM_COUT * 2))
    _check(w_unscale, 'w_unscale')
    if w_unscale.numel() != STEM_COUT:
        raise RuntimeError('w_unscale must have 64 elements')
    if bias is not None:
        _check(bias, 'bias')
        if bias.numel() != STEM_COUT:
            raise RuntimeError('bias must have 64 elements')
    if range_word is not None:
        _check(range_word, 'range_word', torch.int32)
    for t in (img1, wpack, w_unscale, bias, range_word):
        if t is not None and t.device != img0.device:
            raise RuntimeError('flow_stem: every tensor must be on %s' % img0.device)
    hh, wh = hpad // 2, wpad // 2
    out = torch.empty((N, STEM_COUT, (hh - 1) // 2 + 1, (wh - 1) // 2 + 1), dtype=img0.dtype, device=img0.device,
                      memory_format=torch.channels_last)
    lib = _lib.load()
    with torch.cuda.device(img0.device):
        rc = lib.rmnet_flow_stem_f32(_ptr(img0), _ptr(img1), bs0, bs1, _ptr(wpack), _ptr(w_unscale), _ptr(bias), N, H, W, hpad, wpad, lh, lw,
                                     _ptr(out), _ptr(range_word), _stream(img0.device))
    _lib.check(rc, 'rmnet_flow_stem_f32')
    return out


def pred_head(x, weight, bias):
    """conv3x3_p1(relu(x), weight) + bias for a channels-last fp32 ``x`` [n, C, Hq, Wq] (C % 32 == 0) and ``weight`` [2, C, 3, 3],
    ``bias`` [2] -> NCHW-contiguous [n, 2, Hq, Wq], plain fp32 FMA (csrc/pred_head.hip): the decoder's prediction head with its
    ReLU and the layout change inside.  No fall-back: anything else is a RuntimeError.

    Differentiable in ``x``, ``weight`` and ``bias``: when grad mode is on and ``x`` or ``weight`` requires grad, the call is recorded
    as one ``torch.autograd.Function`` that saves x and the weight; the forward is the same launch, the backward is
    ``pred_head_backward`` for what ``needs_input_grad`` asks for.  No double backward.  Every other call -- the inference path's,
    which passes a detached copy of the weight next to the module's bias, among them -- takes the plain path and has no graph."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, weight)):
        for t, name in ((x, 'x'), (weight, 'weight'), (bias, 'bias')):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError('%s must be a torch.Tensor' % name)
        return _PredHeadFn.apply(x, weight, bias)
    _check_act(x, 'x')
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError('x must be a channels-last [n, C, Hq, Wq] tensor')
    n, C, H, W = x.shape
    if C % 32:
        raise RuntimeError('pred_head needs C %% 32 == 0, got %d' % C)
    _check(weight, 'weight')
    _check(bias, 'bias')
    if tuple(weight.shape) != (2, C, 3, 3) or bias.numel() != 2:
        raise RuntimeError('pred_head needs weight [2, %d, 3, 3] and bias [2], got %s / %s' % (C, tuple(weight.shape), tuple(bias.shape)))
    if weight.device != x.device or bias.device != x.device:
        raise RuntimeError('pred_head: every tensor must be on %s' % x.device)
    out = torch.empty((n, 2, H, W), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        rc = lib.rmnet_pred_head_f32(_ptr(x), _ptr(weight), _ptr(bias), n, H, W, C, _ptr(out), _stream(x.device))
    _lib.check(rc, 'rmnet_pred_head_f32')
    return out


def affine_relu_maxpool(x, scale=None, shift=None):
    """max_pool2d(relu(x * scale[c] + shift[c]), 3, stride=2, padding=1) in one pass (csrc/epilogue.hip):
    the ResNet stem's bn1 -> relu -> maxpool without the full-resolution intermediate."""
    _check_act(x, 'x')
    if x.dim() != 4:
        raise RuntimeError('x must be [N,C,H,W]')
    N, C, H, W = x.shape
    cl = _is_cl(x) and C % 4 == 0
    if _is_cl(x) and not cl:
        x = x.contiguous()
    for t, n in ((scale, 'scale'), (shift, 'shift')):
        if t is not None:
            _check(t, n)
            if t.numel() != C:
                raise RuntimeError('%s must have C = %d elements' % (n, C))
    out = torch.empty(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, dtype=x.dtype, device=x.device,
                      memory_format=torch.channels_last if cl else torch.contiguous_format)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        if cl:
            rc = lib.rmnet_affine_relu_maxpool_nhwc_f32(_ptr(x), _ptr(scale), _ptr(shift), N, C, H, W, _ptr(out), _stream(x.device))
            _lib.check(rc, 'rmnet_affine_relu_maxpool_nhwc_f32')
            return out
        rc = lib.rmnet_affine_relu_maxpool_f32(_ptr(x), _ptr(scale), _ptr(shift), N, C, H, W, _ptr(out),
                                               _stream(x.device))
    _lib.check(rc, 'rmnet_affine_relu_maxpool_f32')
    return out


def flow_affine(flow, m1, m2):
    """Device-resident variant: flow [H,W,2] f32 cuda, m1/m2 [2,3] f32 cuda -> [H,W,2]."""
    for t, n in ((flow, 'flow'), (m1, 'm1'), (m2, 'm2')):
        _check(t, n)
    if flow.dim() != 3 or flow.shape[2] != 2 or m1.numel() != 6 or m2.numel() != 6:
        raise RuntimeError('expected flow [H,W,2] and 2x3 matrices')
    lib = _lib.load()
    out = torch.empty_like(flow)
    with torch.cuda.device(flow.device):
        rc = lib.rmnet_flow_affine_f32(_ptr(flow), _ptr(m1), _ptr(m2), flow.shape[0], flow.shape[1],
                                       _ptr(out), _stream(flow.device))
    _lib.check(rc, 'rmnet_flow_affine_f32')
    return out


def update_optical_flow(optical_flow, tr_matrix1, tr_matrix2, device=None):
    """NumPy calling convention of the reference's CPython module
    (flow_affine_transformation.cpp:87-90): ndarray in, new ndarray out -- computed on the GPU.
    Unlike the reference (which reinterprets whatever buffer it is given, .cpp:50-52) the inputs
    are checked/converted to C-contiguous float32."""
    flow = np.ascontiguousarray(optical_flow, dtype=np.float32)
    m1 = np.ascontiguousarray(tr_matrix1, dtype=np.float32)
    m2 = np.ascontiguousarray(tr_matrix2, dtype=np.float32)
    if flow.ndim != 3 or flow.shape[2] != 2 or m1.size != 6 or m2.size != 6:
        raise RuntimeError('expected flow [H,W,2] and 2x3 matrices')
    lib = _lib.load()
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    H, W = flow.shape[:2]
    out = np.empty_like(flow)
    with torch.cuda.device(dev):
        ws = _ws(lib.rmnet_flow_affine_workspace_bytes(H, W), dev)
        rc = lib.rmnet_flow_affine_f32_host(flow.ctypes.data, m1.ctypes.data, m2.ctypes.data, H, W,
                                            out.ctypes.data, _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, 'rmnet_flow_affine_f32_host')
    return out


def boundary_match(pred, gt, n_objects, radius):
    """pred, gt: uint8 [N,H,W] label maps on the GPU (0 = background) -> int32 [N, n_objects, 4], per frame and object
    k = 1 .. n_objects the counts (n_fg, n_gt, fg_match, gt_match) behind the boundary measure F of utils/metrics.py:119-169:
    the sizes of the two boundary maps and of each one's part inside the other's dilation by disk(radius) (csrc/boundary_f.hip,
    include/rmnet_hip.h E1).  Exact integers; 1 <= n_objects <= 64, 0 <= radius <= 40."""
    _check(pred, 'pred', dtype=torch.uint8)
    _check(gt, 'gt', dtype=torch.uint8)
    if pred.shape != gt.shape or pred.dim() != 3:
        raise RuntimeError('expected two [N, H, W] label maps of the same shape')
    if gt.device != pred.device:
        raise RuntimeError('pred and gt must be on the same device')
    lib = _lib.load()
    N, H, W = pred.shape
    K, dev = int(n_objects), pred.device
    with torch.cuda.device(dev):
        counts = torch.empty(N, max(K, 0), 4, dtype=torch.int32, device=dev)
        ws = _ws(lib.rmnet_boundary_match_workspace_bytes(N, K, H, W), dev)
        rc = lib.rmnet_boundary_match_u8(_ptr(pred), _ptr(gt), N, K, H, W, int(radius), _ptr(counts), _ptr(ws), ws.numel(),
                                         _stream(dev))
    _lib.check(rc, 'rmnet_boundary_match_u8')
    return counts


def clip_loss(probs, labels, ignore_index=255, bins=1 << 20, want_hist=False):
    """probs float32 [N,K,H,W] and labels uint8 [N,H,W] on the GPU -> the pieces of the validation loss of core/test.py:97
    (csrc/val_loss.hip, include/rmnet_hip.h I1), as device tensors and without a sync:
      'per_class' float64 [K,3]: G (the class's foreground count), lo, hi -- the class's Lovasz extension lies in [lo, hi] and
                  hi - lo <= 1 / bins; all 0 for a class that no counted pixel has
      'nll_sum'   float64 0-d: the sum of -logf(p_label) over the counted pixels
      'counts'    int64 [3]: counted pixels, pixels left out for a label >= K, pixels left out for a probability outside [0, 1]
      'hist'      with want_hist, int32 [K,2,bins+1]: the integer histograms of the keys (a view of the call's workspace).
    ``bins`` is a power of two from 2 to 2^22; an ``ignore_index`` outside 0 .. 255 ignores nothing."""
    _check(probs, 'probs')
    _check(labels, 'labels', dtype=torch.uint8)
    if probs.dim() != 4 or labels.dim() != 3 or (probs.shape[0],) + tuple(probs.shape[2:]) != tuple(labels.shape):
        raise RuntimeError('expected probs [N, K, H, W] and labels [N, H, W]')
    if labels.device != probs.device:
        raise RuntimeError('probs and labels must be on the same device')
    lib = _lib.load()
    N, K, H, W = probs.shape
    bins, dev = int(bins), probs.device
    with torch.cuda.device(dev):
        per_class = torch.empty(max(K, 1), 3, dtype=torch.float64, device=dev)
        nll_sum = torch.empty((), dtype=torch.float64, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        ws = _ws(lib.rmnet_clip_loss_workspace_bytes(K, bins), dev)
        rc = lib.rmnet_clip_loss_f32(_ptr(probs), _ptr(labels), N, K, H, W, int(ignore_index), bins, _ptr(per_class), _ptr(nll_sum),
                                     _ptr(counts), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, 'rmnet_clip_loss_f32')
    out = {'per_class': per_class, 'nll_sum': nll_sum, 'counts': counts}
    if want_hist:
        out['hist'] = ws[:K * 2 * (bins + 1) * 4].view(torch.int32).view(K, 2, bins + 1)
    return out


def clip_loss_grad(probs, labels, ignore_index=255, bins=1 << 20, want_tables=False):
    """``clip_loss`` and the gradient of the training loss lovasz + nll of core/train.py:180 with respect to ``probs``, from one
    histogram pass (csrc/val_loss_bwd.hip, include/rmnet_hip.h I2), as device tensors and without a sync: 'per_class', 'nll_sum' and
    'counts' with the bits ``clip_loss`` gives them, and
      'grad'      float32 [N,K,H,W]: s * g_kind[c][key] / n_present, plus -1 / (p_label * n_good) on the label's channel; 0 in every
                  channel of an ignored or bad pixel.  Every element is written: nothing is pre-zeroed.
      'tables'    with want_tables, float32 [K,2,bins+1]: g_bg (index 0) and g_fg (index 1) per class and bin (a view of the call's
                  workspace)."""
    _check(probs, 'probs')
    _check(labels, 'labels', dtype=torch.uint8)
    if probs.dim() != 4 or labels.dim() != 3 or (probs.shape[0],) + tuple(probs.shape[2:]) != tuple(labels.shape):
        raise RuntimeError('expected probs [N, K, H, W] and labels [N, H, W]')
    if labels.device != probs.device:
        raise RuntimeError('probs and labels must be on the same device')
    lib = _lib.load()
    N, K, H, W = probs.shape
    bins, dev = int(bins), probs.device
    with torch.cuda.device(dev):
        grad = torch.empty(N, K, H, W, dtype=torch.float32, device=dev)
        per_class = torch.empty(max(K, 1), 3, dtype=torch.float64, device=dev)
        nll_sum = torch.empty((), dtype=torch.float64, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        ws = _ws(lib.rmnet_clip_loss_grad_workspace_bytes(K, bins), dev)
        rc = lib.rmnet_clip_loss_grad_f32(_ptr(probs), _ptr(labels), N, K, H, W, int(ignore_index), bins, _ptr(grad), _ptr(per_class),
                                          _ptr(nll_sum), _ptr(counts), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, 'rmnet_clip_loss_grad_f32')
    out = {'per_class': per_class, 'nll_sum': nll_sum, 'counts': counts, 'grad': grad}
    if want_tables:
        out['tables'] = ws[:K * 2 * (bins + 1) * 4].view(torch.float32).view(K, 2, bins + 1)
    return out


# ------------------------------------------------------------------------------------------------ clip I/O (csrc/clip_io.hip)
def _three_doubles(v, name):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise RuntimeError('%s must hold three numbers' % name)
    return (ctypes.c_double * 3)(*v)


def frames_normalize(frames, mean, std):
    """frames uint8 [N,H,W,3] on the GPU -> float32 [N,3,H,W]: fl32(u / 255.f), then fl32((double(x) - mean[c]) / std[c]), the bits
    of img_normalize + astype(float32) (utils/helpers.py:133-135, utils/data_transforms.py:93; include/rmnet_hip.h F1)."""
    _check(frames, 'frames', dtype=torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise RuntimeError('frames must be [N, H, W, 3]')
    lib = _lib.load()
    N, H, W, _ = frames.shape
    dev = frames.device
    with torch.cuda.device(dev):
        out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
        rc = lib.rmnet_frames_normalize_u8(_ptr(frames), N, H, W, _three_doubles(mean, 'mean'), _three_doubles(std, 'std'), _ptr(out),
                                           _stream(dev))
    _lib.check(rc, 'rmnet_frames_normalize_u8')
    return out


def labels_onehot(labels, K, lut=None):
    """labels uint8 [N,H,W] on the GPU -> uint8 [N,K,H,W], plane k = (lut[label] == k); ``lut`` is a uint8 [256] device table or None
    for the identity.  A remapped label >= K sets no plane (utils/helpers.py:81-90).  1 <= K <= 255."""
    _check(labels, 'labels', dtype=torch.uint8)
    if labels.dim() != 3:
        raise RuntimeError('labels must be [N, H, W]')
    if lut is not None:
        _check(lut, 'lut', dtype=torch.uint8)
        if lut.numel() != 256 or lut.device != labels.device:
            raise RuntimeError('lut must hold 256 entries on the device of labels')
    lib = _lib.load()
    N, H, W = labels.shape
    K, dev = int(K), labels.device
    with torch.cuda.device(dev):
        out = torch.empty(N, max(K, 0), H, W, dtype=torch.uint8, device=dev)
        rc = lib.rmnet_labels_onehot_u8(_ptr(labels), _ptr(lut), N, K, H, W, _ptr(out), _stream(dev))
    _lib.check(rc, 'rmnet_labels_onehot_u8')
    return out


def argmax_labels(prob):
    """prob float32 [N,K,H,W] on the GPU -> uint8 [N,H,W], the first index of the maximum over K (torch.argmax's rule on ties) in
    one pass.  1 <= K <= 255; NaN inputs are out of scope."""
    _check(prob, 'prob')
    if prob.dim() != 4:
        raise RuntimeError('prob must be [N, K, H, W]')
    lib = _lib.load()
    N, K, H, W = prob.shape
    dev = prob.device
    with torch.cuda.device(dev):
        out = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
        rc = lib.rmnet_argmax_labels_f32(_ptr(prob), N, K, H, W, _ptr(out), _stream(dev))
    _lib.check(rc, 'rmnet_argmax_labels_f32')
    return out


def overlay(frames, labels, mean, std, ignore_idx=255, alpha=0.4):
    """frames float32 [N,3,H,W] (normalised), labels uint8 [N,H,W], both on the GPU -> uint8 [N,H,W,3]: get_segmentation of every
    frame (utils/helpers.py:165-176) bit for bit -- denormalise, blend every object but the frame's lowest label with the palette,
    blacken the 4-neighbour contours, in ascending object order (include/rmnet_hip.h F1)."""
    _check(frames, 'frames')
    _check(labels, 'labels', dtype=torch.uint8)
    if frames.dim() != 4 or frames.shape[1] != 3 or labels.dim() != 3 or labels.shape != frames.shape[:1] + frames.shape[2:]:
        raise RuntimeError('expected frames [N, 3, H, W] and labels [N, H, W]')
    if labels.device != frames.device:
        raise RuntimeError('frames and labels must be on the same device')
    lib = _lib.load()
    N, _, H, W = frames.shape
    dev = frames.device
    with torch.cuda.device(dev):
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        rc = lib.rmnet_overlay_u8(_ptr(frames), _ptr(labels), N, H, W, _three_doubles(mean, 'mean'), _three_doubles(std, 'std'),
                                  float(alpha), int(ignore_idx), _ptr(out), _ptr(ws), ws.numel() * 4, _stream(dev))
    _lib.check(rc, 'rmnet_overlay_u8')
    return out


# ------------------------------------------------------------------------------------------------ multi-scale inference (csrc/tta.hip)
TTA_MAX_ENTRIES = 8            # RMNET_TTA_MAX_ENTRIES


def resize_bilinear(x, out_h, out_w, scale_h, scale_w, flip=False, out=None):
    """x float32 [..., Hs, Ws] on the GPU -> float32 [..., out_h, out_w]: torch's bilinear formula with align_corners=False in plain
    fp32, every product and sum rounded on its own (include/rmnet_hip.h H1).  ``scale_h``, ``scale_w`` are the source steps per
    output pixel, rounded to float32 here; F.interpolate(scale_factor=fs) uses float(1.0 / fs).  ``flip`` writes every row
    mirrored.  ``out``: a contiguous float32 tensor of the result's shape to write into (a slice of a batch, say)."""
    _check(x, 'x')
    if x.dim() < 2:
        raise RuntimeError('x must be [..., H, W]')
    lib = _lib.load()
    Hs, Ws = x.shape[-2:]
    P = x.numel() // max(Hs * Ws, 1)
    dev = x.device
    shape = tuple(x.shape[:-2]) + (int(out_h), int(out_w))
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        else:
            _check(out, 'out')
            if tuple(out.shape) != shape or out.device != dev:
                raise RuntimeError('out must be %s on the device of x' % (shape,))
        rc = lib.rmnet_resize_bilinear_f32(_ptr(x), P, Hs, Ws, int(out_h), int(out_w), float(scale_h), float(scale_w), int(bool(flip)),
                                           _ptr(out), _stream(dev))
    _lib.check(rc, 'rmnet_resize_bilinear_f32')
    return out


def tta_merge(sources, flipped, H, W, want_labels=True, mean=None, labels=None):
    """sources: 1 .. 8 float32 [N,K,hs_e,ws_e] GPU tensors, flipped: one flag each -> (mean float32 [N,K,H,W], labels uint8 [N,H,W] or
    None) in one launch: every source resized to (H, W) (F.interpolate(size=), a flipped source read mirrored), summed in entry order,
    divided by the number of entries; the labels are the first index of the maximum of the means (include/rmnet_hip.h H1).  ``mean``
    and ``labels`` may be given as contiguous buffers to write into; without ``want_labels`` a given label buffer is left alone."""
    sources, flipped = list(sources), [int(bool(f)) for f in flipped]
    E = len(sources)
    if not 1 <= E <= TTA_MAX_ENTRIES or len(flipped) != E:
        raise RuntimeError('expected 1 .. %d sources and one flag for each' % TTA_MAX_ENTRIES)
    for s in sources:
        _check(s, 'source')
        if s.dim() != 4 or s.shape[:2] != sources[0].shape[:2] or s.device != sources[0].device:
            raise RuntimeError('the sources must be [N, K, h, w] with the same N and K on one device')
    lib = _lib.load()
    N, K = sources[0].shape[:2]
    H, W, dev = int(H), int(W), sources[0].device
    with torch.cuda.device(dev):
        if mean is None:
            mean = torch.empty(N, K, H, W, dtype=torch.float32, device=dev)
        else:
            _check(mean, 'mean')
            if tuple(mean.shape) != (N, K, H, W):
                raise RuntimeError('mean must be [N, K, H, W]')
        if want_labels:
            if labels is None:
                labels = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
            else:
                _check(labels, 'labels', dtype=torch.uint8)
                if tuple(labels.shape) != (N, H, W):
                    raise RuntimeError('labels must be [N, H, W]')
        ptrs = (ctypes.c_void_p * E)(*[s.data_ptr() for s in sources])
        hs = (ctypes.c_int * E)(*[s.shape[2] for s in sources])
        ws = (ctypes.c_int * E)(*[s.shape[3] for s in sources])
        fl = (ctypes.c_int * E)(*flipped)
        rc = lib.rmnet_tta_merge_f32(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(hs, ctypes.c_void_p), ctypes.cast(ws, ctypes.c_void_p),
                                     ctypes.cast(fl, ctypes.c_void_p), E, N, K, H, W, _ptr(mean), _ptr(labels) if want_labels else None,
                                     _stream(dev))
    _lib.check(rc, 'rmnet_tta_merge_f32')
    return mean, (labels if want_labels else None)


# ------------------------------------------------------------------------------------------------ late objects (csrc/late_objects.hip)
def label_presence_chunk_bytes():
    """Bytes of a frame's 16-byte-aligned body that one workgroup of the presence kernel reads (host arithmetic)."""
    return int(_lib.load().rmnet_label_presence_chunk_bytes())


def label_presence(labels):
    """labels uint8 [N,H,W] on the GPU, contiguous, at any byte offset -> int32 [N,8]: the 256-bit set of the byte values of every
    frame, bit ``v & 31`` of word ``v >> 5`` (the C entry's uint32 words, carried as int32: the same bits).  One memset node and
    one launch on the current stream, no host synchronisation (include/rmnet_hip.h I1)."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise RuntimeError('labels must be a [N, H, W] tensor')
    _check(labels, 'labels', dtype=torch.uint8)
    lib = _lib.load()
    N, H, W = labels.shape
    dev = labels.device
    with torch.cuda.device(dev):
        out = torch.empty(max(N, 0), 8, dtype=torch.int32, device=dev)
        rc = lib.rmnet_label_presence_u8(_ptr(labels), N, H, W, _ptr(out), _stream(dev))
    _lib.check(rc, 'rmnet_label_presence_u8')
    return out


def _batch_slices(t, name, inner, dtype):
    """``t`` must be [B, *inner] of ``dtype`` on the GPU with every batch slice contiguous; returns its batch stride in elements."""
    if not isinstance(t, torch.Tensor) or t.dim() != len(inner) + 1 or tuple(t.shape[1:]) != tuple(inner):
        raise RuntimeError('%s must be [B, %s]' % (name, ', '.join(str(i) for i in inner)))
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if not t.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor' % name)
    if not t[0].is_contiguous():
        raise RuntimeError('every batch slice of %s must be contiguous' % name)
    return int(t.stride(0)) if t.shape[0] > 1 else int(t[0].numel())


def label_presence_nearest_rows():
    """Output rows of one scale that one workgroup of the nearest-resized presence kernel takes (host arithmetic)."""
    return int(_lib.load().rmnet_label_presence_nearest_rows())


def label_presence_nearest(labels, sizes, scales):
    """labels uint8 [N,Hs,Ws] on the GPU, contiguous, at any byte offset; ``sizes``: 1 .. 8 pairs (hd, wd), ``scales``: as many
    pairs (scale_h, scale_w) of source steps per output pixel -> int32 [S,N,8]: row (s, n) is the 256-bit set of the values among
    labels[n][src(y)][src(x)], y < hd, x < wd, with src(d) = min(int(floorf(float(d) * scale)), in - 1): the ids the nearest-resized
    label map of every scale would hold, without the map.  One memset node and one launch for all scales on the current stream, no
    host synchronisation (include/rmnet_hip.h I2)."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise RuntimeError('labels must be a [N, H, W] tensor')
    _check(labels, 'labels', dtype=torch.uint8)
    sizes, scales = [(int(h), int(w)) for h, w in sizes], [(float(a), float(b)) for a, b in scales]
    S = len(sizes)
    if not 1 <= S <= TTA_MAX_ENTRIES or len(scales) != S:
        raise RuntimeError('expected 1 .. %d sizes and one pair of scales for each' % TTA_MAX_ENTRIES)
    lib = _lib.load()
    N, Hs, Ws = labels.shape
    dev = labels.device
    hd, wd = (ctypes.c_int * S)(*[h for h, _ in sizes]), (ctypes.c_int * S)(*[w for _, w in sizes])
    sh, sw = (ctypes.c_float * S)(*[a for a, _ in scales]), (ctypes.c_float * S)(*[b for _, b in scales])
    with torch.cuda.device(dev):
        out = torch.empty(S, max(N, 0), 8, dtype=torch.int32, device=dev)
        rc = lib.rmnet_label_presence_nearest_u8(_ptr(labels), N, Hs, Ws, ctypes.cast(hd, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p),
                                                 ctypes.cast(sh, ctypes.c_void_p), ctypes.cast(sw, ctypes.c_void_p), S, _ptr(out), _stream(dev))
    _lib.check(rc, 'rmnet_label_presence_nearest_u8')
    return out


def object_edit_softmax(logit, labels, lut, action, prob, sampling=None):
    """One frame of models/rmnet.py:436-450 in one launch: ``logit`` float32 [B,K,H,W] is edited in place per ``action`` uint8 [B,K]
    (0 keep, 1 absent = -16.1181f, 2 inject fl(fl(m * 32.0605f) - 16.1181f) with m = (lut[b][label] == k)), then its soft-max
    over K is written to ``prob`` float32 [B,K,H,W].  ``labels`` uint8 [B,H,W] are frame t's raw label maps (None when no action
    is 2), ``lut`` uint8 [B,256] the clips' id tables.  logit, labels and prob may be batch-strided views whose slices are
    contiguous (``est[:, t]``, ``labels[:, t]``); lut and action are contiguous.  1 <= K <= 255.  Returns ``prob``.

    ``sampling = (scale_h, scale_w, flips)``: the frame is a resized clip's and ``labels`` are full-size maps uint8 [B,Hs,Ws] of any
    size; pixel (y, x) of slot b reads labels[b][src(y)][src(W - 1 - x if flips[b] else x)] with the nearest rule of
    ``label_presence_nearest`` (include/rmnet_hip.h I2).  ``flips``: one flag per slot, B <= 64."""
    if not isinstance(logit, torch.Tensor) or logit.dim() != 4:
        raise RuntimeError('logit must be [B, K, H, W]')
    B, K, H, W = logit.shape
    if not 1 <= K <= 255:
        raise RuntimeError('expected 1 <= K <= 255, got %d' % K)
    if not isinstance(prob, torch.Tensor) or tuple(prob.shape) != (B, K, H, W):
        raise RuntimeError('prob must be [B, K, H, W] like logit')
    logit_bs = _batch_slices(logit, 'logit', (K, H, W), torch.float32)
    prob_bs = _batch_slices(prob, 'prob', (K, H, W), torch.float32)
    Hs, Ws = H, W
    if sampling is not None:
        scale_h, scale_w, flips = float(sampling[0]), float(sampling[1]), [bool(f) for f in sampling[2]]
        if len(flips) != B or B > 64:
            raise RuntimeError('sampling needs one flip flag per batch slot and B <= 64')
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
                raise RuntimeError('labels must be [B, Hs, Ws]')
            Hs, Ws = labels.shape[1:]
    labels_bs = _batch_slices(labels, 'labels', (Hs, Ws), torch.uint8) if labels is not None else 0
    _check(lut, 'lut', dtype=torch.uint8)
    _check(action, 'action', dtype=torch.uint8)
    if tuple(lut.shape) != (B, 256) or tuple(action.shape) != (B, K) or prob.shape[0] != B or (labels is not None and labels.shape[0] != B):
        raise RuntimeError('expected lut [B, 256], action [B, K] and the same B everywhere')
    dev = logit.device
    if any(t is not None and t.device != dev for t in (labels, lut, action, prob)):
        raise RuntimeError('every tensor must be on the device of logit')
    lib = _lib.load()
    with torch.cuda.device(dev):
        if sampling is None:
            rc = lib.rmnet_object_edit_softmax_f32(_ptr(logit), logit_bs, _ptr(labels), labels_bs, _ptr(lut), _ptr(action), _ptr(prob), prob_bs,
                                                   B, K, H, W, _stream(dev))
            what = 'rmnet_object_edit_softmax_f32'
        else:
            bits = sum(1 << b for b, f in enumerate(flips) if f)
            rc = lib.rmnet_object_edit_softmax_nearest_f32(_ptr(logit), logit_bs, _ptr(labels), labels_bs, int(Hs), int(Ws), scale_h, scale_w, bits,
                                                           _ptr(lut), _ptr(action), _ptr(prob), prob_bs, B, K, H, W, _stream(dev))
            what = 'rmnet_object_edit_softmax_nearest_f32'
    _lib.check(rc, what)
    return prob
