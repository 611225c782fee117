# -*- coding: utf-8 -*-
"""ctypes binding of librmnet_hip.so (the C ABI of include/rmnet_hip.h).

There is deliberately no fallback: if the library is missing or a call returns a non-zero code
the caller gets a RuntimeError.  Nothing here (or anywhere under rmnet_amd/) imports oracle/.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RMNET_HIP_LIB') or os.path.join(_HERE, 'librmnet_hip.so')   # override: experiments only

c_f32p = ctypes.c_void_p   # device pointers travel as integers
c_i32p = ctypes.c_void_p
c_f64p = ctypes.POINTER(ctypes.c_double)   # host arrays (mean / std of the clip I/O entries)
c_hostp = ctypes.c_void_p                  # host arrays of any element type (the per-entry tables of rmnet_tta_merge_f32)

# name -> (restype, argtypes); must list every symbol declared in include/rmnet_hip.h
SIGNATURES = {
    'rmnet_abi_version': (ctypes.c_int, []),
    'rmnet_error_string': (ctypes.c_char_p, [ctypes.c_int]),
    'rmnet_region_map_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_region_map_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
        ctypes.c_int, c_f32p, c_i32p, c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_region_map_warped_f32': (ctypes.c_int, [
        c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int,
        ctypes.c_int, c_f32p, c_i32p, c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_boxes_to_cell_rects_i32': (ctypes.c_int, [
        c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, c_i32p, ctypes.c_void_p]),
    'rmnet_memory_read_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 7),
    'rmnet_memory_read_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
        ctypes.c_longlong, c_f32p, c_f32p, c_i32p, c_i32p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_memory_read_backward_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 6),
    'rmnet_memory_read_backward_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
        ctypes.c_longlong, c_f32p, c_f32p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_memory_read_f32_ev': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
        ctypes.c_longlong, c_f32p, c_f32p, c_i32p, c_i32p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_bank_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_bank_overflow_offset': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_bank_area_offset': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_bank_append_f32': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p,
        c_f32p, c_i32p, ctypes.c_void_p]),
    'rmnet_bank_append_f32_at': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i32p, c_f32p,
        c_f32p, c_i32p, ctypes.c_void_p]),
    'rmnet_bank_read_f32_at': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i32p, ctypes.c_int, c_f32p,
        c_f32p, c_i32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_bank_read_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 3),
    'rmnet_bank_read_workspace_bytes_for': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_bank_read_f32': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p,
        c_f32p, c_i32p, c_f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_rect_mask_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i32p, c_f32p,
        ctypes.c_void_p]),
    'rmnet_channel_affine_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
        ctypes.c_longlong, c_f32p, ctypes.c_void_p]),
    'rmnet_upsample2x_add_f32': (ctypes.c_int, [
        c_f32p, c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_soft_aggregate_f32': (ctypes.c_int, [
        c_f32p, c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, ctypes.c_void_p]),
    'rmnet_soft_aggregate_bwd_f32': (ctypes.c_int, [
        c_f32p, c_i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        c_f32p, ctypes.c_longlong, c_f32p, ctypes.c_longlong, c_f32p, ctypes.c_longlong, ctypes.c_void_p, c_f32p, ctypes.c_void_p]),
    'rmnet_affine_relu_maxpool_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p,
        ctypes.c_void_p]),
    'rmnet_channel_affine_nhwc_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_upsample2x_add_nhwc_f32': (ctypes.c_int, [
        c_f32p, c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_affine_relu_maxpool_nhwc_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_conv3x3_split_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        c_f32p, c_i32p, ctypes.c_void_p]),
    'rmnet_conv3x3_split_lds_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        c_f32p, c_i32p, ctypes.c_void_p]),
    'rmnet_conv3x3_rows_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        c_f32p, c_i32p, ctypes.c_void_p]),
    'rmnet_conv3x3_wgrad_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_conv3x3_wgrad_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, ctypes.c_void_p,
        ctypes.c_size_t, c_i32p, ctypes.c_void_p]),
    'rmnet_conv_grad_stage_f32': (ctypes.c_int, [c_f32p, c_f32p, c_f32p, ctypes.c_longlong, c_f32p, c_f32p, ctypes.c_void_p]),
    'rmnet_conv3x3_wgrad_n_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 5),
    'rmnet_conv3x3_wgrad_n_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p,
        ctypes.c_void_p, ctypes.c_size_t, c_i32p, ctypes.c_void_p]),
    'rmnet_conv_grad_stage_rect_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, c_i32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, c_f32p, c_f32p, ctypes.c_void_p]),
    'rmnet_conv_split_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, ctypes.c_int, c_i32p, ctypes.c_void_p]),
    'rmnet_conv_split_pre_f32': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_f32p, ctypes.c_int, c_i32p, ctypes.c_void_p]),
    'rmnet_conv_rows_pre_f32': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_f32p, ctypes.c_int, c_i32p, ctypes.c_void_p]),
    'rmnet_conv_split_region_f32': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i32p, c_f32p, c_f32p, ctypes.c_int, c_i32p, ctypes.c_void_p]),
    'rmnet_split_act_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_i32p, ctypes.c_void_p]),
    'rmnet_stem_split_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_i32p,
        ctypes.c_void_p]),
    'rmnet_flow_stem_f32': (ctypes.c_int, [
        c_f32p, c_f32p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_i32p, ctypes.c_void_p]),
    'rmnet_pred_head_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_flow_conv_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, ctypes.c_void_p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int, ctypes.c_int, c_i32p, ctypes.c_void_p]),
    'rmnet_flow_head_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_flow_head_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_flow_up_f32': (ctypes.c_int, [
        c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'rmnet_flow_affine_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_flow_affine_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'rmnet_flow_affine_f32_host': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_boundary_match_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_boundary_match_u8': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_i32p,
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_frames_normalize_u8': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f64p, c_f64p, c_f32p, ctypes.c_void_p]),
    'rmnet_labels_onehot_u8': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_argmax_labels_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_overlay_u8': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f64p, c_f64p, ctypes.c_double, ctypes.c_int,
        ctypes.c_void_p, c_i32p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_resize_bilinear_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
        c_f32p, ctypes.c_void_p]),
    'rmnet_tta_merge_f32': (ctypes.c_int, [
        c_hostp, c_hostp, c_hostp, c_hostp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p,
        ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_label_presence_chunk_bytes': (ctypes.c_int, []),
    'rmnet_label_presence_u8': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'rmnet_object_edit_softmax_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_longlong,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'rmnet_label_presence_nearest_rows': (ctypes.c_int, []),
    'rmnet_label_presence_nearest_u8': (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_hostp, c_hostp, c_hostp, c_hostp, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p]),
    'rmnet_object_edit_softmax_nearest_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
        ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p, c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_void_p]),
    'rmnet_clip_loss_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'rmnet_clip_loss_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_clip_loss_grad_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    'rmnet_clip_loss_grad_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'rmnet_upsample_bwd_f32': (ctypes.c_int, [
        c_f32p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, ctypes.c_void_p]),
    'rmnet_pred_head_bwd_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int] * 4),
    'rmnet_pred_head_bwd_f32': (ctypes.c_int, [
        c_f32p, c_f32p, c_f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_f32p, c_f32p, c_f32p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p]),
}

ABI_VERSION = 6
_lib = None


class RMNetHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once).  Raises RMNetHipError when it is not there -- build it with
    ``python -m rmnet_amd.build`` or ``__graft_entry__.build()``."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RMNetHipError(
            'librmnet_hip.so is missing (%s). The HIP kernels are the only implementation of this '
            'path; build them with `python -m rmnet_amd.build`.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.rmnet_abi_version() != ABI_VERSION:
        raise RMNetHipError('librmnet_hip.so ABI %d != expected %d' % (lib.rmnet_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().rmnet_error_string(code).decode()
        raise RMNetHipError('%s failed: %s (code %d)' % (what, msg, code))
