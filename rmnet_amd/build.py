# -*- coding: utf-8 -*-
"""Build librmnet_hip.so in-tree with hipcc for gfx950 (no JIT cache, no torch build machinery:
the boundary is a plain C ABI, see include/rmnet_hip.h)."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
SOURCES = ['capi.hip', 'region_map.hip', 'flow_affine.hip', 'memory_read.hip', 'bank.hip', 'epilogue.hip', 'conv3x3.hip', 'conv3x3_rows.hip', 'conv_split.hip',
           'conv_rows.hip', 'stem.hip', 'pred_head.hip', 'flow_conv.hip', 'flow_head.hip', 'flow_stem.hip', 'boundary_f.hip', 'clip_io.hip', 'tta.hip',
           'late_objects.hip', 'val_loss.hip', 'memory_read_bwd.hip', 'val_loss_bwd.hip', 'soft_aggregate_bwd.hip', 'conv3x3_wgrad.hip',
           'decoder_glue_bwd.hip', 'conv_wgrad_n.hip']
LIB = os.path.join(HERE, 'librmnet_hip.so')
ARCH = 'gfx950'


def hipcc_path():
    for cand in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found: librmnet_hip.so cannot be built')


def dependencies():
    """Every file whose edit must rebuild the library: the sources, every header of csrc/ and the C ABI's header."""
    headers = sorted(f for f in os.listdir(CSRC) if f.endswith('.h'))
    return [os.path.join(CSRC, f) for f in SOURCES + headers] + [os.path.join(os.path.dirname(HERE), 'include', 'rmnet_hip.h')]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in dependencies())


def build_library(force=False, verbose=False):
    """Compile every HIP source into one shared library.  Returns the library path."""
    if not force and not needs_build():
        return LIB
    cmd = [hipcc_path(), '--offload-arch=' + ARCH, '-O3', '-std=c++17', '-shared', '-fPIC',
           '-o', LIB] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB


if __name__ == '__main__':
    print(build_library(force=True, verbose=True))
