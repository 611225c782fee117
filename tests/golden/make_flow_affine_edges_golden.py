# -*- coding: utf-8 -*-
"""Generate tests/golden/flow_affine_edges.npz by running the REFERENCE's own compiled flow op on the cases of
tests/region_ref.py (exact halves, their fp32 neighbours, dyadic and inexact matrices, the clamp equalities, NaN / Inf, the shapes
1 x 1, 2 x 257 and 4099 x 3).

Like make_golden.py this runs only where the reference is checked out: oracle/Makefile compiles its C++ where it lies into
oracle/_ref/flow_affine_transformation.so, this script imports that module, feeds it the cases and stores inputs and outputs as
data.  The 4099-row case is stored as its seed and the sha256 of the output (region_ref.digest).  No test runs this script.

    make -C oracle && python tests/golden/make_flow_affine_edges_golden.py
"""

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import region_ref as R  # noqa: E402


def _reference():
    so = os.path.join(ROOT, 'oracle', '_ref', 'flow_affine_transformation.so')
    spec = importlib.util.spec_from_file_location('flow_affine_transformation', so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = _reference()
    run = lambda f, a, b: ref.update_optical_flow(np.ascontiguousarray(f, np.float32), np.ascontiguousarray(a, np.float32),
                                                  np.ascontiguousarray(b, np.float32))
    cases = R.flow_cases()
    data = {'names': np.array(list(cases))}
    for i, (name, (flow, m1, m2)) in enumerate(cases.items()):
        out = run(flow, m1, m2)
        assert out.dtype == np.float32 and out.shape == flow.shape
        for key, value in (('flow', flow), ('m1', m1), ('m2', m2), ('out', out)):
            data['case%02d.%s' % (i, key)] = np.ascontiguousarray(value, np.float32)
    name, H, W, seed = R.FLOW_TALL
    out = run(*R.flow_tall_case())
    data['tall.name'], data['tall.seed'], data['tall.shape'] = np.array(name), np.int64(seed), np.array([H, W], np.int64)
    data['tall.digest'] = np.array(R.digest(out))
    data['tall.first_rows'] = out[:2].copy()            # (a readable sample next to the digest)
    data['tall.last_rows'] = out[-3:].copy()
    path = os.path.join(HERE, 'flow_affine_edges.npz')
    np.savez_compressed(path, **data)
    print('%s: %d arrays, %d bytes' % (path, len(data), os.path.getsize(path)))


if __name__ == '__main__':
    main()
