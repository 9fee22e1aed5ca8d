"""Writes tests/golden/kstar_layout_parent.npz: the inputs of every case of tests/test_gpu_kstar_layout.py and what the
resident rollout kernels make of them.  Run ONCE, on the GPU, with the library of the commit BEFORE the row image of the
Kstar phase changed (sx_rollout_rw.hpp: rw_row_slot) -- the recorded outputs are what that change must reproduce bit for bit:

    SX_LIB=<libsxamd.so built from the parent commit> python tests/golden/make_kstar_layout_parent.py

Inputs and outputs only: training sets, hyper-parameters, the linear prior and cost constants, start states and actions;
trajectories, variances, costs and the status word per case.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_gpu_kstar_layout as t  # noqa: E402


def main():
    inputs = t.make_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'inputs.npz')
        np.savez(path, **inputs)
        outs = t.run_children(path, tmp)
    merged = dict(inputs)
    for form in outs:
        merged.update(outs[form])
    np.savez_compressed(t.GOLDEN, **merged)
    print('wrote', t.GOLDEN, os.path.getsize(t.GOLDEN), 'bytes,', len(merged), 'arrays')


if __name__ == '__main__':
    main()
