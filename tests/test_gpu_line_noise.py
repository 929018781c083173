"""The row-noise and the column-noise kernels are one rule (csrc/line_noise.h): rvdd_cols_estimate of a packed input is
rvdd_rows_estimate of its transpose -- the spatial axes swapped, and planes 1 and 2 -- under a clamp that never bites, bit for bit.
tests/test_line_ref_host.py asks the same of the two NumPy restatements."""
import numpy as np
import pytest
import torch

import cols_ref
from gpu_support import bits_of, ops_rt as _rt, upload as _up
from line_ref import NO_CLAMP, transposed

pytestmark = pytest.mark.gpu

# (n, hh, ww): the smallest both kernels accept -- every neighbour mirrored, every one reflected a second time; odd, two frames, a
# strip of 32 columns and a partial one, transposed 2 * 37 = 74 keys over 256 threads; exactly two strips, transposed 18 keys a row
SHAPES = [(1, 5, 5), (2, 37, 53), (1, 9, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_column_kernel_is_the_row_kernel_on_the_transpose(shape):
    from rvdd_release_amd.runtime import cols_cfg, rows_cfg
    rt = _rt()
    cases = cols_ref.cases(shape)
    assert len(cases) == 5
    used = 0
    for name, packed, bits, c in cases:
        gate = [float(v) for v in c]
        co, cs = rt.cols_estimate(_up(packed), cols_cfg(*gate), bits)
        ro, rs, _ = rt.rows_estimate(_up(transposed(packed)), rows_cfg(*gate, NO_CLAMP), bits)
        torch.cuda.synchronize()
        assert tuple(co.shape) == tuple(ro.shape) == (shape[0], 2, shape[2]), name
        assert np.array_equal(bits_of(co), bits_of(ro)), (name, "offsets", np.argwhere(bits_of(co) != bits_of(ro))[:4].tolist())
        assert np.array_equal(cs.cpu().numpy(), rs.cpu().numpy()), (name, "state")      # 1 = applied, 0 = skipped; 2 (clamped) never
        used += int(cs.sum())
    assert used > 0
