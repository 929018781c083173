"""The row-noise and the column-noise restatements are one rule (tests/line_ref.py): the column estimate of a packed input is the row
estimate of its transpose -- the spatial axes swapped, and planes 1 and 2, which turns the pairs (j, j + 2) into (2j, 2j + 1) -- under
a clamp that never bites.  tests/test_gpu_line_noise.py asks the same of the two kernels."""
import numpy as np
import pytest

import cols_ref
import rows_ref
from line_ref import NO_CLAMP, transposed


@pytest.mark.parametrize("shape", [(1, 5, 5), (1, 8, 9), (2, 37, 53)], ids=lambda s: "%dx%dx%d" % s)
def test_the_column_estimate_is_the_row_estimate_of_the_transpose(shape):
    cases = cols_ref.cases(shape)
    assert len(cases) == 5
    for name, packed, bits, c in cases:
        cols = cols_ref.estimate(packed, bits, c)
        rows = rows_ref.estimate(transposed(packed), bits, rows_ref.cfg(*c, max_dn=NO_CLAMP))
        assert cols["offsets"].shape == rows["offsets"].shape == (shape[0], 2, shape[2]), name
        assert np.array_equal(cols["offsets"], rows["offsets"]), (name, "offsets")
        assert np.array_equal(cols["state"], rows["state"]), (name, "state")      # 1 = applied, 0 = skipped: cnt >= hh either way
        assert np.array_equal(cols["cnt"], rows["cnt"]), (name, "cnt")
        assert int(rows["acc"]["clamped"].sum()) == 0, name
