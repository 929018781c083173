"""Flows from the previous denoised frame in the stream, host side: the numpy restatement of rvdd_gray_of_rgb against the
re-mosaic's mean in float64, and the new symbol / option in the binding and the header.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from stream_den_ref import COLOURS, PATTERNS, gray_of_rgb_ref


@pytest.mark.parametrize("bit_depth", [10, 12, 14])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_restatement_is_the_mean_of_the_remosaic(pattern, bit_depth):
    """gray == top * ((remosaick(x) + 1) / 2).mean(channels) computed in float64, to a relative 1e-6: the restatement makes five
    f32 roundings per cell (v + 1 and the three sums; the products by 0.5 and 0.25 are exact, the one by top is the fifth), each
    at most 2^-24 relative, all on non-negative terms -- about 3e-7."""
    from rvdd_release_amd.runtime import BAYER_PATTERNS
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    assert PATTERNS == BAYER_PATTERNS
    rng = np.random.default_rng(7 * bit_depth + PATTERNS.index(pattern))
    x = rng.uniform(-1.0, 1.0, size=(3, 3, 36, 52)).astype(np.float32)
    x[0, :, :2, :2] = -1.0                                      # an all-black and an all-white cell
    x[0, :, :2, 2:4] = 1.0
    top = 2 ** bit_depth - 1
    got = gray_of_rgb_ref(x, pattern, bit_depth)
    planes = HamiltonAdam(pattern).remosaick(torch.from_numpy(x).double())            # [n,4,h,w]
    want = (top * ((planes + 1.0) / 2.0).mean(dim=1)).numpy()
    assert got.shape == want.shape == (3, 18, 26) and got.dtype == np.float32
    print(f"{pattern} {bit_depth}: max relative difference {np.max(np.abs(got - want) / np.maximum(want, 1e-300)):.3e}")
    assert np.all(np.abs(got.astype(np.float64) - want) <= 1e-6 * np.abs(want))
    assert got[0, 0, 0] == 0.0 and got[0, 0, 1] == np.float32(top)
    # the colour table of the restatement is the package's re-mosaic, position by position
    for k in range(4):
        assert np.array_equal(planes[:, k].numpy(), x[:, COLOURS[pattern][k], (k >> 1)::2, (k & 1)::2].astype(np.float64))


def test_restatement_on_a_demosaicked_integer_frame_is_ingests_gray():
    """Where the RGB frame holds, at every CFA site, the normalised value of a sensor frame, the plane is that frame's gray
    plane up to the roundings of the normalisation: the two images of a TV-L1 pair share a scale."""
    from stream_ref import ingest_ref
    rng = np.random.default_rng(3)
    cells = rng.integers(0, 4096, size=(1, 18, 26, 4)).astype(np.float32)
    packed, gray = ingest_ref(cells, "packed_hwc", 12)
    for pattern in PATTERNS:
        rgb = np.zeros((1, 3, 36, 52), np.float32)
        for k in range(4):
            rgb[:, COLOURS[pattern][k], (k >> 1)::2, (k & 1)::2] = packed[:, k]
        assert np.allclose(gray_of_rgb_ref(rgb, pattern, 12), gray, rtol=1e-6, atol=1e-3)


def test_symbol_and_option_are_declared():
    from rvdd_release_amd import _lib
    assert "rvdd_gray_of_rgb" in _lib.exported_symbols()
    txt = open(os.path.join(REPO, "include", "rvdd.h")).read()
    doc = txt[txt.index("Known names:"):txt.index("int rvdd_set_option(")]
    assert "stream_flow_from_denoised" in set(re.findall(r'^ \*   "([a-z0-9_]+)"', doc, flags=re.M))
    assert re.search(r"\bint\s+rvdd_gray_of_rgb\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_denoise_and_stream_bench_know_the_flag():
    from rvdd_release_amd import denoise
    assert "--val_flow_from_denoised" in denoise.__doc__
    opt = denoise._parse(["--val_flow_from_denoised"])
    assert opt.val_flow_from_denoised is True and denoise._parse([]).val_flow_from_denoised is False
    assert "--flow-from-denoised" in open(os.path.join(REPO, "tools", "stream_bench.py")).read()
