"""util/Hamilton_Adam_demo.py of the reference on the HIP runtime."""
from __future__ import annotations

import torch

from ._ops import dev_index, ops_runtime
from ..runtime import BAYER_PATTERNS


class HamiltonAdam:
    def __init__(self, pattern):
        if pattern not in BAYER_PATTERNS:
            raise NotImplementedError(f"rvdd HamiltonAdam: pattern {pattern!r} is not built; the patterns are "
                                      f"{', '.join(repr(p) for p in BAYER_PATTERNS)} (util/Hamilton_Adam_demo.py:175-224)")
        self.pattern = pattern

    def to(self, *a, **k):
        return self

    def __call__(self, x):
        return self.forward(x)

    def forward(self, x):
        """[B,4k,H,W] -> [B,3k,2H,2W] (util/Hamilton_Adam_demo.py:249-289), packed raw in this pattern."""
        return ops_runtime(dev_index(x)).demosaic(x.float(), pattern=self.pattern)

    def remosaick(self, x):
        """[B,3,H,W] RGB -> [B,4,H/2,W/2] packed planes of THIS pattern: channel k is CFA position (k >> 1, k & 1)
        of each 2x2 cell and takes the colour the pattern has there -- the inverse of the packing, so
        remosaick(HA(raw)) is raw.  Pure indexing, no arithmetic.

        This differs from the reference on purpose: its remosaick (util/Hamilton_Adam_demo.py:237-246) indexes
        GBRG whatever the pattern, which would scramble the colours of any other pattern on the --warp_raw and
        online-flow round trips.  For 'gbrg' the two are the same."""
        B, _, H, W = x.size()
        py, px = _PHASE[self.pattern]
        y = torch.zeros(B, 4, H // 2, W // 2, dtype=x.dtype, device=x.device)
        for k in range(4):
            r, c = k >> 1, k & 1
            y[:, k] = x[:, _GBRG_COLOUR[((r ^ py) << 1) | (c ^ px)], r::2, c::2]
        return y


# the colour site of full-resolution pixel (y, x) under a pattern is the GBRG site of (y ^ py, x ^ px)
_PHASE = {"gbrg": (0, 0), "grbg": (1, 1), "rggb": (1, 0), "bggr": (0, 1)}
# RGB channel of each GBRG site: G(e,e), B(e,o), R(o,e), G(o,o)
_GBRG_COLOUR = (1, 2, 0, 1)
