"""numpy restatement of rvdd_gray_of_rgb (include/rvdd.h), one f32 operation at a time.  Beside stream_ref.py; what rvdd_video_push
with option "stream_flow_from_denoised" must equal is stream_compose.compose(from_denoised=True)."""
import numpy as np

PATTERNS = ("gbrg", "grbg", "rggb", "bggr")          # enum rvdd_bayer, in order
# RGB plane at CFA position k = (k >> 1, k & 1) of a 2x2 cell, row by row: GBRG = G B / R G, and so on
COLOURS = {"gbrg": (1, 2, 0, 1), "grbg": (1, 0, 2, 1), "rggb": (0, 1, 1, 2), "bggr": (2, 1, 1, 0)}


def gray_of_rgb_ref(rgb, pattern, bit_depth):
    """rgb [n,3,H,W] float32 -> gray [n,H/2,W/2] float32 in DN: dn_k = ((v_k + 1) * 0.5) * (2^bit_depth - 1) of the pattern's
    colour at each CFA position, then (((dn_0 + dn_1) + dn_2) + dn_3) * 0.25."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.float32 and rgb.ndim == 4 and rgb.shape[1] == 3
    one, half, quarter, top = np.float32(1.0), np.float32(0.5), np.float32(0.25), np.float32(2 ** bit_depth - 1)
    dn = [((rgb[:, COLOURS[pattern][k], (k >> 1)::2, (k & 1)::2] + one) * half) * top for k in range(4)]
    gray = (((dn[0] + dn[1]) + dn[2]) + dn[3]) * quarter
    assert gray.dtype == np.float32
    return np.ascontiguousarray(gray)

