"""Which gather of the feature warps (warp.h warp48_gather_quad) a 2 x 2 quad of pixels takes, restated in torch on top of
hard_flows.gather_paths, and the inputs that test_warp48_quad_host.py and test_gpu_warp48_quad.py share.  A plain module: no
fixtures, no pytest settings; pytest does not rewrite its asserts, so each one carries its message.

A quad is the pixels a = (x, y), b = (x+1, y), c = (x, y+1), d = (x+1, y+1) with x and y even.  Its class:

    quad     both rows are lined-up pairs (hard_flows._lined_up), the rows of c are those of a shifted by one, c has a's four
             columns and d's last column is b's: the four footprints are the same five rows and five columns, 25 loads
    rows     not that, but at least one of its two rows is a lined-up pair (20 loads for that row)
    single   neither row is: 16 loads per pixel

all on the clamped tap indices, as the kernel decides it."""
import torch

import hard_flows as HF

CLASSES = ("quad", "rows", "single")
SHAPES = HF.STEP_SHAPES + ((1, 22, 64),)      # the last: a width that is a multiple of the workgroup's 32 columns
STEPS = 3                                     # frame-steps from a reset: the first warps no features, the other two do
NETS = {"convunet+feat": "recurrent-convunet+feat-iso3200",                   # warp48_kernel
        "next+feat": "recurrent-ConvNeXtUnet+feat-future-iso3200"}            # warp48_proj_kernel (row-pair level only)


def quad_classes(flow_raw, H, W):
    """flow_raw [..., 2, h, w] -> dict of three boolean maps [..., H/2, W/2], exactly one of them true per quad"""
    g = HF.gather_paths(flow_raw, H, W)
    xi, yi, pair = g["xi"], g["yi"], g["lined_up"]
    xa, xb, xc, xd = xi[..., 0::2, 0::2, :], xi[..., 0::2, 1::2, :], xi[..., 1::2, 0::2, :], xi[..., 1::2, 1::2, :]
    ya, yc = yi[..., 0::2, 0::2, :], yi[..., 1::2, 0::2, :]
    top, low = pair[..., 0::2, :], pair[..., 1::2, :]
    quad = top & low & (yc[..., :3] == ya[..., 1:]).all(-1) & (xc == xa).all(-1) & (xd[..., 3] == xb[..., 3])
    rows = ~quad & (top | low)
    return {"quad": quad, "rows": rows, "single": ~quad & ~rows}


def shares(flow_raw, H, W):
    c = quad_classes(flow_raw, H, W)
    return {k: float(c[k].float().mean()) for k in CLASSES}


def step_inputs(family, shape, fut):
    """raw, flow_prev, flow_next of STEPS frame-steps from a reset (hard_flows.step_inputs with as many frames as they read)"""
    return HF.step_inputs(family, shape, STEPS + 1 + fut)


def warping_flows(family, shape, fut):
    """the raw-resolution flows [2, B, 2, h, w] that the feature warps of steps 2 and 3 take"""
    return step_inputs(family, shape, fut)[1][2:STEPS + 1]

