"""The feature warps' gather by 2 x 2 quads (the default) against the gather by pixel pairs (option "warp48_pairs" 1): the same
bits.  Needs a real MI355X: -m gpu.

warp48_kernel (convunet+feat) gathers through warp.h's warp48_gather_quad: 25 loads for a quad whose four footprints are the
same five rows and columns, the pair form row by row otherwise, 16 loads per pixel below that.  warp48_proj_kernel (next+feat)
shares the pair level of the same header and stays there (the option is inert for it; the case pins that).  A pixel's
values, weights and order of sums are the same at every level, so the two options must agree bit for bit: three
frame-steps from a reset (the first warps nothing, the other two do) on every flow family of hard_flows.py -- smooth, broken
at rectangle edges, clamped at all four borders, different from pixel to pixel; test_warp48_quad_host.py holds these inputs
to reaching all three levels -- at two odd shapes of more than one workgroup and one whose width is a multiple of the
workgroup's 32 columns.  The oracle tests (test_gpu_hard_flows.py, test_gpu_parity.py, test_gpu_random_weights.py) hold the
default to the reference."""
import pytest
import torch

import hard_flows as HF
import warp_quads as Q
from gpu_support import launches, make_runtime

pytestmark = pytest.mark.gpu

_id = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _steps(arch, stem, fut, shape, raw, fp, fn, pairs):
    """-> the output frames of the three steps, the features after the last, the launches of the profile"""
    rt = make_runtime(arch, stem, fut, *shape, warp48_pairs=pairs)
    try:
        rt.profile_enable(True)
        outs = [rt.step(raw[0] if t == 1 else None, raw[t], raw[t + 1] if fut else None, fp[t], fn[t] if fut else None).cpu()
                for t in range(1, Q.STEPS + 1)]
        seen = launches(rt)
        rt.profile_enable(False)
        return outs, rt.get_state()[1].cpu(), seen
    finally:
        rt.close()


@pytest.mark.parametrize("shape", Q.SHAPES, ids=_id)
@pytest.mark.parametrize("family", HF.FAMILIES)
@pytest.mark.parametrize("arch", sorted(Q.NETS))
def test_quads_give_the_bits_of_pairs(arch, family, shape):
    stem = Q.NETS[arch]
    assert HF.STEP_NETS[stem][0] == arch
    fut = HF.STEP_NETS[stem][1]
    raw, fp, fn = (t.cuda() for t in Q.step_inputs(family, shape, fut))
    got = {pairs: _steps(arch, stem, fut, shape, raw, fp, fn, pairs) for pairs in (0, 1)}
    for pairs, (outs, feat, seen) in got.items():
        assert seen.get("warp48_kernel", (0, 0))[0] >= Q.STEPS - 1, (pairs, sorted(seen))
        assert all(torch.isfinite(o).all() for o in outs) and torch.isfinite(feat).all(), pairs
    for t, (q, p) in enumerate(zip(got[0][0], got[1][0])):
        assert torch.equal(q, p), (arch, family, shape, "frame", t + 1, float((q - p).abs().max()))
    assert torch.equal(got[0][1], got[1][1]), (arch, family, shape, "features", float((got[0][1] - got[1][1]).abs().max()))
    assert float(got[0][1].abs().max()) > 0, "the features are not all zero"
