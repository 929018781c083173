"""The inputs of test_gpu_warp48_quad.py reach all three levels of the feature warps' gather (warp.h warp48_gather_quad: the
2 x 2 quad, the row pair, the single pixel), and the benchmark's flows take the quad level almost everywhere.  CPU only.  The
shares are conditions on the inputs (tests/warp_quads.py restates the kernel's predicate), not measurements of the kernel."""
import pytest
import torch

import hard_flows as HF
import warp_quads as Q

_id = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def test_classes_are_exclusive_and_follow_the_pair_predicate():
    """Every quad has exactly one class; a quad-level quad has two lined-up rows; on a constant flow every quad -- the clamped
    border included -- is quad-level, and a flow that alternates by several pixels from column to column sends most quads to
    single pixels."""
    H, W = 18, 34
    fl = Q.warping_flows("blocks", (3, H, W), 0)
    c = Q.quad_classes(fl, H, W)
    n = sum(c[k].long() for k in Q.CLASSES)
    assert bool((n == 1).all()), (int(n.min()), int(n.max()))
    pair = HF.gather_paths(fl, H, W)["lined_up"]
    assert bool((c["quad"] <= (pair[..., 0::2, :] & pair[..., 1::2, :])).all())
    assert bool((c["single"] == (~pair[..., 0::2, :] & ~pair[..., 1::2, :])).all())
    const = torch.full((1, 2, H // 2, W // 2), 0.3)
    assert Q.shares(const, H, W)["quad"] == 1.0
    far = torch.full((1, 2, H // 2, W // 2), 40.0)        # every footprint clamped to one corner: the same rows and columns
    assert Q.shares(far, H, W)["quad"] == 1.0
    zig = torch.zeros(1, 2, H // 2, W // 2)
    zig[:, 0, :, 0::2] = 7.0                              # raw columns alternate by 7 px: neighbours share columns only
    assert Q.shares(zig, H, W)["single"] > 0.5, Q.shares(zig, H, W)      # where the border clamps both (0.82 single)


@pytest.mark.parametrize("fut", (0, 1))
@pytest.mark.parametrize("shape", HF.STEP_SHAPES, ids=_id)
@pytest.mark.parametrize("family", ("blocks", "border"))
def test_hard_flows_reach_every_level(family, shape, fut):
    s = Q.shares(Q.warping_flows(family, shape, fut), *shape[1:])
    print(family, shape, fut, s)
    assert all(s[k] >= 0.05 for k in Q.CLASSES), (family, shape, s)


@pytest.mark.parametrize("shape", HF.STEP_SHAPES, ids=_id)
def test_wild_flows_are_single_pixels(shape):
    s = Q.shares(Q.warping_flows("wild", shape, 0), *shape[1:])
    assert s["single"] >= 0.80, (shape, s)


def test_the_benchmarks_flows_are_quads():
    from rvdd_release_amd import synth
    s = Q.shares(synth.make_sequence(2, 720, 1280, iso=3200, seed=2000).flow_prev[1], 720, 1280)
    assert s["quad"] >= 0.95, s
