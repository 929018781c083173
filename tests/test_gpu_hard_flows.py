"""The warps inside a frame-step against the oracle under hard flows (tests/hard_flows.py).  Needs a real MI355X: -m gpu.

The bicubic backward warp is the recurrence: every output frame and every 48-channel feature map of step t enters step t + 1
through warp48_kernel / warp48_proj_kernel and the warps inside netin_kernel, netin_proj_kernel and netin_small_kernel.  The
other oracle tests feed them synth's smooth flows, which send 99 % of warp48_kernel's pixel pairs down its shared gather and
no pixel wholly outside the frame; the tests with harder flows compare one device form with another, and all forms share
warp.h.  Here: two frame-steps from a reset with flows that leave the frame, differ from pixel to pixel (`wild`), break at
rectangle edges (`blocks`) or push the footprints over all four borders (`border`), against the same two steps of the oracle
with ATen's grid_sample.  test_hard_flows_host.py holds the inputs to reaching both gathers, clamped footprints and pixels
wholly outside, shows the references well conditioned there (an independent f32 implementation of the warps lands at
0.57 .. 1.53 e_ref) and shows that a flow upsampled with the wrong corners, without its factor 2, or taken from the
neighbouring batch element misses the bars below by 500x and more.

    dense random weights   rel_err(hip, f64) <= R e_ref, R the kernel family's value of test_gpu_random_weights.py, e_ref the f32
                           oracle's own rel_err over the same two steps, warps included
    trained weights        max|hip - f32 oracle| < 1e-4, the suite's bar (the f32 oracle is within 2e-5 of the f64 one here)

The three outputs are frame 1, frame 2 and the features after step 2.  Worst rel_err(hip, f64) / e_ref measured on an MI355X:
DESIGN.md section 4, row "frame-steps with the warps under hard flows"."""
import pytest
import torch

import bayer_ref
import hard_flows as HF
import random_weights as RW
from random_weights import R

pytestmark = pytest.mark.gpu

NETIN = "netin(ha_green+netin_kernel)"      # the profile's class of netin_kernel, netin_proj_kernel and netin_small_kernel
# stem -> [(kernel family, options)]: the forms of the network input and of the feature warp that the options give
FORMS = {
    # netin_kernel with both warps (previous output, next frame)
    "recurrent-convunet-future-iso3200": [("split-f16 conv", {"conv_kernel": 0}), ("direct f32", {"conv_kernel": 1})],
    # netin_small_kernel / the three-kernel pre-stage, warp48_kernel
    "recurrent-convunet+feat-iso3200": [("composed first layer", {"conv_kernel": 0, "small_prestage": 1}),
                                        ("composed first layer", {"conv_kernel": 0, "small_prestage": 0}),
                                        ("direct f32", {"conv_kernel": 1, "small_prestage": 1}),
                                        ("direct f32", {"conv_kernel": 1, "small_prestage": 0})],
    # netin_kernel with both warps, warp48_kernel
    "recurrent-convunet+feat-future-iso12800": [("composed first layer", {"conv_kernel": 0})],
    # netin_proj_kernel + warp48_proj_kernel; netin_kernel + warp48_kernel + the projection kernel; the f32 ConvBlock
    "recurrent-ConvNeXtUnet+feat-future-iso3200": [("ConvBlock split", {"next_split": 1, "next_projfuse": 1}),
                                                   ("ConvBlock split", {"next_split": 1, "next_projfuse": 0}),
                                                   ("ConvBlock f32", {"next_split": 0})],
    # netin_proj_kernel alone
    "recurrent-ConvNeXtUnet-iso3200": [("ConvBlock split", {})],
}
CASES = [(stem, "gbrg") for stem in FORMS] + [HF.BAYER_CASE]
_id = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


@pytest.mark.parametrize("shape", HF.STEP_SHAPES, ids=_id)
@pytest.mark.parametrize("family", HF.STEP_FLOWS)
@pytest.mark.parametrize("weights", HF.STEP_WEIGHTS)
@pytest.mark.parametrize("stem,pattern", CASES)
def test_steps_with_warps_vs_oracle(stem, pattern, weights, family, shape):
    arch, fut = HF.STEP_NETS[stem]
    sd, raw, fp, fn, o32, o64, e_ref = HF.step_reference(stem, weights, family, shape, pattern)
    bad, proj = [], {}
    for fam, opts in FORMS[stem]:
        if pattern != "gbrg":
            opts = dict(opts, bayer_pattern=bayer_ref.PATTERNS.index(pattern))
        seen = {}
        got = HF._device_steps(arch, fut, shape, sd, raw, opts, fp, fn, seen=seen)
        assert NETIN in seen, sorted(seen)
        assert ("warp48_kernel" in seen) == arch.endswith("+feat"), sorted(seen)
        if "next_projfuse" in opts:
            proj[opts["next_projfuse"]] = seen.get("proj1x1_kernel", 0)
        for name, g, w32, w64, e in zip(("out 1", "out 2", "features"), got, o32, o64, e_ref):
            if w64 is None:
                continue
            assert torch.isfinite(g).all(), (opts, name)
            err, d32 = RW.rel_err(g, w64), float((g - w32).abs().max())
            print(f"RATIO | {fam} | hard-flow steps {stem} {pattern} {weights} {family} {_id(shape)} {opts} {name} | {err / e:.3f} "
                  f"| hip {err:.3g} e_ref {e:.3g} max|hip - f32 oracle| {d32:.3g}")
            if not (d32 < 1e-4 if weights == "trained" else err <= R[fam] * e):
                bad.append((fam, opts, name, err, e, err / e, d32))
    if proj:        # the projection of cat[y, warped features] is a kernel of its own only without the fused halves
        assert proj[0] > proj[1], proj
    assert not bad, bad
