"""rvdd_warp_bicubic and rvdd_upsample_factor_2 against the oracle's explicit f32 restatements (oracle/rvdd_oracle.py warp_explicit,
upsample_factor_2_explicit: "the arithmetic the HIP warp kernel implements"), through the ABI.  Needs a real MI355X: -m gpu.

warp.hip follows the reference's f32 arithmetic operation for operation (the round trip of the coordinates through [-1, 1]
included, -ffp-contract=off), and so do the two restatements on the CPU, ATen's grid_sample and warp_explicit: they agree with
each other within 0.7 .. 2.7e-7 of the output's maximum where both sit 0.2 .. 2.9e-5 from the same warp in f64
(test_hard_flows_host.py recomputes these).  The yardstick is therefore the f32 restatement, and the bar a few ulps:

    max|hip - explicit32| / max|f64| <= 4 * max(s_ref, 2^-23),    s_ref = max|ATen32 - explicit32| / max|f64| of the very case

The 4 is the room for a 16-tap sum whose roundings may fall differently, not a measured number.  Under this bar a block-clamped
footprint, a pair of pixels sharing weights or columns, or coordinates without the round trip fail by 3x .. 10^6x
(test_hard_flows_host.py, hard_flows.warp_mutant).  Beside it: err(hip, f64) <= 2 err(explicit32, f64).

Measured on an MI355X (the RATIO lines): both kernels give the explicit restatement's bits in all 42 + 10
cases, ratio 0."""
import pytest
import torch

import hard_flows as HF
import rvdd_oracle as O
from gpu_support import ops_rt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flows", HF.WARP_FLOWS)
@pytest.mark.parametrize("shape", HF.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_warp_bicubic_vs_explicit_f32(shape, flows):
    """warp_nchw_kernel on the smallest frame the ABI accepts, one-row and one-column strips, odd sizes, 48 channels, and a
    ragged last block with odd rows (129 x 257 = 33 153 pixels); flows N(0, 1.5), N(0, 30), N(0, 1e4) pixels and the four families
    of hard_flows.py upsampled."""
    x, flow, want, s_ref, e32, top = HF.warp_case(shape, flows)
    got = ops_rt().warp(x.cuda(), flow.cuda()).cpu()
    assert torch.isfinite(got).all()
    d = float((got.double() - want.double()).abs().max()) / top
    e = float((got.double() - O.warp(x.double(), flow.double())).abs().max()) / top
    bound = 4 * max(s_ref, HF.EPS32)
    print(f"RATIO | warp_nchw_kernel | {'x'.join(map(str, shape))} {flows} | {d / bound:.3f} | hip-explicit {d:.3g} s_ref {s_ref:.3g} "
          f"| f64: hip {e:.3g} explicit {e32:.3g}")
    assert d <= bound, (d, bound, s_ref)
    assert e <= 2 * e32, (e, e32)


@pytest.mark.parametrize("mul", [1, 2])
@pytest.mark.parametrize("shape", HF.UPSAMPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_factor_2_vs_explicit_f32(shape, mul):
    """upsample_flow_kernel (flow_fetch's arithmetic restated by hand) on a single sample, one-row and one-column strips, an even
    and an odd size; values N(0, 20)."""
    t, want, spread, top = HF.upsample_case(shape, mul)
    got = ops_rt().upsample_factor_2(t.cuda(), mul).cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    d = float((got.double() - want.double()).abs().max()) / top
    bound = 4 * max(spread, HF.EPS32)
    print(f"RATIO | upsample_flow_kernel | {'x'.join(map(str, shape))} x{mul} | {d / bound:.3f} | hip-explicit {d:.3g} spread {spread:.3g}")
    assert d <= bound, (d, bound, spread)
