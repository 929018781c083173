"""What the GPU tests of the warps rest on, recomputed on the CPU (hard_flows.py; test_gpu_warp_ops.py, test_gpu_hard_flows.py):
the inputs reach both gathers of warp48_kernel, clamped footprints and pixels wholly outside the frame; the references are
well conditioned there; and the bounds would catch a warp that is subtly wrong."""
import pytest
import torch

import hard_flows as HF
import random_weights as RW
import rvdd_oracle as O

_id = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
STEP_CASES = [(stem, "gbrg") for stem in HF.STEP_NETS] + [HF.BAYER_CASE]


@pytest.mark.parametrize("shape", [(2, 5, 37, 53), (2, 48, 50, 66), (3, 2, 2, 302)], ids=_id)
@pytest.mark.parametrize("family", HF.FAMILIES)
def test_gather_paths_take_warp_explicit_taps(family, shape):
    """The taps gather_paths reports, summed with warp_explicit's weights in its order, give warp_explicit bit for bit on a
    random image (one wrong index changes a pixel), and so does the form the mutants are built on."""
    n, c, H, W = shape
    x, flow, want, *_ = HF.warp_case(shape, family)
    assert torch.equal(HF.warp_from_taps(x, flow), want)
    if H % 2 == 0 and W % 2 == 0:
        raw = HF.family_flow(family, HF._sequences(n, max(H, 16), max(W, 16), 2, 40)[1][:, :, :, :H // 2, :W // 2], 41)[1]
        g = HF.gather_paths(raw, H, W)
        _, _, wx, wy = HF.taps(HF.full_flow(raw))
        assert torch.equal(HF.gather_sum(x, g["xi"], g["yi"], wx, wy), O.warp_explicit(x, HF.full_flow(raw)))


def _fractions(flow_raw, H, W):
    g = HF.gather_paths(flow_raw, H, W)
    return {k: float(g[k].float().mean()) for k in ("lined_up", "partly", "outside")}


def _check_reach(family, fr, what):
    if family in ("blocks", "border"):
        assert 0.05 <= fr["lined_up"] <= 0.95, (what, fr)              # both gathers of warp48_kernel
    if family in ("blocks", "border", "wild"):
        assert fr["partly"] >= 0.05, (what, fr)
    if family in ("blocks", "wild"):
        assert fr["outside"] >= 0.03, (what, fr)


@pytest.mark.parametrize("shape", HF.STEP_SHAPES, ids=_id)
@pytest.mark.parametrize("family", HF.FAMILIES)
def test_inputs_reach_every_branch_of_the_gather(family, shape):
    """Conditions on the flows of test_gpu_hard_flows.py, for the two steps it runs and for both flows of a step."""
    B, H, W = shape
    _, fp, fn = HF.step_inputs(family, shape, 4)
    for name, fl in (("flow_prev", fp[1:3]), ("flow_next", fn[1:3])):
        fr = _fractions(fl, H, W)
        print(f"REACH | {family} {_id(shape)} {name} | lined_up {fr['lined_up']:.3f} partly {fr['partly']:.3f} outside {fr['outside']:.3f}")
        _check_reach(family, fr, (family, shape, name))
    if family == "synth":       # what the suite had: nearly every pair on the shared gather, no pixel to speak of outside
        assert fr["lined_up"] > 0.95 and fr["outside"] < 0.03, fr


def test_wild_flows_of_the_projection_halves_test():
    """test_gpu_random_weights.py::test_feature_warp_projection_half_dense_weights[wild]: its flow, generated as there."""
    _, fp, _ = HF._sequences(2, 72, 104, 4, 1680)
    fr = _fractions(HF.wild(fp, 5)[1:3], 72, 104)
    print(f"REACH | wild 2x72x104 | {fr}")
    _check_reach("wild", fr, "wild 72x104")


@pytest.mark.parametrize("flows", HF.WARP_FLOWS)
@pytest.mark.parametrize("shape", HF.WARP_SHAPES, ids=_id)
def test_stage_references_agree_to_a_few_ulps(shape, flows):
    """ATen's grid_sample and warp_explicit in f32: within 4 ulps of the output's maximum of each other at every case of
    test_gpu_warp_ops.py (measured 0 .. 2.7e-7), where both sit up to 2.9e-5 from the same warp in f64: the bound of the GPU
    test, 4 max(s_ref, 2^-23), is at most 16 ulps."""
    x, flow, want, s_ref, e32, top = HF.warp_case(shape, flows)
    print(f"SPREAD | warp {_id(shape)} {flows} | s_ref {s_ref:.3g} err(explicit32, f64) {e32:.3g}")
    assert torch.isfinite(want).all() and s_ref <= 4 * HF.EPS32, s_ref


@pytest.mark.parametrize("mul", [1, 2])
@pytest.mark.parametrize("shape", HF.UPSAMPLE_SHAPES, ids=_id)
def test_upsample_references_agree_to_a_few_ulps(shape, mul):
    t, want, spread, top = HF.upsample_case(shape, mul)
    print(f"SPREAD | upsample {_id(shape)} x{mul} | {spread:.3g}")
    assert spread <= 4 * HF.EPS32, spread


@pytest.mark.parametrize("shape", HF.STEP_SHAPES, ids=_id)
@pytest.mark.parametrize("family", HF.STEP_FLOWS)
@pytest.mark.parametrize("weights", HF.STEP_WEIGHTS)
@pytest.mark.parametrize("stem,pattern", STEP_CASES)
def test_step_references_are_well_conditioned(stem, pattern, weights, family, shape):
    """e_ref of every case of test_gpu_hard_flows.py, and the same two steps with an independent f32 implementation of the warps
    (warp_explicit, upsample_factor_2_explicit) in place of ATen's: it lands within [0.5, 2] of e_ref (measured 0.57 .. 1.53), so R
    of DESIGN section 4 keeps its meaning with the warps in the loop.  With the trained weights the f32 oracle is within 2e-5 of
    the f64 one, a fifth of the 1e-4 the device is held to."""
    _, fut = HF.STEP_NETS[stem]
    sd, raw, fp, fn, o32, o64, e_ref = HF.step_reference(stem, weights, family, shape, pattern)
    dm = None
    if pattern != "gbrg":
        import bayer_ref
        dm = lambda r: bayer_ref.hamilton_adams(r, pattern)
    ox = HF._oracle_steps(sd, fut, raw, torch.float32, fp, fn, warp=O.warp_explicit,
                          upsample=lambda fl: O.upsample_factor_2_explicit(fl, 2), demosaic=dm)
    for name, a, b, w, e in zip(("out 1", "out 2", "features"), ox, o32, o64, e_ref):
        if w is None:
            continue
        ratio = RW.rel_err(a, w) / e
        print(f"E_REF | {stem} {pattern} {weights} {family} {_id(shape)} {name} | e_ref {e:.3g} explicit / ATen {ratio:.2f}")
        assert 0.5 <= ratio <= 2.0, (name, ratio, e)
        if weights == "trained":
            assert float((b.double() - w).abs().max()) <= 2e-5, name


MUTANT_FLOWS = {      # where the mistake can show at all
    "a": ("synth", "wild", "blocks"),       # a lined-up pair whose two pixels differ in their vertical fraction: `border`'s vertical flow
                                            # is constant along a row, N(0, 1e4) samples the frame's corners
    "b": ("synth", "wild", "blocks", "border"),
    "c": HF.WARP_FLOWS,                     # a partly clamped footprint: every flow has them at the frame's edge
    "d": tuple(f for f in HF.WARP_FLOWS if f != "n1e4"),      # a pixel that samples inside the frame
}


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_stage_bound_catches_a_wrong_gather(kind):
    shape = (2, 48, 50, 66)
    for flows in MUTANT_FLOWS[kind]:
        x, flow, want, s_ref, e32, top = HF.warp_case(shape, flows)
        d = float((HF.warp_mutant(x, flow, kind).double() - want.double()).abs().max()) / top
        assert d >= 10 * 4 * max(s_ref, HF.EPS32), (kind, flows, d, s_ref)


@pytest.mark.parametrize("shape", [s for s in HF.WARP_SHAPES if s[2] >= 37 and s[3] >= 53], ids=_id)
def test_stage_bound_catches_coordinates_without_the_round_trip(shape):
    for flows in MUTANT_FLOWS["d"]:
        x, flow, want, s_ref, e32, top = HF.warp_case(shape, flows)
        d = float((HF.warp_mutant(x, flow, "d").double() - want.double()).abs().max()) / top
        assert d > 4 * max(s_ref, HF.EPS32), (flows, d, s_ref)


@pytest.mark.parametrize("kind", sorted(HF.STEP_MUTANTS))
def test_step_bound_catches_a_wrong_flow(kind):
    """trained convunet+feat, `blocks`, 2 x 50 x 66: the device is held to 1e-4 of the f32 oracle there"""
    stem = "recurrent-convunet+feat-iso3200"
    sd, raw, fp, fn, o32, _, _ = HF.step_reference(stem, "trained", "blocks", (2, 50, 66))
    om = HF._oracle_steps(sd, 0, raw, torch.float32, fp, fn, **HF.STEP_MUTANTS[kind])
    for name, a, b in zip(("out 1", "out 2", "features"), om, o32):
        assert float((a - b).abs().max()) >= 10 * 1e-4, (kind, name)
