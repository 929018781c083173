"""The nets under dense random weights against the oracle in f64 (tests/random_weights.py).  Needs a real MI355X: -m gpu.

Every other network test loads a trained checkpoint and asks for max-abs < 1e-4, about 100x the arithmetic's own noise on
weights whose taps and channels are mostly near zero.  Here every tap, channel and bias counts, the `pow2` profiles walk
the per-layer powers of two of the split-f16 banks, of the scaled GELU and of the projection halves over their range and
put split-f16 and f32-MFMA ConvBlocks into one handle, and the bar is a multiple of the reference's own f32 noise:

    rel_err(hip, f64) <= R * e_ref,    e_ref = rel_err(f32 oracle on the CPU, f64 oracle), same weights, same inputs

with rel_err = max|got - want| / max|want|.  e_ref is 0.45 .. 1.5e-6 for these cases (test_random_weights_host.py holds
it below 5e-6).  One swapped tap, one f16-rounded layer or one wrong coefficient lands 16x .. 30 000x above e_ref, so R is
capped at 8 whatever is measured; inside the cap R is twice the worst ratio measured on an MI355X, rounded up.

Worst rel_err(hip, f64) / e_ref measured over all cases below, per kernel family, and the R it gives:

    kernel family (options)                                    cases   worst ratio   R
    split-f16 conv (conv_kernel 0; +feat: fuse_pre 0)             96       7.51        8      (twice the worst is 16: capped)
    direct f32 (conv_kernel 1)                                    96       2.72        6
    Winograd f32 (conv_kernel 2)                                  96       1.30        3
    composed first layer (+feat, conv_kernel 0, pre5_cin8 1 / 0)  96 + 24  7.51 / 4.90 8      (forward / frame-steps; capped)
    ConvBlock split (next_split 1: pipe, projfuse 1 / 0)         144 + 12  1.64 / 2.03 5      (forward / frame-steps)
    ConvBlock f32 (next_split 0)                                  48       1.37        3
    projection halves against the projection kernel               12       1.40        2 x 5  (of e_ref, not against f64)

A FINDING, not fixed here: the two split-f16 conv families sit at 1.1 .. 4.2e-6 of the output (median 1.9e-6) where the
direct f32 kernel sits at 0.7 .. 2.4e-6 (median 1.1e-6), and need more than the cap allows as a margin.  The cause is
in how the operands are split, not in any one layer: the kernels split activations with v_cvt_pkrtz_f16_f32 (hi toward
zero) and rvdd_finalize_weights splits the filters the same way (csrc/handle.hip f16_bits(w, true)), so every lo half
has its value's sign, the dropped lo.lo term of every product has the product's sign, each layer's sums come out about
1.1e-7 too small and the layers of a net in series add that up: the outputs carry a gain of 1 - 1 .. 2e-6.  Emulated on
the CPU with exact accumulation the scheme gives rel_err 1.3 .. 2.3e-6 with the filters' hi halves toward zero and
0.3 .. 0.6e-6 with them to nearest; a library built with the hi halves of the banks to nearest (host code only, no
kernel touched) measured 2.21 / 2.21 / 1.41 in the three split families on an MI355X.  That change moves every
output of the split paths by about 1e-6, and the suite holds those paths to stored bits of an earlier library
(tests/golden/prologue_parent_*.npz) and to a count of demosaic sign flips under --warp_raw
(test_gpu_bayer.py::test_sequence_parity_vs_oracle) that such a move re-rolls: it belongs in a change of its own that
regenerates those fixtures.  Until then the two families are held at the cap.

The ConvBlocks that fall back to the f32-MFMA form inside a split-f16 handle (|s1| > 15, 6.86 |ln_w| >= 32768) cannot be
told apart through rvdd_profile_read: both forms are launched under the class "convblock_kernel".  That both forms ran is
therefore pinned on the host (test_random_weights_host.py::test_pow2_profiles_hit_the_edges_they_are_for restates the
decision of rvdd_finalize_weights on the same tensors), not observed on the device."""
import pytest
import torch

import rvdd_oracle as O
import random_weights as RW
from hard_flows import _device_steps, _oracle_steps, _sequences, wild
from random_weights import R

pytestmark = pytest.mark.gpu

# one tile with every pixel within two of the border; ragged tiles, odd level sizes (zero_pad_features at every decoder
# stage), a batch; a second ragged size; 80 tiles: the output-channel split at every level, workgroups of the pipelined
# ConvBlock with more than one tile
SIZES = [(1, 16, 16), (3, 50, 66), (2, 18, 34), (1, 128, 160)]
UNETS = [("convunet", "recurrent-convunet-iso3200", 0), ("convunet", "recurrent-convunet-future-iso3200", 1),
         ("convunet+feat", "recurrent-convunet+feat-iso3200", 0),
         ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1)]
NEXTS = [("next", "recurrent-ConvNeXtUnet-iso3200", 0), ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1)]


def _reference(stem, profile, seed, B, H, W):
    """-> (weights, x, feat_in, f64 oracle's (out, feat_out), e_ref of each)"""
    sd = RW.random_state_dict(stem, seed, profile)
    x, f = RW.net_inputs(B, O.net_input_nc(sd), H, W, 1000 * seed + H, O.net_has_feat(sd))
    with torch.no_grad():
        o32 = O.net_forward(sd, x, f)
        o64 = O.net_forward(RW.to64(sd), x.double(), None if f is None else f.double())
    e_ref = [None if a is None else RW.rel_err(a, b) for a, b in zip(o32, o64)]
    return sd, x, f, o64, e_ref


def _compare(bad, family, tag, got, want64, e_ref):
    for name, g, w, e in zip(("out", "feat_out", "out2", "feat2"), got, want64, e_ref):
        if w is None:
            continue
        assert torch.isfinite(g).all(), (family, tag, name)
        err = RW.rel_err(g, w)
        print(f"RATIO | {family} | {tag} {name} | {err / e:.3f} | hip {err:.3g} e_ref {e:.3g}")
        if not err <= R[family] * e:
            bad.append((family, tag, name, err, e, err / e))


def _forward(arch, fut, shape, sd, x, f, options):
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime(arch, fut, *shape, 0)
    try:
        for k, v in options.items():
            rt.set_option(k, v)
        rt.load_state_dict(sd)
        out, fo = rt.unet_forward(x.cuda(), None if f is None else f.cuda())
        return out.cpu(), None if fo is None else fo.cpu()
    finally:
        rt.close()


@pytest.mark.parametrize("B,H,W", SIZES)
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("profile", ["he", "pow2"])
@pytest.mark.parametrize("arch,stem,fut", UNETS)
def test_convunet_forward_vs_f64_oracle(arch, stem, fut, profile, seed, B, H, W):
    """rvdd_unet_forward of the convunets with every 3x3 conv on the split-f16 kernel, the direct f32 kernel and the Winograd
    f32 kernel; the feature-recurrent ones also with the two convs of the first layer in place of their composition, and
    with the composed layer's 16-channel bank."""
    sd, x, f, o64, e_ref = _reference(stem, profile, seed, B, H, W)
    feat = arch.endswith("+feat")
    forms = [("composed first layer" if feat else "split-f16 conv", {"conv_kernel": 0}),
             ("direct f32", {"conv_kernel": 1}), ("Winograd f32", {"conv_kernel": 2})]
    if feat:
        forms.append(("split-f16 conv", {"conv_kernel": 0, "fuse_pre": 0}))
        if not fut:                                   # "pre5_cin8" is inert with a future frame (9 channels)
            forms.append(("composed first layer", {"conv_kernel": 0, "pre5_cin8": 0}))
    bad = []
    for family, opts in forms:
        got = _forward(arch, fut, (B, H, W), sd, x, f, opts)
        _compare(bad, family, f"{stem} {profile} {seed} {B}x{H}x{W} {opts}", got, o64, e_ref)
    assert not bad, bad


@pytest.mark.parametrize("B,H,W", SIZES)
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("profile", ["he", "pow2"])
@pytest.mark.parametrize("arch,stem,fut", NEXTS)
def test_convnext_forward_vs_f64_oracle(arch, stem, fut, profile, seed, B, H, W):
    """rvdd_unet_forward of the ConvNeXt nets in the four forms the options give: the pipelined split-f16 block with the
    projection halves in the epilogues and with the projection kernel, the phased split-f16 block ("next_projfuse" is
    inert without the pipeline), and the f32-MFMA block ("next_pipe" and "next_projfuse" are inert without the split).
    Under `pow2` a split-f16 handle holds blocks of both forms."""
    sd, x, f, o64, e_ref = _reference(stem, profile, seed, B, H, W)
    bad = []
    for family, opts in (("ConvBlock split", {"next_split": 1, "next_pipe": 1, "next_projfuse": 1}),
                         ("ConvBlock split", {"next_split": 1, "next_pipe": 1, "next_projfuse": 0}),
                         ("ConvBlock split", {"next_split": 1, "next_pipe": 0}),
                         ("ConvBlock f32", {"next_split": 0})):
        got = _forward(arch, fut, (B, H, W), sd, x, f, opts)
        _compare(bad, family, f"{stem} {profile} {seed} {B}x{H}x{W} {opts}", got, o64, e_ref)
    assert not bad, bad


@pytest.mark.parametrize("B,H,W", [(3, 50, 66), (1, 16, 16)])
@pytest.mark.parametrize("profile", ["he", "pow2"])
@pytest.mark.parametrize("arch,stem,fut,family", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, "composed first layer"),
    ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, "composed first layer"),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, "ConvBlock split")])
def test_steps_no_warp_vs_f64_oracle(arch, stem, fut, family, profile, B, H, W):
    """Two frame-steps with option "no_warp" -- the first-step latch with zero features, then recurrent features and a
    previous output -- against the same two steps with the net and the state in f64: the forms only a step has (the
    one-kernel pre-stage and the tiled network input, the network input's projection, the composed first layer behind
    the prologue's border ring) under dense weights.  Every network input is demosaicked frames (bit for bit the
    device's) and the previous output."""
    sd = RW.random_state_dict(stem, 5, profile)
    raw, _, _ = _sequences(B, H, W, 3 + fut, 1300)
    o32 = _oracle_steps(sd, fut, raw, torch.float32)
    o64 = _oracle_steps(sd, fut, raw, torch.float64)
    e_ref = [RW.rel_err(a, b) for a, b in zip(o32, o64)]
    got = _device_steps(arch, fut, (B, H, W), sd, raw, {"no_warp": 1})
    bad = []
    for name, g, w, e in zip(("out 1", "out 2", "features"), got, o64, e_ref):
        assert torch.isfinite(g).all(), name
        err = RW.rel_err(g, w)
        print(f"RATIO | {family} | step {stem} {profile} {B}x{H}x{W} {name} | {err / e:.3f} | hip {err:.3g} e_ref {e:.3g}")
        if not err <= R[family] * e:
            bad.append((name, err, e, err / e))
    assert not bad, bad


@pytest.mark.parametrize("flows", ["synth", "wild"])
@pytest.mark.parametrize("profile", ["he", "pow2"])
def test_feature_warp_projection_half_dense_weights(profile, flows):
    """warp48_proj_kernel (the feature warp with the features' half of the 96 -> 48 projection, "next_projfuse" 1) against
    warp48_kernel and the projection kernel ("next_projfuse" 0) under dense weights, over two recurrent steps, on smooth
    flows and on flows that leave the frame and differ from pixel to pixel.  The two forms share the warp's arithmetic,
    so frames and features are finite and within twice the bound of the forward tests, 2 R e_ref of the larger map's
    maximum; e_ref is that of the very case: the same two steps in the oracle, f32 against f64, warps included."""
    arch, stem, fut, (B, H, W) = "next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, (2, 72, 104)
    sd = RW.random_state_dict(stem, 7, profile)
    raw, fp, fn = _sequences(B, H, W, 4, 1680)
    if flows == "wild":
        fp = wild(fp, 5)
    o32 = _oracle_steps(sd, fut, raw, torch.float32, fp, fn)
    o64 = _oracle_steps(sd, fut, raw, torch.float64, fp, fn)
    e_ref = [RW.rel_err(a, b) for a, b in zip(o32, o64)]
    a, b = (_device_steps(arch, fut, (B, H, W), sd, raw, {"next_projfuse": v}, fp, fn) for v in (1, 0))
    bad = []
    for name, x, y, e in zip(("out 1", "out 2", "features"), a, b, e_ref):
        assert torch.isfinite(x).all() and torch.isfinite(y).all(), name
        d = float((x.double() - y.double()).abs().max() / max(x.abs().max(), y.abs().max()))
        print(f"RATIO | projection halves | {profile} {flows} {name} | {d / e:.3f} | diff {d:.3g} e_ref {e:.3g}")
        if not d <= 2 * R["ConvBlock split"] * e:
            bad.append((name, d, e, d / e))
    assert not bad, bad
