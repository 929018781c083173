"""The nets under dense random weights in launches where every workgroup walks several tiles.  Needs a real MI355X: -m gpu.

Every matrix kernel of the two nets is a persistent workgroup on a tile list with a grid of min(tiles, CUs) (tests/tile_walk.py
restates the four rules), so what lives between two tiles of one workgroup -- the halo fetched a tile ahead, the next tile's
block-floating-point word, the filter bank staged once, the pipelined ConvBlock's hand-over from the front waves to the back
waves, uneven bands and workgroups without a tile -- runs only in a launch of more tiles than the chip has CUs.  The largest case of
test_gpu_random_weights.py has 80 tiles.  Here small frames in a batch larger than the CU count put every level of every
kernel family past it (and a handle past the 64 sequences that the partial-slot calls stop at), for less than one 720p frame:

    case A   (CUs + 3, 18, 34) = 259 sequences: level sizes 18x34, 9x17, 4x8, 2x4, every decoder stage zero-pads
    case B   (CUs // 20, 80, 112) = 12 sequences: interior tiles of two sequences and row changes inside one walk at level 0

Tiles per level and tiles per workgroup (fewest .. most of those that get any; idle = workgroups without a tile), 256 CUs,
as test_tile_walk_host.py prints and pins them:

    case  family      tiles per level          tiles per workgroup per level          idle
    A     split-f16   1554 / 518 / 259 / 259   6..7 / 2..3 / 1..2 / 1..2              -
    A     direct      2331 / 1036 / 259 / 259  9..10 / 4..5 / 1..2 / 1..2             -
    A     winograd    1554 / 518 / 259 / 259   6..7 / 2..3 / 1..2 / 1..2              -
    A     convblock   1554 / 518 / 259 / 259   5..7 / 1..3 / 1..2 / 1..2              4 at levels 2 and 3
    B     split-f16   420 / 144 / 48 / 12      1..2 / 1 / 1 / 1                       -
    B     direct      840 / 240 / 72 / 24      3..4 / 1 / 1 / 1                       -
    B     winograd    480 / 120 / 36 / 24      1..2 / 1 / 1 / 1                       -
    B     convblock   420 / 144 / 48 / 12      1..2 / 1 / 1 / 1                       4 at level 3

The reference of every test is the same sequences through handles small enough that no launch has more tiles than CUs, the
regime test_gpu_random_weights.py holds to f64: case A in chunks of (CUs - 1) // 6 = 42 sequences on one handle and the
remaining 7 on another (between them the output-channel split both ways), case B in two halves.  The direct kernel's 8x16
tiles are nine to an 18x34 frame and 70 to an 80x112 one, so its handles take 28 and 3 sequences.  The big batch equals the
chunked runs BIT FOR BIT (include/rvdd.h, rvdd_step_live: every slot is what a handle of batch 1 gives, with the kernel
choice pinned), which needs no tolerance and tells one wrong halo pixel from f32 noise; on top of that the forward runs are
held to the f64 oracle at the bar of test_gpu_random_weights.py, R * e_ref over the whole batch, R from random_weights.py.

Worst rel_err(hip, f64) / e_ref measured on an MI355X over the cases below, and the R in force:

    kernel family (options)                                      outputs A + B   worst ratio A / B   R
    split-f16 conv (conv_kernel 0; +feat: fuse_pre 0)               12 + 12         3.26 / 3.47       8
    composed first layer (+feat, conv_kernel 0, pre5_cin8 1 / 0)    12 + 12         2.65 / 3.52       8
    direct f32 (conv_kernel 1)                                      12 + 12         2.38 / 2.01       6
    Winograd f32 (conv_kernel 2)                                    12 + 12         1.30 / 1.11       3
    ConvBlock split (next_split 1: pipe, projfuse 1 / 0; phased)     9 + 9          1.18 / 1.28       5
    ConvBlock f32 (next_split 0)                                     3 + 3          1.04 / 1.20       3

Every family stays inside the R that random_weights.py already has, so none is changed, and every form equals its chunked
runs bit for bit: the walks hold.  The mixed-magnitude runs and the frame-steps of the 259-sequence handle (with the
refusals of the batch <= 64 calls between the two steps) equal theirs too.

Measured on an MI355X: the whole file 52 s, of which the CPU oracle is most: the ConvNeXt cases 3.0 .. 6.5 s each (f32 and f64
of 259 frames), the convunet cases 1.1 .. 2.2 s, the mixed-magnitude cases 1.1 and 1.6 s, the frame-step cases under 0.3 s."""
import pytest
import torch

import random_weights as RW
import tile_walk as TW
from hard_flows import _device_steps, wild
from random_weights import R

pytestmark = pytest.mark.gpu

WALK_OF = {"split-f16 conv": "split-f16", "composed first layer": "split-f16", "direct f32": "direct", "Winograd f32": "winograd",
           "ConvBlock split": "convblock", "ConvBlock f32": "convblock"}
ERR_ARG = -1      # RVDD_ERR_ARG (include/rvdd.h)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _forward_parts(arch, fut, H, W, sd, x, f, options, parts):
    """rvdd_unet_forward of sequences [first, first + count) for every (first, count) of `parts`, one handle per count, options
    before the weights -> (out, feat_out) of all of them in order, on the CPU"""
    from rvdd_release_amd.runtime import RvddRuntime
    done = {}
    for n in sorted(set(c for _, c in parts), reverse=True):
        rt = RvddRuntime(arch, fut, n, H, W, 0)
        try:
            for k, v in options.items():
                rt.set_option(k, v)
            rt.load_state_dict(sd)
            for b, c in parts:
                if c == n:
                    out, fo = rt.unet_forward(x[b:b + c].cuda(), None if f is None else f[b:b + c].cuda())
                    done[b] = (out.cpu(), None if fo is None else fo.cpu())
        finally:
            rt.close()
    outs = [done[b] for b, _ in parts]
    return torch.cat([o for o, _ in outs]), None if outs[0][1] is None else torch.cat([g for _, g in outs])


def _first_difference(walk_family, case, name, big, ref):
    """where two [B, C, H, W] maps first differ: sequence, level-0 tile, pixel, and the workgroup that visits that tile"""
    B, _, H, W = big.shape
    ne = (big != ref) | (torch.isnan(big) != torch.isnan(ref))
    b, c, y, x = (int(v) for v in ne.nonzero()[0])
    th, tw = TW.TILE[walk_family]
    ty, tx = TW.tile_grid(walk_family, H, W)
    tile = (b * ty + y // th) * tx + x // tw
    wg, k, n = TW.visitor(walk_family, B * ty * tx, _cus(), tile)
    return (f"case {case} {name}: {int(ne.sum())} values of {int(ne.flatten(1).any(1).sum())} sequences differ from the chunked runs, the first in "
            f"sequence {b} channel {c} pixel ({y}, {x}) = {float(big[b, c, y, x])!r} against {float(ref[b, c, y, x])!r}: level-0 {walk_family} tile "
            f"{tile} (tile row {y // th}, column {x // tw}), tile {k + 1} of the {n} of workgroup {wg}")


def _same_as_chunks(bad, walk_family, case, tag, big, ref):
    for name, g, w in zip(("out", "feat_out"), big, ref):
        if g is not None and not torch.equal(g, w):
            bad.append((tag, _first_difference(walk_family, case, name, g, w)))


def _against_f64(bad, family, tag, got, want64, e_ref):
    for name, g, w, e in zip(("out", "feat_out"), got, want64, e_ref):
        if w is None:
            continue
        assert torch.isfinite(g).all(), (family, tag, name)
        err = RW.rel_err(g, w)
        print(f"RATIO | {family} | {tag} {name} | {err / e:.3f} | hip {err:.3g} e_ref {e:.3g}")
        if not err <= R[family] * e:
            bad.append((family, tag, name, err, e, err / e))


def _check_forms(arch, stem, fut, profile, case, forms):
    cus = _cus()
    assert not TW.premises(case, cus)[1], TW.premises(case, cus)[1]
    B, H, W = TW.CASES[case](cus)
    sd, x, f, o64, e_ref = TW.forward_reference(stem, profile, case, cus)
    bad = []
    for family, opts in forms:
        tag = f"{stem} {profile} {TW.SEED} {B}x{H}x{W} {opts}"
        big = _forward_parts(arch, fut, H, W, sd, x, f, opts, [(0, B)])
        ref = _forward_parts(arch, fut, H, W, sd, x, f, opts, TW.chunks(case, WALK_OF[family], cus))
        _same_as_chunks(bad, WALK_OF[family], case, tag, big, ref)
        _against_f64(bad, family, tag, big, o64, e_ref)
    assert not bad, bad


@pytest.mark.parametrize("profile,case", TW.UNET_CASES)
@pytest.mark.parametrize("arch,stem,fut", TW.UNETS)
def test_convunet_forward_many_tiles_per_workgroup(arch, stem, fut, profile, case):
    """rvdd_unet_forward of the convunets on the split-f16, the direct f32 and the Winograd f32 kernel (and the feature-recurrent
    ones with the two convs of the first layer, and with the composed layer's 16-channel bank): bit for bit the chunked runs,
    finite, within R * e_ref of the f64 oracle, with the case's premises holding for this device's CU count."""
    feat = arch.endswith("+feat")
    forms = [("composed first layer" if feat else "split-f16 conv", {"conv_kernel": 0}),
             ("direct f32", {"conv_kernel": 1}), ("Winograd f32", {"conv_kernel": 2})]
    if feat:
        forms.append(("split-f16 conv", {"conv_kernel": 0, "fuse_pre": 0}))
        if not fut:                                   # "pre5_cin8" is inert with a future frame (9 channels)
            forms.append(("composed first layer", {"conv_kernel": 0, "pre5_cin8": 0}))
    _check_forms(arch, stem, fut, profile, case, forms)


@pytest.mark.parametrize("profile,case", TW.NEXT_CASES)
@pytest.mark.parametrize("arch,stem,fut", TW.NEXTS)
def test_convnext_forward_many_tiles_per_workgroup(arch, stem, fut, profile, case):
    """The four forms of the ConvNeXt nets: the pipelined split-f16 block with the projection halves in the epilogues and with the
    projection kernel, the phased split-f16 block, the f32-MFMA block.  Case A under `pow2` (split and f32 blocks in one
    handle), case B under `he`."""
    _check_forms(arch, stem, fut, profile, case, [
        ("ConvBlock split", {"next_split": 1, "next_pipe": 1, "next_projfuse": 1}),
        ("ConvBlock split", {"next_split": 1, "next_pipe": 1, "next_projfuse": 0}),
        ("ConvBlock split", {"next_split": 1, "next_pipe": 0}), ("ConvBlock f32", {"next_split": 0})])


@pytest.mark.parametrize("case", ["A", "B"])
def test_mixed_magnitudes_across_one_walk(case):
    """Sequence b times 2^13 where b % 5 == 1 and times 2^-10 where b % 5 == 3, both outside the [2^-6, 2^12) that amax_shift leaves
    alone: consecutive tiles of a workgroup belong to sequences of three block-floating-point scales, and the next tile's scale
    is the word the tile loop carries.  Finite, and bit for bit the chunked runs of the same scaled sequences (no f64 bar: the
    whole-batch norm would see the bright sequences only)."""
    arch, stem, fut = TW.UNETS[2]
    cus = _cus()
    B, H, W = TW.CASES[case](cus)
    sd, x, f, _, _ = TW.forward_reference(stem, "he", case, cus)
    mag = torch.tensor([2.0 ** 13 if b % 5 == 1 else 2.0 ** -10 if b % 5 == 3 else 1.0 for b in range(B)])[:, None, None, None]
    x, f = x * mag, f * mag
    walks = TW.walk("split-f16", TW.level_tiles("split-f16", B, H, W)[0], cus)
    per = TW.level_tiles("split-f16", 1, H, W)[0]
    most = min(3, max(len(w) for w in walks))       # case B: two tiles per workgroup, so two scales
    assert most >= 2 and any(len(set(float(mag[t // per]) for t in w)) == most for w in walks), "no workgroup walks sequences of different scales"
    opts = {"conv_kernel": 0}
    big = _forward_parts(arch, fut, H, W, sd, x, f, opts, [(0, B)])
    ref = _forward_parts(arch, fut, H, W, sd, x, f, opts, TW.chunks(case, "split-f16", cus))
    assert all(torch.isfinite(g).all() for g in big)
    bad = []
    _same_as_chunks(bad, "split-f16", case, "mixed magnitudes", big, ref)
    assert not bad, bad


def _step_inputs(B, H, W, T, seed):
    """raw [T,B,4,h,w] and flows [T,B,2,h,w] of B different sequences from five draws of synth.make_sequence: slot b takes draw
    b % 5 with noise of its own on the frames; its flows are the draw's times a factor of its own on the even slots and
    `wild` on the odd ones"""
    from rvdd_release_amd import synth
    gen = torch.Generator().manual_seed(seed)
    draws = [synth.make_sequence(T, H, W, iso=3200, seed=seed + k) for k in range(5)]
    pick = lambda key: torch.stack([getattr(draws[b % 5], key) for b in range(B)], 1)
    raw = (pick("raw") + 0.05 * torch.randn(T, B, 4, H // 2, W // 2, generator=gen)).clamp(-1.0, 1.0)
    gain = 0.5 + torch.rand(B, generator=gen)[None, :, None, None, None]
    fp, fn = pick("flow_prev") * gain, pick("flow_next") * gain
    fp[:, 1::2], fn[:, 1::2] = wild(fp[:, 1::2], seed + 5), wild(fn[:, 1::2], seed + 6)
    return raw, fp, fn


@pytest.mark.parametrize("arch,stem,fut", [TW.UNETS[2], TW.UNETS[3], TW.NEXTS[1]])
def test_steps_of_a_handle_with_more_than_64_sequences(arch, stem, fut):
    """Two frame-steps (the first-step latch, then the recurrence) of case A's batch, `he` weights, wild flows on the odd sequences:
    both outputs and the features equal, bit for bit, the same steps on handles of the chunk sizes.  The big handle takes
    netin_bound_kernel plus the tiled network input where the chunks take the one-kernel pre-stage, the feature warp runs over
    259 sequences, slots_below runs its n >= 64 branch and the second step follows one that spent every mark.  Between the two
    steps the calls that need batch <= 64 refuse the handle and leave it as it was.  (No f64 here: the chunked regime is held
    to f64 by test_steps_no_warp_vs_f64_oracle and test_gpu_hard_flows.py at (3, 18, 34).)"""
    from rvdd_release_amd.runtime import RvddRuntime
    cus = _cus()
    B, H, W = TW.case_a(cus)
    assert B > 64
    sd = RW.random_state_dict(stem, 5, "he")
    raw, fp, fn = _step_inputs(B, H, W, 3 + fut, 4100)
    ref = [_device_steps(arch, fut, (c, H, W), sd, raw[:, b:b + c], {}, fp[:, b:b + c], fn[:, b:b + c])
           for b, c in TW.chunks("A", "convblock" if arch.startswith("next") else "split-f16", cus)]
    ref = [torch.cat(parts) for parts in zip(*ref)]
    rt = RvddRuntime(arch, fut, B, H, W, 0)
    try:
        rt.load_state_dict(sd)
        rawd, fpd, fnd = raw.cuda(), fp.cuda(), fn.cuda() if fut else None
        step = lambda t: rt.step(rawd[0] if t == 1 else None, rawd[t], rawd[t + 1] if fut else None, fpd[t],
                                 fnd[t] if fut else None).cpu()
        got = [step(1)]
        for refused in (lambda: rt.reset([1]), lambda: rt.move_slots([(0, 1)]),
                        lambda: rt.step(None, rawd[2, :3], rawd[3, :3] if fut else None, fpd[2, :3], fnd[2, :3] if fut else None, live=3)):
            with pytest.raises(RuntimeError, match=rf"failed \({ERR_ARG}\): .*batch <= 64 \(batch is {B}\)"):
                refused()
        got.append(step(2))
        got.append(rt.get_state()[1].cpu())
    finally:
        rt.close()
    bad = []
    for name, g, w in zip(("out 1", "out 2", "features"), got, ref):
        assert torch.isfinite(g).all(), name
        if not torch.equal(g, w):
            bad.append(_first_difference(WALK_OF["ConvBlock split" if arch.startswith("next") else "composed first layer"], "A", name, g, w))
    assert not bad, bad
