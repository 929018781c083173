"""Raw video in all four Bayer patterns on the device (rvdd_set_option "bayer_pattern", rvdd_demosaic_ha_bayer,
HamiltonAdam(pattern)).  Needs a real MI355X: -m gpu.

The demosaics are bit for bit the reference's HamiltonAdam(pattern) (tests/golden/op_hamilton_adams_bayer.npz); whole
sequences match the oracle with its demosaic / re-mosaic swapped for the pattern-aware CPU restatement (tests/bayer_ref.py)
at the bars of tests/test_gpu_sequences.py; GBRG handles are untouched by the option."""
import numpy as np
import pytest
import torch

import bayer_ref as R
import rvdd_oracle as O
from conftest import GOLDEN, load_weights

pytestmark = pytest.mark.gpu


def _runtime(arch, stem, future, B, H, W, pattern, **opts):
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime(arch, future, B, H, W, 0)
    rt.load_state_dict(load_weights(stem))
    for k, v in opts.items():
        rt.set_option(k, v)
    if pattern is not None:
        rt.set_option("bayer_pattern", R.PATTERNS.index(pattern))
    return rt


def _run(rt, seqs, T, future):
    """Every output frame of B sequences in lockstep: [T-1-f, B, 3, H, W] on the host."""
    raw = torch.stack([s.raw for s in seqs], 1).cuda()
    fp = torch.stack([s.flow_prev for s in seqs], 1).cuda()
    fn = torch.stack([s.flow_next for s in seqs], 1).cuda()
    outs = []
    for t in range(1, T - future):
        outs.append(rt.step(raw[t - 1] if t == 1 else None, raw[t], raw[t + 1] if future else None, fp[t],
                            fn[t] if future else None).clone())
    return torch.stack(outs, 0).cpu()


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_demosaic_equals_the_reference_fixture(pattern):
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    from rvdd_release_amd.util._ops import ops_runtime
    g = np.load(GOLDEN + "/op_hamilton_adams_bayer.npz")
    raw, want = torch.from_numpy(g["raw"]).cuda(), torch.from_numpy(g[f"rgb_{pattern}"])
    assert torch.equal(HamiltonAdam(pattern)(raw).cpu(), want)
    rt = ops_runtime(0)
    assert torch.equal(rt.demosaic(raw, pattern=pattern).cpu(), want)       # rvdd_demosaic_ha_bayer
    if pattern == "gbrg":                                                    # rvdd_demosaic_ha is the GBRG entry point
        n, c, h, w = raw.shape
        out = torch.empty(n, 3 * c // 4, 2 * h, 2 * w, device="cuda")
        assert rt.lib.rvdd_demosaic_ha(rt.h, raw.data_ptr(), n * c // 4, h, w, out.data_ptr(), rt._stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want)


def test_pattern_arguments_are_checked():
    from rvdd_release_amd.util._ops import ops_runtime
    rt = ops_runtime(0)
    raw = torch.zeros(1, 4, 8, 8, device="cuda")
    out = torch.empty(1, 3, 16, 16, device="cuda")
    for bad in (-1, 4, 7):
        assert rt.lib.rvdd_demosaic_ha_bayer(rt.h, raw.data_ptr(), 1, 8, 8, bad, out.data_ptr(), rt._stream()) == -1
        assert rt.lib.rvdd_set_option(rt.h, b"bayer_pattern", bad) == -1
    for ok in range(4):
        assert rt.lib.rvdd_set_option(rt.h, b"bayer_pattern", ok) == 0
    assert rt.lib.rvdd_set_option(rt.h, b"bayer_pattern", 0) == 0
    with pytest.raises(ValueError):
        rt.demosaic(raw, pattern="rgbg")


@pytest.mark.parametrize("pattern", sorted(R.CROPS))
def test_device_demosaic_interior_identity(pattern):
    """A GBRG mosaic cropped by a row and / or column on each side is a mosaic of `pattern`: the device demosaic of it
    equals the device GBRG demosaic of the whole mosaic, cropped likewise, bit for bit away from the new borders
    (independent of the fixture and of the CPU restatement)."""
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    got, want = R.interior_identity(lambda x, p: HamiltonAdam(p)(x.cuda()).cpu(), pattern, torch.Generator().manual_seed(17))
    assert torch.equal(got, want), float((got - want).abs().max())


# name: (arch, weights stem, future, runtime options, oracle options)
CASES = {
    "convunet": ("convunet", "recurrent-convunet-iso3200", 0, {}, {}),
    "convunet-future": ("convunet", "recurrent-convunet-future-iso3200", 1, {}, {}),
    "convunet+feat": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {}, {}),
    "next+feat-future": ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, {}, {}),
    "warp_raw": ("convunet", "recurrent-convunet-iso3200", 0, {"warp_raw": 1}, {"warp_raw": True}),
    "warp_raw-future": ("convunet", "recurrent-convunet-future-iso3200", 1, {"warp_raw": 1}, {"warp_raw": True}),
    "prev_noisy+feat": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"prev_noisy_frame": 1}, {"prev_noisy_frame": True}),
    "no_warp": ("convunet", "recurrent-convunet-iso3200", 0, {"no_warp": 1}, {"no_warp": True}),
}


def _oracle_for(monkeypatch, pattern):
    monkeypatch.setattr(O, "hamilton_adams", lambda x: R.hamilton_adams(x, pattern))
    monkeypatch.setattr(O, "remosaick", lambda x: R.remosaick(x, pattern))


# every case in RGGB and BGGR; GRBG on the three-kernel pre-stage (netin_kernel<3>, a future frame) and on ConvNeXtUnet's
# (netin_proj_kernel<3>)
PARITY = [(c, p) for p in ("rggb", "bggr") for c in sorted(CASES)] + [("convunet-future", "grbg"), ("next+feat-future", "grbg")]


@pytest.mark.parametrize("case,pattern", PARITY)
def test_sequence_parity_vs_oracle(monkeypatch, case, pattern):
    """10 frames of a pattern-mosaicked sequence at 74x106 (raw frames 37x53: odd on both axes) against the oracle
    with the pattern's demosaic and re-mosaic: max-abs < 1e-4 on every frame, task PSNR within 0.01 dB.

    --warp_raw demosaics the bicubically warped previous OUTPUT again on every step.  The warp (rvdd_warp_bicubic, the
    kernel the step uses) and the oracle's grid_sample differ by an ulp on about a third of the samples (<= 3.6e-7), and a
    hard sign() selection of that demosaic near a tie turns this into a local jump (3.7e-4 .. 1.0e-2 at one step of ten,
    deep inside the frame, GBRG alike: profiles/bayer_warp_raw_stages.txt) that the recurrence then carries on.  There
    the oracle starts every step from the runtime's own previous output (rvdd_get_state); the pattern's own stages are
    checked bit for bit on the warped planes (device HamiltonAdam(P) == the CPU restatement), and a frame may hold such a
    flip: at most 64 of 7844 pixels above 1e-4, the mean difference at fp32 noise (< 2e-6)."""
    from rvdd_release_amd import synth
    arch, stem, fut, opts, oopts = CASES[case]
    T, H, W = 10, 74, 106
    seq = synth.make_sequence(T, H, W, seed=300 + len(case) + 10 * R.PATTERNS.index(pattern), pattern=pattern)
    rt = _runtime(arch, stem, fut, 1, H, W, pattern, **opts)
    _oracle_for(monkeypatch, pattern)
    orc = O.RecurrentOracle(load_weights(stem), future=fut, **oopts)
    synced = "warp_raw" in opts
    raw, fp, fn = seq.raw.cuda(), seq.flow_prev.cuda(), seq.flow_next.cuda()
    got, want = [], []
    for t in range(1, T - fut):
        if synced and t > 1:
            orc.lastden = rt.get_state(want_feat=False)[0].cpu()
            from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
            planes = O.warp(HamiltonAdam(pattern).remosaick(orc.lastden), seq.flow_prev[t][None])
            assert torch.equal(HamiltonAdam(pattern)(planes.cuda()).cpu(), R.hamilton_adams(planes, pattern)), t
        got.append(rt.step(raw[t - 1][None] if t == 1 else None, raw[t][None], raw[t + 1][None] if fut else None, fp[t][None],
                           fn[t][None] if fut else None)[0].cpu())
        want.append(orc.step(seq.raw[t - 1][None], seq.raw[t][None], seq.raw[t + 1][None] if fut else None, seq.flow_prev[t][None],
                             seq.flow_next[t][None] if fut else None, first=(t == 1))[0])
    rt.close()
    curve = [float((g - w).abs().max()) for g, w in zip(got, want)]
    above = [int(((g - w).abs() > 1e-4).any(0).sum()) for g, w in zip(got, want)]
    mean = [float((g - w).abs().mean()) for g, w in zip(got, want)]
    msg = (f"{case} {pattern}: max-abs per frame " + " ".join(f"{v:.1e}" for v in curve) + " | pixels above 1e-4 "
           + " ".join(map(str, above)) + " | mean " + " ".join(f"{v:.1e}" for v in mean))
    assert len(curve) >= 8, msg
    if synced:
        assert max(above) <= 64 and max(mean) < 2e-6, msg
    else:
        assert max(curve) < 1e-4, msg
    for k in (0, len(curve) - 1):
        gt = seq.gt[k + 1][None]
        assert abs(O.psnr(got[k][None], gt) - O.psnr(want[k][None], gt)) < 0.01, (k, msg)


def test_one_kernel_and_three_kernel_prestage_agree_under_a_pattern():
    """The one-kernel pre-stage (a single 256x256 sequence) and the three-kernel one (small_prestage 0) give the same bits
    under RGGB."""
    from rvdd_release_amd import synth
    T, H, W = 6, 256, 256
    seq = synth.make_sequence(T, H, W, seed=41, pattern="rggb")
    outs = []
    for small in (1, 0):
        rt = _runtime("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 1, H, W, "rggb")
        try:
            rt.set_option("small_prestage", small)
            outs.append(_run(rt, [seq], T, 0))
        finally:
            rt.set_option("small_prestage", 1)          # harmless: the option is per handle
            rt.close()
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


def test_three_kernel_prestage_720p_batch_vs_oracle(monkeypatch):
    """A 720p batch of two BGGR sequences (the three-kernel pre-stage: too many tiles for the one-kernel form) against the
    oracle with BGGR demosaics, first and second frame of each."""
    from rvdd_release_amd import synth
    T, H, W = 3, 720, 1280
    seqs = [synth.make_sequence(T, H, W, seed=51 + b, pattern="bggr") for b in range(2)]
    rt = _runtime("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 2, H, W, "bggr")
    got = _run(rt, seqs, T, 0)
    rt.close()
    _oracle_for(monkeypatch, "bggr")
    sd = load_weights("recurrent-convunet+feat-iso3200")
    for b in range(2):
        want = O.RecurrentOracle(sd).run_sequence(seqs[b].raw, seqs[b].flow_prev)
        worst = float((got[:, b] - want).abs().max())
        assert worst < 1e-4, (b, worst)


def test_reset_slots_gives_each_slot_its_batch_one_bits():
    """Packed videos under GRBG: slot 1 restarts with another video mid-run (rvdd_reset_slots); every slot's outputs are
    the bits of the same video run alone on a batch-1 handle."""
    from rvdd_release_amd import synth
    H, W = 96, 128
    A, Bv, Cv = (synth.make_sequence(7, H, W, seed=s, pattern="grbg", device="cuda") for s in (61, 62, 63))
    stem = "recurrent-convunet+feat-iso3200"
    rt = _runtime("convunet+feat", stem, 0, 2, H, W, "grbg")
    plan = [(A, k + 1, Bv if k < 3 else Cv, k + 1 if k < 3 else k - 2) for k in range(6)]
    got0, got1 = [], []
    for k, (s0, t0, s1, t1) in enumerate(plan):
        if k == 3:
            rt.reset(slots=[1])
        st = lambda f0, f1: torch.stack((f0, f1))
        out = rt.step(st(s0.raw[t0 - 1], s1.raw[t1 - 1]), st(s0.raw[t0], s1.raw[t1]), None,
                      st(s0.flow_prev[t0], s1.flow_prev[t1]), None)
        got0.append(out[0].cpu())
        got1.append(out[1].cpu())
    rt.close()
    rt1 = _runtime("convunet+feat", stem, 0, 1, H, W, "grbg")
    def alone(s, n):
        rt1.reset()
        return [rt1.step(s.raw[t - 1][None], s.raw[t][None], None, s.flow_prev[t][None], None)[0].cpu() for t in range(1, n + 1)]
    wa, wb, wc = alone(A, 6), alone(Bv, 3), alone(Cv, 3)
    rt1.close()
    for k in range(6):
        assert torch.equal(got0[k], wa[k]), k
        assert torch.equal(got1[k], (wb + wc)[k]), k


def test_gbrg_option_is_the_default_bit_for_bit():
    """A C2-shaped run (convunet+feat, 720p, two sequences): a handle that sets bayer_pattern 0 -- directly, or after a
    detour through RGGB -- gives the default handle's bits."""
    from rvdd_release_amd import synth
    T, H, W = 4, 720, 1280
    seqs = [synth.make_sequence(T, H, W, seed=71 + b) for b in range(2)]
    stem = "recurrent-convunet+feat-iso3200"
    outs = []
    for how in ("default", "explicit", "detour"):
        rt = _runtime("convunet+feat", stem, 0, 2, H, W, None)
        if how == "explicit":
            rt.set_option("bayer_pattern", 0)
        elif how == "detour":
            rt.set_option("bayer_pattern", 2)
            _run(rt, seqs, 2, 0)
            rt.set_option("bayer_pattern", 0)
            rt.reset()
        outs.append(_run(rt, seqs, T, 0))
        rt.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_end_to_end_denoising_follows_the_pattern():
    """A synthetic RGGB video denoised with bayer_pattern RGGB against the same scene mosaicked GBRG (the checkpoints'
    training pattern), and the RGGB video mistaken for GBRG: mean task PSNR over the 7 outputs of 8 frames at 128x192.

    Measured (CPU oracle, seed 11), whole frame / without an 8-pixel border: GBRG 38.34 / 38.38 dB, RGGB 36.02 / 38.25,
    RGGB run as GBRG 26.32 / 26.45.  The whole-frame gap of the right pattern sits in the outermost rows: Hamilton-Adams
    with replicate padding interpolates the colour that a border row lacks from zeroed neighbours of its sparse plane
    (GBRG: red on the top row, blue on the bottom one), which the GBRG-trained network learned to correct there and
    nowhere else.  So the bar is on the interior: within 0.5 dB of GBRG; the wrong pattern at least 6 dB below the right
    one over the whole frame."""
    from rvdd_release_amd import synth
    T, H, W, c = 8, 128, 192, 8
    stem = "recurrent-convunet+feat-iso3200"

    def mean_psnr(seq, pattern):
        rt = _runtime("convunet+feat", stem, 0, 1, H, W, pattern)
        out = _run(rt, [seq], T, 0)[:, 0]
        rt.close()
        n = out.shape[0]
        whole = sum(O.psnr(out[k][None], seq.gt[k + 1][None]) for k in range(n)) / n
        inner = sum(O.psnr(out[k][None, :, c:-c, c:-c], seq.gt[k + 1][None, :, c:-c, c:-c]) for k in range(n)) / n
        return whole, inner

    gbrg = mean_psnr(synth.make_sequence(T, H, W, seed=11), "gbrg")
    rggb_seq = synth.make_sequence(T, H, W, seed=11, pattern="rggb")
    right, wrong = mean_psnr(rggb_seq, "rggb"), mean_psnr(rggb_seq, "gbrg")
    msg = f"(whole, interior) dB: gbrg {gbrg}, rggb {right}, rggb run as gbrg {wrong}"
    assert right[1] > gbrg[1] - 0.5, msg
    assert wrong[0] < right[0] - 6.0, msg


def test_model_surface_sets_the_pattern_and_online_flow_follows_it():
    """recurrentModel with --bayer_pattern rggb (driven like validate.py:64-88, the flow towards the previous frame
    recomputed online from the previous output): the re-mosaic of that output is RGGB's (the flow is TV-L1 against
    HamiltonAdam('rggb').remosaick, not against GBRG's planes), and every output is the bits of a bare handle set to RGGB
    fed the same flows."""
    import os
    from conftest import WEIGHTS
    from rvdd_release_amd import synth, validate
    from rvdd_release_amd.models import create_model
    from rvdd_release_amd.options import make_opt
    from rvdd_release_amd.util._ops import ops_runtime
    stem = "recurrent-convunet+feat-iso3200"
    T, H, W = 5, 64, 96
    seq = synth.make_sequence(T, H, W, seed=91, pattern="rggb")
    opt = make_opt(netDenoiser="convunet-mode=fixedfeatures+feat", feature_rec=True, bayer_pattern="rggb",
                   path2epoch=os.path.join(WEIGHTS, stem), gpu_ids=[0], val_flow_from_denoised=True)
    model = create_model(opt)
    model.setup(opt)
    opt.isTrain = model.isTrain = False
    model.eval()
    rt = _runtime("convunet+feat", stem, 0, 1, H, W, "rggb")
    tv = ops_runtime(0)
    mean01 = lambda planes: ((planes + 1.0) / 2.0).mean(dim=0).contiguous()
    for t in range(1, T):
        data = {"n": torch.cat((seq.raw[t - 1], seq.raw[t]), 0)[None], "flow": seq.flow_prev[t][None, None].clone(),
                "gt": torch.cat((seq.gt[t - 1], seq.gt[t]), 0)[None], "n_path": [f"seq/{t:03d}.tif"],
                "gt_path": [f"seq/{t:03d}.tif"], "FirstOfVideo": t == 1}
        if t > 1:
            prev = model.denoised.detach().cpu()
            validate.compute_flows_from_denoised(data, model, opt)
            target = mean01(seq.raw[t].cuda())
            want = tv.tvl1flow(target, mean01(R.remosaick(prev, "rggb")[0].cuda()))
            assert torch.equal(data["flow"][0, 0].cpu(), want.cpu()), t
            assert not torch.equal(want.cpu(), tv.tvl1flow(target, mean01(R.remosaick(prev, "gbrg")[0].cuda())).cpu())
        model.set_input(data)
        model.test()
        fl = data["flow"][0, 0].cuda()[None]
        ref = rt.step(seq.raw[t - 1][None].cuda() if t == 1 else None, seq.raw[t][None].cuda(), None, fl, None)
        assert torch.equal(model.denoised.cpu(), ref.cpu()), t
    rt.close()
