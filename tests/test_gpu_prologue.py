"""The stages of a frame-step in front of the 3x3 convs, after their rewrite for speed: the border ring of the composed first
layer by runs of 16 pixels (prologue.hip pre_border_fix_kernel), the tiled network input above 1024 tiles (netin_small_kernel
without its bound) and the first step of a video without work on zero features (step.hip enqueue_step zero_feat).  All three
promise the bits of what they replace.  Needs a real MI355X: -m gpu.

tests/golden/prologue_parent_<H>x<W>.npz hold what the library of the PARENT commit of these rewrites gave for the first two
steps of a video (tools/make_golden_prologue.py wrote them, on the GPU box, with that library)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_weights

pytestmark = pytest.mark.gpu

ARCH, STEM = "convunet+feat", "recurrent-convunet+feat-iso3200"


def _parent(H, W, B):
    """-> the fixture of one size: raw [T,B,4,h,w], flow_prev [T,B,2,h,w], frames [2,B,3,H,W], den [B,3,H,W], feat [B,48,H,W].
    The inputs are synth.make_sequence's with fixed seeds; the fixture stores them too and the tests feed the stored bits,
    after checking that the regenerated ones agree to float noise."""
    from rvdd_release_amd import synth
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, f"prologue_parent_{H}x{W}.npz")).items()}
    T = g["raw"].shape[0]
    assert g["raw"].shape == (T, B, 4, H // 2, W // 2) and g["frames"].shape == (2, B, 3, H, W) and T >= 3
    seqs = [synth.make_sequence(T, H, W, iso=3200, seed=4100 + 10 * H + b) for b in range(B)]
    assert (torch.stack([s.raw for s in seqs], 1) - g["raw"]).abs().max() < 1e-5
    assert (torch.stack([s.flow_prev for s in seqs], 1) - g["flow_prev"]).abs().max() < 1e-5
    planes = g.pop("feat_planes").numpy()          # [4][n]: byte k of every float
    g["feat"] = torch.from_numpy(np.ascontiguousarray(planes.T).reshape(-1).view(np.float32).copy()).reshape(B, 48, H, W)
    return g


def _same(what, got, want):
    d = got.cpu() - want.cpu()
    print(f"[prologue] {what}: max |difference| = {float(d.abs().max()):.3e}, {int((d != 0).sum())} of {d.numel()} differ")
    assert torch.equal(got.cpu(), want.cpu()), (what, float(d.abs().max()))


@pytest.mark.parametrize("H,W,B", [(34, 50, 3), (18, 16, 1)])
def test_border_ring_by_runs_gives_the_bits_of_the_parent_commit(H, W, B):
    """convunet+feat with the composed first layer (the default), two steps, frames whose ring is no whole number of 16-pixel
    runs on any side (34x50: runs of 16, 16, 16, 2 along the rows and 16, 16 along the columns; 18x16: one run per side and
    both corners in the same run): output frames and the recurrent state are torch.equal to what the parent commit's library
    (one 64-thread block per ring pixel) gave for the same inputs."""
    from rvdd_release_amd.runtime import RvddRuntime
    g = _parent(H, W, B)
    rt = RvddRuntime(ARCH, 0, B, H, W, 0)
    rt.load_state_dict(load_weights(STEM))
    raw, flow = g["raw"].cuda(), g["flow_prev"].cuda()
    for t in (1, 2):
        _same(f"{H}x{W} B={B} frame {t}", rt.step(raw[t - 1] if t == 1 else None, raw[t], None, flow[t], None), g["frames"][t - 1])
    den, feat = rt.get_state()
    rt.close()
    _same(f"{H}x{W} B={B} previous output", den, g["den"])
    _same(f"{H}x{W} B={B} features", feat, g["feat"])


# 240x240 B=5: 1125 tiles, just past the 1024 of the one-kernel form, more workgroups than XCD bands; 250x234: partial tiles on
# both edges -- with B=2 (480 tiles) in the one-kernel form, with B=5 (1200 tiles) in the tiled form behind netin_bound_kernel
@pytest.mark.parametrize("pattern", ["gbrg", "rggb"])
@pytest.mark.parametrize("H,W,B", [(240, 240, 5), (250, 234, 2), (250, 234, 5)])
def test_tiled_network_input_equals_three_kernels(H, W, B, pattern):
    """The network input of a frame-step without a future frame with the green plane in LDS (netin_small_kernel, option
    small_prestage 1, the default) against ha_green_kernel + netin_kernel (small_prestage 0): frames over three steps and the
    recurrent state are torch.equal -- on both sides of the tile limit above which the bound and the housekeeping stay in
    netin_bound_kernel, with flows that point outside the frame along one edge."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import BAYER_PATTERNS, RvddRuntime
    sd = load_weights(STEM)
    seqs = [synth.make_sequence(4, H, W, iso=3200, seed=4300 + b, device="cuda", pattern=pattern) for b in range(B)]
    st = lambda f: torch.stack([f(s) for s in seqs], 0)
    outs = []
    for small in (1, 0):
        rt = RvddRuntime(ARCH, 0, B, H, W, 0)
        rt.set_option("small_prestage", small)
        rt.set_option("bayer_pattern", BAYER_PATTERNS.index(pattern))
        rt.load_state_dict(sd)
        o = []
        for t in range(1, 4):
            fl = st(lambda s: s.flow_prev[t]).clone()
            fl[:, :, :, -3:] += 200.0
            o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]), None, fl, None).clone())
        o.extend(x.clone() for x in rt.get_state())
        outs.append(o)
        rt.close()
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))
    assert torch.isfinite(outs[0][2]).all()


@pytest.mark.parametrize("graphs", [0, 1])
def test_first_step_without_work_on_zero_features(graphs):
    """48x64, B = 2.  A handle whose first step takes the path of a whole batch that starts a video (no memset of the features,
    no warp of them, the ReLU of the partial sums in place of the second pass of EncoderConvs[0][0]) against
      * the parent commit's library: frames of steps 1 and 2 and the state after them;
      * the launches that path replaced, run by THIS library for the same inputs: a handle that is in the middle of another
        video marks ONE slot (rvdd_reset_slots) and steps -- the partial path zeroes that slot's features, warps them and runs
        the second pass over them.  A sequence's results do not depend on its neighbours in the batch, so slot k of that handle
        equals slot k of the first one: frames of three steps, previous output and features, for k = 0 and k = 1;
      * itself again after rvdd_reset, three times: with the `graphs` option later passes capture and replay first steps and
        later steps -- a first step's graph is never a later step's and the reverse (they differ in launches);
      * a fresh handle given its state with rvdd_set_state (frame 4)."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    H, W, B = 48, 64, 2
    g = _parent(H, W, B)
    sd = load_weights(STEM)
    raw, flow = g["raw"].cuda(), g["flow_prev"].cuda()           # five frames: steps 1 .. 4

    def make():
        rt = RvddRuntime(ARCH, 0, B, H, W, 0)
        rt.set_option("graphs", graphs)
        rt.load_state_dict(sd)
        return rt

    def video(rt, steps, out):
        return [rt.step(raw[0] if t == 1 else None, raw[t], None, flow[t], None, out=out[t - 1]).clone() for t in range(1, steps + 1)]

    first = make()
    bufs = [torch.empty(B, 3, H, W, device="cuda") for _ in range(4)]      # the same output buffers every pass: the same graph keys
    got = video(first, 2, bufs)
    for t in (1, 2):
        _same(f"graphs={graphs} frame {t} against the parent's", got[t - 1], g["frames"][t - 1])
    den2, feat2 = first.get_state()
    _same(f"graphs={graphs} previous output after step 2 against the parent's", den2, g["den"])
    _same(f"graphs={graphs} features after step 2 against the parent's", feat2, g["feat"])
    got.append(first.step(None, raw[3], None, flow[3], None, out=bufs[2]).clone())
    den3, feat3 = (x.clone() for x in first.get_state())

    # the old launches, slot by slot
    other = [synth.make_sequence(2, H, W, iso=3200, seed=4900 + b, device="cuda") for b in range(B)]
    for k in range(B):
        rt = make()
        rt.step(torch.stack([s.raw[0] for s in other], 0), torch.stack([s.raw[1] for s in other], 0), None,
                torch.stack([s.flow_prev[1] for s in other], 0), None)
        rt.reset(slots=[k])
        part = [rt.step(raw[0] if t == 1 else None, raw[t], None, flow[t], None).clone() for t in (1, 2, 3)]
        pden, pfeat = rt.get_state()
        for t in (1, 2, 3):
            _same(f"graphs={graphs} slot {k} frame {t} against the partial path", got[t - 1][k], part[t - 1][k])
        _same(f"graphs={graphs} slot {k} previous output against the partial path", den3[k], pden[k])
        _same(f"graphs={graphs} slot {k} features against the partial path", feat3[k], pfeat[k])
        rt.close()

    # the same video again on the same handle, three times.  A graph's key carries the step counter modulo 6: with three steps
    # a pass, pass 2 captures a first step at counter 3 and pass 4 replays it; pass 3 replays the later steps pass 1 captured
    for rep in (2, 3, 4):
        first.reset()
        again = video(first, 3, bufs)
        for t in (1, 2, 3):
            _same(f"graphs={graphs} pass {rep} frame {t}", again[t - 1], got[t - 1])
    got.append(first.step(None, raw[4], None, flow[4], None, out=bufs[3]).clone())
    first.close()

    # the state handed to a fresh handle
    rt = make()
    rt.set_state(den3, feat3)
    _same(f"graphs={graphs} frame 4 after rvdd_set_state", rt.step(None, raw[4], None, flow[4], None), got[3])
    rt.close()
