"""What one forward of the net needs is a value of that forward, not state of the handle: a bare rvdd_unet_forward between
two frame-steps leaves the recurrence bit for bit as it was (its amax set, its projected-input flags and its workspace are
its own), and a step of n live slots picks its kernels by n, not by the handle's batch."""
import pytest
import torch

from conftest import load_weights
from gpu_support import launches as _launches, make_runtime, step_frames as _step, synth_videos as _videos

pytestmark = pytest.mark.gpu

H, W = 96, 128


@pytest.mark.parametrize("arch,stem,future", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1),      # the prologue's projections of input and features are live
], ids=["feat", "next-feat-future"])
def test_bare_forward_between_steps(arch, stem, future):
    B = 2
    sd = load_weights(stem)
    seqs = _videos([6] * B, H, W, future, seed0=1300)
    g = torch.Generator(device="cuda").manual_seed(17)
    xs = [(torch.rand(B, 3 * (2 + future), H, W, device="cuda", generator=g) * 2 - 1,
           torch.rand(B, 48, H, W, device="cuda", generator=g)) for _ in range(2)]
    # the forwards on a handle that never stepped
    rt = make_runtime(arch, sd, future, B, H, W)
    fwd_want = [tuple(t.clone() for t in rt.unet_forward(x, f)) for x, f in xs]
    rt.close()

    def run(forwards):
        rt = make_runtime(arch, sd, future, B, H, W)
        rt.reset()
        outs, fwd = [], []
        for t in range(1, 6):
            if forwards and t in (3, 5):
                fwd.append(tuple(o.clone() for o in rt.unet_forward(*xs[len(fwd)])))
            outs.append(_step(rt, seqs, [(v, t) for v in range(B)], future).clone())
        rt.close()
        return outs, fwd

    want, _ = run(False)
    got, fwd = run(True)
    for t, (x, y) in enumerate(zip(want, got)):
        assert torch.equal(x, y), (t + 1, float((x - y).abs().max()))
    assert len(fwd) == 2
    for k, ((o, f), (ow, fw)) in enumerate(zip(fwd, fwd_want)):
        assert torch.equal(o, ow) and torch.equal(f, fw), k


def test_live_count_selects_the_kernel():
    """conv_kernel 4 picks the f32 kernel by launch size: Winograd from 200 units of 32 x 8 pixels on.  96 x 128 is 48 units a
    sequence, so four sequences (192) run direct at full resolution and five (240) run Winograd: four live slots of a batch-5
    handle take the launches of a batch-4 handle."""
    units = ((W + 31) // 32) * ((H + 7) // 8)
    assert 4 * units < 200 <= 5 * units
    sd = load_weights("recurrent-convunet+feat-iso3200")
    seqs = _videos([4] * 5, H, W, 0, seed0=1400)
    seen = {}
    for tag, B, live in (("live4of5", 5, 4), ("full4", 4, None), ("full5", 5, None)):
        rt = make_runtime("convunet+feat", sd, 0, B, H, W, conv_kernel=4)
        rt.reset()
        outs = []
        for t in (1, 2, 3):
            if t == 3:
                rt.profile_enable(True)
            outs.append(_step(rt, seqs, [(v, t) for v in range(live or B)], 0, live=live).clone())
        seen[tag] = (_launches(rt), outs)
        rt.profile_enable(False)
        rt.close()
    live, full, five = seen["live4of5"], seen["full4"], seen["full5"]
    for t, (x, y) in enumerate(zip(live[1], full[1])):
        assert torch.equal(x, y), (t + 1, float((x - y).abs().max()))
    assert full[0] and live[0] == full[0]
    # the sizes do straddle the threshold: no Winograd launch with four sequences, some with five
    assert not any(k.startswith("wino3x3") for k in full[0])
    assert any(k.startswith("wino3x3") for k in five[0])
