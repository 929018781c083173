"""Per-sequence reset (rvdd_reset_slots) and packed validation on the device: videos of different lengths sharing a
batch, each slot restarted when its video ends, give every frame bit for bit as the same video alone on a batch-1
handle; the batched losses equal the per-slot ones; validate.py's packed mode writes what the serial mode writes."""
import math
import os

import pytest
import torch

from conftest import WEIGHTS, load_weights
from formats_support import write_dataset
from gpu_support import frames_of as _frames, make_runtime, parity_psnr, run_alone, synth_videos as _videos

pytestmark = pytest.mark.gpu

LENGTHS = [7, 3, 5, 9, 4]     # frames per video: 6, 2, 4, 8, 3 outputs

# id -> (arch, weights stem, future, options)
CASES = {
    "convunet": ("convunet", "recurrent-convunet-iso3200", 0, {}),
    "convunet-k2": ("convunet", "recurrent-convunet-iso3200", 0, {"conv_kernel": 2}),
    "feat": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {}),
    "feat-k2": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"conv_kernel": 2}),
    "feat-future": ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, {}),
    "feat-future-k2": ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, {"conv_kernel": 2}),
    "next-feat-future": ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, {}),
    "feat-no_warp": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"no_warp": 1}),
    "convunet-warp_raw": ("convunet", "recurrent-convunet-iso3200", 0, {"warp_raw": 1}),
    "feat-prev_noisy": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"prev_noisy_frame": 1}),
    "feat-block_fp0": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"block_fp": 0}),
}


def run_packed(rt, seqs, future):
    """The videos through rt's B slots in order, a slot refilled when its video ends (reset_slots); tail slots repeat
    their last frame.  -> per video, its output frames, and the step at which each video started."""
    B = rt.B
    queue = list(range(len(seqs)))
    cur, pos, last = [None] * B, [0] * B, [None] * B
    outs = [[] for _ in seqs]
    started = {}
    step = 0
    rt.reset()
    while True:
        first = [False] * B
        for b in range(B):
            if (cur[b] is None or pos[b] >= _frames(seqs[cur[b]], future)) and queue:
                cur[b], pos[b] = queue.pop(0), 1
                first[b] = True
                started[cur[b]] = step
        live = [cur[b] is not None and pos[b] < _frames(seqs[cur[b]], future) for b in range(B)]
        if not any(live):
            break
        frame = []
        for b in range(B):
            v = cur[b] if cur[b] is not None else 0
            t = pos[b] if live[b] else last[b]
            frame.append((v, t))
            last[b] = t
        st = lambda f: torch.stack([f(seqs[v], t) for v, t in frame])
        if step and any(first):
            rt.reset(slots=first)
        out = rt.step(st(lambda s, t: s.raw[t - 1]), st(lambda s, t: s.raw[t]),
                      st(lambda s, t: s.raw[t + 1]) if future else None, st(lambda s, t: s.flow_prev[t]),
                      st(lambda s, t: s.flow_next[t]) if future else None)
        for b in range(B):
            if live[b]:
                outs[cur[b]].append(out[b].clone())
                pos[b] += 1
        step += 1
    return [torch.stack(o) for o in outs], started


@pytest.mark.parametrize("case", sorted(CASES))
def test_staggered_resets_exact(case):
    arch, stem, future, opts = CASES[case]
    H, W = 96, 128
    sd = load_weights(stem)
    seqs = _videos(LENGTHS, H, W, future)
    want = run_alone(arch, sd, future, seqs, H, W, opts)
    for B in (2, 3):
        rt = make_runtime(arch, sd, future, B, H, W, **opts)
        got, _ = run_packed(rt, seqs, future)
        rt.close()
        for v in range(len(seqs)):
            assert got[v].shape == want[v].shape
            for t in range(want[v].shape[0]):
                assert torch.equal(got[v][t], want[v][t]), (case, B, v, t, float((got[v][t] - want[v][t]).abs().max()))


def test_staggered_resets_exact_720p_b8():
    """At 1280x720 netin_small does not apply and the split conv picks other forms: still bit for bit."""
    H, W = 720, 1280
    sd = load_weights("recurrent-convunet+feat-iso3200")
    lengths = [3, 5, 2, 4, 3, 2, 6, 3, 4, 2, 3]
    seqs = _videos(lengths, H, W, 0, seed0=700)
    want = run_alone("convunet+feat", sd, 0, seqs, H, W, {})
    rt = make_runtime("convunet+feat", sd, 0, 8, H, W)
    got, started = run_packed(rt, seqs, 0)
    rt.close()
    assert any(s > 0 for s in started.values())
    for v in range(len(seqs)):
        for t in range(want[v].shape[0]):
            assert torch.equal(got[v][t], want[v][t]), (v, t, float((got[v][t] - want[v][t]).abs().max()))


def _steps(rt, seqs, ts, resets=None, raw_prev=True):
    """rt (B = len(seqs)) through frames ts; resets[k] = reset_slots argument before step k (None: nothing)."""
    outs = []
    for k, t in enumerate(ts):
        if resets and resets.get(k) is not None:
            r = resets[k]
            for m in (r if isinstance(r, tuple) else (r,)):
                rt.reset(slots=m)
        st = lambda f: torch.stack([f(s) for s in seqs])
        outs.append(rt.step(st(lambda s: s.raw[t - 1]), st(lambda s: s.raw[t]), None, st(lambda s: s.flow_prev[t]),
                            None).clone())
    return outs


def test_mask_semantics():
    H, W = 96, 128
    sd = load_weights("recurrent-convunet+feat-iso3200")
    seqs = _videos([8, 8, 8], H, W, 0, seed0=900)
    ts = [1, 2, 3, 4, 5, 6]

    def fresh():
        rt = make_runtime("convunet+feat", sd, 0, 3, H, W)
        rt.reset()
        return rt

    base_rt = fresh()
    base = _steps(base_rt, seqs, ts)
    base_state = base_rt.get_state()
    # an all-ones mask is rvdd_reset; an empty mask changes nothing
    rt = fresh()
    ones = _steps(rt, seqs, ts, {3: [True, True, True]})
    rt2 = fresh()
    alls = _steps(rt2, seqs, ts[:3])
    rt2.reset()
    alls += _steps(rt2, seqs, ts[3:])
    for a, b in zip(ones, alls):
        assert torch.equal(a, b)
    rt = fresh()
    empty = _steps(rt, seqs, ts, {2: [False, False, False], 4: []})
    for a, b in zip(empty, base):
        assert torch.equal(a, b)
    # two calls before one step OR together
    rt = fresh()
    two = _steps(rt, seqs, ts, {3: ([0], [2])})
    rt = fresh()
    one = _steps(rt, seqs, ts, {3: [0, 2]})
    for a, b in zip(two, one):
        assert torch.equal(a, b)
    # the untouched slot carries on bit for bit, its state too
    for k in range(len(ts)):
        assert torch.equal(one[k][1], base[k][1])
    st = rt.get_state()
    assert torch.equal(st[0][1], base_state[0][1]) and torch.equal(st[1][1], base_state[1][1])
    assert not torch.equal(one[3][0], base[3][0])        # the reset slots did restart
    # a pending slot without raw_prev: RVDD_ERR_ARG, and it stays pending
    rt = fresh()
    _steps(rt, seqs, ts[:3])
    rt.reset(slots=[1])
    st = lambda f: torch.stack([f(s) for s in seqs])
    with pytest.raises(RuntimeError, match="raw_prev is required"):
        rt.step(None, st(lambda s: s.raw[4]), None, st(lambda s: s.flow_prev[4]), None)
    late = _steps(rt, seqs, ts[3:])
    rt = fresh()
    ref = _steps(rt, seqs, ts, {3: [1]})
    for a, b in zip(late, ref[3:]):
        assert torch.equal(a, b)
    for r in (base_rt, rt2):
        r.close()


@pytest.mark.parametrize("size", [(256, 256), (720, 1280)], ids=["256", "720p"])
def test_psnr_l1_batch_equals_single(size):
    H, W = size
    B = 4
    rt = make_runtime("convunet", load_weights("recurrent-convunet-iso3200"), 0, 1, 64, 64)
    g = torch.Generator(device="cuda").manual_seed(5)
    den = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
    gt = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
    got = rt.psnr_l1_batch(den, gt)
    want = [rt.psnr_l1(den[b:b + 1], gt[b:b + 1]) for b in range(B)]
    assert got == want
    # both calls share one path in the library: anchor them to the CPU.  d in float32 as the kernel forms it, both sums in float64;
    # the library accumulates in double and rounds its two results to float32 once (6e-8 relative), so 1e-6 has an order of
    # magnitude to spare and still catches a wrong count, slice offset or partition
    d = (den - gt).cpu().reshape(B, -1)
    n = d.shape[1]
    for b in range(B):
        d64 = d[b].double()
        ref = (100.0 * float(d64.abs().sum()) / n, 10.0 * math.log10(4.0 / (float((d64 * d64).sum()) / n)))
        for g, r in zip(got[b], ref):
            assert abs(g - r) <= 1e-6 * abs(r), (b, got[b], ref)
    assert rt.psnr_l1_batch(den[:0], gt[:0]) == []
    rt.close()


def test_oracle_anchor_after_mid_batch_reset():
    """A video that starts in a slot mid-batch matches the CPU oracle on the frames right after its reset."""
    import rvdd_oracle as O
    H, W = 64, 96
    stem = "recurrent-convunet+feat-iso3200"
    sd = load_weights(stem)
    seqs = _videos([3, 6, 5], H, W, 0, seed0=1200)
    rt = make_runtime("convunet+feat", sd, 0, 2, H, W)
    got, started = run_packed(rt, seqs, 0)
    rt.close()
    assert started[2] > 0
    s = seqs[2]
    want = O.RecurrentOracle(sd, future=0).run_sequence(s.raw.cpu(), s.flow_prev.cpu())
    for t in range(3):
        g, w = got[2][t].cpu(), want[t]
        assert (g - w).abs().max() < 1e-4 and parity_psnr(g, w) > 120.0, (t, float((g - w).abs().max()))


@pytest.mark.parametrize("online", [False, True], ids=["dataset_flow", "online_flow"])
def test_packed_validation_on_disk(tmp_path, online):
    from rvdd_release_amd import synth, validate
    seqs = [synth.make_sequence(T, 64, 96, iso=3200, seed=80 + v) for v, T in enumerate([4, 2, 5, 3, 3])]
    root = tmp_path / "validation"
    write_dataset(str(root), seqs, iso=3200)
    name = "recurrent-convunet+feat-iso3200"

    def run(B):
        ck = tmp_path / f"ck{B}"
        argv = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, name),
                "--val_dataroot", str(root), "--gtFolder", "gt_iso3200", "--nFolder", "noisy_iso3200",
                "--gt_linear_RGB_Folder", "gt_raw_linear_RGB_iso3200", "--suffix", "t", "--checkpoints_dir", str(ck),
                "--val_videos", "000,001,002,003,004", "--feature_rec", "--val_batch_size", str(B)]
        if online:
            argv.append("--val_flow_from_denoised")
        res = validate.main(argv)
        out = ck / "recurrent-convunet-mode=fixedfeatures+feat-warp-i3o3-t" / "val_visuals"
        files = {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read()
                 for d, _, fs in os.walk(out) for f in fs}
        return res, files

    serial, packed = run(1), run(3)
    assert packed[0] == serial[0]
    assert sorted(packed[1]) == sorted(serial[1])
    assert len([f for f in serial[1] if f.endswith(".tif")]) == 3 + 1 + 4 + 2 + 2
    for f in serial[1]:
        assert packed[1][f] == serial[1][f], f
