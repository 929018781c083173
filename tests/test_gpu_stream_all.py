"""Every frame of a video out of the stream (option "stream_all_frames", --all_frames of the denoise command line): the head
(frame 0) and the tail (the last frame, with a future frame) against the existing entry points of a batch-1 handle that never
saw the option, the head leaving no trace, short videos, slot independence, FIRST straight after a last frame, the option
switched off, and the command line on disk.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import WEIGHTS
from gpu_support import files_of, make_runtime as _runtime, same as _same
from stream_compose import CASES as STREAM_CASES
from stream_compose import FIRST, IDLE, NEXT, compose, push_alone as _stream_alone, push_schedule
from stream_compose import synth_video as _video
from stream_ref import mosaic_of, quantised_dn, to_gpu

pytestmark = pytest.mark.gpu

H, W = 64, 96
ON = {"stream_all_frames": 1}
FEAT = {0: "recurrent-convunet+feat-iso3200", 1: "recurrent-convunet+feat-future-iso12800"}


stream_all = functools.partial(_stream_alone, idle=True)       # with a future frame one IDLE behind the video: the push that gives the tail


# ---- 1. the composition ----------------------------------------------------------------------------------------------------
CASES = STREAM_CASES + [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"prev_noisy_frame": 1}),
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"stream_flow_from_denoised": 1}),
    ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, {"stream_flow_from_denoised": 1}),
]
STREAM_ONLY = ("stream_reset_each", "stream_flow_from_denoised")


@pytest.mark.parametrize("arch,stem,future,options", CASES, ids=[f"{c[1]}-{'-'.join(c[3]) or 'plain'}" for c in CASES])
def test_all_frames_is_the_composition(arch, stem, future, options):
    N = 5
    video = _video(N, H, W, seed=131 + future)
    a = _runtime(arch, stem, future, 1, H, W, **options, **ON)
    b = _runtime(arch, stem, future, 1, H, W, **{k: v for k, v in options.items() if k not in STREAM_ONLY})
    got, flags = stream_all(a, video, future)
    want = compose(b, video, future, all_frames=True, no_warp=bool(options.get("no_warp")), reset_each=bool(options.get("stream_reset_each")),
                   from_denoised=bool(options.get("stream_flow_from_denoised")))
    assert flags == [False] * future + [True] * N
    assert len(got) == N
    _same(got, want)
    a.set_option("tvl1_async", 0)            # the deferred check of the pushes' flow batches: nothing gave up
    if not options.get("no_warp"):
        assert not torch.equal(got[0], got[1])


# ---- 2. the head leaves no trace -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
@pytest.mark.parametrize("options", [{}, {"stream_flow_from_denoised": 1}, {"prev_noisy_frame": 1}], ids=["plain", "from_denoised", "prev_noisy"])
def test_head_leaves_no_trace(future, options):
    N = 5
    video = _video(N, H, W, seed=141 + future)
    a = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **options, **ON)
    b = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **options)
    got, _ = stream_all(a, video, future)
    off, flags = _stream_alone(b, video, future)
    assert flags == [False] * (1 + future) + [True] * (N - 1 - future)
    _same(got[1:N - future], off)            # frames 1 .. N-1-future: bit for bit the pushes without the option
    a.set_option("tvl1_async", 0)


# ---- 3. short videos ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
@pytest.mark.parametrize("N", [1, 2])
def test_short_videos(N, future):
    video = _video(N, H, W, seed=150 + 2 * N + future)
    a = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **ON)
    b = _runtime("convunet+feat", FEAT[future], future, 1, H, W)
    got, flags = stream_all(a, video, future)
    assert flags == [False] * future + [True] * N and len(got) == N
    _same(got, compose(b, video, future, all_frames=True))
    # the slot is idle afterwards (with a future frame), as after any IDLE: NEXT is refused, FIRST starts a video
    if future:
        with pytest.raises(RuntimeError, match=r"\(-2\).*slot 0.*idle"):
            a.video_push(to_gpu(video[:1]), [NEXT], 12, "mosaic")
    again, _ = stream_all(a, video, future)
    _same(again, got)
    a.set_option("tvl1_async", 0)


# ---- 4. slots are independent ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
def test_slots_are_independent(future):
    from rvdd_release_amd.denoise import deal_slots
    B = 3
    lengths = (6, 1, 7, 2, 4)
    videos = [_video(n, H, W, seed=160 + v) for v, n in enumerate(lengths)]
    rt = _runtime("convunet+feat", FEAT[future], future, B, H, W, **ON)
    steps = deal_slots(lengths, B, tail=future)
    pushed = push_schedule(rt, videos, steps)
    got = pushed.by_video
    for step, valid in zip(steps, pushed.flags):
        for b, (c, v, k) in enumerate(step):
            assert valid[b] == (v >= 0 and k >= future), (step, b)
    rt.set_option("tvl1_async", 0)
    # what the dealing is meant to exercise, said of the steps themselves
    kinds = [{"head" if k == future else "tail" if c == IDLE else "mid" for c, v, k in s if v >= 0 and k >= future} for s in steps]
    assert any(len(k) >= 2 and "head" in k for k in kinds)
    if future:
        assert any(k == {"head", "tail", "mid"} for k in kinds)
        assert any(s0[b][0] == IDLE and s0[b][1] >= 0 and s1[b][0] == FIRST for s0, s1 in zip(steps, steps[1:]) for b in range(B))
    alone = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **ON)
    for v, n in enumerate(lengths):
        want, _ = stream_all(alone, videos[v], future)
        assert len(want) == n
        _same(got[v], want, v)
    alone.set_option("tvl1_async", 0)


# ---- 5. FIRST straight after the last frame --------------------------------------------------------------------------------
def test_first_straight_after_the_last_frame_drops_the_tail():
    future = 1
    va, vb = _video(4, H, W, seed=171), _video(3, H, W, seed=172)
    rt = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **ON)
    got_a, flags_a = stream_all(rt, va, future, idle=False)
    got_b, flags_b = stream_all(rt, vb, future)
    assert flags_a == [False, True, True, True] and flags_b == [False, True, True, True]
    rt.set_option("tvl1_async", 0)
    alone = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **ON)
    want_a, _ = stream_all(alone, va, future)
    want_b, _ = stream_all(alone, vb, future)
    assert len(got_a) == 3 and len(want_a) == 4
    _same(got_a, want_a[:3], "a")
    _same(got_b, want_b, "b")


# ---- 6. option off on a handle that had it on ------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
def test_option_off_again_is_todays_stream(future):
    N = 4
    v0, v1 = _video(3, H, W, seed=181), _video(N, H, W, seed=182 + future)
    a = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **ON)
    got0, _ = stream_all(a, v0, future)
    assert len(got0) == 3
    a.set_option("stream_all_frames", 0)
    got, flags = _stream_alone(a, v1, future)
    assert flags == [False] * (1 + future) + [True] * (N - 1 - future)
    # IDLE is an IDLE again: no output, and the slot goes on with FIRST
    _, valid = a.video_push(to_gpu(v1[:1]), [IDLE], 12, "mosaic")
    assert valid == [False]
    want, _ = _stream_alone(_runtime("convunet+feat", FEAT[future], future, 1, H, W), v1, future)
    _same(got, want)
    a.set_option("tvl1_async", 0)


def test_refused_ctl_changes_nothing_with_the_option_on():
    future, B = 1, 2
    videos = [_video(3, H, W, seed=190 + v) for v in range(B)]
    rt = _runtime("convunet+feat", FEAT[future], future, B, H, W, **ON)
    frames = lambda t: to_gpu(np.stack([videos[0][t], videos[1][t]]))
    got = {0: [], 1: []}

    def push(t, ctl):
        out, valid = rt.video_push(frames(t), ctl, 12, "mosaic")
        for b in range(B):
            if valid[b]:
                got[b].append(out[b:b + 1].clone())
        return valid

    assert push(0, [FIRST, FIRST]) == [False, False]
    assert push(1, [NEXT, NEXT]) == [True, True]
    for bad in ([IDLE, 3], [7, IDLE]):                                   # slot 0 / 1 would be a tail: it is not taken
        with pytest.raises(RuntimeError, match=r"\(-1\).*ctl"):
            push(2, bad)
    assert push(2, [NEXT, IDLE]) == [True, True]                         # slot 1: a video of two frames, its tail
    with pytest.raises(RuntimeError, match=r"\(-2\).*slot 1.*idle"):
        push(2, [IDLE, NEXT])                                            # slot 0's tail is not taken either
    assert push(2, [IDLE, IDLE]) == [True, False]
    rt.set_option("tvl1_async", 0)
    alone = _runtime("convunet+feat", FEAT[future], future, 1, H, W, **ON)
    _same(got[0], stream_all(alone, videos[0], future)[0], 0)
    _same(got[1], stream_all(alone, videos[1][:2], future)[0], 1)


# ---- 7. on disk ------------------------------------------------------------------------------------------------------------
def _write_mosaics(root, folder, cells_per_video):
    from rvdd_release_amd import tiffio
    for v, cells in enumerate(cells_per_video):
        d = os.path.join(root, folder, "%03d" % v)
        os.makedirs(d)
        for t in range(cells.shape[0]):
            tiffio.write(os.path.join(d, "%08d.tif" % (3 * t)), mosaic_of(cells[t:t + 1])[0].astype(np.uint16))


@pytest.mark.parametrize("future", [0, 1])
def test_denoise_all_frames_on_disk(tmp_path, future):
    from rvdd_release_amd import denoise, synth
    iso = 12800 if future else 3200
    lengths = (4, 1, 3)
    cells = [quantised_dn(synth.make_sequence(n, H, W, iso=iso, seed=200 + v).raw) for v, n in enumerate(lengths)]
    root = str(tmp_path / "data")
    _write_mosaics(root, "noisy", cells)
    every = sorted("%03d/%08d" % (v, 3 * t) for v, n in enumerate(lengths) for t in range(n))
    inner = sorted("%03d/%08d" % (v, 3 * t) for v, n in enumerate(lengths) for t in range(1, n - future))
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, FEAT[future]), "--feature_rec",
             "--future_patch_depth", str(future)]

    def run(name, dataroot, folder, *more):
        res = str(tmp_path / name)
        stats = denoise.main(flags + ["--dataroot", dataroot, "--nFolder", folder, "--results_dir", res] + list(more))
        return stats, files_of(res)

    stats, plain = run("plain", root, "noisy", "--batch_size", "3")
    assert stats["frames"] == len(inner) and sorted(plain) == [k + "_denoised.tif" for k in inner]
    stats, one = run("all1", root, "noisy", "--batch_size", "1", "--all_frames")
    assert stats["frames"] == sum(lengths) and sorted(one) == [k + "_denoised.tif" for k in every]      # one file per input frame
    assert all(one[k] == plain[k] for k in plain), [k for k in plain if one[k] != plain[k]]              # frames 1 .. N-1-future keep their bytes
    stats, three = run("all3", root, "noisy", "--batch_size", "3", "--all_frames", "--srgb", "%d,1.3,1.9,1.5" % iso)
    assert stats["frames"] == sum(lengths)
    assert sorted(k for k in three if k.endswith("_srgb.png")) == [k + "_srgb.png" for k in every]       # --srgb follows along
    tifs = {k: b for k, b in three.items() if k.endswith(".tif")}
    assert sorted(tifs) == sorted(one) and all(tifs[k] == one[k] for k in one), [k for k in one if tifs.get(k) != one[k]]
    # sensor format out: the results tree is itself a tree denoise reads, and comes back as long as it went in
    stats, mosaic = run("mosaic16", root, "noisy", "--batch_size", "3", "--all_frames", "--out_format", "mosaic16")
    assert stats["frames"] == sum(lengths) and sorted(mosaic) == [k + ".tif" for k in every]
    stats, again = run("again", str(tmp_path), "mosaic16", "--batch_size", "3", "--all_frames", "--out_format", "mosaic16")
    assert stats["frames"] == sum(lengths) and sorted(again) == sorted(mosaic)
