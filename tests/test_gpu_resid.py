"""Residual statistics on the device: rvdd_resid_stats against its NumPy restatement (tests/resid_ref.py) word for word -- both kernel
forms, the four patterns, four bit depths, accumulators that do not start at zero, a batch against its frames, a flat frame, frames
that take more than one walk of the workgroups --, the argument errors, and the stage inside rvdd_video_push (rvdd_set_resid /
rvdd_resid_read) against the same schedule made by hand from the stand-alone entry points of a batch-1 handle."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import dpc_ref
import match_ref
import resid_ref as R
from gpu_support import ops_rt as _rt, same as _same, upload as _up
from stream_compose import push_schedule, small_runtime as _runtime, small_videos as _videos, two_slot_schedule
from stream_ref import to_gpu

pytestmark = pytest.mark.gpu


def _start(n, seed):
    """accumulators that do not start at zero: any 64-bit words, some of them close to the wrap"""
    rng = np.random.default_rng(seed)
    w = rng.integers(-2 ** 40, 2 ** 40, size=(n, 6, 64), dtype=np.int64)
    w[:, :, 5] = -3                                          # as unsigned: three below 2^64
    return w


def _as_acc(words):
    """int64 [n,6,64] -> {field: [n,64]} in the fields' own types"""
    return {name: (words[:, k] if name in R.SIGNED else words[:, k].view(np.uint64)).copy() for k, name in enumerate(R.FIELDS)}


def _check(got, want, what):
    from rvdd_release_amd.runtime import resid_acc_arrays
    got = resid_acc_arrays(got)
    for name in R.FIELDS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), \
            (what, name, np.argwhere(got[name] != want[name])[:4].tolist())


def _run(rt, packed, rgb, pattern, bits, start, offset=False):
    acc = _up(start.reshape(start.shape[0], 384), 8 if offset else False)
    got = rt.resid_stats(_up(packed, offset), _up(rgb, offset), bits, R.PATTERNS[pattern], acc=acc)
    assert got is acc
    torch.cuda.synchronize()
    return got


# ---- 1. the kernel is the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kernel_is_the_restatement(shape):
    rt = _rt()
    n, hh, ww = shape
    for bits in R.BIT_DEPTHS:
        for pattern in range(4):
            packed, rgb, classes = R.make_case(n, hh, ww, bits, pattern, seed=100 * bits + pattern)
            assert {"clamped", "negative", "edge_pair"} <= classes
            start = _start(n, bits + pattern)
            want = R.resid_ref(packed, rgb, pattern, bits, acc=_as_acc(start))
            _check(_run(rt, packed, rgb, pattern, bits, start), want, (shape, bits, pattern))
            if shape == (1, 16, 24):
                # every tensor 4 bytes off a 16-byte boundary (the accumulator 8: its words are 64-bit): the one-cell form on a wide shape
                _check(_run(rt, packed, rgb, pattern, bits, start, offset=True), want, (shape, bits, pattern, "offset"))
    # a new accumulator starts at zero, and a second call adds to it
    packed, rgb, _ = R.make_case(n, hh, ww, 12, 0, seed=1)
    once = R.resid_ref(packed, rgb, 0, 12)
    acc = rt.resid_stats(torch.from_numpy(packed).cuda(), torch.from_numpy(rgb).cuda(), 12, "gbrg")
    _check(acc, once, (shape, "new"))
    assert rt.resid_stats(torch.from_numpy(packed).cuda(), torch.from_numpy(rgb).cuda(), 12, "gbrg", acc=acc) is acc
    _check(acc, R.add(once, once), (shape, "twice"))


@pytest.mark.parametrize("shape", [(1, 260, 512), (1, 130, 257)], ids=["wide", "one-cell"])
def test_frames_of_more_than_one_walk(shape):
    """128 workgroups of 256 threads hold 32768 items: these frames have a few hundred more (of four cells, of one cell), so some waves
    walk twice and the last one has lanes outside the frame"""
    n, hh, ww = shape
    assert hh * ww // (4 if ww % 4 == 0 else 1) > 128 * 256
    packed, rgb, classes = R.make_case(n, hh, ww, 12, 1, seed=77)
    assert "many_bins" in classes
    _check(_run(_rt(), packed, rgb, 1, 12, _start(n, 5)), R.resid_ref(packed, rgb, 1, 12, acc=_as_acc(_start(n, 5))), shape)


def test_a_batch_is_its_frames_and_a_flat_frame_is_exact():
    rt = _rt()
    packed, rgb, classes = R.make_case(3, 16, 20, 12, 2, seed=8)
    assert "batch" in classes
    whole = rt.resid_stats(torch.from_numpy(packed).cuda(), torch.from_numpy(rgb).cuda(), 12, "rggb")
    parts = torch.cat([rt.resid_stats(torch.from_numpy(packed[i:i + 1]).cuda(), torch.from_numpy(rgb[i:i + 1]).cuda(), 12, "rggb") for i in range(3)])
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)
    _check(whole, R.resid_ref(packed, rgb, 2, 12), "batch")
    for shape in ((2, 16, 24), (1, 18, 17)):
        packed, rgb, classes = R.make_case(*shape, 12, 0, seed=9, flat=True)
        assert "flat" in classes
        _check(_run(rt, packed, rgb, 0, 12, _start(shape[0], 1)), R.resid_ref(packed, rgb, 0, 12, acc=_as_acc(_start(shape[0], 1))), ("flat", shape))


def test_argument_errors_launch_nothing():
    rt = _rt()
    n, hh, ww = 2, 4, 8
    packed = torch.zeros(n, 4, hh, ww, device="cuda")
    rgb = torch.zeros(n, 3, 2 * hh, 2 * ww, device="cuda")
    acc = torch.full((n, 384), 7, dtype=torch.int64, device="cuda")

    def call(p=0, r=0, a=0, n_=n, hh_=hh, ww_=ww, pattern=0, bits=12):
        rc = rt.lib.rvdd_resid_stats(rt.h, packed.data_ptr() if p == 0 else p, rgb.data_ptr() if r == 0 else r, n_, hh_, ww_, pattern, bits,
                                     acc.data_ptr() if a == 0 else a, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    bad = [(dict(p=None), "packed"), (dict(r=None), "rgb"), (dict(a=None), "acc"), (dict(a=acc.data_ptr() + 4), "acc"),
           (dict(hh_=0), r"\bhh\b"), (dict(ww_=0), r"\bww\b"), (dict(hh_=-2), r"\bhh\b"), (dict(n_=-1), r"\bn\b"), (dict(pattern=-1), "pattern"),
           (dict(pattern=4), "pattern"), (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"),
           (dict(n_=2 ** 31 - 1, hh_=2 ** 10, ww_=2 ** 10), "blocks")]
    for kwargs, names in bad:
        rc, msg = call(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_resid_stats:") and re.search(names, msg), (kwargs, rc, msg)
    assert call(n_=0)[0] == 0 and call(n_=0, p=None, r=None, a=None)[0] == 0      # an empty batch is fine and needs no tensors
    torch.cuda.synchronize()
    assert (acc == 7).all()
    with pytest.raises(RuntimeError, match="resid_stats: packed is"):
        rt.resid_stats(rgb, rgb)
    with pytest.raises(RuntimeError, match="resid_stats: rgb is"):
        rt.resid_stats(packed, rgb[:, :, :-2])
    with pytest.raises(RuntimeError, match="resid_stats: acc is"):
        rt.resid_stats(packed, rgb, acc=acc[:1])
    for slot, word in ((-1, "slot"), (1, "slot")):
        assert rt.lib.rvdd_resid_read(rt.h, slot, C.byref(_host()), None) == -1 and word in rt.lib.rvdd_last_error(rt.h).decode()
    assert rt.lib.rvdd_resid_read(rt.h, 0, None, None) == -1 and "host_out" in rt.lib.rvdd_last_error(rt.h).decode()


def _host():
    from rvdd_release_amd import _lib
    return _lib.RvddResidAcc()


# ---- 2. the stage inside the stream ---------------------------------------------------------------------------------------------
def _compose(rt, video, future, all_frames, bits=12, dpc=None, match=None):
    """stream_compose.compose's sequence of stand-alone calls on a batch-1 handle, keeping what the stage measures: per output
    (the centre's packed frame as corrected and as mapped, the step's output BEFORE the way back, the output handed to the caller)"""
    N = video.shape[0]
    pg = []
    for t in range(N):
        p, g = rt.ingest_raw(to_gpu(video[t:t + 1]), bits, "mosaic")
        if dpc is not None:
            p = rt.dpc(p, dpc, bits, gray=g)
        if match is not None:
            p = rt.match_raw(p, match)
        pg.append((p, g))
    res = []
    for c in (range(N) if all_frames else range(1, N - future)):
        head, tail = c == 0, bool(future) and c == N - 1
        g = pg[c][1]
        zeros = torch.zeros(1, 2, g.shape[1], g.shape[2], device=g.device)
        fp = zeros if head else rt.tvl1flow_batch(g, pg[c - 1][1])
        fn = (zeros if tail else rt.tvl1flow_batch(g, pg[c + 1][1])) if future else None
        if c <= 1:
            rt.reset()
        out = rt.step(pg[c if head else c - 1][0], pg[c][0], (pg[c if tail else c + 1][0] if future else None), fp, fn).clone()
        res.append((pg[c][0], out, out if match is None else rt.unmatch_rgb(out, match)))
    return res


def _want(res, bits):
    """the restatement summed over the outputs of one or more videos -> {field: [1,64]}"""
    acc = R.new_acc(1)
    for packed, out, _ in res:
        acc = R.resid_ref(packed.cpu().numpy(), out.cpu().numpy(), 0, bits, acc=acc)
    return acc


def _stage_case(future, all_frames, bits=12, dpc=None, match=None, defects=False):
    videos = _videos(bits=bits, defects=defects)
    steps = two_slot_schedule(videos)
    alone = _runtime(future, 1)
    res = [_compose(alone, v, future, all_frames, bits, dpc, match) for v in videos]
    unit = 12 if match is not None else bits
    rt = _runtime(future, 2, stream_all_frames=all_frames)
    zero = R.new_acc(1)
    for name in R.FIELDS:                                     # the stage off: nothing allocated, zeros
        assert np.array_equal(rt.resid_read(0)[name], zero[name])
    rt.set_resid(True)
    if dpc is not None:
        rt.set_dpc(dpc)
    if match is not None:
        rt.set_match(match)
    seen = {}

    def after(i, out):
        if i == len(videos[0]):                               # the push on which both slots idle (with a future frame: the tails)
            seen["slot1"] = rt.resid_read(1)

    got = push_schedule(rt, videos, steps, bits, after=after)
    rt.set_option("tvl1_async", 0)
    for s, want in ((0, res[0] + res[2]), (1, res[1])):
        _same(got.by_slot[s], [w[2] for w in want], "outputs, slot %d" % s)
    # slot 1: everything its video gave, read when the video was over; since then it idled, and idling adds nothing to what the
    # read left at zero.  Slot 0: both of its videos; the pushes on which it was not ready (each video's first) added nothing.
    assert sum(len(r) for r in res) > 0 and int(_want(res[1], unit)["n"].sum()) == len(res[1]) * 4 * 16 * 16
    checks = ((seen["slot1"], _want(res[1], unit), "slot 1"), (rt.resid_read(1), zero, "slot 1, idle since the read"),
              (rt.resid_read(0), _want(res[0] + res[2], unit), "slot 0"), (rt.resid_read(0), zero, "slot 0, read twice"))
    for have, want, what in checks:
        for name in R.FIELDS:
            assert np.array_equal(have[name], want[name]), (what, name)
    # the stage only reads: the same pushes on a handle that never had it give the same outputs, bit for bit
    never = _runtime(future, 2, stream_all_frames=all_frames)
    if dpc is not None:
        never.set_dpc(dpc)
    if match is not None:
        never.set_match(match)
    plain = push_schedule(never, videos, steps, bits)
    never.set_option("tvl1_async", 0)
    assert plain.flags == got.flags
    for s in range(2):
        _same(got.by_slot[s], plain.by_slot[s], "against the stage off, slot %d" % s)
    return res


@pytest.mark.parametrize("all_frames", [0, 1])
@pytest.mark.parametrize("future", [0, 1])
def test_stage_is_the_composition(future, all_frames):
    _stage_case(future, all_frames)


def test_stage_behind_the_correction_and_the_match_measures_the_networks_domain():
    """DPC, then the map: the stage sees the corrected and mapped centre frame and the output before the way back, in 12-bit DN, the unit
    of the checkpoint's curve -- on 10-bit footage, so that the unit is not the push's"""
    from rvdd_release_amd.runtime import dpc_cfg, match_coeffs
    k = 1023.0 / 4095.0
    a, b = dpc_ref.iso_curve(3200, 10)
    cam = match_ref.camera_curve(60.0, 256)
    cfg = match_coeffs(k * cam[0], k * k * cam[1], 10, 3200)[0]
    res = _stage_case(1, 1, bits=10, dpc=dpc_cfg(4, 4, a, b), match=cfg, defects=True)
    # the unit matters: the same frames read at 10 bits give other sums
    assert not np.array_equal(_want(res[1], 10)["s2"], _want(res[1], 12)["s2"])
