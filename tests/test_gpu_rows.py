"""Row noise on the device: rvdd_rows_estimate and rvdd_rows_apply against their NumPy restatement (tests/rows_ref.py) bit for bit --
offsets, states, accumulators, packed planes and gray planes --, the argument errors, and the stage inside rvdd_video_push
(rvdd_set_rows / rvdd_rows_read) against the same schedule composed from the stand-alone entry points of a batch-1 handle."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import dpc_ref
import match_ref
import rows_ref as R
from gpu_support import bits_of, launches, ops_rt as _rt, same as _same, upload as _up
from stream_ref import to_gpu
from stream_compose import FIRST, IDLE, NEXT, compose, push_schedule, push_two_slots, small_runtime as _runtime, small_videos, two_slot_schedule

pytestmark = pytest.mark.gpu

# (n, hh, ww): every neighbour mirrored and two samples a row; the smallest batch; 128 samples, part of one workgroup; an odd width
# over several waves with frame and parity indexing; the 16-byte path with several keys per thread; ww % 4 != 0 at width; the cap
SHAPES = R.SHAPES
POISON = 7.0                                                   # a gray value no frame has: rows that must not be written keep it


def _cfg(c):
    from rvdd_release_amd.runtime import rows_cfg
    return rows_cfg(*[float(v) for v in c])


@functools.lru_cache(maxsize=None)
def _refs(shape):
    """the restatement of every input of one shape, computed once: [(name, packed, bits, cfg, estimate, gray in, packed out, gray out)]"""
    out = []
    for name, packed, bits, c in R.cases(shape):
        est = R.estimate(packed, bits, c)
        gray = R.gray_of(packed, bits)
        gray[:, ::2] = POISON
        p2, g2 = R.apply(packed, gray, est["offsets"], bits)
        out.append((name, packed, bits, c, est, gray, p2, g2))
    return out


def _acc_equal(got, want, what):
    from rvdd_release_amd.runtime import rows_acc_arrays
    got = rows_acc_arrays(got)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())


def _check_case(rt, ref, offset=False):
    name, packed, bits, c, est, gray, p2, g2 = ref
    dev = _up(packed, offset)
    offsets, state, acc = rt.rows_estimate(dev, _cfg(c), bits)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(offsets), est["offsets"].view(np.uint32)), (name, "offsets", np.argwhere(offsets.cpu().numpy() != est["offsets"])[:4].tolist())
    assert np.array_equal(state.cpu().numpy(), est["state"]), (name, "state")
    _acc_equal(acc, est["acc"], name)
    assert np.array_equal(bits_of(dev), packed.view(np.uint32)), (name, "the estimate only reads")
    g = _up(gray, offset)
    assert rt.rows_apply(dev, offsets, bits, gray=g) is dev
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), p2.view(np.uint32)), (name, "packed")
    assert np.array_equal(bits_of(g), g2.view(np.uint32)), (name, "gray")
    # without a gray plane the packed planes are the same
    dev = _up(packed, offset)
    rt.rows_apply(dev, offsets, bits)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), p2.view(np.uint32)), (name, "packed, no gray")


# ---- 1. the kernels are the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kernels_are_the_restatement(shape):
    rt = _rt()
    for ref in _refs(shape):
        _check_case(rt, ref)


def test_one_cell_form_on_a_wide_shape():
    """every tensor 4 bytes off a 16-byte boundary: the apply kernel's one-cell form at ww % 4 == 0"""
    rt = _rt()
    for ref in _refs((1, 8, 640)):
        _check_case(rt, ref, offset=True)


def test_accumulators_add_up_an_empty_batch_is_nothing_and_runs_repeat():
    from rvdd_release_amd.runtime import rows_acc_arrays
    rt = _rt()
    name, packed, bits, c, est, *_ = _refs((3, 7, 129))[0]
    dev = _up(packed)
    o1, s1, acc = rt.rows_estimate(dev, _cfg(c), bits)
    o2, s2, again = rt.rows_estimate(dev, _cfg(c), bits, acc=acc)
    torch.cuda.synchronize()
    assert again is acc and torch.equal(o1, o2) and torch.equal(s1, s2)
    _acc_equal(acc, R.add(est["acc"], est["acc"]), "twice")
    assert int(rows_acc_arrays(acc)["applied"].sum() + rows_acc_arrays(acc)["skipped"].sum()) == 2 * 3 * 2 * 7
    # n = 0: no tensors needed, nothing written
    keep = acc.clone()
    assert rt.lib.rvdd_rows_estimate(rt.h, None, 0, 7, 129, bits, C.byref(_cfg(c)), None, None, None, None) == 0
    assert rt.lib.rvdd_rows_apply(rt.h, None, None, None, 0, 7, 129, bits, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(acc, keep)


def test_argument_errors_launch_nothing():
    from rvdd_release_amd.runtime import rows_cfg
    rt = _rt()
    n, hh, ww = 2, 6, 8
    packed = torch.full((n, 4, hh, ww), 0.25, device="cuda")
    gray = torch.full((n, hh, ww), POISON, device="cuda")
    offsets = torch.full((n, 2, hh), 3.0, device="cuda")
    state = torch.full((n, 2, hh), 9, dtype=torch.uint8, device="cuda")
    acc = torch.full((n, 3), 5, dtype=torch.int64, device="cuda")
    good = dict(k_gate=3.0, noise_a=1.0, noise_b=0.0, var_floor=1.0, max_dn=8.0)

    def estimate(p=0, o=0, s=0, a=0, n_=n, hh_=hh, ww_=ww, bits=12, cfg=0, **fields):
        c = None if cfg is None else rows_cfg(**dict(good, **fields))
        rc = rt.lib.rvdd_rows_estimate(rt.h, packed.data_ptr() if p == 0 else p, n_, hh_, ww_, bits, None if c is None else C.byref(c),
                                       offsets.data_ptr() if o == 0 else o, state.data_ptr() if s == 0 else s, acc.data_ptr() if a == 0 else a, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    def apply(p=0, o=0, n_=n, hh_=hh, ww_=ww, bits=12):
        rc = rt.lib.rvdd_rows_apply(rt.h, packed.data_ptr() if p == 0 else p, gray.data_ptr(), offsets.data_ptr() if o == 0 else o, n_, hh_, ww_, bits, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    inf, nan = float("inf"), float("nan")
    bad = [(dict(cfg=None), "cfg"), (dict(p=None), "packed"), (dict(o=None), "offsets"), (dict(s=None), "state"), (dict(a=acc.data_ptr() + 4), "acc"),
           (dict(k_gate=0.0), "k_gate"), (dict(k_gate=-1.0), "k_gate"), (dict(k_gate=inf), "k_gate"), (dict(k_gate=nan), "k_gate"),
           (dict(max_dn=0.0), "max_dn"), (dict(max_dn=inf), "max_dn"), (dict(max_dn=nan), "max_dn"), (dict(noise_a=inf), "noise_a"),
           (dict(noise_b=nan), "noise_b"), (dict(var_floor=0.0), "var_floor"), (dict(var_floor=nan), "var_floor"),
           (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"), (dict(hh_=4), r"\bhh\b"), (dict(ww_=0), r"\bww\b"),
           (dict(ww_=R.MAX_WW + 1), r"\bww\b"), (dict(n_=-1), r"\bn\b"), (dict(n_=2 ** 30, hh_=2 ** 10), "blocks")]
    for kwargs, names in bad:
        rc, msg = estimate(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_rows_estimate:") and re.search(names, msg), (kwargs, rc, msg)
    for kwargs, names in [(dict(p=None), "packed"), (dict(o=None), "offsets"), (dict(bits=0), "bit_depth"), (dict(hh_=4), r"\bhh\b"),
                          (dict(ww_=0), r"\bww\b"), (dict(ww_=R.MAX_WW + 1), r"\bww\b"), (dict(n_=-1), r"\bn\b")]:
        rc, msg = apply(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_rows_apply:") and re.search(names, msg), (kwargs, rc, msg)
    assert rt.lib.rvdd_set_rows(rt.h, C.byref(rows_cfg(**dict(good, max_dn=-1.0)))) == -1 and "max_dn" in rt.lib.rvdd_last_error(rt.h).decode()
    from rvdd_release_amd import _lib
    host = _lib.RvddRowsAcc()
    for slot in (-1, 1):
        assert rt.lib.rvdd_rows_read(rt.h, slot, C.byref(host), None) == -1 and "slot" in rt.lib.rvdd_last_error(rt.h).decode()
    assert rt.lib.rvdd_rows_read(rt.h, 0, None, None) == -1 and "host_out" in rt.lib.rvdd_last_error(rt.h).decode()
    torch.cuda.synchronize()
    assert (packed == 0.25).all() and (gray == POISON).all() and (offsets == 3.0).all() and (state == 9).all() and (acc == 5).all()
    with pytest.raises(RuntimeError, match="rows_estimate: packed is"):
        rt.rows_estimate(gray, rows_cfg(**good))
    with pytest.raises(RuntimeError, match="rows_apply: offsets is"):
        rt.rows_apply(packed, offsets[:, :1])
    with pytest.raises(RuntimeError, match="rows_estimate: acc is"):
        rt.rows_estimate(packed, rows_cfg(**good), acc=acc[:1])


# ---- 2. the stage inside the stream -------------------------------------------------------------------------------------------------
def _videos(bits=12, defects=False, rows=True):
    """stream_compose.small_videos with one offset per mosaic row and frame (-40 .. 40 DN of 12 bits, scaled to `bits`)"""
    rng = np.random.default_rng(77 + bits)
    out = []
    for m in small_videos(bits=bits, defects=defects):
        if rows:
            o = np.rint(rng.uniform(-40.0, 40.0, (m.shape[0], m.shape[1], 1)) / (1 << (12 - bits))).astype(np.int64)
            m = np.clip(m.astype(np.int64) + o, 0, (1 << bits) - 1).astype(np.uint16)
        out.append(m)
    return out


def _rows_rule(bits=12, k=3.0):
    from rvdd_release_amd.runtime import rows_cfg
    a, b = dpc_ref.iso_curve(3200, bits)
    return rows_cfg(k, a, b, 1.0, ((1 << bits) - 1) / 64.0)


class _WithRows:
    """A batch-1 handle for stream_compose.compose that takes the row offsets out where the stream does: behind the ingest, or, where
    the composition corrects defects, behind rvdd_dpc.  Keeps every frame's accumulator."""

    def __init__(self, rt, cfg, bits, behind_dpc):
        self._rt, self._cfg, self._bits, self._behind_dpc = rt, cfg, bits, behind_dpc
        self.accs = []

    def __getattr__(self, name):
        return getattr(self._rt, name)

    def _rows(self, packed, gray):
        offsets, _, acc = self._rt.rows_estimate(packed, self._cfg, self._bits)
        self._rt.rows_apply(packed, offsets, self._bits, gray=gray)
        self.accs.append(acc)

    def ingest_raw(self, *args, **kwargs):
        packed, gray = self._rt.ingest_raw(*args, **kwargs)
        if not self._behind_dpc:
            self._rows(packed, gray)
        return packed, gray

    def dpc(self, packed, cfg, bit_depth=12, gray=None):
        out = self._rt.dpc(packed, cfg, bit_depth, gray=gray)
        self._rows(out, gray)
        return out


def _composed(videos, future, all_frames, bits, rule, dpc=None, match=None):
    """-> (the outputs per video, the summed accumulators per video)"""
    from rvdd_release_amd.runtime import rows_acc_arrays
    alone = _WithRows(_runtime(future, 1), rule, bits, dpc is not None)
    want, totals = [], []
    for v in videos:
        alone.accs = []
        want.append(compose(alone, v, future, all_frames=all_frames, bit_depth=bits, dpc=dpc, match=match))
        assert len(alone.accs) == len(v)
        t = R.new_acc(1)
        for acc in alone.accs:
            t = R.add(t, rows_acc_arrays(acc))
        totals.append(t)
    return want, totals


def _stage_case(future, all_frames, bits=12, dpc=None, match=None, defects=False, container=None):
    videos = _videos(bits, defects)
    rule = _rows_rule(bits)
    want, totals = _composed(videos, future, all_frames, bits, rule, dpc, match)
    rt = _runtime(future, 2, stream_all_frames=all_frames)
    zero = R.new_acc(1)
    for k in zero:                                                 # the stage off: nothing allocated, zeros
        assert np.array_equal(rt.rows_read(0)[k], zero[k])
    rt.set_rows(rule)
    if dpc is not None:
        rt.set_dpc(dpc)
    if match is not None:
        rt.set_match(match)
    seen = {}

    def after(i, out):
        if i == len(videos[0]):                                    # the push on which both slots idle: slot 1's video is over
            seen["slot1"] = rt.rows_read(1)

    got = push_schedule(rt, videos, two_slot_schedule(videos), bits, container, after=after)
    rt.set_option("tvl1_async", 0)
    _same(got.by_slot[0], want[0] + want[2], "slot 0")
    _same(got.by_slot[1], want[1], "slot 1")
    # every ingested frame is counted once, in its slot; heads and tails are copies and are not counted again
    assert int(totals[1]["applied"][0] + totals[1]["skipped"][0]) == len(videos[1]) * 2 * 16 and int(totals[1]["applied"][0]) > 0
    checks = ((seen["slot1"], totals[1], "slot 1"), (rt.rows_read(1), zero, "slot 1, idle since the read"),
              (rt.rows_read(0), R.add(totals[0], totals[2]), "slot 0"), (rt.rows_read(0), zero, "slot 0, read twice"))
    for have, wanted, what in checks:
        for k in wanted:
            assert np.array_equal(have[k], wanted[k]), (what, k, have[k], wanted[k])
    return videos, got


@pytest.mark.parametrize("all_frames", [0, 1])
@pytest.mark.parametrize("future", [0, 1])
def test_stage_is_the_composition(future, all_frames):
    videos, got = _stage_case(future, all_frames)
    # the stage matters: a handle that never had it gives other outputs
    never = push_two_slots(_runtime(future, 2, stream_all_frames=all_frames), videos)
    assert not torch.equal(never[0][0], got.by_slot[0][0])


def test_stage_between_the_correction_and_the_match():
    """defects first, then the rows in the sensor's DN with the sensor's curve, then the map onto the checkpoint's curve"""
    from rvdd_release_amd.runtime import dpc_cfg, match_coeffs
    a, b = dpc_ref.iso_curve(3200, 12)
    cfg = match_coeffs(*match_ref.camera_curve(60.0, 256), 12, 3200)[0]
    _stage_case(1, 1, dpc=dpc_cfg(4, 4, a, b), match=cfg, defects=True)


def test_stage_on_mipi_raw10_is_the_stage_on_the_unpacked_frames():
    _stage_case(1, 1, bits=10, container="mipi")


@pytest.mark.parametrize("future", [0, 1])
def test_zero_offsets_are_the_plain_stream(future):
    """constant frames: every d is 0, every offset is 0, nothing is written -- the stream of a handle that never had the stage"""
    videos = [np.full((T, 32, 32), 600 + 100 * v, np.uint16) for v, T in enumerate((5, 5, 3))]
    on = _runtime(future, 2, stream_all_frames=1)
    on.set_rows(_rows_rule())
    got = push_two_slots(on, videos)
    want = push_two_slots(_runtime(future, 2, stream_all_frames=1), videos)
    for s in range(2):
        _same(got[s], want[s], s)
    acc = on.rows_read(0)
    assert int(acc["applied"][0]) == 8 * 2 * 16 and int(acc["skipped"][0]) == 0 and int(acc["sum_q2"][0]) == 0


def test_stage_off_restores_the_launches():
    videos = _videos()
    frames = lambda t: to_gpu(np.stack([videos[0][t], videos[1][t]]))

    def counted(rt, t, ctl):
        rt.profile_enable(True)
        rt.video_push(frames(t), ctl, 12, "mosaic")
        torch.cuda.synchronize()
        seen = {k: v[0] for k, v in launches(rt).items()}
        rt.profile_enable(False)
        return seen

    rt, never = _runtime(0, 2), _runtime(0, 2)
    rt.set_rows(_rows_rule())
    ctls = ([FIRST, FIRST], [NEXT, NEXT], [NEXT, IDLE])
    plain = [counted(never, t, c) for t, c in enumerate(ctls)]
    on = [counted(rt, t, c) for t, c in enumerate(ctls)]
    for have, base in zip(on, plain):
        assert have == dict(base, rows_estimate_kernel=1, rows_apply_kernel=1), (have, base)      # two launches per run of slots
    rt.set_rows(None)
    for r in (rt, never):
        r.video_push(frames(3), [IDLE, IDLE], 12, "mosaic")
    off = [counted(rt, t, c) for t, c in enumerate(ctls)]
    assert off == [counted(never, t, c) for t, c in enumerate(ctls)] == plain and "rows_apply_kernel" not in off[1]
    rt.set_option("tvl1_async", 0)
    never.set_option("tvl1_async", 0)
