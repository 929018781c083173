"""Column fixed-pattern noise on the device: rvdd_cols_estimate and rvdd_cols_apply against their NumPy restatement (tests/cols_ref.py)
bit for bit -- offsets, states, packed planes and gray planes --, the argument errors, the stage inside rvdd_video_push (rvdd_set_cols)
against the same schedule composed from the stand-alone entry points of a batch-1 handle, and the map found by col_noise.estimate."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import cols_ref as R
import dpc_ref
import match_ref
from gpu_support import bits_of, launches, ops_rt as _rt, same as _same, upload as _up
from stream_ref import to_gpu
from stream_compose import FIRST, IDLE, NEXT, compose, push_schedule, push_two_slots, small_runtime as _runtime, small_videos, two_slot_schedule

pytestmark = pytest.mark.gpu

# (n, hh, ww): the smallest; fewer than nine columns (the double reflection); odd sizes, two frames, the one-cell apply; ww one below,
# at and one above every strip width of the estimate (32, 16, 8, 4 columns); either side of every hh at which the strip narrows, at a
# width of one strip and a column; the hh cap; a 16-byte shape for the wide apply
SHAPES = R.SHAPES
POISON = 7.0                                                   # a gray value no frame has: cells that must not be written keep it
f32 = np.float32


def _cfg(c):
    from rvdd_release_amd.runtime import cols_cfg
    return cols_cfg(*[float(v) for v in c])


@functools.lru_cache(maxsize=None)
def _refs(shape):
    """the restatement of every input of one shape, computed once: [(name, packed, bits, cfg, estimate, map, gray in, packed out, gray
    out)].  The map is the fit of the shape's own frames with k_sig = 0 (every applied column) and every fifth column put to zero."""
    out = []
    for name, packed, bits, c in R.cases(shape):
        est = R.estimate(packed, bits, c)
        cmap = R.fit(est["offsets"], est["state"], 1, 0.0, float(R.top_of(bits)) / 64.0)["map"]
        cmap[:, ::5] = 0
        cmap[0, 1::2] = np.where(cmap[0, 1::2] == 0, f32(0.5), cmap[0, 1::2])      # constant frames too have columns to rewrite
        gray = R.gray_of(packed, bits)
        gray[:, :, ::2] = POISON
        p2, g2 = R.apply(packed, gray, cmap, bits)
        out.append((name, packed, bits, c, est, cmap, gray, p2, g2))
    return out


def _check_case(rt, ref, offset=False):
    name, packed, bits, c, est, cmap, gray, p2, g2 = ref
    dev = _up(packed, offset)
    offsets, state = rt.cols_estimate(dev, _cfg(c), bits)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(offsets), est["offsets"].view(np.uint32)), (name, "offsets", np.argwhere(offsets.cpu().numpy() != est["offsets"])[:4].tolist())
    assert np.array_equal(state.cpu().numpy(), est["state"]), (name, "state")
    assert np.array_equal(bits_of(dev), packed.view(np.uint32)), (name, "the estimate only reads")
    g, m = _up(gray, offset), _up(cmap, offset)
    assert rt.cols_apply(dev, m, bits, gray=g) is dev
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), p2.view(np.uint32)), (name, "packed")
    assert np.array_equal(bits_of(g), g2.view(np.uint32)), (name, "gray")
    # without a gray plane the packed planes are the same
    dev = _up(packed, offset)
    rt.cols_apply(dev, m, bits)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), p2.view(np.uint32)), (name, "packed, no gray")
    # a map of zeros leaves the tensors bit for bit
    g = _up(gray, offset)
    rt.cols_apply(dev, torch.zeros_like(m), bits, gray=g)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), p2.view(np.uint32)) and np.array_equal(bits_of(g), gray.view(np.uint32)), (name, "zero map")


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


def test_an_empty_batch_is_nothing_and_runs_repeat():
    rt = _rt()
    name, packed, bits, c, est, cmap, *_ = _refs((2, 37, 53))[0]
    dev = _up(packed)
    o1, s1 = rt.cols_estimate(dev, _cfg(c), bits)
    o2, s2 = rt.cols_estimate(dev, _cfg(c), bits)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(o1), bits_of(o2)) and torch.equal(s1, s2) and int(s1.sum()) > 0
    # n = 0: no tensors needed, nothing launched
    rt.profile_enable(True)
    assert rt.lib.rvdd_cols_estimate(rt.h, None, 0, 37, 53, bits, C.byref(_cfg(c)), None, None, None) == 0
    assert rt.lib.rvdd_cols_apply(rt.h, None, None, None, 0, 37, 53, bits, None) == 0
    torch.cuda.synchronize()
    seen = launches(rt)
    rt.profile_enable(False)
    assert seen == {}, seen


def test_argument_errors_launch_nothing():
    from rvdd_release_amd.runtime import cols_cfg
    rt = _rt()
    n, hh, ww = 2, 6, 8
    packed = torch.full((n, 4, hh, ww), 0.25, device="cuda")
    gray = torch.full((n, hh, ww), POISON, device="cuda")
    cmap = torch.full((2, ww), 3.0, device="cuda")
    offsets = torch.full((n, 2, ww), 3.0, device="cuda")
    state = torch.full((n, 2, ww), 9, dtype=torch.uint8, device="cuda")
    good = dict(k_gate=3.0, noise_a=1.0, noise_b=0.0, var_floor=1.0)

    def estimate(p=0, o=0, s=0, n_=n, hh_=hh, ww_=ww, bits=12, cfg=0, **fields):
        c = None if cfg is None else cols_cfg(**dict(good, **fields))
        rc = rt.lib.rvdd_cols_estimate(rt.h, packed.data_ptr() if p == 0 else p, n_, hh_, ww_, bits, None if c is None else C.byref(c),
                                       offsets.data_ptr() if o == 0 else o, state.data_ptr() if s == 0 else s, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    def apply(p=0, m=0, n_=n, hh_=hh, ww_=ww, bits=12):
        rc = rt.lib.rvdd_cols_apply(rt.h, packed.data_ptr() if p == 0 else p, gray.data_ptr(), cmap.data_ptr() if m == 0 else m, n_, hh_, ww_, bits, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    inf, nan = float("inf"), float("nan")
    bad = [(dict(cfg=None), "cfg"), (dict(p=None), "packed"), (dict(o=None), "offsets"), (dict(s=None), "state"),
           (dict(k_gate=0.0), "k_gate"), (dict(k_gate=-1.0), "k_gate"), (dict(k_gate=inf), "k_gate"), (dict(k_gate=nan), "k_gate"),
           (dict(noise_a=inf), "noise_a"), (dict(noise_b=nan), "noise_b"), (dict(var_floor=0.0), "var_floor"), (dict(var_floor=nan), "var_floor"),
           (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"), (dict(ww_=4), r"\bww\b"), (dict(hh_=0), r"\bhh\b"),
           (dict(hh_=R.MAX_HH + 1), r"\bhh\b"), (dict(n_=-1), r"\bn\b"), (dict(n_=2 ** 30, ww_=2 ** 20), "blocks")]
    rt.profile_enable(True)
    for kwargs, names in bad:
        rc, msg = estimate(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_cols_estimate:") and re.search(names, msg), (kwargs, rc, msg)
    for kwargs, names in [(dict(p=None), "packed"), (dict(m=None), "map_dev"), (dict(bits=0), "bit_depth"), (dict(ww_=4), r"\bww\b"),
                          (dict(hh_=0), r"\bhh\b"), (dict(n_=-1), r"\bn\b"), (dict(n_=2 ** 20, hh_=2 ** 20, ww_=2 ** 20), "blocks")]:
        rc, msg = apply(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_cols_apply:") and re.search(names, msg), (kwargs, rc, msg)
    host = np.zeros((2, 8), np.float32)
    assert rt.lib.rvdd_set_cols(rt.h, host.ctypes.data, 4) == -1 and "ww" in rt.lib.rvdd_last_error(rt.h).decode()
    host[1, 3] = nan
    assert rt.lib.rvdd_set_cols(rt.h, host.ctypes.data, 8) == -1 and "map_host[1][3]" in rt.lib.rvdd_last_error(rt.h).decode()
    torch.cuda.synchronize()
    seen = launches(rt)
    assert seen == {}, seen
    assert (packed == 0.25).all() and (gray == POISON).all() and (offsets == 3.0).all() and (state == 9).all()
    # and the calls that are fine are counted, one launch each
    assert estimate()[0] == 0 and apply()[0] == 0
    torch.cuda.synchronize()
    seen = {k: v[0] for k, v in launches(rt).items()}
    rt.profile_enable(False)
    assert seen == {"cols_estimate_kernel": 1, "cols_apply_kernel": 1}, seen
    with pytest.raises(RuntimeError, match="cols_estimate: packed is"):
        rt.cols_estimate(gray, cols_cfg(**good))
    with pytest.raises(RuntimeError, match="cols_apply: cmap is"):
        rt.cols_apply(packed, cmap[:1])
    with pytest.raises(RuntimeError, match="set_cols: cmap is"):
        rt.set_cols(np.zeros((2, 8), np.float64))


# ---- 2. the stage inside the stream -------------------------------------------------------------------------------------------------
def _static_offsets(ww, bits=12, seed=91):
    """one whole-DN offset per column parity and plane column, -40 .. 40 DN of 12 bits scaled to `bits`: [2,ww] int64"""
    return np.rint(np.random.default_rng(seed).uniform(-40.0, 40.0, (2, ww)) / (1 << (12 - bits))).astype(np.int64)


def _videos(bits=12, defects=False, rows=False):
    """stream_compose.small_videos with one static offset per mosaic column (and, with `rows`, one per mosaic row and frame)"""
    rng = np.random.default_rng(78 + bits)
    out = []
    for m in small_videos(bits=bits, defects=defects):
        W = m.shape[2]
        line = R.mosaic_of(_static_offsets(W // 2, bits))[None, None, :]
        m = m.astype(np.int64) + line
        if rows:
            m = m + np.rint(rng.uniform(-40.0, 40.0, (m.shape[0], m.shape[1], 1)) / (1 << (12 - bits))).astype(np.int64)
        out.append(np.clip(m, 0, (1 << bits) - 1).astype(np.uint16))
    return out


def _map(ww=16, bits=12):
    """the map the stage tests take out: the injected offsets, a quarter DN off, every fifth column zero"""
    cmap = (_static_offsets(ww, bits).astype(np.float32) + f32(0.25))
    cmap[:, ::5] = 0
    return cmap


def _rows_rule(bits=12, k=3.0):
    from rvdd_release_amd.runtime import rows_cfg
    a, b = dpc_ref.iso_curve(3200, bits)
    return rows_cfg(k, a, b, 1.0, ((1 << bits) - 1) / 64.0)


class _WithCols:
    """A batch-1 handle for stream_compose.compose that takes the column map out where the stream does: behind the ingest, or, where
    the composition corrects defects, behind rvdd_dpc; and, with `rows`, the row offsets behind it."""

    def __init__(self, rt, cmap, bits, behind_dpc, rows=None):
        self._rt, self._map, self._bits, self._behind_dpc, self._rows_cfg = rt, torch.from_numpy(cmap).cuda(), bits, behind_dpc, rows

    def __getattr__(self, name):
        return getattr(self._rt, name)

    def _cols(self, packed, gray):
        self._rt.cols_apply(packed, self._map, self._bits, gray=gray)
        if self._rows_cfg is not None:
            offsets, _, _ = self._rt.rows_estimate(packed, self._rows_cfg, self._bits)
            self._rt.rows_apply(packed, offsets, self._bits, gray=gray)

    def ingest_raw(self, *args, **kwargs):
        packed, gray = self._rt.ingest_raw(*args, **kwargs)
        if not self._behind_dpc:
            self._cols(packed, gray)
        return packed, gray

    def dpc(self, packed, cfg, bit_depth=12, gray=None):
        out = self._rt.dpc(packed, cfg, bit_depth, gray=gray)
        self._cols(out, gray)
        return out


def _stage_case(future, all_frames, bits=12, dpc=None, match=None, rows=None, defects=False, container=None, cmap=None):
    videos = _videos(bits, defects, rows is not None)
    cmap = _map(16, bits) if cmap is None else cmap
    alone = _WithCols(_runtime(future, 1), cmap, bits, dpc is not None, rows)
    want = [compose(alone, v, future, all_frames=all_frames, bit_depth=bits, dpc=dpc, match=match) for v in videos]
    rt = _runtime(future, 2, stream_all_frames=all_frames)
    rt.set_cols(cmap)
    if dpc is not None:
        rt.set_dpc(dpc)
    if rows is not None:
        rt.set_rows(rows)
    if match is not None:
        rt.set_match(match)
    got = push_schedule(rt, videos, two_slot_schedule(videos), bits, container)
    rt.set_option("tvl1_async", 0)
    _same(got.by_slot[0], want[0] + want[2], "slot 0")
    _same(got.by_slot[1], want[1], "slot 1")
    return videos, got


@pytest.mark.parametrize("all_frames", [0, 1])
@pytest.mark.parametrize("future", [0, 1])
def test_stage_is_the_composition(future, all_frames):
    videos, got = _stage_case(future, all_frames)
    # the stage matters: a handle that never had it gives other outputs
    never = push_two_slots(_runtime(future, 2, stream_all_frames=all_frames), videos)
    assert not torch.equal(never[0][0], got.by_slot[0][0])


def test_stage_between_the_correction_and_the_rows_and_the_match():
    """defects first, then the columns, then the rows -- both in the sensor's DN --, then the map onto the checkpoint's curve"""
    from rvdd_release_amd.runtime import dpc_cfg, match_coeffs
    a, b = dpc_ref.iso_curve(3200, 12)
    cfg = match_coeffs(*match_ref.camera_curve(60.0, 256), 12, 3200)[0]
    _stage_case(1, 1, dpc=dpc_cfg(4, 4, a, b), match=cfg, rows=_rows_rule(), defects=True)


def test_stage_on_mipi_raw10_is_the_stage_on_the_unpacked_frames():
    _stage_case(1, 1, bits=10, container="mipi")


@pytest.mark.parametrize("future", [0, 1])
def test_a_zero_map_is_the_plain_stream(future):
    videos = _videos()
    on = _runtime(future, 2, stream_all_frames=1)
    on.set_cols(np.zeros((2, 16), np.float32))
    got = push_two_slots(on, videos)
    want = push_two_slots(_runtime(future, 2, stream_all_frames=1), videos)
    for s in range(2):
        _same(got[s], want[s], s)


def test_stage_off_restores_the_launches_and_a_map_of_another_width_is_refused():
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
    rt.set_cols(_map())
    ctls = ([FIRST, FIRST], [NEXT, NEXT], [NEXT, IDLE])
    plain = [counted(never, t, c) for t, c in enumerate(ctls)]
    on = [counted(rt, t, c) for t, c in enumerate(ctls)]
    for have, base in zip(on, plain):
        assert have == dict(base, cols_apply_kernel=1), (have, base)      # one launch per run of slots
    # a map of another width: the push is refused and nothing is launched
    rt.set_cols(np.zeros((2, 17), np.float32))
    rt.profile_enable(True)
    with pytest.raises(RuntimeError, match="rvdd_set_cols is one of 17 cell columns"):
        rt.video_push(frames(3), [NEXT, NEXT], 12, "mosaic")
    torch.cuda.synchronize()
    seen = launches(rt)
    rt.profile_enable(False)
    assert seen == {}, seen
    rt.set_cols(None)
    for r in (rt, never):
        r.video_push(frames(3), [IDLE, IDLE], 12, "mosaic")
    off = [counted(rt, t, c) for t, c in enumerate(ctls)]
    assert off == [counted(never, t, c) for t, c in enumerate(ctls)] == plain and "cols_apply_kernel" not in off[1]
    rt.set_option("tvl1_async", 0)
    never.set_option("tvl1_async", 0)


# ---- 3. the map found in the footage ------------------------------------------------------------------------------------------------
class _Footage:
    """what col_noise.estimate reads of a rawvideo dataset: uint16 mosaics held in memory"""
    container, layout = None, "mosaic"

    def __init__(self, videos):
        self._frames = {"v%d/%03d" % (v, t): m[t] for v, m in enumerate(videos) for t in range(m.shape[0])}
        self.videos = [("v%d" % v, ["v%d/%03d" % (v, t) for t in range(m.shape[0])]) for v, m in enumerate(videos)]

    def frame_size(self, path):
        return self._frames[path].shape

    def read_frame(self, path):
        return self._frames[path]


def test_the_map_found_in_the_footage_is_the_restatements_and_serves_as_a_file(tmp_path):
    from rvdd_release_amd import col_noise as M
    from rvdd_release_amd.runtime import cols_cfg
    videos = _videos()
    a, b = dpc_ref.iso_curve(3200, 12)
    rule = (3.0, a, b, 1.0)
    ops = _rt()
    offsets, state = M.estimate(ops, _Footage(videos), 12, cols_cfg(*rule), frames=12)
    # the frames it read: four spread over each video of five, the three of the last -- through the same ingest
    read = [videos[0][[0, 1, 3, 4]], videos[1][[0, 1, 3, 4]], videos[2]]
    assert offsets.shape == (11, 2, 16) and state.shape == offsets.shape
    packed = torch.cat([ops.ingest_raw(to_gpu(r), 12, "mosaic")[0] for r in read]).cpu().numpy()
    est = R.estimate(packed, 12, R.cfg(*rule))
    assert np.array_equal(offsets.view(np.uint32), est["offsets"].view(np.uint32)) and np.array_equal(state, est["state"])
    cmap, r = M.report(offsets, state, 0.0, 4095.0 / 64.0)
    ref = R.fit(offsets, state, (offsets.shape[0] + 1) // 2, 0.0, 4095.0 / 64.0)
    assert np.array_equal(cmap.view(np.uint32), ref["map"].view(np.uint32)) and r["applied"] == ref["stats"]["applied"] + ref["stats"]["clamped"] > 0
    # as a map of the stage, and as a file of the stage: the same outputs
    path = str(tmp_path / "cols.tif")
    M.write_map(path, cmap)
    outs = []
    for m in (cmap, M.read_map(path)):
        rt = _runtime(0, 2)
        rt.set_cols(m)
        outs.append(push_two_slots(rt, videos))
    for s in range(2):
        _same(outs[0][s], outs[1][s], s)
    never = push_two_slots(_runtime(0, 2), videos)
    assert not torch.equal(never[0][0], outs[0][0][0])
