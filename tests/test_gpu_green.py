"""Green equilibration on the device: rvdd_green_estimate and rvdd_green_apply against their NumPy restatement (tests/green_ref.py)
bit for bit -- e, level, states, packed planes and gray planes --, the argument errors, the stage inside rvdd_video_push
(rvdd_set_green) against the same schedule composed from the stand-alone entry points of a batch-1 handle, and the map found by
green_eq.estimate and the command lines."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import dpc_ref
import green_ref as R
import match_ref
from gpu_support import bits_of, files_of, launches, ops_rt as _rt, same as _same, upload as _up
from stream_ref import to_gpu
from stream_compose import FIRST, IDLE, NEXT, compose, push_schedule, push_two_slots, small_runtime as _runtime, small_videos, two_slot_schedule

pytestmark = pytest.mark.gpu

SHAPES = R.SHAPES                                              # tests/green_ref.py says why each
POISON = float(R.POISON)
f32 = np.float32


def _cfg(c):
    from rvdd_release_amd.runtime import green_cfg
    return green_cfg(*[float(v) for v in c])


def _check_case(rt, ref, offset=False):
    name, packed, bits, c, pattern, est = (ref[k] for k in ("name", "packed", "bits", "cfg", "pattern", "est"))
    black = float(c[4])
    dev = _up(packed, offset)
    e, level, state = rt.green_estimate(dev, _cfg(c), bits, pattern)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(e), est["e"].view(np.uint32)), (name, "e", np.argwhere(e.cpu().numpy() != est["e"])[:4].tolist())
    assert np.array_equal(bits_of(level), est["level"].view(np.uint32)), (name, "level", level.cpu().numpy().reshape(-1)[:4], est["level"].reshape(-1)[:4])
    assert np.array_equal(state.cpu().numpy(), est["state"]), (name, "state")
    assert np.array_equal(bits_of(dev), packed.view(np.uint32)), (name, "the estimate only reads")
    g, m = _up(ref["gray"], offset), _up(ref["map"], offset)
    assert rt.green_apply(dev, m, black, bits, gray=g, pattern=pattern) is dev
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), ref["packed_out"].view(np.uint32)), (name, "packed", np.argwhere(dev.cpu().numpy() != ref["packed_out"])[:4].tolist())
    assert np.array_equal(bits_of(g), ref["gray_out"].view(np.uint32)), (name, "gray", np.argwhere(g.cpu().numpy() != ref["gray_out"])[:4].tolist())
    # without a gray plane the packed planes are the same
    dev = _up(packed, offset)
    rt.green_apply(dev, m, black, bits, pattern=pattern)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), ref["packed_out"].view(np.uint32)), (name, "packed, no gray")
    # a map of zeros leaves the tensors bit for bit
    g = _up(ref["gray"], offset)
    rt.green_apply(dev, torch.zeros_like(m), black, bits, gray=g, pattern=pattern)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), ref["packed_out"].view(np.uint32)) and np.array_equal(bits_of(g), ref["gray"].view(np.uint32)), (name, "zero map")
    # a [1,1] map: one gain for the frame
    flat = np.full((1, 1), -0.0125, np.float32)
    p2, g2 = R.apply(packed, ref["gray"], flat, black, bits, pattern)
    dev, g = _up(packed, offset), _up(ref["gray"], offset)
    rt.green_apply(dev, _up(flat), black, bits, gray=g, pattern=pattern)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(dev), p2.view(np.uint32)) and np.array_equal(bits_of(g), g2.view(np.uint32)), (name, "flat map")


# ---- 1. the kernels are the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kernels_are_the_restatement(shape):
    rt = _rt()
    for ref in R.refs(shape):
        _check_case(rt, ref)


def test_one_cell_form_on_a_wide_shape():
    """every tensor 4 bytes off a 16-byte boundary: the apply kernel's one-cell form at ww % 4 == 0"""
    rt = _rt()
    for ref in R.refs((1, 8, 640)):
        _check_case(rt, ref, offset=True)


def test_every_pattern_takes_its_own_planes():
    """GRBG is GBRG's geometry and BGGR is RGGB's: the same planes, the same bits"""
    rt = _rt()
    ref = R.refs((2, 37, 53))[0]
    for pattern in R.PATTERNS:
        est = R.estimate(ref["packed"], ref["bits"], ref["cfg"], pattern)
        e, level, state = rt.green_estimate(_up(ref["packed"]), _cfg(ref["cfg"]), ref["bits"], pattern)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(e), est["e"].view(np.uint32)) and np.array_equal(bits_of(level), est["level"].view(np.uint32)), pattern
        assert np.array_equal(state.cpu().numpy(), est["state"]), pattern
        p2, g2 = R.apply(ref["packed"], ref["gray"], ref["map"], float(ref["cfg"][4]), ref["bits"], pattern)
        dev, g = _up(ref["packed"]), _up(ref["gray"])
        rt.green_apply(dev, _up(ref["map"]), float(ref["cfg"][4]), ref["bits"], gray=g, pattern=pattern)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(dev), p2.view(np.uint32)) and np.array_equal(bits_of(g), g2.view(np.uint32)), pattern


def test_an_empty_batch_is_nothing_and_runs_repeat():
    rt = _rt()
    ref = R.refs((2, 37, 53))[0]
    c, bits = ref["cfg"], ref["bits"]
    dev = _up(ref["packed"])
    a = rt.green_estimate(dev, _cfg(c), bits, ref["pattern"])
    b = rt.green_estimate(dev, _cfg(c), bits, ref["pattern"])
    torch.cuda.synchronize()
    assert all(np.array_equal(bits_of(x), bits_of(y)) for x, y in zip(a[:2], b[:2])) and torch.equal(a[2], b[2]) and int(a[2].sum()) > 0
    # n = 0: no tensors needed, nothing launched
    rt.profile_enable(True)
    assert rt.lib.rvdd_green_estimate(rt.h, None, 0, 37, 53, bits, 0, C.byref(_cfg(c)), None, None, None, None) == 0
    assert rt.lib.rvdd_green_apply(rt.h, None, None, None, 1, 1, 0.0, 0, 37, 53, bits, 0, None) == 0
    torch.cuda.synchronize()
    seen = launches(rt)
    rt.profile_enable(False)
    assert seen == {}, seen


def test_argument_errors_launch_nothing():
    from rvdd_release_amd.runtime import green_cfg
    rt = _rt()
    n, hh, ww = 2, 40, 70                                            # 2 x 3 blocks
    packed = torch.full((n, 4, hh, ww), 0.25, device="cuda")
    gray = torch.full((n, hh, ww), POISON, device="cuda")
    gmap = torch.full((2, 3), 0.03, device="cuda")
    e, level = torch.full((n, 2, 3), 3.0, device="cuda"), torch.full((n, 2, 3), 3.0, device="cuda")
    state = torch.full((n, 2, 3), 9, dtype=torch.uint8, device="cuda")
    good = dict(k_gate=3.0, noise_a=1.0, noise_b=0.0, var_floor=1.0, black=0.0)

    def estimate(p=0, e_=0, l=0, s=0, n_=n, hh_=hh, ww_=ww, bits=12, pattern=0, cfg=0, **fields):
        c = None if cfg is None else green_cfg(**dict(good, **fields))
        rc = rt.lib.rvdd_green_estimate(rt.h, packed.data_ptr() if p == 0 else p, n_, hh_, ww_, bits, pattern, None if c is None else C.byref(c),
                                        e.data_ptr() if e_ == 0 else e_, level.data_ptr() if l == 0 else l, state.data_ptr() if s == 0 else s, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    def apply(p=0, m=0, gh=2, gw=3, black=0.0, n_=n, hh_=hh, ww_=ww, bits=12, pattern=0):
        rc = rt.lib.rvdd_green_apply(rt.h, packed.data_ptr() if p == 0 else p, gray.data_ptr(), gmap.data_ptr() if m == 0 else m, gh, gw, black, n_,
                                     hh_, ww_, bits, pattern, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    inf, nan = float("inf"), float("nan")
    bad = [(dict(cfg=None), "cfg"), (dict(p=None), "packed"), (dict(e_=None), r"\be is"), (dict(l=None), "level"), (dict(s=None), "state"),
           (dict(k_gate=0.0), "k_gate"), (dict(k_gate=-1.0), "k_gate"), (dict(k_gate=inf), "k_gate"), (dict(k_gate=nan), "k_gate"),
           (dict(noise_a=inf), "noise_a"), (dict(noise_b=nan), "noise_b"), (dict(var_floor=0.0), "var_floor"), (dict(var_floor=nan), "var_floor"),
           (dict(black=nan), "black"), (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"), (dict(pattern=-1), "pattern"), (dict(pattern=4), "pattern"),
           (dict(ww_=1), r"\bww\b"), (dict(hh_=1), r"\bhh\b"), (dict(n_=-1), r"\bn\b"), (dict(n_=2 ** 30, hh_=64, ww_=64), "blocks")]
    rt.profile_enable(True)
    for kwargs, names in bad:
        rc, msg = estimate(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_green_estimate:") and re.search(names, msg), (kwargs, rc, msg)
    for kwargs, names in [(dict(p=None), "packed"), (dict(m=None), "map_dev"), (dict(bits=0), "bit_depth"), (dict(pattern=7), "pattern"), (dict(ww_=1), r"\bww\b"),
                          (dict(hh_=1), r"\bhh\b"), (dict(n_=-1), r"\bn\b"), (dict(black=inf), "black"), (dict(gh=2, gw=2), "grid"), (dict(gh=1, gw=3), "grid"),
                          (dict(gh=0, gw=0), "grid"), (dict(n_=2 ** 20, hh_=2 ** 20, ww_=2 ** 20, gh=1, gw=1), "blocks")]:
        rc, msg = apply(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_green_apply:") and re.search(names, msg), (kwargs, rc, msg)
    host = np.zeros((2, 3), np.float32)
    assert rt.lib.rvdd_set_green(rt.h, host.ctypes.data, 0, 3, 0.0) == -1 and "gh" in rt.lib.rvdd_last_error(rt.h).decode()
    assert rt.lib.rvdd_set_green(rt.h, host.ctypes.data, 2, 3, nan) == -1 and "black" in rt.lib.rvdd_last_error(rt.h).decode()
    host[1, 2] = nan
    assert rt.lib.rvdd_set_green(rt.h, host.ctypes.data, 2, 3, 0.0) == -1 and "map_host[1][2]" in rt.lib.rvdd_last_error(rt.h).decode()
    torch.cuda.synchronize()
    seen = launches(rt)
    assert seen == {}, seen
    assert (packed == 0.25).all() and (gray == POISON).all() and (e == 3.0).all() and (level == 3.0).all() and (state == 9).all()
    # and the calls that are fine are counted, one launch each; the estimate writes every word, skipped blocks included
    assert estimate()[0] == 0 and apply()[0] == 0 and apply(gh=1, gw=1)[0] == 0
    torch.cuda.synchronize()
    seen = {k: v[0] for k, v in launches(rt).items()}
    rt.profile_enable(False)
    assert seen == {"green_estimate_kernel": 1, "green_apply_kernel": 2}, seen
    assert (state <= 1).all() and not (e == 3.0).any() and not (level == 3.0).any()
    with pytest.raises(RuntimeError, match="green_estimate: packed is"):
        rt.green_estimate(gray, green_cfg(**good))
    with pytest.raises(RuntimeError, match="green_apply: gmap is"):
        rt.green_apply(packed, gmap[0], 0.0)
    with pytest.raises(RuntimeError, match="set_green: gmap is"):
        rt.set_green(np.zeros((2, 3), np.float64))


# ---- 2. the stage inside the stream -------------------------------------------------------------------------------------------------
GAIN = f32(0.046875)                                           # the stage tests' flat map: 3/64, exact
BLACK = {12: 255.0, 10: 64.0}


def _videos(bits=12, defects=False, rows=False):
    """stream_compose.small_videos, and with `rows` one offset per mosaic row and frame"""
    rng = np.random.default_rng(79 + bits)
    out = []
    for m in small_videos(bits=bits, defects=defects):
        m = m.astype(np.int64)
        if rows:
            m = m + np.rint(rng.uniform(-40.0, 40.0, (m.shape[0], m.shape[1], 1)) / (1 << (12 - bits))).astype(np.int64)
        out.append(np.clip(m, 0, (1 << bits) - 1).astype(np.uint16))
    return out


def _cols_map(ww=16, bits=12):
    cmap = np.rint(np.random.default_rng(91).uniform(-40.0, 40.0, (2, ww)) / (1 << (12 - bits))).astype(np.float32) + f32(0.25)
    cmap[:, ::5] = 0
    return cmap


def _rows_rule(bits=12, k=3.0):
    from rvdd_release_amd.runtime import rows_cfg
    a, b = dpc_ref.iso_curve(3200, bits)
    return rows_cfg(k, a, b, 1.0, ((1 << bits) - 1) / 64.0)


class _WithGreen:
    """A batch-1 handle for stream_compose.compose that takes the green gains out where the stream does: behind the ingest, or, where
    the composition corrects defects, behind rvdd_dpc; with `cols` and `rows` the column map and the row offsets in front of it."""

    def __init__(self, rt, gmap, black, bits, behind_dpc, cols=None, rows=None):
        self._rt, self._map, self._black, self._bits, self._behind_dpc = rt, torch.from_numpy(gmap).cuda(), black, bits, behind_dpc
        self._cols, self._rows_cfg = None if cols is None else torch.from_numpy(cols).cuda(), rows

    def __getattr__(self, name):
        return getattr(self._rt, name)

    def _green(self, packed, gray):
        if self._cols is not None:
            self._rt.cols_apply(packed, self._cols, self._bits, gray=gray)
        if self._rows_cfg is not None:
            offsets, _, _ = self._rt.rows_estimate(packed, self._rows_cfg, self._bits)
            self._rt.rows_apply(packed, offsets, self._bits, gray=gray)
        self._rt.green_apply(packed, self._map, self._black, self._bits, gray=gray)      # the handle's "bayer_pattern"

    def ingest_raw(self, *args, **kwargs):
        packed, gray = self._rt.ingest_raw(*args, **kwargs)
        if not self._behind_dpc:
            self._green(packed, gray)
        return packed, gray

    def dpc(self, packed, cfg, bit_depth=12, gray=None):
        out = self._rt.dpc(packed, cfg, bit_depth, gray=gray)
        self._green(out, gray)
        return out


def _stage_case(future, all_frames, bits=12, dpc=None, match=None, cols=None, rows=None, defects=False, container=None, **options):
    videos = _videos(bits, defects, rows is not None)
    gmap = np.full((1, 1), GAIN, np.float32)
    alone = _WithGreen(_runtime(future, 1, **options), gmap, BLACK[bits], bits, dpc is not None, cols, rows)
    want = [compose(alone, v, future, all_frames=all_frames, bit_depth=bits, dpc=dpc, match=match) for v in videos]
    rt = _runtime(future, 2, stream_all_frames=all_frames, **options)
    rt.set_green(gmap, BLACK[bits])
    if dpc is not None:
        rt.set_dpc(dpc)
    if cols is not None:
        rt.set_cols(cols)
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


def test_stage_between_the_correction_the_columns_the_rows_and_the_match():
    """defects first, then the columns, then the rows, then the greens -- all in the sensor's DN --, then the map onto the checkpoint's curve"""
    from rvdd_release_amd.runtime import dpc_cfg, match_coeffs
    a, b = dpc_ref.iso_curve(3200, 12)
    cfg = match_coeffs(*match_ref.camera_curve(60.0, 256), 12, 3200)[0]
    _stage_case(1, 1, dpc=dpc_cfg(4, 4, a, b), match=cfg, cols=_cols_map(), rows=_rows_rule(), defects=True)


def test_stage_on_mipi_raw10_is_the_stage_on_the_unpacked_frames():
    _stage_case(1, 1, bits=10, container="mipi")


def test_stage_under_rggb_takes_planes_1_and_2():
    videos, got = _stage_case(0, 1, bayer_pattern=2)
    # and they are other planes than GBRG's: the same map under the default pattern gives other outputs
    rt = _runtime(0, 2, stream_all_frames=1, bayer_pattern=2)
    plain = push_two_slots(rt, videos)
    assert not torch.equal(plain[0][0], got.by_slot[0][0])


@pytest.mark.parametrize("future", [0, 1])
def test_a_zero_map_is_the_plain_stream(future):
    videos = _videos()
    on = _runtime(future, 2, stream_all_frames=1)
    on.set_green(np.zeros((1, 1), np.float32), 255.0)
    got = push_two_slots(on, videos)
    want = push_two_slots(_runtime(future, 2, stream_all_frames=1), videos)
    for s in range(2):
        _same(got[s], want[s], s)


def test_stage_off_restores_the_launches_and_a_map_of_another_grid_is_refused():
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
    rt.set_green(np.full((1, 1), GAIN, np.float32), 255.0)
    ctls = ([FIRST, FIRST], [NEXT, NEXT], [NEXT, IDLE])
    plain = [counted(never, t, c) for t, c in enumerate(ctls)]
    on = [counted(rt, t, c) for t, c in enumerate(ctls)]
    for have, base in zip(on, plain):
        assert have == dict(base, green_apply_kernel=1), (have, base)      # one launch per run of slots
    # a map of another grid: the push is refused and nothing is launched
    rt.set_green(np.zeros((2, 1), np.float32), 255.0)
    rt.profile_enable(True)
    with pytest.raises(RuntimeError, match="rvdd_set_green is one of 2 x 1 blocks"):
        rt.video_push(frames(3), [NEXT, NEXT], 12, "mosaic")
    torch.cuda.synchronize()
    seen = launches(rt)
    rt.profile_enable(False)
    assert seen == {}, seen
    rt.set_green(None)
    for r in (rt, never):
        r.video_push(frames(3), [IDLE, IDLE], 12, "mosaic")
    off = [counted(rt, t, c) for t, c in enumerate(ctls)]
    assert off == [counted(never, t, c) for t, c in enumerate(ctls)] == plain and "green_apply_kernel" not in off[1]
    rt.set_option("tvl1_async", 0)
    never.set_option("tvl1_async", 0)


# ---- 3. the map found in the footage, and the command lines ---------------------------------------------------------------------------
T, Hc, Wc = 6, 32, 48                                          # cells: 1 x 2 blocks
CURVE = (8.0, 2048.0)                                          # black at 256 DN


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """2 videos of 6 frames of 32 x 48 cells: green_ref's scene moving 3 cells a frame with 5 % imbalance under the noise of CURVE,
    uint16 TIFFs.  -> (root, the mosaics of both videos)"""
    from rvdd_release_amd import tiffio
    root = tmp_path_factory.mktemp("green_tree")
    rng = np.random.default_rng(20261021)
    videos = []
    for v in range(2):
        clean = R.imbalanced(R.scene(T, Hc, Wc, 40 * v, "gbrg"), 0.05, CURVE[1] / CURVE[0], "gbrg")
        dnv = np.clip(np.rint(clean + rng.normal(0.0, 1.0, clean.shape) * np.sqrt(CURVE[0] * clean - CURVE[1])), 0, 4095)
        m = np.zeros((T, 2 * Hc, 2 * Wc), np.uint16)
        for k in range(4):
            m[:, k >> 1::2, k & 1::2] = dnv[:, k]
        videos.append(m)
        os.makedirs(root / "u16" / ("%03d" % v))
        for t in range(T):
            tiffio.write(str(root / "u16" / ("%03d/%08d.tif" % (v, t))), m[t])
    return root, videos


def test_map_command_is_the_restatement_and_denoise_takes_its_file(tree, tmp_path, capsys):
    from conftest import WEIGHTS
    from rvdd_release_amd import denoise, green_eq
    root, videos = tree
    path = str(tmp_path / "green.tif")
    rule = ["--green_eq_curve", "%g,%g" % CURVE, "--green_eq_frames", str(2 * T)]
    capsys.readouterr()
    r = green_eq.main(["--dataroot", str(root), "--nFolder", "u16", "--bit_depth", "12", "--out", path] + rule)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(line) == 1 and json.loads(line[0])["applied"] == r["applied"] and json.loads(line[0])["frames"] == 2 * T
    # the restatement on the same frames: every frame of both videos, through the same ingest
    ops = _rt()
    packed = torch.cat([ops.ingest_raw(to_gpu(m), 12, "mosaic")[0] for m in videos]).cpu().numpy()
    c = R.cfg(3.0, *CURVE)
    est = R.estimate(packed, 12, c, "gbrg")
    want = R.fit(est["e"], est["level"], est["state"], c[4], T, 3.0, 0.10, 4095.0 / 64.0)
    got = green_eq.read_map(path)
    assert got.shape == (1, 2) and np.array_equal(got.view(np.uint32), want["map"].view(np.uint32))
    assert r["applied"] == want["stats"]["applied"] + want["stats"]["clamped"] == 2 and r["flat_gain"] == want["stats"]["flat_gain"]
    assert (np.abs(got - 0.05) < 0.01).all(), got                        # the injected 5 %, less what the gate keeps
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--dataroot", str(root), "--nFolder", "u16", "--batch_size", "2"]

    def run(name, *more):
        capsys.readouterr()
        res = str(tmp_path / name)
        stats = denoise.main(flags + ["--results_dir", res] + list(more))
        out = capsys.readouterr().out.splitlines()
        assert stats["frames"] == 2 * (T - 1)
        return files_of(res), [ln for ln in out if ln.startswith("green: ")]

    by_file, line = run("file", "--green_eq", path, "--green_eq_black", "256")
    assert len(line) == 1 and line[0].startswith("green: 2 of 2 blocks with a gain") and line[0].endswith("from " + path)
    auto, line = run("auto", "--green_eq", "auto", *rule)
    assert len(line) == 1 and line[0].startswith("green: 2 applied, 0 insignificant, 0 unsupported, 0 clamped of 2 blocks") and auto == by_file
    plain, line = run("plain")
    assert line == [] and sorted(plain) == sorted(by_file) and plain != by_file
    # where no block is significant the map is zero, and the output files are byte for byte those of a run without the flag
    nothing, line = run("nothing", "--green_eq", "auto", "--green_eq_sigma", "1000", *rule)
    assert len(line) == 1 and line[0].startswith("green: 0 applied, 2 insignificant") and nothing == plain
    green_eq.write_map(path, np.zeros((3, 2), np.float32))
    with pytest.raises(SystemExit, match="one camera per run"):
        denoise.main(flags + ["--results_dir", str(tmp_path / "bad"), "--green_eq", path, "--green_eq_black", "256"])
