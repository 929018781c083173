"""The column-noise rule on the CPU: tests/cols_ref.py's vectorised restatement against its scalar one word for word, rvdd_cols_fit
(host code, no device) against both bit for bit on every branch of the fit, the map's file and index forms, and what the rule does to
static Gaussian column offsets under white noise over sixteen frames of a moving scene."""
import ctypes as C
import functools

import numpy as np
import pytest

import cols_ref as R

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5), (1, 3, 8), (2, 5, 11)], ids=lambda s: "%dx%dx%d" % s)
def test_the_restatement_is_its_scalar_form(shape):
    seen = set()
    for name, packed, bits, c in R.cases(shape):
        fast, slow = R.estimate(packed, bits, c), R.estimate_slow(packed, bits, c)
        assert np.array_equal(_bits(fast["offsets"]), _bits(slow["offsets"])), (shape, name, "offsets")
        assert np.array_equal(fast["state"], slow["state"]) and np.array_equal(fast["cnt"], slow["cnt"]), (shape, name, "state / cnt")
        cmap = R.fit(fast["offsets"], fast["state"], 1, 0.0, 64.0)["map"]       # every applied column of the first frames
        cmap[:, ::3] = 0                                                        # and columns that stay as they are
        gray = R.gray_of(packed, bits)
        gray[:, :, ::2] = 7.0                                                   # what a cell that is not rewritten must keep
        pf, gf = R.apply(packed, gray, cmap, bits)
        ps, gs = R.apply_slow(packed, gray, cmap, bits)
        assert np.array_equal(_bits(pf), _bits(ps)) and np.array_equal(_bits(gf), _bits(gs)), (shape, name)
        keep = (cmap == 0).all(axis=0)
        assert np.array_equal(_bits(gf[:, :, keep]), _bits(gray[:, :, keep]))
        assert np.array_equal(_bits(pf[:, 0::2][:, :, :, cmap[0] == 0]), _bits(packed[:, 0::2][:, :, :, cmap[0] == 0]))
        seen |= R.classes(fast, shape[1])
    assert {"applied", "skipped"} <= seen, seen


def test_neighbours_are_mirrored_about_the_site_and_stay_inside():
    for ww in range(5, 20):
        for c in range(ww):
            for dc in R.DCS:
                q = R.neighbour(c, dc, ww)
                assert 0 <= q < ww, (ww, c, dc, q)
                if 0 <= c + dc < ww:
                    assert q == c + dc
                elif 0 <= c - dc < ww:
                    assert q == c - dc                              # the rule as stated; from nine columns on one of the two is inside
        assert ww < 9 or all(0 <= c + dc < ww or 0 <= c - dc < ww for c in range(ww) for dc in R.DCS)


def test_every_class_fires_on_the_inputs_of_the_gpu_test():
    seen, per_case = set(), {}
    for shape in R.SHAPES:
        if shape[1] > 40:
            continue                                                # the tall shapes are there for the strip widths, not the classes
        for name, packed, bits, c in R.cases(shape):
            got = R.classes(R.estimate(packed, bits, c), shape[1])
            per_case.setdefault(name, set()).update(got)
            seen |= got
    assert seen == R.CLASSES, R.CLASSES - seen
    assert {"half", "half_minus_one", "zero"} <= per_case["crafted"], per_case["crafted"]
    assert {"empty", "skipped"} <= per_case["step"], per_case["step"]
    assert per_case["constant"] == {"applied", "zero", "even"}, per_case["constant"]
    assert {"applied", "even", "odd"} <= per_case["scene12"] and {"applied", "zero"} <= per_case["bits4"]
    # the strip widths and their switches are all among the shapes
    assert {R.strip_of(hh) for _, hh, _ in R.SHAPES} == {32, 16, 8, 4}
    for cb, last in R.STRIPS[:-1]:
        assert R.strip_of(last) == cb and R.strip_of(last + 1) == cb // 2 and 4 * cb * ((2 * last) | 1) <= 160 * 1024 < 4 * cb * ((2 * last + 2) | 1)


# ---- the fit: the library's host code against the restatement -------------------------------------------------------------------------
def _fit_all(offsets, state, min_frames, k_sig, max_dn):
    """the library, the restatement and its scalar form: the same bits; -> the restatement's"""
    from rvdd_release_amd.runtime import cols_fit
    offsets, state = np.ascontiguousarray(offsets, np.float32), np.ascontiguousarray(state, np.uint8)
    cmap, mstate, stats = cols_fit(offsets, state, min_frames, k_sig, max_dn)
    for ref in (R.fit(offsets, state, min_frames, k_sig, max_dn), R.fit_slow(offsets, state, min_frames, k_sig, max_dn)):
        assert np.array_equal(_bits(cmap), _bits(ref["map"])), (cmap, ref["map"])
        assert np.array_equal(mstate, ref["mstate"]), (mstate, ref["mstate"])
        assert stats == ref["stats"], (stats, ref["stats"])
    return ref


def _columns(cols, F):
    """cols: a list of per-column lists of values (None = the frame skipped the column) -> offsets, state [F,2,ww] with ww >= 1; the
    list fills parity 0 first, then parity 1"""
    ww = (len(cols) + 1) // 2
    offsets, state = np.zeros((F, 2, ww), np.float32), np.zeros((F, 2, ww), np.uint8)
    for k, col in enumerate(cols):
        for i, v in enumerate(col):
            if v is not None:
                offsets[i, k // ww, k % ww] = v
                state[i, k // ww, k % ww] = 1
    return offsets, state


def test_fit_branches_one_by_one():
    # F = 1: the one estimate is the offset, its mad is 0, so it is significant whatever k_sig
    o, s = _columns([[2.5], [None], [-0.0625], [0.0]], 1)
    r = _fit_all(o, s, 1, 3.0, 64.0)
    assert r["map"].tolist() == [[2.5, 0.0], [-0.0625, 0.0]] and r["mstate"].tolist() == [[1, 0], [1, 1]]
    assert r["stats"]["floor_dn"] == 0.0 and r["stats"]["sum_q2"] == 40 * 40 + 1
    # min_frames below 1 counts as 1: a column nobody estimated is unsupported all the same
    assert _fit_all(o, s, 0, 3.0, 64.0)["mstate"].tolist() == [[1, 0], [1, 1]]
    # odd and even nf, nf one below min_frames, skipped frames in between
    F = 6
    cols = [[1.0, 3.0, 2.0, None, None, None],            # nf = 3: the middle one
            [1.0, 4.0, 2.0, 3.0, None, None],             # nf = 4: the mean of the middle two
            [None, 5.0, None, 5.0, 5.0, 5.0],             # mad = 0
            [5.0, None, 6.0, None, None, None],           # nf = 2 < 3: unsupported
            [0.1, -0.1, 0.2, -0.2, 0.05, 10.0],           # an outlier frame does not move the median; insignificant
            [None] * 6]                                   # all skipped
    o, s = _columns(cols, F)
    r = _fit_all(o, s, 3, 0.0, 64.0)                      # k_sig = 0: every supported column is kept
    assert r["map"].reshape(-1).tolist() == [2.0, 2.5, 5.0, 0.0, f32(f32(f32(0.05) + f32(0.1)) * f32(0.5)), 0.0]
    assert r["mstate"].reshape(-1).tolist() == [1, 1, 1, 0, 1, 0]
    r = _fit_all(o, s, 3, 3.0, 64.0)
    # 2 and 2.5 with a mad of 1 lie within three standard errors of zero (4 * 3 = 12 and 6.25 * 4 = 25 against 9 * 3.4528 = 31); a mad of 0
    # always passes
    assert r["mstate"].reshape(-1).tolist() == [3, 3, 1, 0, 3, 0] and r["stats"]["insignificant"] == 3 and r["stats"]["unsupported"] == 2
    # the clamp on both sides, and a value exactly on it (not clamped)
    o, s = _columns([[9.0, 9.5], [-9.0, -9.5], [8.0, 8.0], [-8.0, -8.0]], 2)
    r = _fit_all(o, s, 1, 0.0, 8.0)
    assert r["map"].tolist() == [[8.0, -8.0], [8.0, -8.0]] and r["mstate"].tolist() == [[2, 2], [1, 1]] and r["stats"]["clamped"] == 2
    # all skipped
    r = _fit_all(np.ones((3, 2, 5), np.float32), np.zeros((3, 2, 5), np.uint8), 1, 3.0, 8.0)
    assert not r["map"].any() and not r["mstate"].any() and r["stats"]["unsupported"] == 10 and r["stats"]["floor_dn"] == 0.0


def test_fit_on_the_significance_boundary_and_one_ulp_below():
    """nf = 4, v = [o - 1, o, o, 10]: the median is o, the deviations 0, 0, 1, 10 - o, mad = 0.5.  With o = 1.5 the left side is
    (1.5 * 1.5) * 4 = 9 exactly; k_sig is searched so that (k_sig * k_sig) * (3.4528f * 0.25) rounds to 9 as well: the column is ON
    the boundary and kept (the test is <).  One ulp of o less gives a left side of 9 - 2^-20, one ulp below: insignificant."""
    rhs_of = lambda k: f32(f32(k * k) * f32(R.VAR_MEDIAN * f32(0.25)))
    k = f32(np.sqrt(9.0 / float(f32(R.VAR_MEDIAN * f32(0.25)))))
    cands = [k]
    for _ in range(64):
        cands = [np.nextafter(cands[0], f32(0))] + cands + [np.nextafter(cands[-1], f32(100))]
    hits = [c for c in cands if rhs_of(c) == f32(9.0)]
    assert hits, "no f32 k_sig puts the right side on 9"
    k_sig = float(hits[0])
    on, below = f32(1.5), np.nextafter(f32(1.5), f32(0))
    assert f32(f32(below * below) * f32(4)) == np.nextafter(f32(9.0), f32(0))
    o, s = _columns([[on - f32(1), on, on, 10.0], [below - f32(1), below, below, 10.0]], 4)
    assert o[0, 1, 0] + f32(1) == below                                   # the column's values are exact
    r = _fit_all(o, s, 4, k_sig, 64.0)
    assert r["mstate"].tolist() == [[1], [3]] and r["map"].tolist() == [[1.5], [0.0]]


def test_fit_refuses_what_it_cannot_take():
    from rvdd_release_amd import _lib
    lib = _lib.load()
    o, s = np.zeros((2, 2, 5), np.float32), np.ones((2, 2, 5), np.uint8)
    m, ms = np.zeros((2, 5), np.float32), np.zeros((2, 5), np.uint8)

    def call(op=o.ctypes.data, sp=s.ctypes.data, F=2, ww=5, cfg=(1, 3.0, 8.0), mp=m.ctypes.data, msp=ms.ctypes.data):
        c = None if cfg is None else C.byref(_lib.RvddColsFitCfg(*cfg))
        rc = lib.rvdd_cols_fit(op, sp, F, ww, c, mp, msp, None)
        return rc, lib.rvdd_last_error(None).decode()

    assert call()[0] == 0                                                 # stats may be NULL
    for kwargs, name in [(dict(op=None), "offsets_host"), (dict(sp=None), "state_host"), (dict(cfg=None), "fit_cfg"), (dict(mp=None), "map_host"),
                         (dict(msp=None), "mstate_host"), (dict(F=0), r"F must"), (dict(ww=0), "ww must"), (dict(cfg=(1, -1.0, 8.0)), "k_sig"),
                         (dict(cfg=(1, float("nan"), 8.0)), "k_sig"), (dict(cfg=(1, 3.0, 0.0)), "max_dn"), (dict(cfg=(1, 3.0, float("inf"))), "max_dn")]:
        rc, msg = call(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_cols_fit:") and name.split()[0] in msg, (kwargs, rc, msg)
    from rvdd_release_amd.runtime import cols_fit
    with pytest.raises(RuntimeError, match="cols_fit: offsets is"):
        cols_fit(o, s[:1], 1)


def test_structs_and_the_cfg():
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import COLS_MAX_HH, cols_cfg
    assert C.sizeof(_lib.RvddColsCfg) == 16 and C.sizeof(_lib.RvddColsFitCfg) == 12 and C.sizeof(_lib.RvddColsStats) == 32
    assert _lib.RvddColsStats.sum_q2.offset == 16 and _lib.RvddColsStats.floor_dn.offset == 24 and COLS_MAX_HH == R.MAX_HH
    c = cols_cfg(3, 8.0, 2043.5)
    assert (c.k_gate, c.noise_a, c.noise_b, c.var_floor) == (3.0, 8.0, 2043.5, 1.0)


# ---- the map's two forms and its file ---------------------------------------------------------------------------------------------------
def test_index_map_and_file_round_trip(tmp_path):
    from rvdd_release_amd import col_noise as M
    from rvdd_release_amd import tiffio
    ww = 7
    cmap = (np.arange(2 * ww, dtype=np.float32).reshape(2, ww) - 6.25) * f32(0.37)
    line = M.mosaic_of(cmap)
    assert line.shape == (2 * ww,) and all(line[x] == cmap[x & 1, x >> 1] for x in range(2 * ww))
    assert np.array_equal(_bits(line), _bits(R.mosaic_of(cmap))) and np.array_equal(_bits(M.map_of(line)), _bits(cmap))
    assert np.array_equal(_bits(R.map_of(line)), _bits(cmap))
    path = str(tmp_path / "cols.tif")
    M.write_map(path, cmap)
    raw = tiffio.read(path)
    assert raw.dtype == np.float32 and raw.reshape(-1).shape == (2 * ww,) and np.array_equal(_bits(raw.reshape(-1)), _bits(line))
    assert np.array_equal(_bits(M.read_map(path)), _bits(cmap))
    # what is not a column map
    for bad in (np.zeros((2, 14), np.float32), np.zeros((1, 13), np.float32), np.zeros((1, 14), np.uint16), np.zeros((1, 8), np.float32),
                np.full((1, 14), np.nan, np.float32)):
        tiffio.write(path, bad)
        with pytest.raises(RuntimeError, match="a column map"):
            M.read_map(path)
    with pytest.raises(RuntimeError, match="even number"):
        M.map_of(np.zeros(13, np.float32))
    with pytest.raises(RuntimeError, match=r"\[2,ww\]"):
        M.mosaic_of(np.zeros((3, 5), np.float32))


# ---- what the rule does to column noise -----------------------------------------------------------------------------------------------
SIGMA, F, HH, WW = 120.0, 16, 64, 96


def _highpassed_col_error(err):
    """the std over the columns of a per-column error [2,ww], a 9-column moving average of it taken out (the columns that have all nine)"""
    hp = [e[4:-4] - np.convolve(e, np.ones(9) / 9.0, mode="valid") for e in err]
    return float(np.std(np.concatenate(hp)))


@functools.lru_cache(maxsize=None)
def _statistical_case(sigma_col):
    """the setup of the rule's prototype: 16 frames of 64 x 96 cells, pixel sigma 120 DN, the scene moving 3 px a frame, K = 3,
    k_sig = 3, min_frames = F / 2"""
    rng = np.random.default_rng(20261021)
    y, x = np.mgrid[0:HH, 0:WW].astype(np.float64)
    cols = rng.normal(0.0, 1.0, (2, WW)) * sigma_col
    frames = []
    for i in range(F):
        base = 1800.0 + 600.0 * np.sin((x + 3.0 * i) / 11.0) * np.cos((y + 3.0 * i) / 17.0) + 150.0 * np.sin((x + 3.0 * i) / 7.0 + y / 5.0)
        clean = np.stack([base, 0.8 * base + 50.0, 0.9 * base, 0.8 * base + 20.0])
        frames.append(clean + rng.normal(0.0, SIGMA, clean.shape) + cols[[0, 1, 0, 1]][:, None, :])
    packed = R.norm_dn(np.stack(frames).astype(np.float32), R.top_of(12))
    est = R.estimate(packed, 12, R.cfg(3.0, 0.0, -SIGMA * SIGMA, 1.0))
    fit = R.fit(est["offsets"], est["state"], F // 2, 3.0, 4095.0 / 64.0)
    return cols, est, fit


def test_column_noise_falls_and_clean_footage_is_left_alone():
    """Measured with this seed (DESIGN.md 4.21 has the same numbers): sigma_col = 30 DN -- high-passed column error 31.21 -> 8.30 DN,
    ratio 0.266 (the bound is 0.5), 127 of 192 columns applied, 12 of them at the clamp of 64 DN, 65 insignificant, floor 4.74 DN;
    sigma_col = 0 -- 2 of 192 columns changed (1 %; the bound is 10 %), map rms 1.24 DN = 0.0104 sigma (the bound is 0.05 sigma),
    per-frame estimate rms 16.55 DN."""
    cols, est, fit = _statistical_case(30.0)
    before, after = _highpassed_col_error(cols), _highpassed_col_error(cols - fit["map"].astype(np.float64))
    print("sigma_col = 30: high-passed column error %.2f -> %.2f DN (ratio %.3f); %s" % (before, after, after / before, fit["stats"]))
    assert after <= 0.5 * before, (before, after)
    cols0, est0, fit0 = _statistical_case(0.0)
    changed = int((fit0["map"] != 0).sum())
    rms0 = float(np.sqrt((fit0["map"].astype(np.float64) ** 2).mean()))
    per_frame = float(np.sqrt((est0["offsets"][est0["state"] == 1].astype(np.float64) ** 2).mean()))
    print("sigma_col = 0: %d of %d columns changed, map rms %.2f DN (%.4f sigma), per-frame estimate rms %.2f DN; %s"
          % (changed, 2 * WW, rms0, rms0 / SIGMA, per_frame, fit0["stats"]))
    assert changed <= 0.10 * 2 * WW, changed
    assert rms0 < 0.05 * SIGMA, rms0
    # pooling is what protects clean footage: one frame's estimates are several times the map's
    assert per_frame > 3.0 * rms0, (per_frame, rms0)
