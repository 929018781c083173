"""Defective-pixel correction without a GPU: the NumPy restatement (tests/dpc_ref.py) on hand-made planes whose results are
written out here, the frame in which nothing is flagged, the false-alarm rate of the rule on defect-free noise, the
arguments of the denoise command line, and the three functions in header and binding."""
import re

import numpy as np
import pytest

import dpc_ref as R

F = np.float32
A12, B12 = R.ISO_CURVES[3200]
# packed values whose DN at 12 bits is exact in f32: dn(v) = ((v + 1) * 0.5) * 4095
DN = {-1.0: 0.0, -0.75: 511.875, -0.5: 1023.75, 0.0: 2047.5, 0.5: 3071.25, 0.75: 3583.125, 1.0: 4095.0}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _sentinel(shape):
    return np.frombuffer(bytes([0xA5]) * (4 * int(np.prod(shape))), dtype=F).reshape(shape).copy()


def test_dn_table_is_exact():
    for v, dn in DN.items():
        assert ((F(v) + F(1)) * F(0.5)) * F(4095) == F(dn) and F(2) * (F(dn) / F(4095)) - F(1) == F(v)


def test_centre_spike_3x3():
    p = np.zeros((1, 4, 3, 3), F)
    p[0, 0] = -0.5
    p[0, 0, 1, 1] = 1.0                                  # plane 0: 1023.75 everywhere, 4095 in the centre
    gray = _sentinel((1, 3, 3))
    out, g, counts, hot, dead = R.dpc_ref(p, gray, 12, 4, 4, A12, B12, 1.0, counts=[[5, 9]])
    want = p.copy()
    want[0, 0, 1, 1] = -0.5                              # the median of eight samples of 1023.75
    assert np.array_equal(_bits(out), _bits(want))
    assert hot.sum() == 1 and hot[0, 0, 1, 1] and not dead.any()
    assert counts.tolist() == [[6, 9]]
    wg = _sentinel((1, 3, 3))
    wg[0, 1, 1] = (((1023.75 + 2047.5) + 2047.5) + 2047.5) * 0.25      # 1791.5625, exact
    assert wg[0, 1, 1] == F(1791.5625) and np.array_equal(_bits(g), _bits(wg))


def test_corner_spike_2x2_uses_mirrored_neighbours():
    p = np.zeros((1, 4, 2, 2), F)
    p[0, 3] = [[-1.0, 0.5], [0.5, 0.75]]                 # plane 3: a dead sample in the corner (0, 0)
    # its neighbours, rows (1, 0, 1) x columns (1, 0, 1) without itself: four times (1,1) = 3583.125, twice (0,1) and twice (1,0) =
    # 3071.25 -> median (3071.25 + 3583.125) / 2 = 3327.1875 = 0.8125 * 4095 -> 0.625; a clamped border would give another median.
    # At K = 6 the corner (1,1) -- 511.875 above its largest neighbour, its own neighbours half of them the dead sample -- stays.
    gray = _sentinel((1, 2, 2))
    out, g, counts, hot, dead = R.dpc_ref(p, gray, 12, 6, 6, A12, B12)
    want = p.copy()
    want[0, 3, 0, 0] = 0.625
    assert np.array_equal(_bits(out), _bits(want))
    assert dead.sum() == 1 and dead[0, 3, 0, 0] and not hot.any() and counts.tolist() == [[0, 1]]
    wg = _sentinel((1, 2, 2))
    wg[0, 0, 0] = (((2047.5 + 2047.5) + 2047.5) + 3327.1875) * 0.25      # the median in DN, not a round trip: 2367.421875
    assert np.array_equal(_bits(g), _bits(wg))
    # one side off: nothing happens
    out, g, counts, hot, dead = R.dpc_ref(p, gray, 12, 6, 0, A12, B12)
    assert np.array_equal(_bits(out), _bits(p)) and np.array_equal(_bits(g), _bits(gray)) and counts.tolist() == [[0, 0]]


def test_line_4x5_is_not_flagged():
    p = np.full((1, 4, 4, 5), -0.5, F)
    p[0, 2, :, 2] = 1.0                                  # plane 2: a one-sample-wide vertical line of 4095 on 1023.75
    gray = _sentinel((1, 4, 5))
    out, g, counts, hot, dead = R.dpc_ref(p, gray, 12, 4, 4, A12, B12, counts=[[3, 4]])
    # every line sample has the line's continuation among its neighbours (mirrored at the ends): hi = 4095, d = 0
    assert not hot.any() and not dead.any() and counts.tolist() == [[3, 4]]
    assert np.array_equal(_bits(out), _bits(p)) and np.array_equal(_bits(g), _bits(gray))


@pytest.mark.parametrize("shape", [(1, 2, 2), (2, 7, 9)])
def test_nothing_flagged_returns_the_input_bits(shape):
    n, hh, ww = shape
    p, _ = R.ingest(R.noisy_cells(n, hh, ww, 12, 12800, seed=3), 12)
    p[0, 0, 0, 0] = 1.0
    gray = _sentinel(shape)
    out, g, counts, hot, dead = R.dpc_ref(p, gray, 12, 1e18, 1e18, A12, B12)      # 1e18 squared is +inf in f32
    assert np.array_equal(_bits(out), _bits(p)) and g.tobytes() == bytes([0xA5]) * g.nbytes
    assert not counts.any() and not hot.any() and not dead.any()


# ---- the false-alarm rate -------------------------------------------------------------------------------------------------
# Measured with this file's `defect_free` and the committed reference on 33.5 M samples per ISO (eight seeds of eight frames of
# 256 x 512 cells), K = 4: 117 flags at ISO 3200 (91 hot, 26 dead) and 447 at ISO 12800 (429 hot, 18 dead; one of them a sample at
# 4095) -- 3.5e-6 and 1.3e-5 of the samples; K = 3: 1.26e-4 and 1.53e-4.  The test draws a quarter of that and allows four times the
# rate: the head room covers the seed-to-seed spread of a count of a few dozen events.
RATE_K4 = {3200: 3.5e-6, 12800: 1.33e-5}


def defect_free(n, hh, ww, iso, seed):
    """n whole-DN 12-bit frames [n,hh,ww,4] without defects: even frames flat at a level of linspace(300, 3800, n), odd frames a
    horizontal ramp 300 -> 3800; noise m + sqrt(max(ka m - kb, 0)) z of the ISO's curve, rounded and clipped"""
    rng = np.random.default_rng(seed)
    ka, kb = R.ISO_CURVES[iso]
    level = np.linspace(300, 3800, n)
    m = np.empty((n, hh, ww, 4))
    for i in range(n):
        m[i] = level[i] if i % 2 == 0 else np.linspace(300, 3800, ww)[None, :, None]
    z = rng.standard_normal(m.shape)
    return np.clip(np.rint(m + np.sqrt(np.maximum(ka * m - kb, 0.0)) * z), 0, 4095).astype(F)


@pytest.mark.parametrize("iso", [3200, 12800])
def test_false_alarm_rate_at_k4(iso):
    ka, kb = R.ISO_CURVES[iso]
    flags = samples = 0
    for chunk in range(2):
        p, _ = R.ingest(defect_free(8, 256, 512, iso, seed=7000 * iso + chunk), 12)
        counts = R.dpc_ref(p, None, 12, 4, 4, ka, kb, 1.0)[2]
        flags += int(counts.sum())
        samples += p.size
    rate = flags / samples
    print("ISO %d, K = 4: %d flags in %d samples, rate %.3g (bound %.3g)" % (iso, flags, samples, rate, 4 * RATE_K4[iso]))
    assert rate <= 4 * RATE_K4[iso], (flags, samples, rate)


# ---- the command line -----------------------------------------------------------------------------------------------------
def test_denoise_dpc_arguments():
    from rvdd_release_amd import denoise
    from rvdd_release_amd.runtime import dpc_cfg
    assert all(f in denoise.__doc__ for f in ("--dpc K", "--dpc_dead", "--dpc_iso", "--dpc_noise"))
    assert denoise._parse([]).dpc is None
    for bits in (10, 12, 14):
        for iso, (ka, kb) in R.ISO_CURVES.items():
            s = (2 ** bits - 1) / 4095.0
            k_hot, k_dead, a, b, floor = denoise._parse(["--dpc", "4", "--dpc_iso", str(iso), "--bit_depth", str(bits)]).dpc
            assert (k_hot, k_dead, floor) == (4.0, 4.0, 1.0)
            assert a == s * ka and b == s * s * kb               # formed in double ...
            cfg = dpc_cfg(k_hot, k_dead, a, b, floor)
            assert F(cfg.noise_a) == F(s * ka) and F(cfg.noise_b) == F(s * s * kb)      # ... rounded to f32 once
    assert denoise._parse(["--dpc", "4", "--dpc_iso", "3200"]).dpc[2:4] == (8.0034, 2043.51144)
    assert denoise._parse(["--dpc", "5", "--dpc_dead", "0", "--dpc_iso", "12800"]).dpc[:2] == (5.0, 0.0)
    assert denoise._parse(["--dpc", "3.5", "--dpc_dead", "6", "--dpc_noise", "2.5,100"]).dpc == (3.5, 6.0, 2.5, 100.0, 1.0)
    assert denoise._parse(["--dpc", "4", "--dpc_noise", "2.5,-3,0.25", "--bit_depth", "14"]).dpc == (4.0, 4.0, 2.5, -3.0, 0.25)
    for bad, what in ((["--dpc", "4"], "exactly one of"), (["--dpc", "4", "--dpc_iso", "3200", "--dpc_noise", "1,2"], "exactly one of"),
                      (["--dpc_iso", "3200"], "belong to --dpc"), (["--dpc_dead", "0"], "belong to --dpc"),
                      (["--dpc", "4", "--dpc_iso", "6400"], "--dpc_iso"), (["--dpc", "-1", "--dpc_iso", "3200"], "thresholds"),
                      (["--dpc", "4", "--dpc_noise", "1"], "--dpc_noise"), (["--dpc", "4", "--dpc_noise", "1,x"], "--dpc_noise"),
                      (["--dpc", "4", "--dpc_noise", "1,2,0"], "floor")):
        with pytest.raises(SystemExit, match=what):
            denoise._parse(bad)


def test_header_binding_and_struct_agree():
    import ctypes as C
    import os
    from conftest import REPO
    from rvdd_release_amd import _lib
    txt = open(os.path.join(REPO, "include", "rvdd.h")).read()
    for fn in ("rvdd_dpc", "rvdd_set_dpc", "rvdd_dpc_counts"):
        assert re.search(r"\bint %s\(" % fn, txt) and fn in _lib.exported_symbols()
    m = re.search(r"typedef struct rvdd_dpc_cfg \{(.*?)\} rvdd_dpc_cfg;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S)
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip() for f in decl.replace("float", "").split(",")]
    assert fields == [f for f, _ in _lib.RvddDpcCfg._fields_] and all(t is C.c_float for _, t in _lib.RvddDpcCfg._fields_)
    # rvdd_set_dpc is documented on its own, outside rvdd_set_option's list of names
    known = txt[txt.index("Known names:"):txt.index("int rvdd_set_option(")]
    assert "dpc" not in known
    lib = _lib.load()
    assert all(hasattr(lib, fn) for fn in ("rvdd_dpc", "rvdd_set_dpc", "rvdd_dpc_counts"))
