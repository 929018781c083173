"""Matching footage to the checkpoint's noise curve without a GPU: rvdd_match_coeffs through ctypes (identity, the algebra of the
map, its errors), the round trip of every integer DN through the NumPy restatement of the two kernels (tests/match_ref.py), and the
flag rules of the denoise command line."""
import ctypes as C

import numpy as np
import pytest

import match_ref as R

ISOS = (3200, 12800)


def _coeffs(a, b, bits, iso_or_curve):
    from rvdd_release_amd.runtime import match_coeffs
    return match_coeffs(a, b, bits, iso_or_curve)


# ---- identity -------------------------------------------------------------------------------------------------------------------
def test_reference_curve_onto_itself_is_the_identity():
    from rvdd_release_amd.runtime import dpc_iso_curve
    cfg, s, t = _coeffs(8.0034, 2043.51144, 12, (8.0034, 2043.51144))
    assert (cfg.scale, cfg.offset, s, t) == (1.0, 0.0, 1.0, 0.0)
    for iso in ISOS:
        cfg, s, t = _coeffs(*R.ISO_CURVES[iso], 12, iso)
        assert (cfg.scale, cfg.offset, s, t) == (1.0, 0.0, 1.0, 0.0)
        for bits in (10, 14):
            a, b = dpc_iso_curve(iso, bits)
            cfg, s, t = _coeffs(a, b, bits, iso)
            off = (s - 1.0) + (2.0 * t) / 4095.0
            assert abs(s - 1) < 1e-12 and abs(off) < 1e-12 and abs(cfg.offset) < 1e-12 and cfg.scale == 1.0, (iso, bits, s, off)


# ---- algebra --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iso", ISOS)
def test_the_map_takes_the_curve_onto_the_reference(iso):
    """With x' = s k m + t (12-bit DN) the variance s^2 k^2 (a m - b) of the mapped sample is the reference curve at x'."""
    a_ref, b_ref = R.ISO_CURVES[iso]
    for bits, a, black in R.CAMERAS:
        a, b = R.camera_curve(a, black)
        cfg, s, t = _coeffs(a, b, bits, iso)
        ws, wo, s_py, t_py = R.coeffs(a, b, bits, a_ref, b_ref)
        # the library's f64 is Python's: the same operations in the same order
        assert (s, t) == (s_py, t_py) and cfg.scale == ws and cfg.offset == wo, (bits, a, iso)
        k = 4095.0 / (2 ** bits - 1)
        top = 2 ** bits - 1
        for m in np.linspace(black + 0.03 * top, top, 16):
            m = float(m)
            got = s * s * k * k * (a * m - b)
            want = a_ref * (s * k * m + t) - b_ref
            assert abs(got - want) <= 1e-9 * abs(want), (bits, a, iso, m, got, want)
        # the map on [-1,1] is the map on DN: v' of sample m is the sample of x'
        v = 2.0 * (m / top) - 1.0
        assert abs((s * v + ((s - 1.0) + 2.0 * t / 4095.0)) - (2.0 * (s * k * m + t) / 4095.0 - 1.0)) < 1e-12


def test_curve_argument_forms():
    cfg, s, t = _coeffs(60.0, 60.0 * 256 - 100, 12, 3200)
    cfg2, s2, t2 = _coeffs(60.0, 60.0 * 256 - 100, 12, R.ISO_CURVES[3200])
    assert (cfg.scale, cfg.offset, s, t) == (cfg2.scale, cfg2.offset, s2, t2) and abs(s - 8.0034 / 60) < 1e-15
    with pytest.raises(ValueError, match="6400"):
        _coeffs(60.0, 0.0, 12, 6400)
    with pytest.raises(ValueError, match="a_ref, b_ref"):
        _coeffs(60.0, 0.0, 12, (1.0, 2.0, 3.0))


# ---- round trip of integer DN -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_bits", [8, 10, 12, 14, 16])
def test_every_dn_survives_match_and_unmatch(grid_bits):
    """Every DN of the grid through packed = 2 (dn / top) - 1, match, unmatch and rint(dn(v)): exactly the DN, for the coefficients of
    every camera against both checkpoint curves.  A = 500 (1 / s up to 62) stays within a small fraction of a DN too."""
    dn = np.arange(2 ** grid_bits, dtype=np.float32)
    v = R.packed_of_dn(dn, grid_bits)
    for bits, a, black in R.CAMERAS + [(12, 500.0, 256)]:
        a, b = R.camera_curve(a, black)
        for iso in ISOS:
            cfg, _, _ = _coeffs(a, b, bits, iso)
            m = R.match_raw_ref(v, cfg.scale, cfg.offset)
            back = R.dn_of(R.unmatch_rgb_ref(m, cfg.scale, cfg.offset), grid_bits)
            worst = float(np.abs(back.astype(np.float64) - dn).max())
            print("grid %d bits, camera (%d bits, a = %g), iso %d: worst deviation %.4f DN" % (grid_bits, bits, a, iso, worst))
            assert np.array_equal(np.rint(back), dn), (grid_bits, bits, a, iso, worst)


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_coeffs_argument_errors():
    from rvdd_release_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    good = dict(a=60.0, b=15260.0, bits=12, a_ref=8.0034, b_ref=2043.51144)
    bad = [("a", 0.0), ("a", -1.0), ("a", nan), ("a", inf), ("b", nan), ("b", inf), ("b", -inf), ("bits", 0), ("bits", 17), ("a_ref", 0.0),
           ("a_ref", -2.0), ("a_ref", nan), ("a_ref", inf), ("b_ref", nan), ("b_ref", -inf)]
    for field, value in bad:
        k = dict(good, **{field: value})
        out, st = _lib.RvddMatchCfg(7.0, 7.0), (C.c_double * 2)(7.0, 7.0)
        rc = lib.rvdd_match_coeffs(k["a"], k["b"], k["bits"], k["a_ref"], k["b_ref"], C.byref(out), st)
        msg = lib.rvdd_last_error(None).decode()
        name = "bit_depth" if field == "bits" else field
        assert rc == -1 and msg.startswith("rvdd_match_coeffs: " + name + " "), (field, value, rc, msg)
        assert (out.scale, out.offset, st[0], st[1]) == (7.0, 7.0, 7.0, 7.0)
    assert lib.rvdd_match_coeffs(60.0, 15260.0, 12, 8.0034, 2043.51144, None, None) == -1
    assert "out" in lib.rvdd_last_error(None).decode()
    # s_t is optional
    out = _lib.RvddMatchCfg()
    assert lib.rvdd_match_coeffs(60.0, 15260.0, 12, 8.0034, 2043.51144, C.byref(out), None) == 0
    assert out.scale == np.float32(8.0034 / 60.0)
    from rvdd_release_amd.runtime import match_coeffs
    with pytest.raises(RuntimeError, match="rvdd_match_coeffs.*a must be"):
        match_coeffs(0.0, 0.0, 12, 3200)


def test_denoise_flag_rules():
    from rvdd_release_amd import denoise, noise
    assert "--match_noise" in denoise.__doc__ and "--match_iso" in denoise.__doc__ and "--match_iso" in noise.__doc__
    assert denoise._parse([]).match is None
    assert denoise._parse(["--match_noise", "60,15260", "--match_iso", "3200"]).match == (60.0, 15260.0, 3200)
    assert denoise._parse(["--match_noise", "auto", "--match_iso", "12800"]).match == (None, None, 12800)
    opt = denoise._parse(["--dpc", "4", "--dpc_noise", "auto", "--match_noise", "auto", "--match_iso", "3200", "--dpc_noise_frames", "2"])
    assert opt.dpc == (4.0, 4.0, None, None, 1.0) and opt.match == (None, None, 3200) and opt.dpc_noise_frames == 2
    for bad, what in ((["--match_noise", "60,15260"], "--match_noise needs --match_iso"), (["--match_noise", "auto"], "needs --match_iso"),
                      (["--match_iso", "3200"], "--match_iso belongs to --match_noise"),
                      (["--match_noise", "auto", "--match_iso", "6400"], "--match_iso must be one of"),
                      (["--match_noise", "60", "--match_iso", "3200"], "--match_noise takes a,b"),
                      (["--match_noise", "60,x", "--match_iso", "3200"], "--match_noise takes numbers"),
                      (["--match_noise", "auto,1", "--match_iso", "3200"], "--match_noise takes"),
                      (["--match_noise", "0,5", "--match_iso", "3200"], "a must be finite and > 0"),
                      (["--match_noise", "nan,5", "--match_iso", "3200"], "a must be finite and > 0"),
                      (["--match_noise", "3,inf", "--match_iso", "3200"], "b finite")):
        with pytest.raises(SystemExit, match=what):
            denoise._parse(bad)


def test_match_line_and_warning(capsys):
    """the `match:` line carries 17 digits and reads back to the same numbers; s > 1 adds the warning, s <= 1 does not"""
    import json
    from rvdd_release_amd import denoise
    cfg = denoise.match_report(60.0, 60.0 * 256 - 100, 12, 3200)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and out[0].startswith("match: {")
    d = json.loads(out[0][len("match: "):])
    want, s, t = _coeffs(60.0, 60.0 * 256 - 100, 12, 3200)
    assert d == {"scale": want.scale, "offset": want.offset, "s": s, "t_dn12": t, "iso": 3200}
    assert (cfg.scale, cfg.offset) == (want.scale, want.offset) and s < 1
    denoise.match_report(3.0, 3.0 * 256 - 100, 12, 12800)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and out[0].startswith("match: {") and "WARNING" in out[1] and "cleaner" in out[1] and "DESIGN.md 4.16" in out[1]
    assert "9.43" in out[1]                               # stretched by s = 28.3015 / 3
