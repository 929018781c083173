"""The row-noise rule on the CPU: tests/rows_ref.py's vectorised restatement against its scalar one word for word, the classes of rows
the shared inputs must reach, what the rule does to Gaussian row offsets under white noise, and the host side of the binding."""
import ctypes as C

import numpy as np
import pytest

import rows_ref as R


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_estimate(a, b, what):
    assert np.array_equal(_bits(a["offsets"]), _bits(b["offsets"])), (what, "offsets")
    assert np.array_equal(a["state"], b["state"]) and np.array_equal(a["cnt"], b["cnt"]), (what, "state / cnt")
    for k in a["acc"]:
        assert a["acc"][k].dtype == b["acc"][k].dtype and np.array_equal(a["acc"][k], b["acc"][k]), (what, k)


@pytest.mark.parametrize("shape", [(1, 5, 1), (2, 6, 3), (1, 9, 7)], ids=lambda s: "%dx%dx%d" % s)
def test_the_restatement_is_its_scalar_form(shape):
    seen = set()
    for name, packed, bits, c in R.cases(shape):
        fast, slow = R.estimate(packed, bits, c), R.estimate_slow(packed, bits, c)
        _same_estimate(fast, slow, (shape, name))
        gray = R.gray_of(packed, bits)
        gray[:, ::2] = 7.0                                      # what a row that is not rewritten must keep
        pf, gf = R.apply(packed, gray, fast["offsets"], bits)
        ps, gs = R.apply_slow(packed, gray, fast["offsets"], bits)
        assert np.array_equal(_bits(pf), _bits(ps)) and np.array_equal(_bits(gf), _bits(gs)), (shape, name)
        keep = (fast["offsets"] == 0).all(axis=1)
        assert np.array_equal(_bits(gf[keep]), _bits(gray[keep]))
        seen |= R.classes(fast, shape[2])
    assert {"applied", "skipped"} <= seen, seen


def test_neighbours_are_mirrored_about_the_site_and_stay_inside():
    for hh in range(5, 20):
        for r in range(hh):
            for dr in R.DRS:
                q = R.neighbour(r, dr, hh)
                assert 0 <= q < hh, (hh, r, dr, q)
                if 0 <= r + dr < hh:
                    assert q == r + dr
                elif 0 <= r - dr < hh:
                    assert q == r - dr                              # the rule as stated; from nine rows on one of the two is inside
        assert hh < 9 or all(0 <= r + dr < hh or 0 <= r - dr < hh for r in range(hh) for dr in R.DRS)


def test_every_class_fires_on_the_inputs_of_the_gpu_test():
    seen, per_case = set(), {}
    for shape in R.SHAPES:
        for name, packed, bits, c in R.cases(shape):
            got = R.classes(R.estimate(packed, bits, c), shape[2])
            per_case.setdefault(name, set()).update(got)
            seen |= got
    assert seen == R.CLASSES, R.CLASSES - seen
    # each input is there for a reason
    assert {"clamped_pos", "clamped_neg", "half", "half_minus_one", "zero"} <= per_case["crafted"], per_case["crafted"]
    assert {"empty", "skipped"} <= per_case["step"], per_case["step"]
    assert per_case["constant"] == {"applied", "zero", "even"}, per_case["constant"]
    assert {"applied", "even", "odd"} <= per_case["scene12"] and {"applied", "zero"} <= per_case["bits4"]
    # a constant frame is a bit copy, and its gray plane is not written
    _, packed, bits, c = [x for x in R.cases((2, 6, 3)) if x[0] == "constant"][0]
    est = R.estimate(packed, bits, c)
    poison = np.full((2, 6, 3), 7.0, np.float32)
    out, gray = R.apply(packed, poison, est["offsets"], bits)
    assert np.array_equal(_bits(out), _bits(packed)) and (gray == 7.0).all()


# ---- what the rule does to row noise ------------------------------------------------------------------------------------------------
SIGMA, HH, WW = 30.0, 180, 320


def _highpassed_row_error(frame, clean):
    """the std over the rows of the row-wise median of (frame - clean) per parity, a 9-row moving average of it taken out (the rows
    that have all nine)"""
    err = np.median(np.concatenate([frame[:, 0::2] - clean[:, 0::2], frame[:, 1::2] - clean[:, 1::2]], axis=3), axis=3)[0]      # [2,hh]
    hp = [e[4:-4] - np.convolve(e, np.ones(9) / 9.0, mode="valid") for e in err]
    return float(np.std(np.concatenate(hp)))


def _statistical_case(sigma_row):
    rng = np.random.default_rng(20261020)
    y, x = np.mgrid[0:HH, 0:WW].astype(np.float64)
    base = 800.0 + 600.0 * np.sin(x / 37.0) * np.cos(y / 23.0) + 2.0 * y
    clean = np.stack([base, 0.8 * base + 50.0, base, 0.8 * base + 50.0])[None]
    noisy, _ = R.with_rows(clean, SIGMA, sigma_row, rng)
    top = R.top_of(12)
    packed = R.norm_dn(noisy.astype(np.float32), top)
    c = R.cfg(3.0, 0.0, -SIGMA * SIGMA, 1.0, 4095.0 / 64.0)
    est = R.estimate(packed, 12, c)
    out, _ = R.apply(packed, None, est["offsets"], 12)
    before = _highpassed_row_error(R.dn(packed, top).astype(np.float64), clean)
    after = _highpassed_row_error(R.dn(out, top).astype(np.float64), clean)
    return before, after, est


def test_row_noise_is_halved_and_clean_footage_is_left_alone():
    before, after, est = _statistical_case(10.0)
    print("sigma_row = 10: high-passed row error %.3f -> %.3f DN (ratio %.3f)" % (before, after, after / before))
    assert (est["state"] != R.SKIPPED).all()
    assert after <= 0.5 * before, (before, after)
    before0, after0, est0 = _statistical_case(0.0)
    rms0 = float(np.sqrt((est0["offsets"].astype(np.float64) ** 2).mean()))
    print("sigma_row = 0: high-passed row error %.3f -> %.3f DN (+%.4f sigma); rms offset %.3f DN" % (before0, after0, (after0 - before0) / SIGMA, rms0))
    assert after0 - before0 < 0.1 * SIGMA, (before0, after0)
    # The rms the estimate has of its own on FLAT footage: 1.35 sqrt(var / (2 ww)) (runtime.rows_floor_rms says where 1.35 comes from);
    # 360 rows give an rms to 1 / sqrt(2 * 360) = 4 %, so 15 % is four standard deviations.  The scene above adds its own curvature
    # to every d, so its offsets are larger than the floor: a user's rms is read against the floor as "at or near", not "equal".
    from rvdd_release_amd.runtime import rows_floor_rms
    floor = rows_floor_rms(0.0, -SIGMA * SIGMA, 1.0, 12, WW)
    flat, _ = R.with_rows(np.full((1, 4, HH, WW), 1000.0), SIGMA, 0.0, np.random.default_rng(3))
    est = R.estimate(R.norm_dn(flat.astype(np.float32), R.top_of(12)), 12, R.cfg(3.0, 0.0, -SIGMA * SIGMA, 1.0, 64.0))
    rms_flat = float(np.sqrt((est["offsets"].astype(np.float64) ** 2).mean()))
    print("flat frame: rms offset %.3f DN, floor %.3f DN" % (rms_flat, floor))
    assert abs(floor - 1.35 * SIGMA / np.sqrt(2 * WW)) < 1e-9 and 0.85 < rms_flat / floor < 1.15, (rms_flat, floor)
    assert floor <= rms0 < 2.0 * floor, (rms0, floor)


# ---- the binding's host side --------------------------------------------------------------------------------------------------------
def test_structs_and_accumulator_arrays():
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import ROWS_ACC_BYTES, rows_acc_arrays, rows_add, rows_cfg, rows_rms
    assert C.sizeof(_lib.RvddRowsCfg) == 20 and ROWS_ACC_BYTES == 24 and _lib.RvddRowsAcc.sum_q2.offset == 16
    c = rows_cfg(3, 8.0, 2043.5, max_dn=12.5)
    assert (c.k_gate, c.noise_a, c.noise_b, c.var_floor, c.max_dn) == (3.0, 8.0, 2043.5, 1.0, 12.5)
    one = _lib.RvddRowsAcc(5, 2, 1, 0, -3)
    a = rows_acc_arrays(one)
    assert [int(a[k][0]) for k in ("applied", "skipped", "clamped", "sum_q2")] == [5, 2, 1, -3] and a["sum_q2"].dtype == np.int64
    two = rows_acc_arrays(bytes(one) + bytes(_lib.RvddRowsAcc(1, 0, 0, 0, 256 * 4)))
    assert two["applied"].tolist() == [5, 1] and two["sum_q2"].tolist() == [-3, 1024]
    s = rows_add(rows_acc_arrays(_lib.RvddRowsAcc(3, 0, 0, 0, 256 * 3)), rows_acc_arrays(_lib.RvddRowsAcc(1, 1, 0, 0, 256)))
    assert rows_rms(s) == 1.0 and rows_rms(rows_acc_arrays(_lib.RvddRowsAcc())) == 0.0
    with pytest.raises(RuntimeError, match="24 bytes"):
        rows_acc_arrays(b"\0" * 25)
