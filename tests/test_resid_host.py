"""Residual statistics without a device: the NumPy restatement (tests/resid_ref.py) hits every class of sample on the shapes the GPU
test compares it on, reads white noise of a known curve as ratio 1, zero correlation and zero bias, and rvdd_resid_fit -- host code of
the library, no device needed -- is the Python restatement of its header to 1e-12."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bayer_ref
import resid_ref as R
from conftest import REPO

ISO3200 = (8.0034, 2043.51144)                            # the project's own curve, 12-bit DN
QUIET = (0.02, 0.0)                                       # sigma 6 DN at mid-range: the mean of 98304 samples is known to 0.02 DN


def _lib():
    from rvdd_release_amd import _lib
    return _lib


# ---- 1. the reference alone meets every class -----------------------------------------------------------------------------------
def test_the_cases_hold_every_class():
    seen = set()
    for k, (n, hh, ww) in enumerate(R.SHAPES):
        for bits in R.BIT_DEPTHS:
            for pattern in range(4):
                _, _, classes = R.make_case(n, hh, ww, bits, pattern, seed=10 * k + pattern)
                assert "clamped" in classes and "negative" in classes and "edge_pair" in classes, ((n, hh, ww), bits, pattern, classes)
                assert ("batch" in classes) == (n > 1) and ("pairs" in classes) == (ww > 1)
                if hh * ww >= 256:
                    assert "many_bins" in classes, ((n, hh, ww), bits, pattern, classes)
                seen |= classes
    _, _, flat = R.make_case(2, 16, 24, 12, 0, seed=3, flat=True)
    assert "flat" in flat and "many_bins" not in flat and "clamped" not in flat
    seen |= flat
    assert seen == {"flat", "many_bins", "clamped", "negative", "edge_pair", "pairs", "batch"}, seen


def test_remosaic_is_the_demosaic_modules_remosaic():
    import torch
    rgb = np.random.default_rng(1).normal(size=(2, 3, 6, 10)).astype(np.float32)
    for p, name in enumerate(R.PATTERNS):
        assert R.PATTERNS == bayer_ref.PATTERNS
        assert np.array_equal(R.remosaic(rgb, p), bayer_ref.remosaick(torch.from_numpy(rgb), name).numpy()), name


def test_sums_are_the_loops():
    """the vectorised restatement against the rule written as loops over samples, on a case small enough for that"""
    n, hh, ww, bits, pattern = 2, 3, 5, 12, 2
    packed, rgb, _ = R.make_case(n, hh, ww, bits, pattern, seed=4)
    got = R.resid_ref(packed, rgb, pattern, bits)
    f = np.float32
    top, S = f(4095), f(8)
    want = R.new_acc(n)
    def one(i, k, y, x):
        c = ((packed[i, k, y, x] + f(1)) * f(0.5)) * top
        d = ((rgb[i, R.col(pattern, k), 2 * y + (k >> 1), 2 * x + (k & 1)] + f(1)) * f(0.5)) * top
        rq = int(min(max(int(np.rint((c - d) * S)), -2 ** 17), 2 ** 17))
        dc = min(max(d, f(0)), top)
        return rq, min(int(dc * f(1 / 64)), 63), int(np.rint(dc * f(16)))
    for i in range(n):
        for k in range(4):
            for y in range(hh):
                for x in range(ww):
                    rq, j, mq = one(i, k, y, x)
                    want["n"][i, j] += np.uint64(1); want["msum"][i, j] += np.uint64(mq); want["s1"][i, j] += rq; want["s2"][i, j] += np.uint64(rq * rq)
                    if x < ww - 1:
                        want["n11"][i, j] += np.uint64(1); want["s11"][i, j] += rq * one(i, k, y, x + 1)[0]
    for name in R.FIELDS:
        assert np.array_equal(got[name], want[name]), name
    # accumulation: onto a start that is not zero, and a batch is its frames
    start = {name: np.full((n, 64), 7, got[name].dtype) for name in R.FIELDS}
    onto = R.resid_ref(packed, rgb, pattern, bits, acc=start)
    for name in R.FIELDS:
        assert np.array_equal(onto[name], got[name] + got[name].dtype.type(7)), name
        for i in range(n):
            assert np.array_equal(R.resid_ref(packed[i:i + 1], rgb[i:i + 1], pattern, bits)[name][0], got[name][i]), (name, i)


# ---- 2. white noise of a known curve ---------------------------------------------------------------------------------------------
HH, WW = 128, 192


@pytest.mark.parametrize("curve", [ISO3200, QUIET], ids=["iso3200", "quiet"])
def test_white_noise_of_a_known_curve_reads_as_one(curve):
    """The clean frame in as rgb, white Gaussian noise of the curve around it: ratio within 2 % of 1, |rho| < 0.01, and the bias
    within 0.1 DN -- where the noise allows that: the mean of N = 98304 samples of variance v is known to sqrt(v / N), which for the
    ISO 3200 curve (sigma 118 DN at mid-range) is 0.38 DN.  There the bound is four standard errors of the mean, worked out from the
    curve, not from the result; for the quiet curve it is the 0.1 DN as stated.  The reference meets all of them (checked before they
    were fixed: ratio 1.0014 / 1.0015, ratio_lo 0.995, ratio_hi 1.003, rho 0.0059 / 0.0059, bias -0.15 / -0.007 DN).  With the noise scaled by sqrt(2) the ratio doubles."""
    a, b = curve
    rgb = R.ramp_rgb(HH, WW, 12)
    clean = (R.remosaic(rgb, 0).astype(np.float64) + 1) * 0.5 * 4095
    se = math.sqrt(float(np.maximum(a * clean - b, 0).mean()) / clean.size)
    bias_bound = max(0.1, 4 * se)
    assert (bias_bound == 0.1) == (curve == QUIET)
    for gain, want in ((1.0, 1.0), (math.sqrt(2.0), 2.0)):
        packed = R.noisy_of(rgb, 0, 12, a, b, seed=11, gain=gain)
        rep = R.fit_ref(R.total(R.resid_ref(packed, rgb, 0, 12)), 12, a, b)
        print(curve, gain, {k: rep[k] for k in ("ratio", "ratio_lo", "ratio_hi", "rho", "bias", "a_fit", "b_fit", "bins")})
        assert rep["bins"] >= 40 and 0.98 * 4 * HH * WW <= rep["samples"] <= 4 * HH * WW      # the ramp's end bins are thin
        for key in ("ratio", "ratio_lo", "ratio_hi"):
            lim = 0.02 if key == "ratio" else 0.02 * math.sqrt(3)          # a third of the samples: sqrt(3) of the spread
            assert abs(rep[key] / want - 1) < lim, (key, rep[key], want)
        assert abs(rep["rho"]) < 0.01, rep["rho"]
        assert abs(rep["bias"]) < bias_bound * gain, (rep["bias"], bias_bound)
        assert abs(rep["a_fit"] / (want * a) - 1) < 0.05, (rep["a_fit"], a)


def test_the_deviations_read_as_the_header_says():
    """noise left in the output lowers the ratio; detail removed raises it together with rho; a level shift is the bias"""
    a, b = ISO3200
    rgb = R.ramp_rgb(HH, WW, 12)
    packed = R.noisy_of(rgb, 0, 12, a, b, seed=5)
    fit = lambda p, r: R.fit_ref(R.total(R.resid_ref(p, r, 0, 12)), 12, a, b)
    # half of the noise stays in the output: the residual is the other half, a quarter of the variance
    mosaic = R.remosaic(rgb, 0)
    left = rgb.copy()
    for k in range(4):
        left[:, R.col(0, k), (k >> 1)::2, (k & 1)::2] = mosaic[:, k] + np.float32(0.5) * (packed[:, k] - mosaic[:, k])
    assert abs(fit(packed, left)["ratio"] - 0.25) < 0.01
    # detail the output lacks: a smooth pattern in the noisy frame only
    # (along y: the levels ramp along x, and what is constant inside a level bin is that bin's mean, not its variance)
    y = np.arange(HH, dtype=np.float64)
    detail = (0.08 * np.sin(2 * np.pi * y / 24.0)).astype(np.float32)
    other = np.float32(1) + np.float32(0.02) * np.sin(np.arange(WW) / 5.0).astype(np.float32)      # not the same in every column
    rep = fit(packed + detail[None, None, :, None] * other[None, None, None, :], rgb)
    assert rep["ratio"] > 1.5 and rep["rho"] > 0.2, rep
    # the black level off by 16 DN
    rep = fit(packed + np.float32(2 * 16 / 4095.0), rgb)
    assert abs(rep["bias"] - 16) < 1.5 and abs(rep["ratio"] - 1) < 0.03, rep


# ---- 3. rvdd_resid_fit is the restatement -------------------------------------------------------------------------------------------
def _call_fit(acc, bits, a, b, out=None, null_acc=False, null_out=False):
    L = _lib()
    lib = L.load()
    host = L.RvddResidAcc.from_buffer_copy(R.acc_bytes(acc))
    out = L.RvddResidReport() if out is None else out
    rc = lib.rvdd_resid_fit(None if null_acc else C.byref(host), bits, a, b, None if null_out else C.byref(out))
    return rc, out, lib.rvdd_last_error(None).decode()


def test_fit_is_the_python_restatement():
    a, b = ISO3200
    rgb = R.ramp_rgb(HH, WW, 12)
    cases = [(R.total(R.resid_ref(R.noisy_of(rgb, p, 12, a, b, seed=20 + p, gain=g), rgb, p, 12)), 12, a * s, b * s)
             for p, g, s in ((0, 1.0, 1.0), (1, 0.7, 1.0), (2, 1.3, 2.0), (3, 1.0, 0.5))]
    # other bit depths, and sums that are negative or have wrapped
    for bits in (10, 16):
        k = (2 ** bits - 1) / 4095.0
        r = R.ramp_rgb(HH, WW, bits)
        cases.append((R.total(R.resid_ref(R.noisy_of(r, 0, bits, k * a, k * k * b, seed=bits), r + np.float32(0.01), 0, bits)), bits, k * a, k * k * b))
    packed, out, _ = R.make_case(3, 64, 96, 12, 2, seed=9)
    cases.append((R.total(R.resid_ref(packed, out, 2, 12)), 12, 1.0, -50.0))
    for acc, bits, ca, cb in cases:
        want = R.fit_ref(acc, bits, ca, cb)
        rc, got, msg = _call_fit(acc, bits, ca, cb)
        assert want is not None and rc == 0, (rc, msg)
        assert got.samples == want["samples"] and got.bins == want["bins"] and got.reserved == 0
        for key in ("ratio", "ratio_lo", "ratio_hi", "bias", "rho", "a_fit", "b_fit"):
            g, w = getattr(got, key), want[key]
            assert math.isfinite(w) and abs(g - w) <= 1e-12 * abs(w), (key, g, w)
    from rvdd_release_amd.runtime import resid_fit
    acc, bits, ca, cb = cases[0]
    assert resid_fit(acc, bits, ca, cb) == {k: getattr(_call_fit(acc, bits, ca, cb)[1], k) for k in R.fit_ref(acc, bits, ca, cb)}


def test_fit_errors_leave_out_untouched():
    L = _lib()
    a, b = ISO3200
    rgb = R.ramp_rgb(HH, WW, 12)
    acc = R.total(R.resid_ref(R.noisy_of(rgb, 0, 12, a, b, seed=1), rgb, 0, 12))
    mark = lambda: L.RvddResidReport(*([7.5] * 7), 7, 7, 7)
    untouched = lambda o: [getattr(o, k) for k, _ in L.RvddResidReport._fields_] == [7.5] * 7 + [7, 7, 7]
    for kwargs, code, word in ((dict(null_acc=True), -1, "acc_host"), (dict(null_out=True), -1, "out"), (dict(bits=0), -1, "bit_depth"),
                               (dict(bits=17), -1, "bit_depth"), (dict(a=float("nan")), -1, r"\ba\b"), (dict(b=float("inf")), -1, r"\bb\b")):
        out = mark()
        args = dict(bits=12, a=a, b=b)
        args.update({k: v for k, v in kwargs.items() if k in args})
        rc, out, msg = _call_fit(acc, args["bits"], args["a"], args["b"], out, kwargs.get("null_acc", False), kwargs.get("null_out", False))
        assert rc == code and msg.startswith("rvdd_resid_fit:") and re.search(word, msg) and untouched(out), (kwargs, rc, msg)
    # RVDD_ERR_STATE: three usable bins; a curve that predicts no noise anywhere; an empty accumulator
    three = {k: v.copy() for k, v in acc.items()}
    keep = np.flatnonzero(three["n"] >= 1024)[:3]
    for k in three:
        rest = np.ones(64, bool)
        rest[keep] = False
        three[k][rest] = 0
    for bad, ca, cb in ((three, a, b), (acc, a, 1e9), (R.total(R.new_acc(1)), a, b)):
        rc, out, msg = _call_fit(bad, 12, ca, cb, mark())
        assert rc == -2 and msg.startswith("rvdd_resid_fit:") and "usable" in msg and untouched(out), (rc, msg)
        assert R.fit_ref(bad, 12, ca, cb) is None
    four = {k: v.copy() for k, v in acc.items()}
    keep = np.flatnonzero(four["n"] >= 1024)[:4]
    for k in four:
        rest = np.ones(64, bool)
        rest[keep] = False
        four[k][rest] = 0
    assert _call_fit(four, 12, a, b)[0] == 0 and R.fit_ref(four, 12, a, b)["bins"] == 4


# ---- 4. the struct ------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    text = open(os.path.join(REPO, "include", "rvdd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"\s*(uint64_t|int64_t|int32_t|double)\s+(.*)", decl.strip(), re.S)
        if m:
            for item in m.group(2).split(","):
                nm = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", item)
                fields.append((nm.group(1), m.group(1), int(nm.group(2) or 1)))
    return fields


def test_struct_layouts_match_the_header():
    L = _lib()
    size = {"uint64_t": 8, "int64_t": 8, "int32_t": 4, "double": 8}
    ctype = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    for name, cls, total in (("rvdd_resid_acc", L.RvddResidAcc, 3072), ("rvdd_resid_report", L.RvddResidReport, 72)):
        fields = _header_struct(name)
        assert [f for f, _, _ in fields] == [f for f, _ in cls._fields_], name
        at = 0
        for (fname, ftype, count), (_, ct) in zip(fields, cls._fields_):
            assert getattr(cls, fname).offset == at and C.sizeof(ct) == size[ftype] * count, (name, fname)
            assert (ct._type_ if count > 1 else ct) is ctype[ftype], (name, fname)
            at += size[ftype] * count
        assert at == total == C.sizeof(cls), (name, at)
    assert R.ACC_BYTES == 3072 and tuple(f for f, _ in L.RvddResidAcc._fields_) == R.FIELDS
    from rvdd_release_amd.runtime import RESID_ACC_BYTES, resid_acc_arrays
    assert RESID_ACC_BYTES == 3072
    acc = R.resid_ref(*R.make_case(2, 4, 6, 12, 1, seed=2)[:2], 1, 12)
    back = resid_acc_arrays(R.acc_bytes(acc, 0) + R.acc_bytes(acc, 1))
    for name in R.FIELDS:
        assert back[name].dtype == acc[name].dtype and np.array_equal(back[name], acc[name]), name
