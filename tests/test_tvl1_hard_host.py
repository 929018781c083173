"""The hard TV-L1 pairs (hard_pairs.py) on the CPU: every case's class is recomputed from the oracle's spread under one ulp of
its inputs, the pinned set keeps the coverage that it exists for, and the oracle is held to the reference library's flows
(tests/golden/tvl1_hard.npz; live against oracle/_ref/libBridge.so where that build exists) on every pinned case."""
import ctypes
import functools
import os

import numpy as np
import pytest

import hard_pairs as HP
import tvl1_oracle as T
from conftest import GOLDEN, REPO

REF_LIB = os.path.join(REPO, "oracle", "_ref", "libBridge.so")


@functools.lru_cache(maxsize=None)
def _spread(key):
    return HP.spread(*HP.case_pair(key), until_chaotic=True)


@pytest.mark.parametrize("key", list(HP.CASES))
def test_class_of_every_case_is_what_the_spread_says(key):
    gen, h, w, _, cls = HP.CASES[key]
    assert gen in HP.NAMES and 16 <= h <= 90 and 16 <= w <= 160
    mx, mean, totals = _spread(key)
    got = HP.PINNED if HP.is_pinned(mx, mean, totals) else HP.CHAOTIC
    assert got == cls, (key, cls, mx, mean, totals)
    assert totals[0] == sum(HP.case_oracle(key)[1])


def test_case_list_covers_what_it_is_for():
    pinned, chaotic = HP.pinned_cases(), HP.chaotic_cases()
    assert len(pinned) >= 12 and len(chaotic) >= 3
    assert set(HP.ZERO_CASES) | set(HP.CAP_CASES) <= set(pinned) and len(HP.CAP_CASES) >= 2
    sizes = lambda keys: {HP.CASES[k][1:3] for k in keys}
    assert {(22, 22), (48, 64), (41, 75)} <= sizes(pinned) and {(48, 64), (41, 75)} <= sizes(chaotic)
    assert any(HP.CASES[k][2] > 64 for k in pinned)                      # two patches across
    assert {HP.CASES[k][0] for k in HP.CASES} >= set(HP.NAMES)           # a candidate that misses the condition is listed, not dropped
    flows = {k: HP.case_oracle(k) for k in pinned}
    flat = [k for k in pinned if k not in HP.ZERO_CASES and HP.flat_fraction(*HP.case_pair(k), flows[k][0]) > 0.10]
    far = [k for k in pinned if np.abs(flows[k][0]).max() > 10.0]
    at_one = [k for k in pinned if 1 in flows[k][1]]
    at_cap = [k for k in pinned if T.MAX_ITERATIONS in flows[k][1]]
    between = [k for k in pinned if 1 in flows[k][1] and max(flows[k][1]) > 50]      # a loop stops at 1 after the scale did real work
    assert flat and far and between and len(at_one) >= 3 and len(at_cap) >= 2, (flat, far, at_one, at_cap, between)
    # the cap next to horizontal exchange: chaotic in the reference itself, kept for the equivalence tests
    gen, h, w, _, cls = HP.CASES["cap_wide_30x90"]
    assert w > 64 and cls == HP.CHAOTIC and HP.case_oracle("cap_wide_30x90")[1][-5] == T.MAX_ITERATIONS      # the finest scale's first loop


def test_oracle_matches_the_reference_library_on_every_pinned_case():
    want = HP.load_hard(GOLDEN)
    assert sorted(want) == sorted(HP.pinned_cases())
    for key in HP.pinned_cases():
        u = HP.case_oracle(key)[0]
        assert want[key].dtype == np.float32 and want[key].shape == u.shape and np.isfinite(want[key]).all(), key
        HP.close(u, want[key], key)


@pytest.mark.parametrize("key", HP.ZERO_CASES)
def test_oracle_flow_of_a_static_pair_is_exactly_zero(key):
    u, counts = HP.case_oracle(key)
    assert not u.any() and counts == (1,) * (5 * HP.num_scales(key)), (key, counts)


@pytest.mark.parametrize("key", HP.CAP_CASES)
def test_oracle_cap_cases_run_into_the_cap_whatever_the_last_bit(key):
    I0, I1 = HP.case_pair(key)
    counts = HP.case_oracle(key)[1]
    assert T.MAX_ITERATIONS in counts and max(counts) == T.MAX_ITERATIONS, counts
    for d in range(3):
        assert tuple(HP.oracle(HP.ulp_perturbed(I0, 100 + d), HP.ulp_perturbed(I1, 100 + d))[1]) == counts, (key, d)


def test_ulp_perturbed_moves_every_pixel_by_one_ulp():
    I0, _ = HP.case_pair("shift12_48x64")
    P = HP.ulp_perturbed(I0, 5)
    assert P.dtype == np.float32 and np.array_equal(HP.ulp_perturbed(I0, 5), P)
    up = P > I0
    assert ((P != I0).all() and 0.4 < up.mean() < 0.6 and np.array_equal(P[up], np.nextafter(I0[up], np.float32(np.inf)))
            and np.array_equal(P[~up], np.nextafter(I0[~up], np.float32(-np.inf))))


def test_live_reference_library_still_computes_the_fixture():
    """Where oracle/_ref has been built from the reference's sources."""
    if not os.path.exists(REF_LIB):
        return
    lib = ctypes.CDLL(REF_LIB)
    lib.tvl1flow.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2
    lib.tvl1flow.restype = None
    want = HP.load_hard(GOLDEN)
    for key in HP.pinned_cases():
        I0, I1 = HP.case_pair(key)
        h, w = I0.shape
        u = np.zeros(2 * h * w, np.float32)
        lib.tvl1flow(I0.ctypes.data, I1.ctypes.data, u.ctypes.data, w, h)
        HP.close(u.reshape(2, h, w), want[key], key)
