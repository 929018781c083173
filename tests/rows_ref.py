"""The row-noise rule of include/rvdd.h (rvdd_rows_estimate, rvdd_rows_apply) restated in NumPy float32, every operation rounded on its
own, and the inputs the host and GPU tests share: tests/line_ref.py along the rows, plus what the rows alone have -- the clamp, its
state and the accumulator.  estimate() / apply() are vectorised; estimate_slow() / apply_slow() say the same with plain loops and
np.float32 scalars (tests/test_rows_host.py holds the two together word for word)."""
import numpy as np

import line_ref as L
from line_ref import dn, f32, gray_of, neighbour, norm_dn, packed_of, top_of      # noqa: F401 -- the tests read them here

DRS = L.OFFS
MAX_WW = 4096
SKIPPED, APPLIED, CLAMPED = L.SKIPPED, L.APPLIED, 2

# (n, hh, ww) of the GPU test: tests/test_gpu_rows.py says why each
SHAPES = [(1, 5, 1), (2, 6, 3), (1, 9, 64), (3, 7, 129), (1, 8, 640), (2, 6, 1030), (1, 5, 4096)]
CLASSES = L.CLASSES | {"clamped_pos", "clamped_neg"}


def cfg(k_gate, noise_a, noise_b, var_floor=1.0, max_dn=64.0):
    """the fields of struct rvdd_rows_cfg, as f32"""
    return L.cfg(k_gate, noise_a, noise_b, var_floor) + (f32(max_dn),)


def new_acc(n):
    return {"applied": np.zeros(n, np.uint32), "skipped": np.zeros(n, np.uint32), "clamped": np.zeros(n, np.uint32),
            "sum_q2": np.zeros(n, np.int64)}


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def deviations(packed, bits, c):
    """-> (d, used): every sample's d = x - median of its eight vertical neighbours, and whether the gate takes it"""
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and hh >= 5 and 1 <= ww <= MAX_WW
    return L.deviations(packed, bits, c, L.ROWS)


def _clamped(est, max_dn, acc):
    """the medians of `est` clamped to +-max_dn, state CLAMPED where that bit, and the rows counted per frame on top of `acc`"""
    o, state = est["offsets"], est["state"]
    acc = {k: v.copy() for k, v in acc.items()}
    for i, j, r in np.ndindex(*o.shape):
        if state[i, j, r] == SKIPPED:
            acc["skipped"][i] += 1
            continue
        oc = min(max(o[i, j, r], f32(-max_dn)), max_dn)
        state[i, j, r] = CLAMPED if oc != o[i, j, r] else APPLIED
        acc["applied"][i] += 1
        acc["clamped"][i] += int(oc != o[i, j, r])
        q = int(np.rint(f32(oc * f32(16.0))))
        acc["sum_q2"][i] += q * q
        o[i, j, r] = oc
    return dict(est, acc=acc)


def estimate(packed, bits, c, acc=None):
    """-> {"offsets": f32 [n,2,hh], "state": u8 [n,2,hh], "cnt": the used samples [n,2,hh], "acc": `acc` (None: zeros) plus the rows}"""
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and hh >= 5 and 1 <= ww <= MAX_WW
    return _clamped(L.estimate(packed, bits, c, L.ROWS), c[4], acc or new_acc(n))


def apply(packed, gray, offsets, bits):
    """-> (packed, gray) with the offsets [n,2,hh] taken out: copies; gray may be None"""
    return L.apply(packed, gray, L.spread(offsets, L.ROWS), bits)


# ---- the same, slowly ---------------------------------------------------------------------------------------------------------------
def estimate_slow(packed, bits, c):
    return _clamped(L.estimate_slow(packed, bits, c, L.ROWS), c[4], new_acc(packed.shape[0]))


def apply_slow(packed, gray, offsets, bits):
    return L.apply_slow(packed, gray, L.spread(offsets, L.ROWS), bits)


# ---- what fired ---------------------------------------------------------------------------------------------------------------------
def classes(est, ww):
    """the classes of CLASSES that an estimate holds"""
    o, st = est["offsets"], est["state"]
    got = L.classes(est, ww)
    got |= {"clamped_pos"} if ((st == CLAMPED) & (o > 0)).any() else set()
    got |= {"clamped_neg"} if ((st == CLAMPED) & (o < 0)).any() else set()
    return got


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def scene(n, hh, ww, seed, level=800.0, swing=600.0):
    """a smooth scene in DN, [n,4,hh,ww]: planes 0, 1 and 0.8 of them + 50 in planes 2, 3, moving a little from frame to frame"""
    return L.scene(n, hh, ww, seed, L.ROWS, level, swing)


def with_rows(clean, sigma, sigma_row, rng):
    """clean DN + white noise + one Gaussian offset per (frame, parity, row) -> (DN, the offsets [n,2,hh])"""
    return L.with_lines(clean, sigma, sigma_row, rng, L.ROWS)


def crafted(n, hh, ww, axis=L.ROWS):
    """line_ref.crafted's rows (row 1 of parity 0 applied on exactly ww used, row hh - 2 of parity 1 skipped on ww - 1) under a clamp
    of 8 DN, and a row 20 DN up and a row 20 DN down: inside the gate, beyond the clamp"""
    v = L.crafted(n, hh, ww, axis)
    v[0, 0:2, hh - 1, :] += 20.0                                           # parity 0, the last row: up
    v[0, 2:4, 0, :] -= 20.0                                                # parity 1, the first row: down
    return v


def cases(shape):
    """The inputs of one shape: [(name, packed f32 [n,4,hh,ww], bit depth, cfg)] -- line_ref.cases with a clamp each."""
    clamps = (4095.0 / 64.0, 0.75, 64.0, 64.0, 8.0)
    return [(name, packed, bits, c + (f32(m),)) for (name, packed, bits, c), m in zip(L.cases(shape, L.ROWS, crafted), clamps)]
