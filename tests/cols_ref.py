"""The column-noise rule of include/rvdd.h (rvdd_cols_estimate, rvdd_cols_fit, rvdd_cols_apply) restated in NumPy float32, every
operation rounded on its own, and the inputs the host and GPU tests share: tests/line_ref.py along the columns, plus what the columns
alone have -- the strips of the estimate kernel, the fit over the frames and the map's file order.  estimate() / fit() / apply() are
vectorised; estimate_slow() / fit_slow() / apply_slow() say the same with plain loops and np.float32 scalars (tests/test_cols_host.py
holds the two together word for word)."""
import numpy as np

import line_ref as L
from line_ref import CLASSES, cfg, classes, dn, f32, gray_of, neighbour, norm_dn, packed_of, top_of      # noqa: F401 -- the tests read them here

DCS = L.OFFS
MAX_HH = 4096
SKIPPED, APPLIED = L.SKIPPED, L.APPLIED
UNSUPPORTED, FIT_APPLIED, FIT_CLAMPED, INSIGNIFICANT = 0, 1, 2, 3
VAR_MEDIAN = f32(3.4528)                # (1.4826 * 1.2533)^2: the variance of a median in units of MAD^2
SE_MEDIAN = f32(1.2533) * f32(1.4826)   # the standard error of a median in units of MAD / sqrt(n)

# the strip widths the estimate kernel takes and the last hh of each (csrc/cols.hip: 4 CB (2 hh | 1) bytes within 160 KiB)
STRIPS = ((32, 639), (16, 1279), (8, 2559), (4, MAX_HH))
# (n, hh, ww) of the GPU test: tests/test_gpu_cols.py says why each
SHAPES = ([(1, 1, 5), (1, 3, 8), (2, 37, 53)] + [(1, 8, cb + e) for cb, _ in STRIPS for e in (-1, 0, 1) if cb + e >= 5]
          + [(1, hh + e, cb + 1) for cb, hh in STRIPS[:-1] for e in (0, 1)] + [(1, MAX_HH, 5), (1, 8, 640)])
SHAPES = sorted(set(SHAPES))


def strip_of(hh):
    return next(cb for cb, last in STRIPS if hh <= last)


def mosaic_of(cmap):
    """map [2,ww] -> one value per mosaic column [2 ww]: file[x] = map[x & 1][x >> 1]"""
    return np.ascontiguousarray(np.asarray(cmap).T).reshape(-1)


def map_of(line):
    """one value per mosaic column [W], W even -> map [2, W / 2]"""
    return np.ascontiguousarray(np.asarray(line).reshape(-1, 2).T)


def deviations(packed, bits, c):
    """-> (d, used): every sample's d = x - median of its eight horizontal neighbours, and whether the gate takes it"""
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and 1 <= hh <= MAX_HH and ww >= 5
    return L.deviations(packed, bits, c, L.COLS)


def estimate(packed, bits, c):
    """-> {"offsets": f32 [n,2,ww], "state": u8 [n,2,ww], "cnt": the used samples [n,2,ww]}"""
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and 1 <= hh <= MAX_HH and ww >= 5
    return L.estimate(packed, bits, c, L.COLS)


def fit(offsets, state, min_frames, k_sig, max_dn):
    """-> {"map": f32 [2,ww], "mstate": u8 [2,ww], "stats": the counts by state, sum_q2 and floor_dn}"""
    F, _, ww = offsets.shape
    k_sig, max_dn = f32(k_sig), f32(max_dn)
    cmap = np.zeros((2, ww), np.float32)
    mstate = np.zeros((2, ww), np.uint8)
    counts, sum_q2, floor_sum, supported = [0, 0, 0, 0], 0, 0.0, 0
    for j in range(2):
        for col in range(ww):
            v = np.sort(offsets[:, j, col][state[:, j, col] == APPLIED])
            nf = v.size
            if nf < max(1, min_frames):
                counts[UNSUPPORTED] += 1
                continue
            o = (v[(nf - 1) // 2] + v[nf // 2]) * f32(0.5)
            a = np.sort(np.abs(v - o))
            mad = (a[(nf - 1) // 2] + a[nf // 2]) * f32(0.5)
            floor_sum += float((SE_MEDIAN * mad) / np.sqrt(f32(nf)))
            supported += 1
            if (o * o) * f32(nf) < (k_sig * k_sig) * (VAR_MEDIAN * (mad * mad)):
                mstate[j, col] = INSIGNIFICANT
                counts[INSIGNIFICANT] += 1
                continue
            oc = np.minimum(np.maximum(o, -max_dn), max_dn)
            cmap[j, col] = oc
            mstate[j, col] = FIT_CLAMPED if oc != o else FIT_APPLIED
            counts[int(mstate[j, col])] += 1
            q = int(np.rint(f32(16.0) * oc))
            sum_q2 += q * q
    stats = {"unsupported": counts[0], "applied": counts[1], "clamped": counts[2], "insignificant": counts[3], "sum_q2": sum_q2,
             "floor_dn": floor_sum / supported if supported else 0.0}
    return {"map": cmap, "mstate": mstate, "stats": stats}


def apply(packed, gray, cmap, bits):
    """-> (packed, gray) with the map [2,ww] taken out: copies; gray may be None"""
    return L.apply(packed, gray, L.spread(cmap, L.COLS), bits)


# ---- the same, slowly ---------------------------------------------------------------------------------------------------------------
def estimate_slow(packed, bits, c):
    return L.estimate_slow(packed, bits, c, L.COLS)


def fit_slow(offsets, state, min_frames, k_sig, max_dn):
    F, _, ww = offsets.shape
    k_sig, max_dn = f32(k_sig), f32(max_dn)
    k2 = f32(k_sig * k_sig)
    cmap = np.zeros((2, ww), np.float32)
    mstate = np.zeros((2, ww), np.uint8)
    counts, sum_q2, floor_sum, supported = [0, 0, 0, 0], 0, 0.0, 0
    for j in range(2):
        for col in range(ww):
            v = sorted(f32(offsets[i, j, col]) for i in range(F) if state[i, j, col] == APPLIED)
            nf = len(v)
            if nf < max(1, min_frames):
                counts[0] += 1
                continue
            o = f32(f32(v[(nf - 1) // 2] + v[nf // 2]) * f32(0.5))
            a = sorted(f32(abs(f32(x - o))) for x in v)
            mad = f32(f32(a[(nf - 1) // 2] + a[nf // 2]) * f32(0.5))
            floor_sum += float(f32(f32(SE_MEDIAN * mad) / f32(np.sqrt(f32(nf)))))
            supported += 1
            if f32(f32(o * o) * f32(nf)) < f32(k2 * f32(VAR_MEDIAN * f32(mad * mad))):
                mstate[j, col] = INSIGNIFICANT
                counts[3] += 1
                continue
            oc = min(max(o, f32(-max_dn)), max_dn)
            cmap[j, col] = oc
            mstate[j, col] = FIT_CLAMPED if oc != o else FIT_APPLIED
            counts[int(mstate[j, col])] += 1
            q = int(np.rint(f32(f32(16.0) * oc)))
            sum_q2 += q * q
    stats = {"unsupported": counts[0], "applied": counts[1], "clamped": counts[2], "insignificant": counts[3], "sum_q2": sum_q2,
             "floor_dn": floor_sum / supported if supported else 0.0}
    return {"map": cmap, "mstate": mstate, "stats": stats}


def apply_slow(packed, gray, cmap, bits):
    return L.apply_slow(packed, gray, L.spread(cmap, L.COLS), bits)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def scene(n, hh, ww, seed, level=800.0, swing=600.0):
    """a smooth scene in DN, [n,4,hh,ww]: planes 0, 2 and 0.8 of them + 50 in planes 1, 3, moving a little from frame to frame"""
    return L.scene(n, hh, ww, seed, L.COLS, level, swing)


def with_cols(clean, sigma, sigma_col, rng):
    """clean DN + white noise + one static Gaussian offset per (parity, column) -> (DN, the offsets [2,ww])"""
    return L.with_lines(clean, sigma, sigma_col, rng, L.COLS)


def crafted(n, hh, ww):
    """line_ref.crafted's columns: column 1 of parity 0 applied on exactly hh used, column ww - 2 of parity 1 skipped on hh - 1"""
    return L.crafted(n, hh, ww, L.COLS)


def cases(shape):
    """The inputs of one shape: [(name, packed f32 [n,4,hh,ww], bit depth, cfg)] -- tests/rows_ref.py's five, transposed."""
    return L.cases(shape, L.COLS)


def fit_cfg_for(bits, frames):
    """the fit the tests pool a shape's frames with: half the frames, three standard errors, top / 64"""
    return max(1, frames // 2), 3.0, float(top_of(bits)) / 64.0
