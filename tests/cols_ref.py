"""The column-noise rule of include/rvdd.h (rvdd_cols_estimate, rvdd_cols_fit, rvdd_cols_apply) restated in NumPy float32, every
operation rounded on its own, and the inputs the host and GPU tests share.  estimate() / fit() / apply() are vectorised;
estimate_slow() / fit_slow() / apply_slow() say the same with plain loops and np.float32 scalars (tests/test_cols_host.py holds the two
together word for word).  The transpose of tests/rows_ref.py."""
import numpy as np

f32 = np.float32
DCS = (-4, -3, -2, -1, 1, 2, 3, 4)
MAX_HH = 4096
SKIPPED, APPLIED = 0, 1
UNSUPPORTED, FIT_APPLIED, FIT_CLAMPED, INSIGNIFICANT = 0, 1, 2, 3
VAR_MEDIAN = f32(3.4528)                # (1.4826 * 1.2533)^2: the variance of a median in units of MAD^2
SE_MEDIAN = f32(1.2533) * f32(1.4826)   # the standard error of a median in units of MAD / sqrt(n)

# the strip widths the estimate kernel takes and the last hh of each (csrc/cols.hip: 4 CB (2 hh | 1) bytes within 160 KiB)
STRIPS = ((32, 639), (16, 1279), (8, 2559), (4, MAX_HH))
# (n, hh, ww) of the GPU test: tests/test_gpu_cols.py says why each
SHAPES = ([(1, 1, 5), (1, 3, 8), (2, 37, 53)] + [(1, 8, cb + e) for cb, _ in STRIPS for e in (-1, 0, 1) if cb + e >= 5]
          + [(1, hh + e, cb + 1) for cb, hh in STRIPS[:-1] for e in (0, 1)] + [(1, MAX_HH, 5), (1, 8, 640)])
SHAPES = sorted(set(SHAPES))
CLASSES = {"applied", "skipped", "half", "half_minus_one", "even", "odd", "zero", "empty"}


def strip_of(hh):
    return next(cb for cb, last in STRIPS if hh <= last)


def cfg(k_gate, noise_a, noise_b, var_floor=1.0):
    """the fields of struct rvdd_cols_cfg, as f32"""
    return tuple(f32(v) for v in (k_gate, noise_a, noise_b, var_floor))


def top_of(bits):
    return f32((1 << bits) - 1)


def dn(v, top):
    return ((v + f32(1.0)) * f32(0.5)) * top


def norm_dn(d, top):
    return f32(2.0) * (d / top) - f32(1.0)


def neighbour(c, dc, ww):
    """the plane column of the horizontal neighbour dc of column c: mirrored about the site, then (fewer than nine columns) about the edge"""
    q = c + dc
    if q < 0 or q >= ww:
        q = c - dc
    if q < 0:
        q = -q
    if q >= ww:
        q = 2 * (ww - 1) - q
    return q


def mosaic_of(cmap):
    """map [2,ww] -> one value per mosaic column [2 ww]: file[x] = map[x & 1][x >> 1]"""
    return np.ascontiguousarray(np.asarray(cmap).T).reshape(-1)


def map_of(line):
    """one value per mosaic column [W], W even -> map [2, W / 2]"""
    return np.ascontiguousarray(np.asarray(line).reshape(-1, 2).T)


def deviations(packed, bits, c):
    """-> (d, used): every sample's d = x - median of its eight horizontal neighbours, and whether the gate takes it"""
    k_gate, a, b, floor = c
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and 1 <= hh <= MAX_HH and ww >= 5
    x = dn(packed, top)
    nb = np.stack([x[:, :, :, [neighbour(col, dc, ww) for col in range(ww)]] for dc in DCS])
    s = np.sort(nb, axis=0)
    m = (s[3] + s[4]) * f32(0.5)
    d = x - m
    var = np.maximum(a * m - b, floor)
    used = d * d <= (k_gate * k_gate) * var
    return d, used


def estimate(packed, bits, c):
    """-> {"offsets": f32 [n,2,ww], "state": u8 [n,2,ww], "cnt": the used samples [n,2,ww]}"""
    n, _, hh, ww = packed.shape
    d, used = deviations(packed, bits, c)
    offsets = np.zeros((n, 2, ww), np.float32)
    state = np.zeros((n, 2, ww), np.uint8)
    cnts = np.zeros((n, 2, ww), np.int64)
    for i in range(n):
        for j in range(2):
            for col in range(ww):
                v = np.sort(np.concatenate([d[i, j, :, col][used[i, j, :, col]], d[i, j + 2, :, col][used[i, j + 2, :, col]]]))
                cnt = cnts[i, j, col] = v.size
                if cnt > 0 and cnt >= hh:
                    offsets[i, j, col] = (v[(cnt - 1) // 2] + v[cnt // 2]) * f32(0.5)
                    state[i, j, col] = APPLIED
    return {"offsets": offsets, "state": state, "cnt": cnts}


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


def gray_of(packed, bits):
    """the gray plane the ingest leaves beside packed frames"""
    x = dn(packed, top_of(bits))
    return (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) * f32(0.25)


def apply(packed, gray, cmap, bits):
    """-> (packed, gray) with the map [2,ww] taken out: copies; gray may be None"""
    top = top_of(bits)
    out = packed.copy()
    g = None if gray is None else gray.copy()
    o = cmap[[0, 1, 0, 1]][None, :, None, :]                              # [1,4,1,ww]: plane k has map[k & 1]
    dd = dn(packed, top) - o
    hit = np.broadcast_to(o != 0, packed.shape)
    out[hit] = norm_dn(dd, top)[hit]
    if g is not None:
        cols = np.broadcast_to((cmap != 0).any(axis=0)[None, None, :], g.shape)
        new = (((dd[:, 0] + dd[:, 1]) + dd[:, 2]) + dd[:, 3]) * f32(0.25)
        g[cols] = new[cols]
    return out, g


# ---- the same, slowly ---------------------------------------------------------------------------------------------------------------
def estimate_slow(packed, bits, c):
    k_gate, a, b, floor = c
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    k2 = f32(k_gate * k_gate)
    offsets = np.zeros((n, 2, ww), np.float32)
    state = np.zeros((n, 2, ww), np.uint8)
    cnts = np.zeros((n, 2, ww), np.int64)
    for i in range(n):
        for j in range(2):
            for col in range(ww):
                ds = []
                for k in (j, j + 2):
                    for r in range(hh):
                        x = f32(f32(f32(packed[i, k, r, col] + f32(1.0)) * f32(0.5)) * top)
                        nb = sorted(f32(f32(f32(packed[i, k, r, neighbour(col, dc, ww)] + f32(1.0)) * f32(0.5)) * top) for dc in DCS)
                        m = f32(f32(nb[3] + nb[4]) * f32(0.5))
                        d = f32(x - m)
                        var = max(f32(f32(a * m) - b), floor)
                        if f32(d * d) <= f32(k2 * var):
                            ds.append(d)
                ds.sort()
                cnt = cnts[i, j, col] = len(ds)
                if cnt > 0 and cnt >= hh:
                    offsets[i, j, col] = f32(f32(ds[(cnt - 1) // 2] + ds[cnt // 2]) * f32(0.5))
                    state[i, j, col] = APPLIED
    return {"offsets": offsets, "state": state, "cnt": cnts}


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
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    out, g = packed.copy(), gray.copy()
    for i in range(n):
        for col in range(ww):
            if cmap[0, col] == 0 and cmap[1, col] == 0:
                continue
            for r in range(hh):
                total = None
                for k in range(4):
                    o = cmap[k & 1, col]
                    d = f32(f32(f32(f32(packed[i, k, r, col] + f32(1.0)) * f32(0.5)) * top) - o)
                    total = d if total is None else f32(total + d)
                    if o != 0:
                        out[i, k, r, col] = f32(f32(f32(2.0) * f32(d / top)) - f32(1.0))
                g[i, r, col] = f32(total * f32(0.25))
    return out, g


# ---- what fired ---------------------------------------------------------------------------------------------------------------------
def classes(est, hh):
    """the classes of CLASSES that an estimate holds"""
    o, st, cnt = est["offsets"], est["state"], est["cnt"]
    got = set()
    got |= {"applied"} if (st != SKIPPED).any() else set()
    got |= {"skipped"} if (st == SKIPPED).any() else set()
    got |= {"half"} if ((cnt == hh) & (st != SKIPPED)).any() else set()
    got |= {"half_minus_one"} if ((cnt == hh - 1) & (st == SKIPPED)).any() else set()
    got |= {"even"} if ((st != SKIPPED) & (cnt % 2 == 0)).any() else set()
    got |= {"odd"} if ((st != SKIPPED) & (cnt % 2 == 1)).any() else set()
    got |= {"zero"} if ((st == APPLIED) & (o == 0)).any() else set()
    got |= {"empty"} if (cnt == 0).any() else set()
    return got


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def packed_of(dnv, bits):
    """whole DN [n,4,hh,ww] -> the packed planes the ingest writes"""
    return norm_dn(np.clip(np.rint(dnv), 0, (1 << bits) - 1).astype(np.float32), top_of(bits)).astype(np.float32)


def scene(n, hh, ww, seed, level=800.0, swing=600.0):
    """a smooth scene in DN, [n,4,hh,ww]: planes 0, 2 and 0.8 of them + 50 in planes 1, 3, moving a little from frame to frame"""
    y, x = np.mgrid[0:hh, 0:ww].astype(np.float64)
    out = np.empty((n, 4, hh, ww))
    for i in range(n):
        base = level + swing * np.sin((y + 3 * i + seed) / 37.0) * np.cos(x / 23.0) + 2.0 * x
        out[i, 0] = out[i, 2] = base
        out[i, 1] = out[i, 3] = 0.8 * base + 50.0
    return out


def with_cols(clean, sigma, sigma_col, rng):
    """clean DN + white noise + one static Gaussian offset per (parity, column) -> (DN, the offsets [2,ww])"""
    n, _, hh, ww = clean.shape
    cols = rng.normal(0.0, 1.0, (2, ww)) * sigma_col
    return clean + rng.normal(0.0, sigma, clean.shape) + cols[[0, 1, 0, 1]][None, :, None, :], cols


def crafted(n, hh, ww):
    """A constant 12-bit frame (every d = 0) with columns made by hand under a constant curve of variance 100 and a gate of 3
    (|d| <= 30): a column of parity 0 whose plane-0 half lies far outside the gate (exactly hh used: applied), a column of parity 1
    with one sample more outside (hh - 1 used: skipped).  The columns lie as far apart as ww lets them; in a narrow plane they meet
    in each other's windows and some classes fall away (the tests ask for the union over the shapes)."""
    v = np.full((n, 4, hh, ww), 1000.0)
    i = n - 1
    v[i, 0, :, 1] = 1500.0                                                 # parity 0, column 1: plane 0 out, plane 2 in
    v[i, 1, :, ww - 2] = 1500.0                                            # parity 1, column ww - 2: plane 1 out ...
    v[i, 3, 0, ww - 2] = 400.0                                             # ... and one sample of plane 3
    return v


def cases(shape):
    """The inputs of one shape: [(name, packed f32 [n,4,hh,ww], bit depth, cfg)] -- tests/rows_ref.py's five, transposed."""
    n, hh, ww = shape
    rng = np.random.default_rng(1000 * n + 10 * hh + ww)
    noisy, _ = with_cols(scene(n, hh, ww, seed=hh), 30.0, 10.0, rng)
    out = [("scene12", packed_of(noisy, 12), 12, cfg(3.0, 1.0, -100.0, 1.0))]
    low, _ = with_cols(scene(n, hh, ww, seed=1, level=7.0, swing=3.0) * [[[[1.0]], [[1.25]], [[1.0]], [[1.25]]]] - 2.0, 0.8, 0.7, rng)
    out.append(("bits4", packed_of(low, 4), 4, cfg(3.0, 0.0, -1.0, 0.25)))
    out.append(("constant", packed_of(np.full((n, 4, hh, ww), 517.0), 12), 12, cfg(3.0, 8.0, 2043.5, 1.0)))
    step = scene(n, hh, ww, seed=5) + rng.normal(0.0, 30.0, (n, 4, hh, ww))
    step[:, :, :, ww // 2:] += 1500.0
    out.append(("step", packed_of(step, 12), 12, cfg(3.0, 0.0, -900.0, 1.0)))
    out.append(("crafted", packed_of(crafted(n, hh, ww), 12), 12, cfg(3.0, 0.0, -100.0, 1.0)))
    return out


def fit_cfg_for(bits, frames):
    """the fit the tests pool a shape's frames with: half the frames, three standard errors, top / 64"""
    return max(1, frames // 2), 3.0, float(top_of(bits)) / 64.0
