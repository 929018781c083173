"""What the row-noise and the column-noise rule of include/rvdd.h share, restated once in NumPy float32, every operation rounded on its
own: tests/rows_ref.py and tests/cols_ref.py (the modules the tests import) are this with an axis, plus what is theirs alone.  A LINE
is a plane row (axis = ROWS) or a plane column (axis = COLS) of packed [n,4,hh,ww]: `axis` is the tensor axis that counts the lines
and along which a sample's eight neighbours lie; a line's samples lie along the other one.  The two planes that share a line's offset
are (2j, 2j + 1) for rows and (j, j + 2) for columns (planes()).  The vectorised functions and the *_slow ones (plain loops, np.float32
scalars) say the same word for word."""
import numpy as np

f32 = np.float32
ROWS, COLS = 2, 3
OFFS = (-4, -3, -2, -1, 1, 2, 3, 4)
SKIPPED, APPLIED = 0, 1
CLASSES = {"applied", "skipped", "half", "half_minus_one", "even", "odd", "zero", "empty"}


def planes(axis, j):
    """the two planes of parity j"""
    return (2 * j, 2 * j + 1) if axis == ROWS else (j, j + 2)


def spread(lines, axis):
    """one value per (parity, line) -> one per plane and line, broadcastable to [n,4,hh,ww]: rows [n,2,hh], columns a static [2,ww]"""
    return np.repeat(lines, 2, axis=1)[:, :, :, None] if axis == ROWS else lines[[0, 1, 0, 1]][None, :, None, :]


def cfg(k_gate, noise_a, noise_b, var_floor=1.0):
    """the gate's four fields of struct rvdd_rows_cfg / rvdd_cols_cfg, as f32"""
    return tuple(f32(v) for v in (k_gate, noise_a, noise_b, var_floor))


def top_of(bits):
    return f32((1 << bits) - 1)


def dn(v, top):
    return ((v + f32(1.0)) * f32(0.5)) * top


def norm_dn(d, top):
    return f32(2.0) * (d / top) - f32(1.0)


def neighbour(i, d, n):
    """the line d lines from line i in a plane of n: mirrored about the site, then (fewer than nine lines) about the edge"""
    q = i + d
    if q < 0 or q >= n:
        q = i - d
    if q < 0:
        q = -q
    if q >= n:
        q = 2 * (n - 1) - q
    return q


def deviations(packed, bits, c, axis):
    """-> (d, used): every sample's d = x - median of its eight neighbours across the lines, and whether the gate takes it"""
    k_gate, a, b, floor = c[:4]
    top = top_of(bits)
    lines = packed.shape[axis]
    x = dn(packed, top)
    nb = np.stack([np.take(x, [neighbour(i, o, lines) for i in range(lines)], axis=axis) for o in OFFS])
    s = np.sort(nb, axis=0)
    m = (s[3] + s[4]) * f32(0.5)
    d = x - m
    var = np.maximum(a * m - b, floor)
    used = d * d <= (k_gate * k_gate) * var
    return d, used


def estimate(packed, bits, c, axis):
    """-> {"offsets": f32 [n,2,lines] (no clamp), "state": u8 [n,2,lines], "cnt": the used samples [n,2,lines]}: the median of a
    line's used d where at least half of its samples are used"""
    n, lines, half = packed.shape[0], packed.shape[axis], packed.shape[5 - axis]
    d, used = (np.moveaxis(v, axis, 2) for v in deviations(packed, bits, c, axis))      # [n,4,lines,samples]
    offsets = np.zeros((n, 2, lines), np.float32)
    state = np.zeros((n, 2, lines), np.uint8)
    cnts = np.zeros((n, 2, lines), np.int64)
    for i in range(n):
        for j in range(2):
            p, q = planes(axis, j)
            for ln in range(lines):
                v = np.sort(np.concatenate([d[i, p, ln][used[i, p, ln]], d[i, q, ln][used[i, q, ln]]]))
                cnt = cnts[i, j, ln] = v.size
                if cnt > 0 and cnt >= half:
                    offsets[i, j, ln] = (v[(cnt - 1) // 2] + v[cnt // 2]) * f32(0.5)
                    state[i, j, ln] = APPLIED
    return {"offsets": offsets, "state": state, "cnt": cnts}


def gray_of(packed, bits):
    """the gray plane the ingest leaves beside packed frames"""
    x = dn(packed, top_of(bits))
    return (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) * f32(0.25)


def apply(packed, gray, o, bits):
    """-> (packed, gray) with the offsets o (spread(): one per plane and line) taken out where they are not zero: copies; gray may be None"""
    top = top_of(bits)
    out = packed.copy()
    g = None if gray is None else gray.copy()
    dd = dn(packed, top) - o
    hit = np.broadcast_to(o != 0, packed.shape)
    out[hit] = norm_dn(dd, top)[hit]
    if g is not None:
        cells = np.broadcast_to((o != 0).any(axis=1), g.shape)            # a gray cell changes where either parity's offset is not zero
        new = (((dd[:, 0] + dd[:, 1]) + dd[:, 2]) + dd[:, 3]) * f32(0.25)
        g[cells] = new[cells]
    return out, g


# ---- the same, slowly ---------------------------------------------------------------------------------------------------------------
def estimate_slow(packed, bits, c, axis):
    k_gate, a, b, floor = c[:4]
    top = top_of(bits)
    n, lines, half = packed.shape[0], packed.shape[axis], packed.shape[5 - axis]
    at = (lambda ln, s: (ln, s)) if axis == ROWS else (lambda ln, s: (s, ln))
    k2 = f32(k_gate * k_gate)
    offsets = np.zeros((n, 2, lines), np.float32)
    state = np.zeros((n, 2, lines), np.uint8)
    cnts = np.zeros((n, 2, lines), np.int64)
    for i in range(n):
        for j in range(2):
            for ln in range(lines):
                ds = []
                for k in planes(axis, j):
                    for s in range(half):
                        x = f32(f32(f32(packed[(i, k) + at(ln, s)] + f32(1.0)) * f32(0.5)) * top)
                        nb = sorted(f32(f32(f32(packed[(i, k) + at(neighbour(ln, o, lines), s)] + f32(1.0)) * f32(0.5)) * top) for o in OFFS)
                        m = f32(f32(nb[3] + nb[4]) * f32(0.5))
                        d = f32(x - m)
                        var = max(f32(f32(a * m) - b), floor)
                        if f32(d * d) <= f32(k2 * var):
                            ds.append(d)
                ds.sort()
                cnt = cnts[i, j, ln] = len(ds)
                if cnt > 0 and cnt >= half:
                    offsets[i, j, ln] = f32(f32(ds[(cnt - 1) // 2] + ds[cnt // 2]) * f32(0.5))
                    state[i, j, ln] = APPLIED
    return {"offsets": offsets, "state": state, "cnt": cnts}


def apply_slow(packed, gray, o, bits):
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    o = np.broadcast_to(o, packed.shape)
    out, g = packed.copy(), gray.copy()
    for i in range(n):
        for r in range(hh):
            for col in range(ww):
                if not o[i, :, r, col].any():
                    continue
                total = None
                for k in range(4):
                    d = f32(f32(f32(f32(packed[i, k, r, col] + f32(1.0)) * f32(0.5)) * top) - o[i, k, r, col])
                    total = d if total is None else f32(total + d)
                    if o[i, k, r, col] != 0:
                        out[i, k, r, col] = f32(f32(f32(2.0) * f32(d / top)) - f32(1.0))
                g[i, r, col] = f32(total * f32(0.25))
    return out, g


# ---- what fired ---------------------------------------------------------------------------------------------------------------------
def classes(est, half):
    """the classes of CLASSES that an estimate holds; half: the samples of one plane's line"""
    o, st, cnt = est["offsets"], est["state"], est["cnt"]
    got = set()
    got |= {"applied"} if (st != SKIPPED).any() else set()
    got |= {"skipped"} if (st == SKIPPED).any() else set()
    got |= {"half"} if ((cnt == half) & (st != SKIPPED)).any() else set()
    got |= {"half_minus_one"} if ((cnt == half - 1) & (st == SKIPPED)).any() else set()
    got |= {"even"} if ((st != SKIPPED) & (cnt % 2 == 0)).any() else set()
    got |= {"odd"} if ((st != SKIPPED) & (cnt % 2 == 1)).any() else set()
    got |= {"zero"} if ((st == APPLIED) & (o == 0)).any() else set()
    got |= {"empty"} if (cnt == 0).any() else set()
    return got


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def packed_of(dnv, bits):
    """whole DN [n,4,hh,ww] -> the packed planes the ingest writes"""
    return norm_dn(np.clip(np.rint(dnv), 0, (1 << bits) - 1).astype(np.float32), top_of(bits)).astype(np.float32)


def scene(n, hh, ww, seed, axis, level=800.0, swing=600.0):
    """a smooth scene in DN, [n,4,hh,ww]: the planes of parity 0 and 0.8 of them + 50 in those of parity 1, moving a little along the
    lines from frame to frame"""
    y, x = np.mgrid[0:hh, 0:ww].astype(np.float64)
    ln, s = (y, x) if axis == ROWS else (x, y)
    out = np.empty((n, 4, hh, ww))
    for i in range(n):
        base = level + swing * np.sin((s + 3 * i + seed) / 37.0) * np.cos(ln / 23.0) + 2.0 * ln
        out[i, planes(axis, 0)] = base
        out[i, planes(axis, 1)] = 0.8 * base + 50.0
    return out


def with_lines(clean, sigma, sigma_line, rng, axis):
    """clean DN + white noise + one Gaussian offset per (frame, parity, row), or one static one per (parity, column)
    -> (DN, the offsets [n,2,hh] / [2,ww])"""
    n, _, hh, ww = clean.shape
    lines = rng.normal(0.0, 1.0, (n, 2, hh) if axis == ROWS else (2, ww)) * sigma_line
    return clean + rng.normal(0.0, sigma, clean.shape) + spread(lines, axis), lines


def crafted(n, hh, ww, axis):
    """A constant 12-bit frame (every d = 0) with lines made by hand under a constant curve of variance 100 and a gate of 3
    (|d| <= 30): line 1 of parity 0 whose first plane lies far outside the gate (exactly half used: applied), the last line but one of
    parity 1 with one sample more outside (half - 1 used: skipped).  The lines lie as far apart as the plane lets them; in a small
    plane they meet in each other's windows and some classes fall away (the tests ask for the union over the shapes)."""
    v = np.full((n, 4, hh, ww), 1000.0)
    w = np.moveaxis(v, axis, 2)                                            # a view: [n,4,lines,samples]
    i, last = n - 1, v.shape[axis] - 2
    w[i, planes(axis, 0)[0], 1, :] = 1500.0                                # parity 0: the first plane out, the second in
    w[i, planes(axis, 1)[0], last, :] = 1500.0                             # parity 1: the first plane out ...
    w[i, planes(axis, 1)[1], last, 0] = 400.0                              # ... and one sample of the second
    return v


def cases(shape, axis, craft=crafted):
    """The inputs of one shape: [(name, packed f32 [n,4,hh,ww], bit depth, cfg)]."""
    n, hh, ww = shape
    rng = np.random.default_rng(1000 * n + 10 * hh + ww)
    gain = np.ones((1, 4, 1, 1))
    gain[0, planes(axis, 1)] = 1.25
    noisy, _ = with_lines(scene(n, hh, ww, shape[4 - axis], axis), 30.0, 10.0, rng, axis)
    out = [("scene12", packed_of(noisy, 12), 12, cfg(3.0, 1.0, -100.0, 1.0))]
    low, _ = with_lines(scene(n, hh, ww, 1, axis, level=7.0, swing=3.0) * gain - 2.0, 0.8, 0.7, rng, axis)
    out.append(("bits4", packed_of(low, 4), 4, cfg(3.0, 0.0, -1.0, 0.25)))
    out.append(("constant", packed_of(np.full((n, 4, hh, ww), 517.0), 12), 12, cfg(3.0, 8.0, 2043.5, 1.0)))
    step = scene(n, hh, ww, 5, axis) + rng.normal(0.0, 30.0, (n, 4, hh, ww))
    np.moveaxis(step, axis, 2)[:, :, shape[axis - 1] // 2:] += 1500.0     # the far half of the lines
    out.append(("step", packed_of(step, 12), 12, cfg(3.0, 0.0, -900.0, 1.0)))
    out.append(("crafted", packed_of(craft(n, hh, ww, axis), 12), 12, cfg(3.0, 0.0, -100.0, 1.0)))
    return out


NO_CLAMP = 3e38                                                            # a max_dn finite in f32 and beyond any offset


def transposed(packed):
    """packed [n,4,hh,ww] -> [n,4,ww,hh], its columns as rows: the spatial axes swapped, and planes 1 and 2, which turns the column
    pairs (j, j + 2) into the row pairs (2j, 2j + 1)"""
    return np.ascontiguousarray(packed.transpose(0, 1, 3, 2)[:, [0, 2, 1, 3]])
