"""The row-noise rule of include/rvdd.h (rvdd_rows_estimate, rvdd_rows_apply) restated in NumPy float32, every operation rounded on its
own, and the inputs the host and GPU tests share.  estimate() / apply() are vectorised; estimate_slow() / apply_slow() say the same
with plain loops and np.float32 scalars (tests/test_rows_host.py holds the two together word for word)."""
import numpy as np

f32 = np.float32
DRS = (-4, -3, -2, -1, 1, 2, 3, 4)
MAX_WW = 4096
SKIPPED, APPLIED, CLAMPED = 0, 1, 2

# (n, hh, ww) of the GPU test: tests/test_gpu_rows.py says why each
SHAPES = [(1, 5, 1), (2, 6, 3), (1, 9, 64), (3, 7, 129), (1, 8, 640), (2, 6, 1030), (1, 5, 4096)]
CLASSES = {"applied", "skipped", "clamped_pos", "clamped_neg", "half", "half_minus_one", "even", "odd", "zero", "empty"}


def cfg(k_gate, noise_a, noise_b, var_floor=1.0, max_dn=64.0):
    """the fields of struct rvdd_rows_cfg, as f32"""
    return tuple(f32(v) for v in (k_gate, noise_a, noise_b, var_floor, max_dn))


def top_of(bits):
    return f32((1 << bits) - 1)


def dn(v, top):
    return ((v + f32(1.0)) * f32(0.5)) * top


def norm_dn(d, top):
    return f32(2.0) * (d / top) - f32(1.0)


def neighbour(r, dr, hh):
    """the plane row of the vertical neighbour dr of row r: mirrored about the site, then (fewer than nine rows) about the edge"""
    q = r + dr
    if q < 0 or q >= hh:
        q = r - dr
    if q < 0:
        q = -q
    if q >= hh:
        q = 2 * (hh - 1) - q
    return q


def new_acc(n):
    return {"applied": np.zeros(n, np.uint32), "skipped": np.zeros(n, np.uint32), "clamped": np.zeros(n, np.uint32),
            "sum_q2": np.zeros(n, np.int64)}


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def deviations(packed, bits, c):
    """-> (d, used): every sample's d = x - median of its eight vertical neighbours, and whether the gate takes it"""
    k_gate, a, b, floor, _ = c
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and hh >= 5 and 1 <= ww <= MAX_WW
    x = dn(packed, top)
    nb = np.stack([x[:, :, [neighbour(r, dr, hh) for r in range(hh)], :] for dr in DRS])
    s = np.sort(nb, axis=0)
    m = (s[3] + s[4]) * f32(0.5)
    d = x - m
    var = np.maximum(a * m - b, floor)
    used = d * d <= (k_gate * k_gate) * var
    return d, used


def estimate(packed, bits, c, acc=None):
    """-> {"offsets": f32 [n,2,hh], "state": u8 [n,2,hh], "cnt": the used samples [n,2,hh], "acc": `acc` (None: zeros) plus the rows}"""
    n, _, hh, ww = packed.shape
    max_dn = c[4]
    d, used = deviations(packed, bits, c)
    offsets = np.zeros((n, 2, hh), np.float32)
    state = np.zeros((n, 2, hh), np.uint8)
    cnts = np.zeros((n, 2, hh), np.int64)
    acc = {k: v.copy() for k, v in (acc or new_acc(n)).items()}
    for i in range(n):
        for j in range(2):
            for r in range(hh):
                v = np.sort(np.concatenate([d[i, 2 * j, r][used[i, 2 * j, r]], d[i, 2 * j + 1, r][used[i, 2 * j + 1, r]]]))
                cnt = cnts[i, j, r] = v.size
                if not (cnt > 0 and 2 * cnt >= 2 * ww):
                    acc["skipped"][i] += 1
                    continue
                o = (v[(cnt - 1) // 2] + v[cnt // 2]) * f32(0.5)
                oc = np.minimum(np.maximum(o, -max_dn), max_dn)
                offsets[i, j, r] = oc
                state[i, j, r] = CLAMPED if oc != o else APPLIED
                acc["applied"][i] += 1
                acc["clamped"][i] += int(oc != o)
                q = int(np.rint(oc * f32(16.0)))
                acc["sum_q2"][i] += q * q
    return {"offsets": offsets, "state": state, "cnt": cnts, "acc": acc}


def gray_of(packed, bits):
    """the gray plane the ingest leaves beside packed frames"""
    x = dn(packed, top_of(bits))
    return (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) * f32(0.25)


def apply(packed, gray, offsets, bits):
    """-> (packed, gray) with the offsets taken out: copies; gray may be None"""
    top = top_of(bits)
    out = packed.copy()
    g = None if gray is None else gray.copy()
    o = np.repeat(offsets, 2, axis=1)[:, :, :, None]                      # [n,4,hh,1]: plane k has o[k >> 1]
    dd = dn(packed, top) - o
    hit = np.broadcast_to(o != 0, packed.shape)
    out[hit] = norm_dn(dd, top)[hit]
    if g is not None:
        rows = (offsets != 0).any(axis=1)                                 # [n,hh]
        new = (((dd[:, 0] + dd[:, 1]) + dd[:, 2]) + dd[:, 3]) * f32(0.25)
        g[rows] = new[rows]
    return out, g


# ---- the same, slowly ---------------------------------------------------------------------------------------------------------------
def estimate_slow(packed, bits, c):
    k_gate, a, b, floor, max_dn = c
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    k2 = f32(k_gate * k_gate)
    offsets = np.zeros((n, 2, hh), np.float32)
    state = np.zeros((n, 2, hh), np.uint8)
    cnts = np.zeros((n, 2, hh), np.int64)
    acc = new_acc(n)
    for i in range(n):
        for j in range(2):
            for r in range(hh):
                ds = []
                for k in (2 * j, 2 * j + 1):
                    for col in range(ww):
                        x = f32(f32(f32(packed[i, k, r, col] + f32(1.0)) * f32(0.5)) * top)
                        nb = sorted(f32(f32(f32(packed[i, k, neighbour(r, dr, hh), col] + f32(1.0)) * f32(0.5)) * top) for dr in DRS)
                        m = f32(f32(nb[3] + nb[4]) * f32(0.5))
                        d = f32(x - m)
                        var = max(f32(f32(a * m) - b), floor)
                        if f32(d * d) <= f32(k2 * var):
                            ds.append(d)
                ds.sort()
                cnt = cnts[i, j, r] = len(ds)
                if cnt > 0 and 2 * cnt >= 2 * ww:
                    o = f32(f32(ds[(cnt - 1) // 2] + ds[cnt // 2]) * f32(0.5))
                    oc = min(max(o, f32(-max_dn)), max_dn)
                    offsets[i, j, r] = oc
                    state[i, j, r] = CLAMPED if oc != o else APPLIED
                    acc["applied"][i] += 1
                    acc["clamped"][i] += int(oc != o)
                    q = int(np.rint(f32(oc * f32(16.0))))
                    acc["sum_q2"][i] += q * q
                else:
                    acc["skipped"][i] += 1
    return {"offsets": offsets, "state": state, "cnt": cnts, "acc": acc}


def apply_slow(packed, gray, offsets, bits):
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    out, g = packed.copy(), gray.copy()
    for i in range(n):
        for r in range(hh):
            if offsets[i, 0, r] == 0 and offsets[i, 1, r] == 0:
                continue
            for col in range(ww):
                total = None
                for k in range(4):
                    o = offsets[i, k >> 1, r]
                    d = f32(f32(f32(f32(packed[i, k, r, col] + f32(1.0)) * f32(0.5)) * top) - o)
                    total = d if total is None else f32(total + d)
                    if o != 0:
                        out[i, k, r, col] = f32(f32(f32(2.0) * f32(d / top)) - f32(1.0))
                g[i, r, col] = f32(total * f32(0.25))
    return out, g


# ---- what fired ---------------------------------------------------------------------------------------------------------------------
def classes(est, ww):
    """the classes of CLASSES that an estimate holds"""
    o, st, cnt = est["offsets"], est["state"], est["cnt"]
    got = set()
    got |= {"applied"} if (st != SKIPPED).any() else set()
    got |= {"skipped"} if (st == SKIPPED).any() else set()
    got |= {"clamped_pos"} if ((st == CLAMPED) & (o > 0)).any() else set()
    got |= {"clamped_neg"} if ((st == CLAMPED) & (o < 0)).any() else set()
    got |= {"half"} if ((cnt == ww) & (st != SKIPPED)).any() else set()
    got |= {"half_minus_one"} if ((cnt == ww - 1) & (st == SKIPPED)).any() else set()
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
    """a smooth scene in DN, [n,4,hh,ww]: planes 0, 1 and 0.8 of them + 50 in planes 2, 3, moving a little from frame to frame"""
    y, x = np.mgrid[0:hh, 0:ww].astype(np.float64)
    out = np.empty((n, 4, hh, ww))
    for i in range(n):
        base = level + swing * np.sin((x + 3 * i + seed) / 37.0) * np.cos(y / 23.0) + 2.0 * y
        out[i, 0] = out[i, 1] = base
        out[i, 2] = out[i, 3] = 0.8 * base + 50.0
    return out


def with_rows(clean, sigma, sigma_row, rng):
    """clean DN + white noise + one Gaussian offset per (frame, parity, row) -> (DN, the offsets [n,2,hh])"""
    n, _, hh, ww = clean.shape
    rows = rng.normal(0.0, 1.0, (n, 2, hh)) * sigma_row
    return clean + rng.normal(0.0, sigma, clean.shape) + np.repeat(rows, 2, axis=1)[:, :, :, None], rows


def crafted(n, hh, ww):
    """A constant 12-bit frame (every d = 0) with rows made by hand under a constant curve of variance 100 and a gate of 3 (|d| <= 30),
    clamp 8 DN: a row of parity 0 whose plane-0 half lies far outside the gate (exactly ww used: applied), a row of parity 1 with one
    sample more outside (ww - 1 used: skipped), a row 20 DN up and a row 20 DN down (inside the gate, beyond the clamp).  The rows lie
    as far apart as hh lets them; in a low plane they meet in each other's windows and some classes fall away (the tests ask for the
    union over the shapes)."""
    v = np.full((n, 4, hh, ww), 1000.0)
    i = n - 1
    v[i, 0, 1, :] = 1500.0                                                 # parity 0, row 1: plane 0 out, plane 1 in
    v[i, 2, hh - 2, :] = 1500.0                                            # parity 1, row hh - 2: plane 2 out ...
    v[i, 3, hh - 2, 0] = 400.0                                             # ... and one sample of plane 3
    v[0, 0:2, hh - 1, :] += 20.0                                           # parity 0, the last row: up
    v[0, 2:4, 0, :] -= 20.0                                                # parity 1, the first row: down
    return v


def cases(shape):
    """The inputs of one shape: [(name, packed f32 [n,4,hh,ww], bit depth, cfg)]."""
    n, hh, ww = shape
    rng = np.random.default_rng(1000 * n + 10 * hh + ww)
    noisy, _ = with_rows(scene(n, hh, ww, seed=ww), 30.0, 10.0, rng)
    out = [("scene12", packed_of(noisy, 12), 12, cfg(3.0, 1.0, -100.0, 1.0, 4095.0 / 64.0))]
    low, _ = with_rows(scene(n, hh, ww, seed=1, level=7.0, swing=3.0) * [[[[1.0]], [[1.0]], [[1.25]], [[1.25]]]] - 2.0, 0.8, 0.7, rng)
    out.append(("bits4", packed_of(low, 4), 4, cfg(3.0, 0.0, -1.0, 0.25, 0.75)))
    out.append(("constant", packed_of(np.full((n, 4, hh, ww), 517.0), 12), 12, cfg(3.0, 8.0, 2043.5, 1.0, 64.0)))
    step = scene(n, hh, ww, seed=5) + rng.normal(0.0, 30.0, (n, 4, hh, ww))
    step[:, :, hh // 2:, :] += 1500.0
    out.append(("step", packed_of(step, 12), 12, cfg(3.0, 0.0, -900.0, 1.0, 64.0)))
    out.append(("crafted", packed_of(crafted(n, hh, ww), 12), 12, cfg(3.0, 0.0, -100.0, 1.0, 8.0)))
    return out
