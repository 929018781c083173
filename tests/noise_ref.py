"""NumPy restatement of rvdd_noise_hist / rvdd_noise_fit (include/rvdd.h): the block statistics in explicit float32 with the sums
in the header's order, the accumulators as int64 arrays filled with np.add.at, the fit in Python doubles in the order of the C
code -- and the synthetic scenes the tests share."""
import math

import numpy as np

import dpc_ref

F = np.float32
MEAN_BINS, VAR_BINS = 64, 512
J0 = (127 - 6) << 4                   # the sub-bin of 2^-6
# the lower quartile / the median of the rule's v on unit white Gaussian samples; tools/noise_cq.py (seed 20261019, 4194304 blocks):
#   "mean 1.000094  C_Q (lower quartile) 0.805112  C_MED (median) 0.972282  (standard error about 1.4e-04)"
C_Q = 0.8051
C_MED = 0.9723
MIN_COUNT, MIN_BINS = 16, 4


def block_stats(x):
    """x [..., 8, 8] f32 DN -> (m, v) [...] f32: the mean and the variance estimate of every block, summed in the rule's order"""
    x = np.asarray(x)
    assert x.dtype == F and x.shape[-2:] == (8, 8)
    rs = x[..., 0]
    for c in range(1, 8):
        rs = rs + x[..., c]                              # [..., 8]: the row sums
    s = rs[..., 0]
    for r in range(1, 8):
        s = s + rs[..., r]
    m = s * F(1.0 / 64.0)
    d = x[..., 1:7] - (x[..., 0:6] + x[..., 2:8]) * F(0.5)
    dd = d * d
    rq = dd[..., 0]                                      # 0 + d d is d d
    for c in range(1, 6):
        rq = rq + dd[..., c]
    q = rq[..., 0]
    for r in range(1, 8):
        q = q + rq[..., r]
    v = q * F(1.0 / 72.0)
    for a in (rs, s, m, d, dd, rq, q, v):
        assert a.dtype == F
    return m, v


def new_acc():
    return {"hist": np.zeros((MEAN_BINS, VAR_BINS), np.int64), "msum": np.zeros(MEAN_BINS, np.int64), "counters": np.zeros(4, np.int64)}


def blocks_of(packed, bit_depth):
    """packed [n,4,hh,ww] -> the whole 8 x 8 blocks in DN, [n,4,hh/8,ww/8,8,8] f32 (None where there is none)"""
    p = np.ascontiguousarray(packed, dtype=F)
    n, four, hh, ww = p.shape
    assert four == 4
    bh, bw = hh // 8, ww // 8
    if n == 0 or bh == 0 or bw == 0:
        return None
    dn = ((p + F(1.0)) * F(0.5)) * F(2 ** bit_depth - 1)
    assert dn.dtype == F
    return np.ascontiguousarray(dn[:, :, :bh * 8, :bw * 8].reshape(n, 4, bh, 8, bw, 8).transpose(0, 1, 2, 4, 3, 5))


def keys_of(m, v, bit_depth):
    """f32 arrays of block means and variance estimates -> (mean bin i, variance sub-bin j, what msum[i] gains), int64 arrays"""
    m, v = np.ascontiguousarray(m, dtype=F), np.ascontiguousarray(v, dtype=F)
    scaled = m * F(64.0 / 2 ** bit_depth)
    assert scaled.dtype == F
    i = np.clip(scaled.astype(np.int64), 0, MEAN_BINS - 1)
    j = np.clip((v.view(np.uint32) >> np.uint32(19)).astype(np.int64) - J0, 0, VAR_BINS - 1)
    return i, j, np.rint(m * F(16.0)).astype(np.int64)


def noise_hist_ref(packed, bit_depth, acc=None):
    """rvdd_noise_hist: the blocks of packed [n,4,hh,ww] f32 added to `acc` (a new one where None) -> acc"""
    acc = new_acc() if acc is None else acc
    x = blocks_of(packed, bit_depth)
    if x is None:
        return acc
    top = F(2 ** bit_depth - 1)
    m, v = block_stats(x)
    clipped = ~((x > F(0)) & (x < top)).all(axis=(-1, -2))
    degenerate = ~clipped & (v == F(0))
    ok = ~clipped & ~degenerate
    i, j, m16 = keys_of(m[ok], v[ok], bit_depth)
    np.add.at(acc["hist"], (i, j), 1)
    np.add.at(acc["msum"], i, m16)
    acc["counters"] += np.array([m.size, clipped.sum(), degenerate.sum(), 0], np.int64)
    return acc


def acc_bytes(acc):
    """the accumulator as struct rvdd_noise_acc lays it out: uint32 hist[64][512], uint64 msum[64], uint64 counters[4]"""
    assert acc["hist"].max(initial=0) < 2 ** 32 and min(acc["hist"].min(initial=0), acc["msum"].min(), acc["counters"].min()) >= 0
    return acc["hist"].astype(np.uint32).tobytes() + acc["msum"].astype(np.uint64).tobytes() + acc["counters"].astype(np.uint64).tobytes()


def edge(j):
    """the lower edge of variance sub-bin j: the f32 whose bits are (j + ((127 - 6) << 4)) << 19"""
    return float(np.array([(j + J0) << 19], np.uint32).view(F)[0])


def quantile_of_row(row, count, q):
    """the value at which the cumulative count of a histogram row reaches q * count, linear inside its sub-bin"""
    target = q * count
    cum = 0
    for j in range(VAR_BINS):
        c = int(row[j])
        if c > 0 and cum + c >= target:
            lo, hi = edge(j), edge(j + 1)
            return lo + ((target - cum) / c) * (hi - lo)
        cum += c
    raise AssertionError("an empty row has no quantile")


class FitRefused(ValueError):
    pass


def noise_fit_ref(acc, bit_depth, q=0.25, c_q=C_Q):
    """rvdd_noise_fit in Python doubles, sum for sum in the order of the C code.  q / c_q: another quantile and its constant (the
    median, for the comparison the tests make).  -> dict(a, b, bins, blocks, m_min, m_max, rms); FitRefused as RVDD_ERR_STATE"""
    ms, vs, ns = [], [], []
    for i in range(MEAN_BINS):
        count = int(acc["hist"][i].sum())
        if count < MIN_COUNT:
            continue
        ms.append(float(acc["msum"][i]) / 16.0 / count)
        vs.append(quantile_of_row(acc["hist"][i], count, q) / c_q)
        ns.append(count)
    if len(ms) < MIN_BINS:
        raise FitRefused("%d usable mean bins, at least %d are needed" % (len(ms), MIN_BINS))
    if max(ms) - min(ms) < 2 ** bit_depth / 16.0:
        raise FitRefused("too little tonal range: the bin means span %g DN" % (max(ms) - min(ms)))
    ws = [n / (v * v) for n, v in zip(ns, vs)]
    sw = swm = swv = 0.0
    for w, m, v in zip(ws, ms, vs):
        sw += w
        swm += w * m
        swv += w * v
    mbar, vbar = swm / sw, swv / sw
    smm = smv = 0.0
    for w, m, v in zip(ws, ms, vs):
        smm += w * ((m - mbar) * (m - mbar))
        smv += w * ((m - mbar) * (v - vbar))
    a = smv / smm
    b = a * mbar - vbar
    sr = 0.0
    blocks = 0
    for n, m, v in zip(ns, ms, vs):
        r = (v - (a * m - b)) / v
        sr += n * (r * r)
        blocks += n
    return {"a": a, "b": b, "bins": len(ms), "blocks": blocks, "m_min": min(ms), "m_max": max(ms), "rms": math.sqrt(sr / blocks)}


def sigma_errors(fit, a, b, bit_depth, levels=(0.20, 0.45, 0.80)):
    """relative error of the fit's predicted standard deviation against the curve (a, b) at `levels` of top"""
    top = 2 ** bit_depth - 1
    return [math.sqrt(max(fit["a"] * l * top - fit["b"], 0.0)) / math.sqrt(a * l * top - b) - 1.0 for l in levels]


# ---- scenes ---------------------------------------------------------------------------------------------------------------
PLANE_GAINS = (1.0, 0.85, 0.95, 0.9)


def scene_cells(n, hh, ww, bit_depth, iso, seed, texture=0.0, clip=False, patch=False):
    """whole-DN frames [n,hh,ww,4] f32.  A smooth scene -- a ramp down the frame, a slighter one across it and a slow cosine, times
    a gain per plane -- covering about 10 .. 85 % of the range, with the noise of dpc_ref.noisy_cells (the ISO's curve, rounded and
    clipped).  texture: that share of the 8 x 8 blocks of every plane carries a hard texture (columns alternately +- 6 % of top);
    clip: the top left 16 x 16 cells sit at top; patch: the 16 x 16 cells right of them are a constant without noise."""
    rng = np.random.default_rng(seed)
    top = 2 ** bit_depth - 1
    a, b = dpc_ref.iso_curve(iso, bit_depth)
    y = np.linspace(0.0, 1.0, hh)[None, :, None, None]
    x = np.linspace(0.0, 1.0, ww)[None, None, :, None]
    u = 0.82 * y + 0.15 * x + 0.015 * (1.0 - np.cos(2.0 * np.pi * x))
    m = (0.12 + 0.73 * u) * np.asarray(PLANE_GAINS)[None, None, None, :] * top * np.ones((n, 1, 1, 1))
    if texture > 0:
        bh, bw = hh // 8, ww // 8
        on = rng.random((n, bh, bw, 4)) < texture
        on = np.repeat(np.repeat(on, 8, axis=1), 8, axis=2)
        sign = np.where(np.arange(bw * 8) % 2 == 0, 1.0, -1.0)[None, None, :, None]
        m[:, :bh * 8, :bw * 8] += np.where(on, 0.06 * top * sign, 0.0)
    z = rng.standard_normal(m.shape)
    cells = np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0.0)) * z), 0, top)
    if clip:
        cells[:, :16, :16] = top
    if patch:
        cells[:, :16, 16:32] = round(0.3 * top)
    return cells.astype(F)


def flat_cells(n, hh, ww, bit_depth, iso, seed, level=0.45):
    """a flat noisy scene at the centre of a mean bin: nearly every block lands in that one bin and a few dozen variance sub-bins"""
    rng = np.random.default_rng(seed)
    top = 2 ** bit_depth - 1
    a, b = dpc_ref.iso_curve(iso, bit_depth)
    width = 2 ** bit_depth / 64.0
    m = (math.floor(level * 64) + 0.5) * width * np.ones((n, hh, ww, 4))
    z = rng.standard_normal(m.shape)
    return np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0.0)) * z), 0, top).astype(F)
