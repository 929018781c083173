"""NumPy restatement of the residual statistics (include/rvdd.h: rvdd_resid_stats) and of the judgement against a curve (rvdd_resid_fit)
in Python floats and integers, with the cases the tests share.  f32 arithmetic one operation at a time, integer sums that wrap modulo
2^64 as the device's do.  A plain module: pytest does not rewrite its asserts, so each one carries its message."""
import numpy as np

F = np.float32
BINS = 64
FIELDS = ("n", "msum", "s1", "s2", "n11", "s11")                  # struct rvdd_resid_acc, in order
SIGNED = ("s1", "s11")
ACC_BYTES = 6 * BINS * 8
CLAMP = 2 ** 17
MIN_SAMPLES, MIN_BINS = 1024, 4
PATTERNS = ("gbrg", "grbg", "rggb", "bggr")                       # enum rvdd_bayer order
_GBRG = (1, 2, 0, 1)                                              # the RGB plane of each GBRG site: G, B, R, G
_PHASE = (0, 3, 2, 1)                                             # CFA position k of pattern p is the GBRG site k ^ _PHASE[p]


def col(pattern, k):
    """the RGB plane of CFA position k = 2 * (row & 1) + (column & 1) of `pattern` (an index into PATTERNS)"""
    return _GBRG[k ^ _PHASE[pattern]]


def remosaic(rgb, pattern):
    """rgb [n,3,2hh,2ww] -> its re-mosaic as packed planes [n,4,hh,ww]: plane k = the pattern's colour at the sites of CFA position k"""
    return np.stack([rgb[:, col(pattern, k), (k >> 1)::2, (k & 1)::2] for k in range(4)], axis=1)


def scale_of(bit_depth):
    return 2.0 ** (15 - bit_depth)


def sample_terms(packed, rgb, pattern, bit_depth):
    """-> (rq int64, j int64, mq int64), [n,4,hh,ww] each: the residual in 1 / S DN, the level bin, rint(dc * 16)"""
    packed, rgb = np.asarray(packed, F), np.asarray(rgb, F)
    n, four, hh, ww = packed.shape
    assert four == 4 and rgb.shape == (n, 3, 2 * hh, 2 * ww), ("sample_terms", packed.shape, rgb.shape)
    top, S, bin_scale = F(2 ** bit_depth - 1), F(scale_of(bit_depth)), F(64.0 / 2 ** bit_depth)
    c = ((packed + F(1)) * F(0.5)) * top
    d = ((remosaic(rgb, pattern) + F(1)) * F(0.5)) * top
    t = np.minimum(np.maximum((c - d) * S, F(-CLAMP)), F(CLAMP))
    dc = np.minimum(np.maximum(d, F(0)), top)
    assert t.dtype == F and dc.dtype == F
    rq = np.rint(t).astype(np.int64)
    j = np.minimum((dc * bin_scale).astype(np.int64), BINS - 1)
    mq = np.rint(dc * F(16)).astype(np.int64)
    return rq, j, mq


def new_acc(n):
    return {name: np.zeros((n, BINS), np.int64 if name in SIGNED else np.uint64) for name in FIELDS}


def resid_ref(packed, rgb, pattern, bit_depth, acc=None):
    """the sums of frame i added to row i of `acc` ({field: [n,64]}; None = zeros) -> acc"""
    rq, j, mq = sample_terms(packed, rgb, pattern, bit_depth)
    n = rq.shape[0]
    acc = new_acc(n) if acc is None else {k: v.copy() for k, v in acc.items()}
    with np.errstate(over="ignore"):
        for i in range(n):
            part = {name: np.zeros(BINS, np.int64) for name in FIELDS}
            ji = j[i].reshape(-1)
            np.add.at(part["n"], ji, 1)
            np.add.at(part["msum"], ji, mq[i].reshape(-1))
            np.add.at(part["s1"], ji, rq[i].reshape(-1))
            np.add.at(part["s2"], ji, (rq[i] * rq[i]).reshape(-1))
            jl = j[i][..., :-1].reshape(-1)                       # pairs: x < ww - 1, binned by j of x
            np.add.at(part["n11"], jl, 1)
            np.add.at(part["s11"], jl, (rq[i][..., :-1] * rq[i][..., 1:]).reshape(-1))
            for name in FIELDS:
                acc[name][i] += part[name].astype(acc[name].dtype)
    return acc


def total(acc):
    """{field: [n,64]} -> {field: [64]}: the frames' accumulators added up (modulo 2^64)"""
    with np.errstate(over="ignore"):
        return {name: acc[name].sum(axis=0, dtype=acc[name].dtype) for name in FIELDS}


def add(a, b):
    with np.errstate(over="ignore"):
        return {name: a[name] + b[name] for name in FIELDS}


def acc_bytes(acc, i=None):
    """struct rvdd_resid_acc of row i (None: of an accumulator of [64] arrays)"""
    return b"".join(np.ascontiguousarray(acc[name] if i is None else acc[name][i]).tobytes() for name in FIELDS)


def fit_ref(acc, bit_depth, a, b):
    """rvdd_resid_fit on ONE accumulator ({field: [64]}) in Python floats, each operation as the header writes it.
    -> the report as a dict, or None where fewer than MIN_BINS bins are usable"""
    S = float(scale_of(bit_depth))
    g = {name: [int(v) for v in np.asarray(acc[name]).reshape(-1)] for name in FIELDS}
    ms, vs, rs, ns = [], [], [], []
    samples = 0
    for j in range(BINS):
        if g["n"][j] < MIN_SAMPLES:
            continue
        n = float(g["n"][j])
        m = float(g["msum"][j]) / 16.0 / n
        p = a * m - b
        if not p > 0.0:
            continue
        u = float(g["s1"][j]) / n / S
        v = float(g["s2"][j]) / n / (S * S) - u * u
        ms.append(m), vs.append(v), rs.append(v / p), ns.append(n)
        samples += g["n"][j]
    bins = len(ns)
    if bins < MIN_BINS:
        return None
    sn = snr = 0.0
    for k in range(bins):
        sn += ns[k]
        snr += ns[k] * rs[k]
    out = {"ratio": snr / sn}
    third = float(samples) / 3.0
    for name, order in (("ratio_lo", range(bins)), ("ratio_hi", range(bins - 1, -1, -1))):
        c = sw = swr = 0.0
        for k in order:
            rest = third - c
            w = ns[k] if ns[k] < rest else rest
            if not w > 0.0:
                break
            sw += w
            swr += w * rs[k]
            c += w
        out[name] = swr / sw
    tn, t1, t2, tn11, t11 = (sum(g[name]) for name in ("n", "s1", "s2", "n11", "s11"))
    out["bias"] = float(t1) / float(tn) / S
    out["rho"] = (float(t11) / float(tn11)) / (float(t2) / float(tn)) if tn11 and t2 else 0.0
    out["a_fit"] = out["b_fit"] = 0.0
    use = [k for k in range(bins) if vs[k] > 0.0]
    if len(use) >= 2:
        sw = swm = swv = 0.0
        for k in use:
            w = ns[k] / (vs[k] * vs[k])
            sw += w
            swm += w * ms[k]
            swv += w * vs[k]
        mbar, vbar = swm / sw, swv / sw
        smm = smv = 0.0
        for k in use:
            w = ns[k] / (vs[k] * vs[k])
            smm += w * ((ms[k] - mbar) * (ms[k] - mbar))
            smv += w * ((ms[k] - mbar) * (vs[k] - vbar))
        if smm > 0.0:
            out["a_fit"] = smv / smm
            out["b_fit"] = out["a_fit"] * mbar - vbar
    out["samples"], out["bins"] = samples, bins
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def make_case(n, hh, ww, bits, pattern, seed, flat=False):
    """-> (packed [n,4,hh,ww], rgb [n,3,2hh,2ww], classes): outputs that ramp over most of the level range (flat: ONE level) with a
    little texture, noisy frames around their re-mosaic, and the special samples where the frame has room for them.  classes: what
    the case contains, found on its own integers --
      flat       every sample falls into one bin            clamped    outputs outside [-1,1] AND rq at either clamp
      many_bins  at least 8 bins hold samples               negative   rq < 0 occurs, some s1 is negative and (ww > 1) some s11
      edge_pair  the cells x = ww - 1 have no pair          pairs      the others have one (ww > 1)
      batch      more than one frame"""
    rng = np.random.default_rng(seed)
    H, W = 2 * hh, 2 * ww
    if flat:
        rgb = np.full((n, 3, H, W), 0.2501, F)
    else:
        ramp = np.linspace(-0.93, 0.93, H * W, dtype=np.float64).reshape(H, W)
        rgb = (ramp[None, None] * np.array([1.0, 0.9, 0.8]).reshape(1, 3, 1, 1) + rng.normal(0, 0.01, (n, 3, H, W))).astype(F)
    packed = (remosaic(rgb, pattern) + rng.normal(0, 0.02, (n, 4, hh, ww))).astype(F)
    if not flat:
        # cell (0, 0): outputs outside [-1,1] on both sides and one at the top of the range (in all three colours, so that whatever
        # the pattern the sites are read), and noisy samples that put the residual at both clamps (more than 4 * 2^bits DN away)
        rgb[:, :, 0, 0], rgb[:, :, 0, 1], rgb[:, :, 1, 0] = F(1.3), F(-1.2), F(1.0)
        packed[:, 0, 0, 0], packed[:, 1, 0, 0] = F(9.5), F(-9.5)
    rq, j, _ = sample_terms(packed, rgb, pattern, bits)
    acc = resid_ref(packed, rgb, pattern, bits)
    used = int((total(acc)["n"] > 0).sum())
    classes = set()
    if used == 1:
        classes.add("flat")
    if used >= 8:
        classes.add("many_bins")
    if (np.abs(rgb) > 1).any() and (rq == CLAMP).any() and (rq == -CLAMP).any():
        classes.add("clamped")
    if (rq < 0).any() and (acc["s1"] < 0).any() and (ww == 1 or (acc["s11"] < 0).any()):
        classes.add("negative")
    classes.add("edge_pair")
    if ww > 1:
        classes.add("pairs")
        assert int(acc["n11"].sum()) == n * 4 * hh * (ww - 1), "make_case: every cell but a row's last has a pair"
    if n > 1:
        classes.add("batch")
    return packed, rgb, classes


def ramp_rgb(hh, ww, bits, lo=0.10, hi=0.88):
    """a clean frame [1,3,2hh,2ww] whose levels ramp from `lo` to `hi` of the range along x, the same in the three colours"""
    v = np.linspace(2 * lo - 1, 2 * hi - 1, 2 * ww, dtype=np.float64)
    return np.broadcast_to(v.astype(F), (1, 3, 2 * hh, 2 * ww)).copy()


def noisy_of(rgb, pattern, bits, a, b, seed, gain=1.0):
    """packed frames: the re-mosaic of `rgb` plus white Gaussian noise of variance gain^2 * (a * m - b) at level m (DN of `bits`)"""
    top = 2.0 ** bits - 1
    clean = (remosaic(rgb, pattern).astype(np.float64) + 1) * 0.5 * top
    var = np.maximum(a * clean - b, 0.0)
    dn = clean + gain * np.sqrt(var) * np.random.default_rng(seed).normal(size=clean.shape)
    return (2 * (dn / top) - 1).astype(F)


# (n, hh, ww) of the parity cases: one cell; a row that is no multiple of 4; a batch on a wide shape of more than one workgroup's
# stride per wave; odd width with rows that end inside a wave; the wide shape that is also run off the 16-byte boundary
SHAPES = [(1, 1, 1), (1, 2, 3), (3, 16, 20), (2, 18, 17), (1, 16, 24)]
BIT_DEPTHS = (10, 12, 14, 16)
