"""NumPy restatement of rvdd_dpc (include/rvdd.h): dynamic defective-pixel correction of packed raw frames, every operation in
explicit float32, the order statistics from np.sort -- and the synthetic frames with injected defects the tests share."""
import numpy as np

F = np.float32
ISO_CURVES = {3200: (8.0034, 2043.51144), 12800: (28.3015, 6307.62081)}      # var(m) = ka m - kb in 12-bit DN (the reference's)


def iso_curve(iso, bit_depth):
    """(a, b) of `iso` in DN of `bit_depth`, formed in double: a = s ka, b = s^2 kb with s = (2^bit_depth - 1) / 4095"""
    ka, kb = ISO_CURVES[iso]
    s = (2 ** bit_depth - 1) / 4095.0
    return s * ka, s * s * kb


def _mirror(n, d):
    """indices i + d for i in 0 .. n-1, mirrored about the site where they leave the plane: -1 -> +1, n -> n - 2"""
    i = np.arange(n) + d
    i[i < 0] = 1
    i[i >= n] = n - 2
    return i


def dpc_ref(packed, gray, bit_depth, k_hot, k_dead, noise_a, noise_b, var_floor=1.0, counts=None):
    """packed [n,4,hh,ww] f32, gray [n,hh,ww] f32 or None, counts [n,2] or None (added to)
    -> (packed_out, gray_out, counts_out, hot [n,4,hh,ww] bool, dead [n,4,hh,ww] bool)"""
    p = np.ascontiguousarray(packed, dtype=F)
    n, four, hh, ww = p.shape
    assert four == 4 and hh >= 2 and ww >= 2
    top = F(2 ** bit_depth - 1)
    k_hot, k_dead, a, b, floor = F(k_hot), F(k_dead), F(noise_a), F(noise_b), F(var_floor)
    dn = ((p + F(1.0)) * F(0.5)) * top
    nb = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                nb.append(dn[:, :, _mirror(hh, dy)][:, :, :, _mirror(ww, dx)])
    s = np.sort(np.stack(nb, 0), axis=0)
    lo, s3, s4, hi = s[0], s[3], s[4], s[7]
    m = (s3 + s4) * F(0.5)
    var = np.maximum(a * m - b, floor)
    with np.errstate(over="ignore"):
        k2h, k2d = k_hot * k_hot, k_dead * k_dead          # 1e18 squared is +inf: nothing is above it
        dh, dl = dn - hi, lo - dn
        hot = (dh > F(0)) & (dh * dh > k2h * var) if k_hot > 0 else np.zeros(p.shape, bool)
        dead = (dl > F(0)) & (dl * dl > k2d * var) if k_dead > 0 else np.zeros(p.shape, bool)
    flag = hot | dead
    for x in (dn, m, var, dh, dl):
        assert x.dtype == F
    out = p.copy()
    fixed = F(2.0) * (m / top) - F(1.0)
    out[flag] = fixed[flag]
    g = None
    if gray is not None:
        g = np.array(gray, dtype=F, copy=True)
        d = np.where(flag, m, dn)
        re = (((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) * F(0.25)
        cell = flag.any(axis=1)
        g[cell] = re[cell]
    c = np.zeros((n, 2), np.int64) if counts is None else np.array(counts, dtype=np.int64, copy=True)
    c[:, 0] += hot.sum(axis=(1, 2, 3))
    c[:, 1] += dead.sum(axis=(1, 2, 3))
    return out, g, c, hot, dead


def ingest(cells, bit_depth):
    """[n,hh,ww,4] DN -> (packed [n,4,hh,ww], gray [n,hh,ww]): rvdd_ingest_raw's arithmetic (stream_ref.ingest_ref)"""
    c = np.asarray(cells, dtype=F)
    packed = (F(2.0) * (c / F(2 ** bit_depth - 1)) - F(1.0)).transpose(0, 3, 1, 2)
    gray = (((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]) * F(0.25)
    return np.ascontiguousarray(packed), np.ascontiguousarray(gray)


def noisy_cells(n, hh, ww, bit_depth, iso, seed, level=0.45):
    """whole-DN frames [n,hh,ww,4] f32: a flat scene at level * top with a gentle ramp, noise of the ISO curve, rounded and clipped"""
    rng = np.random.default_rng(seed)
    top = 2 ** bit_depth - 1
    a, b = iso_curve(iso, bit_depth)
    ramp = np.linspace(-0.05, 0.05, ww)[None, None, :, None] + np.linspace(-0.03, 0.03, hh)[None, :, None, None]
    m = (level + ramp) * top * np.ones((n, hh, ww, 4))
    z = rng.standard_normal(m.shape)
    return np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0.0)) * z), 0, top).astype(F)


def inject(cells, bit_depth):
    """Defects written into `cells` [n,hh,ww,4] in place.  -> [(class, frame, plane, y, x, kind)], kind "hot" (the sample is
    2^bit_depth - 1), "dead" (0) or "marginal" (the largest of its eight neighbours plus one DN: above hi, far below any threshold).
    No two injected sites of a plane are neighbours except the "pair"; the classes:
      corner / edge: at the four corners and on the edges (hh >= 3 and ww >= 5 for edges), spread over the planes so that every plane
      has one ("plane0" .. "plane3"); pair: a hot and a dead sample that are same-colour neighbours of each other, and marginal,
      on frames of at least 8 x 8 cells; batch: one in the last frame of a batch."""
    n, hh, ww, _ = cells.shape
    top = F(2 ** bit_depth - 1)
    sites = []

    def put(cls, i, k, y, x, kind):
        cells[i, y, x, k] = top if kind == "hot" else F(0)
        sites.append((cls, i, k, y, x, kind))

    put("corner", 0, 0, 0, 0, "hot")
    put("corner", 0, 1, 0, ww - 1, "dead")
    put("corner", 0, 2, hh - 1, 0, "hot")
    put("corner", 0, 3, hh - 1, ww - 1, "dead")
    if hh >= 3 and ww >= 5:
        put("edge", 0, 2, 0, ww // 2, "hot")             # top (the plane's corner site is two columns away at least)
        put("edge", 0, 3, hh // 2, 0, "dead") if hh >= 5 else put("edge", 0, 0, hh - 1, ww // 2, "dead")
        put("edge", 0, 1, hh - 1, ww // 2, "dead")       # bottom
        put("edge", 0, 0, hh // 2, ww - 1, "hot") if hh >= 5 else put("edge", 0, 3, 0, ww // 2, "hot")
        if hh >= 5:
            put("edge", 0, 1, hh // 2, 0, "hot")         # left
    if hh >= 8 and ww >= 8:
        put("pair", 0, 0, 4, 3, "hot")
        put("pair", 0, 0, 4, 4, "dead")
        y, x, k = 5, 4, 1
        nb = [cells[0, y + dy, x + dx, k] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]
        cells[0, y, x, k] = min(max(nb) + F(1), top)
        sites.append(("marginal", 0, k, y, x, "marginal"))
    if n > 1:
        put("batch", n - 1, 2, 1, 1, "hot")
    for k in range(4):
        assert any(s[2] == k for s in sites)
    return sites


def make_case(n, hh, ww, bit_depth, iso, seed):
    """-> (packed, gray, sites): ingested noisy frames with the defects of `inject`"""
    cells = noisy_cells(n, hh, ww, bit_depth, iso, seed)
    sites = inject(cells, bit_depth)
    packed, gray = ingest(cells, bit_depth)
    return packed, gray, sites


def check_sites(sites, hot, dead):
    """The reference alone: every injected hot / dead sample is flagged as that, every marginal one is refused although it lies
    above its neighbours.  -> the classes that produced a flag or (marginal) a refusal"""
    seen = set()
    for cls, i, k, y, x, kind in sites:
        if kind == "marginal":
            assert not hot[i, k, y, x] and not dead[i, k, y, x], (cls, i, k, y, x)
        else:
            assert (hot if kind == "hot" else dead)[i, k, y, x], (cls, kind, i, k, y, x)
            seen.add("plane%d" % k)
        seen.add(cls)
    return seen
