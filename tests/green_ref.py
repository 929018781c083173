"""The green-imbalance rule of include/rvdd.h (rvdd_green_estimate, rvdd_green_fit, rvdd_green_apply) restated in NumPy float32, every
operation rounded on its own, and the inputs the host and GPU tests share.  estimate() / fit() / apply() are vectorised;
estimate_slow() / fit_slow() / apply_slow() say the same with plain loops and np.float32 scalars, written from the rule's text and
not from the vectorised form (tests/test_green_host.py holds the two together word for word)."""
import functools

import numpy as np

from line_ref import dn, f32, gray_of, norm_dn, packed_of, top_of      # noqa: F401 -- the tests read them here

BLOCK = 32
PATTERNS = ("gbrg", "grbg", "rggb", "bggr")
SKIPPED, APPLIED = 0, 1
UNSUPPORTED, FIT_APPLIED, FIT_CLAMPED, INSIGNIFICANT = 0, 1, 2, 3
VAR_MEDIAN = f32(3.4528)                # (1.4826 * 1.2533)^2: the variance of a median in units of MAD^2
SE_MEDIAN = f32(1.2533) * f32(1.4826)   # the standard error of a median in units of MAD / sqrt(n)
HALF = f32(0.5)

# (n, hh, ww) of the GPU test: one sample a side; odd and small; one whole block; a partial block whose B side (a row below) or whose
# column side has no sample and must be skipped; two frames of partial blocks; more blocks than one either way; whole blocks; one row
# and column over; the four-cell apply
SHAPES = [(1, 2, 2), (1, 5, 7), (1, 32, 32), (1, 33, 32), (1, 32, 33), (2, 31, 33), (2, 37, 53), (1, 64, 96), (1, 65, 129), (1, 8, 640)]


def geometry(pattern):
    """-> (plane A, plane B, dx): A the green plane of CFA row 0, B that of CFA row 1, dx = -1 where A sits in CFA column 0, else +1"""
    a = 0 if PATTERNS.index(pattern) < 2 else 1
    return a, 3 - a, (-1 if a == 0 else 1)


def grid(hh, ww):
    return (hh + BLOCK - 1) // BLOCK, (ww + BLOCK - 1) // BLOCK


def cfg(k_gate, noise_a, noise_b, var_floor=1.0, black=None):
    """the five fields of struct rvdd_green_cfg, as f32; black None: noise_b / noise_a (0 for a curve without a slope)"""
    if black is None:
        black = noise_b / noise_a if noise_a else 0.0
    return tuple(f32(v) for v in (k_gate, noise_a, noise_b, var_floor, black))


def _shifted(plane, dr, dc):
    """plane [n,hh,ww] -> (its values at (r + dr, c + dc), whether that cell lies in the plane)"""
    n, hh, ww = plane.shape
    r, c = np.arange(hh) + dr, np.arange(ww) + dc
    ok = ((r >= 0) & (r < hh))[:, None] & ((c >= 0) & (c < ww))[None, :]
    return plane[:, np.clip(r, 0, hh - 1)][:, :, np.clip(c, 0, ww - 1)], np.broadcast_to(ok, plane.shape)


def samples(packed, bits, c, pattern):
    """-> per side (A, B): {"is": whether the cell is a sample, "d", "m", "used"}, each [n,hh,ww]"""
    k_gate, a, b, floor = c[:4]
    pa, pb, dx = geometry(pattern)
    x = dn(packed, top_of(bits))
    out = []
    for own, other, drs, dcs in ((x[:, pa], x[:, pb], (0, -1), (0, dx)), (x[:, pb], x[:, pa], (0, 1), (0, -dx))):
        nb, ok = zip(*[_shifted(other, dr, dc) for dr in drs for dc in dcs])
        s = np.sort(np.stack(nb), axis=0)
        m = (s[1] + s[2]) * HALF
        d = own - m
        var = np.maximum(a * m - b, floor)
        valid = np.logical_and.reduce(ok)
        out.append({"is": valid, "d": d, "m": m, "used": valid & (d * d <= (k_gate * k_gate) * var)})
    return out


def _median(v):
    v = np.sort(v)
    return (v[(v.size - 1) // 2] + v[v.size // 2]) * HALF


def estimate(packed, bits, c, pattern):
    """-> {"e", "level": f32 [n,gh,gw], "state": u8 [n,gh,gw], "cnt", "tot": the used samples and the samples [n,2,gh,gw]}"""
    n, _, hh, ww = packed.shape
    assert packed.dtype == np.float32 and hh >= 2 and ww >= 2
    gh, gw = grid(hh, ww)
    sides = samples(packed, bits, c, pattern)
    e, level = np.zeros((n, gh, gw), np.float32), np.zeros((n, gh, gw), np.float32)
    state = np.zeros((n, gh, gw), np.uint8)
    cnt, tot = np.zeros((n, 2, gh, gw), np.int64), np.zeros((n, 2, gh, gw), np.int64)
    for i in range(n):
        for by in range(gh):
            for bx in range(gw):
                blk = (i, slice(by * BLOCK, (by + 1) * BLOCK), slice(bx * BLOCK, (bx + 1) * BLOCK))
                ds, S = [], 0
                for j, sd in enumerate(sides):
                    u = sd["used"][blk]
                    tot[i, j, by, bx], cnt[i, j, by, bx] = sd["is"][blk].sum(), u.sum()
                    ds.append(sd["d"][blk][u])
                    S += int(np.rint(sd["m"][blk][u]).astype(np.int64).sum())
                ca, cb = cnt[i, :, by, bx]
                ta, tb = tot[i, :, by, bx]
                if ca > 0 and cb > 0 and 2 * ca >= ta and 2 * cb >= tb:
                    e[i, by, bx] = (_median(ds[0]) - _median(ds[1])) * HALF
                    level[i, by, bx] = f32(float(S) / float(ca + cb))
                    state[i, by, bx] = APPLIED
    return {"e": e, "level": level, "state": state, "cnt": cnt, "tot": tot}


def pooled(v, need, k_sig, limit, zero_is_nothing=True):
    """rvdd_cols_fit's pooled step over the f32 values v -> (mstate, value, o, se)"""
    nf = v.size
    if nf < need:
        return UNSUPPORTED, f32(0), f32(0), f32(0)
    v = np.sort(v)
    o = (v[(nf - 1) // 2] + v[nf // 2]) * HALF
    a = np.sort(np.abs(v - o))
    mad = (a[(nf - 1) // 2] + a[nf // 2]) * HALF
    se = (SE_MEDIAN * mad) / np.sqrt(f32(nf))
    if (zero_is_nothing and o == 0) or (o * o) * f32(nf) < (k_sig * k_sig) * (VAR_MEDIAN * (mad * mad)):
        return INSIGNIFICANT, f32(0), o, se
    oc = np.minimum(np.maximum(o, -limit), limit)
    return (FIT_CLAMPED if oc != o else FIT_APPLIED), oc, o, se


def fit(e, level, state, black, min_frames, k_sig, max_gain, min_signal):
    """-> {"map": f32 [gh,gw], "mstate": u8 [gh,gw], "stats": the counts by state, sum_q2, floor and the flat estimate}"""
    F, gh, gw = e.shape
    black, k_sig, max_gain, min_signal = f32(black), f32(k_sig), f32(max_gain), f32(min_signal)
    gmap, mstate = np.zeros((gh, gw), np.float32), np.zeros((gh, gw), np.uint8)
    counts, sum_q2, floor_sum, os = [0, 0, 0, 0], 0, 0.0, []
    for by in range(gh):
        for bx in range(gw):
            signal = level[:, by, bx] - black
            keep = (state[:, by, bx] == APPLIED) & (signal >= min_signal)
            ms, value, o, se = pooled(e[:, by, bx][keep] / signal[keep], max(1, min_frames), k_sig, max_gain)
            gmap[by, bx], mstate[by, bx] = value, ms
            counts[ms] += 1
            if ms == UNSUPPORTED:
                continue
            floor_sum += float(se)
            os.append(o)
            if ms != INSIGNIFICANT:
                q = int(np.rint(f32(16384.0) * value))
                sum_q2 += q * q
    fs, fv, _, fse = pooled(np.array(os, np.float32), 1, k_sig, max_gain)
    stats = {"unsupported": counts[0], "applied": counts[1], "clamped": counts[2], "insignificant": counts[3], "sum_q2": sum_q2,
             "floor": floor_sum / len(os) if os else 0.0, "flat_gain": float(fv), "flat_se": float(fse), "flat_state": int(fs)}
    return {"map": gmap, "mstate": mstate, "stats": stats}


def _axis(count, blocks):
    """-> (i0, i1, w) of the `count` cells along one axis of a map of `blocks` blocks"""
    f = np.clip((np.arange(count, dtype=np.float32) + HALF) * f32(1.0 / BLOCK) - HALF, f32(0), f32(blocks - 1))
    i0 = f.astype(np.int64)
    return i0, np.minimum(i0 + 1, blocks - 1), f - i0.astype(np.float32)


def gains(gmap, hh, ww):
    """the map [gh,gw] (the frame's grid, or [1,1]) interpolated to one gain per cell [hh,ww]"""
    gh, gw = gmap.shape
    assert (gh, gw) in ((1, 1), grid(hh, ww)) and gmap.dtype == np.float32
    y0, y1, wy = _axis(hh, gh)
    x0, x1, wx = _axis(ww, gw)
    t = gmap[y0][:, x0] + wx[None, :] * (gmap[y0][:, x1] - gmap[y0][:, x0])
    u = gmap[y1][:, x0] + wx[None, :] * (gmap[y1][:, x1] - gmap[y1][:, x0])
    return t + wy[:, None] * (u - t)


def apply(packed, gray, gmap, black, bits, pattern):
    """-> (packed, gray) with the gains taken out of the two green planes where they are not zero: copies; gray may be None"""
    n, _, hh, ww = packed.shape
    pa, pb, _ = geometry(pattern)
    top, black = top_of(bits), f32(black)
    g = gains(gmap, hh, ww)
    h = HALF * g
    hit = np.broadcast_to(g != 0, (n, hh, ww))
    d = dn(packed, top)
    new = d.copy()
    new[:, pa] = d[:, pa] - h * (d[:, pa] - black)
    new[:, pb] = d[:, pb] + h * (d[:, pb] - black)
    out = packed.copy()
    for k in (pa, pb):
        out[:, k][hit] = norm_dn(new[:, k], top)[hit]
    go = None if gray is None else gray.copy()
    if go is not None:
        go[hit] = ((((new[:, 0] + new[:, 1]) + new[:, 2]) + new[:, 3]) * f32(0.25))[hit]
    return out, go


# ---- the same, slowly: plain loops over the rule's text -------------------------------------------------------------------------------
def _dn1(v, top):
    return f32(f32(f32(v + f32(1.0)) * f32(0.5)) * top)


def estimate_slow(packed, bits, c, pattern):
    k_gate, a, b, floor = c[:4]
    k2 = f32(k_gate * k_gate)
    top = top_of(bits)
    n, _, hh, ww = packed.shape
    gh, gw = grid(hh, ww)
    p = PATTERNS.index(pattern)
    A, B = (0, 3) if p < 2 else (1, 2)
    dx = -1 if A & 1 == 0 else 1
    e, level = np.zeros((n, gh, gw), np.float32), np.zeros((n, gh, gw), np.float32)
    state = np.zeros((n, gh, gw), np.uint8)
    for i in range(n):
        for by in range(gh):
            for bx in range(gw):
                ds, tots, S = ([], []), [0, 0], 0
                for r in range(by * BLOCK, min(hh, (by + 1) * BLOCK)):
                    for col in range(bx * BLOCK, min(ww, (bx + 1) * BLOCK)):
                        for side, (own, other, cells) in enumerate((
                                (A, B, [(r, col), (r, col + dx), (r - 1, col), (r - 1, col + dx)]),
                                (B, A, [(r, col), (r, col - dx), (r + 1, col), (r + 1, col - dx)]))):
                            if not all(0 <= rr < hh and 0 <= cc < ww for rr, cc in cells):
                                continue
                            tots[side] += 1
                            s = sorted(_dn1(packed[i, other, rr, cc], top) for rr, cc in cells)
                            m = f32(f32(s[1] + s[2]) * f32(0.5))
                            d = f32(_dn1(packed[i, own, r, col], top) - m)
                            var = max(f32(f32(a * m) - b), floor)
                            if f32(d * d) <= f32(k2 * var):
                                ds[side].append(d)
                                S += int(np.rint(m))
                ca, cb = len(ds[0]), len(ds[1])
                if ca > 0 and cb > 0 and 2 * ca >= tots[0] and 2 * cb >= tots[1]:
                    med = []
                    for v in ds:
                        v.sort()
                        med.append(f32(f32(v[(len(v) - 1) // 2] + v[len(v) // 2]) * f32(0.5)))
                    e[i, by, bx] = f32(f32(med[0] - med[1]) * f32(0.5))
                    level[i, by, bx] = f32(float(S) / float(ca + cb))
                    state[i, by, bx] = 1
    return {"e": e, "level": level, "state": state}


def _pooled_slow(v, need, k2, limit):
    nf = len(v)
    if nf < need:
        return 0, f32(0), f32(0), f32(0)
    v = sorted(v)
    o = f32(f32(v[(nf - 1) // 2] + v[nf // 2]) * f32(0.5))
    a = sorted(f32(abs(f32(x - o))) for x in v)
    mad = f32(f32(a[(nf - 1) // 2] + a[nf // 2]) * f32(0.5))
    se = f32(f32(SE_MEDIAN * mad) / f32(np.sqrt(f32(nf))))
    if o == 0 or f32(f32(o * o) * f32(nf)) < f32(k2 * f32(VAR_MEDIAN * f32(mad * mad))):
        return 3, f32(0), o, se
    oc = min(max(o, f32(-limit)), limit)
    return (2 if oc != o else 1), oc, o, se


def fit_slow(e, level, state, black, min_frames, k_sig, max_gain, min_signal):
    F, gh, gw = e.shape
    black, k_sig, max_gain, min_signal = f32(black), f32(k_sig), f32(max_gain), f32(min_signal)
    k2 = f32(k_sig * k_sig)
    gmap, mstate = np.zeros((gh, gw), np.float32), np.zeros((gh, gw), np.uint8)
    counts, sum_q2, floor_sum, os = [0, 0, 0, 0], 0, 0.0, []
    for by in range(gh):
        for bx in range(gw):
            v = []
            for i in range(F):
                signal = f32(level[i, by, bx] - black)
                if state[i, by, bx] == 1 and signal >= min_signal:
                    v.append(f32(e[i, by, bx] / signal))
            ms, value, o, se = _pooled_slow(v, max(1, min_frames), k2, max_gain)
            gmap[by, bx], mstate[by, bx] = value, ms
            counts[ms] += 1
            if ms == 0:
                continue
            floor_sum += float(se)
            os.append(o)
            if ms != 3:
                q = int(np.rint(f32(f32(16384.0) * value)))
                sum_q2 += q * q
    fs, fv, _, fse = _pooled_slow(os, 1, k2, max_gain)
    stats = {"unsupported": counts[0], "applied": counts[1], "clamped": counts[2], "insignificant": counts[3], "sum_q2": sum_q2,
             "floor": floor_sum / len(os) if os else 0.0, "flat_gain": float(fv), "flat_se": float(fse), "flat_state": int(fs)}
    return {"map": gmap, "mstate": mstate, "stats": stats}


def apply_slow(packed, gray, gmap, black, bits, pattern):
    n, _, hh, ww = packed.shape
    gh, gw = gmap.shape
    p = PATTERNS.index(pattern)
    A, B = (0, 3) if p < 2 else (1, 2)
    top, black = top_of(bits), f32(black)
    out, go = packed.copy(), gray.copy()

    def along(i, blocks):
        f = f32(f32(f32(f32(i) + f32(0.5)) * f32(0.03125)) - f32(0.5))
        f = min(max(f, f32(0)), f32(blocks - 1))
        i0 = int(f)
        return i0, min(i0 + 1, blocks - 1), f32(f - f32(i0))

    for r in range(hh):
        y0, y1, wy = along(r, gh)
        for col in range(ww):
            x0, x1, wx = along(col, gw)
            t = f32(gmap[y0, x0] + f32(wx * f32(gmap[y0, x1] - gmap[y0, x0])))
            u = f32(gmap[y1, x0] + f32(wx * f32(gmap[y1, x1] - gmap[y1, x0])))
            g = f32(t + f32(wy * f32(u - t)))
            if g == 0:
                continue
            h = f32(f32(0.5) * g)
            for i in range(n):
                total = None
                for k in range(4):
                    d = _dn1(packed[i, k, r, col], top)
                    if k == A:
                        d = f32(d - f32(h * f32(d - black)))
                    elif k == B:
                        d = f32(d + f32(h * f32(d - black)))
                    if k in (A, B):
                        out[i, k, r, col] = f32(f32(f32(2.0) * f32(d / top)) - f32(1.0))
                    total = d if total is None else f32(total + d)
                go[i, r, col] = f32(total * f32(0.25))
    return out, go


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def scene(n, hh, ww, seed, pattern, level=1800.0, swing=600.0, move=3.0):
    """a smooth scene in DN sampled at the mosaic's sites, [n,4,hh,ww] f64: the two green planes see the same light, the other two
    0.8 of it + 50 and 0.9 of it; it moves `move` cells a frame (tests/test_cols_host.py's scene)"""
    pa, pb, _ = geometry(pattern)
    r, c = np.mgrid[0:hh, 0:ww].astype(np.float64)
    out = np.empty((n, 4, hh, ww))
    for i in range(n):
        for k in range(4):
            y, x = r + 0.5 * (k >> 1) + move * i, c + 0.5 * (k & 1) + move * i + seed
            base = level + swing * np.sin(x / 11.0) * np.cos(y / 17.0) + 0.25 * swing * np.sin(x / 7.0 + y / 5.0)
            out[i, k] = base if k in (pa, pb) else (0.8 * base + 50.0 if k < 2 else 0.9 * base)
    return out


def imbalanced(clean, gain, black, pattern):
    """clean DN [n,4,hh,ww] with plane A raised and plane B lowered by half of `gain` (a number, or [hh,ww]) of the signal above black"""
    pa, pb, _ = geometry(pattern)
    out = clean.copy()
    out[:, pa] = clean[:, pa] + 0.5 * gain * (clean[:, pa] - black)
    out[:, pb] = clean[:, pb] - 0.5 * gain * (clean[:, pb] - black)
    return out


def cases(shape):
    """The inputs of one shape: [(name, packed f32 [n,4,hh,ww], bit depth, cfg, pattern)] -- a noisy scene with 3 % imbalance (12 bits,
    GBRG); a constant frame, where every d is equal (10 bits, RGGB); a frame with defects, a hard edge and a field of fine texture,
    so that some blocks fall under half (16 bits, RGGB); coarsely quantised DN (10 bits scaled down to a few levels, GBRG)."""
    n, hh, ww = shape
    rng = np.random.default_rng(4000 * n + 10 * hh + ww)
    out = []
    clean = imbalanced(scene(n, hh, ww, ww, "gbrg"), 0.03, 250.0, "gbrg")
    out.append(("scene12", packed_of(clean + rng.normal(0.0, 40.0, clean.shape), 12), 12, cfg(3.0, 1.0, 250.0, 1.0), "gbrg"))
    out.append(("constant", packed_of(np.full((n, 4, hh, ww), 517.0), 10), 10, cfg(3.0, 2.0, 128.0, 1.0), "rggb"))
    rough = imbalanced(scene(n, hh, ww, 5, "rggb", level=28000.0, swing=9000.0), -0.02, 4000.0, "rggb") + rng.normal(0.0, 600.0, (n, 4, hh, ww))
    rough[:, :, :, ww // 2:] += 12000.0                                   # a hard vertical edge
    chk = (np.add.outer(np.arange(hh), np.arange(ww)) & 1) * 2.0 - 1.0
    rough[:, 1, hh // 2:, :] += 9000.0 * chk[hh // 2:]                    # texture finer than two cells in plane A: the lower half falls out of the gate
    for _ in range(max(1, hh * ww // 50)):                                # defects
        rough[rng.integers(n), rng.integers(4), rng.integers(hh), rng.integers(ww)] = rng.choice([0.0, 65535.0])
    out.append(("rough16", packed_of(rough, 16), 16, cfg(3.0, 12.0, 48000.0, 1.0), "rggb"))
    coarse = np.rint((imbalanced(scene(n, hh, ww, 9, "gbrg", level=500.0, swing=300.0), 0.05, 64.0, "gbrg") + rng.normal(0.0, 20.0, (n, 4, hh, ww))) / 32.0) * 32.0
    out.append(("coarse10", packed_of(coarse, 10), 10, cfg(3.0, 1.0, 64.0, 1.0), "gbrg"))
    return out


POISON = f32(7.0)                      # a gray value no frame has: cells that must not be written keep it
MAX_GAIN = 0.04                        # the clamp of the tests' maps: the 5 % of "coarse10" meets it, the 3 % of "scene12" does not


def map_for(est, c, bits):
    """the map a shape's apply takes out: the fit of the shape's own frames with k_sig = 0 (every supported block), then the first
    column of blocks zero -- or, in a map one block wide, the first row -- and two neighbouring columns further on, so that there are
    whole runs of cells with a gain of exactly zero; a map that would be all zero (a constant frame) gets 1 / 32 in its last block"""
    gmap = fit(est["e"], est["level"], est["state"], c[4], 1, 0.0, MAX_GAIN, float(top_of(bits)) / 64.0)["map"]
    gh, gw = gmap.shape
    if gw > 1:
        gmap[:, 0] = 0
    elif gh > 1:
        gmap[0, :] = 0
    if gw > 7:
        gmap[:, 5:7] = 0
    if not gmap.any():
        gmap[-1, -1] = f32(0.03125)
    return gmap


@functools.lru_cache(maxsize=None)
def refs(shape):
    """the restatement of every input of one shape, computed once for the host and the GPU tests: [{name, packed, bits, cfg, pattern,
    est, map, gray (every second column poisoned), packed_out, gray_out}]"""
    out = []
    for name, packed, bits, c, pattern in cases(shape):
        est = estimate(packed, bits, c, pattern)
        gmap = map_for(est, c, bits)
        gray = gray_of(packed, bits)
        gray[:, :, ::2] = POISON
        p2, g2 = apply(packed, gray, gmap, c[4], bits, pattern)
        out.append(dict(name=name, packed=packed, bits=bits, cfg=c, pattern=pattern, est=est, map=gmap, gray=gray, packed_out=p2, gray_out=g2))
    return out
