"""NumPy restatements of the static defect map (include/rvdd.h: rvdd_dpc_detect, the threshold, rvdd_dpc_map_apply,
rvdd_dpc_map_stats), every operation in explicit float32, the order statistics from np.sort -- and the frames with injected STATIC
defects (the same sites in every frame) the tests share."""
import math

import numpy as np

import dpc_ref as R

F = np.float32
RING1 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]
RING2 = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if max(abs(dy), abs(dx)) == 2]      # dy outer, dx inner, ascending


def detect_ref(packed, bit_depth, k_hot, k_dead, noise_a, noise_b, var_floor=1.0, tolerate=0, hits=None):
    """packed [n,4,hh,ww] f32; hits uint32 [4,hh,ww] or None (added to, each half saturating at 65535)
    -> (hits_out uint32 [4,hh,ww], hot [n,4,hh,ww] bool, dead [n,4,hh,ww] bool)"""
    p = np.ascontiguousarray(packed, dtype=F)
    n, four, hh, ww = p.shape
    assert four == 4 and hh >= 2 and ww >= 2 and 0 <= tolerate <= 3
    top = F(2 ** bit_depth - 1)
    k_hot, k_dead, a, b, floor = F(k_hot), F(k_dead), F(noise_a), F(noise_b), F(var_floor)
    dn = ((p + F(1.0)) * F(0.5)) * top
    nb = [dn[:, :, R._mirror(hh, dy)][:, :, :, R._mirror(ww, dx)] for dy, dx in RING1]
    s = np.sort(np.stack(nb, 0), axis=0) if n else np.zeros((8,) + p.shape, F)
    m = (s[3] + s[4]) * F(0.5)
    var = np.maximum(a * m - b, floor)
    with np.errstate(over="ignore"):
        k2h, k2d = k_hot * k_hot, k_dead * k_dead
        dh, dl = dn - s[7 - tolerate], s[tolerate] - dn
        hot = (dh > F(0)) & (dh * dh > k2h * var) if k_hot > 0 else np.zeros(p.shape, bool)
        dead = (dl > F(0)) & (dl * dl > k2d * var) if k_dead > 0 else np.zeros(p.shape, bool)
    for x in (dn, m, var, dh, dl):
        assert x.dtype == F
    old = np.zeros((4, hh, ww), np.uint32) if hits is None else np.asarray(hits).view(np.uint32).reshape(4, hh, ww)
    lo = np.minimum((old & 0xffff).astype(np.int64) + hot.sum(axis=0), 65535)
    hi = np.minimum((old >> 16).astype(np.int64) + dead.sum(axis=0), 65535)
    return (lo | hi << 16).astype(np.uint32), hot, dead


def map_from_hits(hits, frames, share):
    """-> (cellmask uint8 [hh,ww], hot [4,hh,ww] bool, dead [4,hh,ww] bool): defective iff hot, or dead, in ceil(share frames) frames"""
    w = np.asarray(hits).view(np.uint32)
    need = max(1, math.ceil(share * frames))
    hot, dead = (w & 0xffff) >= need, (w >> 16) >= need
    return mask_of(hot | dead), hot, dead


def mask_of(bad):
    """bool [4,hh,ww] -> cellmask uint8 [hh,ww]"""
    m = np.zeros(bad.shape[1:], np.uint8)
    for k in range(4):
        m |= bad[k].astype(np.uint8) << k
    return m


def planes_of(mask):
    """cellmask -> bool [4,hh,ww]"""
    return np.stack([(mask >> k) & 1 for k in range(4)]).astype(bool)


def to_mosaic(mask):
    out = np.zeros((2 * mask.shape[0], 2 * mask.shape[1]), np.uint8)
    for k in range(4):
        out[k >> 1::2, k & 1::2] = ((mask >> k) & 1) * 255
    return out


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * (n - 1) - i if i >= n else i


def site_plan(mask, k, y, x):
    """-> (ring, [(yy, xx)]): the first ring (1, 2) of the sample with a good site and its good sites; (0, []) = unfixable"""
    hh, ww = mask.shape
    for ring, offs in ((1, RING1), (2, RING2)):
        at = [(_reflect(y + dy, hh), _reflect(x + dx, ww)) for dy, dx in offs]
        good = [(yy, xx) for yy, xx in at if not (mask[yy, xx] >> k) & 1]
        if good:
            return ring, good
    return 0, []


def apply_ref(packed, gray, mask, bit_depth):
    """packed [n,4,hh,ww] f32, gray [n,hh,ww] f32 or None, mask uint8 [hh,ww] -> (packed_out, gray_out, kinds) with kinds
    {(k, y, x): (ring, q)} of every defective sample (ring 0 = unfixable)"""
    p = np.array(packed, dtype=F, copy=True)
    n, four, hh, ww = p.shape
    assert four == 4 and hh >= 3 and ww >= 3 and mask.shape == (hh, ww) and mask.dtype == np.uint8 and not (mask & 0xf0).any()
    top = F(2 ** bit_depth - 1)
    dn = ((np.asarray(packed, dtype=F) + F(1.0)) * F(0.5)) * top
    g = None if gray is None else np.array(gray, dtype=F, copy=True)
    kinds = {}
    for y, x in np.argwhere(mask):
        d = dn[:, :, y, x].copy()
        for k in range(4):
            if not (mask[y, x] >> k) & 1:
                continue
            ring, good = site_plan(mask, k, y, x)
            kinds[(k, int(y), int(x))] = (ring, len(good))
            if not ring:
                continue
            q = len(good)
            s = np.sort(np.stack([dn[:, k, yy, xx] for yy, xx in good], 0), axis=0)
            rep = (s[(q - 1) // 2] + s[q // 2]) * F(0.5)
            assert rep.dtype == F
            p[:, k, y, x] = F(2.0) * (rep / top) - F(1.0)
            d[:, k] = rep
        if g is not None:
            g[:, y, x] = (((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]) * F(0.25)
    return p, g, kinds


def stats_ref(mask):
    """-> (samples, cells, unfixable samples)"""
    samples = cells = unfixable = 0
    for y, x in np.argwhere(mask):
        cells += 1
        for k in range(4):
            if (mask[y, x] >> k) & 1:
                samples += 1
                unfixable += site_plan(mask, k, y, x)[0] == 0
    return samples, cells, unfixable


def inject_static(cells, bit_depth):
    """Static defects written into EVERY frame of `cells` [n,hh,ww,4] in place ("hot": 2^bit_depth - 1, "dead": 0).
    -> [(class, plane, y, x, kind)].  Classes: corner (one per plane) and edge (ww >= 5; four edges with hh >= 5) singles; on frames
    of at least 16 x 16 cells pair (two equal hot neighbours), triple (an L of three), block2 (2 x 2) and block5 (a 5 x 5 block fully
    defective in one plane: its centre is unfixable, its inner ring needs ring 2); on smaller frames instead full (plane 2 defective
    everywhere: all unfixable) and allbut (plane 3 defective everywhere but one site: ring 2 reaches it from the far corner)."""
    n, hh, ww, _ = cells.shape
    top = F(2 ** bit_depth - 1)
    sites = []

    def put(cls, k, y, x, kind):
        cells[:, y, x, k] = top if kind == "hot" else F(0)
        sites.append((cls, k, y, x, kind))

    put("corner", 0, 0, 0, "hot")
    put("corner", 1, 0, ww - 1, "dead")
    put("corner", 2, hh - 1, 0, "hot")
    put("corner", 3, hh - 1, ww - 1, "dead")
    if ww >= 5:
        put("edge", 2, 0, ww // 2, "hot")
        put("edge", 1, hh - 1, ww // 2, "dead")
        if hh >= 5:
            put("edge", 3, hh // 2, 0, "dead")
            put("edge", 0, hh // 2, ww - 1, "hot")
    if hh >= 16 and ww >= 16:
        for x in (3, 4):
            put("pair", 0, 4, x, "hot")
        for y, x in ((8, 3), (8, 4), (9, 3)):
            put("triple", 1, y, x, "hot")
        for y, x in ((12, 3), (12, 4), (13, 3), (13, 4)):
            put("block2", 2, y, x, "hot")
        for y in range(5, 10):
            for x in range(10, 15):
                put("block5", 3, y, x, "hot")
    else:
        have = {(k, y, x) for _, k, y, x, _ in sites}
        for y in range(hh):
            for x in range(ww):
                if (2, y, x) not in have:
                    put("full", 2, y, x, "hot")
                if (3, y, x) not in have and (y, x) != (hh - 1, 0):
                    put("allbut", 3, y, x, "dead")
    return sites


def truth_mask(sites, hh, ww):
    m = np.zeros((hh, ww), np.uint8)
    for _, k, y, x, _ in sites:
        m[y, x] |= 1 << k
    return m


def make_static_case(n, hh, ww, bit_depth, iso, seed):
    """-> (packed, gray, sites, mask): ingested noisy frames with the defects of `inject_static`, and the map of those sites"""
    cells = R.noisy_cells(n, hh, ww, bit_depth, iso, seed)
    sites = inject_static(cells, bit_depth)
    packed, gray = R.ingest(cells, bit_depth)
    return packed, gray, sites, truth_mask(sites, hh, ww)


def speckle_frames(n, hh, ww, bit_depth, iso, seed, shift=(3, 2)):
    """Whole-DN frames [n,hh,ww,4] of a speckled texture, rng.random(...)**6 * 2500 + 300 per sample (12-bit DN, scaled to
    `bit_depth`), translated by `shift` cells per frame (wrapping around), with the noise of the ISO curve"""
    rng = np.random.default_rng(seed)
    top = 2 ** bit_depth - 1
    a, b = R.iso_curve(iso, bit_depth)
    scene = (rng.random((hh, ww, 4)) ** 6 * 2500 + 300) * (top / 4095.0)
    out = np.empty((n, hh, ww, 4), F)
    for i in range(n):
        m = np.roll(scene, (i * shift[0], i * shift[1]), axis=(0, 1))
        z = rng.standard_normal(m.shape)
        out[i] = np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0.0)) * z), 0, top)
    return out
