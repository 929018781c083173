"""NumPy restatement of rvdd_frame_sigs / rvdd_cut_score (include/rvdd.h), integer for integer: the clamp, the product and the rounding in
explicit float32, the counts and sums as integer arrays filled with np.add.at, the score on Python integers converted to double once --
with `find_cuts` restated and the synthetic scenes the tests share."""
import numpy as np

import dpc_ref

F = np.float32
BANDS, COLS, BINS = 16, 16, 64
SIG_BYTES = BANDS * BINS * 4 + BANDS * COLS * 8
T_HIST, T_GRID, MIN_LEN = 0.10, 0.12, 4               # the defaults of python -m rvdd_release_amd.cuts


def cell_keys(gray, bit_depth):
    """gray [...] f32 DN -> (q, j): what a cell adds to its block's sum, and its level bin; int64 arrays"""
    g = np.ascontiguousarray(gray, dtype=F)
    top = F(2 ** bit_depth - 1)
    c = np.minimum(np.maximum(g, F(0)), top)
    c4 = c * F(4.0)
    scaled = c * F(64.0 / 2 ** bit_depth)
    assert c.dtype == F and c4.dtype == F and scaled.dtype == F
    return np.rint(c4).astype(np.int64), np.minimum(scaled.astype(np.int64), BINS - 1)


def frame_sig_ref(gray, bit_depth):
    """rvdd_frame_sigs: gray [n,hh,ww] f32 -> {"hist": uint32 [n,16,64], "sum": uint64 [n,16,16]}"""
    g = np.ascontiguousarray(gray, dtype=F)
    n, hh, ww = g.shape
    assert hh >= 16 and ww >= 16
    q, j = cell_keys(g, bit_depth)
    by = (16 * np.arange(hh, dtype=np.int64)) // hh                   # non-decreasing, every band and column at least once
    bx = (16 * np.arange(ww, dtype=np.int64)) // ww
    assert np.array_equal(np.unique(by), np.arange(BANDS)) and np.array_equal(np.unique(bx), np.arange(COLS))
    keys = (np.arange(n)[:, None, None] * BANDS + by[None, :, None]) * BINS + j
    hist = np.bincount(keys.ravel(), minlength=n * BANDS * BINS).reshape(n, BANDS, BINS)      # integer counts
    # a band is a run of rows and a column a run of cells: int64 sums over the runs
    total = np.add.reduceat(np.add.reduceat(q, np.searchsorted(by, np.arange(BANDS)), axis=1), np.searchsorted(bx, np.arange(COLS)), axis=2)
    assert hist.dtype.kind == "i" and total.dtype == np.int64 and total.shape == (n, BANDS, COLS)
    return {"hist": hist.astype(np.uint32), "sum": total.astype(np.uint64)}


def sig_bytes(sig, i=None):
    """the signatures (frame i alone, or all of them) as struct rvdd_frame_sig lays them out: uint32 hist[16][64], uint64 sum[16][16]"""
    frames = range(len(sig["hist"])) if i is None else [i]
    return b"".join(np.ascontiguousarray(sig["hist"][k], np.uint32).tobytes() + np.ascontiguousarray(sig["sum"][k], np.uint64).tobytes() for k in frames)


def cut_score_ref(a_hist, a_sum, b_hist, b_sum, hh, ww):
    """rvdd_cut_score on Python integers: -> (d_hist, d_grid); ValueError as RVDD_ERR_ARG"""
    ha = [int(v) for v in np.asarray(a_hist, np.uint64).sum(axis=0)]
    hb = [int(v) for v in np.asarray(b_hist, np.uint64).sum(axis=0)]
    cells = int(hh) * int(ww)
    if sum(ha) != cells or sum(hb) != cells:
        raise ValueError("signatures of another frame size: %d and %d cells, hh x ww = %d" % (sum(ha), sum(hb), cells))
    dh = sum(abs(x - y) for x, y in zip(ha, hb))
    sa = [int(v) for v in np.asarray(a_sum).reshape(-1)]
    sb = [int(v) for v in np.asarray(b_sum).reshape(-1)]
    dg = sum(abs(x - y) for x, y in zip(sa, sb))
    mg = sum(max(x, y) for x, y in zip(sa, sb))
    return float(dh) / float(2 * cells), float(dg) / (float(mg) if mg else 1.0)


def scores_ref(sig, hh, ww):
    """the N - 1 score pairs of consecutive frames of a signature dict"""
    return [cut_score_ref(sig["hist"][k - 1], sig["sum"][k - 1], sig["hist"][k], sig["sum"][k], hh, ww) for k in range(1, len(sig["hist"]))]


def find_cuts_ref(scores, t_hist=T_HIST, t_grid=T_GRID, min_len=MIN_LEN):
    """Frame k (1 .. N-1, scores[k - 1] its pair with frame k - 1) starts a shot iff d_hist > t_hist or d_grid > t_grid; a cut fewer than
    min_len frames behind the last accepted cut (or frame 0), or fewer than min_len frames before the end, is dropped."""
    n = len(scores) + 1
    cuts, last = [], 0
    for k in range(1, n):
        d_hist, d_grid = scores[k - 1]
        if (d_hist > t_hist or d_grid > t_grid) and k - last >= min_len and n - k >= min_len:
            cuts.append(k)
            last = k
    return cuts


# ---- scenes ---------------------------------------------------------------------------------------------------------------
PLANE_GAINS = (1.0, 0.6, 0.5, 1.0)
BLACK = 240.0


def scene_cells(seed, frames, hh, ww, iso, speed, bit_depth=12):
    """One shot as whole-DN frames [frames,hh,ww,4] f32.  Per seed: a mean level uniform in 12 .. 60 % of the range; a contrast of 0.3 .. 0.9
    times min(level - 0.07, 0.35); a pattern of four low-frequency sinusoids (0.25 .. 2 periods across the frame, weight 0.75) and four
    fine ones (0.02 .. 0.12 cycles per cell, weight 0.25), each of a random direction and phase; a translation of `speed` cells per
    frame in a random direction; per-plane gains (1, 0.6, 0.5, 1) about a black level of 240; the noise of the ISO's curve, rounded and
    clipped to the bit depth."""
    rng = np.random.default_rng(seed)
    top = 2 ** bit_depth - 1
    a, b = dpc_ref.iso_curve(iso, bit_depth)
    level = rng.uniform(0.12, 0.60)
    contrast = rng.uniform(0.3, 0.9) * min(level - 0.07, 0.35)
    psi = rng.uniform(0, 2 * np.pi, 8)
    phase = rng.uniform(0, 2 * np.pi, 8)
    periods = rng.uniform(0.25, 2.0, 4)
    fine = rng.uniform(0.02, 0.12, 4)
    fx = np.concatenate([periods * np.cos(psi[:4]) / ww, fine * np.cos(psi[4:])])
    fy = np.concatenate([periods * np.sin(psi[:4]) / hh, fine * np.sin(psi[4:])])
    weight = np.array([0.75 / 4] * 4 + [0.25 / 4] * 4)
    heading = rng.uniform(0, 2 * np.pi)
    y = np.arange(hh, dtype=np.float64)[:, None, None] + np.array([0.0, 0.0, 0.5, 0.5])[None, None, :]      # CFA position (k >> 1, k & 1)
    x = np.arange(ww, dtype=np.float64)[None, :, None] + np.array([0.0, 0.5, 0.0, 0.5])[None, None, :]
    out = np.empty((frames, hh, ww, 4), F)
    for t in range(frames):
        u, v = x + t * speed * np.cos(heading), y + t * speed * np.sin(heading)
        pattern = sum(w * np.sin(2 * np.pi * (p * u + r * v) + ph) for w, p, r, ph in zip(weight, fx, fy, phase))
        lin = (level + contrast * pattern) * top
        m = BLACK + np.asarray(PLANE_GAINS)[None, None, :] * (lin - BLACK)
        z = rng.standard_normal(m.shape)
        out[t] = np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0.0)) * z), 0, top)
    return out


def scene_gray(seed, frames, hh, ww, iso, speed, bit_depth=12):
    """the gray planes [frames,hh,ww] the ingest forms of `scene_cells`"""
    return dpc_ref.ingest(scene_cells(seed, frames, hh, ww, iso, speed, bit_depth), bit_depth)[1]
