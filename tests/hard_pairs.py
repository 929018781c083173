"""Image pairs that are hard on TV-L1, and what the tests of it share (test_tvl1_hard_host.py, test_gpu_tvl1_hard.py).  A plain
module: no fixtures, no pytest settings; pytest does not rewrite its asserts, so each one carries its message.

pair(name, h, w, seed) -> (I0, I1) float32, NumPy only, from the seed.  What a camera gives the flow beside smooth motion:

    identical          a frame paired with itself (frame 0 under all_frames, a static shot): every inner loop stops at n == 1
    constant           two frames of one level: no normalisation (max == min), no gradient anywhere
    two_levels         two constant frames of different levels: rho = 255 on zero gradient
    shift12            a texture moved 12 px: the coarse scales find it, 12 columns of the warp leave the frame (g == 0 there)
    plateaus           8x8 blocks of four levels moved (2, 1): gradient on the block edges only
    sensor_clip_noise  whole 12-bit DN over a black level, shot and read noise, highlights clipped at 4095 (a flat region), moved (2, 1)
    hot_pixel          one pixel of 1000 in a +-2 image: the joint normalisation squeezes the scene
    hot_pixel_max      the same with a pixel of 65535: the scene becomes a fraction of a grey level, the flow almost zero
    blob               a Gaussian blob on an almost flat ground, moved (4, 3)
    ramp               a linear ramp against itself plus an offset: brightness change without motion
    checker            a 4 px checkerboard moved 2 px: the motion is ambiguous by construction
    gain               gain 1.5 and offset 0.8 between the frames, 1 px of motion
    white_noise        white noise against other white noise
    cut                the two sides of a hard cut: unrelated textures
    half_cut           the left half cut, the right half moved (1, 2)
    cap                a 22x22-style crop of a texture against the crop at (-9, +4): at one scale the first inner loop runs into
                       the 300-iteration cap

A case is PINNED if the oracle's own flow moves by at most PIN_MAX / PIN_MEAN px (a quarter of CLOSE_MAX / CLOSE_MEAN, the bar
tests/test_tvl1.py holds the kernels to) when both inputs move by one ulp per pixel, and its iteration counts do not move at all;
anything else is CHAOTIC: there the reference itself turns one ulp into pixels (a cut at two or more scales: 10 px), and only bit
identity between this project's own kernels means anything.  The class in CASES is a condition, not a measurement:
test_tvl1_hard_host.py recomputes it.

Seeds of the `cap` cases were searched on the CPU with search_cap: 22x22 pairs (one scale) whose per-loop counts contain 300 and
which are pinned; seeds 3, 19, 54, 72 and 79 of the first 80 qualify, 3 (one loop at the cap) and 72 (two in a row) are kept.
One scale needs a diagonal below 32 px, so a size with nx > 64 has three: there the coarse scales take the motion and no
inner loop of `cap` reaches 300 (60 seeds each at 41x75 and 33x70).  `cut` and `half_cut` do reach it there, always as chaotic
pairs (40 seeds each at 41x75, 33x70 and 30x90), so none is pinned at such a size: cap_wide_30x90 (half_cut, seed 7: the finest
scale's first loop stops at 300, 90 columns = two patches across, equal totals under the perturbations, 7.5e-3 px of spread)
is kept for the equivalence tests only.

What the 1-ulp experiment gave for the classes (max / mean px of spread): the zero cases 0, hot pixels 1e-5, ramp, checker, blob,
white noise at 22x22 and the cap pairs 1e-5 .. 8e-5, shift12 1.2e-4; plateaus 1e-3 .. 0.26, the clipped sensor frames at three
scales 7e-4, gain at 48x64 0.18, cuts 0.1 .. 10 px with totals that move."""
import functools

import numpy as np

import tvl1_oracle as T

F = np.float32
CLOSE_MAX, CLOSE_MEAN = 2e-3, 1e-4                   # tests/test_tvl1.py:_close, restated
PIN_MAX, PIN_MEAN = CLOSE_MAX / 4, CLOSE_MEAN / 4
PAD = 16                                             # margin of the canvas that the moved crops come from

NAMES = ("identical", "constant", "two_levels", "shift12", "plateaus", "sensor_clip_noise", "hot_pixel", "hot_pixel_max", "blob", "ramp",
         "checker", "gain", "white_noise", "cut", "half_cut", "cap")


# ---- the generators ----------------------------------------------------------------------------------------------------------------
def _blur(a):
    """3x3 binomial, edge samples repeated"""
    p = np.pad(a, 1, mode="edge")
    a = (p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]) / 4
    return (a[:-2] + 2 * a[1:-1] + a[2:]) / 4


def canvas(h, w, seed):
    """a texture [h + 2 PAD, w + 2 PAD] in about +-3: six long sinusoids of random direction and a little noise, blurred six times"""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * PAD, w + 2 * PAD
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    t = np.zeros((H, W))
    for _ in range(6):
        fx, fy = rng.uniform(-0.15, 0.15, 2)
        t += rng.uniform(0.3, 1.0) * np.sin(fx * xx + fy * yy + rng.uniform(0, 2 * np.pi))
    n = rng.standard_normal((H, W))
    for _ in range(6):
        n = _blur(n)
    return t + 0.5 * n


def crop(c, h, w, dy=0, dx=0):
    return np.ascontiguousarray(c[PAD + dy:PAD + dy + h, PAD + dx:PAD + dx + w])


def pair(name, h, w, seed):
    rng = np.random.default_rng(seed + 1000)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c = canvas(h, w, seed)
    if name == "identical":
        I0 = I1 = crop(c, h, w)
    elif name == "constant":
        I0 = I1 = np.full((h, w), 0.37)
    elif name == "two_levels":
        I0, I1 = np.full((h, w), 0.25), np.full((h, w), 0.75)
    elif name == "shift12":
        I0, I1 = crop(c, h, w), crop(c, h, w, 0, 12)
    elif name == "plateaus":
        H, W = h + 2 * PAD, w + 2 * PAD
        levels = rng.integers(0, 4, ((H + 7) // 8, (W + 7) // 8)).astype(np.float64)
        big = np.kron(levels, np.ones((8, 8)))[:H, :W]
        I0, I1 = crop(big, h, w), crop(big, h, w, 1, 2)
    elif name == "sensor_clip_noise":
        # a scene whose brightest third is beyond the sensor's range: 240 DN of black level, shot + read noise, whole DN
        def shot(s, r):
            dn = 240.0 + np.clip(2800.0 + 1500.0 * s, 0.0, None)
            dn = dn + np.sqrt(0.4 * dn) * r.standard_normal(s.shape) + 2.0 * r.standard_normal(s.shape)
            return np.clip(np.rint(dn), 0, 4095)
        I0, I1 = shot(crop(c, h, w), rng), shot(crop(c, h, w, 1, 2), rng)
    elif name in ("hot_pixel", "hot_pixel_max"):
        hot = 65535.0 if name == "hot_pixel_max" else 1000.0
        s = np.clip(c / 1.5, -2, 2)
        I0, I1 = crop(s, h, w), crop(s, h, w, 1, 0)
        I0[h // 3, w // 2] = hot
        I1[h // 3, w // 2] = hot                      # a defect of the sensor: it does not move with the scene
    elif name == "blob":
        g = lambda cy, cx: np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (min(h, w) / 6.0) ** 2))
        I0 = g(h / 2, w / 2) + 0.002 * crop(c, h, w)
        I1 = g(h / 2 - 3, w / 2 - 4) + 0.002 * crop(c, h, w, 3, 4)
    elif name == "ramp":
        I0 = 0.01 * xx + 0.004 * yy
        I1 = I0 + 0.05
    elif name == "checker":
        ch = lambda x, y: (((x // 4) + (y // 4)) % 2).astype(np.float64)
        I0, I1 = ch(xx, yy), ch(xx + 2, yy)
    elif name == "gain":
        I0, I1 = crop(c, h, w), 1.5 * crop(c, h, w, 0, 1) + 0.8
    elif name == "white_noise":
        I0, I1 = rng.standard_normal((h, w)), rng.standard_normal((h, w))
    elif name == "cut":
        I0, I1 = crop(c, h, w), crop(canvas(h, w, seed + 500), h, w)
    elif name == "half_cut":
        I0, I1 = crop(c, h, w), crop(c, h, w, 2, 1)
        I1[:, :w // 2] = crop(canvas(h, w, seed + 500), h, w)[:, :w // 2]
    elif name == "cap":
        I0, I1 = crop(c, h, w), crop(c, h, w, 4, -9)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(I0, F), np.ascontiguousarray(I1, F)


# ---- the cases: name -> (generator, h, w, seed, class).  Pinned sizes: 22x22 (one scale, six patches of 64x4 exchanging rows),
# 48x64 (three scales), 41x75 (two patches across, ragged both ways); chaotic ones at 48x64 and 41x75 ---------------------------------
PINNED, CHAOTIC = "pinned", "chaotic"
CASES = {}


def _case(gen, h, w, seed, cls, key=None):
    CASES[key or f"{gen}_{h}x{w}"] = (gen, h, w, seed, cls)


def case_pair(key):
    gen, h, w, seed, _ = CASES[key]
    return pair(gen, h, w, seed)


def num_scales(key):
    _, h, w, _, _ = CASES[key]
    return T.num_scales(w, h)


for _gen, _h, _w, _seed in (("identical", 48, 64, 1), ("identical", 41, 75, 1), ("constant", 41, 75, 1), ("two_levels", 22, 22, 1),
                            ("shift12", 48, 64, 2), ("shift12", 41, 75, 1), ("sensor_clip_noise", 22, 22, 2), ("hot_pixel", 41, 75, 1),
                            ("hot_pixel_max", 48, 64, 1), ("blob", 22, 22, 2), ("blob", 41, 75, 1), ("ramp", 48, 64, 1),
                            ("checker", 48, 64, 1), ("checker", 41, 75, 1), ("gain", 22, 22, 1), ("gain", 41, 75, 1),
                            ("white_noise", 22, 22, 1), ("white_noise", 48, 64, 1)):
    _case(_gen, _h, _w, _seed, PINNED)
_case("cap", 22, 22, 3, PINNED, "cap_a_22x22")
_case("cap", 22, 22, 72, PINNED, "cap_b_22x22")
for _gen, _h, _w, _seed in (("cut", 48, 64, 2), ("cut", 41, 75, 1), ("half_cut", 48, 64, 1), ("plateaus", 48, 64, 1),
                            ("sensor_clip_noise", 48, 64, 1), ("gain", 48, 64, 1), ("white_noise", 41, 75, 1)):
    _case(_gen, _h, _w, _seed, CHAOTIC)
_case("half_cut", 30, 90, 7, CHAOTIC, "cap_wide_30x90")

CAP_CASES = ("cap_a_22x22", "cap_b_22x22")                                  # pinned, an inner loop stops at 300
ZERO_CASES = ("identical_48x64", "constant_41x75", "two_levels_22x22")      # flow exactly 0, every inner loop stops at n == 1


# ---- one-ulp perturbation and the oracle's spread under it -------------------------------------------------------------------------
def ulp_perturbed(I, seed):
    """each pixel moved to the next float32 towards +inf or -inf, with probability 1/2 each"""
    up = np.random.default_rng(seed).random(I.shape) < 0.5
    return np.where(up, np.nextafter(I, F(np.inf)), np.nextafter(I, F(-np.inf))).astype(F)


def oracle(I0, I1):
    """-> (flow [2,h,w], per-loop iteration counts: 5 per scale, coarsest scale first)"""
    stats = []
    with np.errstate(over="ignore"):                 # -rho / g on g of 1e-40: the quotient that the g < GRAD_IS_ZERO branch drops
        return T.tvl1flow(I0, I1, stats), stats


def spread(I0, I1, draws=3, until_chaotic=False):
    """-> (max_abs, mean_abs, totals): the oracle on inputs perturbed by one ulp (both images of a draw with the same signs, so
    that a pair of identical frames stays one) against the oracle on the inputs; totals: the iteration totals of all runs.
    until_chaotic: no further draw once the figures so far miss the pinned condition."""
    base, st = oracle(I0, I1)
    worst_max = worst_mean = 0.0
    totals = [sum(st)]
    for d in range(draws):
        u, st = oracle(ulp_perturbed(I0, 100 + d), ulp_perturbed(I1, 100 + d))
        diff = np.abs(u - base)
        worst_max, worst_mean = max(worst_max, float(diff.max())), max(worst_mean, float(diff.mean()))
        totals.append(sum(st))
        if until_chaotic and not is_pinned(worst_max, worst_mean, totals):
            break
    return worst_max, worst_mean, totals


def is_pinned(max_abs, mean_abs, totals):
    return max_abs <= PIN_MAX and mean_abs <= PIN_MEAN and len(set(totals)) == 1


@functools.lru_cache(maxsize=None)
def case_oracle(key):
    """the oracle's flow (read-only) and per-loop counts of a case, computed once per process"""
    u, st = oracle(*case_pair(key))
    u.setflags(write=False)
    return u, tuple(st)


def flat_fraction(I0, I1, flow):
    """share of the finest scale's pixels whose warped gradient is below GRAD_IS_ZERO under `flow` (the oracle's final flow: the
    last warp's differs from it by that loop's update).  Counted inside the band of one pixel on the left and top and two on the
    right and bottom, where the bicubic stencil leaves the frame (and the warp gives zero) even under a flow of zero: that band
    is flat in every pair, the smooth ones of tests/test_tvl1.py included."""
    mn, mx = min(I0.min(), I1.min()), max(I0.max(), I1.max())
    if mx > mn:
        I1 = (255.0 * (I1.astype(np.float64) - float(mn)) / float(F(mx - mn))).astype(F)
    I1 = T.gaussian(I1, T.PRESMOOTHING_SIGMA)
    I1x, I1y = T.centered_gradient(I1)
    wx, wy = T.warp(I1x, flow[0], flow[1], True), T.warp(I1y, flow[0], flow[1], True)
    flat = (wx * wx + wy * wy).astype(F) < F(T.GRAD_IS_ZERO)
    return float(flat[1:-2, 1:-2].mean())


def close(a, b, what):
    """tests/test_tvl1.py:_close with a message; -> (max, mean)"""
    d = np.abs(np.asarray(a, np.float64) - b)
    assert d.max() < CLOSE_MAX and d.mean() < CLOSE_MEAN, (what, float(d.max()), float(d.mean()))
    return float(d.max()), float(d.mean())


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def load_hard(golden_dir):
    """tests/golden/tvl1_hard.npz (tools/make_golden_tvl1.py) -> {case: the reference library's flow}; the inputs are regenerated
    here and checked against every 7th pixel that the fixture holds of them."""
    import os
    g = np.load(os.path.join(golden_dir, "tvl1_hard.npz"))
    out = {}
    for key in pinned_cases():
        I0, I1 = case_pair(key)
        for got, tag in ((I0, "I0_check"), (I1, "I1_check")):
            want = g[f"{key}/{tag}"]
            assert np.abs(got[::7, ::7] - want).max() <= 1e-6 * max(1.0, float(np.abs(want).max())), f"{key}: regenerated images differ"
        out[key] = g[f"{key}/flow"]
    return out


def search_cap(h, w, seeds, gen="cap"):
    """-> [(seed, pinned?, per-loop counts)] of the seeds whose pair has an inner loop that runs into the cap"""
    found = []
    for seed in seeds:
        I0, I1 = pair(gen, h, w, seed)
        counts = oracle(I0, I1)[1]
        if T.MAX_ITERATIONS in counts:
            found.append((seed, is_pinned(*spread(I0, I1)), counts))
    return found


def pinned_cases():
    return [k for k, v in CASES.items() if v[4] == PINNED]


def chaotic_cases():
    return [k for k, v in CASES.items() if v[4] == CHAOTIC]
