"""CPU restatement of rvdd_unprocess and of its draws (helper of tests/test_unprocess_host.py and tests/test_gpu_unprocess.py;
not a test module).

Written from the arithmetic include/rvdd.h documents: the chain one operation at a time in a chosen float type (float32 = what
the kernel rounds to, float64 = the yardstick), Philox4x32-10 from its constants, and the two streams of draws."""
import numpy as np

from bayer_ref import PATTERNS, PHASE, RGB_OF_SITE

RGB2CAM = ((0.95640505, 0.17353177, -0.13219438), (0.14135948, 0.80402001, 0.07771696), (0.05432832, 0.29852577, 0.67210576))
AFFINE = {3200: (3344, 266), 12800: (3807, 268)}
NOISE = {3200: (8.0034, 2043.51144), 12800: (28.3015, 6307.62081)}

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [((p1 >> _S32) ^ c[1] ^ k0) & _MASK, p1 & _MASK, ((p0 >> _S32) ^ c[3] ^ k1) & _MASK, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def _words(seed, frame, stream, count):
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    e = np.arange(count, dtype=np.uint64)
    return philox4x32_10([e, np.full(count, stream, np.uint64), np.full(count, frame & 0xFFFFFFFF, np.uint64),
                          np.full(count, frame >> 32, np.uint64)], (seed & 0xFFFFFFFF, seed >> 32))


def dither_plane(seed, frame, H, W):
    """[H,W,3] float32, exact: stream 0, element = pixel."""
    w = _words(seed, frame, 0, H * W)
    d = np.stack([(w[c] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5) for c in range(3)], -1)
    return d.reshape(H, W, 3)


def normal_plane(seed, frame, H, W):
    """[H/2,W/2,4] float64 Box-Muller of the stream-1 words, element = cell."""
    w = _words(seed, frame, 1, (H // 2) * (W // 2))
    z = []
    for a, b in ((w[0], w[1]), (w[2], w[3])):
        u = ((a >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        v = (b >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        z += [r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)]
    return np.stack(z, -1).reshape(H // 2, W // 2, 4)


def gains_f32(rgb_gain, red_gain, blue_gain):
    """The three inverted gains as rvdd_unprocess forms them: float32 quotients of the gains rounded to float32."""
    one, rgb = np.float32(1), np.float32(rgb_gain)
    return np.array([(one / np.float32(red_gain)) / rgb, one / rgb, (one / np.float32(blue_gain)) / rgb], np.float32)


def mosaic(lin, pattern="gbrg"):
    """[..,H,W,3] -> [..,H/2,W/2,4]: CFA position k = (k >> 1, k & 1) keeps the colour `pattern` has there."""
    py, px = PHASE[pattern]
    return np.stack([lin[..., k >> 1::2, k & 1::2, RGB_OF_SITE[(((k >> 1) ^ py) << 1) | ((k & 1) ^ px)]] for k in range(4)], -1)


def chain(srgb, dither, normal, rgb_gain, red_gain, blue_gain, iso, pattern="gbrg", T=np.float32):
    """srgb uint8 [..,H,W,3], dither [..,H,W,3], normal [..,H/2,W/2,4] -> dict(lin_f32, lin_u16, gt_raw, noisy) in type T."""
    assert pattern in PATTERNS
    f = T
    x = srgb.astype(np.float32) + dither.astype(np.float32)                  # the reference's float32 sum
    x = (x.astype(T) / f(266)).astype(T)
    x = np.clip(x, f(0), f(1))
    x = (f(0.5) - np.sin((np.arcsin(f(1) - f(2) * x) / f(3)).astype(T))).astype(T)
    p = np.power(np.maximum(x, f(np.float32(1e-8))), f(np.float32(2.2))).astype(T)
    M = np.array(RGB2CAM, np.float32).astype(T)
    cam = np.stack([(p[..., 0] * M[k, 0] + p[..., 1] * M[k, 1]) + p[..., 2] * M[k, 2] for k in range(3)], -1).astype(T)
    y = np.clip((cam * gains_f32(rgb_gain, red_gain, blue_gain).astype(T)).astype(T), f(0), f(1))
    lin = (y * f(3855) + f(240)).astype(T)
    A, B = AFFINE[iso]
    lin = ((f(A) * (lin - f(245))).astype(T) / f(2060) + f(B)).astype(T)
    m = mosaic(lin, pattern)
    ka, kb = NOISE[iso]
    ka, kb = f(np.float32(ka)), f(np.float32(kb))
    noisy = (m + np.sqrt(np.maximum(ka * m - kb, f(0))).astype(T) * normal.astype(T)).astype(T)
    return {"lin_f32": lin, "lin_u16": np.clip(np.rint(lin), 0, 4095).astype(np.uint16), "gt_raw": m, "noisy": noisy}


def unprocess(srgb, rgb_gain, red_gain, blue_gain, iso, seed, frame0, pattern="gbrg", T=np.float32):
    """The whole call with its own draws: srgb uint8 [n,H,W,3]; image i uses frame frame0 + i."""
    n, H, W, _ = srgb.shape
    d = np.stack([dither_plane(seed, frame0 + i, H, W) for i in range(n)])
    z = np.stack([normal_plane(seed, frame0 + i, H, W) for i in range(n)]).astype(np.float32)
    return chain(srgb, d, z, rgb_gain, red_gain, blue_gain, iso, pattern, T)


# ---- the bounds the tests share -------------------------------------------------------------------------------------------
def assert_close_dn(got, want, what):
    """|diff| <= 4e-6 * max(|value|, 255): the project's bound for a chain of this kind across math libraries
    (tests/test_ppipe.py); one DN is 2.4e-4 relative at 4095."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    excess = np.abs(got - want) - 4e-6 * np.maximum(np.abs(want), 255.0)
    print(f"{what}: max |diff| = {np.abs(got - want).max():.3e}, worst excess over the bound = {excess.max():.3e}")
    assert excess.max() <= 0, f"{what}: {np.abs(got - want).max()} DN"


def assert_integers_agree(got, want, what):
    """Rounded outputs (tests/test_ppipe.py): unequal samples differ by exactly 1, at most 0.1 % of them are unequal."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    d = np.abs(got - want)
    print(f"{what}: {int((d > 0).sum())} of {d.size} unequal, max {int(d.max())}")
    assert d.max() <= 1, f"{what}: off by {int(d.max())}"
    assert (d > 0).mean() <= 1e-3, f"{what}: {(d > 0).mean():.2e} of the samples unequal"
