"""numpy restatement of rvdd_egress (include/rvdd.h), one f32 operation at a time: the inverse direction of stream_ref.ingest_ref.
Helper of tests/test_egress_host.py and tests/test_gpu_egress.py; not a test module."""
import numpy as np

PATTERNS = ("gbrg", "grbg", "rggb", "bggr")          # enum rvdd_bayer, in order
LAYOUTS = ("rgb_hwc", "mosaic", "packed_hwc")        # enum rvdd_out_layout, in order
GBRG = (1, 2, 0, 1)                                  # the RGB plane of each GBRG site: G B / R G
PHASE = (0, 3, 2, 1)                                 # (py << 1) | px of each pattern: CFA position k is the GBRG site k ^ phase


def col(pattern, k):
    """The RGB plane `pattern` has at CFA position k = (k >> 1, k & 1) of a 2x2 cell."""
    return GBRG[k ^ PHASE[PATTERNS.index(pattern)]]


def dn_of(v, bit_depth):
    """((v + 1) * 0.5) * (2^bit_depth - 1), each operation rounded to f32."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    dn = ((v + np.float32(1.0)) * np.float32(0.5)) * np.float32(2 ** bit_depth - 1)
    assert dn.dtype == np.float32
    return dn


def to_u16(dn, bit_depth):
    """min(max(rint(dn), 0), top) as uint16: rint rounds half to even; NaN -> 0, -inf -> 0, +inf -> top."""
    top = np.float32(2 ** bit_depth - 1)
    with np.errstate(invalid="ignore"):
        r = np.rint(dn)
        r = np.where(r > 0, r, np.float32(0.0))       # false for NaN
        r = np.where(r < top, r, top)
    return r.astype(np.uint16)


def egress_ref(rgb, layout, dtype, bit_depth, pattern="gbrg"):
    """rgb [n,3,H,W] float32 -> [n,H,W,3] / [n,H,W] / [n,H/2,W/2,4] of np.uint16 or np.float32."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.float32 and rgb.ndim == 4 and rgb.shape[1] == 3
    with np.errstate(invalid="ignore", over="ignore"):
        dn = dn_of(rgb, bit_depth)
    n, _, H, W = rgb.shape
    if layout == "rgb_hwc":
        out = dn.transpose(0, 2, 3, 1)
    else:
        assert H % 2 == 0 and W % 2 == 0
        cells = np.stack([dn[:, col(pattern, k), (k >> 1)::2, (k & 1)::2] for k in range(4)], axis=-1)
        if layout == "packed_hwc":
            out = cells
        else:
            out = np.empty((n, H, W), np.float32)
            for k in range(4):
                out[:, (k >> 1)::2, (k & 1)::2] = cells[..., k]
    out = np.ascontiguousarray(out)
    return out if np.dtype(dtype) == np.float32 else to_u16(out, bit_depth)


def special_values(bit_depth=8):
    """The inputs whose rounding is decided by the rule and not by the arithmetic: the ends and the centre of the range (v = 0 is
    the tie 2^(b-1) - 0.5 at every depth), NaN and the infinities, values past both ends, and for 8 bits every tie
    v = 2 (k + 0.5) / 255 - 1 formed in f32 with its four f32 neighbours."""
    f = np.float32
    v = [f(-1.0), f(1.0), f(0.0), f(-0.0), f(np.nan), f(np.inf), f(-np.inf), f(-1.25), f(1.25), f(-3.0), f(3.0)]
    ties = f(2.0) * (np.arange(255, dtype=np.float32) + f(0.5)) / f(255.0) - f(1.0)
    assert ties.dtype == np.float32
    out = [np.array(v, np.float32), ties]
    for away in (f(-np.inf), f(np.inf)):
        one = np.nextafter(ties, away)
        out += [one, np.nextafter(one, away)]
    return np.concatenate(out).astype(np.float32)


def fill(n, H, W, seed):
    """[n,3,H,W] float32: uniform in [-1.25, 1.25], with the special values -- in the order special_values gives them, as many as
    there are pixels -- at scattered pixels, in all three planes of a pixel (a mosaic layout reads one of them)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.25, 1.25, (n, 3, H, W)).astype(np.float32)
    sp = special_values()
    m = min(sp.size, n * H * W)
    i, p = np.divmod(rng.permutation(n * H * W)[:m], H * W)
    x.reshape(n, 3, H * W)[i, :, p] = sp[:m, None]
    return x
