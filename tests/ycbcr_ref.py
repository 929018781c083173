"""The rule of rvdd_ycbcr (include/rvdd.h) restated in NumPy: display values -> Y'CbCr 4:2:0, BT.709 limited range, integer after one
quantisation -- what the kernel must give bit for bit -- and the real-valued formula it approximates, in float64."""
import numpy as np

K = 65535 * 16384
LUMA = (3483, 11718, 1183)            # sums to 16384
CB = (-1877, -6315, 8192)             # each sums to 0
CR = (8192, -7441, -751)


def quantise(disp):
    """float32 [...] -> int64 0 .. 65535: clamp (a NaN and everything <= 0 give 0), ONE f32 product, rounded half to even"""
    d = np.asarray(disp, dtype=np.float32)
    d = np.where(d > 0, d, np.float32(0))
    d = np.where(d < 255, d, np.float32(255)).astype(np.float32)
    return np.rint(d * np.float32(257.0)).astype(np.int64)


def ycbcr(disp, depth):
    """disp float32 [n,H,W,3] (or [H,W,3]), depth 8 | 10 -> (Y [n,H,W], Cb [n,H/2,W/2], Cr [n,H/2,W/2]), uint8 | uint16"""
    assert depth in (8, 10)
    d = np.asarray(disp, dtype=np.float32)
    d = d[None] if d.ndim == 3 else d
    n, H, W, c = d.shape
    assert c == 3 and H % 2 == 0 and W % 2 == 0
    m = 1 << (depth - 8)
    q = quantise(d)
    L = LUMA[0] * q[..., 0] + LUMA[1] * q[..., 1] + LUMA[2] * q[..., 2]
    Y = 16 * m + (L * (219 * m) + K // 2) // K
    s = q.reshape(n, H // 2, 2, W // 2, 2, 3).sum(axis=(2, 4))
    cb = CB[0] * s[..., 0] + CB[1] * s[..., 1] + CB[2] * s[..., 2]
    cr = CR[0] * s[..., 0] + CR[1] * s[..., 1] + CR[2] * s[..., 2]
    Cb = 128 * m + (cb * (224 * m) + 2 * K) // (4 * K)          # numpy's // on int64 is floor division
    Cr = 128 * m + (cr * (224 * m) + 2 * K) // (4 * K)
    t = np.uint8 if depth == 8 else np.uint16
    return Y.astype(t), Cb.astype(t), Cr.astype(t)


def frame_bytes(disp, depth):
    """-> [n, H*W*3/2] samples, uint8 | uint16: per image Y, Cb, Cr as one Y4M frame body (what rvdd_ycbcr writes)"""
    Y, Cb, Cr = ycbcr(disp, depth)
    n = Y.shape[0]
    return np.concatenate([Y.reshape(n, -1), Cb.reshape(n, -1), Cr.reshape(n, -1)], axis=1)


def real(disp, depth):
    """the real-valued BT.709 limited-range formula in float64, before any rounding: (Y, Cb, Cr) as for `ycbcr`; chroma of the quad's mean"""
    d = np.asarray(disp, dtype=np.float32)
    d = d[None] if d.ndim == 3 else d
    n, H, W, _ = d.shape
    m = float(1 << (depth - 8))
    v = np.where(d > 0, d, np.float32(0))
    v = np.where(v < 255, v, np.float32(255)).astype(np.float64) / 255.0
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    y = kr * v[..., 0] + kg * v[..., 1] + kb * v[..., 2]
    a = v.reshape(n, H // 2, 2, W // 2, 2, 3).mean(axis=(2, 4))
    ya = kr * a[..., 0] + kg * a[..., 1] + kb * a[..., 2]
    pb = (a[..., 2] - ya) / (2.0 * (1.0 - kb))
    pr = (a[..., 0] - ya) / (2.0 * (1.0 - kr))
    return m * (16.0 + 219.0 * y), m * (128.0 + 224.0 * pb), m * (128.0 + 224.0 * pr)
