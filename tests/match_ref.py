"""NumPy restatement of the noise-curve matching (include/rvdd.h: rvdd_match_coeffs, rvdd_match_raw, rvdd_unmatch_rgb) and the
cameras the tests share.  The two maps are f32, one operation at a time; the coefficients are Python doubles in the header's order."""
import numpy as np

F = np.float32
ISO_CURVES = {3200: (8.0034, 2043.51144), 12800: (28.3015, 6307.62081)}      # var = a m - b in 12-bit DN
# The cameras of DESIGN.md 4.16: (bit depth, a, black level).  var(m) = a (m - black) + 100 in DN of that bit depth -- a read-noise
# variance of 100 DN^2 at the black level -- so b = a * black - 100.
CAMERAS = [(12, 3.0, 256), (12, 15.0, 256), (12, 60.0, 256), (12, 120.0, 256), (10, 4.0, 64), (14, 60.0, 1024)]


def camera_curve(a, black):
    return float(a), float(a) * black - 100.0


def coeffs(a, b, bit_depth, a_ref, b_ref):
    """-> (scale f32, offset f32, s, t): the header's formulas, each operation as written"""
    k = 4095.0 / float(2 ** bit_depth - 1)
    a12 = k * a
    b12 = (k * k) * b
    s = a_ref / a12
    t = (b_ref - (s * s) * b12) / a_ref
    return F(s), F((s - 1.0) + (2.0 * t) / 4095.0), s, t


def match_raw_ref(v, scale, offset):
    v = np.asarray(v, F)
    out = (F(scale) * v) + F(offset)
    assert out.dtype == F
    return out


def unmatch_rgb_ref(v, scale, offset):
    v = np.asarray(v, F)
    r = F(1.0 / float(F(scale)))                          # formed once, in double, rounded to f32
    out = (v - F(offset)) * r
    assert out.dtype == F
    return out


def packed_of_dn(dn, bit_depth):
    """rvdd_ingest_raw's sample of a digital number: 2 * (dn / top) - 1, the division correctly rounded"""
    top = F(2 ** bit_depth - 1)
    return F(2.0) * (np.asarray(dn, F) / top) - F(1.0)


def dn_of(v, bit_depth):
    """rvdd_egress's digital number before rounding: ((v + 1) * 0.5) * top"""
    return ((np.asarray(v, F) + F(1.0)) * F(0.5)) * F(2 ** bit_depth - 1)


def camera_frames(gt, a, b, noise_seed=5):
    """The recipe of DESIGN.md 4.16 at 12 bits: synth's `gt` [T,3,H,W] in [-1,1] taken as the scene in the camera's own range, its GBRG
    mosaic in DN, the camera's noise sqrt(max(a dn - b, 0)) z with z from torch.Generator().manual_seed(noise_seed).randn, rounded
    and clipped to 0 .. 4095.  -> packed camera frames [T,4,H/2,W/2] float32 in [-1,1] (torch, CPU)"""
    import torch
    dn = (gt.double() + 1.0) * 0.5 * 4095.0
    u = torch.stack([dn[:, (1, 2, 0, 1)[k], (k >> 1)::2, (k & 1)::2] for k in range(4)], 1)      # G B / R G
    z = torch.randn(u.shape, generator=torch.Generator().manual_seed(noise_seed)).double()
    noisy = torch.round(u + torch.sqrt(torch.clamp(a * u - b, min=0.0)) * z).clamp(0, 4095)
    return (2.0 * (noisy / 4095.0) - 1.0).float().contiguous()


def psnr(x, y):
    """10 log10(4 / mse) of two tensors in [-1,1], in double"""
    import math
    return 10.0 * math.log10(4.0 / float(((x.double() - y.double()) ** 2).mean()))
