"""CPU restatement of the Hamilton-Adams demosaic for any of the four Bayer patterns (helper of tests/test_bayer_host.py and
tests/test_gpu_bayer.py; not a test module).

Written from the algorithm (util/Hamilton_Adam_demo.py:123-172), per colour site: the packing is the same for every
pattern -- channel k of a [B,4,h,w] frame is CFA position (k >> 1, k & 1) -- and the colour site of full-resolution pixel
(y, x) under a pattern is the GBRG site of (y ^ py, x ^ px).  Sites are numbered as GBRG's: 0 = Gb (a green with blue
horizontal neighbours), 1 = B, 2 = R, 3 = Gr.  Replicate padding clamps the coordinate first and then takes the site of
the clamped pixel.  Every stencil weight is a power of two, so only the order of the additions matters; each one is
written in the order of the reference's convolutions (row-major over the window), which makes the sign() ties come
out the same."""
import torch
import torch.nn.functional as F

PATTERNS = ("gbrg", "grbg", "rggb", "bggr")           # enum rvdd_bayer order
PHASE = {"gbrg": (0, 0), "grbg": (1, 1), "rggb": (1, 0), "bggr": (0, 1)}
RGB_OF_SITE = (1, 2, 0, 1)                             # G, B, R, G


def colour_sites(H: int, W: int, pattern: str) -> torch.Tensor:
    """[H,W] GBRG site number of every pixel's colour under `pattern`."""
    py, px = PHASE[pattern]
    yy = torch.arange(H)[:, None]
    xx = torch.arange(W)[None, :]
    return (((yy & 1) ^ py) << 1) | ((xx & 1) ^ px)


def pack_in_one(x: torch.Tensor) -> torch.Tensor:
    """[B,4,h,w] packed planes -> [B,2h,2w] CFA image (the same for every pattern)."""
    B, _, h, w = x.shape
    y = torch.empty(B, 2 * h, 2 * w, dtype=x.dtype)
    for k in range(4):
        y[:, k >> 1::2, k & 1::2] = x[:, k]
    return y


def pack(cfa: torch.Tensor) -> torch.Tensor:
    """[B,H,W] CFA image (H, W even) -> [B,4,H/2,W/2]: the inverse of pack_in_one."""
    return torch.stack([cfa[:, k >> 1::2, k & 1::2] for k in range(4)], 1).contiguous()


def remosaick(x: torch.Tensor, pattern: str) -> torch.Tensor:
    """[B,3,H,W] RGB -> [B,4,H/2,W/2] packed planes of `pattern`: each CFA position keeps the colour it has there."""
    py, px = PHASE[pattern]
    return torch.stack([x[:, RGB_OF_SITE[(((k >> 1) ^ py) << 1) | ((k & 1) ^ px)], k >> 1::2, k & 1::2] for k in range(4)],
                       1).contiguous()


def _window(p: torch.Tensor, r: int):
    """Shifted views of a [B,H,W] plane, replicate padded by r: at(dy, dx)[b, y, x] = p[b, clamp(y + dy), clamp(x + dx)]."""
    H, W = p.shape[-2:]
    q = F.pad(p[:, None], (r, r, r, r), mode="replicate")[:, 0]
    return lambda dy, dx: q[:, r + dy:r + dy + H, r + dx:r + dx + W]


def _green(cfa: torch.Tensor, site: torch.Tensor) -> torch.Tensor:
    """algo1: the measured sample at green sites, the direction-selected estimate elsewhere."""
    at = _window(cfa, 2)
    c = at(0, 0)
    l1, r1, l2, r2 = at(0, -1), at(0, 1), at(0, -2), at(0, 2)
    u1, d1, u2, d2 = at(-1, 0), at(1, 0), at(-2, 0), at(2, 0)
    Kh = 0.5 * l1 + 0.5 * r1
    Kv = 0.5 * u1 + 0.5 * d1
    Dh = (l2 + (-2.0) * c) + r2
    Dv = (u2 + (-2.0) * c) + d2
    Fh = l1 + (-1.0) * r1
    Fv = u1 + (-1.0) * d1
    est_h = Kh - Dh / 4
    est_v = Kv - Dv / 4
    s = torch.sign((Fh.abs() + Dh.abs()) - (Fv.abs() + Dv.abs()))
    est = (1 + s) * est_v / 2 + (1 - s) * est_h / 2
    return torch.where((site == 0) | (site == 3), c, est)


def _chroma(cfa: torch.Tensor, green: torch.Tensor, site: torch.Tensor, own: int) -> torch.Tensor:
    """algo2 for the colour whose samples sit at site `own` (2 = red, 1 = blue)."""
    gsite, osite = (3, 0) if own == 2 else (0, 3)        # greens on the colour's rows / on its columns
    P = _window(torch.where(site == own, cfa, torch.zeros_like(cfa)), 1)
    G = _window(green, 1)
    g0 = G(0, 0)
    along_row = (0.5 * P(0, -1) + 0.5 * P(0, 1)) - ((0.25 * G(0, -1) + (-0.5) * g0) + 0.25 * G(0, 1))
    along_col = (0.5 * P(-1, 0) + 0.5 * P(1, 0)) - ((0.25 * G(-1, 0) + (-0.5) * g0) + 0.25 * G(1, 0))
    a, d, b, c = P(-1, -1), P(1, 1), P(-1, 1), P(1, -1)
    lap_p = (G(-1, -1) + (-2.0) * g0) + G(1, 1)
    lap_n = (G(-1, 1) + (-2.0) * g0) + G(1, -1)
    est_p = (0.5 * a + 0.5 * d) - lap_p / 4
    est_n = (0.5 * b + 0.5 * c) - lap_n / 4
    s = torch.sign((((-1.0) * a + d).abs() + lap_p.abs()) - (((-1.0) * b + c).abs() + lap_n.abs()))
    diag = (1 + s) * est_n / 2 + (1 - s) * est_p / 2
    return torch.where(site == own, cfa, torch.where(site == gsite, along_row, torch.where(site == osite, along_col, diag)))


def hamilton_adams(x: torch.Tensor, pattern: str) -> torch.Tensor:
    """HamiltonAdam(pattern)(x): [B,4k,h,w] packed raw -> [B,3k,2h,2w] RGB, fp32, on the CPU."""
    if pattern not in PHASE:
        raise ValueError(pattern)
    B0, C, h, w = x.shape
    cfa = pack_in_one(x.detach().float().cpu().reshape(-1, 4, h, w))
    site = colour_sites(2 * h, 2 * w, pattern)[None]
    green = _green(cfa, site)
    rgb = torch.stack((_chroma(cfa, green, site, 2), green, _chroma(cfa, green, site, 1)), 1)
    return rgb.reshape(B0, 3 * (C // 4), 2 * h, 2 * w)


# cropping the first row and / or column of a GBRG mosaic turns it into each other pattern
CROPS = {"rggb": (1, 0), "grbg": (1, 1), "bggr": (0, 1)}


def interior_identity(demosaic, pattern, gen):
    """demosaic(packed, pattern) of a GBRG mosaic cropped by one row and / or column on each side equals the GBRG demosaic
    of the whole mosaic, cropped the same way, bit for bit -- except within 3 pixels (Hamilton-Adams' reach) of the new
    borders.  Returns (got, want) on the compared region."""
    cy, cx = CROPS[pattern]
    m = torch.rand(2, 38, 54, generator=gen) * 2 - 1
    m[0, 10:20, 8:30] = 0.25                                 # plateaus: sign() ties
    full = demosaic(pack(m), "gbrg")
    cropped = m[:, cy:m.shape[1] - cy, cx:m.shape[2] - cx]
    got = demosaic(pack(cropped), pattern)
    want = full[:, :, cy:full.shape[2] - cy, cx:full.shape[3] - cx]
    ry, rx = 3 * cy, 3 * cx
    return got[:, :, ry:got.shape[2] - ry, rx:got.shape[3] - rx], want[:, :, ry:want.shape[2] - ry, rx:want.shape[3] - rx]
