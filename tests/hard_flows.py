"""Flows that are hard on the bicubic backward warp, and what the tests of the warps share (test_hard_flows_host.py,
test_gpu_warp_ops.py, test_gpu_hard_flows.py, test_gpu_random_weights.py).  A plain module: no fixtures, no pytest settings;
pytest does not rewrite its asserts, so each one carries its message.

Four flow families at raw resolution [T, B, 2, h, w], each from a seed, on the CPU:

    synth    synth.make_sequence's analytic flows: sub-pixel to a few pixels, smooth
    wild     6 * synth + N(0, 9): leaves the frame, differs from pixel to pixel
    blocks   six rectangles per frame over the synth flow, each with one constant sub-pixel vector of up to +-0.8 of the frame
             size, edges at arbitrary raw columns: object edges and scene cuts
    border   constant per quadrant, (+-1.5, +-2.5) px of the full frame; within four raw pixels of an edge the component that
             points outwards grows linearly from 0 to 3 px: partly clamped footprints on all four sides

gather_paths restates warp.h's taps and warp48_kernel's choice between its two gathers as boolean maps, so that a test can
demand that its inputs reach both.  warp_mutant and the STEP_MUTANTS are the reference with one deliberate mistake each:
the host test proves with them that the bounds of the GPU tests would catch such a mistake."""
import functools

import torch
import torch.nn.functional as F

import rvdd_oracle as O
import random_weights as RW
from conftest import load_weights

FAMILIES = ("synth", "wild", "blocks", "border")
EPS32 = 2.0 ** -23


# ---- the families ------------------------------------------------------------------------------------------------------------------
def wild(flow, seed):
    gen = torch.Generator().manual_seed(seed)
    return flow * 6.0 + torch.randn(flow.shape, generator=gen) * 9.0


def blocks(flow, seed, count=6, reach=0.8):
    gen = torch.Generator().manual_seed(seed)
    T, B, _, h, w = flow.shape
    out = flow.clone()
    u = lambda: float(torch.rand(1, generator=gen))
    for t in range(T):
        for b in range(B):
            for _ in range(count):
                bh, bw = max(1, int(h * (0.25 + 0.5 * u()))), max(1, int(w * (0.25 + 0.5 * u())))
                y0, x0 = int(u() * (h - bh + 1)), int(u() * (w - bw + 1))
                out[t, b, 0, y0:y0 + bh, x0:x0 + bw] = (2 * u() - 1) * reach * w + 0.37      # raw pixels: twice that at full size
                out[t, b, 1, y0:y0 + bh, x0:x0 + bw] = (2 * u() - 1) * reach * h + 0.37
    return out


def border(flow, seed, band=4, push=3.0):
    """`seed` picks which quadrant gets which pair of signs."""
    T, B, _, h, w = flow.shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    right, low = xx >= w // 2, yy >= h // 2
    sx = torch.where(right ^ low, 1.0, -1.0) * (1.0 if seed % 2 else -1.0)
    sy = torch.where(low, 1.0, -1.0) * (1.0 if (seed // 2) % 2 else -1.0)
    ramp = lambda d: push * (1.0 - d / band).clamp(min=0.0)
    fx = 1.5 * sx - ramp(xx) + ramp(w - 1 - xx)          # full-frame pixels
    fy = 2.5 * sy - ramp(yy) + ramp(h - 1 - yy)
    return (torch.stack((fx, fy)) / 2.0).expand(T, B, 2, h, w).clone()      # the step upsamples the flow and doubles it


def family_flow(family, flow, seed):
    """`flow`: the synth flow of the sequences [T, B, 2, h, w] -> the family's, same shape"""
    if family == "synth":
        return flow
    return {"wild": wild, "blocks": blocks, "border": border}[family](flow, seed)


def _sequences(B, H, W, T, seed0, iso=3200, pattern="gbrg"):
    from rvdd_release_amd import synth
    seqs = [synth.make_sequence(T, H, W, iso=iso, seed=seed0 + b, pattern=pattern) for b in range(B)]
    st = lambda key: torch.stack([getattr(s, key) for s in seqs], 1)      # [T,B,...]
    return st("raw"), st("flow_prev"), st("flow_next")


def hard_sequences(family, B, H, W, T, seed0, pattern="gbrg"):
    """-> raw [T,B,4,h,w], flow_prev and flow_next [T,B,2,h,w] of the family (the two from different draws)"""
    raw, fp, fn = _sequences(B, H, W, T, seed0, pattern=pattern)
    return raw, family_flow(family, fp, seed0 + 5), family_flow(family, fn, seed0 + 6)


def full_flow(flow_raw):
    """the full-resolution flow a step warps with, in the arithmetic of warp.h's flow_at"""
    return O.upsample_factor_2_explicit(flow_raw, multiply_by=2)


# ---- the taps of warp.h's make_taps, and which gather of warp48_kernel a pair of pixels takes ------------------------------------------
def taps(flow, round_trip=True):
    """flow [..., 2, H, W] at full resolution -> x0, y0 (long, before any clamp) and the cubic weights wx, wy (4-tuples), in
    O.warp_explicit's f32 arithmetic.  round_trip False leaves out the [-1, 1] normalisation (mutant d)."""
    H, W = flow.shape[-2:]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    vx = xx.float() + flow[..., 0, :, :]
    vy = yy.float() + flow[..., 1, :, :]
    if round_trip:
        gx = 2.0 * vx / (W - 1) - 1.0
        gy = 2.0 * vy / (H - 1) - 1.0
        ix = ((gx + 1.0) / 2.0) * (W - 1)
        iy = ((gy + 1.0) / 2.0) * (H - 1)
    else:
        ix, iy = vx, vy
    x0, y0 = ix.floor(), iy.floor()
    return x0.long(), y0.long(), O._cubic_w(ix - x0), O._cubic_w(iy - y0)


def _clamped_taps(x0, y0, H, W):
    xi = torch.stack([(x0 - 1 + i).clamp(0, W - 1) for i in range(4)], -1)
    yi = torch.stack([(y0 - 1 + j).clamp(0, H - 1) for j in range(4)], -1)
    return xi, yi


def _lined_up(xi, yi):
    """warp48_kernel's predicate for the pair (2p, 2p+1): the same four rows, the columns shifted by one -> [..., H, W/2]"""
    xa, xb, ya, yb = xi[..., 0::2, :], xi[..., 1::2, :], yi[..., 0::2, :], yi[..., 1::2, :]
    return (ya == yb).all(-1) & (xb[..., :3] == xa[..., 1:]).all(-1)


def gather_paths(flow_raw, H, W):
    """flow_raw [..., 2, h, w] -> dict: xi, yi [..., H, W, 4] (the clamped taps), lined_up [..., H, W/2] (the pair takes the
    shared 20-load gather), partly [..., H, W] (some but not all of the 16 taps are clamped), outside [..., H, W] (all are: the
    pixel samples wholly outside the frame)."""
    assert flow_raw.shape[-2:] == (H // 2, W // 2), (flow_raw.shape, H, W)
    x0, y0, _, _ = taps(full_flow(flow_raw))
    xi, yi = _clamped_taps(x0, y0, H, W)
    cx = torch.stack([(x0 - 1 + i < 0) | (x0 - 1 + i > W - 1) for i in range(4)], -1)
    cy = torch.stack([(y0 - 1 + j < 0) | (y0 - 1 + j > H - 1) for j in range(4)], -1)
    every, some = cx.all(-1) | cy.all(-1), cx.any(-1) | cy.any(-1)
    return {"xi": xi, "yi": yi, "lined_up": _lined_up(xi, yi), "partly": some & ~every, "outside": every}


def gather_sum(x, xi, yi, wx, wy):
    """x [B,C,H,W], taps [B,H,W,4], weights 4-tuples of [B,H,W]: the 16-tap sum in O.warp_explicit's order"""
    bidx = torch.arange(x.shape[0])[:, None, None]
    out = torch.zeros_like(x)
    for j in range(4):
        row = torch.zeros_like(x)
        for i in range(4):
            row = row + x[bidx, :, yi[..., j], xi[..., i]].permute(0, 3, 1, 2) * wx[i][:, None]
        out = out + row * wy[j][:, None]
    return out


def warp_from_taps(x, flow):
    """O.warp_explicit through taps / gather_sum: bit for bit the same (the host test holds it to that)"""
    x0, y0, wx, wy = taps(flow)
    return gather_sum(x, *_clamped_taps(x0, y0, *x.shape[-2:]), wx, wy)


# ---- the reference with one deliberate mistake ---------------------------------------------------------------------------------------
WARP_MUTANTS = ("a", "b", "c", "d")


def warp_mutant(x, flow, kind):
    """O.warp_explicit(x, flow) with one mistake: (a) the second pixel of a lined-up pair takes the first one's y-weights,
    (b) ... the first one's four columns, unshifted, (c) the footprint is clamped as a block (x0 - 1 into [0, W - 4], then + i),
    (d) the coordinates skip the round trip through [-1, 1]."""
    H, W = x.shape[-2:]
    x0, y0, wx, wy = taps(flow, round_trip=kind != "d")
    xi, yi = _clamped_taps(x0, y0, H, W)
    if kind in ("a", "b"):
        pair = _lined_up(xi, yi)
        if kind == "a":
            wy = tuple(torch.stack((v[..., 0::2], torch.where(pair, v[..., 0::2], v[..., 1::2])), -1).flatten(-2) for v in wy)
        else:
            xi = torch.stack((xi[..., 0::2, :], torch.where(pair[..., None], xi[..., 0::2, :], xi[..., 1::2, :])), -2).flatten(-3, -2)
    elif kind == "c":
        xi = torch.stack([(x0 - 1).clamp(0, W - 4) + i for i in range(4)], -1)
        yi = torch.stack([(y0 - 1).clamp(0, H - 4) + j for j in range(4)], -1)
    elif kind != "d":
        raise ValueError(kind)
    return gather_sum(x, xi, yi, wx, wy)


# (e) the flow upsample with align_corners=False, (f) without its factor 2, (g) batch element b warps with the flow of b - 1
STEP_MUTANTS = {
    "e": dict(upsample=lambda fl: F.interpolate(fl, scale_factor=2, mode="bilinear", align_corners=False) * 2),
    "f": dict(upsample=lambda fl: O.upsample_factor_2(fl, multiply_by=1)),
    "g": dict(warp=lambda x, fl: O.warp(x, fl.roll(1, 0))),
}


# ---- two frame-steps from a reset ----------------------------------------------------------------------------------------------------
def _oracle_steps(sd, fut, raw, dtype, flow_prev=None, flow_next=None, warp=None, upsample=None, demosaic=None):
    """Two frame-steps of the recurrence (oracle/rvdd_oracle.py RecurrentOracle.step) with the net, the state and the warps in
    `dtype`; flow_prev None = --no_warp.  raw [T,B,4,h,w], flows [T,B,2,h,w] -> [out 1, out 2, features after step 2 (None for a
    net without feature recurrence)].
    The demosaic is always the f32 one (the device's, bit for bit) and is cast: in f32 this is RecurrentOracle itself.
    warp(x, flow) and upsample(raw flow) -> full flow replace the ATen forms (O.warp, O.upsample_factor_2 times 2), demosaic(raw)
    the GBRG one."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    ha = lambda r: (demosaic or O.hamilton_adams)(r).to(dtype)
    wp = warp or O.warp
    ups = upsample or (lambda fl: O.upsample_factor_2(fl, multiply_by=2))
    up = lambda fl: ups(fl.to(dtype))
    lastden = ha(raw[0])
    B, _, H, W = lastden.shape
    feat = torch.zeros(B, 48, H, W, dtype=dtype) if O.net_has_feat(sd) else None
    outs = []
    with torch.no_grad():
        for t in (1, 2):
            n_cur = ha(raw[t])
            if flow_prev is None:
                parts, fin = [lastden, n_cur], feat
            else:
                fp = up(flow_prev[t])
                parts, fin = [wp(lastden, fp), n_cur], None if feat is None else wp(feat, fp)
            if fut:
                parts.append(ha(raw[t + 1]) if flow_prev is None else wp(ha(raw[t + 1]), up(flow_next[t])))
            lastden, feat = O.net_forward(sdd, torch.cat(parts, 1), fin)
            outs.append(lastden)
    return outs + [feat]


def _device_steps(arch, fut, shape, sd, raw, options, flow_prev=None, flow_next=None, seen=None):
    """`seen`: a dict that receives the profile's launches of the two steps (gpu_support.launches)"""
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime(arch, fut, *shape, 0)
    try:
        for k, v in options.items():
            rt.set_option(k, v)
        rt.load_state_dict(sd)
        raw = raw.cuda()
        fp = None if flow_prev is None else flow_prev.cuda()
        fn = None if flow_next is None or not fut else flow_next.cuda()
        if seen is not None:
            rt.profile_enable(True)
        outs = []
        for t in (1, 2):
            outs.append(rt.step(raw[0] if t == 1 else None, raw[t], raw[t + 1] if fut else None,
                                None if fp is None else fp[t], None if fn is None else fn[t]).cpu())
        if seen is not None:
            seen.update({p["name"]: p["launches"] for p in rt.profile_read() if p["launches"]})
            rt.profile_enable(False)
        feat = rt.get_state()[1]
        return outs + [None if feat is None else feat.cpu()]
    finally:
        rt.close()


# ---- the cases of the GPU tests, with the references they share ------------------------------------------------------------------------
STEP_SHAPES = ((2, 50, 66), (3, 18, 34))
STEP_FLOWS = ("wild", "blocks", "border")
STEP_WEIGHTS = ("trained", "he")
STEP_NETS = {     # stem -> (arch, future)
    "recurrent-convunet-future-iso3200": ("convunet", 1),
    "recurrent-convunet+feat-iso3200": ("convunet+feat", 0),
    "recurrent-convunet+feat-future-iso12800": ("convunet+feat", 1),
    "recurrent-ConvNeXtUnet+feat-future-iso3200": ("next+feat", 1),
    "recurrent-ConvNeXtUnet-iso3200": ("next", 0),
}
BAYER_CASE = ("recurrent-convunet+feat-future-iso12800", "rggb")      # the network-input kernels are templated on the pattern's phase
WARP_SHAPES = ((1, 1, 2, 2), (3, 2, 2, 301), (1, 3, 301, 2), (2, 5, 37, 53), (2, 48, 50, 66), (1, 4, 129, 257))
WARP_FLOWS = ("n1.5", "n30", "n1e4") + FAMILIES
UPSAMPLE_SHAPES = ((1, 1, 1), (2, 1, 7), (2, 9, 1), (4, 18, 26), (3, 25, 33))


def step_weights(stem, weights):
    return load_weights(stem) if weights == "trained" else RW.random_state_dict(stem, 5, weights)


@functools.lru_cache(maxsize=4)
def step_inputs(family, shape, T, pattern="gbrg"):
    B, H, W = shape
    return hard_sequences(family, B, H, W, T, 2100 + H, pattern)


@functools.lru_cache(maxsize=4)
def step_reference(stem, weights, family, shape, pattern="gbrg"):
    """-> (state dict, raw, flow_prev, flow_next, the two steps in f32, in f64, e_ref of the three outputs); kept, so that the
    option variants of a case share it, and never written to"""
    _, fut = STEP_NETS[stem]
    sd = step_weights(stem, weights)
    raw, fp, fn = step_inputs(family, shape, 3 + fut, pattern)
    dm = None
    if pattern != "gbrg":
        import bayer_ref
        dm = lambda r: bayer_ref.hamilton_adams(r, pattern)
    o32 = _oracle_steps(sd, fut, raw, torch.float32, fp, fn, demosaic=dm)
    o64 = _oracle_steps(sd, fut, raw, torch.float64, fp, fn, demosaic=dm)
    return sd, raw, fp, fn, o32, o64, [None if a is None else RW.rel_err(a, b) for a, b in zip(o32, o64)]


def _normal(shape, sigma, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * sigma


@functools.lru_cache(maxsize=2)
def warp_case(shape, flows):
    """One case of rvdd_warp_bicubic -> (x, full flow, warp_explicit in f32, s_ref, err(explicit32, f64), max|f64|).  x is
    N(0, 1); odd sizes take their families' flows from the next even size, cropped."""
    n, c, H, W = shape
    x = _normal(shape, 1.0, 17 * H + W)
    if flows in FAMILIES:
        He, We = H + H % 2, W + W % 2
        base = torch.stack([_sequences(1, max(He, 16), max(We, 16), 2, 2300 + b)[1][1, 0, :, :He // 2, :We // 2] for b in range(n)])
        flow = full_flow(family_flow(flows, base[None], 2300 + H)[0])[:, :, :H, :W].contiguous()
    else:
        flow = _normal((n, 2, H, W), float(flows[1:]), 31 * H + W)
    want, aten, w64 = O.warp_explicit(x, flow), O.warp(x, flow), O.warp(x.double(), flow.double())
    top = float(w64.abs().max())
    return x, flow, want, float((aten.double() - want.double()).abs().max()) / top, float((want.double() - w64).abs().max()) / top, top


@functools.lru_cache(maxsize=2)
def upsample_case(shape, mul):
    """-> (t, upsample_factor_2_explicit, the spread of the two CPU forms over the output's maximum, that maximum)"""
    nc, h, w = shape
    t = _normal((nc, 1, h, w), 20.0, 7 * h + w)
    want, aten = O.upsample_factor_2_explicit(t, mul), O.upsample_factor_2(t, mul)
    top = float(want.abs().max())
    return t, want, float((aten.double() - want.double()).abs().max()) / top, top
