"""Packed 10 / 12 / 14-bit raw frames through the C ABI (rvdd_ingest_bits, rvdd_egress_bits, option "stream_container", the denoise
command line): the kernels against rvdd_ingest_raw / rvdd_egress of the unpacked uint16 frames and the numpy packing of
bits_ref.py, both kernel forms, the round trip, the stream against the same pushes of uint16 frames, and the command on disk.
Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bits_ref
from conftest import WEIGHTS
from egress_ref import PATTERNS, fill
from gpu_support import files_of, make_runtime as _runtime, ops_rt as _rt, same, upload
from stream_compose import FIRST, IDLE, NEXT, push_schedule, synth_video as _video
from stream_ref import mosaic_of, quantised_dn, to_gpu

pytestmark = pytest.mark.gpu

U16 = getattr(torch, "uint16", torch.int16)
ORDERS, DEPTHS = bits_ref.ORDERS, bits_ref.DEPTHS


def _mipi_ok(order, bits, ww):
    return order != "mipi" or (2 * ww) % bits_ref.group(bits) == 0


def _frames(kind, n, hh, ww, bits, seed):
    """uint16 [n,2hh,2ww]"""
    top = (1 << bits) - 1
    shape = (n, 2 * hh, 2 * ww)
    if kind == "random":
        x = np.random.default_rng(seed).integers(0, top + 1, shape).astype(np.uint16)
        x[0, 0, :2], x[-1, -1, -2:] = (0, top), (top, 0)
        return x
    if kind == "ramp":
        return (np.arange(int(np.prod(shape)), dtype=np.int64) % (top + 1)).astype(np.uint16).reshape(shape)
    return np.full(shape, 0 if kind == "zeros" else top, np.uint16)


def _check_ingest(rt, x, bits, order, at=0, dirty_pad=False):
    n, H, W = x.shape
    hh, ww = H // 2, W // 2
    want_p, want_g = rt.ingest_raw(to_gpu(x), bits, "mosaic")
    rows = bits_ref.pack(x, bits, order)
    if dirty_pad:
        pad = 8 * rows.shape[-1] - W * bits
        assert pad > 0
        rows = rows.copy()
        rows[..., -1] |= (1 << pad) - 1
    src = upload(rows)
    if at:
        src, _ = upload(src, offset=at, fill=0xA5)            # `at` bytes into a larger allocation
    assert src.data_ptr() % 4 == at % 4
    got_p, got_g = rt.ingest_bits(src, order, bits, hh, ww, n=n)
    assert torch.equal(got_p, want_p) and torch.equal(got_g, want_g), (order, bits, n, hh, ww, at)
    only_g = rt.ingest_bits(src, order, bits, hh, ww, n=n, want_packed=False)
    only_p = rt.ingest_bits(src, order, bits, hh, ww, n=n, want_gray=False)
    assert only_g[0] is None and torch.equal(only_g[1], want_g) and only_p[1] is None and torch.equal(only_p[0], want_p)


# ---- 1. ingest -------------------------------------------------------------------------------------------------------------------
# cells (16,16): the dword form; (9,18): row_bytes 45 at 10 bits -- odd, the byte form, and for n = 3 a frame stride that is no
# multiple of 4; (5,7): an odd ww -- MSB pad bits at 10 and 14 bits, refused for MIPI there
@pytest.mark.parametrize("hh,ww", [(16, 16), (9, 18), (5, 7)])
@pytest.mark.parametrize("bits", DEPTHS)
@pytest.mark.parametrize("order", ORDERS)
def test_ingest_bits_is_ingest_raw_of_the_unpacked_frames(order, bits, hh, ww):
    rt = _rt()
    if not _mipi_ok(order, bits, ww):
        frames = torch.zeros(1, 2 * hh, bits_ref.row_bytes(2 * ww, bits, "msb"), dtype=torch.uint8, device="cuda")
        with pytest.raises(RuntimeError, match=r"\(-1\).*ww"):
            rt.ingest_bits(frames, order, bits, hh, ww)
        return
    for n in (1, 3):
        for kind in ("random", "zeros", "ones"):
            _check_ingest(rt, _frames(kind, n, hh, ww, bits, 1000 * hh + 10 * bits + n), bits, order)
    if (hh, ww) == (16, 16):                           # the same shape one byte into its buffer: the byte form
        for n in (1, 3):
            _check_ingest(rt, _frames("random", n, hh, ww, bits, 77 + n), bits, order, at=1)
            _check_ingest(rt, _frames("random", n, hh, ww, bits, 78 + n), bits, order, at=4)       # still dwords
    if order == "msb" and (2 * ww * bits) % 8:
        for n in (1, 3):
            _check_ingest(rt, _frames("random", n, hh, ww, bits, 99 + n), bits, order, dirty_pad=True)


@pytest.mark.parametrize("bits", [10, 12])
@pytest.mark.parametrize("order", ORDERS)
def test_ingest_bits_ramp_through_every_value(order, bits):
    rt = _rt()
    x = _frames("ramp", 1, 32, 32, bits, 0)            # 4096 samples: every value of 12 bits, of 10 bits four times
    assert np.unique(x).size == 1 << bits
    _check_ingest(rt, x, bits, order)
    _check_ingest(rt, x, bits, order, at=3)
    _check_ingest(rt, np.ascontiguousarray(x[:, :, :36]), bits, order)      # ww = 18: the byte form


def test_footage_ingest_frames_is_the_direct_ingest():
    """`footage.ingest_frames` -- the host-frames-to-packed/gray branch of noise, cuts and dpc_map -- against `ingest_raw` /
    `ingest_bits` called directly, bit for bit: two 32 x 48 frames as a uint16 mosaic, as float32 packed_hwc, as a 10-bit msb and a
    12-bit mipi container, through a stub dataset that carries `container` and `layout` and nothing else."""
    import types
    from rvdd_release_amd import footage
    from rvdd_release_amd.runtime import raw_frames_to_device
    rt = _rt()
    cases = []
    for bits, container in ((12, None), (10, "msb"), (12, "mipi")):
        x = _frames("random", 2, 16, 24, bits, 7 + bits)
        if container is None:
            hwc = np.stack([x[:, k >> 1::2, k & 1::2] for k in range(4)], axis=-1).astype(np.float32)
            cases.append((bits, "mosaic", None, x, rt.ingest_raw(raw_frames_to_device(x, "cuda"), bits, "mosaic")))
            cases.append((bits, "packed_hwc", None, hwc, rt.ingest_raw(upload(hwc), bits, "packed_hwc")))
            assert all(torch.equal(a, b) for a, b in zip(cases[0][4], cases[1][4]))      # the same frames: the same planes
        else:
            rows = bits_ref.pack(x, bits, container)
            assert rows.shape == (2, 32, 48 * bits // 8) and rows.dtype == np.uint8
            cases.append((bits, "mosaic", container, rows, rt.ingest_bits(upload(rows), container, bits, 16, 24, n=2)))
            assert all(torch.equal(a, b) for a, b in zip(cases[-1][4], rt.ingest_raw(to_gpu(x), bits, "mosaic")))
    for bits, layout, container, frames, (want_p, want_g) in cases:
        ds = types.SimpleNamespace(container=container, layout=layout)
        assert want_p.shape == (2, 4, 16, 24) and want_g.shape == (2, 16, 24)
        got_p, got_g = footage.ingest_frames(rt, ds, frames, bits)
        assert torch.equal(got_p, want_p) and torch.equal(got_g, want_g), (bits, layout, container)
        only_p = footage.ingest_frames(rt, ds, frames, bits, want_gray=False)
        only_g = footage.ingest_frames(rt, ds, frames, bits, want_packed=False)
        assert only_p[1] is None and torch.equal(only_p[0], want_p) and only_g[0] is None and torch.equal(only_g[1], want_g)
        assert footage.ingest_frames(rt, ds, frames, bits, want_packed=False, want_gray=False) == (None, None)


# ---- 2. egress -------------------------------------------------------------------------------------------------------------------
# (32,32): the dword form; (18,36): the byte form (W/2 = 18; 45-byte rows at 10 bits); (10,14): an odd ww
@pytest.mark.parametrize("H,W", [(32, 32), (18, 36), (10, 14)])
@pytest.mark.parametrize("bits", DEPTHS)
@pytest.mark.parametrize("order", ORDERS)
def test_egress_bits_is_the_packed_egress(order, bits, H, W):
    rt = _rt()
    if not _mipi_ok(order, bits, W // 2):
        with pytest.raises(RuntimeError, match=r"\(-1\).*ww"):
            rt.egress_bits(torch.zeros(1, 3, H, W, device="cuda"), order, bits, "gbrg")
        return
    rb = bits_ref.row_bytes(W, bits, order)
    for n in (1, 3):
        x = upload(fill(n, H, W, seed=H + W + bits + n))             # values outside [-1,1], NaN, the infinities, every 8-bit tie
        assert x.data_ptr() % 16 == 0
        for pattern in PATTERNS:
            u16 = rt.egress(x, "mosaic", U16, bits, pattern).view(torch.int16).cpu().numpy().view(np.uint16)
            assert int(u16.max()) == (1 << bits) - 1 and int(u16.min()) == 0
            want = bits_ref.pack(u16, bits, order)
            assert want.shape == (n, H, rb)
            got = rt.egress_bits(x, order, bits, pattern)
            assert got.shape == (n, H, rb) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (n, pattern)
            # 8 sentinel bytes on each side; whatever the buffer held, every byte inside is written (pad bits: zero) and none outside.
            # at = 8 keeps the dword form where the shape has it, at = 9 is the byte form of the same shape
            for at in (8, 9):
                for before in (0xFF, 0x00):
                    whole = torch.full((n * H * rb + 2 * at,), before, dtype=torch.uint8, device="cuda")
                    out = whole[at:at + n * H * rb]
                    back = rt.egress_bits(x, order, bits, pattern, out=out)
                    assert back.data_ptr() == out.data_ptr()
                    host = whole.cpu().numpy()
                    assert np.array_equal(host[at:-at].reshape(n, H, rb), want), (n, pattern, at, before)
                    assert (host[:at] == before).all() and (host[-at:] == before).all(), (n, pattern, at, before)
    if (8 * rb - W * bits) > 0:
        assert not (want[..., -1] & ((1 << (8 * rb - W * bits)) - 1)).any()


def test_pattern_defaults_to_the_handles_and_arguments_are_checked():
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime("convunet", 0, 1, 64, 96, 0)
    x = torch.rand(2, 3, 8, 16, device="cuda") * 2 - 1
    assert torch.equal(rt.egress_bits(x, "msb", 12), rt.egress_bits(x, "msb", 12, "gbrg"))
    rt.set_option("bayer_pattern", 2)
    assert torch.equal(rt.egress_bits(x, "msb", 12), rt.egress_bits(x, "msb", 12, "rggb"))
    assert not torch.equal(rt.egress_bits(x, "msb", 12), rt.egress_bits(x, "msb", 12, "gbrg"))
    with pytest.raises(ValueError, match="order"):
        rt.egress_bits(x, "lsb", 12)
    with pytest.raises(ValueError, match="pattern"):
        rt.egress_bits(x, "msb", 12, "xtrans")
    with pytest.raises(RuntimeError, match="out must be"):
        rt.egress_bits(x, "msb", 12, out=torch.empty(2 * 8 * 24 + 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="order"):
        rt.ingest_bits(torch.zeros(8 * 24, dtype=torch.uint8, device="cuda"), "lsb", 12, 4, 8)
    with pytest.raises(RuntimeError, match="bytes"):
        rt.ingest_bits(torch.zeros(8 * 24 + 1, dtype=torch.uint8, device="cuda"), "msb", 12, 4, 8)
    with pytest.raises(RuntimeError, match="uint8"):
        rt.ingest_bits(torch.zeros(4 * 24, dtype=torch.int16, device="cuda"), "msb", 12, 4, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.ingest_bits(torch.zeros(8 * 24, dtype=torch.uint8), "msb", 12, 4, 8)


def test_bits_bad_arguments():
    rt = _rt()
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    out = torch.full((32 * 48,), 0x5A, dtype=torch.uint8, device="cuda")
    src = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    packed = torch.full((1, 4, 16, 16), 7.0, device="cuda")
    gray = torch.full((1, 16, 16), 7.0, device="cuda")

    def egress(n=1, H=32, W=32, order=1, bit_depth=12, pattern=0, rgb=x.data_ptr(), o=out.data_ptr()):
        rc = rt.lib.rvdd_egress_bits(rt.h, rgb, n, H, W, order, bit_depth, pattern, o, None)
        return rc, rt.lib.rvdd_last_error(rt.h)

    def ingest(frames=src.data_ptr(), order=1, n=1, hh=16, ww=16, bit_depth=12, p=packed.data_ptr(), g=gray.data_ptr()):
        rc = rt.lib.rvdd_ingest_bits(rt.h, frames, order, n, hh, ww, bit_depth, p, g, None)
        return rc, rt.lib.rvdd_last_error(rt.h)

    for kw, word in [({"order": -1}, b"order"), ({"order": 2}, b"order"), ({"bit_depth": 11}, b"bit_depth"), ({"bit_depth": 16}, b"bit_depth"),
                     ({"bit_depth": 8}, b"bit_depth"), ({"H": 31}, b" H "), ({"W": 31}, b" W "), ({"H": 0}, b" H "), ({"W": 0}, b" W "),
                     ({"W": 30, "order": 0, "bit_depth": 10}, b"ww"), ({"W": 30, "order": 0, "bit_depth": 14}, b"ww"),
                     ({"pattern": 4}, b"pattern"), ({"pattern": -1}, b"pattern"), ({"n": -1}, b" n "), ({"rgb": None}, b"rgb"), ({"o": None}, b"out"),
                     ({"n": 1 << 24, "H": 1 << 12, "W": 1 << 12}, b"blocks")]:
        rc, msg = egress(**kw)
        assert rc == -1 and msg.startswith(b"rvdd_egress_bits:") and word in msg, (kw, msg)
    for kw, word in [({"order": -1}, b"order"), ({"order": 2}, b"order"), ({"bit_depth": 11}, b"bit_depth"), ({"bit_depth": 16}, b"bit_depth"),
                     ({"hh": 0}, b"hh"), ({"ww": 0}, b"ww"), ({"ww": 15, "order": 0, "bit_depth": 10}, b"ww"),
                     ({"ww": 15, "order": 0, "bit_depth": 14}, b"ww"), ({"n": -1}, b" n "), ({"frames": None}, b"frames"),
                     ({"n": 1 << 24, "hh": 1 << 11, "ww": 1 << 11}, b"blocks")]:
        rc, msg = ingest(**kw)
        assert rc == -1 and msg.startswith(b"rvdd_ingest_bits:") and word in msg, (kw, msg)
    assert egress(n=0)[0] == 0 and egress(n=0, rgb=None, o=None)[0] == 0 and ingest(n=0)[0] == 0 and ingest(n=0, frames=None)[0] == 0
    assert egress(W=30, order=0, bit_depth=12)[0] == 0 and ingest(ww=15, order=0, bit_depth=12)[0] == 0       # RAW12: pairs
    torch.cuda.synchronize()
    # only those two wrote: 32 rows of 45 bytes, and [1,4,16,15] / [1,16,15] planes at the start of the buffers
    assert bool((out[32 * 45:] == 0x5A).all()) and not bool((out[:32 * 45] == 0x5A).any())
    assert bool((packed.reshape(-1)[4 * 16 * 15:] == 7.0).all()) and bool((gray.reshape(-1)[16 * 15:] == 7.0).all())


# ---- 3. the round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["gbrg", "rggb"])
@pytest.mark.parametrize("bits", DEPTHS)
@pytest.mark.parametrize("order", ORDERS)
def test_packed_frames_come_back(order, bits, pattern):
    rt = _rt()
    for hh, ww in ((16, 16), (9, 18), (5, 7)):
        if not _mipi_ok(order, bits, ww):
            continue
        x = _frames("random", 3, hh, ww, bits, hh + bits)
        rows = upload(bits_ref.pack(x, bits, order))
        packed, _ = rt.ingest_bits(rows, order, bits, hh, ww, want_gray=False)
        back = rt.egress_bits(rt.demosaic(packed, pattern), order, bits, pattern)
        assert torch.equal(back, rows), (hh, ww)


# ---- 4. the stream -----------------------------------------------------------------------------------------------------------------
H, W, B = 36, 52, 3                                    # 18 x 26 cells
FEAT = {0: "recurrent-convunet+feat-iso3200", 1: "recurrent-convunet+feat-future-iso12800"}
LENGTHS = (4, 2, 3, 2)


def _videos(bits):
    """12-bit synthetic videos moved to `bits` bits"""
    vs = [_video(n, H, W, seed=300 + v) for v, n in enumerate(LENGTHS)]
    return [(v >> 2) if bits == 10 else v if bits == 12 else ((v << 2) | (v & 3)) for v in vs]


def _run(rt, videos, steps, bits, container, between=None):
    """the pushes of `steps` (denoise.deal_slots) -> {video: [outputs]}, [valid flags of every push]"""
    got = push_schedule(rt, videos, steps, bits, container, between=between)
    return got.by_video, got.flags


STREAM_CASES = [(0, {}), (1, {"stream_all_frames": 1}), (0, {"stream_flow_from_denoised": 1}), (0, {"bayer_pattern": 2, "stream_reset_each": 1}),
                (1, {"no_warp": 1})]


@pytest.mark.parametrize("future,options", STREAM_CASES, ids=["-".join(o) or "plain" for _, o in STREAM_CASES])
def test_stream_container_is_the_stream_of_the_unpacked_frames(future, options):
    from rvdd_release_amd.denoise import deal_slots
    rt = _runtime("convunet+feat", FEAT[future], future, B, H, W, **options)
    steps = deal_slots(LENGTHS, B, tail=future if options.get("stream_all_frames") else 0)
    ctls = {c for s in steps for c, _, _ in s}
    assert ctls == {FIRST, NEXT, IDLE}
    for bits in DEPTHS:
        videos = _videos(bits)
        want, want_flags = _run(rt, videos, steps, bits, None)
        assert sum(len(w) for w in want.values()) > 0 and any(not all(f) for f in want_flags)
        for order in ORDERS:
            got, flags = _run(rt, videos, steps, bits, order)
            assert rt.stream_container == 1 + ORDERS.index(order)
            assert flags == want_flags, (bits, order)
            for v in want:
                same(got[v], want[v], (bits, order, v), allow_empty=True)      # a video of two frames has no output before a future frame
    rt.set_option("tvl1_async", 0)


def test_stream_container_argument_errors_change_nothing():
    from rvdd_release_amd import _lib
    from rvdd_release_amd.denoise import deal_slots
    from rvdd_release_amd.runtime import RvddRuntime
    rt = _runtime("convunet+feat", FEAT[0], 0, B, H, W)
    steps = deal_slots(LENGTHS, B)
    videos = _videos(12)
    want, want_flags = _run(rt, videos, steps, 12, None)
    out = torch.empty(B, 3, H, W, device="cuda")

    def refused(i, frames):
        """between two valid pushes, with the option on: each is RVDD_ERR_ARG and leaves the stream as it was"""
        if i != 2:
            return
        assert rt.stream_container == 1
        with pytest.raises(RuntimeError, match=r"\(-1\).*stream_container"):
            rt.set_option("stream_container", 3)
        ctl = (C.c_uint8 * B)(*[NEXT] * B)
        valid = (C.c_uint8 * B)()
        for dtype, layout, depth, word in ((_lib.RAW_F32, _lib.RAW_MOSAIC, 12, b"dtype"), (_lib.RAW_U16, _lib.RAW_PACKED_HWC, 12, b"layout"),
                                           (_lib.RAW_U16, _lib.RAW_MOSAIC, 11, b"bit_depth"), (_lib.RAW_U16, _lib.RAW_MOSAIC, 16, b"bit_depth")):
            rc = rt.lib.rvdd_video_push(rt.h, frames.data_ptr(), dtype, layout, depth, ctl, out.data_ptr(), valid, None)
            msg = rt.lib.rvdd_last_error(rt.h)
            assert rc == -1 and msg.startswith(b"rvdd_video_push:") and word in msg, msg

    got, flags = _run(rt, videos, steps, 12, "mipi", between=refused)
    assert flags == want_flags
    for v in want:
        assert len(got[v]) == len(want[v]) and all(torch.equal(g, w) for g, w in zip(got[v], want[v])), v
    rt.set_option("tvl1_async", 0)
    # container None puts the option back: the plain stream again
    again, _ = _run(rt, videos, steps, 12, None)
    assert rt.stream_container == 0 and all(torch.equal(g, w) for v in want for g, w in zip(again[v], want[v]))
    rt.set_option("tvl1_async", 0)
    # MIPI RAW10 / RAW14 need an even ww: 25 cells across
    odd = RvddRuntime("convunet", 0, 1, 36, 50, 0)
    for bits in (10, 14):
        frames = torch.zeros(36 * bits_ref.row_bytes(50, bits, "msb"), dtype=torch.uint8, device="cuda")
        with pytest.raises(RuntimeError, match=r"\(-1\).*ww"):
            odd.video_push(frames, [FIRST], bits, "mosaic", container="mipi")


# ---- 5. the command ----------------------------------------------------------------------------------------------------------------
def test_denoise_reads_and_writes_packed_frames(tmp_path):
    from rvdd_release_amd import denoise, synth, tiffio
    Hc, Wc, T, bits = 32, 48, 4, 12
    root = tmp_path / "data"
    for v in range(2):
        m = mosaic_of(quantised_dn(synth.make_sequence(T, Hc, Wc, iso=3200, seed=70 + v).raw)).astype(np.uint16)
        for folder in ("u16", "msb", "mipi"):
            os.makedirs(root / folder / ("%03d" % v))
        for t in range(T):
            stem = "%03d/%08d" % (v, 3 * t)
            tiffio.write(str(root / "u16" / (stem + ".tif")), m[t])
            tiffio.write_packed(str(root / "msb" / (stem + ".tif")), bits_ref.pack(m[t], bits, "msb"), Wc, bits)
            bits_ref.pack(m[t], bits, "mipi").tofile(str(root / "mipi" / (stem + ".raw")))
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, FEAT[0]), "--feature_rec",
             "--batch_size", "2", "--bit_depth", str(bits)]

    def run(name, dataroot, folder, *more):
        res = str(tmp_path / name)
        stats = denoise.main(flags + ["--dataroot", str(dataroot), "--nFolder", folder, "--results_dir", res] + list(more))
        return stats, files_of(res)

    stats, want = run("res_u16", root, "u16")
    assert stats["frames"] == 2 * (T - 1) == len(want) and all(k.endswith("_denoised.tif") for k in want)
    for folder, more in (("msb", ()), ("mipi", ("--raw_container", "mipi", "--raw_size", "%dx%d" % (Wc, Hc)))):
        stats, got = run("res_" + folder, root, folder, *more)
        assert stats["frames"] == len(want) and got == want, folder
    # packed out: the mosaic16 samples, bit-packed; the MSB tree is itself a tree the command reads, as long as it went in
    _, m16 = run("m16", root, "u16", "--out_format", "mosaic16", "--all_frames")
    _, msb = run("out_msb", root, "msb", "--out_format", "mosaic_msb", "--all_frames")
    _, mipi = run("out_mipi", root, "msb", "--out_format", "mosaic_mipi", "--all_frames")
    assert sorted(msb) == sorted(m16) and len(m16) == 2 * T and sorted(mipi) == sorted(k[:-4] + ".raw" for k in m16)
    for k in m16:
        u = tiffio.read(str(tmp_path / "m16" / k))[:, :, 0]
        rows, w, b = tiffio.read_packed(str(tmp_path / "out_msb" / k))
        assert (w, b) == (Wc, bits) and np.array_equal(rows, bits_ref.pack(u, bits, "msb")), k
        assert mipi[k[:-4] + ".raw"] == bits_ref.pack(u, bits, "mipi").tobytes(), k
    stats, again = run("again", tmp_path, "out_msb", "--out_format", "mosaic_msb", "--all_frames")
    assert stats["frames"] == 2 * T and sorted(again) == sorted(msb)
