"""Denoised frames out in sensor formats (rvdd_egress, RvddRuntime.egress, --out_format of the denoise command line), through the
C ABI: the kernel against its numpy restatement, against rvdd_gray_of_rgb, the round trip from sensor frames, the image the
command writes today, the wide form against the one-sample form, the argument checks, and the command on disk.  Every
comparison of samples is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import WEIGHTS
from egress_ref import LAYOUTS, PATTERNS, col, egress_ref, fill, special_values
from gpu_support import files_of, ops_rt as _rt, upload
from stream_ref import mosaic_of, quantised_dn, to_gpu

pytestmark = pytest.mark.gpu

U16 = getattr(torch, "uint16", torch.int16)
DTYPES = ((U16, np.uint16), (torch.float32, np.float32))


def _host(t):
    """A result tensor on the host: uint16 / float32 numpy."""
    if t.dtype == torch.float32:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _same(got, want):
    """Equal shapes, types and bits; a NaN equals a NaN."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _patterns(layout):
    return PATTERNS if layout != "rgb_hwc" else (None,)


# ---- 1. the kernel against its restatement ----------------------------------------------------------------------------------
# (2,2) one cell; (6,10) the one-cell form (W/2 no multiple of 4; 60 pixels: the wide RGB form in f32, the one-pixel form in
# u16); (16,32) the wide forms; (18,40) wide, a row count that is a multiple of nothing; (5,7) odd sizes, RGB only
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10), (16, 32), (18, 40), (5, 7)])
def test_egress_is_the_restatement(H, W):
    rt = _rt()
    for n in (1, 3):
        x = fill(n, H, W, seed=100 * H + W + n)
        dev = torch.from_numpy(x).cuda()
        assert dev.data_ptr() % 16 == 0
        for layout in LAYOUTS:
            if layout != "rgb_hwc" and (H % 2 or W % 2):
                continue
            for tdt, ndt in DTYPES:
                for pattern in _patterns(layout):
                    for bit_depth in (1, 8, 12, 16):
                        want = egress_ref(x, layout, ndt, bit_depth, pattern or "gbrg")
                        got = rt.egress(dev, layout, tdt, bit_depth, pattern)
                        assert got.dtype == tdt and _same(_host(got), want), (n, layout, ndt.__name__, pattern, bit_depth)


@pytest.mark.parametrize("n,H,W", [(3, 16, 32), (2, 22, 30)])
def test_every_tie_and_special_value_in_every_form(n, H, W):
    """All of egress_ref.special_values (the ends, the centre tie, NaN, the infinities, the 255 ties of 8 bits with their f32
    neighbours) in every plane, through the wide forms (16,32) and the one-sample forms (22,30: W/2 = 15; 660 pixels per image:
    the wide RGB form in f32, the one-pixel form in u16) and, from a source one float off a 16-byte boundary, the one-sample
    forms of everything."""
    rt = _rt()
    assert n * H * W >= special_values().size
    x = fill(n, H, W, seed=H)
    dev = torch.from_numpy(x).cuda()
    odd = upload(dev, offset=True)
    assert odd.data_ptr() % 16 == 4
    for layout in LAYOUTS:
        for tdt, ndt in DTYPES:
            for pattern in _patterns(layout):
                for bit_depth in (1, 8):
                    want = egress_ref(x, layout, ndt, bit_depth, pattern or "gbrg")
                    for src in (dev, odd):
                        assert _same(_host(rt.egress(src, layout, tdt, bit_depth, pattern)), want), (layout, ndt.__name__, pattern, bit_depth)
    # half to even at one bit: the centre of the range is the tie 0.5
    z = torch.zeros(1, 3, 2, 2, device="cuda")
    assert _host(rt.egress(z, "rgb_hwc", U16, 1)).max() == 0 and _host(rt.egress(z, "mosaic", U16, 12)).tolist() == [[[2048, 2048]] * 2]


# ---- 2. against rvdd_gray_of_rgb ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 32), (6, 10)])
def test_the_cells_of_the_f32_mosaic_sum_to_gray_of_rgb(H, W):
    rt = _rt()
    x = torch.from_numpy(np.random.default_rng(H).uniform(-1.25, 1.25, (3, 3, H, W)).astype(np.float32)).cuda()
    for pattern in PATTERNS:
        for bit_depth in (12, 16):
            gray = rt.gray_of_rgb(x, bit_depth, pattern).cpu().numpy()
            packed = _host(rt.egress(x, "packed_hwc", torch.float32, bit_depth, pattern))
            m = _host(rt.egress(x, "mosaic", torch.float32, bit_depth, pattern))
            cells = np.stack([m[:, (k >> 1)::2, (k & 1)::2] for k in range(4)], axis=-1)
            for c in (packed, cells):
                s = (((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]) * np.float32(0.25)
                assert s.dtype == np.float32 and np.array_equal(s.view(np.uint32), gray.view(np.uint32)), (pattern, bit_depth)


# ---- 3. the round trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 32), (6, 10)])
def test_sensor_frames_come_back(H, W):
    rt = _rt()
    rng = np.random.default_rng(W)
    for bit_depth in (12, 16):
        cells = rng.integers(0, 2 ** bit_depth, (3, H // 2, W // 2, 4), dtype=np.uint16)
        cells[0, 0, 0], cells[-1, -1, -1] = 0, 2 ** bit_depth - 1
        for layout, frames in (("mosaic", mosaic_of(cells)), ("packed_hwc", cells)):
            packed, _ = rt.ingest_raw(to_gpu(frames), bit_depth, layout, want_gray=False)
            for pattern in PATTERNS:
                back = rt.egress(rt.demosaic(packed, pattern), layout, U16, bit_depth, pattern)
                assert np.array_equal(_host(back), frames), (bit_depth, layout, pattern)


# ---- 4. the image validate / denoise write -------------------------------------------------------------------------------------
def test_rgb_f32_at_8_bits_is_tensor2im():
    from rvdd_release_amd.util import util
    rt = _rt()
    x = torch.from_numpy(np.random.default_rng(4).uniform(-1.25, 1.25, (3, 3, 18, 40)).astype(np.float32)).cuda()
    got = _host(rt.egress(x, "rgb_hwc", torch.float32, 8))
    for b in range(3):
        want = util.tensor2im(x[b:b + 1])
        assert want.dtype == np.float32 and np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), b


# ---- 5. the wide form is the one-sample form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_equals_narrow_and_nothing_else_is_written(layout):
    rt = _rt()
    n, H, W = 2, 16, 32
    x = torch.from_numpy(fill(n, H, W, seed=5)).cuda()
    x_odd = upload(x, offset=True)
    assert x.data_ptr() % 16 == 0 and x_odd.data_ptr() % 16 == 4
    for tdt, ndt in DTYPES:
        sentinel = 7.0 if tdt == torch.float32 else 0x5A5A
        for bit_depth in (8, 12):
            wide = rt.egress(x, layout, tdt, bit_depth, "grbg")
            assert wide.data_ptr() % 16 == 0
            want = _host(wide)
            assert _same(want, egress_ref(x.cpu().numpy(), layout, ndt, bit_depth, "grbg"))
            store = wide.view(torch.int16) if tdt != torch.float32 else wide          # (fills and copies of 16-bit words)
            for src in (x, x_odd):
                # into a 16-byte aligned tensor (wide only with the aligned source) and into one that starts one element in
                for out, whole in ((torch.full_like(store, sentinel), None), upload(torch.full_like(store, sentinel), offset=store.element_size(), fill=sentinel)):
                    assert (out.data_ptr() % 16 == 0) == (whole is None)
                    got = rt.egress(src, layout, tdt, bit_depth, "grbg", out=out.view(tdt))
                    assert got.data_ptr() == out.data_ptr() and _same(_host(got), want), (ndt.__name__, bit_depth, whole is None)
                    if whole is not None:
                        torch.cuda.synchronize()
                        outside = torch.cat([whole[:1], whole[1 + out.numel():]])
                        assert bool((outside == sentinel).all()), (ndt.__name__, bit_depth)


def test_pattern_defaults_to_the_handles_and_out_is_checked():
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime("convunet", 0, 1, 64, 96, 0)
    x = torch.rand(2, 3, 6, 10, device="cuda") * 2 - 1
    same = lambda a, b: np.array_equal(_host(a), _host(b))
    assert same(rt.egress(x, "mosaic"), rt.egress(x, "mosaic", U16, 12, "gbrg"))
    rt.set_option("bayer_pattern", 2)
    assert same(rt.egress(x, "mosaic"), rt.egress(x, "mosaic", U16, 12, "rggb")) and not same(rt.egress(x, "mosaic"), rt.egress(x, "mosaic", U16, 12, "gbrg"))
    assert same(rt.egress(x, "rgb_hwc", torch.int16), rt.egress(x, "rgb_hwc", U16))
    with pytest.raises(ValueError, match="pattern"):
        rt.egress(x, "mosaic", pattern="xtrans")
    with pytest.raises(ValueError, match="layout"):
        rt.egress(x, "chw")
    with pytest.raises(RuntimeError, match="dtype"):
        rt.egress(x, "mosaic", torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.egress(x.cpu())
    with pytest.raises(RuntimeError, match=r"\[n,3,H,W\]"):
        rt.egress(x[:, :2])
    with pytest.raises(RuntimeError, match="out must be"):
        rt.egress(x, "mosaic", torch.float32, out=torch.empty(2, 6, 10, 1, device="cuda"))
    with pytest.raises(RuntimeError, match="out must be"):
        rt.egress(x, "mosaic", torch.float32, out=torch.empty(2, 6, 10, dtype=torch.int16, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.egress(x, "mosaic", torch.float32, out=torch.empty(2, 6, 10))
    with pytest.raises(RuntimeError, match=r"\(-1\).*bit_depth"):
        rt.egress(x, "mosaic", bit_depth=0)
    with pytest.raises(RuntimeError, match=r"\(-1\).* W "):
        rt.egress(x[..., :9], "packed_hwc")


# ---- 6. the argument checks -----------------------------------------------------------------------------------------------------
def test_egress_bad_arguments():
    rt = _rt()
    x = torch.zeros(1, 3, 32, 32, device="cuda")
    out = torch.full((1, 32, 32, 3), 7.0, device="cuda")

    def call(n=1, H=32, W=32, layout=1, dtype=1, bit_depth=12, pattern=0, rgb=x.data_ptr(), o=out.data_ptr()):
        rc = rt.lib.rvdd_egress(rt.h, rgb, n, H, W, layout, dtype, bit_depth, pattern, o, None)
        return rc, rt.lib.rvdd_last_error(rt.h)

    bad = [({"layout": -1}, b"layout"), ({"layout": 3}, b"layout"), ({"dtype": -1}, b"dtype"), ({"dtype": 2}, b"dtype"),
           ({"bit_depth": 0}, b"bit_depth"), ({"bit_depth": 17}, b"bit_depth"),
           ({"pattern": -1}, b"pattern"), ({"pattern": 4}, b"pattern"), ({"pattern": 4, "layout": 2}, b"pattern"),
           ({"H": 0}, b" H "), ({"W": 0}, b" W "), ({"H": 0, "layout": 0}, b" H "), ({"W": -2, "layout": 0}, b" W "),
           ({"H": 31}, b" H "), ({"W": 31}, b" W "), ({"H": 31, "layout": 2}, b" H "), ({"W": 31, "layout": 2}, b" W "),
           ({"n": -1}, b" n "), ({"rgb": None}, b"rgb"), ({"o": None}, b"out"),
           # 2^24 images of 2^12 x 2^12: 2^44 threads of four cells, 2^36 blocks (nothing is launched, nothing is read)
           ({"n": 1 << 24, "H": 1 << 12, "W": 1 << 12}, b"blocks"), ({"n": (1 << 31) - 1, "H": (1 << 31) - 1, "W": (1 << 31) - 1, "layout": 0}, b"blocks")]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b"rvdd_egress:") and word in msg, (kw, msg)
    assert call(n=0)[0] == 0 and call(n=0, rgb=None, o=None)[0] == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                       # none of these wrote anything
    # RGB_HWC ignores the pattern and takes odd sizes
    assert call(layout=0, pattern=9, H=31, W=31)[0] == 0
    torch.cuda.synchronize()
    assert bool((out.reshape(-1)[:31 * 31 * 3] == 2047.5).all()) and bool((out.reshape(-1)[31 * 31 * 3:] == 7.0).all())


# ---- 7. the command ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
def test_denoise_main_writes_sensor_formats(tmp_path, future):
    from rvdd_release_amd import denoise, synth, tiffio
    from rvdd_release_amd.library import iio_read
    H, W, T, bit_depth = 32, 48, 4, 12
    top = 2 ** bit_depth - 1
    iso = 12800 if future else 3200
    name = "recurrent-convunet+feat-future-iso12800" if future else "recurrent-convunet+feat-iso3200"
    root = tmp_path / "data"
    for v in range(3):
        cells = quantised_dn(synth.make_sequence(T, H, W, iso=iso, seed=60 + v).raw)
        os.makedirs(root / "noisy" / ("%03d" % v))
        for t in range(T):
            tiffio.write(str(root / "noisy" / ("%03d" % v) / ("%08d.tiff" % (3 * t))), mosaic_of(cells[t:t + 1])[0].astype(np.uint16))
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, name), "--feature_rec",
             "--future_patch_depth", str(future), "--batch_size", "2"]

    def run(fmt, dataroot=str(root), folder="noisy", extra=()):
        res = tmp_path / ("res_" + fmt + "_" + folder)
        stats = denoise.main(flags + ["--dataroot", dataroot, "--nFolder", folder, "--results_dir", str(res), "--out_format", fmt] + list(extra))
        return res, files_of(str(res)), stats

    res32, f32, stats = run("f32")
    stems = sorted(k[:-len("_denoised.tif")] for k in f32)
    assert len(stems) == 3 * (T - 1 - future) == stats["frames"] and all(k.endswith("_denoised.tif") for k in f32)
    shapes = {"rgb16": (H, W, 3), "mosaic16": (H, W), "packed16": (H // 2, W // 2, 4)}
    window = 4 * 2.0 ** -24 * top              # the two f32 roundings on each side of the comparison, in DN
    for fmt in ("mosaic16", "packed16", "rgb16"):
        res, files, stats = run(fmt, extra=["--srgb", "%d,1.3,1.9,1.5" % iso] if fmt == "rgb16" else [])
        assert sorted(k for k in files if not k.endswith("_srgb.png")) == [s + ".tif" for s in stems], fmt
        assert stats["frames"] == len(stems)
        if fmt == "rgb16":
            assert sorted(k for k in files if k.endswith("_srgb.png")) == [s + "_srgb.png" for s in stems]
        for s in stems:
            got = iio_read(str(res / (s + ".tif")))
            got = got[:, :, 0] if got.ndim == 3 and got.shape[2] == 1 else got
            assert got.dtype == np.uint16 and got.shape == shapes[fmt], (fmt, s, got.dtype, got.shape)
            rec = iio_read(str(res32 / (s + "_denoised.tif"))).astype(np.float64) / 255.0 * top          # [H,W,3]
            if fmt != "rgb16":
                cells = np.stack([rec[(k >> 1)::2, (k & 1)::2, col("gbrg", k)] for k in range(4)], axis=-1)
                rec = cells if fmt == "packed16" else mosaic_of(cells[None])[0]
            want = np.clip(np.rint(rec), 0, top)
            diff = np.abs(got.astype(np.float64) - want)
            near_tie = np.abs(np.abs(rec - np.floor(rec)) - 0.5) <= window
            print(f"{fmt} {s}: {int((diff != 0).sum())} of {diff.size} samples differ from rint of the f32 image, {int(near_tie.sum())} near a tie")
            assert diff.max() <= 1 and not np.any((diff == 1) & ~near_tie), (fmt, s)
    # the packed results are a dataset the command reads back: 3 videos of T - 1 - future frames each
    res_p = tmp_path / "res_packed16_noisy"
    again, files, stats = run("f32", dataroot=str(tmp_path), folder=res_p.name)
    assert len(files) == stats["frames"] == 3 * max(0, (T - 1 - future) - 1 - future)
