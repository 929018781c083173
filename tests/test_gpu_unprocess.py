"""rvdd_unprocess / rvdd_unprocess_draws on the device: against fixtures written by the reference's own program with its own
dither and normals supplied (the bounds of tests/test_unprocess_host.py), the other Bayer patterns against the restatement, the
draws against the numpy Philox restatement, the contract of include/rvdd.h (fused = supplied planes, n frames = n calls, NULL
outputs, argument errors), and the command line on disk -- its tree into `denoise` and `ppipe.main`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import unprocess_ref as U
from conftest import GOLDEN, WEIGHTS
from gpu_support import files_of, ops_rt

pytestmark = pytest.mark.gpu

ISOS = (3200, 12800)
TAGS = ("odd", "wide")                       # 17 x 23 cells: one cell per thread; 16 x 32 cells: the wide form
OUTPUTS = ("lin_f32", "lin_u16", "gt_raw", "noisy")


@pytest.fixture(scope="module")
def rt():
    return ops_rt()


@pytest.fixture(scope="module")
def golden():
    return {iso: dict(np.load(os.path.join(GOLDEN, f"unprocess_iso{iso}.npz"))) for iso in ISOS}


def _frames(g, tag, s):
    x = g[f"in_{tag}"][s]
    H, W = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    return torch.from_numpy(np.ascontiguousarray(x[:, :H, :W])).cuda()


def _np(t):
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int16) if a[k].dtype == torch.uint16 else a[k],
                           b[k].view(torch.int16) if b[k].dtype == torch.uint16 else b[k]) for k in a) and set(a) == set(b)


def _random_srgb(n, H, W, seed):
    x = np.random.default_rng(seed).integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    x[:, :2] = 0
    x[:, 2:4] = 255
    return torch.from_numpy(x).cuda()


@pytest.mark.parametrize("iso", ISOS)
@pytest.mark.parametrize("tag", TAGS)
def test_fixtures_with_the_reference_draws(rt, golden, iso, tag):
    g = golden[iso]
    for s in range(2):
        n, red, blue = (float(v) for v in g[f"gains_{tag}"][s])
        out = rt.unprocess(_frames(g, tag, s), 1 / n, red, blue, iso, dither=torch.from_numpy(g[f"dither_{tag}"][s]).cuda(),
                           normal=torch.from_numpy(g[f"normal_{tag}"][s]).cuda())
        assert out["lin_u16"].dtype == torch.uint16 and out["noisy"].dtype == torch.float32
        for k in ("lin_f32", "gt_raw", "noisy"):
            assert tuple(out[k].shape) == g[f"{k}_{tag}"][s].shape
            U.assert_close_dn(_np(out[k]), g[f"{k}_{tag}"][s], f"iso{iso} {tag} seq{s} {k}")
        U.assert_integers_agree(_np(out["lin_u16"]), g[f"lin_u16_{tag}"][s], f"iso{iso} {tag} seq{s} lin_u16")
        rgb = rt.ppipe(out["lin_f32"], 1 / n, red, blue, iso, 12, "hwc")
        U.assert_integers_agree(_np(rgb), g[f"gt_rgb_{tag}"][s], f"iso{iso} {tag} seq{s} gt_rgb")
        # the mosaic and the rounding are exact functions of lin_f32
        lin = _np(out["lin_f32"])
        assert np.array_equal(_np(out["gt_raw"]), U.mosaic(lin)) and np.array_equal(_np(out["lin_u16"]), np.clip(np.rint(lin), 0, 4095))


@pytest.mark.parametrize("pattern", ["grbg", "rggb", "bggr"])
@pytest.mark.parametrize("tag", TAGS)
def test_other_patterns_against_the_restatement(rt, golden, pattern, tag):
    g = golden[12800]
    n, red, blue = (float(v) for v in g[f"gains_{tag}"][1])
    d, z = g[f"dither_{tag}"][1], g[f"normal_{tag}"][1]
    srgb = _frames(g, tag, 1)
    out = rt.unprocess(srgb, 1 / n, red, blue, 12800, pattern=pattern, dither=torch.from_numpy(d).cuda(), normal=torch.from_numpy(z).cuda())
    want = U.chain(_np(srgb), d, z, 1 / n, red, blue, 12800, pattern)
    for k in ("lin_f32", "gt_raw", "noisy"):
        U.assert_close_dn(_np(out[k]), want[k], f"{pattern} {tag} {k}")
    U.assert_integers_agree(_np(out["lin_u16"]), want["lin_u16"], f"{pattern} {tag} lin_u16")
    assert np.array_equal(_np(out["gt_raw"]), U.mosaic(_np(out["lin_f32"]), pattern))
    gbrg = rt.unprocess(srgb, 1 / n, red, blue, 12800, dither=torch.from_numpy(d).cuda(), normal=torch.from_numpy(z).cuda())
    assert torch.equal(gbrg["lin_f32"], out["lin_f32"]) and not torch.equal(gbrg["gt_raw"], out["gt_raw"])


@pytest.mark.parametrize("H,W", [(34, 46), (32, 64)])
def test_draws_are_the_philox_restatement(rt, H, W):
    seed, frame0, n = 0x123456789ABCDEF, (1 << 32) - 1, 2                  # the frame index crosses 2^32 inside the call
    d, z = rt.unprocess_draws(seed, frame0, n, H, W)
    assert d.shape == (n, H, W, 3) and z.shape == (n, H // 2, W // 2, 4)
    for i in range(n):
        assert torch.equal(d[i].cpu(), torch.from_numpy(U.dither_plane(seed, frame0 + i, H, W))), i
        want = U.normal_plane(seed, frame0 + i, H, W)
        err = np.abs(_np(z[i]).astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
        print(f"normals {H}x{W} frame {i}: max error {err.max():.3e} relative to max(|z|, 1)")
        assert err.max() <= 4e-6
    d2, z2 = rt.unprocess_draws(seed, frame0, n, H, W)
    assert torch.equal(d, d2) and torch.equal(z, z2)                        # run to run
    for other in ((seed + 1, frame0), (seed ^ (1 << 40), frame0), (seed, frame0 + 7)):
        d3, z3 = rt.unprocess_draws(other[0], other[1], n, H, W)
        assert not torch.equal(d, d3) and not torch.equal(z, z3), other
    only_d, none = rt.unprocess_draws(seed, frame0, n, H, W, want_normal=False)
    assert none is None and torch.equal(only_d, d)
    none, only_z = rt.unprocess_draws(seed, frame0, n, H, W, want_dither=False)
    assert none is None and torch.equal(only_z, z)


@pytest.mark.parametrize("H,W", [(34, 46), (32, 64), (66, 136)])          # (66, 136): the wide form over more than one block
def test_fused_draws_batching_and_null_outputs(rt, H, W):
    n, seed, frame0 = 3, 99, 41
    srgb = _random_srgb(n, H, W, seed=H)
    gains = (1 / 0.7644, 1.9503, 3.5006)
    fused = rt.unprocess(srgb, *gains, 3200, seed=seed, frame0=frame0)
    d, z = rt.unprocess_draws(seed, frame0, n, H, W)
    assert _same(fused, rt.unprocess(srgb, *gains, 3200, dither=d, normal=z))
    # one plane supplied, the other drawn
    assert _same(fused, rt.unprocess(srgb, *gains, 3200, dither=d, seed=seed, frame0=frame0))
    assert _same(fused, rt.unprocess(srgb, *gains, 3200, normal=z, seed=seed, frame0=frame0))
    # n frames = n calls of one frame at frame0 + i
    for i in range(n):
        one = rt.unprocess(srgb[i:i + 1], *gains, 3200, seed=seed, frame0=frame0 + i)
        assert _same({k: v[i:i + 1] for k, v in fused.items()}, one), i
    assert not torch.equal(fused["noisy"], rt.unprocess(srgb, *gains, 3200, seed=seed + 1, frame0=frame0)["noisy"])
    # an unaligned base (the narrow form on a wide shape): the same bits
    flat = torch.empty(srgb.numel() + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = srgb.reshape(-1)
    assert _same(fused, rt.unprocess(flat[1:].view(n, H, W, 3), *gains, 3200, seed=seed, frame0=frame0))
    # every output NULL in turn (and alone): the others unchanged
    for k in OUTPUTS:
        rest = tuple(o for o in OUTPUTS if o != k)
        assert _same({o: fused[o] for o in rest}, rt.unprocess(srgb, *gains, 3200, seed=seed, frame0=frame0, want=rest)), k
        assert _same({k: fused[k]}, rt.unprocess(srgb, *gains, 3200, seed=seed, frame0=frame0, want=(k,))), k
    assert rt.unprocess(srgb, *gains, 3200, want=()) == {}
    # the noise model, read backwards: (noisy - m) / sqrt(ka m - kb) is the normal plane.  The variance is positive on every
    # value the chain can produce (m >= 257.88 gives 20.4 DN^2 at ISO 3200).  noisy is rounded to f32 -- half an ulp, at most
    # 2^-12 DN below 8192 -- over a sigma of at least 4.5 DN; sigma itself is good to 4e-6 relative and |z| <= 5.77
    m, nz = fused["gt_raw"].double(), fused["noisy"].double()
    var = 8.0034 * m - 2043.51144
    assert var.min() > 20 and nz.abs().max() < 8192
    assert ((nz - m) / var.sqrt() - z.double()).abs().max() <= 2.0 ** -12 / 4.5 + 4e-6 * 5.77


def test_argument_errors(rt):
    lib, h = rt.lib, rt.h
    buf = torch.zeros(4 * 4 * 3 * 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4 * 4 * 3, dtype=torch.float32, device="cuda")

    def call(n=1, H=4, W=4, gains=(1.3, 1.9, 1.5), iso=3200, pattern=0, srgb=buf.data_ptr()):
        return lib.rvdd_unprocess(h, srgb, n, H, W, *gains, iso, pattern, None, None, 0, 0, out.data_ptr(), None, None, None, None)

    assert call() == 0
    for kw, word in ((dict(iso=1600), "iso"), (dict(pattern=4), "pattern"), (dict(pattern=-1), "pattern"), (dict(H=5), "H must be even"),
                     (dict(W=3), "W must be even"), (dict(H=0), "H must be even"), (dict(H=1 << 17, W=1 << 15), "2^32"), (dict(n=-1), "n must be"),
                     (dict(srgb=None), "srgb"), (dict(gains=(0.0, 1.9, 1.5)), "gain")):
        assert call(**kw) == -1, kw                                      # RVDD_ERR_ARG
        assert word in lib.rvdd_last_error(h).decode(), (kw, lib.rvdd_last_error(h))
    assert call(n=0, srgb=None) == 0                                     # n = 0 does nothing
    assert lib.rvdd_unprocess_draws(h, 1, 0, 1, 4, 6, None, None, None) == 0
    for args, word in (((1, 0, 1, 5, 6), "H must be even"), ((1, 0, 1, 4, 7), "W must be even"), ((1, 0, -2, 4, 6), "n must be"),
                       ((1, 0, 1, 1 << 16, 1 << 16), "2^32")):
        assert lib.rvdd_unprocess_draws(h, *args, None, None, None) == -1, args
        assert word in lib.rvdd_last_error(h).decode() and "rvdd_unprocess_draws" in lib.rvdd_last_error(h).decode()
    assert lib.rvdd_unprocess(None, buf.data_ptr(), 1, 4, 4, 1.3, 1.9, 1.5, 3200, 0, None, None, 0, 0, None, None, None, None, None) == -1
    # the Python wrapper's own checks
    x = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.unprocess(x.cpu(), 1.3, 1.9, 1.5, 3200)
    with pytest.raises(RuntimeError, match="uint8"):
        rt.unprocess(x.float(), 1.3, 1.9, 1.5, 3200)
    with pytest.raises(RuntimeError, match="even"):
        rt.unprocess(x[:, :3], 1.3, 1.9, 1.5, 3200)
    with pytest.raises(RuntimeError, match="dither has shape"):
        rt.unprocess(x, 1.3, 1.9, 1.5, 3200, dither=torch.zeros(1, 4, 4, 4, device="cuda"))
    with pytest.raises(ValueError, match="pattern"):
        rt.unprocess(x, 1.3, 1.9, 1.5, 3200, pattern="xtrans")
    with pytest.raises(RuntimeError, match="iso must be"):
        rt.unprocess(x, 1.3, 1.9, 1.5, 100)


# ---- on disk ------------------------------------------------------------------------------------------------------------------
def test_main_on_disk_feeds_denoise_and_ppipe(rt, tmp_path):
    from PIL import Image
    from rvdd_release_amd import denoise, ppipe, tiffio, unprocess
    from rvdd_release_amd.library import iio_read
    # smooth moving clips of 36 x 48 (TV-L1 takes 18 x 24 cells), two sequences x three frames
    yy, xx = np.mgrid[0:36, 0:48]
    for s in range(2):
        os.makedirs(tmp_path / "clips" / ("%03d" % s))
        for i in range(3):
            img = np.stack([127 + 100 * np.sin((xx + 2 * i + 5 * s) / 7.0), 127 + 100 * np.cos((yy - i) / 5.0), (3 * xx + 2 * yy + 9 * i) % 256], -1)
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(tmp_path / "clips" / ("%03d" % s) / ("%08d.png" % i))
    trees = {}
    for batch in (1, 3):
        out = tmp_path / f"data{batch}"
        n = unprocess.main(["--input_val_dataset", str(tmp_path / "clips" / "%03d" / "%08d.png"), "--output_val_dataset", str(out),
                            "--nb_seq_val", "2", "--nb_seq_train", "0", "--ISO", "3200", "--first", "0", "--last", "2", "--seed", "3",
                            "--batch", str(batch)])
        assert n == {"train": 0, "val": 6}
        trees[batch] = files_of(str(out))
    assert set(trees[1]) == {f"{folder}_iso3200/{s:03d}/{i:08d}.{'png' if folder == 'gt_RGB' else 'tiff'}"
                             for folder in ("gt", "gt_raw_linear_RGB", "noisy", "gt_RGB") for s in range(2) for i in range(3)}
    assert trees[1] == trees[3]                                          # byte for byte, whatever --batch is
    root = tmp_path / "data3"
    for s in range(2):
        n_gain, red, blue = ppipe.find_gains(s, 3200)
        srgb = torch.from_numpy(np.stack([iio_read(str(tmp_path / "clips" / ("%03d" % s) / ("%08d.png" % i))) for i in range(3)])).cuda()
        want = rt.unprocess(srgb, 1 / n_gain, red, blue, 3200, seed=unprocess.sequence_seed(3, "val", s), frame0=0)
        for i in range(3):
            gt = tiffio.read(str(root / f"gt_iso3200/{s:03d}/{i:08d}.tiff"))
            nz = tiffio.read(str(root / f"noisy_iso3200/{s:03d}/{i:08d}.tiff"))
            u16 = tiffio.read(str(root / f"gt_raw_linear_RGB_iso3200/{s:03d}/{i:08d}.tiff"))
            png = iio_read(str(root / f"gt_RGB_iso3200/{s:03d}/{i:08d}.png"))
            assert gt.dtype == np.float32 and gt.shape == (18, 24, 4) and nz.dtype == np.float32 and nz.shape == (18, 24, 4)
            assert u16.dtype == np.uint16 and u16.shape == (36, 48, 3) and png.dtype == np.uint8 and png.shape == (36, 48, 3)
            assert np.array_equal(gt, _np(want["gt_raw"][i])) and np.array_equal(nz, _np(want["noisy"][i]))
            assert np.array_equal(u16, _np(want["lin_u16"][i]))
            # gt_RGB is ppipe of the linear image
            assert np.array_equal(png, _np(rt.ppipe(want["lin_f32"][i:i + 1], 1 / n_gain, red, blue, 3200, 12, "hwc"))[0])
    # the noisy tree through the denoiser (the flags of tests/test_gpu_stream.py's command-line test), its output through
    # ppipe.main against the generated gt_RGB
    res = tmp_path / "res"
    stats = denoise.main(["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, "recurrent-convunet+feat-iso3200"),
                          "--feature_rec", "--future_patch_depth", "0", "--dataroot", str(root), "--nFolder", "noisy_iso3200",
                          "--results_dir", str(res), "--batch_size", "2"])
    assert stats["frames"] == 4
    psnr, ssim = ppipe.main(["--validation_path", str(root), "--result_folder", str(res), "--videos", "0,1", "--first", "1", "--last", "2",
                             "--step", "1", "--bit_depth", "8", "--ISO", "3200"])
    print(f"denoised against the generated gt_RGB: PSNR {psnr:.2f} dB, SSIM {ssim:.3f}")
    assert np.isfinite(psnr) and psnr > 20 and 0 < ssim <= 1                # the frames belong to each other
