"""Raw-dataset synthesis, the part that needs no GPU: the numpy restatement of rvdd_unprocess (tests/unprocess_ref.py) against
fixtures written by the reference's own program (tools/make_golden_unprocess.py), Philox against its known answers, the
statistics of the restated draws, the fixture recipe, and the host logic of `python -m rvdd_release_amd.unprocess` on a stub
runtime that computes with the restatement.

Measured when the fixtures were made (34 x 46 frames): the reference sits 1.2e-3 .. 1.5e-3 DN (3.2e-7 relative) from the float64
chain, a float32 restatement at most 2.0e-3 DN from the reference; the bound below is 4e-6 * max(|value|, 255) = 1.6e-2 DN at
full scale.  One DN is 2.4e-4 relative."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppipe_oracle as P
import unprocess_ref as U
from conftest import GOLDEN, REPO

ISOS = (3200, 12800)
TAGS = ("odd", "wide")


@pytest.fixture(scope="module")
def golden():
    return {iso: dict(np.load(os.path.join(GOLDEN, f"unprocess_iso{iso}.npz"))) for iso in ISOS}


def cropped(x):
    H, W = x.shape[-3] // 2 * 2, x.shape[-2] // 2 * 2
    return np.ascontiguousarray(x[..., :H, :W, :])


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        assert " ".join("%08x" % int(w) for w in U.philox4x32_10(counter, key)) == want
    # vectorised: element e of an array call is the scalar call
    w = U.philox4x32_10([np.arange(5), np.full(5, 1), np.full(5, 7), np.zeros(5)], (2023, 0))
    one = U.philox4x32_10([3, 1, 7, 0], (2023, 0))
    assert [int(x[3]) for x in w] == [int(x) for x in one]


def test_fixtures_hold_the_sizes_and_hit_the_clamps(golden):
    for iso in ISOS:
        g = golden[iso]
        assert g["in_odd"].shape == (2, 2, 35, 47, 3) and g["in_wide"].shape == (2, 2, 32, 64, 3) and g["in_odd"].dtype == np.uint8
        assert g["gt_raw_odd"].shape == (2, 2, 17, 23, 4) and g["gt_raw_wide"].shape == (2, 2, 16, 32, 4)
        for tag in TAGS:
            assert (g[f"in_{tag}"][:, :, :3] == 0).all() and (g[f"in_{tag}"][:, :, 3:6] == 255).all()
            lin = g[f"lin_f32_{tag}"]
            A, B = U.AFFINE[iso]
            # the rows of 0 sit on the lower clamps (v < 0 under a negative dither, y = 0: DN 240 before the affine map); the rows
            # of 255 pass the uint16 clip (with this gain table y stays below 1: the upper clamp of y is not reachable from 8 bits)
            assert abs(lin.min() - (A * (240 - 245) / 2060 + B)) < 1e-3 and (lin[:, :, :3] == lin.min()).mean() > 0.05
            assert lin.max() > 4095.5 and g[f"lin_u16_{tag}"].max() == 4095


@pytest.mark.parametrize("iso", ISOS)
@pytest.mark.parametrize("tag", TAGS)
def test_f32_restatement_is_the_reference(golden, iso, tag):
    g = golden[iso]
    srgb = cropped(g[f"in_{tag}"])
    for s in range(2):
        n, red, blue = (float(v) for v in g[f"gains_{tag}"][s])
        got = U.chain(srgb[s], g[f"dither_{tag}"][s], g[f"normal_{tag}"][s], 1 / n, red, blue, iso)
        for k in ("lin_f32", "gt_raw", "noisy"):
            assert got[k].dtype == np.float32 and got[k].shape == g[f"{k}_{tag}"][s].shape
            U.assert_close_dn(got[k], g[f"{k}_{tag}"][s], f"iso{iso} {tag} seq{s} {k}")
        U.assert_integers_agree(got["lin_u16"], g[f"lin_u16_{tag}"][s], f"iso{iso} {tag} seq{s} lin_u16")
        rgb = np.stack([P.to_uint8(P.ppipe(x, 1 / n, red, blue, iso)) for x in got["lin_f32"]])
        U.assert_integers_agree(rgb, g[f"gt_rgb_{tag}"][s], f"iso{iso} {tag} seq{s} gt_rgb")


def test_reference_is_as_close_to_the_f64_chain(golden):
    """The yardstick behind the bound: the reference's own distance from the same chain in float64."""
    for iso in ISOS:
        g = golden[iso]
        n, red, blue = (float(v) for v in g["gains_odd"][0])
        want = U.chain(cropped(g["in_odd"])[0], g["dither_odd"][0], g["normal_odd"][0], 1 / n, red, blue, iso, T=np.float64)
        for k in ("lin_f32", "gt_raw", "noisy"):
            U.assert_close_dn(g[f"{k}_odd"][0], want[k], f"reference vs f64, iso{iso} {k}")


def test_patterns_move_colours_not_values(golden):
    g = golden[3200]
    lin = g["lin_f32_odd"][0, 0]
    m = {p: U.mosaic(lin, p) for p in U.PATTERNS}
    assert np.array_equal(m["gbrg"], g["gt_raw_odd"][0, 0])                  # the reference's mosaic() of its own linear image
    # GBRG: G B / R G (the reference's mosaic()); RGGB: R G / G B
    assert np.array_equal(m["gbrg"][..., 1], lin[0::2, 1::2, 2]) and np.array_equal(m["gbrg"][..., 2], lin[1::2, 0::2, 0])
    assert np.array_equal(m["rggb"][..., 0], lin[0::2, 0::2, 0]) and np.array_equal(m["rggb"][..., 3], lin[1::2, 1::2, 2])
    assert np.array_equal(m["grbg"][..., 1], lin[0::2, 1::2, 0]) and np.array_equal(m["bggr"][..., 0], lin[0::2, 0::2, 2])


def test_draw_statistics():
    """64 x 64 cells at a fixed seed: N = 16 384 normals, |mean| <= 4 / sqrt(N), |var - 1| <= 4 sqrt(2 / N); the dither's mean
    under the same limit scaled by its sigma, its variance near 1/12; the tail ends at 5.77 sigma."""
    H = W = 128
    z = U.normal_plane(2023, 5, H, W).ravel()
    N = z.size
    assert N == 16384
    print("normals: mean", z.mean(), "var", z.var(), "max", np.abs(z).max())
    assert abs(z.mean()) <= 4 / np.sqrt(N) and abs(z.var() - 1) <= 4 * np.sqrt(2 / N)
    assert np.abs(z).max() <= np.sqrt(48 * np.log(2)) + 1e-12
    d = U.dither_plane(2023, 5, H, W).astype(np.float64).ravel()
    print("dither: mean", d.mean(), "var", d.var())
    assert d.min() >= -0.5 and d.max() < 0.5
    assert abs(d.mean()) <= 4 * np.sqrt(1 / 12 / d.size)
    assert abs(d.var() - 1 / 12) <= 4 * np.sqrt(1 / 180 / d.size)           # var of x^2 for a uniform of width 1 is 1/180
    # another seed or frame: other planes; the same pair: the same planes
    assert np.array_equal(U.dither_plane(2023, 5, 8, 8), U.dither_plane(2023, 5, 8, 8))
    assert not np.array_equal(U.dither_plane(2023, 5, 8, 8), U.dither_plane(2024, 5, 8, 8))
    assert not np.array_equal(U.normal_plane(2023, 5, 8, 8), U.normal_plane(2023, 6, 8, 8))
    assert not np.array_equal(U.normal_plane(2023, 5, 8, 8), U.normal_plane(2023 + 2 ** 32, 5, 8, 8))


@pytest.mark.skipif(not os.path.isfile("/root/reference/dataset/generate_raw_from_RGB.py"), reason="reference tree not present")
def test_make_golden_unprocess_regenerates(tmp_path):
    e = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_golden_unprocess.py"), "--out", str(tmp_path)], cwd=REPO, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(str(tmp_path), "*.npz")))
    assert names == ["unprocess_iso12800.npz", "unprocess_iso3200.npz"]
    for f in names:
        a, b = np.load(os.path.join(str(tmp_path), f)), np.load(os.path.join(GOLDEN, f))
        assert set(a.files) == set(b.files), f
        for k in a.files:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (f, k)
            if not np.array_equal(a[k], b[k]):                              # another host's libm: the last bit of a float
                assert a[k].dtype.kind == "f" and np.abs(a[k].astype(np.float64) - b[k]).max() < 4e-6 * 4095, (f, k)


# ---- the command line on a stub runtime -------------------------------------------------------------------------------------
class StubRuntime:
    """What unprocess.main needs of a runtime, computed by the restatement on the CPU; records its calls."""
    _tdev = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def unprocess(self, srgb, rgb_gain, red_gain, blue_gain, iso, pattern="gbrg", dither=None, normal=None, seed=0, frame0=0, want=()):
        self.calls.append(dict(n=srgb.shape[0], seed=seed, frame0=frame0, pattern=pattern, gains=(rgb_gain, red_gain, blue_gain), iso=iso))
        out = U.unprocess(srgb.numpy(), rgb_gain, red_gain, blue_gain, iso, seed, frame0, pattern)
        return {k: torch.from_numpy(np.ascontiguousarray(out[k])) for k in want}

    def ppipe(self, img, rgb_gain, red_gain, blue_gain, iso, bit_depth, layout="nchw", want_float=False):
        assert bit_depth == 12 and layout == "hwc"
        return torch.from_numpy(np.stack([P.to_uint8(P.ppipe(x.numpy(), rgb_gain, red_gain, blue_gain, iso)) for x in img]))


def _write_clips(root, nseq, indices, H, W, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for s in range(nseq):
        os.makedirs(os.path.join(root, "%03d" % s))
        for i in indices:
            Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(root, "%03d" % s, "%08d.png" % i))
    return os.path.join(root, "%03d", "%08d.png")


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_sequence_seed_and_batches():
    from rvdd_release_amd import unprocess as M
    seeds = {M.sequence_seed(sd, split, q) for sd in (0, 1, 2 ** 40) for split in M.SPLITS for q in range(4)}
    assert len(seeds) == 24 and all(0 <= s < 2 ** 64 for s in seeds)
    assert M.sequence_seed(7, "val", 3) == M.sequence_seed(7, "val", 3)
    assert list(M._batches([0, 1, 2, 3, 4], 2)) == [[0, 1], [2, 3], [4]]
    assert list(M._batches([0, 2, 4], 8)) == [[0], [2], [4]]                 # image i of a call is frame frame0 + i
    assert list(M._batches([3, 4, 5, 9, 10], 8)) == [[3, 4, 5], [9, 10]]
    with pytest.raises(RuntimeError, match="8-bit"):
        M.crop_even(np.zeros((4, 4, 3), np.uint16))
    assert M.crop_even(np.zeros((5, 7, 4), np.uint8)).shape == (4, 6, 3)


def test_main_writes_the_reference_tree_whatever_the_batch(tmp_path):
    from rvdd_release_amd import tiffio, unprocess as M
    from rvdd_release_amd.library import iio_read
    from rvdd_release_amd.ppipe import find_gains
    val = _write_clips(str(tmp_path / "val_in"), 2, range(1, 4), 13, 18, seed=1)       # cropped to 12 x 18
    train = _write_clips(str(tmp_path / "train_in"), 1, range(1, 4), 8, 10, seed=2)
    trees, stubs = {}, {}
    for batch in (1, 3):
        out = tmp_path / f"out{batch}"
        stubs[batch] = StubRuntime()
        n = M.main(["--input_val_dataset", val, "--output_val_dataset", str(out / "val"), "--input_train_dataset", train,
                    "--output_train_dataset", str(out / "train"), "--nb_seq_val", "2", "--nb_seq_train", "1", "--ISO", "12800",
                    "--first", "1", "--last", "3", "--seed", "5", "--batch", str(batch)], runtime=stubs[batch])
        assert n == {"train": 3, "val": 6}
        trees[batch] = _tree(str(out))
    assert [c["n"] for c in stubs[1].calls] == [1] * 9 and [c["n"] for c in stubs[3].calls] == [3] * 3
    assert [c["frame0"] for c in stubs[3].calls] == [1, 1, 1] and [c["frame0"] for c in stubs[1].calls] == [1, 2, 3] * 3
    assert [c["seed"] for c in stubs[3].calls] == [M.sequence_seed(5, "train", 0), M.sequence_seed(5, "val", 0), M.sequence_seed(5, "val", 1)]
    n_gain, red, blue = find_gains(1, 12800)
    assert stubs[3].calls[2]["gains"] == (1 / n_gain, red, blue) and stubs[3].calls[2]["iso"] == 12800
    want = {f"{split}/{folder}_iso12800/{s:03d}/{i:08d}.{ext}"
            for split, nseq, folders in (("train", 1, ("gt", "gt_raw_linear_RGB", "noisy")), ("val", 2, ("gt", "gt_raw_linear_RGB", "noisy", "gt_RGB")))
            for folder in folders for s in range(nseq) for i in (1, 2, 3) for ext in (("png",) if folder == "gt_RGB" else ("tiff",))}
    assert set(trees[1]) == want
    assert trees[1] == trees[3]                                              # byte for byte
    v = tmp_path / "out3" / "val"
    a = tiffio.read(str(v / "gt_iso12800/001/00000002.tiff"))
    assert a.dtype == np.float32 and a.shape == (6, 9, 4)
    assert tiffio.read(str(v / "noisy_iso12800/001/00000002.tiff")).dtype == np.float32
    u = tiffio.read(str(v / "gt_raw_linear_RGB_iso12800/001/00000002.tiff"))
    assert u.dtype == np.uint16 and u.shape == (12, 18, 3)
    p = iio_read(str(v / "gt_RGB_iso12800/001/00000002.png"))
    assert p.dtype == np.uint8 and p.shape == (12, 18, 3)
    # the mosaic on disk is the mosaic of the linear image on disk, up to its rounding
    assert np.abs(U.mosaic(u.astype(np.float64)) - a).max() <= 0.5
    # a split without an input pattern is left out; --step 2 gives frames 1 and 3, one call each
    s2 = StubRuntime()
    n = M.main(["--input_val_dataset", val, "--output_val_dataset", str(tmp_path / "o2"), "--nb_seq_val", "1", "--first", "1", "--last", "3",
                "--step", "2", "--seed", "5", "--ISO", "12800", "--bayer_pattern", "rggb"], runtime=s2)
    assert n == {"train": 0, "val": 2} and [c["frame0"] for c in s2.calls] == [1, 3] and s2.calls[0]["pattern"] == "rggb"
    # frame 3 regenerated alone is the frame 3 of the whole run (the draws are keyed by the frame index): the linear image,
    # which does not depend on the pattern
    assert _tree(str(tmp_path / "o2"))["gt_raw_linear_RGB_iso12800/000/00000003.tiff"] == trees[3]["val/gt_raw_linear_RGB_iso12800/000/00000003.tiff"]
    with pytest.raises(SystemExit):
        M.main(["--ISO", "1600"], runtime=s2)
