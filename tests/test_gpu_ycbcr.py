"""Denoised footage as playable video (rvdd_ycbcr, RvddRuntime.ycbcr, --video_out of the denoise command line), through the C ABI:
the kernel against its NumPy restatement (tests/ycbcr_ref.py) in both of its forms, what it may not write, the argument checks, the
composed path behind rvdd_ppipe, and the command on disk.  Every comparison of samples is exact."""
import json
import os

import numpy as np
import pytest
import torch

import ycbcr_ref as R
from conftest import WEIGHTS
from gpu_support import files_of, ops_rt as _rt, upload
from stream_ref import mosaic_of, quantised_dn

pytestmark = pytest.mark.gpu

# n x H x W: one quad; the narrow form (W no multiple of 8), several images; the wide form (W % 8 == 0, aligned pointers), two images
# ... and the wide form on images of 24 and 72 samples at 8 bits, no multiple of 16: the second image starts on 8 bytes only
SHAPES = [(1, 2, 2), (3, 6, 10), (2, 32, 48), (2, 2, 8), (3, 6, 8)]


def _host(t):
    """a result tensor on the host: uint8, or uint16 whatever the 16-bit view was"""
    if t.dtype == torch.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _specials(n, H, W):
    """values in range with what is no number, the zeros and the edge of the clamp strewn over them"""
    rng = np.random.default_rng(n * 1000 + H * W)
    d = rng.uniform(0.0, 255.0, (n, H, W, 3)).astype(np.float32)
    words = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 255.0, 255.0001, 254.99998, 1e-30, -1e-30, 3e38, -3e38], np.float32)
    flat = d.reshape(-1)
    at = rng.permutation(flat.size)[:min(flat.size, 4 * words.size)]
    flat[at] = np.resize(words, at.size)
    return d


def _inputs(n, H, W):
    rng = np.random.default_rng(n + 10 * H + 100 * W)
    return {"random": rng.uniform(-8.0, 262.0, (n, H, W, 3)).astype(np.float32),
            "integers": rng.integers(0, 256, (n, H, W, 3)).astype(np.float32),
            "specials": _specials(n, H, W)}


@pytest.mark.parametrize("n,H,W", SHAPES)
@pytest.mark.parametrize("depth", [8, 10])
def test_ycbcr_is_the_restatement(n, H, W, depth):
    rt = _rt()
    per = H * W * 3 // 2
    for name, d in _inputs(n, H, W).items():
        want = R.frame_bytes(d, depth)
        dev = upload(d)
        got = rt.ycbcr(dev, depth)
        assert got.shape == (n, per) and got.dtype == (torch.uint8 if depth == 8 else getattr(torch, "uint16", torch.int16))
        got = _host(got)
        assert got.dtype == want.dtype and np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:3])
        # the same values four bytes off the 16-byte boundary: the narrow form, the same bits
        off = _host(rt.ycbcr(upload(d, offset=True), depth))
        assert np.array_equal(off, want), (name, "input off its alignment")


@pytest.mark.parametrize("depth", [8, 10])
def test_every_colour_of_a_coarse_grid(depth):
    """all (r,g,b) of 18 levels each, every one a flat 2 x 2 quad: 108 x 108 quads in the narrow form, and cropped to a width of 208 the wide"""
    rt = _rt()
    lv = np.array(list(range(0, 256, 16)) + [127.5, 255], np.float32)
    rgb = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(54, 108, 3)
    d = np.repeat(np.repeat(rgb, 2, axis=0), 2, axis=1)[None]
    for crop in (216, 208):
        x = np.ascontiguousarray(d[:, :, :crop])
        assert np.array_equal(_host(rt.ycbcr(upload(x), depth)), R.frame_bytes(x, depth)), crop
    m = 1 << (depth - 8)
    Y, Cb, Cr = R.ycbcr(d, depth)
    grey = (rgb[..., 0] == rgb[..., 1]) & (rgb[..., 1] == rgb[..., 2])
    assert grey.sum() == 18 and np.all(Cb[0][grey] == 128 * m) and np.all(Cr[0][grey] == 128 * m)


@pytest.mark.parametrize("depth", [8, 10])
def test_nothing_is_written_beyond_the_frames(depth):
    """the output lies inside a larger allocation filled with a guard value; wide and narrow form, aligned and off by one sample"""
    rt = _rt()
    tdt, guard = (torch.uint8, 0xA5) if depth == 8 else (torch.int16, 0x5AA5)
    for n, H, W in SHAPES:
        d = _inputs(n, H, W)["random"]
        want = R.frame_bytes(d, depth)
        count = want.size
        for lead in (0, 1, 16):                       # samples in front: on a 16-byte boundary, off it (the narrow form), on one again
            whole = torch.full((lead + count + 64,), guard, dtype=tdt, device="cuda")
            out = whole[lead:lead + count].view(n, -1)
            back = rt.ycbcr(upload(d), depth, out=out)
            assert back.data_ptr() == out.data_ptr()
            host = _host(whole)
            assert np.array_equal(host[lead:lead + count].reshape(n, -1), want), (n, H, W, lead)
            assert np.all(host[:lead] == guard) and np.all(host[lead + count:] == guard), (n, H, W, lead)
    # no image: nothing is written, null pointers are fine
    whole = torch.full((64,), guard, dtype=tdt, device="cuda")
    assert rt.ycbcr(torch.empty(0, 4, 8, 3, device="cuda"), depth).shape == (0, 48)
    assert rt.lib.rvdd_ycbcr(rt.h, None, 0, 4, 8, depth, None, None) == 0
    assert rt.lib.rvdd_ycbcr(rt.h, None, 0, 4, 8, depth, whole.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((whole == guard).all())


def test_refusals_name_the_argument_and_write_nothing():
    rt = _rt()
    x = torch.full((1, 32, 48, 3), 99.0, device="cuda")
    out = torch.full((32 * 48 * 3,), 7, dtype=torch.uint8, device="cuda")

    def call(n=1, H=32, W=48, depth=8, disp=x.data_ptr(), o=out.data_ptr()):
        rc = rt.lib.rvdd_ycbcr(rt.h, disp, n, H, W, depth, o, None)
        return rc, rt.lib.rvdd_last_error(rt.h)

    bad = [({"H": 31}, b" H "), ({"H": 0}, b" H "), ({"H": -2}, b" H "), ({"W": 47}, b" W "), ({"W": 0}, b" W "), ({"W": -4}, b" W "),
           ({"depth": 9}, b"depth"), ({"depth": 12}, b"depth"), ({"depth": 0}, b"depth"), ({"depth": 16}, b"depth"),
           ({"n": -1}, b" n "), ({"disp": None}, b"disp is required"), ({"o": None}, b"frames is required"),
           # 2^24 images of 2^12 x 2^12: 2^41 strips of the wide form, 2^33 blocks (nothing is launched, nothing is read)
           ({"n": 1 << 24, "H": 1 << 12, "W": 1 << 12}, b"2^31 - 1 blocks"),
           ({"n": (1 << 31) - 1, "H": (1 << 31) - 2, "W": (1 << 31) - 2}, b"2^31 - 1 blocks")]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b"rvdd_ycbcr:") and word in msg, (kw, msg)
    assert rt.lib.rvdd_ycbcr(None, x.data_ptr(), 1, 32, 48, 8, out.data_ptr(), None) == -1
    assert call(n=0)[0] == 0 and call(n=0, disp=None, o=None)[0] == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                          # none of these wrote anything
    # the Python side says the same before the library is asked
    with pytest.raises(ValueError, match="depth must be 8 or 10"):
        rt.ycbcr(x, 12)
    with pytest.raises(RuntimeError, match="H and W must be even"):
        rt.ycbcr(x[:, :31], 8)
    with pytest.raises(RuntimeError, match=r"disp is float32 \[n,H,W,3\]"):
        rt.ycbcr(x[..., :2], 8)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        rt.ycbcr(x.cpu(), 8)
    with pytest.raises(RuntimeError, match="ycbcr: out must be a contiguous"):
        rt.ycbcr(x, 8, out=out[:-1].view(1, -1))
    assert call()[0] == 0                                                  # ... and the valid call goes through
    torch.cuda.synchronize()
    assert np.array_equal(out[:32 * 48 * 3 // 2].cpu().numpy()[None], R.frame_bytes(x.cpu().numpy(), 8)) and bool((out[32 * 48 * 3 // 2:] == 7).all())


@pytest.mark.parametrize("depth", [8, 10])
def test_behind_ppipe_it_is_the_restatement_of_that_float_image(depth):
    """the composed path of `denoise`: a network output through rvdd_ppipe's float image into rvdd_ycbcr, all slots at once"""
    from rvdd_release_amd import _lib
    rt = _rt()
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-1.1, 1.1, (2, 3, 32, 48)).astype(np.float32)).cuda()
    for iso in (3200, 12800):
        u8, disp = rt.ppipe(x, 1.0 / 1.3, 1.9, 1.5, iso, _lib.PPIPE_FROM_NET, "nchw", want_float=True)
        assert disp.shape == (2, 32, 48, 3) and disp.is_contiguous()
        got = _host(rt.ycbcr(disp, depth))
        assert np.array_equal(got, R.frame_bytes(disp.cpu().numpy(), depth)), iso


# ---- the command ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
def test_denoise_main_writes_y4m(tmp_path, future):
    from rvdd_release_amd import denoise, synth, tiffio
    from rvdd_release_amd.library import iio_read
    from rvdd_release_amd.y4m import read_y4m
    H, W, T = 32, 48, 4
    iso = 12800 if future else 3200
    render = (iso, 1.3, 1.9, 1.5)
    name = "recurrent-convunet+feat-future-iso12800" if future else "recurrent-convunet+feat-iso3200"
    root = tmp_path / "data"
    for v in range(3):
        cells = quantised_dn(synth.make_sequence(T, H, W, iso=iso, seed=60 + v).raw)
        os.makedirs(root / "noisy" / ("%03d" % v))
        for t in range(T):
            tiffio.write(str(root / "noisy" / ("%03d" % v) / ("%08d.tiff" % (3 * t))), mosaic_of(cells[t:t + 1])[0].astype(np.uint16))
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, name), "--feature_rec",
             "--future_patch_depth", str(future), "--batch_size", "2", "--dataroot", str(root), "--nFolder", "noisy"]
    video = ["--video_render", "%d,%r,%r,%r" % render]
    rt = _rt()

    def run(tag, *extra):
        res = tmp_path / ("res_" + tag)
        stats = denoise.main(flags + ["--results_dir", str(res)] + list(extra))
        return res, files_of(str(res)), stats

    def frames_are_their_tiffs(res, y4m, stems, depth):
        """the stream's frames, in order, are the restatement of rvdd_ppipe's float image of the TIFFs of `stems` of the same run"""
        head, frames = read_y4m(str(res / y4m))
        assert (head["W"], head["H"], head["depth"], head["fps"]) == (W, H, depth, (24, 1)) and len(frames) == len(stems), (y4m, len(frames), stems)
        for (Y, Cb, Cr), stem in zip(frames, stems):
            tif = iio_read(str(res / (stem + "_denoised.tif")))
            assert tif.dtype == np.float32 and tif.shape == (H, W, 3)
            _, disp = rt.ppipe(torch.from_numpy(tif)[None].cuda(), 1.0 / render[1], render[2], render[3], iso, 8, "hwc", want_float=True)
            wy, wb, wr = R.ycbcr(disp.cpu().numpy(), depth)
            assert np.array_equal(Y, wy[0]) and np.array_equal(Cb, wb[0]) and np.array_equal(Cr, wr[0]), (y4m, stem)

    keys = ["%03d" % v for v in range(3)]
    names = lambda ts: ["%08d" % (3 * t) for t in ts]
    # without the flag: the files of before
    _, plain, stats = run("plain")
    inner = list(range(1, T - future))
    assert sorted(plain) == sorted(os.path.join(k, s + "_denoised.tif") for k in keys for s in names(inner)) and stats["frames"] == 3 * len(inner)
    # y4m8 beside the TIFFs: one stream per video, the TIFFs keep their bytes
    res, files, stats = run("y4m8", "--video_out", "y4m8", *video)
    assert sorted(k for k in files if k.endswith(".y4m")) == [k + ".y4m" for k in keys] and stats["frames"] == 3 * len(inner)
    assert {k: v for k, v in files.items() if not k.endswith(".y4m")} == plain
    for k in keys:
        frames_are_their_tiffs(res, k + ".y4m", [os.path.join(k, s) for s in names(inner)], 8)
    y4m8 = files
    # y4m10 alone: --out_format none leaves only the streams; their frames are those of the TIFFs of the run above
    res10, files, stats = run("y4m10", "--video_out", "y4m10", "--out_format", "none", "--video_fps", "24", *video)
    assert sorted(files) == [k + ".y4m" for k in keys] and stats["frames"] == 3 * len(inner)
    for k in keys:
        os.replace(str(res10 / (k + ".y4m")), str(res / (k + ".10.y4m")))
        frames_are_their_tiffs(res, k + ".10.y4m", [os.path.join(k, s) for s in names(inner)], 10)
    # ... and --out_format none changes no stream
    _, files, _ = run("y4m8_none", "--video_out", "y4m8", "--out_format", "none", *video)
    assert files == {k: v for k, v in y4m8.items() if k.endswith(".y4m")}
    # --all_frames: T frames per video; --cuts FILE splits video 001 in front of its frame 2: two streams named after the shots' first frames
    listed = str(tmp_path / "cuts.txt")
    with open(listed, "w") as f:
        f.write(json.dumps({"video": "001", "frames": T, "cuts": [2]}) + "\n")
    res, files, stats = run("cuts", "--video_out", "y4m8", "--all_frames", "--cuts", listed, *video)
    shots = {"000." + names([0])[0]: ("000", range(T)), "001." + names([0])[0]: ("001", range(2)), "001." + names([2])[0]: ("001", range(2, T)),
             "002." + names([0])[0]: ("002", range(T))}
    assert sorted(k for k in files if k.endswith(".y4m")) == sorted(s + ".y4m" for s in shots) and stats["frames"] == 3 * T
    assert sorted(k for k in files if not k.endswith(".y4m")) == sorted(os.path.join(k, s + "_denoised.tif") for k in keys for s in names(range(T)))
    for shot, (k, ts) in shots.items():
        frames_are_their_tiffs(res, shot + ".y4m", [os.path.join(k, s) for s in names(ts)], 8)
    # ... and without --cuts one stream of T frames per video, the uncut videos' byte for byte those of the run with the list
    res_all, whole, stats = run("all", "--video_out", "y4m8", "--all_frames", *video)
    assert sorted(k for k in whole if k.endswith(".y4m")) == [k + ".y4m" for k in keys] and stats["frames"] == 3 * T
    for k in keys:
        frames_are_their_tiffs(res_all, k + ".y4m", [os.path.join(k, s) for s in names(range(T))], 8)
    assert whole["000.y4m"] == files["000." + names([0])[0] + ".y4m"] and whole["002.y4m"] == files["002." + names([0])[0] + ".y4m"]
