"""Y'CbCr 4:2:0 video out, the parts that need no GPU: the NumPy restatement of rvdd_ycbcr's rule (tests/ycbcr_ref.py) against the
real-valued BT.709 formula in float64, the Y4M container's round trip, the refusals of the new flags of the denoise command line, and
the symbol in the header and the library."""
import os
import subprocess

import numpy as np
import pytest

import ycbcr_ref as R
from conftest import REPO

H, W = 64, 96
# include/rvdd.h: 0.5 for the one rounding + 3 * 2^-15 * 876 = 0.08 for the 14-bit coefficients + 0.007 for the 16-bit input
# quantisation, at 10 bits (a quarter of the last two at 8)
BOUND = 0.6


def _inputs():
    rng = np.random.default_rng(5)
    rnd = rng.uniform(-8.0, 262.0, (2, H, W, 3)).astype(np.float32)           # values outside [0,255] included
    ints = rng.integers(0, 256, (2, H, W, 3)).astype(np.float32)
    flat = np.repeat(np.repeat(rng.uniform(0.0, 255.0, (1, H // 2, W // 2, 3)).astype(np.float32), 2, axis=1), 2, axis=2)
    return {"random": rnd, "integers": ints, "flat quads": flat}


@pytest.mark.parametrize("depth", [8, 10])
def test_restatement_is_the_real_formula_rounded(depth):
    for name, d in _inputs().items():
        got = R.ycbcr(d, depth)
        want = R.real(d, depth)
        for plane, g, w in zip(("Y", "Cb", "Cr"), got, want):
            err = np.abs(g.astype(np.float64) - w)
            off = np.abs(g.astype(np.float64) - np.rint(w))
            print("depth %d, %s, %s: worst error %.4f codes, %d of %d samples off their rounding" % (depth, name, plane, err.max(), int((off != 0).sum()), off.size))
            assert err.max() <= BOUND, (depth, name, plane, err.max())
            assert off.max() <= 1, (depth, name, plane)
            assert g.dtype == (np.uint8 if depth == 8 else np.uint16)
        m = 1 << (depth - 8)
        assert got[0].min() >= 16 * m and got[0].max() <= 235 * m
        assert min(got[1].min(), got[2].min()) >= 16 * m and max(got[1].max(), got[2].max()) <= 240 * m


@pytest.mark.parametrize("depth", [8, 10])
def test_anchors_hold_exactly(depth):
    m = 1 << (depth - 8)

    def of(r, g, b):
        Y, Cb, Cr = R.ycbcr(np.full((2, 2, 3), (r, g, b), np.float32), depth)
        assert Y.shape == (1, 2, 2) and Cb.shape == Cr.shape == (1, 1, 1) and len(set(Y.ravel().tolist())) == 1
        return int(Y[0, 0, 0]), int(Cb[0, 0, 0]), int(Cr[0, 0, 0])

    assert of(255, 255, 255) == (235 * m, 128 * m, 128 * m)
    assert of(0, 0, 0) == (16 * m, 128 * m, 128 * m)
    assert of(0, 0, 255)[1] == 240 * m and of(255, 0, 0)[2] == 240 * m
    assert of(255, 255, 0)[1] == 16 * m and of(0, 255, 255)[2] == 16 * m
    for v in list(range(0, 256, 5)) + [0.25, 17.5, 99.999, 254.9]:
        assert of(v, v, v)[1:] == (128 * m, 128 * m), v
    # outside the range, and what is no number: the clamp
    assert of(300, 1e9, np.inf) == of(255, 255, 255) and of(-3, -np.inf, -0.0) == of(0, 0, 0) and of(np.nan, np.nan, np.nan) == of(0, 0, 0)
    assert of(255.0001, 255.0001, 255.0001) == of(255, 255, 255)


@pytest.mark.parametrize("depth", [8, 10])
def test_shift_and_divide_forms_are_the_floor_divisions(depth):
    """csrc/ycbcr.hip divides by K = 65535 * 2^14 and 4K = 65535 * 2^16 as a shift and a division by 65535 of a number below 2^26, the
    signed chroma numerator lifted by 512 * 4K first: the same integers as the rule's floor divisions, on every corner, on the grey and
    the primary axes and on random values"""
    m = 1 << (depth - 8)
    rng = np.random.default_rng(depth)
    e = np.array([0, 1, 2, 255, 256, 257, 32767, 32768, 65278, 65534, 65535], np.int64)
    axis = np.arange(65536, dtype=np.int64)
    zero = np.zeros_like(axis)
    corners = np.stack(np.meshgrid(e, e, e, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([corners, np.stack([axis, axis, axis], -1), np.stack([axis, zero, zero], -1), np.stack([zero, axis, zero], -1),
                        np.stack([zero, zero, axis], -1), rng.integers(0, 65536, (2000000, 3))])
    L = R.LUMA[0] * q[:, 0] + R.LUMA[1] * q[:, 1] + R.LUMA[2] * q[:, 2]
    t = (L * (219 * m) + R.K // 2) >> 14
    assert t.max() < 1 << 26 and np.array_equal(16 * m + t // 65535, 16 * m + (L * (219 * m) + R.K // 2) // R.K)
    s = np.concatenate([4 * q, 4 * q - rng.integers(0, 4, q.shape) * (q > 0), q])       # sums of four samples, 0 .. 4 * 65535
    for row in (R.CB, R.CR):
        c = row[0] * s[:, 0] + row[1] * s[:, 1] + row[2] * s[:, 2]
        assert np.abs(c).max() < 1 << 31
        num = c * (224 * m) + 2 * R.K + 512 * 4 * R.K
        assert num.min() > 0 and (num >> 16).max() < 1 << 26
        assert np.array_equal(128 * m - 512 + (num >> 16) // 65535, 128 * m + (c * (224 * m) + 2 * R.K) // (4 * R.K))


def test_frame_bytes_is_y_then_cb_then_cr():
    d = _inputs()["random"][:, :6, :10]
    for depth in (8, 10):
        Y, Cb, Cr = R.ycbcr(d, depth)
        body = R.frame_bytes(d, depth)
        assert body.shape == (2, 6 * 10 * 3 // 2) and body.dtype == Y.dtype
        for i in range(2):
            assert np.array_equal(body[i], np.concatenate([Y[i].ravel(), Cb[i].ravel(), Cr[i].ravel()]))


# ---- the container ----
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10)])
def test_y4m_round_trip(tmp_path, depth, H, W):
    from rvdd_release_amd.y4m import Y4MError, Y4MWriter, read_y4m
    rng = np.random.default_rng(depth + H)
    d = rng.uniform(0, 255, (3, H, W, 3)).astype(np.float32)
    body = R.frame_bytes(d, depth)
    path = str(tmp_path / "v.y4m")
    with Y4MWriter(path, W, H, depth, 30000, 1001) as w:
        w.write(body[0])
        w.write(body[1].tobytes())                                          # bytes serve as well
        w.write(body[2].view(np.int16) if depth == 10 else body[2])         # ... and the int16 view of the 16-bit samples
        with pytest.raises(ValueError, match="bytes, got"):
            w.write(body[0][:-1])
        assert w.frames == 3
    raw = open(path, "rb").read()
    line = b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 " % (W, H) + \
        (b"C420jpeg XYSCSS=420JPEG" if depth == 8 else b"C420p10 XYSCSS=420P10") + b" XCOLORRANGE=LIMITED\n"
    assert raw.startswith(line)
    per = H * W * 3 // 2 * (1 if depth == 8 else 2)
    assert len(raw) == len(line) + 3 * (6 + per) and raw[len(line):len(line) + 6] == b"FRAME\n"
    assert raw[len(line) + 6:len(line) + 6 + per] == body[0].astype("<u2" if depth == 10 else np.uint8).tobytes()
    head, frames = read_y4m(path)
    assert (head["W"], head["H"], head["depth"], head["fps"]) == (W, H, depth, (30000, 1001)) and head["line"].encode() == line[:-1]
    assert head["interlace"] == "p" and head["aspect"] == "1:1" and "COLORRANGE=LIMITED" in head["extra"]
    Y, Cb, Cr = R.ycbcr(d, depth)
    assert len(frames) == 3
    for i, (y, cb, cr) in enumerate(frames):
        assert y.dtype == Y.dtype and np.array_equal(y, Y[i]) and np.array_equal(cb, Cb[i]) and np.array_equal(cr, Cr[i])
    # a file that ends inside a frame, and one with something else where a frame starts
    open(path, "wb").write(raw[:-1])
    with pytest.raises(Y4MError, match="truncated: frame 2 has %d of its %d bytes" % (per - 1, per)):
        read_y4m(path)
    open(path, "wb").write(raw[:len(line)] + b"FRAMF\n" + raw[len(line) + 6:])
    with pytest.raises(Y4MError, match="frame 0: expected a FRAME line"):
        read_y4m(path)
    open(path, "wb").write(b"RIFF" + raw)
    with pytest.raises(Y4MError, match="not a YUV4MPEG2 stream"):
        read_y4m(path)


def test_y4m_writer_refuses_what_is_no_420_stream(tmp_path):
    from rvdd_release_amd.y4m import Y4MWriter
    for args, word in (((3, 2, 8, 24, 1), "even"), ((2, 0, 8, 24, 1), "even"), ((2, 2, 12, 24, 1), "depth"), ((2, 2, 8, 0, 1), "frame rate")):
        with pytest.raises(ValueError, match=word):
            Y4MWriter(str(tmp_path / "x.y4m"), *args)
    assert not os.path.exists(tmp_path / "x.y4m")


# ---- the command line ----
RENDER = ["--video_render", "3200,1.3,1.9,1.5"]


@pytest.mark.parametrize("argv,sentence", [
    (["--video_out", "y4m8"], "--video_out needs --video_render ISO,n,red_gain,blue_gain"),
    (["--video_out", "y4m8", "--video_render", "3200,1.3,1.9"], "--video_render takes ISO,n,red_gain,blue_gain"),
    (["--video_out", "y4m8", "--video_render", "3200,1.3,x,1.5"], "--video_render takes ISO,n,red_gain,blue_gain: an integer and three numbers"),
    (["--video_out", "y4m8", "--video_render", "3200,0,1.9,1.5"], "--video_render: n, red_gain and blue_gain must be finite and not zero"),
    (["--video_out", "y4m10", "--video_fps", "0"] + RENDER, "--video_fps takes N or N:D, positive integers, got '0'"),
    (["--video_out", "y4m10", "--video_fps", "24:1:1"] + RENDER, "--video_fps takes N or N:D"),
    (["--video_out", "y4m10", "--video_fps", "23.976"] + RENDER, "--video_fps takes N or N:D"),
    (["--video_out", "y4m12"] + RENDER, "--video_out 'y4m12' is not one of y4m8, y4m10"),
    (["--video_out", "mp4"] + RENDER, "--video_out 'mp4' is not one of y4m8, y4m10"),
    (["--out_format", "none"], "--out_format none writes no per-frame file: it needs --video_out y4m8 | y4m10"),
    (RENDER, "--video_render and --video_fps belong to --video_out"),
    (["--video_fps", "25"], "--video_render and --video_fps belong to --video_out"),
    (["--srgb", "3200,1.3,1.9"], "--srgb takes ISO,n,red_gain,blue_gain"),
])
def test_parse_refusals(argv, sentence):
    from rvdd_release_amd import denoise
    with pytest.raises(SystemExit) as err:
        denoise._parse(list(argv))
    assert sentence in str(err.value), err.value


def test_parse_reads_the_flags():
    from rvdd_release_amd import denoise
    opt = denoise._parse(["--video_out", "y4m10", "--video_fps", "30000:1001", "--out_format", "none"] + RENDER)
    assert opt.video == denoise.VideoOut(10, (3200, 1.3, 1.9, 1.5), (30000, 1001)) and opt.out_format == "none" and opt.srgb is None
    opt = denoise._parse(["--video_out", "y4m8", "--srgb", "12800,1.2,2,1.25"] + RENDER)
    assert opt.video == denoise.VideoOut(8, (3200, 1.3, 1.9, 1.5), (24, 1)) and opt.out_format == "f32" and opt.srgb == (12800, 1.2, 2.0, 1.25)
    assert denoise._parse([]).video is None


# ---- the ABI ----
def test_symbol_is_declared_and_exported():
    from rvdd_release_amd import _lib
    header = open(os.path.join(REPO, "include", "rvdd.h")).read()
    assert "int rvdd_ycbcr(rvdd_t* h, const float* disp" in header
    assert "rvdd_ycbcr" in _lib.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T rvdd_ycbcr\n" in out
    assert b"ycbcr_kernel" in open(_lib.LIB_PATH, "rb").read()
