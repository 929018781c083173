"""YUV4MPEG2 (Y4M) streams of Y'CbCr 4:2:0 frames: the container `denoise --video_out` writes.  Pure host code.

A stream is one header line and, per frame, the line `FRAME` and the frame's body: the Y plane [H,W], then Cb, then Cr [H/2,W/2] --
bytes at 8 bits, little-endian 16-bit words at 10 bits -- which is exactly one row of `RvddRuntime.ycbcr`.  The header names the
sampling the way the players and encoders that read Y4M expect it: `C420jpeg` (chroma sited in the centre of its quad) at 8 bits,
`C420p10` at 10, and the range as `XCOLORRANGE=LIMITED`.

    with Y4MWriter(path, W, H, 8, 24, 1) as w:
        w.write(body)                       # bytes, or a uint8 / uint16 array of H*W*3/2 samples
    header, frames = read_y4m(path)         # {"W", "H", "depth", "fps", "line", ...}, [(Y, Cb, Cr), ...]
"""
from __future__ import annotations

import sys
from typing import Dict, List, Tuple

import numpy as np

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME\n"
# depth -> the colour-space words of the header
_CSP = {8: "C420jpeg XYSCSS=420JPEG", 10: "C420p10 XYSCSS=420P10"}


class Y4MError(ValueError):
    """a file that is not a Y4M stream of the kinds written here, with the reason"""


def frame_samples(W: int, H: int) -> int:
    return W * H * 3 // 2


def header_line(W: int, H: int, depth: int, fps_num: int, fps_den: int) -> bytes:
    """the stream header, its newline included"""
    if depth not in _CSP:
        raise ValueError("y4m: depth must be 8 or 10, got %r" % (depth,))
    if W < 2 or H < 2 or W % 2 or H % 2:
        raise ValueError("y4m: W and H must be even and >= 2 (4:2:0), got %d x %d" % (W, H))
    if fps_num < 1 or fps_den < 1:
        raise ValueError("y4m: the frame rate is a ratio of positive integers, got %r:%r" % (fps_num, fps_den))
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=LIMITED\n" % (W, H, fps_num, fps_den, _CSP[depth])).encode("ascii")


class Y4MWriter:
    """An open Y4M file: the header is written once, here; `write` appends one frame; `close` (or leaving the `with`) ends it."""

    def __init__(self, path: str, W: int, H: int, depth: int, fps_num: int = 24, fps_den: int = 1):
        line = header_line(W, H, depth, fps_num, fps_den)
        self.path, self.W, self.H, self.depth = path, int(W), int(H), int(depth)
        self.frames = 0
        self._bytes = frame_samples(self.W, self.H) * (1 if depth == 8 else 2)
        self._f = open(path, "wb")
        self._f.write(line)

    def write(self, body) -> None:
        """one frame: `bytes`, or an array of H*W*3/2 samples -- uint8 at 8 bits, (u)int16 at 10, in this machine's byte order"""
        if isinstance(body, np.ndarray):
            want = np.uint8 if self.depth == 8 else np.uint16
            if body.dtype == np.int16 and self.depth == 10:
                body = body.view(np.uint16)
            if body.dtype != want:
                raise ValueError("y4m: a frame of a %d-bit stream is %s, got %s" % (self.depth, np.dtype(want).name, body.dtype))
            if self.depth == 10 and sys.byteorder != "little":
                body = body.astype("<u2")
            body = np.ascontiguousarray(body).tobytes()
        if len(body) != self._bytes:
            raise ValueError("y4m: a frame of %d x %d at %d bits is %d bytes, got %d" % (self.W, self.H, self.depth, self._bytes, len(body)))
        self._f.write(FRAME)
        self._f.write(body)
        self.frames += 1

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def parse_header(line: bytes) -> Dict:
    """the fields of a header line (without its newline): W, H, depth, fps (num, den), interlace, aspect, colorspace, extra [X...]"""
    words = line.split(b" ")
    if not words or words[0] != MAGIC:
        raise Y4MError("not a YUV4MPEG2 stream (it starts with %r)" % line[:16])
    h = {"W": None, "H": None, "fps": None, "interlace": None, "aspect": None, "colorspace": "420jpeg", "extra": [], "line": line.decode("ascii", "replace")}
    try:
        for w in words[1:]:
            tag, val = w[:1], w[1:].decode("ascii")
            if tag == b"W":
                h["W"] = int(val)
            elif tag == b"H":
                h["H"] = int(val)
            elif tag == b"F":
                a, b = val.split(":")
                h["fps"] = (int(a), int(b))
            elif tag == b"I":
                h["interlace"] = val
            elif tag == b"A":
                h["aspect"] = val
            elif tag == b"C":
                h["colorspace"] = val
            elif tag == b"X":
                h["extra"].append(val)
            elif w:
                raise ValueError("unknown field %r" % w)
    except ValueError as err:
        raise Y4MError("a header that cannot be read: %s (%s)" % (h["line"], err))
    if h["W"] is None or h["H"] is None:
        raise Y4MError("a header without W or H: %s" % h["line"])
    if h["colorspace"] in ("420jpeg", "420", "420mpeg2", "420paldv"):
        h["depth"] = 8
    elif h["colorspace"] == "420p10":
        h["depth"] = 10
    else:
        raise Y4MError("colour space C%s: only 4:2:0 at 8 bits (C420jpeg) and 10 bits (C420p10) is read here" % h["colorspace"])
    if h["W"] < 2 or h["H"] < 2 or h["W"] % 2 or h["H"] % 2:
        raise Y4MError("4:2:0 frames of %d x %d: W and H must be even and >= 2" % (h["W"], h["H"]))
    return h


def read_y4m(path: str) -> Tuple[Dict, List[Tuple[np.ndarray, np.ndarray, np.ndarray]]]:
    """-> (the header's fields (`parse_header`), [(Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2]) per frame]), uint8 or uint16.  Y4MError, with the
    frame named, for a file that ends inside a frame or holds something else where a frame starts."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"\n")
    if end < 0:
        raise Y4MError("%s: no header line" % path)
    try:
        h = parse_header(data[:end])
    except Y4MError as err:
        raise Y4MError("%s: %s" % (path, err))
    W, H = h["W"], h["H"]
    dtype = np.dtype(np.uint8) if h["depth"] == 8 else np.dtype("<u2")
    nbytes = frame_samples(W, H) * dtype.itemsize
    frames, pos = [], end + 1
    while pos < len(data):
        eol = data.find(b"\n", pos)
        line = data[pos:eol if eol >= 0 else len(data)]
        if eol < 0 or not (line == b"FRAME" or line.startswith(b"FRAME ")):
            raise Y4MError("%s: frame %d: expected a FRAME line at byte %d, found %r" % (path, len(frames), pos, line[:16]))
        pos = eol + 1
        if len(data) - pos < nbytes:
            raise Y4MError("%s: truncated: frame %d has %d of its %d bytes" % (path, len(frames), len(data) - pos, nbytes))
        s = np.frombuffer(data, dtype=dtype, count=frame_samples(W, H), offset=pos).astype(dtype.newbyteorder("="))
        y, c = W * H, W * H // 4
        frames.append((s[:y].reshape(H, W), s[y:y + c].reshape(H // 2, W // 2), s[y + c:].reshape(H // 2, W // 2)))
        pos += nbytes
    return h, frames
