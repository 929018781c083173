"""Where the shots of a reel begin:
`python -m rvdd_release_amd.cuts --dataroot D --nFolder noisy --bit_depth 12 [--cut_hist T] [--cut_grid T] [--cut_min_len L] [--scores]
[container flags of denoise]`.

Reads the tree `denoise` reads (`--dataset_mode rawvideo`: uint16 / float32 mosaics or packed frames, TIFFs of packed 10 / 12 / 14-bit
samples, or with `--raw_container mipi --raw_size WxH` headerless MIPI CSI-2 frames), ingests EVERY frame of every video on the device
through the calls `denoise` uses (`rvdd_ingest_raw` / `rvdd_ingest_bits`, the gray plane only), takes one 6 KiB integer signature per
frame (`rvdd_frame_sigs`: level counts per band of rows, sums per block of a 16 x 16 grid; the rule is in include/rvdd.h) and compares
consecutive signatures on the host (`rvdd_cut_score`).  Prints one JSON line per video:

    {"video": key, "frames": N, "cuts": [k, ...]}

k: the index, 1 .. N-1 in the video's sorted frames, of a frame that starts a new shot -- frame k differs from frame k-1 by
d_hist > --cut_hist (default 0.10: a tenth of the cells changed their level bin) or d_grid > --cut_grid (default 0.12: the 16 x 16 layout
moved by 12 % of its mass).  A cut fewer than --cut_min_len frames (default 4) behind the previous one, or before the end, is dropped.
With --scores the line also carries "scores": [[d_hist, d_grid], ...], the N-1 pairs with 17 significant digits.  `denoise --cuts FILE`
reads these lines; `denoise --cuts auto` runs this pass itself.

The thresholds rest on synthetic scenes of at least about 128 x 192 cells; NOTHING here is measured on real footage.  Two
shots with the same level statistics and no large-scale structure are not told apart, and a fade or a dissolve is no cut.  A false cut (a
flash) costs a few frames of fresh recurrence and nothing else.
"""
from __future__ import annotations

import argparse
import json
from typing import List, Sequence, Tuple

import numpy as np

from .footage import ingest_frames, open_rawvideo
from .runtime import FRAME_SIG_BYTES, cut_score

T_HIST, T_GRID, MIN_LEN = 0.10, 0.12, 4


def signatures(rt, dataset, paths: Sequence[str], bit_depth: int, batch: int = 16) -> np.ndarray:
    """The signatures of the frames at `paths` (one video: one frame size) of a rawvideo dataset as a host uint8 array [N,6144], one
    struct rvdd_frame_sig per frame: read, ingested on `rt`'s device as `video_push` ingests them (gray only) and measured `batch`
    frames at a time, one copy to the host per batch."""
    out = np.empty((len(paths), FRAME_SIG_BYTES), np.uint8)
    for k in range(0, len(paths), max(1, int(batch))):
        part = paths[k:k + max(1, int(batch))]
        _, gray = ingest_frames(rt, dataset, np.stack([dataset.read_frame(p) for p in part]), bit_depth, want_packed=False)
        out[k:k + len(part)] = rt.frame_sigs(gray, int(bit_depth)).cpu().numpy()
    return out


def scores_of(sig: np.ndarray, hh: int, ww: int) -> List[Tuple[float, float]]:
    """(d_hist, d_grid) of every pair (k - 1, k) of the signatures [N,6144] of frames of hh x ww cells: N - 1 pairs"""
    return [cut_score(sig[k - 1], sig[k], hh, ww) for k in range(1, len(sig))]


def find_cuts(scores: Sequence[Tuple[float, float]], t_hist: float = T_HIST, t_grid: float = T_GRID, min_len: int = MIN_LEN) -> List[int]:
    """The frames that start a new shot, from the len(scores) + 1 frames' score pairs: frame k iff d_hist > t_hist or d_grid > t_grid for
    the pair (k - 1, k).  A cut fewer than `min_len` frames after the previous accepted cut (or after frame 0) is dropped, and so is one
    fewer than `min_len` frames before the video's end: no shot is shorter than min_len."""
    n = len(scores) + 1
    cuts: List[int] = []
    last = 0
    for k in range(1, n):
        d_hist, d_grid = scores[k - 1]
        if not (d_hist > t_hist or d_grid > t_grid):
            continue
        if k - last < min_len or n - k < min_len:
            continue
        cuts.append(k)
        last = k
    return cuts


def add_arguments(p: argparse.ArgumentParser) -> None:
    """the three flags this command and `denoise --cuts auto` share"""
    p.add_argument('--cut_hist', type=float, default=None, help='threshold on d_hist, the share of cells whose level bin changed (default %g)' % T_HIST)
    p.add_argument('--cut_grid', type=float, default=None, help='threshold on d_grid, the share of the 16 x 16 layout that moved (default %g)' % T_GRID)
    p.add_argument('--cut_min_len', type=int, default=None, help='the shortest shot, in frames (default %d)' % MIN_LEN)


def thresholds(own, least_len: int = 2) -> Tuple[float, float, int]:
    """(t_hist, t_grid, min_len) of the parsed flags; SystemExit where one makes no sense.  least_len: the shortest shot the caller
    can take (`denoise`: 2 + future, a video that yields a frame)."""
    t_hist = T_HIST if own.cut_hist is None else own.cut_hist
    t_grid = T_GRID if own.cut_grid is None else own.cut_grid
    min_len = max(MIN_LEN, least_len) if own.cut_min_len is None else own.cut_min_len
    if not (t_hist >= 0 and t_grid >= 0):
        raise SystemExit("--cut_hist and --cut_grid are thresholds >= 0, got %r and %r" % (t_hist, t_grid))
    if min_len < least_len:
        raise SystemExit("--cut_min_len must be at least %d, got %d" % (least_len, min_len))
    return float(t_hist), float(t_grid), int(min_len)


def format_line(key: str, frames: int, cuts: Sequence[int], scores=None) -> str:
    """the JSON line of one video; the scores as %.17g, which float() reads back to the same doubles"""
    line = '{"video": %s, "frames": %d, "cuts": [%s]' % (json.dumps(key), frames, ", ".join("%d" % k for k in cuts))
    if scores is not None:
        line += ', "scores": [%s]' % ", ".join("[%.17g, %.17g]" % (h, g) for h, g in scores)
    return line + "}"


def detect(rt, dataset, videos, bit_depth: int, t_hist: float, t_grid: float, min_len: int, batch: int = 16):
    """[(key, frames, cuts, scores)] of `videos` ([(key, [paths])], as `dataset.videos`)"""
    found = []
    for key, paths in videos:
        H, W = dataset.frame_size(paths[0])
        if H // 2 < 16 or W // 2 < 16:
            raise SystemExit("cuts: %s: frames of %d x %d pixels are too small for a 16 x 16 grid of cells (at least 32 x 32)" % (key, W, H))
        scores = scores_of(signatures(rt, dataset, paths, bit_depth, batch), H // 2, W // 2)
        found.append((key, len(paths), find_cuts(scores, t_hist, t_grid, min_len), scores))
    return found


def main(argv=None) -> list:
    from .options import parse
    from .util._ops import ops_runtime
    p = argparse.ArgumentParser(add_help=False)
    add_arguments(p)
    p.add_argument('--scores', action='store_true', help='also print the N-1 score pairs of every video')
    own, rest = p.parse_known_args(argv)
    t_hist, t_grid, min_len = thresholds(own, 1)
    opt = parse(rest)
    dataset = open_rawvideo(opt, rest, "cuts")
    rt = ops_runtime(opt.gpu_ids[0] if opt.gpu_ids else 0)
    found = detect(rt, dataset, dataset.videos, int(opt.bit_depth), t_hist, t_grid, min_len)
    for key, frames, cuts, scores in found:
        print(format_line(key, frames, cuts, scores if own.scores else None))
    return [{"video": key, "frames": frames, "cuts": cuts, "scores": scores} for key, frames, cuts, scores in found]


if __name__ == '__main__':
    main()
