"""The static defect map of a camera, found from its own footage:
`python -m rvdd_release_amd.dpc_map --dataroot D --nFolder noisy --bit_depth 12 --dpc 4 (--dpc_iso ISO | --dpc_noise a,b | --dpc_noise auto)
[--dpc_dead K] [--frames 16] [--share 0.5] [--tolerate 0] --out map.tif [container flags of denoise]`.

A real defect sits at the same site in every frame while scene detail moves.  The command reads the tree `denoise` reads
(`--dataset_mode rawvideo`), takes --frames frames per video SPREAD EVENLY over the video -- indices round(i (N - 1) / (K - 1)), not
the first K: persistence needs the scene to change -- of up to 16 videos of ONE frame size, ingests them on the device as
`noise.estimate` does, counts per site in how many of them the rule of `--dpc` fires (`rvdd_dpc_detect`; --tolerate t: with t other
defects allowed among the eight neighbours), and calls a sample defective where it was hot, or dead, in at least ceil(share * frames)
of the frames read.  It writes the map as a one-sample uint8 TIFF of the mosaic [H,W], 255 = defective, 0 = good -- independent of
the Bayer pattern, viewable and editable in any image tool, and the form in which a camera's own calibration can be supplied -- and
prints one JSON line:

    {"frames": ..., "share": ..., "tolerate": ..., "samples": ..., "hot": ..., "dead": ..., "cells": ..., "planes": [n0, n1, n2, n3],
     "unfixable": ...}

samples: defective samples; hot / dead: the sites that passed on that side; cells: 2 x 2 cells with a defective sample; planes: per
CFA position; unfixable: samples without a good same-colour site within two sites (`rvdd_dpc_map_stats`), which the correction
leaves as they are.  `denoise --dpc_map map.tif` corrects by the file; `denoise --dpc_map auto` makes this pass itself.

Limits, plainly.  A tripod shot of a static scene gives the map every false alarm of the dynamic rule, since nothing moves: no worse
than `--dpc`, and no better.  --tolerate above 0 is meant for flat or dark calibration footage (a lens-cap shot): on texture it
flags edges and thin lines.  One camera per run: the map is the sensor's, footage of several cameras in one tree gives a map of
none.  The rule is tested on synthetic frames only; NOTHING is measured on real footage.
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import tiffio
from .footage import MAX_VIDEOS, add_dpc_arguments, dpc_arguments, estimate_noise, open_rawvideo, sampled_frames
from .footage import spread_indices  # noqa: F401 -- lives in footage.py with the sampler; kept under this name too
from .runtime import dpc_detect_cfg, dpc_map_from_hits, dpc_map_from_mosaic, dpc_map_stats, dpc_map_to_mosaic

def detect(rt, dataset, bit_depth: int, rule, frames: int = 16, tolerate: int = 0, max_videos: int = MAX_VIDEOS):
    """The persistence counts (a device tensor [4,hh,ww], `RvddRuntime.dpc_detect`) of `frames` frames spread over each of the first
    `max_videos` videos of a rawvideo dataset, ingested on `rt`'s device as `video_push` ingests them; rule = `dpc_cfg(...)`.
    -> (hits, frames read).  RuntimeError where the videos differ in frame size.  Nothing is synchronised."""
    cfg = dpc_detect_cfg(rule, tolerate)
    hits, read = None, 0
    for packed in sampled_frames(rt, dataset, bit_depth, frames, "a defect map", max_videos=max_videos):
        hits = rt.dpc_detect(packed, cfg, int(bit_depth), hits)
        read += 1
    return hits, read


def report(hits, frames: int, share: float, tolerate: int):
    """-> (cellmask uint8 [hh,ww], the dict of the JSON line)"""
    mask, hot, dead = dpc_map_from_hits(hits, frames, share)
    st = dpc_map_stats(mask)
    r = {"frames": int(frames), "share": float(share), "tolerate": int(tolerate), "samples": st["samples"], "hot": int(hot.sum()),
         "dead": int(dead.sum()), "cells": st["cells"], "planes": [int(((mask >> k) & 1).sum()) for k in range(4)], "unfixable": st["unfixable"]}
    return mask, r


def format_line(r: dict) -> str:
    return ('{"frames": %d, "share": %.6g, "tolerate": %d, "samples": %d, "hot": %d, "dead": %d, "cells": %d, "planes": [%s], "unfixable": %d}'
            % (r["frames"], r["share"], r["tolerate"], r["samples"], r["hot"], r["dead"], r["cells"], ", ".join(str(v) for v in r["planes"]),
               r["unfixable"]))


def summary_line(mask, source: str) -> str:
    """the line `denoise` prints: `dpc_map: N samples in M cells, U unfixable, from <source>`"""
    st = dpc_map_stats(mask)
    return 'dpc_map: %d samples in %d cells, %d unfixable, from %s' % (st["samples"], st["cells"], st["unfixable"], source)


def write_map(path: str, mask) -> None:
    """cellmask uint8 [hh,ww] -> the one-sample uint8 TIFF of the mosaic [2hh,2ww], 0 / 255"""
    tiffio.write(path, dpc_map_to_mosaic(mask))


def read_map(path: str):
    """A one-sample image of the mosaic (any integer sample type, nonzero = defective) -> cellmask uint8 [hh,ww]; RuntimeError for
    anything else"""
    a = np.asarray(tiffio.read(path))
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2 or a.dtype.kind not in "iub":
        raise RuntimeError("%s: a defect map is a one-sample integer image of the mosaic, got %s %s" % (path, a.dtype, a.shape))
    return dpc_map_from_mosaic(a)


def check_detect_flags(frames, share, tolerate, prefix="--"):
    """the ranges of --frames / --share / --tolerate (denoise: --dpc_map_frames ...); SystemExit with the reason"""
    if frames < 1:
        raise SystemExit("%sframes must be >= 1, got %d" % (prefix, frames))
    if not 0.0 < share <= 1.0:
        raise SystemExit("%sshare is a share of the frames read, 0 < share <= 1, got %r" % (prefix, share))
    if not 0 <= tolerate <= 3:
        raise SystemExit("%stolerate must be 0..3 (the median of eight neighbours bears three defects), got %d" % (prefix, tolerate))


def main(argv=None) -> dict:
    from .options import parse
    from .util._ops import ops_runtime
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--frames', type=int, default=16, help='frames read per video, spread evenly over it')
    p.add_argument('--share', type=float, default=0.5, help='a site is defective where the rule fired in at least this share of the frames')
    p.add_argument('--tolerate', type=int, default=0, help='0..3 other defects among the eight neighbours (for flat calibration footage)')
    p.add_argument('--out', type=str, default=None, help='the map: a one-sample uint8 TIFF of the mosaic')
    add_dpc_arguments(p)
    own, rest = p.parse_known_args(argv)
    if own.out is None:
        raise SystemExit("--out FILE is required: where the map goes")
    if own.dpc is None:
        raise SystemExit("--dpc K with --dpc_iso ISO or --dpc_noise a,b / auto is required: the rule whose persistence is counted")
    check_detect_flags(own.frames, own.share, own.tolerate)
    opt = parse(rest)
    rule = dpc_arguments(own.dpc, own.dpc_dead, own.dpc_iso, own.dpc_noise, int(opt.bit_depth), own.dpc_noise_frames)
    dataset = open_rawvideo(opt, rest, "dpc_map")
    dev = torch.device("cuda", opt.gpu_ids[0] if opt.gpu_ids else 0)
    if rule.needs_curve:
        rule = rule.with_curve(*estimate_noise(dataset, dev, int(opt.bit_depth), own.dpc_noise_frames or 4))
    rt = ops_runtime(dev.index or 0)
    try:
        hits, read = detect(rt, dataset, int(opt.bit_depth), rule.cfg(), own.frames, own.tolerate)
        mask, r = report(hits, read, own.share, own.tolerate)
    except RuntimeError as err:
        raise SystemExit(str(err))
    write_map(own.out, mask)
    print(format_line(r))
    return r


if __name__ == '__main__':
    main()
