"""The sensor's noise curve from the footage itself:
`python -m rvdd_release_amd.noise --dataroot D --nFolder noisy --bit_depth 12 [--frames K] [--match_iso ISO] [container flags of denoise]`.

Reads the tree `denoise` reads (`--dataset_mode rawvideo`: uint16 / float32 mosaics or packed frames, TIFFs of packed 10 / 12 / 14-bit
samples, or with `--raw_container mipi --raw_size WxH` headerless MIPI CSI-2 frames), ingests the first K frames (default 4) of up
to 16 videos on the device through the calls `denoise` uses (`rvdd_ingest_raw` / `rvdd_ingest_bits`), gathers the 8 x 8 block
statistics of their packed planes (`rvdd_noise_hist`) and fits var(m) = a * m - b in DN of --bit_depth (`rvdd_noise_fit`; the rule
is in include/rvdd.h).  Prints one JSON line:

    {"a": ..., "b": ..., "bins": ..., "blocks": ..., "clipped": ..., "rms": ..., "m_min": ..., "m_max": ..., "frames": ...,
     "nearest_iso": ..., "ratio_20_45_80": [...]}

a and b with 17 significant digits, so that `denoise --dpc K --dpc_noise a,b` gets exactly the numbers `--dpc_noise auto` uses;
clipped: the share of the blocks seen that touch 0 or the top of the range; rms: the weighted RMS of the relative residuals of the
fit; nearest_iso: which of the two checkpoint families' curves (ISO 3200 / 12800 of the reference's synthetic camera, rescaled to
--bit_depth) predicts the closest standard deviation at 20 / 45 / 80 % of the range, and the ratios estimate / that curve there.

With `--match_iso ISO` (3200 / 12800) a second line follows, the one `denoise --match_noise a,b --match_iso ISO` prints:

    match: {"scale": ..., "offset": ..., "s": ..., "t_dn12": ..., "iso": ...}

the affine map v' = scale * v + offset on samples in [-1,1] that takes the estimated curve onto that checkpoint family's
(`rvdd_match_coeffs`; x' = s x + t_dn12 in 12-bit DN), every number with 17 digits.  s > 1: the footage is cleaner than the curve and
the map stretches it beyond the trained range.

The estimate assumes ONE camera setting -- one gain, one curve -- for everything it reads: footage of several gains in one tree gives
a curve of none of them.  Texture only ever raises a block's variance and the fit reads the lower quartile, so a busy scene comes out
a few per cent high in sigma, the safe side for --dpc.  Footage with too little tonal range is refused with the
fit's message.
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from .footage import MAX_VIDEOS, ingest_frames, open_rawvideo
from .runtime import DPC_ISO_CURVES, NOISE_ACC_BYTES, match_coeffs, nearest_iso, noise_acc_arrays, noise_fit


def estimate(rt, dataset, bit_depth: int, frames: int = 4, max_videos: int = MAX_VIDEOS):
    """The accumulator (a device tensor, `RvddRuntime.noise_hist`) of the first `frames` frames of the first `max_videos` videos of a
    rawvideo dataset, ingested on `rt`'s device as `video_push` ingests them.  -> (acc, frames read).  Nothing is synchronised."""
    acc = torch.zeros(NOISE_ACC_BYTES // 4, dtype=torch.int32, device=rt._tdev)
    read = 0
    for _, paths in dataset.videos[:max_videos]:
        paths = paths[:max(1, int(frames))]
        packed, _ = ingest_frames(rt, dataset, np.stack([dataset.read_frame(p) for p in paths]), bit_depth, want_gray=False)
        rt.noise_hist(packed, int(bit_depth), acc)
        read += len(paths)
    return acc, read


def report(acc, bit_depth: int, frames: int) -> dict:
    """noise_fit of the accumulator with what the command prints beside it; RuntimeError with the fit's message where it refuses"""
    fit = noise_fit(acc, bit_depth)
    counters = noise_acc_arrays(acc)["counters"]
    iso, ratios = nearest_iso(fit["a"], fit["b"], bit_depth)
    fit.update(clipped=float(counters[1]) / max(int(counters[0]), 1), frames=int(frames), nearest_iso=iso, ratios=ratios)
    return fit


def format_line(r: dict) -> str:
    """the JSON line: a and b as %.17g, which float() reads back to the same doubles"""
    return ('{"a": %.17g, "b": %.17g, "bins": %d, "blocks": %d, "clipped": %.6g, "rms": %.6g, "m_min": %.8g, "m_max": %.8g, "frames": %d, '
            '"nearest_iso": %d, "ratio_20_45_80": [%s]}'
            % (r["a"], r["b"], r["bins"], r["blocks"], r["clipped"], r["rms"], r["m_min"], r["m_max"], r["frames"], r["nearest_iso"],
               ", ".join("%.4f" % v for v in r["ratios"])))


def format_match_line(cfg, s: float, t: float, iso: int) -> str:
    """the JSON of the `match:` line: what `runtime.match_coeffs` returned, every number as %.17g"""
    return '{"scale": %.17g, "offset": %.17g, "s": %.17g, "t_dn12": %.17g, "iso": %d}' % (cfg.scale, cfg.offset, s, t, iso)


def main(argv=None) -> dict:
    from .options import parse
    from .util._ops import ops_runtime
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--frames', type=int, default=4, help='frames read per video (the first ones)')
    p.add_argument('--match_iso', type=int, default=None, help="also print the map onto this checkpoint family's curve (3200 / 12800)")
    own, rest = p.parse_known_args(argv)
    if own.frames < 1:
        raise SystemExit("--frames must be >= 1, got %d" % own.frames)
    if own.match_iso is not None and own.match_iso not in DPC_ISO_CURVES:
        raise SystemExit("--match_iso must be one of %s, got %r" % (', '.join(str(k) for k in DPC_ISO_CURVES), own.match_iso))
    opt = parse(rest)
    dataset = open_rawvideo(opt, rest, "noise")
    rt = ops_runtime(opt.gpu_ids[0] if opt.gpu_ids else 0)
    acc, read = estimate(rt, dataset, int(opt.bit_depth), own.frames)
    try:
        r = report(acc, int(opt.bit_depth), read)
    except RuntimeError as err:
        raise SystemExit(str(err))
    print(format_line(r))
    if own.match_iso is not None:
        try:
            cfg, s, t = match_coeffs(r["a"], r["b"], int(opt.bit_depth), own.match_iso)
        except RuntimeError as err:
            raise SystemExit(str(err))
        print('match: ' + format_match_line(cfg, s, t, own.match_iso))
        r["match"] = {"scale": cfg.scale, "offset": cfg.offset, "s": s, "t_dn12": t, "iso": own.match_iso}
    return r


if __name__ == '__main__':
    main()
