"""Denoise raw footage: `python -m rvdd_release_amd.denoise --dataroot D --nFolder noisy --results_dir R <model flags>`.

Reads `<dataroot>/<nFolder>/<video>/<frame>.tif` (`--dataset_mode rawvideo`: sensor frames as 1-channel mosaics or
4-channel packed frames, uint16 or float32; no ground truth, no flow folder) -- or frames of packed 10 / 12 / 14-bit samples,
which go to the device as they lie (`RvddRuntime.video_push(container=...)`): TIFFs with BitsPerSample = --bit_depth, or with
`--raw_container mipi --raw_size WxH` headerless `<frame>.raw` files of MIPI CSI-2 RAW<bit_depth> rows -- and writes, for every frame the reference's
test-time dataset yields (frames 1 .. N-1-future of a video of N frames; every frame with --all_frames),

    <results_dir>/<video>/<frame>_denoised.tif

-- the float32 [H,W,3] image `validate.py` writes for that frame (`util.visualizer.save_images`).  Everything between
the file and the output frame runs on the device (`RvddRuntime.video_push`: ingest, TV-L1 flows, the frame-step;
`RvddRuntime.egress`: the file's samples, one call per push over all slots and one copy to the host).

The model flags are the reference's (`--netDenoiser --path2epoch / --checkpoints_dir --feature_rec --future_patch_depth
--no_warp --warp_raw --prev_noisy_frame --bayer_pattern --bit_depth --patch_depth --gpu_ids --val_flow_from_denoised`;
`options.parse`).  `--val_flow_from_denoised`: from a video's second output on, the flow towards the previous frame is matched
against the re-mosaicked previous OUTPUT instead of the previous noisy frame (option "stream_flow_from_denoised").  Beside them:
  --results_dir DIR   where the frames go (default ./results)
  --batch_size B      B videos advance in lockstep: the videos are dealt to B slots in order, a slot whose video ended
                      takes the next unstarted one, or idles when none is left (`deal_slots`).  Same files, same bytes.
  --srgb ISO,n,red_gain,blue_gain   also write <frame>_srgb.png: the display image of dataset/fwd_ppipe.py for that ISO and
                      white balance (rgb_gain = 1/n), `rvdd_ppipe` on the network output.
  --out_format F      f32 (default): the file above.  rgb16 / mosaic16 / packed16: <results_dir>/<video>/<frame>.tif under the
                      input frame's own base name, uint16 digital numbers as [H,W,3] linear RGB / the [H,W] mosaic in
                      --bayer_pattern / the packed [H/2,W/2,4] frame (`rvdd_egress`) -- the results directory is then itself a
                      --dataroot/--nFolder tree that `--dataset_mode rawvideo` reads (mosaic16, packed16).
                      mosaic_msb: that mosaic as <frame>.tif with BitsPerSample = --out_bit_depth (10 / 12 / 14), the samples
                      bit-packed as TIFF stores them (`rvdd_egress_bits`) -- again a tree `denoise` reads; mosaic_mipi: the same
                      samples as headerless <frame>.raw of MIPI CSI-2 RAW10 / 12 / 14 rows (read back with --raw_container mipi).
  --out_bit_depth N   the digital numbers' bit depth (default: --bit_depth)
  --video_out V       y4m8 / y4m10: also write every video as ONE playable stream <results_dir>/<video>.y4m -- YUV4MPEG2, Y'CbCr 4:2:0 at 8
                      or 10 bits (`y4m.Y4MWriter`), which players and encoders read.  Per push and for all slots at once: the display
                      image of --video_render (`rvdd_ppipe`, its float image), BT.709 limited-range Y'CbCr with chroma averaged per
                      2 x 2 quad (`rvdd_ycbcr`), one copy to the host; the frames of a video are appended in order.  Under --cuts one
                      file per shot, <video>.<first frame of the shot>.y4m.  --all_frames decides, as for the other outputs, whether
                      a video's first and last frames are in the stream.  Needs
  --video_render ISO,n,red_gain,blue_gain   the four values of --srgb: the rendering is the reference's display pipeline with the
                      gains given here, not a colour-managed one.
  --video_fps N[:D]   the frame rate the header states (default 24).
  --out_format none   with --video_out: no per-frame file, and no egress launch or copy for one.
                      Without --video_out no new call is made and the output files keep their bytes.
  --all_frames        write EVERY input frame (option "stream_all_frames"): also frame 0 of a video -- denoised with itself as the
                      previous frame, a zero flow and a fresh recurrence; frame 1 then starts as always -- and, with a future frame,
                      the last frame, with itself as the next frame.  The files of frames 1 .. N-1-future keep their bytes.
  --dpc K             defective-pixel correction on the device, between the ingest and the frames the stream keeps (`rvdd_set_dpc`):
                      a sample that lies above the largest (hot) or below the smallest (dead, stuck low) of its eight same-colour
                      neighbours by more than K standard deviations of the noise at their median is replaced by that median; TV-L1
                      and the network see the corrected frames.  K = 4 flags about 1e-5 of the samples of defect-free noise
                      (DESIGN.md 4.14).  Needs exactly one of
  --dpc_iso ISO       the reference's noise curve of ISO 3200 / 12800, rescaled from 12 bits to --bit_depth, or
  --dpc_noise a,b[,floor]   the curve var = a * m - b in DN of the frames' own bit depth, and the least variance (default 1).
  --dpc_noise auto[,floor]  the curve estimated from the run's own footage before streaming starts (`rvdd_noise_hist`, `rvdd_noise_fit`;
                      python -m rvdd_release_amd.noise is the same estimate on its own): the first --dpc_noise_frames K (default 4)
                      frames of up to 16 of the videos.  Prints `noise: {"a": ..., "b": ..., ...}` -- a and b with 17 digits, so that
                      --dpc_noise a,b repeats the run exactly -- and which checkpoint family's curve lies nearest.
                      Assumes ONE camera setting (one gain) for all videos of the run; footage with too little tonal range is
                      refused: pass a,b then.
  --dpc_dead K        another threshold for the dead side; 0 switches that side off.
                      Prints, per video, `dpc: <hot> hot, <dead> dead samples corrected in <frames> frames`.  Without --dpc the
                      output files keep their bytes.
  --dpc_map FILE      correct the persistent defects of the sensor by a static map (`rvdd_set_dpc_map`): a one-sample image of the mosaic,
                      nonzero = defective (python -m rvdd_release_amd.dpc_map writes one; a camera's own calibration serves as well).
                      Every ingested frame has the map's samples, and only those, replaced by the middle value of their good same-colour
                      neighbours, clusters of any shape included; scene highlights are not touched.  Needs no --dpc; with --dpc the map
                      is applied first and the dynamic rule sees cleaned neighbours.
  --dpc_map auto      the map found in the run's own footage before streaming starts (`rvdd_dpc_detect`; python -m rvdd_release_amd.dpc_map
                      is the same pass on its own): --dpc_map_frames K (default 16) frames spread evenly over each of up to 16 videos,
                      a sample being defective where the rule of --dpc fired in at least --dpc_map_share (default 0.5) of them;
                      --dpc_map_tolerate t (0..3, default 0) for clusters in flat calibration footage.
  --dpc_static_only   with --dpc_map auto: --dpc only names the detection rule, the dynamic stage stays off.
                      Prints `dpc_map: N samples in M cells, U unfixable, from F frames` (or `from FILE`).  Limits: a tripod shot of a
                      static scene gives the map the dynamic rule's false alarms, since nothing moves -- no worse than --dpc; one
                      camera (one frame size, one map) per run; NOTHING is measured on real footage.  Without the
                      flags no new call is made and the output files keep their bytes.
  --match_noise a,b   map the footage onto the checkpoint's noise curve (`rvdd_set_match`): a,b is the footage's curve var = a * m - b in
                      DN of --bit_depth.  The kept frames are mapped by x' = s x + t with s = a_ref / a (in 12-bit DN) behind the ingest
                      and the correction of --dpc, which keeps the sensor's curve; the outputs are mapped back, so every output format
                      stays in the sensor's range; flows are matched on the sensor's own planes.  Needs
  --match_iso ISO     the checkpoint's family, 3200 or 12800: the curve it was trained on.  Either flag without the other is an error.
  --match_noise auto  the curve estimated from the footage as --dpc_noise auto estimates it (--dpc_noise_frames frames per video,
                      default 4); with both on auto one estimate and one `noise:` line serve both.
                      Prints `match: {"scale": ..., "offset": ..., "s": ..., "t_dn12": ..., "iso": ...}` with 17 digits.  Footage
                      noisier than the curve (s < 1, low light) is what the map is for: +3.5 to +4.6 dB on the synthetic camera.
                      Footage cleaner than the curve (s > 1) is stretched beyond the trained range and can LOSE quality: a warning
                      says so (DESIGN.md 4.16 has the table).  Without the flags the output files keep their bytes.
  --cuts auto         a folder need not be one shot: before the first push every frame of the run is measured on the device (one 6 KiB
                      integer signature per frame, `rvdd_frame_sigs`; python -m rvdd_release_amd.cuts is the same pass on its own) and
                      every video is split where consecutive frames differ by more than --cut_hist T (default 0.10: the share of cells
                      whose level bin changed) or --cut_grid T (default 0.12: the share of the 16 x 16 layout that moved).  Each shot is
                      then streamed as a video of its own under the SAME key: a fresh recurrence and no flow across the cut, the files in
                      the same folder under the frames' own names -- byte for byte the run on a tree in which every shot is its own
                      folder.  --cut_min_len L (default 4, at least 2 + future): cuts that would leave a shorter shot are dropped.
                      Prints `cuts: <key>: N frames, shots at [0, k1, ...]` per video; `dpc:` lines are then per shot and name its first
                      frame.  Without --all_frames the first frame and the last `future` frames of every SHOT are not written, as for
                      any video: pass --all_frames with --cuts.  The pass reads every frame a second time;
  --cuts FILE         reads the lines python -m rvdd_release_amd.cuts printed (`{"video": key, "frames": N, "cuts": [k, ...]}`) instead.
                      A key that is not in the run, or a cut outside 1 .. N-1, is an error that names it.
                      The thresholds rest on synthetic scenes of 128 x 192 cells and more; NOTHING is measured on
                      real footage.  Look-alike shots and fades are not found, which leaves today's behaviour.  --dpc_noise auto still
                      reads the first frames of every FOLDER.  Without --cuts no new call is made and the output files keep their bytes.
  --row_noise K       take row noise (horizontal banding that flickers: one readout offset per mosaic row and frame) out of every frame
                      on the device (`rvdd_set_rows`), behind --dpc_map / --dpc and in front of --match_noise: per frame, row parity and
                      plane row one offset is the median, over the row's two colour planes, of every sample's difference to the median
                      of its eight vertical same-colour neighbours; samples further than K standard deviations of the noise curve from
                      that median (edges, texture, defects) are left out, a row with fewer than half of its samples left is not touched.
                      K is around 3.  TV-L1, the network and --report see the corrected frames.  Prints, per video (per shot under
                      --cuts), `rows: <applied> applied, <skipped> skipped, <clamped> clamped rows, rms offset <x> DN (the estimate
                      alone, on flat footage without row noise: <y> DN)`: y = 1.35 sqrt(var(mid level) / (2 ww)) is what the estimate
                      finds in white noise; footage whose x sits at or near y has no row noise, and the flag should stay off -- it
                      then only adds y.  About 0.4 of the offsets' amplitude stays behind as a slow vertical drift (the neighbours carry
                      offsets too); rows crossed by a long horizontal edge are skipped or biased by less than the gate; column pattern
                      noise is not touched; NOTHING is measured on real footage.
  --row_noise_curve C the sensor's curve in DN of --bit_depth: a,b[,floor], auto (the run's own estimate, shared with --dpc_noise auto),
                      iso3200 or iso12800.  Default: the curve of --dpc; without either it is an error.
  --row_noise_max DN  the largest offset taken out (default (2^bit_depth - 1) / 64, a guess).
                      Without --row_noise no new call is made and the output files keep their bytes.
  --col_noise FILE    take column fixed-pattern noise (vertical stripes that stay put: one readout offset per mosaic column, the same in
                      every frame) out of every frame on the device (`rvdd_set_cols`), behind --dpc_map / --dpc and in front of
                      --row_noise and --match_noise: FILE is a one-row float32 TIFF of one offset per mosaic column in DN of --bit_depth
                      (python -m rvdd_release_amd.col_noise writes one; a camera's own calibration serves as well).  Columns whose
                      offset is 0 keep their bits.  TV-L1, the network and --report see the corrected frames.
  --col_noise auto    the map found in the run's own footage before streaming starts (`rvdd_cols_estimate`, `rvdd_cols_fit`; python -m
                      rvdd_release_amd.col_noise is the same pass on its own): --col_noise_frames F (default 32) frames spread evenly
                      over up to 16 videos; per frame and column the median, over the column's two colour planes, of every sample's
                      difference to the median of its eight horizontal same-colour neighbours, samples further than --col_noise_gate K
                      (default 3) standard deviations of the noise curve left out; per column the median over the frames, taken only
                      where at least half of the frames gave an estimate and it is at least --col_noise_sigma (default 3) standard
                      errors of itself, measured from the column's own spread over the frames; --col_noise_max DN is the largest
                      offset taken out (default (2^bit_depth - 1) / 64, a guess).
  --col_noise_curve C with --col_noise auto, the sensor's curve in DN of --bit_depth: a,b[,floor], auto (the run's own estimate, shared
                      with --dpc_noise auto), iso3200 or iso12800.  Default: the curve of --dpc; without either it is an error.
                      Prints `cols: <applied> applied, <insignificant> insignificant, <unsupported> unsupported, <clamped> clamped of
                      <n> columns, map rms <x> DN (the pooled estimate alone: <y> DN), from F frames` (or what a FILE holds).  Limits: the
                      neighbours carry offsets too, so slow horizontal shading of the pattern stays; in a tripod shot of a static scene
                      a vertical edge passes the significance test, since its spread over time is only noise -- estimate on footage
                      that moves; one camera setting per run; offsets per plane and per-column gains are not modelled; NOTHING is
                      measured on real footage.  Without --col_noise no new call is made and the output files keep
                      their bytes.
  --green_eq FILE     balance the two green planes (the green sites of the red rows and of the blue rows see the same light through
                      different neighbours; crosstalk makes them differ by up to a few per cent, slowly over the field and the same in
                      every frame; Hamilton-Adams turns that into a maze pattern) of every frame on the device (`rvdd_set_green`),
                      behind --dpc_map / --dpc, --col_noise and --row_noise and in front of --match_noise: FILE is a one-sample float32
                      TIFF of one gain per block of 32 x 32 cells, or one value (python -m rvdd_release_amd.green_eq writes one).  It
                      needs the level without signal: --green_eq_black DN, or b / a of --green_eq_curve or of the curve of --dpc.
                      Cells whose gain is 0 keep their bits.  TV-L1, the network and --report see the corrected frames.
  --green_eq auto     the map found in the run's own footage before streaming starts (`rvdd_green_estimate`, `rvdd_green_fit`; python -m
                      rvdd_release_amd.green_eq is the same pass on its own): --green_eq_frames F (default 32) frames spread evenly
                      over up to 16 videos; per frame and block either green plane's samples against the middle of their four diagonal
                      neighbours of the other plane, samples further than --green_eq_gate K (default 3) standard deviations of the
                      noise curve left out; per block the median over the frames of the difference over the level above black, taken
                      only where at least half of the frames gave an estimate at a level of --green_eq_min_signal DN (default
                      (2^bit_depth - 1) / 64, a guess) above black and it is at least --green_eq_sigma (default 3) standard errors of
                      itself; --green_eq_max (default 0.10) is the largest gain taken out; --green_eq_field map (default) | flat takes
                      one gain per block, or the one pooled over the blocks.
  --green_eq_curve C  the sensor's curve in DN of --bit_depth: a,b[,floor], auto (the run's own estimate, shared with --dpc_noise auto),
                      iso3200 or iso12800.  Default: the curve of --dpc; without either it is an error under auto.
                      Prints `green: <applied> applied, <insignificant> insignificant, <unsupported> unsupported, <clamped> clamped of
                      <n> blocks, map rms gain <x> (the pooled estimate alone: <y>), flat estimate <g> +- <se> (<state>), ...` (or what a
                      FILE holds).  Limits: the gate is centred on zero, so an imbalance shrinks by about phi(K) / phi(0) of itself
                      (a prototype recovered 0.93 - 0.95 of an injected 1 - 5 %; 0.63 - 0.72 on dark-heavy `synth` blocks); texture finer than two cells aliases; one camera,
                      lens and aperture per map; NOTHING is measured on real footage.  A map in which no block is
                      significant leaves every byte of the output alone; without --green_eq no new call is made.
  --report FILE       check the outputs without ground truth: if the output is the clean frame, noisy - remosaic(denoised) is the noise.
                      The stream reduces every output and its (corrected, matched) centre frame to residual statistics on the device
                      (`rvdd_set_resid`), read at the end of every video -- of every shot under --cuts -- and judged against a noise curve
                      (`rvdd_resid_fit`).  FILE gets one JSON line per video: {"video": key, "frames": N, "ratio", "ratio_lo", "ratio_hi",
                      "bias", "rho", "a_fit", "b_fit", "samples", "bins", "curve": {"a", "b", "bit_depth", "source"}} (under --cuts also
                      "from": the shot's first frame).  ratio = measured / predicted variance of the residual (lo / hi: the darkest / brightest
                      third): below the baseline means noise left in, or a curve that is too high; above it WITH a positive rho (the
                      correlation of horizontal neighbours of one colour) means detail removed; bias (DN) is a level shift.  The baseline
                      is not 1: DESIGN.md 4.19 has the measured table, and says what the numbers separate and what they do not.
                      The curve: with --match_noise the checkpoint family's (--match_iso), in the 12-bit DN the network sees; otherwise
  --report_noise C    a,b in DN of --bit_depth, auto (the run's own estimate, shared with --dpc_noise auto), iso3200 or iso12800.
                      Required without --match_noise.  Prints one `report:` line with the totals over all videos at the end.
                      Without --report no new call is made and the output files keep their bytes.
Videos of different frame sizes are grouped by size and run one group after the other, one runtime per size.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import tiffio
from .footage import (FileSpec, add_cols_arguments, add_dpc_arguments, add_green_arguments, add_report_arguments, add_rows_arguments,
                      cols_arguments, dpc_arguments, estimate_noise, green_arguments, match_arguments, open_rawvideo, report_arguments,
                      report_record, rows_arguments, rows_line, to_device)
from .y4m import Y4MWriter
from .runtime import BAYER_PATTERNS, BITS_DEPTHS, bits_row_bytes, green_grid, match_coeffs, resid_add

# --dpc_map auto and --cuts auto, kind "auto"; their FILE forms are a FileSpec, kind "file"
DpcMapAuto = NamedTuple("DpcMapAuto", [("kind", str), ("frames", int), ("share", float), ("tolerate", int)])
CutsAuto = NamedTuple("CutsAuto", [("kind", str), ("t_hist", float), ("t_grid", float), ("min_len", int)])
# --video_out with --video_render and --video_fps: sample depth, (ISO, n, red_gain, blue_gain), (fps numerator, denominator)
VideoOut = NamedTuple("VideoOut", [("depth", int), ("render", tuple), ("fps", tuple)])
VIDEO_OUTS = {"y4m8": 8, "y4m10": 10}

NEXT, FIRST, IDLE = _lib.PUSH_NEXT, _lib.PUSH_FIRST, _lib.PUSH_IDLE
# --out_format -> (layout of RvddRuntime.egress, sample type, file suffix); f32 is the reference's image: 8-bit scale, float32
OUT_FORMATS = {"f32": ("rgb_hwc", torch.float32, "_denoised.tif"), "rgb16": ("rgb_hwc", torch.int16, ".tif"),
               "mosaic16": ("mosaic", torch.int16, ".tif"), "packed16": ("packed_hwc", torch.int16, ".tif"),
               # the mosaic's samples bit-packed (RvddRuntime.egress_bits): layout "bits", the order in the sample type's place
               "mosaic_msb": ("bits", "msb", ".tif"), "mosaic_mipi": ("bits", "mipi", ".raw")}


def deal_slots(lengths: Sequence[int], slots: int, tail: int = 0) -> List[List[Tuple[int, int, int]]]:
    """The pushes of videos of `lengths` frames on `slots` batch slots: a list of steps, each a list of one
    (ctl, video, frame) per slot.  The videos are dealt in order; a slot whose video ended takes the next unstarted
    video (FIRST on its frame 0), or goes IDLE -- (IDLE, -1, -1) -- when none is left; the list ends with the last step
    that carries a frame.  Every frame of every video appears once, in order, and NEXT never follows IDLE.
    tail=1 (option "stream_all_frames" with a future frame): a slot whose video v of N frames has ended first sits out one
    step, returned as (IDLE, v, N) -- the push that outputs the video's last frame -- and the list ends with the last such step."""
    if slots < 1:
        raise ValueError("deal_slots: at least one slot")
    if any(n < 1 for n in lengths):
        raise ValueError("deal_slots: a video has at least one frame")
    nxt = 0                                   # the next unstarted video
    cur = [(-1, 0)] * slots                   # per slot: (video, frames already pushed)
    steps = []
    while True:
        step = []
        for b in range(slots):
            v, k = cur[b]
            if v >= 0 and k < lengths[v]:
                step.append((NEXT, v, k))
                cur[b] = (v, k + 1)
            elif v >= 0 and tail:
                step.append((IDLE, v, k))
                cur[b] = (-1, 0)
            elif nxt < len(lengths):
                step.append((FIRST, nxt, 0))
                cur[b] = (nxt, 1)
                nxt += 1
            else:
                step.append((IDLE, -1, -1))
                cur[b] = (-1, 0)
        if all(v < 0 for _, v, _ in step):
            return steps
        steps.append(step)


def dpc_map_arguments(dpc_map, frames, share, tolerate, static_only, have_dpc):
    """--dpc_map / --dpc_map_frames / --dpc_map_share / --dpc_map_tolerate / --dpc_static_only -> None (no --dpc_map), a FileSpec or a
    DpcMapAuto; `have_dpc`: --dpc K was given.  SystemExit where the flags do not fit together."""
    from .dpc_map import check_detect_flags
    given = [n for n, v in (("dpc_map_frames", frames), ("dpc_map_share", share), ("dpc_map_tolerate", tolerate)) if v is not None]
    if dpc_map is None:
        if given or static_only:
            raise SystemExit("--dpc_map_frames, --dpc_map_share, --dpc_map_tolerate and --dpc_static_only belong to --dpc_map auto")
        return None
    if dpc_map != "auto":
        if given:
            raise SystemExit("--%s belongs to --dpc_map auto: --dpc_map %s reads a map that is already made" % (given[0], dpc_map))
        if static_only:
            raise SystemExit("--dpc_static_only belongs to --dpc_map auto: with --dpc_map FILE leave --dpc away to keep the dynamic stage off")
        return FileSpec("file", dpc_map)
    if not have_dpc:
        raise SystemExit("--dpc_map auto needs --dpc K with --dpc_iso ISO or --dpc_noise a,b / auto: the rule whose persistence is counted "
                         "(--dpc_static_only keeps the dynamic stage itself off)")
    frames, share, tolerate = 16 if frames is None else frames, 0.5 if share is None else share, 0 if tolerate is None else tolerate
    check_detect_flags(frames, share, tolerate, "--dpc_map_")
    return DpcMapAuto("auto", int(frames), float(share), int(tolerate))


def find_dpc_map(dataset, dev, opt):
    """--dpc_map: the run's map as a cellmask uint8 [hh,ww], its `dpc_map: N samples in M cells, U unfixable, from ...` line sent to the
    log.  auto: `dpc_map.detect` on the run's own videos with the rule of --dpc, before any push."""
    from . import dpc_map as M
    from .util._ops import ops_runtime
    spec = opt.dpc_map
    try:
        if spec.kind == "file":
            mask = M.read_map(spec.path)
            print(M.summary_line(mask, spec.path))
            return mask
        hits, read = M.detect(ops_runtime(dev.index or 0), dataset, int(opt.bit_depth), opt.dpc.cfg(), spec.frames, spec.tolerate)
        mask, _ = M.report(hits, read, spec.share, spec.tolerate)
    except (RuntimeError, tiffio.TiffError, OSError) as err:
        raise SystemExit("--dpc_map %s: %s" % ("auto" if spec.kind == "auto" else spec.path, err))
    print(M.summary_line(mask, '%d frames' % read))
    return mask


def match_report(a, b, bit_depth, iso):
    """The coefficients of --match_noise a,b --match_iso iso (`runtime.match_coeffs`), the `match:` line sent to the log, and the
    warning where the footage is cleaner than the checkpoint's curve.  -> struct rvdd_match_cfg"""
    from . import noise
    try:
        cfg, s, t = match_coeffs(a, b, bit_depth, iso)
    except RuntimeError as err:
        raise SystemExit("--match_noise: %s" % err)
    print('match: ' + noise.format_match_line(cfg, s, t, iso))
    if s > 1.0:
        print('match: WARNING: the footage is cleaner than the ISO %d checkpoints\' noise curve: matching stretches it by s = %.3f beyond '
              'the range the network was trained on, which can lose quality (DESIGN.md 4.16: the table of measured gains and losses)' % (iso, s))
    return cfg


def render_arguments(flag, word):
    """--srgb / --video_render ISO,n,red_gain,blue_gain -> (ISO, n, red_gain, blue_gain); SystemExit that names `flag` for anything else"""
    f = word.split(',')
    if len(f) != 4:
        raise SystemExit("%s takes ISO,n,red_gain,blue_gain" % flag)
    try:
        iso, gains = int(f[0]), tuple(float(v) for v in f[1:])
    except ValueError:
        raise SystemExit("%s takes ISO,n,red_gain,blue_gain: an integer and three numbers, got %r" % (flag, word))
    if not all(np.isfinite(g) and g != 0.0 for g in gains):
        raise SystemExit("%s: n, red_gain and blue_gain must be finite and not zero, got %r" % (flag, word))
    return (iso,) + gains


def video_arguments(video_out, render, fps):
    """--video_out / --video_render / --video_fps -> None (no --video_out) or a VideoOut; SystemExit where the flags do not fit together"""
    if video_out is None:
        if render is not None or fps is not None:
            raise SystemExit("--video_render and --video_fps belong to --video_out")
        return None
    if video_out not in VIDEO_OUTS:
        raise SystemExit("--video_out %r is not one of %s" % (video_out, ', '.join(VIDEO_OUTS)))
    if render is None:
        raise SystemExit("--video_out needs --video_render ISO,n,red_gain,blue_gain: the display rendering of the frames (the four values of --srgb)")
    f = ("24" if fps is None else fps).split(':')
    try:
        rate = (int(f[0]), int(f[1]) if len(f) == 2 else 1)
        if len(f) > 2 or min(rate) < 1:
            raise ValueError
    except ValueError:
        raise SystemExit("--video_fps takes N or N:D, positive integers, got %r" % fps)
    return VideoOut(VIDEO_OUTS[video_out], render_arguments("--video_render", render), rate)


def cuts_arguments(cuts, own, future):
    """--cuts / --cut_hist / --cut_grid / --cut_min_len -> None (no --cuts), a CutsAuto or a FileSpec;
    SystemExit where the flags do not fit together.  min_len is at least 2 + future: a shot that yields a frame."""
    from . import cuts as C
    given = [f for f in ("cut_hist", "cut_grid", "cut_min_len") if getattr(own, f) is not None]
    if cuts is None:
        if given:
            raise SystemExit("--cut_hist, --cut_grid and --cut_min_len belong to --cuts auto")
        return None
    if cuts == "auto":
        return CutsAuto("auto", *C.thresholds(own, 2 + int(future)))
    if given:
        raise SystemExit("--%s belongs to --cuts auto: --cuts %s reads cuts that are already decided" % (given[0], cuts))
    return FileSpec("file", cuts)


def read_cuts_file(path):
    """The lines `python -m rvdd_release_amd.cuts` printed -> {video key: [k, ...]}; other lines of a log are skipped; SystemExit for a
    file that cannot be read or a line that starts like one of them and is not."""
    found = {}
    try:
        with open(path) as f:
            lines = f.read().splitlines()
    except OSError as err:
        raise SystemExit("--cuts %s: %s" % (path, err))
    for no, line in enumerate(lines, 1):
        line = line.strip()
        if not line.startswith('{"video"'):
            continue
        try:
            rec = json.loads(line)
            key, cuts = rec["video"], [int(k) for k in rec["cuts"]]
            if not isinstance(key, str) or any(k != v for k, v in zip(cuts, rec["cuts"])):
                raise ValueError("a video is a string and a cut an integer")
        except (ValueError, KeyError, TypeError) as err:
            raise SystemExit('--cuts %s, line %d: not a {"video": ..., "frames": ..., "cuts": [...]} line (%s)' % (path, no, err))
        if key in found:
            raise SystemExit("--cuts %s, line %d: video %r appears twice" % (path, no, key))
        found[key] = cuts
    return found


def split_shots(videos, cuts_by_key):
    """videos [(key, [paths])] and {key: [k, ...]} -> the shots [(key, [paths of the shot])], in order: every video cut in front of its
    frames k -- each shot a video of its own under the SAME key, so that its files land in the video's folder under the frames' own
    names.  A video without an entry stays whole.  SystemExit that names it for a key that is not among the videos, and for an index
    outside 1 .. N-1."""
    keys = {key for key, _ in videos}
    for key in cuts_by_key:
        if key not in keys:
            raise SystemExit("--cuts: video %r is not in this run (its videos: %s)" % (key, ', '.join(sorted(keys))))
    shots = []
    for key, frames in videos:
        starts = [0]
        for k in sorted(set(cuts_by_key.get(key, ()))):
            if not 1 <= k <= len(frames) - 1:
                raise SystemExit("--cuts: video %r: cut %d is outside 1 .. %d (the video has %d frames)" % (key, k, len(frames) - 1, len(frames)))
            starts.append(k)
        for a, b in zip(starts, starts[1:] + [len(frames)]):
            shots.append((key, frames[a:b]))
    return shots


def find_cols_map(dataset, dev, opt):
    """--col_noise: the run's column map float32 [2,ww] in DN of --bit_depth, its `cols:` line sent to the log.  auto:
    `col_noise.estimate` on the run's own videos and the fit (`col_noise.report`), before any push."""
    from . import col_noise as M
    from .util._ops import ops_runtime
    spec = opt.cols
    try:
        if spec.kind == "file":
            cmap = M.read_map(spec.path)
            print(M.file_line(cmap, spec.path))
            return cmap
        offsets, state = M.estimate(ops_runtime(dev.index or 0), dataset, int(opt.bit_depth), spec.cfg(), spec.frames)
        cmap, r = M.report(offsets, state, spec.k_sig, spec.max_dn)
    except (RuntimeError, tiffio.TiffError, OSError) as err:
        raise SystemExit("--col_noise %s: %s" % ("auto" if spec.kind == "auto" else spec.path, err))
    print(M.summary_line(r, '%d frames' % r["frames"]))
    return cmap


def find_green_map(dataset, dev, opt):
    """--green_eq: the run's map of green gains float32 [gh,gw] (or [1,1]), its `green:` line sent to the log.  auto:
    `green_eq.estimate` on the run's own videos and the fit (`green_eq.report`), before any push."""
    from . import green_eq as M
    from .util._ops import ops_runtime
    spec = opt.green
    try:
        if spec.kind == "file":
            gmap = M.read_map(spec.path)
            print(M.file_line(gmap, spec.black_dn, spec.path))
            return gmap
        e, level, state = M.estimate(ops_runtime(dev.index or 0), dataset, int(opt.bit_depth), spec.cfg(), spec.frames, opt.bayer_pattern)
        gmap, r = M.report(e, level, state, spec.black_dn, spec.k_sig, spec.max_gain, spec.min_signal, spec.field)
    except (RuntimeError, tiffio.TiffError, OSError) as err:
        raise SystemExit("--green_eq %s: %s" % ("auto" if spec.kind == "auto" else spec.path, err))
    print(M.summary_line(r, '%d frames' % r["frames"]))
    return gmap


def find_shots(dataset, dev, opt):
    """--cuts: the run's videos as their shots (`split_shots`), one `cuts: <key>: N frames, shots at [0, k1, ...]` line per video sent to
    the log.  auto: `cuts.detect` on the run's own videos, before any push."""
    spec = opt.cuts
    if spec.kind == "auto":
        from . import cuts as C
        from .util._ops import ops_runtime
        t0 = time.time()
        found = C.detect(ops_runtime(dev.index or 0), dataset, dataset.videos, int(opt.bit_depth), spec.t_hist, spec.t_grid, spec.min_len)
        by_key = {key: cuts for key, _, cuts, _ in found}
        print('cuts: measured %d frames in %.3f s (--cuts FILE with the lines of python -m rvdd_release_amd.cuts saves the pass)'
              % (sum(n for _, n, _, _ in found), time.time() - t0))
    else:
        by_key = read_cuts_file(spec.path)
    shots = split_shots(dataset.videos, by_key)
    for key, frames in dataset.videos:
        print('cuts: %s: %d frames, shots at [%s]' % (key, len(frames), ', '.join(str(k) for k in [0] + sorted(set(by_key.get(key, ()))))))
    return shots


def _parse(argv):
    from . import cuts as C
    from .options import parse
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--cuts', type=str, default=None, help='auto: split every video at its scene cuts, found on the device before streaming '
                   'starts; FILE: at the cuts of the lines python -m rvdd_release_amd.cuts printed')
    C.add_arguments(p)
    p.add_argument('--results_dir', type=str, default='./results')
    p.add_argument('--srgb', type=str, default=None, help='ISO,n,red_gain,blue_gain: also write <frame>_srgb.png')
    p.add_argument('--out_format', type=str, default='f32', help=', '.join(OUT_FORMATS))
    p.add_argument('--out_bit_depth', type=int, default=None, help='bit depth of the sensor formats (default: --bit_depth)')
    p.add_argument('--video_out', type=str, default=None, help='y4m8, y4m10: also write every video as one Y4M stream <results_dir>/<video>.y4m')
    p.add_argument('--video_render', type=str, default=None, help='ISO,n,red_gain,blue_gain: the display rendering of --video_out (the values of --srgb)')
    p.add_argument('--video_fps', type=str, default=None, help='N or N:D: the frame rate the stream states (default 24)')
    p.add_argument('--all_frames', action='store_true', help='write every input frame, the first and the last of a video too')
    add_dpc_arguments(p)
    add_rows_arguments(p)
    add_cols_arguments(p)
    add_green_arguments(p)
    p.add_argument('--dpc_map', type=str, default=None, help='FILE: correct the sites of this defect map (python -m rvdd_release_amd.dpc_map '
                   'writes one); auto: find the map in the footage before streaming starts, with the rule of --dpc')
    p.add_argument('--dpc_map_frames', type=int, default=None, help='with --dpc_map auto: frames read per video, spread over it (default 16)')
    p.add_argument('--dpc_map_share', type=float, default=None, help='with --dpc_map auto: the share of those frames a defect fires in (default 0.5)')
    p.add_argument('--dpc_map_tolerate', type=int, default=None, help='with --dpc_map auto: 0..3 other defects among the neighbours (default 0)')
    p.add_argument('--dpc_static_only', action='store_true', help='with --dpc_map auto: --dpc only names the detection rule, the dynamic stage stays off')
    p.add_argument('--match_noise', type=str, default=None, help="a,b: the footage's curve var = a * m - b in DN of the frames, mapped onto "
                   'the curve of --match_iso; auto: estimated from the footage')
    p.add_argument('--match_iso', type=int, default=None, help="the checkpoint family's noise curve: 3200 or 12800")
    add_report_arguments(p)
    own, rest = p.parse_known_args(argv)
    if own.out_format not in OUT_FORMATS and own.out_format != "none":
        raise SystemExit("--out_format %r is not one of %s" % (own.out_format, ', '.join(OUT_FORMATS)))
    opt = parse(rest)
    opt.results_dir, opt.srgb, opt.out_format, opt.all_frames = own.results_dir, own.srgb, own.out_format, own.all_frames
    opt.out_bit_depth = int(opt.bit_depth) if own.out_bit_depth is None else own.out_bit_depth
    if not 1 <= opt.out_bit_depth <= 16:
        raise SystemExit("--out_bit_depth must be 1..16, got %d" % opt.out_bit_depth)
    opt.video = video_arguments(own.video_out, own.video_render, own.video_fps)
    if opt.out_format == "none" and opt.video is None:
        raise SystemExit("--out_format none writes no per-frame file: it needs --video_out %s" % ' | '.join(VIDEO_OUTS))
    if opt.out_format != "none" and OUT_FORMATS[opt.out_format][0] == "bits" and opt.out_bit_depth not in BITS_DEPTHS:
        raise SystemExit("--out_format %s needs --out_bit_depth (default: --bit_depth) 10, 12 or 14, got %d" % (opt.out_format, opt.out_bit_depth))
    opt.dpc = dpc_arguments(own.dpc, own.dpc_dead, own.dpc_iso, own.dpc_noise, int(opt.bit_depth), own.dpc_noise_frames)
    opt.dpc_noise_frames = 4 if own.dpc_noise_frames is None else own.dpc_noise_frames
    opt.dpc_map = dpc_map_arguments(own.dpc_map, own.dpc_map_frames, own.dpc_map_share, own.dpc_map_tolerate, own.dpc_static_only,
                                    opt.dpc is not None)
    opt.dpc_static_only = own.dpc_static_only
    opt.rows = rows_arguments(own.row_noise, own.row_noise_curve, own.row_noise_max, opt.dpc, int(opt.bit_depth))
    opt.cols = cols_arguments(own.col_noise, own.col_noise_curve, own.col_noise_frames, own.col_noise_gate, own.col_noise_sigma,
                              own.col_noise_max, opt.dpc, int(opt.bit_depth))
    opt.green = green_arguments(own.green_eq, own.green_eq_curve, own.green_eq_field, own.green_eq_frames, own.green_eq_gate, own.green_eq_sigma,
                                own.green_eq_max, own.green_eq_min_signal, own.green_eq_black, opt.dpc, int(opt.bit_depth))
    opt.match = match_arguments(own.match_noise, own.match_iso)
    opt.report = report_arguments(own.report, own.report_noise, opt.match, int(opt.bit_depth))
    opt.cuts = cuts_arguments(own.cuts, own, opt.future_patch_depth)
    opt.cols_map = None                           # the column map of --col_noise: `prepasses` leaves it here
    opt.green_map = None                          # the map of green gains of --green_eq, likewise
    if opt.raw_container is not None:
        if opt.raw_container != 'mipi':
            raise SystemExit("--raw_container %r: headerless frames are 'mipi' (packed TIFFs are recognised by themselves)" % opt.raw_container)
        if opt.raw_size is None:
            raise SystemExit("--raw_container mipi needs --raw_size WxH")
        if int(opt.bit_depth) not in BITS_DEPTHS:
            raise SystemExit("--raw_container mipi needs --bit_depth 10, 12 or 14, got %d" % int(opt.bit_depth))
    if not any(a == '--dataset_mode' or a.startswith('--dataset_mode=') for a in rest):
        opt.dataset_mode = 'rawvideo'
    if opt.srgb is not None:
        opt.srgb = render_arguments("--srgb", opt.srgb)
    return opt


def prepasses(opt, dataset, dev):
    """What is decided on the run's own footage before any push, in this order: the noise curve of the stages on `auto` (ONE estimate
    for --dpc_noise, --row_noise_curve, --col_noise_curve, --green_eq_curve, --match_noise and --report_noise, made for the first that
    asks), the defect map, the column map, the map of green gains, the match coefficients, the shots.  Completes the records opt.dpc,
    opt.rows, opt.cols, opt.green, opt.match and opt.report, leaves the maps of --col_noise and --green_eq in opt.cols_map and opt.green_map; -> (dmap: the cellmask or None, match: struct rvdd_match_cfg or
    None, shots [(key, [paths])])."""
    found = []

    def auto(flag):
        """the run's ONE estimate: whoever asks first is named where the fit refuses"""
        if not found:
            found.append(estimate_noise(dataset, dev, int(opt.bit_depth), opt.dpc_noise_frames, flag))
        return found[0]

    for stage, flag in (("dpc", '--dpc_noise'), ("rows", '--row_noise_curve'), ("cols", '--col_noise_curve'), ("green", '--green_eq_curve')):
        spec = getattr(opt, stage, None)
        if getattr(spec, "needs_curve", False):     # auto, or the curve of --dpc_noise auto; a stage that is off, or reads a FILE, has none
            setattr(opt, stage, spec.with_curve(*auto(flag)))
    # --dpc_map: ONE map for the run, read or found before any push; --dpc_static_only: --dpc has named the rule and is done
    dmap = None if opt.dpc_map is None else find_dpc_map(dataset, dev, opt)
    # --col_noise: ONE column map for the run, read or found before any push
    opt.cols_map = None if opt.cols is None else find_cols_map(dataset, dev, opt)
    # --green_eq: ONE map of green gains for the run, read or found before any push
    opt.green_map = None if getattr(opt, "green", None) is None else find_green_map(dataset, dev, opt)
    if opt.dpc_static_only:
        opt.dpc = None
    match = None
    if opt.match is not None:
        if opt.match.needs_curve:
            opt.match = opt.match.with_curve(*auto('--match_noise'))
        match = match_report(opt.match.a, opt.match.b, int(opt.bit_depth), opt.match.iso)
    if opt.report is not None and opt.report.needs_curve:
        opt.report = opt.report.with_curve(*auto('--report_noise'))
    # --cuts: every shot is a video of its own from here on, under its video's key
    shots = dataset.videos if opt.cuts is None else find_shots(dataset, dev, opt)
    return dmap, match, shots


def write_frame(opt, rt, out_b, host_b, key, path, W):
    """One output frame to <results_dir>/<key>/: the file of --out_format from `host_b`, the frame's samples on the host, under the base
    name of `path`, and with --srgb the display image of `out_b`, the network output [1,3,H,W] on the device."""
    from .library import iio_write
    from .util import util
    if opt.out_format == "none" and opt.srgb is None:      # --video_out alone: no per-frame file, no folder for one
        return
    layout, sample, suffix = OUT_FORMATS.get(opt.out_format, (None, None, None))
    stem = os.path.splitext(os.path.basename(path))[0]
    util.mkdir(os.path.join(opt.results_dir, key))
    if layout is None:
        pass
    elif layout != "bits":
        iio_write(host_b, os.path.join(opt.results_dir, key, stem + suffix))
    elif sample == "msb":
        tiffio.write_packed(os.path.join(opt.results_dir, key, stem + suffix), host_b, W, opt.out_bit_depth)
    else:
        host_b.tofile(os.path.join(opt.results_dir, key, stem + suffix))
    if opt.srgb is not None:
        iso, n, red, blue = opt.srgb
        png = rt.ppipe(out_b, 1.0 / n, red, blue, iso, _lib.PPIPE_FROM_NET, "nchw")
        iio_write(png[0].cpu().numpy(), os.path.join(opt.results_dir, key, stem + '_srgb.png'))


def shot_name(key, first):
    """what the `dpc:` and `rows:` lines call a video, or the shot of it that starts with the frame `first`"""
    return key if first is None else '%s from %s' % (key, first)


def run_group(opt, model, dataset, videos, H, W, dmap, match, report_out=None) -> int:
    """`push_group`, and the streams of --video_out that a refusal or an error in the middle of a video left open closed on the way out"""
    writers = {}                                # slot -> the open Y4MWriter of its video (of its shot under --cuts)
    try:
        return push_group(opt, model, dataset, videos, H, W, dmap, match, report_out, writers)
    finally:
        for w in writers.values():
            w.close()


def push_group(opt, model, dataset, videos, H, W, dmap, match, report_out, writers) -> int:
    """The videos [(key, [paths])] of one frame size H x W through one runtime: its options and stages set, the videos dealt to the
    slots (`deal_slots`), every step pushed, its valid outputs taken to the host in one egress and written (`write_frame`) -- with
    --video_out also rendered and converted for all slots at once (`ppipe`, `ycbcr`), taken to the host in one copy and appended to the
    open stream of the slot's video, which is closed where the video ends --, and the
    `dpc:` and `rows:` lines of every video that ended and, with --report, its record (`report_out`: {"file": the open file, "total": the sum of
    the accumulators read so far or None, "frames": those they cover}; `writers`: the caller's dict of the open streams by slot).  -> the
    frames written."""
    layout, sample, _ = OUT_FORMATS.get(opt.out_format, (None, None, None))      # none (with --video_out): no per-frame file, no egress
    depth = 8 if opt.out_format == "f32" else opt.out_bit_depth
    video = getattr(opt, "video", None)         # --video_out: a VideoOut
    vframes = None
    dev, fut = model.device, int(opt.future_patch_depth)
    B = max(1, min(int(opt.batch_size), len(videos)))
    rt = model._netDenoise.runtime_for(B, H, W, pin=True)
    rt.set_option("no_warp", int(bool(opt.no_warp)))
    rt.set_option("prev_noisy_frame", int(bool(opt.prev_noisy_frame)))
    rt.set_option("warp_raw", int(bool(opt.warp_raw)))
    rt.set_option("bayer_pattern", BAYER_PATTERNS.index(opt.bayer_pattern))
    rt.set_option("stream_reset_each", int(model.training_unrollings == 1))
    rt.set_option("stream_flow_from_denoised", int(bool(getattr(opt, "val_flow_from_denoised", False))))
    rt.set_option("stream_all_frames", int(opt.all_frames))
    rt.set_dpc(None if opt.dpc is None else opt.dpc.cfg())
    if dmap is not None and dmap.shape != (H // 2, W // 2):
        raise SystemExit("--dpc_map: the map is one of a %d x %d mosaic, video %r has frames of %d x %d (one camera per run)"
                         % (2 * dmap.shape[1], 2 * dmap.shape[0], videos[0][0], W, H))
    if dmap is not None:
        rt.set_dpc_map(dmap)
    cmap, rows, report = opt.cols_map, opt.rows, opt.report
    if cmap is not None and cmap.shape[1] != W // 2:
        raise SystemExit("--col_noise: the map is one of %d mosaic columns, video %r has frames of %d x %d (one camera per run)"
                         % (2 * cmap.shape[1], videos[0][0], W, H))
    if cmap is not None:
        rt.set_cols(cmap)
    if rows is not None:
        rt.set_rows(rows.cfg())
    gmap = getattr(opt, "green_map", None)
    if gmap is not None and gmap.shape != (1, 1) and gmap.shape != green_grid(H // 2, W // 2):
        raise SystemExit("--green_eq: the map is one of %d x %d blocks, video %r has frames of %d x %d, which are %d x %d blocks (one camera per run)"
                         % ((gmap.shape[0], gmap.shape[1], videos[0][0], W, H) + green_grid(H // 2, W // 2)))
    if gmap is not None:
        rt.set_green(gmap, opt.green.black_dn)
    rt.set_match(match)
    if report is not None:
        rt.set_resid(True)
    measured = [0] * B                          # outputs of the slot's video the stage has measured
    dpc_seen = rt.dpc_counts() if opt.dpc is not None else None      # rvdd_dpc_counts at the end of the slot's last video
    dpc_frames = [0] * B                        # frames the slot's video has pushed
    container = dataset.container               # None, or "msb" / "mipi": the frames stay bit-packed up to the device
    if layout == "bits" and sample == "mipi" and W % (2 if depth == 12 else 4):
        raise SystemExit("--out_format mosaic_mipi: a RAW%d row is groups of %d pixels, the frames are %d wide" % (depth, 2 if depth == 12 else 4, W))
    if container is not None:
        shape = (B, H, bits_row_bytes(W, int(opt.bit_depth), container))
    else:
        shape = (B, H, W) if dataset.layout == "mosaic" else (B, H // 2, W // 2, 4)
    out = files = None
    written = 0
    # --all_frames with a future frame: the step behind a video's last frame (k = N) is the IDLE that outputs that frame
    for step in deal_slots([len(f) for _, f in videos], B, tail=fut if opt.all_frames else 0):
        batch = np.zeros(shape, dtype=dataset.dtype)
        for b, (c, vid, k) in enumerate(step):
            if c != IDLE:
                batch[b] = dataset.read_frame(videos[vid][1][k])
        out, valid = rt.video_push(to_device(dataset, batch, dev), [c for c, _, _ in step], int(opt.bit_depth), dataset.layout, out,
                                   container=container)
        host = vhost = None
        if any(valid) and layout is not None:        # the files' samples of all slots: one kernel, one copy
            files = rt.egress_bits(out, sample, depth, out=files) if layout == "bits" else rt.egress(out, layout, sample, depth, out=files)
            host = files.cpu().numpy()
            host = host.view(np.uint16) if host.dtype == np.int16 else host
        if any(valid) and video is not None:         # the streams' frame bodies of all slots: two kernels, one copy
            iso, n, red, blue = video.render
            _, disp = rt.ppipe(out, 1.0 / n, red, blue, iso, _lib.PPIPE_FROM_NET, "nchw", want_float=True)
            vframes = rt.ycbcr(disp, video.depth, out=vframes)
            vhost = vframes.cpu().numpy()
            vhost = vhost.view(np.uint16) if vhost.dtype == np.int16 else vhost
        ended, ends = False, []
        for b, (c, vid, k) in enumerate(step):
            if vid < 0:
                continue
            key, frames = videos[vid]
            last = k == len(frames) - (0 if opt.all_frames and fut else 1)      # the step that ends the video
            ended = ended or last
            dpc_frames[b] = min(k + 1, len(frames))
            if last:                                # --cuts: several shots share a key; the lines name the shot's first frame
                ends.append((b, key, None if opt.cuts is None else os.path.basename(frames[0])))
            if video is not None and k == 0:        # the slot starts a video (a shot): its stream, named after the shot's first frame under --cuts
                name = key if opt.cuts is None else '%s.%s' % (key, os.path.splitext(os.path.basename(frames[0]))[0])
                os.makedirs(os.path.dirname(os.path.join(opt.results_dir, name)), exist_ok=True)
                writers[b] = Y4MWriter(os.path.join(opt.results_dir, name + '.y4m'), W, H, video.depth, *video.fps)
            if valid[b]:
                measured[b] += 1
                write_frame(opt, rt, out[b:b + 1], None if host is None else host[b], key, frames[k - fut], W)      # the centre frame
                if video is not None:
                    writers[b].write(vhost[b])
                written += 1
        if ended:
            for b, _, _ in ends:                    # the streams of the videos (shots) that ended
                if b in writers:
                    writers.pop(b).close()
            rt.set_option("tvl1_async", 0)          # synchronises: reports a TV-L1 exchange of this video's pushes that gave up
            if opt.dpc is not None:                 # ... and before the slot's next FIRST push: the difference is this video's
                now = rt.dpc_counts()
                for b, key, first in ends:
                    print('dpc: %d hot, %d dead samples corrected in %d frames (%s)'
                          % (now[b][0] - dpc_seen[b][0], now[b][1] - dpc_seen[b][1], dpc_frames[b], shot_name(key, first)))
                    dpc_seen[b] = now[b]
            if rows is not None:                    # the slot's counts are this video's frames: read, which zeroes them
                for b, key, first in ends:
                    print(rows_line(rt.rows_read(b), dpc_frames[b], rows, int(opt.bit_depth), W // 2, shot_name(key, first)))
            if report is not None:                  # the slot's accumulator holds this video's outputs: read, which zeroes it
                for b, key, first in ends:
                    acc = rt.resid_read(b)
                    names = {"video": key} if first is None else {"video": key, "from": first}
                    report_out["file"].write(json.dumps(report_record(acc, measured[b], report, **names)) + '\n')
                    report_out["total"] = acc if report_out["total"] is None else resid_add(report_out["total"], acc)
                    report_out["frames"] += measured[b]
                    measured[b] = 0
    rt.set_option("tvl1_async", 0)
    if report is not None:
        rt.set_resid(False)
    if rows is not None:
        rt.set_rows(None)
    if cmap is not None:
        rt.set_cols(None)
    if gmap is not None:
        rt.set_green(None)
    return written


def main(argv=None) -> dict:
    from .models import create_model
    opt = _parse(argv)
    dataset = open_rawvideo(opt, None, "denoise")          # _parse has settled --dataset_mode
    model = create_model(opt)
    model.setup(opt)
    dmap, match, shots = prepasses(opt, dataset, model.device)
    groups = {}                                   # frame size -> its videos, in dataset order
    for key, frames in shots:
        groups.setdefault(dataset.frame_size(frames[0]), []).append((key, frames))
    written = 0
    t0 = time.time()
    report_out = None if opt.report is None else {"file": open(opt.report.path, "w"), "total": None, "frames": 0}
    for (H, W), videos in groups.items():
        written += run_group(opt, model, dataset, videos, H, W, dmap, match, report_out)
    torch.cuda.synchronize(model.device)
    dt = time.time() - t0
    if report_out is not None:
        report_out["file"].close()
        if report_out["total"] is not None:      # the sums of all videos judged as one: every figure weighted by its samples
            print('report: ' + json.dumps(report_record(report_out["total"], report_out["frames"], opt.report, videos=len(shots))))
    print('(denoise, %d frames, %.3f s, %.2f frames/s)' % (written, dt, written / max(dt, 1e-9)))
    return {'frames': written, 'seconds': dt, 'fps': written / max(dt, 1e-9)}


if __name__ == '__main__':
    main()
