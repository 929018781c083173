"""What the five footage commands (`denoise`, `noise`, `cuts`, `dpc_map`, `col_noise`) share: opening the rawvideo dataset, host frames to the device
and through the ingest, the `--dpc*` flags with the noise estimate they may ask for, the `--row_noise*` flags, the `--col_noise*` flags and the `--report*` flags.  The commands import this module and the
feature modules; nothing here or there imports a command.
"""
from __future__ import annotations

import copy

import torch

from .runtime import DPC_ISO_CURVES, dpc_iso_curve, raw_frames_to_device


def open_rawvideo(opt, rest, who: str):
    """The dataset of a footage command: `--dataset_mode rawvideo` unless `rest` (the arguments `options.parse` read; None: the caller
    has settled opt.dataset_mode) names another, every frame of every video, in order, read in this process.  SystemExit for a
    dataset that has no frames to read one by one."""
    from .data import create_dataset
    if rest is not None and not any(a == '--dataset_mode' or a.startswith('--dataset_mode=') for a in rest):
        opt.dataset_mode = 'rawvideo'
    v = copy.deepcopy(opt)
    v.max_dataset_size, v.num_threads, v.batch_size, v.serial_batches = float("inf"), 0, 1, True
    dataset = create_dataset(v).dataset
    if not hasattr(dataset, "read_frame"):
        raise SystemExit("%s reads --dataset_mode rawvideo" % who)
    return dataset


def to_device(dataset, frames_np, dev):
    """Host frames as `dataset.read_frame` gives them, stacked, -> the device tensor `video_push` / the ingest take: bit-packed
    containers travel as their bytes, sensor samples as `raw_frames_to_device` sends them."""
    return torch.from_numpy(frames_np).to(dev) if dataset.container is not None else raw_frames_to_device(frames_np, dev)


def ingest_frames(rt, dataset, frames_np, bit_depth: int, want_packed: bool = True, want_gray: bool = True):
    """n stacked host frames of one size -> (packed [n,4,hh,ww], gray [n,hh,ww]) on `rt`'s device, None for one not wanted, as
    `video_push` ingests them: `ingest_bits` for a dataset of bit-packed frames, `ingest_raw` in the dataset's layout otherwise."""
    t = to_device(dataset, frames_np, rt._tdev)
    if dataset.container is None:
        return rt.ingest_raw(t, int(bit_depth), dataset.layout, want_packed=want_packed, want_gray=want_gray)
    # [n,H,row_bytes]: a row of W samples is W * bit_depth / 8 bytes, rounded up to a whole byte ("msb") -- fewer than 8 pad bits,
    # less than one sample of 10 bits or more, so the whole samples of a row are W again
    n, H, row_bytes = frames_np.shape
    return rt.ingest_bits(t, dataset.container, int(bit_depth), H // 2, row_bytes * 8 // int(bit_depth) // 2, n=n,
                          want_packed=want_packed, want_gray=want_gray)


def add_dpc_arguments(p) -> None:
    """the five flags that name the rule of --dpc, for `denoise` and `dpc_map`; `dpc_arguments` reads them"""
    p.add_argument('--dpc', type=float, default=None, help='defective-pixel correction: threshold K in standard deviations (both sides)')
    p.add_argument('--dpc_dead', type=float, default=None, help='threshold of the dead side (default: --dpc; 0 = off)')
    p.add_argument('--dpc_iso', type=int, default=None, help='the noise curve of ISO 3200 / 12800, rescaled to --bit_depth')
    p.add_argument('--dpc_noise', type=str, default=None, help='a,b[,floor]: var = a * m - b in DN of the frames, the least variance; '
                   'auto[,floor]: estimated from the footage (assumes one camera setting for the whole run)')
    p.add_argument('--dpc_noise_frames', type=int, default=None, help='with --dpc_noise auto: frames read per video (default 4)')


def dpc_arguments(dpc, dpc_dead, dpc_iso, dpc_noise, bit_depth, dpc_noise_frames=None):
    """--dpc / --dpc_dead / --dpc_iso / --dpc_noise -> None (no --dpc) or (k_hot, k_dead, noise_a, noise_b, var_floor) as Python
    doubles (`runtime.dpc_cfg` rounds each to f32 once); SystemExit where the flags do not fit together.  --dpc_noise auto[,floor]:
    noise_a and noise_b are None, for the command to estimate from the footage (`estimate_noise`)."""
    if dpc is None:
        if dpc_dead is not None or dpc_iso is not None or dpc_noise is not None or dpc_noise_frames is not None:
            raise SystemExit("--dpc_dead, --dpc_iso and --dpc_noise belong to --dpc K")
        return None
    auto = dpc_noise is not None and dpc_noise.split(',')[0] == 'auto'
    if dpc_noise_frames is not None and not auto:
        raise SystemExit("--dpc_noise_frames belongs to --dpc_noise auto")
    if dpc_noise_frames is not None and dpc_noise_frames < 1:
        raise SystemExit("--dpc_noise_frames must be >= 1, got %d" % dpc_noise_frames)
    if (dpc_iso is None) == (dpc_noise is None):
        raise SystemExit("--dpc needs exactly one of --dpc_iso {%s} and --dpc_noise a,b[,floor]" % ','.join(str(k) for k in DPC_ISO_CURVES))
    k_dead = dpc if dpc_dead is None else dpc_dead
    if not (dpc >= 0 and k_dead >= 0 and dpc < float("inf") and k_dead < float("inf")):
        raise SystemExit("--dpc and --dpc_dead are thresholds >= 0, got %r and %r" % (dpc, k_dead))
    floor = 1.0
    if dpc_iso is not None:
        if dpc_iso not in DPC_ISO_CURVES:
            raise SystemExit("--dpc_iso must be one of %s, got %r" % (', '.join(str(k) for k in DPC_ISO_CURVES), dpc_iso))
        a, b = dpc_iso_curve(dpc_iso, bit_depth)
    else:
        f = dpc_noise.split(',')
        if auto:
            f = [None] + f                         # auto[,floor]: a and b come from the footage
        if len(f) not in (2, 3):
            raise SystemExit("--dpc_noise takes a,b, a,b,floor or auto[,floor]")
        try:
            a, b = (None, None) if auto else (float(f[0]), float(f[1]))
            floor = float(f[2]) if len(f) == 3 else 1.0
        except ValueError:
            raise SystemExit("--dpc_noise takes numbers a,b[,floor] or auto[,floor], got %r" % dpc_noise)
        if not floor > 0:
            raise SystemExit("--dpc_noise: the floor must be > 0, got %r" % floor)
    return (float(dpc), float(k_dead), a, b, floor)


def estimate_noise(dataset, dev, bit_depth, frames, flag='--dpc_noise'):
    """--dpc_noise auto / --match_noise auto: (a, b) of `noise.estimate` on the run's videos, the line `python -m rvdd_release_amd.noise` prints sent to
    the log; SystemExit with the fit's message where it refuses."""
    from . import noise
    from .util._ops import ops_runtime
    acc, read = noise.estimate(ops_runtime(dev.index or 0), dataset, bit_depth, frames)
    try:
        r = noise.report(acc, bit_depth, read)
    except RuntimeError as err:
        raise SystemExit("%s auto: %s -- pass the curve as %s a,b" % (flag, err, flag))
    print('noise: ' + noise.format_line(r))
    return (r["a"], r["b"])


def curve_argument(flag, curve, dpc, bit_depth):
    """--row_noise_curve / --col_noise_curve (`flag`, with its dashes) -> (source, a, b, floor): where the curve var = a * m - b (DN of
    `bit_depth`) comes from -- "a,b", "iso<ISO>", "auto" (a and b None, for the command to estimate from the footage) or, without the
    flag, "dpc" (dpc = what `dpc_arguments` returned: its curve and floor, a and b None under --dpc_noise auto) -- and the least
    variance.  SystemExit where it cannot be read."""
    owner = {'--row_noise_curve': "--row_noise", '--col_noise_curve': "--col_noise auto"}[flag]      # what the curve is asked for
    floor = 1.0
    if curve is None:
        if dpc is None:
            raise SystemExit("%s needs the sensor's noise curve: %s a,b[,floor] (var = a * m - b in DN of the frames), "
                             "%s auto (estimated from the footage), %s iso3200 / iso12800 (a checkpoint "
                             "family's curve, rescaled to --bit_depth) -- or the curve of --dpc, which then serves" % (owner, flag, flag, flag))
        return ("dpc", dpc[2], dpc[3], dpc[4])
    if curve == 'auto':
        return ("auto", None, None, floor)
    if curve.startswith('iso'):
        try:
            iso = int(curve[3:])
            a, b = dpc_iso_curve(iso, bit_depth)
        except ValueError:
            raise SystemExit("%s %s: the families are %s" % (flag, curve, ', '.join('iso%d' % k for k in DPC_ISO_CURVES)))
        return ("iso%d" % iso, a, b, floor)
    f = curve.split(',')
    try:
        if len(f) not in (2, 3):
            raise ValueError(curve)
        a, b = float(f[0]), float(f[1])
        floor = float(f[2]) if len(f) == 3 else 1.0
    except ValueError:
        raise SystemExit("%s takes a,b[,floor], auto, iso3200 or iso12800, got %r" % (flag, curve))
    if not abs(a) < float("inf") or not abs(b) < float("inf"):
        raise SystemExit("%s: a and b must be finite, got %r" % (flag, curve))
    if not (floor > 0 and floor < float("inf")):
        raise SystemExit("%s: the floor must be > 0, got %r" % (flag, floor))
    return ("a,b", a, b, floor)


def add_rows_arguments(p) -> None:
    """the three flags of the row-noise correction, beside --dpc; `rows_arguments` reads them"""
    p.add_argument('--row_noise', type=float, default=None, help='take row noise (banding) out of every frame on the device: the gate K in '
                   'standard deviations of the noise curve, around 3')
    p.add_argument('--row_noise_curve', type=str, default=None, help='the curve of --row_noise: a,b[,floor] (var = a * m - b in DN of the frames), '
                   'auto (estimated from the footage), iso3200 or iso12800; default: the curve of --dpc')
    p.add_argument('--row_noise_max', type=float, default=None, help='the largest offset taken out, in DN (default (2^bit_depth - 1) / 64)')


def rows_arguments(row_noise, curve, max_dn, dpc, bit_depth):
    """--row_noise / --row_noise_curve / --row_noise_max -> None (no --row_noise) or (k_gate, source, a, b, floor, max_dn): the gate, where
    the curve var = a * m - b (DN of `bit_depth`) comes from -- "a,b", "iso<ISO>", "auto" (a and b None, for the command to estimate from
    the footage) or "dpc" (dpc = what `dpc_arguments` returned: its curve and floor, a and b None under --dpc_noise auto) -- the least
    variance and the clamp.  SystemExit where the flags do not fit together."""
    if row_noise is None:
        if curve is not None or max_dn is not None:
            raise SystemExit("--row_noise_curve and --row_noise_max belong to --row_noise K")
        return None
    if not (row_noise > 0 and row_noise < float("inf")):
        raise SystemExit("--row_noise is the gate in standard deviations, > 0 (around 3), got %r" % row_noise)
    top = float((1 << int(bit_depth)) - 1)
    max_dn = top / 64.0 if max_dn is None else float(max_dn)
    if not (max_dn > 0 and max_dn < float("inf")):
        raise SystemExit("--row_noise_max is the largest offset taken out in DN, > 0, got %r" % max_dn)
    source, a, b, floor = curve_argument('--row_noise_curve', curve, dpc, bit_depth)
    return (float(row_noise), source, a, b, floor, max_dn)


def rows_line(acc, frames, spec, bit_depth, ww, key):
    """the `rows:` line of one video or shot: `acc` as `runtime.rows_acc_arrays` gives it, spec = what `rows_arguments` returned"""
    from .runtime import rows_floor_rms, rows_rms
    _, _, a, b, floor, _ = spec
    return ('rows: %d applied, %d skipped, %d clamped rows, rms offset %.3f DN (the estimate alone, on flat footage without row noise: %.3f DN) '
            'in %d frames (%s)' % (int(acc["applied"].sum()), int(acc["skipped"].sum()), int(acc["clamped"].sum()), rows_rms(acc),
                                   rows_floor_rms(a, b, floor, bit_depth, ww), frames, key))


def add_cols_arguments(p) -> None:
    """the six flags of the column-noise correction, beside --row_noise; `cols_arguments` reads them"""
    p.add_argument('--col_noise', type=str, default=None, help='take column fixed-pattern noise out of every frame on the device: FILE (a map '
                   'python -m rvdd_release_amd.col_noise wrote) or auto (found in the footage before streaming starts)')
    p.add_argument('--col_noise_curve', type=str, default=None, help='with --col_noise auto, the curve of the gate: a,b[,floor] (var = a * m - b in '
                   'DN of the frames), auto (estimated from the footage), iso3200 or iso12800; default: the curve of --dpc')
    p.add_argument('--col_noise_frames', type=int, default=None, help='with --col_noise auto: frames estimated per run, spread over the videos (default 32)')
    p.add_argument('--col_noise_gate', type=float, default=None, help='with --col_noise auto: the gate K in standard deviations of the curve (default 3)')
    p.add_argument('--col_noise_sigma', type=float, default=None, help='with --col_noise auto: a column is changed where its offset is at least this '
                   'many standard errors of its own estimate (default 3; 0 changes every column)')
    p.add_argument('--col_noise_max', type=float, default=None, help='with --col_noise auto: the largest offset taken out, in DN (default (2^bit_depth - 1) / 64)')


def cols_arguments(col_noise, curve, frames, gate, sigma, max_dn, dpc, bit_depth):
    """--col_noise and its five flags -> None (no --col_noise), ("file", path) or ("auto", frames, k_gate, k_sig, max_dn, source, a, b,
    floor): source says where the curve var = a * m - b (DN of `bit_depth`) comes from, as `rows_arguments` does ("a,b", "iso<ISO>",
    "auto" with a and b None for the command to estimate, or "dpc": dpc = what `dpc_arguments` returned).  SystemExit where the flags
    do not fit together."""
    given = [n for n, v in (("col_noise_curve", curve), ("col_noise_frames", frames), ("col_noise_gate", gate), ("col_noise_sigma", sigma),
                            ("col_noise_max", max_dn)) if v is not None]
    if col_noise is None:
        if given:
            raise SystemExit("--col_noise_curve, --col_noise_frames, --col_noise_gate, --col_noise_sigma and --col_noise_max belong to --col_noise auto")
        return None
    if col_noise != "auto":
        if given:
            raise SystemExit("--%s belongs to --col_noise auto: --col_noise %s reads a map that is already made" % (given[0], col_noise))
        return ("file", col_noise)
    inf = float("inf")
    frames, gate, sigma = 32 if frames is None else int(frames), 3.0 if gate is None else float(gate), 3.0 if sigma is None else float(sigma)
    if frames < 1:
        raise SystemExit("--col_noise_frames must be >= 1, got %d" % frames)
    if not (gate > 0 and gate < inf):
        raise SystemExit("--col_noise_gate is the gate in standard deviations, > 0 (around 3), got %r" % gate)
    if not (sigma >= 0 and sigma < inf):
        raise SystemExit("--col_noise_sigma is a number of standard errors, >= 0 (around 3; 0 changes every column), got %r" % sigma)
    max_dn = float((1 << int(bit_depth)) - 1) / 64.0 if max_dn is None else float(max_dn)      # a guess, as for the rows
    if not (max_dn > 0 and max_dn < inf):
        raise SystemExit("--col_noise_max is the largest offset taken out in DN, > 0, got %r" % max_dn)
    return ("auto", frames, gate, sigma, max_dn) + curve_argument('--col_noise_curve', curve, dpc, bit_depth)


def add_report_arguments(p) -> None:
    """the two flags of the residual report, for `denoise`; `report_arguments` reads them"""
    p.add_argument('--report', type=str, default=None, help='FILE: one JSON line per video with the residual statistics of its outputs '
                   '(noisy - remosaic(denoised)) judged against a noise curve: no ground truth needed')
    p.add_argument('--report_noise', type=str, default=None, help='the curve of --report without --match_noise: a,b (var = a * m - b in DN of '
                   'the frames), auto (estimated from the footage), iso3200 or iso12800')


def report_arguments(report, report_noise, match, bit_depth):
    """--report / --report_noise -> None (no --report) or (path, source, a, b, unit): the curve var = a * m - b in DN of `unit` bits the
    residual is judged against, and where it comes from -- "match_iso<ISO>" (match = what `match_arguments` returned: the checkpoint
    family's curve in 12-bit DN, the unit the stage measures in under the match), "a,b", "iso<ISO>" or "auto" (a and b None, for the
    command to estimate from the footage).  SystemExit where the flags do not fit together."""
    if report is None:
        if report_noise is not None:
            raise SystemExit("--report_noise belongs to --report FILE")
        return None
    if match is not None:
        if report_noise is not None:
            raise SystemExit("--report_noise does not go with --match_noise: matched footage is judged against the curve of --match_iso, "
                             "the one the network sees")
        a, b = DPC_ISO_CURVES[match[2]]
        return (report, "match_iso%d" % match[2], a, b, 12)
    if report_noise is None:
        raise SystemExit("--report needs the noise curve the residual is judged against: --report_noise a,b (var = a * m - b in DN of the "
                         "frames), --report_noise auto (estimated from the footage), --report_noise iso3200 / iso12800 (a checkpoint "
                         "family's curve, rescaled to --bit_depth) -- or --match_noise, whose --match_iso curve then serves")
    if report_noise == 'auto':
        return (report, "auto", None, None, int(bit_depth))
    if report_noise.startswith('iso'):
        try:
            iso = int(report_noise[3:])
            a, b = dpc_iso_curve(iso, bit_depth)
        except ValueError:
            raise SystemExit("--report_noise %s: the families are %s" % (report_noise, ', '.join('iso%d' % k for k in DPC_ISO_CURVES)))
        return (report, "iso%d" % iso, a, b, int(bit_depth))
    f = report_noise.split(',')
    try:
        a, b = (float(v) for v in f)
    except ValueError:
        raise SystemExit("--report_noise takes a,b, auto, iso3200 or iso12800, got %r" % report_noise)
    if not abs(a) < float("inf") or not abs(b) < float("inf"):
        raise SystemExit("--report_noise: a and b must be finite, got %r" % report_noise)
    return (report, "a,b", a, b, int(bit_depth))


REPORT_KEYS = ("ratio", "ratio_lo", "ratio_hi", "bias", "rho", "a_fit", "b_fit", "samples", "bins")


def report_record(acc, frames, spec, **names):
    """One record of --report: `names` (the video's key, ...), the frames measured, the fields of `runtime.resid_fit` on `acc` -- None,
    with "error": the library's message, where the fit refuses (fewer than 4 usable level bins) -- and the curve it was judged against."""
    from .runtime import resid_fit
    _, source, a, b, unit = spec
    rec = dict(names, frames=int(frames))
    try:
        rec.update(resid_fit(acc, unit, a, b))
    except RuntimeError as err:
        rec.update({k: None for k in REPORT_KEYS}, error=str(err))
    rec["curve"] = {"a": a, "b": b, "bit_depth": unit, "source": source}
    return rec
