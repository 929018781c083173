"""What the footage commands (`denoise`, `noise`, `cuts`, `dpc_map`, `col_noise`, `green_eq`) share: opening the rawvideo dataset, host frames to
the device and through the ingest, the frames a map pre-pass samples (`sampled_frames`), one named record per stage's settings
(`DpcSpec`, `RowsSpec`, `ColsSpec`, `GreenSpec`, `MatchSpec`, `ReportSpec`), the one reader of a noise curve given on the command line
(`curve_word` over the table CURVE_WORDS) with the `*_arguments` functions that hold each stage's cross-flag rules, and the
estimate `auto` asks for.  The commands import this module and the feature modules; nothing here or there imports a command.
"""
from __future__ import annotations

import copy
import math
from typing import NamedTuple, Optional

import torch

from .runtime import DPC_ISO_CURVES, cols_cfg, dpc_cfg, dpc_iso_curve, green_cfg, raw_frames_to_device, rows_cfg

MAX_VIDEOS = 16                                   # the videos a pre-pass reads of a run
INF = float("inf")


# ---- the stage records: what the `*_arguments` functions return.  Fields in the order the tuples they replace had, so that a record
# still equals that tuple; a and b are None where the curve is the run's own estimate, until `with_curve` fills them in ----
def _needs_curve(spec) -> bool:
    return spec.a is None


def _with_curve(spec, a, b):
    return spec._replace(a=a, b=b)


class DpcSpec(NamedTuple):
    """--dpc: Python doubles, `dpc_cfg` rounds each to f32 once"""
    k_hot: float
    k_dead: float
    a: Optional[float]
    b: Optional[float]
    floor: float
    needs_curve, with_curve = property(_needs_curve), _with_curve

    def cfg(self):
        return dpc_cfg(k_hot=self.k_hot, k_dead=self.k_dead, noise_a=self.a, noise_b=self.b, var_floor=self.floor)


class RowsSpec(NamedTuple):
    """--row_noise: source is where the curve comes from, "a,b", "iso<ISO>", "auto" or "dpc" """
    k_gate: float
    source: str
    a: Optional[float]
    b: Optional[float]
    floor: float
    max_dn: float
    needs_curve, with_curve = property(_needs_curve), _with_curve

    def cfg(self):
        return rows_cfg(k_gate=self.k_gate, noise_a=self.a, noise_b=self.b, var_floor=self.floor, max_dn=self.max_dn)


class ColsSpec(NamedTuple):
    """--col_noise auto: kind is "auto"; source as for the rows"""
    kind: str
    frames: int
    k_gate: float
    k_sig: float
    max_dn: float
    source: str
    a: Optional[float]
    b: Optional[float]
    floor: float
    needs_curve, with_curve = property(_needs_curve), _with_curve

    def cfg(self):
        return cols_cfg(k_gate=self.k_gate, noise_a=self.a, noise_b=self.b, var_floor=self.floor)


class GreenSpec(NamedTuple):
    """--green_eq: kind is "auto" (path None) or "file" (the map is read from path; frames .. field are not used); black None: the level
    noise_b / noise_a at which the curve's variance is zero; source as for the rows, or "black" where --green_eq_black alone serves a FILE"""
    kind: str
    path: Optional[str]
    frames: int
    k_gate: float
    k_sig: float
    max_gain: float
    min_signal: float
    field: str
    black: Optional[float]
    source: str
    a: Optional[float]
    b: Optional[float]
    floor: float

    @property
    def needs_curve(self) -> bool:
        return self.a is None and (self.kind == "auto" or self.black is None)

    with_curve = _with_curve

    @property
    def black_dn(self) -> float:
        """the level without signal in DN: --green_eq_black, else noise_b / noise_a (0 for a curve without a slope)"""
        if self.black is not None:
            return self.black
        return self.b / self.a if self.a else 0.0

    def cfg(self):
        return green_cfg(k_gate=self.k_gate, noise_a=self.a, noise_b=self.b, var_floor=self.floor, black=self.black_dn)


class MatchSpec(NamedTuple):
    """--match_noise / --match_iso: the footage's curve in DN of --bit_depth and the checkpoint's family"""
    a: Optional[float]
    b: Optional[float]
    iso: int
    needs_curve, with_curve = property(_needs_curve), _with_curve


class ReportSpec(NamedTuple):
    """--report: the curve in DN of `unit` bits the residual is judged against; source "match_iso<ISO>", "a,b", "iso<ISO>" or "auto" """
    path: str
    source: str
    a: Optional[float]
    b: Optional[float]
    unit: int
    needs_curve, with_curve = property(_needs_curve), _with_curve


# --col_noise FILE, --dpc_map FILE, --cuts FILE: kind is "file"; a map or a list that is already made
FileSpec = NamedTuple("FileSpec", [("kind", str), ("path", str)])


# ---- a noise curve given on the command line ----
class CurveWord(NamedTuple):
    """what one flag allows of a curve word"""
    takes: str                 # the refusal of a word of the wrong form ({!r}: the word) ...
    numbers: str               # ... and of numbers that do not read
    floor: bool = False        # a,b,floor
    floor_inf: bool = False    # ... which may be infinite
    auto_floor: bool = False   # auto,floor
    iso: bool = False          # iso3200 / iso12800, rescaled to --bit_depth
    check: tuple = ()          # (what a and b must be, its sentence)


_FINITE = (lambda a, b: abs(a) < INF and abs(b) < INF, "a and b must be finite")
_LINE = "takes a,b[,floor], auto, iso3200 or iso12800, got {!r}"
_REPORT = "takes a,b, auto, iso3200 or iso12800, got {!r}"
CURVE_WORDS = {
    # --dpc_noise checks the floor alone: a and b may be anything a float reads, and an infinite floor passes
    '--dpc_noise': CurveWord("takes a,b, a,b,floor or auto[,floor]", "takes numbers a,b[,floor] or auto[,floor], got {!r}", floor=True,
                             floor_inf=True, auto_floor=True),
    '--match_noise': CurveWord("takes a,b or auto, got {!r}", "takes numbers a,b or auto, got {!r}",
                               check=(lambda a, b: 0 < a < INF and abs(b) < INF, "a must be finite and > 0 and b finite")),
    '--row_noise_curve': CurveWord(_LINE, _LINE, floor=True, iso=True, check=_FINITE),
    '--col_noise_curve': CurveWord(_LINE, _LINE, floor=True, iso=True, check=_FINITE),
    '--green_eq_curve': CurveWord(_LINE, _LINE, floor=True, iso=True, check=_FINITE),
    '--report_noise': CurveWord(_REPORT, _REPORT, iso=True, check=_FINITE),
}


def curve_word(flag, word, bit_depth):
    """One curve word of `flag` (a key of CURVE_WORDS, which says what that flag allows) -> (source, a, b, floor): var = a * m - b in DN
    of `bit_depth` and the least variance (1 where the word has none), source "a,b", "iso<ISO>" or "auto" -- a and b None then, for
    the command to estimate from the footage.  SystemExit with the flag's own sentence for a word it cannot read."""
    rule = CURVE_WORDS[flag]
    f = word.split(',')
    auto = f[0] == 'auto' and (rule.auto_floor or len(f) == 1)
    if rule.iso and word.startswith('iso'):
        try:
            iso = int(word[3:])
            return ("iso%d" % iso,) + dpc_iso_curve(iso, bit_depth) + (1.0,)
        except ValueError:
            raise SystemExit("%s %s: the families are %s" % (flag, word, ', '.join('iso%d' % k for k in DPC_ISO_CURVES)))
    rest = f[1:] if auto else f[2:]                # what stands behind auto, or behind a,b: the floor
    if len(rest) > rule.floor or len(f) < 2 - auto:
        raise SystemExit("%s %s" % (flag, rule.takes.format(word)))
    try:
        a, b = (None, None) if auto else (float(f[0]), float(f[1]))
        floor = float(rest[0]) if rest else 1.0
    except ValueError:
        raise SystemExit("%s %s" % (flag, rule.numbers.format(word)))
    if not auto and rule.check and not rule.check[0](a, b):
        raise SystemExit("%s: %s, got %r" % (flag, rule.check[1], word))
    if not floor > 0 or not (floor < INF or rule.floor_inf):
        raise SystemExit("%s: the floor must be > 0, got %r" % (flag, floor))
    return ("auto" if auto else "a,b", a, b, floor)


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


def spread_indices(n: int, k: int):
    """min(k, n) frame indices spread evenly over a video of n frames: round(i (n - 1) / (k - 1)), halves up; ascending, no repeats"""
    k = max(1, min(int(k), int(n)))
    if k == 1:
        return [0]
    return sorted({int(math.floor(i * (n - 1) / (k - 1) + 0.5)) for i in range(k)})


def sampled_frames(rt, dataset, bit_depth: int, frames: int, noun: str, in_all: bool = False, max_videos: int = MAX_VIDEOS):
    """The frames a map pre-pass reads, as packed [1,4,hh,ww] on `rt`'s device, one per step: of the first `max_videos` videos of a
    rawvideo dataset `frames` frames of each, which `spread_indices` picks -- in_all: `frames` in all, ceil(frames / videos) of each
    until that many are read -- ingested as `video_push` ingests them.  RuntimeError, with the caller's `noun` ("a defect map"), where
    the videos differ in frame size, or where there is none."""
    videos = dataset.videos[:max_videos]
    if not videos:
        raise RuntimeError("no video to read")
    left = int(frames) * (1 if in_all else len(videos))       # the frames still to read ...
    per = -(-left // len(videos))                             # ... at most this many of one video
    size = None
    for key, paths in videos:
        if left <= 0:
            return
        paths = [paths[i] for i in spread_indices(len(paths), min(per, left))]
        H, W = dataset.frame_size(paths[0])
        if size is not None and (H, W) != size:
            raise RuntimeError("%s is one sensor's: video %r has frames of %d x %d, the videos before it %d x %d" % (noun, key, W, H, size[1], size[0]))
        size = (H, W)
        for p in paths:                               # one frame per call: the results do not depend on the split, the memory does
            yield ingest_frames(rt, dataset, dataset.read_frame(p)[None], bit_depth, want_gray=False)[0]
            left -= 1


def add_dpc_arguments(p) -> None:
    """the five flags that name the rule of --dpc, for `denoise` and `dpc_map`; `dpc_arguments` reads them"""
    p.add_argument('--dpc', type=float, default=None, help='defective-pixel correction: threshold K in standard deviations (both sides)')
    p.add_argument('--dpc_dead', type=float, default=None, help='threshold of the dead side (default: --dpc; 0 = off)')
    p.add_argument('--dpc_iso', type=int, default=None, help='the noise curve of ISO 3200 / 12800, rescaled to --bit_depth')
    p.add_argument('--dpc_noise', type=str, default=None, help='a,b[,floor]: var = a * m - b in DN of the frames, the least variance; '
                   'auto[,floor]: estimated from the footage (assumes one camera setting for the whole run)')
    p.add_argument('--dpc_noise_frames', type=int, default=None, help='with --dpc_noise auto: frames read per video (default 4)')


def dpc_arguments(dpc, dpc_dead, dpc_iso, dpc_noise, bit_depth, dpc_noise_frames=None):
    """--dpc / --dpc_dead / --dpc_iso / --dpc_noise -> None (no --dpc) or a DpcSpec; SystemExit where the flags do not fit together.
    --dpc_noise auto[,floor]: a and b are None, for the command to estimate from the footage (`estimate_noise`)."""
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
    if not (dpc >= 0 and k_dead >= 0 and dpc < INF and k_dead < INF):
        raise SystemExit("--dpc and --dpc_dead are thresholds >= 0, got %r and %r" % (dpc, k_dead))
    if dpc_iso is not None:
        if dpc_iso not in DPC_ISO_CURVES:
            raise SystemExit("--dpc_iso must be one of %s, got %r" % (', '.join(str(k) for k in DPC_ISO_CURVES), dpc_iso))
        (a, b), floor = dpc_iso_curve(dpc_iso, bit_depth), 1.0
    else:
        _, a, b, floor = curve_word('--dpc_noise', dpc_noise, bit_depth)
    return DpcSpec(float(dpc), float(k_dead), a, b, floor)


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
    """--row_noise_curve / --col_noise_curve (`flag`, with its dashes) -> (source, a, b, floor) as `curve_word` reads the word, or,
    without the flag, source "dpc": the curve and floor of dpc, the DpcSpec of the run (a and b None under --dpc_noise auto).
    SystemExit where there is neither."""
    if curve is not None:
        return curve_word(flag, curve, bit_depth)
    if dpc is None:
        owner = {'--row_noise_curve': "--row_noise", '--col_noise_curve': "--col_noise auto", '--green_eq_curve': "--green_eq"}[flag]      # what the curve is asked for
        raise SystemExit("%s needs the sensor's noise curve: %s a,b[,floor] (var = a * m - b in DN of the frames), "
                         "%s auto (estimated from the footage), %s iso3200 / iso12800 (a checkpoint "
                         "family's curve, rescaled to --bit_depth) -- or the curve of --dpc, which then serves" % (owner, flag, flag, flag))
    return ("dpc", dpc.a, dpc.b, dpc.floor)


def add_rows_arguments(p) -> None:
    """the three flags of the row-noise correction, beside --dpc; `rows_arguments` reads them"""
    p.add_argument('--row_noise', type=float, default=None, help='take row noise (banding) out of every frame on the device: the gate K in '
                   'standard deviations of the noise curve, around 3')
    p.add_argument('--row_noise_curve', type=str, default=None, help='the curve of --row_noise: a,b[,floor] (var = a * m - b in DN of the frames), '
                   'auto (estimated from the footage), iso3200 or iso12800; default: the curve of --dpc')
    p.add_argument('--row_noise_max', type=float, default=None, help='the largest offset taken out, in DN (default (2^bit_depth - 1) / 64)')


def rows_arguments(row_noise, curve, max_dn, dpc, bit_depth):
    """--row_noise / --row_noise_curve / --row_noise_max -> None (no --row_noise) or a RowsSpec: the gate, the curve with its source
    (`curve_argument`; dpc = the DpcSpec of the run or None), the least variance and the clamp.  SystemExit where the flags do not
    fit together."""
    if row_noise is None:
        if curve is not None or max_dn is not None:
            raise SystemExit("--row_noise_curve and --row_noise_max belong to --row_noise K")
        return None
    if not (row_noise > 0 and row_noise < INF):
        raise SystemExit("--row_noise is the gate in standard deviations, > 0 (around 3), got %r" % row_noise)
    top = float((1 << int(bit_depth)) - 1)
    max_dn = top / 64.0 if max_dn is None else float(max_dn)
    if not (max_dn > 0 and max_dn < INF):
        raise SystemExit("--row_noise_max is the largest offset taken out in DN, > 0, got %r" % max_dn)
    source, a, b, floor = curve_argument('--row_noise_curve', curve, dpc, bit_depth)
    return RowsSpec(float(row_noise), source, a, b, floor, max_dn)


def rows_line(acc, frames, spec, bit_depth, ww, key):
    """the `rows:` line of one video or shot: `acc` as `runtime.rows_acc_arrays` gives it, spec = the RowsSpec of the run"""
    from .runtime import rows_floor_rms, rows_rms
    return ('rows: %d applied, %d skipped, %d clamped rows, rms offset %.3f DN (the estimate alone, on flat footage without row noise: %.3f DN) '
            'in %d frames (%s)' % (int(acc["applied"].sum()), int(acc["skipped"].sum()), int(acc["clamped"].sum()), rows_rms(acc),
                                   rows_floor_rms(spec.a, spec.b, spec.floor, bit_depth, ww), frames, key))


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
    """--col_noise and its five flags -> None (no --col_noise), a FileSpec or a ColsSpec, its curve as `rows_arguments` takes it
    (`curve_argument`; dpc = the DpcSpec of the run or None).  SystemExit where the flags do not fit together."""
    given = [n for n, v in (("col_noise_curve", curve), ("col_noise_frames", frames), ("col_noise_gate", gate), ("col_noise_sigma", sigma),
                            ("col_noise_max", max_dn)) if v is not None]
    if col_noise is None:
        if given:
            raise SystemExit("--col_noise_curve, --col_noise_frames, --col_noise_gate, --col_noise_sigma and --col_noise_max belong to --col_noise auto")
        return None
    if col_noise != "auto":
        if given:
            raise SystemExit("--%s belongs to --col_noise auto: --col_noise %s reads a map that is already made" % (given[0], col_noise))
        return FileSpec("file", col_noise)
    frames, gate, sigma = 32 if frames is None else int(frames), 3.0 if gate is None else float(gate), 3.0 if sigma is None else float(sigma)
    if frames < 1:
        raise SystemExit("--col_noise_frames must be >= 1, got %d" % frames)
    if not (gate > 0 and gate < INF):
        raise SystemExit("--col_noise_gate is the gate in standard deviations, > 0 (around 3), got %r" % gate)
    if not (sigma >= 0 and sigma < INF):
        raise SystemExit("--col_noise_sigma is a number of standard errors, >= 0 (around 3; 0 changes every column), got %r" % sigma)
    max_dn = float((1 << int(bit_depth)) - 1) / 64.0 if max_dn is None else float(max_dn)      # a guess, as for the rows
    if not (max_dn > 0 and max_dn < INF):
        raise SystemExit("--col_noise_max is the largest offset taken out in DN, > 0, got %r" % max_dn)
    return ColsSpec("auto", frames, gate, sigma, max_dn, *curve_argument('--col_noise_curve', curve, dpc, bit_depth))


GREEN_FLAGS = ("green_eq_curve", "green_eq_field", "green_eq_frames", "green_eq_gate", "green_eq_sigma", "green_eq_max", "green_eq_min_signal",
               "green_eq_black")


def add_green_arguments(p) -> None:
    """the nine flags of the green equilibration, beside --col_noise; `green_arguments` reads them"""
    p.add_argument('--green_eq', type=str, default=None, help='balance the two green planes of every frame on the device: FILE (a map python -m '
                   'rvdd_release_amd.green_eq wrote) or auto (found in the footage before streaming starts)')
    p.add_argument('--green_eq_curve', type=str, default=None, help='the curve of the gate, and of the black level: a,b[,floor] (var = a * m - b in DN '
                   'of the frames), auto (estimated from the footage), iso3200 or iso12800; default: the curve of --dpc')
    p.add_argument('--green_eq_field', type=str, default=None, help='with --green_eq auto: map (one gain per block of 32 x 32 cells, the default) or '
                   'flat (one gain for the frame)')
    p.add_argument('--green_eq_frames', type=int, default=None, help='with --green_eq auto: frames estimated per run, spread over the videos (default 32)')
    p.add_argument('--green_eq_gate', type=float, default=None, help='with --green_eq auto: the gate K in standard deviations of the curve (default 3)')
    p.add_argument('--green_eq_sigma', type=float, default=None, help='with --green_eq auto: a block is changed where its gain is at least this many '
                   'standard errors of its own estimate (default 3)')
    p.add_argument('--green_eq_max', type=float, default=None, help='with --green_eq auto: the largest gain taken out (default 0.10)')
    p.add_argument('--green_eq_min_signal', type=float, default=None, help="with --green_eq auto: the least level above black, in DN, at which a frame's "
                   'block counts (default (2^bit_depth - 1) / 64, a guess)')
    p.add_argument('--green_eq_black', type=float, default=None, help='the level without signal, in DN of the frames (default: b / a of the curve)')


def green_arguments(green_eq, curve, field, frames, gate, sigma, max_gain, min_signal, black, dpc, bit_depth):
    """--green_eq and its eight flags -> None (no --green_eq) or a GreenSpec, its curve as `rows_arguments` takes it (`curve_argument`;
    dpc = the DpcSpec of the run or None).  A FILE needs the black level alone: --green_eq_black, or a curve.  SystemExit where the
    flags do not fit together."""
    values = (curve, field, frames, gate, sigma, max_gain, min_signal, black)
    given = [n for n, v in zip(GREEN_FLAGS, values) if v is not None]
    if green_eq is None:
        if given:
            raise SystemExit("%s belong to --green_eq auto | FILE" % ', '.join('--' + n for n in GREEN_FLAGS))
        return None
    if black is not None and not abs(black) < INF:
        raise SystemExit("--green_eq_black is a level in DN, finite, got %r" % black)
    top = float((1 << int(bit_depth)) - 1)
    if green_eq != "auto":
        own = [n for n in given if n not in ("green_eq_curve", "green_eq_black")]
        if own:
            raise SystemExit("--%s belongs to --green_eq auto: --green_eq %s reads a map that is already made" % (own[0], green_eq))
        if curve is None and dpc is None:
            if black is None:
                raise SystemExit("--green_eq %s needs the level without signal: --green_eq_black DN, or a noise curve whose b / a it is "
                                 "(--green_eq_curve, or the curve of --dpc)" % green_eq)
            source, a, b, floor = "black", None, None, 1.0
        else:
            source, a, b, floor = curve_argument('--green_eq_curve', curve, dpc, bit_depth)
        return GreenSpec("file", green_eq, 0, 3.0, 3.0, 0.10, top / 64.0, "map", black, source, a, b, floor)
    field = "map" if field is None else field
    if field not in ("map", "flat"):
        raise SystemExit("--green_eq_field is map or flat, got %r" % field)
    frames, gate, sigma = 32 if frames is None else int(frames), 3.0 if gate is None else float(gate), 3.0 if sigma is None else float(sigma)
    if frames < 1:
        raise SystemExit("--green_eq_frames must be >= 1, got %d" % frames)
    if not (gate > 0 and gate < INF):
        raise SystemExit("--green_eq_gate is the gate in standard deviations, > 0 (around 3), got %r" % gate)
    if not (sigma >= 0 and sigma < INF):
        raise SystemExit("--green_eq_sigma is a number of standard errors, >= 0 (around 3), got %r" % sigma)
    max_gain = 0.10 if max_gain is None else float(max_gain)
    if not (max_gain > 0 and max_gain < INF):
        raise SystemExit("--green_eq_max is the largest gain taken out, > 0 (0.10 = 10 %%), got %r" % max_gain)
    min_signal = top / 64.0 if min_signal is None else float(min_signal)      # a guess, as the clamps of the rows and columns are
    if not (min_signal > 0 and min_signal < INF):
        raise SystemExit("--green_eq_min_signal is a level above black in DN, > 0, got %r" % min_signal)
    return GreenSpec("auto", None, frames, gate, sigma, max_gain, min_signal, field, black,
                     *curve_argument('--green_eq_curve', curve, dpc, bit_depth))


def match_arguments(match_noise, match_iso):
    """--match_noise / --match_iso -> None (neither) or a MatchSpec, a and b Python doubles in DN of --bit_depth -- None with
    --match_noise auto, for the command to estimate from the footage; SystemExit where the flags do not fit together."""
    if match_noise is None and match_iso is None:
        return None
    isos = ', '.join(str(k) for k in DPC_ISO_CURVES)
    if match_iso is None:
        raise SystemExit("--match_noise needs --match_iso {%s}: the checkpoint family whose curve the footage is mapped onto" % isos)
    if match_noise is None:
        raise SystemExit("--match_iso belongs to --match_noise a,b or --match_noise auto")
    if match_iso not in DPC_ISO_CURVES:
        raise SystemExit("--match_iso must be one of %s, got %r" % (isos, match_iso))
    _, a, b, _ = curve_word('--match_noise', match_noise, None)
    return MatchSpec(a, b, match_iso)


def add_report_arguments(p) -> None:
    """the two flags of the residual report, for `denoise`; `report_arguments` reads them"""
    p.add_argument('--report', type=str, default=None, help='FILE: one JSON line per video with the residual statistics of its outputs '
                   '(noisy - remosaic(denoised)) judged against a noise curve: no ground truth needed')
    p.add_argument('--report_noise', type=str, default=None, help='the curve of --report without --match_noise: a,b (var = a * m - b in DN of '
                   'the frames), auto (estimated from the footage), iso3200 or iso12800')


def report_arguments(report, report_noise, match, bit_depth):
    """--report / --report_noise -> None (no --report) or a ReportSpec: under the match (match = the MatchSpec of the run or None) the
    checkpoint family's curve in 12-bit DN, the unit the stage then measures in; otherwise the curve of --report_noise in DN of
    `bit_depth`.  SystemExit where the flags do not fit together."""
    if report is None:
        if report_noise is not None:
            raise SystemExit("--report_noise belongs to --report FILE")
        return None
    if match is not None:
        if report_noise is not None:
            raise SystemExit("--report_noise does not go with --match_noise: matched footage is judged against the curve of --match_iso, "
                             "the one the network sees")
        return ReportSpec(report, "match_iso%d" % match.iso, *DPC_ISO_CURVES[match.iso], 12)
    if report_noise is None:
        raise SystemExit("--report needs the noise curve the residual is judged against: --report_noise a,b (var = a * m - b in DN of the "
                         "frames), --report_noise auto (estimated from the footage), --report_noise iso3200 / iso12800 (a checkpoint "
                         "family's curve, rescaled to --bit_depth) -- or --match_noise, whose --match_iso curve then serves")
    source, a, b, _ = curve_word('--report_noise', report_noise, bit_depth)
    return ReportSpec(report, source, a, b, int(bit_depth))


REPORT_KEYS = ("ratio", "ratio_lo", "ratio_hi", "bias", "rho", "a_fit", "b_fit", "samples", "bins")


def report_record(acc, frames, spec, **names):
    """One record of --report: `names` (the video's key, ...), the frames measured, the fields of `runtime.resid_fit` on `acc` -- None,
    with "error": the library's message, where the fit refuses (fewer than 4 usable level bins) -- and the curve it was judged against."""
    from .runtime import resid_fit
    spec = ReportSpec(*spec)                       # a plain tuple in the fields' order serves as well
    rec = dict(names, frames=int(frames))
    try:
        rec.update(resid_fit(acc, spec.unit, spec.a, spec.b))
    except RuntimeError as err:
        rec.update({k: None for k in REPORT_KEYS}, error=str(err))
    rec["curve"] = {"a": spec.a, "b": spec.b, "bit_depth": spec.unit, "source": spec.source}
    return rec
