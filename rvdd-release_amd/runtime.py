"""Thin object wrapper over one ``rvdd_t`` handle.

PyTorch-ROCm is plumbing here: it owns device memory (``tensor.data_ptr()``
is what crosses the C ABI) and the HIP stream; all arithmetic is in
``librvdd_hip.so``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib

ARCH_BY_NAME = {
    "convunet": _lib.ARCH_CONVUNET,
    "convunet+feat": _lib.ARCH_CONVUNET_FEAT,
    "next": _lib.ARCH_CONVNEXT,
    "next+feat": _lib.ARCH_CONVNEXT_FEAT,
}

# enum rvdd_bayer, in order: the index of a pattern is its value (rvdd_set_option "bayer_pattern", rvdd_demosaic_ha_bayer)
BAYER_PATTERNS = ("gbrg", "grbg", "rggb", "bggr")


# enum rvdd_raw_layout by name (rvdd_ingest_raw, rvdd_video_push)
RAW_LAYOUTS = {"mosaic": _lib.RAW_MOSAIC, "packed_hwc": _lib.RAW_PACKED_HWC}
# enum rvdd_out_layout by name (rvdd_egress)
OUT_LAYOUTS = {"rgb_hwc": _lib.OUT_RGB_HWC, "mosaic": _lib.OUT_MOSAIC, "packed_hwc": _lib.OUT_PACKED_HWC}
# enum rvdd_bits_order by name (rvdd_ingest_bits, rvdd_egress_bits; option "stream_container" is the value plus one)
BITS_ORDERS = {"mipi": _lib.BITS_MIPI, "msb": _lib.BITS_MSB}
BITS_DEPTHS = (10, 12, 14)


def bits_row_bytes(width: int, bit_depth: int, order: str = "msb") -> int:
    """Bytes of one row of `width` packed samples of `bit_depth` bits: width * bit_depth / 8, for "msb" rounded up to a whole
    byte (zero pad bits); a "mipi" row is whole groups of 4 pixels (2 at 12 bits), which the library checks."""
    return (int(width) * int(bit_depth) + 7) // 8


# the reference's noise curves var(m) = ka * m - kb in 12-bit DN (dataset/generate_raw_from_RGB.py; rvdd_unprocess draws with them)
DPC_ISO_CURVES = {3200: (8.0034, 2043.51144), 12800: (28.3015, 6307.62081)}


def dpc_iso_curve(iso: int, bit_depth: int = 12) -> Tuple[float, float]:
    """The reference's noise curve of `iso` (3200 / 12800) in DN of `bit_depth`: with s = (2^bit_depth - 1) / 4095 a sample scales by s
    and its variance by s^2, so a = s * ka and b = s^2 * kb -- formed in double; the C ABI rounds them to f32 once."""
    if iso not in DPC_ISO_CURVES:
        raise ValueError(f"dpc_iso_curve: iso {iso!r} is not one of {', '.join(str(k) for k in DPC_ISO_CURVES)}")
    ka, kb = DPC_ISO_CURVES[iso]
    s = (2 ** int(bit_depth) - 1) / 4095.0
    return s * ka, s * s * kb


def dpc_cfg(k_hot: float, k_dead: float, noise_a: float, noise_b: float, var_floor: float = 1.0) -> "_lib.RvddDpcCfg":
    """struct rvdd_dpc_cfg of Python doubles, each rounded to f32 once"""
    return _lib.RvddDpcCfg(float(k_hot), float(k_dead), float(noise_a), float(noise_b), float(var_floor))


def dpc_detect_cfg(rule, tolerate: int = 0) -> "_lib.RvddDpcDetectCfg":
    """struct rvdd_dpc_detect_cfg: `rule` = `dpc_cfg(...)`, tolerate 0..3 (the library checks the range)"""
    return _lib.RvddDpcDetectCfg(rule, int(tolerate), 0)


def dpc_map_from_hits(hits, frames: int, share: float = 0.5):
    """The map of persistence counts: hits = what `RvddRuntime.dpc_detect` accumulated over `frames` frames (a tensor or array of
    32-bit words [4,hh,ww]: hot frames in the low 16 bits, dead frames in the high 16).  A sample is defective iff it was hot, or
    dead, in at least ceil(share * frames) of them.  -> (cellmask uint8 [hh,ww] with bit k = plane k, hot bool [4,hh,ww], dead bool
    [4,hh,ww]), NumPy arrays on the host (a device tensor is copied, which synchronises)."""
    import math
    import numpy as np
    if torch.is_tensor(hits):
        hits = hits.detach().cpu().contiguous().numpy()
    w = np.ascontiguousarray(hits).view(np.uint32)
    if w.ndim != 3 or w.shape[0] != 4:
        raise RuntimeError(f"dpc_map_from_hits: hits is [4,hh,ww] 32-bit words, got {w.shape}")
    if int(frames) < 1 or not 0.0 < float(share) <= 1.0:
        raise ValueError(f"dpc_map_from_hits: frames >= 1 and 0 < share <= 1, got frames = {frames}, share = {share}")
    need = max(1, math.ceil(float(share) * int(frames)))
    hot, dead = (w & 0xffff) >= need, (w >> 16) >= need
    bad = hot | dead
    mask = np.zeros(w.shape[1:], np.uint8)
    for k in range(4):
        mask |= bad[k].astype(np.uint8) << k
    return mask, hot, dead


def dpc_map_to_mosaic(cellmask):
    """cellmask uint8 [hh,ww] -> the file form: uint8 [2hh,2ww], sample (2y + (k >> 1), 2x + (k & 1)) = 255 where bit k is set, else 0"""
    import numpy as np
    m = np.asarray(cellmask)
    if m.ndim != 2 or m.dtype != np.uint8 or (m & 0xf0).any():
        raise RuntimeError("dpc_map_to_mosaic: cellmask is uint8 [hh,ww] with bits 0..3 only")
    out = np.zeros((2 * m.shape[0], 2 * m.shape[1]), np.uint8)
    for k in range(4):
        out[k >> 1::2, k & 1::2] = ((m >> k) & 1) * 255
    return out


def dpc_map_from_mosaic(plane):
    """The file form back: a one-sample image of the mosaic [2hh,2ww] (any integer or bool type, nonzero = defective) -> cellmask"""
    import numpy as np
    p = np.asarray(plane)
    if p.ndim != 2 or p.shape[0] % 2 or p.shape[1] % 2 or p.shape[0] < 2 or p.shape[1] < 2:
        raise RuntimeError(f"dpc_map_from_mosaic: a map is a one-sample image of the mosaic [2hh,2ww], got {p.shape}")
    m = np.zeros((p.shape[0] // 2, p.shape[1] // 2), np.uint8)
    for k in range(4):
        m |= (p[k >> 1::2, k & 1::2] != 0).astype(np.uint8) << k
    return m


def _host_call(name: str, *args) -> None:
    """One of the library's host-only entry points (no handle, no GPU needed); RuntimeError with its message where it refuses"""
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.rvdd_last_error(None).decode()}")


def _host_bytes(x, struct, message: str, n: Optional[int] = None):
    """The bytes of whole structs (n: of exactly n) as a flat uint8 array on the host: x is a struct instance, a tensor (a device tensor is
    copied, which synchronises), an array or bytes.  RuntimeError(`message`, got <bytes>) for any other size."""
    import numpy as np
    if torch.is_tensor(x):
        raw = x.detach().cpu().contiguous().view(torch.uint8).numpy()
    elif isinstance(x, np.ndarray):
        raw = np.ascontiguousarray(x).view(np.uint8)
    else:
        raw = np.frombuffer(bytes(x), np.uint8)
    if raw.size % C.sizeof(struct) or (n is not None and raw.size != n * C.sizeof(struct)):
        raise RuntimeError(f"{message}, got {raw.size}")
    return raw.reshape(-1)


def _host_map(x, dtype: Optional[str] = None, what: Optional[str] = None, shape: Tuple = ()):
    """x -- a NumPy array or a tensor (a device tensor is copied, which synchronises) -- as a contiguous host array.  With `what`, the
    caller's sentence: RuntimeError(`what`, got <dtype> <shape>) unless it is of `dtype` and of `shape` (None: any size along that axis)."""
    import numpy as np
    m = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if what is not None and (m.dtype != np.dtype(dtype) or m.ndim != len(shape) or any(want not in (None, got) for want, got in zip(shape, m.shape))):
        raise RuntimeError(f"{what}, got {m.dtype} {m.shape}")
    return m


def dpc_map_stats(cellmask) -> Dict[str, int]:
    """{"samples", "cells", "unfixable"} of a map uint8 [hh,ww] (rvdd_dpc_map_stats: on the host, no GPU needed): its defective
    samples and cells, and the samples no ring of which has a good site -- `dpc_map_apply` leaves those as they are."""
    m = _host_map(cellmask, "uint8", "dpc_map_stats: cellmask is uint8 [hh,ww]", (None, None))
    out = (C.c_int64 * 3)()
    _host_call("rvdd_dpc_map_stats", m.ctypes.data, m.shape[0], m.shape[1], out)
    return {"samples": int(out[0]), "cells": int(out[1]), "unfixable": int(out[2])}


NOISE_ACC_BYTES = C.sizeof(_lib.RvddNoiseAcc)     # struct rvdd_noise_acc: u32 hist[64][512], u64 msum[64], u64 counters[4]


def noise_acc_arrays(acc):
    """struct rvdd_noise_acc as numpy arrays (copies on the host): {"hist": int64 [64,512], "msum": int64 [64], "counters": int64 [4]}
    of an accumulator `RvddRuntime.noise_hist` returned (any tensor or array of its 131616 bytes)."""
    import numpy as np
    raw = _host_bytes(acc, _lib.RvddNoiseAcc, f"a noise accumulator is {NOISE_ACC_BYTES} bytes (struct rvdd_noise_acc)", 1)
    return {"hist": np.frombuffer(raw, np.uint32, 64 * 512).reshape(64, 512).astype(np.int64),
            "msum": np.frombuffer(raw, np.uint64, 64, 64 * 512 * 4).astype(np.int64),
            "counters": np.frombuffer(raw, np.uint64, 4, 64 * 512 * 4 + 64 * 8).astype(np.int64)}


def noise_fit(acc, bit_depth: int) -> Dict[str, float]:
    """The noise curve var(m) = a * m - b, in DN of `bit_depth`, from an accumulator of `RvddRuntime.noise_hist` (rvdd_noise_fit: on
    the host, no GPU needed; a device tensor is copied, which synchronises).  acc: the tensor, or any array / bytes of struct
    rvdd_noise_acc.  -> {"a", "b", "bins", "blocks", "m_min", "m_max", "rms"}; RuntimeError with the library's message where the
    fit refuses (fewer than 4 usable mean bins, or too little tonal range)."""
    host = _lib.RvddNoiseAcc.from_buffer_copy(
        _host_bytes(acc, _lib.RvddNoiseAcc, f"noise_fit: an accumulator is {NOISE_ACC_BYTES} bytes (struct rvdd_noise_acc)", 1))
    out = _lib.RvddNoiseCurve()
    _host_call("rvdd_noise_fit", C.byref(host), int(bit_depth), C.byref(out))
    return {"a": out.a, "b": out.b, "bins": int(out.bins), "blocks": int(out.blocks), "m_min": out.m_min, "m_max": out.m_max,
            "rms": out.rms}


FRAME_SIG_BYTES = C.sizeof(_lib.RvddFrameSig)      # struct rvdd_frame_sig: u32 hist[16][64], u64 sum[16][16]


def _frame_sig_bytes(sig, what: str):
    """the bytes of n whole structs rvdd_frame_sig as a C-contiguous uint8 array [n,6144] on the host (a device tensor is copied)"""
    raw = _host_bytes(sig, _lib.RvddFrameSig, f"{what}: a frame signature is {FRAME_SIG_BYTES} bytes (struct rvdd_frame_sig)")
    return raw.reshape(-1, FRAME_SIG_BYTES)


def frame_sig_arrays(sig):
    """Signatures of `RvddRuntime.frame_sigs` (the tensor [n,6144], or any array / bytes of n structs rvdd_frame_sig) as NumPy views of
    ONE host copy: {"hist": uint32 [n,16,64] (cells per band and level bin), "sum": uint64 [n,16,16] (sum of q per band and column)}."""
    import numpy as np
    raw = _frame_sig_bytes(sig, "frame_sig_arrays")
    rec = raw.reshape(-1).view(np.dtype([("hist", np.uint32, (16, 64)), ("sum", np.uint64, (16, 16))]))
    return {"hist": rec["hist"], "sum": rec["sum"]}


def cut_score(a, b, hh: int, ww: int) -> Tuple[float, float]:
    """(d_hist, d_grid) of two frames of hh x ww cells from their signatures (rvdd_cut_score: on the host, no GPU needed).  a, b: one
    struct rvdd_frame_sig each -- a row of the tensor `RvddRuntime.frame_sigs` returned (a device tensor is copied, which
    synchronises), an array or bytes of its 6144 bytes.  RuntimeError with the library's message for signatures of another frame size."""
    host = []
    for s, name in ((a, "a"), (b, "b")):
        raw = _frame_sig_bytes(s, "cut_score")
        if raw.shape[0] != 1:
            raise RuntimeError(f"cut_score: {name} is ONE signature of {FRAME_SIG_BYTES} bytes, got {raw.shape[0]}")
        host.append(_lib.RvddFrameSig.from_buffer_copy(raw.tobytes()))
    out = (C.c_double * 2)()
    _host_call("rvdd_cut_score", C.byref(host[0]), C.byref(host[1]), int(hh), int(ww), out)
    return float(out[0]), float(out[1])


RESID_ACC_BYTES = C.sizeof(_lib.RvddResidAcc)     # struct rvdd_resid_acc: six arrays of 64 64-bit words
RESID_FIELDS = tuple(name for name, _ in _lib.RvddResidAcc._fields_)
RESID_REPORT_FIELDS = tuple(name for name, _ in _lib.RvddResidReport._fields_ if name != "reserved")


def _resid_struct(acc, what: str) -> "_lib.RvddResidAcc":
    """ONE struct rvdd_resid_acc on the host: the struct itself, the dict `resid_acc_arrays` gives, or a tensor / array / bytes of its
    3072 bytes (a device tensor is copied, which synchronises)"""
    import numpy as np
    if isinstance(acc, _lib.RvddResidAcc):
        return acc
    if isinstance(acc, dict):
        acc = b"".join(np.ascontiguousarray(np.asarray(acc[name]).astype(np.int64 if name in ("s1", "s11") else np.uint64)).tobytes()
                       for name in RESID_FIELDS)
    return _lib.RvddResidAcc.from_buffer_copy(
        _host_bytes(acc, _lib.RvddResidAcc, f"{what}: an accumulator is {RESID_ACC_BYTES} bytes (struct rvdd_resid_acc)", 1))


def resid_acc_arrays(acc):
    """Accumulators of `RvddRuntime.resid_stats` / `resid_read` (a tensor [n,384] of 64-bit words, one struct, or any array / bytes of n
    structs rvdd_resid_acc) as NumPy arrays on the host: {"n", "msum", "s2", "n11": uint64 [n,64]; "s1", "s11": int64 [n,64]}."""
    import numpy as np
    raw = _host_bytes(acc, _lib.RvddResidAcc, f"resid_acc_arrays: an accumulator is {RESID_ACC_BYTES} bytes (struct rvdd_resid_acc)")
    words = raw.view(np.uint64).reshape(-1, 6, 64)
    return {name: (words[:, k].view(np.int64) if name in ("s1", "s11") else words[:, k]).copy() for k, name in enumerate(RESID_FIELDS)}


def resid_add(a, b):
    """the sum of two accumulators as `resid_acc_arrays` gives them (modulo 2^64, as the device adds)"""
    return {name: a[name] + b[name] for name in RESID_FIELDS}


def resid_fit(acc, bit_depth: int, a: float, b: float) -> Dict[str, float]:
    """ONE accumulator judged against the curve var(m) = a * m - b in DN of `bit_depth` (rvdd_resid_fit: on the host, no GPU needed).
    acc: as `_resid_struct` takes it; a dict of [1,64] or [64] arrays is one accumulator.  -> {"ratio", "ratio_lo", "ratio_hi", "bias",
    "rho", "a_fit", "b_fit", "samples", "bins"}; RuntimeError with the library's message where fewer than 4 level bins are usable."""
    host = _resid_struct(acc, "resid_fit")
    out = _lib.RvddResidReport()
    _host_call("rvdd_resid_fit", C.byref(host), int(bit_depth), float(a), float(b), C.byref(out))
    return {name: (int if name in ("samples", "bins") else float)(getattr(out, name)) for name in RESID_REPORT_FIELDS}


ROWS_ACC_BYTES = C.sizeof(_lib.RvddRowsAcc)       # struct rvdd_rows_acc: three counts, a reserved word, one 64-bit sum
ROWS_FIELDS = ("applied", "skipped", "clamped", "sum_q2")
ROWS_MAX_WW = 4096                                # the widest plane rvdd_rows_estimate takes


def rows_cfg(k_gate: float, noise_a: float, noise_b: float, var_floor: float = 1.0, max_dn: float = 64.0) -> "_lib.RvddRowsCfg":
    """struct rvdd_rows_cfg: the gate in standard deviations of the curve var(m) = noise_a * m - noise_b (DN of the frames' bit
    depth), the least variance assumed, and the largest offset taken out (DN)."""
    return _lib.RvddRowsCfg(float(k_gate), float(noise_a), float(noise_b), float(var_floor), float(max_dn))


def rows_acc_arrays(acc) -> Dict[str, "object"]:
    """Accumulators of `RvddRuntime.rows_estimate` (an int64 tensor [n,3] of 24-byte structs rvdd_rows_acc, one struct, or bytes) on
    the host: {"applied", "skipped", "clamped": uint32 [n]; "sum_q2": int64 [n]}."""
    import numpy as np
    raw = _host_bytes(acc, _lib.RvddRowsAcc, f"rows_acc_arrays: an accumulator is {ROWS_ACC_BYTES} bytes (struct rvdd_rows_acc)")
    words = raw.view(np.uint32).reshape(-1, 6)
    return {"applied": words[:, 0].copy(), "skipped": words[:, 1].copy(), "clamped": words[:, 2].copy(),
            "sum_q2": np.ascontiguousarray(words[:, 4:6]).view(np.int64).reshape(-1).copy()}


def rows_add(a, b):
    """the sum of two accumulators as `rows_acc_arrays` gives them"""
    return {name: a[name] + b[name] for name in ROWS_FIELDS}


def rows_rms(acc) -> float:
    """the rms offset in DN of accumulators as `rows_acc_arrays` gives them, summed: sqrt(sum_q2 / applied) / 16; 0 without a row"""
    applied, q2 = int(acc["applied"].sum()), int(acc["sum_q2"].sum())
    return (q2 / applied) ** 0.5 / 16.0 if applied else 0.0


def rows_floor_rms(noise_a: float, noise_b: float, var_floor: float, bit_depth: int, ww: int) -> float:
    """The rms the estimate has of its own on flat footage WITHOUT row noise, in DN: 1.35 sqrt(var(mid) / (2 ww)) with var at the
    mid level (2^bit_depth - 1) / 2 of the curve.  The median of eight normal samples has 0.168 of their variance, so a sample's
    d = x - median of eight has 1.168 var; the median of N = 2 ww independent such d has pi / (2 N) of theirs; sqrt(pi / 2 * 1.168) =
    1.355, and a gate at three standard deviations changes it by a per cent.  The rule gives 1.38 on white noise (tests/test_rows_host.py).
    A scene's vertical curvature adds to every d, so footage with detail sits somewhat above the floor without any row noise."""
    mid = ((1 << int(bit_depth)) - 1) / 2.0
    return 1.35 * (max(noise_a * mid - noise_b, var_floor) / (2.0 * ww)) ** 0.5


COLS_MAX_HH = 4096                                # the tallest plane rvdd_cols_estimate takes
COLS_STATES = ("unsupported", "applied", "clamped", "insignificant")      # mstate 0 .. 3 of rvdd_cols_fit


def cols_cfg(k_gate: float, noise_a: float, noise_b: float, var_floor: float = 1.0) -> "_lib.RvddColsCfg":
    """struct rvdd_cols_cfg: the gate in standard deviations of the curve var(m) = noise_a * m - noise_b (DN of the frames' bit
    depth) and the least variance assumed."""
    return _lib.RvddColsCfg(float(k_gate), float(noise_a), float(noise_b), float(var_floor))


def cols_fit(offsets, state, min_frames: int, k_sig: float = 3.0, max_dn: float = 64.0):
    """The static column map from the per-frame estimates of F frames (rvdd_cols_fit: on the host, no GPU needed; device tensors are
    copied, which synchronises).  offsets float32 [F,2,ww], state uint8 [F,2,ww], as `RvddRuntime.cols_estimate` gives them.
    -> (map float32 [2,ww] in DN, mstate uint8 [2,ww]: 0 unsupported, 1 applied, 2 applied and clamped, 3 insignificant,
    stats {"unsupported", "applied", "clamped", "insignificant", "sum_q2": ints; "floor_dn": float})."""
    import numpy as np
    o, st = _host_map(offsets), _host_map(state)
    if o.ndim != 3 or o.shape[1] != 2 or o.dtype != np.float32 or st.shape != o.shape or st.dtype != np.uint8:
        raise RuntimeError(f"cols_fit: offsets is float32 [F,2,ww] and state uint8 [F,2,ww], got {o.dtype} {o.shape} and {st.dtype} {st.shape}")
    F, _, ww = o.shape
    m = np.zeros((2, ww), np.float32)
    ms = np.zeros((2, ww), np.uint8)
    stats = _lib.RvddColsStats()
    cfg = _lib.RvddColsFitCfg(int(min_frames), float(k_sig), float(max_dn))
    _host_call("rvdd_cols_fit", o.ctypes.data, st.ctypes.data, F, ww, C.byref(cfg), m.ctypes.data, ms.ctypes.data, C.byref(stats))
    out = {name: int(stats.counts[i]) for i, name in enumerate(COLS_STATES)}
    out.update(sum_q2=int(stats.sum_q2), floor_dn=float(stats.floor_dn))
    return m, ms, out


GREEN_BLOCK = 32                                  # RVDD_GREEN_BLOCK: the cells along either side of a block of rvdd_green_estimate
GREEN_STATES = COLS_STATES                        # mstate 0 .. 3 of rvdd_green_fit


def green_grid(hh: int, ww: int) -> Tuple[int, int]:
    """(gh, gw): the blocks of a frame of hh x ww cells"""
    return (int(hh) + GREEN_BLOCK - 1) // GREEN_BLOCK, (int(ww) + GREEN_BLOCK - 1) // GREEN_BLOCK


def green_cfg(k_gate: float, noise_a: float, noise_b: float, var_floor: float = 1.0, black: Optional[float] = None) -> "_lib.RvddGreenCfg":
    """struct rvdd_green_cfg: the gate in standard deviations of the curve var(m) = noise_a * m - noise_b (DN of the frames' bit
    depth), the least variance assumed, and the level without signal -- None: noise_b / noise_a, where the curve's variance is zero
    (0 for a curve without a slope)."""
    if black is None:
        black = float(noise_b) / float(noise_a) if noise_a else 0.0
    return _lib.RvddGreenCfg(float(k_gate), float(noise_a), float(noise_b), float(var_floor), float(black))


def green_fit(e, level, state, black: float, min_frames: int, k_sig: float = 3.0, max_gain: float = 0.10, min_signal: float = 64.0):
    """The static map of green gains from the per-frame estimates of F frames (rvdd_green_fit: on the host, no GPU needed; device
    tensors are copied, which synchronises).  e, level float32 [F,gh,gw], state uint8 [F,gh,gw], as `RvddRuntime.green_estimate`
    gives them.  -> (map float32 [gh,gw]: gains of plane A relative to plane B, mstate uint8 [gh,gw]: 0 unsupported, 1 applied, 2
    applied and clamped, 3 insignificant, stats {"unsupported", "applied", "clamped", "insignificant", "sum_q2": ints; "floor",
    "flat_gain", "flat_se": floats; "flat_state": int})."""
    import numpy as np
    e, level, st = _host_map(e), _host_map(level), _host_map(state)
    if e.ndim != 3 or e.dtype != np.float32 or level.shape != e.shape or level.dtype != np.float32 or st.shape != e.shape or st.dtype != np.uint8:
        raise RuntimeError(f"green_fit: e and level are float32 [F,gh,gw] and state uint8 [F,gh,gw], got {e.dtype} {e.shape}, "
                           f"{level.dtype} {level.shape} and {st.dtype} {st.shape}")
    F, gh, gw = e.shape
    m = np.zeros((gh, gw), np.float32)
    ms = np.zeros((gh, gw), np.uint8)
    stats = _lib.RvddGreenStats()
    cfg = _lib.RvddGreenFitCfg(int(min_frames), float(k_sig), float(max_gain), float(min_signal))
    _host_call("rvdd_green_fit", e.ctypes.data, level.ctypes.data, st.ctypes.data, F, gh, gw, float(black), C.byref(cfg), m.ctypes.data,
               ms.ctypes.data, C.byref(stats))
    out = {name: int(stats.counts[i]) for i, name in enumerate(GREEN_STATES)}
    out.update(sum_q2=int(stats.sum_q2), floor=float(stats.floor), flat_gain=float(stats.flat_gain), flat_se=float(stats.flat_se),
               flat_state=int(stats.flat_state))
    return m, ms, out


def nearest_iso(a: float, b: float, bit_depth: int = 12, levels=(0.20, 0.45, 0.80)):
    """Which of DPC_ISO_CURVES lies closest to the curve (a, b) in DN of `bit_depth`: -> (iso, ratios), the ISO whose predicted
    standard deviation at 20 %, 45 % and 80 % of 2^bit_depth - 1 is nearest in the log (the largest |log ratio| over the levels is
    the distance), and the ratios sigma(a, b) / sigma(iso) at those levels."""
    import math
    top = 2 ** int(bit_depth) - 1
    best = None
    for iso in DPC_ISO_CURVES:
        ia, ib = dpc_iso_curve(iso, bit_depth)
        ratios = [math.sqrt(max(a * l * top - b, 0.0) / (ia * l * top - ib)) for l in levels]
        dist = max(abs(math.log(max(r, 1e-300))) for r in ratios)
        if best is None or dist < best[0]:
            best = (dist, iso, ratios)
    return best[1], best[2]


def match_cfg(scale: float, offset: float) -> "_lib.RvddMatchCfg":
    """struct rvdd_match_cfg of Python doubles, each rounded to f32 once"""
    return _lib.RvddMatchCfg(float(scale), float(offset))


def match_coeffs(a: float, b: float, bit_depth: int, iso_or_curve):
    """The affine map that takes footage of the noise curve var(m) = a * m - b, in DN of `bit_depth` (what `noise_fit` returns), onto a
    checkpoint's curve (rvdd_match_coeffs: on the host, no GPU needed).  iso_or_curve: 3200 / 12800, a key of DPC_ISO_CURVES, or the
    curve itself as (a_ref, b_ref) in 12-bit DN.  -> (cfg, s, t): cfg the struct `match_raw` / `unmatch_rgb` / `set_match` take
    (v' = cfg.scale * v + cfg.offset on samples in [-1,1]), s and t the map x' = s * x + t in 12-bit DN.  s > 1 means footage cleaner
    than the checkpoint's curve: the map stretches it beyond the trained range."""
    if isinstance(iso_or_curve, (tuple, list)):
        if len(iso_or_curve) != 2:
            raise ValueError(f"match_coeffs: a curve is (a_ref, b_ref) in 12-bit DN, got {iso_or_curve!r}")
        a_ref, b_ref = (float(v) for v in iso_or_curve)
    elif iso_or_curve in DPC_ISO_CURVES:
        a_ref, b_ref = DPC_ISO_CURVES[iso_or_curve]
    else:
        raise ValueError(f"match_coeffs: {iso_or_curve!r} is not one of {', '.join(str(k) for k in DPC_ISO_CURVES)} or a curve (a_ref, b_ref)")
    cfg, st = _lib.RvddMatchCfg(), (C.c_double * 2)()
    _host_call("rvdd_match_coeffs", float(a), float(b), int(bit_depth), a_ref, b_ref, C.byref(cfg), st)
    return cfg, float(st[0]), float(st[1])


def raw_frames_to_device(frames, device) -> torch.Tensor:
    """Host sensor frames (a numpy array or CPU tensor of uint16 / int16 / float32) -> a tensor on `device` that
    `ingest_raw` / `video_push` accept.  uint16 arrays travel as their int16 view: the bytes are what crosses the ABI."""
    import numpy as np
    if not torch.is_tensor(frames):
        a = np.ascontiguousarray(frames)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        elif a.dtype not in (np.int16, np.float32):
            raise RuntimeError(f"raw frames must be uint16 or float32, got {a.dtype}")
        frames = torch.from_numpy(a)
    return frames.to(device)


_WORD32 = (torch.int32, getattr(torch, "uint32", torch.int32))     # counters the library adds to: either reading of the 32 bits


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev_tensor(t, name: str, device: Optional[int], dtype=torch.float32, shape=None, nbytes: Optional[int] = None,
                contiguous: Optional[str] = "copy", form: Optional[str] = None) -> torch.Tensor:
    """The one check of a tensor that crosses the ABI: on the GPU, on cuda:`device` (None: any), then its form -- `dtype` (one, a
    tuple of alternatives, None: any), `shape` (None: any; an entry None: any extent), `nbytes`, and its layout: contiguous "copy"
    returns a dense copy of a strided tensor, "require" refuses one (an output, or frames corrected in place), None leaves the
    strides to the caller.  form: the sentence that describes the form, for callers whose message names all of it at once."""
    if not getattr(t, "is_cuda", False):
        raise RuntimeError(f"{name} must be a GPU tensor (rvdd has no CPU path)")
    if device is not None and t.device.index != device:
        raise RuntimeError(f"{name} lives on cuda:{t.device.index} but this runtime drives cuda:{device}")
    if shape is not None and t.shape != shape and (        # shape: a tuple or a torch.Size, which compare as tuples
            len(shape) != t.dim() or any(e is not None and e != g for e, g in zip(shape, t.shape))):
        raise RuntimeError(f"{form}, got {t.dtype} {tuple(t.shape)}" if form else f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if dtype is not None and t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
        raise RuntimeError(f"{form}, got {t.dtype} {tuple(t.shape)}" if form else f"{name} must be {str(dtype).replace('torch.', '')}")
    if nbytes is not None and t.numel() * t.element_size() != nbytes:
        raise RuntimeError(f"{form}, got {t.dtype} {tuple(t.shape)}" if form else f"{name} must hold {nbytes} bytes, got {t.numel() * t.element_size()}")
    if contiguous is None or t.is_contiguous():
        return t
    if contiguous == "require":
        raise RuntimeError(f"{form}, got {t.dtype} {tuple(t.shape)} with strides {t.stride()}" if form else
                           f"{name} must be contiguous (it is written where it lies)")
    return t.contiguous()


def _out_or_new(out, name: str, shape, tdev: torch.device, dtype=torch.float32, *, zero: bool = False, nbytes: Optional[int] = None,
                form: Optional[str] = None) -> torch.Tensor:
    """The output of an op: a new tensor of `shape` and `dtype` (the first of a tuple) on `tdev` -- zeroed for an accumulator -- or
    the caller's `out`, checked: on that device, of that dtype and shape (with nbytes: of any shape of that many bytes), contiguous."""
    if out is None:
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype[0] if isinstance(dtype, tuple) else dtype, device=tdev)
    return _dev_tensor(out, name, tdev.index, dtype, None if nbytes is not None else shape, nbytes, "require", form)


def _frames(t, c: int, spec: str, name: str, device: int, contiguous: str = "copy"):
    """A batch of c-channel frames [n,c,h,w] -> (the tensor checked, n, h, w).  spec: "<op>: <what> is [n,c,h,w]", the sentence of
    the message for anything else -- said first, whatever device the argument is on."""
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != c:
        raise RuntimeError(f"{spec}, got {tuple(getattr(t, 'shape', ()))}")
    return _dev_tensor(t, name, device, contiguous=contiguous), t.shape[0], t.shape[2], t.shape[3]


def _raw_dtype(dtype) -> Optional[int]:
    """enum rvdd_raw_dtype of a torch dtype: float32, or uint16 / int16 (read as the same 16 bits, unsigned: the view numpy's uint16
    arrays upload as where torch's own uint16 support is thin); None for any other"""
    if dtype == torch.float32:
        return _lib.RAW_F32
    if dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
        return _lib.RAW_U16
    return None


def _pattern_index(pattern, who: str) -> int:
    if pattern not in BAYER_PATTERNS:
        raise ValueError(f"{who}: pattern {pattern!r} is not one of {', '.join(BAYER_PATTERNS)}")
    return BAYER_PATTERNS.index(pattern)


def _raw_frames(t: torch.Tensor, layout: str, name: str, device: int):
    """-> (contiguous tensor, enum rvdd_raw_dtype, enum rvdd_raw_layout, n, hh, ww) of sensor frames [n,2hh,2ww] ("mosaic")
    or [n,hh,ww,4] ("packed_hwc"), of the dtypes `_raw_dtype` knows."""
    if layout not in RAW_LAYOUTS:
        raise ValueError(f"{name}: layout {layout!r} is not one of {', '.join(RAW_LAYOUTS)}")
    t = _dev_tensor(t, f"{name}: frames", device, dtype=None)
    dtype = _raw_dtype(t.dtype)
    if dtype is None:
        raise RuntimeError(f"{name}: frames must be uint16 (or its int16 view) or float32, got {t.dtype}")
    if layout == "mosaic":
        if t.dim() != 3 or t.shape[1] % 2 or t.shape[2] % 2:
            raise RuntimeError(f"{name}: mosaic frames are [n,2hh,2ww], got {tuple(t.shape)}")
        n, hh, ww = t.shape[0], t.shape[1] // 2, t.shape[2] // 2
    else:
        if t.dim() != 4 or t.shape[3] != 4:
            raise RuntimeError(f"{name}: packed_hwc frames are [n,hh,ww,4], got {tuple(t.shape)}")
        n, hh, ww = t.shape[0], t.shape[1], t.shape[2]
    return t, dtype, RAW_LAYOUTS[layout], n, hh, ww


def _batch_strided(t: Optional[torch.Tensor], shape: Tuple[int, ...], name: str, device: int):
    """A [B,C,h,w] input of a step: dense inside a sequence, any stride from one sequence to the next (a channel
    slice of the reference's `n` / `flow` tensors is exactly that).  -> (tensor, batch stride in floats); copies
    only what is not laid out like that."""
    if t is None:
        return None, 0
    _dev_tensor(t, name, device, torch.float32, shape, None, None)       # positional: once per input of every step
    C, h, w = shape[1:]
    if t.stride()[1:] == (h * w, w, 1) and t.stride(0) >= C * h * w:
        return t, t.stride(0)
    t = t.contiguous()
    return t, C * h * w


def _common_stride(items, dense: int):
    """[(tensor or None, batch stride)] of `_batch_strided` -> (the items, their one batch stride); `dense` where all are None"""
    strides = {st for t, st in items if t is not None}
    if len(strides) > 1:        # slices of different tensors: fall back to dense copies
        return [(None if t is None else t.contiguous(), dense) for t, _ in items], dense
    return items, (strides.pop() if strides else dense)


class RvddRuntime:
    """One handle = one device, one (arch, future, B, H, W) configuration."""

    def __init__(self, arch: str, future: int, batch: int, height: int, width: int, device: int = 0):
        self.lib = _lib.load()
        self.arch = arch
        self.future = int(future)
        self.B, self.H, self.W = int(batch), int(height), int(width)
        self.device = int(device)
        self.feat = arch.endswith("+feat")
        cfg = _lib.RvddCfg(ARCH_BY_NAME[arch], self.future, self.B, self.H, self.W, self.device)
        h = C.c_void_p()
        rc = self.lib.rvdd_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"rvdd_create failed ({rc}): {self.lib.rvdd_last_error(None).decode()}")
        self.h = h
        self._tdev = torch.device("cuda", self.device)

    # -- helpers ----------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != 0 and not (getattr(self, "h", None) is not None and self.h.value):
            raise RuntimeError(f"{what}: this RvddRuntime is closed (evicted from the denoiser's cache of frame sizes, or "
                               "closed explicitly) -- fetch a live one with net.runtime_for(B, H, W)")
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.rvdd_last_error(self.h).decode()}")

    def _stream(self) -> int:
        return torch.cuda.current_stream(self._tdev).cuda_stream

    def _set_cfg(self, name: str, cfg):
        """a stage's setter `name` with its struct, or NULL for None = off"""
        self._check(getattr(self.lib, name)(self.h, None if cfg is None else C.byref(cfg)), name)

    def _slot_read(self, name: str, struct, slot: int):
        """the reader `name` of a stage's per-slot accumulator -> the host copy of slot `slot`'s, which the call zeroes on the device"""
        host = struct()
        self._check(getattr(self.lib, name)(self.h, int(slot), C.byref(host), self._stream()), name)
        return host

    def _in_place(self, who: str, packed, gray, between=None):
        """packed [n,4,hh,ww] and gray [n,hh,ww] (or None) of a call that writes both where they lie: contiguous, on this device.
        between(n, hh, ww): the caller's check of its own tensor, made between the two as it always was -> (packed, n, hh, ww, its result)"""
        packed, n, hh, ww = _frames(packed, 4, f"{who}: packed is [n,4,hh,ww]", "packed", self.device, contiguous="require")
        mine = between(n, hh, ww) if between else None
        if gray is not None:
            _dev_tensor(gray, "gray", self.device, shape=(n, hh, ww), contiguous="require")
        return packed, n, hh, ww, mine

    def _pattern(self, pattern: Optional[str], who: str) -> int:
        """enum rvdd_bayer of one of BAYER_PATTERNS; None = the pattern set_option("bayer_pattern", ...) gave this runtime"""
        return getattr(self, "bayer_pattern", 0) if pattern is None else _pattern_index(pattern, who)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.rvdd_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights (BaseModel.load_networks, models/base_model.py:173-196) ---
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        for k, v in sd.items():
            t = v.detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            self._check(self.lib.rvdd_set_weight(self.h, k.encode(), t.data_ptr(), shape, t.dim()),
                        f"rvdd_set_weight({k})")
        self._check(self.lib.rvdd_finalize_weights(self.h), "rvdd_finalize_weights")

    # -- hot path -----------------------------------------------------------
    def reset(self, slots=None):
        """FirstOfVideo.  `slots=None`: every sequence (rvdd_reset); otherwise the sequences that start a new video on the
        next step, as an iterable of slot indices or a [B] bool mask (rvdd_reset_slots; the others carry on)."""
        if slots is None:
            self._check(self.lib.rvdd_reset(self.h), "rvdd_reset")
            return
        items = slots.tolist() if hasattr(slots, "tolist") else list(slots)
        mask = (C.c_uint8 * self.B)()
        if items and all(isinstance(v, bool) for v in items):      # a [B] bool mask
            if len(items) != self.B:
                raise ValueError(f"reset: a slot mask needs {self.B} entries, got {len(items)}")
            for b, v in enumerate(items):
                mask[b] = int(v)
        else:                                                     # slot indices
            for b in items:
                b = int(b)
                if not 0 <= b < self.B:
                    raise ValueError(f"reset: slot {b} outside 0..{self.B - 1}")
                mask[b] = 1
        self._check(self.lib.rvdd_reset_slots(self.h, mask), "rvdd_reset_slots")

    def set_option(self, name: str, value: int):
        """Options of recurrentModel that change what a step does; "no_warp" = --no_warp (flows then unused)."""
        self._check(self.lib.rvdd_set_option(self.h, name.encode(), int(value)), "rvdd_set_option")
        if name == "no_warp":
            self.no_warp = bool(value)
        if name == "bayer_pattern":
            self.bayer_pattern = int(value)
        if name == "stream_container":
            self.stream_container = int(value)

    def move_slots(self, pairs):
        """The whole recurrent state of slot `f` replaces that of slot `t` for every (f, t) of `pairs`, one launch
        (rvdd_move_slots).  The pairs are disjoint; a source slot is undefined afterwards."""
        pairs = [(int(f), int(t)) for f, t in pairs]
        n = len(pairs)
        if n == 0:
            return
        fr = (C.c_int32 * n)(*[f for f, _ in pairs])
        to = (C.c_int32 * n)(*[t for _, t in pairs])
        self._check(self.lib.rvdd_move_slots(self.h, fr, to, n, self._stream()), "rvdd_move_slots")

    def step(self, raw_prev, raw_cur, raw_next, flow_prev, flow_next, out=None, live=None) -> torch.Tensor:
        """One frame for every sequence.  `live=n`: slots 0 .. n-1 alone (rvdd_step_live); the tensors then hold n
        sequences and the other slots are undefined afterwards."""
        B, H, W = self.B, self.H, self.W
        if live is not None:
            live = int(live)
            if not 1 <= live <= self.B:
                raise ValueError(f"step: live={live} outside 1..{self.B}")
            B = live
        rs, fs = (B, 4, H // 2, W // 2), (B, 2, H // 2, W // 2)
        if getattr(self, "no_warp", False):
            flow_prev = flow_next = None
        elif flow_prev is None:
            raise RuntimeError("rvdd_step: flow_prev is required (no --no_warp option set on this runtime)")
        dev = self.device
        raws = [_batch_strided(raw_prev, rs, "raw_prev", dev), _batch_strided(raw_cur, rs, "raw_cur", dev), _batch_strided(raw_next, rs, "raw_next", dev)]
        flows = [_batch_strided(flow_prev, fs, "flow_prev", dev), _batch_strided(flow_next, fs, "flow_next", dev)]
        if raws[1][0] is None:
            raise RuntimeError("rvdd_step: raw_cur is required")
        raws, rstride = _common_stride(raws, rs[1] * rs[2] * rs[3])
        flows, fstride = _common_stride(flows, fs[1] * fs[2] * fs[3])
        out = _out_or_new(out, "out", (B, 3, H, W), self._tdev)
        if live is not None:
            self._check(self.lib.rvdd_step_live(self.h, live, _ptr(raws[0][0]), _ptr(raws[1][0]), _ptr(raws[2][0]),
                                                _ptr(flows[0][0]), _ptr(flows[1][0]), rstride, fstride, _ptr(out),
                                                self._stream()), "rvdd_step_live")
            return out
        self._check(self.lib.rvdd_step_strided(self.h, _ptr(raws[0][0]), _ptr(raws[1][0]), _ptr(raws[2][0]),
                                               _ptr(flows[0][0]), _ptr(flows[1][0]), rstride, fstride, _ptr(out),
                                               self._stream()), "rvdd_step")
        return out

    # -- raw footage ----------------------------------------------------------
    def ingest_raw(self, frames: torch.Tensor, bit_depth: int = 12, layout: str = "mosaic", want_packed: bool = True,
                   want_gray: bool = True):
        """Sensor frames -> (packed [n,4,hh,ww] in [-1,1], gray [n,hh,ww] in DN), None for an output not wanted
        (rvdd_ingest_raw).  frames: [n,2hh,2ww] ("mosaic") or [n,hh,ww,4] ("packed_hwc") GPU tensor of torch.uint16,
        torch.int16 (the same 16 bits, read unsigned) or torch.float32 digital numbers."""
        t, dtype, lay, n, hh, ww = _raw_frames(frames, layout, "ingest_raw", self.device)
        packed = torch.empty(n, 4, hh, ww, dtype=torch.float32, device=self._tdev) if want_packed else None
        gray = torch.empty(n, hh, ww, dtype=torch.float32, device=self._tdev) if want_gray else None
        self._check(self.lib.rvdd_ingest_raw(self.h, _ptr(t), dtype, lay, n, hh, ww, int(bit_depth), _ptr(packed), _ptr(gray),
                                             self._stream()), "rvdd_ingest_raw")
        return packed, gray

    def gray_of_rgb(self, rgb: torch.Tensor, bit_depth: int = 12, pattern: Optional[str] = None) -> torch.Tensor:
        """[n,3,H,W] RGB in [-1,1] -> [n,H/2,W/2]: the gray plane, in DN, of its re-mosaic in `pattern` (one of BAYER_PATTERNS;
        None = the pattern set_option("bayer_pattern", ...) gave this runtime) -- what `ingest_raw` gives for the sensor frame
        (rvdd_gray_of_rgb)."""
        pat = self._pattern(pattern, "gray_of_rgb")
        rgb, n, H, W = _frames(rgb, 3, "gray_of_rgb: rgb is [n,3,H,W]", "rgb", self.device)
        gray = torch.empty(n, H // 2, W // 2, dtype=torch.float32, device=self._tdev)
        self._check(self.lib.rvdd_gray_of_rgb(self.h, _ptr(rgb), n, H, W, pat, int(bit_depth), _ptr(gray), self._stream()),
                    "rvdd_gray_of_rgb")
        return gray

    def egress(self, rgb: torch.Tensor, layout: str = "rgb_hwc", dtype: torch.dtype = getattr(torch, "uint16", torch.int16),
               bit_depth: int = 12, pattern: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n,3,H,W] RGB in [-1,1] -> the frames in a sensor container (rvdd_egress): digital numbers of `bit_depth` bits as
        [n,H,W,3] ("rgb_hwc"), the re-mosaic in `pattern` as one plane [n,H,W] ("mosaic") or as [n,H/2,W/2,4] ("packed_hwc").
        dtype torch.uint16 (rounded half to even, clamped to 0 .. 2^bit_depth - 1; torch.int16 gives the same 16 bits as the
        view `ingest_raw` reads) or torch.float32 (neither rounded nor clamped).  pattern: one of BAYER_PATTERNS, None = the
        pattern set_option("bayer_pattern", ...) gave this runtime.  out: a tensor of that shape and dtype to write into."""
        if layout not in OUT_LAYOUTS:
            raise ValueError(f"egress: layout {layout!r} is not one of {', '.join(OUT_LAYOUTS)}")
        pat = self._pattern(pattern, "egress")
        dt = _raw_dtype(dtype)
        if dt is None:
            raise RuntimeError(f"egress: dtype must be torch.uint16 (or torch.int16, its view) or torch.float32, got {dtype}")
        rgb, n, H, W = _frames(rgb, 3, "egress: rgb is [n,3,H,W]", "rgb", self.device)
        shape = {"rgb_hwc": (n, H, W, 3), "mosaic": (n, H, W), "packed_hwc": (n, H // 2, W // 2, 4)}[layout]
        out = _out_or_new(out, "egress: out", shape, self._tdev, dtype,
                          form=f"egress: out must be a contiguous {dtype} tensor of shape {shape}")
        self._check(self.lib.rvdd_egress(self.h, _ptr(rgb), n, H, W, OUT_LAYOUTS[layout], dt, int(bit_depth), pat, _ptr(out),
                                         self._stream()), "rvdd_egress")
        return out

    def _bits_frames(self, frames: torch.Tensor, order: str, bit_depth: int, n: int, hh: int, ww: int, name: str) -> torch.Tensor:
        """the uint8 GPU tensor of n tight frames of 2hh rows of bits_row_bytes(2ww, bit_depth, order) bytes, checked"""
        if order not in BITS_ORDERS:
            raise ValueError(f"{name}: order {order!r} is not one of {', '.join(BITS_ORDERS)}")
        _dev_tensor(frames, f"{name}: frames", self.device, dtype=torch.uint8, contiguous="require",
                    form=f"{name}: packed frames are a contiguous uint8 tensor")
        rb = bits_row_bytes(2 * ww, bit_depth, order)
        if frames.numel() != n * 2 * hh * rb:
            raise RuntimeError(f"{name}: {n} frames of {2 * hh} rows of {rb} bytes ({2 * ww} samples of {bit_depth} bits, {order}) are "
                               f"{n * 2 * hh * rb} bytes, got {frames.numel()}")
        return frames

    def ingest_bits(self, frames: torch.Tensor, order: str, bit_depth: int, hh: int, ww: int, n: Optional[int] = None,
                    want_packed: bool = True, want_gray: bool = True):
        """Frames of packed 10 / 12 / 14-bit samples -> (packed [n,4,hh,ww], gray [n,hh,ww]) exactly as `ingest_raw` gives them for
        the unpacked uint16 mosaic (rvdd_ingest_bits).  frames: contiguous uint8 GPU tensor, n tight frames of 2hh rows of
        bits_row_bytes(2ww, bit_depth, order) bytes ([n,2hh,row_bytes], or flat); order "mipi" (CSI-2 RAW10 / 12 / 14) or "msb"
        (TIFF FillOrder 1).  n: None = frames.shape[0]."""
        hh, ww = int(hh), int(ww)
        if n is None:
            n = frames.shape[0] if torch.is_tensor(frames) and frames.dim() == 3 else 1
        t = self._bits_frames(frames, order, int(bit_depth), int(n), hh, ww, "ingest_bits")
        packed = torch.empty(n, 4, hh, ww, dtype=torch.float32, device=self._tdev) if want_packed else None
        gray = torch.empty(n, hh, ww, dtype=torch.float32, device=self._tdev) if want_gray else None
        self._check(self.lib.rvdd_ingest_bits(self.h, _ptr(t), BITS_ORDERS[order], n, hh, ww, int(bit_depth), _ptr(packed), _ptr(gray),
                                              self._stream()), "rvdd_ingest_bits")
        return packed, gray

    def egress_bits(self, rgb: torch.Tensor, order: str, bit_depth: int, pattern: Optional[str] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n,3,H,W] RGB in [-1,1] -> uint8 [n,H,row_bytes]: the uint16 mosaic `egress` writes, its samples packed `bit_depth` = 10 /
        12 / 14 bits each in `order` ("mipi" / "msb"), pad bits zero (rvdd_egress_bits).  pattern: one of BAYER_PATTERNS, None =
        the pattern set_option("bayer_pattern", ...) gave this runtime.  out: a contiguous uint8 GPU tensor of n * H * row_bytes
        elements to write into."""
        if order not in BITS_ORDERS:
            raise ValueError(f"egress_bits: order {order!r} is not one of {', '.join(BITS_ORDERS)}")
        pat = self._pattern(pattern, "egress_bits")
        rgb, n, H, W = _frames(rgb, 3, "egress_bits: rgb is [n,3,H,W]", "rgb", self.device)
        rb = bits_row_bytes(W, int(bit_depth), order)
        out = _out_or_new(out, "egress_bits: out", (n, H, rb), self._tdev, torch.uint8, nbytes=n * H * rb,
                          form=f"egress_bits: out must be a contiguous uint8 tensor of {n * H * rb} elements")
        self._check(self.lib.rvdd_egress_bits(self.h, _ptr(rgb), n, H, W, BITS_ORDERS[order], int(bit_depth), pat, _ptr(out),
                                              self._stream()), "rvdd_egress_bits")
        return out

    # -- defective-pixel correction -----------------------------------------------
    def dpc(self, packed: torch.Tensor, cfg, bit_depth: int = 12, gray: Optional[torch.Tensor] = None,
            counts: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Hot and stuck samples of packed frames [n,4,hh,ww] (as `ingest_raw` writes them) replaced by the median of their eight
        same-colour neighbours (rvdd_dpc; `cfg`: `dpc_cfg(k_hot, k_dead, noise_a, noise_b, var_floor)`, the curve in DN of
        `bit_depth`).  -> the corrected frames (`out`, or a new tensor; never `packed` itself).  gray [n,hh,ww]: patched in place at
        the cells with a flag; counts: int32 / uint32 [n,2] on the device, the hot / dead flags of every frame are added to it."""
        packed, n, hh, ww = _frames(packed, 4, "dpc: packed is [n,4,hh,ww]", "packed", self.device)
        out = _out_or_new(out, "out", packed.shape, self._tdev)
        if gray is not None:
            _dev_tensor(gray, "gray", self.device, shape=(n, hh, ww), contiguous="require")
        if counts is not None:
            _dev_tensor(counts, "dpc: counts", self.device, dtype=_WORD32, shape=(n, 2), contiguous="require",
                        form=f"dpc: counts is a contiguous int32 / uint32 tensor [{n},2] on cuda:{self.device}")
        self._check(self.lib.rvdd_dpc(self.h, _ptr(packed), _ptr(out), _ptr(gray), n, hh, ww, int(bit_depth), C.byref(cfg), _ptr(counts),
                                      self._stream()), "rvdd_dpc")
        return out

    # -- the static defect map -----------------------------------------------------------
    def dpc_detect(self, packed: torch.Tensor, cfg, bit_depth: int = 12, hits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The hot and dead frames of every site of packed frames [n,4,hh,ww] added to `hits` (rvdd_dpc_detect; cfg:
        `dpc_detect_cfg(dpc_cfg(...), tolerate)`): a device int32 tensor [4,hh,ww] -- None = a new zeroed one -- which is returned;
        hot frames in the low 16 bits, dead frames in the high 16, each saturating at 65535.  Accumulate any number of calls, then
        `dpc_map_from_hits(hits, frames, share)`.  Nothing is synchronised."""
        packed, n, hh, ww = _frames(packed, 4, "dpc_detect: packed is [n,4,hh,ww]", "packed", self.device)
        hits = _out_or_new(hits, "dpc_detect: hits", (4, hh, ww), self._tdev, _WORD32, zero=True,
                           form=f"dpc_detect: hits is a contiguous int32 / uint32 tensor [4,{hh},{ww}] on cuda:{self.device}")
        self._check(self.lib.rvdd_dpc_detect(self.h, _ptr(packed), n, hh, ww, int(bit_depth), C.byref(cfg), _ptr(hits), self._stream()),
                    "rvdd_dpc_detect")
        return hits

    def set_dpc_map(self, cellmask=None):
        """The handle's defect map (rvdd_set_dpc_map): cellmask uint8 [hh,ww] on the host (a NumPy array or CPU tensor; bit k = plane k
        of the cell is defective), None = off (the default).  `dpc_map_apply` corrects by it, and `video_push` corrects every
        ingested frame by it, in front of `set_dpc`'s rule.  Synchronises the device."""
        if cellmask is None:
            self._check(self.lib.rvdd_set_dpc_map(self.h, None, 0, 0), "rvdd_set_dpc_map")
            return
        m = _host_map(cellmask, "uint8", "set_dpc_map: cellmask is uint8 [hh,ww]", (None, None))
        self._check(self.lib.rvdd_set_dpc_map(self.h, m.ctypes.data, m.shape[0], m.shape[1]), "rvdd_set_dpc_map")

    def dpc_map_apply(self, packed: torch.Tensor, bit_depth: int = 12, gray: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed frames [n,4,hh,ww] corrected by the handle's map IN PLACE (rvdd_dpc_map_apply), gray [n,hh,ww] re-formed at the
        map's cells.  -> packed.  Both must be contiguous: they are written where they lie.  Nothing is synchronised."""
        packed, n, hh, ww, _ = self._in_place("dpc_map_apply", packed, gray)
        self._check(self.lib.rvdd_dpc_map_apply(self.h, _ptr(packed), _ptr(gray), n, hh, ww, int(bit_depth), self._stream()),
                    "rvdd_dpc_map_apply")
        return packed

    # -- the noise curve from the footage ---------------------------------------------
    def noise_hist(self, packed: torch.Tensor, bit_depth: int = 12, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 8 x 8 block statistics of packed frames [n,4,hh,ww] (as `ingest_raw` / `ingest_bits` / `dpc` write them) added to `acc`
        (rvdd_noise_hist): a device tensor holding struct rvdd_noise_acc -- int32 [32904]; None = a new zeroed one -- which is
        returned.  Accumulate any number of calls of one bit depth, then `noise_fit(acc, bit_depth)`; `noise_acc_arrays(acc)` gives
        the histogram, the sums of means and the counters.  Nothing is synchronised."""
        packed, n, hh, ww = _frames(packed, 4, "noise_hist: packed is [n,4,hh,ww]", "packed", self.device)
        if acc is None:
            acc = torch.zeros(NOISE_ACC_BYTES // 4, dtype=torch.int32, device=self._tdev)
        else:           # words of any type: the struct's bytes
            _dev_tensor(acc, "noise_hist: acc", self.device, dtype=None, nbytes=NOISE_ACC_BYTES, contiguous="require",
                        form=f"noise_hist: acc is a contiguous tensor of {NOISE_ACC_BYTES} bytes on cuda:{self.device} (what noise_hist returned)")
        self._check(self.lib.rvdd_noise_hist(self.h, _ptr(packed), n, hh, ww, int(bit_depth), _ptr(acc), self._stream()), "rvdd_noise_hist")
        return acc

    # -- scene cuts: one signature per frame ----------------------------------------------
    def frame_sigs(self, gray: torch.Tensor, bit_depth: int = 12, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The signatures of gray planes [n,hh,ww] (f32, in DN: what `ingest_raw` / `ingest_bits` return) as a device uint8 tensor
        [n,6144], one struct rvdd_frame_sig per frame (rvdd_frame_sigs).  out: a contiguous uint8 tensor of that shape on this device to
        overwrite.  `frame_sig_arrays` gives the counts and sums, `cut_score(sig[k - 1], sig[k], hh, ww)` the distance of two frames.
        Nothing is synchronised."""
        if not torch.is_tensor(gray) or gray.dim() != 3:
            raise RuntimeError(f"frame_sigs: gray is [n,hh,ww], got {tuple(getattr(gray, 'shape', ()))}")
        n, hh, ww = gray.shape
        gray = _dev_tensor(gray, "gray", self.device)
        out = _out_or_new(out, "frame_sigs: out", (n, FRAME_SIG_BYTES), self._tdev, torch.uint8,
                          form=f"frame_sigs: out is a contiguous uint8 tensor [{n},{FRAME_SIG_BYTES}] on cuda:{self.device}")
        self._check(self.lib.rvdd_frame_sigs(self.h, _ptr(gray), n, hh, ww, int(bit_depth), _ptr(out), self._stream()), "rvdd_frame_sigs")
        return out

    # -- footage matched to the checkpoint's noise curve ---------------------------------
    def _match(self, fn, name: str, t: torch.Tensor, c: int, cfg, out: Optional[torch.Tensor]) -> torch.Tensor:
        t, n, d0, d1 = _frames(t, c, f"{name}: the frames are [n,{c},h,w]", "frames", self.device)
        out = _out_or_new(out, "out", t.shape, self._tdev)
        self._check(fn(self.h, _ptr(t), _ptr(out), n, d0, d1, None if cfg is None else C.byref(cfg), self._stream()), "rvdd_" + name)
        return out

    def match_raw(self, packed: torch.Tensor, cfg, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed frames [n,4,hh,ww] mapped onto the checkpoint's noise curve: (cfg.scale * v) + cfg.offset (rvdd_match_raw; cfg:
        `match_cfg(scale, offset)` or the first item `match_coeffs` returns).  -> `out`, or a new tensor; out = packed maps in place.
        Nothing is synchronised."""
        return self._match(self.lib.rvdd_match_raw, "match_raw", packed, 4, cfg, out)

    def unmatch_rgb(self, rgb: torch.Tensor, cfg, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Network outputs [n,3,H,W] mapped back to the sensor's domain: (v - cfg.offset) * (1 / cfg.scale) (rvdd_unmatch_rgb).
        -> `out`, or a new tensor; out = rgb maps in place.  Nothing is synchronised."""
        return self._match(self.lib.rvdd_unmatch_rgb, "unmatch_rgb", rgb, 3, cfg, out)

    def set_match(self, cfg=None):
        """The map as a stage of `video_push` (rvdd_set_match): the kept packed frames are mapped behind the ingest (and the
        correction of `set_dpc`), the outputs mapped back; flows are still matched on the sensor's own gray planes.
        cfg = `match_cfg(...)`, None = off (the default)."""
        self._set_cfg("rvdd_set_match", cfg)

    # -- denoised footage checked without ground truth ---------------------------------------
    def resid_stats(self, packed: torch.Tensor, rgb: torch.Tensor, bit_depth: int = 12, pattern: Optional[str] = None,
                    acc: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The residual statistics of noisy packed frames [n,4,hh,ww] against the outputs for them, rgb [n,3,2hh,2ww], added to `acc`
        (rvdd_resid_stats): a device int64 tensor [n,384], one struct rvdd_resid_acc per frame -- None = a new zeroed one -- which is
        returned.  pattern: one of BAYER_PATTERNS, None = the pattern set_option("bayer_pattern", ...) gave this runtime.
        `resid_acc_arrays(acc)` gives the sums, `resid_fit` judges one accumulator against a curve.  Nothing is synchronised."""
        pat = self._pattern(pattern, "resid_stats")
        packed, n, hh, ww = _frames(packed, 4, "resid_stats: packed is [n,4,hh,ww]", "packed", self.device)
        rgb = _dev_tensor(rgb, "rgb", self.device, shape=(n, 3, 2 * hh, 2 * ww),
                          form=f"resid_stats: rgb is a float32 tensor [{n},3,{2 * hh},{2 * ww}], the outputs of packed")
        acc = _out_or_new(acc, "resid_stats: acc", (n, RESID_ACC_BYTES // 8), self._tdev, torch.int64, zero=True, nbytes=n * RESID_ACC_BYTES,
                          form=f"resid_stats: acc is a contiguous int64 tensor of {n} x {RESID_ACC_BYTES // 8} words on cuda:{self.device}")
        self._check(self.lib.rvdd_resid_stats(self.h, _ptr(packed), _ptr(rgb), n, hh, ww, pat, int(bit_depth), _ptr(acc), self._stream()),
                    "rvdd_resid_stats")
        return acc

    def set_resid(self, on: bool = True):
        """The measurement as a stage of `video_push` (rvdd_set_resid): every output is measured against its centre frame -- as
        corrected and as mapped -- into the slot's accumulator, which `resid_read` fetches.  With `set_match` on the unit is 12-bit DN,
        the checkpoint curve's; otherwise the push's bit depth."""
        self._check(self.lib.rvdd_set_resid(self.h, 1 if on else 0), "rvdd_set_resid")

    def resid_read(self, slot: int):
        """Slot `slot`'s accumulator as `resid_acc_arrays` gives one ([1,64] arrays), zeroed on the device (rvdd_resid_read; synchronises)."""
        return resid_acc_arrays(self._slot_read("rvdd_resid_read", _lib.RvddResidAcc, slot))

    # -- row noise ------------------------------------------------------------------------------
    def rows_estimate(self, packed: torch.Tensor, cfg, bit_depth: int = 12, acc: Optional[torch.Tensor] = None):
        """One offset per frame, row parity and plane row of packed frames [n,4,hh,ww] (rvdd_rows_estimate; cfg: `rows_cfg(...)`, the
        curve in DN of `bit_depth`).  -> (offsets float32 [n,2,hh], state uint8 [n,2,hh]: 0 skipped, 1 applied, 2 applied and clamped,
        acc: a device int64 tensor [n,3], one struct rvdd_rows_acc per frame -- None = a new zeroed one -- to which the rows are
        added; `rows_acc_arrays(acc)` gives the counts).  Nothing is synchronised."""
        packed, n, hh, ww = _frames(packed, 4, "rows_estimate: packed is [n,4,hh,ww]", "packed", self.device)
        offsets = torch.empty((n, 2, hh), dtype=torch.float32, device=self._tdev)
        state = torch.empty((n, 2, hh), dtype=torch.uint8, device=self._tdev)
        acc = _out_or_new(acc, "rows_estimate: acc", (n, ROWS_ACC_BYTES // 8), self._tdev, torch.int64, zero=True, nbytes=n * ROWS_ACC_BYTES,
                          form=f"rows_estimate: acc is a contiguous int64 tensor of {n} x {ROWS_ACC_BYTES // 8} words on cuda:{self.device}")
        self._check(self.lib.rvdd_rows_estimate(self.h, _ptr(packed), n, hh, ww, int(bit_depth), C.byref(cfg), _ptr(offsets), _ptr(state),
                                                _ptr(acc), self._stream()), "rvdd_rows_estimate")
        return offsets, state, acc

    def rows_apply(self, packed: torch.Tensor, offsets: torch.Tensor, bit_depth: int = 12, gray: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`offsets` [n,2,hh] taken out of packed frames [n,4,hh,ww] IN PLACE (rvdd_rows_apply), gray [n,hh,ww] re-formed in the rows
        with a non-zero offset.  -> packed.  Both must be contiguous: they are written where they lie.  Nothing is synchronised."""
        packed, n, hh, ww, offsets = self._in_place("rows_apply", packed, gray, lambda n, hh, ww: _dev_tensor(
            offsets, "offsets", self.device, shape=(n, 2, hh), form=f"rows_apply: offsets is a float32 tensor [{n},2,{hh}], as rows_estimate gives it"))
        self._check(self.lib.rvdd_rows_apply(self.h, _ptr(packed), _ptr(gray), _ptr(offsets), n, hh, ww, int(bit_depth), self._stream()),
                    "rvdd_rows_apply")
        return packed

    def set_rows(self, cfg=None):
        """The row-noise correction as a stage of `video_push`, behind `set_dpc` and in front of `set_match` (rvdd_set_rows): cfg =
        `rows_cfg(...)`, the sensor's own curve in DN of the pushes' bit depth; None = off (the default).  Synchronises the device."""
        self._set_cfg("rvdd_set_rows", cfg)

    def rows_read(self, slot: int):
        """Slot `slot`'s accumulator as `rows_acc_arrays` gives one ([1] arrays), zeroed on the device (rvdd_rows_read; synchronises)."""
        return rows_acc_arrays(self._slot_read("rvdd_rows_read", _lib.RvddRowsAcc, slot))

    # -- column fixed-pattern noise -------------------------------------------------------------
    def cols_estimate(self, packed: torch.Tensor, cfg, bit_depth: int = 12):
        """One offset per frame, column parity and plane column of packed frames [n,4,hh,ww] (rvdd_cols_estimate; cfg:
        `cols_cfg(...)`, the curve in DN of `bit_depth`).  -> (offsets float32 [n,2,ww], state uint8 [n,2,ww]: 0 skipped, 1 applied);
        `cols_fit` pools them over the frames.  Nothing is synchronised."""
        packed, n, hh, ww = _frames(packed, 4, "cols_estimate: packed is [n,4,hh,ww]", "packed", self.device)
        offsets = torch.empty((n, 2, ww), dtype=torch.float32, device=self._tdev)
        state = torch.empty((n, 2, ww), dtype=torch.uint8, device=self._tdev)
        self._check(self.lib.rvdd_cols_estimate(self.h, _ptr(packed), n, hh, ww, int(bit_depth), C.byref(cfg), _ptr(offsets), _ptr(state),
                                                self._stream()), "rvdd_cols_estimate")
        return offsets, state

    def cols_apply(self, packed: torch.Tensor, cmap: torch.Tensor, bit_depth: int = 12, gray: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The map `cmap` (a device float32 tensor [2,ww], DN of `bit_depth`) taken out of packed frames [n,4,hh,ww] IN PLACE
        (rvdd_cols_apply), gray [n,hh,ww] re-formed in the columns with a non-zero offset.  -> packed.  Both must be contiguous: they
        are written where they lie.  Nothing is synchronised."""
        packed, n, hh, ww, cmap = self._in_place("cols_apply", packed, gray, lambda n, hh, ww: _dev_tensor(
            cmap, "cmap", self.device, shape=(2, ww), form=f"cols_apply: cmap is a float32 tensor [2,{ww}], as cols_fit gives it"))
        self._check(self.lib.rvdd_cols_apply(self.h, _ptr(packed), _ptr(gray), _ptr(cmap), n, hh, ww, int(bit_depth), self._stream()),
                    "rvdd_cols_apply")
        return packed

    def set_cols(self, cmap=None):
        """The column map as a stage of `video_push`, behind `set_dpc` and in front of `set_rows` and `set_match` (rvdd_set_cols):
        cmap float32 [2,ww] on the host (a NumPy array or CPU tensor, DN of the pushes' bit depth), None = off (the default).
        Synchronises the device."""
        if cmap is None:
            self._check(self.lib.rvdd_set_cols(self.h, None, 0), "rvdd_set_cols")
            return
        m = _host_map(cmap, "float32", "set_cols: cmap is float32 [2,ww]", (2, None))
        self._check(self.lib.rvdd_set_cols(self.h, m.ctypes.data, m.shape[1]), "rvdd_set_cols")

    # -- green imbalance ------------------------------------------------------------------------
    def green_estimate(self, packed: torch.Tensor, cfg, bit_depth: int = 12, pattern: Optional[str] = None):
        """The imbalance of the two green planes per frame and block of 32 x 32 cells of packed frames [n,4,hh,ww]
        (rvdd_green_estimate; cfg: `green_cfg(...)`, the curve in DN of `bit_depth`; pattern: one of BAYER_PATTERNS, None = the
        pattern set_option("bayer_pattern", ...) gave this runtime).  -> (e float32 [n,gh,gw] in DN, level float32 [n,gh,gw] in
        DN, state uint8 [n,gh,gw]: 0 skipped, 1 applied); `green_fit` pools them over the frames.  Nothing is synchronised."""
        packed, n, hh, ww = _frames(packed, 4, "green_estimate: packed is [n,4,hh,ww]", "packed", self.device)
        gh, gw = green_grid(hh, ww)
        e = torch.empty((n, gh, gw), dtype=torch.float32, device=self._tdev)
        level = torch.empty((n, gh, gw), dtype=torch.float32, device=self._tdev)
        state = torch.empty((n, gh, gw), dtype=torch.uint8, device=self._tdev)
        self._check(self.lib.rvdd_green_estimate(self.h, _ptr(packed), n, hh, ww, int(bit_depth), self._pattern(pattern, "green_estimate"),
                                                 C.byref(cfg), _ptr(e), _ptr(level), _ptr(state), self._stream()), "rvdd_green_estimate")
        return e, level, state

    def green_apply(self, packed: torch.Tensor, gmap: torch.Tensor, black: float, bit_depth: int = 12, gray: Optional[torch.Tensor] = None,
                    pattern: Optional[str] = None) -> torch.Tensor:
        """The gains `gmap` (a device float32 tensor [gh,gw]: the frames' own grid, or [1,1] for a flat gain) taken out of the two
        green planes of packed frames [n,4,hh,ww] IN PLACE (rvdd_green_apply), gray [n,hh,ww] re-formed in the cells with a
        non-zero gain.  -> packed.  Both must be contiguous: they are written where they lie.  Nothing is synchronised."""
        packed, n, hh, ww, gmap = self._in_place("green_apply", packed, gray, lambda n, hh, ww: _dev_tensor(
            gmap, "gmap", self.device, shape=(None, None), form="green_apply: gmap is a float32 tensor [gh,gw], as green_fit gives it"))
        self._check(self.lib.rvdd_green_apply(self.h, _ptr(packed), _ptr(gray), _ptr(gmap), gmap.shape[0], gmap.shape[1], float(black), n, hh, ww,
                                              int(bit_depth), self._pattern(pattern, "green_apply"), self._stream()), "rvdd_green_apply")
        return packed

    def set_green(self, gmap=None, black: float = 0.0):
        """The map of green gains as a stage of `video_push`, behind `set_dpc`, `set_cols` and `set_rows` and in front of `set_match`
        (rvdd_set_green): gmap float32 [gh,gw] on the host (a NumPy array or CPU tensor; the frames' grid, or [1,1]), black in DN of
        the pushes' bit depth; None = off (the default).  The planes are those of option "bayer_pattern".  Synchronises the device."""
        if gmap is None:
            self._check(self.lib.rvdd_set_green(self.h, None, 0, 0, 0.0), "rvdd_set_green")
            return
        m = _host_map(gmap, "float32", "set_green: gmap is float32 [gh,gw]", (None, None))
        self._check(self.lib.rvdd_set_green(self.h, m.ctypes.data, m.shape[0], m.shape[1], float(black)), "rvdd_set_green")

    def set_dpc(self, cfg=None):
        """The correction as a stage of `video_push`, between the ingest and the kept frames (rvdd_set_dpc): cfg = `dpc_cfg(...)`,
        None = off (the default)."""
        self._set_cfg("rvdd_set_dpc", cfg)

    def dpc_counts(self) -> List[Tuple[int, int]]:
        """[(hot, dead)] * B: the samples the stage corrected per slot since it was last switched on (rvdd_dpc_counts; synchronises)."""
        out = (C.c_uint64 * (2 * self.B))()
        self._check(self.lib.rvdd_dpc_counts(self.h, out, self._stream()), "rvdd_dpc_counts")
        return [(int(out[2 * b]), int(out[2 * b + 1])) for b in range(self.B)]

    def video_push(self, frames: torch.Tensor, ctl=None, bit_depth: int = 12, layout: str = "mosaic", out=None,
                   container: Optional[str] = None):
        """Every slot's next sensor frame in, at most one denoised frame per slot out (rvdd_video_push).
        frames: [B,2hh,2ww] / [B,hh,ww,4] as `ingest_raw` takes them; ctl: None (every slot continues its video) or B
        values of _lib.PUSH_NEXT / PUSH_FIRST / PUSH_IDLE.  -> (out [B,3,H,W], valid: B bools); out[b] is the denoised
        centre frame of slot b where valid[b], unspecified elsewhere.  Nothing is synchronised.
        container "mipi" / "msb" (option "stream_container", set here; None sets it back to 0): frames is a uint8 tensor of B tight
        frames of packed `bit_depth` = 10 / 12 / 14-bit samples as `ingest_bits` takes them, and the outputs are those of the
        same pushes with the unpacked uint16 frames.
        A video of N frames gives its frames 1 .. N-1-future.  With option "stream_all_frames" it gives every frame: frame 0 on
        the push that completes 1 + future frames, and with a future frame the last one on a PUSH_IDLE straight after it (a
        PUSH_FIRST there drops it); valid[b] is then also set on such a FIRST / IDLE push, and out[b] is the oldest frame of
        the slot's video not yet output."""
        B, H, W = self.B, self.H, self.W
        if container is not None and container not in BITS_ORDERS:
            raise ValueError(f"video_push: container {container!r} is not None or one of {', '.join(BITS_ORDERS)}")
        want = 0 if container is None else 1 + BITS_ORDERS[container]
        if container is None:
            t, dtype, lay, n, hh, ww = _raw_frames(frames, layout, "video_push", self.device)
        else:
            if layout != "mosaic":
                raise ValueError(f"video_push: packed frames ({container}) are a mosaic, got layout {layout!r}")
            dtype, lay, n, hh, ww = _lib.RAW_U16, _lib.RAW_MOSAIC, B, H // 2, W // 2
            t = self._bits_frames(frames, container, int(bit_depth), n, hh, ww, "video_push")
        if getattr(self, "stream_container", 0) != want:
            self.set_option("stream_container", want)
        if (n, 2 * hh, 2 * ww) != (B, H, W):
            raise RuntimeError(f"video_push: frames of {n} x {2 * hh} x {2 * ww} sites for a runtime of {B} slots of {H} x {W}")
        c = None
        if ctl is not None:
            items = [int(v) for v in (ctl.tolist() if hasattr(ctl, "tolist") else ctl)]
            if len(items) != B:
                raise ValueError(f"video_push: ctl needs {B} entries, got {len(items)}")
            if any(not 0 <= v <= 255 for v in items):
                raise ValueError("video_push: ctl entries are PUSH_NEXT (0), PUSH_FIRST (1) or PUSH_IDLE (2)")
            c = (C.c_uint8 * B)(*items)
        out = _out_or_new(out, "out", (B, 3, H, W), self._tdev)
        valid = (C.c_uint8 * B)()
        self._check(self.lib.rvdd_video_push(self.h, _ptr(t), dtype, lay, int(bit_depth), c, _ptr(out), valid, self._stream()),
                    "rvdd_video_push")
        return out, [bool(v) for v in valid]

    def get_state(self, want_feat: bool = True):
        B, H, W = self.B, self.H, self.W
        den = torch.empty(B, 3, H, W, dtype=torch.float32, device=self._tdev)
        feat = torch.empty(B, 48, H, W, dtype=torch.float32, device=self._tdev) if (self.feat and want_feat) else None
        self._check(self.lib.rvdd_get_state(self.h, _ptr(den), _ptr(feat), self._stream()), "rvdd_get_state")
        return den, feat

    def set_state(self, lastden=None, lastfeat=None):
        B, H, W = self.B, self.H, self.W
        if lastden is not None:
            lastden = _dev_tensor(lastden, "lastden", self.device, shape=(B, 3, H, W))
        if lastfeat is not None:
            lastfeat = _dev_tensor(lastfeat, "lastfeat", self.device, shape=(B, 48, H, W))
        self._check(self.lib.rvdd_set_state(self.h, _ptr(lastden), _ptr(lastfeat), self._stream()),
                    "rvdd_set_state")

    def psnr_l1(self, den: torch.Tensor, gt: torch.Tensor) -> Tuple[float, float]:
        """-> (L1*100, PSNR) as compute_losses (models/recurrent_model.py:512-525)."""
        den = _dev_tensor(den, "den", self.device)
        gt = _dev_tensor(gt, "gt", self.device, shape=den.shape)
        out = (C.c_float * 2)()
        self._check(self.lib.rvdd_psnr_l1(self.h, _ptr(den), _ptr(gt), den.numel(), out, self._stream()),
                    "rvdd_psnr_l1")
        return float(out[0]), float(out[1])

    def psnr_l1_batch(self, den: torch.Tensor, gt: torch.Tensor) -> List[Tuple[float, float]]:
        """psnr_l1 of every sequence of a batch ([n, ...] each), one synchronisation: [(L1*100, PSNR)] * n, each pair
        bit for bit what psnr_l1 gives for that sequence alone."""
        den = _dev_tensor(den, "den", self.device)
        gt = _dev_tensor(gt, "gt", self.device, shape=den.shape)
        n = den.shape[0] if den.dim() else 1
        if n == 0:
            return []
        out = (C.c_float * (2 * n))()
        self._check(self.lib.rvdd_psnr_l1_batch(self.h, _ptr(den), _ptr(gt), n, den.numel() // n, out, self._stream()),
                    "rvdd_psnr_l1_batch")
        return [(float(out[2 * i]), float(out[2 * i + 1])) for i in range(n)]

    # -- single ops -----------------------------------------------------------
    def unet_forward(self, x, feat_in=None):
        B, H, W = self.B, self.H, self.W
        x = _dev_tensor(x, "x", self.device, shape=(B, 3 * (2 + self.future), H, W))
        if feat_in is not None:
            feat_in = _dev_tensor(feat_in, "feat_in", self.device, shape=(B, 48, H, W))
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=self._tdev)
        fo = torch.empty(B, 48, H, W, dtype=torch.float32, device=self._tdev) if self.feat else None
        self._check(self.lib.rvdd_unet_forward(self.h, _ptr(x), _ptr(feat_in), _ptr(out), _ptr(fo),
                                               self._stream()), "rvdd_unet_forward")
        return out, fo

    def demosaic(self, raw: torch.Tensor, pattern: str = "gbrg") -> torch.Tensor:
        """HamiltonAdam(pattern)(raw): [n,4k,h,w] packed raw -> [n,3k,2h,2w] (pattern: one of BAYER_PATTERNS)."""
        pat = _pattern_index(pattern, "demosaic")
        n, c, h, w = raw.shape
        raw = _dev_tensor(raw, "raw", self.device)
        assert c % 4 == 0
        k = n * (c // 4)
        out = torch.empty(n, 3 * (c // 4), 2 * h, 2 * w, dtype=torch.float32, device=raw.device)
        self._check(self.lib.rvdd_demosaic_ha_bayer(self.h, _ptr(raw), k, h, w, pat, _ptr(out),
                                                    self._stream()), "rvdd_demosaic_ha_bayer")
        return out

    def warp(self, x: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
        n, c, H, W = x.shape
        x = _dev_tensor(x, "x", self.device)
        flow = _dev_tensor(flow, "flow", self.device, shape=(n, 2, H, W))
        y = torch.empty_like(x)
        self._check(self.lib.rvdd_warp_bicubic(self.h, _ptr(x), _ptr(flow), n, c, H, W, _ptr(y),
                                               self._stream()), "rvdd_warp_bicubic")
        return y

    def upsample_factor_2(self, t: torch.Tensor, multiply_by: float = 1.0) -> torch.Tensor:
        *rem, c, h, w = t.shape
        t = _dev_tensor(t, "t", self.device)
        n = 1
        for r in rem:
            n *= r
        out = torch.empty(*rem, c, 2 * h, 2 * w, dtype=torch.float32, device=t.device)
        self._check(self.lib.rvdd_upsample_factor_2(self.h, _ptr(t), n, c, h, w, float(multiply_by),
                                                    _ptr(out), self._stream()), "rvdd_upsample_factor_2")
        return out

    def tvl1flow(self, I0: torch.Tensor, I1: torch.Tensor, want_iterations: bool = False):
        """[ny,nx] x2 -> flow [2,ny,nx] (libBridge tvl1flow, libBridge.cpp:44)."""
        ny, nx = I0.shape
        I0 = _dev_tensor(I0, "I0", self.device, shape=(ny, nx))
        I1 = _dev_tensor(I1, "I1", self.device, shape=(ny, nx))
        u = torch.empty(2, ny, nx, dtype=torch.float32, device=I0.device)
        it = C.c_int32(0)
        self._check(self.lib.rvdd_tvl1flow(self.h, _ptr(I0), _ptr(I1), _ptr(u), nx, ny,
                                           C.byref(it) if want_iterations else None, self._stream()), "rvdd_tvl1flow")
        return (u, int(it.value)) if want_iterations else u

    def tvl1flow_batch(self, I0: torch.Tensor, I1: torch.Tensor, want_iterations: bool = False):
        """[n,ny,nx] x2 -> flows [n,2,ny,nx]: n independent pairs, two per cooperative launch."""
        n, ny, nx = I0.shape
        I0 = _dev_tensor(I0, "I0", self.device, shape=(n, ny, nx))
        I1 = _dev_tensor(I1, "I1", self.device, shape=(n, ny, nx))
        u = torch.empty(n, 2, ny, nx, dtype=torch.float32, device=I0.device)
        it = (C.c_int32 * max(n, 1))()
        self._check(self.lib.rvdd_tvl1flow_batch(self.h, _ptr(I0), _ptr(I1), _ptr(u), n, nx, ny,
                                                 it if want_iterations else None, self._stream()), "rvdd_tvl1flow_batch")
        return (u, list(it)[:n]) if want_iterations else u

    def ppipe(self, img: torch.Tensor, rgb_gain: float, red_gain: float, blue_gain: float, iso: int,
              bit_depth: int, layout: str = "nchw", want_float: bool = False):
        """dataset/fwd_ppipe.py:48-77,131-141.  img [n,3,H,W] ("nchw") or [n,H,W,3] ("hwc"), any strides.
        -> uint8 [n,H,W,3] (and the float32 sRGB x 255 image before rounding)."""
        _dev_tensor(img, "ppipe: img", self.device, shape=(None,) * 4, contiguous=None,
                    form="ppipe: img must be a 4-D float32 GPU tensor (rvdd has no CPU path)")
        if layout == "nchw":
            n, c, H, W = img.shape
            sn, sc, sy, sx = img.stride()
        elif layout == "hwc":
            n, H, W, c = img.shape
            sn, sy, sx, sc = img.stride()
        else:
            raise ValueError("layout must be 'nchw' or 'hwc'")
        if c != 3:
            raise AssertionError("The data should have 3 channels.")              # fwd_ppipe.py:129
        u8 = torch.empty(n, H, W, 3, dtype=torch.uint8, device=img.device)
        f32 = torch.empty(n, H, W, 3, dtype=torch.float32, device=img.device) if want_float else None
        self._check(self.lib.rvdd_ppipe(self.h, _ptr(img), n, H, W, sn, sc, sy, sx, int(bit_depth), float(rgb_gain),
                                        float(red_gain), float(blue_gain), int(iso), _ptr(u8), _ptr(f32),
                                        self._stream()), "rvdd_ppipe")
        return (u8, f32) if want_float else u8

    def ycbcr(self, disp: torch.Tensor, depth: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n,H,W,3] float32 display values in [0,255] -- the float image of `ppipe(..., want_float=True)` -- -> the frames of a
        Y'CbCr 4:2:0 video (rvdd_ycbcr: BT.709, limited range, chroma the average of each 2 x 2 quad): [n, H*W*3//2] samples, uint8
        for depth 8, torch.uint16 for depth 10 (torch.int16 where this torch has no uint16: the same 16 bits, as `egress` gives
        them); per image the Y plane [H,W], then Cb, then Cr [H/2,W/2] -- the body of one Y4M frame (`y4m.Y4MWriter`).  H and W
        even.  out: a tensor of that shape and dtype to write into."""
        if depth not in (8, 10):
            raise ValueError(f"ycbcr: depth must be 8 or 10, got {depth!r}")
        disp = _dev_tensor(disp, "ycbcr: disp", self.device, shape=(None, None, None, 3), form="ycbcr: disp is float32 [n,H,W,3]")
        n, H, W, _ = disp.shape
        if H < 2 or W < 2 or H % 2 or W % 2:
            raise RuntimeError(f"ycbcr: H and W must be even and >= 2 (chroma is one sample per 2 x 2 quad), got {H} x {W}")
        dtype = torch.uint8 if depth == 8 else getattr(torch, "uint16", torch.int16)
        shape = (n, H * W * 3 // 2)
        out = _out_or_new(out, "ycbcr: out", shape, self._tdev, (dtype, torch.int16) if depth == 10 else dtype,
                          form=f"ycbcr: out must be a contiguous {dtype} tensor of shape {shape}")
        self._check(self.lib.rvdd_ycbcr(self.h, _ptr(disp), n, H, W, int(depth), _ptr(out), self._stream()), "rvdd_ycbcr")
        return out

    # -- raw datasets from sRGB video -------------------------------------------
    UNPROCESS_OUTPUTS = ("lin_f32", "lin_u16", "gt_raw", "noisy")

    def unprocess(self, srgb: torch.Tensor, rgb_gain: float, red_gain: float, blue_gain: float, iso: int,
                  pattern: str = "gbrg", dither: Optional[torch.Tensor] = None, normal: Optional[torch.Tensor] = None,
                  seed: int = 0, frame0: int = 0, want=UNPROCESS_OUTPUTS) -> Dict[str, torch.Tensor]:
        """dataset/generate_raw_from_RGB.py:45-127, :168-189 (rvdd_unprocess).  srgb: uint8 [n,H,W,3] GPU tensor, H and W even.
        -> the outputs named in `want`: lin_f32 [n,H,W,3] float32 (what `ppipe(..., bit_depth=12, layout="hwc")` takes),
        lin_u16 [n,H,W,3] uint16, gt_raw and noisy [n,H/2,W/2,4] float32 in `pattern` (one of BAYER_PATTERNS), the packed HWC
        layout `ingest_raw` / `video_push` read.  dither [n,H,W,3] / normal [n,H/2,W/2,4]: the random planes; where None the
        kernel draws them from (seed, frame0 + i) for image i (`unprocess_draws` gives the same planes)."""
        pat = _pattern_index(pattern, "unprocess")
        unknown = [w for w in want if w not in self.UNPROCESS_OUTPUTS]
        if unknown:
            raise ValueError(f"unprocess: unknown outputs {unknown}; known: {', '.join(self.UNPROCESS_OUTPUTS)}")
        srgb = _dev_tensor(srgb, "unprocess: srgb", self.device, dtype=torch.uint8, shape=(None, None, None, 3),
                           form="unprocess: srgb is uint8 [n,H,W,3]")
        n, H, W, _ = srgb.shape
        if H % 2 or W % 2:
            raise RuntimeError(f"unprocess: H and W must be even (crop the frame as the reference does), got {H} x {W}")
        if dither is not None:
            dither = _dev_tensor(dither, "dither", self.device, shape=(n, H, W, 3))
        if normal is not None:
            normal = _dev_tensor(normal, "normal", self.device, shape=(n, H // 2, W // 2, 4))
        out = {}
        for name, shape, dt in (("lin_f32", (n, H, W, 3), torch.float32), ("lin_u16", (n, H, W, 3), torch.uint16),
                                ("gt_raw", (n, H // 2, W // 2, 4), torch.float32), ("noisy", (n, H // 2, W // 2, 4), torch.float32)):
            if name in want:
                out[name] = torch.empty(shape, dtype=dt, device=self._tdev)
        self._check(self.lib.rvdd_unprocess(self.h, _ptr(srgb), n, H, W, float(rgb_gain), float(red_gain), float(blue_gain), int(iso),
                                            pat, _ptr(dither), _ptr(normal), int(seed) & (2 ** 64 - 1),
                                            int(frame0), _ptr(out.get("lin_f32")), _ptr(out.get("lin_u16")), _ptr(out.get("gt_raw")),
                                            _ptr(out.get("noisy")), self._stream()), "rvdd_unprocess")
        return out

    def unprocess_draws(self, seed: int, frame0: int, n: int, H: int, W: int, want_dither: bool = True, want_normal: bool = True):
        """-> (dither [n,H,W,3], normal [n,H/2,W/2,4]), None for one not wanted: the planes `unprocess` draws for
        (seed, frame0 .. frame0 + n - 1) (rvdd_unprocess_draws)."""
        n, H, W = int(n), int(H), int(W)
        if n < 0 or H < 2 or W < 2 or H % 2 or W % 2:
            raise RuntimeError(f"unprocess_draws: n >= 0 and even H, W >= 2, got n = {n}, {H} x {W}")
        dither = torch.empty(n, H, W, 3, dtype=torch.float32, device=self._tdev) if want_dither else None
        normal = torch.empty(n, H // 2, W // 2, 4, dtype=torch.float32, device=self._tdev) if want_normal else None
        self._check(self.lib.rvdd_unprocess_draws(self.h, int(seed) & (2 ** 64 - 1), int(frame0), n, H, W, _ptr(dither), _ptr(normal),
                                                  self._stream()), "rvdd_unprocess_draws")
        return dither, normal

    def srgb_metrics(self, a: torch.Tensor, b: torch.Tensor):
        """dataset/fwd_ppipe.py:79-86 on uint8 [n,H,W,3] images -> (psnr[n], ssim[n]) Python floats."""
        if a.shape != b.shape:
            raise RuntimeError(f"srgb_metrics: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        a, b = (_dev_tensor(t, f"srgb_metrics: {name}", self.device, dtype=torch.uint8, shape=(None, None, None, 3),
                            form="srgb_metrics: a, b must be uint8 GPU tensors [n,H,W,3]") for t, name in ((a, "a"), (b, "b")))
        n, H, W, _ = a.shape
        ps, ss = (C.c_double * n)(), (C.c_double * n)()
        self._check(self.lib.rvdd_srgb_metrics(self.h, _ptr(a), _ptr(b), n, H, W, ps, ss, self._stream()),
                    "rvdd_srgb_metrics")
        return list(ps), list(ss)

    # -- measurement ------------------------------------------------------------
    def profile_enable(self, on: bool):
        self._check(self.lib.rvdd_profile_enable(self.h, 1 if on else 0), "rvdd_profile_enable")

    def profile_select(self, kernel_class=None, stride: int = 1):
        self._check(self.lib.rvdd_profile_select(self.h, None if kernel_class is None else kernel_class.encode(),
                                                 stride), "rvdd_profile_select")

    def profile_read(self):
        out = []
        for i in range(self.lib.rvdd_profile_count(self.h)):
            name = C.create_string_buffer(128)
            n = C.c_int64()
            ms, fl, by = C.c_double(), C.c_double(), C.c_double()
            self._check(self.lib.rvdd_profile_read(self.h, i, name, 128, C.byref(n), C.byref(ms),
                                                   C.byref(fl), C.byref(by)), "rvdd_profile_read")
            out.append(dict(name=name.value.decode(), launches=n.value, ms=ms.value, flops=fl.value,
                            bytes=by.value))
        return out

    def debug_conv_bench(self, variant: int, level: int = 0, iters: int = 20) -> float:
        ms = C.c_float()
        self._check(self.lib.rvdd_debug_conv_bench(self.h, variant, level, iters, C.byref(ms), self._stream()),
                    "rvdd_debug_conv_bench")
        return float(ms.value)

    def timer_start(self):
        self._check(self.lib.rvdd_timer_start(self.h, self._stream()), "rvdd_timer_start")

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        self._check(self.lib.rvdd_timer_stop_ms(self.h, self._stream(), C.byref(ms)), "rvdd_timer_stop_ms")
        return float(ms.value)
