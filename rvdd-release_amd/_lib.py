"""ctypes binding of ``librvdd_hip.so`` (declared in ``include/rvdd.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C
rvdd-release_amd/csrc``).  Loading fails loudly when it is missing: there is
no CPU fallback behind this package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librvdd_hip.so")

RVDD_OK = 0
ARCH_CONVUNET, ARCH_CONVUNET_FEAT, ARCH_CONVNEXT, ARCH_CONVNEXT_FEAT = 0, 1, 2, 3
# enum rvdd_raw_dtype / rvdd_raw_layout (rvdd_ingest_raw, rvdd_video_push) and enum rvdd_push (rvdd_video_push's ctl)
RAW_U16, RAW_F32 = 0, 1
RAW_MOSAIC, RAW_PACKED_HWC = 0, 1
PUSH_NEXT, PUSH_FIRST, PUSH_IDLE = 0, 1, 2
# enum rvdd_out_layout (rvdd_egress)
OUT_RGB_HWC, OUT_MOSAIC, OUT_PACKED_HWC = 0, 1, 2
# enum rvdd_bits_order (rvdd_ingest_bits, rvdd_egress_bits; option "stream_container" is the value plus one)
BITS_MIPI, BITS_MSB = 0, 1
PPIPE_FROM_NET = -1      # RVDD_PPIPE_FROM_NET: rvdd_ppipe's bit_depth for a network output in [-1,1]


class RvddCfg(C.Structure):
    _fields_ = [("arch", C.c_int32), ("future", C.c_int32), ("batch", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("device", C.c_int32)]


class RvddDpcCfg(C.Structure):
    """struct rvdd_dpc_cfg (rvdd_dpc, rvdd_set_dpc)"""
    _fields_ = [("k_hot", C.c_float), ("k_dead", C.c_float), ("noise_a", C.c_float), ("noise_b", C.c_float),
                ("var_floor", C.c_float)]


class RvddDpcDetectCfg(C.Structure):
    """struct rvdd_dpc_detect_cfg (rvdd_dpc_detect)"""
    _fields_ = [("rule", RvddDpcCfg), ("tolerate", C.c_int32), ("reserved", C.c_int32)]


class RvddMatchCfg(C.Structure):
    """struct rvdd_match_cfg (rvdd_match_coeffs, rvdd_match_raw, rvdd_unmatch_rgb, rvdd_set_match)"""
    _fields_ = [("scale", C.c_float), ("offset", C.c_float)]


class RvddNoiseAcc(C.Structure):
    """struct rvdd_noise_acc (rvdd_noise_hist, rvdd_noise_fit): 131616 bytes"""
    _fields_ = [("hist", (C.c_uint32 * 512) * 64), ("msum", C.c_uint64 * 64), ("counters", C.c_uint64 * 4)]


class RvddNoiseCurve(C.Structure):
    """struct rvdd_noise_curve (rvdd_noise_fit)"""
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("m_min", C.c_double), ("m_max", C.c_double), ("rms", C.c_double),
                ("blocks", C.c_uint64), ("bins", C.c_int32), ("reserved", C.c_int32)]


class RvddFrameSig(C.Structure):
    """struct rvdd_frame_sig (rvdd_frame_sigs, rvdd_cut_score): 6144 bytes"""
    _fields_ = [("hist", (C.c_uint32 * 64) * 16), ("sum", (C.c_uint64 * 16) * 16)]


class RvddResidAcc(C.Structure):
    """struct rvdd_resid_acc (rvdd_resid_stats, rvdd_resid_read, rvdd_resid_fit): 3072 bytes"""
    _fields_ = [("n", C.c_uint64 * 64), ("msum", C.c_uint64 * 64), ("s1", C.c_int64 * 64), ("s2", C.c_uint64 * 64),
                ("n11", C.c_uint64 * 64), ("s11", C.c_int64 * 64)]


class RvddResidReport(C.Structure):
    """struct rvdd_resid_report (rvdd_resid_fit)"""
    _fields_ = [("ratio", C.c_double), ("ratio_lo", C.c_double), ("ratio_hi", C.c_double), ("bias", C.c_double), ("rho", C.c_double),
                ("a_fit", C.c_double), ("b_fit", C.c_double), ("samples", C.c_uint64), ("bins", C.c_int32), ("reserved", C.c_int32)]


class RvddRowsCfg(C.Structure):
    """struct rvdd_rows_cfg (rvdd_rows_estimate, rvdd_set_rows)"""
    _fields_ = [("k_gate", C.c_float), ("noise_a", C.c_float), ("noise_b", C.c_float), ("var_floor", C.c_float), ("max_dn", C.c_float)]


class RvddRowsAcc(C.Structure):
    """struct rvdd_rows_acc (rvdd_rows_estimate, rvdd_rows_read): 24 bytes"""
    _fields_ = [("applied", C.c_uint32), ("skipped", C.c_uint32), ("clamped", C.c_uint32), ("reserved", C.c_uint32), ("sum_q2", C.c_int64)]


class RvddColsCfg(C.Structure):
    """struct rvdd_cols_cfg (rvdd_cols_estimate)"""
    _fields_ = [("k_gate", C.c_float), ("noise_a", C.c_float), ("noise_b", C.c_float), ("var_floor", C.c_float)]


class RvddColsFitCfg(C.Structure):
    """struct rvdd_cols_fit_cfg (rvdd_cols_fit)"""
    _fields_ = [("min_frames", C.c_int32), ("k_sig", C.c_float), ("max_dn", C.c_float)]


class RvddColsStats(C.Structure):
    """struct rvdd_cols_stats (rvdd_cols_fit): 32 bytes"""
    _fields_ = [("counts", C.c_uint32 * 4), ("sum_q2", C.c_int64), ("floor_dn", C.c_double)]


class RvddGreenCfg(C.Structure):
    """struct rvdd_green_cfg (rvdd_green_estimate)"""
    _fields_ = [("k_gate", C.c_float), ("noise_a", C.c_float), ("noise_b", C.c_float), ("var_floor", C.c_float), ("black", C.c_float)]


class RvddGreenFitCfg(C.Structure):
    """struct rvdd_green_fit_cfg (rvdd_green_fit)"""
    _fields_ = [("min_frames", C.c_int32), ("k_sig", C.c_float), ("max_gain", C.c_float), ("min_signal", C.c_float)]


class RvddGreenStats(C.Structure):
    """struct rvdd_green_stats (rvdd_green_fit): 48 bytes"""
    _fields_ = [("counts", C.c_uint32 * 4), ("sum_q2", C.c_int64), ("floor", C.c_double), ("flat_gain", C.c_float), ("flat_se", C.c_float),
                ("flat_state", C.c_int32), ("reserved", C.c_int32)]


# symbol -> (restype, argtypes); exactly the functions include/rvdd.h declares
_P = C.c_void_p
_PROTOS = {
    "rvdd_create": (C.c_int, [C.POINTER(RvddCfg), C.POINTER(_P)]),
    "rvdd_destroy": (None, [_P]),
    "rvdd_last_error": (C.c_char_p, [_P]),
    "rvdd_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    "rvdd_finalize_weights": (C.c_int, [_P]),
    "rvdd_reset": (C.c_int, [_P]),
    "rvdd_reset_slots": (C.c_int, [_P, _P]),
    "rvdd_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "rvdd_step_strided": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    "rvdd_step_live": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    "rvdd_move_slots": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, _P]),
    "rvdd_get_state": (C.c_int, [_P, _P, _P, _P]),
    "rvdd_set_state": (C.c_int, [_P, _P, _P, _P]),
    "rvdd_psnr_l1": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_float), _P]),
    "rvdd_psnr_l1_batch": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, C.POINTER(C.c_float), _P]),
    "rvdd_unet_forward": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "rvdd_demosaic_ha": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_demosaic_ha_bayer": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_warp_bicubic": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_upsample_factor_2": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                         _P, _P]),
    "rvdd_tvl1flow": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P]),
    "rvdd_tiff_lzw_decode": (C.c_int64, [_P, C.c_int64, _P, C.c_int64]),
    "rvdd_set_option": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "rvdd_tvl1flow_batch": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P]),
    "rvdd_ingest_raw": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "rvdd_gray_of_rgb": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_egress": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_ingest_bits": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "rvdd_egress_bits": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_dpc": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddDpcCfg), _P, _P]),
    "rvdd_set_dpc": (C.c_int, [_P, C.POINTER(RvddDpcCfg)]),
    "rvdd_dpc_counts": (C.c_int, [_P, C.POINTER(C.c_uint64), _P]),
    "rvdd_dpc_detect": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddDpcDetectCfg), _P, _P]),
    "rvdd_dpc_map_stats": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "rvdd_set_dpc_map": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "rvdd_dpc_map_apply": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "rvdd_noise_hist": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_noise_fit": (C.c_int, [C.POINTER(RvddNoiseAcc), C.c_int32, C.POINTER(RvddNoiseCurve)]),
    "rvdd_frame_sigs": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_cut_score": (C.c_int, [C.POINTER(RvddFrameSig), C.POINTER(RvddFrameSig), C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "rvdd_match_coeffs": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.POINTER(RvddMatchCfg),
                                    C.POINTER(C.c_double)]),
    "rvdd_match_raw": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddMatchCfg), _P]),
    "rvdd_unmatch_rgb": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddMatchCfg), _P]),
    "rvdd_set_match": (C.c_int, [_P, C.POINTER(RvddMatchCfg)]),
    "rvdd_resid_stats": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_resid_fit": (C.c_int, [C.POINTER(RvddResidAcc), C.c_int32, C.c_double, C.c_double, C.POINTER(RvddResidReport)]),
    "rvdd_set_resid": (C.c_int, [_P, C.c_int32]),
    "rvdd_resid_read": (C.c_int, [_P, C.c_int32, C.POINTER(RvddResidAcc), _P]),
    "rvdd_rows_estimate": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddRowsCfg), _P, _P, _P, _P]),
    "rvdd_rows_apply": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "rvdd_set_rows": (C.c_int, [_P, C.POINTER(RvddRowsCfg)]),
    "rvdd_rows_read": (C.c_int, [_P, C.c_int32, C.POINTER(RvddRowsAcc), _P]),
    "rvdd_cols_estimate": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddColsCfg), _P, _P, _P]),
    "rvdd_cols_fit": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(RvddColsFitCfg), _P, _P, C.POINTER(RvddColsStats)]),
    "rvdd_cols_apply": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "rvdd_set_cols": (C.c_int, [_P, _P, C.c_int32]),
    "rvdd_green_estimate": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RvddGreenCfg), _P, _P, _P, _P]),
    "rvdd_green_fit": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(RvddGreenFitCfg), _P, _P,
                                 C.POINTER(RvddGreenStats)]),
    "rvdd_green_apply": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "rvdd_set_green": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float]),
    "rvdd_video_push": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "rvdd_unprocess": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                 _P, _P, C.c_uint64, C.c_int64, _P, _P, _P, _P, _P]),
    "rvdd_unprocess_draws": (C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "rvdd_ppipe": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                             C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, _P, _P, _P]),
    "rvdd_ycbcr": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "rvdd_srgb_metrics": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), _P]),
    "rvdd_profile_enable": (C.c_int, [_P, C.c_int32]),
    "rvdd_profile_select": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "rvdd_profile_count": (C.c_int, [_P]),
    "rvdd_profile_read": (C.c_int, [_P, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rvdd_timer_start": (C.c_int, [_P, _P]),
    "rvdd_timer_stop_ms": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "rvdd_debug_conv_bench": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), _P]),
    "rvdd_version": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP runtime library; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C rvdd-release_amd/csrc`). This package has no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 and an
    # unversioned libhsa-runtime64.so.  Import torch FIRST so that our NEEDED
    # libamdhip64.so.7 resolves to the copy torch already mapped; loaded the
    # other way round the process ends up with two HSA runtimes and
    # hipGetDeviceCount() reports no device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_PROTOS)
