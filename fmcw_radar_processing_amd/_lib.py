"""ctypes binding of libfmcw.so (include/fmcw.h).

The library is built in-tree (``fmcw_radar_processing_amd/libfmcw.so``, see
``csrc/Makefile`` / ``__graft_entry__.build``).  There is no CPU fallback:
if the shared object is missing, or no gfx950 device is present, the calls
raise ``FmcwError`` instead of silently computing elsewhere.
"""
from __future__ import annotations

import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMCW_LIB", os.path.join(_HERE, "libfmcw.so"))

FMCW_OK = 0
FMCW_E_ARG, FMCW_E_HIP, FMCW_E_OOM, FMCW_E_STATE, FMCW_E_DATA = -1, -2, -3, -4, -5
FMCW_C64, FMCW_C32H = 0, 1
FMCW_PIPE_AUTO, FMCW_PIPE_STREAMS, FMCW_PIPE_ONEPASS, FMCW_PIPE_XCD = 0, 1, 3, 4
ABI_VERSION = 4
STATUS_NAMES = {0: "OK", -1: "E_ARG", -2: "E_HIP", -3: "E_OOM", -4: "E_STATE", -5: "E_DATA"}
STAGES = ("range", "doppler", "detect", "compact", "stft_power", "stft_db", "range_only", "range_doppler", "onepass",
          "render", "cfar", "cluster", "track", "mti", "aoa", "beam", "oscfar", "ra")
MUSIC_STAGE = 18           # fmcw_timing_read's stage of fmcw_music_device ("music" in Engine.timing_read)
DOA_STAGE = 19             # fmcw_timing_read_ext's stage of fmcw_doa_device ("doa" in Engine.timing_read)
FMCW_CFAR_LOCAL_MAX = 1
FMCW_SIG_DB = 1
FMCW_MTI_RAMP, FMCW_MTI_FREEZE = 1, 2
FMCW_BEAM_NCI = 1
FMCW_RA_CAPON = 1
FMCW_MUSIC_FB = 1
FMCW_DOA_EDGES, FMCW_DOA_WRAP, FMCW_DOA_INV = 1, 2, 4


class FmcwError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"fmcw:{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class Params(ct.Structure):
    """fmcw_params (include/fmcw.h)."""
    _fields_ = [
        ("nts", ct.c_int32), ("pn", ct.c_int32), ("nr", ct.c_int32), ("nd", ct.c_int32),
        ("max_targets", ct.c_int32), ("doppler_fallback_idx", ct.c_int32),
        ("if_scale", ct.c_float), ("range_thr", ct.c_float), ("doppler_thr", ct.c_float),
        ("min_d", ct.c_float), ("max_d", ct.c_float), ("dist_per_bin", ct.c_float),
    ]


class CfarParams(ct.Structure):
    """fmcw_cfar_params (include/fmcw.h)."""
    _fields_ = [
        ("guard_r", ct.c_int32), ("guard_d", ct.c_int32), ("train_r", ct.c_int32), ("train_d", ct.c_int32),
        ("r_lo", ct.c_int32), ("r_hi", ct.c_int32), ("max_det", ct.c_int32), ("flags", ct.c_int32),
        ("alpha", ct.c_float),
    ]


class OsCfarParams(ct.Structure):
    """fmcw_oscfar_params (include/fmcw.h)."""
    _fields_ = [("win", CfarParams), ("rank", ct.c_int32)]


class SigParams(ct.Structure):
    """fmcw_sig_params (include/fmcw.h)."""
    _fields_ = [
        ("r_lo", ct.c_int32), ("r_hi", ct.c_int32), ("track_half", ct.c_int32), ("dc_half", ct.c_int32),
        ("flags", ct.c_int32), ("floor_db", ct.c_float),
    ]


class ClusterParams(ct.Structure):
    """fmcw_cluster_params (include/fmcw.h)."""
    _fields_ = [("link_r", ct.c_int32), ("link_d", ct.c_int32), ("min_cells", ct.c_int32), ("max_tgt", ct.c_int32),
                ("flags", ct.c_int32)]


class Targets(ct.Structure):
    """fmcw_targets (include/fmcw.h): output pointers, [F][max_tgt] each but tgt_count [F]."""
    _fields_ = [(k, ct.c_void_p) for k in ("tgt_count", "cells", "peak_range_idx", "peak_doppler_idx", "extent_r",
                                           "extent_d", "peak_power", "peak_noise", "power", "range", "doppler")]


TARGET_INT_KEYS = ("cells", "peak_range_idx", "peak_doppler_idx", "extent_r", "extent_d")
TARGET_FLOAT_KEYS = ("peak_power", "peak_noise", "power", "range", "doppler")


class AoaParams(ct.Structure):
    """fmcw_aoa_params (include/fmcw.h)."""
    _fields_ = [("n_chan", ct.c_int32), ("max_tgt", ct.c_int32), ("flags", ct.c_int32), ("spacing", ct.c_float),
                ("w", ct.c_float * 16)]


class Angles(ct.Structure):
    """fmcw_angles (include/fmcw.h): output pointers, det_* [F][max_det], tgt_* [F][max_tgt]."""
    _fields_ = [(k, ct.c_void_p) for k in ("det_zre", "det_zim", "det_phase", "det_sin", "tgt_zre", "tgt_zim", "tgt_e0",
                                           "tgt_e1", "tgt_phase", "tgt_sin", "tgt_coh", "tgt_cells")]


ANGLE_DET_KEYS = ("det_zre", "det_zim", "det_phase", "det_sin")
ANGLE_TGT_FLOAT_KEYS = ("tgt_zre", "tgt_zim", "tgt_e0", "tgt_e1", "tgt_phase", "tgt_sin", "tgt_coh")


class TrackParams(ct.Structure):
    """fmcw_track_params (include/fmcw.h)."""
    _fields_ = [("gate_r", ct.c_float), ("gate_d", ct.c_float), ("alpha_r", ct.c_float), ("alpha_d", ct.c_float),
                ("beta_r", ct.c_float), ("confirm_hits", ct.c_int32), ("max_coast", ct.c_int32),
                ("max_trk", ct.c_int32), ("flags", ct.c_int32)]


class Tracks(ct.Structure):
    """fmcw_tracks (include/fmcw.h): output pointers, [S*F][max_trk] each but trk_count [S*F]."""
    _fields_ = [(k, ct.c_void_p) for k in ("trk_count", "trk_id", "trk_status", "trk_age", "trk_misses", "trk_range",
                                           "trk_range_rate", "trk_doppler", "trk_power")]


TRACK_INT_KEYS = ("trk_id", "trk_status", "trk_age", "trk_misses")
TRACK_FLOAT_KEYS = ("trk_range", "trk_range_rate", "trk_doppler", "trk_power")


class MtiParams(ct.Structure):
    """fmcw_mti_params (include/fmcw.h)."""
    _fields_ = [("lambda_", ct.c_float), ("flags", ct.c_int32)]


class BeamParams(ct.Structure):
    """fmcw_beam_params (include/fmcw.h): w is float w[8][8][2] laid out flat, (re, im) of beam b,
    channel a at w[16 b + 2 a]."""
    _fields_ = [("n_chan", ct.c_int32), ("n_beam", ct.c_int32), ("flags", ct.c_int32), ("w", ct.c_float * 128)]


class RaParams(ct.Structure):
    """fmcw_ra_params (include/fmcw.h)."""
    _fields_ = [("n_chan", ct.c_int32), ("n_ang", ct.c_int32), ("r_lo", ct.c_int32), ("r_hi", ct.c_int32),
                ("dc_half", ct.c_int32), ("flags", ct.c_int32), ("load", ct.c_float)]


class MusicParams(ct.Structure):
    """fmcw_music_params (include/fmcw.h)."""
    _fields_ = [("n_chan", ct.c_int32), ("n_ang", ct.c_int32), ("r_lo", ct.c_int32), ("r_hi", ct.c_int32),
                ("n_src", ct.c_int32), ("max_src", ct.c_int32), ("sweeps", ct.c_int32), ("flags", ct.c_int32),
                ("src_thr", ct.c_float)]


class DoaParams(ct.Structure):
    """fmcw_doa_params (include/fmcw.h)."""
    _fields_ = [("n_ang", ct.c_int32), ("r_lo", ct.c_int32), ("r_hi", ct.c_int32), ("max_pk", ct.c_int32),
                ("flags", ct.c_int32), ("min_abs", ct.c_float), ("min_rel", ct.c_float), ("min_prom", ct.c_float)]


class JsonField(ct.Structure):
    """fmcw_json_field (include/fmcw.h)."""
    _fields_ = [("name", ct.c_char_p), ("kind", ct.c_int32), ("data", ct.c_void_p),
                ("rows", ct.c_int64), ("cols", ct.c_int64), ("row_stride", ct.c_int64), ("col_stride", ct.c_int64)]


FMCW_JSON_STRING, FMCW_JSON_F32, FMCW_JSON_F64, FMCW_JSON_I32, FMCW_JSON_BOOL = 0, 1, 2, 3, 4

_P = ct.c_void_p
_I32, _I64, _F, _D = ct.c_int32, ct.c_int64, ct.c_float, ct.c_double
_PP = ct.POINTER(Params)

# name -> (restype, argtypes); every symbol declared in include/fmcw.h
SIGNATURES = {
    "fmcw_abi_version": (_I32, []),
    "fmcw_last_error": (ct.c_char_p, []),
    "fmcw_device_count": (ct.c_int, [ct.POINTER(_I32)]),
    "fmcw_default_devices": (ct.c_int, [_I32, ct.POINTER(_I32), ct.POINTER(_I32)]),
    "fmcw_ctx_create": (ct.c_int, [_I32, ct.POINTER(_I32), ct.POINTER(_P)]),
    "fmcw_ctx_destroy": (ct.c_int, [_P]),
    "fmcw_ctx_devices": (ct.c_int, [_P, ct.POINTER(_I32), ct.POINTER(_I32), ct.POINTER(_I32)]),
    "fmcw_set_taps": (ct.c_int, [_P, _PP, _P, _P, _P]),
    "fmcw_process": (ct.c_int, [_P, _PP, _P, _I32, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "fmcw_range_fft": (ct.c_int, [_P, _PP, _P, _I32, _I64, _P, _P]),
    "fmcw_stft_sizes": (ct.c_int, [_I64, _I32, _I32, _I32, _I32, ct.POINTER(_I64), ct.POINTER(_I32),
                                   ct.POINTER(_I32)]),
    "fmcw_stft": (ct.c_int, [_P, _P, _I64, _P, _I32, _I32, _I32, _D, _I32, _P, _P, _P]),
    "fmcw_process_device": (ct.c_int, [_P, _PP, _P, _I32, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I64,
                                       _P, _P]),
    "fmcw_range_fft_device": (ct.c_int, [_P, _PP, _P, _I32, _I64, _P, _I32, _P, _P]),
    "fmcw_process_slow_device": (ct.c_int, [_P, _PP, _P, _I32, _I64, _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P, _P,
                                            _P]),
    "fmcw_compact_device": (ct.c_int, [_P, _P, _I64, _I32, _P, _P, _P]),
    "fmcw_stft_power_device": (ct.c_int, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P, _I32, _I32, _I32, _D, _I64,
                                          _P, _P, _P, _P]),
    "fmcw_stft_db_device": (ct.c_int, [_P, _P, _P, _I64, _I32, _D, _P, _I32, _P, _P]),
    "fmcw_stft_db_direct_device": (ct.c_int, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P, _I32, _I32, _I32, _D, _I64,
                                              _P, _P, _P]),
    "fmcw_synth_device": (ct.c_int, [_P, _PP, _I64, _I64, _P, _I32, _P]),
    "fmcw_timing_enable": (ct.c_int, [_P, _I32]),
    "fmcw_timing_read": (ct.c_int, [_P, _I32, ct.POINTER(_D), ct.POINTER(_I64)]),
    "fmcw_timing_reset": (ct.c_int, [_P]),
    "fmcw_set_chunk_frames": (ct.c_int, [_P, _I64]),
    "fmcw_set_pipeline": (ct.c_int, [_P, _I32]),
    "fmcw_synchronize": (ct.c_int, [_P]),
    "fmcw_rdx_clock": (ct.c_int, [_P, ct.POINTER(_D), ct.POINTER(_D)]),
    "fmcw_copy_device": (ct.c_int, [_P, _P, _P, _I64, _P]),
    "fmcw_cfar_check": (ct.c_int, [ct.POINTER(CfarParams), _I32, _I32, ct.POINTER(_I32)]),
    "fmcw_cfar_alpha": (ct.c_int, [_I32, _D, ct.POINTER(_F)]),
    "fmcw_cfar_device": (ct.c_int, [_P, ct.POINTER(CfarParams), _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P,
                                    _P]),
    "fmcw_cfar": (ct.c_int, [_P, ct.POINTER(CfarParams), _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "fmcw_oscfar_check": (ct.c_int, [ct.POINTER(OsCfarParams), _I32, _I32, ct.POINTER(_I32)]),
    "fmcw_oscfar_alpha": (ct.c_int, [_I32, _I32, _D, ct.POINTER(_F)]),
    "fmcw_oscfar_device": (ct.c_int, [_P, ct.POINTER(OsCfarParams), _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P,
                                      _P]),
    "fmcw_oscfar": (ct.c_int, [_P, ct.POINTER(OsCfarParams), _P, _I32, _I64, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "fmcw_sig_check": (ct.c_int, [ct.POINTER(SigParams), _I32, _I32]),
    "fmcw_sig_device": (ct.c_int, [_P, ct.POINTER(SigParams), _P, _I32, _I64, _I32, _I32, _P, _I32, _P, _P, _P, _P, _P]),
    "fmcw_sig_db_device": (ct.c_int, [_P, _P, _I64, _P, _F, _P, _P]),
    "fmcw_sig": (ct.c_int, [_P, ct.POINTER(SigParams), _P, _I32, _I64, _I32, _I32, _P, _I32, _P, _P, _P, _P]),
    "fmcw_cluster_check": (ct.c_int, [ct.POINTER(ClusterParams), _I32, _I32, _I32]),
    "fmcw_cluster_device": (ct.c_int, [_P, ct.POINTER(ClusterParams), _I64, _I32, _I32, _I32, _P, _P, _P, _P, _P,
                                       ct.POINTER(Targets), _P, _P]),
    "fmcw_cluster": (ct.c_int, [_P, ct.POINTER(ClusterParams), _I64, _I32, _I32, _I32, _P, _P, _P, _P, _P,
                                ct.POINTER(Targets), _P]),
    "fmcw_aoa_check": (ct.c_int, [ct.POINTER(AoaParams), _I32, _I32, _I32]),
    "fmcw_aoa_device": (ct.c_int, [_P, ct.POINTER(AoaParams), ct.POINTER(_P), _I32, _I64, _I32, _I32, _I32, _P, _P, _P, _P,
                                   ct.POINTER(Angles), _P]),
    "fmcw_aoa": (ct.c_int, [_P, ct.POINTER(AoaParams), ct.POINTER(_P), _I32, _I64, _I32, _I32, _I32, _P, _P, _P, _P,
                            ct.POINTER(Angles)]),
    "fmcw_track_check": (ct.c_int, [ct.POINTER(TrackParams), _I32, _I32, _I32]),
    "fmcw_track_state_bytes": (_I32, [_I32]),
    "fmcw_track_device": (ct.c_int, [_P, ct.POINTER(TrackParams), _I64, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _P,
                                     ct.POINTER(Tracks), _P, _P]),
    "fmcw_track": (ct.c_int, [_P, ct.POINTER(TrackParams), _I64, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _P,
                              ct.POINTER(Tracks), _P]),
    "fmcw_mti_check": (ct.c_int, [ct.POINTER(MtiParams), _I32, _I32]),
    "fmcw_mti_ring": (_I32, [_I32]),
    "fmcw_mti_device": (ct.c_int, [_P, ct.POINTER(MtiParams), _P, _I32, _I64, _I64, _I32, _I32, _P, _P, _P, _P]),
    "fmcw_mti": (ct.c_int, [_P, ct.POINTER(MtiParams), _P, _I32, _I64, _I64, _I32, _I32, _P, _P, _P]),
    "fmcw_beam_check": (ct.c_int, [ct.POINTER(BeamParams), _I32, _I32]),
    "fmcw_beam_steer": (ct.c_int, [_I32, _I32, _F, _P, _P, _P, _I32, ct.POINTER(BeamParams)]),
    "fmcw_beam_device": (ct.c_int, [_P, ct.POINTER(BeamParams), ct.POINTER(_P), _I32, _I64, _I32, _I32, ct.POINTER(_P), _P]),
    "fmcw_beam": (ct.c_int, [_P, ct.POINTER(BeamParams), ct.POINTER(_P), _I32, _I64, _I32, _I32, ct.POINTER(_P)]),
    "fmcw_ra_check": (ct.c_int, [ct.POINTER(RaParams), _I32, _I32]),
    "fmcw_ra_steer": (ct.c_int, [_I32, _I32, _F, _P, _P, _P, _I32, _P]),
    "fmcw_cov_device": (ct.c_int, [_P, ct.POINTER(RaParams), ct.POINTER(_P), _I32, _I64, _I32, _I32, _P, _P]),
    "fmcw_ra_device": (ct.c_int, [_P, ct.POINTER(RaParams), _P, _I64, _I32, _P, _P, _P, _P]),
    "fmcw_ra": (ct.c_int, [_P, ct.POINTER(RaParams), ct.POINTER(_P), _I32, _I64, _I32, _I32, _P, _P, _P, _P]),
    "fmcw_music_check": (ct.c_int, [ct.POINTER(MusicParams), _I32]),
    "fmcw_music_device": (ct.c_int, [_P, ct.POINTER(MusicParams), _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "fmcw_music": (ct.c_int, [_P, ct.POINTER(MusicParams), _P, _I64, _I32, _P, _P, _P, _P, _P, _P]),
    "fmcw_doa_check": (ct.c_int, [ct.POINTER(DoaParams), _I32]),
    "fmcw_doa_device": (ct.c_int, [_P, ct.POINTER(DoaParams), _P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "fmcw_doa": (ct.c_int, [_P, ct.POINTER(DoaParams), _P, _I64, _I32, _P, _P, _P, _P, _P, _P]),
    "fmcw_timing_read_ext": (ct.c_int, [_P, _I32, ct.POINTER(_D), ct.POINTER(_I64)]),
    "fmcw_json_write": (ct.c_int, [ct.c_char_p, ct.POINTER(JsonField), _I32, _I32, _I32, ct.POINTER(_I64)]),
    "fmcw_stft_png": (ct.c_int, [_P, _P, _I64, _P, _I32, _I32, _I32, _D, _I32, _P, _P, _P, ct.c_char_p, _I32, _I32,
                                 ct.POINTER(_I64)]),
    "fmcw_render_spectrogram_device": (ct.c_int, [_P, _P, _I32, _P, _P, _I32, _D, _D, _D, _I32, _I32, _P, _P]),
}

_lib = None


def load() -> ct.CDLL:
    """Load libfmcw.so once; raise loudly (no fallback) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's): when
    # both are used in one process, torch's copy must be the one loaded first
    # so that libfmcw binds to the same HIP runtime instead of a second one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise FmcwError(FMCW_E_HIP, f"{LIB_PATH} not found: build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    lib = ct.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fmcw_abi_version() != ABI_VERSION:
        raise FmcwError(FMCW_E_STATE, "libfmcw ABI version mismatch")
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != FMCW_OK:
        msg = load().fmcw_last_error()
        raise FmcwError(status, msg.decode() if msg else "")
