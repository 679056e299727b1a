"""ctypes binding of libturbo_mi355x.so (the C ABI in include/turbo_mi355x.h).

The library is built in-tree by turbo_decoder_cuda_amd/build.py.  There is no fallback: if
the shared object is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TD_LIB_PATH") or os.path.join(PKG, "libturbo_mi355x.so")

TD_OK, TD_EINVAL, TD_ENOMEM, TD_EHIP, TD_ENODEV = 0, 1, 2, 3, 4
TD_ALGO_LOGMAP, TD_ALGO_MAXLOG = 0, 1
TD_F64, TD_F32, TD_FIXED = 0, 1, 2
TD_WMAXSTAR_FAST, TD_WMAXSTAR_EXACT = 0, 1
TD_MAXSTAR_WINDOW_FAST = 2   # td_maxstar_host_* algo: the windowed one-read table
TD_STOP_NONE, TD_STOP_HDA, TD_STOP_CRC = 0, 1, 2
CRC24A, CRC24B = 0x864CFB, 0x800063   # the LTE generators' 24 low-order coefficients (td_stop_params.crc_poly)

# every symbol include/turbo_mi355x.h declares (tests check the .so exports all of them)
EXPORTS = (
    "td_create", "td_destroy", "td_reserve", "td_decode_device", "td_decode_host", "td_siso_host",
    "td_last_error", "td_device_count", "td_abi_version", "td_maxstar_host_f64", "td_maxstar_host_f32",
    "td_trellis_tables", "td_qpp_table", "td_profile_enable", "td_profile_read", "td_debug_set_stamps",
    "td_debug_stamp_slots", "td_synth_seed", "td_synth_frames", "td_count_errors", "td_rand_window", "td_synth_seek",
    "td_set_window", "td_synth_modulation", "td_modulate", "td_demodulate", "td_debug_placement",
    "td_debug_placement_rule", "td_clock_read", "td_window_steps", "td_debug_placement_cost", "td_debug_window_layout",
    "td_debug_workspace_bytes", "td_set_window_maxstar", "td_set_early_stop", "td_decode_device_stop",
    "td_decode_host_stop", "td_crc24_host", "td_crc24_syndromes", "td_set_window_stop",
    "td_rm_set", "td_rm_info", "td_rate_match", "td_rate_dematch", "td_rm_index_host",
    "td_set_fixed", "td_set_fixed_stop", "td_set_fixed_window", "td_set_fixed_window_stop",
    "td_set_fixed_maxstar", "td_fixed_maxstar_table", "td_set_fixed_window_nii", "td_debug_workspace_fill",
    "td_encode_device", "td_crc_set", "td_crc_attach", "td_crc_check",
    "td_llr_convert", "td_demod_dematch",
    "td_tb_plan_host", "td_tb_rm_sizes_host", "td_rm_index_host_filler", "td_tb_create", "td_tb_destroy",
    "td_tb_get_plan", "td_tb_segment", "td_tb_rate_match", "td_tb_rate_dematch", "td_tb_concat",
    "td_gold_sequence", "td_gold_sequence_host", "td_scramble", "td_descramble_llr", "td_tb_demod_dematch",
)


class TdParams(C.Structure):
    _fields_ = [
        ("K", C.c_int), ("f1", C.c_int), ("f2", C.c_int), ("iterations", C.c_int),
        ("algo", C.c_int), ("precision", C.c_int), ("device", C.c_int),
    ]


class TdWindowParams(C.Structure):
    _fields_ = [("window", C.c_int), ("overlap", C.c_int), ("nii", C.c_int), ("concurrent", C.c_int),
                ("ext_scale", C.c_double)]


class TdStopParams(C.Structure):
    _fields_ = [("rule", C.c_int), ("min_iters", C.c_int), ("crc_poly", C.c_uint32)]


class TdFixedParams(C.Structure):
    _fields_ = [("le_max", C.c_int), ("ext_scale_q", C.c_int)]


class TdFixedWindowParams(C.Structure):
    _fields_ = [("window", C.c_int), ("overlap", C.c_int)]


class TdFixedMaxstarParams(C.Structure):
    _fields_ = [("shift", C.c_int), ("corr", C.c_uint8 * 8)]


class TdTbPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("A", "B", "L", "C", "K_plus", "K_minus", "C_plus", "C_minus", "F")]


class TdTbParams(C.Structure):
    _fields_ = [("A", C.c_int), ("Ncb_cap", C.c_int), ("device", C.c_int), ("filler_llr", C.c_double)]


class TurboError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"turbo_mi355x error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m turbo_decoder_cuda_amd.build` "
            "(there is no CPU fallback)")
    try:   # torch ships its own libamdhip64.so.7 (same soname): load it first so the library and
        import torch  # noqa: F401  torch bind to one HIP runtime (the other order hides the GPUs from torch)
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P, I = C.c_void_p, C.c_int
    L.td_create.argtypes = [C.POINTER(P), C.POINTER(TdParams)]
    L.td_destroy.argtypes = [P]
    L.td_reserve.argtypes = [P, I]
    L.td_decode_device.argtypes = [P, P, I, P, I, P, P]
    L.td_decode_host.argtypes = [P, P, I, P, P]
    L.td_siso_host.argtypes = [P, P, P, I, P, I, I]
    L.td_last_error.restype = C.c_char_p
    L.td_device_count.restype = I
    L.td_abi_version.restype = I
    L.td_maxstar_host_f64.argtypes = [C.c_double, C.c_double, I]
    L.td_maxstar_host_f64.restype = C.c_double
    L.td_maxstar_host_f32.argtypes = [C.c_float, C.c_float, I]
    L.td_maxstar_host_f32.restype = C.c_float
    L.td_trellis_tables.argtypes = [P, P, P]
    L.td_qpp_table.argtypes = [I, I, I, P]
    L.td_profile_enable.argtypes = [P, I]
    L.td_debug_set_stamps.argtypes = [P, P]
    L.td_debug_stamp_slots.restype = I
    L.td_debug_placement.argtypes = [P, C.POINTER(C.c_float), I, C.POINTER(C.c_int)]
    L.td_debug_placement_rule.argtypes = [C.POINTER(C.c_float), I]
    if hasattr(L, "td_debug_placement_cost"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_debug_placement_cost.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.td_profile_read.argtypes = [P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    if hasattr(L, "td_clock_read"):   # measurement support (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_clock_read.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.td_synth_seed.argtypes = [P, C.c_uint]
    L.td_rand_window.argtypes = [C.c_uint, C.c_ulonglong, P]
    L.td_synth_seek.argtypes = [P, C.c_ulonglong]
    L.td_synth_frames.argtypes = [P, C.c_double, I, P, P, P]
    L.td_count_errors.argtypes = [P, P, I, P, I, P, P]
    L.td_set_window.argtypes = [P, C.POINTER(TdWindowParams)]
    if hasattr(L, "td_set_early_stop"):   # early termination (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_early_stop.argtypes = [P, C.POINTER(TdStopParams)]
        L.td_decode_device_stop.argtypes = [P, P, I, P, I, P, P, P]
        L.td_decode_host_stop.argtypes = [P, P, I, P, P, P]
        L.td_crc24_host.argtypes = [P, I, C.c_uint32]
        L.td_crc24_host.restype = C.c_uint32
        L.td_crc24_syndromes.argtypes = [I, C.c_uint32, P]
    if hasattr(L, "td_set_window_stop"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_window_stop.argtypes = [P, C.POINTER(TdStopParams)]
    if hasattr(L, "td_rm_set"):   # rate matching (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_rm_set.argtypes = [P, I]
        L.td_rm_info.argtypes = [P] + [C.POINTER(C.c_int)] * 5
        L.td_rate_match.argtypes = [P, P, I, I, I, I, P, P]
        L.td_rate_dematch.argtypes = [P, P, I, I, I, P, I, P]
        L.td_rm_index_host.argtypes = [I, I, I, I, P]
    if hasattr(L, "td_set_fixed"):   # the fixed-point decoder (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_fixed.argtypes = [P, C.POINTER(TdFixedParams)]
    if hasattr(L, "td_set_fixed_stop"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_fixed_stop.argtypes = [P, C.POINTER(TdStopParams)]
    if hasattr(L, "td_set_fixed_window"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_fixed_window.argtypes = [P, C.POINTER(TdFixedWindowParams)]
    if hasattr(L, "td_set_fixed_window_stop"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_fixed_window_stop.argtypes = [P, C.POINTER(TdStopParams)]
    if hasattr(L, "td_set_fixed_window_nii"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_fixed_window_nii.argtypes = [P, I]
    if hasattr(L, "td_set_fixed_maxstar"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_set_fixed_maxstar.argtypes = [P, C.POINTER(TdFixedMaxstarParams)]
        L.td_fixed_maxstar_table.argtypes = [C.c_double, I, C.POINTER(TdFixedMaxstarParams)]
    if hasattr(L, "td_debug_workspace_fill"):   # (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_debug_workspace_fill.argtypes = [P, I, C.POINTER(C.c_ulonglong)]
    if hasattr(L, "td_encode_device"):   # the transmit side (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_encode_device.argtypes = [P, P, I, P, P]
        L.td_crc_set.argtypes = [P, C.c_uint32]
        L.td_crc_attach.argtypes = [P, P, I, P]
        L.td_crc_check.argtypes = [P, P, I, P, P]
    if hasattr(L, "td_llr_convert"):   # the receive front end (older A/B builds loaded by TD_LIB_PATH lack it)
        L.td_llr_convert.argtypes = [P, C.c_longlong, I, C.c_double, P, P]
        L.td_demod_dematch.argtypes = [P, P, P, I, I, I, I, C.c_double, C.c_double, P, I, P]
    if hasattr(L, "td_tb_create"):   # transport blocks (older A/B builds loaded by TD_LIB_PATH lack them)
        LL = C.c_longlong
        L.td_tb_plan_host.argtypes = [I, C.POINTER(TdTbPlan)]
        L.td_tb_rm_sizes_host.argtypes = [C.POINTER(TdTbPlan), LL] + [I] + [C.POINTER(C.c_int)] * 3
        L.td_rm_index_host_filler.argtypes = [I, I, I, I, I, P]
        L.td_tb_create.argtypes = [C.POINTER(P), C.POINTER(TdTbParams)]
        L.td_tb_destroy.argtypes = [P]
        L.td_tb_get_plan.argtypes = [P, C.POINTER(TdTbPlan)]
        L.td_tb_segment.argtypes = [P, P, I, P, P, P]
        L.td_tb_rate_match.argtypes = [P, P, P, I, I, LL, I, P, P]
        L.td_tb_rate_dematch.argtypes = [P, P, I, I, I, LL, I, P, P, I, P]
        L.td_tb_concat.argtypes = [P, P, P, I, P, P, P, P]
    if hasattr(L, "td_gold_sequence"):   # scrambling (older A/B builds loaded by TD_LIB_PATH lack it)
        LL = C.c_longlong
        L.td_gold_sequence.argtypes = [P, I, LL, P, P]
        L.td_gold_sequence_host.argtypes = [C.c_uint32, LL, P]
        L.td_scramble.argtypes = [P, P, I, LL, P, P]
        L.td_descramble_llr.argtypes = [P, I, P, I, LL, P, P]
        L.td_tb_demod_dematch.argtypes = [P, P, P, I, I, I, LL, I, I, C.c_double, C.c_double, P, P, P, I, P]
    L.td_synth_modulation.argtypes = [P, I]
    L.td_modulate.argtypes = [P, C.c_longlong, I, P, P, P]
    L.td_demodulate.argtypes = [P, P, C.c_longlong, I, C.c_double, P, P]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != TD_OK:
        raise TurboError(rc, lib().td_last_error().decode(errors="replace"))
