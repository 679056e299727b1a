"""Early termination of the fixed-point decoder's sub-block schedule (td_set_fixed_window_stop) without a
GPU: the ABI's checks that need no device, and the stopping lane code with the judge (csrc/td_fixed_core.h
siso_window_pass with STOP, window_judge) as a stand-alone host program under ASan + UBSan against the rule
applied to fixed_window_ref.decode's rows."""
import ctypes as C

import numpy as np
import pytest

import fixed_size_cases as Z
import fixed_window_stop_cases as FS
import pyoracle as O
import window_stop_cases as W
from fixed_host import SENTINEL, core_host, run_core   # noqa: F401  (core_host is a fixture)
from turbo_decoder_cuda_amd import _native as N


def test_export_exists():
    assert "td_set_fixed_window_stop" in N.EXPORTS and hasattr(N.lib(), "td_set_fixed_window_stop")
    assert N.lib().td_abi_version() == 1


def test_null_handle_is_einval():
    s = N.TdStopParams(N.TD_STOP_HDA, 1, 0)
    assert N.lib().td_set_fixed_window_stop(None, C.byref(s)) == N.TD_EINVAL
    assert b"td_set_fixed_window_stop" in N.lib().td_last_error()
    assert N.lib().td_set_fixed_window_stop(None, None) == N.TD_EINVAL


def test_python_interface_has_the_call():
    from turbo_decoder_cuda_amd import TurboCodec
    assert callable(TurboCodec.set_fixed_window_early_stop)


# ------------------------------------------------------------------ the kernels' lane code on the host
def _run_core(exe, tmp_path, q, K, iters, all_iters, setting, win, rule, min_iters, poly):
    return run_core(exe, tmp_path, q, O.qpp(K, *FS.QPP[K]), iters, all_iters, setting, win, rule, min_iters, poly)


def _check(exe, tmp_path, K, iters, setting, win, rule, min_iters, seen):
    q, rows, le = FS.host_case(K, iters, win, setting)
    used = W.stops(rows, rule, min_iters, FS.CRC24B)
    print(f"K={K} {win} {rule} min_iters={min_iters}: {W.spread(used)}")
    seen.update(int(v) for v in used)
    assert used.min() >= max(2 if rule == "hda" else 1, min_iters)
    g_rows, g_le, g_used = _run_core(exe, tmp_path, q, K, iters, True, setting, win, rule, min_iters, FS.CRC24B)
    assert np.array_equal(g_used, used), (W.spread(g_used), W.spread(used))
    assert np.array_equal(g_rows, W.frozen(rows, used))
    mask = FS.le_mask(used, iters)
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))
    assert (np.where(mask, SENTINEL, g_le) == SENTINEL).all(), "a stopped codeword writes no Le"
    g_last, _, g_used = _run_core(exe, tmp_path, q, K, iters, False, setting, win, rule, min_iters, FS.CRC24B)
    assert np.array_equal(g_used, used)
    assert np.array_equal(g_last[:, 0], rows[np.arange(len(used)), used - 1])


@pytest.mark.parametrize("K", Z.SIZES)
def test_stopping_lane_code_at_every_size_equals_rule_on_restatement(core_host, tmp_path, K):
    """Every residue of L mod 16 and the longest last sub-block through {16, 0}, {16, 5}, {32, 7} and {64, 48}:
    HDA, and CRC with gCRC24B where K > 24, min_iters 1 and (one window a size) 3; the rows (frozen), the
    final bits alone, the counts, the Le of iterations <= used -- and nothing written after a stop."""
    seen = set()
    for j, win in enumerate(Z.WINDOWS):
        for rule in ("hda", "crc") if K > 24 else ("hda",):
            _check(core_host, tmp_path, K, 4, Z.setting(K), win, rule, 1, seen)
            if j == Z.SIZES.index(K) % len(Z.WINDOWS):
                _check(core_host, tmp_path, K, 4, Z.setting(K), win, rule, 3, seen)
    assert min(seen) < 4 and len(seen) >= 2, "the batch's codewords stop early, and not all together"


@pytest.mark.parametrize("K,iters,setting,win", [(40, 6, (255, 3), (16, 0)), (40, 6, (255, 3), (16, 5)),
                                                 (40, 6, (255, 3), (16, 48)), (200, 5, (255, 3), (32, 7)),
                                                 (200, 5, (31, 2), (16, 0)), (1024, 5, (127, 3), (64, 48)),
                                                 (1024, 5, (255, 3), (32, 7))])
def test_stopping_lane_code_equals_rule_on_restatement(core_host, tmp_path, K, iters, setting, win):
    seen = set()
    for rule in ("hda", "crc"):
        for min_iters in (1, 3):
            _check(core_host, tmp_path, K, iters, setting, win, rule, min_iters, seen)
    assert min(seen) < iters and len(seen) >= 2, "the batch's codewords stop early, and not all together"


def test_min_iters_equal_to_iterations_is_the_full_decode(core_host, tmp_path):
    K, iters, setting, win = 40, 4, (255, 3), (16, 5)
    q, rows, le = FS.host_case(K, iters, win, setting)
    for rule in ("hda", "crc"):
        g_rows, g_le, g_used = _run_core(core_host, tmp_path, q, K, iters, True, setting, win, rule, iters, FS.CRC24B)
        assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le) and (g_used == iters).all()
