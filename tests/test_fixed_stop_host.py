"""Early termination of the fixed-point decoder (td_set_fixed_stop) without a GPU: the ABI's checks,
and the stopping lane code of the gfx950 kernel (csrc/td_fixed_core.h decode_codeword_stop) as a
stand-alone host program under ASan + UBSan against the rule applied to fixed_ref.decode's rows."""
import ctypes as C

import numpy as np
import pytest

import fixed_size_cases as Z
import fixed_stop_cases as S
import pyoracle as O
import window_stop_cases as W
from fixed_host import SENTINEL, core_host, run_core   # noqa: F401  (core_host is a fixture)
from turbo_decoder_cuda_amd import _native as N


def test_export_exists():
    assert "td_set_fixed_stop" in N.EXPORTS and hasattr(N.lib(), "td_set_fixed_stop")
    assert N.lib().td_abi_version() == 1


def test_null_handle_is_einval():
    s = N.TdStopParams(N.TD_STOP_HDA, 1, 0)
    assert N.lib().td_set_fixed_stop(None, C.byref(s)) == N.TD_EINVAL
    assert b"td_set_fixed_stop" in N.lib().td_last_error()
    assert N.lib().td_set_fixed_stop(None, None) == N.TD_EINVAL


# ------------------------------------------------------------------ the kernel's lane code on the host
def _run_core(exe, tmp_path, q, K, iters, all_iters, setting, rule, min_iters, poly):
    return run_core(exe, tmp_path, q, O.qpp(K, *S.QPP[K]), iters, all_iters, setting, None, rule, min_iters, poly)


# block lengths round the 16-step window (L = 11, 16, 19, 32, 43, 1027), as test_fixed_host.py
@pytest.mark.parametrize("K,iters,setting", [(8, 4, (255, 4)), (13, 4, (31, 2)), (16, 4, (255, 3)), (29, 4, (127, 3)),
                                             (40, 6, (255, 3)), (1024, 5, (127, 3))]
                         + [(K, 4, Z.setting(K)) for K in Z.SIZES if K not in (8, 13, 16)])
def test_stopping_lane_code_on_the_host_equals_rule_on_restatement(core_host, tmp_path, K, iters, setting):
    """HDA, and CRC with gCRC24B where K > 24; min_iters 1 and 3; with and without all_iters: the rows
    (frozen), the counts, the Le of iterations <= used -- and nothing written after a stop."""
    key = ("host",)
    q, rows, le = S.reference(key, K, iters, setting)
    seen = set()
    for rule in ("hda", "crc") if K > 24 else ("hda",):
        for min_iters in (1, 3):
            used = S.used(key, K, iters, setting, rule, min_iters)
            print(f"K={K} {rule} min_iters={min_iters}: {W.spread(used)}")
            seen.update(int(v) for v in used)
            assert used.min() >= max(2 if rule == "hda" else 1, min_iters)
            g_rows, g_le, g_used = _run_core(core_host, tmp_path, q, K, iters, True, setting, rule, min_iters, S.CRC24B)
            assert np.array_equal(g_used, used)
            assert np.array_equal(g_rows, W.frozen(rows, used))
            mask = S.le_mask(used, iters)
            assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))
            assert (np.where(mask, SENTINEL, g_le) == SENTINEL).all(), "a stopped codeword writes no Le"
            g_last, _, g_used = _run_core(core_host, tmp_path, q, K, iters, False, setting, rule, min_iters, S.CRC24B)
            assert np.array_equal(g_used, used)
            assert np.array_equal(g_last[:, 0], rows[np.arange(len(used)), used - 1])
    assert min(seen) < iters and len(seen) >= 2, "the batch's codewords stop early, and not all together"


def test_min_iters_equal_to_iterations_is_the_full_decode(core_host, tmp_path):
    K, iters, setting = 40, 4, (255, 3)
    q, rows, le = S.reference(("host",), K, iters, setting)
    for rule in ("hda", "crc"):
        g_rows, g_le, g_used = _run_core(core_host, tmp_path, q, K, iters, True, setting, rule, iters, S.CRC24B)
        assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le) and (g_used == iters).all()
