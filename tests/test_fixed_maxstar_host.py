"""The fixed-point decoder's integer log-MAP (td_set_fixed_maxstar) without a GPU: the ABI's checks that need
no device, the table rule (td_fixed_maxstar_table against an independent numpy statement), the restatement
(tests/fixed_maxstar_ref.py) against fixed_ref on an all-zero table and against Max-Log-MAP's error count,
and the lane code (csrc/td_fixed_core.h instantiated with fx::MaxStar) as a stand-alone host program under
ASan + UBSan, bit for bit against the restatement on both schedules, with and without a stop rule.

The setter's checks that need a handle (another precision, shift, entries, corr[7]) are in
test_gpu_fixed_maxstar.py: td_create needs a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixed_maxstar_ref as M
import fixed_ref as F
import fixed_size_cases as Z
import fixed_stop_cases as S
import pyoracle as O
import window_stop_cases as W
from fixed_host import SENTINEL, core_host, run_core   # noqa: F401  (core_host is a fixture)
from turbo_decoder_cuda_amd import _native as N


def _params(shift, corr):
    return N.TdFixedMaxstarParams(int(shift), (C.c_uint8 * 8)(*corr))


# ------------------------------------------------------------------ the ABI
def test_exports_exist():
    for name in ("td_set_fixed_maxstar", "td_fixed_maxstar_table"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)
    assert N.lib().td_abi_version() == 1


def test_null_handle_is_einval():
    m = _params(*M.DEFAULT)
    assert N.lib().td_set_fixed_maxstar(None, C.byref(m)) == N.TD_EINVAL
    assert b"td_set_fixed_maxstar" in N.lib().td_last_error()
    assert N.lib().td_set_fixed_maxstar(None, None) == N.TD_EINVAL


def test_python_interface_has_the_calls():
    import turbo_decoder_cuda_amd as T
    assert callable(T.TurboCodec.set_fixed_maxstar) and callable(T.fixed_maxstar_table)


# ------------------------------------------------------------------ the table rule
def _c_table(steps, shift):
    m = N.TdFixedMaxstarParams()
    rc = N.lib().td_fixed_maxstar_table(float(steps), -1 if shift is None else shift, C.byref(m))
    return rc, (int(m.shift), tuple(int(v) for v in m.corr))


def test_default_table():
    assert _c_table(8, None) == (N.TD_OK, (3, (9, 6, 4, 3, 2, 1, 1, 0)))
    assert M.table(8) == M.DEFAULT == (3, (9, 6, 4, 3, 2, 1, 1, 0))
    from turbo_decoder_cuda_amd import fixed_maxstar_table
    assert fixed_maxstar_table(8.0) == M.DEFAULT and fixed_maxstar_table(8.0, 3) == M.DEFAULT


@pytest.mark.parametrize("steps", [2, 4, 8, 16])
def test_c_helper_equals_numpy_rule(steps):
    for shift in (None, 0, 1, 2, 3, 4, 5, 6):
        want = M.table(steps, shift)
        rc, got = _c_table(steps, shift)
        print(steps, shift, want, rc, got)
        if want is None:
            assert rc == N.TD_EINVAL
        else:
            assert rc == N.TD_OK and got == want
            assert got[1][7] == 0 and max(got[1]) <= 63 and list(got[1]) == sorted(got[1], reverse=True)


def test_table_helper_bad_arguments_are_einval_and_change_nothing():
    for steps, shift in ((0.0, -1), (-1.0, -1), (32.5, -1), (float("nan"), -1), (float("inf"), -1), (8.0, 9)):
        m = _params(2, (1, 2, 3, 4, 5, 6, 7, 0))
        assert N.lib().td_fixed_maxstar_table(steps, shift, C.byref(m)) == N.TD_EINVAL, (steps, shift)
        assert b"td_fixed_maxstar_table" in N.lib().td_last_error()
        assert (m.shift, tuple(m.corr)) == (2, (1, 2, 3, 4, 5, 6, 7, 0))
    assert N.lib().td_fixed_maxstar_table(8.0, -1, None) == N.TD_EINVAL
    assert _c_table(32, None)[0] == N.TD_OK and _c_table(32, 8)[0] == N.TD_OK


# ------------------------------------------------------------------ the restatement
def _patterns(K):
    return np.concatenate([S.FRAMES["pattern"](K, name, 1) for name in ("plus127", "minus128", "alternating")]
                          + [S.FRAMES["pattern"](K, "mixed", 4)[3:]])


@pytest.mark.parametrize("K", [8, 40, 1024])
def test_all_zero_table_is_the_maxlog_restatement(K):
    q = np.concatenate([S.FRAMES["awgn"](K, 1.0, 4), _patterns(K)])
    iters = 3
    rows, le, _ = F.decode(q, K, *S.QPP[K], iters)
    g_rows, g_le, _ = M.decode(q, K, *S.QPP[K], iters, M.ZERO, 255, 3)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le)


def test_fewer_bit_errors_than_maxlog():
    """K = 1024, 256 generator frames at 0.6 dB (seed 9), 6 iterations, 8 steps per unit: integer log-MAP
    with the default table and {255, 4} against Max-Log-MAP with {255, 3}."""
    K, f1, f2 = 1024, 31, 64
    u, flow = O.synth_batch(K, f1, f2, 0.6, 9, 256)[:2]
    q = F.quantise(flow, 8)
    maxlog = int((F.decode(q, K, f1, f2, 6, 255, 3)[0][:, -1] != u).sum())
    logmap = int((M.decode(q, K, f1, f2, 6, M.DEFAULT, 255, 4)[0][:, -1] != u).sum())
    print(f"bit errors: Max-Log-MAP {{255, 3}} {maxlog}, integer log-MAP {{255, 4}} {logmap}")
    assert logmap < maxlog


# ------------------------------------------------------------------ the kernels' lane code on the host
def _run_core(exe, tmp_path, q, K, iters, all_iters, setting, win, rule, min_iters, tab):
    return run_core(exe, tmp_path, q, O.qpp(K, *S.QPP[K]), iters, all_iters, setting, win, rule, min_iters, S.CRC24B, tab,
                    timeout=600)


@functools.lru_cache(maxsize=None)
def _host_batch(K):
    """fixed_stop_cases' host batch (AWGN and gCRC24B frames at 16 steps per unit, zeros, +127, -128, random
    bytes) and an alternating +-127 codeword."""
    q = np.concatenate([S.FRAMES["host"](K), S.FRAMES["pattern"](K, "alternating", 1)])
    q.setflags(write=False)
    return q


def _check(exe, tmp_path, q, K, iters, setting, win, tab, rules=(None, "hda", "crc"), min_iters=1):
    """The exact (win None) or sub-block pass of the program against the restatement: without a rule every
    byte; with one the frozen rows, the final bits alone, the counts, the Le of the iterations used -- and
    nothing written after a stop."""
    rows, le, _ = M.decode(q, K, *S.QPP[K], iters, tab, *setting, win=win)
    for rule in rules:
        if rule == "crc" and K <= 24:
            continue
        if rule is None:
            g_rows, g_le, g_used = _run_core(exe, tmp_path, q, K, iters, True, setting, win, None, 1, tab)
            assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le) and (g_used == iters).all()
            g_last, g_le, _ = _run_core(exe, tmp_path, q, K, iters, False, setting, win, None, 1, tab)
            assert np.array_equal(g_last[:, 0], rows[:, -1]) and np.array_equal(g_le, le)
            continue
        used = W.stops(rows, rule, min_iters, S.CRC24B)
        print(f"K={K} {win} {tab} {rule}: {W.spread(used)}")
        g_rows, g_le, g_used = _run_core(exe, tmp_path, q, K, iters, True, setting, win, rule, min_iters, tab)
        assert np.array_equal(g_used, used), (W.spread(g_used), W.spread(used))
        assert np.array_equal(g_rows, W.frozen(rows, used))
        mask = S.le_mask(used, iters)
        assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))
        assert (np.where(mask, SENTINEL, g_le) == SENTINEL).all(), "a stopped codeword writes no Le"
        g_last, _, g_used = _run_core(exe, tmp_path, q, K, iters, False, setting, win, rule, min_iters, tab)
        assert np.array_equal(g_used, used)
        assert np.array_equal(g_last[:, 0], rows[np.arange(len(used)), used - 1])
    return rows


# K = 8 .. 1024 as the issue lists them, and two lengths of fixed_size_cases.SIZES for each residue of
# L = K + 3 modulo the 16-step window at which the lane code takes another path: 0 (the last window is
# whole: 13 above and 109, 189), 1 (it is one step: 14, 110), 15 (one step short: 28, 124) -- and 188,
# L = 191, whose last sub-block at W = 64 is the longest the contract allows
LENGTHS = [8, 13, 16, 29, 40, 1024, 14, 28, 109, 110, 124, 188, 189]
TABLES = [(M.DEFAULT, (255, 4)), (M.table(16), (127, 3)), (M.CONSTANT, (31, 2))]


@pytest.mark.parametrize("K", LENGTHS)
def test_lane_code_equals_restatement(core_host, tmp_path, K):
    assert K in S.QPP and (K in (8, 13, 16, 29, 40, 1024) or K in Z.SIZES)
    q = _host_batch(K)
    iters = 4 if K < 1024 else 3
    at = LENGTHS.index(K)
    for j, (tab, setting) in enumerate(TABLES):
        wins = Z.WINDOWS if K < 1024 and j == 0 else [Z.WINDOWS[(at + j) % len(Z.WINDOWS)]]
        exact = _check(core_host, tmp_path, q, K, iters, setting, None, tab)
        differs = 0
        for win in wins:
            rows = _check(core_host, tmp_path, q, K, iters, setting, win, tab, min_iters=1 + (at + j) % 3)
            if Z.window_is_exact_by_contract(K, win):
                assert np.array_equal(rows, exact)
            differs += int((rows != exact).any())
        if j == 0:
            maxlog = F.decode(q, K, *S.QPP[K], iters, *setting)[0]
            assert (exact != maxlog).any(), "the table changes decisions on this batch"
            assert K < 40 or differs, "a sub-block decode that is not the exact one"


def test_maxlog_instantiation_of_the_program_is_fixed_ref(core_host, tmp_path):
    """The program with the table off runs the MaxLog instantiation: fixed_ref's bytes."""
    K, iters = 40, 4
    q = _host_batch(K)
    rows, le, _ = F.decode(q, K, *S.QPP[K], iters)
    g_rows, g_le, _ = _run_core(core_host, tmp_path, q, K, iters, True, (255, 3), None, None, 1, None)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le)
    z_rows, z_le, _ = _run_core(core_host, tmp_path, q, K, iters, True, (255, 3), None, None, 1, M.ZERO)
    assert np.array_equal(z_rows, rows) and np.array_equal(z_le, le)


def test_widest_table_stays_inside_int32_at_the_longest_block(core_host, tmp_path):
    """{63 x 7, 0} with shift 8 and {255, 4} at K = 10000 on the saturated patterns: the int32 lane code under
    UBSan (a signed overflow is an error) against the restatement's int64 metrics -- the overflow bound of
    td_fixed_core.h, 572 * 10003 < 2^23."""
    K, iters = 10000, 2
    q = np.concatenate([S.FRAMES["pattern"](K, name, 1) for name in ("plus127", "minus128", "alternating")])
    _check(core_host, tmp_path, q, K, iters, (255, 4), None, M.WIDEST, rules=(None, "hda"))
    _check(core_host, tmp_path, q, K, iters, (255, 4), (64, 16), M.WIDEST, rules=(None,))
