"""The fixed-point decoder's sub-block schedule (td_set_fixed_window) without a GPU: the numpy restatement
(tests/fixed_window_ref.py) against the exact restatement where the contract says they coincide, the
ABI's checks that need no device, and the lane code (csrc/td_fixed_core.h siso_window_pass) as a
stand-alone host program under ASan + UBSan against the restatement, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fixed_ref as F
import fixed_size_cases as Z
import fixed_window_ref as FW
import pyoracle as O
from fixed_host import core_host, run_core   # noqa: F401  (core_host is a fixture)
from turbo_decoder_cuda_amd import _native as N


def test_fixed_window_export():
    assert "td_set_fixed_window" in N.EXPORTS and hasattr(N.lib(), "td_set_fixed_window")
    assert C.sizeof(N.TdFixedWindowParams) == 8


def test_set_fixed_window_null_handle_is_einval():
    w = N.TdFixedWindowParams(64, 32)
    assert N.lib().td_set_fixed_window(None, C.byref(w)) == N.TD_EINVAL
    assert b"td_set_fixed_window" in N.lib().td_last_error()


def _small():
    K, f1, f2 = 40, 3, 10
    return K, f1, f2, F.quantise(O.synth_batch(K, f1, f2, 0.5, 5, 8)[1], 8)


def test_overlap_past_the_trellis_is_the_exact_decode():
    """K = 40, W = 16, overlap 48 >= L = 43: every recursion starts terminated at the trellis' ends, so
    rows and every Le equal the exact fixed decode; with overlap 0 they do not on these frames."""
    K, f1, f2, q = _small()
    rows, le, _ = F.decode(q, K, f1, f2, 4)
    w_rows, w_le = FW.decode(q, K, f1, f2, 4, 16, 48)
    assert np.array_equal(w_rows, rows) and np.array_equal(w_le, le)
    z_rows, z_le = FW.decode(q, K, f1, f2, 4, 16, 0)
    print(f"overlap 0: {int((z_rows != rows).sum())} row bits, {int((z_le != le).sum())} Le values differ")
    assert (z_rows != rows).any() and (z_le != le).any()


def test_one_sub_block_is_the_exact_decode():
    """window > L/2: nS = 1, whatever the overlap."""
    K, f1, f2, q = _small()
    rows, le, _ = F.decode(q, K, f1, f2, 2)
    w_rows, w_le = FW.decode(q, K, f1, f2, 2, 32, 0)
    assert np.array_equal(w_rows, rows) and np.array_equal(w_le, le)


def test_default_window_differs_from_exact_at_K1024():
    """K = 1024 (31, 64), 0.5 dB, seed 5, 8 steps per unit, 8 iterations: {64, 32} is not the exact decode
    on these frames, so a test against the restatement cannot pass with the window ignored."""
    K, f1, f2 = 1024, 31, 64
    q = F.quantise(O.synth_batch(K, f1, f2, 0.5, 5, 32)[1], 8)
    rows, le, _ = F.decode(q, K, f1, f2, 8)
    w_rows, w_le = FW.decode(q, K, f1, f2, 8, 64, 32)
    print(f"{{64, 32}}: {int((w_rows != rows).sum())} row bits, {int((w_le != le).sum())} Le values differ")
    assert (w_rows != rows).any() and (w_le != le).any()


def test_lambda_is_even():
    """siso_window asserts it on every value; here on saturated and random bytes, with a warm-up that
    starts from equal metrics on both sides."""
    K, f1, f2 = 40, 3, 10
    n = 3 * K + 12
    q = np.concatenate([np.full((1, n), 127, dtype=np.int8), np.full((1, n), -128, dtype=np.int8),
                        np.random.default_rng(3).integers(-128, 128, (6, n)).astype(np.int8)])
    FW.decode(q, K, f1, f2, 3, 16, 5)


# ------------------------------------------------------------------ the kernel's lane code on the host
def _run_core(exe, tmp_path, q, K, f1, f2, iters, all_iters, le_max, scale, W, g):
    return run_core(exe, tmp_path, q, O.qpp(K, f1, f2), iters, all_iters, (le_max, scale), (W, g))[:2]


CASES = [(8, 3, 4, 3, (255, 4), 16, 0), (8, 3, 4, 3, (255, 4), 16, 48),
         (13, 1, 0, 2, (31, 2), 16, 5),
         (29, 1, 0, 2, (127, 3), 16, 0), (29, 1, 0, 2, (127, 3), 16, 16),
         (40, 3, 10, 4, (255, 3), 16, 0), (40, 3, 10, 4, (255, 3), 16, 5), (40, 3, 10, 4, (255, 3), 16, 16),
         (40, 3, 10, 4, (255, 3), 16, 48),
         (1024, 31, 64, 3, (127, 3), 32, 7), (1024, 31, 64, 3, (255, 3), 64, 32), (1024, 31, 64, 3, (255, 3), 128, 384)]
# every residue of L mod 16 and the longest last sub-block (fixed_size_cases.SIZES), non-identity interleavers
CASES += [(K, *Z.interleaver(K), 3, Z.setting(K), W, g) for K in Z.SIZES for W, g in Z.WINDOWS]


@pytest.mark.parametrize("K,f1,f2,iters,setting,W,g", CASES)
def test_lane_code_on_the_host_equals_restatement(core_host, tmp_path, K, f1, f2, iters, setting, W, g):
    """Block lengths round the 16-step window and the sub-block (L = 11, 16, 32, 43, 1027: one sub-block,
    a last sub-block with a remainder, a partial last window), overlaps that are no multiple of 16,
    reach past the trellis' ends or cover it whole; AWGN at 16 steps per unit next to the saturated
    patterns; every row and every Le.  ASan watches the workspace's bounds (an odd pitch)."""
    n = 3 * K + 12
    q = np.concatenate([
        F.quantise(O.synth_batch(K, f1, f2, 1.0, 5, 3)[1], 16),
        np.full((1, n), 127, dtype=np.int8), np.full((1, n), -128, dtype=np.int8),
        (127 * (1 - 2 * (np.arange(n) & 1))).astype(np.int8)[None, :],
        np.random.default_rng(K).integers(-128, 128, (2, n)).astype(np.int8)])
    rows, le = FW.decode(q, K, f1, f2, iters, W, g, *setting)
    g_rows, g_le = _run_core(core_host, tmp_path, q, K, f1, f2, iters, True, *setting, W, g)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le)
    g_last, _ = _run_core(core_host, tmp_path, q, K, f1, f2, iters, False, *setting, W, g)
    assert np.array_equal(g_last[:, 0], rows[:, -1])
