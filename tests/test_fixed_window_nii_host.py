"""Next-iteration initialisation of the fixed-point decoder's sub-block schedule (td_set_fixed_window_nii)
without a GPU: the identities of the numpy restatement (tests/fixed_window_nii_ref.py), the ABI's checks that
need no device, and the lane code (csrc/td_fixed_core.h siso_window_pass with NII) as a stand-alone host program
under ASan + UBSan against the restatement, bit for bit."""
import numpy as np
import pytest

import fixed_maxstar_ref as FM
import fixed_ref as F
import fixed_window_nii_cases as NC
import fixed_window_nii_ref as FN
import fixed_window_ref as FW
import pyoracle as O
from fixed_host import core_host, run_core   # noqa: F401  (core_host is a fixture)
from turbo_decoder_cuda_amd import _native as N


def test_fixed_window_nii_export():
    assert "td_set_fixed_window_nii" in N.EXPORTS and hasattr(N.lib(), "td_set_fixed_window_nii")


def test_set_fixed_window_nii_null_handle_is_einval():
    assert N.lib().td_set_fixed_window_nii(None, 1) == N.TD_EINVAL
    assert b"td_set_fixed_window_nii" in N.lib().td_last_error()


# ------------------------------------------------------------------ the restatement's identities
def _small():
    K, f1, f2 = 40, 3, 10
    return K, f1, f2, F.quantise(O.synth_batch(K, f1, f2, 0.5, 5, 8)[1], 8)


def test_iteration_one_is_the_nii_off_decode():
    """Nothing is loaded in iteration 1: its row and both its Le equal fixed_window_ref's, plain max and (against
    fixed_maxstar_ref's sub-block geometry) with a table."""
    K, f1, f2, q = _small()
    rows, le = FN.decode(q, K, f1, f2, 3, 16, 16)
    w_rows, w_le = FW.decode(q, K, f1, f2, 3, 16, 16)
    assert np.array_equal(rows[:, 0], w_rows[:, 0]) and np.array_equal(le[:, 0], w_le[:, 0])
    rows, le = FN.decode(q, K, f1, f2, 2, 16, 16, FM.DEFAULT, 255, 4)
    m_rows, m_le, _ = FM.decode(q, K, f1, f2, 2, FM.DEFAULT, 255, 4, win=(16, 16))
    assert np.array_equal(rows[:, 0], m_rows[:, 0]) and np.array_equal(le[:, 0], m_le[:, 0])


@pytest.mark.parametrize("W,g", [(16, 48), (32, 0), (32, 16)])
def test_no_inner_start_is_the_exact_decode(W, g):
    """Overlap 48 >= L = 43, or one sub-block (window 32 > L / 2): nothing starts inside the trellis."""
    K, f1, f2, q = _small()
    rows, le, _ = F.decode(q, K, f1, f2, 4)
    n_rows, n_le = FN.decode(q, K, f1, f2, 4, W, g)
    assert np.array_equal(n_rows, rows) and np.array_equal(n_le, le)
    m_rows, m_le, _ = FM.decode(q, K, f1, f2, 4, FM.DEFAULT, 255, 4)
    n_rows, n_le = FN.decode(q, K, f1, f2, 4, W, g, FM.DEFAULT, 255, 4)
    assert np.array_equal(n_rows, m_rows) and np.array_equal(n_le, m_le)


@pytest.mark.parametrize("K,W,g", [(40, 16, 0), (62, 16, 16), (63, 16, 16), (1024, 64, 64)])
@pytest.mark.parametrize("table", [False, True])
def test_a_constant_added_to_every_stored_vector_changes_no_byte(K, W, g, table):
    """A and B are defined up to one constant per vector: an implementation may store them normalised."""
    q = NC.batch(K)
    rows, le = NC.reference(K, W, g, table)
    tab = FM.DEFAULT if table else None
    j_rows, j_le = FN.decode(q, K, *NC.interleaver(K), 4, W, g, tab, *NC.setting(table), jitter=K + g)
    assert np.array_equal(j_rows, rows[:, :4]) and np.array_equal(j_le, le[:, :4])


def test_nii_differs_from_nii_off_at_K1024():
    """K = 1024 (31, 64), 0.5 dB, seed 5, {64, 16}, 8 iterations: NII on is not the NII-off decode on these
    frames, in rows and in Le, so a kernel that ignored the flag could not pass a test against the restatement."""
    K, f1, f2 = 1024, 31, 64
    q = F.quantise(O.synth_batch(K, f1, f2, 0.5, 5, 8)[1], 8)
    rows, le = FN.decode(q, K, f1, f2, 8, 64, 16)
    w_rows, w_le = FW.decode(q, K, f1, f2, 8, 64, 16)
    print(f"{{64, 16}}: {int((w_rows != rows).sum())} row bits, {int((w_le != le).sum())} Le values differ")
    assert np.array_equal(rows[:, 0], w_rows[:, 0]) and np.array_equal(le[:, 0], w_le[:, 0])
    assert (w_rows[:, 1:] != rows[:, 1:]).any() and (w_le[:, 1:] != le[:, 1:]).any()
    # and on the shared batch of the lane-code and GPU tests
    rows, le = NC.reference(1024, 64, 16, False)
    w_rows, w_le = FW.decode(NC.batch(1024), K, f1, f2, 8, 64, 16)
    assert (w_rows != rows).any() and (w_le != le).any()


# ------------------------------------------------------------------ the kernel's lane code on the host
def _run_core(exe, tmp_path, q, K, f1, f2, iters, all_iters, le_max, scale, W, g, tab):
    return run_core(exe, tmp_path, q, O.qpp(K, f1, f2), iters, all_iters, (le_max, scale), (W, g), tab=tab, nii=True)[:2]


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("K,W,g", NC.GEOMETRIES)
def test_lane_code_on_the_host_equals_restatement(core_host, tmp_path, K, W, g, table):
    """Every geometry of fixed_window_nii_cases at 1, 2, 3 and 8 iterations (the state's two parities, and the
    last iteration, which stores nothing), frames next to the saturated and alternating patterns, plain
    max and the default table; every row and every Le, then the last row alone.  SISO1's sub-blocks run
    last to first and SISO2's first to last; ASan watches the bounds of the workspace and of the state."""
    q = NC.batch(K)
    rows, le = NC.reference(K, W, g, table)
    tab = FM.DEFAULT if table else None
    for iters in (1, 2, 3, 8):
        args = (q, K, *NC.interleaver(K), iters)
        g_rows, g_le = _run_core(core_host, tmp_path, *args, True, *NC.setting(table), W, g, tab)
        assert np.array_equal(g_rows, rows[:, :iters]) and np.array_equal(g_le, le[:, :iters]), iters
        g_last, g_le = _run_core(core_host, tmp_path, *args, False, *NC.setting(table), W, g, tab)
        assert np.array_equal(g_last[:, 0], rows[:, iters - 1]) and np.array_equal(g_le, le[:, :iters]), iters
