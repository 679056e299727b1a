"""The cases of fixed_size_cases.py without a GPU: that the sizes reach every residue and tile edge they
are meant to, that their interleavers are permutations and not the identity, and that the windowed
restatement the GPU tests compare against is not the exact decode wherever the contract lets it differ."""
import numpy as np
import pytest

import fixed_size_cases as Z
import pyoracle as O


def test_sizes_reach_every_residue_and_tile_edge():
    S = set(Z.SIZES)
    assert len(Z.SIZES) == len(S) and min(S) == 8
    assert {K + 3 for K in S if K + 3 < 16} == set(range(11, 16)), "one partial window"
    for lo in (16, 112):   # one or two windows; seven or eight
        assert {(K + 3) % 16 for K in S if lo <= K + 3 < lo + 16} == set(range(16)), lo
    assert {K for K in S if (3 * K + 12) % 64 == 0} >= {60, 124}
    assert {K for K in S if (K + 3) % 64 == 0} >= {61, 189}
    assert any(K % 64 == 0 for K in S) and any(K % 64 == 1 for K in S)
    L = 188 + 3   # at W = 64 two sub-blocks, the last as long as the contract allows
    assert 188 in S and L // 64 == 2 and L - 64 == 2 * 64 - 1
    assert {Z.setting(K) for K in S} == set(Z.SETTINGS)


@pytest.mark.parametrize("K", Z.SIZES)
def test_interleaver_is_a_permutation_and_not_the_identity(K):
    f1, f2 = Z.interleaver(K)
    pi = O.qpp(K, f1, f2)
    assert 2 <= f1 < K and 0 <= f2 < K
    assert np.array_equal(np.sort(pi), np.arange(K)) and not np.array_equal(pi, np.arange(K))


@pytest.mark.parametrize("K", Z.SIZES)
def test_windowed_restatement_differs_from_exact_where_it_may(K):
    """One sub-block, or an overlap that covers the trellis: the exact decode by contract.  Otherwise
    -- {16, 0} and {16, 5} at every K >= 29 among them -- rows or Le differ on the size's batch, so a
    kernel that ignored the window could not pass test_gpu_fixed_sizes.py."""
    rows, le = Z.exact(K)
    for win in Z.WINDOWS:
        w_rows, w_le = Z.windowed(K, win)
        same = np.array_equal(w_rows, rows) and np.array_equal(w_le, le)
        if Z.window_is_exact_by_contract(K, win):
            assert same, win
        else:
            assert not same, win
    if K >= 29:
        assert not Z.window_is_exact_by_contract(K, (16, 0)) and not Z.window_is_exact_by_contract(K, (16, 5))
