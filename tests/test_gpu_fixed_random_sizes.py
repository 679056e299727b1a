"""Seeded random block sizes through the fixed-point decoder (TD_FIXED) against its numpy restatements:
the sibling of test_gpu_random_sizes.py, beside the fixed sizes of test_gpu_fixed*.py.

The ABI takes any 8 <= K <= 10000 whose (f1, f2) gives a QPP permutation.  Each of the 24 cases draws K
(multiples of 8 up to 2048 and arbitrary K in [8, 2048], alternately within each schedule), a valid
(f1, f2) that is not the identity, a batch of 1 to 150 codewords, an Eb/N0 in [-0.5, 1.0], one of the
four extrinsic settings and a window from one seeded generator; the schedule cycles with the case
index through
  * the exact schedule, 3 iterations: rows of every iteration, every Le, the final bits (fixed_ref);
  * the sub-block schedule, W from {16, 32, 48, 64, 96} and an overlap in [0, 3W] (fixed_window_ref);
  * early termination by HDA, 5 iterations: counts, frozen rows, Le up to the stop, the stop row;
  * the same by CRC with gCRC24B on frames that carry it (HDA where K <= 24).
The batches are fixed_size_cases': frames at 8 steps per unit with the saturated and random rows.  K stops
at 2048 for the restatement's sake; 6144 and 10000 are test_gpu_fixed*.py's.  The draws are fixed by the
seed, so a failure names a reproducible case."""
import functools

import numpy as np
import pytest

import fixed_ref as F
import fixed_size_cases as Z
import fixed_window_ref as FW
import pyoracle as O
import window_stop_cases as W
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SCHEDULES = ("exact", "window", "hda", "crc")
SENTINEL = 12345


def _valid(K, f1, f2):
    return Z.is_permutation(K, f1, f2) and not np.array_equal(O.qpp(K, f1, f2), np.arange(K))


def _draw(rng, n):
    cases = []
    while len(cases) < n:
        i = len(cases)
        K = int(rng.integers(1, 257)) * 8 if (i + i // 4) % 2 == 0 else int(rng.integers(8, 2049))
        for _ in range(200):   # a random valid pair ...
            f1, f2 = int(rng.integers(1, K)), int(rng.integers(0, K))
            if _valid(K, f1, f2):
                break
        else:                  # ... or a linear one: an odd square-free K has no other
            f1, f2 = next(f for f in (int(v) for v in rng.permutation(np.arange(2, K))) if np.gcd(f, K) == 1), 0
            assert _valid(K, f1, f2)
        B = int(rng.integers(1, 151))
        ebn0 = float(np.round(rng.uniform(-0.5, 1.0), 2))
        setting = Z.SETTINGS[int(rng.integers(0, len(Z.SETTINGS)))]
        win = int(rng.choice([16, 32, 48, 64, 96]))
        overlap = int(rng.integers(0, 3 * win + 1))
        schedule = SCHEDULES[i % 4]
        if schedule == "crc" and K <= 24:
            schedule = "hda"
        cases.append((schedule, K, f1, f2, B, ebn0, setting, (win, overlap)))
    return cases


CASES = _draw(np.random.default_rng(20261020), 24)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(q, rows, Le, counts or None) of a case, from the restatements."""
    schedule, K, f1, f2, B, ebn0, setting, win = CASES[case]
    if schedule == "crc":   # Es/N0 of the rate 1/3 code -> the noise of window_stop_cases.crc_frames
        q = Z.crc(K, f1, f2, B, float(np.sqrt(1.5 / 10 ** (ebn0 / 10))))
    else:
        q = Z.awgn(K, f1, f2, B, ebn0, seed=9000 + case)
    if schedule == "window":
        rows, le = FW.decode(q, K, f1, f2, 3, *win, *setting)
        return q, rows, le, None
    rows, le, _ = F.decode(q, K, f1, f2, 3 if schedule == "exact" else 5, *setting)
    return q, rows, le, None if schedule == "exact" else W.stops(rows, schedule, 1, Z.CRC24B)


def _decode(c, q, all_iters, counts):
    import torch
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(q).to(dev)
    le = torch.full((q.shape[0], c.iterations, 2, c.K + 3), SENTINEL, dtype=torch.int16, device=dev)
    out = c.decode(x, all_iters=all_iters, le=le, iters_out=True if counts else None)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), q), "d_llr is not modified"
    out, n = out if counts else (out, None)
    return out.cpu().numpy(), le.cpu().numpy(), n.cpu().numpy() if counts else None


@pytest.mark.parametrize("case", range(len(CASES)))
def test_random_size_fixed_vs_restatement(case):
    from turbo_decoder_cuda_amd import TurboCodec
    schedule, K, f1, f2, B, ebn0, setting, win = CASES[case]
    q, rows, le, used = reference(case)
    iters = rows.shape[1]
    with TurboCodec(K, f1, f2, iterations=iters, algo="maxlog", precision="fixed") as c:
        c.set_fixed(*setting)
        if schedule == "window":
            c.set_fixed_window(*win)
        if used is not None:
            c.set_fixed_early_stop(schedule, min_iters=1, crc_poly=Z.CRC24B)
        g_rows, g_le, g_used = _decode(c, q, True, used is not None)
        g_bits, _, g_used1 = _decode(c, q, False, used is not None)
    if used is None:
        assert np.array_equal(g_rows, rows), CASES[case]
        assert np.array_equal(g_le, le), CASES[case]
        assert np.array_equal(g_bits, rows[:, -1]), CASES[case]
        return
    print(W.spread(used))
    assert np.array_equal(g_used, used) and np.array_equal(g_used1, used), (CASES[case], W.spread(g_used), W.spread(used))
    assert np.array_equal(g_rows, W.frozen(rows, used)), CASES[case]
    mask = np.broadcast_to((np.arange(iters)[None, :] < used[:, None])[:, :, None, None], le.shape)
    assert np.array_equal(g_le[mask], le[mask]), CASES[case]
    assert (g_le[~mask] == SENTINEL).all(), (CASES[case], "a stopped codeword writes no Le")
    assert np.array_equal(g_bits, rows[np.arange(B), used - 1]), CASES[case]
