"""Shared by test_fixed_window_nii_host.py (CPU) and test_gpu_fixed_window_nii.py: the geometries of
td_set_fixed_window_nii's tests, one batch for each and its reference (tests/fixed_window_nii_ref.py), computed once
per case and read-only.  A codeword's result does not depend on its batch and an iteration's not on the
ones after it, so a test takes the codewords and the iterations it needs from the one reference.

  K = 40    L = 43 at W = 16: two sub-blocks, the last 27 long.  Overlap 0 (own end stored), 16, and 48 >= L
            (every warm-up reaches a trellis end: the exact decode)
  K = 62, 63  L = 65, 66 at {16, 16}: a beta vector taken at L - 1 and L - 2, where states are unreachable
  K = 61    L = 64: that b_from is L itself, terminated
  K = 1024  {64, 16}; {64, 64}: the overlap a multiple of W, the last sub-block stores two beta vectors;
            {32, 0}; {128, 384}: an overlap of three sub-blocks
"""
import functools

import numpy as np

import fixed_maxstar_ref as FM
import fixed_ref as F
import fixed_size_cases as Z
import fixed_window_nii_ref as FN
import pyoracle as O

GEOMETRIES = [(40, 16, 0), (40, 16, 16), (40, 16, 48), (62, 16, 16), (63, 16, 16), (61, 16, 16),
              (1024, 64, 16), (1024, 64, 64), (1024, 32, 0), (1024, 128, 384)]
ITERS = 8
TABLE_SETTING = (255, 4)   # log-MAP wants no extrinsic scale
PLAIN_SETTING = (255, 3)


def interleaver(K):
    return {40: (3, 10), 1024: (31, 64), 6144: (263, 480)}.get(K) or Z.interleaver(K)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def batch(K):
    """Eight codewords: a frame, +127, -128, alternating +-127, two more frames (AWGN at 0.5 dB, 8 steps
    per unit) and two rows of random bytes.  The first five hold the three patterns."""
    n = 3 * K + 12
    fr = F.quantise(O.synth_batch(K, *interleaver(K), 0.5, 5, 3)[1], 8)
    q = np.concatenate([fr[:1], np.full((1, n), 127, dtype=np.int8), np.full((1, n), -128, dtype=np.int8),
                        (127 * (1 - 2 * (np.arange(n) & 1))).astype(np.int8)[None, :], fr[1:],
                        np.random.default_rng(K).integers(-128, 128, (2, n)).astype(np.int8)])
    return _frozen(q)[0]


def setting(table):
    return TABLE_SETTING if table else PLAIN_SETTING


@functools.lru_cache(maxsize=None)
def reference(K, W, g, table, iters=ITERS):
    """(rows [8, iters, K], Le [8, iters, 2, K+3]) of batch(K) under {W, g} with NII: the plain max, or the
    default table (fixed_maxstar_ref.DEFAULT) with set_fixed(255, 4)."""
    return _frozen(*FN.decode(batch(K), K, *interleaver(K), iters, W, g, FM.DEFAULT if table else None,
                              *setting(table)))


STOP_K, STOP_WIN, STOP_B = 1024, (64, 16), 130


@functools.lru_cache(maxsize=None)
def stop_reference(key, table=False, win=STOP_WIN):
    """(q, rows [130, 8, K], Le) of fixed_stop_cases' frames key = ("awgn", ebn0) or ("crc", sigma) at K = 1024
    under `win` with NII and the rule off: what td_set_fixed_window_stop's rules judge."""
    import fixed_stop_cases as S
    q = np.ascontiguousarray(S.FRAMES[key[0]](STOP_K, key[1], STOP_B))
    rows, le = FN.decode(q, STOP_K, *interleaver(STOP_K), ITERS, *win, FM.DEFAULT if table else None, *setting(table))
    return _frozen(q, rows, le)


@functools.lru_cache(maxsize=None)
def stop_used(key, rule, table=False, min_iters=1):
    import window_stop_cases as W
    u = W.stops(stop_reference(key, table)[1], rule, min_iters, W.CRC24B)
    u.setflags(write=False)
    return u
