"""Shared by the encoder's host-program test (CPU) and test_gpu_encode.py: block lengths, an interleaver
and the row patterns for each, and their reference -- pyoracle.encode, computed once per size and read-only.

Sizes: the list of the encoder's issue (1, 2, 3, 6, 7, 8, 40, 63 .. 65, 127 .. 129, 4095 .. 4097, 6144,
10000) and the edges of the design in csrc/td_encode_core.h:
  5, 9          K mod 4 = 1: the last group of four info bits is partial and the tail follows it unaligned
  1024          the third LTE pair
  4096, 4097    64 and 65 words: the carry scan crosses from the first wave to the second
  8192, 8193    128 and 129 words: into the third wave
Every K up to 65 with B > 1 also puts rows at every alignment modulo 16 (3K + 12 is odd for odd K).
"""
import functools

import numpy as np

import fixed_size_cases as Z
import pyoracle as O

SIZES = [1, 2, 3, 5, 6, 7, 8, 9, 40, 63, 64, 65, 127, 128, 129, 1024, 4095, 4096, 4097, 6144, 8192, 8193, 10000]
LTE = {40: (3, 10), 1024: (31, 64), 6144: (263, 480)}
# fixed_size_cases.interleaver scans a (K-2) x K table per f2, which is gigabytes at these lengths.  These
# are chosen by the rule it finds its pairs with: f1 coprime to K, every prime factor of K in f2 (an odd
# square-free K only has linear ones); interleaver() checks each is a permutation other than the identity.
LARGE = {4095: (2, 0), 4096: (31, 64), 4097: (2, 0), 8192: (31, 64), 8193: (2, 0), 10000: (3, 10)}


@functools.lru_cache(maxsize=None)
def interleaver(K):
    if K in LTE:
        got = LTE[K]
    elif K <= 3:
        return 1, 0   # the identity
    elif K in LARGE:
        got = LARGE[K]
    else:
        try:
            got = Z.interleaver(K)
        except ValueError:
            return 1, 0
    pi = O.qpp(K, *got)
    assert np.array_equal(np.sort(pi), np.arange(K)) and not np.array_equal(pi, np.arange(K)), (K, got)
    return got


@functools.lru_cache(maxsize=None)
def rows(K):
    """The patterns as bytes [R, K]: all zero, all one, a single 1 at each of 0, 1, 2, K-3, K-2, K-1, 16
    random rows, and a random row whose ones are the bytes 0x02, 0x80 and 0xFF (any non-zero byte is a 1)."""
    rng = np.random.default_rng(1000 + K)
    out = [np.zeros(K, np.uint8), np.ones(K, np.uint8)]
    for p in sorted({p for p in (0, 1, 2, K - 3, K - 2, K - 1) if 0 <= p < K}):
        r = np.zeros(K, np.uint8)
        r[p] = 1
        out.append(r)
    out += list(rng.integers(0, 2, (16, K), dtype=np.uint8))
    odd = rng.integers(0, 2, K, dtype=np.uint8) * rng.choice(np.array([0x02, 0x80, 0xFF], np.uint8), K)
    odd[:min(K, 3)] = np.array([0x02, 0x80, 0xFF], np.uint8)[:min(K, 3)]   # each of the three at least once (K >= 3)
    out.append(odd.astype(np.uint8))
    a = np.stack(out)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def coded(K):
    """pyoracle.encode of every row of rows(K): uint8 [R, 3K+12]."""
    f1, f2 = interleaver(K)
    a = np.stack([O.encode((r != 0).astype(np.int32), f1, f2) for r in rows(K)]).astype(np.uint8)
    a.setflags(write=False)
    return a


def batch(K, B, start=0):
    """(info [B, K], coded [B, 3K+12]): the patterns from row `start` on, repeated round to fill B."""
    idx = (start + np.arange(B)) % rows(K).shape[0]
    return np.ascontiguousarray(rows(K)[idx]), np.ascontiguousarray(coded(K)[idx])
