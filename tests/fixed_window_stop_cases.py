"""Shared by test_fixed_window_stop_host.py (CPU) and test_gpu_fixed_window_stop.py: the cases of
td_set_fixed_window_stop's tests and their references.  The rule is post-processing of the rows of the
full windowed fixed decode (fixed_window_ref.decode) with window_stop_cases' numpy rules, on
fixed_stop_cases' frames; every reference is computed once per case and read-only."""
import functools

import numpy as np

import fixed_size_cases as Z
import fixed_stop_cases as S
import fixed_window_ref as FW
import window_stop_cases as W

CRC24A, CRC24B = S.CRC24A, S.CRC24B
QPP = S.QPP
ITERS = W.ITERS
B = 130

# K, frames' key, (window, overlap), rule: the counts of each were checked on the CPU (the GPU test pins some)
CASES = [
    (40, ("awgn", 1.0, B), (16, 5), "hda"),
    (40, ("crc", 1.1, B), (16, 5), "crc"),
    (200, ("awgn", 1.0, B), (32, 7), "hda"),
    (200, ("crc", 1.15, B), (32, 7), "crc"),
    (200, ("awgn", 1.0, B), (16, 0), "hda"),
    (1024, ("awgn", 1.0, B), (64, 48), "hda"),
    (1024, ("awgn", 0.5, B), (64, 16), "hda"),
    (1024, ("crc", 1.15, B), (64, 48), "crc"),
]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(key, K, iters, win, setting=(255, 3)):
    """(q, rows [B, iters, K], Le [B, iters, 2, K+3]) of the frames S.FRAMES[key[0]](K, *key[1:]) under the
    sub-block schedule `win` with the rule off."""
    q = np.ascontiguousarray(S.FRAMES[key[0]](K, *key[1:]))
    rows, le = FW.decode(q, K, *QPP[K], iters, *win, *setting)
    return _frozen(q, rows, le)


@functools.lru_cache(maxsize=None)
def used(key, K, iters, win, rule, min_iters=1, poly=CRC24B, setting=(255, 3)):
    u = W.stops(reference(key, K, iters, win, setting)[1], rule, min_iters, poly)
    u.setflags(write=False)
    return u


def not_for_nothing(key, K, iters, win, rule, setting=(255, 3)):
    """What keeps a case from passing for nothing, asserted on the restatements: at least 3 distinct
    counts, one below `iters`; at least 2 in every full wave of 64; windowed rows that are not the exact
    fixed decode's, and counts that are not the exact fixed rule's (a kernel that judged the exact
    schedule's rows fails).  -> the counts' spread."""
    u = used(key, K, iters, win, rule, setting=setting)
    sp = W.spread(u)
    assert len(sp) >= 3 and min(sp) < iters, sp
    for w0 in range(0, len(u) - 63, 64):
        assert len(W.spread(u[w0:w0 + 64])) >= 2, (w0, W.spread(u[w0:w0 + 64]))
    rows = reference(key, K, iters, win, setting)[1]
    exact_rows = S.reference(key, K, iters, setting)[1]
    d_rows = int((rows != exact_rows).any(axis=(1, 2)).sum())
    d_used = int((u != S.used(key, K, iters, setting, rule)).sum())
    print(f"K={K} {key} {win} {rule}: {sp}; rows differ from the exact decode's in {d_rows} codewords, "
          f"counts in {d_used}")
    assert d_rows >= 1 and d_used >= 1
    return sp


@functools.lru_cache(maxsize=None)
def whole_wave_case(K=1024, win=(64, 48)):
    """(q, rows, Le) of 130 codewords: 0..63 are copies of the earliest-stopping frame (HDA) of the
    1.0 dB case, a wave that may leave early; the rest are the 0.5 dB frames.  A codeword's reference
    does not depend on its batch, so the references are those cases' own."""
    one = reference(("awgn", 1.0, B), K, ITERS, win)
    half = reference(("awgn", 0.5, B), K, ITERS, win)
    first = int(np.argmin(W.stops(one[1], "hda")))
    return _frozen(*(np.concatenate([np.repeat(a[first:first + 1], 64, axis=0), b[:66]]) for a, b in zip(one, half)))


# one size per residue of L mod 16 (K > 24, so both rules), and L = 191: at W = 64 the longest last sub-block
RESIDUE_SIZES = [*range(109, 125), 188]
SIZE_B, SIZE_ITERS = 65, 6


@functools.lru_cache(maxsize=None)
def size_case(K, rule, win):
    """(q, rows, Le, counts) of the size's batch (fixed_size_cases' interleaver, setting and frames: "hda" on
    generator frames at 0.0 dB, "crc" on gCRC24B frames at sigma 1.1, the pattern rows among them): 65
    codewords, 6 iterations, min_iters 1."""
    f1, f2 = Z.interleaver(K)
    q = Z.awgn(K, f1, f2, SIZE_B, 0.0) if rule == "hda" else Z.crc(K, f1, f2, SIZE_B, 1.1)
    rows, le = FW.decode(q, K, f1, f2, SIZE_ITERS, *win, *Z.setting(K))
    return _frozen(np.ascontiguousarray(q), rows, le, W.stops(rows, rule, 1, CRC24B))


@functools.lru_cache(maxsize=None)
def host_case(K, iters, win, setting):
    """(q, rows, Le) of fixed_stop_cases' host batch (AWGN and gCRC24B frames at 16 steps per unit, zeros,
    +127, -128, random bytes) under the sub-block schedule, with the size's own interleaver."""
    q = np.ascontiguousarray(S.FRAMES["host"](K))
    rows, le = FW.decode(q, K, *QPP[K], iters, *win, *setting)
    return _frozen(q, rows, le)


le_mask = S.le_mask
