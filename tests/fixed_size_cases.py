"""Shared by the fixed-point decoder's host-program tests (CPU) and test_gpu_fixed_sizes.py /
test_gpu_fixed_random_sizes.py: block lengths at every residue of L = K + 3 modulo the 16-step
recomputation window of csrc/td_fixed_core.h and at the edges of the 64 x 64 byte transposes round it,
an interleaver and a batch for each, and their references -- fixed_ref / fixed_window_ref, computed
once per case and read-only.

  8 .. 12     L < 16: one partial window
  13 .. 28    L = 16 .. 31: every residue of L mod 16, one or two windows
  109 .. 124  L = 112 .. 127: every residue again with 7 or 8 windows; 3 * 124 + 12 = 6 * 64
  60, 61      3 * 60 + 12 = 3 * 64 with L = 63; L = 64
  64, 65      K mod 64 = 0 and 1
  188         L = 191: at W = 64 two sub-blocks, the last 127 long (the longest the contract allows)
  189, 191    L = 192 = 3 * 64: no remainder; L = 194
"""
import functools

import numpy as np

import fixed_ref as F
import fixed_window_ref as FW
import pyoracle as O
import window_stop_cases as W

SIZES = sorted([*range(8, 29), *range(109, 125), 60, 61, 64, 65, 188, 189, 191])
SETTINGS = [(255, 3), (255, 4), (127, 3), (31, 2)]          # (le_max, ext_scale_q)
WINDOWS = [(16, 0), (16, 5), (32, 7), (64, 48)]             # (window, overlap)
STEPS = 8                                                   # steps per unit LLR
CRC24B = W.CRC24B


def setting(K):
    """The size's extrinsic setting: the four rotate through SIZES."""
    return SETTINGS[SIZES.index(K) % len(SETTINGS)]


def is_permutation(K, f1, f2):
    return np.array_equal(np.sort(O.qpp(K, f1, f2)), np.arange(K))


@functools.lru_cache(maxsize=None)
def interleaver(K):
    """The first (f1, f2), scanning f2 = 1, 2, ..., K-1, 0 and within it f1 = 2, 3, ..., K-1, whose QPP
    is a permutation and not the identity (the identity would hide a swapped pi / pinv).  An odd
    square-free K (the primes among them) only has linear ones: (2, 0)."""
    i = np.arange(K, dtype=np.int64)
    f1 = np.arange(2, K, dtype=np.int64)
    odd = [p for p in range(3, K + 1, 2) if K % p == 0 and all(p % d for d in range(3, p, 2))]
    for f2 in (*range(1, K), 0):
        if any(f2 % p for p in odd):
            continue   # modulo an odd prime factor of K the polynomial is a quadratic: no permutation
        pi = (f1[:, None] * i[None, :] + f2 * i[None, :] * i[None, :]) % K
        ok = (np.sort(pi, axis=1) == i[None, :]).all(axis=1) & (pi != i[None, :]).any(axis=1)
        if ok.any():
            got = int(f1[int(np.argmax(ok))]), f2
            assert np.array_equal(O.qpp(K, *got), pi[int(np.argmax(ok))]), "the oracle's QPP is this polynomial"
            return got
    raise ValueError(f"K = {K} has no interleaver but the identity")


def patterns(q, seed):
    """Rows B-1, B-3, B-5 and B-7 of q replaced by -128, random bytes, +127 and alternating +-127 (fewer
    in a batch of fewer than eight): demultiplexing clamps -128 to -127 at every tile edge, and the lane
    after a full wave of 64 in a batch of 65 is the -128 row.  Every second row stays a frame, so a
    batch's last wave holds frames too."""
    q = np.array(q, dtype=np.int8)
    B, n = q.shape
    # a whole row of -128 drives every Le to the clamp, with or without the -128 -> -127 step; in the
    # row of random bytes a -128 decides Le values, so that row has one at both ends of every 64-byte
    # tile, at the stream's last byte and at one position in eight besides
    rng = np.random.default_rng(seed)
    noise = rng.integers(-128, 128, n)
    at = np.arange(n) % 64
    noise[(at == 0) | (at == 63) | (np.arange(n) == n - 1) | (rng.random(n) < 0.125)] = -128
    rows = [np.full(n, -128), noise, np.full(n, 127), 127 * (1 - 2 * (np.arange(n) & 1))]
    for j, row in enumerate(rows[:min(4, B // 2)]):
        q[B - 1 - 2 * j] = row.astype(np.int8)
    return q


def awgn(K, f1, f2, B, ebn0, seed=4242):
    """B generator frames at ebn0 dB, quantised at 8 steps per unit, with the pattern rows."""
    return patterns(F.quantise(O.synth_batch(K, f1, f2, ebn0, seed, B)[1], STEPS), K + B)


def crc(K, f1, f2, B, sigma=1.1):
    """B frames carrying gCRC24B (window_stop_cases.crc_frames), quantised alike, with the pattern rows."""
    return patterns(F.quantise(W.crc_frames(K, f1, f2, CRC24B, sigma, B), STEPS), K + B)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def batch(K, B=65, ebn0=0.5):
    return _frozen(awgn(K, *interleaver(K), B, ebn0))[0]


@functools.lru_cache(maxsize=None)
def exact(K, B=65, iters=3):
    """(rows [B, iters, K], Le [B, iters, 2, K+3]) of batch(K, B) under the exact schedule."""
    rows, le, _ = F.decode(batch(K, B), K, *interleaver(K), iters, *setting(K))
    return _frozen(rows, le)


@functools.lru_cache(maxsize=None)
def windowed(K, win, B=65, iters=3):
    return _frozen(*FW.decode(batch(K, B), K, *interleaver(K), iters, *win, *setting(K)))


def window_is_exact_by_contract(K, win):
    """One sub-block, or an overlap that reaches both ends of the trellis from every sub-block."""
    L, (w, g) = K + 3, win
    return max(1, L // w) == 1 or g >= L


STOP_B, STOP_ITERS = 130, 6


@functools.lru_cache(maxsize=None)
def stop_case(K, rule):
    """(q, rows, Le, counts) of the size's early-termination batch: 130 codewords, 6 iterations,
    min_iters 1; `rule` "hda" on generator frames at 0.0 dB, "crc" (K > 24) on gCRC24B frames at sigma 1.1.
    The last wave holds two codewords, a frame and the -128 row, which stops at once.  A codeword's
    reference does not depend on its place in the batch, so the frame of the first wave that runs
    longest changes places with that frame: the two lanes of the last wave stop apart as well."""
    f1, f2 = interleaver(K)
    q = awgn(K, f1, f2, STOP_B, 0.0) if rule == "hda" else crc(K, f1, f2, STOP_B, 1.1)
    rows, le, _ = F.decode(q, K, f1, f2, STOP_ITERS, *setting(K))
    used = W.stops(rows, rule, 1, CRC24B)
    order = np.arange(STOP_B)
    longest = int(np.argmax(used[:64]))
    order[[longest, STOP_B - 2]] = STOP_B - 2, longest
    return _frozen(*(np.ascontiguousarray(a[order]) for a in (q, rows, le, used)))


def spread_in_every_wave(used, iters):
    """Lanes of one wave of 64 stop at different iterations: at least two distinct counts in each wave,
    one of them below `iters`."""
    for w0 in range(0, len(used), 64):
        sp = W.spread(used[w0:w0 + 64])
        assert len(sp) >= 2 and min(sp) < iters, (w0, sp)
