"""The scrambling sequence of 3GPP TS 36.211 7.2 restated in numpy from its definition, for the tests, with the
two ways the library applies it (td_scramble, td_descramble_llr).

    x1(n+31) = (x1(n+3) + x1(n)) mod 2,                           x1(0) = 1, x1(1..30) = 0
    x2(n+31) = (x2(n+3) + x2(n+2) + x2(n+1) + x2(n)) mod 2,       c_init = sum x2(i) 2^i
    c(n)     = (x1(n+1600) + x2(n+1600)) mod 2

Nothing here is computed the way the library does it: the registers are arrays of bits filled from position 0
onwards, 28 positions a numpy step (both recurrences reach back 28 positions at least), and there is no jump.
"""
import numpy as np

NC = 1600
RUN = 1024   # td_gold_core.h's kGoldRun: the lengths around it are the tests' edge cases
STEP = 28

# the issue's spot values: c_init -> {word: value}; word w is bits 32w .. 32w+31, bit n at position n & 31
SPOT = {0x00000000: {0: 0x5e485840, 1: 0x6ac0a9a4, 3125: 0xa91c06b3, 6249: 0x8228f53e},
        0x00000001: {0: 0x2ec0c140, 1: 0x47bf59d4, 3125: 0x84a6f115, 6249: 0x77638445},
        0x7fffffff: {0: 0x71cfd0bf, 1: 0x71ea0674, 3125: 0x4d8a542e, 6249: 0xd111da17},
        0x12345678: {0: 0x9e7b874b, 1: 0x0ed0f7f2, 3125: 0x8c3e5fc6, 6249: 0xe04a2e88},
        0x048d2f2d: {0: 0x9e510d58, 1: 0xaec8e99c, 3125: 0xe7ed715c, 6249: 0x7dd63876}}


def edge_lengths(top=True):
    """1, 31, 32, 33, run-1, run, run+1, 3 run + 17, and (top) 2^22 + 5"""
    return [1, 31, 32, 33, RUN - 1, RUN, RUN + 1, 3 * RUN + 17] + ([(1 << 22) + 5] if top else [])


def _fill(x, taps):
    """x [rows, total] with positions 0 .. 30 set: the others by the recurrence x(n+31) = sum of x(n+t), t in taps"""
    total = x.shape[1]
    for n in range(0, total - 31, STEP):
        m = min(STEP, total - 31 - n)
        acc = x[:, n:n + m].copy()
        for t in taps:
            if t:
                acc ^= x[:, n + t:n + t + m]
        x[:, n + 31:n + 31 + m] = acc
    return x


def bits(cinit, length):
    """c(0 .. length-1) for every c_init of the array: uint8 [N, length]; bit 31 of a c_init is not part of it"""
    cinit = np.atleast_1d(np.asarray(cinit)).astype(np.uint64) & np.uint64(0x7FFFFFFF)
    total = max(NC + int(length), 31)
    x1 = np.zeros((1, total), dtype=np.uint8)
    x1[0, 0] = 1
    x2 = np.zeros((len(cinit), total), dtype=np.uint8)
    x2[:, :31] = (cinit[:, None] >> np.arange(31, dtype=np.uint64)) & np.uint64(1)
    _fill(x1, (0, 3))
    _fill(x2, (0, 1, 2, 3))
    return (x1[:, NC:NC + length] ^ x2[:, NC:NC + length]).astype(np.uint8)


def pack(b):
    """bits uint8 [N, len] -> words uint32 [N, (len + 31) // 32], bit g at position g & 31 of word g >> 5, tail zero"""
    n, length = b.shape
    W = (length + 31) // 32
    padded = np.zeros((n, W * 32), dtype=np.uint32)
    padded[:, :length] = b
    return (padded.reshape(n, W, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)


def words(cinit, length):
    """td_gold_sequence: uint32 [N, W]"""
    return pack(bits(cinit, length))


def unpack(seq, length):
    """words [N, W] -> bits uint8 [N, length]"""
    seq = np.asarray(seq).view(np.uint32) if np.asarray(seq).dtype == np.int32 else np.asarray(seq, dtype=np.uint32)
    b = (seq[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(seq.shape[0], -1)[:, :length].astype(np.uint8)


def scramble(x, c):
    """td_scramble: bytes [N, len], any non-zero byte a 1, and the sequence's bits c [N, len] -> uint8 0 / 1"""
    return ((np.asarray(x) != 0).astype(np.uint8) ^ c).astype(np.uint8)


def descramble(v, c):
    """td_descramble_llr: float64 / float32: the sign bit flipped where c = 1; int8: -128 read as -127, then
    negated, where c = 1; copied elsewhere"""
    v = np.ascontiguousarray(v)
    if v.dtype == np.int8:
        return np.where(c != 0, -np.maximum(v.astype(np.int32), -127), v.astype(np.int32)).astype(np.int8)
    u = {8: np.uint64, 4: np.uint32}[v.dtype.itemsize]
    sign = u(1) << u(8 * v.dtype.itemsize - 1)
    return (v.view(u) ^ (c.astype(u) * sign)).view(v.dtype)
