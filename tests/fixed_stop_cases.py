"""Shared by test_fixed_stop_host.py (CPU) and test_gpu_fixed_stop.py: the cases of td_set_fixed_stop's
tests and their references.  The rule is post-processing of the rows of the full fixed decode
(fixed_ref.decode) with window_stop_cases' numpy rules; every reference is computed once per case and
read-only."""
import functools

import numpy as np

import fixed_ref as F
import fixed_size_cases
import llr_families
import pyoracle as O
import window_stop_cases as W
from conftest import GOLD

CRC24A, CRC24B = W.CRC24A, W.CRC24B
STEPS = 8   # steps per unit LLR of the GPU cases

QPP = {8: (3, 4), 13: (1, 0), 16: (1, 4), 29: (1, 0), 40: (3, 10), 200: (13, 50), 1024: (31, 64), 6144: (263, 480)}
_z = np.load(f"{GOLD}/frames_K10000_e0.8_s43.npz")
QPP[int(_z["K"])] = (int(_z["f1"]), int(_z["f2"]))
for _K in fixed_size_cases.SIZES:   # every residue of L mod 16, non-identity interleavers
    QPP.setdefault(_K, fixed_size_cases.interleaver(_K))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(key, K, iters, setting):
    """(q, rows [B, iters, K], Le [B, iters, 2, K+3]) of the frames FRAMES[key[0]](K, *key[1:])."""
    q = np.ascontiguousarray(FRAMES[key[0]](K, *key[1:]))
    rows, le, _ = F.decode(q, K, *QPP[K], iters, *setting)
    return _frozen(q, rows, le)


def _awgn(K, ebn0, B, steps=STEPS, seed=4242):
    return F.quantise(O.synth_batch(K, *QPP[K], ebn0, seed, B)[1], steps)


def _crc(K, sigma, B, steps=STEPS):
    return F.quantise(W.crc_frames(K, *QPP[K], CRC24B, sigma, B), steps)


def _pattern(K, name, B):
    """test_gpu_fixed.py's saturated and all-zero batches."""
    n = 3 * K + 12
    if name == "plus127":
        return np.full((B, n), 127, dtype=np.int8)
    if name == "minus128":
        return np.full((B, n), -128, dtype=np.int8)
    if name == "alternating":
        return np.tile((127 * (1 - 2 * (np.arange(n) & 1))).astype(np.int8), (B, 1))
    if name == "mixed":
        rng = np.random.default_rng(K + B)
        q = rng.integers(-128, 128, (B, n)).astype(np.int8)
        q[0::4] = 127
        q[1::4] = -128
        q[2::4] = _pattern(K, "alternating", B)[2::4]
        return q
    flow = O.synth_batch(K, *QPP[K], 0.5, 5, B)[1]
    return llr_families.apply(name, flow).astype(np.int8)   # "zero"


def _host_batch(K):
    """The CPU test's batch: AWGN frames at 16 steps per unit (generator frames, and frames carrying
    gCRC24B where K > 24), an all-zero codeword, +127, -128 and random bytes."""
    n = 3 * K + 12
    parts = [_awgn(K, 1.0, 3, 16, 5)]
    if K > 24:
        parts.append(_crc(K, 1.0, 3, 16))
    parts += [np.zeros((1, n), dtype=np.int8), np.full((1, n), 127, dtype=np.int8), np.full((1, n), -128, dtype=np.int8),
              np.random.default_rng(K).integers(-128, 128, (2, n)).astype(np.int8)]
    return np.concatenate(parts)


FRAMES = {"awgn": _awgn, "crc": _crc, "pattern": _pattern, "host": _host_batch}


@functools.lru_cache(maxsize=None)
def whole_wave_case(K=1024):
    """(q, rows, Le) of 130 codewords: 0..63 are copies of the earliest-stopping frame (HDA) of the
    1.0 dB case, a wave that may leave early; the rest are the 0.5 dB frames.  A codeword's reference
    does not depend on its batch, so the references are those cases' own."""
    one = reference(("awgn", 1.0, 130), K, W.ITERS, (255, 3))
    half = reference(("awgn", 0.5, 130), K, W.ITERS, (255, 3))
    first = int(np.argmin(W.stops(one[1], "hda")))
    return _frozen(*(np.concatenate([np.repeat(a[first:first + 1], 64, axis=0), b[:66]]) for a, b in zip(one, half)))


@functools.lru_cache(maxsize=None)
def used(key, K, iters, setting, rule, min_iters=1, poly=CRC24B):
    u = W.stops(reference(key, K, iters, setting)[1], rule, min_iters, poly)
    u.setflags(write=False)
    return u


def le_mask(u, iters):
    """bool [B, iters, 1, 1]: the Le entries a stopped decode defines (iterations <= used)."""
    return (np.arange(iters)[None, :] < np.asarray(u)[:, None])[:, :, None, None]
