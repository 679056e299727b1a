"""Shared by test_window_stop_oracle.py (CPU) and test_gpu_window_stop.py: the two stopping rules in
numpy (include/turbo_mi355x.h), the windowed cases of td_set_window_stop's tests and their
references -- pyoracle.turbo_decode_window's per-iteration rows, computed once per case and read-only.

  HDA  stop after the smallest n >= max(2, min_iters) with row(n) == row(n-1), else at `iterations`
  CRC  stop after the smallest n >= max(1, min_iters) with CRC-24(row(n)) == 0, else at `iterations`
"""
import functools
from collections import Counter

import numpy as np

import pyoracle as O

CRC24A, CRC24B = 0x864CFB, 0x800063
ITERS = 8

# the windowed schedule's max* forms (tests/test_gpu_window.py): "logmap" = the one-read table
OALGO = {"logmap": O.ALGO_LOGMAP_Q, "logmap-exact": O.ALGO_LOGMAP, "maxlog": O.ALGO_MAXLOG}

# name -> (K, f1, f2, W, g, nii, concurrent, ext_scale)
SCHED = {
    "A": (40, 3, 10, 16, 16, False, False, 1.0),
    "B": (40, 3, 10, 16, 0, True, True, 0.77),
    "C": (200, 13, 50, 48, 6, True, False, 1.0),
    "D": (1024, 31, 64, 64, 30, False, False, 1.0),
    "Dn": (1024, 31, 64, 64, 30, True, True, 0.77),   # D's frames with NII, concurrent SISOs, x0.77
    "E": (6144, 263, 480, 64, 30, False, False, 1.0),
}


def crc24(bits, poly):
    reg = 0
    for b in bits:
        top = ((reg >> 23) & 1) ^ int(b)
        reg = (reg << 1) & 0xFFFFFF
        if top:
            reg ^= poly
    return reg


def hda_stop(rows, min_iters=1):
    """rows [iters, K] of one codeword -> iterations used (1-based)."""
    for n in range(max(2, min_iters), rows.shape[0] + 1):
        if np.array_equal(rows[n - 1], rows[n - 2]):
            return n
    return rows.shape[0]


def crc_stop(rows, poly, min_iters=1):
    for n in range(max(1, min_iters), rows.shape[0] + 1):
        if crc24(rows[n - 1], poly) == 0:
            return n
    return rows.shape[0]


def stops(rows, rule, min_iters=1, poly=CRC24B):
    """rows [B, iters, K] -> int32 [B]."""
    f = (lambda r: hda_stop(r, min_iters)) if rule == "hda" else (lambda r: crc_stop(r, poly, min_iters))
    return np.array([f(r) for r in rows], dtype=np.int32)


def frozen(rows, used):
    """The all_iters rows of a stopped decode: rows after the stop are copies of the stop row."""
    out = rows.copy()
    for b, n in enumerate(used):
        out[b, n:] = rows[b, n - 1]
    return out


def spread(used):
    return dict(sorted(Counter(int(v) for v in used).items()))


def crc_frames(K, f1, f2, poly, sigma, B):
    """B frames whose K bits are K-24 random bits (default_rng(5), drawn first) and their CRC-24,
    turbo-encoded, BPSK (bit 1 -> +1) over AWGN of that sigma, as channel LLRs 2y/sigma^2."""
    rng = np.random.default_rng(5)
    payload = rng.integers(0, 2, (B, K - 24))
    flow = np.zeros((B, 3 * K + 12))
    for b in range(B):
        c = crc24(payload[b], poly)
        row = np.concatenate([payload[b], [(c >> (23 - j)) & 1 for j in range(24)]]).astype(np.int32)
        coded = O.encode(row, f1, f2)
        y = (2.0 * coded - 1.0) + rng.normal(0.0, sigma, coded.size)
        flow[b] = 2.0 * y / sigma ** 2
    return flow


def _oracle(flow, sched, algo):
    K, f1, f2, W, g, nii, conc, scale = SCHED[sched]
    rows, les = zip(*(O.turbo_decode_window(flow[b], K, f1, f2, ITERS, W, g, algo=OALGO[algo], nii=nii,
                                            concurrent=conc, scale=scale) for b in range(flow.shape[0])))
    rows, les = np.array(rows).astype(np.uint8), np.array(les)
    for a in (flow, rows, les):
        a.setflags(write=False)
    return flow, rows, les


@functools.lru_cache(maxsize=None)
def synth_case(sched, ebn0, B, algo="logmap", precision="f64"):
    """(flow [B, 3K+12], oracle rows [B, ITERS, K] uint8, oracle Le [B, ITERS, 2, K+3]) of the frames
    O.synth_batch(K, f1, f2, ebn0, 4242, B) under SCHED[sched]; fp32: the flow cast to float32."""
    K, f1, f2 = SCHED[sched][:3]
    _, flow = O.synth_batch(K, f1, f2, ebn0, 4242, B)
    if precision == "f32":
        flow = flow.astype(np.float32)
    return _oracle(flow, sched, algo)


@functools.lru_cache(maxsize=None)
def crc_case(sched, poly, sigma, B):
    K, f1, f2 = SCHED[sched][:3]
    return _oracle(crc_frames(K, f1, f2, poly, sigma, B), sched, "logmap")
