"""Transport blocks (3GPP TS 36.212 5.1.2, 5.1.4.1.2, 5.1.5) restated in numpy from their definition, for the
tests: the segmentation plan, segmentation with filler bits and both CRCs, the filler-aware rate-matching
index, rate matching / de-rate-matching of a transport block's code blocks and the concatenation.

Nothing here is computed the way the library does it.  The blocks are built forwards: the B-bit sequence is
prefixed with the filler and cut into consecutive payloads; CRCs are long divisions; the circular buffer is
ratematch_ref's, with the filler's entries nulled, and is then read.  Block-major layout as the library's:
a pair (minus [C_minus, N, K_minus] or None, plus [C_plus, N, K_plus]).
"""
import bisect
from collections import namedtuple

import numpy as np

import ratematch_ref as RM

Z = 6144
CRC24A, CRC24B = 0x864CFB, 0x800063
VALID_K = (list(range(40, 513, 8)) + list(range(528, 1025, 16)) + list(range(1056, 2049, 32))
           + list(range(2112, 6145, 64)))
assert len(VALID_K) == 188

Plan = namedtuple("Plan", "A B L C K_plus K_minus C_plus C_minus F")
FILLER, TB, TBCRC, CBCRC = 0, 1, 2, 3   # what sits at an offset of a block


def plan(A):
    B = A + 24
    if B <= Z:
        L, C, Bp = 0, 1, B
    else:
        L = 24
        C = -(-B // (Z - L))
        Bp = B + C * L
    i = bisect.bisect_left(VALID_K, -(-Bp // C))   # the smallest K with C K >= B'
    Kp = VALID_K[i]
    if C == 1:
        Cp, Km, Cm = 1, 0, 0
    else:
        Km = VALID_K[i - 1]
        Cm = (C * Kp - Bp) // (Kp - Km)
        Cp = C - Cm
    return Plan(A, B, L, C, Kp, Km, Cp, Cm, Cp * Kp + Cm * Km - Bp)


def block_sizes(p):
    return [p.K_minus] * p.C_minus + [p.K_plus] * p.C_plus


def labels(p):
    """Per block r: (kind [K_r], idx [K_r]) -- what segmentation puts at each offset: the filler, bit idx of
    the transport block, bit idx of its gCRC24A (0 = most significant), bit idx of the block's gCRC24B."""
    kind = np.concatenate([np.full(p.F, FILLER), np.full(p.A, TB), np.full(24, TBCRC)])
    idx = np.concatenate([np.zeros(p.F, dtype=np.int64), np.arange(p.A), np.arange(24)])
    out, at = [], 0
    for K in block_sizes(p):
        n = K - p.L
        out.append((np.concatenate([kind[at:at + n], np.full(p.L, CBCRC)]),
                    np.concatenate([idx[at:at + n], np.arange(p.L)])))
        at += n
    assert at == len(kind)
    return out


def crc24(bits, poly):
    """bits [n, len] (non-zero = 1) -> uint32 [n]: the remainder of the long division, register 0, no final XOR."""
    bits = (np.asarray(bits) != 0).astype(np.uint32)
    reg = np.zeros(bits.shape[0], dtype=np.uint32)
    for i in range(bits.shape[1]):
        top = ((reg >> 23) & 1) ^ bits[:, i]
        reg = ((reg << 1) & 0xFFFFFF) ^ (top * np.uint32(poly))
    return reg


def crc_bits(rem):
    """uint32 [n] -> uint8 [n, 24], most significant bit first"""
    return ((np.asarray(rem)[:, None] >> (23 - np.arange(24))) & 1).astype(np.uint8)


def pair(p, blocks):
    """blocks: list of C arrays [N, x_r] -> the block-major pair"""
    m, pl = blocks[:p.C_minus], blocks[p.C_minus:]
    return (np.stack(m) if m else None), np.stack(pl)


def unpair(p, pr):
    """the block-major pair -> list of C arrays [N, x_r]"""
    return ([pr[0][r] for r in range(p.C_minus)] if p.C_minus else []) + [pr[1][r] for r in range(p.C_plus)]


def segment(p, tb):
    """tb [N, A] -> the pair of code blocks, uint8 0 / 1"""
    bits = (np.asarray(tb) != 0).astype(np.uint8)
    crc_a = crc_bits(crc24(bits, CRC24A))
    blocks = []
    for kind, idx in labels(p):
        blk = np.zeros((bits.shape[0], len(kind)), dtype=np.uint8)
        blk[:, kind == TB] = bits[:, idx[kind == TB]]
        blk[:, kind == TBCRC] = crc_a[:, idx[kind == TBCRC]]
        if p.L:
            blk[:, -24:] = crc_bits(crc24(blk[:, :-24], CRC24B))
        blocks.append(blk)
    return pair(p, blocks)


def concat(p, pr):
    """the pair of hard decisions -> (tb [N, A] uint8, cb_rem [N, C] uint32, tb_rem [N] uint32)"""
    blocks = [(np.asarray(b) != 0).astype(np.uint8) for b in unpair(p, pr)]
    blocks[0][:, :p.F] = 0   # the filler is known
    cb = np.stack([crc24(b, CRC24B) if p.L else np.zeros(b.shape[0], dtype=np.uint32) for b in blocks], axis=1)
    b = np.concatenate([blk[:, :blk.shape[1] - p.L] for blk in blocks], axis=1)[:, p.F:]
    assert b.shape[1] == p.B
    return b[:, :p.A].copy(), cb, crc24(b, CRC24A)


def ncb(K, cap):
    Kw = RM.layout(K)[3]
    return Kw if cap == 0 else min(cap, Kw)


def index_filler(K, Ncb, F, rv, E):
    """RM.index with d0 and d1 of the first F bits <NULL> in the circular buffer"""
    w = RM.circular_buffer(K).copy()
    w[(w >= 0) & (w // 3 < F) & (w % 3 != 2)] = -1
    Ncb = Ncb or len(w)
    assert RM.layout(K)[2] <= Ncb <= len(w)
    ring = np.roll(w[:Ncb], -(RM.k0(K, Ncb, rv) % Ncb))
    return np.resize(ring[ring >= 0], E).astype(np.int64)


def rm_sizes(C, G, NlQm):
    """(E_lo, E_hi, n_lo)"""
    assert G % NlQm == 0 and G // NlQm >= C
    Gp = G // NlQm
    return NlQm * (Gp // C), NlQm * -(-Gp // C), C - Gp % C


def block_e(p, G, NlQm):
    E_lo, E_hi, n_lo = rm_sizes(p.C, G, NlQm)
    return [E_lo if r <= p.C - (G // NlQm) % p.C - 1 else E_hi for r in range(p.C)]


def block_index(p, cap, rv, G, NlQm):
    """idx_r of every block"""
    return [index_filler(K, ncb(K, cap), p.F if r == 0 else 0, rv, E)
            for r, (K, E) in enumerate(zip(block_sizes(p), block_e(p, G, NlQm)))]


def rate_match(p, coded, cap, rv, G, NlQm):
    """the pair of coded streams [C, N, 3K+12] -> f [N, G]"""
    return np.concatenate([c[:, idx] for c, idx in zip(unpair(p, coded), block_index(p, cap, rv, G, NlQm))], axis=1)


def filler_value(x, dtype):
    if np.dtype(dtype) == np.int8:
        return np.int8(np.clip(np.rint(x), -127, 127))
    return np.dtype(dtype).type(x)


def rate_dematch(p, f, cap, rv, NlQm, filler_llr, prior=None):
    """f [N, G] float64 / float32 / int8 -> the pair of soft buffers [C, N, 3K+12] of f's dtype: per block the
    sums in ascending k in f's precision (int8: saturated to +-127 after every addition, a prior -128 read as
    -127 when it is added to), onto `prior` (a pair; not modified) or zero; then the filler's d0 and d1 of
    block 0 are filler_llr."""
    f = np.asarray(f)
    n, G = f.shape
    pri = unpair(p, prior) if prior is not None else [None] * p.C
    out, at = [], 0
    for r, (K, idx) in enumerate(zip(block_sizes(p), block_index(p, cap, rv, G, NlQm))):
        e = f[:, at:at + len(idx)]
        at += len(idx)
        if f.dtype == np.int8:
            acc = np.zeros((n, 3 * K + 12), dtype=np.int32) if pri[r] is None else pri[r].astype(np.int32)
            # one trip round the buffer at a time: inside a trip every position is selected once, and the
            # trips come in ascending k
            again = np.flatnonzero(idx[1:] == idx[0])
            trip = int(again[0]) + 1 if again.size else len(idx)
            for k in range(0, len(idx), trip):
                q = idx[k:k + trip]
                assert len(np.unique(q)) == len(q)
                acc[:, q] = np.clip(np.maximum(acc[:, q], -127) + e[:, k:k + trip], -127, 127)
            o = acc.astype(np.int8)
        else:
            o = _dematch_float(e, K, idx, pri[r])
        if r == 0 and p.F:
            k = np.arange(p.F)
            o[:, 3 * k] = o[:, 3 * k + 1] = filler_value(filler_llr, f.dtype)
        out.append(o)
    assert at == G
    return pair(p, out)


def _dematch_float(e, K, idx, prior):
    out = np.zeros((e.shape[0], 3 * K + 12), dtype=e.dtype) if prior is None else np.array(prior, dtype=e.dtype, copy=True)
    for b in range(e.shape[0]):
        np.add.at(out[b], idx, e[b])   # applies its adds in index order: ascending k
    return out
