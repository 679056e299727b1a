"""The fixed-point decoder's sub-block schedule (td_set_fixed_window) restated in numpy from the
contract in include/turbo_mi355x.h, for the tests.

L = K + 3, nS = max(1, L // W).  Sub-block s covers [s W, (s+1) W), the last one up to L.  Its alpha
starts at max(s W - g, 0) -- terminated if s W - g <= 0, else all states 0 -- and its beta at
min(end + g, L) -- terminated if end + g >= L, else all states 0.  Everything else (branch metric,
plain max, Lambda, LLR = Lambda >> 1, f, the iteration, the hard decision) is fixed_ref's.  State
metrics are int64 and never normalised; an unreachable state is fixed_ref.FLOOR.
"""
import numpy as np

import fixed_ref as F
import pyoracle as O

_CHUNK = 64


def siso_window(xs, xp, La, W, g):
    """One windowed integer Max-Log-MAP pass: int64 [B, L] each -> LLR = Lambda >> 1, int64 [B, L]."""
    nextstat, laststat, par = F._tables()
    B, L = xs.shape
    S = xs + La
    gm = [(2 * u - 1) * S[:, :, None] + par[None, None, :, u] * xp[:, :, None] for u in range(2)]
    p0, p1 = laststat[:, 0], laststat[:, 1]
    n0, n1 = nextstat[:, 0], nextstat[:, 1]
    a0, a1 = gm[0][:, :, p0], gm[1][:, :, p1]   # into state j, from its u = 0 / u = 1 predecessor
    nS = max(1, L // W)
    lam = np.zeros((B, L), dtype=np.int64)
    for s in range(nS):
        start = s * W
        end = L if s == nS - 1 else start + W
        a_from, b_from = max(start - g, 0), min(end + g, L)
        alpha = np.zeros((B, end + 1, 8), dtype=np.int64)   # rows a_from .. end are used
        if start - g <= 0:
            alpha[:, a_from] = F.FLOOR
            alpha[:, a_from, 0] = 0
        for i in range(a_from, end):
            a = alpha[:, i]
            alpha[:, i + 1] = np.maximum(np.maximum(a[:, p0] + a0[:, i], a[:, p1] + a1[:, i]), F.FLOOR)
        beta = np.zeros((B, b_from + 1, 8), dtype=np.int64)   # rows start .. b_from are used
        if end + g >= L:
            beta[:, b_from] = F.FLOOR
            beta[:, b_from, 0] = 0
        for i in range(b_from - 1, start - 1, -1):
            b = beta[:, i + 1]
            beta[:, i] = np.maximum(np.maximum(gm[0][:, i] + b[:, n0], gm[1][:, i] + b[:, n1]), F.FLOOR)
        sl = slice(start, end)
        t0 = (alpha[:, sl][:, :, p0] + a0[:, sl] + beta[:, start + 1:end + 1]).max(axis=2)
        t1 = (alpha[:, sl][:, :, p1] + a1[:, sl] + beta[:, start + 1:end + 1]).max(axis=2)
        lam[:, sl] = t1 - t0
    assert not (lam & 1).any(), "Lambda is even"
    return lam >> 1


def decode(q, K, f1, f2, iters, W, g, le_max=255, ext_scale_q=3):
    """q [B, 3K+12] int8 -> (rows uint8 [B, iters, K], Le int16 [B, iters, 2, K+3]) of the windowed
    fixed decode with sub-blocks of W and an overlap of g."""
    q = np.asarray(q)
    assert q.dtype == np.int8 and q.ndim == 2 and q.shape[1] == 3 * K + 12 and K >= 8
    assert W >= 16 and W % 16 == 0 and 0 <= g <= 3 * W
    B, L = q.shape[0], K + 3
    pi = O.qpp(K, f1, f2).astype(np.int64)
    rows = np.zeros((B, iters, K), dtype=np.uint8)
    le_out = np.zeros((B, iters, 2, L), dtype=np.int16)
    for c0 in range(0, B, _CHUNK):
        sl = slice(c0, min(B, c0 + _CHUNK))
        xs1, xp1, xs2, xp2 = F.demux(q[sl], pi)
        n = xs1.shape[0]
        Le = np.zeros((n, L), dtype=np.int64)
        for it in range(iters):
            La = np.zeros((n, L), dtype=np.int64)
            La[:, pi] = Le[:, :K]
            Le = F.f_ext(siso_window(xs1, xp1, La, W, g) - La - xs1, le_max, ext_scale_q)
            le_out[sl, it, 0] = Le
            La = np.zeros((n, L), dtype=np.int64)
            La[:, :K] = Le[:, pi]
            llr = siso_window(xs2, xp2, La, W, g)
            Le = F.f_ext(llr - La - xs2, le_max, ext_scale_q)
            le_out[sl, it, 1] = Le
            rows[sl, it][:, pi] = (llr[:, :K] >= 0).astype(np.uint8)
    return rows, le_out
