"""The fixed-point decoder (TD_FIXED) restated in numpy from its definition, for the tests.

int8 channel LLRs in the reference stream layout, integer Max-Log-MAP on twice the float branch
metric, the extrinsic through f(r) = clamp(sign(r) * ((|r| * ext_scale_q) >> 2), +-le_max).  State
metrics are int64 and never normalised; an unreachable state is -2**24.  With ext_scale_q = 4 and
nothing clamped this is the fp64 Max-Log-MAP oracle on the same integers, bit for bit
(tests/test_fixed_host.py).  Also the saturating int8 de-rate-matching, on ratematch_ref's index.
"""
import numpy as np

import pyoracle as O
import ratematch_ref as RM

FLOOR = -(1 << 24)
_CHUNK = 32   # codewords decoded together (bounds the [B, L, 8] temporaries)


def _tables():
    t = O.trellis()
    nextstat = np.array([[t.nextstat[s][u] for u in range(2)] for s in range(8)])
    laststat = np.array([[t.laststat[s][u] for u in range(2)] for s in range(8)])
    par = np.array([[t.nextout[s][2 * u + 1] for u in range(2)] for s in range(8)])   # o_u(s)
    return nextstat, laststat, par


def quantise(flow, steps_per_unit):
    """Round to nearest (ties to even, as torch.round), clamp +-127, int8."""
    return np.clip(np.rint(np.asarray(flow, dtype=np.float64) * steps_per_unit), -127, 127).astype(np.int8)


def demux(q, pi):
    """q [B, 3K+12] int8 -> xs1, xp1, xs2, xp2, each int64 [B, K+3] (log_map.cpp:1083-1127 without the 0.5)."""
    q = np.asarray(q).astype(np.int64)
    q = np.where(q == -128, -127, q)
    B, n = q.shape
    K = (n - 12) // 3
    L = K + 3
    xs1, xp1, xs2, xp2 = (np.zeros((B, L), dtype=np.int64) for _ in range(4))
    body = q[:, :3 * K].reshape(B, K, 3)
    xs1[:, :K], xp1[:, :K], xp2[:, :K] = body[:, :, 0], body[:, :, 1], body[:, :, 2]
    xs2[:, :K] = xs1[:, pi]
    t1, t2 = q[:, 3 * K:3 * K + 6], q[:, 3 * K + 6:]
    xs1[:, K:], xp1[:, K:] = t1[:, 0::2], t1[:, 1::2]
    xs2[:, K:], xp2[:, K:] = t2[:, 0::2], t2[:, 1::2]
    return xs1, xp1, xs2, xp2


def siso(xs, xp, La):
    """One terminated integer Max-Log-MAP pass: int64 [B, L] each -> LLR = Lambda >> 1, int64 [B, L]."""
    nextstat, laststat, par = _tables()
    B, L = xs.shape
    S = xs + La
    # g[u][b, i, s]: the metric of the branch leaving state s with input u at position i
    g = [(2 * u - 1) * S[:, :, None] + par[None, None, :, u] * xp[:, :, None] for u in range(2)]
    p0, p1 = laststat[:, 0], laststat[:, 1]
    n0, n1 = nextstat[:, 0], nextstat[:, 1]
    a0, a1 = g[0][:, :, p0], g[1][:, :, p1]         # into state j, from its u = 0 / u = 1 predecessor
    alpha = np.full((B, L + 1, 8), FLOOR, dtype=np.int64)
    beta = np.full((B, L + 1, 8), FLOOR, dtype=np.int64)
    alpha[:, 0, 0] = 0
    beta[:, L, 0] = 0
    for i in range(L):
        a = alpha[:, i]
        alpha[:, i + 1] = np.maximum(np.maximum(a[:, p0] + a0[:, i], a[:, p1] + a1[:, i]), FLOOR)
    for i in range(L - 1, -1, -1):
        b = beta[:, i + 1]
        beta[:, i] = np.maximum(np.maximum(g[0][:, i] + b[:, n0], g[1][:, i] + b[:, n1]), FLOOR)
    t0 = (alpha[:, :L][:, :, p0] + a0 + beta[:, 1:]).max(axis=2)
    t1 = (alpha[:, :L][:, :, p1] + a1 + beta[:, 1:]).max(axis=2)
    lam = t1 - t0
    assert not (lam & 1).any(), "Lambda is even"
    return lam >> 1


def f_ext(r, le_max, ext_scale_q):
    return np.clip(np.sign(r) * ((np.abs(r) * ext_scale_q) >> 2), -le_max, le_max)


def decode(q, K, f1, f2, iters, le_max=255, ext_scale_q=3):
    """q [B, 3K+12] int8 -> (rows uint8 [B, iters, K], Le int16 [B, iters, 2, K+3], share of the Le
    values that the +-le_max clamp changed)."""
    q = np.asarray(q)
    assert q.dtype == np.int8 and q.ndim == 2 and q.shape[1] == 3 * K + 12 and K >= 8
    B, L = q.shape[0], K + 3
    pi = O.qpp(K, f1, f2).astype(np.int64)
    rows = np.zeros((B, iters, K), dtype=np.uint8)
    le_out = np.zeros((B, iters, 2, L), dtype=np.int16)
    clamped = 0
    for c0 in range(0, B, _CHUNK):
        sl = slice(c0, min(B, c0 + _CHUNK))
        xs1, xp1, xs2, xp2 = demux(q[sl], pi)
        n = xs1.shape[0]
        Le = np.zeros((n, L), dtype=np.int64)
        for it in range(iters):
            La = np.zeros((n, L), dtype=np.int64)
            La[:, pi] = Le[:, :K]
            r = siso(xs1, xp1, La) - La - xs1
            Le = f_ext(r, le_max, ext_scale_q)
            clamped += int((np.abs((np.abs(r) * ext_scale_q) >> 2) > le_max).sum())
            le_out[sl, it, 0] = Le
            La = np.zeros((n, L), dtype=np.int64)
            La[:, :K] = Le[:, pi]
            llr = siso(xs2, xp2, La)
            r = llr - La - xs2
            Le = f_ext(r, le_max, ext_scale_q)
            clamped += int((np.abs((np.abs(r) * ext_scale_q) >> 2) > le_max).sum())
            le_out[sl, it, 1] = Le
            rows[sl, it][:, pi] = (llr[:, :K] >= 0).astype(np.uint8)
    return rows, le_out, clamped / float(B * iters * 2 * L)


def sat_add(acc, v):
    return np.clip(acc + v, -127, 127)


def dematch(e, K, Ncb, rv, prior=None):
    """Saturating int8 de-rate-matching: e int8 [B, E] -> int8 [B, 3K+12].  Each position is the sum of
    its e in ascending k, saturated to [-127, 127] after every addition, starting from `prior` (-128
    read as -127; not modified) or 0; a position nothing selects keeps its prior value or is 0."""
    e = np.asarray(e)
    assert e.dtype == np.int8
    B, E = e.shape
    n = 3 * K + 12
    out = np.zeros((B, n), dtype=np.int64) if prior is None else np.asarray(prior).astype(np.int64).copy()
    raw = out.copy()
    touched = np.zeros(n, dtype=bool)
    out = np.maximum(out, -127)
    idx = RM.index(K, Ncb, rv, E)
    ev = e.astype(np.int64)
    touched[idx] = True
    # ascending k, a run of k without a repeated position at a time (within a run the order is free)
    start, seen = 0, set()
    for k in range(E + 1):
        if k == E or int(idx[k]) in seen:
            run = idx[start:k]
            out[:, run] = sat_add(out[:, run], ev[:, start:k])
            start, seen = k, set()
        if k < E:
            seen.add(int(idx[k]))
    out[:, ~touched] = raw[:, ~touched]
    return out.astype(np.int8)
