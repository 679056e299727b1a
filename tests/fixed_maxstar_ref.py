"""The fixed-point decoder's integer log-MAP (td_set_fixed_maxstar) restated in numpy from the contract in
include/turbo_mi355x.h, for the tests: the exact schedule and the sub-block geometry of td_set_fixed_window.

Every max of the TD_FIXED contract becomes maxs(a, b) = max(a, b) + corr[min(|a - b| >> shift, 7)], in the
contract's order: alpha into state j from its u = 0 predecessor first; beta of state s from its u = 0
branch first; each of Lambda's two terms a left fold over the source state s = 0 .. 7 of alpha[s] +
gamma_u(s) + beta[next(s, u)].  LLR = Lambda / 2 towards zero.  Demultiplexing, f and the quantiser are
fixed_ref's, the geometry is fixed_window_ref's.  State metrics are int64, never normalised and never
clamped; an unreachable state is FLOOR, and with corr[7] == 0 no output depends on its value.
"""
import numpy as np

import fixed_ref as F
import pyoracle as O

FLOOR = -(1 << 28)
_CHUNK = 130
ZERO = (0, (0,) * 8)              # Max-Log-MAP
CONSTANT = (0, (5, 5, 0, 0, 0, 0, 0, 0))
WIDEST = (8, (63,) * 7 + (0,))    # the largest entries and the widest buckets the setter takes


def table(steps_per_unit, shift=None):
    """The table rule, stated independently of the C helper: s = 2 steps_per_unit metric steps per nat,
    corr[j] = floor(s log1p(exp(-(j + 1/2) 2^shift / s)) + 1/2) for j < 7, corr[7] = 0; without a shift the
    smallest one at which s log1p(exp(-7 2^shift / s)) < 1.  -> (shift, corr), or None where the rule is
    not valid (an entry above 63 or a shift above 8)."""
    s = 2.0 * float(steps_per_unit)
    if shift is None:
        shift = next((k for k in range(0, 64) if s * np.log1p(np.exp(-7.0 * 2.0 ** k / s)) < 1.0))
    if shift > 8:
        return None
    corr = [int(np.floor(s * np.log1p(np.exp(-(j + 0.5) * 2.0 ** shift / s)) + 0.5)) for j in range(7)] + [0]
    return None if max(corr) > 63 else (int(shift), tuple(corr))


DEFAULT = (3, (9, 6, 4, 3, 2, 1, 1, 0))   # table(8), asserted by the tests


def maxs(a, b, tab):
    shift, corr = tab
    return np.maximum(a, b) + np.asarray(corr, dtype=np.int64)[np.minimum(np.abs(a - b) >> shift, 7)]


def half(lam):
    """Lambda / 2 towards zero."""
    return np.sign(lam) * (np.abs(lam) >> 1)


def siso(xs, xp, La, tab, W=None, g=0):
    """One integer log-MAP pass, int64 [B, L] each -> LLR int64 [B, L]: terminated over the whole trellis
    (W None), or td_set_fixed_window's sub-blocks of W with an overlap of g."""
    nextstat, laststat, par = F._tables()
    B, L = xs.shape
    S = xs + La
    # gm[u][b, i, s]: the metric of the branch leaving state s with input u at position i
    gm = [(2 * u - 1) * S[:, :, None] + par[None, None, :, u] * xp[:, :, None] for u in range(2)]
    p0, p1 = laststat[:, 0], laststat[:, 1]
    n0, n1 = nextstat[:, 0], nextstat[:, 1]
    a0, a1 = gm[0][:, :, p0], gm[1][:, :, p1]   # into state j, from its u = 0 / u = 1 predecessor
    nS = 1 if W is None else max(1, L // W)
    if W is None:
        W, g = L, 0
    lam = np.zeros((B, L), dtype=np.int64)
    for s in range(nS):
        start = s * W
        end = L if s == nS - 1 else start + W
        a_from, b_from = max(start - g, 0), min(end + g, L)
        alpha = np.zeros((B, end + 1, 8), dtype=np.int64)   # rows a_from .. end are used
        if start - g <= 0:
            alpha[:, a_from] = FLOOR
            alpha[:, a_from, 0] = 0
        for i in range(a_from, end):
            a = alpha[:, i]
            alpha[:, i + 1] = maxs(a[:, p0] + a0[:, i], a[:, p1] + a1[:, i], tab)
        beta = np.zeros((B, b_from + 1, 8), dtype=np.int64)   # rows start .. b_from are used
        if end + g >= L:
            beta[:, b_from] = FLOOR
            beta[:, b_from, 0] = 0
        for i in range(b_from - 1, start - 1, -1):
            b = beta[:, i + 1]
            beta[:, i] = maxs(gm[0][:, i] + b[:, n0], gm[1][:, i] + b[:, n1], tab)
        sl = slice(start, end)
        al, be = alpha[:, sl], beta[:, start + 1:end + 1]
        t = [al + gm[u][:, sl] + be[:, :, (n0, n1)[u]] for u in range(2)]   # [b, i, source state]
        m = [t[u][:, :, 0] for u in range(2)]
        for st in range(1, 8):
            m = [maxs(m[u], t[u][:, :, st], tab) for u in range(2)]
        lam[:, sl] = m[1] - m[0]
    return half(lam)


def decode(q, K, f1, f2, iters, tab, le_max=255, ext_scale_q=4, win=None):
    """q [B, 3K+12] int8 -> (rows uint8 [B, iters, K], Le int16 [B, iters, 2, K+3], share of the Le values
    that the +-le_max clamp changed) of the decode with the table tab = (shift, corr) on the exact schedule
    (win None) or on the sub-block schedule win = (window, overlap)."""
    q = np.asarray(q)
    assert q.dtype == np.int8 and q.ndim == 2 and q.shape[1] == 3 * K + 12 and K >= 8
    shift, corr = tab
    assert 0 <= shift <= 8 and len(corr) == 8 and corr[7] == 0 and all(0 <= c <= 63 for c in corr)
    W, g = win if win is not None else (None, 0)
    B, L = q.shape[0], K + 3
    pi = O.qpp(K, f1, f2).astype(np.int64)
    rows = np.zeros((B, iters, K), dtype=np.uint8)
    le_out = np.zeros((B, iters, 2, L), dtype=np.int16)
    clamped = 0
    for c0 in range(0, B, _CHUNK):
        sl = slice(c0, min(B, c0 + _CHUNK))
        xs1, xp1, xs2, xp2 = F.demux(q[sl], pi)
        n = xs1.shape[0]
        Le = np.zeros((n, L), dtype=np.int64)
        for it in range(iters):
            La = np.zeros((n, L), dtype=np.int64)
            La[:, pi] = Le[:, :K]
            r = siso(xs1, xp1, La, tab, W, g) - La - xs1
            Le = F.f_ext(r, le_max, ext_scale_q)
            clamped += int((np.abs((np.abs(r) * ext_scale_q) >> 2) > le_max).sum())
            le_out[sl, it, 0] = Le
            La = np.zeros((n, L), dtype=np.int64)
            La[:, :K] = Le[:, pi]
            llr = siso(xs2, xp2, La, tab, W, g)
            r = llr - La - xs2
            Le = F.f_ext(r, le_max, ext_scale_q)
            clamped += int((np.abs((np.abs(r) * ext_scale_q) >> 2) > le_max).sum())
            le_out[sl, it, 1] = Le
            rows[sl, it][:, pi] = (llr[:, :K] >= 0).astype(np.uint8)
    return rows, le_out, clamped / float(B * iters * 2 * L)
