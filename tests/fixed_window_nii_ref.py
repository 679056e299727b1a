"""Next-iteration initialisation of the fixed-point decoder's sub-block schedule (td_set_fixed_window_nii)
restated in numpy from the contract in include/turbo_mi355x.h, for the tests.

The geometry is td_set_fixed_window's (tests/fixed_window_ref.py): L = K + 3, nS = max(1, L // W), sub-block s
covers [s W, e) with e = L for the last one, a_from = s W - g, b_from = e + g.  In iteration n >= 2 the
alpha warm-up of a sub-block with a_from > 0 starts from A[a_from] of the same SISO in iteration n - 1, and
the beta warm-up of one with b_from < L from B[b_from]:

  A[p]  alpha before step p, as computed by the sub-block that outputs position p - 1
  B[p]  beta after the backward step over position p, as computed by the sub-block that outputs position p

Here every sub-block leaves the A and B of all of its own positions in two [L + 1] arrays per SISO and the
next iteration picks the rows it needs: no slots, no normalisation.  State metrics are int64 and never
normalised; an unreachable state is FLOOR, far enough below that eight iterations' growth does not bring
it near a reachable one.  tab = None is the plain max (Max-Log-MAP), tab = (shift, corr) td_set_fixed_maxstar's
maxs in the contract's order (tests/fixed_maxstar_ref.py).  Both are unchanged by a constant added to all
eight states: `jitter` (a seed) adds a random one to every stored vector, and no output may move.
"""
import numpy as np

import fixed_maxstar_ref as FM
import fixed_ref as F
import pyoracle as O

FLOOR = -(1 << 40)
_CHUNK = 130


def _mx(a, b, tab):
    return np.maximum(a, b) if tab is None else FM.maxs(a, b, tab)


def siso(xs, xp, La, W, g, tab, prev, rng=None):
    """One pass of nS sub-blocks: int64 [B, L] each -> (LLR int64 [B, L], state).  prev is the state this
    SISO returned in the previous iteration, or None (iteration 1: equal metrics).  state = (A, B), each
    int64 [B, L + 1, 8]: the rows a later iteration may start from."""
    nextstat, laststat, par = F._tables()
    B, L = xs.shape
    S = xs + La
    gm = [(2 * u - 1) * S[:, :, None] + par[None, None, :, u] * xp[:, :, None] for u in range(2)]
    p0, p1 = laststat[:, 0], laststat[:, 1]
    n0, n1 = nextstat[:, 0], nextstat[:, 1]
    a0, a1 = gm[0][:, :, p0], gm[1][:, :, p1]   # into state j, from its u = 0 / u = 1 predecessor
    nS = max(1, L // W)
    lam = np.zeros((B, L), dtype=np.int64)
    A_out = np.zeros((B, L + 1, 8), dtype=np.int64)
    B_out = np.zeros((B, L + 1, 8), dtype=np.int64)
    term = np.full(8, FLOOR, dtype=np.int64)
    term[0] = 0
    for s in range(nS):
        start = s * W
        end = L if s == nS - 1 else start + W
        a_from, b_from = max(start - g, 0), min(end + g, L)
        alpha = np.zeros((B, end + 1 - a_from, 8), dtype=np.int64)   # row i - a_from: before step i
        if start - g <= 0:
            alpha[:, 0] = term
        elif prev is not None:
            alpha[:, 0] = prev[0][:, a_from]
        for i in range(a_from, end):
            a = alpha[:, i - a_from]
            alpha[:, i + 1 - a_from] = _mx(a[:, p0] + a0[:, i], a[:, p1] + a1[:, i], tab)
        beta = np.zeros((B, b_from + 1 - start, 8), dtype=np.int64)   # row i - start: after the step over i
        if end + g >= L:
            beta[:, b_from - start] = term
        elif prev is not None:
            beta[:, b_from - start] = prev[1][:, b_from]
        for i in range(b_from - 1, start - 1, -1):
            b = beta[:, i + 1 - start]
            beta[:, i - start] = _mx(gm[0][:, i] + b[:, n0], gm[1][:, i] + b[:, n1], tab)
        sl = slice(start, end)
        al, be = alpha[:, start - a_from:end - a_from], beta[:, 1:end + 1 - start]
        t = [al + gm[u][:, sl] + be[:, :, (n0, n1)[u]] for u in range(2)]   # [b, i, source state]
        m = [t[u][:, :, 0] for u in range(2)]
        for st in range(1, 8):
            m = [_mx(m[u], t[u][:, :, st], tab) for u in range(2)]
        lam[:, sl] = m[1] - m[0]
        # A[p] for p - 1 in [start, end), B[p] for p in [start, end): this sub-block outputs those positions
        A_out[:, start + 1:end + 1] = alpha[:, start + 1 - a_from:end + 1 - a_from]
        B_out[:, start:end] = beta[:, 0:end - start]
    if rng is not None:   # a constant per stored vector: the contract defines them up to one
        A_out += rng.integers(-(1 << 20), 1 << 20, (B, L + 1, 1))
        B_out += rng.integers(-(1 << 20), 1 << 20, (B, L + 1, 1))
    if tab is None:
        assert not (lam & 1).any(), "Lambda is even"
    return FM.half(lam), (A_out, B_out)


def decode(q, K, f1, f2, iters, W, g, tab=None, le_max=255, ext_scale_q=3, jitter=None):
    """q [B, 3K+12] int8 -> (rows uint8 [B, iters, K], Le int16 [B, iters, 2, K+3]) of the sub-block decode
    {W, g} with next-iteration initialisation, with the plain max (tab None) or the table tab."""
    q = np.asarray(q)
    assert q.dtype == np.int8 and q.ndim == 2 and q.shape[1] == 3 * K + 12 and K >= 8
    assert W >= 16 and W % 16 == 0 and 0 <= g <= 3 * W and g % 16 == 0
    B, L = q.shape[0], K + 3
    pi = O.qpp(K, f1, f2).astype(np.int64)
    rng = None if jitter is None else np.random.default_rng(jitter)
    rows = np.zeros((B, iters, K), dtype=np.uint8)
    le_out = np.zeros((B, iters, 2, L), dtype=np.int16)
    for c0 in range(0, B, _CHUNK):
        sl = slice(c0, min(B, c0 + _CHUNK))
        xs1, xp1, xs2, xp2 = F.demux(q[sl], pi)
        n = xs1.shape[0]
        Le = np.zeros((n, L), dtype=np.int64)
        st1 = st2 = None   # both SISOs keep their own state
        for it in range(iters):
            La = np.zeros((n, L), dtype=np.int64)
            La[:, pi] = Le[:, :K]
            llr, st1 = siso(xs1, xp1, La, W, g, tab, st1, rng)
            Le = F.f_ext(llr - La - xs1, le_max, ext_scale_q)
            le_out[sl, it, 0] = Le
            La = np.zeros((n, L), dtype=np.int64)
            La[:, :K] = Le[:, pi]
            llr, st2 = siso(xs2, xp2, La, W, g, tab, st2, rng)
            Le = F.f_ext(llr - La - xs2, le_max, ext_scale_q)
            le_out[sl, it, 1] = Le
            rows[sl, it][:, pi] = (llr[:, :K] >= 0).astype(np.uint8)
    return rows, le_out
