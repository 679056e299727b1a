"""LTE rate matching (3GPP TS 36.212 5.1.4.1) restated in numpy from its definition, for the tests.

The coded stream s[0..3K+12) is the three LTE streams interleaved: d_i(k) = s[3k+i], k < D = K+4.
Everything here works on stream positions (the index into s), with -1 standing for <NULL>: the
sub-block interleaver output v_i, the circular buffer w, and the selection e_0 .. e_{E-1}.  Nothing is
inverted or tabulated the way the library does it: the buffer is built forwards and then read.
"""
import numpy as np

P = np.array([0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30,
              1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31])


def layout(K):
    """(D, R, Kpi, Kw, ND)"""
    D = K + 4
    R = -(-D // 32)
    Kpi = 32 * R
    return D, R, Kpi, 3 * Kpi, Kpi - D


def circular_buffer(K):
    """w[0..Kw) as stream positions, -1 = <NULL>."""
    D, R, Kpi, Kw, ND = layout(K)
    y = np.full((3, Kpi), -1, dtype=np.int64)          # y_j = <NULL> for j < ND, y_{ND+k} = d(k)
    for i in range(3):
        y[i, ND:] = 3 * np.arange(D) + i
    k = np.arange(Kpi)
    base = P[k // R] + 32 * (k % R)
    v0, v1, v2 = y[0, base], y[1, base], y[2, (base + 1) % Kpi]
    w = np.empty(Kw, dtype=np.int64)
    w[:Kpi] = v0
    w[Kpi::2] = v1
    w[Kpi + 1::2] = v2
    return w


def k0(K, Ncb, rv):
    _, R, _, Kw, _ = layout(K)
    Ncb = Ncb or Kw
    return R * (2 * -(-Ncb // (8 * R)) * rv + 2)


def n_nonnull(K, Ncb=0):
    w = circular_buffer(K)
    return int((w[:Ncb or len(w)] >= 0).sum())


def index(K, Ncb, rv, E):
    """Stream position of e_k, k < E: the non-NULL entries of w[(k0 + j) mod Ncb], j = 0, 1, 2, ..."""
    w = circular_buffer(K)
    Ncb = Ncb or len(w)
    assert layout(K)[2] <= Ncb <= len(w)
    ring = np.roll(w[:Ncb], -(k0(K, Ncb, rv) % Ncb))   # one trip round the buffer from k0
    return np.resize(ring[ring >= 0], E).astype(np.int64)   # np.resize repeats it for as long as needed


def dematch(e, K, Ncb, rv, prior=None):
    """e [B, E] -> [B, 3K+12] of e's dtype: position q gets the sum of the e_k selected from it, added
    in ascending k in e's precision (np.add.at applies its adds in index order), onto `prior` (HARQ
    accumulation; not modified) or +0.0."""
    e = np.asarray(e)
    B, E = e.shape
    out = np.zeros((B, 3 * K + 12), dtype=e.dtype) if prior is None else np.array(prior, dtype=e.dtype, copy=True)
    idx = index(K, Ncb, rv, E)
    for b in range(B):
        np.add.at(out[b], idx, e[b])
    return out
