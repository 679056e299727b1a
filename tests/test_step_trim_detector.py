"""The exact log-MAP kernel's speculation detector in the form the alpha window issues it
(td_kernels.hip spec_check): per step the exact difference's bucket -- the bit field of d clamped to
the table's 29 rows -- is XOR-ed with the bucket the row was read from and ADDED into a per-lane
32-bit word; the window is recomputed when any lane of the wave (8 codewords) holds a non-zero word.
(Before, the xor was OR-ed in: two operations a step where the xor-add is one.)

The form is restated here in numpy, on the per-step differences d (normalised metrics) and dr
(unnormalised) of the oracle's alpha recursion, which this file recomputes with numpy's IEEE
arithmetic in the oracle's operation order (oracle/turbo_oracle_spec.inc) -- checked against
pyoracle.spec_miss_turbo's own count per codeword before anything is concluded from it.  Asserted:
  (a) every (wave, SISO, window) with a true bucket mismatch in any lane has a non-zero word (the sum
      cannot wrap: at most 15 terms below 2^13), and no window without one has;
  (b) on AWGN frames the share of windows flagged is the parent detector's, which is zero.
"""
import functools

import numpy as np
import pytest

import pyoracle as O
import quantised_cases as Q

K, F1, F2, ITERS = 1024, 31, 64, 4
W = O.SPEC_WINDOW
NLUT = 29   # td_tables.h kLutSize
GEOM = {np.float64: dict(shift=18, width=13, base=(1023 - 4) << 2, hi=lambda a: (a.view(np.uint64) >> np.uint64(32)).astype(np.uint32)),
        np.float32: dict(shift=21, width=10, base=(127 - 4) << 2, hi=lambda a: a.view(np.uint32))}


@functools.lru_cache(maxsize=None)
def maxstar_table(dt):
    """E_algorithm's correction as a step function of |d|, read off pyoracle's max* by bisection:
    (thresholds ascending, values), value[i] applying from threshold[i-1] (inclusive) on."""
    mx = O.maxstar if dt == np.float64 else O.maxstar_f32
    corr = lambda d: dt(mx(-float(d), 0.0))   # noqa: E731  (d >= 0: max(-d, 0) = 0, so the sum is the correction)
    thr, val = [], [corr(dt(0))]
    lo, top = dt(0), dt(64)
    while corr(top) != val[-1]:
        a, b = lo, top   # corr(a) == val[-1] != corr(b): the first step above a
        while np.nextafter(a, b) != b:
            m = dt((a + b) / dt(2))
            if corr(m) == val[-1]:
                a = m
            else:
                b = m
        thr.append(b)
        val.append(corr(b))
        lo = b
    return np.array(thr, dtype=dt), np.array(val, dtype=dt)


def maxstar_np(x, y, dt):
    thr, val = maxstar_table(dt)
    return np.maximum(x, y) + val[np.searchsorted(thr, np.abs(y - x), side="right")]


def test_numpy_maxstar_is_the_oracles():
    for dt, mx in ((np.float64, O.maxstar), (np.float32, O.maxstar_f32)):
        thr, val = maxstar_table(dt)
        assert thr.size == 15 and val[-1] == 0
        rng = np.random.default_rng(5)
        x = np.concatenate([rng.normal(0, 6, 4000), np.zeros(15), np.zeros(15), np.zeros(15)]).astype(dt)
        y = np.concatenate([rng.normal(0, 6, 4000), thr, np.nextafter(thr, dt(0)), -thr]).astype(dt)
        ref = np.array([mx(float(a), float(b)) for a, b in zip(x, y)], dtype=dt)
        assert np.array_equal(maxstar_np(x, y, dt), ref)


def alpha_differences(recs, La, dt):
    """(d, dr) [B, L, 8] of every alpha step of one SISO per row: turbo_oracle_spec.inc's tx - ty on the
    normalised and on the unnormalised metrics, in its operation order, vectorised over the batch."""
    t = O.trellis()
    B, L = La.shape
    p0 = np.array([t.laststat[j][0] for j in range(8)])
    p1 = np.array([t.laststat[j][1] for j in range(8)])
    o0 = np.array([t.nextout[p0[j]][1] for j in range(8)], dtype=dt)
    o1 = np.array([t.nextout[p1[j]][3] for j in range(8)], dtype=dt)
    raw = np.full((B, 8), -1e20, dtype=dt)
    raw[:, 0] = 0
    alpha = raw.copy()
    d, dr = np.empty((B, L, 8), dtype=dt), np.empty((B, L, 8), dtype=dt)
    for k in range(L):
        ys, yp, la2 = recs[:, 2 * k, None], recs[:, 2 * k + 1, None], La[:, k, None] / dt(2)
        g0 = -ys + yp * o0 - la2
        g1 = ys + yp * o1 + la2
        tx, ty = g0 + alpha[:, p0], g1 + alpha[:, p1]
        d[:, k] = ty - tx
        dr[:, k] = (g1 + raw[:, p1]) - (g0 + raw[:, p0])
        raw = maxstar_np(tx, ty, dt)
        alpha = raw - raw.max(axis=1, keepdims=True)
    return d, dr


def siso_inputs(flow, K, f1, f2, iters, dt):
    """(recs [B, 2L], La [B, L]) of each of the 2 * iters SISOs of the oracle's turbo decode of flow."""
    B, L = flow.shape[0], K + 3
    pi = O.qpp(K, f1, f2)
    rec = (flow * flow.dtype.type(0.5)).astype(dt)                      # exact
    yk = np.zeros((B, 4 * L), dtype=dt)                                 # the oracle's demultiplex
    yk[:, 0:2 * K:2], yk[:, 1:2 * K:2] = rec[:, 0:3 * K:3], rec[:, 1:3 * K:3]
    yk[:, 2 * L + 1:2 * L + 2 * K:2] = rec[:, 2:3 * K:3]
    yk[:, 2 * L:2 * L + 2 * K:2] = rec[:, 3 * pi]                      # interleaved information bits
    yk[:, 2 * K:2 * K + 6], yk[:, 2 * L + 2 * K:2 * L + 2 * K + 6] = rec[:, 3 * K:3 * K + 6], rec[:, 3 * K + 6:3 * K + 12]
    le = np.array([O.turbo_decode(np.ascontiguousarray(flow[b]), K, f1, f2, iters)[1] for b in range(B)])
    out = []
    for it in range(iters):
        La = np.zeros((B, L), dtype=dt)
        if it:
            La[:, pi] = le[:, it - 1, 1, :K]
        out.append((yk[:, :2 * L], La))
        La = np.zeros((B, L), dtype=dt)
        La[:, :K] = le[:, it, 0][:, pi]
        out.append((yk[:, 2 * L:], La))
    return out


def clamped_field(a, dt):
    g = GEOM[dt]
    f = (g["hi"](np.ascontiguousarray(a)) >> np.uint32(g["shift"])) & np.uint32((1 << g["width"]) - 1)
    return np.clip(f, g["base"], g["base"] + NLUT - 1).astype(np.uint32)   # v_med3_u32(field, base, base + 28)


def true_bucket(a):
    """td_tables.h's bucket geometry from its definition (test_quantised_oracle._bucket), vectorised."""
    a = np.abs(a.astype(np.float64))
    m, e = np.frexp(np.where(a < 2.0 ** -4, 1.0, a))
    q = 4 * (e - 1 + 4) + np.floor(4 * (2 * m - 1)).astype(np.int64)
    return np.where(a < 2.0 ** -4, 0, np.minimum(q, NLUT - 1))


@functools.lru_cache(maxsize=None)
def detector_run(family, B, precision, seed=Q.SEED):
    """Per (SISO, group of 8 codewords, window): true mismatches and the kernel's word, plus the true
    mismatches per codeword (spec_miss_turbo's count)."""
    dt = np.float64 if precision == "f64" else np.float32
    flow = np.ascontiguousarray(Q.as_precision(Q.family_flow(K, F1, F2, B, family, Q.EBN0, seed), precision))
    L = K + 3
    nT = -(-L // W)
    per_cw = np.zeros(B, dtype=np.int64)
    true_win, word_win = [], []
    for recs, La in siso_inputs(flow, K, F1, F2, ITERS, dt):
        d, dr = alpha_differences(recs, La, dt)
        d, dr = d[:, W:(nT - 1) * W], dr[:, W:(nT - 1) * W]          # the speculated windows 1 .. nT-2
        mism = (true_bucket(d) != true_bucket(dr)).reshape(B, nT - 2, W * 8)
        per_cw += mism.sum(axis=(1, 2))
        x = (clamped_field(d, dt) ^ clamped_field(dr, dt)).reshape(B, nT - 2, W, 8)
        word = x.sum(axis=2, dtype=np.uint32)                        # per lane (codeword, state): kW xor-adds
        for g in range(0, B, 8):
            true_win.append(mism[g:g + 8].any(axis=(0, 2)))
            word_win.append((word[g:g + 8] != 0).any(axis=(0, 2)))
    return per_cw, np.array(true_win), np.array(word_win), flow


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("family", ["q4", "int31", "int8_q16", "zero"])
def test_every_true_mismatch_raises_the_flag(family, precision):
    """(a) on the fixed-point families, 9 codewords (a second wave with one codeword): the numpy
    recursion counts the oracle's misses per codeword, and the xor-add word is non-zero in exactly the
    windows that hold a mismatch."""
    per_cw, true_win, word_win, flow = detector_run(family, 9, precision)
    total, share = O.spec_miss_turbo(flow, K, F1, F2, ITERS)
    print(family, precision, "misses", per_cw.tolist(), "windows flagged", int(word_win.sum()), "of", word_win.size)
    assert np.array_equal(per_cw, total), "the numpy recursion is not the oracle's"
    assert np.all(word_win[true_win]), "a true bucket mismatch did not raise the flag"
    assert np.array_equal(word_win, true_win), "false misses"
    assert word_win.mean() == pytest.approx(share)
    if family in ("q4", "int31"):
        assert per_cw.sum() > 0, "this input does not reach the detector"


def test_awgn_share_stays_at_the_parents():
    """(b) synth_batch(1024, 31, 64, 0.5, 77, 64), 4 iterations, fp64: the parent detector flags no
    window (pyoracle.spec_miss_turbo, checked here first), and neither does the xor-add form."""
    assert (Q.EBN0, Q.SEED) == (0.5, 77)
    per_cw, true_win, word_win, flow = detector_run("awgn", 64, "f64")
    total, share = O.spec_miss_turbo(flow, K, F1, F2, ITERS)
    assert total.sum() == 0 and share == 0.0, "the parent's detector does not meet the condition"
    assert per_cw.sum() == 0 and not true_win.any()
    assert word_win.mean() == share == 0.0
