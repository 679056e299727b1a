"""CPU side of the fixed-point input tests (no GPU): the input families, the restatement of the exact
log-MAP kernel's speculation detector (oracle/turbo_oracle_spec.inc), the conditions that keep the
GPU cases of test_gpu_quantised_inputs.py from going vacuous, and the fp32 == fp64 precondition of
their zero-tolerance Max-Log-MAP checks."""
import math

import numpy as np
import pytest

import llr_families as F
import pyoracle as O
import quantised_cases as Q

K, F1, F2 = 1024, 31, 64


# ---------------------------------------------------------------- the families
@pytest.mark.parametrize("name,quantum,limit", [("q4", 0.25, 8.0), ("q8", 0.125, 16.0), ("int31", 1.0, 31.0),
                                                ("int8", 1.0, 127.0), ("sign", 1.0, 1.0), ("zero", 1.0, 0.0),
                                                ("int8_q16", 65536.0, 127.0 * 65536.0)])
def test_family_is_a_saturated_grid(name, quantum, limit):
    base = Q.awgn(K, F1, F2, 9)
    f = Q.family_flow(K, F1, F2, 9, name)
    assert f.shape == base.shape and f.dtype == np.float64
    assert np.array_equal(f / quantum, np.round(f / quantum)) and np.abs(f).max() <= limit
    assert np.array_equal(f.astype(np.float32).astype(np.float64), f)
    if limit:   # exact zeros occur (sign: none, an AWGN sample is never 0) and no sign flips
        assert name == "sign" or (f == 0).sum() > 0
        assert np.array_equal(np.sign(f)[f != 0], np.sign(base)[f != 0])
    if name in ("q4", "int8", "int8_q16", "sign"):   # these frames (|LLR| up to about 12) reach the narrower limits
        assert (np.abs(f) == limit).sum() > 0


def test_family_punct_zeroes_every_second_parity():
    base = Q.awgn(K, F1, F2, 9)
    f = Q.family_flow(K, F1, F2, 9, "punct")
    body, ref = f[:, :3 * K].reshape(9, K, 3), base[:, :3 * K].reshape(9, K, 3)
    assert np.all(body[:, 1::2, 1:] == 0.0)
    assert np.array_equal(body[:, ::2], ref[:, ::2]) and np.array_equal(body[:, :, 0], ref[:, :, 0])
    assert np.array_equal(f[:, 3 * K:], base[:, 3 * K:])


# ---------------------------------------------------------------- the detector's restatement
def _bucket(d):
    """td_tables.h's bucket geometry from its definition: 4 buckets an octave from 2^-4 * 1.25 to 8."""
    d = abs(float(d))
    if d < 2.0 ** -4:
        return 0
    m, e = math.frexp(d)            # d = m 2^e, m in [0.5, 1)
    return min(4 * (e - 1 + 4) + int(4 * (2 * m - 1)), 28)


def _misses_py(recs, La, dt):
    """The detector in plain Python on dt scalars (one rounding per numpy scalar operation)."""
    t = O.trellis()
    mx = O.maxstar if dt == np.float64 else O.maxstar_f32
    L = La.size
    nT = -(-L // 15)
    raw = [dt(0)] + [dt(-1e20)] * 7
    alpha = list(raw)
    win = np.zeros(nT, dtype=np.int32)
    for k in range(L):
        ys, yp, la = dt(recs[2 * k]), dt(recs[2 * k + 1]), dt(La[k])
        new = []
        for j in range(8):
            p0, p1 = t.laststat[j][0], t.laststat[j][1]
            g0 = -ys + yp * dt(t.nextout[p0][1]) - la / dt(2)
            g1 = ys + yp * dt(t.nextout[p1][3]) + la / dt(2)
            if 1 <= k // 15 <= nT - 2:
                dr = (g1 + raw[p1]) - (g0 + raw[p0])
                d = (g1 + alpha[p1]) - (g0 + alpha[p0])
                win[k // 15] += _bucket(dr) != _bucket(d)
            new.append(dt(mx(float(g0 + alpha[p0]), float(g1 + alpha[p1]))))
        m = max(new)
        raw, alpha = new, [v - m for v in new]
    return win


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("family", ["q4", "int31", "awgn"])
def test_detector_restatement_vs_python(family, dt):
    """One SISO of L = 253 (17 windows, the last one partial) with a quantised a-priori: the C count
    per window equals a scalar Python statement of the same definition, and only interior windows count."""
    L = 253
    flow = Q.family_flow(K, F1, F2, 9, family)[3]
    recs = (0.5 * flow[:2 * L]).astype(dt)
    La = (np.round(8 * flow[2 * L:3 * L]) / 8 if family != "awgn" else flow[2 * L:3 * L]).astype(dt)
    total, win, _ = O.spec_miss_siso(recs, La)
    assert np.array_equal(win, _misses_py(recs, La, dt))
    assert total == win.sum() and win[0] == 0 and win[-1] == 0
    assert (total > 0) == (family != "awgn")


def test_detector_needs_an_interior_window():
    """L <= 30 has no speculated window (nT <= 2); K = 40 (L = 43) has one."""
    flow = Q.family_flow(K, F1, F2, 9, "q4")[0]
    for L in (4, 15, 30):
        assert O.spec_miss_siso(0.5 * flow[:2 * L], np.zeros(L))[0] == 0
    assert O.spec_miss_siso(0.5 * flow[:2 * 43], np.zeros(43))[1].size == 3


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_detector_silent_on_awgn(precision):
    """On the continuous frames every other test uses, no step's buckets differ."""
    total, share = Q.misses(K, F1, F2, 9, "awgn", 4, precision)
    assert total.sum() == 0 and share == 0.0


# the family totals on synth_batch(1024, 31, 64, 0.5, 77, 9), 4 iterations, measured in fp64: q4 503,
# int31 400, int8 58, sign 140 (fp32: 505, 362, 59, 169).  The floors are conditions: they keep the
# fixture from silently ceasing to reach the detector.
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("family,floor", [("q4", 100), ("int31", 100), ("int8", 20), ("sign", 20)])
def test_detector_fires_on_families(family, floor, precision):
    total, share = Q.misses(K, F1, F2, 9, family, 4, precision)
    print(family, precision, int(total.sum()), total.tolist(), share)
    assert total.sum() >= floor
    assert 0.0 < share <= 1.0


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("family", ["q4", "q8", "int31", "int8", "sign"])
def test_misses_of_narrow_families_are_harmless(family, precision):
    """Every miss of these families sits beside a bucket edge: the speculated row and the exact row give
    d the same correction (the neighbour's vlo is this row's vhi), so they reach the detector, the ballot
    and the recomputation, but a kernel that skipped the recomputation would decode them the same."""
    total, _, harm = O.spec_miss_turbo(Q.as_precision(Q.family_flow(K, F1, F2, 9, family), precision), K, F1, F2, 4,
                                       harmful=True)
    assert total.sum() > 0 and harm.sum() == 0


def test_misses_of_the_wide_family_are_harmful_in_fp32():
    """int8 as raw Q16 integers: in fp32 a part of the misses reads another correction from the
    speculated row than from the exact one (measured on these 9 frames, 4 iterations: 118 of 225
    misses), so this family tells a kernel that recomputes from one that does not.  In fp64 the
    roundings stay far below the edge-to-threshold distances: none is harmful."""
    flow = Q.family_flow(K, F1, F2, 9, "int8_q16")
    total, _, harm = O.spec_miss_turbo(flow.astype(np.float32), K, F1, F2, 4, harmful=True)
    print("fp32", int(total.sum()), harm.tolist())
    assert np.all(harm > 0)
    total, _, harm = O.spec_miss_turbo(flow, K, F1, F2, 4, harmful=True)
    print("fp64", int(total.sum()), harm.tolist())
    assert harm.sum() == 0


def test_redo_share_counts_groups_of_eight():
    """The share is over (group of 8, iteration, SISO, window) executions: one codeword that misses
    among 15 silent ones marks its own group's windows only."""
    a, q = Q.awgn(K, F1, F2, 9), Q.family_flow(K, F1, F2, 9, "q4")
    batch = np.concatenate([a[:8], a[:3], q[:1], a[3:7]])   # group 0 silent, group 1 has one q4 codeword
    total, share = O.spec_miss_turbo(batch, K, F1, F2, 4)
    alone, share1 = O.spec_miss_turbo(q[:1], K, F1, F2, 4)
    assert total[11] == alone[0] > 0 and total.sum() == alone[0]
    assert share == pytest.approx(share1 / 2)


# ---------------------------------------------------------------- Max-Log-MAP on dyadic inputs
@pytest.mark.parametrize("family", ["int31", "q4"])
def test_maxlog_dyadic_fp32_equals_fp64_exact(family):
    _, _, le = Q.dyadic_maxlog_precondition(K, F1, F2, 13, family, 8)
    assert np.abs(le).max() < 2 ** 12   # with a quantum of 2^-4 at the finest: far inside fp32's 24 bits


@pytest.mark.parametrize("family", ["int31", "q4"])
@pytest.mark.parametrize("nii,conc", [(False, False), (True, False), (False, True), (True, True)])
def test_maxlog_dyadic_fp32_equals_fp64_window(family, nii, conc):
    Q.dyadic_maxlog_precondition(K, F1, F2, 13, family, 8, window=(64, 30, nii, conc))


@pytest.mark.parametrize("family", ["int31", "q4"])
def test_maxlog_dyadic_fp32_equals_fp64_small(family):
    """The K = 40 frames of the occupancy-variant case (a sample of its 6150)."""
    Q.dyadic_maxlog_precondition(40, 3, 10, 151, family, 8)
