"""The decoders on fixed-point LLRs (tests/llr_families.py): multiples of a quantum, saturated, with
exact zeros -- what a receiver hands a turbo decoder, and what no other test feeds the kernels.

On such input the max* differences sit exactly on bucket edges (the `fabs(d) >= thr` select, the
bucket bit field, the windowed one-read table's finer grid), hard decisions tie at LLR == 0, and the
exact log-MAP kernel's speculative alpha window (td_kernels.hip kASpec) misses and recomputes windows
in the committed order; on continuous AWGN frames its detector never fires
(tests/test_quantised_oracle.py counts both on the CPU).  Every case that claims to exercise the
detector first asserts that the CPU restatement of it (pyoracle.spec_miss_turbo) counts misses on its
own input.

What each kind of input can show: a miss of the narrow families (q4, q8, int31, int8, sign) sits
beside a bucket edge, where the speculated and the exact table row give the same correction, so these
inputs run the detector, the ballot and the recomputation (and the bucket-edge compares of every
pass) but would decode the same if the recomputation were skipped.  int8_q16 (int8 as raw Q16
integers) in fp32 has misses whose two rows differ (spec_miss_turbo's harmful count): on it the
production kernel must equal the committed-order builds byte for byte, and a build with `miss`
forced to 0 does not.

References and inputs are made once in tests/quantised_cases.py.  Tolerances are the project's:
fp64 bits identical and Le within 1e-9 of the oracle (same operation order); fp32 log-MAP as
test_three_workgroups_per_cu (Le within 1e-3 relative) and test_window_f32_vs_c_restatement (1e-4);
Max-Log-MAP on dyadic inputs is rounding-free, so there fp32, fp64 and the oracle agree on every bit
and every Le value."""
import os
import subprocess

import numpy as np
import pytest

import pyoracle as O
import quantised_cases as Q
import test_gpu_early_stop as ES
import test_gpu_window_stop as WS
import window_stop_cases as WC
from conftest import REPO
import test_gpu_decode as GD
import test_gpu_window as GW

pytestmark = pytest.mark.gpu

PKG = os.path.join(REPO, "turbo_decoder_cuda_amd")
K1, F1, F2 = 1024, 31, 64
WIN, OVL = 64, 30
DETECTOR_FAMILIES = ["q4", "int31", "int8", "sign"]   # the detector fires on these (not on punct: continuous values)


# the other modules' decode helpers, on a private copy of the (shared, read-only) input
def _decode_all(K, f1, f2, iters, flow, **kw):
    return GD._decode_all(K, f1, f2, iters, np.array(flow), **kw)


def _decode_bits(K, f1, f2, iters, flow, **kw):
    return GD._decode_bits(K, f1, f2, iters, np.array(flow), **kw)


def _decode_window(K, f1, f2, iters, flow, algo, window, overlap, **kw):
    return GW._decode(K, f1, f2, iters, np.array(flow), algo, window, overlap, **kw)


def assert_detector_fires(K, f1, f2, B, family, iters, precision="f64", **kw):
    total, share = Q.misses(K, f1, f2, B, family, iters, precision, **kw)
    print(f"K={K} {family} {precision}: {int(total.sum())} CPU misses, {total.tolist()}, redo share {share:.3f}")
    assert total.sum() > 0, "this input does not reach the speculation detector"
    return total


def assert_f64_equals_oracle(bits, le, rows, les, what=""):
    for b in range(rows.shape[0]):
        assert np.array_equal(bits[b], rows[b]), f"{what} codeword {b}: bits"
        assert np.abs(le[b] - les[b]).max() <= 1e-9, f"{what} codeword {b}: Le"


# ------------------------------------------------------------------ a. exact schedule, fp64 log-MAP
@pytest.mark.parametrize("le_dump", [True, False], ids=["le-dump", "fast-fold"])
@pytest.mark.parametrize("K,f1,f2,B,iters,family", [
    (1024, 31, 64, 13, 4, "q4"), (1024, 31, 64, 13, 4, "int31"), (1024, 31, 64, 13, 4, "int8"),
    (1024, 31, 64, 13, 4, "sign"), (1024, 31, 64, 13, 4, "punct"),
    (432, 47, 72, 13, 4, "q4"),          # L = 0 mod 15: the last speculated window is followed by a full one
    (88, 5, 22, 13, 4, "int31"),         # L = 1 mod 15: a one-step last window
    (6144, 263, 480, 3, 3, "q4"),        # 410 windows, hundreds of misses a codeword
])
def test_exact_f64_logmap_vs_oracle(K, f1, f2, B, iters, family, le_dump):
    """Every iteration's bits identical to the oracle's and Le within 1e-9, with the Le dump (the
    generic fold) and without it (the fast fold: bits only)."""
    if family != "punct":
        assert_detector_fires(K, f1, f2, B, family, iters)
    flow, rows, les = Q.exact_ref(K, f1, f2, B, family, iters)
    if le_dump:
        bits, le = _decode_all(K, f1, f2, iters, flow)
        assert_f64_equals_oracle(bits, le, rows, les, family)
    else:
        assert np.array_equal(_decode_bits(K, f1, f2, iters, flow), rows)


# ------------------------------------------------------------------ b. the wave-wide redo does not leak
def test_redo_of_a_neighbour_does_not_change_a_codeword():
    """A miss in any lane makes the whole wave (8 codewords) recompute the window.  16 codewords,
    continuous AWGN at the even places and q4 at the odd ones: each AWGN codeword's bits and Le are
    byte-identical to decoding it alone (where no window is recomputed), the q4 ones equal the oracle's."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    B, iters = 16, 4
    tq = assert_detector_fires(K1, F1, F2, B, "q4", iters)
    ta, _ = Q.misses(K1, F1, F2, B, "awgn", iters)
    assert np.all(tq[1::2] > 0) and ta.sum() == 0
    flow = np.array(Q.family_flow(K1, F1, F2, B, "awgn"))
    flow[1::2] = Q.family_flow(K1, F1, F2, B, "q4")[1::2]
    rows, les = Q.oracle_rows(flow, K1, F1, F2, iters)
    bits, le = _decode_all(K1, F1, F2, iters, flow)
    assert_f64_equals_oracle(bits, le, rows, les)
    x = torch.from_numpy(flow).to("cuda:0")
    with TurboCodec(K1, F1, F2, iterations=iters) as c:
        for b in range(0, B, 2):
            b1 = torch.empty((1, iters, K1), dtype=torch.uint8, device=x.device)
            l1 = torch.empty((1, iters, 2, K1 + 3), dtype=torch.float64, device=x.device)
            c.decode(x[b:b + 1].contiguous(), b1, all_iters=True, le=l1)
            torch.cuda.synchronize()
            assert b1.cpu().numpy()[0].tobytes() == bits[b].tobytes(), f"codeword {b}: bits"
            assert l1.cpu().numpy()[0].tobytes() == le[b].tobytes(), f"codeword {b}: Le"


# ------------------------------------------------------------------ c. fp32 log-MAP: committed-order cross-checks
def assert_harmful_misses(flow32, K, f1, f2, iters):
    """The wide family's condition: misses whose speculated row gives another correction than the exact
    row (pyoracle.spec_miss_turbo), which only the recomputation repairs."""
    total, _, harm = O.spec_miss_turbo(flow32, K, f1, f2, iters, harmful=True)
    print(f"K={K} wide f32: {int(total.sum())} CPU misses, harmful {harm.tolist()}")
    assert harm.sum() > 0, "no miss of this input would change a value without the recomputation"


def test_speculation_equals_redo_library_on_families(tmp_path):
    """The production library against the redo-forced one (libturbo_mi355x_redo.so, every window in
    the committed order; loaded in a fresh child through TD_LIB_PATH): bits and Le byte-identical in
    fp64 and fp32 on the K = 1024 families of (a) and on int8_q16, decoded as one batch of 6 x 13.
    The narrow families' misses run the detector, the ballot and the recomputation, but read the same
    correction from either row; int8_q16's fp32 misses do not (asserted on the CPU first), so there the
    recomputation is what makes the two libraries agree.  Against the oracle, on the narrow families:
    fp64 bit for bit (Le to 1e-9), fp32 Le within 1e-3 relative of the fp32 restatement."""
    redo = os.path.join(PKG, "libturbo_mi355x_redo.so")
    assert os.path.exists(redo), "build() makes the redo-forced library"
    fams, B, iters = DETECTOR_FAMILIES + ["punct", "int8_q16"], 13, 4
    for fam in DETECTOR_FAMILIES:
        for prec in ("f64", "f32"):
            assert_detector_fires(K1, F1, F2, B, fam, iters, prec)
    assert_harmful_misses(Q.family_flow(K1, F1, F2, B, "int8_q16").astype(np.float32), K1, F1, F2, iters)
    flow = np.concatenate([Q.family_flow(K1, F1, F2, B, fam) for fam in fams])
    np.savez(tmp_path / "in.npz", K=K1, f1=F1, f2=F2, iters=iters, flow=flow)
    subprocess.run(["python", "-c", GD._REDO_CHILD, REPO, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                   env=dict(os.environ, TD_LIB_PATH=redo), check=True, timeout=300)
    r = np.load(tmp_path / "out.npz")
    for prec in ("f64", "f32"):
        bits, le = _decode_all(K1, F1, F2, iters, flow, precision=prec)
        for k, fam in enumerate(fams):
            s = slice(k * B, (k + 1) * B)
            assert r["bits_" + prec][s].tobytes() == bits[s].tobytes(), (fam, prec)
            assert r["le_" + prec][s].tobytes() == le[s].tobytes(), (fam, prec)
            if fam == "int8_q16":   # (no tolerance of the project's is stated for |LLR| of 8e6)
                continue
            _, rows, les = Q.exact_ref(K1, F1, F2, B, fam, iters, "logmap", prec)
            if prec == "f64":
                assert_f64_equals_oracle(bits[s], le[s], rows, les, fam)
            else:
                for b in range(B):
                    d = np.abs(le[s][b] - les[b]).max()
                    assert d <= 1e-3 * max(1.0, np.abs(les[b]).max()), (fam, b, d)


@pytest.mark.parametrize("family", ["q4", "int31", "int8_q16"])
def test_speculation_equals_twelve_step_build(monkeypatch, family):
    """fp32 log-MAP at B = 6150, K = 117: four workgroups per CU run the 12-step-window build, which
    does not speculate; TD_OCC3=0 keeps the 15-step kernel, which does.  Bits and Le byte-identical,
    with the Le dump and without (int8_q16: with misses that only the recomputation repairs); on q4
    and int31 a sample equals the oracle's fp32 restatement within test_three_workgroups_per_cu's
    tolerances (the last iteration's bits on converged frames at 2.5 dB, Le within 1e-3 relative)."""
    K, f1, f2, B, iters, ebn0, seed = 117, 2, 39, 6150, 3, 2.5, 4217
    sample = list(range(0, B, 409)) + [B - 1]
    flow = Q.family_flow(K, f1, f2, B, family, ebn0, seed).astype(np.float32)
    total, _ = O.spec_miss_turbo(np.ascontiguousarray(flow[sample]), K, f1, f2, iters)
    print(f"K={K} {family} f32: CPU misses of the sample {total.tolist()}")
    assert total.sum() > 0, "this input does not reach the speculation detector"
    if family == "int8_q16":
        assert_harmful_misses(np.ascontiguousarray(flow[sample]), K, f1, f2, iters)
    monkeypatch.setenv("TD_OCC3", "0")
    bits2, le2 = _decode_all(K, f1, f2, iters, flow, precision="f32")
    fast2 = _decode_bits(K, f1, f2, iters, flow, precision="f32")
    monkeypatch.setenv("TD_OCC3", "1")
    bits4, le4 = _decode_all(K, f1, f2, iters, flow, precision="f32")
    fast4 = _decode_bits(K, f1, f2, iters, flow, precision="f32")
    assert bits2.tobytes() == bits4.tobytes()
    assert le2.tobytes() == le4.tobytes()
    assert np.array_equal(fast2, bits2) and np.array_equal(fast4, bits4)
    for b in sample if family != "int8_q16" else []:
        ob, ol = O.turbo_decode(np.ascontiguousarray(flow[b]), K, f1, f2, iters)
        assert np.array_equal(bits2[b, -1], ob[-1].astype(np.uint8)), f"codeword {b}"
        assert np.abs(le2[b] - ol).max() <= 1e-3 * max(1.0, np.abs(ol).max()), f"codeword {b}"


# ------------------------------------------------------------------ d. Max-Log-MAP on dyadic inputs, zero tolerance
def assert_equal_values(bits, le, rows, les, what):
    assert np.array_equal(bits, rows), f"{what}: bits"
    assert np.array_equal(le.astype(np.float64), les), f"{what}: Le"


@pytest.mark.parametrize("family", ["int31", "q4"])
def test_maxlog_dyadic_exact_schedule_is_rounding_free(family):
    """K = 1024, B = 13, 8 iterations: the fp32 and fp64 kernels' bits of every iteration equal the
    oracle's and their Le equal it as values, with the Le dump and without."""
    iters = 8
    flow, rows, les = Q.dyadic_maxlog_precondition(K1, F1, F2, 13, family, iters)
    for prec in ("f64", "f32"):
        bits, le = _decode_all(K1, F1, F2, iters, flow, algo="maxlog", precision=prec)
        assert_equal_values(bits, le, rows, les, prec)
        assert np.array_equal(_decode_bits(K1, F1, F2, iters, flow, algo="maxlog", precision=prec), rows), prec


@pytest.mark.parametrize("family", ["int31", "q4"])
def test_maxlog_dyadic_occupancy_variants_are_rounding_free(monkeypatch, family):
    """B = 6150 at K = 40 (769 groups): two workgroups per CU (TD_OCC3=0) and the three / four per CU
    kernels, fp64 and fp32, with the Le dump and without: all four decodes agree on every bit and every
    Le value, and a sample (every 41st codeword and the last) equals the oracle."""
    K, f1, f2, B, iters = 40, 3, 10, 6150, 8
    flow = Q.family_flow(K, f1, f2, B, family)
    sample = list(range(0, B, 41)) + [B - 1]
    rows, les = Q.maxlog_dyadic_ref(np.ascontiguousarray(flow[sample]), K, f1, f2, iters)
    ref = None
    for occ in ("0", "1"):
        monkeypatch.setenv("TD_OCC3", occ)
        for prec in ("f64", "f32"):
            bits, le = _decode_all(K, f1, f2, iters, flow, algo="maxlog", precision=prec)
            fast = _decode_bits(K, f1, f2, iters, flow, algo="maxlog", precision=prec)
            assert np.array_equal(fast, bits), (occ, prec)
            assert_equal_values(bits[sample], le[sample], rows, les, (occ, prec))
            if ref is None:
                ref = (bits, le)
            assert_equal_values(bits, le, ref[0], ref[1], (occ, prec))


@pytest.mark.parametrize("family", ["int31", "q4"])
@pytest.mark.parametrize("nii,conc", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["serial", "serial-nii", "concurrent", "concurrent-nii"])
def test_maxlog_dyadic_window_schedule_is_rounding_free(family, nii, conc):
    """The windowed schedule at W = 64, overlap 30, ext_scale 1.0, in both lane layouts (runs 0 and 3):
    fp32 and fp64 equal the C restatement on every bit and every Le value."""
    iters = 8
    flow, rows, les = Q.dyadic_maxlog_precondition(K1, F1, F2, 13, family, iters, (WIN, OVL, nii, conc))
    for run in (0, 3):
        for prec in ("f64", "f32"):
            bits, le = _decode_window(K1, F1, F2, iters, flow, "maxlog", WIN, OVL, precision=prec, nii=nii,
                                      concurrent=conc, run=run)
            assert_equal_values(bits, le, rows, les, (run, prec))


# ------------------------------------------------------------------ e. windowed log-MAP against the C restatement
WALGO = {"logmap": "logmap-q", "logmap-exact": "logmap"}   # test_gpu_window's names -> quantised_cases'


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("algo", ["logmap", "logmap-exact"])
@pytest.mark.parametrize("family", ["q4", "int31"])
def test_window_logmap_vs_c_restatement(family, algo, precision):
    """K = 1024, W = 64, overlap 30, B = 9, both max* forms (the one-read table's 8-per-octave grid and
    E_algorithm's thresholds both sit on dyadic differences): fp64 bits identical and Le within 1e-9;
    fp32 bits identical and Le within 1e-4 relative, as test_window_f32_vs_c_restatement."""
    B, iters = 9, 4
    flow, rows, les = Q.window_ref(K1, F1, F2, B, family, iters, WIN, OVL, WALGO[algo], precision)
    bits, le = _decode_window(K1, F1, F2, iters, flow, algo, WIN, OVL, precision=precision)
    for b in range(B):
        assert np.array_equal(bits[b], rows[b]), f"codeword {b}"
        tol = 1e-9 if precision == "f64" else 1e-4 * max(1.0, np.abs(les[b]).max())
        assert np.abs(le[b] - les[b]).max() <= tol, f"codeword {b}"


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("algo", ["logmap", "logmap-exact"])
def test_window_logmap_single_frame_vs_c_restatement(algo, precision):
    """A batch of one q4 codeword takes the beta kernel's lane-fold variant."""
    iters = 4
    flow, rows, les = Q.window_ref(K1, F1, F2, 9, "q4", iters, WIN, OVL, WALGO[algo], precision)
    bits, le = _decode_window(K1, F1, F2, iters, flow[4:5], algo, WIN, OVL, precision=precision)
    assert np.array_equal(bits[0], rows[4])
    tol = 1e-9 if precision == "f64" else 1e-4 * max(1.0, np.abs(les[4]).max())
    assert np.abs(le[0] - les[4]).max() <= tol


# ------------------------------------------------------------------ f. ties and erasures
ZERO_ROWS = (3, 10)


def _mixed_with_zeros():
    flow = np.array(Q.family_flow(K1, F1, F2, 11, "q4"))
    flow[list(ZERO_ROWS)] = 0.0
    return flow


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("schedule,algo", [("exact", "logmap"), ("exact", "maxlog"), ("window", "logmap"),
                                           ("window", "logmap-exact"), ("window", "maxlog")])
def test_all_zero_codeword(schedule, algo, precision):
    """A fully erased code block (every LLR 0.0: every hard decision starts from a tie) alone and
    inside a batch of q4 codewords, 4 iterations.  Its bits and Le are whatever the oracle gives (the
    exact oracle, or the windowed C restatement): fp64 bits identical and Le within 1e-9; Max-Log-MAP
    equal as values in both precisions on every codeword of the batch (dyadic input); fp32 log-MAP bits
    identical on the zero codeword (sums of table constants in the oracle's order) and Le within the
    schedule's fp32 tolerance on every codeword.  In the batch the zero codeword's bytes equal the lone
    decode's."""
    iters = 4
    flow = Q.as_precision(_mixed_with_zeros(), precision)
    if schedule == "exact":
        rows, les = Q.oracle_rows(flow, K1, F1, F2, iters, algo)
        dec = lambda f: _decode_all(K1, F1, F2, iters, f, algo=algo, precision=precision)
        rel = 2e-3 if algo == "maxlog" else 1e-3
    else:
        rows, les = Q.oracle_window_rows(flow, K1, F1, F2, iters, WIN, OVL, WALGO.get(algo, algo))
        dec = lambda f: _decode_window(K1, F1, F2, iters, f, algo, WIN, OVL, precision=precision)
        rel = 1e-4
    z = ZERO_ROWS[0]
    assert np.array_equal(rows[z], rows[ZERO_ROWS[1]]) and np.array_equal(les[z], les[ZERO_ROWS[1]])
    zb, zl = dec(np.ascontiguousarray(flow[z:z + 1]))
    bits, le = dec(flow)
    for r in ZERO_ROWS:
        assert bits[r].tobytes() == zb[0].tobytes() and le[r].tobytes() == zl[0].tobytes(), f"zero codeword {r}"
    for b in range(flow.shape[0]):
        if algo == "maxlog":
            assert_equal_values(bits[b], le[b], rows[b], les[b].astype(np.float64), f"codeword {b}")
        elif precision == "f64":
            assert np.array_equal(bits[b], rows[b]), f"codeword {b}"
            assert np.abs(le[b] - les[b]).max() <= 1e-9, f"codeword {b}"
        else:
            if b in ZERO_ROWS:
                assert np.array_equal(bits[b], rows[b]), f"zero codeword {b}"
            assert np.abs(le[b] - les[b]).max() <= rel * max(1.0, np.abs(les[b]).max()), f"codeword {b}"


# ------------------------------------------------------------------ g. early termination
STOP_B, STOP_ZERO = 19, (2, 9, 18)


def _stop_flow():
    flow = np.array(Q.family_flow(K1, F1, F2, STOP_B, "q4", 1.0, 4242))
    flow[list(STOP_ZERO)] = 0.0
    return flow


def test_hda_stop_on_quantised_batch_exact():
    """HDA rule, exact schedule, K = 1024, B = 19: q4 codewords and three all-zero ones in one batch.
    iters_used and the frozen rows are what the oracle's full-decode rows imply (the expectation
    helpers of test_gpu_early_stop.py), Le of the iterations used within 1e-9."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    flow = _stop_flow()
    total, _ = O.spec_miss_turbo(flow, K1, F1, F2, 2)
    assert total.sum() > 0, "this input does not reach the speculation detector"
    rows, les = Q.oracle_rows(flow, K1, F1, F2, ES.ITERS)
    used = ES.stops(rows, "hda")
    print("stop counts", used.tolist())
    ES.assert_not_vacuous(used)
    x = torch.tensor(flow).to("cuda:0")
    with TurboCodec(K1, F1, F2, iterations=ES.ITERS) as c:
        c.set_early_stop("hda")
        ES.check_against(c, x, rows, used, les)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_hda_stop_on_quantised_batch_window(precision):
    """The same batch under the windowed schedule (W = 64, overlap 30: window_stop_cases' schedule D)
    against the C restatement's rows, fp64 and fp32 (test_gpu_window_stop.py's helpers and tolerances)."""
    import torch
    assert WC.SCHED["D"] == (K1, F1, F2, WIN, OVL, False, False, 1.0) and WC.ITERS == ES.ITERS
    flow = Q.as_precision(_stop_flow(), precision)
    rows, les = Q.oracle_window_rows(flow, K1, F1, F2, WC.ITERS, WIN, OVL, "logmap-q")
    used = WC.stops(rows, "hda")
    print("stop counts", used.tolist())
    assert len(set(used.tolist())) >= 3
    with WS.codec("D", "logmap", precision) as c:
        c.set_window_early_stop("hda")
        WS.check_against(c, torch.tensor(flow).to("cuda:0"), rows, used, les)


# ------------------------------------------------------------------ h. td_siso_host
@pytest.mark.parametrize("terminated", [1, 0])
@pytest.mark.parametrize("L", [43, 1027])
@pytest.mark.parametrize("algo", ["logmap", "maxlog"])
def test_siso_host_on_quantised_input(algo, L, terminated):
    """The standalone SISO (Log_MAP_decoder) in fp64 on q4 channel values and a q8 a-priori with exact
    zeros: every LLR bit for bit the oracle's O.siso."""
    from turbo_decoder_cuda_amd import TurboCodec
    flow = Q.family_flow(K1, F1, F2, 9, "q4")
    recs = np.ascontiguousarray(0.5 * flow[1, :2 * L])
    La = np.array(Q.family_flow(K1, F1, F2, 9, "q8")[2, :L])
    La[::7] = 0.0
    if algo == "logmap" and L > 30:
        n, _, _ = O.spec_miss_siso(recs, La)
        print(f"L={L}: {n} CPU misses")
        assert L < 1027 or n > 0
    with TurboCodec(L - 3, 1, 0, iterations=1, algo=algo) as c:
        llr = c.Log_MAP_decoder(recs, La, terminated)
    ref = O.siso(recs, La, terminated, algo=Q.OALGO[algo])
    print("max |dLLR|", np.abs(llr - ref).max())
    assert llr.tobytes() == ref.tobytes()
