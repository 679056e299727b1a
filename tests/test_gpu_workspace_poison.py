"""No decode may depend on what its workspace held before it.

The library never initialises its scratch (td_api.cpp: ensure_ws, ensure_fixed_ws, ensure_wws, the staging
buffers), and in every other test a fresh allocation is zeros or the harmless leftovers of the previous
handle.  Here td_debug_workspace_fill (TurboCodec.debug_fill_workspace) fills every scratch buffer of a handle
before each decode, with three bytes in turn:

  0xFF  NaN as f64 / f32, -1 as any integer
  0x7F  1.4e306 / 3.4e38: finite and larger than any metric; 127 / 32639 as int8 / int16
  0xFE  -5e303 / -1.7e38; -2 / -258

and the outputs, themselves pre-filled with sentinels (bits 7, Le NaN or 12345, counts -1), must (a) equal the
schedule's reference to the standard of that schedule's own test, (b) be byte-identical across the three
fills, (c) hold no sentinel where the schedule defines them (the Le rows after a codeword's stop are
unspecified), and (d) the call must report at least workspace_bytes() written, more on a windowed float handle.
The references are the oracles and restatements of the other tests (pyoracle, fixed_ref, fixed_window_ref,
fixed_window_nii_ref, fixed_maxstar_ref), computed once per case on a few codewords: a codeword's result does
not depend on its batch, so the batches are those codewords tiled.  The last two tests use no hook: one handle
goes through its schedules and batch sizes in turn, each decode on fresh input, over whatever the previous
one left behind."""
import functools

import numpy as np
import pytest

import fixed_maxstar_ref as FM
import fixed_ref as F
import fixed_stop_cases as S
import fixed_window_nii_ref as FN
import fixed_window_ref as FW
import pyoracle as O
import window_stop_cases as W
from conftest import gpu_available
from test_gpu_decode import WINDOW_EDGE_SIZES

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

FILLS = (0xFF, 0x7F, 0xFE)
BITS_SENTINEL, LE_SENTINEL_INT, ITERS_SENTINEL = 7, 12345, -1
OALGO = {"logmap": O.ALGO_LOGMAP, "maxlog": O.ALGO_MAXLOG}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _x(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # a copy: the references are read-only


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _outputs(c, B, all_iters=True, le=True, iters=True):
    """Output tensors of one decode, pre-filled with the sentinels."""
    import torch
    le_dt = c._torch_dtypes()[1]
    bits = torch.full((B, c.iterations, c.K) if all_iters else (B, c.K), BITS_SENTINEL, dtype=torch.uint8, device=_dev())
    led = None
    if le:
        led = torch.full((B, c.iterations, 2, c.L), LE_SENTINEL_INT if le_dt == torch.int16 else float("nan"),
                         dtype=le_dt, device=_dev())
    n = torch.full((B,), ITERS_SENTINEL, dtype=torch.int32, device=_dev()) if iters else None
    return bits, led, n


def _decode(c, x, all_iters=True, le=True):
    import torch
    bits, led, n = _outputs(c, x.shape[0], all_iters, le)
    c.decode(x, bits, all_iters=all_iters, le=led, iters_out=n)
    torch.cuda.synchronize()
    return bits, led, n


def _same_bytes(a, b):
    import torch
    if a is None or b is None:
        return a is b
    if isinstance(a, np.ndarray):
        return a.tobytes() == b.tobytes()
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))   # NaNs compare as bytes


def _poisoned(c, decode, windowed=False):
    """decode() after each fill: (d) and (b) asserted here; -> the first fill's outputs."""
    outs = []
    for byte in FILLS:
        filled = c.debug_fill_workspace(byte)
        ws = c.workspace_bytes()
        assert ws > 0 and filled >= ws, (hex(byte), filled, ws)
        if windowed:
            assert filled > ws, (hex(byte), filled, ws)
        outs.append(decode())
    c.debug_fill_workspace(-1)
    for byte, o in zip(FILLS[1:], outs[1:]):
        for k, (a, b) in enumerate(zip(outs[0], o)):
            assert _same_bytes(a, b), f"output {k} after fill {byte:#x} differs from the one after {FILLS[0]:#x}"
    return outs[0]


def _np(out):
    return tuple(None if t is None else (t if isinstance(t, np.ndarray) else t.cpu().numpy()) for t in out)


def _no_sentinel(bits, le, n, used=None):
    """(c).  With a rule the Le of iterations after a codeword's stop is unspecified (fixed_stop_cases.le_mask)."""
    assert not (bits == BITS_SENTINEL).any(), "a decision byte was never written"
    assert bits.max() <= 1
    if n is not None:
        assert not (n == ITERS_SENTINEL).any(), "a count was never written"
    if le is not None:
        mask = np.ones(le.shape[:2], dtype=bool) if used is None else np.arange(le.shape[1])[None, :] < used[:, None]
        v = le[mask]
        bad = np.isnan(v) if le.dtype.kind == "f" else v == LE_SENTINEL_INT
        assert not bad.any(), "an Le entry the decode defines was never written (or is NaN)"


# ================================================================== the float decoders
def _flow(K, f1, f2, ebn0, seed, B, precision):
    flow = O.synth_batch(K, f1, f2, ebn0, seed, B)[1]
    return flow.astype(np.float32) if precision == "f32" else flow


def _check_float_exact(got, flow, K, f1, f2, iters, algo, precision, sample=None):
    """(a) to test_gpu_decode.py's standard (test_window_edge_residues_vs_oracle): fp64 bits identical and Le
    within 1e-9; fp32 against the oracle's fp32 restatement, Max-Log-MAP bits identical, log-MAP bits
    identical at the last iteration (converged frames), Le within 2e-3 / 1e-3 relative."""
    bits, le, n = got
    assert (n == iters).all()
    for b in (range(flow.shape[0]) if sample is None else sample):
        ob, ol = O.turbo_decode(np.ascontiguousarray(flow[b]), K, f1, f2, iters, algo=OALGO[algo])
        if precision == "f64":
            assert np.array_equal(bits[b], ob.astype(np.uint8)), f"codeword {b}"
            d = np.abs(le[b] - ol).max()
            assert d <= 1e-9, f"codeword {b}: {d:g}"
            continue
        if algo == "maxlog":
            assert np.array_equal(bits[b], ob.astype(np.uint8)), f"codeword {b}"
        else:
            assert np.array_equal(bits[b, -1], ob[-1].astype(np.uint8)), f"codeword {b}"
        tol = 2e-3 if algo == "maxlog" else 1e-3
        d = np.abs(le[b] - ol).max()
        assert d <= tol * max(1.0, np.abs(ol).max()), f"codeword {b}: {d:g}"


# K = 40 (L = 43: three windows, the last 13 steps) and K = 1024 (L = 1027: 69 windows, the last 7 steps);
# K = 72 and 88 of WINDOW_EDGE_SIZES: a full last window (the B pass reads row L of the alpha scratch) and a
# one-step one.  B = 1 and 13: seven and three codewords of padding in the last group of 8.
EXACT_SHAPES = [(40, 3, 10, 1), (40, 3, 10, 13), (1024, 31, 64, 13), WINDOW_EDGE_SIZES[0] + (13,), WINDOW_EDGE_SIZES[1] + (13,)]


@pytest.mark.parametrize("K,f1,f2,B", EXACT_SHAPES)
@pytest.mark.parametrize("algo", ["logmap", "maxlog"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_exact_float(K, f1, f2, B, algo, precision):
    from turbo_decoder_cuda_amd import TurboCodec
    iters = 4
    flow = _flow(K, f1, f2, 0.4 if precision == "f64" else 1.5, 1300 + K, B, precision)
    x = _x(flow)
    with TurboCodec(K, f1, f2, iterations=iters, algo=algo, precision=precision) as c:
        c.reserve(B)
        got = _np(_poisoned(c, lambda: _decode(c, x)))
        fast = _np(_poisoned(c, lambda: _decode(c, x, le=False)))   # without an Le dump: the folds' fast path
    _no_sentinel(*got)
    _no_sentinel(*fast)
    assert np.array_equal(fast[0], got[0])
    _check_float_exact(got, flow, K, f1, f2, iters, algo, precision)


@pytest.mark.parametrize("algo", ["logmap", "maxlog"])
def test_exact_float_three_workgroups_per_cu(monkeypatch, algo):
    """test_gpu_decode.py's test_three_workgroups_per_cu set-up (TD_OCC3, fp32, K = 40, B = 5000: 625 groups).
    reserve(5000) runs the placement search, so the workspace is the candidate it kept, filled on the way."""
    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, B, iters = 40, 3, 10, 5000, 3
    monkeypatch.setenv("TD_OCC3", "1")
    flow = _flow(K, f1, f2, 0.3 if algo == "maxlog" else 1.0, 31, B, "f32")
    x = _x(flow)
    with TurboCodec(K, f1, f2, iterations=iters, algo=algo, precision="f32") as c:
        c.debug_fill_workspace(FILLS[0])   # armed before the workspace exists: reserve fills what it keeps
        c.reserve(B)
        got = _np(_poisoned(c, lambda: _decode(c, x)))
    _no_sentinel(*got)
    _check_float_exact(got, flow, K, f1, f2, iters, algo, "f32", sample=list(range(0, B, 41)) + [B - 1])


@pytest.mark.parametrize("rule", ["hda", "crc"])
def test_exact_float_early_stop(rule):
    """td_set_early_stop on test_gpu_early_stop.py's frames (K = 40, B = 19: a ragged last group)."""
    import test_gpu_early_stop as ES
    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, B = 40, 3, 10, 19
    if rule == "hda":
        flow, rows, les = ES.synth_case(K, f1, f2, 1.0, B, "logmap")
    else:
        flow, rows = ES.crc_case(K, f1, f2, ES.CRC24B, 1.2, B)
        les = None
    used = ES.stops(rows, rule)
    ES.assert_not_vacuous(used)
    x = _x(flow)
    with TurboCodec(K, f1, f2, iterations=ES.ITERS) as c:
        c.set_early_stop(rule)
        c.reserve(B)
        bits, le, n = _np(_poisoned(c, lambda: _decode(c, x)))
        last = _np(_poisoned(c, lambda: _decode(c, x, all_iters=False, le=False)))
    _no_sentinel(bits, le, n, used)
    _no_sentinel(*last)
    assert np.array_equal(n, used) and np.array_equal(last[2], used)
    assert np.array_equal(bits, ES.frozen(rows, used))
    assert np.array_equal(last[0], rows[np.arange(B), used - 1])
    if les is not None:
        for b in range(B):
            assert np.abs(le[b, :used[b]] - les[b, :used[b]]).max() <= 1e-9, f"codeword {b}"


@pytest.mark.parametrize("terminated", [0, 1])
@pytest.mark.parametrize("algo,precision", [("maxlog", "f64"), ("maxlog", "f32"), ("logmap", "f64")])
def test_bare_siso(terminated, algo, precision):
    """Log_MAP_decoder allocates its scratch per call: armed, every call's is filled.  test_gpu_parity.py's
    Max-Log-MAP case (L = 1027) and its tolerance; log-MAP in fp64 to the oracle's 1e-9 (the same operations
    in the same order, as test_siso_vs_reference and smoke())."""
    from turbo_decoder_cuda_amd import TurboCodec
    rng = np.random.default_rng(11 + terminated)
    L = 1027
    recs, La = rng.normal(0.0, 2.0, 2 * L), rng.normal(0.0, 3.0, L)
    with TurboCodec(L - 3, 1, 0, 1, algo=algo, precision=precision) as c:
        recs, La = recs.astype(c.dtype), La.astype(c.dtype)
        ref = O.siso(recs.astype(np.float64), La.astype(np.float64), terminated, algo=OALGO[algo])
        outs = []
        for byte in FILLS:
            c.debug_fill_workspace(byte)
            outs.append(c.Log_MAP_decoder(recs, La, terminated))
    tol = 1e-9 if precision == "f64" else 1e-3 * max(1.0, float(np.abs(ref).max()))
    for o in outs:
        assert o.tobytes() == outs[0].tobytes()
    assert not np.isnan(outs[0]).any() and np.abs(outs[0] - ref).max() <= tol


def test_host_entry_staging():
    """TurboDecoding (td_decode_host) with B = 1, 5, 1: armed, the staging buffers are filled as they are
    allocated and as they grow, and the third call decodes one frame in buffers sized for five."""
    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, iters = 1024, 31, 64, 3
    flow = _flow(K, f1, f2, 0.4, 77, 7, "f64")
    with TurboCodec(K, f1, f2, iterations=iters) as c:
        for byte in FILLS:
            filled = c.debug_fill_workspace(byte)
            for rows in (slice(0, 1), slice(1, 6), slice(6, 7)):
                out, le, n = c.TurboDecoding(flow[rows], return_le=True, return_iters=True)
                assert (n == iters).all() and not np.isnan(le).any()
                for k, b in enumerate(range(rows.start, rows.stop)):
                    ob, ol = O.turbo_decode(flow[b], K, f1, f2, iters)
                    assert np.array_equal(out[k], ob), (hex(byte), b)
                    assert np.abs(le[k] - ol).max() <= 1e-9, (hex(byte), b)
            if byte != FILLS[0]:   # the staging buffers exist by now and are scratch too
                assert filled > c.workspace_bytes()


# ------------------------------------------------------------------ the windowed schedule
WALGO = {"logmap": O.ALGO_LOGMAP_Q, "logmap-exact": O.ALGO_LOGMAP, "maxlog": O.ALGO_MAXLOG}


def _window_codec(K, f1, f2, iters, algo, precision, W_, g, scale=1.0, nii=False, conc=False, run=0):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, f1, f2, iterations=iters, algo=algo.split("-")[0], precision=precision)
    c.debug_window_layout(run)
    c.set_window_maxstar(algo == "logmap-exact")
    c.set_window(W_, g, scale, nii=nii, concurrent=conc)
    return c


def _check_window(got, flow, K, f1, f2, iters, algo, W_, g, scale=1.0, nii=False, conc=False, sample=None,
                  last_only=False):
    """(a) to test_gpu_window.py's standard: bits identical to the C restatement, Le within 1e-9 (fp64) or
    1e-4 relative (fp32)."""
    bits, le, n = got
    assert n is None or (n == iters).all()
    for b in (range(flow.shape[0]) if sample is None else sample):
        ob, ol = O.turbo_decode_window(flow[b], K, f1, f2, iters, W_, g, algo=WALGO[algo], nii=nii, concurrent=conc,
                                       scale=scale)
        assert np.array_equal(bits[b], ob[-1] if last_only else ob), f"codeword {b}"
        tol = 1e-9 if flow.dtype == np.float64 else 1e-4 * max(1.0, np.abs(ol).max())
        d = np.abs(le[b] - ol).max()
        assert d <= tol, f"codeword {b}: {d:g}"


# K = 512 at {64, 30}: eight sub-blocks, the last 67 long.  B = 1: the lane-fold kernels and the beta hand-over
# through a checkpoint slot; B = 9 and 65: 55 and 63 lanes of padding, one wave and two.
@pytest.mark.parametrize("B", [1, 9, 65])
@pytest.mark.parametrize("algo,precision,scale,nii,conc,g,run", [
    ("logmap", "f64", 1.0, False, False, 30, 0),
    ("logmap-exact", "f64", 1.0, False, False, 30, 0),
    ("maxlog", "f32", 1.0, False, False, 30, 0),
    ("maxlog", "f32", 0.77, True, True, 0, 0),     # the NII state and the second extrinsic pair
    ("maxlog", "f64", 0.77, True, True, 0, 0),
    ("logmap", "f64", 1.0, False, False, 30, 1),   # td_debug_window_layout: one sub-block a lane
    ("logmap", "f64", 1.0, False, False, 30, 4),   # runs of four
    ("maxlog", "f32", 0.77, True, True, 0, 4),
])
def test_window_float(B, algo, precision, scale, nii, conc, g, run):
    K, f1, f2, iters, W_ = 512, 31, 64, 3, 64
    flow = _flow(K, f1, f2, 0.4, 500 + B, B, precision)
    x = _x(flow)
    with _window_codec(K, f1, f2, iters, algo, precision, W_, g, scale, nii, conc, run) as c:
        c.reserve(B)
        got = _np(_poisoned(c, lambda: _decode(c, x), windowed=True))
        last = _np(_poisoned(c, lambda: _decode(c, x, all_iters=False, le=False), windowed=True))
    _no_sentinel(*got)
    _no_sentinel(*last)
    assert np.array_equal(last[0], got[0][:, -1])
    _check_window(got, flow, K, f1, f2, iters, algo, W_, g, scale, nii, conc)


def test_window_float_two_parts():
    """B = 2 * 64 * 64 + 5 (129 waves: two batch parts on two streams), tiled from 64 frames, as
    test_gpu_handle.py's test_graph_capture_windowed_two_streams; sampled codewords of both parts against the C
    restatement.  The parts need a decode of the last iteration's bits only."""
    K, f1, f2, iters, W_, g = 512, 31, 64, 3, 64, 30
    B = 2 * 64 * 64 + 5
    flow = np.ascontiguousarray(np.tile(O.synth_batch(K, f1, f2, 0.3, 900, 64)[1], (B // 64 + 1, 1))[:B])
    x = _x(flow)
    sample = (0, 63, 64 * 64 + 5, B - 6, B - 1)
    with _window_codec(K, f1, f2, iters, "logmap", "f64", W_, g) as c:
        c.reserve(B)
        bits, le, n = _poisoned(c, lambda: _decode(c, x, all_iters=False), windowed=True)
        assert not bool((bits == BITS_SENTINEL).any()) and not bool(le.isnan().any()) and bool((n == iters).all())
        idx = _x(np.array(sample))
        got = (bits[idx].cpu().numpy(), le[idx].cpu().numpy(), None)
    _check_window(got, flow[list(sample)], K, f1, f2, iters, "logmap", W_, g, last_only=True)


@pytest.mark.parametrize("rule,sched,arg,B", [("hda", "D", 1.0, 19), ("hda", "A", 0.0, 70), ("crc", "D", 1.1, 19),
                                              ("crc", "A", 1.2, 70)])
def test_window_float_early_stop(rule, sched, arg, B):
    """td_set_window_stop on test_gpu_window_stop.py's frames: schedule D (K = 1024, {64, 30}) and A (K = 40)."""
    import test_gpu_window_stop as WS
    flow, rows, les = W.synth_case(sched, arg, B) if rule == "hda" else W.crc_case(sched, W.CRC24B, arg, B)
    used = W.stops(rows, rule)
    assert len(set(used.tolist())) >= 3
    x = _x(flow)
    with WS.codec(sched) as c:
        c.set_window_early_stop(rule)
        c.reserve(B)
        bits, le, n = _np(_poisoned(c, lambda: _decode(c, x), windowed=True))
        last = _np(_poisoned(c, lambda: _decode(c, x, all_iters=False, le=False), windowed=True))
        one = _np(_poisoned(c, lambda: _decode(c, x[:1]), windowed=True))   # B = 1: decisions straight to the caller's rows
    _no_sentinel(bits, le, n, used)
    _no_sentinel(*last)
    _no_sentinel(*one, used=used[:1])
    assert np.array_equal(n, used) and np.array_equal(last[2], used) and one[2][0] == used[0]
    assert np.array_equal(bits, W.frozen(rows, used)) and np.array_equal(one[0], W.frozen(rows[:1], used[:1]))
    assert np.array_equal(last[0], rows[np.arange(B), used - 1])
    for b in range(B):
        assert np.abs(le[b, :used[b]] - les[b, :used[b]]).max() <= 1e-9, f"codeword {b}"
    assert np.abs(one[1][0, :used[0]] - les[0, :used[0]]).max() <= 1e-9


# ================================================================== the fixed-point decoder
FX_ITERS, FX_B = 4, 65


@functools.lru_cache(maxsize=None)
def _fixed_unique(K):
    """fixed_stop_cases' mixed batch: AWGN frames, frames carrying gCRC24B, zeros, +127, -128, random bytes."""
    return _ro(np.ascontiguousarray(S._host_batch(K)))[0]


@functools.lru_cache(maxsize=None)
def _fixed_ref(K, kind, win, table):
    """(rows, Le) of _fixed_unique(K) on the exact schedule, the sub-block schedule `win` or that with NII; with
    the default table and set_fixed(255, 4), or the plain max and (255, 3)."""
    q, qpp = _fixed_unique(K), S.QPP[K]
    tab, setting = (FM.DEFAULT, (255, 4)) if table else (None, (255, 3))
    if kind == "nii":
        rows, le = FN.decode(q, K, *qpp, FX_ITERS, *win, tab, *setting)
    elif table:
        rows, le = FM.decode(q, K, *qpp, FX_ITERS, tab, *setting, win=win if kind == "win" else None)[:2]
    elif kind == "win":
        rows, le = FW.decode(q, K, *qpp, FX_ITERS, *win, *setting)
    else:
        rows, le = F.decode(q, K, *qpp, FX_ITERS, *setting)[:2]
    return _ro(rows, le)


FX_SCHEDULES = [("exact", None), ("win", (64, 48)), ("win", (16, 16)), ("nii", (64, 32)), ("nii", (16, 16))]


def _fixed_codec(K, kind, win, rule, table, iters=FX_ITERS):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *S.QPP[K], iterations=iters, algo="maxlog", precision="fixed")
    _fixed_schedule(c, kind, win, rule, table)
    return c


def _fixed_schedule(c, kind, win, rule, table):
    """From any earlier schedule: rules off first (a rule of one kind excludes the other schedule)."""
    c.set_fixed_early_stop(None)
    if c._fixed_window[0]:
        c.set_fixed_window_early_stop(None)
    c.set_fixed_maxstar() if table else c.set_fixed_maxstar(None)
    c.set_fixed(255, 4 if table else 3)
    if kind == "exact":
        c.set_fixed_window(0)
        c.set_fixed_early_stop(rule)
    else:
        c.set_fixed_window(*win, nii=kind == "nii")
        c.set_fixed_window_early_stop(rule)


def _check_fixed(got, rows, le, rule, iters=FX_ITERS):
    """(a): bit for bit, as every fixed test; with a rule the frozen rows, the counts and Le up to the stop."""
    g_bits, g_le, g_n = got
    used = W.stops(rows, rule) if rule else np.full(rows.shape[0], iters, dtype=np.int32)
    _no_sentinel(g_bits, g_le, g_n, used)
    assert np.array_equal(g_n, used), (W.spread(g_n), W.spread(used))
    assert np.array_equal(g_bits, W.frozen(rows, used))
    mask = S.le_mask(used, iters)
    assert np.array_equal(np.where(mask, g_le, 0), np.where(mask, le, 0))
    return used


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("rule", [None, "hda", "crc"])
@pytest.mark.parametrize("kind,win", FX_SCHEDULES)
@pytest.mark.parametrize("K", [40, 1024])
def test_fixed(K, kind, win, rule, table):
    """B = 65: one full wave and one lane, 63 lanes of padding.  K = 40 under {64, .}: one sub-block."""
    rows, le = _fixed_ref(K, kind, win, table)
    u = _fixed_unique(K)
    idx = np.arange(FX_B) % u.shape[0]
    x = _x(u[idx])
    with _fixed_codec(K, kind, win, rule, table) as c:
        c.reserve(FX_B)
        got = _np(_poisoned(c, lambda: _decode(c, x)))
        last = _np(_poisoned(c, lambda: _decode(c, x, all_iters=False, le=False)))
    used = _check_fixed(got, rows[idx], le[idx], rule)
    if rule:
        print(W.spread(used))
    _no_sentinel(*last)
    assert np.array_equal(last[0], rows[idx][np.arange(FX_B), used - 1]) and np.array_equal(last[2], used)


# ================================================================== stale state, no hook
def _stale_float_ref(flow, K, f1, f2, iters, algo, window):
    if window:
        fn = lambda f: O.turbo_decode_window(f, K, f1, f2, iters, *window, algo=WALGO[algo])   # noqa: E731
    else:
        fn = lambda f: O.turbo_decode(np.ascontiguousarray(f), K, f1, f2, iters, algo=OALGO[algo])   # noqa: E731
    rows, les = zip(*(fn(f) for f in flow))
    return np.array(rows).astype(np.uint8), np.array(les)


@pytest.mark.parametrize("precision,algo", [("f64", "logmap"), ("f32", "maxlog")])
def test_stale_state_float(precision, algo):
    """One handle: exact at B = 65 and 5, {64, 30} at 65 and 9, exact again at 13, HDA at 13, the rule off at
    13 -- every decode on frames of its own and against its own reference, over the previous decode's
    leftovers (a larger batch's, the other schedule's, a stopped decode's frozen state)."""
    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, iters, win = 1024, 31, 64, 4, (64, 30)
    steps = [("exact", 65, None), ("exact", 5, None), ("window", 65, None), ("window", 9, None), ("exact", 13, None),
             ("exact", 13, "hda"), ("exact", 13, None)]
    with TurboCodec(K, f1, f2, iterations=iters, algo=algo, precision=precision) as c:
        for k, (sched, B, rule) in enumerate(steps):
            flow = _flow(K, f1, f2, 1.0, 7000 + k, B, precision)
            if sched == "window":
                c.set_window(*win)
            else:
                c.set_window(0)
                c.set_early_stop(rule)
            bits, le, n = _np(_decode(c, _x(flow)))
            rows, les = _stale_float_ref(flow, K, f1, f2, iters, algo, win if sched == "window" else None)
            used = W.stops(rows, rule) if rule else np.full(B, iters, dtype=np.int32)
            _no_sentinel(bits, le, n, used)
            assert np.array_equal(n, used), (k, n.tolist(), used.tolist())
            assert np.array_equal(bits, W.frozen(rows, used)), k
            for b in range(B):   # the tolerances of test_gpu_decode.py (exact) and test_gpu_window.py (windowed)
                rel = (1e-4 if sched == "window" else 2e-3) * max(1.0, np.abs(les[b]).max())
                d = np.abs(le[b, :used[b]] - les[b, :used[b]]).max()
                assert d <= (1e-9 if precision == "f64" else rel), (k, b, d)


@functools.lru_cache(maxsize=None)
def _stale_fixed_unique(K, k):
    """Ten codewords of step k: AWGN frames of its own seed, frames carrying gCRC24B, random bytes of its own."""
    n = 3 * K + 12
    return _ro(np.ascontiguousarray(np.concatenate([
        S._awgn(K, 1.0, 4, 8, 100 + k), S._crc(K, 1.0, 3, 8),
        np.random.default_rng(1000 + k).integers(-128, 128, (3, n)).astype(np.int8)])))[0]


def test_stale_state_fixed():
    """One fixed handle: exact at B = 130 and 3; {64, 32} with NII (and reserve) at 130 and 3; NII off at 65;
    the window's HDA at 65; the exact schedule at 65; its CRC at 65; the table at 65."""
    K, iters = 1024, FX_ITERS
    steps = [("exact", None, None, False, 130), ("exact", None, None, False, 3), ("nii", (64, 32), None, False, 130),
             ("nii", (64, 32), None, False, 3), ("win", (64, 32), None, False, 65), ("win", (64, 32), "hda", False, 65),
             ("exact", None, None, False, 65), ("exact", None, "crc", False, 65), ("exact", None, "crc", True, 65)]
    with _fixed_codec(K, "exact", None, None, False, iters) as c:
        for k, (kind, win, rule, table, B) in enumerate(steps):
            u = _stale_fixed_unique(K, k)
            tab, setting = (FM.DEFAULT, (255, 4)) if table else (None, (255, 3))
            if kind == "nii":
                rows, le = FN.decode(u, K, *S.QPP[K], iters, *win, tab, *setting)
            elif table:
                rows, le = FM.decode(u, K, *S.QPP[K], iters, tab, *setting)[:2]
            elif kind == "win":
                rows, le = FW.decode(u, K, *S.QPP[K], iters, *win, *setting)
            else:
                rows, le = F.decode(u, K, *S.QPP[K], iters, *setting)[:2]
            idx = (np.arange(B) * 3 + k) % u.shape[0]
            _fixed_schedule(c, kind, win, rule, table)
            if kind == "nii":
                c.reserve(B)   # the NII state is part of the workspace only while it is on
            _check_fixed(_np(_decode(c, _x(u[idx]))), rows[idx], le[idx], rule, iters)
