"""Per-codeword early termination of the windowed schedule (td_set_window_stop) on the MI355X.

Expected values: pyoracle.turbo_decode_window's per-iteration rows pushed through the numpy statement
of the two rules (tests/window_stop_cases.py; tests/test_window_stop_oracle.py shows on the CPU that
the cases are not vacuous).  Counts must equal the rule's, bits row(n) or the frozen rows, and Le of
the iterations <= n the oracle's within test_gpu_window.py's tolerances (1e-9 in fp64, 1e-4 relative
in fp32).  Every case is checked on the three ways a decode writes its decisions: the final row only,
all_iters, and all_iters with an Le dump."""
import os
import subprocess

import numpy as np
import pytest

import window_stop_cases as W
from conftest import REPO, gpu_available
from window_stop_cases import CRC24A, CRC24B, ITERS, SCHED, frozen, stops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

PKG = os.path.join(REPO, "turbo_decoder_cuda_amd")


def _dev():
    import torch
    return torch.device("cuda", 0)


def codec(sched, algo="logmap", precision="f64", run=0, run_a=0, parts=0, iters=ITERS):
    """A windowed TurboCodec with SCHED[sched]'s schedule and no rule yet."""
    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, Wn, g, nii, conc, scale = SCHED[sched]
    c = TurboCodec(K, f1, f2, iterations=iters, algo=algo.split("-")[0], precision=precision)
    c.debug_window_layout(run, run_a, parts)
    c.set_window_maxstar(algo == "logmap-exact")
    c.set_window(Wn, g, scale, nii=nii, concurrent=conc)
    return c


def run(c, x, all_iters=False, le=False):
    """One decode with the counts: (bits, iters_used[, le]) as numpy."""
    import torch
    B = x.shape[0]
    led = torch.empty((B, c.iterations, 2, c.L), dtype=x.dtype, device=x.device) if le else None
    bits, used = c.decode(x, all_iters=all_iters, le=led, iters_out=True)
    torch.cuda.synchronize()
    res = (bits.cpu().numpy(), used.cpu().numpy())
    return res + (led.cpu().numpy(),) if le else res


def check_against(c, x, rows, used, les=None):
    B = rows.shape[0]
    stop_rows = rows[np.arange(B), used - 1]
    bits, n = run(c, x)
    print("counts", W.spread(n), "expected", W.spread(used))
    assert np.array_equal(n, used), (n.tolist(), used.tolist())
    assert np.array_equal(bits, stop_rows)
    bits, n = run(c, x, all_iters=True)
    assert np.array_equal(n, used), (n.tolist(), used.tolist())
    assert np.array_equal(bits, frozen(rows, used))
    bits, n, le = run(c, x, all_iters=True, le=True)
    assert np.array_equal(n, used), (n.tolist(), used.tolist())
    assert np.array_equal(bits, frozen(rows, used))
    if les is not None:
        f32 = les.dtype == np.float32
        for b in range(B):
            ol = les[b, :used[b]]
            tol = 1e-4 * max(1.0, np.abs(ol).max()) if f32 else 1e-9
            d = np.abs(le[b, :used[b]] - ol).max()
            assert d <= tol, f"codeword {b}: Le differs by {d:g} within its {used[b]} iterations"


def _x(flow):
    import torch
    return torch.tensor(flow).to(_dev())


# ------------------------------------------------------------------ 1. cases A-D, HDA and CRC
@pytest.mark.parametrize("sched,ebn0,B,algo,precision,run_", [
    ("A", 0.0, 70, "logmap", "f64", 0),
    ("A", 0.0, 70, "logmap-exact", "f64", 0),
    ("A", 0.0, 70, "maxlog", "f64", 0),
    ("A", 0.0, 70, "logmap", "f32", 0),
    ("B", 0.0, 70, "logmap", "f64", 0),
    ("C", 0.5, 70, "logmap", "f64", 0),
    ("C", 0.5, 70, "logmap", "f64", 2),
    ("D", 1.0, 19, "logmap", "f64", 0),
    ("D", 0.5, 19, "logmap", "f64", 5),
    ("D", 1.0, 19, "logmap", "f32", 0),
    ("D", 1.0, 19, "logmap", "f32", 5),
])
def test_hda(sched, ebn0, B, algo, precision, run_):
    flow, rows, les = W.synth_case(sched, ebn0, B, algo, precision)
    used = stops(rows, "hda")
    assert len(set(used.tolist())) >= 3
    with codec(sched, algo, precision, run=run_) as c:
        c.set_window_early_stop("hda")
        check_against(c, _x(flow), rows, used, les)


@pytest.mark.parametrize("min_iters", [1, 4, 8])
def test_hda_min_iters(min_iters):
    flow, rows, les = W.synth_case("A", 0.0, 70)
    used = stops(rows, "hda", min_iters)
    x = _x(flow)
    with codec("A") as c:
        off = c.decode(x, all_iters=True).cpu().numpy()
        assert np.array_equal(off, rows)
        c.set_window_early_stop("hda", min_iters=min_iters)
        check_against(c, x, rows, used, les)
        if min_iters == ITERS:   # the full decode exactly
            assert np.all(used == ITERS)
            bits, n = run(c, x, all_iters=True)
            assert bits.tobytes() == off.tobytes() and np.all(n == ITERS)


@pytest.mark.parametrize("sched,poly,sigma,B", [("A", CRC24B, 1.2, 70), ("A", CRC24A, 1.2, 70), ("D", CRC24B, 1.1, 19)])
def test_crc(sched, poly, sigma, B):
    flow, rows, les = W.crc_case(sched, poly, sigma, B)
    used = stops(rows, "crc", poly=poly)
    assert len(set(used.tolist())) >= 3
    x = _x(flow)
    with codec(sched) as c:
        c.set_window_early_stop("crc", crc_poly=poly)
        check_against(c, x, rows, used, les)
        c.set_window_early_stop("crc", min_iters=3, crc_poly=poly)
        check_against(c, x, rows, stops(rows, "crc", 3, poly), les)


# ------------------------------------------------------------------ 2. config 5's schedule in lane runs
def test_hda_case_e_in_runs():
    flow, rows, les = W.synth_case("E", 1.0, 9)
    used = stops(rows, "hda")
    assert set(used.tolist()) == {4, 5}
    with codec("E", run=7) as c:
        c.set_window_early_stop("hda")
        check_against(c, _x(flow), rows, used, les)


# ------------------------------------------------------------------ 3. batches of one codeword
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("sched,full,frames", [("D", 19, 6), ("Dn", 19, 6), ("E", 9, 2)])
def test_single_frames(sched, full, frames, precision):
    """One frame per call on one handle: the lane-fold kernels (with and without the beta warm-up in the
    alpha kernel), decisions straight into the caller's row, the rows after the stop filled in."""
    flow, rows, les = W.synth_case(sched, 1.0, full, "logmap", precision)
    used = stops(rows, "hda")
    with codec(sched, precision=precision) as c:
        c.set_window_early_stop("hda")
        for b in range(frames):
            check_against(c, _x(flow[b:b + 1]), rows[b:b + 1], used[b:b + 1], les[b:b + 1])


# ------------------------------------------------------------------ 4. parts, waves and workgroups
@pytest.mark.parametrize("sched,algo,precision", [("A", "logmap", "f64"), ("B", "maxlog", "f32")])
def test_parts_waves_and_workgroups(sched, algo, precision):
    """The 70 frames tiled to a ragged batch big enough for four parts, in tiled order and sorted by
    expected stop count (whole waves and workgroups finishing at 2, 3, ... 8), with 1-4 parts and two
    alpha run lengths: a codeword's result does not depend on its neighbours, so the 70 oracle results
    are the whole reference."""
    flow, rows, _ = W.synth_case(sched, 0.0, 70, algo, precision)
    used = stops(rows, "hda")
    assert len(set(used.tolist())) >= 4
    B = 4 * 64 * 64 + 37
    idx = np.arange(B) % 70
    for order in (idx, idx[np.argsort(used[idx], kind="stable")]):
        x = _x(flow[order])
        want_bits, want_n = rows[order, used[order] - 1], used[order]
        for parts, run_a in ((1, 0), (2, 0), (3, 0), (4, 0), (2, 1), (4, 3)):
            with codec(sched, algo, precision, run_a=run_a, parts=parts) as c:
                c.set_window_early_stop("hda")
                bits, n = run(c, x)
                assert np.array_equal(n, want_n), (parts, run_a)
                assert np.array_equal(bits, want_bits), (parts, run_a)
        with codec(sched, algo, precision) as c:   # all_iters: one part, a transpose per iteration
            c.set_window_early_stop("hda")
            bits, n = run(c, x, all_iters=True)
            assert np.array_equal(n, want_n) and np.array_equal(bits, frozen(rows, used)[order])


# ------------------------------------------------------------------ 5. interface
def test_interface():
    import ctypes as C

    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    from turbo_decoder_cuda_amd import _native as N
    K, f1, f2, Wn, g = SCHED["A"][:5]
    B = 19
    flow, rows, _ = W.synth_case("A", 0.0, 70)
    flow, rows = flow[:B], rows[:B]
    used = stops(rows, "hda")
    assert len(set(used.tolist())) >= 3
    x = _x(flow)
    with TurboCodec(K, f1, f2, iterations=ITERS) as c:
        # only on a handle whose schedule is windowed
        with pytest.raises(N.TurboError) as e:
            c.set_window_early_stop("hda")
        assert e.value.code == N.TD_EINVAL and c.early_stop is None
        c.set_window(Wn, g)
        plain = c.decode(x, all_iters=True).cpu().numpy()
        bits, n = run(c, x, all_iters=True)   # no rule: the counts are all `iterations`
        assert plain.tobytes() == bits.tobytes() and np.all(n == ITERS)
        assert np.array_equal(plain, rows)
        c.set_window_early_stop("hda")
        assert c.early_stop == "hda"
        # the plain entry points (null count pointer) stop all the same
        assert np.array_equal(c.decode(x, all_iters=True).cpu().numpy(), frozen(rows, used))
        out = torch.empty((B, K), dtype=torch.uint8, device=x.device)
        c.decode_raw(x.data_ptr(), B, out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), rows[np.arange(B), used - 1])
        cnt = torch.zeros(B, dtype=torch.int32, device=x.device)
        c.decode_raw(x.data_ptr(), B, out.data_ptr(), iters_ptr=cnt.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), used)
        with pytest.raises(ValueError):
            c.decode(x, iters_out=torch.zeros(B + 1, dtype=torch.int32, device=x.device))
        with pytest.raises(ValueError):
            c.decode(x, iters_out=torch.zeros(B, dtype=torch.int64, device=x.device))
        hb, hn = c.TurboDecoding(flow, return_iters=True)   # host arrays
        assert np.array_equal(hn, used) and np.array_equal(hb.astype(np.uint8), frozen(rows, used))
        # the stopping kernels take no clock sample
        with pytest.raises(N.TurboError) as e:
            c.clock()
        assert e.value.code == N.TD_EINVAL
        # bad parameters leave the rule as it was
        for kw in (dict(min_iters=0), dict(min_iters=ITERS + 1)):
            with pytest.raises(N.TurboError) as e:
                c.set_window_early_stop("hda", **kw)
            assert e.value.code == N.TD_EINVAL
        with pytest.raises(N.TurboError):
            c.set_window_early_stop("crc", crc_poly=0)
        with pytest.raises(N.TurboError):
            c.set_window_early_stop("crc", crc_poly=0x1000000)
        bad = N.TdStopParams(7, 1, 0)
        assert N.lib().td_set_window_stop(c._h, C.byref(bad)) == N.TD_EINVAL
        assert np.array_equal(run(c, x)[1], used)
        # the exact schedule's switch stays an error on a windowed handle
        with pytest.raises(N.TurboError) as e:
            c.set_early_stop("hda")
        assert e.value.code == N.TD_EINVAL
        # the rule survives a second set_window
        c.set_window(Wn, g)
        bits, n = run(c, x, all_iters=True)
        assert np.array_equal(n, used) and np.array_equal(bits, frozen(rows, used))
        # off again: the rule-off bytes, and a clock sample again
        c.set_window_early_stop(None)
        bits, n = run(c, x, all_iters=True)
        assert plain.tobytes() == bits.tobytes() and np.all(n == ITERS)
        c.clock()
        # set_window(0) clears the rule: back on a windowed schedule nothing stops
        c.set_window_early_stop("hda")
        c.set_window(0)
        assert c.early_stop is None
        c.set_window(Wn, g)
        bits, n = run(c, x, all_iters=True)
        assert plain.tobytes() == bits.tobytes() and np.all(n == ITERS)
        assert N.lib().td_set_window_stop(c._h, None) == N.TD_OK   # NULL: off
    with TurboCodec(24, 1, 6, iterations=2) as c:   # K = 24: no room for a CRC
        c.set_window(8, 8)
        with pytest.raises(N.TurboError) as e:
            c.set_window_early_stop("crc")
        assert e.value.code == N.TD_EINVAL
        c.set_window_early_stop("hda")


# ------------------------------------------------------------------ 6. graph capture
def test_graph_capture_hda():
    """td_reserve, then one HDA decode captured and replayed twice on fresh input: bits and counts equal
    the eager decode's and the oracle rule's (the decision is made on the device between the iterations'
    launches, the per-codeword state is reset inside the captured work, nothing is allocated)."""
    import torch

    B = 19
    dev = _dev()
    cases = [W.synth_case("A", 0.0, 70), W.synth_case("A", 1.0, 19)]
    xs = [_x(f[:B]) for f, _, _ in cases]
    sb = torch.cuda.Stream(dev)
    with codec("A") as c:
        c.set_window_early_stop("hda")
        c.reserve(B)
        gin = xs[0].clone()
        gout = torch.empty((B, ITERS, SCHED["A"][0]), dtype=torch.uint8, device=dev)
        gcnt = torch.empty((B,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            c.decode(gin, gout, all_iters=True, stream=sb, iters_out=gcnt)
        replayed = []
        for k in (1, 0):
            gin.copy_(xs[k])
            graph.replay()
            torch.cuda.synchronize()
            replayed.append((gout.cpu().numpy().copy(), gcnt.cpu().numpy().copy()))
        for (bits, n), k in zip(replayed, (1, 0)):
            eb, en = run(c, xs[k], all_iters=True)
            assert np.array_equal(bits, eb) and np.array_equal(n, en), k
            rows = cases[k][1][:B]
            assert np.array_equal(n, stops(rows, "hda")) and np.array_equal(bits, frozen(rows, n))


# ------------------------------------------------------------------ 7. the BER harness
def test_ber_harness_counts_frozen_rows():
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    from turbo_decoder_cuda_amd.ber import ber_sweep
    K, f1, f2, iters, B, seed, ebn0 = 1024, 31, 64, 6, 48, 5, 0.3
    with TurboCodec(K, f1, f2, iterations=iters) as c:
        c.set_window(64, 30)
        c.synth_seed(seed)
        info, x = c.synth(B, ebn0)
        rows = c.decode(x, all_iters=True).cpu().numpy()
        torch.cuda.synchronize()
        used = stops(rows, "hda")
        assert len(set(used.tolist())) >= 2 and used.min() < iters
        want = (frozen(rows, used) != info.cpu().numpy()[:, None, :]).sum(axis=(0, 2))
        c.set_window_early_stop("hda")
        pt = ber_sweep(c, [ebn0], seed, B, min_block_errors=0, batch=32)[0]
        assert pt.frames == B and pt.bit_errors == want.tolist()
        assert pt.iters_used == int(used.sum()) and abs(pt.mean_iters - used.mean()) < 1e-12


# ------------------------------------------------------------------ 8. the drop-in
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compat_wstop") / "compat_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(REPO, "tests", "compat_driver.cpp"),
                           f"-L{PKG}", "-lturbo_logmap_compat", "-lturbo_mi355x", f"-Wl,-rpath,{PKG}"])
    return out


def _drop_in_env(**kw):
    env = dict(os.environ, TD_ITERATIONS=str(ITERS))
    for v in ("TD_EARLY_STOP", "TD_WINDOW_EARLY_STOP", "TD_WINDOW", "TD_OVERLAP", "TD_STOP_MIN_ITERS", "TD_STOP_CRC_POLY",
              "TD_NII", "TD_CONCURRENT", "TD_EXT_SCALE", "TD_WINDOW_MAXSTAR", "TD_ALGO"):
        env.pop(v, None)
    env.update(kw)
    return env


@pytest.mark.parametrize("stop", ["hda", ""])
def test_compat_window_early_stop(driver, tmp_path, stop):
    """The unchanged caller's TurboDecoding on the windowed schedule with TD_WINDOW_EARLY_STOP=hda, one
    frame per call: the oracle's rows with those after each frame's stop copies of its stop row; without
    the variable, the rule-off rows."""
    K, f1, f2 = SCHED["A"][:3]
    B = 19
    flow, rows, _ = W.synth_case("A", 0.0, 70)
    flow, rows = flow[:B], rows[:B]
    flow.astype(np.float64).tofile(tmp_path / "flow.bin")
    env = _drop_in_env(TD_WINDOW="16", TD_OVERLAP="16")
    if stop:
        env["TD_WINDOW_EARLY_STOP"] = stop
    subprocess.run([driver, "decode", str(K), str(f1), str(f2), str(B), str(tmp_path / "flow.bin"),
                    str(tmp_path / "out.bin")], env=env, timeout=300, check=True)
    out = np.fromfile(tmp_path / "out.bin", dtype=np.int32).reshape(B, 15, K)[:, :ITERS].astype(np.uint8)
    assert np.array_equal(out, frozen(rows, stops(rows, "hda")) if stop else rows)


def test_compat_window_early_stop_without_window_is_an_error(driver, tmp_path):
    K, f1, f2 = SCHED["A"][:3]
    flow = W.synth_case("A", 0.0, 70)[0][:1]
    flow.astype(np.float64).tofile(tmp_path / "flow.bin")
    env = _drop_in_env(TD_WINDOW_EARLY_STOP="hda")
    r = subprocess.run([driver, "decode", str(K), str(f1), str(f2), "1", str(tmp_path / "flow.bin"),
                        str(tmp_path / "out.bin")], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 1 and "TD_WINDOW_EARLY_STOP" in r.stdout
