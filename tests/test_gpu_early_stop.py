"""Per-codeword early termination of the exact schedule (td_set_early_stop) on the MI355X.

Expected values: pyoracle.turbo_decode's per-iteration rows pushed through a numpy statement of the
two rules (include/turbo_mi355x.h):
  HDA  stop after the smallest n >= max(2, min_iters) with row(n) == row(n-1), else at `iterations`
  CRC  stop after the smallest n >= max(1, min_iters) with CRC-24(row(n)) == 0, else at `iterations`
with the decoded bits = row(n), the all_iters rows after n copies of row(n), and Le of iterations
<= n the full decode's.  Every case first asserts on the reference rows that it is not vacuous:
several distinct stop counts in the batch and a group of 8 whose members stop at different
iterations (the kernel decides per codeword inside a workgroup of 8)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pyoracle as O
from conftest import REPO, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

PKG = os.path.join(REPO, "turbo_decoder_cuda_amd")
CRC24A, CRC24B = 0x864CFB, 0x800063
ITERS = 8


def _dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ the rules, in numpy
def crc24(bits, poly):
    reg = 0
    for b in bits:
        top = ((reg >> 23) & 1) ^ int(b)
        reg = (reg << 1) & 0xFFFFFF
        if top:
            reg ^= poly
    return reg


def hda_stop(rows, min_iters=1):
    """rows [iters, K] of one codeword -> iterations used (1-based)."""
    for n in range(max(2, min_iters), rows.shape[0] + 1):
        if np.array_equal(rows[n - 1], rows[n - 2]):
            return n
    return rows.shape[0]


def crc_stop(rows, poly, min_iters=1):
    for n in range(max(1, min_iters), rows.shape[0] + 1):
        if crc24(rows[n - 1], poly) == 0:
            return n
    return rows.shape[0]


def stops(rows, rule, min_iters=1, poly=CRC24B):
    """rows [B, iters, K] -> int32 [B]."""
    f = (lambda r: hda_stop(r, min_iters)) if rule == "hda" else (lambda r: crc_stop(r, poly, min_iters))
    return np.array([f(r) for r in rows], dtype=np.int32)


def frozen(rows, used):
    """The all_iters rows of a stopped decode: rows after the stop are copies of the stop row."""
    out = rows.copy()
    for b, n in enumerate(used):
        out[b, n:] = rows[b, n - 1]
    return out


def assert_not_vacuous(used, distinct=3, spread=None):
    vals = set(int(v) for v in used)
    if spread is not None:
        assert vals == set(spread), f"stop counts {sorted(vals)}, the case was built for {sorted(spread)}"
    else:
        assert len(vals) >= distinct, f"only the stop counts {sorted(vals)}"
    groups = [used[g:g + 8] for g in range(0, len(used), 8)]
    assert any(len(set(g.tolist())) > 1 for g in groups), "no group of 8 whose members stop at different iterations"


# ------------------------------------------------------------------ inputs and references, made once
@functools.lru_cache(maxsize=None)
def synth_case(K, f1, f2, ebn0, B, algo):
    """(flow [B, 3K+12], oracle rows [B, iters, K] uint8, oracle Le [B, iters, 2, K+3]); read-only."""
    _, flow = O.synth_batch(K, f1, f2, ebn0, 4242, B)
    oalgo = O.ALGO_MAXLOG if algo == "maxlog" else O.ALGO_LOGMAP
    rows, les = zip(*(O.turbo_decode(flow[b], K, f1, f2, ITERS, algo=oalgo) for b in range(B)))
    rows, les = np.array(rows).astype(np.uint8), np.array(les)
    for a in (flow, rows, les):
        a.setflags(write=False)
    return flow, rows, les


def crc_frames(K, f1, f2, poly, sigma, B):
    """B frames whose K bits are K-24 random bits (default_rng(5), drawn first) and their CRC-24,
    turbo-encoded, BPSK (bit 1 -> +1) over AWGN of that sigma, as channel LLRs 2y/sigma^2."""
    rng = np.random.default_rng(5)
    payload = rng.integers(0, 2, (B, K - 24))
    flow = np.zeros((B, 3 * K + 12))
    for b in range(B):
        c = crc24(payload[b], poly)
        row = np.concatenate([payload[b], [(c >> (23 - j)) & 1 for j in range(24)]]).astype(np.int32)
        coded = O.encode(row, f1, f2)
        y = (2.0 * coded - 1.0) + rng.normal(0.0, sigma, coded.size)
        flow[b] = 2.0 * y / sigma ** 2
    return flow


@functools.lru_cache(maxsize=None)
def crc_case(K, f1, f2, poly, sigma, B):
    flow = crc_frames(K, f1, f2, poly, sigma, B)
    rows = np.array([O.turbo_decode(flow[b], K, f1, f2, ITERS)[0] for b in range(B)]).astype(np.uint8)
    flow.setflags(write=False)
    rows.setflags(write=False)
    return flow, rows


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
    """The three ways a decode writes its decisions: final row only (a fold lane compares with the
    byte it overwrites), all_iters (with the row before), all_iters with an Le dump (the generic
    fold)."""
    B = rows.shape[0]
    stop_rows = rows[np.arange(B), used - 1]
    bits, n = run(c, x)
    assert np.array_equal(n, used), (n.tolist(), used.tolist())
    assert np.array_equal(bits, stop_rows)
    bits, n = run(c, x, all_iters=True)
    assert np.array_equal(n, used), (n.tolist(), used.tolist())
    assert np.array_equal(bits, frozen(rows, used))
    bits, n, le = run(c, x, all_iters=True, le=True)
    assert np.array_equal(n, used), (n.tolist(), used.tolist())
    assert np.array_equal(bits, frozen(rows, used))
    if les is not None:
        for b in range(B):
            d = np.abs(le[b, :used[b]] - les[b, :used[b]]).max()
            assert d <= 1e-9, f"codeword {b}: Le differs by {d:g} within its {used[b]} iterations"


# ------------------------------------------------------------------ HDA against the oracle
@pytest.mark.parametrize("min_iters", [1, 4, 8])
@pytest.mark.parametrize("algo", ["logmap", "maxlog"])
@pytest.mark.parametrize("ebn0", [0.0, 1.0])
def test_hda_small(ebn0, algo, min_iters):
    """K = 40, B = 19 (two full groups and a ragged one of 3), fp64."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, B = 40, 3, 10, 19
    flow, rows, les = synth_case(K, f1, f2, ebn0, B, algo)
    assert_not_vacuous(stops(rows, "hda"))
    used = stops(rows, "hda", min_iters)
    x = torch.tensor(flow).to(_dev())
    with TurboCodec(K, f1, f2, iterations=ITERS, algo=algo) as c:
        off = c.decode(x, all_iters=True).cpu().numpy()
        c.set_early_stop("hda", min_iters=min_iters)
        check_against(c, x, rows, used, les)
        if min_iters == ITERS:   # the full decode exactly
            assert np.all(used == ITERS)
            bits, n = run(c, x, all_iters=True)
            assert np.array_equal(bits, off) and np.all(n == ITERS)


@pytest.mark.parametrize("K,f1,f2,B,spread", [(1024, 31, 64, 19, (3, 4, 5)), (6144, 263, 480, 9, (4, 5))])
def test_hda_at_size(K, f1, f2, B, spread):
    """Many windows per SISO (the folds' fast path), 1.0 dB, fp64 log-MAP."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    flow, rows, les = synth_case(K, f1, f2, 1.0, B, "logmap")
    used = stops(rows, "hda")
    assert_not_vacuous(used, spread=spread)
    x = torch.tensor(flow).to(_dev())
    with TurboCodec(K, f1, f2, iterations=ITERS) as c:
        c.set_early_stop("hda")
        check_against(c, x, rows, used, les)


# ------------------------------------------------------------------ CRC against the oracle
@pytest.mark.parametrize("K,f1,f2,poly,sigma,spread", [(40, 3, 10, CRC24B, 1.2, (1, 2, 3, 8)),
                                                       (40, 3, 10, CRC24A, 1.2, None),
                                                       (1024, 31, 64, CRC24B, 1.1, None)])
def test_crc(K, f1, f2, poly, sigma, spread):
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    B = 19
    flow, rows = crc_case(K, f1, f2, poly, sigma, B)
    used = stops(rows, "crc", poly=poly)
    assert_not_vacuous(used, spread=spread)
    if spread:   # stops after the first iteration, and frames that never pass
        assert sum(crc24(rows[b, -1], poly) != 0 for b in range(B)) == 8
    x = torch.tensor(flow).to(_dev())
    with TurboCodec(K, f1, f2, iterations=ITERS) as c:
        c.set_early_stop("crc", crc_poly=poly)
        check_against(c, x, rows, used)
        c.set_early_stop("crc", min_iters=3, crc_poly=poly)
        check_against(c, x, rows, stops(rows, "crc", 3, poly))


# ------------------------------------------------------------------ fp32 and three / four workgroups per CU
@functools.lru_cache(maxsize=None)
def big_flow(kind, B):
    """B frames of K = 40 tiled from 19 (19 and 8 are coprime: every group of 8 gets its own mix)."""
    if kind == "crc":
        base = crc_case(40, 3, 10, CRC24B, 1.2, 19)[0]
    else:
        base = synth_case(40, 3, 10, 0.0, 19, "logmap")[0]
    flow = np.ascontiguousarray(np.tile(base, (B // 19 + 1, 1))[:B].astype(np.float32))
    flow.setflags(write=False)
    return flow


@pytest.mark.parametrize("rule,algo", [("hda", "logmap"), ("hda", "maxlog"), ("crc", "logmap")])
@pytest.mark.parametrize("occ3", ["1", "0"])
@pytest.mark.parametrize("B", [5000, 6150])
def test_f32_large_batch(monkeypatch, B, occ3, rule, algo):
    """fp32, more codeword groups than two per CU: B = 5000 runs the three-per-CU stopping kernel,
    6150 the four-per-CU one of the 12-step-window build; TD_OCC3=0 keeps both on two per CU.  The
    reference is the numpy rule on the same handle's rule-off all_iters decode (the path the
    existing suite pins)."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, iters = 40, 3, 10, 6
    monkeypatch.setenv("TD_OCC3", occ3)
    x = torch.tensor(big_flow(rule, B)).to(_dev())
    with TurboCodec(K, f1, f2, iterations=iters, algo=algo, precision="f32") as c:
        rows = c.decode(x, all_iters=True).cpu().numpy()
        used = stops(rows[:64], rule)
        assert_not_vacuous(used)
        # (the frames repeat with period 19 and a codeword's result does not depend on its neighbours)
        assert np.array_equal(rows[:B - B % 19].reshape(-1, 19, iters, K)[1:], np.broadcast_to(
            rows[:19], (B // 19 - 1, 19, iters, K)))
        used = np.tile(stops(rows[:19], rule), B // 19 + 1)[:B]
        c.set_early_stop(rule)
        check_against(c, x, rows, used)


# ------------------------------------------------------------------ interface
def test_interface():
    import ctypes as C

    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    from turbo_decoder_cuda_amd import _native as N
    K, f1, f2, B = 40, 3, 10, 19
    flow, rows, _ = synth_case(K, f1, f2, 0.0, B, "logmap")
    used = stops(rows, "hda")
    x = torch.tensor(flow).to(_dev())
    with TurboCodec(K, f1, f2, iterations=ITERS) as c:
        # no rule: the _stop entry point equals td_decode_device byte for byte, counts all `iterations`
        plain = c.decode(x, all_iters=True).cpu().numpy()
        bits, n = run(c, x, all_iters=True)
        assert plain.tobytes() == bits.tobytes() and np.all(n == ITERS)
        assert np.array_equal(plain, rows)
        # a rule set: the plain entry point (null count pointer) stops all the same
        c.set_early_stop("hda")
        assert np.array_equal(c.decode(x, all_iters=True).cpu().numpy(), frozen(rows, used))
        out = torch.empty((B, K), dtype=torch.uint8, device=x.device)
        c.decode_raw(x.data_ptr(), B, out.data_ptr())   # raw pointers, null iters_ptr
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
        # host arrays
        hb, hn = c.TurboDecoding(flow, return_iters=True)
        assert np.array_equal(hn, used) and np.array_equal(hb.astype(np.uint8), frozen(rows, used))
        # the windowed schedule and a rule exclude each other, either way round
        with pytest.raises(N.TurboError) as e:
            c.set_window(16, 16)
        assert e.value.code == N.TD_EINVAL
        # bad parameters leave the rule as it was
        for kw in (dict(min_iters=0), dict(min_iters=ITERS + 1)):
            with pytest.raises(N.TurboError) as e:
                c.set_early_stop("hda", **kw)
            assert e.value.code == N.TD_EINVAL
        with pytest.raises(N.TurboError):
            c.set_early_stop("crc", crc_poly=0)
        bad = N.TdStopParams(7, 1, 0)
        assert N.lib().td_set_early_stop(c._h, C.byref(bad)) == N.TD_EINVAL
        assert np.array_equal(run(c, x)[1], used)
        # off again: the full decode
        c.set_early_stop(None)
        bits, n = run(c, x, all_iters=True)
        assert plain.tobytes() == bits.tobytes() and np.all(n == ITERS)
        c.set_window(16, 16)
        with pytest.raises(N.TurboError) as e:
            c.set_early_stop("hda")
        assert e.value.code == N.TD_EINVAL
    with TurboCodec(24, 1, 6, iterations=2) as c:   # K = 24: no room for a CRC
        with pytest.raises(N.TurboError) as e:
            c.set_early_stop("crc")
        assert e.value.code == N.TD_EINVAL
        c.set_early_stop("hda")


# ------------------------------------------------------------------ the BER harness
def test_ber_harness_counts_frozen_rows():
    """ber.py with a rule set: the per-iteration error counts are those of the frozen rows (rows after
    a frame's stop are copies of its stop row) and the point reports the mean iterations used."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    from turbo_decoder_cuda_amd.ber import ber_sweep
    K, f1, f2, iters, B, seed, ebn0 = 1024, 31, 64, 6, 48, 5, 0.3
    with TurboCodec(K, f1, f2, iterations=iters) as c:
        c.synth_seed(seed)
        info, x = c.synth(B, ebn0)
        rows = c.decode(x, all_iters=True).cpu().numpy()
        torch.cuda.synchronize()
        used = stops(rows, "hda")
        assert len(set(used.tolist())) >= 2 and used.min() < iters
        want = (frozen(rows, used) != info.cpu().numpy()[:, None, :]).sum(axis=(0, 2))
        c.set_early_stop("hda")
        pt = ber_sweep(c, [ebn0], seed, B, min_block_errors=0, batch=32)[0]
        assert pt.frames == B and pt.bit_errors == want.tolist()
        assert pt.iters_used == int(used.sum()) and abs(pt.mean_iters - used.mean()) < 1e-12


# ------------------------------------------------------------------ graph capture
def test_graph_capture_hda():
    """td_reserve, then one HDA decode captured on the handle's one stream and replayed twice on
    fresh input: bits and counts equal the eager decode's (the stop is decided on the device, and the
    decode allocates nothing)."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    K, f1, f2, B = 40, 3, 10, 19
    dev = _dev()
    flows = [synth_case(K, f1, f2, e, B, "logmap")[0] for e in (0.0, 1.0)]
    xs = [torch.tensor(f).to(dev) for f in flows]
    sb = torch.cuda.Stream(dev)
    with TurboCodec(K, f1, f2, iterations=ITERS) as c:
        c.set_early_stop("hda")
        c.reserve(B)
        gin = xs[0].clone()
        gout = torch.empty((B, ITERS, K), dtype=torch.uint8, device=dev)
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
            rows = synth_case(K, f1, f2, (0.0, 1.0)[k], B, "logmap")[1]
            assert np.array_equal(n, stops(rows, "hda")) and np.array_equal(bits, frozen(rows, n))


# ------------------------------------------------------------------ the drop-in
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compat_stop") / "compat_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(REPO, "tests", "compat_driver.cpp"),
                           f"-L{PKG}", "-lturbo_logmap_compat", "-lturbo_mi355x", f"-Wl,-rpath,{PKG}"])
    return out


@pytest.mark.parametrize("stop", ["hda", ""])
def test_compat_early_stop(driver, tmp_path, stop):
    """The unchanged caller's TurboDecoding with TD_EARLY_STOP=hda: its flow_decoded rows are the
    oracle's with the rows after each frame's stop copies of its stop row; without the variable, the
    oracle's rows unchanged."""
    K, f1, f2, B = 40, 3, 10, 19
    flow, rows, _ = synth_case(K, f1, f2, 0.0, B, "logmap")
    flow.astype(np.float64).tofile(tmp_path / "flow.bin")
    env = dict(os.environ, TD_ITERATIONS=str(ITERS))
    env.pop("TD_EARLY_STOP", None)
    if stop:
        env["TD_EARLY_STOP"] = stop
    subprocess.run([driver, "decode", str(K), str(f1), str(f2), str(B), str(tmp_path / "flow.bin"),
                    str(tmp_path / "out.bin")], env=env, timeout=300, check=True)
    out = np.fromfile(tmp_path / "out.bin", dtype=np.int32).reshape(B, 15, K)[:, :ITERS].astype(np.uint8)
    assert np.array_equal(out, frozen(rows, stops(rows, "hda")) if stop else rows)


def test_compat_early_stop_with_window_is_an_error(driver, tmp_path):
    K, f1, f2 = 40, 3, 10
    flow = synth_case(K, f1, f2, 0.0, 19, "logmap")[0][:1]
    flow.astype(np.float64).tofile(tmp_path / "flow.bin")
    env = dict(os.environ, TD_ITERATIONS="4", TD_EARLY_STOP="hda", TD_WINDOW="16", TD_OVERLAP="16")
    r = subprocess.run([driver, "decode", str(K), str(f1), str(f2), "1", str(tmp_path / "flow.bin"),
                        str(tmp_path / "out.bin")], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 1 and "TD_EARLY_STOP" in r.stdout
