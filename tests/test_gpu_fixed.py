"""The fixed-point decoder (TD_FIXED) on the MI355X against its numpy restatement (tests/fixed_ref.py):
hard-decision rows of every iteration, final bits and every extrinsic value, bit for bit.  The kernel
decodes one codeword per lane, 64 to a wave and to a workgroup, so the batch sizes sit round 64."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixed_ref as F
import llr_families
import pyoracle as O
import ratematch_ref as RM
from conftest import GOLD, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]


def _golden_code(name):
    z = np.load(f"{GOLD}/{name}.npz")
    return int(z["K"]), int(z["f1"]), int(z["f2"])


QPP = {8: (3, 4), 40: (3, 10), 1024: (31, 64), 6144: (263, 480)}
for _n in ("frames_K10000_e0.8_s43", "frames_K432_e0.8_s46"):
    _K, _f1, _f2 = _golden_code(_n)
    QPP[_K] = (_f1, _f2)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _codec(K, iters, setting=None):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *QPP[K], iterations=iters, algo="maxlog", precision="fixed")
    if setting is not None:
        c.set_fixed(*setting)
    return c


@functools.lru_cache(maxsize=None)
def _awgn(K, B, steps, ebn0=0.5):
    q = F.quantise(O.synth_batch(K, *QPP[K], ebn0, 5, B)[1], steps)
    q.setflags(write=False)
    return q


def _pattern(name, K, B):
    n = 3 * K + 12
    if name == "plus127":
        return np.full((B, n), 127, dtype=np.int8)
    if name == "minus128":
        return np.full((B, n), -128, dtype=np.int8)
    if name == "alternating":
        return np.tile((127 * (1 - 2 * (np.arange(n) & 1))).astype(np.int8), (B, 1))
    if name == "mixed":   # every saturated pattern and noise side by side in one batch
        rng = np.random.default_rng(K + B)
        q = rng.integers(-128, 128, (B, n)).astype(np.int8)
        q[0::4] = 127
        q[1::4] = -128
        q[2::4] = _pattern("alternating", K, B)[2::4]
        return q
    flow = O.synth_batch(K, *QPP[K], 0.5, 5, B)[1]
    return llr_families.apply(name, flow).astype(np.int8)   # "int8": x16, saturated at +-127; "zero"


def _check(q, K, iters, setting, min_clamped=None, max_clamped=None):
    """Decode q on the GPU (rows of all iterations and Le, then the final bits alone) and compare with
    the restatement."""
    import torch
    q = np.ascontiguousarray(q)
    B = q.shape[0]
    rows, le, share = F.decode(q, K, *QPP[K], iters, *setting)
    if min_clamped is not None:
        assert share > min_clamped, f"the clamp path is exercised: share {share}"
    if max_clamped is not None:
        assert share <= max_clamped, f"nothing clamps: share {share}"
    x = _gpu(q)
    with _codec(K, iters, setting) as c:
        g_le = torch.full((B, iters, 2, K + 3), 12345, dtype=torch.int16, device=_dev())
        g_rows = c.decode(x, all_iters=True, le=g_le)
        g_bits = c.decode(x)
        torch.cuda.synchronize()
        assert g_rows.dtype == torch.uint8 and tuple(g_rows.shape) == (B, iters, K)
        assert np.array_equal(g_rows.cpu().numpy(), rows)
        assert np.array_equal(g_bits.cpu().numpy(), rows[:, -1])
        assert np.array_equal(g_le.cpu().numpy(), le)
        assert np.array_equal(x.cpu().numpy(), q), "d_llr is not modified"
    return rows


# K, iterations, B, (le_max, ext_scale_q): every K, iteration count, batch edge and setting of the issue
CASES = [
    (8, 1, 1, (255, 3)), (8, 4, 65, (255, 4)), (8, 8, 130, (31, 2)),
    (40, 8, 63, (127, 3)), (40, 4, 130, (31, 2)), (40, 1, 64, (255, 4)),
    (432, 4, 65, (255, 3)),
    (1024, 4, 130, (255, 4)), (1024, 8, 63, (255, 3)), (1024, 1, 1, (31, 2)), (1024, 4, 65, (127, 3)),
    (6144, 8, 2, (255, 3)), (6144, 4, 65, (127, 3)), (6144, 1, 1, (255, 4)),
    (10000, 4, 3, (255, 4)),
]


@pytest.mark.parametrize("K,iters,B,setting", CASES)
def test_awgn_equals_restatement(K, iters, B, setting):
    """AWGN at 4 steps per unit LLR: with le_max 255 nothing clamps."""
    _check(_awgn(K, B, 4), K, iters, setting, max_clamped=0.0 if setting[0] == 255 else None)


@pytest.mark.parametrize("K,B", [(1024, 65), (6144, 3)])
def test_clamped_extrinsics_equal_restatement(K, B):
    """1.0 dB at 16 steps per unit with le_max 127: a third of the Le values sits on the clamp after
    four iterations."""
    _check(_awgn(K, B, 16, 1.0), K, 4, (127, 3), min_clamped=0.10)


@pytest.mark.parametrize("family", ["int8", "zero", "plus127", "minus128", "alternating", "mixed"])
@pytest.mark.parametrize("K,iters,B,setting", [(40, 4, 65, (255, 3)), (1024, 4, 65, (255, 4)), (1024, 8, 63, (127, 3))])
def test_saturated_inputs_equal_restatement(family, K, iters, B, setting):
    """The overflow test of the state metrics: whole batches at the int8 limits."""
    _check(_pattern(family, K, B), K, iters, setting)


@pytest.mark.parametrize("K,family", [(6144, "plus127"), (6144, "alternating"), (10000, "minus128"), (10000, "mixed")])
def test_saturated_long_blocks(K, family):
    """The metrics grow with the block length (they are not normalised): the longest blocks, unscaled
    extrinsic, the widest clamp."""
    _check(_pattern(family, K, 4), K, 4, (255, 4))


def test_codeword_alone_equals_its_rows_in_a_batch():
    import torch
    K, iters, B = 1024, 4, 130
    q = _awgn(K, B, 4)
    x = _gpu(q)
    with _codec(K, iters) as c:
        le = torch.empty((B, iters, 2, K + 3), dtype=torch.int16, device=_dev())
        rows = c.decode(x, all_iters=True, le=le)
        for b in (0, 63, 64, 129):
            le1 = torch.empty((1, iters, 2, K + 3), dtype=torch.int16, device=_dev())
            r1 = c.decode(x[b:b + 1].contiguous(), all_iters=True, le=le1)
            assert torch.equal(r1[0], rows[b]) and torch.equal(le1[0], le[b]), b


def test_default_setting_and_set_fixed_null():
    """A fresh handle decodes with {255, 3}; td_set_fixed(NULL) goes back to it."""
    from turbo_decoder_cuda_amd import _native as N
    K, iters, B = 40, 4, 5
    q = _awgn(K, B, 16)
    rows, _, _ = F.decode(q, K, *QPP[K], iters, 255, 3)
    other, _, _ = F.decode(q, K, *QPP[K], iters, 31, 2)
    with _codec(K, iters) as c:
        assert np.array_equal(c.decode(_gpu(q), all_iters=True).cpu().numpy(), rows)
        c.set_fixed(31, 2)
        assert np.array_equal(c.decode(_gpu(q), all_iters=True).cpu().numpy(), other)
        for bad in ((0, 3), (256, 3), (255, 0), (255, 5)):
            with pytest.raises(N.TurboError) as e:
                c.set_fixed(*bad)
            assert e.value.code == N.TD_EINVAL
        assert np.array_equal(c.decode(_gpu(q), all_iters=True).cpu().numpy(), other), "a failed call changes nothing"
        N.check(N.lib().td_set_fixed(c._h, None))
        assert np.array_equal(c.decode(_gpu(q), all_iters=True).cpu().numpy(), rows)


def test_graph_capture_after_reserve_replays_the_eager_result():
    import torch
    K, iters, B = 1024, 4, 65
    qs = [_awgn(K, B, 4), _awgn(K, B, 16)]
    sb = torch.cuda.Stream(_dev())
    with _codec(K, iters) as c:
        c.reserve(B)
        gin = _gpu(qs[0]).clone()
        gout = torch.empty((B, iters, K), dtype=torch.uint8, device=_dev())
        gle = torch.empty((B, iters, 2, K + 3), dtype=torch.int16, device=_dev())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            c.decode(gin, gout, all_iters=True, le=gle, stream=sb)
        for k in (1, 0):
            gin.copy_(_gpu(qs[k]))
            graph.replay()
            torch.cuda.synchronize()
            got, got_le = gout.cpu().numpy().copy(), gle.cpu().numpy().copy()
            ele = torch.empty_like(gle)
            eager = c.decode(_gpu(qs[k]), all_iters=True, le=ele)
            torch.cuda.synchronize()
            assert np.array_equal(got, eager.cpu().numpy()) and np.array_equal(got_le, ele.cpu().numpy()), k
            assert np.array_equal(got, F.decode(qs[k], K, *QPP[K], iters)[0])


def test_host_entry_points_counts_and_profile():
    """td_decode_host(_stop) with int8 in and int16 Le out, the counts filled with `iterations`, and the
    profile events round the fixed kernels."""
    import torch
    K, iters, B = 40, 4, 7
    q = _awgn(K, B, 4)
    rows, le, _ = F.decode(q, K, *QPP[K], iters)
    with _codec(K, iters) as c:
        out, hle, used = c.TurboDecoding(q, return_le=True, return_iters=True)
        assert out.dtype == np.int32 and hle.dtype == np.int16
        assert np.array_equal(out, rows) and np.array_equal(hle, le) and np.array_equal(used, np.full(B, iters))
        assert np.array_equal(c.TurboDecoding(q), rows)
        bits, n = c.decode(_gpu(q), iters_out=True)
        assert np.array_equal(n.cpu().numpy(), np.full(B, iters)) and np.array_equal(bits.cpu().numpy(), rows[:, -1])
        c.profile(True)
        for _ in range(3):
            c.decode(_gpu(q))
        demux_ms, decode_ms, launches = c.kernel_ms()
        assert launches == 3 and decode_ms > 0 and demux_ms >= 0
        c.profile(False)
        with pytest.raises(ValueError):
            c.decode(_gpu(q.astype(np.float32)))
        with pytest.raises(ValueError):
            c.decode(_gpu(q), le=torch.empty((B, iters, 2, K + 3), dtype=torch.float32, device=_dev()))


def test_calls_that_do_not_apply_are_einval():
    from turbo_decoder_cuda_amd import _native as N
    L = N.lib()
    with _codec(40, 2) as c:
        h = c._h
        w = N.TdWindowParams(16, 8, 0, 0, 1.0)
        s = N.TdStopParams(N.TD_STOP_HDA, 1, 0)
        g, ms = C.c_double(), C.c_double()
        buf = np.zeros(64)
        p = buf.ctypes.data_as(C.c_void_p)
        calls = {
            "td_set_window": lambda: L.td_set_window(h, C.byref(w)),
            "td_set_window_maxstar": lambda: L.td_set_window_maxstar(h, N.TD_WMAXSTAR_EXACT),
            "td_set_early_stop": lambda: L.td_set_early_stop(h, C.byref(s)),
            "td_set_window_stop": lambda: L.td_set_window_stop(h, C.byref(s)),
            "td_siso_host": lambda: L.td_siso_host(h, p, p, 1, p, 8, 1),
            "td_clock_read": lambda: L.td_clock_read(h, C.byref(g), C.byref(ms)),
            "td_debug_set_stamps": lambda: L.td_debug_set_stamps(h, None),
        }
        for name, call in calls.items():
            assert call() == N.TD_EINVAL, name
            msg = L.td_last_error().decode()
            assert name in msg and "TD_FIXED" in msg, msg
        c.decode(_gpu(_awgn(40, 2, 4)))
        assert calls["td_clock_read"]() == N.TD_EINVAL   # also after a decode
    from turbo_decoder_cuda_amd import TurboCodec
    with TurboCodec(40, 3, 10, iterations=2) as f64:      # td_set_fixed belongs to fixed handles
        with pytest.raises(N.TurboError) as e:
            f64.set_fixed()
        assert e.value.code == N.TD_EINVAL
    for kw in ({"algo": "logmap"}, {}):                    # the constructor's default algo is log-MAP
        with pytest.raises(N.TurboError) as e:
            TurboCodec(40, 3, 10, iterations=2, precision="fixed", **kw)
        assert e.value.code == N.TD_EINVAL


def test_quantise():
    import torch
    from turbo_decoder_cuda_amd import decoder
    flow = O.synth_batch(40, 3, 10, 0.5, 5, 3)[1] * 3.0
    for steps in (4, 16):
        got = decoder.quantise(_gpu(flow), steps)
        assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), F.quantise(flow, steps))


# ------------------------------------------------------------------ rate matching in int8
def _e_values(B, E, seed, big=False):
    rng = np.random.default_rng(seed)
    lo, hi = (-128, 128) if big else (-40, 41)
    return rng.integers(lo, hi, (B, E)).astype(np.int8)


@pytest.mark.parametrize("K,B", [(40, 3), (1024, 65)])
def test_rate_dematch_int8_equals_saturating_reference(K, B):
    """E = 2K (puncturing), 3K+12 and 5K (repetition, so saturation), every rv, a limited Ncb, and
    accumulation onto a soft buffer that holds -128 and values near the limits."""
    import torch
    _, _, Kpi, Kw, _ = RM.layout(K)
    mid = (Kpi + (Kw - Kpi) // 2) | 1
    n = 3 * K + 12
    with _codec(K, 1) as c:
        for Ncb in (0, mid):
            c.set_rate_matching(Ncb)
            for E in (2 * K, n, 5 * K):
                for rv in range(4):
                    e = _e_values(B, E, K + E + rv, big=(rv & 1) == 1)
                    got = c.rate_dematch(_gpu(e), rv)
                    assert got.dtype == torch.int8
                    assert np.array_equal(got.cpu().numpy(), F.dematch(e, K, Ncb, rv)), (Ncb, E, rv)
                    prior = _e_values(B, n, 7 * K + E + rv, big=True)
                    prior[:, ::5] = -128
                    buf = _gpu(prior).clone()
                    c.rate_dematch(_gpu(e), rv, out=buf, accumulate=True)
                    assert np.array_equal(buf.cpu().numpy(), F.dematch(e, K, Ncb, rv, prior=prior)), (Ncb, E, rv, "acc")
        # rate_match moves int8 as it moves bytes
        x = _e_values(B, n, 99, big=True)
        c.set_rate_matching(0)
        assert np.array_equal(c.rate_match(_gpu(x), 2, 2 * K).cpu().numpy(), x[:, RM.index(K, 0, 2, 2 * K)])
        with pytest.raises(ValueError):
            c.rate_dematch(_gpu(x.astype(np.float32)), 0)


def test_rate_half_and_harq_through_the_decoder():
    """Rate 1/2 (E = 2K, rv 0) alone, then combined with an rv 2 retransmission: the GPU chain
    quantise -> rate_dematch (-> accumulate) -> decode equals the reference chain."""
    from turbo_decoder_cuda_amd import decoder
    K, iters, B = 1024, 4, 9
    f1, f2 = QPP[K]
    flow = O.synth_batch(K, f1, f2, 1.5, 21, B)[1]
    flow2 = O.synth_batch(K, f1, f2, 1.5, 22, B)[1]   # other noise; the chain is compared, not the BER
    E = 2 * K
    with _codec(K, iters) as c:
        c.set_rate_matching(0)
        q1, q2 = decoder.quantise(_gpu(flow), 8), decoder.quantise(_gpu(flow2), 8)
        e1, e2 = c.rate_match(q1, 0, E), c.rate_match(q2, 2, E)
        r1 = F.quantise(flow, 8)[:, RM.index(K, 0, 0, E)]
        r2 = F.quantise(flow2, 8)[:, RM.index(K, 0, 2, E)]
        assert np.array_equal(e1.cpu().numpy(), r1) and np.array_equal(e2.cpu().numpy(), r2)
        buf = c.rate_dematch(e1, 0)
        want = F.dematch(r1, K, 0, 0)
        assert np.array_equal(buf.cpu().numpy(), want)
        assert np.array_equal(c.decode(buf, all_iters=True).cpu().numpy(), F.decode(want, K, f1, f2, iters)[0])
        c.rate_dematch(e2, 2, out=buf, accumulate=True)
        want = F.dematch(r2, K, 0, 2, prior=want)
        assert np.array_equal(buf.cpu().numpy(), want)
        assert np.array_equal(c.decode(buf, all_iters=True).cpu().numpy(), F.decode(want, K, f1, f2, iters)[0])
