"""The fixed-point decoder's sub-block schedule (td_set_fixed_window) on the MI355X against its numpy
restatement (tests/fixed_window_ref.py): hard-decision rows of every iteration, final bits and every
extrinsic value, bit for bit.  A wave is 64 codewords times one sub-block, a launch one SISO of one
iteration; the integer arithmetic rounds nowhere, so every schedule detail shows in the bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixed_ref as F
import fixed_window_ref as FW
import llr_families
import pyoracle as O
import ratematch_ref as RM
from conftest import GOLD, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

QPP = {40: (3, 10), 1024: (31, 64), 6144: (263, 480)}
_z = np.load(f"{GOLD}/frames_K10000_e0.8_s43.npz")
QPP[int(_z["K"])] = (int(_z["f1"]), int(_z["f2"]))
DEFAULT = (64, 48)   # TurboCodec.set_fixed_window's


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _codec(K, iters, win=None, setting=None):
    from turbo_decoder_cuda_amd import TurboCodec
    c = TurboCodec(K, *QPP[K], iterations=iters, algo="maxlog", precision="fixed")
    if setting is not None:
        c.set_fixed(*setting)
    if win is not None:
        c.set_fixed_window(*win)
    return c


@functools.lru_cache(maxsize=None)
def _awgn(K, B, steps=8, ebn0=0.5):
    q = F.quantise(O.synth_batch(K, *QPP[K], ebn0, 5, B)[1], steps)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _ref_awgn(K, B, iters, win, setting=(255, 3), steps=8):
    """The restatement of an _awgn batch, computed once and shared; never written to."""
    rows, le = FW.decode(_awgn(K, B, steps), K, *QPP[K], iters, *win, *setting)
    rows.setflags(write=False)
    le.setflags(write=False)
    return rows, le


def _decode_all(c, q):
    """(rows of every iteration, Le, final bits alone) of q on the GPU, as numpy."""
    import torch
    B, iters, K = q.shape[0], c.iterations, c.K
    x = _gpu(q)
    g_le = torch.full((B, iters, 2, K + 3), 12345, dtype=torch.int16, device=_dev())
    g_rows = c.decode(x, all_iters=True, le=g_le)
    g_bits = c.decode(x)
    torch.cuda.synchronize()
    assert g_rows.dtype == torch.uint8 and tuple(g_rows.shape) == (B, iters, K)
    assert np.array_equal(x.cpu().numpy(), q), "d_llr is not modified"
    return g_rows.cpu().numpy(), g_le.cpu().numpy(), g_bits.cpu().numpy()


def _check(q, K, iters, win, setting=(255, 3), ref=None):
    rows, le = ref if ref is not None else FW.decode(q, K, *QPP[K], iters, *win, *setting)
    with _codec(K, iters, win, setting) as c:
        g_rows, g_le, g_bits = _decode_all(c, np.ascontiguousarray(q))
    assert np.array_equal(g_rows, rows)
    assert np.array_equal(g_le, le)
    assert np.array_equal(g_bits, rows[:, -1]), "all_iters=False gives the last row"


# K, iterations, B, (window, overlap): one sub-block, a last sub-block with a remainder and a partial last
# 16-step window; overlaps of 0, no multiple of 16, past the trellis' ends; the longest blocks
GEOMETRY = [
    (40, 1, 5, (16, 0)), (40, 4, 5, (16, 0)), (40, 8, 5, (16, 0)),
    (40, 1, 5, (16, 5)), (40, 4, 5, (16, 5)), (40, 8, 5, (16, 5)),
    (40, 1, 5, (16, 48)), (40, 4, 5, (16, 48)), (40, 8, 5, (16, 48)),
    (1024, 1, 3, (64, 32)), (1024, 4, 3, (64, 32)), (1024, 8, 3, (64, 32)),
    (1024, 1, 3, (32, 7)), (1024, 4, 3, (32, 7)),
    (1024, 1, 3, (128, 384)), (1024, 4, 3, (128, 384)),
    (6144, 2, 3, (64, 32)),
    (10000, 2, 2, (64, 32)),
]


@pytest.mark.parametrize("K,iters,B,win", GEOMETRY)
def test_window_geometry_equals_restatement(K, iters, B, win):
    _check(_awgn(K, B), K, iters, win, ref=_ref_awgn(K, B, iters, win))


def test_restatement_differs_from_exact_on_these_inputs():
    """What the tests above compare against is not the exact decode: a kernel that ignored the window
    could not pass them."""
    K, B, iters = 1024, 3, 4
    rows, le, _ = F.decode(_awgn(K, B), K, *QPP[K], iters)
    for win in ((64, 32), (32, 7)):
        w_rows, w_le = _ref_awgn(K, B, iters, win)
        assert (w_rows != rows).any() and (w_le != le).any(), win


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_batch_sizes_round_the_wave(B):
    """A codeword's result does not depend on the batch: the first B codewords of one 130-frame
    restatement."""
    K, iters = 1024, 2
    rows, le = _ref_awgn(K, 130, iters, DEFAULT)
    _check(_awgn(K, 130)[:B], K, iters, DEFAULT, ref=(rows[:B], le[:B]))


@pytest.mark.parametrize("setting", [(255, 3), (255, 4), (31, 2), (127, 3)])
def test_extrinsic_settings(setting):
    """16 steps per unit: with le_max 31 and 127 the clamp works."""
    K, B, iters = 1024, 3, 4
    _check(_awgn(K, B, 16), K, iters, DEFAULT, setting, ref=_ref_awgn(K, B, iters, DEFAULT, setting, 16))


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


@pytest.mark.parametrize("family", ["int8", "zero", "plus127", "minus128", "alternating", "mixed"])
def test_saturated_inputs_equal_restatement(family):
    """Whole batches at the int8 limits, unscaled extrinsic, the widest clamp: the state metrics'
    widest excursions, from equal-metric starts too."""
    _check(_pattern(family, 1024, 8), 1024, 4, DEFAULT, (255, 4))


def test_codeword_alone_equals_its_rows_in_a_batch():
    import torch
    K, iters, B = 1024, 2, 130
    x = _gpu(_awgn(K, B))
    with _codec(K, iters, DEFAULT) as c:
        le = torch.empty((B, iters, 2, K + 3), dtype=torch.int16, device=_dev())
        rows = c.decode(x, all_iters=True, le=le)
        for b in (0, 63, 64, 129):
            le1 = torch.empty((1, iters, 2, K + 3), dtype=torch.int16, device=_dev())
            r1 = c.decode(x[b:b + 1].contiguous(), all_iters=True, le=le1)
            assert torch.equal(r1[0], rows[b]) and torch.equal(le1[0], le[b]), b


def test_overlap_past_the_trellis_and_window_zero_are_the_exact_decode():
    """{16, 48} at K = 40 (overlap >= L) and one sub-block ({32, 0}: nS = 1) equal the exact GPU decode,
    {16, 0} does not, and set_fixed_window(0) returns to the exact decode's bytes."""
    K, iters, B = 40, 4, 65
    q = _awgn(K, B)
    with _codec(K, iters) as c:
        exact = _decode_all(c, q)
        assert np.array_equal(exact[0], F.decode(q, K, *QPP[K], iters)[0])
        for win in ((16, 48), (32, 0)):
            c.set_fixed_window(*win)
            for a, b in zip(_decode_all(c, q), exact):
                assert np.array_equal(a, b), win
        c.set_fixed_window(16, 0)
        got = _decode_all(c, q)
        assert (got[0] != exact[0]).any() and (got[1] != exact[1]).any()
        c.set_fixed_window(0)
        for a, b in zip(_decode_all(c, q), exact):
            assert np.array_equal(a, b)
        c.set_fixed_window(16, 0)
        from turbo_decoder_cuda_amd import _native as N
        N.check(N.lib().td_set_fixed_window(c._h, None))
        for a, b in zip(_decode_all(c, q), exact):
            assert np.array_equal(a, b)


def test_window_survives_set_fixed():
    K, iters, B = 1024, 4, 3
    with _codec(K, iters, DEFAULT) as c:
        c.set_fixed(127, 3)
        g_rows, g_le, _ = _decode_all(c, np.ascontiguousarray(_awgn(K, B, 16)))
    rows, le = _ref_awgn(K, B, iters, DEFAULT, (127, 3), 16)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le)


def test_graph_capture_after_reserve_replays_the_eager_result():
    import torch
    K, iters, B = 1024, 2, 65
    qs = [_awgn(K, 130)[:B], _awgn(K, 130)[B:]]
    ref = _ref_awgn(K, 130, iters, DEFAULT)
    sb = torch.cuda.Stream(_dev())
    with _codec(K, iters, DEFAULT) as c:
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
            sl = slice(k * B, (k + 1) * B)
            assert np.array_equal(got, ref[0][sl]) and np.array_equal(got_le, ref[1][sl])


def test_host_entry_points_counts_and_profile():
    K, iters, B = 40, 4, 5
    q = np.ascontiguousarray(_awgn(K, B))
    rows, le = _ref_awgn(K, B, iters, (16, 5))
    with _codec(K, iters, (16, 5)) as c:
        out, hle, used = c.TurboDecoding(q, return_le=True, return_iters=True)
        assert out.dtype == np.int32 and hle.dtype == np.int16
        assert np.array_equal(out, rows) and np.array_equal(hle, le) and np.array_equal(used, np.full(B, iters))
        bits, n = c.decode(_gpu(q), iters_out=True)
        assert np.array_equal(n.cpu().numpy(), np.full(B, iters)) and np.array_equal(bits.cpu().numpy(), rows[:, -1])
        c.profile(True)
        for _ in range(3):
            c.decode(_gpu(q))
        demux_ms, decode_ms, launches = c.kernel_ms()
        assert launches == 3 and decode_ms > 0 and demux_ms >= 0
        c.profile(False)


def test_rate_half_chain_through_the_windowed_decode():
    """quantise -> rate_match (E = 2K, rv 0) -> rate_dematch -> windowed decode equals the restatement on
    the dematched bytes."""
    from turbo_decoder_cuda_amd import decoder
    K, iters, B = 1024, 2, 5
    f1, f2 = QPP[K]
    flow = O.synth_batch(K, f1, f2, 1.5, 21, B)[1]
    E = 2 * K
    with _codec(K, iters, DEFAULT) as c:
        c.set_rate_matching(0)
        e1 = c.rate_match(decoder.quantise(_gpu(flow), 8), 0, E)
        buf = c.rate_dematch(e1, 0)
        want = F.dematch(F.quantise(flow, 8)[:, RM.index(K, 0, 0, E)], K, 0, 0)
        assert np.array_equal(buf.cpu().numpy(), want)
        rows, _ = FW.decode(want, K, f1, f2, iters, *DEFAULT)
        assert np.array_equal(c.decode(buf, all_iters=True).cpu().numpy(), rows)


def test_bad_arguments_and_exclusions_are_einval():
    from turbo_decoder_cuda_amd import TurboCodec
    from turbo_decoder_cuda_amd import _native as N
    L = N.lib()
    K, iters, B = 40, 2, 5
    q = np.ascontiguousarray(_awgn(K, B))

    def einval(call, who="td_set_fixed_window"):
        assert call() == N.TD_EINVAL
        msg = L.td_last_error().decode()
        assert who in msg and "TD_FIXED" in msg, msg

    def setw(c, w, g):
        p = N.TdFixedWindowParams(w, g)
        return L.td_set_fixed_window(c._h, C.byref(p))

    with _codec(K, iters, (16, 5)) as c:
        ref = _decode_all(c, q)
        assert np.array_equal(ref[0], FW.decode(q, K, *QPP[K], iters, 16, 5)[0])
        for w, g in ((8, 0), (24, 8), (-16, 0), (-1, 0), (17, 0), (16, -1), (16, 49), (32, 97)):
            einval(lambda: setw(c, w, g))
            for a, b in zip(_decode_all(c, q), ref):
                assert np.array_equal(a, b), ("a failed call changes nothing", w, g)
        # a rule cannot join a window
        for rule in (N.TD_STOP_HDA, N.TD_STOP_CRC):
            s = N.TdStopParams(rule, 1, N.CRC24B)
            einval(lambda: L.td_set_fixed_stop(c._h, C.byref(s)), "td_set_fixed_stop")
        with pytest.raises(N.TurboError):
            c.set_fixed_early_stop("hda")
        for a, b in zip(_decode_all(c, q), ref):
            assert np.array_equal(a, b)
        c.set_fixed_early_stop(None)   # turning the (absent) rule off is no error
        # td_set_window stays what it was on a fixed handle, and td_clock_read too
        w = N.TdWindowParams(16, 8, 0, 0, 1.0)
        einval(lambda: L.td_set_window(c._h, C.byref(w)), "td_set_window")
        g, ms = C.c_double(), C.c_double()
        einval(lambda: L.td_clock_read(c._h, C.byref(g), C.byref(ms)), "td_clock_read")
        # nor a window a rule
        c.set_fixed_window(0)
        c.set_fixed_early_stop("hda", min_iters=2)
        stop = c.decode(_gpu(q), all_iters=True).cpu().numpy()
        einval(lambda: setw(c, 16, 5))
        assert np.array_equal(c.decode(_gpu(q), all_iters=True).cpu().numpy(), stop), "the rule is still in force"
        assert setw(c, 0, 0) == N.TD_OK   # restoring the exact schedule is always allowed
        c.set_fixed_early_stop(None)
        c.set_fixed_window(16, 5)
        for a, b in zip(_decode_all(c, q), ref):
            assert np.array_equal(a, b)
    for prec in ("f64", "f32"):   # td_set_fixed_window belongs to fixed handles, NULL included
        with TurboCodec(K, *QPP[K], iterations=iters, algo="maxlog", precision=prec) as f:
            einval(lambda: setw(f, 16, 5))
            einval(lambda: L.td_set_fixed_window(f._h, None))
            with pytest.raises(N.TurboError) as e:
                f.set_fixed_window()
            assert e.value.code == N.TD_EINVAL


def test_default_overlap_ber_within_the_window_gate():
    """The gate of test_window_ber_close_to_exact on the fixed decoder's waterfall: K = 6144, 8 iterations,
    8 steps per unit, the same 32768 generator frames at 0.5 dB through the exact fixed schedule and
    the windowed one at the default {64, 48}.  Bit and block errors of the window within 1.1x the exact
    schedule's.  48 is the smallest measured overlap inside that gate at 0.4, 0.5 and 0.6 dB (32 is at
    1.106x the frame errors at 0.6 dB on 262144 frames): scripts/fixed_window_ber.py,
    profiles/fixed/window_ber.json, DESIGN.md "Fixed point"."""
    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    K, f1, f2, iters, frames, chunk, ebn0 = 6144, 263, 480, 8, 32768, 4096, 0.5
    res = {"exact": [0, 0], "window": [0, 0]}
    with TurboCodec(K, f1, f2, iterations=iters, algo="maxlog", precision="fixed") as ex, \
            TurboCodec(K, f1, f2, iterations=iters, algo="maxlog", precision="fixed") as win, \
            TurboCodec(K, f1, f2, iterations=iters, algo="maxlog", precision="f64") as gen:
        win.set_fixed_window()   # the Python default
        gen.synth_seed(100)
        for _ in range(frames // chunk):
            info, llr = gen.synth(chunk, ebn0)
            x = decoder.quantise(llr, 8)
            for name, c in (("exact", ex), ("window", win)):
                wrong = (c.decode(x) != info).sum(dim=1)
                res[name][0] += int(wrong.sum().item())
                res[name][1] += int((wrong > 0).sum().item())
            del info, llr, x
    print(res)
    (be, ke), (bw, kw) = res["exact"], res["window"]
    assert be > 1000 and ke > 50, res
    assert bw <= 1.1 * be and kw <= 1.1 * ke, res
