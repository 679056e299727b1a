"""LTE rate matching on the MI355X (td_rate_match / td_rate_dematch through TurboCodec): the kernels
against the numpy restatement of 36.212 5.1.4.1 (tests/ratematch_ref.py), bit for bit, and end to end
in front of the decoder against the CPU oracle."""
import functools

import numpy as np
import pytest

import pyoracle as O
import ratematch_ref as RM
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

QPP = {13: (1, 0), 28: (1, 0), 29: (1, 0), 40: (3, 10), 1024: (31, 64), 6144: (263, 480)}   # K = 13, 28, 29: identity
NP_DT = {"f64": np.float64, "f32": np.float32}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _codec(K, precision="f64", iterations=2, **kw):
    from turbo_decoder_cuda_amd import TurboCodec
    f1, f2 = QPP[K]
    return TurboCodec(K, f1, f2, iterations=iterations, precision=precision, **kw)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _soft(shape, seed, dtype):
    """Values whose sums depend on the order they are added in (so a wrong order shows)."""
    return (np.random.default_rng(seed).normal(0, 4, shape) * 1.2345678).astype(dtype)


# ------------------------------------------------------------------ rate_match: the gather
@pytest.mark.parametrize("K,B", [(K, B) for K in (13, 28, 29, 40, 1024) for B in (1, 3, 65)] + [(6144, 2)])
def test_rate_match_is_the_indexed_gather(K, B):
    n = 3 * K + 12
    rng = np.random.default_rng(K * 100 + B)
    xs = [rng.integers(0, 2, (B, n)).astype(np.uint8), _soft((B, n), K + B, np.float32), _soft((B, n), K + 7 * B, np.float64)]
    with _codec(K) as c:
        for Ncb, rv, E in ((0, 0, n), (0, 1, n // 2 + 1), (0, 3, 2 * n + 5), (RM.layout(K)[2] + 1, 2, n - 7)):
            info = c.set_rate_matching(Ncb)
            assert info["n_nonnull"] == RM.n_nonnull(K, Ncb) and info["R"] == RM.layout(K)[1]
            idx = RM.index(K, Ncb, rv, E)
            for x in xs:
                e = c.rate_match(_gpu(x), rv, E)
                assert e.dtype == _gpu(x).dtype and tuple(e.shape) == (B, E)
                assert np.array_equal(e.cpu().numpy(), x[:, idx]), (Ncb, rv, E, x.dtype)


# ------------------------------------------------------------------ rate_dematch: the transpose
def _dematch_cases(K):
    """(Ncb, rv, E): puncturing, repetition, a soft buffer of Kpi+1 and of a mid length, odd E."""
    _, _, Kpi, Kw, _ = RM.layout(K)
    mid = (Kpi + (Kw - Kpi) // 2) | 1
    nnn = RM.n_nonnull(K)
    return [(0, 0, nnn - nnn // 3), (0, 1, 2 * nnn + 5), (Kpi + 1, 2, nnn // 2 + 1), (Kpi + 1, 0, 2 * Kpi + 1),
            (mid, 3, nnn - 1), (mid, 1, 2 * RM.n_nonnull(K, mid) + 5), (0, 2, nnn), (0, 3, 1)]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("K,B", [(13, 3), (28, 3), (29, 3), (40, 3), (1024, 3), (1024, 65), (6144, 2)])
def test_rate_dematch_equals_restatement(K, B, precision):
    """B = 3 with an odd E puts the rows of e an odd number of elements apart; R = 33 (K = 1024) and
    R = 193 (K = 6144) leave a ragged last band of rows."""
    dt = NP_DT[precision]
    with _codec(K, precision) as c:
        seen_odd = False
        for Ncb, rv, E in _dematch_cases(K):
            c.set_rate_matching(Ncb)                      # called again and again with different Ncb
            e = _soft((B, E), K + E + rv, dt)
            want = RM.dematch(e, K, Ncb, rv)
            got = c.rate_dematch(_gpu(e), rv).cpu().numpy()
            assert got.dtype == dt and np.array_equal(got, want), (Ncb, rv, E)
            idx = RM.index(K, Ncb, rv, E)
            untouched = np.setdiff1d(np.arange(3 * K + 12), idx)
            assert not got[:, untouched].any() and not np.signbit(got[:, untouched]).any()
            seen_odd |= E % 2 == 1
        assert seen_odd


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("K,B,Ncb", [(40, 3, 0), (1024, 5, 0), (1024, 3, 2112), (6144, 2, 0)])
def test_harq_accumulation(K, B, Ncb, precision):
    """rv 0, 2, 3, 1 combined into one soft buffer whose prior content is not zero: each transmission
    is added onto the buffer in ascending k, exactly as the restatement does."""
    import torch
    dt = NP_DT[precision]
    n = 3 * K + 12
    nnn = RM.n_nonnull(K, Ncb)
    prior = _soft((B, n), K, dt)
    with _codec(K, precision) as c:
        c.set_rate_matching(Ncb)
        buf = _gpu(prior)
        want = prior
        for t, rv in enumerate((0, 2, 3, 1)):
            E = (nnn // 2 + 1, nnn + 7, 2 * nnn + 5, nnn // 3)[t]
            e = _soft((B, E), K + t, dt)
            want = RM.dematch(e, K, Ncb, rv, prior=want)
            out = c.rate_dematch(_gpu(e), rv, out=buf, accumulate=True)
            assert out is buf
            assert np.array_equal(buf.cpu().numpy(), want), (t, rv)
        with pytest.raises(ValueError):
            c.rate_dematch(_gpu(e), 0, accumulate=True)           # nothing to accumulate into
        with pytest.raises(ValueError):
            c.rate_dematch(_gpu(e), 0, out=buf[:, :-1].contiguous())
        with pytest.raises(ValueError):
            c.rate_dematch(_gpu(e.astype(np.float32 if dt == np.float64 else np.float64)), 0)
        with pytest.raises(ValueError):
            c.rate_match(torch.zeros((B, n - 1), dtype=torch.uint8, device=_dev()), 0, 8)
        with pytest.raises(ValueError):
            c.rate_match(torch.zeros((B, n), dtype=torch.uint8), 0, 8)   # a host tensor


def test_non_default_stream_and_reset_tables():
    """The launches follow the caller's stream, and a second td_rm_set replaces the tables."""
    import torch
    K, B = 1024, 4
    n = 3 * K + 12
    x = _soft((B, n), 5, np.float64)
    s = torch.cuda.Stream(device=_dev())
    with _codec(K) as c:
        for Ncb in (0, 2112, 0):
            c.set_rate_matching(Ncb)
            E = 1800
            idx = RM.index(K, Ncb, 2, E)
            xg = _gpu(x)
            torch.cuda.synchronize(_dev())
            with torch.cuda.stream(s):
                e = c.rate_match(xg, 2, E)                    # torch's current stream
            back = c.rate_dematch(e, 2, stream=s)             # an explicit stream
            s.synchronize()
            assert np.array_equal(e.cpu().numpy(), x[:, idx])
            assert np.array_equal(back.cpu().numpy(), RM.dematch(x[:, idx], K, Ncb, 2))


def test_errors_on_the_device_handle():
    import ctypes as C
    import torch
    from turbo_decoder_cuda_amd import _native as N
    K = 40
    n = 3 * K + 12
    x = torch.zeros((2, n), dtype=torch.float64, device=_dev())
    e = torch.zeros((2, 50), dtype=torch.float64, device=_dev())
    L = N.lib()
    px, pe = C.c_void_p(x.data_ptr()), C.c_void_p(e.data_ptr())
    with _codec(K) as c:
        h = c._h
        for rc in (L.td_rate_match(h, px, 8, 2, 0, 50, pe, None), L.td_rate_dematch(h, pe, 2, 0, 50, px, 0, None),
                   L.td_rm_info(h, None, None, None, None, None)):
            assert rc == N.TD_EINVAL and b"td_rm_set first" in L.td_last_error()
        for Ncb in (63, 193, -5):
            assert L.td_rm_set(h, Ncb) == N.TD_EINVAL and L.td_last_error().startswith(b"td_rm_set")
        c.set_rate_matching(128)
        assert c.rate_matching == {"R": 2, "Kpi": 64, "Kw": 192, "Ncb": 128, "n_nonnull": 88}
        bad = [lambda: L.td_rate_match(h, None, 8, 2, 0, 50, pe, None), lambda: L.td_rate_match(h, px, 8, 2, 0, 50, None, None),
               lambda: L.td_rate_match(h, px, 2, 2, 0, 50, pe, None), lambda: L.td_rate_match(h, px, 8, 2, 4, 50, pe, None),
               lambda: L.td_rate_match(h, px, 8, 2, -1, 50, pe, None), lambda: L.td_rate_match(h, px, 8, 2, 0, 0, pe, None),
               lambda: L.td_rate_match(h, px, 8, -1, 0, 50, pe, None), lambda: L.td_rate_dematch(h, None, 2, 0, 50, px, 0, None),
               lambda: L.td_rate_dematch(h, pe, 2, 0, 50, None, 0, None), lambda: L.td_rate_dematch(h, pe, 2, 5, 50, px, 0, None),
               lambda: L.td_rate_dematch(h, pe, 2, 0, 0, px, 0, None), lambda: L.td_rate_dematch(h, pe, -2, 0, 50, px, 0, None)]
        for f in bad:
            assert f() == N.TD_EINVAL and L.td_last_error().startswith(b"td_rate_")
        x.fill_(7.0)
        assert L.td_rate_dematch(h, pe, 0, 0, 50, px, 0, None) == N.TD_OK    # B = 0: nothing happens
        assert L.td_rate_match(h, px, 8, 0, 0, 50, pe, None) == N.TD_OK
        torch.cuda.synchronize(_dev())
        assert bool((x == 7.0).all()) and bool((e == 0.0).all())


# ------------------------------------------------------------------ in front of the decoder
def test_identity_and_decode_unchanged():
    """Ncb = Kw, rv 0, E = 3K+12: every position is sent once, so de-matching the matched LLRs gives
    them back and the decode of that is the decode of the original, bit for bit."""
    K, B = 1024, 8
    n = 3 * K + 12
    _, llr = O.make_frames(K, 31, 64, 1.0, 3, B)
    with _codec(K, iterations=4) as c:
        c.set_rate_matching(0)
        x = _gpu(llr)
        back = c.rate_dematch(c.rate_match(x, 0, n), 0)
        assert np.array_equal(back.cpu().numpy(), llr)
        assert np.array_equal(c.decode(back, all_iters=True).cpu().numpy(), c.decode(x, all_iters=True).cpu().numpy())


@functools.lru_cache(maxsize=None)
def _frames(ebn0):
    return O.make_frames(1024, 31, 64, ebn0, 7, 32)


def _gpu_decode_of(c, txs):
    """txs: (rv, e) transmissions combined in order into one soft buffer on the GPU -> decoded bits."""
    buf = None
    for rv, e in txs:
        buf = c.rate_dematch(_gpu(e), rv) if buf is None else c.rate_dematch(_gpu(e), rv, out=buf, accumulate=True)
    return c.decode(buf).cpu().numpy()


def _oracle_decode_of(txs, Ncb):
    buf = None
    for rv, e in txs:
        buf = RM.dematch(e, 1024, Ncb, rv, prior=buf)
    return O.decode_batch(buf, 1024, 31, 64, 8, nthreads=4)


def test_end_to_end_rate_half():
    """(a) rate ~ 1/2: rv 0, E = 2064 at 4.0 dB -- every info bit recovered (the CPU oracle: 0 of 32
    frames in error at 3.0 and 4.0 dB, 32 of 32 at 2.0 dB)."""
    src, llr = _frames(4.0)
    txs = [(0, llr[:, RM.index(1024, 0, 0, 2064)])]
    with _codec(1024, iterations=8) as c:
        c.set_rate_matching(0)
        bits = _gpu_decode_of(c, txs)
    assert np.array_equal(bits, _oracle_decode_of(txs, 0))
    assert np.array_equal(bits, src.astype(np.uint8))


def test_end_to_end_harq():
    """(b) HARQ at 2.0 dB, E = 1600 per transmission: rv 0 alone leaves frames in error (the CPU oracle:
    32 of 32); rv 0 and rv 2 combined with accumulate recover every info bit (oracle: 0 of 32 at 1.0,
    2.0 and 3.0 dB)."""
    src, llr = _frames(2.0)
    t0 = (0, llr[:, RM.index(1024, 0, 0, 1600)])
    t2 = (2, llr[:, RM.index(1024, 0, 2, 1600)])
    with _codec(1024, iterations=8) as c:
        c.set_rate_matching(0)
        alone = _gpu_decode_of(c, [t0])
        both = _gpu_decode_of(c, [t0, t2])
    assert np.array_equal(alone, _oracle_decode_of([t0], 0))
    assert np.array_equal(both, _oracle_decode_of([t0, t2], 0))
    assert (alone != src).any(axis=1).sum() >= 1
    assert np.array_equal(both, src.astype(np.uint8))


def test_end_to_end_limited_buffer():
    """(c) limited buffer: Ncb = 2112, rv 0, E = 2400 (the transmission wraps round the soft buffer) at
    4.0 dB -- every info bit recovered (the CPU oracle: 0 of 32 at 4.0 dB, 8 of 32 in error at 3.0 dB)."""
    src, llr = _frames(4.0)
    txs = [(0, llr[:, RM.index(1024, 2112, 0, 2400)])]
    with _codec(1024, iterations=8) as c:
        c.set_rate_matching(2112)
        bits = _gpu_decode_of(c, txs)
    assert np.array_equal(bits, _oracle_decode_of(txs, 2112))
    assert np.array_equal(bits, src.astype(np.uint8))
