"""The fused receive front end on the MI355X (td_llr_convert, td_demod_dematch through convert_llr and
TurboCodec.demod_dematch): byte for byte the three calls it replaces -- demodulate, convert_llr, rate_dematch
-- and the numpy restatement (tests/frontend_ref.py), in front of the decoder, with HARQ accumulation, past
the launch's grid cap and captured into a graph."""
import functools

import numpy as np
import pytest

import frontend_ref as FR
import pyoracle as O
import ratematch_ref as RM
from conftest import gpu_available
from turbo_decoder_cuda_amd import _native as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

QPP = {13: (1, 0), 29: (1, 0), 40: (3, 10), 1024: (31, 64), 6144: (263, 480)}   # K = 13, 29: identity
PRECS = ("f64", "f32", "fixed")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _codec(K, precision="f64", iterations=2, **kw):
    from turbo_decoder_cuda_amd import TurboCodec
    kw.setdefault("algo", "maxlog" if precision == "fixed" else "logmap")
    return TurboCodec(K, *QPP[K], iterations=iterations, precision=precision, **kw)


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a)).to(_dev())   # (a copy: the shared references are read-only)


def _same_bits(a, b):
    """Equal as bytes: for floats that includes the sign of zero."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _three_calls(c, yi, yq, rv, E, M, s=8.0, out=None, accumulate=False):
    """The definition on the device: demodulate -> convert_llr -> rate_dematch."""
    from turbo_decoder_cuda_amd import convert_llr, demodulate
    e = convert_llr(demodulate(yi, yq, M, FR.KF).view(yi.shape[0], E), c.precision, s)
    return c.rate_dematch(e, rv, out=out, accumulate=accumulate)


@functools.lru_cache(maxsize=None)
def _demapped(K, B, M, t, E):
    """Case t's symbols and their float64 LLRs [B, E] by the oracle: computed once, shared by the precisions."""
    yi, yq = FR.symbols((B, E // M), 1000 * K + 10 * t + M)
    llr = O.demodulate(yi.reshape(-1), yq.reshape(-1), M, FR.KF).reshape(B, E)
    for a in (yi, yq, llr):
        a.setflags(write=False)
    return yi, yq, llr


def _prior(shape, seed, precision):
    rng = np.random.default_rng(seed)
    if precision == "fixed":
        return rng.integers(-127, 128, shape).astype(np.int8)
    return (rng.normal(0, 4, shape) * 1.2345678).astype(FR.NP_DT[precision])


# ------------------------------------------------------------------ convert_llr
@pytest.mark.parametrize("precision", PRECS)
def test_convert_llr_equals_torch(precision):
    """Sizes around a wave and the vector width, one with many workgroups; then the same with the input 8 bytes
    off a 16-byte boundary and the output one element off (int8: 1 byte), which takes the element-wide path."""
    import torch
    from turbo_decoder_cuda_amd import convert_llr, quantise
    dt = {"f64": torch.float64, "f32": torch.float32, "fixed": torch.int8}[precision]
    for n in (1, 63, 64, 65, 1001, 200003):
        x = _gpu(np.random.default_rng(n).normal(0, 9, n + 1))
        want = quantise(x, 8.0) if precision == "fixed" else x.to(dt)
        got = convert_llr(x[:n], precision, 8.0)
        assert got.dtype == dt and torch.equal(got, want[:n]), n
        buf = torch.full((n + 2,), 77, dtype=dt, device=_dev())
        out = convert_llr(x[1:], precision, 8.0, out=buf[1:n + 1])
        assert out.data_ptr() == buf.data_ptr() + buf.element_size()
        assert torch.equal(buf[1:n + 1], want[1:]) and buf[0] == 77 and buf[n + 1] == 77, n   # nothing past the ends
    assert convert_llr(x[:0], precision).numel() == 0


def test_convert_llr_ties_overflow_and_errors():
    import torch
    from turbo_decoder_cuda_amd import convert_llr, quantise
    x = FR.tie_vector(8.0)
    g = _gpu(x)
    q = convert_llr(g, "fixed", 8.0).cpu().numpy()
    assert np.array_equal(q, FR.convert(x, "fixed", 8.0)) and q.min() >= -127
    fin = np.isfinite(x)
    assert np.array_equal(q[fin], quantise(g, 8.0).cpu().numpy()[fin])          # Python's quantiser on the finite entries
    assert q[np.isinf(x)].tolist() == [127, -127]
    assert _same_bits(convert_llr(g, "f32").cpu().numpy(), FR.convert(x, "f32"))   # +-inf past the float range, -0 kept
    assert _same_bits(convert_llr(g, "f64").cpu().numpy(), x)
    for s in (0.0, -1.0, float("inf")):
        with pytest.raises(N.TurboError):
            convert_llr(g, "fixed", s)
    convert_llr(g, "f32", 0.0)                                                    # ignored off the fixed precision
    with pytest.raises(ValueError):
        convert_llr(g.to(torch.float32), "f32")
    with pytest.raises(ValueError):
        convert_llr(g.cpu(), "f32")
    with pytest.raises(ValueError):
        convert_llr(g, "f32", out=torch.empty(x.size, dtype=torch.float64, device=_dev()))
    with pytest.raises(ValueError):
        convert_llr(g, "bf16")


# ------------------------------------------------------------------ demod_dematch against its definition
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("K,B", [(13, 3), (29, 3), (40, 1), (40, 65), (1024, 3), (6144, 2)])
@pytest.mark.parametrize("M", FR.MODS)
def test_demod_dematch_equals_the_three_calls_and_the_restatement(M, K, B, precision):
    """B = 3 with an odd number of symbols a codeword puts the rows an odd number of elements apart; R = 33
    (K = 1024) and R = 193 (K = 6144) leave a ragged last band of rows."""
    n = 3 * K + 12
    with _codec(K, precision) as c:
        for t, (Ncb, rv, E) in enumerate(FR.cases(K, M)):
            c.set_rate_matching(Ncb)
            yi, yq, llr = _demapped(K, B, M, t, E)
            gi, gq = _gpu(yi), _gpu(yq)
            want = (FR.FX if precision == "fixed" else RM).dematch(FR.convert(llr, precision), K, Ncb, rv)
            got = c.demod_dematch(gi, gq, rv, E, M, FR.KF).cpu().numpy()
            assert _same_bits(got, _three_calls(c, gi, gq, rv, E, M).cpu().numpy()), (Ncb, rv, E)
            assert got.dtype == FR.NP_DT[precision] and np.array_equal(got, want), (Ncb, rv, E)
            untouched = np.setdiff1d(np.arange(n), RM.index(K, Ncb, rv, E))
            assert not got[:, untouched].any()
            if precision != "fixed":   # +0.0 where nothing was selected, as td_rate_dematch leaves it
                assert not np.signbit(got[:, untouched]).any()


@pytest.mark.parametrize("M", [2, 6])
def test_demod_dematch_fixed_saturates_at_40_steps(M):
    """Repetition sums of values quantised at 40 steps a unit hit the +-127 clamp -- some, not all."""
    K, B = 40, 65
    Ncb, rv, E = FR.cases(K, M)[1]   # E > 2 Nnn
    yi, yq = FR.symbols((B, E // M), 77 + M)
    with _codec(K, "fixed") as c:
        c.set_rate_matching(Ncb)
        gi, gq = _gpu(yi), _gpu(yq)
        got = c.demod_dematch(gi, gq, rv, E, M, FR.KF, steps_per_unit=40.0).cpu().numpy()
        assert np.array_equal(got, _three_calls(c, gi, gq, rv, E, M, s=40.0).cpu().numpy())
        assert np.array_equal(got, FR.restate(yi, yq, M, "fixed", K, Ncb, rv, steps_per_unit=40.0))
        sat = np.abs(got.astype(int)) == 127
        assert sat.any() and not sat.all() and (got == 127).any() and (got == -127).any() and got.min() >= -127
        single = FR.values(yi, yq, M, "fixed", 40.0)   # ... and the clamp was the sums', not only the quantiser's
        assert (np.abs(single.astype(int)) < 127).mean() > 0.5


# ------------------------------------------------------------------ HARQ
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("K,B,Ncb", [(40, 3, 0), (1024, 2, 1100)])
def test_harq_accumulation(K, B, Ncb, precision):
    """rv 0, 2, 3, 1 into one soft buffer whose prior content is not zero (int8: with a -128 in it, at a
    position the first transmission selects and at one it does not), a different modulation each time."""
    n = 3 * K + 12
    nnn = RM.n_nonnull(K, Ncb)
    prior = _prior((B, n), K, precision)
    with _codec(K, precision) as c:
        c.set_rate_matching(Ncb)
        if precision == "fixed":
            E0 = nnn // 2 + 1 + (nnn // 2 + 1) % 2
            idx0 = RM.index(K, Ncb, 0, E0)
            prior[0, idx0[0]] = -128
            prior[1, np.setdiff1d(np.arange(n), idx0)[0]] = -128
        buf, ref = _gpu(prior), _gpu(prior)
        want = prior
        for t, (rv, M) in enumerate(((0, 2), (2, 6), (3, 3), (1, 4))):
            E = -(-(nnn // 2 + 1, nnn + 7, 2 * nnn + 5, nnn // 3)[t] // M) * M
            yi, yq = FR.symbols((B, E // M), K + t)
            gi, gq = _gpu(yi), _gpu(yq)
            want = FR.restate(yi, yq, M, precision, K, Ncb, rv, prior=want)
            out = c.demod_dematch(gi, gq, rv, E, M, FR.KF, out=buf, accumulate=True)
            assert out is buf
            _three_calls(c, gi, gq, rv, E, M, out=ref, accumulate=True)
            assert _same_bits(buf.cpu().numpy(), ref.cpu().numpy()), (t, rv)
            assert np.array_equal(buf.cpu().numpy(), want), (t, rv)


# ------------------------------------------------------------------ past the grid cap
@pytest.mark.parametrize("precision", ["f32", "fixed"])
@pytest.mark.parametrize("B", [513, 1100])
def test_demod_dematch_past_the_grid_cap(B, precision):
    """More than 512 codewords: the later ones share a workgroup with the earlier."""
    K, M = 40, 2
    Ncb, rv, E = FR.cases(K, M)[1]
    yi, yq = FR.symbols((B, E // M), B)
    with _codec(K, precision) as c:
        c.set_rate_matching(Ncb)
        gi, gq = _gpu(yi), _gpu(yq)
        got = c.demod_dematch(gi, gq, rv, E, M, FR.KF).cpu().numpy()
        assert _same_bits(got, _three_calls(c, gi, gq, rv, E, M).cpu().numpy())
        assert np.array_equal(got, FR.restate(yi, yq, M, precision, K, Ncb, rv))
        prior = _prior(got.shape, B, precision)
        buf = _gpu(prior)
        c.demod_dematch(gi, gq, rv, E, M, FR.KF, out=buf, accumulate=True)
        assert np.array_equal(buf.cpu().numpy(), FR.restate(yi, yq, M, precision, K, Ncb, rv, prior=prior))


# ------------------------------------------------------------------ in front of the decoder
def _received(c, K, B, M, seed, sigma=0.25):
    """crc_attach -> encode -> rate_match (rv 0, E = 3K+12) -> modulate -> noise of a fixed seed: the symbols
    [B, E / M] of one transmission that decodes, and the rows that were sent."""
    import torch
    from turbo_decoder_cuda_amd import modulate
    E = 3 * K + 12
    rows = _gpu(np.random.default_rng(seed).integers(0, 2, (B, K), dtype=np.uint8))
    c.set_crc(N.CRC24B)
    c.crc_attach(rows)
    si, sq = modulate(c.rate_match(c.encode(rows), 0, E).reshape(-1), M)
    g = torch.Generator(device="cpu").manual_seed(seed)
    noise = torch.randn((2, B, E // M), generator=g, dtype=torch.float64).to(_dev()) * sigma
    return si.view(B, E // M) + noise[0], sq.view(B, E // M) + noise[1], rows.cpu().numpy()


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("K", [40, 1024])
def test_fused_buffer_decodes_like_the_three_calls(K, precision):
    B, M, E, sigma = 3, 2, 3 * K + 12, 0.25
    Kf = 1 / (2 * sigma ** 2)
    from turbo_decoder_cuda_amd import convert_llr, demodulate
    with _codec(K, precision, iterations=4) as c:
        if precision == "fixed":
            c.set_fixed_window(64, 48)
        c.set_rate_matching(0)
        yi, yq, sent = _received(c, K, B, M, K + 1, sigma)
        fused = c.demod_dematch(yi, yq, 0, E, M, Kf, steps_per_unit=4.0)
        e = convert_llr(demodulate(yi, yq, M, Kf).view(B, E), precision, 4.0)
        three = c.rate_dematch(e, 0)
        assert _same_bits(fused.cpu().numpy(), three.cpu().numpy())
        bits = c.decode(fused).cpu().numpy()
        assert np.array_equal(bits, c.decode(three).cpu().numpy())
        assert np.array_equal(bits, sent)


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("precision", ["f32", "fixed"])
def test_demod_dematch_and_decode_captured_into_a_graph(precision):
    import torch
    K, B, M, E, sigma = 1024, 3, 4, 3 * 1024 + 12, 0.2
    Kf = 1 / (2 * sigma ** 2)
    dev = _dev()
    sb = torch.cuda.Stream(dev)
    with _codec(K, precision, iterations=3) as c:
        c.set_rate_matching(0)
        c.reserve(B)
        sym = [_received(c, K, B, M, 50 + k, sigma)[:2] for k in range(2)]
        gi, gq = sym[0][0].clone(), sym[0][1].clone()
        soft = torch.empty((B, 3 * K + 12), dtype=c._torch_dtypes()[0], device=dev)
        gout = torch.empty((B, K), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sb):
            c.demod_dematch(gi, gq, 0, E, M, Kf, steps_per_unit=4.0, out=soft, stream=sb)
            c.decode(soft, gout, stream=sb)
        replayed = []
        for k in (1, 0):
            gi.copy_(sym[k][0])
            gq.copy_(sym[k][1])
            graph.replay()
            torch.cuda.synchronize()
            replayed.append((soft.cpu().numpy().copy(), gout.cpu().numpy().copy()))
        for (s, b), k in zip(replayed, (1, 0)):
            eager = c.demod_dematch(sym[k][0], sym[k][1], 0, E, M, Kf, steps_per_unit=4.0)
            assert _same_bits(s, eager.cpu().numpy()), k
            assert np.array_equal(b, c.decode(eager).cpu().numpy()), k
        assert not np.array_equal(replayed[0][0], replayed[1][0])


# ------------------------------------------------------------------ errors
def test_demod_dematch_errors():
    import torch
    K, B, M, E = 40, 3, 2, 64
    yi, yq = (_gpu(a) for a in FR.symbols((B, E // M), 5))
    with _codec(K, "f32") as c:
        with pytest.raises(N.TurboError):
            c.demod_dematch(yi, yq, 0, E, M, FR.KF)                       # before set_rate_matching
        c.set_rate_matching(0)
        c.demod_dematch(yi, yq, 0, E, M, FR.KF, steps_per_unit=0.0)        # ignored on a float handle
        c.demod_dematch(yi, yq, 0, E, M, FR.KF, steps_per_unit=-3.0)
        with pytest.raises((ValueError, N.TurboError)):
            c.demod_dematch(yi[:, :21].contiguous(), yq[:, :21].contiguous(), 0, 63, 2, FR.KF)   # E not a multiple of M
        with pytest.raises((ValueError, N.TurboError)):
            c.demod_dematch(yi[:, :13].contiguous(), yq[:, :13].contiguous(), 0, 65, 5, FR.KF)   # M = 5
        with pytest.raises(ValueError):
            c.demod_dematch(yi.cpu(), yq.cpu(), 0, E, M, FR.KF)           # host tensors
        with pytest.raises(ValueError):
            c.demod_dematch(yi.float(), yq.float(), 0, E, M, FR.KF)       # float32 symbols
        with pytest.raises(ValueError):
            c.demod_dematch(yi, yq[:, :-1].contiguous(), 0, E, M, FR.KF)
        with pytest.raises(ValueError):
            c.demod_dematch(yi, yq, 0, E, M, FR.KF, out=torch.empty((B, 132), dtype=torch.float64, device=_dev()))
        with pytest.raises(ValueError):
            c.demod_dematch(yi, yq, 0, E, M, FR.KF, accumulate=True)      # nothing to accumulate into
        with pytest.raises(N.TurboError):
            c.demod_dematch(yi, yq, 4, E, M, FR.KF)                       # rv
        # the C entry point's own checks, past Python's
        L, p = N.lib(), lambda t: t.data_ptr()
        out = torch.empty((B, 132), dtype=torch.float32, device=_dev())
        assert L.td_demod_dematch(c._h, p(yi), p(yq), B, 0, 63, 2, FR.KF, 8.0, p(out), 0, None) == N.TD_EINVAL
        assert L.td_demod_dematch(c._h, p(yi), p(yq), B, 0, 65, 5, FR.KF, 8.0, p(out), 0, None) == N.TD_EINVAL
        assert L.td_demod_dematch(c._h, p(yi), None, B, 0, E, M, FR.KF, 8.0, p(out), 0, None) == N.TD_EINVAL
        assert L.td_demod_dematch(c._h, p(yi), p(yq), 0, 0, E, M, FR.KF, 8.0, p(out), 0, None) == N.TD_OK   # B = 0
    with _codec(K, "fixed") as c:
        c.set_rate_matching(0)
        for s in (0.0, -8.0, float("nan")):
            with pytest.raises(N.TurboError):
                c.demod_dematch(yi, yq, 0, E, M, FR.KF, steps_per_unit=s)
        assert c.demod_dematch(yi, yq, 0, E, M, FR.KF).dtype == torch.int8
