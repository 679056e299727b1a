"""Rate matching on the MI355X with more codewords than grid rows.  The kernels cap their grid's y
dimension (kRmGridY = 512 of rate_dematch_kernel, the 512 of launch_fixed_dematch, the 65535 of
launch_match_t) and let the codewords beyond it share a workgroup through a batch-stride loop; in
rate_dematch_kernel a double-buffered LDS tile and its barriers sit inside that loop.  Batches of

  513    two trips for one workgroup, one for the rest
  1100   a mix of two and three trips
  1537   four trips for one workgroup, three for the rest: both tile buffers are reused
  65600  (rate_match) two trips for 65 workgroups

against the references of test_gpu_ratematch.py and test_gpu_fixed.py, bit for bit."""
import numpy as np
import pytest

import fixed_ref as F
import ratematch_ref as RM
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

QPP = {13: (2, 0), 40: (3, 10), 1024: (31, 64)}
NP_DT = {"f64": np.float64, "f32": np.float32}
SHAPES = [(40, 513), (40, 1100), (40, 1537), (1024, 1100)]   # K = 40: R = 2, one ragged band; K = 1024: R = 33, three


def _dev():
    import torch
    return torch.device("cuda", 0)


def _codec(K, precision="f64", **kw):
    from turbo_decoder_cuda_amd import TurboCodec
    return TurboCodec(K, *QPP[K], iterations=2, precision=precision, **kw)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _soft(shape, seed, dtype):
    """Values whose sums depend on the order they are added in, different in every codeword."""
    return (np.random.default_rng(seed).normal(0, 4, shape) * 1.2345678).astype(dtype)


def _mid(K):
    _, _, Kpi, Kw, _ = RM.layout(K)
    return (Kpi + (Kw - Kpi) // 2) | 1


def _dematch_cases(K):
    """(Ncb, rv, E): punctured and repeated (odd E), on the whole buffer and on a limited one; four rv."""
    nnn, mid = RM.n_nonnull(K), _mid(K)
    return [(0, 0, nnn - nnn // 3), (0, 1, 2 * nnn + 5), (mid, 3, nnn - 1), (mid, 2, 2 * RM.n_nonnull(K, mid) + 5)]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("K,B", SHAPES)
def test_rate_dematch_past_the_grid_cap(K, B, precision):
    """Every codeword of the batch, without accumulate (positions nothing selects are +0.0) and
    accumulated onto a non-zero prior (a tile preload and a second barrier per trip)."""
    dt = NP_DT[precision]
    n = 3 * K + 12
    assert B > 512
    with _codec(K, precision) as c:
        for Ncb, rv, E in _dematch_cases(K):
            c.set_rate_matching(Ncb)
            e = _soft((B, E), K + E + rv, dt)
            assert e.nbytes + B * n * e.itemsize < 100e6
            eg = _gpu(e)
            want = RM.dematch(e, K, Ncb, rv)
            got = c.rate_dematch(eg, rv).cpu().numpy()
            assert got.dtype == dt
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (Ncb, rv, E, "codewords", bad[:8], "of", bad.size)
            untouched = np.setdiff1d(np.arange(n), RM.index(K, Ncb, rv, E))
            assert not got[:, untouched].any() and not np.signbit(got[:, untouched]).any()
            prior = _soft((B, n), K + E, dt)
            buf = _gpu(prior)
            c.rate_dematch(eg, rv, out=buf, accumulate=True)
            want = RM.dematch(e, K, Ncb, rv, prior=prior)
            bad = np.flatnonzero((buf.cpu().numpy() != want).any(axis=1))
            assert bad.size == 0, (Ncb, rv, E, "accumulate: codewords", bad[:8], "of", bad.size)


def _bytes(shape, seed):
    return np.random.default_rng(seed).integers(-128, 128, shape).astype(np.int8)


@pytest.mark.parametrize("K,B", SHAPES)
def test_rate_dematch_int8_past_the_grid_cap(K, B):
    """The whole int8 range in, so the saturation after every addition decides bytes (E = 5K repeats
    every position), and accumulation onto a prior that holds -128 and values near the limits."""
    import torch
    n = 3 * K + 12
    with _codec(K, "fixed", algo="maxlog") as c:
        for Ncb, rv, E in ((0, 0, 5 * K), (0, 3, 2 * K), (_mid(K), 1, 5 * K), (_mid(K), 2, 2 * K + 1)):
            c.set_rate_matching(Ncb)
            e = _bytes((B, E), K + E + rv)
            eg = _gpu(e)
            got = c.rate_dematch(eg, rv)
            assert got.dtype == torch.int8
            want = F.dematch(e, K, Ncb, rv)
            if E == 5 * K:
                assert (np.abs(want.astype(np.int32)) == 127).mean() > 0.05, "the sums saturate"
            bad = np.flatnonzero((got.cpu().numpy() != want).any(axis=1))
            assert bad.size == 0, (Ncb, rv, E, "codewords", bad[:8], "of", bad.size)
            prior = _bytes((B, n), 7 * K + E + rv)
            prior[:, ::5] = -128
            prior[:, 1::7] = 126
            prior[:, 2::11] = -127
            buf = _gpu(prior)
            c.rate_dematch(eg, rv, out=buf, accumulate=True)
            want = F.dematch(e, K, Ncb, rv, prior=prior)
            bad = np.flatnonzero((buf.cpu().numpy() != want).any(axis=1))
            assert bad.size == 0, (Ncb, rv, E, "accumulate: codewords", bad[:8], "of", bad.size)


@pytest.mark.parametrize("elem", [1, 4, 8])
def test_rate_match_past_the_grid_cap(elem):
    """65600 codewords of K = 13 (3K + 12 = 51): 65 workgroups of each grid column take a second trip."""
    K, B = 13, 65600
    n = 3 * K + 12
    assert B > 65535
    x = {1: lambda: np.random.default_rng(1).integers(0, 256, (B, n)).astype(np.uint8),
         4: lambda: _soft((B, n), 4, np.float32), 8: lambda: _soft((B, n), 8, np.float64)}[elem]()
    assert x.itemsize == elem
    xg = _gpu(x)
    with _codec(K) as c:
        c.set_rate_matching(0)
        for rv, E in ((1, n // 2 + 1), (3, 2 * n + 5)):
            got = c.rate_match(xg, rv, E)
            assert got.dtype == xg.dtype and tuple(got.shape) == (B, E)
            bad = np.flatnonzero((got.cpu().numpy() != x[:, RM.index(K, 0, rv, E)]).any(axis=1))
            assert bad.size == 0, (rv, E, "codewords", bad[:8], "of", bad.size)
