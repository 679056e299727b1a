"""The closed loop on the MI355X, every step on device-resident data: crc_attach -> encode -> rate_match ->
modulate -> (no noise) -> demodulate -> rate_dematch -> decode with the CRC stop rule.  The frames are
noiseless, so no BER is asserted: the decoded bits are the attached rows, after one iteration."""
import numpy as np
import pytest

from conftest import gpu_available
from turbo_decoder_cuda_amd import _native as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

QPP = {40: (3, 10), 6144: (263, 480)}
B, ITERS = 65, 4


def _dev():
    import torch
    return torch.device("cuda", 0)


def _codec(K):
    from turbo_decoder_cuda_amd import TurboCodec
    return TurboCodec(K, *QPP[K], iterations=ITERS, algo="logmap", precision="f64")


def _attached(c, K, seed):
    """Random payloads with gCRC24B attached on the device: (the tensor, its host copy)."""
    import torch
    rows = np.random.default_rng(seed).integers(0, 2, (B, K), dtype=np.uint8)
    t = torch.from_numpy(rows).to(_dev())
    c.set_crc(N.CRC24B)
    c.crc_attach(t)
    att = t.cpu().numpy()
    assert np.array_equal(att[:, :K - 24], rows[:, :K - 24])
    return t, att


def _over_the_air(c, coded, rv, E):
    """rate_match -> BPSK -> demodulate: the received soft values [B, E] of one noiseless transmission."""
    from turbo_decoder_cuda_amd.decoder import demodulate, modulate
    e = c.rate_match(coded, rv, E)
    si, sq = modulate(e.reshape(-1), 1)
    return demodulate(si, sq, 1, 1.0).view(B, E)


@pytest.mark.parametrize("K", [40, 6144])
def test_closed_loop_full_rate(K):
    n = 3 * K + 12
    with _codec(K) as c:
        bits_in, att = _attached(c, K, K)
        c.set_rate_matching(0)
        c.set_early_stop("crc", crc_poly=N.CRC24B)
        llr = c.rate_dematch(_over_the_air(c, c.encode(bits_in), 0, n), 0)
        bits, used = c.decode(llr, iters_out=True)
        assert np.array_equal(bits.cpu().numpy(), att)
        assert (used.cpu().numpy() == 1).all()
        assert not c.crc_check(bits).cpu().numpy().any()


def test_closed_loop_two_transmissions():
    """K = 6144 at E = 2K: rv 0, then rv 2 combined into the soft buffer."""
    K = 6144
    with _codec(K) as c:
        bits_in, att = _attached(c, K, 99)
        c.set_rate_matching(0)
        c.set_early_stop("crc", crc_poly=N.CRC24B)
        coded = c.encode(bits_in)
        llr = c.rate_dematch(_over_the_air(c, coded, 0, 2 * K), 0)
        c.rate_dematch(_over_the_air(c, coded, 2, 2 * K), 2, out=llr, accumulate=True)
        bits = c.decode(llr)
        assert np.array_equal(bits.cpu().numpy(), att)
        assert not c.crc_check(bits).cpu().numpy().any()
