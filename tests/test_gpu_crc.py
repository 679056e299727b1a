"""The device CRC-24 (td_crc_set / td_crc_attach / td_crc_check through TurboCodec) on the MI355X, against
td_crc24_host, and its independence from the early-termination rules' polynomial."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as O
import window_stop_cases as W
from conftest import gpu_available
from turbo_decoder_cuda_amd import _native as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

QPP = {25: (1, 0), 40: (3, 10), 65: (2, 0), 6144: (263, 480)}   # 25: the identity (no other QPP is tried here)
POLYS = [N.CRC24A, N.CRC24B]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _codec(K, **kw):
    from turbo_decoder_cuda_amd import TurboCodec
    return TurboCodec(K, *QPP[K], **kw)


def _host(rows, poly):
    L, K = N.lib(), rows.shape[1]
    return np.array([L.td_crc24_host(np.ascontiguousarray(r).ctypes.data_as(C.c_void_p), K, poly) for r in rows],
                    dtype=np.int64)


def _rows(K, B, seed):
    rows = np.random.default_rng(seed).integers(0, 2, (B, K), dtype=np.uint8)
    rows[B // 2] *= 0x80   # any non-zero byte is a 1
    return rows


@pytest.mark.parametrize("K", [25, 40, 65, 6144])
def test_check_equals_the_host_crc(K):
    """B = 1, 65, 257: one wave, a ragged last workgroup, several; odd K puts rows at odd addresses."""
    with _codec(K, iterations=2) as c:
        for poly in POLYS:
            c.set_crc(poly)   # called again with the other polynomial
            for B in (1, 65, 257):
                rows = _rows(K, B, K + B)
                got = c.crc_check(_gpu(rows)).cpu().numpy().astype(np.int64)
                assert np.array_equal(got, _host(rows, poly)), (poly, B)


@pytest.mark.parametrize("K", [25, 40, 65, 6144])
def test_attach_overwrites_the_last_24_and_any_flip_shows(K):
    import torch
    B = 65
    with _codec(K, iterations=2) as c:
        for poly in POLYS:
            c.set_crc(poly)
            rows = _rows(K, B, 7 * K + 1)
            rows[:, K - 24:] = 0xA5   # garbage where the CRC goes
            t = _gpu(rows)
            assert c.crc_attach(t) is t
            att = t.cpu().numpy()
            assert np.array_equal(att[:, :K - 24], rows[:, :K - 24]) and att[:, K - 24:].max() <= 1
            for b in (0, B // 2, B - 1):   # the payload's CRC, most significant bit first
                crc = W.crc24((rows[b, :K - 24] != 0).astype(int), poly)
                assert [int(v) for v in att[b, K - 24:]] == [(crc >> (23 - j)) & 1 for j in range(24)]
            assert not _host(att, poly).any()
            assert not c.crc_check(t).cpu().numpy().any()
            for pos in (0, K - 25, K - 24, K - 1):
                bad = att.copy()
                bad[:, pos] = att[:, pos] == 0   # the bit's flip, whatever non-zero byte stood for a 1
                got = c.crc_check(_gpu(bad)).cpu().numpy().astype(np.int64)
                assert got.all() and np.array_equal(got, _host(bad, poly)), pos
            torch.cuda.synchronize()


def test_crc_table_is_independent_of_the_stop_rule():
    """td_crc_set(gCRC24A), then the CRC stop rule with gCRC24B: crc_check keeps A and the decode stops on
    B; clearing the rule leaves crc_check working, and a later td_crc_set leaves the rule its B."""
    K, B, iters = 40, 16, 4
    f1, f2 = QPP[K]
    flow = W.crc_frames(K, f1, f2, N.CRC24B, 0.6, B)        # frames that carry gCRC24B
    rows = O.decode_batch(np.ascontiguousarray(flow), K, f1, f2, iters, nthreads=4).astype(np.uint8)
    assert not _host(rows, N.CRC24B).any() and _host(rows, N.CRC24A).any(), "the frames decode; A does not pass them"
    probe = _rows(K, 33, 5)
    with _codec(K, iterations=iters) as c:
        c.set_crc(N.CRC24A)
        c.set_early_stop("crc", crc_poly=N.CRC24B)
        assert np.array_equal(c.crc_check(_gpu(probe)).cpu().numpy().astype(np.int64), _host(probe, N.CRC24A))
        bits, used = c.decode(_gpu(flow), iters_out=True)
        used = used.cpu().numpy()
        assert np.array_equal(bits.cpu().numpy(), rows) and (used < iters).any(), "the decode stops on gCRC24B"
        assert np.array_equal(c.crc_check(bits).cpu().numpy().astype(np.int64), _host(rows, N.CRC24A))
        c.set_early_stop(None)
        assert np.array_equal(c.crc_check(_gpu(probe)).cpu().numpy().astype(np.int64), _host(probe, N.CRC24A))
        c.set_early_stop("crc", crc_poly=N.CRC24B)
        c.set_crc(N.CRC24B)                                  # the reverse: the rule's table is its own
        c.set_crc(N.CRC24A)
        _, used2 = c.decode(_gpu(flow), iters_out=True)
        assert np.array_equal(used2.cpu().numpy(), used)
