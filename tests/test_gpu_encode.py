"""The batched device encoder (td_encode_device through TurboCodec.encode) on the MI355X: byte for byte
against pyoracle.encode at every size, batch and alignment; against the frame generator that is
bit-identical to the reference; inside a captured graph; and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import encode_cases as E
from conftest import gpu_available
from turbo_decoder_cuda_amd import _native as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

GUARD = 0xA5
PAD = 64


def _dev():
    import torch
    return torch.device("cuda", 0)


def _codec(K, precision="f64", **kw):
    from turbo_decoder_cuda_amd import TurboCodec
    f1, f2 = E.interleaver(K)
    algo = "maxlog" if precision == "fixed" else "logmap"
    return TurboCodec(K, f1, f2, iterations=2, precision=precision, algo=algo, **kw)


def _guarded(rows_np, offset):
    """rows [B, n] copied into a buffer of guard bytes, `offset` bytes in: (the [B, n] view, the buffer)."""
    import torch
    B, n = rows_np.shape
    buf = torch.full((offset + B * n + PAD,), GUARD, dtype=torch.uint8, device=_dev())
    view = buf[offset:offset + B * n].view(B, n)
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows_np)).to(_dev()))
    return view, buf


def _encode_guarded(c, info, offset):
    """encode through guarded input and output buffers `offset` bytes off their allocation's start; checks
    both guard bands and the input, returns the coded bytes."""
    import torch
    B, K = info.shape
    n = 3 * K + 12
    vin, bin_ = _guarded(info, offset)
    vout, bout = _guarded(np.full((B, n), GUARD, np.uint8), offset)
    assert vin.data_ptr() % 16 == offset % 16 and vout.data_ptr() % 16 == offset % 16
    c.encode(vin, out=vout)
    torch.cuda.synchronize()
    bo, bi = bout.cpu().numpy(), bin_.cpu().numpy()
    assert (bo[:offset] == GUARD).all() and (bo[offset + B * n:] == GUARD).all(), "guard band round d_coded"
    assert (bi[:offset] == GUARD).all() and (bi[offset + B * K:] == GUARD).all(), "guard band round d_info"
    assert np.array_equal(bi[offset:offset + B * K].reshape(B, K), info), "d_info is only read"
    return bo[offset:offset + B * n].reshape(B, n)


def _batches(K):
    """(B, first pattern row): every pattern is in some batch; K = 6144 and 10000 keep to B = 5."""
    R = E.rows(K).shape[0]
    if K >= 6144:
        return [(5, s) for s in range(0, R, 5)]
    return [(1, 0), (3, 1), (5, 4), (65, 0), (257, 9)]


@pytest.mark.parametrize("K", E.SIZES)
def test_encode_equals_the_oracle(K):
    """B = 1, 3, 5, 65, 257: partial grids, and with odd K rows at every alignment modulo 16.  Bytes are 0
    or 1 and the guard bands stay."""
    with _codec(K) as c:
        for B, start in _batches(K):
            info, want = E.batch(K, B, start)
            got = _encode_guarded(c, info, 0)
            assert got.max() <= 1
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"K = {K}, B = {B}: first difference at (row, byte) {bad[0]}"


@pytest.mark.parametrize("K", [1, 7, 40, 65, 129, 4097, 6144])
def test_misaligned_base_gives_the_same_bytes(K):
    """A view one byte into a larger buffer, for the input and the output."""
    B = 5
    info, want = E.batch(K, B, 8)
    with _codec(K) as c:
        assert np.array_equal(_encode_guarded(c, info, 1), want)
        assert np.array_equal(_encode_guarded(c, info, 16 + 7), want)


def test_every_precision_gives_the_same_output():
    info, want = E.batch(40, 65)
    for precision in ("f64", "f32", "fixed"):
        with _codec(40, precision) as c:
            assert np.array_equal(_encode_guarded(c, info, 0), want), precision


def test_default_output_and_empty_batch():
    import torch
    info, want = E.batch(40, 3)
    with _codec(40) as c:
        out = c.encode(torch.from_numpy(info).to(_dev()))
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
        empty = c.encode(torch.empty((0, 40), dtype=torch.uint8, device=_dev()))
        assert tuple(empty.shape) == (0, 132)
        with pytest.raises(ValueError):
            c.encode(torch.from_numpy(info).to(_dev()).to(torch.int32))
        with pytest.raises(ValueError):
            c.encode(torch.from_numpy(info).to(_dev()), out=torch.empty((3, 131), dtype=torch.uint8, device=_dev()))


@pytest.mark.parametrize("K", [40, 6144])
def test_encode_equals_the_frame_generator(K):
    """td_synth_frames is bit-identical to the reference's frames.  At 60 dB its noise (a sum of 12
    uniforms: bounded) cannot flip a sample, so the hard decision of its LLRs is the reference's coded
    stream of its info bits -- and encode(info) must be that stream.  The sign a 1 demodulates to is read
    off demodulate(modulate(bits)), not assumed."""
    import torch
    from turbo_decoder_cuda_amd.decoder import demodulate, modulate
    B = 64
    with _codec(K) as c:
        c.synth_seed(12345)
        info, llr = c.synth(B, 60.0)
        coded = c.encode(info)
        probe = torch.tensor([0, 1], dtype=torch.uint8, device=_dev())
        si, sq = modulate(probe, 1)
        sign = demodulate(si, sq, 1, 1.0).cpu().numpy()
        torch.cuda.synchronize()
        assert sign[0] * sign[1] < 0
        hard = ((llr.cpu().numpy() * np.sign(sign[1])) > 0).astype(np.uint8)
        info_np = info.cpu().numpy()
        assert 0.3 < info_np.mean() < 0.7
        assert np.array_equal(coded.cpu().numpy(), hard)


def test_attach_and_encode_in_a_captured_graph():
    """td_crc_attach + td_encode_device captured on one stream (no parallel branches), replayed twice on
    changed inputs: the outputs equal the eager calls'."""
    import torch
    K, B = 1024, 33
    rng = np.random.default_rng(77)
    ins = [rng.integers(0, 2, (B, K), dtype=np.uint8) for _ in range(2)]
    with _codec(K) as c:
        c.set_crc(N.CRC24B)
        eager = []
        for x in ins:
            t = torch.from_numpy(x).to(_dev())
            c.crc_attach(t)
            eager.append((t.cpu().numpy().copy(), c.encode(t).cpu().numpy().copy()))
        gin = torch.zeros((B, K), dtype=torch.uint8, device=_dev())
        gout = torch.zeros((B, 3 * K + 12), dtype=torch.uint8, device=_dev())
        s = torch.cuda.Stream(_dev())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            c.crc_attach(gin, stream=s)
            c.encode(gin, out=gout, stream=s)
        for k in (1, 0):
            gin.copy_(torch.from_numpy(ins[k]).to(_dev()))
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(gin.cpu().numpy(), eager[k][0]) and np.array_equal(gout.cpu().numpy(), eager[k][1]), k


def test_bad_arguments_are_einval_and_change_nothing():
    import torch
    L = N.lib()
    K, B = 40, 3
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 2, (B, K), dtype=np.uint8)
    host = lambda r, poly: L.td_crc24_host(np.ascontiguousarray(r).ctypes.data_as(C.c_void_p), K, poly)

    def einval(rc):
        assert rc == N.TD_EINVAL and L.td_last_error() != b""

    with _codec(K) as c:
        h = c._h
        bits = torch.from_numpy(rows).to(_dev())
        coded = torch.empty((B, 3 * K + 12), dtype=torch.uint8, device=_dev())
        rem = torch.empty((B,), dtype=torch.int32, device=_dev())
        pb, pc, pr = (C.c_void_p(t.data_ptr()) for t in (bits, coded, rem))
        einval(L.td_encode_device(h, None, B, pc, None))
        einval(L.td_encode_device(h, pb, B, None, None))
        einval(L.td_encode_device(h, pb, -1, pc, None))
        einval(L.td_encode_device(None, pb, B, pc, None))
        einval(L.td_crc_attach(h, pb, B, None))            # before td_crc_set
        einval(L.td_crc_check(h, pb, B, pr, None))
        einval(L.td_crc_set(h, 0))
        einval(L.td_crc_set(h, 1 << 24))
        einval(L.td_crc_check(h, pb, B, pr, None))         # the failed sets set nothing
        c.set_crc(N.CRC24A)
        einval(L.td_crc_set(h, 0))
        einval(L.td_crc_set(h, 0x1800063))
        einval(L.td_crc_attach(h, None, B, None))
        einval(L.td_crc_attach(h, pb, -1, None))
        einval(L.td_crc_check(h, None, B, pr, None))
        einval(L.td_crc_check(h, pb, B, None, None))
        einval(L.td_crc_check(h, pb, -2, pr, None))
        got = c.crc_check(bits).cpu().numpy()              # gCRC24A is still the setting
        assert [int(v) for v in got] == [host(r, N.CRC24A) for r in rows]
        assert np.array_equal(bits.cpu().numpy(), rows), "no failed call wrote"
    from turbo_decoder_cuda_amd import TurboCodec
    with TurboCodec(24, 1, 0, iterations=2) as c:          # K = 24: no room for a CRC-24
        einval(L.td_crc_set(c._h, N.CRC24B))
        einval(L.td_crc_attach(c._h, pb, B, None))
