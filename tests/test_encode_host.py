"""The batched encoder and the CRC-24 attach / check without a GPU: csrc/td_encode_core.h -- the word-level
routines the gfx950 kernels of td_encode.hip call -- as a stand-alone host program under ASan + UBSan,
against pyoracle.encode, synth.turbo_encode and td_crc24_host; and the ABI's argument checks that need no
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import encode_cases as E
import pyoracle as O
from conftest import REPO
from turbo_decoder_cuda_amd import _native as N
from turbo_decoder_cuda_amd import synth

SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def core_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("encode_core") / "encode_core_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *SAN, f"-I{REPO}/turbo_decoder_cuda_amd/csrc",
                           os.path.join(REPO, "tests", "encode_core_host.cpp"), "-o", exe])
    return exe


def _run(exe, tmp_path, header, *blobs):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(header, dtype=np.int32).tobytes())
        for b in blobs:
            f.write(np.ascontiguousarray(b).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return np.fromfile(fout, dtype=np.uint8)


@pytest.mark.parametrize("K", E.SIZES)
def test_core_encoder_equals_the_oracle_and_the_numpy_encoder(core_host, tmp_path, K):
    """Every pattern row at every size, byte for byte; the rows leave for addresses 0 and 5 bytes past a
    16-byte boundary (odd K then walks every alignment), and ASan and the guard bytes watch both ends."""
    f1, f2 = E.interleaver(K)
    info, want = E.rows(K), E.coded(K)
    assert np.array_equal(want, synth.turbo_encode((info != 0).astype(np.uint8), f1, f2)), "the two references agree"
    for mis in (0, 5):
        got = _run(core_host, tmp_path, [0, K, info.shape[0], mis], O.qpp(K, f1, f2).astype(np.int32), info)
        got = got.reshape(info.shape[0], 3 * K + 12)
        assert got.max() <= 1
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"K = {K}, misalign {mis}: first difference at (row, byte) {bad[0]}"


@pytest.mark.parametrize("poly", [N.CRC24A, N.CRC24B])
@pytest.mark.parametrize("K", [25, 40, 64, 65, 6144])
def test_core_crc_attach_and_check(core_host, tmp_path, K, poly):
    B = 9
    rng = np.random.default_rng(K + poly)
    rows = rng.integers(0, 2, (B, K), dtype=np.uint8)
    rows[1] *= 0xFF   # any non-zero byte is a 1
    rows[2, K - 24:] = 0xA5   # garbage where the CRC goes
    raw = _run(core_host, tmp_path, [1, K, B, poly], rows)
    before = raw[:4 * B].view(np.uint32)
    att = raw[4 * B:4 * B + B * K].reshape(B, K)
    after = raw[4 * B + B * K:].view(np.uint32)
    L = N.lib()
    host = lambda r: L.td_crc24_host(np.ascontiguousarray(r).ctypes.data_as(C.c_void_p), K, poly)
    assert [int(v) for v in before] == [host(r) for r in rows]
    assert not after.any() and all(host(r) == 0 for r in att)
    assert np.array_equal(att[:, :K - 24], rows[:, :K - 24]) and att[:, K - 24:].max() <= 1
    for b in range(B):   # the attached bits are the payload's CRC, most significant bit first
        crc = L.td_crc24_host(np.ascontiguousarray(rows[b, :K - 24]).ctypes.data_as(C.c_void_p), K - 24, poly)
        assert [int(v) for v in att[b, K - 24:]] == [(crc >> (23 - j)) & 1 for j in range(24)]


def test_exports_and_null_handle_are_einval():
    L = N.lib()
    for name in ("td_encode_device", "td_crc_set", "td_crc_attach", "td_crc_check"):
        assert name in N.EXPORTS and hasattr(L, name)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    for call, who in ((lambda: L.td_encode_device(None, p, 1, p, None), b"td_encode_device"),
                      (lambda: L.td_crc_set(None, N.CRC24B), b"td_crc_set"),
                      (lambda: L.td_crc_attach(None, p, 1, None), b"td_crc_attach"),
                      (lambda: L.td_crc_check(None, p, 1, p, None), b"td_crc_check")):
        assert call() == N.TD_EINVAL and who in L.td_last_error()
