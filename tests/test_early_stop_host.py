"""Early termination, the host side (no GPU): the CRC-24 behind TD_STOP_CRC.  td_crc24_host is the
LTE code-block CRC (row of K bits, first bit first, zero initial state, no final XOR), and
td_crc24_syndromes is the per-position table the kernel's fold lanes XOR -- the remainder of a row
is the XOR of the entries of its set bits.  csrc/td_crc.h also runs under ASan + UBSan as a
stand-alone program (tests/early_stop_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

from turbo_decoder_cuda_amd import _native as N

CSRC = os.path.join(REPO, "turbo_decoder_cuda_amd", "csrc")
POLYS = [0x800063, 0x864CFB]   # gCRC24B, gCRC24A
SIZES = [25, 40, 1024, 6144]


def crc24_serial(bits, poly):
    """Bit-serial long division by x^24 + poly of bits(x) * x^24."""
    reg = 0
    for b in bits:
        top = ((reg >> 23) & 1) ^ int(b)
        reg = (reg << 1) & 0xFFFFFF
        if top:
            reg ^= poly
    return reg


def host_crc(bits, poly):
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    return int(N.lib().td_crc24_host(bits.ctypes.data_as(C.c_void_p), bits.size, poly))


def syndromes(K, poly):
    tab = np.zeros(K, dtype=np.uint32)
    assert N.lib().td_crc24_syndromes(K, poly, tab.ctypes.data_as(C.c_void_p)) == 0
    return tab


def with_crc(payload, poly):
    c = crc24_serial(payload, poly)
    return np.concatenate([payload, [(c >> (23 - j)) & 1 for j in range(24)]]).astype(np.uint8)


@pytest.mark.parametrize("poly", POLYS)
@pytest.mark.parametrize("K", SIZES)
def test_crc24_host_equals_bit_serial(K, poly):
    rng = np.random.default_rng(100 + K)
    for _ in range(3):
        row = rng.integers(0, 2, K).astype(np.uint8)
        assert host_crc(row, poly) == crc24_serial(row, poly)


@pytest.mark.parametrize("poly", POLYS)
@pytest.mark.parametrize("K", SIZES)
def test_row_with_its_crc_appended_has_zero_remainder(K, poly):
    rng = np.random.default_rng(200 + K)
    row = with_crc(rng.integers(0, 2, K - 24).astype(np.uint8), poly)
    assert row.size == K and host_crc(row, poly) == 0


@pytest.mark.parametrize("poly", POLYS)
@pytest.mark.parametrize("K", SIZES)
def test_syndrome_xor_equals_crc(K, poly):
    tab = syndromes(K, poly)
    assert tab.max() < (1 << 24)
    rng = np.random.default_rng(300 + K)
    for _ in range(3):
        row = rng.integers(0, 2, K).astype(np.uint8)
        assert int(np.bitwise_xor.reduce(tab[row == 1], initial=0)) == host_crc(row, poly)
    assert int(np.bitwise_xor.reduce(tab)) == host_crc(np.ones(K, dtype=np.uint8), poly)


@pytest.mark.parametrize("poly", POLYS)
def test_single_bit_flip_of_a_valid_row_is_detected(poly):
    K = 40
    row = with_crc(np.random.default_rng(5).integers(0, 2, K - 24).astype(np.uint8), poly)
    assert host_crc(row, poly) == 0
    for i in range(K):
        bad = row.copy()
        bad[i] ^= 1
        assert host_crc(bad, poly) != 0, i


def test_syndromes_rejects_bad_arguments():
    assert N.lib().td_crc24_syndromes(0, 0x800063, None) == N.TD_EINVAL
    assert N.lib().td_crc24_syndromes(40, 0x800063, None) == N.TD_EINVAL


def test_crc_header_under_asan_ubsan(tmp_path):
    """csrc/td_crc.h compiles with plain g++ (no HIP) and runs clean under ASan + UBSan as its own
    program, K = 25, 40 and 10000."""
    exe = str(tmp_path / "early_stop_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                           os.path.join(REPO, "tests", "early_stop_sanitize.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
