"""Scrambling without a GPU: td_gold_sequence_host against gold_ref's restatement of 36.211 7.2 and the issue's
spot values, the sequence's linearity, csrc/td_gold_core.h -- the step and the jump the gfx950 kernels of
td_scramble.hip use -- as a stand-alone host program under ASan + UBSan, and the argument checks that need no
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gold_ref as G
from conftest import REPO
from turbo_decoder_cuda_amd import _native as N

SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
GUARD = 0xA5A5A5A5
CINITS = [0, 1, 0x7FFFFFFF] + [int(v) for v in np.random.default_rng(31).integers(0, 1 << 31, 3)]


def lib_words(cinit, length):
    W = (length + 31) // 32
    seq = np.full(W + 2, GUARD, dtype=np.uint32)
    assert N.lib().td_gold_sequence_host(cinit, length, C.c_void_p(seq.ctypes.data)) == N.TD_OK
    assert seq[W] == GUARD and seq[W + 1] == GUARD, "the two words after the output"
    return seq[:W]


@pytest.fixture(scope="module")
def ref_top():
    """the restatement at the longest length, once: every shorter sequence is a prefix of it"""
    return G.bits(CINITS, (1 << 22) + 5)


def test_spot_values_of_the_restatement_and_the_library():
    b = G.bits(list(G.SPOT), 6250 * 32)
    w = G.pack(b)
    for row, (cinit, spots) in enumerate(G.SPOT.items()):
        got = lib_words(cinit, 6250 * 32)
        for at, value in spots.items():
            assert int(w[row, at]) == value, (hex(cinit), at)
            assert int(got[at]) == value, (hex(cinit), at)
        assert np.array_equal(got, w[row])


@pytest.mark.parametrize("length", G.edge_lengths())
def test_host_sequence_equals_the_restatement(length, ref_top):
    want = G.pack(ref_top[:, :length])
    for row, cinit in enumerate(CINITS):
        got = lib_words(cinit, length)
        assert np.array_equal(got, want[row]), (hex(cinit), length)
        if length % 32:
            assert int(got[-1]) >> (length % 32) == 0, "tail bits"
        assert np.array_equal(lib_words(cinit | 0x80000000, length), got), "bit 31 of c_init"


def test_linearity():
    """c(a ^ b) ^ c(0) = (c(a) ^ c(0)) ^ (c(b) ^ c(0)): x1 does not depend on c_init and x2 is linear in it"""
    length = 3 * G.RUN + 17
    zero = lib_words(0, length)
    rng = np.random.default_rng(5)
    for a, b in rng.integers(0, 1 << 31, (8, 2)):
        a, b = int(a), int(b)
        assert np.array_equal(lib_words(a ^ b, length) ^ zero, (lib_words(a, length) ^ zero) ^ (lib_words(b, length) ^ zero))
    assert not np.array_equal(lib_words(1, length), zero)


def test_exports_and_argument_checks_that_need_no_device():
    L = N.lib()
    for name in ("td_gold_sequence", "td_gold_sequence_host", "td_scramble", "td_descramble_llr", "td_tb_demod_dematch"):
        assert name in N.EXPORTS and hasattr(L, name)
    buf = (C.c_uint32 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.td_gold_sequence_host(1, 64, None) == N.TD_EINVAL and b"td_gold_sequence_host" in L.td_last_error()
    for length in (-1, 1 << 31, 1 << 40):
        assert L.td_gold_sequence_host(1, length, p) == N.TD_EINVAL, length
    assert L.td_gold_sequence_host(1, 0, p) == N.TD_OK and not any(buf)
    for call, who in ((lambda: L.td_gold_sequence(None, 1, 64, p, None), b"td_gold_sequence"),
                      (lambda: L.td_gold_sequence(p, 1, 64, None, None), b"td_gold_sequence"),
                      (lambda: L.td_gold_sequence(p, -1, 64, p, None), b"td_gold_sequence"),
                      (lambda: L.td_gold_sequence(p, 1, -1, p, None), b"td_gold_sequence"),
                      (lambda: L.td_gold_sequence(p, 1, 1 << 31, p, None), b"td_gold_sequence"),
                      (lambda: L.td_scramble(None, p, 1, 64, p, None), b"td_scramble"),
                      (lambda: L.td_scramble(p, None, 1, 64, p, None), b"td_scramble"),
                      (lambda: L.td_scramble(p, p, 1, 64, None, None), b"td_scramble"),
                      (lambda: L.td_scramble(p, p, -1, 64, p, None), b"td_scramble"),
                      (lambda: L.td_scramble(p, p, 1, -64, p, None), b"td_scramble"),
                      (lambda: L.td_descramble_llr(None, N.TD_F64, p, 1, 8, p, None), b"td_descramble_llr"),
                      (lambda: L.td_descramble_llr(p, N.TD_F64, None, 1, 8, p, None), b"td_descramble_llr"),
                      (lambda: L.td_descramble_llr(p, N.TD_F64, p, 1, 8, None, None), b"td_descramble_llr"),
                      (lambda: L.td_descramble_llr(p, 7, p, 1, 8, p, None), b"td_descramble_llr"),
                      (lambda: L.td_descramble_llr(p, N.TD_F32, p, -1, 8, p, None), b"td_descramble_llr"),
                      (lambda: L.td_descramble_llr(p, N.TD_FIXED, p, 1, 1 << 31, p, None), b"td_descramble_llr"),
                      (lambda: L.td_tb_demod_dematch(None, p, p, N.TD_F64, 1, 0, 120, 2, 2, 1.0, 8.0, None, p, p, 0, None),
                       b"td_tb_demod_dematch")):
        assert call() == N.TD_EINVAL and who in L.td_last_error()
    # N = 0 and len = 0 launch nothing
    assert L.td_gold_sequence(p, 0, 64, p, None) == N.TD_OK and L.td_gold_sequence(p, 3, 0, p, None) == N.TD_OK
    assert L.td_scramble(p, p, 0, 64, p, None) == N.TD_OK and L.td_descramble_llr(p, N.TD_F32, p, 2, 0, p, None) == N.TD_OK


# ---- csrc/td_gold_core.h under ASan + UBSan ----

CORE_CASES = [(c, n) for n in G.edge_lengths() for c in (CINITS[3], 0x7FFFFFFF)] + [(0, 151424), (0x80000001, 100)]
WALK_CINIT = 0x12345678


@pytest.fixture(scope="module")
def core_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("gold_core")
    exe, fin, fout = str(d / "gold_core_host"), str(d / "in.bin"), str(d / "out.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *SAN, f"-I{REPO}/turbo_decoder_cuda_amd/csrc",
                           os.path.join(REPO, "tests", "gold_core_host.cpp"), "-o", exe])
    with open(fin, "wb") as f:
        f.write(np.array([WALK_CINIT, len(CORE_CASES)] + [v for c in CORE_CASES for v in c], dtype=np.uint32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return np.fromfile(fout, dtype=np.uint32)


def test_core_jump_equals_the_stepped_registers_at_every_level(core_out):
    """2^31 bits stepped word by word; the jump compared at t = 0, 2^j (j <= 20) and 2^j - 1 (j <= 21): 42 offsets"""
    compared, differed = int(core_out[0]), int(core_out[1])
    assert compared == 42 and differed == 0
    assert int(core_out[3]) == 0, "the 32-position step against 4096 single steps, and T^1600 against 1600 of them"


def test_core_words_equal_the_restatement(core_out, ref_top):
    at = 4
    for cinit, length in CORE_CASES:
        W = (length + 31) // 32
        got, guard, same = core_out[at:at + W], core_out[at + W:at + W + 2], int(core_out[at + W + 2])
        at += W + 3
        want = G.pack(ref_top[CINITS.index(cinit)][None, :length]) if cinit in CINITS else G.words([cinit], length)
        assert np.array_equal(got, want[0]), (hex(cinit), length)
        assert (guard == GUARD).all() and same == 1, (hex(cinit), length)
    assert at == core_out.size
