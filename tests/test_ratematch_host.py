"""LTE rate matching on a host without a GPU: td_rm_index_host (the selection the device kernels
follow) against the numpy restatement of 36.212 5.1.4.1 (tests/ratematch_ref.py) and against known
answers, its argument errors, and the compat layer's rate_match / de_rate_match (ITTC/main.h:23-24)."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import ratematch_ref as RM
from conftest import REPO

from turbo_decoder_cuda_amd import _native as N
from turbo_decoder_cuda_amd import rate_match_index

PKG = os.path.join(REPO, "turbo_decoder_cuda_amd")
COMPAT = os.path.join(PKG, "libturbo_logmap_compat.so")


def ncb_values(K):
    _, _, Kpi, Kw, _ = RM.layout(K)
    return [0, Kpi, Kpi + 1, (Kpi + (Kw - Kpi) // 2) | 1, Kw - 1]


@pytest.mark.parametrize("K", [1, 13, 28, 29, 40, 1024, 6144, 10000])
def test_index_equals_restatement(K):
    """K = 28: ND = 0 (no <NULL>s); K = 29: ND = 31, R = 2; every Ncb edge, every rv, E through
    puncturing, the exact buffer, and repetition."""
    D, R, Kpi, Kw, ND = RM.layout(K)
    if K == 28:
        assert ND == 0
    if K == 29:
        assert (ND, R) == (31, 2)
    for Ncb in ncb_values(K):
        nnn = RM.n_nonnull(K, Ncb)
        for rv in range(4):
            for E in (1, nnn - 1, nnn, nnn + 1, 2 * nnn + 5):
                got = rate_match_index(K, Ncb, rv, E)
                assert got.dtype == np.int32 and got.shape == (E,)
                assert np.array_equal(got, RM.index(K, Ncb, rv, E)), (K, Ncb, rv, E)


KNOWN = [   # K, Ncb, rv, k0, first 8 stream positions
    (40, 192, 0, 4, [60, 12, 108, 48, 0, 96, 72, 24]),
    (40, 192, 1, 52, [69, 21, 117, 57, 9, 105, 81, 33]),
    (40, 192, 2, 100, [91, 95, 67, 71, 19, 23, 115, 119]),
    (40, 192, 3, 148, [4, 8, 100, 104, 76, 80, 28, 32]),
    (40, 128, 2, 68, [85, 89, 61, 65, 13, 17, 109, 113]),
    (13, 0, 0, None, [27, 15, 39, 9, 33, 21, 45, 6]),
    (6144, 0, 0, 386, [36, 132, 228, 324, 420, 516, 612, 708]),
    (6144, 0, 2, 9650, [67, 71, 163, 167, 259, 263, 355, 359]),
    (6144, 0, 1, 5018, None),
    (6144, 0, 3, 14282, None),
]


@pytest.mark.parametrize("K,Ncb,rv,k0,first", KNOWN)
def test_known_answers(K, Ncb, rv, k0, first):
    if k0 is not None:
        assert RM.k0(K, Ncb, rv) == k0
    if first is not None:
        assert rate_match_index(K, Ncb, rv, 8).tolist() == first
        assert RM.index(K, Ncb, rv, 8).tolist() == first


def test_known_layouts():
    assert RM.layout(40)[1:] == (2, 64, 192, 20)
    assert RM.layout(13)[1:] == (1, 32, 96, 15)
    assert RM.layout(6144)[1:] == (193, 6176, 18528, 28)
    assert RM.n_nonnull(40, 128) == 88


@pytest.mark.parametrize("K,rv,crc", [(1024, 0, 2492200822), (6144, 0, 3589039777), (6144, 1, 2107736247),
                                      (6144, 2, 3179259893), (6144, 3, 3058932438)])
def test_known_crc32_of_whole_index(K, rv, crc):
    idx = rate_match_index(K, 0, rv, 3 * K + 12)
    assert zlib.crc32(idx.astype("<i4").tobytes()) == crc


@pytest.mark.parametrize("K", [1, 13, 28, 29, 40, 1024, 6144])
def test_full_buffer_is_a_permutation(K):
    n = 3 * K + 12
    for rv in range(4):
        assert np.array_equal(np.sort(rate_match_index(K, 0, rv, n)), np.arange(n))


def test_argument_errors():
    L = N.lib()
    idx = np.zeros(64, dtype=np.int32)
    p = idx.ctypes.data
    bad = [(40, 0, 0, 8, None), (40, 0, -1, 8, p), (40, 0, 4, 8, p), (40, 0, 0, 0, p), (40, 0, 0, -3, p),
           (0, 0, 0, 8, p), (10001, 0, 0, 8, p), (40, 63, 0, 8, p), (40, 193, 0, 8, p), (40, -1, 0, 8, p)]
    for K, Ncb, rv, E, ptr in bad:
        assert L.td_rm_index_host(K, Ncb, rv, E, ptr) == N.TD_EINVAL, (K, Ncb, rv, E)
        assert L.td_last_error().startswith(b"td_rm_index_host")
    assert L.td_rm_index_host(40, 64, 3, 8, p) == N.TD_OK and L.td_rm_index_host(40, 192, 0, 8, p) == N.TD_OK
    # the handle's entry points refuse a null handle (before any GPU work)
    for call, name in ((lambda: L.td_rm_set(None, 0), b"td_rm_set"),
                       (lambda: L.td_rm_info(None, None, None, None, None, None), b"td_rm_info"),
                       (lambda: L.td_rate_match(None, None, 1, 1, 0, 8, None, None), b"td_rate_match"),
                       (lambda: L.td_rate_dematch(None, None, 1, 0, 8, None, 0, None), b"td_rate_dematch")):
        assert call() == N.TD_EINVAL
        assert L.td_last_error().startswith(name)
    assert L.td_abi_version() == 1
    for args in ((40, 0, 4, 8), (40, 0, 0, 0), (40, 63, 0, 8)):
        with pytest.raises(N.TurboError):
            rate_match_index(*args)


# ---------------------------------------------------------------- compat layer (ITTC/main.h:23-24)
def compat_symbols():
    """The two functions' exported (mangled) names, found by their demangled signatures."""
    raw = subprocess.run(["nm", "-D", "-p", "--defined-only", COMPAT], check=True, capture_output=True, text=True).stdout
    dem = subprocess.run(["nm", "-D", "-p", "--defined-only", "-C", COMPAT], check=True, capture_output=True, text=True).stdout
    names = {}
    for r, d in zip(raw.splitlines(), dem.splitlines()):
        m = re.search(r"\b(rate_match|de_rate_match)\((.*)\)$", d)
        if m:
            names[m.group(1)] = (r.split()[-1], m.group(2).replace(" ", ""))
    return names


def test_compat_exports_rate_matching():
    names = compat_symbols()
    assert names["rate_match"][1] == "int*,int,int*,int"
    assert names["de_rate_match"][1] == "double*,double*,int,int"


@pytest.mark.parametrize("E", [50, 132, 200])
def test_compat_rate_matching_matches_restatement(tmp_path, E):
    """The caller's two lines (main.cpp:196,204) link against the compat layer and give the restatement's
    selection at rv 0 over the whole buffer; de_rate_match(rate_match(x)) is x on the selected positions
    (times the number of times each was sent) and zero elsewhere."""
    K, n = 40, 132
    drv = str(tmp_path / "ratematch_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", drv, os.path.join(REPO, "tests", "ratematch_driver.cpp"),
                           f"-L{PKG}", "-lturbo_logmap_compat", "-lturbo_mi355x", f"-Wl,-rpath,{PKG}"])
    und = subprocess.run(["nm", "--undefined-only", drv], check=True, capture_output=True, text=True).stdout
    for sym, _ in compat_symbols().values():
        assert re.search(rf"\b{re.escape(sym)}\b", und), sym
    x = np.random.default_rng(E).integers(1, 1000, n).astype(np.int32)   # non-zero, so a zero means "not sent"
    x.tofile(tmp_path / "in.bin")
    subprocess.check_call([drv, str(K), str(E), str(tmp_path / "in.bin"), str(tmp_path / "e.bin"),
                           str(tmp_path / "back.bin")], timeout=60)
    e = np.fromfile(tmp_path / "e.bin", dtype=np.int32)
    back = np.fromfile(tmp_path / "back.bin", dtype=np.float64)
    idx = RM.index(K, 0, 0, E)
    assert np.array_equal(e, x[idx])
    assert np.array_equal(back, RM.dematch(e[None].astype(np.float64), K, 0, 0)[0])
    sent = np.bincount(idx, minlength=n)
    assert np.array_equal(back, x * sent)
    if E <= n:
        assert np.array_equal(back[idx], x[idx]) and not back[sent == 0].any()
