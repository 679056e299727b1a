"""Transport blocks without a GPU: the planners of the C ABI (td_tb_plan_host, td_tb_rm_sizes_host,
td_rm_index_host_filler) against tb_ref's restatement and the issue's spot values, csrc/td_tb_core.h -- the
index arithmetic the gfx950 kernels of td_tb.hip use -- as a stand-alone host program under ASan + UBSan, and
the argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ratematch_ref as RM
import tb_ref as T
from conftest import REPO
from turbo_decoder_cuda_amd import _native as N
from turbo_decoder_cuda_amd import transport

SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]

# A: (C, K_plus, K_minus, C_plus, C_minus, F)
SPOT = {1: (1, 40, 0, 1, 0, 15), 16: (1, 40, 0, 1, 0, 0), 17: (1, 48, 0, 1, 0, 7), 6120: (1, 6144, 0, 1, 0, 0),
        6121: (2, 3136, 3072, 1, 1, 15), 12217: (3, 4160, 4096, 1, 2, 39), 12257: (3, 4160, 4096, 2, 1, 63),
        12321: (3, 4160, 4096, 3, 0, 63), 40000: (7, 5760, 5696, 5, 2, 0), 75376: (13, 5824, 5760, 13, 0, 0)}


def lib_plan(A):
    s = N.TdTbPlan()
    assert N.lib().td_tb_plan_host(A, C.byref(s)) == N.TD_OK
    return T.Plan(*(getattr(s, f) for f in T.Plan._fields))


def test_plan_equals_the_restatement_for_every_size():
    for A in range(1, 100001):
        p = lib_plan(A)
        assert p == T.plan(A), A
        assert 0 <= p.F <= 63 and p.C_plus * p.K_plus + p.C_minus * p.K_minus == p.B + p.C * p.L + p.F, A
        assert p.C_plus >= 1 and p.C_plus + p.C_minus == p.C


def test_plan_spot_values_and_the_python_wrapper():
    for A, (Cn, Kp, Km, Cp, Cm, F) in SPOT.items():
        p = lib_plan(A)
        assert (p.C, p.K_plus, p.C_plus, p.C_minus, p.F) == (Cn, Kp, Cp, Cm, F), A
        if Cn > 1:   # K_minus is the size below K_plus whenever C > 1, also where no block has it (C_minus = 0)
            assert p.K_minus == Km, A
        else:
            assert p.K_minus == 0 and p.L == 0
        assert p.B == A + 24 and p.L == (24 if Cn > 1 else 0)
        assert transport.tb_plan(A) == tuple(p)
    for A in (1 << 20, (1 << 20) - 7):
        assert lib_plan(A) == T.plan(A)


def test_plan_rejects_bad_arguments():
    L = N.lib()
    s = N.TdTbPlan()
    for A in (0, -1, (1 << 20) + 1):
        assert L.td_tb_plan_host(A, C.byref(s)) == N.TD_EINVAL and b"td_tb_plan_host" in L.td_last_error()
    assert L.td_tb_plan_host(100, None) == N.TD_EINVAL


def lib_index(K, Ncb, F, rv, E):
    idx = np.full(E + 2, -7, dtype=np.int32)
    assert N.lib().td_rm_index_host_filler(K, Ncb, F, rv, E, C.c_void_p(idx.ctypes.data)) == N.TD_OK
    assert idx[E] == -7 and idx[E + 1] == -7
    return idx[:E]


@pytest.mark.parametrize("K", [40, 3072, 4160])
def test_index_without_filler_is_td_rm_index_host(K):
    Kpi, Kw = RM.layout(K)[2:4]
    for Ncb in (0, Kpi, Kw - 5):
        for rv in range(4):
            E = 2 * Kw + 3
            ref = np.empty(E, dtype=np.int32)
            assert N.lib().td_rm_index_host(K, Ncb, rv, E, C.c_void_p(ref.ctypes.data)) == N.TD_OK
            assert np.array_equal(lib_index(K, Ncb, 0, rv, E), ref)


@pytest.mark.parametrize("K,F", [(40, 7), (40, 15), (48, 7), (3072, 15), (4096, 63), (4160, 63)])
def test_index_with_filler_equals_the_restatement_and_never_selects_filler(K, F):
    Kpi, Kw = RM.layout(K)[2:4]
    for Ncb in (0, Kpi + (Kw - Kpi) // 2 + 1):   # the whole buffer, and one that ends inside the parity part
        w = RM.circular_buffer(K)[:Ncb or Kw]
        nnn = int(((w >= 0) & ~((w // 3 < F) & (w % 3 != 2))).sum())
        for rv in range(4):
            for E in (nnn // 3, nnn, 2 * nnn + 11):   # puncturing, exactly once round, repetition (wrap)
                got = lib_index(K, Ncb, F, rv, E)
                assert np.array_equal(got, T.index_filler(K, Ncb, F, rv, E)), (Ncb, rv, E)
                assert not ((got // 3 < F) & (got % 3 != 2)).any()
                assert got.min() >= 0 and got.max() < 3 * K + 12
                if E >= nnn:   # every other position of the buffer is sent
                    assert len(np.unique(got)) == nnn
    assert np.array_equal(transport.rate_match_index_filler(K, 0, F, 1, 99), T.index_filler(K, 0, F, 1, 99))


def test_index_rejects_bad_arguments():
    L = N.lib()
    idx = np.zeros(8, dtype=np.int32)
    p = C.c_void_p(idx.ctypes.data)
    for args in ((40, 0, -1, 0, 8), (40, 0, 64, 0, 8), (40, 0, 7, 4, 8), (40, 0, 7, -1, 8), (40, 0, 7, 0, 0),
                 (40, 63, 7, 0, 8), (0, 0, 0, 0, 8), (10001, 0, 0, 0, 8), (30, 0, 30, 0, 8)):
        assert L.td_rm_index_host_filler(*args, p) == N.TD_EINVAL, args
        assert b"td_rm_index_host_filler" in L.td_last_error()
    assert L.td_rm_index_host_filler(40, 0, 7, 0, 8, None) == N.TD_EINVAL


def lib_sizes(p, G, NlQm):
    s = N.TdTbPlan(*p)
    v = [C.c_int(-1) for _ in range(3)]
    rc = N.lib().td_tb_rm_sizes_host(C.byref(s), G, NlQm, *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def test_rm_sizes():
    p = T.plan(12257)   # C = 3
    assert lib_sizes(p, 3 * 4000 * 2, 2) == (N.TD_OK, (8000, 8000, 3))          # gamma = 0
    assert lib_sizes(p, (3 * 4000 + 1) * 2, 2) == (N.TD_OK, (8000, 8002, 2))    # gamma = 1
    assert lib_sizes(p, (3 * 4000 + 2) * 4, 4) == (N.TD_OK, (16000, 16004, 1))  # gamma = 2
    assert lib_sizes(p, 3, 1) == (N.TD_OK, (1, 1, 3))                           # G' = C
    assert lib_sizes(T.plan(100), 77, 1) == (N.TD_OK, (77, 77, 1))              # C = 1
    for A, G, Q in ((12257, 24002, 2), (6121, 12347, 1), (40000, 7 * 9000 + 6 * 6, 6), (75376, 13 * 12000 + 4 * 5, 4)):
        p = T.plan(A)
        rc, got = lib_sizes(p, G, Q)
        assert rc == N.TD_OK and got == T.rm_sizes(p.C, G, Q)
        assert got[2] * got[0] + (p.C - got[2]) * got[1] == G and sum(T.block_e(p, G, Q)) == G
        assert transport.rm_sizes(p, G, Q) == got
    L = N.lib()
    p = T.plan(12257)
    for G, Q in ((24001, 2), (2, 1), (0, 1), (-6, 2), (24000, 0), (24000, -2), (1 << 31, 1)):
        assert lib_sizes(p, G, Q)[0] == N.TD_EINVAL and b"td_tb_rm_sizes_host" in L.td_last_error(), (G, Q)
    assert L.td_tb_rm_sizes_host(None, 24000, 2, None, None, None) == N.TD_EINVAL
    s = N.TdTbPlan(*p)
    assert L.td_tb_rm_sizes_host(C.byref(s), 24000, 2, None, None, None) == N.TD_OK   # any output may be null


def test_exports_and_argument_checks_that_need_no_device():
    L = N.lib()
    for name in ("td_tb_plan_host", "td_tb_rm_sizes_host", "td_rm_index_host_filler", "td_tb_create", "td_tb_destroy",
                 "td_tb_get_plan", "td_tb_segment", "td_tb_rate_match", "td_tb_rate_dematch", "td_tb_concat"):
        assert name in N.EXPORTS and hasattr(L, name)
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    for call, who in ((lambda: L.td_tb_segment(None, p, 1, p, p, None), b"td_tb_segment"),
                      (lambda: L.td_tb_rate_match(None, p, p, 1, 0, 100, 1, p, None), b"td_tb_rate_match"),
                      (lambda: L.td_tb_rate_dematch(None, p, N.TD_F64, 1, 0, 100, 1, p, p, 0, None), b"td_tb_rate_dematch"),
                      (lambda: L.td_tb_concat(None, p, p, 1, p, None, None, None), b"td_tb_concat"),
                      (lambda: L.td_tb_get_plan(None, C.byref(N.TdTbPlan())), b"td_tb_get_plan"),
                      (lambda: L.td_tb_create(None, C.byref(N.TdTbParams(100, 0, 0, -64.0))), b"td_tb_create")):
        assert call() == N.TD_EINVAL and who in L.td_last_error()
    assert L.td_tb_destroy(None) == N.TD_OK
    h = C.c_void_p()
    for prm in ((0, 0, 0, -64.0), ((1 << 20) + 1, 0, 0, -64.0), (100, -1, 0, -64.0), (100, 127, 0, -64.0),   # Kpi(128) = 160
                (12257, 4191, 0, -64.0),                                                                       # Kpi(4160) = 4192
                (100, 0, 0, 1.0), (100, 0, 0, float("inf")), (100, 0, 0, float("-inf")), (100, 0, 0, float("nan"))):
        assert L.td_tb_create(C.byref(h), C.byref(N.TdTbParams(*prm))) == N.TD_EINVAL, prm
        assert not h.value and b"td_tb_create" in L.td_last_error()
    assert L.td_tb_create(C.byref(h), None) == N.TD_EINVAL


# ---- csrc/td_tb_core.h under ASan + UBSan ----

CORE_CASES = [(A, G, Q) for A, (G, Q) in zip(SPOT, ((120, 1), (39, 3), (146, 2), (18434, 2), (12348, 2), (24002 * 2, 4),
                                                    (25000 * 3 + 6, 6), (24000, 1), (7 * 17000 + 5 * 2, 2),
                                                    (13 * 17000 + 12 * 4, 4)))]


@pytest.fixture(scope="module")
def core_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("tb_core")
    exe, fin, fout = str(d / "tb_core_host"), str(d / "in.bin"), str(d / "out.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *SAN, f"-I{REPO}/turbo_decoder_cuda_amd/csrc",
                           os.path.join(REPO, "tests", "tb_core_host.cpp"), "-o", exe])
    with open(fin, "wb") as f:
        f.write(np.array([len(CORE_CASES)] + [v for c in CORE_CASES for v in c], dtype=np.int32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return np.fromfile(fout, dtype=np.int32)


def core_expected(A, G, Q):
    """The program's words for one case, from tb_ref: the blocks are built forwards there and inverted here."""
    p = T.plan(A)
    words = [np.array(p)]
    lab = T.labels(p)
    where = np.full((p.B, 2), -1, dtype=np.int64)   # bit s of the B-bit sequence -> (r, i)
    at = -p.F
    for r, (kind, idx) in enumerate(lab):
        K = len(kind)
        row = (r if r < p.C_minus else r - p.C_minus) * 5 + 2
        words += [np.array([K, at, row]), np.stack([kind, idx], axis=1).ravel()]
        at += K - p.L
        for k, off in ((T.TB, 0), (T.TBCRC, p.A)):
            i = np.flatnonzero(kind == k)
            where[idx[i] + off] = np.stack([np.full(len(i), r), i], axis=1)
    assert (where >= 0).all()
    words.append(where.ravel())
    E = T.block_e(p, G, Q)
    words.append(np.array(T.rm_sizes(p.C, G, Q)))
    starts = np.concatenate([[0], np.cumsum(E)[:-1]])
    words.append(np.stack([starts, E], axis=1).ravel())
    words.append(np.stack([np.repeat(np.arange(p.C), E), np.concatenate([np.arange(e) for e in E])], axis=1).ravel())
    return np.concatenate(words).astype(np.int32)


def test_core_index_arithmetic_equals_the_restatement_byte_for_byte(core_out):
    want = np.concatenate([core_expected(*c) for c in CORE_CASES])
    assert core_out.size == want.size
    bad = np.flatnonzero(core_out != want)
    assert bad.size == 0, f"first difference at word {bad[0]}: {core_out[bad[0]]} != {want[bad[0]]}"
    assert core_out.tobytes() == want.tobytes()
