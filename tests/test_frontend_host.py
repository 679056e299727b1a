"""The receive front end without a GPU: csrc/td_demap_core.h -- the demappers, the LLR conversion and the
value source the fused gfx950 kernels read -- as a stand-alone host program under ASan + UBSan, against the
reference's recorded LLRs, pyoracle.demodulate and the numpy restatement (tests/frontend_ref.py); and the
ABI's argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frontend_ref as FR
import pyoracle as O
from conftest import GOLD, REPO
from turbo_decoder_cuda_amd import _native as N

SAN = ["-fsanitize=address", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
PREC = {"f64": 0, "f32": 1, "fixed": 2}


@pytest.fixture(scope="module")
def core_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frontend_core") / "frontend_core_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN,
                           f"-I{REPO}/turbo_decoder_cuda_amd/csrc", os.path.join(REPO, "tests", "frontend_core_host.cpp"),
                           "-o", exe])
    return exe


def _run(exe, tmp_path, ints, *blobs):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(ints, dtype=np.int32).tobytes())
        for b in blobs:
            f.write(np.ascontiguousarray(b).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return np.fromfile(fout, dtype=np.uint8)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("M", FR.MODS)
def test_core_demappers_equal_the_reference_and_the_oracle(core_host, tmp_path, M):
    """demod_symbol<M> (BPSK: demod_bpsk) on the recorded symbols: the reference's doubles, bit for bit; the
    program itself fails if demod_bit<M> gives another double for any bit."""
    d = np.load(os.path.join(GOLD, "demod.npz"))
    yi, yq, Kf = d[f"yi_{M}"], d[f"yq_{M}"], float(d["Kf"])
    got = _run(core_host, tmp_path, [0, M, yi.size], np.float64(Kf), yi, yq).view(np.float64)
    assert _same_bits(got, d[f"llr_{M}"])
    assert _same_bits(got, O.demodulate(yi, yq, M, Kf))
    yi, yq = FR.symbols(1001, 10 + M)   # noisy symbols, off the constellation points
    got = _run(core_host, tmp_path, [0, M, yi.size], np.float64(FR.KF), yi, yq).view(np.float64)
    assert _same_bits(got, O.demodulate(yi, yq, M, FR.KF))


@pytest.mark.parametrize("s", [8.0, 40.0, 0.3])
def test_core_conversion_equals_numpy(core_host, tmp_path, s):
    """Ties to even, the clamp before the integer conversion (+-1e300 and +-inf are +-127, never -128), the
    float narrowing with its overflow to +-inf, +-0 and a subnormal."""
    x = np.concatenate([FR.tie_vector(8.0), np.random.default_rng(3).normal(0, 9, 500)])
    raw = _run(core_host, tmp_path, [1, x.size, 0], np.float64(s), x)
    n = x.size
    assert _same_bits(raw[:8 * n].view(np.float64), x)
    assert _same_bits(raw[8 * n:12 * n].view(np.float32), FR.convert(x, "f32"))
    q = raw[12 * n:].view(np.int8)
    assert np.array_equal(q, FR.convert(x, "fixed", s)) and q.min() >= -127
    if s == 8.0:   # the ties really are ties, and they went to the even neighbour
        t = x[:12] * s
        assert np.array_equal(t - np.floor(t), np.full(12, 0.5)) and not (q[:10].astype(int) % 2).any()
        assert q[np.isinf(x)].tolist() == [127, -127] and q[np.abs(x) == 1e300].tolist() == [127, -127]


@pytest.mark.parametrize("precision", ["f64", "f32", "fixed"])
@pytest.mark.parametrize("M", [2, 6])
def test_core_definition_equals_the_restatement(core_host, tmp_path, M, precision):
    """The whole definition at K = 40 -- the kernels' own value source, summed at td_rm_index_host's positions
    in ascending k -- with and without a prior buffer (int8: a -128 in it)."""
    K, B, n = 40, 3, 132
    dt = FR.NP_DT[precision]
    for t, (Ncb, rv, E) in enumerate(FR.cases(K, M)):
        s = 40.0 if t == 1 else 8.0
        yi, yq = FR.symbols((B, E // M), 100 * M + t)
        idx = np.empty(E, dtype=np.int32)
        assert N.lib().td_rm_index_host(K, Ncb, rv, E, idx.ctypes.data_as(C.c_void_p)) == N.TD_OK
        rng = np.random.default_rng(t)
        prior = rng.integers(-128, 128, (B, n)).astype(np.int8) if precision == "fixed" else (rng.normal(0, 4, (B, n)) * 1.2345678).astype(dt)
        if precision == "fixed":
            prior[0, :8] = -128
        for acc in (0, 1):
            got = _run(core_host, tmp_path, [2, M, PREC[precision], B, E, n, acc], np.array([FR.KF, s]), idx, yi, yq, prior)
            want = FR.restate(yi, yq, M, precision, K, Ncb, rv, prior=prior if acc else None, steps_per_unit=s)
            assert _same_bits(got.view(dt).reshape(B, n), want), (Ncb, rv, E, acc)


def test_exports_and_argument_checks_without_a_device():
    L = N.lib()
    for name in ("td_llr_convert", "td_demod_dematch"):
        assert name in N.EXPORTS and hasattr(L, name)
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.td_demod_dematch(None, p, p, 1, 0, 2, 2, 1.0, 8.0, p, 0, None) == N.TD_EINVAL
    assert b"td_demod_dematch" in L.td_last_error()
    for call in (lambda: L.td_llr_convert(None, 4, N.TD_F32, 8.0, p, None),
                 lambda: L.td_llr_convert(p, 4, N.TD_F32, 8.0, None, None),
                 lambda: L.td_llr_convert(p, -1, N.TD_F32, 8.0, p, None),
                 lambda: L.td_llr_convert(p, 4, 3, 8.0, p, None),
                 lambda: L.td_llr_convert(p, 4, -1, 8.0, p, None),
                 lambda: L.td_llr_convert(p, 4, N.TD_FIXED, 0.0, p, None),
                 lambda: L.td_llr_convert(p, 4, N.TD_FIXED, -8.0, p, None),
                 lambda: L.td_llr_convert(p, 4, N.TD_FIXED, float("inf"), p, None),
                 lambda: L.td_llr_convert(p, 4, N.TD_FIXED, float("nan"), p, None)):
        assert call() == N.TD_EINVAL and b"td_llr_convert" in L.td_last_error()
    assert L.td_llr_convert(p, 0, N.TD_FIXED, 8.0, p, None) == N.TD_OK   # n = 0: a no-op, no device needed
