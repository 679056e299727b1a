"""The fixed-point decoder (TD_FIXED) without a GPU: the ABI's argument checks, and the numpy
restatement of its arithmetic (tests/fixed_ref.py) against the fp64 Max-Log-MAP oracle."""
import ctypes as C

import numpy as np
import pytest

import fixed_ref as F
import fixed_size_cases as Z
import pyoracle as O
from fixed_host import core_host, run_core   # noqa: F401  (core_host is a fixture)
from turbo_decoder_cuda_amd import _native as N

CODES = [(8, 3, 4), (40, 3, 10), (1024, 31, 64), (6144, 263, 480)]


def test_fixed_precision_constant():
    assert N.TD_FIXED == 2
    assert "td_set_fixed" in N.EXPORTS and hasattr(N.lib(), "td_set_fixed")
    assert N.lib().td_abi_version() == 1


def test_set_fixed_null_handle_is_einval():
    f = N.TdFixedParams(255, 3)
    assert N.lib().td_set_fixed(None, C.byref(f)) == N.TD_EINVAL
    assert b"td_set_fixed" in N.lib().td_last_error()


@pytest.mark.parametrize("K,algo", [(1024, N.TD_ALGO_LOGMAP), (7, N.TD_ALGO_MAXLOG)])
def test_create_fixed_rejects_logmap_and_short_blocks(K, algo):
    h = C.c_void_p()
    p = N.TdParams(K, 31 if K == 1024 else 1, 64 if K == 1024 else 0, 4, algo, N.TD_FIXED, 0)
    assert N.lib().td_create(C.byref(h), C.byref(p)) == N.TD_EINVAL
    assert b"TD_FIXED" in N.lib().td_last_error() and not h.value


def test_fixed_codec_without_gpu_fails_loudly():
    from turbo_decoder_cuda_amd import TurboCodec, device_count
    if device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(N.TurboError) as e:
        TurboCodec(1024, 31, 64, iterations=4, algo="maxlog", precision="fixed")
    assert e.value.code == N.TD_ENODEV


@pytest.mark.parametrize("K,f1,f2", CODES)
def test_reference_equals_float_maxlog_oracle(K, f1, f2):
    """With ext_scale_q = 4 and nothing clamped the integer decoder is the fp64 Max-Log-MAP oracle on
    the same integers: max-log on integers rounds nowhere and Lambda is even."""
    B, iters = 2, 4
    _, flow = O.synth_batch(K, f1, f2, 0.5, 5, B)
    q = F.quantise(flow, 4)
    rows, le, share = F.decode(q, K, f1, f2, iters, le_max=255, ext_scale_q=4)
    assert share == 0.0 and int(np.abs(le).max()) < 255, "the reference clamped nothing"
    for b in range(B):
        ob, ol = O.turbo_decode(q[b].astype(np.float64), K, f1, f2, iters, O.ALGO_MAXLOG)
        assert np.array_equal(rows[b], ob.astype(np.uint8))
        assert np.array_equal(le[b].astype(np.float64), ol)   # every Le value, tail positions included


def test_scaled_extrinsic_beats_float_maxlog():
    """The 3/4 extrinsic scale is what makes Max-Log-MAP usable: fewer bit errors than the unscaled float
    Max-Log-MAP oracle on the same quantised frames (K = 1024, 1.0 dB, seed 9, 384 frames, 6 iterations)."""
    K, f1, f2, B, iters = 1024, 31, 64, 384, 6
    src, flow = O.synth_batch(K, f1, f2, 1.0, 9, B)
    q = F.quantise(flow, 4)
    rows, _, _ = F.decode(q, K, f1, f2, iters, le_max=255, ext_scale_q=3)
    fixed_err = int((rows[:, -1] != src).sum())
    float_err = int((O.decode_batch(q.astype(np.float64), K, f1, f2, iters, O.ALGO_MAXLOG, nthreads=4) != src).sum())
    print(f"bit errors: fixed (3/4) {fixed_err}, float Max-Log-MAP {float_err}")
    assert fixed_err < float_err


def test_saturating_dematch_reference():
    """The reference's own corner cases: repetition saturates, -128 is read as -127 when it is added to,
    and an unselected position keeps its prior byte."""
    K = 40
    n = 3 * K + 12
    E = 5 * K
    e = np.full((1, E), 100, dtype=np.int8)
    out = F.dematch(e, K, 0, 0)
    assert out.max() == 127 and out.min() >= 0
    prior = np.full((1, n), -128, dtype=np.int8)
    few = F.dematch(np.zeros((1, 10), dtype=np.int8), K, 0, 0, prior=prior)
    assert (few == -127).sum() == 10 and (few == -128).sum() == n - 10


# ------------------------------------------------------------------ the kernel's arithmetic on the host
def _run_core(exe, tmp_path, q, K, f1, f2, iters, all_iters, le_max, scale):
    """tests/fixed_core_host.cpp (csrc/td_fixed_core.h, what a lane of the gfx950 kernel runs, as a stand-alone
    host program under ASan + UBSan): the exact schedule, no rule, no table."""
    return run_core(exe, tmp_path, q, O.qpp(K, f1, f2), iters, all_iters, (le_max, scale))[:2]


@pytest.mark.parametrize("K,f1,f2,iters,setting", [(8, 3, 4, 3, (255, 4)), (13, 1, 0, 2, (31, 2)), (16, 1, 4, 2, (255, 3)),
                                                   (29, 1, 0, 2, (127, 3)), (40, 3, 10, 4, (255, 3)),
                                                   (1024, 31, 64, 3, (127, 3))]
                         + [(K, *Z.interleaver(K), 3, Z.setting(K)) for K in Z.SIZES])
def test_kernel_arithmetic_on_the_host_equals_restatement(core_host, tmp_path, K, f1, f2, iters, setting):
    """Block lengths round the 16-step window (L = 11, 16, 19, 32, 43, 1027) and fixed_size_cases.SIZES
    (every residue of L mod 16 with one, two and eight windows; non-identity interleavers), AWGN at 16
    steps per unit next to the saturated patterns, every row and every Le; ASan watches the workspace's
    bounds."""
    n = 3 * K + 12
    q = np.concatenate([
        F.quantise(O.synth_batch(K, f1, f2, 1.0, 5, 3)[1], 16),
        np.full((1, n), 127, dtype=np.int8), np.full((1, n), -128, dtype=np.int8),
        (127 * (1 - 2 * (np.arange(n) & 1))).astype(np.int8)[None, :],
        np.random.default_rng(K).integers(-128, 128, (2, n)).astype(np.int8)])
    rows, le, _ = F.decode(q, K, f1, f2, iters, *setting)
    g_rows, g_le = _run_core(core_host, tmp_path, q, K, f1, f2, iters, True, *setting)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_le, le)
    g_last, _ = _run_core(core_host, tmp_path, q, K, f1, f2, iters, False, *setting)
    assert np.array_equal(g_last[:, 0], rows[:, -1])
