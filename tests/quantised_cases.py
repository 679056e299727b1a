"""Shared by test_quantised_oracle.py (CPU) and test_gpu_quantised_inputs.py: the fixed-point input
batches (llr_families on pyoracle.synth_batch frames) and their references -- the oracle's rows and
Le, and the CPU count of the speculation detector's misses -- each computed once and read-only.

The base batch of every case is O.synth_batch(K, f1, f2, EBN0, SEED, B): for K = 1024 the frames the
detector's floors are stated on (test_quantised_oracle.py)."""
import functools

import numpy as np

import llr_families as F
import pyoracle as O

EBN0, SEED = 0.5, 77

OALGO = {"logmap": O.ALGO_LOGMAP, "maxlog": O.ALGO_MAXLOG, "logmap-q": O.ALGO_LOGMAP_Q}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def awgn(K, f1, f2, B, ebn0=EBN0, seed=SEED):
    return _ro(O.synth_batch(K, f1, f2, ebn0, seed, B)[1])


@functools.lru_cache(maxsize=None)
def family_flow(K, f1, f2, B, family, ebn0=EBN0, seed=SEED):
    """float64 [B, 3K+12]; family "awgn" is the continuous batch itself."""
    base = awgn(K, f1, f2, B, ebn0, seed)
    return base if family == "awgn" else F.apply(family, base)


def as_precision(flow, precision):
    return flow if precision == "f64" else flow.astype(np.float32)


def oracle_rows(flow, K, f1, f2, iters, algo="logmap"):
    """The exact oracle on every row of flow (in flow's precision): (rows [B, iters, K] uint8, Le)."""
    rows, les = zip(*(O.turbo_decode(np.ascontiguousarray(flow[b]), K, f1, f2, iters, algo=OALGO[algo])
                      for b in range(flow.shape[0])))
    return _ro(np.array(rows).astype(np.uint8), np.array(les))


def oracle_window_rows(flow, K, f1, f2, iters, W, g, algo="logmap-q", nii=False, concurrent=False):
    rows, les = zip(*(O.turbo_decode_window(np.ascontiguousarray(flow[b]), K, f1, f2, iters, W, g, algo=OALGO[algo],
                                            nii=nii, concurrent=concurrent) for b in range(flow.shape[0])))
    return _ro(np.array(rows).astype(np.uint8), np.array(les))


@functools.lru_cache(maxsize=None)
def exact_ref(K, f1, f2, B, family, iters, algo="logmap", precision="f64", ebn0=EBN0, seed=SEED):
    """(flow in that precision, oracle rows, oracle Le) of a family batch under the exact schedule."""
    flow = _ro(np.ascontiguousarray(as_precision(family_flow(K, f1, f2, B, family, ebn0, seed), precision)))
    return (flow,) + tuple(oracle_rows(flow, K, f1, f2, iters, algo))


@functools.lru_cache(maxsize=None)
def window_ref(K, f1, f2, B, family, iters, W, g, algo="logmap-q", precision="f64", nii=False, concurrent=False):
    flow = _ro(np.ascontiguousarray(as_precision(family_flow(K, f1, f2, B, family), precision)))
    return (flow,) + tuple(oracle_window_rows(flow, K, f1, f2, iters, W, g, algo, nii, concurrent))


@functools.lru_cache(maxsize=None)
def misses(K, f1, f2, B, family, iters, precision="f64", ebn0=EBN0, seed=SEED):
    """(misses per codeword int64 [B], redo share) of the detector's CPU restatement on a family batch."""
    flow = as_precision(family_flow(K, f1, f2, B, family, ebn0, seed), precision)
    total, share = O.spec_miss_turbo(flow, K, f1, f2, iters)
    return _ro(total), share


def maxlog_dyadic_ref(flow, K, f1, f2, iters, window=None):
    """Max-Log-MAP on dyadic inputs is rounding-free: the fp32 and fp64 oracles agree on every bit and
    every Le value.  Asserts it on the rows of flow (float64) and returns (rows, Le float64).
    window = (W, g, nii, concurrent) for the windowed restatement (normalised every 4 positions in fp64
    and every 8 in fp32, as the kernels: without roundings that changes nothing either)."""
    f32 = flow.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), flow)
    if window is None:
        r64, l64 = oracle_rows(flow, K, f1, f2, iters, "maxlog")
        r32, l32 = oracle_rows(f32, K, f1, f2, iters, "maxlog")
    else:
        W, g, nii, conc = window
        r64, l64 = oracle_window_rows(flow, K, f1, f2, iters, W, g, "maxlog", nii, conc)
        r32, l32 = oracle_window_rows(f32, K, f1, f2, iters, W, g, "maxlog", nii, conc)
    assert l32.dtype == np.float32 and l64.dtype == np.float64
    assert np.array_equal(r32, r64), "fp32 and fp64 Max-Log-MAP oracles differ in a bit on dyadic input"
    assert np.array_equal(l32.astype(np.float64), l64), "fp32 and fp64 Max-Log-MAP oracles differ in an Le value"
    return r64, l64


@functools.lru_cache(maxsize=None)
def dyadic_maxlog_precondition(K, f1, f2, B, family, iters, window=None):
    """maxlog_dyadic_ref on a family batch: (flow float64, rows, Le float64)."""
    flow = family_flow(K, f1, f2, B, family)
    return (flow,) + tuple(maxlog_dyadic_ref(flow, K, f1, f2, iters, window))
