"""The receive front end restated in numpy (td_llr_convert, td_demod_dematch): pyoracle.demodulate, the
conversion, then ratematch_ref.dematch (float) or fixed_ref.dematch (int8).  Shared by test_frontend_host.py
and test_gpu_frontend.py, with the test vectors and the (Ncb, rv, E) families both use."""
import numpy as np

import fixed_ref as FX
import pyoracle as O
import ratematch_ref as RM

NP_DT = {"f64": np.float64, "f32": np.float32, "fixed": np.int8}
MODS = (1, 2, 3, 4, 6)
KF = 0.83


def convert(x, precision, steps_per_unit=8.0):
    """td_llr_convert: float64 -> the precision's dtype."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if precision == "fixed":
            return np.clip(np.rint(x * steps_per_unit), -127, 127).astype(np.int8)
        return x.astype(NP_DT[precision])


def tie_vector(s=8.0):
    """Exact ties (n + 1/2) / s for even and odd n of both signs (s a power of two: the products are
    exact), +-0, a subnormal, values just inside and outside +-127 / s, +-1e300, +-inf."""
    n = np.array([0, 1, 2, 3, 4, 5, 62, 63, 125, 126, 127, 128], dtype=np.float64)
    ties = (n + 0.5) / s
    edge = np.array([127 / s, np.nextafter(127.5 / s, 0), 127.5 / s, np.nextafter(127.5 / s, 1e9),
                     np.nextafter(126.5 / s, 0), np.nextafter(126.5 / s, 1e9), 128 / s, 1000.0])
    x = np.concatenate([ties, -ties, edge, -edge, [0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1e-30, 0.3, -0.3],
                        [1e300, -1e300, np.inf, -np.inf, 3.5e38, -3.5e38, 3.4028235677973366e38]])
    return x.astype(np.float64)


def symbols(shape, seed):
    """Received symbols as tests/test_gpu_modem.py has them: normal(0, 1.2), demapped at Kf = 0.83."""
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1.2, shape), rng.normal(0, 1.2, shape)


def values(yi, yq, M, precision, steps_per_unit=8.0, Kf=KF):
    """e [B, E]: the transmitted values of codeword b demapped from its own E / M symbols and converted."""
    B = yi.shape[0]
    return convert(O.demodulate(yi.reshape(-1), yq.reshape(-1), M, Kf).reshape(B, -1), precision, steps_per_unit)


def restate(yi, yq, M, precision, K, Ncb, rv, prior=None, steps_per_unit=8.0, Kf=KF):
    """td_demod_dematch: yi, yq [B, E / M] -> [B, 3K+12] of the precision's dtype."""
    e = values(yi, yq, M, precision, steps_per_unit, Kf)
    return (FX if precision == "fixed" else RM).dematch(e, K, Ncb, rv, prior=prior)


def cases(K, M):
    """The (Ncb, rv, E) families of test_gpu_ratematch._dematch_cases -- puncturing, repetition with
    E > 2 Nnn, a soft buffer of Kpi + 1 and of a mid length, rv 0-3 -- with E rounded UP to a multiple of M
    (odd E survives for M = 1 and 3) and the tiny case at E = M."""
    _, _, Kpi, Kw, _ = RM.layout(K)
    mid = (Kpi + (Kw - Kpi) // 2) | 1
    nnn = RM.n_nonnull(K)
    raw = [(0, 0, nnn - nnn // 3), (0, 1, 2 * nnn + 5), (Kpi + 1, 2, nnn // 2 + 1), (Kpi + 1, 0, 2 * Kpi + 1),
           (mid, 3, nnn - 1), (mid, 1, 2 * RM.n_nonnull(K, mid) + 5), (0, 2, nnn), (0, 3, 1)]
    return [(Ncb, rv, -(-E // M) * M) for Ncb, rv, E in raw]
