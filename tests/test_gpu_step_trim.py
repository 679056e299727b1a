"""The exact decoder's hot loop bodies (td_kernels.hip: the alpha window, whose bucket check is a
xor-add issued one step late inside the tempmax tree; the beta window; the fast fold) against the
oracle, at the smallest shapes at which each loop can go wrong:
  K = 40    L = 43: three windows, one speculated, a ragged last one (13 steps);
  K = 88    L = 91: seven windows, the last of one step;
  K = 1024  the reference's golden frames (69 windows), also against the reference's own bits;
batches of 1, 8 and 9 codewords (9: a second group with seven padding codewords).
fp64 log-MAP is the oracle's arithmetic in the oracle's order: every iteration's bits equal and
max |dLe| == 0.0 with the Le dump (generic fold), every iteration's bits equal without it (the fast
fold, whose extrinsic feeds the next SISO).  The fixed-point families run the same shapes through
the production library and the redo-forced one (every alpha window in the committed order) in one
child process each; fp32 log-MAP and fp64 Max-Log-MAP, which compile from the same templates, take one
case each with test_gpu_parity.py's / test_gpu_decode.py's tolerances."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as O
import quantised_cases as Q
import test_gpu_decode as GD
from conftest import GOLD, REPO

pytestmark = pytest.mark.gpu

PKG = os.path.join(REPO, "turbo_decoder_cuda_amd")
CODES = {40: (3, 10), 88: (5, 22), 1024: (31, 64)}
ITERS = 4


def gold_1024():
    """The six K = 1024 golden frames (one per file) and the reference's bits, 8 iterations."""
    ds = [np.load(p) for p in sorted(glob.glob(os.path.join(GOLD, "frames_K1024_*.npz")))]
    assert len(ds) == 6 and all(int(d["iters"]) == 8 and d["flow"].shape[0] == 1 for d in ds)
    return np.concatenate([d["flow"] for d in ds]), np.concatenate([d["bits"] for d in ds])


def awgn_case(K, B):
    """(flow [B, 3K+12], iterations, the reference's bits or None)."""
    if K == 1024:
        flow, bits = gold_1024()
        pick = [b % 6 for b in range(B)]   # nine codewords: the six frames and the first three again
        return np.ascontiguousarray(flow[pick]), 8, bits[pick]
    f1, f2 = CODES[K]
    return np.array(O.synth_batch(K, f1, f2, 0.5, 100 + K, 9)[1][:B]), ITERS, None


def assert_equals_oracle(K, iters, flow, bits, le, fast, what):
    f1, f2 = CODES[K]
    worst = 0.0
    for b in range(flow.shape[0]):
        ob, ol = O.turbo_decode(np.ascontiguousarray(flow[b]), K, f1, f2, iters)
        assert np.array_equal(bits[b], ob.astype(np.uint8)), f"{what} codeword {b}: bits (Le dump)"
        assert np.array_equal(fast[b], ob.astype(np.uint8)), f"{what} codeword {b}: bits (fast fold)"
        worst = max(worst, float(np.abs(le[b] - ol).max()))
    print(f"{what}: max |dLe| = {worst!r}")
    assert worst == 0.0, f"{what}: Le differs from the oracle by {worst!r}"


@pytest.mark.parametrize("B", [1, 8, 9])
@pytest.mark.parametrize("K", [40, 88, 1024])
def test_f64_logmap_equals_oracle(K, B):
    flow, iters, ref_bits = awgn_case(K, B)
    f1, f2 = CODES[K]
    bits, le = GD._decode_all(K, f1, f2, iters, flow)
    fast = GD._decode_bits(K, f1, f2, iters, flow)
    assert_equals_oracle(K, iters, flow, bits, le, fast, f"K={K} B={B}")
    if ref_bits is not None:
        assert np.array_equal(bits, ref_bits), "hard bits differ from the reference's"


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from turbo_decoder_cuda_amd import TurboCodec
d, out = np.load(sys.argv[2]), {}
K, it = int(d["K"]), int(d["iters"])
for prec, dt in (("f64", torch.float64), ("f32", torch.float32)):
    x = torch.from_numpy(d["flow"]).to("cuda").to(dt).contiguous()
    with TurboCodec(K, int(d["f1"]), int(d["f2"]), iterations=it, precision=prec) as c:
        bits = torch.empty((x.shape[0], it, K), dtype=torch.uint8, device=x.device)
        fast = torch.empty_like(bits)
        le = torch.empty((x.shape[0], it, 2, K + 3), dtype=dt, device=x.device)
        c.decode(x, bits, all_iters=True, le=le)
        c.decode(x, fast, all_iters=True)
        torch.cuda.synchronize()
    out["bits_" + prec], out["fast_" + prec], out["le_" + prec] = bits.cpu().numpy(), fast.cpu().numpy(), le.cpu().numpy()
np.savez(sys.argv[3], **out)
"""
FAMILIES = ["int8_q16", "zero", "q4"]   # q4 beside the two wide ones: its fp64 misses reach the detector at both sizes


@pytest.mark.parametrize("K", [40, 1024])
def test_families_production_redo_and_oracle(tmp_path, K):
    """int8_q16, zero and q4 batches of 9, decoded as one batch of 27 by the production library (here)
    and by the redo-forced library (a fresh child, TD_LIB_PATH): bits (both folds) and Le byte-identical
    in fp64 and fp32; the fp64 decode equals the oracle (bits, max |dLe| == 0.0).  The CPU restatement's
    miss counts are printed; where it counts misses (K = 1024: q4 in both precisions, int8_q16 in fp32)
    the production library has taken its redo path on them."""
    redo = os.path.join(PKG, "libturbo_mi355x_redo.so")
    assert os.path.exists(redo), "build() makes the redo-forced library"
    f1, f2 = CODES[K]
    B = 9
    flow = np.concatenate([Q.family_flow(K, f1, f2, B, fam) for fam in FAMILIES])
    for fam in FAMILIES:
        for prec in ("f64", "f32"):
            total, share = Q.misses(K, f1, f2, B, fam, ITERS, prec)
            print(f"K={K} {fam} {prec}: CPU misses {int(total.sum())}, redo share {share:.3f}")
            if K == 1024 and (fam == "q4" or (fam, prec) == ("int8_q16", "f32")):
                assert total.sum() > 0, "this input does not reach the speculation detector"
    np.savez(tmp_path / "in.npz", K=K, f1=f1, f2=f2, iters=ITERS, flow=flow)
    subprocess.run([sys.executable, "-c", _CHILD, REPO, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                   env=dict(os.environ, TD_LIB_PATH=redo), check=True, timeout=300)
    r = np.load(tmp_path / "out.npz")
    for prec in ("f64", "f32"):
        bits, le = GD._decode_all(K, f1, f2, ITERS, flow, precision=prec)
        fast = GD._decode_bits(K, f1, f2, ITERS, flow, precision=prec)
        assert r["bits_" + prec].tobytes() == bits.tobytes(), prec
        assert r["fast_" + prec].tobytes() == fast.tobytes(), prec
        assert r["le_" + prec].tobytes() == le.tobytes(), prec
        if prec == "f64":
            assert_equals_oracle(K, ITERS, flow, bits, le, fast, f"K={K} families")


def test_f32_logmap_small():
    """K = 88, B = 9, fp32 log-MAP against the oracle's fp32 restatement: Le within 1e-3 relative
    (test_gpu_parity.py / test_f32_logmap_vs_oracle_f32); the fast fold's bits equal the Le-dump decode's."""
    K, B = 88, 9
    f1, f2 = CODES[K]
    flow = awgn_case(K, B)[0].astype(np.float32)
    bits, le = GD._decode_all(K, f1, f2, ITERS, flow, precision="f32")
    assert np.array_equal(GD._decode_bits(K, f1, f2, ITERS, flow, precision="f32"), bits)
    for b in range(B):
        _, ol = O.turbo_decode(flow[b], K, f1, f2, ITERS)
        d = float(np.abs(le[b] - ol).max())
        print(f"codeword {b}: max |dLe| = {d:.3g} of {np.abs(ol).max():.3g}")
        assert d <= 1e-3 * max(1.0, np.abs(ol).max()), f"codeword {b}"


def test_f64_maxlog_small():
    """K = 88, B = 9, fp64 Max-Log-MAP against the oracle: bits identical, Le within 1e-9."""
    K, B = 88, 9
    f1, f2 = CODES[K]
    flow = awgn_case(K, B)[0]
    bits, le = GD._decode_all(K, f1, f2, ITERS, flow, algo="maxlog")
    assert np.array_equal(GD._decode_bits(K, f1, f2, ITERS, flow, algo="maxlog"), bits)
    for b in range(B):
        ob, ol = O.turbo_decode(flow[b], K, f1, f2, ITERS, algo=O.ALGO_MAXLOG)
        assert np.array_equal(bits[b], ob.astype(np.uint8)), f"codeword {b}"
        assert np.abs(le[b] - ol).max() <= 1e-9, f"codeword {b}"
