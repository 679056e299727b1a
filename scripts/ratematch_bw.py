"""Speed of the soft de-rate-matching kernel (td_rate_dematch) at BASELINE config 2's shape
(B = 4096, K = 6144, fp64, Ncb = Kw), for E = 3K+12 (every position once) and E = 2K (rate 1/2):

  dematch   rate_dematch, hipEvents round `reps` back-to-back launches per sample (median of samples)
  copy      a device-to-device copy that moves the same bytes (reads and writes (B*E + B*(3K+12)) / 2
            doubles), timed the same way in the same process
  demux     the decoder's own demultiplex kernel (3K+12 doubles a codeword in, as many out, with a
            permutation), through td_profile_read on one-iteration decodes of the same batch

GB/s counts the bytes the kernel must move: E doubles in and 3K+12 doubles out per codeword (the rank
table is 74 KB and stays in cache).  Needs an MI355X: there is no CPU path.

    python scripts/ratematch_bw.py [--B 4096] [--K 6144] [--reps 100] [--samples 9] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TD_PLACEMENT_TRIALS", "1")   # the demux time does not depend on the workspace's placement

QPP = {6144: (263, 480), 1024: (31, 64), 40: (3, 10)}


def timed(fn, reps, samples):
    """Median ms of one call of fn, over `samples` event-bracketed runs of `reps` calls."""
    import torch
    ms = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--K", type=int, default=6144)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    if not torch.cuda.is_available():
        raise SystemExit("ratematch_bw: needs an MI355X")
    dev = torch.device("cuda", 0)
    B, K = a.B, a.K
    n = 3 * K + 12
    f1, f2 = QPP[K]
    res = {"B": B, "K": K, "precision": "f64", "reps": a.reps, "samples": a.samples, "cases": []}
    with TurboCodec(K, f1, f2, iterations=1) as c:
        info = c.set_rate_matching(0)
        res["layout"] = info
        llr = torch.randn((B, n), dtype=torch.float64, device=dev)
        # the decoder's demux kernel on the same batch
        bits = torch.empty((B, K), dtype=torch.uint8, device=dev)
        c.reserve(B)
        c.decode(llr, bits)
        c.profile(True)
        for _ in range(a.reps):
            c.decode(llr, bits)
        demux_ms, _, launches = c.kernel_ms()
        c.profile(False)
        res["demux"] = {"ms": demux_ms, "launches": launches, "GBps": 2 * B * n * 8 / demux_ms / 1e6}
        out = torch.empty((B, n), dtype=torch.float64, device=dev)
        for E in (n, 2 * K):
            e = c.rate_match(llr, 0, E)
            nbytes = (B * E + B * n) * 8
            src = torch.randn(((B * E + B * n) // 2,), dtype=torch.float64, device=dev)
            dst = torch.empty_like(src)
            case = {"E": E, "bytes": nbytes}
            for name, fn in (("dematch", lambda: c.rate_dematch(e, 0, out=out)),
                             ("dematch_accumulate", lambda: c.rate_dematch(e, 0, out=out, accumulate=True)),
                             ("copy", lambda: dst.copy_(src))):
                timed(fn, 3, 1)   # warm-up
                med, lo, hi = timed(fn, a.reps, a.samples)
                moved = nbytes + (B * n * 8 if name == "dematch_accumulate" else 0)   # accumulate also reads d_llr
                case[name] = {"ms": med, "min_ms": lo, "max_ms": hi, "GBps": moved / med / 1e6}
            case["dematch_over_copy"] = case["dematch"]["ms"] / case["copy"]["ms"]
            case["dematch_over_demux"] = case["dematch"]["ms"] / demux_ms
            if E == n:   # every position sent once: the round trip is the identity
                c.rate_dematch(e, 0, out=out)
                case["identity"] = bool(torch.equal(out, llr))
            res["cases"].append(case)
            del src, dst, e
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
