"""Speed of the batched device encoder (td_encode_device) and of the CRC-24 attach / check at K = 6144,
B = 4096 and 32768, each next to a device-to-device copy of the bytes it must move, in one process:

  encode      td_encode_device, hipEvents round `reps` back-to-back launches per sample (median of samples)
  copy        a device-to-device copy of the same bytes (K in + 3K+12 out per codeword: it reads and writes
              (K + 3K+12) / 2 bytes a codeword), timed the same way
  synth       for context, td_synth_frames at the same B: the frame generator whose encoder runs one thread a
              frame, serial over K (it also draws the bits and the noise and writes fp64 LLRs, and it
              synchronises; fewer launches per sample)
  crc_attach  td_crc_attach: reads K - 24 bytes, writes 24 a codeword; crc_check: reads K, writes 4; each with
              its own copy

GB/s counts the bytes the kernel must move (the QPP and syndrome tables are 24 KB and stay in cache).  The
bar is DESIGN.md "Rate matching"'s: within a factor of two of the copy.  Needs an MI355X: there is no CPU path.

    python scripts/encode_bw.py [--K 6144] [--B 4096 32768] [--reps 100] [--samples 9] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def measure(fn, nbytes, reps, samples):
    timed(fn, 3, 1)   # warm-up
    med, lo, hi = timed(fn, reps, samples)
    return {"ms": med, "min_ms": lo, "max_ms": hi, "bytes": nbytes, "GBps": nbytes / med / 1e6}


def copy_of(nbytes, reps, samples, dev):
    """A device-to-device copy that moves nbytes in all: nbytes / 2 read, nbytes / 2 written."""
    import torch
    src = torch.randint(0, 255, (nbytes // 2,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return measure(lambda: dst.copy_(src), nbytes, reps, samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=6144)
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--synth-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, _native as N
    if not torch.cuda.is_available():
        raise SystemExit("encode_bw: needs an MI355X")
    dev = torch.device("cuda", 0)
    K = a.K
    n = 3 * K + 12
    f1, f2 = QPP[K]
    res = {"K": K, "reps": a.reps, "samples": a.samples, "synth_reps": a.synth_reps, "cases": []}
    with TurboCodec(K, f1, f2, iterations=1) as c:
        c.set_crc(N.CRC24B)
        c.synth_seed(1)
        for B in a.B:
            info = torch.randint(0, 2, (B, K), dtype=torch.uint8, device=dev)
            coded = torch.empty((B, n), dtype=torch.uint8, device=dev)
            rem = torch.empty((B,), dtype=torch.int32, device=dev)
            case = {"B": B}
            case["encode"] = measure(lambda: c.encode(info, out=coded), B * (K + n), a.reps, a.samples)
            case["copy"] = copy_of(B * (K + n), a.reps, a.samples, dev)
            case["encode_over_copy"] = case["encode"]["ms"] / case["copy"]["ms"]
            case["crc_attach"] = measure(lambda: c.crc_attach(info), B * K, a.reps, a.samples)
            case["crc_attach_copy"] = copy_of(B * K, a.reps, a.samples, dev)
            case["crc_attach_over_copy"] = case["crc_attach"]["ms"] / case["crc_attach_copy"]["ms"]
            case["crc_check"] = measure(lambda: c.crc_check(info, out=rem), B * (K + 4), a.reps, a.samples)
            case["crc_check_copy"] = copy_of(B * (K + 4) // 2 * 2, a.reps, a.samples, dev)
            case["crc_check_over_copy"] = case["crc_check"]["ms"] / case["crc_check_copy"]["ms"]
            case["crc_check_all_zero_after_attach"] = not bool(c.crc_check(info).any().item())
            # the frame generator at the same B (its LLR buffer is B * n doubles)
            sinfo = torch.empty((B, K), dtype=torch.uint8, device=dev)
            sllr = torch.empty((B, n), dtype=torch.float64, device=dev)
            case["synth"] = measure(lambda: c.synth(B, 1.0, info=sinfo, llr=sllr), B * (K + 8 * n), a.synth_reps, 3)
            case["synth_over_encode"] = case["synth"]["ms"] / case["encode"]["ms"]
            res["cases"].append(case)
            del info, coded, rem, sinfo, sllr
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
