"""Decoded Mbit/s of the fixed-point decoder (precision "fixed") against this tree's fp32 Max-Log-MAP
exact schedule, in one process on one GPU: K = 6144, 8 iterations, frames of the device generator at
1.0 dB; the fixed decoder gets them quantised at 8 steps per unit LLR, fp32 gets them as they are.

Per batch size and decoder: td_reserve, warm-up decodes, then `samples` readings of td_profile_read
over `reps` decodes each (demultiplex + decode kernels; the median reading counts).  Mbit/s = B * K
information bits over that time.  The bit errors of both decoders on the same frames go along, so that
a fast wrong answer shows.  Needs an MI355X: there is no CPU path.

    python scripts/fixed_throughput.py [--B 4096 32768] [--reps 10] [--samples 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, F1, F2, ITERS, EBN0, STEPS = 6144, 263, 480, 8, 1.0, 8
CHUNK = 4096   # frames generated at a time (the generator's output is fp64)


def measure(c, x, reps, samples, warm=3):
    import torch
    B = x.shape[0]
    bits = torch.empty((B, K), dtype=torch.uint8, device=x.device)
    c.reserve(B)
    for _ in range(warm):
        c.decode(x, bits)
    torch.cuda.synchronize()
    c.profile(True)
    ms = []
    for _ in range(samples):
        for _ in range(reps):
            c.decode(x, bits)
        demux_ms, decode_ms, n = c.kernel_ms()
        assert n == reps
        ms.append((demux_ms + decode_ms, demux_ms))
    c.profile(False)
    tot = [m[0] for m in ms]
    med = statistics.median(tot)
    return bits, {"ms": med, "min_ms": min(tot), "max_ms": max(tot), "demux_ms": statistics.median(m[1] for m in ms),
                  "Mbps": B * K / med / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    if not torch.cuda.is_available():
        raise SystemExit("fixed_throughput: needs an MI355X")
    dev = torch.device("cuda", 0)
    res = {"K": K, "iterations": ITERS, "ebn0_db": EBN0, "steps_per_unit": STEPS, "reps": a.reps, "samples": a.samples,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for B in a.B:
        with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="f32") as f32, \
                TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as fx:
            f32.synth_seed(1)
            info = torch.empty((B, K), dtype=torch.uint8, device=dev)
            x32 = torch.empty((B, 3 * K + 12), dtype=torch.float32, device=dev)
            for b0 in range(0, B, CHUNK):
                n = min(CHUNK, B - b0)
                i, llr = f32.synth(n, EBN0)
                info[b0:b0 + n] = i
                x32[b0:b0 + n] = llr.to(torch.float32)
                del llr
            x8 = decoder.quantise(x32, STEPS)
            case = {"B": B}
            # alternate the two decoders: both see the same clocks and neighbours
            runs = {"fixed": [], "f32_maxlog": []}
            for _ in range(2):
                for name, c, x in (("fixed", fx, x8), ("f32_maxlog", f32, x32)):
                    bits, r = measure(c, x, a.reps, a.samples)
                    r["bit_errors"] = int((bits != info).sum().item())
                    runs[name].append(r)
            for name, rs in runs.items():
                case[name] = min(rs, key=lambda r: r["ms"])
                case[name]["runs_ms"] = [r["ms"] for r in rs]
            case["fixed_over_f32"] = case["fixed"]["Mbps"] / case["f32_maxlog"]["Mbps"]
            case["fixed_workspace_bytes"] = fx.workspace_bytes()
            case["f32_workspace_bytes"] = f32.workspace_bytes()
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del x32, x8, info
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
