"""Decoded Mbit/s of the fixed-point decoder's sub-block schedule (td_set_fixed_window, the Python
default {64, 48}) against the exact fixed schedule and this tree's fp32 Max-Log-MAP exact schedule, in
one process on one GPU: scripts/fixed_throughput.py's protocol (K = 6144, 8 iterations, frames of the
device generator at 1.0 dB; the fixed decoders get them quantised at 8 steps per unit LLR).

Per batch size the three decoders alternate, twice; each turn is td_reserve, warm-up decodes, then
`samples` readings of td_profile_read over `reps` decodes each (demultiplex + decode kernels; the
median reading counts, the better turn is reported and both are kept).  B = 1 is one frame's latency.
The bit errors on the same frames go along, so that a fast wrong answer shows.  Needs an MI355X.

    python scripts/fixed_window_throughput.py [--B 1 64 1024 4096 32768 131072] [--overlap 48] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fixed_throughput import CHUNK, EBN0, F1, F2, ITERS, K, STEPS, measure   # noqa: E402

WINDOW = (64, 48)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 1024, 4096, 32768, 131072])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--overlap", type=int, default=WINDOW[1])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    win = (WINDOW[0], a.overlap)

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    if not torch.cuda.is_available():
        raise SystemExit("fixed_window_throughput: needs an MI355X")
    dev = torch.device("cuda", 0)
    res = {"K": K, "iterations": ITERS, "ebn0_db": EBN0, "steps_per_unit": STEPS, "reps": a.reps, "samples": a.samples,
           "window": {"window": win[0], "overlap": win[1]}, "device": torch.cuda.get_device_name(0), "cases": []}
    for B in a.B:
        with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="f32") as f32, \
                TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as fx, \
                TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as fw:
            fw.set_fixed_window(*win)
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
            runs = {"fixed": [], "fixed_window": [], "f32_maxlog": []}
            for _ in range(2):   # alternate: all see the same clocks and neighbours
                for name, c, x in (("fixed", fx, x8), ("fixed_window", fw, x8), ("f32_maxlog", f32, x32)):
                    bits, r = measure(c, x, a.reps, a.samples)
                    r["bit_errors"] = int((bits != info).sum().item())
                    runs[name].append(r)
            for name, rs in runs.items():
                case[name] = min(rs, key=lambda r: r["ms"])
                case[name]["runs_ms"] = [r["ms"] for r in rs]
            case["window_over_fixed"] = case["fixed_window"]["Mbps"] / case["fixed"]["Mbps"]
            case["window_over_f32"] = case["fixed_window"]["Mbps"] / case["f32_maxlog"]["Mbps"]
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del x32, x8, info
            torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
