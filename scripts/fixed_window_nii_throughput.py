"""Decoded Mbit/s of the fixed-point decoder's sub-block schedule with next-iteration initialisation
(td_set_fixed_window_nii) against the Python default {64, 48} without it, in one process on one GPU:
scripts/fixed_window_throughput.py's protocol and `measure` (K = 6144, 8 iterations, frames of the device
generator at 1.0 dB quantised at 8 steps per unit LLR).

Three handles alternate, twice, per batch size: {64, 48} with NII off, {64, --nii-overlap} with NII on (the
setting profiles/fixed/window_nii_ber.json recommends) and {64, 16} with NII off -- the floor that NII's
loads, stores and first iteration are paid against.  The median reading counts, the better turn is
reported and both are kept; the bit errors on the same frames go along.  Needs an MI355X.

    python scripts/fixed_window_nii_throughput.py [--B 1 64 1024 4096 32768 131072] [--nii-overlap 16] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fixed_throughput import CHUNK, EBN0, F1, F2, ITERS, K, STEPS, measure   # noqa: E402

WINDOW = 64
DEFAULT_OVERLAP = 48
FLOOR_OVERLAP = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 1024, 4096, 32768, 131072])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--nii-overlap", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = a.nii_overlap

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    if not torch.cuda.is_available():
        raise SystemExit("fixed_window_nii_throughput: needs an MI355X")
    dev = torch.device("cuda", 0)
    res = {"K": K, "iterations": ITERS, "ebn0_db": EBN0, "steps_per_unit": STEPS, "reps": a.reps, "samples": a.samples,
           "window": WINDOW, "default_overlap": DEFAULT_OVERLAP, "nii_overlap": g, "floor_overlap": FLOOR_OVERLAP,
           "recursion_work": {"default": (WINDOW + 2 * DEFAULT_OVERLAP) / WINDOW, "nii": (WINDOW + 2 * g) / WINDOW,
                              "floor": (WINDOW + 2 * FLOOR_OVERLAP) / WINDOW},
           "device": torch.cuda.get_device_name(0), "cases": []}
    settings = (("default", (WINDOW, DEFAULT_OVERLAP), False), ("nii", (WINDOW, g), True), ("floor", (WINDOW, FLOOR_OVERLAP), False))
    for B in a.B:
        codecs = [TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") for _ in settings]
        try:
            for c, (_, win, nii) in zip(codecs, settings):
                c.set_fixed_window(*win, nii=nii)   # before measure's reserve
            with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="f64") as gen:
                gen.synth_seed(1)
                info = torch.empty((B, K), dtype=torch.uint8, device=dev)
                x8 = torch.empty((B, 3 * K + 12), dtype=torch.int8, device=dev)
                for b0 in range(0, B, CHUNK):
                    n = min(CHUNK, B - b0)
                    i, llr = gen.synth(n, EBN0)
                    info[b0:b0 + n] = i
                    x8[b0:b0 + n] = decoder.quantise(llr.to(torch.float32), STEPS)
                    del llr
            case = {"B": B}
            runs = {name: [] for name, _, _ in settings}
            for _ in range(2):   # alternate: all see the same clocks and neighbours
                for c, (name, _, _) in zip(codecs, settings):
                    bits, r = measure(c, x8, a.reps, a.samples)
                    r["bit_errors"] = int((bits != info).sum().item())
                    r["workspace_bytes"] = c.workspace_bytes()
                    runs[name].append(r)
            for name, rs in runs.items():
                case[name] = min(rs, key=lambda r: r["ms"])
                case[name]["runs_ms"] = [r["ms"] for r in rs]
            case["nii_over_default"] = case["nii"]["Mbps"] / case["default"]["Mbps"]
            case["floor_over_default"] = case["floor"]["Mbps"] / case["default"]["Mbps"]
            case["nii_over_floor"] = case["nii"]["Mbps"] / case["floor"]["Mbps"]
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
        finally:
            for c in codecs:
                c.close()
        del x8, info
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
