"""Decoded Mbit/s of the fixed-point decoder with td_set_fixed_maxstar's table (integer log-MAP, the default
table at 8 steps per unit, {255, 4}) against the same decoder with the table off (Max-Log-MAP, {255, 3}) and
this tree's fp32 log-MAP exact schedule, in one process on one GPU: scripts/fixed_throughput.py's protocol
(K = 6144, 8 iterations, frames of the device generator at 1.0 dB; the fixed decoders get them quantised at 8
steps per unit LLR).

The points: the exact schedule at B = 32768 and 131072, and the {64, 48} sub-block schedule at B = 64, 4096 and
32768.  Per point the three decoders alternate `turns` times; each turn is td_reserve, warm-up decodes, then
`samples` readings of td_profile_read over `reps` decodes each (demultiplex + decode kernels; the median
reading counts).  Every turn's time is kept: the ratios are those of the turns' medians, and their spread is
the smallest and the largest ratio of a turn's pair.  The bit errors on the same frames go along, so that a
fast wrong answer shows.  --parent FILE.json (a run of this script on the parent commit: there the table
does not exist and only the off and fp32 decoders run) adds the off figures' distance from the parent's.
Needs an MI355X.

    python scripts/fixed_maxstar_throughput.py [--turns 3] [--reps 5] [--samples 5] [--parent FILE.json] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fixed_throughput import CHUNK, EBN0, F1, F2, ITERS, K, STEPS, measure   # noqa: E402

WINDOW = (64, 48)
POINTS = (("exact", 32768), ("exact", 131072), ("window", 64), ("window", 4096), ("window", 32768))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", default=[f"{s}:{B}" for s, B in POINTS])
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    if not torch.cuda.is_available():
        raise SystemExit("fixed_maxstar_throughput: needs an MI355X")
    dev = torch.device("cuda", 0)
    has_table = hasattr(TurboCodec, "set_fixed_maxstar")
    parent = {(c["schedule"], c["B"]): c for c in json.load(open(a.parent))["cases"]} if a.parent else {}
    res = {"K": K, "iterations": ITERS, "ebn0_db": EBN0, "steps_per_unit": STEPS, "reps": a.reps, "samples": a.samples,
           "turns": a.turns, "window": {"window": WINDOW[0], "overlap": WINDOW[1]}, "table": has_table,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for point in a.points:
        sched, B = point.split(":")[0], int(point.split(":")[1])
        with TurboCodec(K, F1, F2, iterations=ITERS, algo="logmap", precision="f32") as f32, \
                TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as off, \
                TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as on:
            if has_table:
                on.set_fixed(255, 4)
                on.set_fixed_maxstar(float(STEPS))
            if sched == "window":
                off.set_fixed_window(*WINDOW)
                on.set_fixed_window(*WINDOW)
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
            decoders = [("fixed_off", off, x8), ("f32_logmap", f32, x32)]
            if has_table:
                decoders.insert(1, ("fixed_on", on, x8))
            case = {"schedule": sched, "B": B}
            runs = {name: [] for name, _, _ in decoders}
            for _ in range(a.turns):   # alternate: all see the same clocks and neighbours
                for name, c, x in decoders:
                    bits, r = measure(c, x, a.reps, a.samples)
                    r["bit_errors"] = int((bits != info).sum().item())
                    runs[name].append(r)
            for name, rs in runs.items():
                ms = [r["ms"] for r in rs]
                med = statistics.median(ms)
                case[name] = {"ms": med, "Mbps": B * K / med / 1e3, "runs_ms": ms, "min_ms": min(ms), "max_ms": max(ms),
                              "spread": (max(ms) - min(ms)) / med, "bit_errors": rs[0]["bit_errors"]}

            def ratio(num, den):
                per_turn = [d["ms"] / n["ms"] for n, d in zip(runs[num], runs[den])]   # of rates: the times' inverse
                return {"median": case[den]["ms"] / case[num]["ms"], "min": min(per_turn), "max": max(per_turn)}

            if has_table:
                case["on_over_off"] = ratio("fixed_on", "fixed_off")
                case["on_over_f32_logmap"] = ratio("fixed_on", "f32_logmap")
            case["off_over_f32_logmap"] = ratio("fixed_off", "f32_logmap")
            if (sched, B) in parent:
                p = parent[sched, B]["fixed_off"]
                d = case["fixed_off"]["ms"] / p["ms"] - 1.0
                case["off_vs_parent"] = {"parent_ms": p["ms"], "parent_runs_ms": p["runs_ms"], "relative": d,
                                         "within_spread": abs(d) <= max(case["fixed_off"]["spread"], p["spread"])}
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
