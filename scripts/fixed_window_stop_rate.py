#!/usr/bin/env python3
"""Decode rate of the fixed-point decoder's sub-block schedule with per-codeword early termination
(td_set_fixed_window_stop) against the same schedule with the rule off (DESIGN.md "Fixed point").  The
protocol of fixed_stop_rate.py: K = 6144, 8 iterations, the Python default window {64, 48}, LLRs
quantised at 8 steps per unit, td_reserve, warm-up, then the median of `samples` td_profile_read
readings over `reps` decodes each (demultiplex + decode kernels).

Rule off and rule on alternate on one handle in one process, so both see the same clocks and
neighbours.  HDA runs on the device generator's frames (td_synth_frames, seed 4242), CRC on up to 4096
host-made frames that carry gCRC24B (early_stop_rate.crc_frames), tiled to B.  Eb/N0 1.0 dB, and 0.3 dB
for what the rule costs where nothing converges.  A third mode, the rule with min_iters == iterations
("unjudged"), runs the stopping kernels and the decision launches but gathers no evidence and stops
nothing: unjudged - off is what the decision launches, the state reads and a stored row per iteration
cost, on - unjudged (where nothing converges) what the evidence costs: the previous row's loads and the
per-iteration stores of the sub-blocks' words.

Per run: ms and Mbit/s of each mode, on / off, the mean of iters_used, the mean over the waves of 64
codewords of the wave's maximum (what a wave actually runs: 8 over it is the ceiling of the gain), and
the bit errors of both decodes.  Needs an MI355X: there is no CPU path.

    python scripts/fixed_window_stop_rate.py [--B 1 64 1024 4096 32768] [--ebn0 1.0 0.3] [--rules hda crc]
                                             [--out profiles/fixed/window_stop_rate.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from fixed_stop_rate import frames  # noqa: E402
from fixed_throughput import F1, F2, ITERS, K, STEPS, measure  # noqa: E402
from fixed_window_throughput import WINDOW  # noqa: E402

MODES = ("off", "on", "unjudged")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 1024, 4096, 32768])
    ap.add_argument("--ebn0", type=float, nargs="+", default=[1.0, 0.3])
    ap.add_argument("--rules", nargs="+", default=["hda", "crc"], choices=["hda", "crc"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fixed", "window_stop_rate.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    if not torch.cuda.is_available():
        raise SystemExit("fixed_window_stop_rate: needs an MI355X")
    dev = torch.device("cuda", 0)
    res = {"K": K, "iterations": ITERS, "steps_per_unit": STEPS, "window": {"window": WINDOW[0], "overlap": WINDOW[1]},
           "reps": a.reps, "samples": a.samples, "device": torch.cuda.get_device_name(0), "runs": []}
    if os.path.exists(a.out):   # a long measurement may be split over several calls
        res["runs"] = json.load(open(a.out)).get("runs", [])
    for ebn0 in a.ebn0:
        for rule in a.rules:
            with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as c:
                c.set_fixed_window(*WINDOW)
                info_all, x_all = frames(c, rule, ebn0, max(a.B), dev)
                for B in a.B:
                    info, x = info_all[:B], x_all[:B]
                    ms = {m: [] for m in MODES}
                    err = {}
                    for _ in range(2):   # off, on, unjudged, off, on, unjudged
                        for mode in MODES:
                            if mode == "off":
                                c.set_fixed_window_early_stop(None)
                            else:
                                c.set_fixed_window_early_stop(rule, min_iters=1 if mode == "on" else ITERS)
                            bits, r = measure(c, x, a.reps, a.samples)
                            ms[mode].append(r)
                            err[mode] = int((bits != info).sum().item())
                    assert err["unjudged"] == err["off"], "min_iters == iterations is the rule-off decode"
                    c.set_fixed_window_early_stop(rule)
                    used = torch.empty((B,), dtype=torch.int32, device=dev)
                    c.decode(x, iters_out=used)
                    torch.cuda.synchronize()
                    n = used.cpu().numpy()
                    wave = np.concatenate([n, np.zeros((-len(n)) % 64, dtype=n.dtype)]).reshape(-1, 64).max(axis=1)
                    off, on, unj = (min(ms[m], key=lambda r: r["ms"]) for m in MODES)
                    run = {"rule": rule, "frames": "crc24b" if rule == "crc" else "generator", "ebn0_db": ebn0, "B": B,
                           "off": off, "on": on, "unjudged": unj, "off_runs_ms": [r["ms"] for r in ms["off"]],
                           "on_runs_ms": [r["ms"] for r in ms["on"]], "unjudged_runs_ms": [r["ms"] for r in ms["unjudged"]],
                           "on_over_off": off["ms"] / on["ms"], "unjudged_over_off": off["ms"] / unj["ms"],
                           "mean_iters_used": float(n.mean()), "mean_wave_max": float(wave.mean()),
                           "ceiling": ITERS / float(wave.mean()),
                           "iters_hist": [int((n == k).sum()) for k in range(1, ITERS + 1)],
                           "wave_max_hist": [int((wave == k).sum()) for k in range(1, ITERS + 1)],
                           "bit_errors_off": err["off"], "bit_errors_on": err["on"]}
                    res["runs"] = [r for r in res["runs"] if (r["rule"], r["ebn0_db"], r["B"]) != (rule, ebn0, B)] + [run]
                    print(json.dumps(run), flush=True)
                del info_all, x_all
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
