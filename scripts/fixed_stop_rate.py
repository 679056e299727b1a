#!/usr/bin/env python3
"""Decode rate of the fixed-point decoder with per-codeword early termination (td_set_fixed_stop)
against the full fixed decode (DESIGN.md "Fixed point", early termination).  The fixed sibling of
window_stop_rate.py, measured the way fixed_throughput.py measures: K = 6144, 8 iterations, LLRs
quantised at 8 steps per unit, td_reserve, warm-up, then the median of `samples` td_profile_read
readings over `reps` decodes each (demultiplex + decode kernels).

Rule on and rule off alternate on one handle in one process, so both see the same clocks and
neighbours.  HDA runs on the device generator's frames (td_synth_frames, seed 4242), CRC on 4096
host-made frames that carry gCRC24B (early_stop_rate.crc_frames), tiled to B.  Eb/N0 1.0 dB, and 0.3 dB
for what the rule costs where nothing converges.

Per run: Mbit/s both ways, the mean of iters_used, the mean over the waves of 64 codewords of the
wave's maximum (what a wave actually runs: 8 over it is the ceiling of the decode kernel's gain),
the bit errors of both decodes, and the rule-off time next to profiles/fixed/throughput.json's for
the same B (1.0 dB generator frames: the same workload).  Needs an MI355X: there is no CPU path.

    python scripts/fixed_stop_rate.py [--B 4096 32768 131072] [--ebn0 1.0 0.3] [--rules hda crc]
                                      [--out profiles/fixed/stop_rate.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from fixed_throughput import CHUNK, F1, F2, ITERS, K, STEPS, measure  # noqa: E402

CRC_DISTINCT = 4096


def frames(c, rule, ebn0, B, dev):
    """(info uint8 [B, K], int8 LLRs [B, 3K+12]) on the device."""
    import torch

    from turbo_decoder_cuda_amd import decoder
    if rule == "crc":
        from early_stop_rate import crc_frames
        n = min(B, CRC_DISTINCT)
        info, x = crc_frames(n, ebn0, 7, dev)
        x = decoder.quantise(x, STEPS)
        rep = (B + n - 1) // n
        return info.repeat(rep, 1)[:B].contiguous(), x.repeat(rep, 1)[:B].contiguous()
    c.synth_seed(4242)
    info = torch.empty((B, K), dtype=torch.uint8, device=dev)
    x8 = torch.empty((B, 3 * K + 12), dtype=torch.int8, device=dev)
    for b0 in range(0, B, CHUNK):
        n = min(CHUNK, B - b0)
        i, llr = c.synth(n, ebn0)
        info[b0:b0 + n] = i
        x8[b0:b0 + n] = decoder.quantise(llr, STEPS)
        del llr
    return info, x8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 32768, 131072])
    ap.add_argument("--ebn0", type=float, nargs="+", default=[1.0, 0.3])
    ap.add_argument("--rules", nargs="+", default=["hda", "crc"], choices=["hda", "crc"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fixed", "stop_rate.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    if not torch.cuda.is_available():
        raise SystemExit("fixed_stop_rate: needs an MI355X")
    dev = torch.device("cuda", 0)
    parent = {}
    tp = os.path.join(REPO, "profiles", "fixed", "throughput.json")
    if os.path.exists(tp):
        parent = {c["B"]: c["fixed"] for c in json.load(open(tp))["cases"]}
    res = {"K": K, "iterations": ITERS, "steps_per_unit": STEPS, "reps": a.reps, "samples": a.samples,
           "device": torch.cuda.get_device_name(0), "runs": []}
    if os.path.exists(a.out):   # a long measurement may be split over several calls
        res["runs"] = json.load(open(a.out)).get("runs", [])
    for ebn0 in a.ebn0:
        for rule in a.rules:
            with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as c:
                info_all, x_all = frames(c, rule, ebn0, max(a.B), dev)
                for B in a.B:
                    info, x = info_all[:B], x_all[:B]
                    ms = {"off": [], "on": []}
                    err = {}
                    for _ in range(2):   # off, on, off, on
                        for mode in ("off", "on"):
                            c.set_fixed_early_stop(rule if mode == "on" else None)
                            bits, r = measure(c, x, a.reps, a.samples)
                            ms[mode].append(r)
                            err[mode] = int((bits != info).sum().item())
                    used = torch.empty((B,), dtype=torch.int32, device=dev)
                    c.decode(x, iters_out=used)   # the rule is on
                    torch.cuda.synchronize()
                    n = used.cpu().numpy()
                    wave = np.concatenate([n, np.zeros((-len(n)) % 64, dtype=n.dtype)]).reshape(-1, 64).max(axis=1)
                    off, on = (min(ms[m], key=lambda r: r["ms"]) for m in ("off", "on"))
                    run = {"rule": rule, "frames": "crc24b" if rule == "crc" else "generator", "ebn0_db": ebn0, "B": B,
                           "off": off, "on": on, "off_runs_ms": [r["ms"] for r in ms["off"]],
                           "on_runs_ms": [r["ms"] for r in ms["on"]], "speedup": off["ms"] / on["ms"],
                           "mean_iters_used": float(n.mean()), "mean_wave_max": float(wave.mean()),
                           "iters_hist": [int((n == k).sum()) for k in range(1, ITERS + 1)],
                           "wave_max_hist": [int((wave == k).sum()) for k in range(1, ITERS + 1)],
                           "bit_errors_off": err["off"], "bit_errors_on": err["on"]}
                    if B in parent and rule == "hda" and ebn0 == 1.0:
                        p = parent[B]
                        run["parent_off"] = {"ms": p["ms"], "runs_ms": p["runs_ms"], "min_ms": p["min_ms"],
                                             "max_ms": p["max_ms"]}
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
