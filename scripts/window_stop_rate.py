#!/usr/bin/env python3
"""Decode rate of the windowed schedule with per-codeword early termination (td_set_window_stop)
against the full windowed decode, and the cost of the feature with the rule off (DESIGN.md "Early
termination", windowed).  The windowed sibling of early_stop_rate.py, same method: one child process
per row (its own handle and clocks), timed with td_profile_read over the decode's launches alone.

Config 5: K = 6144, W = 64, g = 30, B = 32768, 8 iterations.  Frames: the device generator
(td_synth_frames, seed 4242) for the rule-off and HDA rows; for CRC rows 4096 host-made frames that
carry gCRC24B (early_stop_rate.crc_frames), tiled to B.

    window_stop_rate.py [--out profiles/early_stop/window_stop_rate.json]
    window_stop_rate.py --ab OTHER_LIB.so   rule-off A/B of this tree's library against another build
                                            (the parent commit's), interleaved, the other build first
                                            in each pair, 5 runs each: fp64 log-MAP, fp32, Max-Log-MAP

Per row: decoded Mbit/s, mean iterations used per codeword, the mean over the waves of 64 codewords
of the wave's last iteration (what the launches actually run: 8 over it is the gain's ceiling), and
the bits that differ from the full windowed decode of the same frames.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

K, F1, F2, ITERS, W, G = 6144, 263, 480, 8, 64, 30
CRC_DISTINCT = 4096


def child(a):
    import numpy as np
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    dev = torch.device("cuda", 0)
    with TurboCodec(K, F1, F2, iterations=ITERS, algo=a.algo, precision=a.precision) as c:
        c.set_window(W, G)
        if a.frames == "crc":
            from early_stop_rate import crc_frames
            n = min(a.B, CRC_DISTINCT)
            info, x = crc_frames(n, a.ebn0, 7, dev)
            rep = (a.B + n - 1) // n
            info, x = info.repeat(rep, 1)[:a.B].contiguous(), x.repeat(rep, 1)[:a.B].contiguous()
        else:
            c.synth_seed(4242)
            info, x = c.synth(a.B, a.ebn0)
        if a.precision == "f32":
            x = x.float()
        c.reserve(a.B)
        bits = torch.empty((a.B, K), dtype=torch.uint8, device=dev)
        used = torch.empty((a.B,), dtype=torch.int32, device=dev)
        full = None
        if a.rule != "off":
            full = c.decode(x).clone()
            c.set_window_early_stop(a.rule)
        for _ in range(a.warmup):
            c.decode(x, bits)
        torch.cuda.synchronize()
        c.profile(True)
        for _ in range(a.steps):
            c.decode(x, bits)
        torch.cuda.synchronize()
        _, ms, launches = c.kernel_ms()
        c.profile(False)
        row = {"rule": a.rule, "frames": a.frames, "algo": a.algo, "precision": a.precision, "B": a.B,
               "ebn0_db": a.ebn0, "K": K, "iterations": ITERS, "window": W, "overlap": G,
               "decode_ms": round(ms, 4), "launches": launches, "mbit_s": round(a.B * K / ms / 1e3, 1),
               "lib": os.environ.get("TD_LIB_PATH", "")}
        if a.rule != "off":
            c.decode(x, bits, iters_out=used)
            torch.cuda.synchronize()
            n = used.cpu().numpy()
            wave = np.concatenate([n, np.zeros((-len(n)) % 64, dtype=n.dtype)]).reshape(-1, 64).max(axis=1)
            row.update(mean_iters_used=round(float(n.mean()), 4), mean_wave_last_iter=round(float(wave.mean()), 4),
                       iters_hist=[int((n == k).sum()) for k in range(1, ITERS + 1)],
                       bits_differing_from_full=int((bits != full).sum().item()),
                       ber_stopped=float((bits != info).float().mean().item()),
                       ber_full=float((full != info).float().mean().item()))
    print("ROW " + json.dumps(row), flush=True)


def run_child(extra, env=None, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *extra], capture_output=True, text=True,
                       env=env, timeout=timeout)
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            return json.loads(line[4:])
    raise RuntimeError(f"child {extra} failed ({r.returncode}): {r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rule", default="off", choices=["off", "hda", "crc"])
    ap.add_argument("--frames", default="synth", choices=["synth", "crc"])
    ap.add_argument("--algo", default="logmap", choices=["logmap", "maxlog"])
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    ap.add_argument("--B", type=int, default=32768)
    ap.add_argument("--ebn0", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ab", default="", metavar="LIB", help="rule-off A/B against this other build of the library")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "early_stop", "window_stop_rate.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    if os.path.exists(a.out):
        res = json.load(open(a.out))
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--B", str(a.B)]
    if a.ab:
        rows, cfgs = [], (("logmap", "f64"), ("logmap", "f32"), ("maxlog", "f64"))
        for algo, prec in cfgs:
            for run in range(a.runs):
                for tag, lib in (("other", a.ab), ("this", "")):   # the other build first in each pair
                    env = dict(os.environ)
                    env.pop("TD_LIB_PATH", None)
                    if lib:
                        env["TD_LIB_PATH"] = os.path.abspath(lib)
                    r = run_child(["--rule", "off", "--algo", algo, "--precision", prec, "--ebn0", "1.0", *common], env)
                    r.update(build=tag, run=run)
                    rows.append(r)
                    print(algo, prec, tag, run, r["mbit_s"], flush=True)
        summ = {}
        for algo, prec in cfgs:
            for tag in ("other", "this"):
                v = [r["mbit_s"] for r in rows if (r["algo"], r["precision"], r["build"]) == (algo, prec, tag)]
                summ[f"{algo}_{prec}_{tag}"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        res["rule_off_ab"] = {"rows": rows, "summary": summ}
    else:
        rows = []
        for ebn0 in (1.0, 0.3):
            for frames, rules in (("synth", ("off", "hda")), ("crc", ("off", "crc"))):
                for rule in rules:
                    r = run_child(["--rule", rule, "--frames", frames, "--ebn0", str(ebn0), *common], timeout=900)
                    rows.append(r)
                    print(json.dumps(r), flush=True)
        res["gain"] = rows
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(res, fp, indent=1)
        fp.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
