#!/usr/bin/env python3
"""Decode rate with per-codeword early termination (td_set_early_stop) against the full decode, and
the cost of the feature with the rule off (DESIGN.md "Early termination").

One child process per configuration (its own handle, workspace placement and clocks), timed with
td_profile_read over the turbo launch alone.  Frames: the device generator (td_synth_frames) for the
rule-off and HDA rows; for CRC rows, frames whose last 24 information bits are the gCRC24B of the
rest, encoded and put through BPSK + AWGN on the host and uploaded.

    early_stop_rate.py [--out profiles/early_stop/early_stop_rate.json] [--quick]
    early_stop_rate.py --ab OTHER_LIB.so      rule-off A/B of this tree's library against another build
                                              (e.g. the parent commit's), interleaved, 5 runs each

Per row: decoded Mbit/s (information bits over the turbo launch), mean iterations used per codeword,
mean over the groups of 8 of the group's last iteration (what the workgroup actually ran: their ratio
is what per-group stopping leaves on the table), and the bit differences of the stopped decode
against the full decode of the same frames.
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

K, F1, F2, ITERS = 6144, 263, 480, 8
CRC24B = 0x800063


def crc_frames(B, ebn0_db, seed, dev):
    """B frames with a code-block CRC, as a float64 device tensor [B, 3K+12] and their info bits."""
    import ctypes as C

    import numpy as np
    import pyoracle as O
    import torch

    from turbo_decoder_cuda_amd import _native as N
    tab = np.zeros(K - 24, dtype=np.uint32)   # the CRC of the K-24 payload bits, by position
    N.check(N.lib().td_crc24_syndromes(K - 24, CRC24B, tab.ctypes.data_as(C.c_void_p)))
    rng = np.random.default_rng(seed)
    n = 3 * K + 12
    rate = K / n
    sigma = (2.0 * rate * 10.0 ** (ebn0_db / 10.0)) ** -0.5
    flow = torch.empty((B, n), dtype=torch.float64, device=dev)
    info = torch.empty((B, K), dtype=torch.uint8, device=dev)
    for b0 in range(0, B, 256):
        nb = min(256, B - b0)
        rows = np.zeros((nb, K), dtype=np.int32)
        rows[:, :K - 24] = rng.integers(0, 2, (nb, K - 24))
        chunk = np.zeros((nb, n))
        for b in range(nb):
            c = int(np.bitwise_xor.reduce(tab[rows[b, :K - 24] == 1], initial=0))
            rows[b, K - 24:] = [(c >> (23 - j)) & 1 for j in range(24)]
            coded = O.encode(rows[b], F1, F2)
            chunk[b] = 2.0 * ((2.0 * coded - 1.0) + rng.normal(0.0, sigma, n)) / sigma ** 2
        flow[b0:b0 + nb] = torch.from_numpy(chunk).to(dev)
        info[b0:b0 + nb] = torch.from_numpy(rows.astype(np.uint8)).to(dev)
    return info, flow


def child(a):
    import numpy as np
    import torch

    from turbo_decoder_cuda_amd import TurboCodec
    dev = torch.device("cuda", 0)
    with TurboCodec(K, F1, F2, iterations=ITERS, algo=a.algo) as c:
        if a.rule == "crc":
            info, x = crc_frames(a.B, a.ebn0, 7, dev)
        else:
            c.synth_seed(4242)
            info, x = c.synth(a.B, a.ebn0)
        c.reserve(a.B)
        bits = torch.empty((a.B, K), dtype=torch.uint8, device=dev)
        used = torch.empty((a.B,), dtype=torch.int32, device=dev)
        full = None
        if a.rule != "off":
            full = c.decode(x).clone()
            c.set_early_stop(a.rule)
        for _ in range(a.warmup):
            c.decode(x, bits)
        torch.cuda.synchronize()
        c.profile(True)
        for _ in range(a.steps):
            c.decode(x, bits)
        torch.cuda.synchronize()
        _, ms, launches = c.kernel_ms()
        c.profile(False)
        row = {"rule": a.rule, "algo": a.algo, "B": a.B, "ebn0_db": a.ebn0, "K": K, "iterations": ITERS,
               "turbo_ms": round(ms, 4), "launches": launches, "mbit_s": round(a.B * K / ms / 1e3, 1),
               "lib": os.environ.get("TD_LIB_PATH", "")}
        if a.rule != "off":
            c.decode(x, bits, iters_out=used)
            torch.cuda.synchronize()
            n = used.cpu().numpy()
            grp = np.concatenate([n, np.zeros((-len(n)) % 8, dtype=n.dtype)]).reshape(-1, 8).max(axis=1)
            row.update(mean_iters_used=round(float(n.mean()), 4), mean_group_last_iter=round(float(grp.mean()), 4),
                       iters_hist=[int((n == k).sum()) for k in range(1, ITERS + 1)],
                       bits_differing_from_full=int((bits != full).sum().item()),
                       ber_vs_full=float((bits != full).float().mean().item()),
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
    ap.add_argument("--algo", default="logmap", choices=["logmap", "maxlog"])
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--ebn0", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ab", default="", metavar="LIB", help="rule-off A/B against this other build of the library")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="B = 4096 only")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "early_stop", "early_stop_rate.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    if os.path.exists(a.out):
        res = json.load(open(a.out))
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup)]
    if a.ab:
        rows = []
        for algo in ("logmap", "maxlog"):   # configs 2 and 3
            for run in range(a.runs):
                for tag, lib in (("other", a.ab), ("this", "")):
                    env = dict(os.environ)
                    env.pop("TD_LIB_PATH", None)
                    if lib:
                        env["TD_LIB_PATH"] = os.path.abspath(lib)
                    r = run_child(["--rule", "off", "--algo", algo, "--B", "4096", "--ebn0", "1.0", *common], env)
                    r.update(build=tag, run=run)
                    rows.append(r)
                    print(algo, tag, run, r["mbit_s"], flush=True)
        summ = {}
        for algo in ("logmap", "maxlog"):
            for tag in ("other", "this"):
                v = [r["mbit_s"] for r in rows if r["algo"] == algo and r["build"] == tag]
                summ[f"{algo}_{tag}"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        res["rule_off_ab"] = {"rows": rows, "summary": summ}
    else:
        rows = []
        for B in ((4096,) if a.quick else (4096, 32768)):
            for ebn0 in (1.0, 0.3):
                for rule in ("off", "hda") + (("crc",) if B == 4096 else ()):
                    r = run_child(["--rule", rule, "--B", str(B), "--ebn0", str(ebn0), *common], timeout=900)
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
