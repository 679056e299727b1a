"""BER of the fixed-point decoder's sub-block schedule (td_set_fixed_window) against the exact fixed
schedule on the same frames: scripts/fixed_ber.py's protocol (K = 6144, 8 iterations, the device
generator's frames quantised at 8 steps per unit LLR, {le_max 255, ext_scale_q 3}).

Per point: bit and frame errors after the last iteration of the exact fixed decode and of the windowed
one at every {window, overlap} of WINDOWS, and each window's ratio to the exact schedule's counts.  The
yardstick is the exact fixed decoder.  `default_overlap` is 32 if its bit and frame errors stay within
GATE x the exact schedule's at every point (the window gate of tests/test_gpu_window.py), else the
smallest measured overlap that does, else null.  Needs an MI355X.

    python scripts/fixed_window_ber.py [--frames 32768] [--batch 4096] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TD_PLACEMENT_TRIALS", "1")   # results do not depend on the workspace's placement

K, F1, F2, ITERS, STEPS = 6144, 263, 480, 8, 8
POINTS = (0.4, 0.5, 0.6)
WINDOWS = ((64, 16), (64, 32), (64, 48), (64, 64))
GATE = 1.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--points", type=float, nargs="+", default=list(POINTS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    if not torch.cuda.is_available():
        raise SystemExit("fixed_window_ber: needs an MI355X")
    names = ["exact"] + [f"w{w}_g{g}" for w, g in WINDOWS]
    res = {"K": K, "iterations": ITERS, "steps_per_unit": STEPS, "fixed": {"le_max": 255, "ext_scale_q": 3},
           "frames": a.frames, "seed": a.seed, "gate": GATE, "points": []}
    with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as fx, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="f64") as gen:
        fx.reserve(a.batch)
        for ebn0 in a.points:
            gen.synth_seed(a.seed)
            bit = dict.fromkeys(names, 0)
            frm = dict.fromkeys(names, 0)
            done = 0
            while done < a.frames:
                n = min(a.batch, a.frames - done)
                info, llr = gen.synth(n, ebn0)
                x = decoder.quantise(llr, STEPS)
                for name, win in zip(names, ((0, 0),) + WINDOWS):
                    fx.set_fixed_window(*win)
                    wrong = (fx.decode(x) != info).sum(dim=1)
                    bit[name] += int(wrong.sum().item())
                    frm[name] += int((wrong > 0).sum().item())
                done += n
            pt = {"ebn0_db": ebn0, "frames": done, "bits": done * K}
            # the counts that tests/test_gpu_window.py asks of the exact decoder before it trusts a ratio
            pt["exact_counts_enough"] = bit["exact"] > 1000 and frm["exact"] > 50
            for name in names:
                pt[name] = {"bit_errors": bit[name], "frame_errors": frm[name], "ber": bit[name] / (done * K),
                            "fer": frm[name] / done}
                if name != "exact":
                    pt[name]["bits_over_exact"] = bit[name] / bit["exact"] if bit["exact"] else None
                    pt[name]["frames_over_exact"] = frm[name] / frm["exact"] if frm["exact"] else None
            res["points"].append(pt)
            print(json.dumps(pt), flush=True)

    def passes(name):
        return all(p[name]["bit_errors"] <= GATE * p["exact"]["bit_errors"]
                   and p[name]["frame_errors"] <= GATE * p["exact"]["frame_errors"] for p in res["points"])

    res["within_gate"] = {n: passes(n) for n in names[1:]}
    ok = [g for (w, g), n in zip(WINDOWS, names[1:]) if res["within_gate"][n]]
    res["default_overlap"] = 32 if 32 in ok else (min(ok) if ok else None)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
