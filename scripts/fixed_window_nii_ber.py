"""BER of the fixed-point decoder's sub-block schedule with next-iteration initialisation
(td_set_fixed_window_nii) against the exact fixed schedule on the same frames: scripts/fixed_window_ber.py's
protocol (K = 6144, 8 iterations, the device generator's frames quantised at 8 steps per unit LLR,
{le_max 255, ext_scale_q 3}), gate and points.

Per point: bit and frame errors after the last iteration of the exact fixed decode, of {64, 0}, {64, 16} and
{64, 32} with NII and of {64, 16} and {64, 48} without, and each one's ratio to the exact schedule's counts.
`nii_overlap` is the smallest NII overlap whose bit and frame errors stay within GATE x the exact
schedule's at every point, or null.  Needs an MI355X.

    python scripts/fixed_window_nii_ber.py [--frames 32768] [--batch 4096] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("TD_PLACEMENT_TRIALS", "1")   # results do not depend on the workspace's placement

from fixed_window_ber import F1, F2, GATE, ITERS, K, POINTS, STEPS   # noqa: E402

# name, (window, overlap), nii
SETTINGS = (("exact", (0, 0), False), ("w64_g0_nii", (64, 0), True), ("w64_g16_nii", (64, 16), True),
            ("w64_g32_nii", (64, 32), True), ("w64_g16", (64, 16), False), ("w64_g48", (64, 48), False))


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
        raise SystemExit("fixed_window_nii_ber: needs an MI355X")
    names = [s[0] for s in SETTINGS]
    res = {"K": K, "iterations": ITERS, "steps_per_unit": STEPS, "fixed": {"le_max": 255, "ext_scale_q": 3},
           "frames": a.frames, "seed": a.seed, "gate": GATE, "points": []}
    with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as fx, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="f64") as gen:
        fx.set_fixed_window(64, 16, nii=True)
        fx.reserve(a.batch)   # with the NII state: no decode below grows the workspace
        for ebn0 in a.points:
            gen.synth_seed(a.seed)
            bit = dict.fromkeys(names, 0)
            frm = dict.fromkeys(names, 0)
            done = 0
            while done < a.frames:
                n = min(a.batch, a.frames - done)
                info, llr = gen.synth(n, ebn0)
                x = decoder.quantise(llr, STEPS)
                for name, win, nii in SETTINGS:
                    fx.set_fixed_window(*win, nii=nii)
                    wrong = (fx.decode(x) != info).sum(dim=1)
                    bit[name] += int(wrong.sum().item())
                    frm[name] += int((wrong > 0).sum().item())
                done += n
            pt = {"ebn0_db": ebn0, "frames": done, "bits": done * K}
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
    ok = [win[1] for name, win, nii in SETTINGS if nii and res["within_gate"][name]]
    res["nii_overlap"] = min(ok) if ok else None
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
