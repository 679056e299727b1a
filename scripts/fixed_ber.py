"""BER of the fixed-point decoder against the fp64 decoders on the same frames: K = 6144, 8
iterations, the device generator's frames (td_synth_frames, srand(seed)) at 0.3 .. 0.8 dB.

  fixed        precision "fixed", inputs quantised at 8 steps per unit LLR, {le_max 255, ext_scale_q 3}
  f64_maxlog   fp64 Max-Log-MAP, exact schedule, unquantised inputs
  f64_logmap   fp64 log-MAP (the reference decoder), unquantised inputs

Per point: bit and frame errors after the last iteration over `frames` frames, and from the curves
the Eb/N0 at which each decoder reaches BER 1e-4 (linear interpolation of log10 BER between the two
points that bracket it) with the fixed decoder's shift against the other two.  Needs an MI355X.

    python scripts/fixed_ber.py [--frames 32768] [--batch 4096] [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TD_PLACEMENT_TRIALS", "1")   # results do not depend on the workspace's placement

K, F1, F2, ITERS, STEPS = 6144, 263, 480, 8, 8
POINTS = (0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
TARGET = 1e-4


def crossing(points, bers):
    """Eb/N0 where log10(BER) crosses log10(TARGET), or None when the curve does not bracket it."""
    for (x0, y0), (x1, y1) in zip(zip(points, bers), zip(points[1:], bers[1:])):
        if y0 >= TARGET > y1 and y1 > 0:
            l0, l1, lt = math.log10(y0), math.log10(y1), math.log10(TARGET)
            return x0 + (x1 - x0) * (l0 - lt) / (l0 - l1)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder
    if not torch.cuda.is_available():
        raise SystemExit("fixed_ber: needs an MI355X")
    names = ("fixed", "f64_maxlog", "f64_logmap")
    res = {"K": K, "iterations": ITERS, "steps_per_unit": STEPS, "fixed": {"le_max": 255, "ext_scale_q": 3},
           "frames": a.frames, "seed": a.seed, "points": []}
    with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as fx, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="f64") as ml, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="logmap", precision="f64") as lm:
        codecs = dict(zip(names, (fx, ml, lm)))
        for c in codecs.values():
            c.reserve(a.batch)
        for ebn0 in POINTS:
            ml.synth_seed(a.seed)
            bit = dict.fromkeys(names, 0)
            frm = dict.fromkeys(names, 0)
            done = 0
            while done < a.frames:
                n = min(a.batch, a.frames - done)
                info, llr = ml.synth(n, ebn0)
                inputs = {"fixed": decoder.quantise(llr, STEPS), "f64_maxlog": llr, "f64_logmap": llr}
                for name, c in codecs.items():
                    wrong = (c.decode(inputs[name]) != info).sum(dim=1)
                    bit[name] += int(wrong.sum().item())
                    frm[name] += int((wrong > 0).sum().item())
                done += n
            pt = {"ebn0_db": ebn0, "frames": done, "bits": done * K}
            for name in names:
                pt[name] = {"bit_errors": bit[name], "frame_errors": frm[name], "ber": bit[name] / (done * K),
                            "fer": frm[name] / done}
            res["points"].append(pt)
            print(json.dumps(pt), flush=True)
    cross = {n: crossing(POINTS, [p[n]["ber"] for p in res["points"]]) for n in names}
    res["ebn0_at_ber_1e-4"] = cross
    res["fixed_shift_db"] = {n: (cross["fixed"] - cross[n]) if cross["fixed"] is not None and cross[n] is not None else None
                             for n in names[1:]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
