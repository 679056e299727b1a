"""BER of the fixed-point decoder with td_set_fixed_maxstar's table against itself without it and against the
fp64 log-MAP decoder, on the same frames: K = 6144, 8 iterations, the device generator's frames
(td_synth_frames, srand(seed)) at 0.3 .. 0.6 dB, the fixed decoders' inputs quantised at 8 steps per unit LLR.

  fixed_maxlog       the table off, {le_max 255, ext_scale_q 3}: the fixed decoder as it always was
  fixed_logmap_q4    the default table at 8 steps per unit, {255, 4}
  fixed_logmap_q3    the same table, {255, 3}
  f64_logmap         fp64 log-MAP (the reference decoder), unquantised inputs

Per point: bit and frame errors after the last iteration over `frames` frames; from the curves the Eb/N0 at
which each decoder reaches BER 1e-4 (scripts/fixed_ber.py's interpolation) and every fixed decoder's distance
from fp64 log-MAP.  The condition: fixed_logmap_q4 has fewer bit errors than fixed_maxlog at 0.4 and at
0.5 dB; the result is recorded, and the script exits 1 if it does not hold.  Needs an MI355X.

    python scripts/fixed_maxstar_ber.py [--frames 32768] [--batch 4096] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("TD_PLACEMENT_TRIALS", "1")   # results do not depend on the workspace's placement

from fixed_ber import F1, F2, ITERS, K, STEPS, crossing   # noqa: E402

POINTS = (0.3, 0.4, 0.5, 0.6)
NAMES = ("fixed_maxlog", "fixed_logmap_q4", "fixed_logmap_q3", "f64_logmap")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, decoder, fixed_maxstar_table
    if not torch.cuda.is_available():
        raise SystemExit("fixed_maxstar_ber: needs an MI355X")
    shift, corr = fixed_maxstar_table(STEPS)
    res = {"K": K, "iterations": ITERS, "steps_per_unit": STEPS, "table": {"shift": shift, "corr": list(corr)},
           "settings": {"fixed_maxlog": [255, 3], "fixed_logmap_q4": [255, 4], "fixed_logmap_q3": [255, 3]},
           "frames": a.frames, "seed": a.seed, "points": []}
    with TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as ml, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as q4, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="maxlog", precision="fixed") as q3, \
            TurboCodec(K, F1, F2, iterations=ITERS, algo="logmap", precision="f64") as lm:
        q4.set_fixed(255, 4)
        q4.set_fixed_maxstar(float(STEPS))
        q3.set_fixed_maxstar(float(STEPS))
        codecs = dict(zip(NAMES, (ml, q4, q3, lm)))
        for c in codecs.values():
            c.reserve(a.batch)
        for ebn0 in POINTS:
            lm.synth_seed(a.seed)
            bit = dict.fromkeys(NAMES, 0)
            frm = dict.fromkeys(NAMES, 0)
            done = 0
            while done < a.frames:
                n = min(a.batch, a.frames - done)
                info, llr = lm.synth(n, ebn0)
                q = decoder.quantise(llr, STEPS)
                for name, c in codecs.items():
                    wrong = (c.decode(llr if name == "f64_logmap" else q) != info).sum(dim=1)
                    bit[name] += int(wrong.sum().item())
                    frm[name] += int((wrong > 0).sum().item())
                done += n
            pt = {"ebn0_db": ebn0, "frames": done, "bits": done * K}
            for name in NAMES:
                pt[name] = {"bit_errors": bit[name], "frame_errors": frm[name], "ber": bit[name] / (done * K),
                            "fer": frm[name] / done}
            res["points"].append(pt)
            print(json.dumps(pt), flush=True)
    cross = {n: crossing(POINTS, [p[n]["ber"] for p in res["points"]]) for n in NAMES}
    res["ebn0_at_ber_1e-4"] = cross
    res["distance_from_f64_logmap_db"] = {n: (cross[n] - cross["f64_logmap"]) if None not in (cross[n], cross["f64_logmap"])
                                          else None for n in NAMES[:3]}
    by = {p["ebn0_db"]: p for p in res["points"]}
    cond = {str(e): {"fixed_logmap_q4": by[e]["fixed_logmap_q4"]["bit_errors"], "fixed_maxlog": by[e]["fixed_maxlog"]["bit_errors"],
                     "fewer": by[e]["fixed_logmap_q4"]["bit_errors"] < by[e]["fixed_maxlog"]["bit_errors"]} for e in (0.4, 0.5)}
    res["condition_fewer_bit_errors_than_maxlog"] = cond
    res["condition_holds"] = all(v["fewer"] for v in cond.values())
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["condition_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
