"""Speed of the transport-block receive front end and of scrambling at A = 75376, N = 256 (13 blocks of
K = 5824) and A = 6121, N = 4096 (one block of 3072 and one of 3136, F = 15), QPSK and 64QAM (NlQm = the
modulation), float32 and int8, G about 2 sum K_r, in one process:

  fused          td_tb_demod_dematch with a sequence: reads 16 N G / M symbol bytes and N G / 8 sequence bytes,
                 writes N sum (3 K_r + 12) values
  separate       td_demodulate -> td_descramble_llr (in place) -> td_llr_convert -> td_tb_rate_dematch on the
                 whole [N][G] array: the same result (checked), with the double array in between
  fused_copy     torch's device-to-device copy of the fused call's bytes (half read, half written)
  gold_sequence  td_gold_sequence of N rows of G bits (writes N ceil(G / 32) words), and a copy of twice that
  scramble       td_scramble of [N][G] bytes (reads and writes N G, reads N G / 8), and its copy

Times are hipEvents round `reps` back-to-back calls per sample, the median of `samples`.  Needs an MI355X.

    python scripts/tb_frontend_bw.py [--reps 50] [--samples 7] [--out profiles/tb/tb_frontend_bw.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from encode_bw import copy_of, measure   # noqa: E402  the project's timing of a call and of its yardstick copy

CASES = ((75376, 256), (6121, 4096))
MODS = (2, 6)
PRECISIONS = ("f32", "fixed")
KF, STEPS = 0.83, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tb", "tb_frontend_bw.json"))
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TransportBlock, convert_llr, demodulate, descramble, gold_sequence, scramble
    if not torch.cuda.is_available():
        raise SystemExit("tb_frontend_bw: needs an MI355X")
    dev = torch.device("cuda", 0)
    res = {"reps": a.reps, "samples": a.samples, "Kf": KF, "steps_per_unit": STEPS, "cases": []}

    for A, n in CASES:
        with TransportBlock(A) as t:
            p = t.plan
            sizes = [p.K_minus] * p.C_minus + [p.K_plus] * p.C_plus
            sumK, sumS = sum(sizes), sum(3 * K + 12 for K in sizes)
            for M in MODS:
                G = M * (2 * sumK // (M * p.C) * p.C)   # NlQm = M, G' a multiple of C
                W = (G + 31) // 32
                cinit = torch.randint(0, 1 << 31, (n,), dtype=torch.int64, device=dev).to(torch.int32)
                seq = gold_sequence(cinit, G)
                case = {"A": A, "N": n, "plan": p._asdict(), "modulation": M, "NlQm": M, "G": G}
                case["gold_sequence"] = measure(lambda: gold_sequence(cinit, G, out=seq), 4 * n * W, a.reps, a.samples)
                case["gold_sequence_copy"] = copy_of(8 * n * W, a.reps, a.samples, dev)
                bits = torch.randint(0, 2, (n, G), dtype=torch.uint8, device=dev)
                sbits = torch.empty_like(bits)
                nb = 2 * n * G + 4 * n * W
                case["scramble"] = measure(lambda: scramble(bits, seq, out=sbits), nb, a.reps, a.samples)
                case["scramble_copy"] = copy_of(nb // 2 * 2, a.reps, a.samples, dev)
                case["scramble_over_copy"] = case["scramble"]["ms"] / case["scramble_copy"]["ms"]
                del bits, sbits
                yi = 1.2 * torch.randn((n, G // M), dtype=torch.float64, device=dev)
                yq = 1.2 * torch.randn((n, G // M), dtype=torch.float64, device=dev)
                for precision in PRECISIONS:
                    es = 4 if precision == "f32" else 1
                    nb = 16 * n * (G // M) + 4 * n * W + es * n * sumS
                    out = t.demod_dematch(yi, yq, 0, M, M, KF, precision, STEPS, seq=seq)
                    fused = lambda: t.demod_dematch(yi, yq, 0, M, M, KF, precision, STEPS, seq=seq, out=out)
                    f = torch.empty((n, G), dtype=out[1].dtype, device=dev)
                    out2 = tuple(None if o is None else torch.empty_like(o) for o in out)

                    def separate():
                        llr = demodulate(yi.view(-1), yq.view(-1), M, KF).view(n, G)
                        descramble(llr, seq, out=llr)
                        convert_llr(llr, precision, STEPS, out=f)
                        t.rate_dematch(f, 0, M, out=out2)
                    r = {"precision": precision,
                         "fused": measure(fused, nb, a.reps, a.samples),
                         "separate": measure(separate, nb, a.reps, a.samples),
                         "fused_copy": copy_of(nb // 2 * 2, a.reps, a.samples, dev)}
                    r["equal"] = all(o is None or torch.equal(o, o2) for o, o2 in zip(out, out2))
                    r["separate_over_fused"] = r["separate"]["ms"] / r["fused"]["ms"]
                    r["fused_over_copy"] = r["fused"]["ms"] / r["fused_copy"]["ms"]
                    case[precision] = r
                    del out, out2, f
                    torch.cuda.empty_cache()
                res["cases"].append(case)
                del yi, yq, seq
                torch.cuda.empty_cache()

    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
