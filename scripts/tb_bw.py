"""Speed of the four transport-block calls (td_tb_segment, td_tb_rate_match, td_tb_rate_dematch, td_tb_concat)
at A = 75376, N = 256 (13 blocks of K = 5824, no filler) and A = 6121, N = 4096 (one block of 3072 and one of
3136, F = 15), each next to a device-to-device copy of the bytes it reads plus writes, in one process:

  segment        reads N A, writes N sum K_r
  rate_match     NlQm = 2, G about 2 sum K_r: reads the N G selected bytes, writes N G
  rate_dematch   float32, the same G: reads 4 N G, writes 4 N sum (3 K_r + 12)
  concat         with both remainders: reads N sum K_r, writes N A + 4 N (C + 1)
  *_copy         torch's copy of that many bytes (half read, half written), timed the same way
  *_torch        where F = 0 and one block size make it possible (A = 75376): the same result from the
                 single-block calls and torch slicing --
                 segment: the [N, B] sequence WITH its gCRC24A already attached (td_crc_attach takes K <= 10000,
                 so the composition cannot compute it and does less work than td_tb_segment) sliced block-major
                 into [C, N, K] and td_crc_attach (gCRC24B) on the C N rows;
                 rate_match: td_rate_match on the C N rows with one E (G' a multiple of C) and a permuting copy
                 into [N, G]

Times are hipEvents round `reps` back-to-back calls per sample, the median of `samples`.  Needs an MI355X.

    python scripts/tb_bw.py [--reps 50] [--samples 7] [--out profiles/tb/tb_bw.json]
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
QPP = {5824: (89, 182)}   # the LTE pair of the composition's one block size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tb", "tb_bw.json"))
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TransportBlock, TurboCodec, _native as N
    if not torch.cuda.is_available():
        raise SystemExit("tb_bw: needs an MI355X")
    dev = torch.device("cuda", 0)
    res = {"reps": a.reps, "samples": a.samples, "cases": []}

    def both(case, name, fn, nbytes):
        case[name] = measure(fn, nbytes, a.reps, a.samples)
        case[name + "_copy"] = copy_of(nbytes // 2 * 2, a.reps, a.samples, dev)
        case[name + "_over_copy"] = case[name]["ms"] / case[name + "_copy"]["ms"]

    for A, n in CASES:
        with TransportBlock(A) as t:
            p = t.plan
            sizes = [p.K_minus] * p.C_minus + [p.K_plus] * p.C_plus
            sumK, sumS = sum(sizes), sum(3 * K + 12 for K in sizes)
            G = 2 * (2 * sumK // (2 * p.C) * p.C)   # NlQm = 2, G' a multiple of C: one E, as the composition needs
            case = {"A": A, "N": n, "plan": p._asdict(), "G": G, "NlQm": 2}
            rnd = lambda shape: None if shape is None else torch.randint(0, 2, shape, dtype=torch.uint8, device=dev)
            tb = rnd((n, A))
            cb = t.segment(tb)
            both(case, "segment", lambda: t.segment(tb, out=cb), n * (A + sumK))
            coded = tuple(rnd(s) for s in t.block_shapes(n, lambda K: 3 * K + 12))
            f = t.rate_match(coded, 0, G, 2)
            both(case, "rate_match", lambda: t.rate_match(coded, 0, G, 2, out=f), 2 * n * G)
            soft_in = torch.randn((n, G), dtype=torch.float32, device=dev)
            soft = t.rate_dematch(soft_in, 0, 2)
            both(case, "rate_dematch", lambda: t.rate_dematch(soft_in, 0, 2, out=soft), 4 * n * (G + sumS))
            out = t.concat(cb)
            both(case, "concat", lambda: t.concat(cb, out=out[0], cb_rem=out[1], tb_rem=out[2]),
                 n * (sumK + A + 4 * (p.C + 1)))
            case["round_trip_ok"] = bool(torch.equal(out[0], tb)) and not out[1].any().item() and not out[2].any().item()

            if p.F == 0 and p.C_minus == 0 and p.K_plus in QPP:
                K, C_, P = p.K_plus, p.C, p.K_plus - p.L
                with TurboCodec(K, *QPP[K], iterations=1) as c:
                    c.set_crc(N.CRC24B)
                    c.set_rate_matching(0)
                    # the B-bit sequence as td_tb_segment forms it: read back from its blocks
                    b = cb[1][:, :, :P].permute(1, 0, 2).reshape(n, p.B).contiguous()
                    mine = cb[1].clone()
                    theirs = torch.empty_like(mine)

                    def segment_torch():
                        theirs[:, :, :P].copy_(b.view(n, C_, P).permute(1, 0, 2))
                        c.crc_attach(theirs.view(C_ * n, K))
                    case["segment_torch"] = measure(segment_torch, n * (p.B + sumK), a.reps, a.samples)
                    case["segment_torch_equal"] = bool(torch.equal(theirs, mine))
                    case["segment_over_torch"] = case["segment"]["ms"] / case["segment_torch"]["ms"]
                    E = G // C_
                    e = torch.empty((C_ * n, E), dtype=torch.uint8, device=dev)
                    f2 = torch.empty_like(f)

                    def rate_match_torch():
                        c.rate_match(coded[1].view(C_ * n, 3 * K + 12), 0, E, out=e)
                        f2.view(n, C_, E).copy_(e.view(C_, n, E).permute(1, 0, 2))
                    case["rate_match_torch"] = measure(rate_match_torch, 4 * n * G, a.reps, a.samples)
                    case["rate_match_torch_equal"] = bool(torch.equal(f2, f))
                    case["rate_match_over_torch"] = case["rate_match"]["ms"] / case["rate_match_torch"]["ms"]
            res["cases"].append(case)
            del tb, cb, coded, f, soft_in, soft, out
            torch.cuda.empty_cache()

    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
