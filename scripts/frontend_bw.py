"""Speed of the fused receive front end (td_demod_dematch) at K = 6144, Ncb = Kw, rv 0, for E = 3K+12 and
E = 2K, QPSK and 64QAM, B = 4096 and 32768, each precision, against three baselines timed in the same run:

  fused        td_demod_dematch: symbols in, soft buffer out, one launch
  three_calls  td_demodulate -> td_llr_convert -> td_rate_dematch through the C ABI on buffers allocated
               beforehand (a B*E double array and a B*E array of the precision in between)
  python       the path Python had before: demodulate(), then torch (quantise's three calls for int8, .to(float32)
               for fp32, nothing for fp64), then rate_dematch
  copy         a device-to-device copy that moves the bytes the fused call must move: B*E/M symbols of 16 bytes
               in, B*(3K+12) soft values out

hipEvents round `reps` back-to-back calls per sample, after a warm-up of the same calls; the median of `samples`
samples.  GB/s counts the bytes the fused call must move (the rank table is 74 KB and stays in cache), whatever
the method moves.  The outputs of fused and three_calls are compared at every shape ("equal").  The shader clock
noted is the sustained clock of a decode on the same device in the same process (td_clock_read).  Needs an
MI355X: there is no CPU path.

    python scripts/frontend_bw.py [--B 4096 32768] [--precisions f64 f32 fixed] [--reps 20] [--samples 7]
                                  [--label TEXT] [--out FILE.json]

A library built with other flags (TD_LIB_PATH) is timed by the same command; --label names it in the result.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("TD_PLACEMENT_TRIALS", "1")

K, F1, F2 = 6144, 263, 480
KF, STEPS = 0.83, 8.0


def timed(fn, reps, samples):
    """Median ms of one call of fn, over `samples` event-bracketed runs of `reps` calls."""
    import torch
    ms = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--precisions", nargs="+", default=["f64", "f32", "fixed"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from turbo_decoder_cuda_amd import TurboCodec, _native as N, demodulate, quantise
    if not torch.cuda.is_available():
        raise SystemExit("frontend_bw: needs an MI355X")
    dev = torch.device("cuda", 0)
    L = N.lib()
    n = 3 * K + 12
    ptr = lambda t: C.c_void_p(t.data_ptr())
    res = {"K": K, "Kf": KF, "steps_per_unit": STEPS, "reps": a.reps, "samples": a.samples, "label": a.label,
           "library": os.path.basename(N.LIB_PATH), "cases": []}
    with TurboCodec(K, F1, F2, iterations=1) as c:   # the box's clock: a decode's sustained shader clock
        x = torch.randn((256, n), dtype=torch.float64, device=dev)
        c.decode(x)
        c.decode(x)
        ghz, span = c.clock()
        res["sclk_ghz"], res["sclk_span_ms"] = ghz, span
    tdt = {"f64": torch.float64, "f32": torch.float32, "fixed": torch.int8}
    pcode = {"f64": N.TD_F64, "f32": N.TD_F32, "fixed": N.TD_FIXED}
    for precision in a.precisions:
        algo = "maxlog" if precision == "fixed" else "logmap"
        with TurboCodec(K, F1, F2, iterations=1, algo=algo, precision=precision) as c:
            c.set_rate_matching(0)
            for B in a.B:
                for E in (n, 2 * K):
                    for M in (2, 6):
                        nsym = B * E // M
                        g = torch.Generator(device=dev).manual_seed(B + E + M)
                        yi = torch.randn((B, E // M), dtype=torch.float64, device=dev, generator=g) * 1.2
                        yq = torch.randn((B, E // M), dtype=torch.float64, device=dev, generator=g) * 1.2
                        llr = torch.empty((B, E), dtype=torch.float64, device=dev)
                        e = torch.empty((B, E), dtype=tdt[precision], device=dev)
                        out = torch.empty((B, n), dtype=tdt[precision], device=dev)
                        out3 = torch.empty_like(out)
                        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                        nbytes = nsym * 16 + B * n * out.element_size()
                        src = torch.empty((nbytes // 2,), dtype=torch.uint8, device=dev).random_()
                        dst = torch.empty_like(src)

                        def fused():
                            N.check(L.td_demod_dematch(c._h, ptr(yi), ptr(yq), B, 0, E, M, KF, STEPS, ptr(out), 0, st))

                        def three_calls():
                            N.check(L.td_demodulate(ptr(yi), ptr(yq), nsym, M, KF, ptr(llr), st))
                            N.check(L.td_llr_convert(ptr(llr), B * E, pcode[precision], STEPS, ptr(e), st))
                            N.check(L.td_rate_dematch(c._h, ptr(e), B, 0, E, ptr(out3), 0, st))

                        def python():
                            v = demodulate(yi, yq, M, KF).view(B, E)
                            v = quantise(v, STEPS) if precision == "fixed" else v.to(tdt[precision])
                            c.rate_dematch(v, 0, out=out3)

                        case = {"precision": precision, "B": B, "E": E, "M": M, "bytes": nbytes,
                                "separate_bytes": nsym * 16 + 2 * B * E * 8 + 2 * B * E * out.element_size()
                                                  + B * n * out.element_size()}
                        for name, fn in (("fused", fused), ("three_calls", three_calls), ("python", python),
                                         ("copy", lambda: dst.copy_(src))):
                            timed(fn, 3, 1)   # warm-up
                            med, lo, hi = timed(fn, a.reps, a.samples)
                            case[name] = {"ms": med, "min_ms": lo, "max_ms": hi, "GBps": nbytes / med / 1e6}
                        fused()
                        three_calls()
                        torch.cuda.synchronize()
                        case["equal"] = bool(torch.equal(out.view(torch.uint8), out3.view(torch.uint8)))
                        case["three_calls_over_fused"] = case["three_calls"]["ms"] / case["fused"]["ms"]
                        case["python_over_fused"] = case["python"]["ms"] / case["fused"]["ms"]
                        case["fused_over_copy"] = case["fused"]["ms"] / case["copy"]["ms"]
                        res["cases"].append(case)
                        print(json.dumps(case), flush=True)
                        del yi, yq, llr, e, out, out3, src, dst
                        torch.cuda.empty_cache()
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
