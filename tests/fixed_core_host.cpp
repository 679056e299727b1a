// fixed_core_host.cpp -- the fixed-point decoder's lane code (csrc/td_fixed_core.h, what a lane of
// td_fixed.hip's fx_turbo_kernel and fx_window_siso_kernel runs, in every instantiation) on the host, for the
// tests/test_fixed_*_host.py files through tests/fixed_host.py: a stand-alone program, built with
// AddressSanitizer + UndefinedBehaviorSanitizer (a signed overflow of an int32 metric is an error), that
// decodes a batch a lane at a time over the workspace of fixed_host_common.h.  The launches are
// launch_fixed_decode's.  On the sub-block schedule that is one "launch" per SISO and iteration with the
// launcher's own arguments (nii_args): every sub-block of every lane, SISO1's from the last sub-block to the
// first and SISO2's from the first to the last (the sub-blocks of a launch run in no fixed order) -- so with
// NII a consumer runs before its producer in one SISO and after it in the other, and a state that is not
// double-buffered by the iteration's parity gives other bytes -- then the judge.  The NII state starts as a
// pattern that no store writes: a slot that is loaded without having been stored shows in the result.
//
//   fixed_core_host IN OUT
//   IN   int32 K, iters, all_iters, le_max, ext_scale_q, B, window (0: the exact schedule), overlap,
//        rule (0: none), min_iters, crc_poly, table (0: the MaxLog instantiation), shift, corr[8], nii (0 / 1);
//        int32 pi[K];  int8 q[B][3K+12]
//   OUT  uint8 bits[B][rows][K] (rows = all_iters ? iters : 1);  int16 le[B][iters][2][K+3], 0x5a5a where
//        nothing was written;  int32 used[B] (without a rule: iters)
#include <type_traits>

#include "fixed_host_common.h"

using namespace fxhost;

struct Run {
    FxArgs p;
    FxStop s;
    FxWindow wn;
    bool stop;
    Workspace* w;
    uint32_t* nii;   // null: NII off
};

template <class M>
static void decode(const Run& r, const M& m)
{
    const FxArgs& p = r.p;
    if (!r.wn.window) {
        for (size_t b = 0; b < p.Bp; ++b) {   // the padding's lane too: it stores nothing outside (a rule: only its count)
            if (r.stop)
                decode_codeword_stop(p, r.s, b, m);
            else
                decode_codeword(p, b, m);
        }
        return;
    }
    const int nS = window_blocks(p.L, r.wn.window);
    if (r.stop)
        for (size_t b = 0; b < p.Bp; ++b) r.w->used[b] = 0;   // the decode's reset: every codeword runs
    uint32_t* ev = r.w->ev.data();
    uint16_t* hist = r.w->hist.data();
    // one lane of SISO `DEC`, by the setting's own entry (a rule and NII together run on the GPU alone)
    auto lane = [&](auto DEC, const FxNii& n, size_t b, int it, int sb) {
        constexpr int D = decltype(DEC)::value;
        if (r.stop)
            siso_window_stop<D>(p, r.wn, r.s, ev, hist, b, it, sb, m);
        else if (r.nii)
            siso_window_pass_nii<D>(p, r.wn, n, b, it, sb, m);
        else
            siso_window_pass<D>(p, r.wn, b, it, sb, m);
    };
    for (int it = 0; it < p.iters; ++it) {
        const FxNii n0 = r.nii ? nii_args(r.nii, p.L, r.wn, p.Bp, it, 0) : FxNii{};
        const FxNii n1 = r.nii ? nii_args(r.nii, p.L, r.wn, p.Bp, it, 1) : FxNii{};
        for (int sb = nS - 1; sb >= 0; --sb)
            for (size_t b = 0; b < p.Bp; ++b) lane(std::integral_constant<int, 0>(), n0, b, it, sb);   // the padding's lane too
        for (int sb = 0; sb < nS; ++sb)
            for (size_t b = 0; b < p.Bp; ++b) lane(std::integral_constant<int, 1>(), n1, b, it, sb);
        if (r.stop)
            for (size_t b = 0; b < p.Bp; ++b) window_judge(p, r.s, ev, nS, b, it);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    int32_t hdr[22];
    std::vector<int32_t> pi;
    std::vector<int8_t> q;
    if (!read_input(argv[1], hdr, 22, pi, q)) return 2;
    const int K = hdr[0], iters = hdr[1], all_iters = hdr[2], le_max = hdr[3], scale = hdr[4], B = hdr[5];
    const FxWindow wn{hdr[6], hdr[7]};
    const int rule = hdr[8], min_iters = hdr[9];
    const uint32_t poly = (uint32_t)hdr[10];
    MaxStar ms{0, 0, hdr[12]};
    for (int j = 0; j < 4; ++j) {
        ms.lo |= (uint32_t)hdr[13 + j] << (8 * j);
        ms.hi |= (uint32_t)hdr[17 + j] << (8 * j);
    }

    Workspace w(K, iters, all_iters, B, pi, q, rule != 0);
    if (wn.window && window_blocks(w.L, wn.window) > w.nW) return 3;
    if (rule && hdr[21]) return 2;   // no host entry runs a rule with NII
    std::vector<uint32_t> nii;   // two int16 of 23130: above every stored value
    if (hdr[21]) nii.assign(nii_words(w.L, wn.window, w.Bp), 0x5a5a5a5au);
    const Run r{w.args(all_iters, le_max, scale), rule ? w.stop(rule, min_iters, poly) : FxStop{}, wn, rule != 0, &w,
                hdr[21] ? nii.data() : nullptr};
    if (hdr[11])
        decode(r, ms);
    else
        decode(r, MaxLog());

    // With a rule a lane of the padding never runs: it stores nothing into the rows, the exact schedule writes
    // its count, and on the sub-block schedule the judge leaves it alone.
    if (rule) {
        if (w.used[B] != (wn.window ? 0 : iters)) return 3;
        for (size_t i = 0; i < (size_t)iters * K; ++i)
            if (w.bT[i * w.Bp + B] != 9) return 3;
        for (size_t i = 0; wn.window && i < (size_t)w.nW; ++i)
            if (w.ev[i * w.Bp + B] != 0xdeadbeefu || w.hist[i * w.Bp + B] != 0xbeef) return 3;
    } else {
        for (int b = 0; b < B; ++b) w.used[b] = iters;
    }
    const std::vector<uint8_t> out = rule ? w.bits_stop() : w.bits();
    if (out.empty()) return 3;
    return w.write(argv[2], out) ? 0 : 2;
}
