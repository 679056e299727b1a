// fixed_maxstar_core_host.cpp -- the lane code of the fixed-point decoder with td_set_fixed_maxstar's table
// (csrc/td_fixed_core.h instantiated with fx::MaxStar, what a lane of the four *_maxstar kernels of
// td_fixed.hip runs) on the host, for tests/test_fixed_maxstar_host.py: a stand-alone program, built with
// AddressSanitizer + UndefinedBehaviorSanitizer (a signed overflow of an int32 metric is an error), that
// decodes a batch over a workspace of the kernel's layout and sizes with an odd pitch.  The file protocol
// is fixed_core_host.cpp's, extended by the schedule and the table; the launches are td_fixed.hip's.
//
//   fixed_maxstar_core_host IN OUT
//   IN   int32 K, iters, all_iters, le_max, ext_scale_q, B, window (0: the exact schedule), overlap,
//        rule (0: none), min_iters, crc_poly, table (0: the MaxLog instantiation), shift, corr[8];
//        int32 pi[K];  int8 q[B][3K+12]
//   OUT  uint8 bits[B][rows][K] (rows = all_iters ? iters : 1);  int16 le[B][iters][2][K+3], 0x5a5a where
//        nothing was written;  int32 used[B]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_crc.h"
#include "td_fixed_core.h"

using namespace td::fx;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

struct Ws {
    FxArgs p;
    FxStop s;
    FxWindow wn;
    int rule, nS;
    size_t Bp;
    uint32_t* ev;
    uint16_t* hist;
    int32_t* used;
};

// the launches of launch_fixed_turbo, _turbo_stop, _window and _window_stop, a lane at a time, the padding's too
template <class M>
static void run(const Ws& w, const M& m)
{
    const FxArgs& p = w.p;
    if (!w.wn.window) {
        for (size_t b = 0; b < w.Bp; ++b) {
            if (w.rule)
                decode_codeword_stop(p, w.s, b, m);
            else
                decode_codeword(p, b, m);
        }
        return;
    }
    if (w.rule)
        for (size_t b = 0; b < w.Bp; ++b) w.used[b] = 0;   // the decode's reset: every codeword runs
    for (int it = 0; it < p.iters; ++it) {
        for (int sb = w.nS - 1; sb >= 0; --sb)   // the sub-blocks of a launch run in no fixed order
            for (size_t b = 0; b < w.Bp; ++b) {
                if (w.rule)
                    siso_window_stop<0>(p, w.wn, w.s, w.ev, w.hist, b, it, sb, m);
                else
                    siso_window_pass<0>(p, w.wn, b, it, sb, m);
            }
        for (int sb = 0; sb < w.nS; ++sb)
            for (size_t b = 0; b < w.Bp; ++b) {
                if (w.rule)
                    siso_window_stop<1>(p, w.wn, w.s, w.ev, w.hist, b, it, sb, m);
                else
                    siso_window_pass<1>(p, w.wn, b, it, sb, m);
            }
        if (w.rule)
            for (size_t b = 0; b < w.Bp; ++b) window_judge(p, w.s, w.ev, w.nS, b, it);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t hdr[21];
    if (!f || !rd(f, hdr, 21)) return 2;
    const int K = hdr[0], iters = hdr[1], all_iters = hdr[2], le_max = hdr[3], scale = hdr[4], B = hdr[5];
    const FxWindow wn{hdr[6], hdr[7]};
    const int rule = hdr[8], min_iters = hdr[9];
    const uint32_t poly = (uint32_t)hdr[10];
    const int table = hdr[11];
    MaxStar ms{0, 0, hdr[12]};
    for (int j = 0; j < 4; ++j) {
        ms.lo |= (uint32_t)hdr[13 + j] << (8 * j);
        ms.hi |= (uint32_t)hdr[17 + j] << (8 * j);
    }
    const int L = K + 3, n = 3 * K + 12, rows = all_iters ? iters : 1, nW = (L + kW - 1) / kW;
    std::vector<int32_t> pi(K), pinv(K);
    std::vector<int8_t> q((size_t)B * n);
    if (!rd(f, pi.data(), pi.size()) || !rd(f, q.data(), q.size())) return 2;
    fclose(f);
    for (int i = 0; i < K; ++i) pinv[pi[i]] = i;

    const size_t Bp = (size_t)B + 1;   // an odd pitch: one lane of padding, as the kernel's last wave has
    std::vector<int8_t> xs((size_t)(L + 3) * Bp, 0), xp1((size_t)L * Bp, 0), xp2((size_t)L * Bp, 0);
    std::vector<int16_t> e12((size_t)K * Bp, 0x5a5a), e21((size_t)K * Bp, 0x5a5a);
    std::vector<int32_t> ck((size_t)nW * 8 * Bp, 0x5a5a5a5a);   // read before written: wrong bits, or a signed overflow under UBSan
    std::vector<uint8_t> bT((size_t)iters * K * Bp, 9);   // a row per iteration, whatever all_iters is (fx_carve)
    std::vector<int16_t> le((size_t)B * iters * 2 * L, 0x5a5a);
    std::vector<int32_t> used(Bp, -1);
    std::vector<uint32_t> ev((size_t)nW * Bp, 0xdeadbeefu);
    std::vector<uint16_t> hist((size_t)nW * Bp, 0xbeef);
    std::vector<int32_t> syn;   // exactly what the rule reads: nothing for HDA, syndrome[pi[i]] for CRC
    if (rule == 2) {
        std::vector<uint32_t> nat(K);
        td::crc24_syndromes(K, poly, nat.data());
        syn.resize(K);
        for (int i = 0; i < K; ++i) syn[i] = (int32_t)nat[pi[i]];
    }
    auto c = [](int8_t v) { return v == -128 ? (int8_t)-127 : v; };
    for (int b = 0; b < B; ++b) {   // the demultiplex of fx_demux_kernel
        const int8_t* s = &q[(size_t)b * n];
        for (int i = 0; i < K; ++i) {
            xs[(size_t)i * Bp + b] = c(s[3 * i]);
            xp1[(size_t)i * Bp + b] = c(s[3 * i + 1]);
            xp2[(size_t)i * Bp + b] = c(s[3 * i + 2]);
        }
        for (int j = 0; j < 3; ++j) {
            xs[(size_t)(K + j) * Bp + b] = c(s[3 * K + 2 * j]);
            xp1[(size_t)(K + j) * Bp + b] = c(s[3 * K + 2 * j + 1]);
            xs[(size_t)(L + j) * Bp + b] = c(s[3 * K + 6 + 2 * j]);
            xp2[(size_t)(K + j) * Bp + b] = c(s[3 * K + 6 + 2 * j + 1]);
        }
    }
    Ws w{};
    w.p = FxArgs{xs.data(), xp1.data(), xp2.data(), e12.data(), e21.data(), ck.data(), bT.data(), le.data(),
                 pi.data(), pinv.data(), K, L, B, iters, all_iters, le_max, scale, Bp};
    const int floor_n = rule == 1 ? 2 : 1;
    w.s = FxStop{rule, min_iters > floor_n ? min_iters : floor_n, syn.data(), used.data()};
    w.wn = wn;
    w.rule = rule;
    w.nS = wn.window ? window_blocks(L, wn.window) : 1;
    w.Bp = Bp;
    w.ev = ev.data();
    w.hist = hist.data();
    w.used = used.data();
    if (w.nS > nW) return 3;
    if (table)
        run(w, ms);
    else
        run(w, MaxLog());

    // a lane of the padding stores nothing into the rows; with a rule it never runs
    if (rule) {
        if (used[B] != (wn.window ? 0 : iters)) return 3;
        for (size_t i = 0; i < (size_t)iters * K; ++i)
            if (bT[i * Bp + B] != 9) return 3;
    }
    std::vector<uint8_t> bits((size_t)B * rows * K);
    for (int b = 0; b < B; ++b) {
        if (!rule) used[b] = iters;
        if (used[b] < 1 || used[b] > iters) return 3;
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k) {
                if (rule) {   // fx_bits_stop_kernel: the frozen rows, kept by interleaved position
                    const int src = rows == 1 ? used[b] - 1 : r < used[b] - 1 ? r : used[b] - 1;
                    bits[((size_t)b * rows + r) * K + k] = bT[((size_t)src * K + pinv[k]) * Bp + b];
                } else {      // fx_bits_kernel
                    bits[((size_t)b * rows + r) * K + k] = bT[((size_t)r * K + k) * Bp + b];
                }
            }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(bits.data(), 1, bits.size(), o);
    fwrite(le.data(), sizeof(int16_t), le.size(), o);
    fwrite(used.data(), sizeof(int32_t), (size_t)B, o);
    fclose(o);
    return 0;
}
