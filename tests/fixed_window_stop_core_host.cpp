// fixed_window_stop_core_host.cpp -- the stopping lane code of the fixed-point decoder's sub-block schedule
// (csrc/td_fixed_core.h siso_window_stop and window_judge, what a lane of fx_window_siso_stop_kernel and a
// thread of fx_window_judge_kernel run) on the host, for tests/test_fixed_window_stop_host.py: a stand-alone
// program, built with AddressSanitizer + UndefinedBehaviorSanitizer, that decodes a batch over a workspace
// of the kernel's layout and sizes with an odd pitch.  The launches are td_fixed.hip's
// launch_fixed_window_stop's: the counts reset to 0, then per iteration SISO1 -- every sub-block of every
// lane, from the last sub-block to the first --, SISO2 from the first to the last (the sub-blocks of a launch
// run in no fixed order) and the judge; the rows are read back as fx_bits_stop_kernel does.
//
//   fixed_window_stop_core_host IN OUT
//   IN   int32 K, iters, all_iters, le_max, ext_scale_q, B, window, overlap, rule, min_iters, crc_poly;
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

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t hdr[11];
    if (!f || !rd(f, hdr, 11)) return 2;
    const int K = hdr[0], iters = hdr[1], all_iters = hdr[2], le_max = hdr[3], scale = hdr[4], B = hdr[5];
    const FxWindow wn{hdr[6], hdr[7]};
    const int rule = hdr[8], min_iters = hdr[9];
    const uint32_t poly = (uint32_t)hdr[10];
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
    std::vector<uint32_t> ev((size_t)nW * Bp, 0xdeadbeefu);   // fx_carve's: nW words a codeword
    std::vector<uint16_t> hist((size_t)nW * Bp, 0xbeef);      // and nW packed windows (HDA)
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
    FxArgs p{xs.data(), xp1.data(), xp2.data(), e12.data(), e21.data(), ck.data(), bT.data(), le.data(),
             pi.data(), pinv.data(), K, L, B, iters, all_iters, le_max, scale, Bp};
    const int floor_n = rule == 1 ? 2 : 1;
    const FxStop s{rule, min_iters > floor_n ? min_iters : floor_n, syn.data(), used.data()};
    const int nS = window_blocks(L, wn.window);
    if (nS > nW) return 3;

    for (size_t b = 0; b < Bp; ++b) used[b] = 0;   // the decode's reset: every codeword runs
    for (int it = 0; it < iters; ++it) {
        for (int sb = nS - 1; sb >= 0; --sb)
            for (size_t b = 0; b < Bp; ++b) siso_window_stop<0>(p, wn, s, ev.data(), hist.data(), b, it, sb);   // the padding's lane too
        for (int sb = 0; sb < nS; ++sb)
            for (size_t b = 0; b < Bp; ++b) siso_window_stop<1>(p, wn, s, ev.data(), hist.data(), b, it, sb);
        for (size_t b = 0; b < Bp; ++b) window_judge(p, s, ev.data(), nS, b, it);
    }
    if (used[B] != 0) return 3;   // the padding's lane never runs, and the judge leaves it alone
    for (size_t i = 0; i < (size_t)iters * K; ++i)
        if (bT[i * Bp + B] != 9) return 3;
    for (size_t i = 0; i < (size_t)nW; ++i)
        if (ev[i * Bp + B] != 0xdeadbeefu || hist[i * Bp + B] != 0xbeef) return 3;

    std::vector<uint8_t> bits((size_t)B * rows * K);
    for (int b = 0; b < B; ++b) {
        if (used[b] < 1 || used[b] > iters) return 3;
        for (int r = 0; r < rows; ++r) {
            const int src = rows == 1 ? used[b] - 1 : r < used[b] - 1 ? r : used[b] - 1;   // fx_bits_stop_kernel
            for (int k = 0; k < K; ++k)   // the stopping decoder keeps its rows by interleaved position
                bits[((size_t)b * rows + r) * K + k] = bT[((size_t)src * K + pinv[k]) * Bp + b];
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
