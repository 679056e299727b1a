// fixed_window_core_host.cpp -- the lane code of the fixed-point decoder's sub-block schedule
// (siso_window_pass of csrc/td_fixed_core.h, what a lane of fx_window_siso_kernel runs) on the host, for
// tests/test_fixed_window_host.py: a stand-alone program, built with AddressSanitizer +
// UndefinedBehaviorSanitizer, that decodes a batch over a workspace of exactly the kernel's layout and
// sizes, so that an index past an array shows here and not on the GPU.  One "launch" per SISO and
// iteration, as the kernel's: every sub-block of every codeword, SISO1's from the last sub-block to the
// first and SISO2's from the first to the last (the sub-blocks of a launch run in no fixed order).
//
//   fixed_window_core_host IN OUT
//   IN   int32 K, iters, all_iters, le_max, ext_scale_q, B, window, overlap;  int32 pi[K];  int8 q[B][3K+12]
//   OUT  uint8 bits[B][rows][K] (rows = all_iters ? iters : 1);  int16 le[B][iters][2][K+3]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_fixed_core.h"

using namespace td::fx;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t hdr[8];
    if (!f || !rd(f, hdr, 8)) return 2;
    const int K = hdr[0], iters = hdr[1], all_iters = hdr[2], le_max = hdr[3], scale = hdr[4], B = hdr[5];
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
    std::vector<uint8_t> bT((size_t)rows * K * Bp, 9);
    std::vector<int16_t> le((size_t)B * iters * 2 * L, 0x5a5a);
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
    const FxWindow wn{hdr[6], hdr[7]};
    const int nS = window_blocks(L, wn.window);
    for (int it = 0; it < iters; ++it) {
        for (int sb = nS - 1; sb >= 0; --sb)
            for (size_t b = 0; b < Bp; ++b) siso_window_pass<0>(p, wn, b, it, sb);   // the padding's lane too
        for (int sb = 0; sb < nS; ++sb)
            for (size_t b = 0; b < Bp; ++b) siso_window_pass<1>(p, wn, b, it, sb);
    }

    std::vector<uint8_t> bits((size_t)B * rows * K);
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k) bits[((size_t)b * rows + r) * K + k] = bT[((size_t)r * K + k) * Bp + b];
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(bits.data(), 1, bits.size(), o);
    fwrite(le.data(), sizeof(int16_t), le.size(), o);
    fclose(o);
    return 0;
}
