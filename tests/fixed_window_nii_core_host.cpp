// fixed_window_nii_core_host.cpp -- the lane code of the fixed-point decoder's sub-block schedule with
// next-iteration initialisation (siso_window_pass_nii of csrc/td_fixed_core.h, what a lane of
// fx_window_siso_nii_kernel and fx_window_siso_maxstar_nii_kernel runs) on the host, for
// tests/test_fixed_window_nii_host.py: a stand-alone program, built with AddressSanitizer +
// UndefinedBehaviorSanitizer, that decodes a batch over a workspace and an NII state of exactly the
// kernel's layout and sizes.  One "launch" per SISO and iteration, as the kernel's, with the launcher's own
// arguments (nii_args): SISO1's sub-blocks from the last to the first and SISO2's from the first to the last,
// so a consumer runs before its producer in one SISO and after it in the other, and a state that is not
// double-buffered by the iteration's parity gives other bytes.  The state starts as a pattern that no
// store writes: a slot that is loaded without having been stored shows in the result.
//
//   fixed_window_nii_core_host IN OUT
//   IN   int32 K, iters, all_iters, le_max, ext_scale_q, B, window, overlap, table (0 / 1), shift, corr[8];
//        int32 pi[K];  int8 q[B][3K+12]
//   OUT  uint8 bits[B][rows][K] (rows = all_iters ? iters : 1);  int16 le[B][iters][2][K+3]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_fixed_core.h"

using namespace td::fx;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

template <class M>
static void decode(const FxArgs& p, const FxWindow& wn, uint32_t* nii, const M& m)
{
    const int nS = window_blocks(p.L, wn.window);
    for (int it = 0; it < p.iters; ++it) {
        const FxNii n0 = nii_args(nii, p.L, wn, p.Bp, it, 0), n1 = nii_args(nii, p.L, wn, p.Bp, it, 1);
        for (int sb = nS - 1; sb >= 0; --sb)
            for (size_t b = 0; b < p.Bp; ++b) siso_window_pass_nii<0>(p, wn, n0, b, it, sb, m);   // the padding's lane too
        for (int sb = 0; sb < nS; ++sb)
            for (size_t b = 0; b < p.Bp; ++b) siso_window_pass_nii<1>(p, wn, n1, b, it, sb, m);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t hdr[18];
    if (!f || !rd(f, hdr, 18)) return 2;
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
    std::vector<uint32_t> nii(nii_words(L, wn.window, Bp), 0x5a5a5a5au);   // two int16 of 23130: above every stored value
    if (hdr[8]) {
        MaxStar m{0, 0, hdr[9]};
        for (int j = 0; j < 4; ++j) {
            m.lo |= (uint32_t)hdr[10 + j] << (8 * j);
            m.hi |= (uint32_t)hdr[14 + j] << (8 * j);
        }
        decode(p, wn, nii.data(), m);
    } else {
        decode(p, wn, nii.data(), MaxLog());
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
