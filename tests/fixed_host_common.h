// fixed_host_common.h -- what the stand-alone host program of the fixed-point decoder's lane code
// (tests/fixed_core_host.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/fixed_host.py)
// needs around the launches: the reader, fx_demux_kernel's demultiplex, a workspace of exactly the kernel's
// layout and sizes -- so that an index past an array shows here and not on the GPU --, the two transposes
// back and the writer.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_crc.h"
#include "td_fixed_core.h"

namespace fxhost {

using namespace td::fx;

// IN: int32 hdr[nhdr] with hdr[0] = K and hdr[5] = B;  int32 pi[K];  int8 q[B][3K+12]
inline bool read_input(const char* path, int32_t* hdr, size_t nhdr, std::vector<int32_t>& pi, std::vector<int8_t>& q)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    bool ok = fread(hdr, sizeof(int32_t), nhdr, f) == nhdr && hdr[0] > 0 && hdr[5] > 0;
    if (ok) {
        pi.resize((size_t)hdr[0]);
        q.resize((size_t)hdr[5] * (3 * (size_t)hdr[0] + 12));
        ok = fread(pi.data(), sizeof(int32_t), pi.size(), f) == pi.size() && fread(q.data(), 1, q.size(), f) == q.size();
    }
    fclose(f);
    return ok;
}

// The workspace of fx_carve with an odd pitch, every array that the lane code writes before it reads
// holding a pattern: read before written gives wrong bits, or a signed overflow under UBSan.
struct Workspace {
    int K, L, B, iters, rows, nW;
    size_t Bp;            // B + 1: one lane of padding, as the kernel's last wave has
    std::vector<int32_t> pi, pinv, ck, used, syn;
    std::vector<int8_t> xs, xp1, xp2;
    std::vector<int16_t> e12, e21, le;
    std::vector<uint8_t> bT;
    std::vector<uint32_t> ev;     // fx_carve's: nW words a codeword
    std::vector<uint16_t> hist;   // and nW packed windows (HDA)

    // stopping: bitsT has a row per iteration, whatever all_iters is (fx_carve); else only the rows that are written
    Workspace(int K_, int iters_, int all_iters, int B_, const std::vector<int32_t>& pi_, const std::vector<int8_t>& q,
              bool stopping)
        : K(K_), L(K_ + 3), B(B_), iters(iters_), rows(all_iters ? iters_ : 1), nW((K_ + 3 + kW - 1) / kW),
          Bp((size_t)B_ + 1), pi(pi_), pinv(K_), ck((size_t)nW * 8 * Bp, 0x5a5a5a5a), used(Bp, -1),
          xs((size_t)(L + 3) * Bp, 0), xp1((size_t)L * Bp, 0), xp2((size_t)L * Bp, 0), e12((size_t)K * Bp, 0x5a5a),
          e21((size_t)K * Bp, 0x5a5a), le((size_t)B * iters * 2 * L, 0x5a5a),
          bT((size_t)(stopping ? iters : rows) * K * Bp, 9), ev((size_t)nW * Bp, 0xdeadbeefu),
          hist((size_t)nW * Bp, 0xbeef)
    {
        for (int i = 0; i < K; ++i) pinv[pi[i]] = i;
        const int n = 3 * K + 12;
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
    }

    FxArgs args(int all_iters, int le_max, int scale)
    {
        return FxArgs{xs.data(), xp1.data(), xp2.data(), e12.data(), e21.data(), ck.data(), bT.data(), le.data(),
                      pi.data(), pinv.data(), K, L, B, iters, all_iters, le_max, scale, Bp};
    }

    // the rule as decode_fixed passes it; syn is exactly what the rule reads: nothing for HDA, syndrome[pi[i]] for CRC
    FxStop stop(int rule, int min_iters, uint32_t poly)
    {
        if (rule == 2) {
            std::vector<uint32_t> nat(K);
            td::crc24_syndromes(K, poly, nat.data());
            syn.resize(K);
            for (int i = 0; i < K; ++i) syn[i] = (int32_t)nat[pi[i]];
        }
        const int floor_n = rule == 1 ? 2 : 1;
        return FxStop{rule, min_iters > floor_n ? min_iters : floor_n, syn.data(), used.data()};
    }

    // fx_bits_kernel
    std::vector<uint8_t> bits() const
    {
        std::vector<uint8_t> out((size_t)B * rows * K);
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < rows; ++r)
                for (int k = 0; k < K; ++k) out[((size_t)b * rows + r) * K + k] = bT[((size_t)r * K + k) * Bp + b];
        return out;
    }

    // fx_bits_stop_kernel: the frozen rows, which the stopping decoder keeps by interleaved position; empty if
    // a count is out of range
    std::vector<uint8_t> bits_stop() const
    {
        std::vector<uint8_t> out((size_t)B * rows * K);
        for (int b = 0; b < B; ++b) {
            if (used[b] < 1 || used[b] > iters) return {};
            for (int r = 0; r < rows; ++r) {
                const int src = rows == 1 ? used[b] - 1 : r < used[b] - 1 ? r : used[b] - 1;
                for (int k = 0; k < K; ++k) out[((size_t)b * rows + r) * K + k] = bT[((size_t)src * K + pinv[k]) * Bp + b];
            }
        }
        return out;
    }

    // OUT: uint8 bits[B][rows][K];  int16 le[B][iters][2][K+3], 0x5a5a where nothing was written;  int32 used[B]
    bool write(const char* path, const std::vector<uint8_t>& out) const
    {
        FILE* o = fopen(path, "wb");
        if (!o) return false;
        fwrite(out.data(), 1, out.size(), o);
        fwrite(le.data(), sizeof(int16_t), le.size(), o);
        fwrite(used.data(), sizeof(int32_t), (size_t)B, o);
        return fclose(o) == 0;
    }
};

}  // namespace fxhost
