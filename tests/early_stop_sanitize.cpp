// Stand-alone check of csrc/td_crc.h (the CRC-24 behind TD_STOP_CRC), built by
// tests/test_early_stop_host.py with -fsanitize=address,undefined and run as a plain process.
// Exit 0: the bit-serial remainder, the per-position table and the appended-CRC property agree for
// K = 25, 40 and 10000 and both LTE generators, with every table exactly K entries long (heap
// buffers of exactly that size, so an index past either end is an ASan report).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_crc.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main()
{
    const uint32_t polys[2] = {0x800063u, 0x864CFBu};
    const int Ks[3] = {25, 40, 10000};
    uint32_t seed = 12345u;
    for (uint32_t poly : polys)
        for (int K : Ks) {
            std::vector<uint32_t> tab((size_t)K);
            td::crc24_syndromes(K, poly, tab.data());
            for (int rep = 0; rep < 4; ++rep) {
                std::vector<uint8_t> row((size_t)K);
                for (int i = 0; i < K; ++i) row[i] = (lcg(seed) >> 16) & 1u;
                if (rep == 0) std::fill(row.begin(), row.end(), (uint8_t)0);
                if (rep == 1) std::fill(row.begin(), row.end(), (uint8_t)1);
                const uint32_t r = td::crc24_bits(row.data(), K, poly);
                uint32_t x = 0;
                for (int i = 0; i < K; ++i)
                    if (row[i]) x ^= tab[i];
                if (x != r || (r & ~td::kCrc24Mask)) {
                    std::printf("K=%d poly=%06x rep=%d: table %06x, serial %06x\n", K, poly, rep, x, r);
                    return 1;
                }
                // the last 24 bits replaced by the CRC of the first K-24: remainder 0
                const uint32_t c = td::crc24_bits(row.data(), K - 24, poly);
                for (int j = 0; j < 24; ++j) row[K - 24 + j] = (c >> (23 - j)) & 1u;
                if (td::crc24_bits(row.data(), K, poly) != 0) {
                    std::printf("K=%d poly=%06x rep=%d: appended CRC leaves a remainder\n", K, poly, rep);
                    return 1;
                }
            }
        }
    std::printf("ok\n");
    return 0;
}
