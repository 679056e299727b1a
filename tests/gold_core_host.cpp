// gold_core_host.cpp -- csrc/td_gold_core.h as a stand-alone host program (ASan + UBSan; tests/test_scramble_host.py):
// the registers' 32-position step, the jump at every level, and the words of whole sequences.
//
//   gold_core_host in.bin out.bin
// in:  uint32 c_init of the walk, uint32 count, then `count` pairs (c_init, len), len < 2^31
// out: uint32 words
//   the walk: both registers stepped word by word from position 1600 through 2^31 bits.  At every position
//   1600 + kGoldRun t with t a power of two or one less than a power of two, t < 2^21 -- every level of the jump
//   alone and all levels below one together -- the stepped states are compared with gold_jump's: the program
//   writes the number of positions compared, the number that differed (0), and the XOR of all output words
//   the first 4096 bits stepped one position a time against the 32-position step: the number of words that differ
//   per pair: the (len + 31) / 32 words of gold_words from word 0, written into a buffer with two guard words
//   behind it, then the two guard words as found; and 1 or 0: the words from the run holding the last word
//   onwards, made on their own (a jump, then steps), equal the same words of the whole
#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_gold_core.h"

using namespace td::gold;

constexpr uint32_t kGuard = 0xA5A5A5A5u;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[2] = {0, 0};
    if (std::fread(head, 4, 2, f) != 2) return 2;
    std::vector<uint32_t> in(2 * (size_t)head[1]);
    if (!in.empty() && std::fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    std::fclose(f);
    const uint32_t walk_cinit = head[0];
    std::vector<uint32_t> out;

    {   // the walk
        uint32_t s1 = gold_jump(kGoldTables.x1, 1u, 0), s2 = gold_jump(kGoldTables.x2, walk_cinit, 0);
        uint32_t compared = 0, differed = 0, all = 0;
        const uint64_t words = 1ull << 26;   // 2^31 bits
        for (uint64_t w = 0; w < words; ++w) {
            if (w % kGoldRunWords == 0) {
                const uint64_t t = w / kGoldRunWords;
                if ((t & (t - 1)) == 0 || (t & (t + 1)) == 0) {   // 0, 2^j, 2^j - 1
                    ++compared;
                    if (s1 != gold_jump(kGoldTables.x1, 1u, (uint32_t)t) || s2 != gold_jump(kGoldTables.x2, walk_cinit, (uint32_t)t))
                        ++differed;
                }
            }
            all ^= gold_step32<false>(s1) ^ gold_step32<true>(s2);
        }
        out.push_back(compared);
        out.push_back(differed);
        out.push_back(all);
    }
    {   // one position a time, from position 0 (no jump: 1600 single steps first)
        uint32_t a1 = 1u, a2 = walk_cinit & kStateMask;
        for (int n = 0; n < kGoldNc; ++n) a1 = gold_step1<false>(a1), a2 = gold_step1<true>(a2);
        uint32_t s1 = gold_jump(kGoldTables.x1, 1u, 0), s2 = gold_jump(kGoldTables.x2, walk_cinit, 0);
        uint32_t bad = (a1 != s1) + (a2 != s2);
        for (int w = 0; w < 128; ++w) {
            uint32_t c = 0;
            for (int i = 0; i < 32; ++i) {
                c |= ((a1 ^ a2) & 1u) << i;
                a1 = gold_step1<false>(a1), a2 = gold_step1<true>(a2);
            }
            bad += c != (gold_step32<false>(s1) ^ gold_step32<true>(s2));
            bad += (a1 != s1) + (a2 != s2);
        }
        out.push_back(bad);
    }
    for (uint32_t c = 0; c < head[1]; ++c) {
        const uint32_t cinit = in[2 * c];
        const long long len = in[2 * c + 1];
        if (len < 1 || len > kGoldMaxLen) return 3;
        const long long W = (len + 31) / 32;
        std::vector<uint32_t> seq((size_t)W + 2, kGuard);   // exactly W words and the guard: ASan sees one word further
        gold_words(kGoldTables, cinit, len, 0, W, seq.data());
        out.insert(out.end(), seq.begin(), seq.end());
        const long long w0 = (W - 1) / kGoldRunWords * kGoldRunWords;
        std::vector<uint32_t> part((size_t)W, 0u);
        gold_words(kGoldTables, cinit, len, w0, W, part.data());
        uint32_t same = 1;
        for (long long w = w0; w < W; ++w) same &= part[(size_t)w] == seq[(size_t)w];
        out.push_back(same);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty() && std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
