// encode_core_host.cpp -- csrc/td_encode_core.h as a stand-alone host program (tests/test_encode_host.py,
// built with ASan + UBSan).  It walks a row exactly as the workgroup of td_encode.hip does -- pack the bytes
// to bits (eight bytes a lane, or a wave's ballot), gather the second encoder's input through the
// permutation a byte at a time, the per-word prefixes, the exclusive XOR scan of the carries, the staged
// (x, p1, p2) bytes, the split into head bytes, 16-byte pieces and tail bytes -- through the same
// word-level routines, with every buffer sized as the kernel sizes its own.
//
//   encode_core_host <in> <out>
//   in:  int32 mode
//        mode 0 (encode): int32 K, B, misalign; int32 pi[K]; uint8 info[B][K]
//             out: uint8 coded[B][3K+12]   (rows written at a base address `misalign` bytes off 16)
//        mode 1 (crc):    int32 K, B, poly; uint8 rows[B][K]
//             out: uint32 check[B] of the rows as given; uint8 attached[B][K]; uint32 check[B] after attach
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "td_crc.h"
#include "td_encode_core.h"

using namespace td::enc;

static std::vector<uint8_t> slurp(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

// one constituent encoder over nW words: a and p (what a thread per word plus the scan computes)
static void constituent(const std::vector<uint64_t>& u, int nW, std::vector<uint64_t>& a, std::vector<uint64_t>& p)
{
    std::vector<WordLocal> l(nW);
    for (int w = 0; w < nW; ++w) l[w] = word_local(u[w], w ? u[w - 1] : 0, w);
    uint32_t r = 0;   // the exclusive scan
    for (int w = 0; w < nW; ++w) {
        word_finish(l[w], r, w, a[w], p[w]);
        r ^= l[w].q;
    }
}

static void encode_row(const uint8_t* info, const int32_t* pi, int K, uint8_t* dst, bool wide)
{
    const int nW = words_for(K), n = 3 * K + 12;
    std::vector<uint16_t> pi16(K);
    for (int i = 0; i < K; ++i) pi16[i] = (uint16_t)pi[i];
    std::vector<uint64_t> u1(nW, 0), u2(nW, 0), a1(nW), p1(nW), a2(nW), p2(nW);
    uint8_t* u1b = reinterpret_cast<uint8_t*>(u1.data());
    if (wide) {   // an 8-byte aligned row: eight bytes a lane, the rest singly
        for (int j = 0; j < K / 8; ++j) {
            uint32_t lo, hi;
            std::memcpy(&lo, info + 8 * j, 4);
            std::memcpy(&hi, info + 8 * j + 4, 4);
            u1b[j] = (uint8_t)nonzero8(lo, hi);
        }
        for (int i = K & ~7; i < K; ++i)
            if (info[i]) u1b[i >> 3] |= (uint8_t)(1u << (i & 7));
    } else {
        for (int i = 0; i < K; ++i)   // the ballot of 64 lanes' bytes
            if (info[i]) u1[i >> 6] |= 1ull << (i & 63);
    }
    const uint32_t* u32 = reinterpret_cast<const uint32_t*>(u1.data());
    uint8_t* u2b = reinterpret_cast<uint8_t*>(u2.data());
    for (int j = 0; j < (K + 7) / 8; ++j) {   // a byte of u2 a thread
        uint32_t acc = 0;
        for (int t = 0; t < 8 && 8 * j + t < K; ++t) {
            const uint32_t s = pi16[8 * j + t];
            acc |= ((u32[s >> 5] >> (s & 31)) & 1u) << t;
        }
        u2b[j] = (uint8_t)acc;
    }
    constituent(u1, nW, a1, p1);
    constituent(u2, nW, a2, p2);

    const RowSplit sp = row_split(reinterpret_cast<uintptr_t>(dst), n);
    // the stage as the kernel sizes it, 16-byte aligned like the LDS: UBSan checks stage_vec's aligned reads
    uint32_t* stage = static_cast<uint32_t*>(std::aligned_alloc(16, ((size_t)stage_dwords(n) * 4 + 15) / 16 * 16));
    std::vector<uint32_t> exact(stage_dwords(n));   // and an exactly sized copy for ASan's view of its end
    uint8_t* stage8 = reinterpret_cast<uint8_t*>(stage) + 4 * sp.s4;   // row byte x
    const uint8_t* p1b = reinterpret_cast<const uint8_t*>(p1.data());
    const uint8_t* p2b = reinterpret_cast<const uint8_t*>(p2.data());
    for (int j = 0; j < (K + 7) / 8; ++j) pack24(u1b[j], p1b[j], p2b[j], &exact[sp.s4 + 6 * j]);
    std::memcpy(stage, exact.data(), exact.size() * 4);
    tail6(row_bit(a1.data(), K - 1), row_bit(a1.data(), K - 2), row_bit(a1.data(), K - 3), stage8 + 3 * K);
    tail6(row_bit(a2.data(), K - 1), row_bit(a2.data(), K - 2), row_bit(a2.data(), K - 3), stage8 + 3 * K + 6);

    for (int t = 0; t < sp.head; ++t) dst[t] = stage8[t];
    for (int j = 0; j < sp.nvec; ++j) {
        const int o = 4 * sp.s4 + sp.head + 16 * j;
        if (o - (o & 3) + ((o & 3) ? 20 : 16) > 4 * stage_dwords(n)) { std::fprintf(stderr, "stage overread\n"); std::exit(3); }
        const Vec16 v = stage_vec(stage, sp, j);
        std::memcpy(dst + sp.head + 16 * j, v.v, 16);
    }
    const int done = sp.head + 16 * sp.nvec;
    for (int t = 0; t < sp.tail; ++t) dst[done + t] = stage8[done + t];
    std::free(stage);
}

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    const std::vector<uint8_t> in = slurp(argv[1]);
    int32_t hd[4];
    if (in.size() < sizeof hd) return 2;
    std::memcpy(hd, in.data(), sizeof hd);
    const int mode = hd[0], K = hd[1], B = hd[2];
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::perror(argv[2]); return 2; }
    if (mode == 0) {
        const int mis = hd[3] & 15, n = 3 * K + 12;
        if (K < 1 || K > kMaxK || in.size() != sizeof hd + 4u * K + (size_t)B * K) return 2;
        std::vector<int32_t> pi(K);
        std::memcpy(pi.data(), in.data() + sizeof hd, 4u * K);
        const uint8_t* info = in.data() + sizeof hd + 4u * K;
        std::vector<uint8_t> out((size_t)B * n);
        for (int b = 0; b < B; ++b) {
            // row b at the alignment it has in a [B][3K+12] array that starts `mis` bytes past a 16-byte
            // boundary, inside a block of guard bytes
            std::vector<uint8_t> block((size_t)n + 32);
            uint8_t* al = block.data() + ((16 - (reinterpret_cast<uintptr_t>(block.data()) & 15)) & 15);
            uint8_t* dst = al + ((mis + (size_t)b * n) & 15);
            std::memset(block.data(), 0xA5, block.size());
            encode_row(info + (size_t)b * K, pi.data(), K, dst, ((b + mis) & 1) == 0);   // both input paths, every other row
            for (uint8_t* q = block.data(); q < block.data() + block.size(); ++q)
                if ((q < dst || q >= dst + n) && *q != 0xA5) { std::fprintf(stderr, "guard byte written\n"); return 3; }
            std::memcpy(&out[(size_t)b * n], dst, n);
        }
        std::fwrite(out.data(), 1, out.size(), fo);
    } else if (mode == 1) {
        const uint32_t poly = (uint32_t)hd[3];
        if (K <= 24 || in.size() != sizeof hd + (size_t)B * K) return 2;
        std::vector<uint8_t> rows(in.begin() + sizeof hd, in.end());
        std::vector<uint32_t> syn(K), before(B), after(B);
        td::crc24_syndromes(K, poly, syn.data());
        auto check = [&](const uint8_t* r) {
            uint32_t acc = 0;
            for (int i = 0; i < K; ++i) acc ^= crc_term(r[i], syn[i]);
            return acc;
        };
        for (int b = 0; b < B; ++b) {
            uint8_t* r = &rows[(size_t)b * K];
            before[b] = check(r);
            uint32_t crc = 0;
            for (int i = 0; i < K - 24; ++i) crc ^= crc_term(r[i], syn[i + 24]);
            for (int j = 0; j < 24; ++j) r[K - 24 + j] = crc_out_bit(crc, j);
            after[b] = check(r);
        }
        std::fwrite(before.data(), 4, B, fo);
        std::fwrite(rows.data(), 1, rows.size(), fo);
        std::fwrite(after.data(), 4, B, fo);
    } else {
        return 2;
    }
    std::fclose(fo);
    return 0;
}
