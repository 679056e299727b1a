// td_encode_core.h -- the arithmetic of the batched turbo encoder and of the CRC-24 attach / check.
//
// Plain integer C++ shared by the gfx950 kernels of td_encode.hip and by the stand-alone host program of
// the tests (tests/encode_core_host.cpp, under ASan + UBSan).  The library never encodes on the host.
//
// The constituent code (Rsc::step; encode_bit, log_map.cpp:247-269): register input a[i] = u[i] ^ a[i-2] ^
// a[i-3] (feedback 1 + D^2 + D^3), parity p[i] = a[i] ^ a[i-1] ^ a[i-3] (forward 1 + D + D^3), zero start.
// It is linear over GF(2), and the feedback polynomial divides 1 + D^7:
//   a = u (1 + D^2 + D^3 + D^4) / (1 + D^7)            p = u (1 + D + D^2 + D^3 + D^6 + D^7) / (1 + D^7)
// A row is held as 64-bit words, bit i of the row in bit i % 64 of word i / 64, so D is a left shift with
// the previous word's top bits shifted in, and 1 / (1 + D^7) is a prefix XOR at stride 7.  Inside a word
// that is four shift-XORs (prefix7).  Across words the only thing carried is, for each of the seven
// residue classes of the bit index modulo 7, the parity of the numerator's bits so far: seven bits a
// sequence, which add up by plain XOR.  So the kernel's carry is an exclusive XOR scan over the words of a
// 7-bit value (word_local's q), and word_finish folds the scanned value back in as a period-7 pattern.
// No step depends on more than its own word, the previous word of the input and the scan.
//
// The three tail steps feed the register its own feedback (a = 0), so they follow from the last three
// bits of a (tail6).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TDE_HD __host__ __device__ __forceinline__
#else
#define TDE_HD inline
#endif

namespace td {
namespace enc {

constexpr int kMaxK = 10000;
constexpr int kMaxWords = (kMaxK + 63) / 64;   // 157

TDE_HD int words_for(int K) { return (K + 63) >> 6; }

// x / (1 + D^7) inside one word: bit k becomes x[k] ^ x[k-7] ^ x[k-14] ^ ...
TDE_HD uint64_t prefix7(uint64_t x)
{
    x ^= x << 7;
    x ^= x << 14;
    x ^= x << 28;
    x ^= x << 56;
    return x;
}

// u D^s of the word u whose predecessor in the row is `prev`, 1 <= s <= 7
TDE_HD uint64_t delay(uint64_t u, uint64_t prev, int s) { return (u << s) | (prev >> (64 - s)); }

// the numerators: u (1 + D^2 + D^3 + D^4) and u (1 + D + D^2 + D^3 + D^6 + D^7)
TDE_HD uint64_t num_a(uint64_t u, uint64_t prev) { return u ^ delay(u, prev, 2) ^ delay(u, prev, 3) ^ delay(u, prev, 4); }
TDE_HD uint64_t num_p(uint64_t u, uint64_t prev)
{
    return u ^ delay(u, prev, 1) ^ delay(u, prev, 2) ^ delay(u, prev, 3) ^ delay(u, prev, 6) ^ delay(u, prev, 7);
}

// 7-bit rotate: bit j of x goes to bit (j + s) mod 7, 0 <= s <= 6
TDE_HD uint32_t rotl7(uint32_t x, int s) { return ((x << s) | (x >> (7 - s))) & 0x7Fu; }
// bit k of the result = bit k % 7 of x (x < 128): copies at 0, 7, ..., 63
TDE_HD uint64_t expand7(uint32_t x) { return (uint64_t)x * 0x8102040810204081ull; }

// One word of one constituent encoder before the carry is known.
struct WordLocal {
    uint64_t a, p;   // the in-word prefix XORs of the two numerators
    uint32_t q;      // what the word adds to the carry: a's seven class parities in bits 0..6, p's in 7..13,
                     // by the residue of the ROW index modulo 7
};

// u = word w of the encoder's input (bits at and beyond K zero), prev = word w - 1 (0 for w = 0)
TDE_HD WordLocal word_local(uint64_t u, uint64_t prev, int w)
{
    WordLocal l;
    l.a = prefix7(num_a(u, prev));
    l.p = prefix7(num_p(u, prev));
    // bit 57 + j of a prefix is the parity of the word's bits k = 57 + j (mod 7); bit k of word w is row
    // index 64 w + k = w + k (mod 7), so that is class (w + 1 + j) mod 7
    const int s = (w + 1) % 7;
    l.q = rotl7((uint32_t)(l.a >> 57), s) | (rotl7((uint32_t)(l.p >> 57), s) << 7);
    return l;
}

// r = the XOR of q over the words before w (the exclusive scan).  Bit k of word w takes class (w + k) mod 7.
TDE_HD void word_finish(const WordLocal& l, uint32_t r, int w, uint64_t& a, uint64_t& p)
{
    const int s = (7 - w % 7) % 7;   // rotate right by w mod 7
    a = l.a ^ expand7(rotl7(r & 0x7Fu, s));
    p = l.p ^ expand7(rotl7((r >> 7) & 0x7Fu, s));
}

// bit i of a row of words, 0 for i < 0 (the register starts at zero)
TDE_HD uint32_t row_bit(const uint64_t* words, int i) { return i < 0 ? 0u : (uint32_t)((words[i >> 6] >> (i & 63)) & 1u); }

// The three tail steps (log_map.cpp:483-491): x = the register's feedback, so its input is 0.  out = the
// three (x, p) pairs, from s0 = a[K-1] (the newest register bit), s1 = a[K-2], s2 = a[K-3].
TDE_HD void tail6(uint32_t s0, uint32_t s1, uint32_t s2, uint8_t out[6])
{
    out[0] = (uint8_t)(s1 ^ s2), out[1] = (uint8_t)(s0 ^ s2);   // state (s0, s1, s2) -> (0, s0, s1)
    out[2] = (uint8_t)(s0 ^ s1), out[3] = (uint8_t)s1;          //                    -> (0, 0, s0)
    out[4] = (uint8_t)s0, out[5] = (uint8_t)s0;
}

// Four bytes (a little-endian dword) -> four bits: bit j = (byte j != 0).  The ORs fold every byte onto its
// lowest bit (what they drag in from the next byte never reaches it); the multiply gathers the four lowest
// bits (products land on distinct bits: no carries) into bits 24 .. 27.
TDE_HD uint32_t nonzero4(uint32_t x)
{
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;
    return ((x & 0x01010101u) * 0x01020408u) >> 24;
}
// eight info bytes -> a byte of the row's bit array
TDE_HD uint32_t nonzero8(uint32_t lo, uint32_t hi) { return nonzero4(lo) | (nonzero4(hi) << 4); }

// a nibble -> its four bits as the low bits of four bytes
TDE_HD uint32_t spread4(uint32_t n) { return ((n & 0xFu) * 0x00204081u) & 0x01010101u; }
// Four info bits' (x, p1, p2) bytes from the spread nibbles: byte j of u, p1, p2 goes to bytes 3j, 3j+1,
// 3j+2 of the 12 (little-endian dwords).
TDE_HD void weave12(uint32_t u, uint32_t p1, uint32_t p2, uint32_t d[3])
{
    d[0] = (u & 0xFFu) | ((p1 & 0xFFu) << 8) | ((p2 & 0xFFu) << 16) | ((u & 0xFF00u) << 16);
    d[1] = ((p1 >> 8) & 0xFFu) | (p2 & 0xFF00u) | (u & 0xFF0000u) | ((p1 & 0xFF0000u) << 8);
    d[2] = ((p2 >> 16) & 0xFFu) | ((u >> 24) << 8) | ((p1 >> 24) << 16) | (p2 & 0xFF000000u);
}
// Eight info bits (a byte of each of the bit arrays u, p1, p2): 24 bytes, row bytes 24 j .. 24 j + 23.
TDE_HD void pack24(uint32_t u, uint32_t p1, uint32_t p2, uint32_t d[6])
{
    weave12(spread4(u), spread4(p1), spread4(p2), d);
    weave12(spread4(u >> 4), spread4(p1 >> 4), spread4(p2 >> 4), d + 3);
}

// A row of n = 3K + 12 bytes leaves for an address that is only byte-aligned: `head` single bytes up to the
// first 16-byte boundary, nvec 16-byte pieces, `tail` single bytes.  The row is staged (in LDS) s4 dwords
// into the stage, s4 = the dword of its 16-byte line the address falls in: row byte x is stage byte
// 4 s4 + x, so a 16-byte piece of the destination is a 16-byte aligned piece of the stage moved by
// addr % 4 bytes -- by nothing when the row is dword-aligned, as every row of a K that is a multiple of 4 is.
struct RowSplit {
    int s4, head, nvec, tail;
};
struct alignas(16) Vec16 {
    uint32_t v[4];
};
TDE_HD RowSplit row_split(uintptr_t addr, int n)
{
    RowSplit s;
    const int h = (int)((16u - (unsigned)(addr & 15u)) & 15u);
    s.s4 = (int)((addr >> 2) & 3u);
    s.head = h < n ? h : n;
    s.nvec = (n - s.head) / 16;
    s.tail = n - s.head - 16 * s.nvec;
    return s;
}
// dwords of the stage: the shift (up to 3), the last byte's 24 bytes may end at row byte 24 ceil(K/8) <=
// n + 9 (what lies past 3K there is overwritten by the tail or never leaves), and stage_vec reads whole
// 16-byte pieces up to 4 bytes past the row's end
TDE_HD int stage_dwords(int n) { return (n + 3) / 4 + 8; }
TDE_HD uint32_t funnel(uint32_t hi, uint32_t lo, int bits) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> bits); }
// piece j (row_split's nvec > 0, so `head` reaches the boundary): stage bytes [o, o + 16), o = 4 s4 + head + 16 j
TDE_HD Vec16 stage_vec(const uint32_t* stage, const RowSplit& sp, int j)
{
    const int o = 4 * sp.s4 + sp.head + 16 * j, d = o >> 2, f = 8 * (o & 3);
    if (f == 0) return *reinterpret_cast<const Vec16*>(stage + d);   // o is a multiple of 16
    const uint32_t lo = stage[d];                                         // o = 16 m - addr % 4: d + 1 = 4 m
    const Vec16 x = *reinterpret_cast<const Vec16*>(stage + d + 1);
    Vec16 r;
    r.v[0] = funnel(x.v[0], lo, f);
    r.v[1] = funnel(x.v[1], x.v[0], f);
    r.v[2] = funnel(x.v[2], x.v[1], f);
    r.v[3] = funnel(x.v[3], x.v[2], f);
    return r;
}

// CRC-24 (td_crc.h): syn[i] = x^(K-1-i+24) mod g is the remainder of the row with only bit i set.
// check  = the XOR of syn[i] over the set bits i < K
// attach = the XOR of syn[i + 24] over the set bits i < K - 24: x^(K-1-i) mod g summed is the CRC of the
//          payload; it is written most significant bit first into bits K-24 .. K-1.
TDE_HD uint32_t crc_term(uint8_t byte, uint32_t syn) { return byte ? syn : 0u; }
TDE_HD uint8_t crc_out_bit(uint32_t crc, int j) { return (uint8_t)((crc >> (23 - j)) & 1u); }   // j = 0 .. 23

}  // namespace enc
}  // namespace td
