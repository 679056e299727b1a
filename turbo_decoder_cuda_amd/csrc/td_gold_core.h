// td_gold_core.h -- the length-31 Gold sequence of 3GPP TS 36.211 7.2 (the scrambling sequence of PDSCH 6.3.1
// and PUSCH 5.3.1): the two shift registers, their step of 32 positions, the jump to a far offset, the tables
// the jump reads and the element operations of td_scramble / td_descramble_llr.
//
//   x1(n+31) = x1(n+3) ^ x1(n),                          x1(0) = 1, x1(1..30) = 0
//   x2(n+31) = x2(n+3) ^ x2(n+2) ^ x2(n+1) ^ x2(n),      x2(i) = bit i of c_init, i < 31
//   c(n)     = x1(n+1600) ^ x2(n+1600)
//
// Plain integer C++ shared by the gfx950 kernels of td_scramble.hip, by td_api.cpp (td_gold_sequence_host) and
// by the stand-alone host program of the tests (tests/gold_core_host.cpp, under ASan + UBSan).
//
// A register's state at position n is the word s with bit i = x(n+i), i < 31.  Both recurrences reach back at
// least 28 positions, so 28 new positions follow from a state in one shift-and-XOR; two of those give the 63
// positions n .. n+62, which are the 32 output bits at n and the state at n+32 (gold_step32).
//
// Advancing a state is linear over GF(2): state(n+d) = T^d state(n), T the 31 x 31 one-step matrix.  A matrix
// is held as its 31 columns, column i the image of the state with only bit i set; applying it XORs the columns
// of the state's set bits (gold_apply).  The tables hold, per register, T^1600 (the standard's offset Nc) and
// T^(kGoldRun 2^j), j < kGoldLevels, by repeated squaring at compile time.  The state at 1600 + kGoldRun t is
// T^1600's image with the matrices of t's set bits applied: at most kGoldLevels + 1 applications, whatever t
// (gold_jump).  kGoldRun 2^kGoldLevels = 2^31: every offset below the largest length.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TDG_HD __host__ __device__ __forceinline__
#else
#define TDG_HD inline
#endif

namespace td {
namespace gold {

constexpr int kGoldRun = 1024;       // bits a jump lands on a multiple of: a thread's run in gold_kernel
constexpr int kGoldRunWords = kGoldRun / 32;
constexpr int kGoldLevels = 21;      // kGoldRun << kGoldLevels = 2^31
constexpr int kGoldNc = 1600;
constexpr long long kGoldMaxLen = 0x7FFFFFFFll;   // len < 2^31
constexpr uint32_t kStateMask = 0x7FFFFFFFu;

// s ^ (the taps' shifts): bit i = x(n+31+i) wherever bits i .. i+3 of s are positions n+i .. n+i+3
template <bool X2>
constexpr TDG_HD uint64_t taps(uint64_t s)
{
    return X2 ? s ^ (s >> 1) ^ (s >> 2) ^ (s >> 3) : s ^ (s >> 3);
}

// The state at n -> the 32 bits x(n) .. x(n+31) (bit i = x(n+i)); the state becomes the one at n+32.
template <bool X2>
constexpr TDG_HD uint32_t gold_step32(uint32_t& state)
{
    uint64_t s = state & kStateMask;                       // positions 0 .. 30
    s |= (taps<X2>(s) & 0x0FFFFFFFull) << 31;              // 31 .. 58: taps read up to position 30
    s |= ((taps<X2>(s) >> 28) & 0xFull) << 59;             // 59 .. 62: taps read up to position 34
    state = (uint32_t)(s >> 32) & kStateMask;
    return (uint32_t)s;
}

// one position, for the tables' construction and the tests
template <bool X2>
constexpr TDG_HD uint32_t gold_step1(uint32_t state)
{
    return ((state & kStateMask) >> 1) | ((uint32_t)(taps<X2>(state) & 1u) << 30);
}

// a matrix (31 columns) applied to a state
constexpr TDG_HD uint32_t gold_apply(const uint32_t* col, uint32_t s)
{
    uint32_t r = 0;
    for (int i = 0; i < 31; ++i) r ^= (0u - ((s >> i) & 1u)) & col[i];
    return r;
}

struct GoldJump {
    uint32_t first[31];                // T^1600
    uint32_t run[kGoldLevels][31];     // T^(kGoldRun 2^j)
};
struct GoldTables {
    GoldJump x1, x2;
};

// out = a b (a applied after b)
constexpr void gold_mul(const uint32_t* a, const uint32_t* b, uint32_t* out)
{
    uint32_t t[31] = {};
    for (int i = 0; i < 31; ++i) t[i] = gold_apply(a, b[i]);
    for (int i = 0; i < 31; ++i) out[i] = t[i];
}

template <bool X2>
constexpr GoldJump make_jump()
{
    GoldJump j{};
    uint32_t p[31] = {};   // T^(2^k), k = 0, 1, ...
    for (int i = 0; i < 31; ++i) p[i] = gold_step1<X2>(1u << i);
    bool have_first = false;
    for (int k = 0; k < 10 + kGoldLevels; ++k) {
        if ((kGoldNc >> k) & 1) {   // 1600 = 2^10 + 2^9 + 2^6
            if (have_first)
                gold_mul(p, j.first, j.first);
            else
                for (int i = 0; i < 31; ++i) j.first[i] = p[i];
            have_first = true;
        }
        if (k >= 10)
            for (int i = 0; i < 31; ++i) j.run[k - 10][i] = p[i];
        gold_mul(p, p, p);
    }
    return j;
}
static_assert(kGoldRun == 1 << 10 && kGoldNc < (1 << 11), "make_jump's exponents");

constexpr GoldJump kJumpX1 = make_jump<false>();
constexpr GoldJump kJumpX2 = make_jump<true>();
constexpr GoldTables kGoldTables = {kJumpX1, kJumpX2};

// The state at 1600 + kGoldRun t of the register whose state at 0 is s0 (x1: 1; x2: c_init's 31 low bits).
TDG_HD uint32_t gold_jump(const GoldJump& j, uint32_t s0, uint32_t t)
{
    uint32_t s = gold_apply(j.first, s0 & kStateMask);
    for (int l = 0; l < kGoldLevels; ++l)
        if ((t >> l) & 1u) s = gold_apply(j.run[l], s);
    return s;
}

// the last word's bits >= len are zero
TDG_HD uint32_t gold_tail_mask(long long len, long long w)
{
    const long long left = len - 32 * w;
    return left >= 32 ? 0xFFFFFFFFu : (1u << (int)left) - 1u;
}

// Words [w0, w1) of c for one c_init, w0 a multiple of kGoldRunWords; `x` holds the two tables.
inline void gold_words(const GoldTables& x, uint32_t cinit, long long len, long long w0, long long w1, uint32_t* seq)
{
    const uint32_t t = (uint32_t)(w0 / kGoldRunWords);
    uint32_t s1 = gold_jump(x.x1, 1u, t), s2 = gold_jump(x.x2, cinit, t);
    for (long long w = w0; w < w1; ++w) {
        const uint32_t c = gold_step32<false>(s1) ^ gold_step32<true>(s2);
        seq[w] = c & gold_tail_mask(len, w);
    }
}

// ---- the element operations of td_scramble / td_descramble_llr

// bit g of a row of words
TDG_HD uint32_t gold_bit(const uint32_t* row, long long g) { return (row[g >> 5] >> (int)(g & 31)) & 1u; }

TDG_HD uint8_t scramble_bit(uint8_t b, uint32_t c) { return (uint8_t)((b != 0 ? 1u : 0u) ^ c); }

// the sign flipped where c = 1: IEEE negation on the bits (0.0 -> -0.0, a NaN keeps its payload) ...
TDG_HD uint64_t flip_bits(uint64_t v, uint32_t c) { return v ^ ((uint64_t)c << 63); }
TDG_HD uint32_t flip_bits(uint32_t v, uint32_t c) { return v ^ (c << 31); }
// ... and int8: -128 read as -127, then negated; c = 0 copies, -128 included
TDG_HD uint8_t flip_bits(uint8_t v, uint32_t c)
{
    const int x = (int8_t)v;
    return c ? (uint8_t)(int8_t)(x < -127 ? 127 : -x) : v;
}
TDG_HD double flip_sign(double x, uint32_t c)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    u = flip_bits(u, c);
    __builtin_memcpy(&x, &u, sizeof u);
    return x;
}

}  // namespace gold
}  // namespace td
