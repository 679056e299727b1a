// td_crc.h -- host-side CRC-24 of a hard-decision row (the early-termination rule TD_STOP_CRC).
// Plain C++, no HIP: td_api.cpp builds the kernel's table with it, the host tests compile it alone.
//
// The row is K bits in natural order, first bit first; the register starts at zero and there is no
// final XOR (the LTE code-block CRC, 3GPP TS 36.212 5.1.1): remainder = (sum_i bit[i] x^(K-1-i)) x^24
// mod g, with g = x^24 + poly (poly = the 24 low-order coefficients: 0x800063 gCRC24B, 0x864CFB
// gCRC24A).  A row that ends in its own CRC has remainder 0.
//
// The remainder is linear over GF(2): it is the XOR over the set bits of a per-position value
// syndrome[i] = x^(K-1-i+24) mod g.  The kernel's fold lanes, which meet the bits in interleaved
// order, XOR syndrome[position] of their 1-bits; nobody walks the row in order.
#pragma once

#include <cstdint>

namespace td {

constexpr uint32_t kCrc24Mask = 0xFFFFFFu;

// x * v mod g
inline uint32_t crc24_mulx(uint32_t v, uint32_t poly)
{
    const uint32_t top = (v >> 23) & 1u;
    v = (v << 1) & kCrc24Mask;
    return top ? v ^ (poly & kCrc24Mask) : v;
}

// bit-serial remainder of bits[0..K) (any non-zero byte is a 1)
inline uint32_t crc24_bits(const uint8_t* bits, int K, uint32_t poly)
{
    uint32_t reg = 0;
    for (int i = 0; i < K; ++i) {
        const uint32_t top = ((reg >> 23) & 1u) ^ (bits[i] ? 1u : 0u);
        reg = (reg << 1) & kCrc24Mask;
        if (top) reg ^= poly & kCrc24Mask;
    }
    return reg;
}

// table[i] = x^(K-1-i+24) mod g, i in [0, K)
inline void crc24_syndromes(int K, uint32_t poly, uint32_t* table)
{
    uint32_t v = poly & kCrc24Mask;   // x^24 mod g
    for (int i = K - 1; i >= 0; --i) {
        table[i] = v;
        v = crc24_mulx(v, poly);
    }
}

}  // namespace td
