// td_encode.h -- the launchers of td_encode.hip: the batched turbo encoder (td_encode_device) and the
// CRC-24 attach / check (td_crc_attach, td_crc_check).  The arithmetic is td_encode_core.h's.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace td {

struct EncParams {
    int K, B;
    const int* pi;          // [K] the handle's QPP table
    const uint8_t* info;    // [B][K]
    uint8_t* coded;         // [B][3K+12]
    int cus;                // compute units of the device (sizes the grid)
};

struct CrcParams {
    int K, B;
    const uint32_t* syn;    // [K] td_crc24_syndromes of the handle's (K, poly)
    int cus;
};

// Weak references, as td_ratematch.h's: a host-only link of td_api.cpp that leaves td_encode.hip out still
// links, and the entry points then fail with TD_EHIP instead of launching.
__attribute__((weak)) hipError_t launch_encode(const EncParams& p, hipStream_t st);
// in place: bits K-24 .. K-1 of every row of d_bits [B][K] become the CRC of the bits before them
__attribute__((weak)) hipError_t launch_crc_attach(const CrcParams& p, uint8_t* d_bits, hipStream_t st);
// d_rem[b] = the remainder of row b
__attribute__((weak)) hipError_t launch_crc_check(const CrcParams& p, const uint8_t* d_bits, uint32_t* d_rem,
                                                  hipStream_t st);

}  // namespace td
