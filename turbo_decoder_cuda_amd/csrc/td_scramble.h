// td_scramble.h -- the launchers of td_scramble.hip: the scrambling sequence of 36.211 7.2 (td_gold_sequence) and
// its application to bits and to soft values (td_scramble, td_descramble_llr).  Registers and jump: td_gold_core.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace td {

// Weak references, as td_tb.h's: a host-only link of td_api.cpp that leaves td_scramble.hip out still links, and
// the entry points then fail with TD_EHIP instead of launching.  N >= 1, 1 <= len < 2^31.
// d_cinit [N] -> d_seq [N][(len + 31) / 32]
__attribute__((weak)) hipError_t launch_gold_sequence(const uint32_t* d_cinit, int N, long long len, uint32_t* d_seq,
                                                      hipStream_t st);
// d_in, d_out [N][len] bytes; d_out may be d_in
__attribute__((weak)) hipError_t launch_scramble(const uint8_t* d_in, const uint32_t* d_seq, int N, long long len,
                                                 uint8_t* d_out, hipStream_t st);
// d_in, d_out [N][len] of elem_size 8 (double), 4 (float) or 1 (int8); else hipErrorInvalidValue
__attribute__((weak)) hipError_t launch_descramble_llr(const void* d_in, int elem_size, const uint32_t* d_seq, int N,
                                                       long long len, void* d_out, hipStream_t st);

}  // namespace td
