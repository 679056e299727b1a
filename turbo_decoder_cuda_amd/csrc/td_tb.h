// td_tb.h -- the launchers of td_tb.hip: transport-block segmentation, rate matching of a transport block's
// code blocks into one concatenated row, its transpose, and the reassembly (td_tb_segment, td_tb_rate_match,
// td_tb_rate_dematch, td_tb_concat).  Plan, layout and index arithmetic: td_tb_core.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "td_tb_core.h"

namespace td {

// One class of code blocks' circular-buffer tables (td_ratematch.h), device pointers.  A transport block has
// up to four: size K_minus or K_plus, with the filler's <NULL>s (its block 0) or without.
struct TbRmClass {
    int K, R, ND, Nnn, c0;   // c0 of the launch's rv
    const int32_t* rank;     // [3K+12]
    const int32_t* pos;      // [Nnn]
};

// One launch's view of a td_tb (device pointers).
struct TbTables {
    tb::Plan plan;
    const uint32_t* syn_a;        // [B] gCRC24A syndromes of the B-bit sequence (td_crc.h)
    const uint32_t* syn_b[2];     // [K_minus], [K_plus] gCRC24B syndromes (null: no such block, or C = 1)
    TbRmClass cls[2][2];          // [K_plus?][filler?]; set for td_tb_rate_match / td_tb_rate_dematch only
    int cus;                      // compute units of the device (sizes the grids)
};

// Weak references, as td_ratematch.h's: a host-only link of td_api.cpp that leaves td_tb.hip out still links,
// and the entry points then fail with TD_EHIP instead of launching.
// d_tb [N][A] -> d_cb_minus [C_minus][N][K_minus], d_cb_plus [C_plus][N][K_plus]
__attribute__((weak)) hipError_t launch_tb_segment(const TbTables& t, const uint8_t* d_tb, int N, uint8_t* d_cb_minus,
                                                   uint8_t* d_cb_plus, hipStream_t st);
// coded rows [..][N][3K+12] -> d_f [N][G]
__attribute__((weak)) hipError_t launch_tb_rate_match(const TbTables& t, const tb::RmSizes& sz, long long G,
                                                      const uint8_t* d_coded_minus, const uint8_t* d_coded_plus, int N,
                                                      uint8_t* d_f, hipStream_t st);
// d_f [N][G] -> soft buffers [..][N][3K+12]; `filler` goes to d0 and d1 of block 0's filler bits
template <typename T>
__attribute__((weak)) hipError_t launch_tb_rate_dematch(const TbTables& t, const tb::RmSizes& sz, long long G, const T* d_f,
                                                        int N, T* d_llr_minus, T* d_llr_plus, T filler, int accumulate,
                                                        hipStream_t st);
// td_tb_demod_dematch's received symbols: yi, yq [N][G / M]; seq [N][(G + 31) / 32] words of the scrambling
// sequence, or null
struct TbDemodArgs {
    const double* yi;
    const double* yq;
    const uint32_t* seq;
    int M;   // 1, 2, 3, 4 or 6; else hipErrorInvalidValue
    double Kf, steps_per_unit;
};
// symbols -> soft buffers [..][N][3K+12]: launch_tb_rate_dematch of the demapped, descrambled, converted values
template <typename T>
__attribute__((weak)) hipError_t launch_tb_demod_dematch(const TbTables& t, const tb::RmSizes& sz, long long G,
                                                         const TbDemodArgs& a, int N, T* d_llr_minus, T* d_llr_plus, T filler,
                                                         int accumulate, hipStream_t st);
// hard decisions [..][N][K] -> d_tb [N][A], d_cb_rem [N][C] (or null), d_tb_rem [N] (or null)
__attribute__((weak)) hipError_t launch_tb_concat(const TbTables& t, const uint8_t* d_bits_minus, const uint8_t* d_bits_plus,
                                                  int N, uint8_t* d_tb, uint32_t* d_cb_rem, uint32_t* d_tb_rem, hipStream_t st);

}  // namespace td
