// td_fixed.h -- launchers of the fixed-point decoder (TD_FIXED, td_fixed.hip) and its workspace carve.
//
// One lane decodes one codeword; every workspace array is [row][Bp] with the codeword as the fastest
// index (Bp = B rounded up to kFxLanes), so that a wave's accesses to a row are contiguous.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "td_fixed_core.h"
#include "td_ratematch.h"

namespace td {

constexpr int kFxLanes = 64;   // codewords of a wave = of a workgroup

struct FxCarve {
    size_t xs, xp1, xp2, ext12, ext21, ckpt, bitsT, used, ev, hist, total;
    size_t Bp;
};

inline FxCarve fx_carve(int B, int K, int iters)
{
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t L = (size_t)K + 3, Bp = ((size_t)B + kFxLanes - 1) / kFxLanes * kFxLanes;
    const size_t nW = (L + fx::kW - 1) / fx::kW;
    FxCarve c{};
    c.Bp = Bp;
    c.xs = 0;
    c.xp1 = c.xs + up((L + 3) * Bp);
    c.xp2 = c.xp1 + up(L * Bp);
    c.ext12 = c.xp2 + up(L * Bp);
    c.ext21 = c.ext12 + up((size_t)K * Bp * 2);
    c.ckpt = c.ext21 + up((size_t)K * Bp * 2);
    c.bitsT = c.ckpt + up(nW * 8 * Bp * 4);
    c.used = c.bitsT + up((size_t)iters * K * Bp);   // a row per iteration (all_iters, early termination)
    c.ev = c.used + up(Bp * 4);                      // int32 [Bp]: iterations used (td_set_fixed_stop), always carved
    // uint32 [nW][Bp]: a word of evidence per sub-block and codeword (td_set_fixed_window_stop); nW bounds the
    // sub-blocks of every allowed window (>= kW).  Then uint16 [nW][Bp]: the rule's HDA form keeps the sixteen
    // decisions of every 16-step window packed for the next iteration's comparison.  Both are always carved, so
    // that td_reserve does not depend on the rule: 6 B per 16 positions and codeword, 2.2 % of the workspace at
    // K = 6144 and 8 iterations.
    c.hist = c.ev + up(nW * Bp * 4);
    c.total = c.hist + up(nW * Bp * 2);
    return c;
}

// The state of next-iteration initialisation (td_set_fixed_window_nii) follows the carve, and only while NII is
// on: a handle that never turns it on keeps fx_carve's workspace byte for byte.  It is sized for the
// current window's sub-blocks: 128 B per sub-block and codeword (two parities, two SISOs, alpha and beta,
// eight int16), 12 % more at K = 6144, {64, g} and 8 iterations.
inline size_t fx_nii_bytes(int B, int K, int window)
{
    const size_t Bp = ((size_t)B + kFxLanes - 1) / kFxLanes * kFxLanes;
    return (fx::nii_words(K + 3, window, Bp) * 4 + 255) / 256 * 256;
}

// Weak references, like td_ratematch.h's: a host-only link of td_api.cpp without td_fixed.hip still
// links, and the fixed entry points then fail with TD_EHIP.  libturbo_mi355x.so always has them.
// d_q [B][3K+12] int8 -> xs / xp1 / xp2 of the workspace (-128 read as -127, the padding zeroed)
__attribute__((weak)) hipError_t launch_fixed_demux(const fx::FxArgs& p, const int8_t* d_q, hipStream_t st);
// One decode on st, then bitsT -> d_bits ([B][K] or [B][iters][K]).  The optional parts are nullable:
//   w       the sub-block schedule (td_set_fixed_window): a launch per SISO and iteration, grid (Bp / kFxLanes) x
//           sub-blocks; null: the exact schedule, all iterations of all codewords in one launch
//   s       early termination (td_set_fixed_stop / td_set_fixed_window_stop): a codeword's rows past its stop are
//           copies of its stop row, d_bits without all_iters is its stop row, and d_iters (nullable, [B]) gets
//           s->used; on the sub-block schedule s->used is reset on st, every iteration ends with the judge's
//           launch, and d_ev and d_hist are the carve's ev and hist.  null: no rule, d_iters is not written
//   m       td_set_fixed_maxstar's table: the kernels instantiated with fx::MaxStar; null: Max-Log-MAP
//   d_nii   the state of td_set_fixed_window_nii (fx::nii_words words, right after the carve's total); null: off
// A part that is null launches the kernels without it.
__attribute__((weak)) hipError_t launch_fixed_decode(const fx::FxArgs& p, const fx::FxWindow* w, const fx::FxStop* s,
                                                     const fx::MaxStar* m, uint32_t* d_ev, uint16_t* d_hist,
                                                     uint32_t* d_nii, uint8_t* d_bits, int32_t* d_iters, hipStream_t st);
// saturating int8 de-rate-matching: d_e [B][E] -> d_out [B][3K+12]
__attribute__((weak)) hipError_t launch_fixed_dematch(const RmParams& p, const int8_t* d_e, int8_t* d_out,
                                                      int accumulate, hipStream_t st);

}  // namespace td
