// td_dematch_band.h -- the body of the soft de-rate-matching kernels (device code): one band of one code
// block's circular buffer, summed and written in stream order.  td_ratematch.hip wraps it for td_rate_dematch
// and td_demod_dematch, td_tb.hip for td_tb_rate_dematch (a transport block's blocks, each with its own
// tables and its own piece of the concatenated row).  Tables and notation: td_ratematch.h.
#pragma once

#include <hip/hip_runtime.h>

#include "td_demap_core.h"
#include "td_ratematch.h"

namespace td {
namespace band {

constexpr int kRmThreads = 256;

// One addition of a position's sum: in the buffer's precision; int8 (td_demod_dematch on a TD_FIXED handle)
// saturates to +-127 and reads a prior -128 as -127.  A position nothing selects is never added to.
template <typename T>
__device__ __forceinline__ T sum_add(T acc, T v)
{
    return acc + v;
}
__device__ __forceinline__ int8_t sum_add(int8_t acc, int8_t v)
{
    const int a = (acc < -127 ? -127 : acc) + v;
    return (int8_t)(a > 127 ? 127 : a < -127 ? -127 : a);
}

// What leaves for stream position q in place of its sum v: nothing but v for a code block of its own ...
struct NoFill {
    template <typename T>
    __device__ __forceinline__ T operator()(int, T v) const
    {
        return v;
    }
};
// ... and the known value of a filler bit at d0 and d1 of a transport block's first F bits (36.212 5.1.2):
// stream positions 3k and 3k+1, k < F, which the block's tables hold as <NULL>.
template <typename T>
struct FillerFill {
    int F;
    T value;
    __device__ __forceinline__ T operator()(int q, T v) const { return q < 3 * F && q % 3 != 2 ? value : v; }
};

// De-rate-matching.  Stream position q = 3k+i sits in row (ND+k) / 32, column (ND+k) % 32 of its
// stream's 32-column matrix, and the buffer reads that matrix column by column: consecutive q are
// consecutive columns, R elements apart in e (2R in the parity part).  One thread per q in stream
// order would make every wave load touch 64 different 128-byte lines.
//
// So a workgroup owns a band of kRows rows -- 96 kRows consecutive stream positions -- of one codeword
// at a time.  In the buffer that band is 32 runs of kRows consecutive systematic entries and 32 runs of
// 2 kRows consecutive parity entries (stream 1 and stream 2 alternating; stream 2's run is the one of
// the column to its left, which the rank table folds in).  The threads walk the band in that buffer
// order: the lanes' loads of e are consecutive within a run, a wave's load touches 2 to 4 runs, and
// every line is used up by this workgroup in one pass.  Each sum goes to LDS at its stream position
// (row pitch 97: the lanes of a run are one row apart, 96 would put them all on one bank), and after a
// barrier the band leaves in stream order: every wave stores one contiguous piece of d_llr.
//
// All accesses are one element wide (8, 4 or 1 bytes), so rows of e or d_llr that are only
// element-aligned (odd E or odd K with B > 1) take the same path as aligned ones.
//
// The sum of a position is formed by its one owning thread, in ascending k, starting from the prior
// value (accumulate) or +0.0: no atomics, the same bits on every run.
//
// Where e comes from is the body's one parameter: src.row(b)[k] is e[b][k] -- td_rate_dematch's array
// (rate_dematch_kernel), or td_demod_dematch's symbols, demapped and converted where the array would be
// read (demod_dematch_kernel; td_demap_core.h).  There a run of consecutive k is a run of consecutive
// symbols, M values each, so a wave's loads of symbols are as contiguous as its loads of e are.  The int8
// front end (a TD_FIXED handle) takes this layout too, with sum_add's saturating addition: one thread per
// stream position, td_rate_dematch's own int8 kernel (td_fixed.hip), has every lane fetch a 16-byte symbol
// from a line of its own and measured 2.9 - 6.1 x slower at B = 32768 (DESIGN.md "Receive front end").
//
// The band is blockIdx.x's, the codewords blockIdx.y's (grid-stride); `fill` has the last word on what is
// stored (NoFill: the sum).
template <typename T, bool ACC, int kRows, typename Src, typename Fill = NoFill>
__device__ __forceinline__ void dematch_band(const RmParams& p, const Src& src, T* out, const Fill& fill = Fill{})
{
    constexpr int kTile = 96 * kRows, kPitch = 97, kPer = kTile / kRmThreads;
    static_assert(kTile % kRmThreads == 0, "whole passes over the band");
    __shared__ T tile[2][kRows * kPitch];

    const int r0 = blockIdx.x * kRows;
    const int nout = 3 * p.K + 12;
    const int q0 = 3 * (32 * r0 - p.ND);   // stream position of the band's first matrix entry (< 0: <NULL>s)

    // this thread's elements in buffer order: LDS slot, and the first k that selects it (-1: none)
    int slot[kPer], first[kPer];
#pragma unroll
    for (int n = 0; n < kPer; ++n) {
        const int t = n * kRmThreads + threadIdx.x;
        int pc, roff, i;
        if (t < 32 * kRows) {                  // systematic part: runs of kRows
            pc = t / kRows, roff = t % kRows, i = 0;
        } else {                               // parity part: runs of 2 kRows, streams 1 and 2 alternating
            const int u = t - 32 * kRows;
            pc = u / (2 * kRows), roff = (u % (2 * kRows)) >> 1, i = 1 + (u & 1);
        }
        int c = (int)(__builtin_bitreverse32((unsigned)pc) >> 27);   // kRmPerm[pc]
        if (i == 2) c = (c + 1) & 31;
        const int k = 32 * (r0 + roff) + c - p.ND;
        slot[n] = roff * kPitch + 3 * c + i;
        first[n] = -1;
        if (r0 + roff < p.R && k >= 0) {
            const int rk = p.rank[3 * k + i];
            if (rk >= 0) first[n] = rk >= p.c0 ? rk - p.c0 : rk - p.c0 + p.Nnn;
        }
    }

    int it = 0;
    for (size_t b = blockIdx.y; b < (size_t)p.B; b += gridDim.y, ++it) {
        T* buf = tile[it & 1];   // two tiles: one barrier separates a codeword's stores from the next one's sums
        const auto eb = src.row(b);
        T* ob = out + b * (size_t)nout;
        if constexpr (ACC) {
#pragma unroll
            for (int n = 0; n < kPer; ++n) {
                const int x = n * kRmThreads + threadIdx.x, q = q0 + x;
                if (q >= 0 && q < nout) buf[(x / 96) * kPitch + x % 96] = ob[q];
            }
            __syncthreads();
        }
        // the first selection of every element first (independent loads, all in flight together), then
        // the repetitions, which only E > Nnn has
        T v[kPer];
#pragma unroll
        for (int n = 0; n < kPer; ++n) v[n] = first[n] >= 0 && first[n] < p.E ? eb[first[n]] : T(0);
#pragma unroll
        for (int n = 0; n < kPer; ++n) {
            T acc = T(0);
            if constexpr (ACC) acc = buf[slot[n]];
            if (first[n] >= 0 && first[n] < p.E) {
                acc = sum_add(acc, v[n]);
                for (size_t k = (size_t)first[n] + (size_t)p.Nnn; k < (size_t)p.E; k += (size_t)p.Nnn) acc = sum_add(acc, eb[k]);
            }
            buf[slot[n]] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < kPer; ++n) {
            const int x = n * kRmThreads + threadIdx.x, q = q0 + x;
            if (q >= 0 && q < nout) ob[q] = fill(q, buf[(x / 96) * kPitch + x % 96]);
        }
    }
}

}  // namespace band
}  // namespace td
