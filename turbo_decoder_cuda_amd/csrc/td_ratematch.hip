// td_ratematch.hip -- LTE rate matching (36.212 5.1.4.1) on the device: the transmit-side bit
// selection (rate_match_kernel, a gather) and the receive-side soft de-rate-matching with repetition
// combining and HARQ accumulation (rate_dematch_kernel), also fused behind the demapper and the LLR conversion
// (demod_dematch_kernel: td_demod_dematch, symbols in, soft buffer out).  Tables and notation: td_ratematch.h.
#include <hip/hip_runtime.h>

#include "td_demap_core.h"
#include "td_ratematch.h"

namespace td {

namespace {

constexpr int kRmThreads = 256;

// e[b][k] = in[b][pos[(c0 + k) mod Nnn]]: one selected element per thread, consecutive lanes write
// consecutive e; the codewords of one grid column share the thread's table entry.
template <typename T>
__global__ __launch_bounds__(kRmThreads) void rate_match_kernel(RmParams p, const T* __restrict__ in, T* __restrict__ e)
{
    const size_t k = (size_t)blockIdx.x * kRmThreads + threadIdx.x;
    if (k >= (size_t)p.E) return;
    const int src = p.pos[(k + (size_t)p.c0) % (size_t)p.Nnn];
    const size_t n = 3 * (size_t)p.K + 12;
    for (size_t b = blockIdx.y; b < (size_t)p.B; b += gridDim.y) e[b * (size_t)p.E + k] = in[b * n + src];
}

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
template <typename T, bool ACC, int kRows, typename Src>
__device__ __forceinline__ void dematch_band(const RmParams& p, const Src& src, T* out)
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
            if (q >= 0 && q < nout) ob[q] = buf[(x / 96) * kPitch + x % 96];
        }
    }
}

template <typename T, bool ACC, int kRows>
__global__ __launch_bounds__(kRmThreads) void rate_dematch_kernel(RmParams p, const T* __restrict__ e, T* out)
{
    dematch_band<T, ACC, kRows>(p, ArraySrc<T>{e, (size_t)p.E}, out);
}

// td_demod_dematch: d_yi, d_yq [B][E / M] -> out [B][3K+12] in one pass; T = double, float or int8_t
template <int M, typename T, bool ACC, int kRows>
__global__ __launch_bounds__(kRmThreads) void demod_dematch_kernel(RmParams p, const double* __restrict__ yi,
                                                                    const double* __restrict__ yq, double Kf,
                                                                    double steps_per_unit, T* out)
{
    dematch_band<T, ACC, kRows>(p, DemapSrc<M, T>{yi, yq, (size_t)(p.E / M), Kf, steps_per_unit}, out);
}

constexpr int kRmRows = 16;
// crossed by tests/test_gpu_ratematch_batches.py test_rate_dematch_past_the_grid_cap (B = 513, 1100, 1537)
constexpr unsigned kRmGridY = 512;   // codewords beyond it share a workgroup (and its table reads)

template <typename T>
hipError_t launch_match_t(const RmParams& p, const void* in, void* e, hipStream_t st)
{
    // 65535: crossed by tests/test_gpu_ratematch_batches.py test_rate_match_past_the_grid_cap (B = 65600)
    const dim3 grid((unsigned)(((size_t)p.E + kRmThreads - 1) / kRmThreads), (unsigned)(p.B < 65535 ? p.B : 65535));
    hipLaunchKernelGGL(rate_match_kernel<T>, grid, dim3(kRmThreads), 0, st, p, static_cast<const T*>(in),
                       static_cast<T*>(e));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rate_match(const RmParams& p, const void* d_in, int elem, void* d_e, hipStream_t st)
{
    switch (elem) {
        case 1: return launch_match_t<uint8_t>(p, d_in, d_e, st);
        case 4: return launch_match_t<uint32_t>(p, d_in, d_e, st);
        case 8: return launch_match_t<uint64_t>(p, d_in, d_e, st);
        default: return hipErrorInvalidValue;
    }
}

template <typename T>
hipError_t launch_rate_dematch(const RmParams& p, const T* d_e, T* d_out, int accumulate, hipStream_t st)
{
    const dim3 grid((unsigned)((p.R + kRmRows - 1) / kRmRows), (unsigned)p.B < kRmGridY ? (unsigned)p.B : kRmGridY);
    if (accumulate)
        hipLaunchKernelGGL((rate_dematch_kernel<T, true, kRmRows>), grid, dim3(kRmThreads), 0, st, p, d_e, d_out);
    else
        hipLaunchKernelGGL((rate_dematch_kernel<T, false, kRmRows>), grid, dim3(kRmThreads), 0, st, p, d_e, d_out);
    return hipGetLastError();
}

template <int M, typename T>
static hipError_t launch_demod_dematch_m(const RmParams& p, const double* yi, const double* yq, double Kf,
                                         double steps_per_unit, T* d_out, int accumulate, hipStream_t st)
{
    // td_rate_dematch's grid, cap included (crossed by tests/test_gpu_frontend.py test_demod_dematch_past_the_grid_cap)
    const dim3 grid((unsigned)((p.R + kRmRows - 1) / kRmRows), (unsigned)p.B < kRmGridY ? (unsigned)p.B : kRmGridY);
    if (accumulate)
        hipLaunchKernelGGL((demod_dematch_kernel<M, T, true, kRmRows>), grid, dim3(kRmThreads), 0, st, p, yi, yq, Kf, steps_per_unit,
                           d_out);
    else
        hipLaunchKernelGGL((demod_dematch_kernel<M, T, false, kRmRows>), grid, dim3(kRmThreads), 0, st, p, yi, yq, Kf, steps_per_unit,
                           d_out);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_demod_dematch(const RmParams& p, const double* d_yi, const double* d_yq, int M, double Kf,
                                double steps_per_unit, T* d_out, int accumulate, hipStream_t st)
{
    switch (M) {
        case 1: return launch_demod_dematch_m<1>(p, d_yi, d_yq, Kf, steps_per_unit, d_out, accumulate, st);
        case 2: return launch_demod_dematch_m<2>(p, d_yi, d_yq, Kf, steps_per_unit, d_out, accumulate, st);
        case 3: return launch_demod_dematch_m<3>(p, d_yi, d_yq, Kf, steps_per_unit, d_out, accumulate, st);
        case 4: return launch_demod_dematch_m<4>(p, d_yi, d_yq, Kf, steps_per_unit, d_out, accumulate, st);
        case 6: return launch_demod_dematch_m<6>(p, d_yi, d_yq, Kf, steps_per_unit, d_out, accumulate, st);
        default: return hipErrorInvalidValue;
    }
}

template hipError_t launch_demod_dematch<double>(const RmParams&, const double*, const double*, int, double, double,
                                                 double*, int, hipStream_t);
template hipError_t launch_demod_dematch<float>(const RmParams&, const double*, const double*, int, double, double, float*,
                                                int, hipStream_t);
template hipError_t launch_demod_dematch<int8_t>(const RmParams&, const double*, const double*, int, double, double,
                                                 int8_t*, int, hipStream_t);
template hipError_t launch_rate_dematch<double>(const RmParams&, const double*, double*, int, hipStream_t);
template hipError_t launch_rate_dematch<float>(const RmParams&, const float*, float*, int, hipStream_t);

}  // namespace td
