// td_scramble.hip -- the scrambling sequence of 36.211 7.2 on the device (td_gold_sequence) and its two uses as
// calls of their own: td_scramble (bits) and td_descramble_llr (soft values).  Registers, step, jump and the
// tables: td_gold_core.h.  The transport-block receive front end applies the sequence where it demaps
// (td_tb.hip, tb_demod_dematch_kernel) and needs neither of the two.
//
//   gold_kernel      a thread a run of kGoldRun bits of a row: both registers jump to 1600 + kGoldRun t (x1's
//                    state is the same for every row, so it is found once and kept for the thread's rows; x2's
//                    is the jump applied to the row's c_init), then step 32 positions a time.  A thread's 32
//                    words are consecutive in its row, so they go through LDS (pitch 33) and leave with the
//                    lanes on consecutive words.  A workgroup is runs x rows, the runs a power of two: a short
//                    sequence fills the workgroup with rows instead of idle threads.
//   scramble_kernel  an element a thread; the lanes of a wave read one or two sequence words between them.
//                    Byte rows that are 4-byte aligned, with len a multiple of 4, go four bytes a thread.
// Every other access is one element wide: data pointers need only element alignment.
#include <hip/hip_runtime.h>

#include "td_gold_core.h"
#include "td_scramble.h"

namespace td {

namespace {

using namespace gold;

constexpr int kGoldThreads = 256;
constexpr unsigned kGoldGridY = 256;   // row groups: crossed by tests/test_gpu_scramble.py (N = 257 at 148 runs)
constexpr int kGoldPitch = kGoldRunWords + 1;

__constant__ GoldTables kGoldDev = {make_jump<false>(), make_jump<true>()};

// log2_runs: the workgroup is (1 << log2_runs) runs by (kGoldThreads >> log2_runs) rows
__global__ __launch_bounds__(kGoldThreads) void gold_kernel(const uint32_t* __restrict__ cinit, int N, long long len,
                                                             long long W, int log2_runs, uint32_t* __restrict__ seq)
{
    __shared__ uint32_t tile[kGoldThreads * kGoldPitch];
    const int tid = threadIdx.x;
    const unsigned runs = 1u << log2_runs, rows = (unsigned)kGoldThreads >> log2_runs;
    const unsigned tx = (unsigned)tid & (runs - 1), ty = (unsigned)tid >> log2_runs;
    const long long nruns = (W + kGoldRunWords - 1) / kGoldRunWords;
    const long long t = (long long)blockIdx.x * runs + tx;
    const bool live = t < nruns;
    const uint32_t s1_0 = live ? gold_jump(kGoldDev.x1, 1u, (uint32_t)t) : 0u;
    for (size_t n0 = (size_t)blockIdx.y * rows; n0 < (size_t)N; n0 += (size_t)gridDim.y * rows) {
        const size_t n = n0 + ty;
        if (live && n < (size_t)N) {
            uint32_t s1 = s1_0, s2 = gold_jump(kGoldDev.x2, cinit[n], (uint32_t)t);
#pragma unroll 4
            for (int k = 0; k < kGoldRunWords; ++k) tile[tid * kGoldPitch + k] = gold_step32<false>(s1) ^ gold_step32<true>(s2);
        }
        __syncthreads();
        // slot i / 32 = the thread that made the word: consecutive i are consecutive words of one row
        for (int i = tid; i < kGoldThreads * kGoldRunWords; i += kGoldThreads) {
            const unsigned slot = (unsigned)i / kGoldRunWords, k = (unsigned)i % kGoldRunWords;
            const size_t row = n0 + (slot >> log2_runs);
            const long long w = ((long long)blockIdx.x * runs + (slot & (runs - 1))) * kGoldRunWords + k;
            if (row < (size_t)N && w < W) seq[row * (size_t)W + (size_t)w] = tile[slot * kGoldPitch + k] & gold_tail_mask(len, w);
        }
        __syncthreads();
    }
}

constexpr int kScrThreads = 256;
constexpr unsigned kScrGridX = 4096, kScrGridY = 4096;

// U = uint64_t / uint32_t (the bits of a double / float) or uint8_t (int8): out = in with the sign flipped where c = 1
template <typename U>
struct FlipOp {
    __device__ __forceinline__ U operator()(U v, uint32_t c) const { return flip_bits(v, c); }
};
struct BitOp {
    __device__ __forceinline__ uint8_t operator()(uint8_t v, uint32_t c) const { return scramble_bit(v, c); }
};

// V = 1: an element a thread.  V = 4 (U = uint8_t only): four bytes a thread, one 4-byte access.
template <typename U, int V, typename Op>
__global__ __launch_bounds__(kScrThreads) void scramble_kernel(const U* in, const uint32_t* __restrict__ seq, int N,
                                                               long long len, long long W, U* out, Op op)
{
    const long long step = (long long)gridDim.x * kScrThreads * V;
    for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) {
        const U* ib = in + n * (size_t)len;
        U* ob = out + n * (size_t)len;
        const uint32_t* sb = seq + n * (size_t)W;
        for (long long g = ((long long)blockIdx.x * kScrThreads + threadIdx.x) * V; g < len; g += step) {
            if constexpr (V == 1) {
                ob[g] = op(ib[g], gold_bit(sb, g));
            } else {   // g % 4 = 0: the four bits lie in one word
                const uint32_t c = sb[g >> 5] >> (int)(g & 31), v = *reinterpret_cast<const uint32_t*>(ib + g);
                uint32_t r = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) r |= (uint32_t)op((uint8_t)(v >> (8 * j)), (c >> j) & 1u) << (8 * j);
                *reinterpret_cast<uint32_t*>(ob + g) = r;
            }
        }
    }
}

template <typename U, typename Op>
hipError_t launch_elements(const void* in, const uint32_t* seq, int N, long long len, void* out, hipStream_t st)
{
    const long long W = (len + 31) / 32;
    bool quad = false;
    if constexpr (sizeof(U) == 1)
        quad = len % 4 == 0 && (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 4 == 0;
    const long long per = (long long)kScrThreads * (quad ? 4 : 1), need = (len + per - 1) / per;
    const dim3 grid((unsigned)(need < kScrGridX ? need : kScrGridX), (unsigned)N < kScrGridY ? (unsigned)N : kScrGridY);
    if constexpr (sizeof(U) == 1) {
        if (quad) {
            hipLaunchKernelGGL((scramble_kernel<U, 4, Op>), grid, dim3(kScrThreads), 0, st, static_cast<const U*>(in), seq, N, len,
                               W, static_cast<U*>(out), Op{});
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((scramble_kernel<U, 1, Op>), grid, dim3(kScrThreads), 0, st, static_cast<const U*>(in), seq, N, len, W,
                       static_cast<U*>(out), Op{});
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gold_sequence(const uint32_t* d_cinit, int N, long long len, uint32_t* d_seq, hipStream_t st)
{
    const long long W = (len + 31) / 32, nruns = (W + kGoldRunWords - 1) / kGoldRunWords;
    int log2_runs = 0;
    while ((1 << log2_runs) < kGoldThreads && (1ll << log2_runs) < nruns) ++log2_runs;
    const long long runs = 1ll << log2_runs, rows = kGoldThreads >> log2_runs;
    const long long gy = ((long long)N + rows - 1) / rows;
    const dim3 grid((unsigned)((nruns + runs - 1) / runs), (unsigned)(gy < kGoldGridY ? gy : kGoldGridY));
    hipLaunchKernelGGL(gold_kernel, grid, dim3(kGoldThreads), 0, st, d_cinit, N, len, W, log2_runs, d_seq);
    return hipGetLastError();
}

hipError_t launch_scramble(const uint8_t* d_in, const uint32_t* d_seq, int N, long long len, uint8_t* d_out, hipStream_t st)
{
    return launch_elements<uint8_t, BitOp>(d_in, d_seq, N, len, d_out, st);
}

hipError_t launch_descramble_llr(const void* d_in, int elem_size, const uint32_t* d_seq, int N, long long len, void* d_out,
                                 hipStream_t st)
{
    switch (elem_size) {
        case 8: return launch_elements<uint64_t, FlipOp<uint64_t>>(d_in, d_seq, N, len, d_out, st);
        case 4: return launch_elements<uint32_t, FlipOp<uint32_t>>(d_in, d_seq, N, len, d_out, st);
        case 1: return launch_elements<uint8_t, FlipOp<uint8_t>>(d_in, d_seq, N, len, d_out, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace td
