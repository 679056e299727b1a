// td_fixed.hip -- the fixed-point decoder (TD_FIXED) on gfx950: int8 channel LLRs in, integer
// Max-Log-MAP (or, with td_set_fixed_maxstar's table, integer log-MAP), int16 extrinsics, uint8 decisions.
// The arithmetic is td_fixed_core.h's; here are the kernels around it.
//
//   fx_demux_kernel    q [B][3K+12] -> xs, xp1, xp2 [row][Bp]: a 64 x 64 byte transpose through LDS, so
//                      that both the reads (along the stream) and the writes (along the batch) are
//                      contiguous; -128 becomes -127 and the lanes of the padding get zeros.
//   fx_turbo_kernel<STOP, M>  the exact schedule: one codeword per lane, all iterations in one launch.  A
//                      lane keeps its eight state metrics in registers (int32, never normalised); the forward
//                      pass leaves alpha at every kW-th step in the workspace (32 B per kW steps and codeword),
//                      the backward pass recomputes a window's alpha rows into registers and runs beta,
//                      Lambda and the extrinsic over them.  The interleaver is a row index that the
//                      whole wave shares, so every access to the workspace is one contiguous row piece.
//                      STOP (td_set_fixed_stop): a lane whose codeword has stopped is skipped, a wave whose
//                      lanes have all stopped returns.
//   fx_window_siso_kernel<DEC, STOP, NII, M>  the sub-block schedule (td_set_fixed_window): one SISO of one
//                      iteration a launch, a wave = 64 codewords x one sub-block (blockIdx.y), the kernel
//                      boundary as the ordering between a SISO's extrinsic writes and the next SISO's reads.
//                      STOP (td_set_fixed_window_stop): used[b] is the state (0 = running), a wave with no
//                      running codeword returns, SISO2 leaves each sub-block's evidence in the workspace (and,
//                      for the next iteration's HDA comparison, every 16-step window's decisions packed).
//                      NII (td_set_fixed_window_nii): the state's two halves (read: the previous iteration's,
//                      written: this one's) are the kernel's FxNii.
//   fx_window_judge_kernel  a launch of its own after SISO2's of a stopping sub-block decode: folds the
//                      evidence and stops the codeword.
//   fx_bits_kernel     bitsT [rows][K][Bp] -> the caller's [B][rows][K], the transpose back.
//   fx_bits_stop_kernel  the same after a stopping decode: reads row min(row, used - 1) and undoes the
//                      interleaved order that the stopping decoders keep their decisions in.
//   fx_dematch_kernel  saturating int8 de-rate-matching, one thread per stream position.
//
// The two decoding templates are the lane code of td_fixed_core.h instantiated by the handle's settings: M is
// fx::MaxLog, or fx::MaxStar while td_set_fixed_maxstar's table is set.  Each has one argument list whatever
// the instantiation -- FxArgs, then the schedule's structs --, an argument that the instantiation does not use
// is passed zeroed and never read, and launch_fixed_decode picks the instantiation: a setting that is off
// launches the kernel without it.  The table's two words and its shift are kernel arguments (scalar
// registers) in every instantiation; MaxLog is built in the kernel.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "td_fixed.h"

namespace td {

namespace {

constexpr int kTile = 64;
constexpr int kTileThreads = 256;

__global__ __launch_bounds__(kTileThreads) void fx_demux_kernel(const int8_t* __restrict__ q, int K, int B, size_t Bp,
                                                                 int8_t* __restrict__ xs, int8_t* __restrict__ xp1,
                                                                 int8_t* __restrict__ xp2)
{
    __shared__ int8_t tile[kTile][kTile + 4];
    const int n = 3 * K + 12, L = K + 3;
    const int n0 = blockIdx.x * kTile;
    const size_t b0 = (size_t)blockIdx.y * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    for (int r = ty; r < kTile; r += kTileThreads / kTile) {
        int v = 0;
        if (b0 + r < (size_t)B && n0 + tx < n) v = q[(b0 + r) * (size_t)n + n0 + tx];
        tile[r][tx] = (int8_t)(v < -127 ? -127 : v);
    }
    __syncthreads();
    for (int c = ty; c < kTile; c += kTileThreads / kTile) {
        const int pos = n0 + c;
        if (pos >= n) break;
        int8_t* dst;
        int row;
        if (pos < 3 * K) {
            row = pos / 3;
            const int comp = pos - 3 * row;
            dst = comp == 0 ? xs : comp == 1 ? xp1 : xp2;
        } else {   // tails: (xs, xp) x 3 of the first encoder, then of the second (log_map.cpp:1119-1123)
            const int t = pos - 3 * K, second = t >= 6, u = second ? t - 6 : t;
            row = K + (u >> 1);
            if (u & 1)
                dst = second ? xp2 : xp1;
            else {
                dst = xs;
                if (second) row = L + (u >> 1);
            }
        }
        dst[(size_t)row * Bp + b0 + tx] = tile[tx][c];
    }
}

// the max of instantiation M: the table of the kernel's arguments, or the plain max
template <class M>
__device__ __forceinline__ M max_of(const fx::MaxStar& m)
{
    if constexpr (M::kTable)
        return m;
    else
        return M();
}

// The exact schedule.  STOP (td_set_fixed_stop): a wave ends once its 64 codewords have stopped.
template <bool STOP, class M>
__global__ __launch_bounds__(kFxLanes) void fx_turbo_kernel(fx::FxArgs p, fx::FxStop s, fx::MaxStar m)
{
    const size_t b = blockIdx.x * kFxLanes + threadIdx.x;
    if (STOP)
        fx::decode_codeword_stop(p, s, b, max_of<M>(m));
    else
        fx::decode_codeword(p, b, max_of<M>(m));
}

__global__ __launch_bounds__(kTileThreads) void fx_bits_kernel(const uint8_t* __restrict__ bitsT, int K, int B, size_t Bp,
                                                                int rows, uint8_t* __restrict__ bits)
{
    __shared__ uint8_t tile[kTile][kTile + 4];
    const int k0 = blockIdx.x * kTile, row = blockIdx.z;
    const size_t b0 = (size_t)blockIdx.y * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    for (int r = ty; r < kTile; r += kTileThreads / kTile)
        tile[r][tx] = k0 + r < K ? bitsT[((size_t)row * K + k0 + r) * Bp + b0 + tx] : (uint8_t)0;
    __syncthreads();
    for (int c = ty; c < kTile; c += kTileThreads / kTile) {
        const size_t b = b0 + c;
        if (b < (size_t)B && k0 + tx < K) bits[(b * rows + row) * (size_t)K + k0 + tx] = tile[tx][c];
    }
}

// fx_bits_kernel after a stopping decode: bitsT holds rows 0 .. used[b] - 1 of codeword b by interleaved
// position, and output row r is row min(r, used[b] - 1) -- the frozen rows -- or, without all_iters
// (rows == 1), the stop row.  Natural position k is workspace row pinv[k]: still one contiguous piece.
__global__ __launch_bounds__(kTileThreads) void fx_bits_stop_kernel(const uint8_t* __restrict__ bitsT,
                                                                     const int32_t* __restrict__ used,
                                                                     const int* __restrict__ pinv, int K, int B,
                                                                     size_t Bp, int rows, int iters,
                                                                     uint8_t* __restrict__ bits, int32_t* __restrict__ d_iters)
{
    __shared__ uint8_t tile[kTile][kTile + 4];
    const int k0 = blockIdx.x * kTile, row = blockIdx.z;
    const size_t b0 = (size_t)blockIdx.y * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    int n = iters;   // a lane of the padding has no rows: any row inside the workspace
    if (b0 + tx < (size_t)B) {
        n = used[b0 + tx];
        n = n < 1 ? 1 : n > iters ? iters : n;
        if (d_iters && blockIdx.x == 0 && row == 0 && ty == 0) d_iters[b0 + tx] = n;
    }
    const int src = rows == 1 ? n - 1 : row < n - 1 ? row : n - 1;
    for (int r = ty; r < kTile; r += kTileThreads / kTile)
        tile[r][tx] = k0 + r < K ? bitsT[((size_t)src * K + pinv[k0 + r]) * Bp + b0 + tx] : (uint8_t)0;
    __syncthreads();
    for (int c = ty; c < kTile; c += kTileThreads / kTile) {
        const size_t b = b0 + c;
        if (b < (size_t)B && k0 + tx < K) bits[(b * rows + row) * (size_t)K + k0 + tx] = tile[tx][c];
    }
}

// The sub-block schedule: SISO `DEC` of iteration `it`, sub-block blockIdx.y of the wave's 64 codewords.
// The sub-block index is the block's, so the interleaver entries stay scalar loads and every row access one
// contiguous piece.  SISO1 reads ext21 and writes ext12, SISO2 the reverse (and bitsT): no launch
// reads an array that it writes, apart from a sub-block's own checkpoint slots.
// STOP (td_set_fixed_window_stop), on the same grid: a wave whose 64 codewords have all stopped returns at
// once, and SISO2 leaves the sub-block's evidence at ev[blockIdx.y][b].  NII (td_set_fixed_window_nii): n, the
// same in every lane.
template <int DEC, bool STOP, bool NII, class M>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_kernel(fx::FxArgs p, fx::FxWindow w, fx::FxStop s,
                                                                   fx::MaxStar m, fx::FxNii n,
                                                                   uint32_t* __restrict__ ev,
                                                                   uint16_t* __restrict__ hist, int it)
{
    fx::siso_window_pass<DEC, STOP, NII>(p, w, s, ev, hist, n, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y,
                                         max_of<M>(m));
}

// One thread per codeword after SISO2's launch of iteration `it`: folds the sub-blocks' evidence and
// sets used[b] where the codeword stops.  The kernel boundaries order it after the stores of ev and
// before the next launch's reads of used.
__global__ __launch_bounds__(kTileThreads) void fx_window_judge_kernel(fx::FxArgs p, fx::FxStop s,
                                                                       const uint32_t* __restrict__ ev, int nS, int it)
{
    fx::window_judge(p, s, ev, nS, (size_t)blockIdx.x * kTileThreads + threadIdx.x, it);
}

// The owner of stream position q adds its e in ascending k, saturating to [-127, 127] after every
// addition: no atomics, the same bytes on every run.
template <bool ACC>
__global__ __launch_bounds__(kTileThreads) void fx_dematch_kernel(RmParams p, const int8_t* __restrict__ e, int8_t* out)
{
    const int nout = 3 * p.K + 12;
    const int q = blockIdx.x * kTileThreads + threadIdx.x;
    if (q >= nout) return;
    const int rk = p.rank[q];
    int first = -1;
    if (rk >= 0) first = rk >= p.c0 ? rk - p.c0 : rk - p.c0 + p.Nnn;
    const bool sel = first >= 0 && first < p.E;
    if (ACC && !sel) return;   // not selected: the soft buffer keeps its value
    for (size_t b = blockIdx.y; b < (size_t)p.B; b += gridDim.y) {
        int acc = 0;
        if (ACC) {
            acc = out[b * (size_t)nout + q];
            acc = acc < -127 ? -127 : acc;
        }
        if (sel) {
            const int8_t* eb = e + b * (size_t)p.E;
            for (size_t k = (size_t)first; k < (size_t)p.E; k += (size_t)p.Nnn) {
                acc += eb[k];
                acc = acc > 127 ? 127 : acc < -127 ? -127 : acc;
            }
        }
        out[b * (size_t)nout + q] = (int8_t)acc;
    }
}

// A runtime flag as a compile-time one: f(std::true_type()) or f(std::false_type()).
template <class F>
void with_flag(bool v, F&& f)
{
    if (v)
        f(std::true_type());
    else
        f(std::false_type());
}

}  // namespace

hipError_t launch_fixed_demux(const fx::FxArgs& p, const int8_t* d_q, hipStream_t st)
{
    const int n = 3 * p.K + 12;
    const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)(p.Bp / kTile));
    hipLaunchKernelGGL(fx_demux_kernel, grid, dim3(kTileThreads), 0, st, d_q, p.K, p.B, p.Bp,
                       const_cast<int8_t*>(p.xs), const_cast<int8_t*>(p.xp1), const_cast<int8_t*>(p.xp2));
    return hipGetLastError();
}

hipError_t launch_fixed_decode(const fx::FxArgs& p, const fx::FxWindow* w, const fx::FxStop* s, const fx::MaxStar* m,
                               uint32_t* d_ev, uint16_t* d_hist, uint32_t* d_nii, uint8_t* d_bits, int32_t* d_iters,
                               hipStream_t st)
{
    const fx::FxStop stop = s ? *s : fx::FxStop{};     // what a setting that is off leaves zeroed is never read
    const fx::MaxStar tab = m ? *m : fx::MaxStar{};
    const dim3 lanes(kFxLanes);
    // the instantiation of the handle's settings: f(STOP, NII, M) with the flags as types
    auto pick = [&](auto&& f) {
        with_flag(s != nullptr, [&](auto STOP) {
            with_flag(d_nii != nullptr, [&](auto NII) {
                with_flag(m != nullptr, [&](auto TAB) {
                    f(STOP, NII, std::conditional_t<decltype(TAB)::value, fx::MaxStar, fx::MaxLog>());
                });
            });
        });
    };
    if (!w) {
        const dim3 grid((unsigned)(p.Bp / kFxLanes));
        pick([&](auto STOP, auto, auto M) {
            hipLaunchKernelGGL((fx_turbo_kernel<decltype(STOP)::value, decltype(M)>), grid, lanes, 0, st, p, stop, tab);
        });
    } else {
        if (s) {
            hipError_t e = hipMemsetAsync(s->used, 0, p.Bp * sizeof(int32_t), st);   // every codeword runs
            if (e != hipSuccess) return e;
        }
        const int nS = fx::window_blocks(p.L, w->window);
        const dim3 wgrid((unsigned)(p.Bp / kFxLanes), (unsigned)nS);
        const dim3 jgrid((unsigned)((p.Bp + kTileThreads - 1) / kTileThreads));
        for (int it = 0; it < p.iters; ++it) {
            const fx::FxNii n0 = d_nii ? fx::nii_args(d_nii, p.L, *w, p.Bp, it, 0) : fx::FxNii{};
            const fx::FxNii n1 = d_nii ? fx::nii_args(d_nii, p.L, *w, p.Bp, it, 1) : fx::FxNii{};
            pick([&](auto STOP, auto NII, auto M) {
                constexpr bool S = decltype(STOP)::value, N = decltype(NII)::value;
                hipLaunchKernelGGL((fx_window_siso_kernel<0, S, N, decltype(M)>), wgrid, lanes, 0, st, p, *w, stop, tab, n0,
                                   d_ev, d_hist, it);
                hipLaunchKernelGGL((fx_window_siso_kernel<1, S, N, decltype(M)>), wgrid, lanes, 0, st, p, *w, stop, tab, n1,
                                   d_ev, d_hist, it);
            });
            if (s) hipLaunchKernelGGL(fx_window_judge_kernel, jgrid, dim3(kTileThreads), 0, st, p, stop, d_ev, nS, it);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int rows = p.all_iters ? p.iters : 1;
    const dim3 grid((unsigned)((p.K + kTile - 1) / kTile), (unsigned)(p.Bp / kTile), (unsigned)rows);
    if (s)
        hipLaunchKernelGGL(fx_bits_stop_kernel, grid, dim3(kTileThreads), 0, st, p.bitsT, s->used, p.pinv, p.K, p.B, p.Bp,
                           rows, p.iters, d_bits, d_iters);
    else
        hipLaunchKernelGGL(fx_bits_kernel, grid, dim3(kTileThreads), 0, st, p.bitsT, p.K, p.B, p.Bp, rows, d_bits);
    return hipGetLastError();
}

hipError_t launch_fixed_dematch(const RmParams& p, const int8_t* d_e, int8_t* d_out, int accumulate, hipStream_t st)
{
    const int nout = 3 * p.K + 12;
    // 512: crossed by tests/test_gpu_ratematch_batches.py test_rate_dematch_int8_past_the_grid_cap (B = 513, 1100, 1537)
    const dim3 grid((unsigned)((nout + kTileThreads - 1) / kTileThreads), (unsigned)(p.B < 512 ? p.B : 512));
    if (accumulate)
        hipLaunchKernelGGL(fx_dematch_kernel<true>, grid, dim3(kTileThreads), 0, st, p, d_e, d_out);
    else
        hipLaunchKernelGGL(fx_dematch_kernel<false>, grid, dim3(kTileThreads), 0, st, p, d_e, d_out);
    return hipGetLastError();
}

}  // namespace td
