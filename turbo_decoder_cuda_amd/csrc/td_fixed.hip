// td_fixed.hip -- the fixed-point decoder (TD_FIXED) on gfx950: int8 channel LLRs in, integer
// Max-Log-MAP (or, with td_set_fixed_maxstar's table, integer log-MAP), int16 extrinsics, uint8 decisions.
// The arithmetic is td_fixed_core.h's; here are the kernels around it.
//
//   fx_demux_kernel    q [B][3K+12] -> xs, xp1, xp2 [row][Bp]: a 64 x 64 byte transpose through LDS, so
//                      that both the reads (along the stream) and the writes (along the batch) are
//                      contiguous; -128 becomes -127 and the lanes of the padding get zeros.
//   fx_turbo_kernel    one codeword per lane, all iterations in one launch.  A lane keeps its eight
//                      state metrics in registers (int32, never normalised); the forward pass leaves
//                      alpha at every kW-th step in the workspace (32 B per kW steps and codeword), the
//                      backward pass recomputes a window's alpha rows into registers and runs beta,
//                      Lambda and the extrinsic over them.  The interleaver is a row index that the
//                      whole wave shares, so every access to the workspace is one contiguous row piece.
//   fx_bits_kernel     bitsT [rows][K][Bp] -> the caller's [B][rows][K], the transpose back.
//   fx_turbo_stop_kernel, fx_bits_stop_kernel  the same two with early termination (td_set_fixed_stop): a
//                      lane whose codeword has stopped is skipped, a wave whose lanes have all stopped
//                      returns, and the transpose back reads row min(row, used - 1) and undoes the interleaved
//                      order that the stopping decoder keeps its decisions in.
//   fx_window_siso_kernel  the sub-block schedule (td_set_fixed_window): one SISO of one iteration a launch,
//                      a wave = 64 codewords x one sub-block (blockIdx.y), the kernel boundary as the
//                      ordering between a SISO's extrinsic writes and the next SISO's reads.
//   fx_window_siso_stop_kernel, fx_window_judge_kernel  the sub-block schedule with early termination
//                      (td_set_fixed_window_stop): used[b] is the state (0 = running), a wave with no running
//                      codeword returns, SISO2 leaves each sub-block's evidence in the workspace (and, for
//                      the next iteration's HDA comparison, every 16-step window's decisions packed) and the
//                      judge, a launch of its own after SISO2's, folds it and stops the codeword; then
//                      fx_bits_stop_kernel.
//   fx_turbo_maxstar_kernel, fx_turbo_stop_maxstar_kernel, fx_window_siso_maxstar_kernel,
//   fx_window_siso_stop_maxstar_kernel  the decoding kernels above with td_set_fixed_maxstar's table: the lane
//                      code instantiated with fx::MaxStar for fx::MaxLog, the table's two words and its shift
//                      as kernel arguments (scalar registers).  Launched only while a table is set; without
//                      one a decode launches the kernels above, which do not change.
//   fx_window_siso_nii_kernel, fx_window_siso_stop_nii_kernel, fx_window_siso_maxstar_nii_kernel,
//   fx_window_siso_stop_maxstar_nii_kernel  the four sub-block kernels with next-iteration initialisation
//                      (td_set_fixed_window_nii): the lane code instantiated with NII, the state's two halves
//                      (read: the previous iteration's, written: this one's) as kernel arguments.  Launched
//                      only while NII is on; with it off a decode launches the kernels above, which do not change.
//   fx_dematch_kernel  saturating int8 de-rate-matching, one thread per stream position.
#include <hip/hip_runtime.h>

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

__global__ __launch_bounds__(kFxLanes) void fx_turbo_kernel(fx::FxArgs p)
{
    fx::decode_codeword(p, blockIdx.x * kFxLanes + threadIdx.x);
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

// The stopping decoder (td_set_fixed_stop): a wave ends once its 64 codewords have stopped.
__global__ __launch_bounds__(kFxLanes) void fx_turbo_stop_kernel(fx::FxArgs p, fx::FxStop s)
{
    fx::decode_codeword_stop(p, s, blockIdx.x * kFxLanes + threadIdx.x);
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
template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_kernel(fx::FxArgs p, fx::FxWindow w, int it)
{
    fx::siso_window_pass<DEC>(p, w, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y);
}

// The same with early termination (td_set_fixed_window_stop), on the same grid: a wave whose 64 codewords
// have all stopped returns at once, and SISO2 leaves the sub-block's evidence at ev[blockIdx.y][b].
template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_stop_kernel(fx::FxArgs p, fx::FxWindow w, fx::FxStop s,
                                                                        uint32_t* __restrict__ ev,
                                                                        uint16_t* __restrict__ hist, int it)
{
    fx::siso_window_stop<DEC>(p, w, s, ev, hist, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y);
}

// One thread per codeword after SISO2's launch of iteration `it`: folds the sub-blocks' evidence and
// sets used[b] where the codeword stops.  The kernel boundaries order it after the stores of ev and
// before the next launch's reads of used.
__global__ __launch_bounds__(kTileThreads) void fx_window_judge_kernel(fx::FxArgs p, fx::FxStop s,
                                                                       const uint32_t* __restrict__ ev, int nS, int it)
{
    fx::window_judge(p, s, ev, nS, (size_t)blockIdx.x * kTileThreads + threadIdx.x, it);
}

// The four decoding kernels with the correction table (td_set_fixed_maxstar): the same grids and arguments,
// and m, the same in every lane.
__global__ __launch_bounds__(kFxLanes) void fx_turbo_maxstar_kernel(fx::FxArgs p, fx::MaxStar m)
{
    fx::decode_codeword(p, blockIdx.x * kFxLanes + threadIdx.x, m);
}

__global__ __launch_bounds__(kFxLanes) void fx_turbo_stop_maxstar_kernel(fx::FxArgs p, fx::FxStop s, fx::MaxStar m)
{
    fx::decode_codeword_stop(p, s, blockIdx.x * kFxLanes + threadIdx.x, m);
}

template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_maxstar_kernel(fx::FxArgs p, fx::FxWindow w, fx::MaxStar m,
                                                                           int it)
{
    fx::siso_window_pass<DEC>(p, w, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y, m);
}

template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_stop_maxstar_kernel(fx::FxArgs p, fx::FxWindow w, fx::FxStop s,
                                                                                fx::MaxStar m, uint32_t* __restrict__ ev,
                                                                                uint16_t* __restrict__ hist, int it)
{
    fx::siso_window_stop<DEC>(p, w, s, ev, hist, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y, m);
}

// The four sub-block kernels with next-iteration initialisation (td_set_fixed_window_nii): the same grids, and
// n, the same in every lane.
template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_nii_kernel(fx::FxArgs p, fx::FxWindow w, fx::FxNii n, int it)
{
    fx::siso_window_pass_nii<DEC>(p, w, n, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y);
}

template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_stop_nii_kernel(fx::FxArgs p, fx::FxWindow w, fx::FxStop s,
                                                                            fx::FxNii n, uint32_t* __restrict__ ev,
                                                                            uint16_t* __restrict__ hist, int it)
{
    fx::siso_window_stop_nii<DEC>(p, w, s, ev, hist, n, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y);
}

template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_maxstar_nii_kernel(fx::FxArgs p, fx::FxWindow w, fx::MaxStar m,
                                                                               fx::FxNii n, int it)
{
    fx::siso_window_pass_nii<DEC>(p, w, n, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y, m);
}

template <int DEC>
__global__ __launch_bounds__(kFxLanes) void fx_window_siso_stop_maxstar_nii_kernel(fx::FxArgs p, fx::FxWindow w,
                                                                                    fx::FxStop s, fx::MaxStar m, fx::FxNii n,
                                                                                    uint32_t* __restrict__ ev,
                                                                                    uint16_t* __restrict__ hist, int it)
{
    fx::siso_window_stop_nii<DEC>(p, w, s, ev, hist, n, blockIdx.x * kFxLanes + threadIdx.x, it, (int)blockIdx.y, m);
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

}  // namespace

hipError_t launch_fixed_demux(const fx::FxArgs& p, const int8_t* d_q, hipStream_t st)
{
    const int n = 3 * p.K + 12;
    const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)(p.Bp / kTile));
    hipLaunchKernelGGL(fx_demux_kernel, grid, dim3(kTileThreads), 0, st, d_q, p.K, p.B, p.Bp,
                       const_cast<int8_t*>(p.xs), const_cast<int8_t*>(p.xp1), const_cast<int8_t*>(p.xp2));
    return hipGetLastError();
}

hipError_t launch_fixed_turbo(const fx::FxArgs& p, const fx::MaxStar* m, uint8_t* d_bits, hipStream_t st)
{
    if (m)
        hipLaunchKernelGGL(fx_turbo_maxstar_kernel, dim3((unsigned)(p.Bp / kFxLanes)), dim3(kFxLanes), 0, st, p, *m);
    else
        hipLaunchKernelGGL(fx_turbo_kernel, dim3((unsigned)(p.Bp / kFxLanes)), dim3(kFxLanes), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int rows = p.all_iters ? p.iters : 1;
    const dim3 grid((unsigned)((p.K + kTile - 1) / kTile), (unsigned)(p.Bp / kTile), (unsigned)rows);
    hipLaunchKernelGGL(fx_bits_kernel, grid, dim3(kTileThreads), 0, st, p.bitsT, p.K, p.B, p.Bp, rows, d_bits);
    return hipGetLastError();
}

hipError_t launch_fixed_turbo_stop(const fx::FxArgs& p, const fx::FxStop& s, const fx::MaxStar* m, uint8_t* d_bits,
                                   int32_t* d_iters, hipStream_t st)
{
    if (m)
        hipLaunchKernelGGL(fx_turbo_stop_maxstar_kernel, dim3((unsigned)(p.Bp / kFxLanes)), dim3(kFxLanes), 0, st, p, s, *m);
    else
        hipLaunchKernelGGL(fx_turbo_stop_kernel, dim3((unsigned)(p.Bp / kFxLanes)), dim3(kFxLanes), 0, st, p, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int rows = p.all_iters ? p.iters : 1;
    const dim3 grid((unsigned)((p.K + kTile - 1) / kTile), (unsigned)(p.Bp / kTile), (unsigned)rows);
    hipLaunchKernelGGL(fx_bits_stop_kernel, grid, dim3(kTileThreads), 0, st, p.bitsT, s.used, p.pinv, p.K, p.B, p.Bp,
                       rows, p.iters, d_bits, d_iters);
    return hipGetLastError();
}

hipError_t launch_fixed_window(const fx::FxArgs& p, const fx::FxWindow& w, const fx::MaxStar* m, uint32_t* d_nii,
                               uint8_t* d_bits, hipStream_t st)
{
    const dim3 wgrid((unsigned)(p.Bp / kFxLanes), (unsigned)fx::window_blocks(p.L, w.window));
    for (int it = 0; it < p.iters; ++it) {
        if (d_nii) {
            const fx::FxNii n0 = fx::nii_args(d_nii, p.L, w, p.Bp, it, 0), n1 = fx::nii_args(d_nii, p.L, w, p.Bp, it, 1);
            if (m) {
                hipLaunchKernelGGL(fx_window_siso_maxstar_nii_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, *m, n0, it);
                hipLaunchKernelGGL(fx_window_siso_maxstar_nii_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, *m, n1, it);
            } else {
                hipLaunchKernelGGL(fx_window_siso_nii_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, n0, it);
                hipLaunchKernelGGL(fx_window_siso_nii_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, n1, it);
            }
        } else if (m) {
            hipLaunchKernelGGL(fx_window_siso_maxstar_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, *m, it);
            hipLaunchKernelGGL(fx_window_siso_maxstar_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, *m, it);
        } else {
            hipLaunchKernelGGL(fx_window_siso_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, it);
            hipLaunchKernelGGL(fx_window_siso_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, it);
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int rows = p.all_iters ? p.iters : 1;
    const dim3 grid((unsigned)((p.K + kTile - 1) / kTile), (unsigned)(p.Bp / kTile), (unsigned)rows);
    hipLaunchKernelGGL(fx_bits_kernel, grid, dim3(kTileThreads), 0, st, p.bitsT, p.K, p.B, p.Bp, rows, d_bits);
    return hipGetLastError();
}

hipError_t launch_fixed_window_stop(const fx::FxArgs& p, const fx::FxWindow& w, const fx::FxStop& s, const fx::MaxStar* m,
                                    uint32_t* d_ev, uint16_t* d_hist, uint32_t* d_nii, uint8_t* d_bits, int32_t* d_iters,
                                    hipStream_t st)
{
    hipError_t e = hipMemsetAsync(s.used, 0, p.Bp * sizeof(int32_t), st);   // every codeword runs
    if (e != hipSuccess) return e;
    const int nS = fx::window_blocks(p.L, w.window);
    const dim3 wgrid((unsigned)(p.Bp / kFxLanes), (unsigned)nS);
    const dim3 jgrid((unsigned)((p.Bp + kTileThreads - 1) / kTileThreads));
    for (int it = 0; it < p.iters; ++it) {
        if (d_nii) {
            const fx::FxNii n0 = fx::nii_args(d_nii, p.L, w, p.Bp, it, 0), n1 = fx::nii_args(d_nii, p.L, w, p.Bp, it, 1);
            if (m) {
                hipLaunchKernelGGL(fx_window_siso_stop_maxstar_nii_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, s, *m, n0, d_ev, d_hist, it);
                hipLaunchKernelGGL(fx_window_siso_stop_maxstar_nii_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, s, *m, n1, d_ev, d_hist, it);
            } else {
                hipLaunchKernelGGL(fx_window_siso_stop_nii_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, s, n0, d_ev, d_hist, it);
                hipLaunchKernelGGL(fx_window_siso_stop_nii_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, s, n1, d_ev, d_hist, it);
            }
        } else if (m) {
            hipLaunchKernelGGL(fx_window_siso_stop_maxstar_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, s, *m, d_ev, d_hist, it);
            hipLaunchKernelGGL(fx_window_siso_stop_maxstar_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, s, *m, d_ev, d_hist, it);
        } else {
            hipLaunchKernelGGL(fx_window_siso_stop_kernel<0>, wgrid, dim3(kFxLanes), 0, st, p, w, s, d_ev, d_hist, it);
            hipLaunchKernelGGL(fx_window_siso_stop_kernel<1>, wgrid, dim3(kFxLanes), 0, st, p, w, s, d_ev, d_hist, it);
        }
        hipLaunchKernelGGL(fx_window_judge_kernel, jgrid, dim3(kTileThreads), 0, st, p, s, d_ev, nS, it);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int rows = p.all_iters ? p.iters : 1;
    const dim3 grid((unsigned)((p.K + kTile - 1) / kTile), (unsigned)(p.Bp / kTile), (unsigned)rows);
    hipLaunchKernelGGL(fx_bits_stop_kernel, grid, dim3(kTileThreads), 0, st, p.bitsT, s.used, p.pinv, p.K, p.B, p.Bp,
                       rows, p.iters, d_bits, d_iters);
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
