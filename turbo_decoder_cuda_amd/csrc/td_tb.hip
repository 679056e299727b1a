// td_tb.hip -- transport blocks on the device (36.212 5.1.2, 5.1.4.1.2, 5.1.5): segmentation with filler bits
// and the two CRCs (td_tb_segment), rate matching of every code block into its piece of the concatenated row
// (td_tb_rate_match), the transpose with HARQ combining (td_tb_rate_dematch), and the reassembly with both
// CRC checks (td_tb_concat).  Plan, block-major layout and index arithmetic: td_tb_core.h.
//
// The code blocks of N transport blocks are rows of two arrays, [C_minus][N][K_minus] and [C_plus][N][K_plus].
// The kernels that walk rows (tb_fill_kernel, tb_concat_kernel) serve both arrays in one launch: the grid's
// first `gm` workgroups take the K_minus array, the others the K_plus array, a wave a row at a time, the
// lanes consecutive bytes.  The syndrome tables are read where they lie: the gCRC24A table is 4 B bytes --
// beyond LDS from A = 41 000 on -- and a copy of a size's gCRC24B table in LDS (td_encode.hip's crc_kernel)
// is four times a row's bytes, which a workgroup that gets four rows (N = 256, C = 13) never earns back;
// every wave of the call reads the same few tables, which the caches hold.
//
//   td_tb_segment       tb_crc_kernel: a workgroup a transport block, gCRC24A of its A bits, written as 24
//                       bits where the plan puts them (the end of the last block's payload);
//                       tb_fill_kernel: a wave a code block: filler zeros, the payload from d_tb (the
//                       gCRC24A bits are read back from the row), gCRC24B over both into the last 24
//   td_tb_rate_match    one thread per element of the concatenated row: its block, its table, one gather
//   td_tb_rate_dematch  td_dematch_band.h's body, a grid plane per code block
//   td_tb_demod_dematch the same body and grid; where f would be read, the received symbol is demapped, its
//                       sign flipped by the scrambling sequence's bit (td_gold_core.h) and converted
//   td_tb_concat        tb_concat_kernel: a wave a code block: payload out, gCRC24B remainder;
//                       tb_rem_kernel (only with d_tb_rem): a workgroup a transport block, gCRC24A remainder
//                       of the blocks' payloads
// Every access is one element wide: pointers need only element alignment.
#include <hip/hip_runtime.h>

#include "td_dematch_band.h"
#include "td_encode_core.h"
#include "td_gold_core.h"
#include "td_tb.h"

namespace td {

namespace {

using namespace band;
using enc::crc_out_bit;
using enc::crc_term;

constexpr int kTbThreads = 256, kTbWaves = kTbThreads / 64;
// a workgroup a transport block (tb_crc_kernel, tb_rem_kernel): few of them at a small N, so wide ones
constexpr int kTbWide = 1024, kTbWideWaves = kTbWide / 64;

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d);
    return v;
}

// XOR over a workgroup of kTbWide threads, in every thread; `part` [kTbWideWaves] in LDS, free again after the call
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t* part)
{
    v = wave_xor(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int w = 0; w < kTbWideWaves; ++w) r ^= part[w];
    __syncthreads();
    return r;
}

// gCRC24A of every transport block, as bits b[A .. A+24) in the code blocks
__global__ __launch_bounds__(kTbWide) void tb_crc_kernel(TbTables t, const uint8_t* __restrict__ tb, int N,
                                                            uint8_t* cb_minus, uint8_t* cb_plus)
{
    __shared__ uint32_t part[kTbWideWaves];
    const tb::Plan& p = t.plan;
    const int tid = threadIdx.x;
    for (size_t n = blockIdx.x; n < (size_t)N; n += gridDim.x) {
        const uint8_t* row = tb + n * (size_t)p.A;
        uint32_t acc = 0;
#pragma unroll 8
        for (int s = tid; s < p.A; s += kTbWide) acc ^= crc_term(row[s], t.syn_a[s + 24]);
        const uint32_t crc = block_xor(acc, part);
        if (tid < 24) {
            const tb::Loc l = tb::locate(p, p.A + tid);
            uint8_t* out = l.r < p.C_minus ? cb_minus : cb_plus;
            out[tb::block_row(p, l.r, n, (size_t)N) * (size_t)tb::block_k(p, l.r) + l.i] = crc_out_bit(crc, tid);
        }
    }
}

// the workgroup's array (K_plus?), its index among that array's workgroups and their number
struct RowShare {
    bool plus;
    unsigned wg, nwg;
};
__device__ __forceinline__ RowShare row_share(unsigned gm)
{
    const bool plus = blockIdx.x >= gm;
    return RowShare{plus, plus ? blockIdx.x - gm : blockIdx.x, plus ? gridDim.x - gm : gm};
}

// the code blocks but for gCRC24A's bits: filler, payload, gCRC24B
__global__ __launch_bounds__(kTbThreads) void tb_fill_kernel(TbTables t, const uint8_t* __restrict__ tb, int N,
                                                             uint8_t* cb_minus, uint8_t* cb_plus, unsigned gm)
{
    const tb::Plan& p = t.plan;
    const RowShare sh = row_share(gm);
    const int K = sh.plus ? p.K_plus : p.K_minus, pay = K - p.L;
    const size_t rows = (size_t)(sh.plus ? p.C_plus : p.C_minus) * (size_t)N;
    uint8_t* out = sh.plus ? cb_plus : cb_minus;
    const uint32_t* __restrict__ syn = t.syn_b[sh.plus ? 1 : 0];   // read only where L != 0
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (size_t j = (size_t)sh.wg * kTbWaves + wave; j < rows; j += (size_t)sh.nwg * kTbWaves) {
        const size_t rl = j / (size_t)N, n = j - rl * (size_t)N;
        const int s0 = tb::block_start(p, (int)rl + (sh.plus ? p.C_minus : 0));
        const uint8_t* src = tb + n * (size_t)p.A;
        uint8_t* row = out + j * (size_t)K;
        uint32_t acc = 0;
#pragma unroll 4
        for (int i = lane; i < pay; i += 64) {
            const int s = s0 + i;
            uint8_t bit;
            if (s < 0)
                row[i] = bit = 0;                        // filler
            else if (s < p.A)
                row[i] = bit = src[s] != 0 ? 1 : 0;
            else
                bit = row[i];                            // gCRC24A's, tb_crc_kernel's
            if (p.L) acc ^= crc_term(bit, syn[i + 24]);
        }
        if (p.L) {
            acc = wave_xor(acc);
            if (lane < 24) row[pay + lane] = crc_out_bit(acc, lane);
        }
    }
}

// code blocks -> the transport block's A bits and every block's gCRC24B remainder (the filler read as zeros)
__global__ __launch_bounds__(kTbThreads) void tb_concat_kernel(TbTables t, const uint8_t* __restrict__ bits_minus,
                                                               const uint8_t* __restrict__ bits_plus, int N,
                                                               uint8_t* __restrict__ tb, uint32_t* __restrict__ cb_rem,
                                                               unsigned gm)
{
    const tb::Plan& p = t.plan;
    const RowShare sh = row_share(gm);
    const int K = sh.plus ? p.K_plus : p.K_minus, pay = K - p.L;
    const size_t rows = (size_t)(sh.plus ? p.C_plus : p.C_minus) * (size_t)N;
    const uint8_t* in = sh.plus ? bits_plus : bits_minus;
    const uint32_t* __restrict__ syn = t.syn_b[sh.plus ? 1 : 0];   // read only with crc
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool crc = p.L && cb_rem;
    for (size_t j = (size_t)sh.wg * kTbWaves + wave; j < rows; j += (size_t)sh.nwg * kTbWaves) {
        const size_t rl = j / (size_t)N, n = j - rl * (size_t)N;
        const int r = (int)rl + (sh.plus ? p.C_minus : 0);
        const int s0 = tb::block_start(p, r);
        const uint8_t* row = in + j * (size_t)K;
        uint8_t* dst = tb + n * (size_t)p.A;
        uint32_t acc = 0;
#pragma unroll 4
        for (int i = lane; i < K; i += 64) {
            const int s = s0 + i;
            const uint8_t bit = s < 0 ? 0 : (row[i] != 0 ? 1 : 0);
            if (i < pay && s >= 0 && s < p.A) dst[s] = bit;
            if (crc) acc ^= crc_term(bit, syn[i]);
        }
        if (cb_rem) {
            acc = wave_xor(acc);
            if (lane == 0) cb_rem[n * (size_t)p.C + r] = acc;   // C = 1: no block CRC, 0
        }
    }
}

// gCRC24A's remainder of the B bits the blocks' payloads hold
__global__ __launch_bounds__(kTbWide) void tb_rem_kernel(TbTables t, const uint8_t* __restrict__ bits_minus,
                                                            const uint8_t* __restrict__ bits_plus, int N,
                                                            uint32_t* __restrict__ tb_rem)
{
    __shared__ uint32_t part[kTbWideWaves];
    const tb::Plan& p = t.plan;
    const int tid = threadIdx.x;
    for (size_t n = blockIdx.x; n < (size_t)N; n += gridDim.x) {
        uint32_t acc = 0;
        for (int r = 0; r < p.C; ++r) {
            const int K = tb::block_k(p, r), pay = K - p.L, s0 = tb::block_start(p, r);
            const uint8_t* row = (r < p.C_minus ? bits_minus : bits_plus) + tb::block_row(p, r, n, (size_t)N) * (size_t)K;
#pragma unroll 4
            for (int i = tid; i < pay; i += kTbWide) {
                const int s = s0 + i;
                if (s >= 0) acc ^= crc_term(row[i], t.syn_a[s]);
            }
        }
        const uint32_t rem = block_xor(acc, part);
        if (tid == 0) tb_rem[n] = rem;
    }
}

__device__ __forceinline__ TbRmClass pick_class(const TbTables& t, bool plus, bool filler)
{
    return plus ? (filler ? t.cls[1][1] : t.cls[1][0]) : (filler ? t.cls[0][1] : t.cls[0][0]);
}

// f[n][g] = coded_r[n][pos_r[(c0_r + k) mod Nnn_r]], g = e_start(r) + k: a thread an element of the row, the
// transport blocks of one grid column share its table entry
__global__ __launch_bounds__(kTbThreads) void tb_rate_match_kernel(TbTables t, tb::RmSizes sz, long long G, int N,
                                                                   const uint8_t* __restrict__ coded_minus,
                                                                   const uint8_t* __restrict__ coded_plus,
                                                                   uint8_t* __restrict__ f)
{
    const long long g = (long long)blockIdx.x * kTbThreads + threadIdx.x;
    if (g >= G) return;
    const tb::Plan& p = t.plan;
    const tb::Loc l = tb::e_locate(sz, g);
    const bool plus = l.r >= p.C_minus;
    const TbRmClass c = pick_class(t, plus, l.r == 0 && p.F > 0);
    const int src = c.pos[((unsigned)l.i + (unsigned)c.c0) % (unsigned)c.Nnn];
    const size_t nrow = 3 * (size_t)c.K + 12;
    const uint8_t* in = (plus ? coded_plus : coded_minus) + tb::block_row(p, l.r, 0, (size_t)N) * nrow + src;
    for (size_t n = blockIdx.y; n < (size_t)N; n += gridDim.y) f[n * (size_t)G + (size_t)g] = in[n * nrow];
}

constexpr int kTbRows = 16;   // td_rate_dematch's band
constexpr unsigned kTbGridY = 512;

// blockIdx.z: the code block; blockIdx.x: its band (the grid has the larger size's bands); blockIdx.y: the
// transport blocks
template <typename T, bool ACC>
__global__ __launch_bounds__(kTbThreads) void tb_rate_dematch_kernel(TbTables t, tb::RmSizes sz, long long G, int N,
                                                                     const T* __restrict__ f, T* llr_minus, T* llr_plus,
                                                                     T filler)
{
    const tb::Plan& p = t.plan;
    const int r = blockIdx.z;
    const bool plus = r >= p.C_minus, fill = r == 0 && p.F > 0;
    const TbRmClass c = pick_class(t, plus, fill);
    if ((int)blockIdx.x * kTbRows >= c.R) return;   // the whole workgroup: before any barrier
    const RmParams rp{c.K, c.R, c.ND, c.Nnn, c.c0, tb::e_size(sz, r), N, c.rank, c.pos};
    const size_t nout = 3 * (size_t)c.K + 12;
    T* out = (plus ? llr_plus : llr_minus) + tb::block_row(p, r, 0, (size_t)N) * nout;
    const ArraySrc<T> src{f + tb::e_start(sz, r), (size_t)G};   // row n of this block's piece: f[n][e_start ..]
    dematch_band<T, ACC, kTbRows>(rp, src, out, FillerFill<T>{fill ? p.F : 0, filler});
}

// td_tb_demod_dematch's source of block r: e_r[n][k] is bit g % M of symbol n (G / M) + g / M with g = e0 + k,
// e0 = e_start(r) (a multiple of NlQm, so of M) -- demapped, its sign flipped by bit g of row n of seq (null:
// no scrambling), converted.  The same double, the same negation and the same conversion as td_demodulate ->
// td_descramble_llr -> td_llr_convert on the whole [N][G] array.  Consecutive k share a sequence word.
template <int M, typename T>
struct TbDemapRow {
    const double* yi;      // the row's symbols
    const double* yq;
    const uint32_t* seq;   // the row's words, or null
    unsigned e0;
    double Kf, steps_per_unit;
    __device__ __forceinline__ T operator[](size_t k) const
    {
        const unsigned g = e0 + (unsigned)k, s = g / (unsigned)M, b = g - s * (unsigned)M;
        double x = demod_bit<M>(yi[s], yq[s], Kf, (int)b);
        if (seq) x = gold::flip_sign(x, (seq[g >> 5] >> (g & 31)) & 1u);
        return llr_to<T>(x, steps_per_unit);
    }
};
template <int M, typename T>
struct TbDemapSrc {
    const double* yi;      // [N][G / M]
    const double* yq;
    const uint32_t* seq;   // [N][W] or null
    size_t nsym, W;
    unsigned e0;
    double Kf, steps_per_unit;
    __device__ __forceinline__ TbDemapRow<M, T> row(size_t n) const
    {
        return TbDemapRow<M, T>{yi + n * nsym, yq + n * nsym, seq ? seq + n * W : nullptr, e0, Kf, steps_per_unit};
    }
};

// tb_rate_dematch_kernel with the symbols where f would be read
template <int M, typename T, bool ACC>
__global__ __launch_bounds__(kTbThreads) void tb_demod_dematch_kernel(TbTables t, tb::RmSizes sz, long long G, int N,
                                                                      const double* __restrict__ yi,
                                                                      const double* __restrict__ yq,
                                                                      const uint32_t* __restrict__ seq, double Kf,
                                                                      double steps_per_unit, T* llr_minus, T* llr_plus, T filler)
{
    const tb::Plan& p = t.plan;
    const int r = blockIdx.z;
    const bool plus = r >= p.C_minus, fill = r == 0 && p.F > 0;
    const TbRmClass c = pick_class(t, plus, fill);
    if ((int)blockIdx.x * kTbRows >= c.R) return;   // the whole workgroup: before any barrier
    const RmParams rp{c.K, c.R, c.ND, c.Nnn, c.c0, tb::e_size(sz, r), N, c.rank, c.pos};
    const size_t nout = 3 * (size_t)c.K + 12;
    T* out = (plus ? llr_plus : llr_minus) + tb::block_row(p, r, 0, (size_t)N) * nout;
    const TbDemapSrc<M, T> src{yi, yq, seq, (size_t)(G / M), (size_t)((G + 31) / 32), (unsigned)tb::e_start(sz, r), Kf,
                               steps_per_unit};
    dematch_band<T, ACC, kTbRows>(rp, src, out, FillerFill<T>{fill ? p.F : 0, filler});
}

// workgroups for `rows` rows, a wave each, at most four workgroups a compute unit
unsigned row_wgs(size_t rows, int cus)
{
    const size_t need = (rows + kTbWaves - 1) / kTbWaves, cap = (size_t)(cus > 0 ? cus : 256) * 4;
    return (unsigned)(need < cap ? need : cap);
}
unsigned tb_wgs(int N, int cus)
{
    const size_t cap = (size_t)(cus > 0 ? cus : 256) * 2;
    return (unsigned)((size_t)N < cap ? (size_t)N : cap);
}

}  // namespace

hipError_t launch_tb_segment(const TbTables& t, const uint8_t* d_tb, int N, uint8_t* d_cb_minus, uint8_t* d_cb_plus,
                             hipStream_t st)
{
    const tb::Plan& p = t.plan;
    hipLaunchKernelGGL(tb_crc_kernel, dim3(tb_wgs(N, t.cus)), dim3(kTbWide), 0, st, t, d_tb, N, d_cb_minus, d_cb_plus);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned gm = row_wgs((size_t)p.C_minus * (size_t)N, t.cus), gp = row_wgs((size_t)p.C_plus * (size_t)N, t.cus);
    hipLaunchKernelGGL(tb_fill_kernel, dim3(gm + gp), dim3(kTbThreads), 0, st, t, d_tb, N, d_cb_minus, d_cb_plus, gm);
    return hipGetLastError();
}

hipError_t launch_tb_rate_match(const TbTables& t, const tb::RmSizes& sz, long long G, const uint8_t* d_coded_minus,
                                const uint8_t* d_coded_plus, int N, uint8_t* d_f, hipStream_t st)
{
    const dim3 grid((unsigned)((G + kTbThreads - 1) / kTbThreads), (unsigned)(N < 65535 ? N : 65535));
    hipLaunchKernelGGL(tb_rate_match_kernel, grid, dim3(kTbThreads), 0, st, t, sz, G, N, d_coded_minus, d_coded_plus, d_f);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_tb_rate_dematch(const TbTables& t, const tb::RmSizes& sz, long long G, const T* d_f, int N, T* d_llr_minus,
                                  T* d_llr_plus, T filler, int accumulate, hipStream_t st)
{
    const int R = (t.plan.K_plus + 4 + 31) / 32;
    const dim3 grid((unsigned)((R + kTbRows - 1) / kTbRows), (unsigned)N < kTbGridY ? (unsigned)N : kTbGridY,
                    (unsigned)t.plan.C);
    if (accumulate)
        hipLaunchKernelGGL((tb_rate_dematch_kernel<T, true>), grid, dim3(kTbThreads), 0, st, t, sz, G, N, d_f, d_llr_minus,
                           d_llr_plus, filler);
    else
        hipLaunchKernelGGL((tb_rate_dematch_kernel<T, false>), grid, dim3(kTbThreads), 0, st, t, sz, G, N, d_f, d_llr_minus,
                           d_llr_plus, filler);
    return hipGetLastError();
}

namespace {

template <int M, typename T>
hipError_t launch_tb_demod_dematch_m(const TbTables& t, const tb::RmSizes& sz, long long G, const TbDemodArgs& a, int N,
                                     T* d_llr_minus, T* d_llr_plus, T filler, int accumulate, hipStream_t st)
{
    // td_tb_rate_dematch's grid, cap included (crossed by tests/test_gpu_scramble.py at N = 513)
    const int R = (t.plan.K_plus + 4 + 31) / 32;
    const dim3 grid((unsigned)((R + kTbRows - 1) / kTbRows), (unsigned)N < kTbGridY ? (unsigned)N : kTbGridY,
                    (unsigned)t.plan.C);
    if (accumulate)
        hipLaunchKernelGGL((tb_demod_dematch_kernel<M, T, true>), grid, dim3(kTbThreads), 0, st, t, sz, G, N, a.yi, a.yq, a.seq,
                           a.Kf, a.steps_per_unit, d_llr_minus, d_llr_plus, filler);
    else
        hipLaunchKernelGGL((tb_demod_dematch_kernel<M, T, false>), grid, dim3(kTbThreads), 0, st, t, sz, G, N, a.yi, a.yq, a.seq,
                           a.Kf, a.steps_per_unit, d_llr_minus, d_llr_plus, filler);
    return hipGetLastError();
}

}  // namespace

template <typename T>
hipError_t launch_tb_demod_dematch(const TbTables& t, const tb::RmSizes& sz, long long G, const TbDemodArgs& a, int N,
                                   T* d_llr_minus, T* d_llr_plus, T filler, int accumulate, hipStream_t st)
{
    switch (a.M) {
        case 1: return launch_tb_demod_dematch_m<1>(t, sz, G, a, N, d_llr_minus, d_llr_plus, filler, accumulate, st);
        case 2: return launch_tb_demod_dematch_m<2>(t, sz, G, a, N, d_llr_minus, d_llr_plus, filler, accumulate, st);
        case 3: return launch_tb_demod_dematch_m<3>(t, sz, G, a, N, d_llr_minus, d_llr_plus, filler, accumulate, st);
        case 4: return launch_tb_demod_dematch_m<4>(t, sz, G, a, N, d_llr_minus, d_llr_plus, filler, accumulate, st);
        case 6: return launch_tb_demod_dematch_m<6>(t, sz, G, a, N, d_llr_minus, d_llr_plus, filler, accumulate, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_tb_concat(const TbTables& t, const uint8_t* d_bits_minus, const uint8_t* d_bits_plus, int N, uint8_t* d_tb,
                            uint32_t* d_cb_rem, uint32_t* d_tb_rem, hipStream_t st)
{
    const tb::Plan& p = t.plan;
    const unsigned gm = row_wgs((size_t)p.C_minus * (size_t)N, t.cus), gp = row_wgs((size_t)p.C_plus * (size_t)N, t.cus);
    hipLaunchKernelGGL(tb_concat_kernel, dim3(gm + gp), dim3(kTbThreads), 0, st, t, d_bits_minus, d_bits_plus, N, d_tb,
                       d_cb_rem, gm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_tb_rem) return e;
    hipLaunchKernelGGL(tb_rem_kernel, dim3(tb_wgs(N, t.cus)), dim3(kTbWide), 0, st, t, d_bits_minus, d_bits_plus, N, d_tb_rem);
    return hipGetLastError();
}

template hipError_t launch_tb_rate_dematch<double>(const TbTables&, const tb::RmSizes&, long long, const double*, int, double*,
                                                   double*, double, int, hipStream_t);
template hipError_t launch_tb_rate_dematch<float>(const TbTables&, const tb::RmSizes&, long long, const float*, int, float*,
                                                  float*, float, int, hipStream_t);
template hipError_t launch_tb_rate_dematch<int8_t>(const TbTables&, const tb::RmSizes&, long long, const int8_t*, int, int8_t*,
                                                   int8_t*, int8_t, int, hipStream_t);
template hipError_t launch_tb_demod_dematch<double>(const TbTables&, const tb::RmSizes&, long long, const TbDemodArgs&, int,
                                                    double*, double*, double, int, hipStream_t);
template hipError_t launch_tb_demod_dematch<float>(const TbTables&, const tb::RmSizes&, long long, const TbDemodArgs&, int,
                                                   float*, float*, float, int, hipStream_t);
template hipError_t launch_tb_demod_dematch<int8_t>(const TbTables&, const tb::RmSizes&, long long, const TbDemodArgs&, int,
                                                    int8_t*, int8_t*, int8_t, int, hipStream_t);

}  // namespace td
