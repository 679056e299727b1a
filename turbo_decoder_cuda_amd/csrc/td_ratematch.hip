// td_ratematch.hip -- LTE rate matching (36.212 5.1.4.1) on the device: the transmit-side bit
// selection (rate_match_kernel, a gather) and the receive-side soft de-rate-matching with repetition
// combining and HARQ accumulation (rate_dematch_kernel), also fused behind the demapper and the LLR conversion
// (demod_dematch_kernel: td_demod_dematch, symbols in, soft buffer out).  Tables and notation: td_ratematch.h;
// the de-rate-matching body, which the transport-block kernel shares: td_dematch_band.h.
#include <hip/hip_runtime.h>

#include "td_dematch_band.h"
#include "td_demap_core.h"
#include "td_ratematch.h"

namespace td {

namespace {

using namespace band;   // kRmThreads, sum_add, dematch_band (td_dematch_band.h)

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
