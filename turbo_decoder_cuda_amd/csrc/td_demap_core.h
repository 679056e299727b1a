// td_demap_core.h -- the arithmetic of the receive front end: the constellations, the max-log demappers
// (modanddem.cpp:189-685), the conversion of a double LLR to the decoder's precision, and the value source
// that the fused de-rate-matching kernels read in place of an array of e.
//
// Plain C++ shared by the gfx950 kernels of td_synth.hip and td_ratematch.hip and by the
// stand-alone host program of the tests (tests/frontend_core_host.cpp, under ASan + UBSan).  The library
// never demaps on the host.  Every floating-point operation keeps the reference's order; all users are
// built with -ffp-contract=off.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TDM_HD __host__ __device__ __forceinline__
#define TDM_UNROLL _Pragma("unroll")
#else
#define TDM_HD inline
#define TDM_UNROLL
#endif

namespace td {

// constellations (modanddem.cpp:7-71)
constexpr double kQpskI[4] = {0.7071, 0.7071, -0.7071, -0.7071};
constexpr double kQpskQ[4] = {0.7071, -0.7071, 0.7071, -0.7071};
constexpr double k8pskI[8] = {-0.7071, -1, 0, 0.7071, 0, -0.7071, 0.7071, 1};
constexpr double k8pskQ[8] = {0.7071, 0, 1, 0.7071, -1, -0.7071, -0.7071, 0};
constexpr double k16qam[4] = {-0.948683, -0.316228, 0.948683, 0.316228};
constexpr double k64qam[4] = {0.4629, 0.1543, 0.7615, 1.0801};

// point of label j, M = 1, 2, 3, 4, 6 bits per symbol
template <int M>
TDM_HD void constellation(int j, double& ci, double& cq)
{
    if constexpr (M == 1) {
        ci = j ? 1.0 : -1.0;
        cq = 0.0;
    } else if constexpr (M == 2) {
        ci = kQpskI[j];
        cq = kQpskQ[j];
    } else if constexpr (M == 3) {
        ci = k8pskI[j];
        cq = k8pskQ[j];
    } else if constexpr (M == 4) {   // i: label bits 3-2, q: bits 1-0
        ci = k16qam[j >> 2];
        cq = k16qam[j & 3];
    } else {                         // 64QAM: sign bit 5 / 2, level bits 4-3 / 1-0
        ci = ((j >> 5) & 1) ? -k64qam[(j >> 3) & 3] : k64qam[(j >> 3) & 3];
        cq = ((j >> 2) & 1) ? -k64qam[j & 3] : k64qam[j & 3];
    }
}

// calculate_sqr_dis (modanddem.cpp:73-84) and the BPSK demodulator's LLR (modanddem.cpp:189-224)
TDM_HD double demod_bpsk(double yi, double yq, double Kf)
{
    const double dr1 = yi - 1.0, di1 = yq - 0.0;
    const double m1 = dr1 * dr1 + di1 * di1;   // distance to the symbol of bit 1
    const double dr0 = yi - (-1.0), di0 = yq - 0.0;
    const double m2 = dr0 * dr0 + di0 * di0;   // distance to the symbol of bit 0
    return -Kf * (m1 - m2);
}

// ---- The max-log bit LLRs of one received symbol, in the reference's operation order: per output bit,
// the minimum squared distance over the labels with that bit 1 and with it 0 (strict <, label order),
// out = -Kf (d1 - d0).  The minima start from the functions' own constants.  demod_symbol<M> gives all M
// of a symbol, demod_bit<M> one of them -- the very double demod_symbol puts in out[b] -- and both are
// made of the same pieces: the distances (axis_sq / point_sq) and the bit's minima (square_bit / scan_bit).
//
// Square constellations (M = 2, 4, 6) are a product of an I and a Q alphabet: the label's high M/2 bits
// pick i, the low M/2 bits pick q, so d[j] = fl(dI[jI] + dQ[jQ]) with the reference's own dI = fl(dr*dr),
// dQ = fl(di*di).  Rounded addition is monotone in each operand, so the minimum over a product set is
// fl(min dI + min dQ): the same value as the reference's scan, from 2^(M/2+1) squares and 2M + 4 minima
// instead of 2^M points (NaN symbols too: every d is NaN there and both the scan and this keep the
// initial minima).  A bit's LLR needs the minima of its own axis by the bit and the other axis' overall
// minimum.

// The axis alphabet of a square constellation: the i of label (l, 0), which is also the q of label (0, l).
template <int M>
TDM_HD double axis_level(int l)
{
    double ci, cq;
    constellation<M>(l << (M / 2), ci, cq);
    return ci;
}

// squared distances of one coordinate to the 2^(M/2) levels of its axis
template <int M>
TDM_HD void axis_sq(double y, double* d)
{
    TDM_UNROLL
    for (int l = 0; l < (1 << (M / 2)); ++l) {
        const double dr = y - axis_level<M>(l);
        d[l] = dr * dr;
    }
}

// the minimum of v[l] over the levels l with ((l & mask) != 0) == want; mask 0, want 0: over all of them
template <int M>
TDM_HD double min_if(const double* v, int mask, int want)
{
    double m = __builtin_inf();
    TDM_UNROLL
    for (int l = 0; l < (1 << (M / 2)); ++l)
        if (((l & mask) != 0) == (want != 0) && v[l] < m) m = v[l];
    return m;
}

// bit b of a square constellation: own = axis_sq of the bit's axis (I for b < M/2), other = the other
// axis' overall minimum
template <int M>
TDM_HD double square_bit(const double* own, double other, double Kf, int b)
{
    constexpr int H = M / 2;
    const int mask = 1 << (H - 1 - (b < H ? b : b - H));
    double m1 = M == 2 ? (double)0x7fffffffffff : (double)0x7fffffff;
    double m0 = (M == 2 && b == 0) ? (double)0x7fffffffffff : (double)0x7fffffff;
    const double c1 = min_if<M>(own, mask, 1) + other, c0 = min_if<M>(own, mask, 0) + other;
    if (c1 < m1) m1 = c1;
    if (c0 < m0) m0 = c0;
    return -Kf * (m1 - m0);
}

// squared distances to all 2^M points (calculate_sqr_dis, modanddem.cpp:73-84)
template <int M>
TDM_HD void point_sq(double yi, double yq, double* d)
{
    TDM_UNROLL
    for (int j = 0; j < (1 << M); ++j) {
        double ci, cq;
        constellation<M>(j, ci, cq);
        const double dr = yi - ci, di = yq - cq;
        d[j] = dr * dr + di * di;
    }
}

// bit b by the reference's scan over the 2^M distances (8PSK: first bit = LSB of the label)
template <int M>
TDM_HD double scan_bit(const double* d, double Kf, int b)
{
    const int mask = M == 3 ? 1 << b : 1 << (M - 1 - b);
    double m1 = M <= 2 ? (double)0x7fffffffffff : (double)0x7fffffff;
    double m0 = (M == 1 || (M == 2 && b == 0)) ? (double)0x7fffffffffff : (double)0x7fffffff;
    TDM_UNROLL
    for (int j = 0; j < (1 << M); ++j) {
        if (j & mask) {
            if (d[j] < m1) m1 = d[j];
        } else {
            if (d[j] < m0) m0 = d[j];
        }
    }
    return -Kf * (m1 - m0);
}

template <int M>
TDM_HD void demod_symbol(double yi, double yq, double Kf, double* out)
{
    if constexpr (M == 2 || M == 4 || M == 6) {
        constexpr int H = M / 2, NL = 1 << H;
        double dI[NL], dQ[NL];
        axis_sq<M>(yi, dI);
        axis_sq<M>(yq, dQ);
        const double allI = min_if<M>(dI, 0, 0), allQ = min_if<M>(dQ, 0, 0);
        TDM_UNROLL
        for (int b = 0; b < M; ++b) out[b] = b < H ? square_bit<M>(dI, allQ, Kf, b) : square_bit<M>(dQ, allI, Kf, b);
    } else {
        double d[1 << M];
        point_sq<M>(yi, yq, d);
        TDM_UNROLL
        for (int b = 0; b < M; ++b) out[b] = scan_bit<M>(d, Kf, b);
    }
}

// Bit b (0 <= b < M, a run-time value) of the symbol: element b of what demod_symbol<M> writes, and for
// M = 1 what td_demodulate writes, demod_bpsk.  No array is indexed by b: the bit only picks the axis'
// coordinate and the mask of the minima.
template <int M>
TDM_HD double demod_bit(double yi, double yq, double Kf, int b)
{
    if constexpr (M == 1) {
        return demod_bpsk(yi, yq, Kf);
    } else if constexpr (M == 2 || M == 4 || M == 6) {
        constexpr int NL = 1 << (M / 2);
        const bool in_i = b < M / 2;
        double own[NL], oth[NL];
        axis_sq<M>(in_i ? yi : yq, own);
        axis_sq<M>(in_i ? yq : yi, oth);
        return square_bit<M>(own, min_if<M>(oth, 0, 0), Kf, b);
    } else {
        double d[1 << M];
        point_sq<M>(yi, yq, d);
        return scan_bit<M>(d, Kf, b);
    }
}

// ---- td_llr_convert's element: a double LLR in the decoder's precision.
//   double  the value itself
//   float   the IEEE round-to-nearest-even narrowing (too large: +-inf)
//   int8    clamp(rint(x * steps_per_unit), -127, 127): one rounded multiply, ties to even, and the clamp
//           in double BEFORE the conversion to integer, so +-1e300 and +-inf give +-127 and no conversion
//           is undefined; -128 is never produced
template <typename T>
TDM_HD T llr_to(double x, double steps_per_unit);
template <>
TDM_HD double llr_to<double>(double x, double)
{
    return x;
}
template <>
TDM_HD float llr_to<float>(double x, double)
{
    return (float)x;
}
template <>
TDM_HD int8_t llr_to<int8_t>(double x, double steps_per_unit)
{
    double r = __builtin_rint(x * steps_per_unit);
    r = r > 127.0 ? 127.0 : r < -127.0 ? -127.0 : r;
    return (int8_t)(int)r;
}

// ---- What the de-rate-matching kernels read.  A source gives row(b), and row(b)[k] is e[b][k].
// the array of td_rate_dematch
template <typename T>
struct ArraySrc {
    const T* e;   // [B][E]
    size_t E;
    TDM_HD const T* row(size_t b) const { return e + b * E; }
};
// td_demod_dematch: e[b][k] = bit k % M of symbol b (E / M) + k / M, demapped and converted.  E < 2^31.
template <int M, typename T>
struct DemapRow {
    const double* yi;
    const double* yq;
    double Kf, steps_per_unit;
    TDM_HD T operator[](size_t k) const
    {
        const unsigned s = (unsigned)k / (unsigned)M, b = (unsigned)k - s * (unsigned)M;
        return llr_to<T>(demod_bit<M>(yi[s], yq[s], Kf, (int)b), steps_per_unit);
    }
};
template <int M, typename T>
struct DemapSrc {
    const double* yi;   // [B][E / M]
    const double* yq;
    size_t nsym;        // E / M
    double Kf, steps_per_unit;
    TDM_HD DemapRow<M, T> row(size_t b) const { return DemapRow<M, T>{yi + b * nsym, yq + b * nsym, Kf, steps_per_unit}; }
};

}  // namespace td
