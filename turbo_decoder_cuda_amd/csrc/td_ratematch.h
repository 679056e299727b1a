// td_ratematch.h -- LTE rate matching (3GPP TS 36.212 5.1.4.1) around the decoder's 3K+12 stream:
// the host tables (td_rm_set, td_rm_index_host) and the launchers of td_ratematch.hip.
//
// The coded stream s[0..3K+12) of encoderm_turbo (log_map.cpp:566-578) is the three LTE streams
// interleaved, d_i(k) = s[3k+i], k < D = K+4.  Each stream goes through the sub-block interleaver
// (32 columns, R = ceil(D/32) rows, ND = 32R - D leading <NULL>s, column permutation P; stream 2 reads
// one position further on), the three are laid into the circular buffer w (stream 0, then streams 1
// and 2 alternating), and a transmission reads E non-NULL entries of w[0..Ncb) from k0(rv) on, wrapping.
// Only the ordinal of a buffer position among the non-NULL entries matters, so two tables carry it all:
//   rank[q]  ordinal of stream position q's buffer position among the non-NULLs of w[0..Ncb), or -1
//            (its buffer position is >= Ncb)
//   pos[j]   the inverse: stream position of ordinal j, j < Nnn
// and a redundancy version rotates the ordinal: e_k = s[pos[(c0(rv) + k) mod Nnn]].
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace td {

struct RmTables {
    int K = 0, R = 0, Kpi = 0, Kw = 0, ND = 0;
    int Ncb = 0, Nnn = 0;   // soft buffer length, non-NULL entries of w[0..Ncb)
    int c0[4] = {};         // non-NULL entries before k0(rv) mod Ncb
    std::vector<int32_t> rank, pos;
};

// The column permutation of the sub-block interleaver (36.212 table 5.1.4-1): the 5-bit reversal.
constexpr int kRmPerm[32] = {0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30,
                             1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31};

// Ncb: 0 = the whole buffer Kw, otherwise Kpi <= Ncb <= Kw.  F: the block's first F bits are filler (a
// transport block's first code block, 36.212 5.1.2; 0 <= F <= 63 and F < K): their d0 and d1, stream positions
// 3k and 3k+1 with k < F, are <NULL> in w; d2 stays, as in the standard.  False on a bad K, Ncb or F.
inline bool rm_build(int K, int Ncb, RmTables& t, int F = 0)
{
    if (K < 1 || K > 10000) return false;
    if (F < 0 || F > 63 || F >= K) return false;
    const int D = K + 4, R = (D + 31) / 32, Kpi = 32 * R, Kw = 3 * Kpi, ND = Kpi - D;
    if (Ncb == 0) Ncb = Kw;
    if (Ncb < Kpi || Ncb > Kw) return false;
    t.K = K, t.R = R, t.Kpi = Kpi, t.Kw = Kw, t.ND = ND, t.Ncb = Ncb;
    int inv[32];
    for (int c = 0; c < 32; ++c) inv[kRmPerm[c]] = c;
    // w as stream positions (-1 = <NULL>): y_j sits in row j / 32, column j % 32; v reads column by
    // column in permuted order, so y_j is v[inv[column] * R + row]
    std::vector<int32_t> w(Kw, -1);
    for (int k = 0; k < D; ++k) {
        const int j = ND + k, m = inv[j % 32] * R + j / 32;
        w[m] = 3 * k;
        w[Kpi + 2 * m] = 3 * k + 1;
        const int j2 = (j + Kpi - 1) % Kpi, m2 = inv[j2 % 32] * R + j2 / 32;   // v2 reads y one further on
        w[Kpi + 2 * m2 + 1] = 3 * k + 2;
        if (k < F) w[m] = w[Kpi + 2 * m] = -1;
    }
    t.rank.assign(3 * D, -1);
    t.pos.clear();
    std::vector<int32_t> before(Ncb + 1);
    for (int i = 0; i < Ncb; ++i) {
        before[i] = (int32_t)t.pos.size();
        if (w[i] >= 0) {
            t.rank[w[i]] = before[i];
            t.pos.push_back(w[i]);
        }
    }
    t.Nnn = (int)t.pos.size();
    const int step = 2 * ((Ncb + 8 * R - 1) / (8 * R));
    for (int rv = 0; rv < 4; ++rv) t.c0[rv] = before[(R * (step * rv + 2)) % Ncb] % t.Nnn;
    return true;
}

// One launch's view of the tables (device pointers) and shape.
struct RmParams {
    int K, R, ND, Nnn, c0;   // c0 of the launch's rv
    int E, B;
    const int32_t* rank;     // [3K+12]
    const int32_t* pos;      // [Nnn]
};

// The launchers are weak references: a host-only link of td_api.cpp that leaves td_ratematch.hip out (the
// sanitizer build of the host ABI checks, tests/test_host_sanitizers.py) still links, and td_rate_match /
// td_rate_dematch then fail with TD_EHIP instead of launching.  libturbo_mi355x.so always has them.
// d_in [B][3K+12] -> d_e [B][E], elements of `elem` bytes (1, 4 or 8; else hipErrorInvalidValue)
__attribute__((weak)) hipError_t launch_rate_match(const RmParams& p, const void* d_in, int elem, void* d_e,
                                                   hipStream_t st);
// d_e [B][E] -> d_out [B][3K+12]
template <typename T>
__attribute__((weak)) hipError_t launch_rate_dematch(const RmParams& p, const T* d_e, T* d_out, int accumulate,
                                                     hipStream_t st);
// td_demod_dematch: d_yi, d_yq [B][E / M] symbols -> d_out [B][3K+12], the values demapped (M = 1, 2, 3, 4, 6
// bits per symbol; else hipErrorInvalidValue) and converted to T where launch_rate_dematch reads d_e.  T =
// double, float, or int8_t (a TD_FIXED handle: quantised at steps_per_unit, every addition saturated to +-127,
// the bytes of launch_fixed_dematch on the quantised values).  p.E is a multiple of M.
template <typename T>
__attribute__((weak)) hipError_t launch_demod_dematch(const RmParams& p, const double* d_yi, const double* d_yq, int M,
                                                      double Kf, double steps_per_unit, T* d_out, int accumulate,
                                                      hipStream_t st);

}  // namespace td
