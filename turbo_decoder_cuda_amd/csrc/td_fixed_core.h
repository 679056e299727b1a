// td_fixed_core.h -- the arithmetic of the fixed-point decoder (TD_FIXED), one codeword per caller.
//
// Plain integer C++ shared by the gfx950 kernel of td_fixed.hip (one codeword per lane) and by the
// stand-alone host program of the tests (tests/fixed_core_host.cpp, under ASan + UBSan): the functions
// only read and write through FxArgs, whose arrays are laid out [row][Bp] with the codeword as the
// fastest index.  The library never decodes on the host.
//
// Metrics.  The branch metric is twice the float decoder's: gamma_u(s) = (2u-1) S + o_u(s) P with
// S = xs + La, P = xp.  |xs|, |xp| <= 127 and |La| <= le_max <= 255, so |gamma| <= 509.  State metrics
// are int32 and are never normalised: after i steps |alpha| <= 509 i <= 509 * 10003 < 2^23, the same
// for beta, and |alpha + gamma + beta| < 2^24.  An unreachable state is kNeg = -2^28: sums of up to two
// of them and a reachable part stay above -2^30, so nothing wraps, and no sum that contains one
// reaches a reachable path's (>= -2^24).  Nothing saturates except the two clamps of the contract
// (the input's -128 -> -127 and the extrinsic's +-le_max).  With td_set_fixed_maxstar's correction table
// (MaxStar below) a step adds up to 63 more: the same bounds hold, as worked out there.
#pragma once

#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define TDF_HD __host__ __device__ __forceinline__
#else
#define TDF_HD inline
#endif

namespace td {
namespace fx {

constexpr int kW = 16;               // trellis steps per recomputation window (alpha rows held in registers)
constexpr int kNeg = -(1 << 28);     // an unreachable state

// The LTE constituent code (feedback 13, forward 15 octal) as gen_trellis builds it (td_tables.h
// build_trellis): state s = (r0 r1 r2) with r0 the newest register bit in bit 2.
constexpr int fb(int s, int u) { return u ^ ((s >> 1) & 1) ^ (s & 1); }                 // the register's input bit
constexpr int next_state(int s, int u) { return (fb(s, u) << 2) | (s >> 1); }
constexpr int parity(int s, int u) { return 2 * (fb(s, u) ^ ((s >> 2) & 1) ^ (s & 1)) - 1; }   // o_u(s) = +-1
constexpr int prev_state(int j, int u) { return next_state(2 * (j & 3), u) == j ? 2 * (j & 3) : 2 * (j & 3) + 1; }

struct FxArgs {
    const int8_t* xs;     // [L+3][Bp] rows 0..L-1: systematic of SISO1 (natural order, tail included);
                          //           rows L..L+2: the systematic tail of SISO2
    const int8_t* xp1;    // [L][Bp]
    const int8_t* xp2;    // [L][Bp]
    int16_t* ext12;       // [K][Bp] Le of SISO1 by natural position
    int16_t* ext21;       // [K][Bp] Le of SISO2 by interleaved position
    int32_t* ckpt;        // [nW][8][Bp] alpha at the start of every window
    uint8_t* bitsT;       // [rows][K][Bp] hard decisions by natural position (the stopping decoder: by interleaved
                          //                 position, a row per iteration)
    int16_t* le;          // nullable, the caller's [B][iters][2][L]
    const int* pi;        // [K]
    const int* pinv;      // [K]
    int K, L, B, iters, all_iters;
    int le_max, scale_q;
    size_t Bp;            // codewords of the padded batch (the row pitch)
};

// Early termination (td_set_fixed_stop, and td_set_fixed_window_stop on the sub-block schedule), next to
// FxArgs and not in it: tests/fixed_host_common.h initialises FxArgs member by member.
struct FxStop {
    int rule;             // 1: the rows repeat (HDA), 2: the row's CRC-24 is zero (enum td_stop_rule)
    int first;            // the smallest iteration count a codeword may stop after: max(HDA ? 2 : 1, min_iters)
    const int* syn;       // [K] CRC, by interleaved position i: the remainder of the row with only bit pi(i) set
                          //     (td_crc.h's syndrome[pi[i]]), as bit patterns
    int32_t* used;        // [Bp] the iterations each codeword took (the sub-block schedule: 0 while it runs)
};

// f of the contract: towards zero, symmetric in sign, clamped
TDF_HD int ext_f(int r, int le_max, int scale_q)
{
    int m = ((r < 0 ? -r : r) * scale_q) >> 2;
    m = m < le_max ? m : le_max;
    return r < 0 ? -m : m;
}

TDF_HD int imax(int a, int b) { return a > b ? a : b; }

// The max of the recursions and of the two folds of Lambda, a compile-time choice through the lane code.
// MaxLog is the contract's plain max (Max-Log-MAP).  MaxStar is td_set_fixed_maxstar's integer log-MAP:
//   maxs(a, b) = max(a, b) + corr[min(|a - b| >> shift, 7)],  corr[j] <= 63, corr[7] == 0
// with the eight entries packed a byte each into two words (lo: buckets 0..3, hi: 4..7), next to FxArgs
// and not in it, as FxStop and FxWindow are.  The words and the shift are kernel arguments, the same in
// every lane: they stay in scalar registers and the entry is one byte permute of them -- no LDS, no memory.
// maxs rounds, so it is not associative: the order of the operands and of the folds below is the
// contract's (include/turbo_mi355x.h).
//
// Bounds with a table.  A step adds at most 509 + 63 to a metric, so after i steps |alpha| <=
// 572 * 10003 < 2^23 (5.73e6 < 8.39e6), the same for beta; a Lambda term is alpha + gamma + beta plus the
// seven corrections of its fold, |.| <= 2 * 572 * 10003 + 509 + 441 < 2^24.  A warm-up from equal metrics
// (all 0) is inside the same bounds: its metrics are at most 572 per step from 0.  corr[7] == 0 makes
// maxs of a reachable sum (>= -2^24) and one that holds kNeg (<= kNeg + 2^24, more than 7 * 2^8 below it)
// the reachable sum exactly; maxs of two sums that hold kNeg adds at most 63 to one of them, and a fold
// at most 441: still above -2^30 and below every reachable sum.  So int32 and kNeg stay as they are.
struct MaxLog {
    static constexpr bool kTable = false;
    TDF_HD int operator()(int a, int b) const { return imax(a, b); }
};

struct MaxStar {
    static constexpr bool kTable = true;
    uint32_t lo, hi;      // corr[0..3], corr[4..7], entry j in byte j & 3
    int shift;            // bucket width 2^shift, 0 .. 8
    TDF_HD int operator()(int a, int b) const
    {
        const int mx = a > b ? a : b, mn = a > b ? b : a;
        unsigned j = (unsigned)(mx - mn) >> shift;   // the difference of two int32 metrics of the bounds above: no wrap
        j = j < 7u ? j : 7u;
#if defined(__HIP_DEVICE_COMPILE__)
        return mx + (int)(__builtin_amdgcn_perm(hi, lo, j) & 0xffu);   // byte j of hi:lo
#else
        return mx + (int)(((j < 4 ? lo : hi) >> (8 * (j & 3))) & 0xffu);
#endif
    }
};

// LLR = Lambda / 2 towards zero, as f truncates.  Max-Log-MAP's Lambda is even: there it is the shift.
template <class M>
TDF_HD int half_lambda(int lam)
{
    return M::kTable ? lam / 2 : lam >> 1;
}

// An interleaver entry.  The tables do not change while a decode runs and the index is the same for
// the whole wave, so the device reads them through the constant address space: a scalar load, whose
// result (a row number) stays in a scalar register and makes the row's address a scalar too.
TDF_HD int table_entry(const int* tbl, int i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const int __attribute__((address_space(4))) * const_ptr;
    return ((const_ptr)tbl)[i];
#else
    return tbl[i];
#endif
}

// the four values a branch metric takes: index 2u + (o_u(s) > 0)
TDF_HD void gammas(int S, int P, int (&c)[4])
{
    c[0] = -S - P;
    c[1] = -S + P;
    c[2] = S - P;
    c[3] = S + P;
}
constexpr int gsel(int s, int u) { return 2 * u + (parity(s, u) > 0 ? 1 : 0); }

template <class M = MaxLog>
TDF_HD void alpha_step(const int (&a)[8], int S, int P, int (&n)[8], const M& mx = M())
{
    int c[4];
    gammas(S, P, c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p0 = prev_state(j, 0), p1 = prev_state(j, 1);
        n[j] = mx(a[p0] + c[gsel(p0, 0)], a[p1] + c[gsel(p1, 1)]);
    }
}

TDF_HD void copy8(int (&a)[8], const int (&n)[8])
{
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = n[s];
}

// One beta step backwards over position i's branch metrics, without an output (the warm-up).
template <class M = MaxLog>
TDF_HD void beta_step(int (&bt)[8], int S, int P, const M& mx = M())
{
    int c[4];
    gammas(S, P, c);
    int n[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) n[s] = mx(c[gsel(s, 0)] + bt[next_state(s, 0)], c[gsel(s, 1)] + bt[next_state(s, 1)]);
    copy8(bt, n);
}

// S = xs + La and P = xp of position i (i < L) of SISO `DEC` in iteration `it`
template <int DEC>
TDF_HD void load_step(const FxArgs& p, size_t b, int it, int i, int& S, int& P)
{
    const int K = p.K;
    if (DEC == 0) {
        int la = 0;
        if (it > 0 && i < K) la = p.ext21[(size_t)table_entry(p.pinv, i) * p.Bp + b];
        S = p.xs[(size_t)i * p.Bp + b] + la;
        P = p.xp1[(size_t)i * p.Bp + b];
    } else {
        int la = 0;
        size_t row = (size_t)i + 3;   // tail: rows L .. L+2 = K+3 ..
        if (i < K) {
            row = (size_t)table_entry(p.pi, i);
            la = p.ext12[row * p.Bp + b];
        }
        S = p.xs[row * p.Bp + b] + la;
        P = p.xp2[(size_t)i * p.Bp + b];
    }
}

// alpha over the sixteen positions from i, their loads ahead of the arithmetic
template <int DEC, class M>
TDF_HD void alpha_block(const FxArgs& p, size_t b, int it, int i, int (&a)[8], const M& mx)
{
    int S[kW], P[kW];
#pragma unroll
    for (int t = 0; t < kW; ++t) load_step<DEC>(p, b, it, i + t, S[t], P[t]);
#pragma unroll
    for (int t = 0; t < kW; ++t) {
        int n[8];
        alpha_step(a, S[t], P[t], n, mx);
        copy8(a, n);
    }
}

// beta over the sixteen positions below i, i - 1 first (the warm-up), their loads ahead of the arithmetic
template <int DEC, class M>
TDF_HD void beta_block(const FxArgs& p, size_t b, int it, int i, int (&bt)[8], const M& mx)
{
    int S[kW], P[kW];
#pragma unroll
    for (int t = 0; t < kW; ++t) load_step<DEC>(p, b, it, i - 1 - t, S[t], P[t]);
#pragma unroll
    for (int t = 0; t < kW; ++t) beta_step(bt, S[t], P[t], mx);
}

// The sub-block schedule (td_set_fixed_window), next to FxArgs and not in it, as FxStop is.
struct FxWindow {
    int window;           // W: a multiple of kW, so that a sub-block is a run of whole recomputation windows
    int overlap;          // warm-up steps before a sub-block's start and after its end, any number >= 0
};

constexpr int window_blocks(int L, int window) { return L / window > 1 ? L / window : 1; }

// Next-iteration initialisation (td_set_fixed_window_nii), next to FxArgs and not in it.  In iterations
// after the first a warm-up that does not begin at a trellis end starts from the vector that the
// neighbouring chain had at that position one iteration earlier.  With the overlap a multiple of kW those
// positions are starts of 16-step windows (or a sub-block's own end), so the stores sit between the
// windows' step loops and their conditions are the wave's.  A vector is stored relative to its maximum,
// two int16 a word, in the slot of the sub-block that will start from it: every consumer has one alpha
// slot and one beta slot per SISO and parity of the iteration.
//
// Bounds.  Every stored vector has run at least kW steps from its start, except beta inside the last
// three positions of the trellis.  Three steps reach every state from every state, so three steps after
// a vector whose maximum was m every state is at least m - 3 * 509 and at most m + 3 * (509 + 63): the
// spread of the reachable states is at most 3 * (2 * 509 + 63) = 3243, and the one or two steps next to
// the termination spread the states they reach by less.  An unreachable state is below kNeg + 2^24,
// more than 2^27 under the maximum.  So a difference below -32767 means unreachable: it is stored as
// -32768 and loaded as kNeg, and every other difference fits int16 exactly.  A loaded vector lies in
// [-3243, 0] (or is kNeg), and from there a recursion runs at most min(3 W + 2 W + 2, L) steps: |metric| <=
// 3243 + 572 * 10003 < 2^23 and a Lambda term stays below 2^24, the bounds at the head of this file,
// whatever the number of iterations.
struct FxNii {
    const uint32_t* rd;   // [2][nS][4][Bp]: alpha slots, then beta slots, as this SISO left them in iteration it - 1
    uint32_t* wr;         // the same of this iteration: the other parity, so no launch reads a word that it writes
    int q, r;             // overlap / window and overlap % window
};

// words of the NII state: [parity 2][SISO 2][alpha, beta][nS][4][Bp]
constexpr size_t nii_words(int L, int window, size_t Bp) { return (size_t)32 * window_blocks(L, window) * Bp; }

// the arguments of SISO `dec` in iteration `it` over the state at base
inline FxNii nii_args(uint32_t* base, int L, const FxWindow& wn, size_t Bp, int it, int dec)
{
    const size_t reg = nii_words(L, wn.window, Bp) / 4;
    return FxNii{base + (size_t)(((it + 1) & 1) * 2 + dec) * reg, base + (size_t)((it & 1) * 2 + dec) * reg,
                 wn.overlap / wn.window, wn.overlap % wn.window};
}

TDF_HD void nii_store(uint32_t* slot, size_t Bp, size_t b, const int (&v)[8])
{
    int m = v[0];
#pragma unroll
    for (int s = 1; s < 8; ++s) m = imax(m, v[s]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int lo = v[2 * j] - m, hi = v[2 * j + 1] - m;
        lo = lo < -32767 ? -32768 : lo;
        hi = hi < -32767 ? -32768 : hi;
        slot[(size_t)j * Bp + b] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
    }
}

TDF_HD void nii_load(const uint32_t* slot, size_t Bp, size_t b, int (&v)[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t w = slot[(size_t)j * Bp + b];
        const int lo = (int16_t)(w & 0xffffu), hi = (int16_t)(w >> 16);
        v[2 * j] = lo == -32768 ? kNeg : lo;
        v[2 * j + 1] = hi == -32768 ? kNeg : hi;
    }
}

// The positions one call of siso_span covers.  A span over [0, L) that starts at both ends of the trellis
// is the exact schedule's pass; sub-block sb of the sub-block schedule is window_span's.
struct FxSpan {
    int start, end;       // the call's own positions, start a multiple of kW: a run of recomputation windows
    int a_from, b_from;   // alpha warms up over [a_from, start) and beta over [end, b_from); a recursion that
                          // starts at the trellis' end (a_from == 0, b_from == L) starts from the terminated state
    int sb, nS, W;        // the sub-block's index, their number and their width: the row of ev, the slots of NII
};

// Sub-block sb: positions [sb W, (sb + 1) W), the last sub-block up to L.  alpha warms up from
// max(sb W - overlap, 0) and beta from min(end + overlap, L).
TDF_HD FxSpan window_span(int L, const FxWindow& wn, int sb)
{
    const int nS = window_blocks(L, wn.window);
    const int start = sb * wn.window, end = sb == nS - 1 ? L : start + wn.window;
    return FxSpan{start, end, start - wn.overlap <= 0 ? 0 : start - wn.overlap,
                  end + wn.overlap >= L ? L : end + wn.overlap, sb, nS, wn.window};
}

// HDA's previous bits of the window at i0 for the exact stopping decoder: sixteen bytes of a row of bitsT
// (prev is the row's entry of the lane's codeword), bit t = the bit of position i0 + t.  No branch per
// step: sixteen loads in flight, the tail's masked off.
TDF_HD unsigned row_bits(const uint8_t* prev, size_t Bp, int K, int i0)
{
    unsigned was = 0;
#pragma unroll
    for (int t = 0; t < kW; ++t) {
        const int i = i0 + t < K ? i0 + t : K - 1;
        was |= (unsigned)prev[(size_t)i * Bp] << t;
    }
    const int nv = K - i0;   // the window's positions below K
    return was & (nv >= kW ? (1u << kW) - 1 : nv > 0 ? (1u << nv) - 1 : 0u);
}

// SISO `DEC` of iteration `it` over the positions [g.start, g.end) of codeword b (Max-Log-MAP, or log-MAP
// with mx a MaxStar), with everything that follows it in the iteration: the extrinsic (ext12 / ext21 and
// the caller's Le), and after SISO2 the hard decisions.  A recursion that starts at the trellis' end starts
// from the terminated state, any other from equal metrics (all 0: never normalised, so the sums stay inside
// the bounds at the head of this file).  The warm-ups take any start: sixteen steps at a time with their
// loads ahead of the arithmetic, then the rest one by one.  The span's own steps: alpha checkpoints at
// ckpt[w], w the window's index in the whole trellis (sub-blocks own disjoint slots), then per window,
// backwards, alpha again from its checkpoint, beta, Lambda, f and the stores.  g must be the same in every
// lane of a wave.  Sub-blocks of one SISO read ext / xs / xp anywhere and write only their own positions of
// the other ext array, so they may run in any order or at once; the next SISO may start when all of them
// are done.
//
// STOP (the stopping decoders, sp their rule; the caller runs only the lanes whose codeword has not
// stopped): SISO2 writes row `it` of bitsT in every iteration, and in a judged iteration
// (it + 1 >= sp->first) makes the rule's evidence on the span's own positions below K, zero where the
// codeword may stop: HDA the bits that differ from row it - 1 (OR over the windows), CRC the XOR of
// syn[i] over the 1 bits.  Both rules hold in any fixed order of the bits, so the stopping decoders keep
// bitsT in SISO2's own order, by interleaved position i: the stores and the rule need no entry of pi (a
// scalar load and its wait in every step otherwise), and the transpose back undoes the order
// (fx_bits_stop_kernel reads row pinv[k]).  The window's new bits are packed one bit a step into a
// register and compared with its previous bits at its end; the state is the evidence and two bit masks.
// SUB chooses where the previous bits come from and where the evidence goes:
//   the exact schedule (SUB false) loads the window's sixteen bytes of row it - 1 with the window's inputs
//     (row_bits) -- sixteen loads in flight ahead of the arithmetic, not one per step behind a store that
//     the compiler must assume aliases it; the previous row stays in the workspace.  It packs the new bits
//     only in a judged iteration and returns the evidence to decode_codeword_stop.
//   the sub-block schedule (SUB true) does not read them back from bitsT: sixteen byte loads a window cost
//     this schedule, which keeps the chip full, 16-20 % of the decode where nothing converges.  A lane
//     leaves the sixteen bits of each of its 16-step windows packed at hist[w][b] (w the window's index in
//     the whole trellis, as for ckpt) when the next iteration is judged, and the window's previous bits are
//     one 16-bit load together with the window's inputs; the slot is the lane's own, read before it is
//     written.  It packs the new bits whenever the rule is HDA and stores the evidence at ev[sb][b]: the
//     codeword's is the fold of its sub-blocks' words, which the launch after SISO2's makes
//     (fx_window_judge_kernel): no atomics, and no launch reads a word of ev that it writes.
//
// NII (td_set_fixed_window_nii, ni its state): in iterations after the first a warm-up that does not start at
// a trellis end loads its start vector from the sub-block's own slot, and the sub-block stores the vectors
// that others will start from in the next iteration.  With g = q W + r, sub-block sb's chain holds
//   A[(sb + 1) W - r], the start of sub-block sb + 1 + q: a window start of the forward pass, or for r = 0
//                      the sub-block's own end, one alpha step past the last window's recompute;
//   B[sb W + r],       the start of sub-block sb - 1 - q, and in the last sub-block, whose positions run
//                      past (sb + 1) W, also B[(sb + 1) W + r], the start of sub-block sb - q;
// bt after the backward loop's window that begins there.  The last sub-block holds no A, as nothing starts
// to its right.  Every slot that is loaded was stored by the launch of this SISO one iteration earlier.
template <int DEC, bool STOP, bool NII, bool SUB, class M>
TDF_HD int siso_span(const FxArgs& p, const FxSpan g, const FxStop* sp, uint32_t* ev, uint16_t* hist, const FxNii* ni,
                     size_t b, int it, const M& mx)
{
    const int L = p.L, K = p.K;
    const bool live = b < (size_t)p.B;   // a lane of the padding decodes zeros and stores nothing outside the workspace
    const int start = g.start, end = g.end, sb = g.sb, nS = g.nS;
    const bool a_term = g.a_from == 0, b_term = g.b_from == L;
    const int w0 = start / kW, w1 = (end + kW - 1) / kW;   // the span's recomputation windows
    // NII: the positions whose vectors this sub-block stores (-1: none) and the consumers' slots
    int a_st = -1, a_slot = 0, b_st0 = -1, b_st1 = -1, b_slot = 0;
    if (NII && it + 1 < p.iters) {
        a_slot = sb + 1 + ni->q;
        if (a_slot <= nS - 1) a_st = start + g.W - ni->r;
        b_slot = sb - 1 - ni->q;
        if (b_slot >= 0) b_st0 = start + ni->r;
        if (sb == nS - 1 && ni->q >= 1 && b_slot + 1 >= 0 && start + g.W + ni->r < L) b_st1 = start + g.W + ni->r;
    }

    // forward: the warm-up, then alpha at every window start
    {
        int a[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) a[s] = s && a_term ? kNeg : 0;
        if (NII && it > 0 && !a_term) nii_load(ni->rd + (size_t)sb * 4 * p.Bp, p.Bp, b, a);
        int i = g.a_from;
        for (; i + kW <= start; i += kW) alpha_block<DEC>(p, b, it, i, a, mx);
        for (; i < start; ++i) {
            int S, P, n[8];
            load_step<DEC>(p, b, it, i, S, P);
            alpha_step(a, S, P, n, mx);
            copy8(a, n);
        }
        for (int w = w0; w < w1; ++w) {
#pragma unroll
            for (int s = 0; s < 8; ++s) p.ckpt[((size_t)w * 8 + s) * p.Bp + b] = a[s];
            if (NII && w * kW == a_st) nii_store(ni->wr + (size_t)a_slot * 4 * p.Bp, p.Bp, b, a);
            if (w == w1 - 1) break;   // a window that is not the span's last is whole
            alpha_block<DEC>(p, b, it, w * kW, a, mx);
        }
    }

    // backward: the warm-up, then per window alpha again from its checkpoint, beta and the outputs
    int bt[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) bt[s] = s && b_term ? kNeg : 0;
    if (NII && it > 0 && !b_term) nii_load(ni->rd + (size_t)(nS + sb) * 4 * p.Bp, p.Bp, b, bt);
    {
        int i = g.b_from;
        for (; i - kW >= end; i -= kW) beta_block<DEC>(p, b, it, i, bt, mx);
        for (; i > end; --i) {
            int S, P;
            load_step<DEC>(p, b, it, i - 1, S, P);
            beta_step(bt, S, P, mx);
        }
    }
    const int row = STOP || p.all_iters ? it : 0;
    const bool want_bits = DEC == 1 && (STOP || p.all_iters || it == p.iters - 1);
    const bool judge = STOP && DEC == 1 && it + 1 >= sp->first;   // iterations before sp->first are not judged
    const bool hda = STOP && DEC == 1 && sp->rule == 1;
    const bool pack = SUB ? hda : hda && judge;
    int acc = 0;
    for (int w = w1 - 1; w >= w0; --w) {
        const int i0 = w * kW;
        int S[kW], P[kW];
#pragma unroll
        for (int t = 0; t < kW; ++t) {
            const int i = i0 + t < L ? i0 + t : L - 1;   // past the end (last window): a valid row, never used
            load_step<DEC>(p, b, it, i, S[t], P[t]);
        }
        unsigned was = 0, now = 0;   // HDA: bit t = the bit of position i0 + t in row it - 1, in row it
        if (STOP && judge && hda)    // first >= 2: row it - 1 exists
            was = SUB ? hist[(size_t)w * p.Bp + b] : row_bits(p.bitsT + (size_t)(row - 1) * K * p.Bp + b, p.Bp, K, i0);
        int A[kW][8];
#pragma unroll
        for (int s = 0; s < 8; ++s) A[0][s] = p.ckpt[((size_t)w * 8 + s) * p.Bp + b];
#pragma unroll
        for (int t = 0; t + 1 < kW; ++t) alpha_step(A[t], S[t], P[t], A[t + 1], mx);
        if (NII && a_st == end && w == w1 - 1) {   // the sub-block's own end: its last window is whole
            int n[8];
            alpha_step(A[kW - 1], S[kW - 1], P[kW - 1], n, mx);
            nii_store(ni->wr + (size_t)a_slot * 4 * p.Bp, p.Bp, b, n);
        }
#pragma unroll
        for (int t = kW - 1; t >= 0; --t) {
            const int i = i0 + t;
            if (i < L) {
                int c[4];
                gammas(S[t], P[t], c);
                int e0[8], e1[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    e0[s] = c[gsel(s, 0)] + bt[next_state(s, 0)];
                    e1[s] = c[gsel(s, 1)] + bt[next_state(s, 1)];
                }
                int m0 = A[t][0] + e0[0], m1 = A[t][0] + e1[0];
#pragma unroll
                for (int s = 1; s < 8; ++s) {
                    m0 = mx(m0, A[t][s] + e0[s]);
                    m1 = mx(m1, A[t][s] + e1[s]);
                }
                const int llr = half_lambda<M>(m1 - m0);
                const int le = ext_f(llr - S[t], p.le_max, p.scale_q);
                if (i < K) (DEC == 0 ? p.ext12 : p.ext21)[(size_t)i * p.Bp + b] = (int16_t)le;
                if (p.le && live) p.le[(((size_t)b * p.iters + it) * 2 + DEC) * L + i] = (int16_t)le;
                if (!STOP) {
                    if (want_bits && i < K)
                        p.bitsT[((size_t)row * K + (size_t)table_entry(p.pi, i)) * p.Bp + b] = llr < 0 ? 0 : 1;
                } else if (want_bits && i < K) {
                    const int bit = llr < 0 ? 0 : 1;
                    p.bitsT[((size_t)row * K + (size_t)i) * p.Bp + b] = (uint8_t)bit;
                    if (pack)
                        now |= (unsigned)bit << t;
                    else if (judge && !hda)   // CRC: the syndrome of every 1 bit, from a table in the same order
                        acc ^= -bit & table_entry(sp->syn, i);
                }
#pragma unroll
                for (int s = 0; s < 8; ++s) bt[s] = mx(e0[s], e1[s]);
            }
        }
        if (STOP && hda) {
            if (judge) acc |= (int)(was ^ now);
            if (SUB && it + 2 >= sp->first && it + 1 < p.iters)   // there is a next iteration, and it is judged
                hist[(size_t)w * p.Bp + b] = (uint16_t)now;
        }
        if (NII && (i0 == b_st0 || i0 == b_st1))
            nii_store(ni->wr + (size_t)(nS + (i0 == b_st0 ? b_slot : b_slot + 1)) * 4 * p.Bp, p.Bp, b, bt);
    }
    if (SUB && STOP && judge) ev[(size_t)sb * p.Bp + b] = (uint32_t)acc;
    return acc;
}

// The exact schedule's pass: one terminated span over the whole trellis.  With STOP it returns the rule's
// evidence on row `it`, zero where the codeword may stop.
template <int DEC, bool STOP, class M = MaxLog>
TDF_HD int siso_pass(const FxArgs& p, const FxStop* sp, size_t b, int it, const M& mx = M())
{
    return siso_span<DEC, STOP, false, false>(p, FxSpan{0, p.L, 0, p.L, 0, 1, p.L}, sp, nullptr, nullptr, nullptr, b, it, mx);
}

template <class M = MaxLog>
TDF_HD void decode_codeword(const FxArgs& p, size_t b, const M& mx = M())
{
    for (int it = 0; it < p.iters; ++it) {
        siso_pass<0, false>(p, nullptr, b, it, mx);
        siso_pass<1, false>(p, nullptr, b, it, mx);
    }
}

// true if `run` holds in any lane of the wave (on the host: for the one codeword of the call)
TDF_HD bool any_lane(bool run)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(run) != 0;
#else
    return run;
#endif
}

// decode_codeword with early termination.  Codeword b stops after the first judged iteration whose
// evidence is zero, else after p.iters; from then on its lane is skipped by a branch and writes
// nothing more: bitsT holds rows 0 .. used - 1, and the rows a caller sees beyond them are the copies
// that the transpose back makes (fx_bits_stop_kernel).  The loop's exit is the wave's: it leaves once
// none of its lanes runs, so `it` and every table index stay uniform.  A lane of the padding never
// runs (its zeros decode to an all-ones row, which no CRC passes).
template <class M = MaxLog>
TDF_HD void decode_codeword_stop(const FxArgs& p, const FxStop& s, size_t b, const M& mx = M())
{
    bool run = b < (size_t)p.B;
    int used = p.iters;
    for (int it = 0; it < p.iters; ++it) {
        if (run) {
            siso_pass<0, true>(p, &s, b, it, mx);
            const int acc = siso_pass<1, true>(p, &s, b, it, mx);
            if (it + 1 >= s.first && acc == 0) {
                used = it + 1;
                run = false;
            }
        }
        if (!any_lane(run)) break;
    }
    s.used[b] = used;
}

// One lane of the sub-block kernels: SISO `DEC` of iteration `it`, sub-block sb of codeword b, the span of
// window_span.  sb must be the same in every lane of a wave.  Without STOP s, ev and hist are not read, and
// without NII ni is not.
// STOP: s.used is the state that the decode resets to 0 at its start: 0 = running, n = stopped after n
// iterations.  A wave none of whose lanes runs returns on the ballot -- where the time is saved -- and a
// stopped lane of a running wave is skipped by a branch and writes nothing; a lane of the padding never
// runs.  With NII too: a codeword that runs in iteration `it` ran in it - 1, so its slots hold its own vectors.
template <int DEC, bool STOP, bool NII, class M>
TDF_HD void siso_window_pass(const FxArgs& p, const FxWindow& wn, const FxStop& s, uint32_t* ev, uint16_t* hist,
                             const FxNii& ni, size_t b, int it, int sb, const M& mx)
{
    if (STOP) {
        const bool run = b < (size_t)p.B && s.used[b] == 0;
        if (!any_lane(run) || !run) return;
    }
    siso_span<DEC, STOP, NII, true>(p, window_span(p.L, wn, sb), &s, ev, hist, &ni, b, it, mx);
}

// The entry with one setting's arguments alone -- none, NII, a rule -- for a caller that knows its setting when
// it is written: the host program of the tests, a lane at a time.  The kernels take all arguments and use the
// entry above.
template <int DEC, class M = MaxLog>
TDF_HD void siso_window_pass(const FxArgs& p, const FxWindow& wn, size_t b, int it, int sb, const M& mx = M())
{
    siso_window_pass<DEC, false, false>(p, wn, FxStop{}, nullptr, nullptr, FxNii{}, b, it, sb, mx);
}

template <int DEC, class M = MaxLog>
TDF_HD void siso_window_pass_nii(const FxArgs& p, const FxWindow& wn, const FxNii& ni, size_t b, int it, int sb,
                                 const M& mx = M())
{
    siso_window_pass<DEC, false, true>(p, wn, FxStop{}, nullptr, nullptr, ni, b, it, sb, mx);
}

template <int DEC, class M = MaxLog>
TDF_HD void siso_window_stop(const FxArgs& p, const FxWindow& wn, const FxStop& s, uint32_t* ev, uint16_t* hist, size_t b,
                             int it, int sb, const M& mx = M())
{
    siso_window_pass<DEC, true, false>(p, wn, s, ev, hist, FxNii{}, b, it, sb, mx);
}

// The decision after SISO2's launch of iteration `it`, one call per codeword: a running codeword stops
// after n = it + 1 iterations if n >= s.first and the fold of its nS sub-blocks' evidence (OR for HDA,
// XOR for CRC) is zero, and at n = p.iters in any case.
TDF_HD void window_judge(const FxArgs& p, const FxStop& s, const uint32_t* ev, int nS, size_t b, int it)
{
    if (b >= (size_t)p.B || s.used[b] != 0) return;
    const int n = it + 1;
    bool stop = n == p.iters;
    if (!stop && n >= s.first) {
        const bool hda = s.rule == 1;
        uint32_t acc = 0;
        int sb = 0;
        for (; sb + 8 <= nS; sb += 8) {   // eight loads in flight: one thread's fold is a chain of load latencies
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ev[(size_t)(sb + j) * p.Bp + b];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = hda ? acc | v[j] : acc ^ v[j];
        }
        for (; sb < nS; ++sb) {
            const uint32_t v = ev[(size_t)sb * p.Bp + b];
            acc = hda ? acc | v : acc ^ v;
        }
        stop = acc == 0;
    }
    if (stop) s.used[b] = n;
}

}  // namespace fx
}  // namespace td
