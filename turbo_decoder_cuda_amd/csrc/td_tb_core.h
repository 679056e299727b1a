// td_tb_core.h -- transport blocks (3GPP TS 36.212 5.1.2, 5.1.4.1.2, 5.1.5): the segmentation plan, the sizes
// of the rate-matched pieces and the index arithmetic between a transport block and its code blocks.
//
// Plain integer C++ shared by td_api.cpp (the planners), by the gfx950 kernels of td_tb.hip and by the
// stand-alone host program of the tests (tests/tb_core_host.cpp, under ASan + UBSan).  The filler-aware
// circular-buffer tables are rm_build's (td_ratematch.h, its F argument); this file says which block, which
// offset and which table an element belongs to.
//
// A transport block of A bits and its gCRC24A are the B = A + 24 bit sequence b.  It is cut into C code
// blocks: the first C_minus of size K_minus, the others of size K_plus.  Block 0 starts with F filler bits
// (zeros, <NULL> in its circular buffer); every block then carries payload = K_r - L bits of b in order,
// and, when C > 1, its own gCRC24B in its last L = 24.  So with t = s + F the position of bit s of b in the
// payload stream, block r holds t in [r P_minus, ...) -- block_start() is that range's first s.
//
// Block-major layout: block r of transport block n is row r N + n of the K_minus array [C_minus][N][K_minus]
// when r < C_minus, else row (r - C_minus) N + n of the K_plus array [C_plus][N][K_plus].
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TDT_HD __host__ __device__ __forceinline__
#else
#define TDT_HD inline
#endif

namespace td {
namespace tb {

constexpr int kZ = 6144;            // the largest code block
constexpr int kMaxA = 1 << 20;      // td_tb_plan_host's largest transport block
constexpr int kValidK = 188;        // code block sizes of table 5.1.3-3
constexpr int kMaxFiller = 63;

struct Plan {
    int A, B, L, C, K_plus, K_minus, C_plus, C_minus, F;
};

// The i-th code block size, i < kValidK, by the table's rule: 40..512 step 8, 528..1024 step 16, 1056..2048
// step 32, 2112..6144 step 64.
TDT_HD int valid_k(int i)
{
    return i < 60 ? 40 + 8 * i : i < 92 ? 512 + 16 * (i - 59) : i < 124 ? 1024 + 32 * (i - 91) : 2048 + 64 * (i - 123);
}

// 5.1.2.  False on an A outside [1, kMaxA].
inline bool plan(int A, Plan& p)
{
    if (A < 1 || A > kMaxA) return false;
    p.A = A, p.B = A + 24;
    long long Bp;
    if (p.B <= kZ)
        p.L = 0, p.C = 1, Bp = p.B;
    else {
        p.L = 24, p.C = (p.B + (kZ - 24) - 1) / (kZ - 24);
        Bp = p.B + (long long)p.C * p.L;
    }
    int i = 0;
    while (i < kValidK - 1 && (long long)p.C * valid_k(i) < Bp) ++i;   // C 6144 >= B' always
    p.K_plus = valid_k(i);
    if (p.C == 1)
        p.C_plus = 1, p.K_minus = 0, p.C_minus = 0;
    else {
        p.K_minus = valid_k(i - 1);   // C > 1: K_plus > 3000, so i > 0
        p.C_minus = (int)(((long long)p.C * p.K_plus - Bp) / (p.K_plus - p.K_minus));
        p.C_plus = p.C - p.C_minus;
    }
    p.F = (int)((long long)p.C_plus * p.K_plus + (long long)p.C_minus * p.K_minus - Bp);
    return true;
}

TDT_HD int block_k(const Plan& p, int r) { return r < p.C_minus ? p.K_minus : p.K_plus; }
// bits of b a block carries
TDT_HD int block_payload(const Plan& p, int r) { return block_k(p, r) - p.L; }
// The index in b of the bit at offset 0 of block r; -F for block 0: its first F offsets are the filler.
TDT_HD int block_start(const Plan& p, int r)
{
    const int pm = p.K_minus - p.L, pp = p.K_plus - p.L;
    return (r < p.C_minus ? r * pm : p.C_minus * pm + (r - p.C_minus) * pp) - p.F;
}
// row of block r of transport block n in its size's array, N transport blocks a call
TDT_HD size_t block_row(const Plan& p, int r, size_t n, size_t N)
{
    return (size_t)(r < p.C_minus ? r : r - p.C_minus) * N + n;
}

// What segmentation puts at offset i of block r.
enum SegKind { kSegFiller = 0, kSegTb = 1, kSegTbCrc = 2, kSegCbCrc = 3 };
struct SegSrc {
    int kind;   // SegKind
    int idx;    // kSegTb: the transport block's bit; kSegTbCrc: the gCRC24A bit (0 = most significant);
                // kSegCbCrc: the block's gCRC24B bit; kSegFiller: 0
};
TDT_HD SegSrc seg_src(const Plan& p, int r, int i)
{
    const int pay = block_payload(p, r);
    if (i >= pay) return SegSrc{kSegCbCrc, i - pay};
    const int s = block_start(p, r) + i;
    if (s < 0) return SegSrc{kSegFiller, 0};
    return s < p.A ? SegSrc{kSegTb, s} : SegSrc{kSegTbCrc, s - p.A};
}

// Where bit s of b (s < B) sits: block r, offset i (< its payload).
struct Loc {
    int r, i;
};
TDT_HD Loc locate(const Plan& p, int s)
{
    const int pm = p.K_minus - p.L, pp = p.K_plus - p.L;
    int t = s + p.F;
    if (t < p.C_minus * pm) return Loc{t / pm, t % pm};
    t -= p.C_minus * pm;
    return Loc{p.C_minus + t / pp, t % pp};
}

// 5.1.4.1.2: the first n_lo blocks send E_lo values each, the others E_hi; row n of the concatenation
// (5.1.5) is e_0 | e_1 | ... | e_{C-1}, G values.
struct RmSizes {
    int E_lo, E_hi, n_lo;
};
// False if G is not a positive multiple of NlQm below 2^31 or G' = G / NlQm < C.
inline bool rm_sizes(int C, long long G, int NlQm, RmSizes& s)
{
    if (C < 1 || NlQm < 1 || G < 1 || G > 0x7FFFFFFFll || G % NlQm) return false;
    const long long Gp = G / NlQm;
    if (Gp < C) return false;
    const int gamma = (int)(Gp % C);
    s.E_lo = (int)(NlQm * (Gp / C));
    s.E_hi = (int)(NlQm * ((Gp + C - 1) / C));
    s.n_lo = C - gamma;
    return true;
}
TDT_HD int e_size(const RmSizes& s, int r) { return r < s.n_lo ? s.E_lo : s.E_hi; }
// the offset of e_r in a row of the concatenation
TDT_HD long long e_start(const RmSizes& s, int r)
{
    return r < s.n_lo ? (long long)r * s.E_lo : (long long)s.n_lo * s.E_lo + (long long)(r - s.n_lo) * s.E_hi;
}
// element g (< G) of a row of the concatenation: block r, and k: it is e_r[k]
TDT_HD Loc e_locate(const RmSizes& s, long long g)
{
    const long long lo = (long long)s.n_lo * s.E_lo;
    if (g < lo) return Loc{(int)(g / s.E_lo), (int)(g % s.E_lo)};
    g -= lo;
    return Loc{s.n_lo + (int)(g / s.E_hi), (int)(g % s.E_hi)};
}

}  // namespace tb
}  // namespace td
