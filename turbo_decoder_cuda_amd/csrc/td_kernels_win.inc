// td_kernels_win.inc -- the windowed schedule's three recursion kernels (sw_alpha_kernel,
// sw_alpha_lps_kernel, sw_beta_kernel), textually included twice by td_kernels.hip: once as they
// always were, and once with SW_STOP_BUILD as the stopping variants sw_*_stop_kernel of
// td_set_window_stop, which take one further argument (SwStop).  Two inclusions rather than a
// `bool STOP` template over a shared body: the default kernels' parameter blocks and code stay
// exactly the ones built before the stopping variants existed (a shared inlined body that takes the
// kernel arguments by reference compiled them differently).  Everything the variants add stands under
// `if constexpr (STOP)`.
#ifdef SW_STOP_BUILD
#define SW_KERNEL(name) name##_stop_kernel
#define SW_STOP_PARAM , SwStop sp_
#define SW_STOP_DECL                 \
    constexpr bool STOP = true;      \
    const SwStop* const sp = &sp_;
#else
#define SW_KERNEL(name) name##_kernel
#define SW_STOP_PARAM
#define SW_STOP_DECL                 \
    constexpr bool STOP = false;     \
    const SwStop* const sp = nullptr;
#endif

// ---- alpha: forward over the run, checkpoints every S positions of each sub-block
// (s_setprio 2 on the alpha waves, to issue ahead of a co-resident beta wave, measured level: not kept;
// an amdgpu_waves_per_eu hint on this kernel and on sw_beta_kernel, measured: not kept)
template <typename T, int ALGO, int S>
__global__ __launch_bounds__(256) void SW_KERNEL(sw_alpha)(DecodeParams<T> p, WinArgs<T> a SW_STOP_PARAM)
{
    SW_STOP_DECL
    __shared__ alignas(16) char lut_s[sw_lut_bytes<T, ALGO>()];
    if constexpr (ALGO != 1) sw_lut_fill<T, ALGO>(lut_s, p);
    SwTask t;
    if (!sw_task(p, a, t)) return;
    if constexpr (STOP)
        if (!sw_stop_task(*sp, t.live, t.b)) return;
    const int lane = threadIdx.x & 63;
    const char* lut = sw_lut_lane<T, ALGO>(lut_s, lane);
    const int W = a.W, g = a.g, nS = a.nS, L = p.L, dec = t.dec, cwv = t.cwv;
    T* const niw = a.nii_wr + ((size_t)dec * a.Bp + t.b) * nS * 16;
    const T* const nir = a.nii_rd + ((size_t)dec * a.Bp + t.b) * nS * 16;
    const bool use_nii = a.nii && a.it > 0;
    const int base0 = t.s0 * W;

    // the chain of sub-block s0 starts at i0 (clamped to 0)
    T al[8], bl[8];
    const int i0 = base0 - g;
    if (i0 <= 0)
        sw_set(al, 1, (T)0);
    else if (use_nii)
        sw_load_nii(al, nir + (size_t)t.s0 * 16);
    else
        sw_set(al, 0, (T)0);
    sw_set(bl, 0, (T)0);
    const int ps = max(i0, 0);

    // per sub-block bookkeeping (wave-uniform)
    int s = t.s0, st = 0, en = 0, qb = 0, need = 0;
    bool hasB = false;
    auto enter = [&](int ns) {
        s = ns;
        st = s * W;
        en = sw_end(s, nS, W, L);
        hasB = s + 1 < t.s1;                     // the next sub-block's chain runs in this lane
        qb = st + W - g;                         // its start = the NII alpha position of s+1
        const int lc = st + ((en - st - 1) / S) * S;   // last checkpoint
        need = s < nS - 1 ? max(lc, qb) : lc;    // alpha wanted up to here
    };
    enter(t.s0);
    if (s < nS - 1 && qb < 0 && t.live)          // (g > W) the NII position lies before step 0
#pragma unroll
        for (int j = 0; j < 8; ++j) niw[(size_t)(s + 1) * 16 + j] = j == 0 ? (T)0 : (T)-kInfty;
    const int stop = [&] {                        // the run's last position with work
        const int sl = t.s1 - 1, stl = sl * W, enl = sw_end(sl, nS, W, L);
        const int lc = stl + ((enl - stl - 1) / S) * S;
        return sl < nS - 1 ? max(lc, stl + W - g) : lc;
    }();

    int bp = base0 + floor_div(ps - base0, S) * S;
    SwRaw<T> nx[S];
#pragma unroll
    for (int m = 0; m < S; ++m) nx[m] = sw_raw(p, a, dec, cwv, lane, bp + m);
    for (; bp <= stop; bp += S) {
        // the segment's inputs from the prefetch registers, then the next segment's loads into them
        // (converting first keeps one copy of them live: no register moves at the loop edge)
        SwIn<T> x[S];
#pragma unroll
        for (int m = 0; m < S; ++m) x[m] = sw_cvt(nx[m], bp + m < a.la_len);
#pragma unroll
        for (int m = 0; m < S; ++m) nx[m] = sw_raw(p, a, dec, cwv, lane, bp + S + m);
        // Fast segments (all but about one in eight): whole, no chain start or NII position inside, each
        // chain stepping at every position or at none -- one straight block, the two chains' max*
        // interleaved.  The others take the per-position path below.
        const bool qin = (hasB || s < nS - 1) && qb >= bp && qb < bp + S;
        const bool aAll = bp + S <= need, aNone = bp >= need;
        const bool bAll = hasB && bp > qb, bNone = !hasB || bp + S <= qb;
        if (bp >= ps && bp + S - 1 <= stop && !qin && (aAll || aNone) && (bAll || bNone) && !(aNone && bNone)) {
            if (bp >= st) {                               // checkpoint alpha[bp] (normalised)
                T* ck = sw_ck(a, t, s, (bp - st) / S);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if constexpr (!kDiag<kDiagSwNoCk>) sw_ck_store(ck + j * 64, al[j]);
            }
            if (aAll && bAll) {
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    sw_alpha_step2<T, ALGO>(al, bl, x[m], lut);
                    sw_fence();
                }
                sw_normalise(al);
                sw_normalise(bl);
            } else if (aAll) {
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    sw_alpha_step<T, ALGO>(al, x[m], lut);
                    sw_fence();
                }
                sw_normalise(al);
            } else {
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    sw_alpha_step<T, ALGO>(bl, x[m], lut);
                    sw_fence();
                }
                sw_normalise(bl);
            }
        } else {
            // sub-block s+1's chain starts at qb: set once at the segment's start (the positions below qb
            // leave it alone), as a branch, not per-position selects (see the beta kernel)
            if (hasB && qb >= bp && qb < bp + S && qb >= ps && qb <= stop) {
                asm volatile("" ::: "memory");
                if (qb <= 0)
                    sw_set(bl, 1, (T)0);
                else if (use_nii)
                    sw_load_nii(bl, nir + (size_t)(s + 1) * 16);
                else
                    sw_set(bl, 0, (T)0);
            }
#pragma unroll
            for (int m = 0; m < S; ++m) {
                const int pos = bp + m;
                if (pos < ps || pos > stop) continue;
                if (m == 0 && pos >= st && pos < en) {       // checkpoint alpha[pos] (normalised)
                    T* ck = sw_ck(a, t, s, (pos - st) / S);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if constexpr (!kDiag<kDiagSwNoCk>) sw_ck_store(ck + j * 64, al[j]);
                }
                if (s < nS - 1 && pos == qb && t.live)
#pragma unroll
                    for (int j = 0; j < 8; ++j) niw[(size_t)(s + 1) * 16 + j] = al[j];
                const bool doA = pos < need, doB = hasB && pos >= qb;
                if (doA && doB)
                    sw_alpha_step2<T, ALGO>(al, bl, x[m], lut);
                else if (doA)
                    sw_alpha_step<T, ALGO>(al, x[m], lut);
                else if (doB)
                    sw_alpha_step<T, ALGO>(bl, x[m], lut);
                if (m == S - 1) {                            // alpha[bp + S]: an aligned position
                    if (doA) sw_normalise(al);
                    if (doB) sw_normalise(bl);
                }
            }
        }
        if (hasB && bp + S == en) {                      // hand over to sub-block s+1
            if (qb >= en) {                              // g = 0: its chain starts at its first position
                if (t.live)                              // (alpha[en] of this chain is its NII metric)
#pragma unroll
                    for (int j = 0; j < 8; ++j) niw[(size_t)(s + 1) * 16 + j] = al[j];
                if (use_nii)
                    sw_load_nii(bl, nir + (size_t)(s + 1) * 16);
                else
                    sw_set(bl, 0, (T)0);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) al[j] = bl[j];
            enter(s + 1);
        }
    }
}

// ---- alpha for a batch of one codeword (the drop-in's frame): the chain's 8 states across 8 lanes
// (state j in lane j of each group of 8 lanes; the groups mirror each other, lanes 0-7 store), the two
// predecessors fetched by ds_bpermute.  A lone sw_alpha_kernel wave issues a step's 8 max* from one lane
// (about 650 cycles a step); here each lane does one.  Per state the operations and their order are
// sw_alpha_step's; the normalising max (sw_normalise) is exact in any order.
template <typename T, int ALGO, int S>
__global__ __launch_bounds__(256) void SW_KERNEL(sw_alpha_lps)(DecodeParams<T> p, WinArgs<T> a SW_STOP_PARAM)
{
    SW_STOP_DECL
    __shared__ alignas(16) char lut_s[sw_lut_bytes<T, ALGO>()];
    __shared__ T lin_s[4][3][kSwLpsChunk];   // per wave: codeword 0's ys, yp, La of a chunk of positions
    if constexpr (ALGO != 1) sw_lut_fill<T, ALGO>(lut_s, p);
    SwTask t;
    if (!sw_task(p, a, t)) return;
    if constexpr (STOP)   // every lane works for the wave's first codeword: stopped, nothing is left to do
        if (sp->stop_at[t.cwv * 64] != 0) return;
    const int lane = threadIdx.x & 63;
    const char* lut = sw_lut_lane<T, ALGO>(lut_s, lane);
    T (&lin)[3][kSwLpsChunk] = lin_s[threadIdx.x >> 6];
    SwLps l;
    l.j = lane & 7;
    l.p0 = (lane & ~7) + (int)((kSwLast0 >> (4 * l.j)) & 7);
    l.p1 = (lane & ~7) + (int)((kSwLast1 >> (4 * l.j)) & 7);
    l.q0 = (kSwQ >> (l.p0 & 7)) & 1;
    l.q1 = (kSwQ >> (l.p1 & 7)) & 1;
    const int W = a.W, g = a.g, nS = a.nS, L = p.L, dec = t.dec, cwv = t.cwv, b0 = cwv * 64;
    const bool wr = lane < 8 && b0 < p.B;          // lanes 0-7 store codeword 0's states
    T* const niw = a.nii_wr + ((size_t)dec * a.Bp + b0) * nS * 16;
    const T* const nir = a.nii_rd + ((size_t)dec * a.Bp + b0) * nS * 16;
    const bool use_nii = a.nii && a.it > 0;
    const int base0 = t.s0 * W;
    auto set = [&](bool slot0_only, T x0) -> T { return (l.j == 0 || !slot0_only) ? x0 : (T)-kInfty; };
    auto load_nii = [&](const T* src) -> T {
        T v = src[l.j];
        asm volatile("" ::"v"(v));
        return v;
    };

    T al, bl;
    const int i0 = base0 - g;
    if (i0 <= 0)
        al = set(true, (T)0);
    else if (use_nii)
        al = load_nii(nir + (size_t)t.s0 * 16);
    else
        al = set(false, (T)0);
    bl = set(false, (T)0);
    const int ps = max(i0, 0);

    int s = t.s0, st = 0, en = 0, qb = 0, need = 0;
    bool hasB = false;
    auto enter = [&](int ns) {
        s = ns;
        st = s * W;
        en = sw_end(s, nS, W, L);
        hasB = s + 1 < t.s1;
        qb = st + W - g;
        const int lc = st + ((en - st - 1) / S) * S;
        need = s < nS - 1 ? max(lc, qb) : lc;
    };
    enter(t.s0);
    if (s < nS - 1 && qb < 0 && wr) niw[(size_t)(s + 1) * 16 + lane] = lane == 0 ? (T)0 : (T)-kInfty;
    const int stop = [&] {
        const int sl = t.s1 - 1, stl = sl * W, enl = sw_end(sl, nS, W, L);
        const int lc = stl + ((enl - stl - 1) / S) * S;
        return sl < nS - 1 ? max(lc, stl + W - g) : lc;
    }();
    auto ck_store = [&](int c) {                     // checkpoint alpha (normalised), column of codeword 0
        if (wr) (sw_ck(a, t, s, c) - lane)[lane * 64] = al;
    };
    // a.hand (one sub-block a lane): lanes 8-15 run this sub-block's beta warm-up chain, positions
    // en + g - 1 down to en, beside alpha -- the same exchange-and-max* step with the beta trellis
    // (sw_beta_step: b[next0] - G, b[next1] + G, G = gamma of the state), normalised where the beta
    // kernel normalises it -- and leave beta[en] in column 1 of the sub-block's first checkpoint slot
    // (unused with one codeword), where sw_beta_kernel<LF> starts from it.
    const bool hand = a.hand && s < nS - 1;
    const bool wl = hand && (lane >> 3) == 1;
    const int nw = hand ? g : 0;
    int kw = 0;
    if (wl) {
        l.p0 = 8 + (int)((kSwNext0 >> (4 * l.j)) & 7);
        l.p1 = 8 + (int)((kSwNext1 >> (4 * l.j)) & 7);
        l.q0 = l.q1 = (kSwQ >> l.j) & 1;
    }
    if (hand) {
        const T w0 = use_nii ? nir[(size_t)s * 16 + 8 + l.j] : (T)0;   // the chain of s starts at en + g
        if (wl) al = w0;
    }

    int bp = base0 + floor_div(ps - base0, S) * S;
    // The inputs come a chunk of kSwLpsChunk positions at a time into LDS, every lane loading its share
    // at once: one memory latency a chunk.  (A lone wave's steps are short enough here that loads issued
    // one segment ahead were waited for at every segment.)
    int c0 = bp, c1 = bp;                            // the chunk [c0, c1) in lin
    auto load_chunk = [&](int from) {
        c0 = from;
        c1 = from + kSwLpsChunk;
        for (int k = lane; k < kSwLpsChunk; k += 64) {
            const SwRaw<T> r = sw_raw(p, a, dec, cwv, 0, c0 + k);
            lin[0][k] = r.ys;
            lin[1][k] = r.yp;
            lin[2][k] = r.la;
        }
        __builtin_amdgcn_wave_barrier();
    };
    static_assert(kSwLpsChunk % S == 0, "whole segments a chunk");
    for (; bp <= stop; bp += S) {
        if (bp >= c1) load_chunk(bp);
        SwIn<T> x[S];
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const SwRaw<T> r{lin[0][bp - c0 + m], lin[1][bp - c0 + m], lin[2][bp - c0 + m]};
            x[m] = sw_cvt(r, bp + m < a.la_len);
        }
        if (hasB && qb >= bp && qb < bp + S && qb >= ps && qb <= stop) {
            asm volatile("" ::: "memory");
            if (qb <= 0)
                bl = set(true, (T)0);
            else if (use_nii)
                bl = load_nii(nir + (size_t)(s + 1) * 16);
            else
                bl = set(false, (T)0);
        }
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const int pos = bp + m;
            if (pos < ps || pos > stop) continue;
            if (m == 0 && pos >= st && pos < en) ck_store((pos - st) / S);
            if (s < nS - 1 && pos == qb && wr) niw[(size_t)(s + 1) * 16 + lane] = al;
            const bool doA = pos < need, doB = hasB && pos >= qb;
            const bool wact = kw < nw;
            const int pw = en + g - 1 - kw;                  // the warm-up chain's position
            T na = al, nbv = bl;
            if (doA || wact) {
                SwIn<T> xs = x[m];
                if (wact) {
                    const int iw = min(max(pw - c0, 0), kSwLpsChunk - 1);
                    const SwRaw<T> r{lin[0][iw], lin[1][iw], lin[2][iw]};
                    const SwIn<T> xw = sw_cvt(r, pw < a.la_len);
                    if (wl) xs = xw;
                }
                const T n = sw_lps_step<T, ALGO>(al, xs, l, lut);
                if (wl ? wact : doA) na = n;
            }
            if (doB) nbv = sw_lps_step<T, ALGO>(bl, x[m], l, lut);
            al = na;
            bl = nbv;
            const bool nA = m == S - 1 && doA, nW = wact && (pw - base0) % S == 0;
            if (nA || nW) {
                const T nv = sw_lps_norm(al, lane);
                if (wl ? nW : nA) al = nv;
            }
            if (m == S - 1 && doB) bl = sw_lps_norm(bl, lane);
            if (wact) ++kw;
        }
        if (hasB && bp + S == en) {
            if (qb >= en) {
                if (wr) niw[(size_t)(s + 1) * 16 + lane] = al;
                if (use_nii)
                    bl = load_nii(nir + (size_t)(s + 1) * 16);
                else
                    bl = set(false, (T)0);
            }
            al = bl;
            enter(s + 1);
        }
    }
    if (wl && b0 < p.B) (sw_ck(a, t, s, 0) - lane)[l.j * 64 + 1] = al;   // beta[en] for sw_beta_kernel<LF>
}

// ---- beta + LLR: backward over the run in segments of S positions
// LF (lane folds; a batch of one codeword, the drop-in's frame): every lane of the wave runs codeword
// 0's chains, and the S LLRs of a segment are folded side by side, position m in lane m, once the
// segment's beta steps are done -- one fold latency a segment instead of S (the folds are the beta
// kernel's longest dependent chains: 2 x 7 table max* a position).  Same operations, same order.
// STOP (td_set_window_stop): SISO2's lanes also gather the rule's evidence on the decisions they store.
// The old bytes (HDA; four codewords' to a lane, its own among them) or the syndromes (CRC) of a
// segment's S decisions are fetched by DMA into LDS slots when the segment's write positions are known
// and read in the next segment's flush, behind the wait that covers that segment's prefetch anyway: no
// further memory round trip a segment.  LF keeps lane m's in a register instead.
template <typename T, int ALGO, int S, bool LF>
__global__ __launch_bounds__(256) void SW_KERNEL(sw_beta)(DecodeParams<T> p, WinArgs<T> a, const int* __restrict__ pi,
                                                          const int* __restrict__ pinv SW_STOP_PARAM)
{
    SW_STOP_DECL
    __shared__ alignas(16) char lut_s[sw_lut_bytes<T, ALGO>()];
    __shared__ alignas(16) T ck_lds[4 * 8 * 64];   // per wave: the next segment's checkpoint (DMA slot)
    __shared__ alignas(16) T in_lds[4 * 3 * S * 64];   // per wave: the next segment's ys, yp, La rows (DMA slot)
    __shared__ alignas(16) int ix_lds[4 * 64];         // per wave: the next segment's interleaver entries (DMA slot)
    if constexpr (ALGO != 1) sw_lut_fill<T, ALGO>(lut_s, p);
    SwTask t;
    if (!sw_task(p, a, t)) return;
    if constexpr (STOP) {
        if constexpr (LF) {
            if (sp->stop_at[t.cwv * 64] != 0) return;
        } else {
            if (!sw_stop_task(*sp, t.live, t.b)) return;
        }
    }
    const int lane = threadIdx.x & 63;
    const char* lut = sw_lut_lane<T, ALGO>(lut_s, lane);
    const int W = a.W, g = a.g, nS = a.nS, L = p.L, K = p.K, dec = t.dec, cwv = t.cwv;
    const int col = LF ? 0 : lane;                // this lane's codeword within the wave
    const int b = LF ? t.cwv * 64 : t.b;
    T* const niw = a.nii_wr + ((size_t)dec * a.Bp + b) * nS * 16;
    const T* const nir = a.nii_rd + ((size_t)dec * a.Bp + b) * nS * 16;
    const bool use_nii = a.nii && a.it > 0;
    const int base0 = t.s0 * W;
    const int* const perm = dec ? pi : pinv;
    T* const le = a.le[dec] + (size_t)cwv * K * kSwCw;
    uint8_t* const bitsT = dec ? a.bitsT : nullptr;
    uint8_t* const bits1 = LF && dec ? a.bits1 : nullptr;
    const int bcol = LF ? t.cwv * 64 : t.cwv * 64 + lane;
    // clock sample (as turbo_decode_kernel's): workgroup 0's shader clock and 100 MHz counter at its
    // start and end, two scalar reads each, written by its first lane with one vector store
    const bool clk = a.clk && p.clk && blockIdx.x == 0;
    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (clk) {
        clk_c0 = __builtin_amdgcn_s_memtime();
        clk_r0 = __builtin_amdgcn_s_memrealtime();
    }

    int s = t.s1 - 1, st = 0, en = 0, qb = 0;
    bool hasB = false;
    auto enter = [&](int ns) {
        s = ns;
        st = s * W;
        en = sw_end(s, nS, W, L);
        hasB = s > t.s0;                          // the previous sub-block's chain runs in this lane
        qb = min(st + g, L);                      // its start (= the NII beta position of s-1)
    };
    enter(t.s1 - 1);
    // the chain of sub-block s1-1 starts at e = end + g (clamped to L)
    T be[8], bb[8];
    const int e = en + g;
    if (e >= L)
        sw_set(be, 1, (T)0);
    else if (use_nii)
        sw_load_nii(be, nir + (size_t)s * 16 + 8);
    else
        sw_set(be, 0, (T)0);
    sw_set(bb, 0, (T)0);
    if (s > 0 && st + g >= L && t.live)           // NII position at or past L: the terminated state
#pragma unroll
        for (int j = 0; j < 8; ++j) niw[(size_t)(s - 1) * 16 + 8 + j] = j == 0 ? (T)0 : (T)-kInfty;
    const int pe = min(e, L) - 1;                 // first position stepped

    // Segment prefetch, one segment ahead, all of it by DMA into this wave's LDS slots
    // (global_load_lds_dwordx4, 1 KB a wave instruction): the segment's three input rows (ys, yp, La:
    // S consecutive 64-codeword rows each, contiguous in the wide layout) and, for a segment of a
    // sub-block's own range, its checkpoint (8 x 64 lane-contiguous values).  Nothing in flight sits in
    // a VGPR: with the inputs loaded into registers the allocator copied a pending load into the
    // loop-carried register right after issuing it, so the wave waited for the prefetch it had just
    // issued (vmcnt) in every segment.  Rows past the array ends stay inside the workspace (td_api.cpp:
    // kWideSlack); their values are never used (positions >= L are not stepped, La >= K is masked).
    // Ordering: the extrinsic / decision stores of a segment are issued at the start of the next one,
    // before its DMA, so one `s_waitcnt vmcnt(0)` at each segment start covers exactly this segment's
    // DMA and the stores before it, all issued a segment earlier.
    auto seg_sub = [&](int sbp) {                 // sub-block whose chain covers segment sbp
        return sbp >= en ? s : min(t.s0 + (sbp - base0) / W, t.s1 - 1);
    };
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T* const ckslot = ck_lds + wave * 8 * 64;
    T* const inslot = in_lds + wave * 3 * S * 64;
    const unsigned ckslot_lds = __builtin_amdgcn_readfirstlane(lds_addr(ckslot));   // DMA bases (M0): wave-uniform
    const unsigned inslot_lds = __builtin_amdgcn_readfirstlane(lds_addr(inslot));
    constexpr int kRowBytes = kSwCw * (int)sizeof(T);
    constexpr int kInDma = S * kRowBytes / 1024;                    // DMA instructions per input array
    static_assert(S * kRowBytes % 1024 == 0, "whole 1 KB DMA chunks");
    int bp = base0 + floor_div(pe - base0, S) * S;
    if constexpr (LF) {
        // a.hand: sw_alpha_lps_kernel ran this chain's warm-up and left beta[en] in column 1 of the
        // sub-block's first checkpoint slot; start at the sub-block's last segment from it
        if (a.hand && s < nS - 1) {
            const T* hb = sw_ck(a, t, s, 0) - lane + 1;
#pragma unroll
            for (int j = 0; j < 8; ++j) be[j] = hb[j * 64];
            bp = en - S;
        }
    }
    // the segment's interleaver entries (wave-uniform: scalar loads), one segment ahead
    int* const ixslot = ix_lds + wave * 64;                           // the next segment's perm / pi entries
    const unsigned ixslot_lds = __builtin_amdgcn_readfirstlane(lds_addr(ixslot));
    // STOP: this lane's evidence, and where it comes from
    unsigned ev_acc = 0, lf_old = 0;
    const unsigned* oldslot = nullptr;
    unsigned oldslot_lds = 0;
    if constexpr (STOP && !LF) {
        oldslot = sw_stop_slots<S>() + wave * S * 64;
        oldslot_lds = __builtin_amdgcn_readfirstlane(lds_addr(oldslot));
    }
    auto prefetch = [&](int nbp) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the slots' previous reads are done
        // The interleaver entries by DMA too (lane l < S: perm, S <= l < 2S: pi, of position nbp + l % S),
        // waited for with the rest at the next segment's start.  As scalar loads they were waited out at
        // the lgkmcnt(0) above or at the first table read after it (scalar loads complete out of order,
        // so while one is in flight every LDS wait of the wave is an lgkmcnt(0)).
        dma4(ixslot_lds, (lane & S ? pi : perm) + min(nbp + (lane & (S - 1)), K - 1));
        const int ns = seg_sub(nbp), nst = ns * W;
        if (nbp >= base0 && nbp < sw_end(ns, nS, W, L)) {
            const char* src = reinterpret_cast<const char*>(sw_ck(a, t, ns, (nbp - nst) / S) - lane) + lane * 16;
            constexpr int kDma = 8 * 64 * (int)sizeof(T) / 1024;
#pragma unroll
            for (int q = 0; q < kDma; ++q)
                if constexpr (!kDiag<kDiagSwNoCk>) sw_ck_dma(ckslot_lds + q * 1024, src + q * 1024);
        }
        const size_t row = (size_t)cwv * L + nbp, rowk = (size_t)cwv * K + nbp;
        const char* src0 = reinterpret_cast<const char*>((dec ? p.sys2 : p.sys1) + row * kSwCw) + lane * 16;
        const char* src1 = reinterpret_cast<const char*>((dec ? p.par2 : p.par1) + row * kSwCw) + lane * 16;
        const char* src2 = reinterpret_cast<const char*>(a.la[dec] + rowk * kSwCw) + lane * 16;
#pragma unroll
        for (int q = 0; q < kInDma; ++q) {
            dma16(inslot_lds + q * 1024, src0 + q * 1024);
            dma16(inslot_lds + S * kRowBytes + q * 1024, src1 + q * 1024);
            dma16(inslot_lds + 2 * S * kRowBytes + q * 1024, src2 + q * 1024);
        }
    };
    prefetch(bp);
    // the previous segment's extrinsics and decisions, stored at the start of the next one
    T dlev[S];
    int dbit[S], dpm[S], dpk[S];
    bool dst[S];
#pragma unroll
    for (int m = 0; m < S; ++m) dst[m] = false;
    // LF: lane m < S keeps position m's extrinsic, decision and write positions
    T lf_lev = 0;
    int lf_bit = 0, lf_pm = 0, lf_pk = 0, cur_pm = 0, cur_pk = 0;
    bool lf_st = false;
    auto flush = [&] {
        if constexpr (LF) {
            if (lf_st) {
                le[(size_t)lf_pm * kSwCw] = lf_lev;
                if (bitsT) bitsT[(size_t)lf_pk * a.Bp + bcol] = (uint8_t)lf_bit;
                if (bits1) bits1[lf_pk] = (uint8_t)lf_bit;
                if constexpr (STOP)
                    if (bits1) {
                        if (sp->rule == 2)
                            ev_acc ^= lf_bit ? lf_old : 0u;
                        else
                            ev_acc |= (unsigned)(lf_old != (unsigned)lf_bit);
                    }
            }
        } else {
#pragma unroll
            for (int m = 0; m < S; ++m)
                if (dst[m] && t.live) {
                    if constexpr (kSwExtNt)
                        __builtin_nontemporal_store(dlev[m], &le[(size_t)dpm[m] * kSwCw + lane]);
                    else
                        le[(size_t)dpm[m] * kSwCw + lane] = dlev[m];
                    if (bitsT) bitsT[(size_t)dpk[m] * a.Bp + bcol] = (uint8_t)dbit[m];
                    if constexpr (STOP)
                        if (bitsT) {
                            const unsigned o = oldslot[m * 64 + lane];
                            if (sp->rule == 2)
                                ev_acc ^= dbit[m] ? o : 0u;
                            else
                                ev_acc |= (unsigned)(((o >> (8 * (lane & 3))) & 0xffu) != (unsigned)dbit[m]);
                        }
                }
        }
    };
    int pm[S], pk[S];
    // one position's LLR, extrinsic and decision (beta = beta[pos + 1]), kept for the flush
    auto llr_out = [&](int pos, const T (&al)[8], const SwIn<T>& xm, int m) {
        const T llr = sw_llr<T, ALGO>(al, be, xm, lut);
        const T lev = (llr - xm.la - (T)2 * xm.ys) * a.ext_scale;
        dlev[m] = lev;
        dbit[m] = llr < (T)0 ? 0 : 1;
        dst[m] = pos < K;
        if (p.le_dump && t.live) p.le_dump[(size_t)b * p.iters * 2 * L + (size_t)(2 * a.it + dec) * L + pos] = lev;
    };
    for (; bp >= base0; bp -= S) {
        SwIn<T> x[S];
        T as[S][8];
        const bool main = bp < en;                        // the segment lies in sub-block s's own range
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this segment's DMA (and the stores before it)
        flush();
        if constexpr (LF) {
            lf_st = false;
            cur_pm = ixslot[lane & (S - 1)];          // lane m: position m's write positions
            cur_pk = ixslot[S + (lane & (S - 1))];
            if constexpr (STOP)
                if (bits1) lf_old = sp->rule == 2 ? sp->crc_tab[cur_pk] : (unsigned)sp->old1[cur_pk];
        }
#pragma unroll
        for (int m = 0; m < S; ++m) {
            SwRaw<T> r;
            r.ys = inslot[m * 64 + col];
            r.yp = inslot[(S + m) * 64 + col];
            r.la = inslot[(2 * S + m) * 64 + col];
            x[m] = sw_cvt(r, bp + m < a.la_len);
            pm[m] = __builtin_amdgcn_readfirstlane(ixslot[m]);
            pk[m] = __builtin_amdgcn_readfirstlane(ixslot[S + m]);
            dst[m] = false;
            dpm[m] = pm[m];
            dpk[m] = pk[m];
        }
        if (main)
#pragma unroll
            for (int j = 0; j < 8; ++j) as[0][j] = ckslot[j * 64 + col];
        if (bp - S >= base0) prefetch(bp - S);
        if constexpr (STOP && !LF) {
            if (bitsT) {   // the evidence inputs of this segment's decisions, for the next segment's flush
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the flush above has read the slots
#pragma unroll
                for (int m = 0; m < S; ++m) {
                    const void* src = sp->rule == 2
                                          ? static_cast<const void*>(sp->crc_tab + pk[m])
                                          : static_cast<const void*>(bitsT + (size_t)pk[m] * a.Bp + cwv * 64 + (lane & ~3));
                    dma4(oldslot_lds + m * 256, src);
                }
            }
        }
        if (main) {                                       // alpha of the segment from its checkpoint
#pragma unroll
            for (int m = 1; m < S; ++m) {                 // (past en in the last segment: computed, unused)
#pragma unroll
                for (int j = 0; j < 8; ++j) as[m][j] = as[m - 1][j];
                sw_alpha_step<T, ALGO>(as[m], x[m - 1], lut);
                sw_fence();
            }
        }
        const int nb = st + g;                            // NII beta position of s-1
        // Sub-block s-1's chain starts at qb (its first step at qb - 1).  Its metrics are set once at
        // the segment's start: the positions above qb - 1 leave them alone, so this equals setting
        // them at qb - 1.  A branch, not a select (the empty asm keeps the compiler from if-converting
        // it into 16 v_cndmask + 16 v_mov at every position: 8 % of the kernel's VALU).
        if (hasB && qb - 1 >= bp && qb - 1 < bp + S && qb - 1 <= pe) {
            asm volatile("" ::: "memory");
            if (qb >= L)
                sw_set(bb, 1, (T)0);
            else if (use_nii)
                sw_load_nii(bb, nir + (size_t)(s - 1) * 16 + 8);
            else
                sw_set(bb, 0, (T)0);
        }
        T asel[LF ? 8 : 1], bsel[LF ? 8 : 1];           // LF: lane m's position's alpha, beta[pos + 1], inputs
        SwIn<T> xsel{};
        bool sel = false;
#pragma unroll
        for (int m = S - 1; m >= 0; --m) {
            const int pos = bp + m;
            if (pos > pe) continue;
            if constexpr (LF) {
                if (main && pos < en && lane == m) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        asel[j] = as[m][j];
                        bsel[j] = be[j];
                    }
                    xsel = x[m];
                    sel = true;
                }
            } else if (main && pos < en) {
                llr_out(pos, as[m], x[m], m);
            }
            const bool doB = hasB && pos < qb;
            if (doB)
                sw_beta_step2<T, ALGO>(be, bb, x[m], lut);
            else
                sw_beta_step<T, ALGO>(be, x[m], lut);
            if (m == 0) {                                 // beta[bp]: an aligned position
                sw_normalise(be);
                if (doB) sw_normalise(bb);
            }
            if (s > 0 && pos == nb && t.live)
#pragma unroll
                for (int j = 0; j < 8; ++j) niw[(size_t)(s - 1) * 16 + 8 + j] = be[j];
        }
        if constexpr (LF) {                               // the segment's S folds, one per lane
            if (!sel)
#pragma unroll
                for (int j = 0; j < 8; ++j) asel[j] = bsel[j] = (T)0;   // (computed and dropped)
            const T llr = sw_llr<T, ALGO>(asel, bsel, xsel, lut);
            const T lev = (llr - xsel.la - (T)2 * xsel.ys) * a.ext_scale;
            const int pos = bp + lane;
            lf_lev = lev;
            lf_bit = llr < (T)0 ? 0 : 1;
            lf_pm = cur_pm;
            lf_pk = cur_pk;
            lf_st = sel && pos < K && b < p.B;
            if (p.le_dump && sel && b < p.B)
                p.le_dump[(size_t)b * p.iters * 2 * L + (size_t)(2 * a.it + dec) * L + pos] = lev;
        }
        if (hasB && bp == st) {                           // hand over to sub-block s-1
            if (qb <= st) {                               // g = 0: its chain starts at its end
                if (use_nii)
                    sw_load_nii(bb, nir + (size_t)(s - 1) * 16 + 8);
                else
                    sw_set(bb, 0, (T)0);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) be[j] = bb[j];
            enter(s - 1);
            if (s > 0 && st + g == en && t.live)          // g = W: the NII position is this chain's start
#pragma unroll
                for (int j = 0; j < 8; ++j) niw[(size_t)(s - 1) * 16 + 8 + j] = be[j];
        }
    }
    if constexpr (STOP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last segment's evidence inputs
    flush();
    if constexpr (STOP) {   // one merge per lane and launch
        if (ev_acc) {
            if (sp->rule == 2)
                atomicXor(sp->ev + b, ev_acc);
            else
                atomicOr(sp->ev + b, ev_acc);
        }
    }
    if (clk) {
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) *reinterpret_cast<ulonglong4*>(p.clk) = make_ulonglong4(clk_c0, clk_r0, c1, r1);
    }
}

#undef SW_KERNEL
#undef SW_STOP_PARAM
#undef SW_STOP_DECL
