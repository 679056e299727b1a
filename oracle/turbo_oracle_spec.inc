/*
 * turbo_oracle_spec.inc -- CPU restatement of the exact log-MAP kernel's speculation detector.
 * TEST INFRASTRUCTURE (see turbo_oracle.h).  Included twice by turbo_oracle.c after
 * turbo_oracle_siso.inc, with the same REAL / SFX / MAXSTAR.
 *
 * The kernel's alpha pass (td_kernels.hip AlphaSchedS, kASpec) reads a step's max* row from the
 * bucket of the UNnormalised difference
 *     dr = fl(fl(g_p + a_raw[p1]) - fl(g_s + a_raw[p0]))
 * and compares that bucket with the bucket of the exact difference, the same expression on the
 * normalised metrics alpha = a_raw - tempmax.  A step whose two buckets differ is a miss; a window
 * with a miss in any lane of the wave is computed again in the committed order.  The kernel
 * speculates on the full interior windows only: windows 1 .. nT-2 of 15 steps, nT = ceil(L/15).
 * This file counts the misses of one SISO pass on the oracle's own arithmetic (tdo_siso's gamma and
 * alpha recursion), so it says which inputs reach the detector; it is a count on the CPU, not a
 * statement about any GPU run.
 */

#define CAT_(a, b) a##_##b
#define CAT(a, b) CAT_(a, b)

/* td_tables.h BucketBits + bucket_of_bits: exponent + top 2 mantissa bits of |d|, clamped to [0, 28] */
static int CAT(spec_bucket, SFX)(REAL d)
{
    int q;
    if (sizeof(REAL) == 8) {
        double dd = (double)d;
        uint64_t b;
        memcpy(&b, &dd, sizeof b);
        q = (int)((b >> (32 + 18)) & ((1u << 13) - 1)) - ((1023 - 4) << 2);
    } else {
        float df = (float)d;
        uint32_t b;
        memcpy(&b, &df, sizeof b);
        q = (int)((b >> 21) & ((1u << 10) - 1)) - ((127 - 4) << 2);
    }
    return q < 0 ? 0 : (q > 28 ? 28 : q);
}

/*
 * The max* correction a step takes when it reads table row r but compares d itself with the row's
 * threshold (td_kernels.hip sched_finish on td_tables.h build_lut's rows: vlo below the row's
 * threshold, the next row's vlo from it on).  With r = the bucket of d it is E_algorithm's correction.
 */
static REAL CAT(spec_row_value, SFX)(int r, REAL d)
{
    int base = 0, in_row = -1;
    for (int k = 1; k < 16; k++) {
        const int qk = CAT(spec_bucket, SFX)((REAL)k_idx[k]);
        if (qk < r) base++;
        if (qk == r) in_row = k;
    }
    const REAL ad = d < 0 ? -d : d;
    const int i = base + (in_row >= 0 && ad >= (REAL)k_idx[in_row]);
    return i >= 15 ? (REAL)0 : (REAL)k_tab[i];
}

/*
 * Misses of the alpha pass of one log-MAP SISO (tdo_siso's recs / La / L).  Returns the number of
 * (step, state) pairs in windows 1 .. nT-2 whose speculated and exact buckets differ;
 * win_miss (nullable) [nT] receives the count of each window (0 for windows 0 and nT-1).
 * *harm (nullable) receives the number of those misses that matter: the step's correction read from
 * the speculated row differs from the exact row's, so a kernel that did not recompute the window
 * would compute another alpha.  (A miss whose d lies just beside the bucket edge reads the same
 * value from either row: the neighbour's vlo is this row's vhi.)
 */
int CAT(tdo_spec_miss_siso, SFX)(const tdo_trellis* t, const REAL* recs, const REAL* La, int L, int* win_miss,
                                 int* harm)
{
    const int S = TDO_NSTATES, W = TDO_SPEC_WINDOW;
    const int nT = (L + W - 1) / W;
    REAL raw[TDO_NSTATES], alpha[TDO_NSTATES], nraw[TDO_NSTATES];
    int total = 0, harmful = 0;
    if (win_miss)
        for (int w = 0; w < nT; w++) win_miss[w] = 0;
    /* alpha[.][0] (:943-948); its tempmax is 0, so raw == normalised */
    for (int s = 0; s < S; s++) raw[s] = alpha[s] = s ? (REAL)-TDO_INFTY : (REAL)0;
    for (int k = 0; k < L; k++) {   /* step k: position k -> k+1 (tdo_siso's i = k+1) */
        const int w = k / W;
        const int spec = w >= 1 && w <= nT - 2;
        for (int j = 0; j < S; j++) {
            const int p0 = t->laststat[j][0], p1 = t->laststat[j][1];
            const REAL g0 = -recs[2 * k] + recs[2 * k + 1] * (REAL)t->nextout[p0][1] - La[k] / 2;
            const REAL g1 = recs[2 * k] + recs[2 * k + 1] * (REAL)t->nextout[p1][3] + La[k] / 2;
            const REAL tx = g0 + alpha[p0], ty = g1 + alpha[p1];
            if (spec) {
                const REAL rx = g0 + raw[p0], ry = g1 + raw[p1];
                const REAL dr = ry - rx, d = ty - tx;
                const int qr = CAT(spec_bucket, SFX)(dr), q = CAT(spec_bucket, SFX)(d);
                if (qr != q) {
                    total++;
                    if (win_miss) win_miss[w]++;
                    if (CAT(spec_row_value, SFX)(qr, d) != CAT(spec_row_value, SFX)(q, d)) harmful++;
                }
            }
            nraw[j] = MAXSTAR(tx, ty);
        }
        REAL m = nraw[0];
        for (int j = 1; j < S; j++)
            if (m < nraw[j]) m = nraw[j];
        for (int j = 0; j < S; j++) {
            raw[j] = nraw[j];
            alpha[j] = nraw[j] - m;
        }
    }
    if (harm) *harm = harmful;
    return total;
}

/*
 * The turbo loop of tdo_turbo_decode (log-MAP) with the detector's count taken in front of each
 * SISO.  win_miss (nullable) [iters][2][nT], *harm (nullable) as tdo_spec_miss_siso's, summed; returns
 * the total over iterations and both SISOs.
 */
int CAT(tdo_spec_miss_turbo, SFX)(const tdo_trellis* t, const int* pi, const REAL* flow, int K, int iters,
                                  int* win_miss, int* harm)
{
    const int L = K + TDO_MREG;
    const int n = 3 * K + 4 * TDO_MREG;
    const int nT = (L + TDO_SPEC_WINDOW - 1) / TDO_SPEC_WINDOW;
    REAL* rec = (REAL*)malloc(sizeof(REAL) * n);
    REAL* yk = (REAL*)malloc(sizeof(REAL) * 4 * L);
    REAL* La = (REAL*)malloc(sizeof(REAL) * L);
    REAL* Le = (REAL*)malloc(sizeof(REAL) * L);
    REAL* LLR = (REAL*)malloc(sizeof(REAL) * L);
    int total = 0, harmful = 0, h = 0;
    if (!rec || !yk || !La || !Le || !LLR) abort();

    for (int i = 0; i < n; i++) rec[i] = flow[i] * (REAL)0.5;
    CAT(demux, SFX)(rec, K, pi, yk);
    for (int i = 0; i < L; i++) La[i] = Le[i] = LLR[i] = 0;

    for (int it = 0; it < iters; it++) {
        for (int i = 0; i < K; i++) La[pi[i]] = Le[i];
        for (int i = K; i < L; i++) La[i] = 0;
        total += CAT(tdo_spec_miss_siso, SFX)(t, yk, La, L, win_miss ? win_miss + ((size_t)it * 2 + 0) * nT : NULL,
                                              &h);
        harmful += h;
        CAT(tdo_siso, SFX)(t, yk, La, 1, LLR, L, TDO_ALGO_LOGMAP);
        for (int i = 0; i < L; i++) Le[i] = LLR[i] - La[i] - 2 * yk[2 * i];

        for (int i = 0; i < K; i++) La[i] = Le[pi[i]];
        for (int i = K; i < L; i++) La[i] = 0;
        total += CAT(tdo_spec_miss_siso, SFX)(t, yk + 2 * L, La, L,
                                              win_miss ? win_miss + ((size_t)it * 2 + 1) * nT : NULL, &h);
        harmful += h;
        CAT(tdo_siso, SFX)(t, yk + 2 * L, La, 1, LLR, L, TDO_ALGO_LOGMAP);
        for (int i = 0; i < L; i++) Le[i] = LLR[i] - La[i] - 2 * yk[2 * L + 2 * i];
    }
    free(rec);
    free(yk);
    free(La);
    free(Le);
    free(LLR);
    if (harm) *harm = harmful;
    return total;
}

#undef CAT
#undef CAT_
