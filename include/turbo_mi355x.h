/*
 * turbo_mi355x.h -- C ABI of the MI355X-native LTE turbo decoder (libturbo_mi355x.so).
 *
 * Plain pointers and sizes only (no HIP / torch types).  Every entry point names the
 * reference interface it replaces (/root/reference/ITTC/...).  The reference's own C++
 * entry points (TurboCodingInit / TurboEnCoding / TurboDecoding / TurboCodingRelease /
 * AWGN / Log_MAP_decoder) are provided on top of this ABI by libturbo_logmap_compat.so
 * (turbo_decoder_cuda_amd/csrc/log_map_compat.cpp), see INTEGRATION.md.
 *
 * Status codes: 0 = TD_OK; non-zero = error, message via td_last_error() (thread-local).
 * The reference has no return codes: it printf()s and exit(1)s (log_map.cpp:288-292,357-368).
 */
#ifndef TURBO_MI355X_H
#define TURBO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_ABI_VERSION 1

enum td_status {
    TD_OK = 0,
    TD_EINVAL = 1,   /* bad argument (K, f1/f2, iterations, batch, null pointer) */
    TD_ENOMEM = 2,   /* host or device allocation failed */
    TD_EHIP = 3,     /* HIP runtime error (message carries hipGetErrorString) */
    TD_ENODEV = 4    /* no MI355X (gfx950) device visible */
};

/* Jacobian used by the SISO: TYPE_DECODER of ITTC/log_map.h:26-29. */
enum td_algo {
    TD_ALGO_LOGMAP = 0,  /* 16-step table max* (E_algorithm, log_map.cpp:779-801) -- the reference */
    TD_ALGO_MAXLOG = 1   /* max* = max (Max-Log-MAP, BASELINE config 3) */
};

/* Arithmetic of the decode. */
enum td_precision {
    TD_F64 = 0,   /* IEEE fp64 with the reference's operation order: the parity mode */
    TD_F32 = 1,   /* fp32, same schedule and op order (throughput mode) */
    TD_FIXED = 2  /* fixed point: int8 channel LLRs, integer Max-Log-MAP, int16 extrinsics (below) */
};

/* Code and schedule parameters.  Reference: globals source_length/f1/f2 (ITTC/main.h:6-11,
 * main.cpp:29-37), macros N_ITERATION / TERMINATED / TYPE_DECODER (ITTC/log_map.h:24-30). */
typedef struct td_params {
    int K;            /* information bits per codeword, 1 <= K <= 10000 (MAX_FRAME_LENGTH); TD_FIXED: K >= 8 */
    int f1, f2;       /* QPP interleaver: pi(i) = (f1*i + f2*i*i) mod K (log_map.cpp:616-624) */
    int iterations;   /* turbo iterations (N_ITERATION) */
    int algo;         /* enum td_algo */
    int precision;    /* enum td_precision */
    int device;       /* HIP device ordinal this handle is bound to */
} td_params;

typedef struct td_handle td_handle;

/* Replaces TurboCodingInit (log_map.cpp:349-434): builds the trellis (gen_g_matrix 13/15 +
 * gen_trellis), the QPP table and the max* bucket table, on `p->device`. */
int td_create(td_handle** out, const td_params* p);
/* Replaces TurboCodingRelease (log_map.cpp:1330-1345). */
int td_destroy(td_handle* h);
/* Size the device workspace for batches up to B codewords (and, with a windowed schedule set by
 * td_set_window, the windowed schedule's buffers).  td_decode_device grows them on demand, which
 * synchronises the device; call td_reserve (after td_set_window) before a decode is captured
 * into a hipGraph. */
int td_reserve(td_handle* h, int B);
/* td_reserve of the exact schedule for B >= 1024 also picks the workspace's placement: the turbo
 * kernel's speed depends on the physical pages behind it (two modes 6-7 % apart on MI355X; the
 * slow one shows 5-8x the DRAM credit stalls), so it times one iteration on candidate workspaces
 * and keeps the fastest.  Up to TD_PLACEMENT_TRIALS candidates (environment variable, default 24;
 * 1 = a plain allocation); after at least TD_PLACEMENT_MIN candidates (default 8) the search
 * stops once one candidate runs >= 4 % below the median of those timed, never on a slow
 * straggler.  Transient memory (round 6): at most three candidates are held at a time -- the
 * slowest is released before the next one is allocated, after a 48 MiB spacer so that the next
 * does not get the same pages back -- so the search holds at most 3 workspaces + 48 MiB per probe
 * beyond the third (config 2: ~2.6 GB a workspace, <= 8.9 GB held; never more than half the free
 * device memory).  A workspace that is already big enough for B is kept as it is (placed or not):
 * call td_reserve before the first decode to have it placed.  Results do not depend on it.
 * Occupancy: a decode of more than 512 groups of 8 codewords (B > 4096 on 256 CUs) in fp32 runs
 * three or four workgroups per CU instead of two where that finishes sooner (fp32 log-MAP 1.5x,
 * Max-Log-MAP 1.6x at B = 32768); fp64 always runs two.  Bits and Le are identical either way.
 * TD_OCC3=0 (environment, read at td_create) keeps every decode on two. */

/*
 * Batched TurboDecoding (log_map.cpp:1146-1280) on device-resident data.
 *   d_llr   [B][3K+12] channel LLRs in the reference stream layout (main.cpp:202 output),
 *           double for TD_F64, float for TD_F32.  Not modified (the reference scales its
 *           buffer by 0.5 in place, :1202-1205; the compat layer reproduces that side effect).
 *   d_bits  all_iters ? [B][iterations][K] : [B][K]  uint8 hard decisions in natural order
 *           (row `it` = flow_decoded + K*it of the reference, :1261-1264).
 *   d_le    nullable, [B][iterations][2][K+3] extrinsic Le after SISO1 and SISO2
 *           (:1234-1238, :1255-1259), same dtype as d_llr.
 *   stream  hipStream_t (NULL = default stream).  Asynchronous; no host synchronisation.
 * A handle owns ONE device workspace: decodes on one handle never overlap.  A decode issued on a
 * different stream than the previous one waits on the device (hipStreamWaitEvent) until the
 * previous decode is done with the workspace; for concurrent decodes use one handle per stream.
 * A decode captured into a hipGraph (stream capture) neither waits on nor records that event, so
 * graph replays are not ordered against eager decodes on the same handle: issue them on one
 * stream, or order them with events.  Call td_reserve before capturing (no allocation inside).
 * A handle is not thread-safe: one host thread uses it at a time; handles on different threads
 * (and devices) are independent (examples/multi_gpu_decode.cpp).
 */
int td_decode_device(td_handle* h, const void* d_llr, int B, uint8_t* d_bits, int all_iters, void* d_le,
                     void* stream);

/*
 * Decoding schedule of the handle (BASELINE config 5).  NULL or window = 0
 * (the default) is the exact full-trellis schedule of log_map.cpp.  Otherwise each codeword's
 * trellis is cut into floor(L/window) sub-blocks (the last also takes the remainder, e.g. the 3
 * tail steps) decoded in parallel: a sub-block's alpha starts `overlap` steps early and its beta
 * `overlap` steps late from equal metrics, or with nii = 1 from the metrics the neighbouring
 * chain had there in the previous iteration (NII, turboDecoderBianJieZhi.cu:248,302-304,
 * 312,397-400); concurrent = 1 runs both SISOs at once on the other's extrinsic of the previous
 * iteration (turboDecoderBianJieZhi.cu:642-690) instead of the serial order; the extrinsic is
 * multiplied by ext_scale (1 = none; 0.77 in the reference GPU decoders, :423-434).  Windowed
 * decoding changes the arithmetic: its gate is the BER curve, not bit-exactness.
 *   the reference GPU decoder with P sub-blocks: {6144/P, 0, 1, 1, 0.77}, TD_ALGO_MAXLOG, TD_F32
 */
/* Debug / measurement: the windowed kernels' layout (sub-blocks per lane run of the beta kernel and
 * of the alpha kernel, batch parts on as many streams; 0 = the layout's own choice).  Results do
 * not depend on it; speed does.  Applies to the current and later td_set_window. */
int td_debug_window_layout(td_handle* h, int run, int run_a, int parts);
typedef struct td_window_params {
    int window;        /* sub-block length W (0 = exact schedule) */
    int overlap;       /* warm-up steps, 0 <= overlap <= 3*window */
    int nii;           /* 1: boundary metrics from the previous iteration */
    int concurrent;    /* 1: both SISOs concurrently (Jacobi) */
    double ext_scale;  /* extrinsic scale, (0, 4] */
} td_window_params;
/* The max* of the windowed log-MAP schedule (round 6).  TD_WMAXSTAR_FAST (the default): the
 * reference's 16-step correction (log_map.cpp:14-18, 779-801) on a finer bucket grid (8 buckets an
 * octave of d, each with the reference's value at its midpoint), read with ONE table read and no
 * threshold compare -- it differs from E_algorithm only for d within half a bucket of one of its
 * thresholds, by one table step; TD_WMAXSTAR_EXACT: E_algorithm exactly (the exact schedule's
 * form).  The windowed schedule is BER-gated either way (the BER curves of both).
 * No effect on the exact schedule or Max-Log-MAP. */
enum td_window_maxstar { TD_WMAXSTAR_FAST = 0, TD_WMAXSTAR_EXACT = 1 };
int td_set_window_maxstar(td_handle* h, int form);
/* Creates the windowed schedule's extra streams and events on the handle's device (once), so a
 * decode after td_set_window + td_reserve allocates and creates nothing and may be captured. */
int td_set_window(td_handle* h, const td_window_params* w);

/*
 * Per-codeword early termination of the exact schedule (an extension: the reference always runs all
 * N_ITERATION).  Off by default; with it off every decode launches the kernels it always did.
 * Iteration numbers below are 1-based counts; row(n) is the hard-decision row after n iterations,
 * exactly as a full decode produces it (row n-1 of an all_iters decode).
 *   TD_STOP_HDA  codeword b stops after the smallest n >= max(2, min_iters) with row(n) == row(n-1)
 *                on all K bits (hard-decision aided rule); without such an n, at `iterations`.
 *   TD_STOP_CRC  it stops after the smallest n >= max(1, min_iters) at which the CRC-24 remainder of
 *                row(n) is zero: the K bits in natural order, first bit first, zero initial state, no
 *                final XOR -- the LTE code-block CRC.  crc_poly holds the 24 low-order coefficients
 *                of the generator: 0x800063 gCRC24B, 0x864CFB gCRC24A.  Needs K > 24.
 * Both: iters_used[b] = n and the decoded bits of b are row(n).  A codeword's result does not depend
 * on the codewords it shares a batch (or a workgroup's group of 8) with: a stopped codeword's
 * outputs are frozen while its group's other codewords go on, and the workgroup ends once all of
 * its codewords have stopped.  With all_iters, rows <= n equal the full decode's and rows
 * n+1 .. iterations are copies of row(n) (the frozen-row convention: per-iteration error counts and
 * the drop-in's flow_decoded rows stay meaningful).  d_le entries of iterations <= iters_used[b]
 * equal the full decode's; later entries are unspecified.  min_iters in [1, iterations];
 * min_iters == iterations reproduces the full decode, with every count = iterations.
 * These entry points belong to the exact schedule: setting a rule on a windowed handle, or a window
 * on a handle with a rule, is TD_EINVAL.  The windowed schedule's rule is td_set_window_stop (below).
 * td_set_early_stop(NULL or rule TD_STOP_NONE) turns it off.  TD_EINVAL: unknown rule, min_iters out
 * of range, TD_STOP_CRC with crc_poly == 0 or K <= 24, a windowed handle.  The CRC rule's device
 * table is built here, so a decode allocates nothing for the feature (td_reserve + capture holds).
 */
enum td_stop_rule { TD_STOP_NONE = 0, TD_STOP_HDA = 1, TD_STOP_CRC = 2 };
typedef struct td_stop_params {
    int rule;            /* enum td_stop_rule */
    int min_iters;       /* no codeword stops before this many iterations */
    uint32_t crc_poly;   /* TD_STOP_CRC: the generator's 24 low-order coefficients */
} td_stop_params;
int td_set_early_stop(td_handle* h, const td_stop_params* s);
/*
 * Per-codeword early termination of the windowed schedule: the same two rules, td_stop_params, frozen-row
 * convention and iters_used output, judged on the windowed decode's own rows.  Off by default; with it
 * off a windowed decode launches the kernels it always did.
 *   row(n)  the hard-decision row after n iterations of the full windowed decode with the handle's
 *           window parameters, max* form, precision and algorithm (row n-1 of an all_iters decode with
 *           the rule off).
 *   TD_STOP_HDA  codeword b stops after the smallest n >= max(2, min_iters) with row(n) == row(n-1) on
 *                all K bits; without such an n, at `iterations`.
 *   TD_STOP_CRC  after the smallest n >= max(1, min_iters) with CRC-24(row(n)) == 0 (the polynomial
 *                convention of td_set_early_stop).  Needs K > 24.
 * iters_used[b] = n and the decoded bits of b are row(n).  With all_iters, rows <= n equal the full
 * decode's and rows n+1 .. iterations are copies of row(n).  d_le entries of iterations <= n equal the
 * full decode's; later entries are unspecified.  A codeword's result does not depend on its batch
 * companions: not on its wave of 64, its workgroup, its lane-run layout (td_debug_window_layout), nor
 * on the batch parts and streams -- a stopped codeword's outputs are frozen while its wave's other
 * codewords go on, and a wave ends its launches at once when all of its codewords have stopped (which
 * is where the time is saved).  min_iters == iterations reproduces the full decode byte for byte.
 * This holds for every schedule option: serial and concurrent SISOs, NII on and off, any ext_scale and
 * overlap, both max* forms and Max-Log-MAP, fp64 and fp32, batches of one codeword.
 * Valid only on a handle whose current schedule is windowed (td_set_window first): otherwise
 * TD_EINVAL.  Argument checks as td_set_early_stop (TD_EINVAL: unknown rule, min_iters outside
 * [1, iterations], TD_STOP_CRC with crc_poly == 0 or K <= 24); a failed call leaves the previous
 * setting in place.  NULL or rule TD_STOP_NONE turns the rule off.  The rule survives later
 * td_set_window calls with window > 0; td_set_window(NULL or window 0) clears it.  The CRC rule's
 * device table is built here, and the rule's per-codeword state lives in the windowed buffers that
 * td_reserve sizes (whether or not a rule is set), so after td_reserve a decode allocates and creates
 * nothing and may be captured into a hipGraph.  td_decode_device_stop / td_decode_host_stop fill the
 * counts; the plain entry points behave like them with a null count pointer.
 * td_clock_read after a decode with this rule returns TD_EINVAL: the stopping kernels take no clock
 * sample (the workgroup that takes it may have nothing left to do).
 */
int td_set_window_stop(td_handle* h, const td_stop_params* s);
/* td_decode_device plus d_iters: nullable int32 [B], iterations used per codeword.  td_decode_device
 * (and td_decode_host) on a handle with a rule set behave like these with a null count pointer; these
 * on a handle without a rule (of either schedule) behave like the plain entry points and fill the
 * counts with `iterations`. */
int td_decode_device_stop(td_handle* h, const void* d_llr, int B, uint8_t* d_bits, int all_iters, void* d_le,
                          int32_t* d_iters, void* stream);
int td_decode_host_stop(td_handle* h, const void* llr, int B, int* out, void* le, int* iters_used);
/* Host only (no GPU): the CRC-24 remainder of bits[0..K) (one bit per byte) as TD_STOP_CRC defines it,
 * and the per-position table the kernel uses -- table[i] = the remainder of the row with only bit i
 * set, so that the remainder of any row is the XOR of the entries of its set bits. */
uint32_t td_crc24_host(const uint8_t* bits, int K, uint32_t poly);
int td_crc24_syndromes(int K, uint32_t poly, uint32_t* table /* [K] */);

/*
 * The fixed-point decoder, precision TD_FIXED (an extension: ITTC/main.h:21-24 declares TurboDecodingfixpoint
 * and the reference never defines it).  The decoder an LTE receiver with an int8 soft buffer uses: exact
 * full-trellis schedule, TD_ALGO_MAXLOG only, K >= 8 (td_create: TD_EINVAL otherwise).  All values are
 * integers:
 *   input      q[3K+12] int8 in the reference stream layout; -128 is read as -127.
 *   demultiplex  as log_map.cpp:1083-1127 without the x0.5: xs1, xp1, xs2 = xs1 o pi, xp2, each K+3 long.
 *   SISO       branch metric of state s, input u at position i: (2u-1)(xs[i] + La[i]) + o_u(s) xp[i], with
 *              o_u(s) = +-1 the branch's parity (twice the float decoder's metric).  alpha and beta with
 *              plain max, both terminated in state 0.  Lambda[i] = max over the u = 1 branches of
 *              alpha + gamma + beta, minus the same over u = 0; LLR[i] = Lambda[i] >> 1 (Lambda is even).
 *   iteration  as log_map.cpp:1217-1265: La = deinterleaved Le (tails 0), SISO1, Le = f(LLR - La - xs1),
 *              interleave, SISO2, Le = f(LLR - La - xs2), hard bit = (LLR < 0) ? 0 : 1, deinterleaved.
 *   f(r)       clamp(sign(r) ((|r| ext_scale_q) >> 2), -le_max, +le_max): the extrinsic scaled by
 *              ext_scale_q quarters, truncated towards zero, clamped.
 * Nothing else saturates: the state metrics are wide enough for any int8 input and any allowed
 * parameters.  With ext_scale_q = 4 and no clamp in effect the decode equals the fp64
 * Max-Log-MAP decode of the same integers, bits and Le.
 * On a TD_FIXED handle td_decode_device / td_decode_device_stop / td_decode_host / td_decode_host_stop take
 * int8 LLRs [B][3K+12] (not modified) and give the bits as ever and d_le / le as int16
 * [B][iterations][2][K+3]; the _stop forms fill the counts with `iterations` unless a rule is set
 * (td_set_fixed_stop below: the fixed decoder's early termination).  Asynchronous, one workspace, event ordering and capture as
 * documented at td_decode_device.  td_reserve sizes the workspace with a plain allocation (no placement
 * search); after it a decode allocates nothing and may be captured into a hipGraph.  td_profile_read
 * reports the demultiplex (the transpose of the int8 stream into the workspace) and the decode.
 * td_rate_dematch takes int8 d_e and int8 d_llr (see there); td_rate_match with elem_size 1 moves int8.
 * TD_EINVAL on a TD_FIXED handle, never silently ignored: td_set_window, td_set_window_maxstar,
 * td_set_early_stop, td_set_window_stop, td_siso_host, td_clock_read, td_debug_set_stamps.  The other
 * way round, td_set_fixed, td_set_fixed_stop, td_set_fixed_window and td_set_fixed_window_stop are TD_EINVAL
 * on a handle of another precision.
 *
 * td_set_fixed: le_max in [1, 255], ext_scale_q in [1, 4] (quarters; 4 = no scaling); the default is
 * {255, 3}, which NULL restores.  TD_EINVAL on a handle of another precision or a value out of range; a
 * failed call leaves the setting as it was.
 */
typedef struct td_fixed_params {
    int le_max;        /* the extrinsic's clamp */
    int ext_scale_q;   /* the extrinsic's scale in quarters */
} td_fixed_params;
int td_set_fixed(td_handle* h, const td_fixed_params* f);
/*
 * Integer log-MAP on a TD_FIXED handle: max plus a small correction table (max*), the fixed decoder's form
 * of the float decoders' TD_ALGO_LOGMAP.  Off by default (Max-Log-MAP, whose kernels do not change; td_create
 * keeps taking TD_ALGO_MAXLOG only for TD_FIXED); NULL turns it off.  With a table set every max(a, b) of the
 * TD_FIXED contract above -- and of td_set_fixed_window's sub-blocks, warm-ups included -- becomes
 *   maxs(a, b) = max(a, b) + corr[min(|a - b| >> shift, 7)]
 * maxs rounds, so it is not associative, and the order of every operation is part of the contract:
 *   alpha   into state j: maxs(alpha[p0] + gamma, alpha[p1] + gamma), p0 the u = 0 predecessor of j first.
 *   beta    of state s: maxs(gamma_0(s) + beta[next(s,0)], gamma_1(s) + beta[next(s,1)]).
 *   Lambda  each of its two terms is a left fold with maxs over the source state s = 0, 1, ..., 7 of
 *           alpha[s] + gamma_u(s) + beta[next(s,u)]; Lambda = the u = 1 fold minus the u = 0 fold.
 * Lambda is no longer even: LLR = Lambda / 2 truncated towards zero, as f truncates (on even Lambda the
 * contract's >> 1).  The hard bit, f, the iteration, the sub-block geometry, both early-termination rules
 * (judged on the rows of the decode with the table) and the layouts of d_bits and d_le are unchanged.
 * corr[7] == 0 makes maxs of a reachable sum and an unreachable one the reachable sum exactly, so no output
 * depends on the value that stands for "unreachable".  With entries <= 63 a step adds at most 509 + 63 to a
 * state metric, |alpha|, |beta| <= 572 * 10003 < 2^23 and a Lambda term with its fold's corrections stays below
 * 2^24: nothing saturates but the contract's two clamps, and every value is defined bit for bit
 * (tests/fixed_maxstar_ref.py restates it).  An all-zero table is Max-Log-MAP.
 * td_set_fixed's default {255, 3} is not changed by a table, but its 3/4 scale exists to compensate Max-Log-MAP's
 * overestimate: log-MAP wants {255, 4} (DESIGN.md "Fixed point").
 * The table applies to all four fixed schedules -- exact, td_set_fixed_stop, td_set_fixed_window,
 * td_set_fixed_window_stop -- whatever the order of the calls, and survives td_set_fixed, the window setters and
 * the stop setters.  It travels as kernel arguments: the workspace does not grow, and after td_reserve a decode
 * allocates nothing and may be captured into a hipGraph.
 * TD_EINVAL, never silently ignored, and a failed call changes nothing: a null handle or one of another
 * precision; shift outside [0, 8]; an entry above 63; corr[7] != 0.
 *
 * td_fixed_maxstar_table (host only, no handle): the table for inputs quantised at steps_per_unit steps per
 * unit LLR.  The integer branch metric is twice the float one, so a nat is s = 2 steps_per_unit metric steps:
 *   corr[j] = floor(s log1p(exp(-(j + 1/2) 2^shift / s)) + 1/2) for j < 7, corr[7] = 0
 * and with shift < 0 the smallest shift at which s log1p(exp(-7 2^shift / s)) < 1.  At 8 steps per unit:
 * shift 3 and {9, 6, 4, 3, 2, 1, 1, 0}.  TD_EINVAL: a null output, steps_per_unit outside (0, 32], or a rule
 * that gives an entry above 63 or a shift above 8.
 */
typedef struct td_fixed_maxstar_params {
    int shift;          /* bucket width 2^shift, 0 .. 8 */
    uint8_t corr[8];    /* correction of bucket j, each 0 .. 63, corr[7] == 0 */
} td_fixed_maxstar_params;
int td_set_fixed_maxstar(td_handle* h, const td_fixed_maxstar_params* m);   /* NULL: off (Max-Log-MAP) */
int td_fixed_maxstar_table(double steps_per_unit, int shift /* < 0: choose */, td_fixed_maxstar_params* out);
/*
 * Per-codeword early termination of the fixed-point decoder: the third sibling of td_set_early_stop and
 * td_set_window_stop, with their two rules, td_stop_params, frozen-row convention and iters_used output,
 * judged on the fixed decode's own rows.  Off by default; with it off a fixed decode launches the
 * kernels it always did.
 *   row(n)  the hard-decision row after n iterations of the full fixed decode with the handle's
 *           td_set_fixed setting (row n-1 of an all_iters decode with the rule off).
 *   TD_STOP_HDA  codeword b stops after the smallest n >= max(2, min_iters) with row(n) == row(n-1) on
 *                all K bits; without such an n, at `iterations`.
 *   TD_STOP_CRC  after the smallest n >= max(1, min_iters) with CRC-24(row(n)) == 0 (the polynomial
 *                convention of td_set_early_stop and td_crc24_host).  Needs K > 24.
 * iters_used[b] = n and the decoded bits of b are row(n).  With all_iters, rows <= n equal the full
 * decode's and rows n+1 .. iterations are copies of row(n).  d_le entries of iterations <= n equal the
 * full decode's; later entries are unspecified (the decoder does not write them).  A codeword's result
 * does not depend on its wave of 64, its batch or the batch size: a stopped codeword's lane is skipped
 * while its wave's other codewords go on, and a wave returns once all of its codewords have stopped
 * (which is where time can be saved).  min_iters == iterations reproduces the full decode byte for byte.
 * Valid only on a TD_FIXED handle: otherwise TD_EINVAL.  Argument checks as td_set_early_stop
 * (TD_EINVAL: unknown rule, min_iters outside [1, iterations], TD_STOP_CRC with crc_poly == 0 or
 * K <= 24); a failed call leaves the previous setting in place.  NULL or rule TD_STOP_NONE turns the
 * rule off.  The rule survives td_set_fixed.  The CRC rule's device table (td_crc24_syndromes) is built
 * here, and the per-codeword counts live in the workspace that td_reserve sizes (whether or not a rule
 * is set), so after td_reserve a decode allocates nothing and may be captured into a hipGraph.
 * td_decode_device_stop / td_decode_host_stop fill the counts; the plain entry points behave like them
 * with a null count pointer.
 */
int td_set_fixed_stop(td_handle* h, const td_stop_params* s);
/*
 * The fixed-point decoder's sub-block schedule: the integer form of td_set_window's geometry, for
 * batches too small to fill the chip with one lane a codeword.  Off by default (the exact full-trellis
 * schedule above, whose kernels do not change); NULL or window == 0 restores it.  Otherwise window (W)
 * is a multiple of 16, >= 16, and 0 <= overlap <= 3 W.  With L = K + 3 and nS = max(1, L / W) (integer
 * division) each SISO pass of the TD_FIXED contract above becomes nS independent passes:
 *   sub-block s   covers the positions [s W, (s+1) W); the last one, s = nS - 1, runs up to L (it takes the
 *                 remainder and the tail: up to 2 W - 1 + 3 positions).  Call its end e.
 *   alpha         starts at position max(s W - overlap, 0): from the terminated state (state 0 = 0, the
 *                 others unreachable) if s W - overlap <= 0, else from equal metrics (all states 0).
 *   beta          starts at position min(e + overlap, L): from the terminated state if e + overlap >= L,
 *                 else from equal metrics.
 *   warm-up       the steps outside [s W, e) only carry the recursions; they produce no output.
 *   output        Lambda, LLR = Lambda >> 1 (Lambda stays even), Le = f(LLR - La - xs) with the handle's
 *                 td_set_fixed setting and the hard bit at the sub-block's own positions, from its own
 *                 alpha and beta: exactly the TD_FIXED contract's branch metric, plain max and f.
 * The iteration (SISO1 over all sub-blocks, then SISO2 over all sub-blocks, serially), the hard decision
 * and the layouts of d_bits and d_le are the TD_FIXED contract's.  No concurrent SISOs and no extra
 * extrinsic scale (td_window_params' concurrent and ext_scale have no counterpart here; its nii is
 * td_set_fixed_window_nii below, off by default).  The state metrics are wide enough that nothing saturates but the contract's two
 * clamps; the result is the one that un-normalised integers of unlimited width give (max-log does not
 * change when a constant is added to all states, so an implementation may normalise or not).  Every
 * value is therefore defined bit for bit (tests/fixed_window_ref.py restates it).
 * Consequences: with overlap >= L, or window > L/2 (nS = 1), the decode equals the exact fixed decode
 * bit for bit, bits and Le; and a codeword's result does not depend on the batch size, its lane or its
 * wave.
 * TD_EINVAL, never silently ignored, and a failed call changes nothing: a handle of another precision;
 * window negative or not a multiple of 16; overlap outside [0, 3 W]; a handle with a td_set_fixed_stop
 * rule set.  The other way round td_set_fixed_stop with a rule is TD_EINVAL while a window is set (as
 * td_set_early_stop and td_set_window exclude each other): the windowed fixed decode's early
 * termination is td_set_fixed_window_stop's (below), and without it the _stop entry points fill the counts
 * with `iterations`.  td_set_fixed works on either schedule and the window survives it.  td_reserve sizes
 * everything (the workspace is the exact schedule's -- a sub-block checkpoints only its own 16-step
 * windows -- and 6 bytes per 16 positions and codeword for td_set_fixed_window_stop's evidence, carved
 * whether or not a rule is set: 2.2 % more at K = 6144); after it a decode allocates and creates nothing
 * and may be captured into a hipGraph.  Without a rule a decode is one launch per SISO and iteration on
 * the decode's stream.  td_profile_read reports the demultiplex and the decode as before;
 * td_clock_read stays TD_EINVAL; td_rate_dematch's int8 output decodes unchanged.
 */
typedef struct td_fixed_window_params {
    int window;    /* positions per sub-block: 0 = the exact schedule, else a multiple of 16 */
    int overlap;   /* warm-up positions on each side, 0 .. 3 * window */
} td_fixed_window_params;
int td_set_fixed_window(td_handle* h, const td_fixed_window_params* w);
/*
 * Next-iteration initialisation (NII) of the sub-block schedule: the integer counterpart of
 * td_window_params.nii, which lets a smaller overlap do (profiles/fixed/window_nii_ber.json).  Off by
 * default; with it off a decode launches the kernels it always did.  With it on the schedule is
 * td_set_fixed_window's in every detail except the start vectors of warm-ups that do not begin at a trellis
 * end, in iterations n >= 2 (1-based).  For SISO d in {1, 2}, sub-block s covering [s W, e), a_from =
 * s W - overlap and b_from = e + overlap:
 *   alpha   if a_from > 0, starts from A[a_from] of SISO d in iteration n - 1, where A[p] is the alpha
 *           vector before step p as computed by the sub-block that outputs position p - 1, sub-block
 *           (p - 1) / W (the neighbouring chain that has run longest, not another sub-block's warm-up).
 *   beta    if b_from < L, starts from B[b_from] of SISO d in iteration n - 1, where B[p] is the beta
 *           vector after the backward step over position p as computed by the sub-block that outputs
 *           position p, sub-block min(p / W, nS - 1).
 * Iteration 1 starts from equal metrics, and a warm-up that reaches a trellis end starts terminated, as
 * without NII.  Both max and td_set_fixed_maxstar's maxs are unchanged by a constant added to all eight
 * states, so A and B are defined up to one constant per vector: the outputs are those of un-normalised
 * integers of unlimited width (the implementation stores the vectors relative to their maximum, an
 * unreachable state staying unreachable), and rows of every iteration and every Le stay defined bit for
 * bit (tests/fixed_window_nii_ref.py restates it).  Consequences: row 1 and Le of iteration 1 equal the NII-off
 * decode's; with overlap >= L or nS = 1 the decode is still the exact fixed decode; a codeword's result
 * does not depend on its lane, wave, batch or the batch size, nor on what the handle decoded before
 * (the state is never read in iteration 1, so a graph replay repeats the bytes); the two SISOs keep
 * separate state.
 * Valid on a TD_FIXED handle with a window set, otherwise TD_EINVAL.  With NII on the overlap must be a
 * multiple of 16 (the vectors are then taken between the 16-step windows of the kernel): turning NII on
 * with another overlap is TD_EINVAL, and so is td_set_fixed_window with such an overlap while NII is on.  A
 * failed call changes nothing.  NII survives td_set_fixed, td_set_fixed_maxstar, td_set_fixed_window_stop and a
 * later td_set_fixed_window with window > 0; td_set_fixed_window(NULL or window 0) clears it.  It works with
 * td_set_fixed_maxstar's table and with td_set_fixed_window_stop's rules, which judge the NII decode's own
 * rows (min_iters == iterations still reproduces the rule-off NII decode byte for byte).
 * The state is 128 bytes per sub-block and codeword behind the workspace, carved only while NII is on
 * and sized for the current window (12 % more at K = 6144, window 64, 8 iterations): a handle that never
 * turns NII on keeps the workspace it had.  So td_reserve belongs after td_set_fixed_window_nii (and after
 * td_set_fixed_window): a decode after it allocates nothing and may be captured into a hipGraph; without it
 * a decode grows the workspace on demand, as it does for B.
 */
int td_set_fixed_window_nii(td_handle* h, int on);   /* 0 = off (default) */
/*
 * Per-codeword early termination of the fixed-point decoder's sub-block schedule: the fourth sibling of
 * td_set_early_stop, td_set_window_stop and td_set_fixed_stop, with their two rules, td_stop_params,
 * frozen-row convention and iters_used output, judged on the windowed fixed decode's own rows.  Off by
 * default; with it off a windowed fixed decode launches the kernels it always did and the _stop entry
 * points fill the counts with `iterations`.
 *   row(n)  the hard-decision row after n iterations of the full td_set_fixed_window decode with the
 *           handle's window, overlap and td_set_fixed setting (row n-1 of an all_iters decode with the
 *           rule off).
 *   TD_STOP_HDA  codeword b stops after the smallest n >= max(2, min_iters) with row(n) == row(n-1) on
 *                all K bits; without such an n, at `iterations`.
 *   TD_STOP_CRC  after the smallest n >= max(1, min_iters) with CRC-24(row(n)) == 0 (td_crc24_host's
 *                convention).  Needs K > 24.
 * iters_used[b] = n and the decoded bits of b are row(n).  With all_iters, rows <= n equal the full
 * decode's and rows n+1 .. iterations are copies of row(n).  d_le entries of iterations <= n equal the
 * full decode's; later entries are unspecified (the decoder does not write them).  min_iters ==
 * iterations reproduces the rule-off decode byte for byte, every count `iterations`.  A codeword's
 * result does not depend on its lane, its wave of 64, its batch or the batch size.
 * Valid only on a TD_FIXED handle whose schedule is the sub-block one (td_set_fixed_window with window > 0
 * first): otherwise TD_EINVAL, NULL included.  Argument checks as td_set_fixed_stop (TD_EINVAL: unknown
 * rule, min_iters outside [1, iterations], TD_STOP_CRC with crc_poly == 0, with coefficients above the
 * 24 low-order ones or with K <= 24); a failed call changes nothing.  NULL or rule TD_STOP_NONE turns the
 * rule off.  The rule survives td_set_fixed and a later td_set_fixed_window with window > 0;
 * td_set_fixed_window(NULL or window 0) clears it, as td_set_window does td_set_window_stop's.
 * td_set_fixed_stop stays TD_EINVAL while a window is set, and td_set_fixed_window while a
 * td_set_fixed_stop rule is.
 * A decode with the rule resets the per-codeword state on its stream, then launches per iteration
 * SISO1, SISO2 and a decision kernel (one thread per codeword): a wave all of whose 64 codewords have
 * stopped returns at once, which is where time is saved; a stopped codeword in a running wave is
 * skipped.  The state and the evidence live in the workspace that td_reserve sizes, and the CRC rule's
 * device table is built here, so after td_reserve a decode allocates and creates nothing and may be
 * captured into a hipGraph (a replay repeats the reset).  td_decode_device_stop / td_decode_host_stop
 * fill the counts; the plain entry points behave like them with a null count pointer.  td_clock_read
 * stays TD_EINVAL.
 */
int td_set_fixed_window_stop(td_handle* h, const td_stop_params* s);

/* Kernel timing (measurement support): while enabled, hipEvents on the decode stream bracket
 * the demultiplex kernel and the turbo kernel of every td_decode_device call.
 * td_profile_read synchronises on them, returns the average durations (ms) over the
 * `launches` decodes since the last read/enable, and starts a new accumulation. */
int td_profile_enable(td_handle* h, int on);
int td_profile_read(td_handle* h, float* demux_ms, float* decode_ms, int* launches);
/* Launch clock (measurement support): every exact-schedule turbo launch records, in its first
 * workgroup, the shader clock (s_memtime) and the 100 MHz real-time counter (s_memrealtime) at that
 * workgroup's start and end; a windowed decode records the same in the first workgroup of its
 * last SISO2 beta launch (round 5).  td_clock_read waits for this handle's last decode (not the
 * whole device) and returns the sustained shader clock (GHz) over that workgroup's span (ms: the
 * whole launch for the exact schedule, one workgroup's lifetime for a windowed one);
 * TD_EINVAL before any decode, when the last decode was graph-captured, or when it was a windowed
 * decode with early termination (td_set_window_stop). */
int td_clock_read(td_handle* h, double* sclk_ghz, double* span_ms);

/* Diagnostics: in a library built with -DTD_STAMPS (td_debug_stamp_slots() > 0) the turbo
 * kernel writes per-wave shader-clock totals of its phases into d_buf [ceil(B/8)][slots]
 * (uint64).  The production library ignores the buffer and reports 0 slots. */
int td_debug_set_stamps(td_handle* h, void* d_buf);
int td_debug_stamp_slots(void);
/* Workspace placement of the last td_reserve that allocated (see td_reserve): the number of
 * candidate workspaces timed (0 = plain allocation), their probe times in ms (up to cap of them)
 * and the index kept. */
int td_debug_placement(td_handle* h, float* ms, int cap, int* pick);
/* Cost of that search: its wall time (ms) and the peak bytes of candidate workspaces it held. */
int td_debug_placement_cost(td_handle* h, double* wall_ms, double* held_bytes);
/* Bytes of the handle's decode workspace (0 before the first reserve / decode). */
int td_debug_workspace_bytes(td_handle* h, unsigned long long* bytes);
/* Fill the handle's scratch with one byte, so that a test can show that no decode depends on what its
 * workspace held before (tests only).  byte in 0..255: synchronises the device, sets every device
 * buffer a decode uses as scratch to that byte -- the decode workspace, the windowed schedule's buffers
 * (second extrinsic pair, checkpoints, NII metrics, bits, stop state) and td_decode_host's staging
 * buffers, where allocated -- synchronises again and arms the handle: from then on every allocation or
 * growth of those buffers (td_reserve's kept candidate included) and td_siso_host's scratch are filled
 * with the same byte right after they are allocated.  byte == -1 disarms the handle.  The handle's
 * tables (permutations, max* tables, lane tables, CU slots, CRC syndromes, rate-matching tables) and
 * the frame generator's state are never touched.  *filled (may be null) receives the bytes this call
 * wrote.  Must not be called while a stream is capturing (it synchronises the device), and an armed
 * handle must not allocate inside a capture either (td_reserve first, as always).  A disarmed handle
 * launches and synchronises exactly what it did without this call.  TD_EINVAL for any other byte. */
int td_debug_workspace_fill(td_handle* h, int byte, unsigned long long* filled);
/* The placement search's stop rule on probe times ms[0..n) (host only, for tests): 1 if the search
 * would stop after them (the fast mode seen), else 0; TD_EINVAL on a bad argument. */
int td_debug_placement_rule(const float* ms, int n);

/* Trellis steps per window of the exact schedule's turbo kernel (15; fp32 at four workgroups per
 * CU runs a 12-step build).  Measurement support: bench.py's traffic model. */
int td_window_steps(void);

/* Host-pointer convenience (pageable buffers; copies, decodes, synchronises).  The device staging
 * buffers are the handle's, allocated on the first call and grown when B grows, so the per-frame
 * caller (the drop-in's TurboDecoding) allocates nothing after its first frame.
 *   out  int[B][iterations][K] exactly like the reference's flow_decoded (one row per iteration)
 *   le   nullable host [B][iterations][2][K+3]. */
int td_decode_host(td_handle* h, const void* llr, int B, int* out, void* le);

/*
 * Batched Log_MAP_decoder (log_map.cpp:898-1047) -- the SISO, host pointers.
 *   recs [B][2L] (ys, yp) pairs, La [B][L], LLR [B][L] out; dtype by h's precision.
 *   terminated: 1 = beta starts in state 0 (TERMINATED, log_map.h:24), 0 = all states equal.
 */
int td_siso_host(td_handle* h, const void* recs, const void* La, int terminated, void* LLR, int L, int B);

/*
 * Device frame generator: the frames ITTC/main.cpp makes (main.cpp:170-202)
 * -- source bits rand() % 2, TurboEnCoding, BPSK, AWGN on I and Q (mgrns, log_map.cpp:1359-1400),
 * BPSK demodulation (modanddem.cpp:189-224) -- with the process-wide glibc rand() stream of
 * srand(seed), bit-identical to the reference, generated on the GPU.
 *   td_synth_seed    srand(seed): (re)starts the handle's frame stream (main.cpp:170)
 *   td_synth_frames  the next B frames of the stream at Eb/N0 = ebn0_db:
 *                    d_info [B][K] uint8 source bits, d_llr [B][3K+12] double channel LLRs
 *                    (TurboDecoding's input).  Synchronous with respect to the host.
 */
int td_synth_seed(td_handle* h, unsigned seed);
/* Position the stream at frame `frame` of srand(seed) (each frame draws K+2 rand() values). */
int td_synth_seek(td_handle* h, unsigned long long frame);
/* Host utility behind td_synth_frames (exported for tests): the generator window
 * x[n-31 .. n-1] of srand(seed) after `draws` rand() calls; the next rand() is
 * (win[0] + win[28]) >> 1. */
int td_rand_window(unsigned seed, unsigned long long draws, uint32_t* win);
int td_synth_frames(td_handle* h, double ebn0_db, int B, uint8_t* d_info, double* d_llr, void* stream);

/* Modulation of the generator's frames (MODULATION, main.cpp:13-15, 174, 197-202): 1 = BPSK
 * (default), 2 = QPSK, 3 = 8PSK, 4 = 16QAM, 6 = 64QAM bits per symbol; SYMBOL_NUM = (3K+12)/M
 * symbols, sigma = 10^(-EbN0/20) sqrt(0.5 / (rate M)) with rate = K / SYMBOL_NUM.  TD_EINVAL when
 * 3K+12 is not a multiple of M. */
int td_synth_modulation(td_handle* h, int modulation);

/* Replaces module (modanddem.cpp:175-187, _bpsk/_qpsk/_8psk/_16qam/_64qam_module :88-173) on
 * device arrays: d_bits [nsym * modulation] uint8 (0/1; the reference takes int) -> d_si, d_sq [nsym]. */
int td_modulate(const uint8_t* d_bits, long long nsym, int modulation, double* d_si, double* d_sq, void* stream);
/* Replaces demodule (modanddem.cpp:674-685, the max-log demappers :189-671) on device arrays:
 * d_yi, d_yq [nsym] received symbols -> d_llr [nsym * modulation], bit-exact with the reference. */
int td_demodulate(const double* d_yi, const double* d_yq, long long nsym, int modulation, double Kf, double* d_llr,
                  void* stream);

/*
 * d_in [n] double -> d_out [n] in `precision` (enum td_precision): the conversion between td_demodulate's
 * output and what td_rate_dematch and td_decode_device take (an extension: the reference decodes doubles only).
 * No handle.
 *   TD_F64    a copy.
 *   TD_F32    (float)x, the IEEE round-to-nearest-even narrowing; a value too large becomes +-inf.
 *   TD_FIXED  the int8 q = clamp(rint(x * steps_per_unit), -127, 127): the product is one rounded double
 *             multiply, rint rounds to nearest with ties to even, and the clamp happens in double before the
 *             conversion to integer, so +-1e300 and +-inf give +-127 and no conversion is undefined.  -128 is
 *             never produced.
 * NaN inputs: unspecified (the library is built with -fno-honor-nans).  steps_per_unit is used only with
 * TD_FIXED.  Asynchronous on `stream`, allocates nothing, may be captured into a hipGraph.  n = 0 is a no-op.
 * Pointers need only element alignment; the bytes do not depend on it.
 * TD_EINVAL: a null pointer, n < 0, an unknown precision, with TD_FIXED steps_per_unit not finite or <= 0.
 */
int td_llr_convert(const double* d_in, long long n, int precision, double steps_per_unit, void* d_out, void* stream);

/* Error counts per frame and iteration for the BER harness (main.cpp:224-237):
 * d_err[b][it] = #{i < K : d_bits[b][it][i] != d_info[b][i]}, d_bits as td_decode_device's
 * all_iters output with `iters` rows. */
int td_count_errors(td_handle* h, const uint8_t* d_bits, int iters, const uint8_t* d_info, int B, int* d_err,
                    void* stream);

/*
 * LTE rate matching (3GPP TS 36.212 5.1.4.1) around the decoder's stream (an extension: ITTC/main.h:23-24
 * declares rate_match / de_rate_match and the reference never defines them; the compat layer now does).
 * The coded stream s[0..3K+12) of encoderm_turbo (log_map.cpp:566-578) is the three LTE streams
 * interleaved, d_i(k) = s[3k+i], k < D = K+4 (the 12 tail values in order are d0_K, d1_K, d2_K, d0_K+1,
 * ... of 5.1.3.2.2); no filler bits (a transport block's: td_tb_* below).  Sub-block interleaver: 32 columns, R = ceil(D/32) rows, Kpi = 32R,
 * ND = Kpi - D leading <NULL>s.  Circular buffer: Kw = 3 Kpi entries, of which a soft buffer of Ncb <= Kw
 * is used; a transmission of redundancy version rv reads the E non-NULL entries from
 * k0 = R (2 ceil(Ncb / 8R) rv + 2) on, wrapping round w[0..Ncb) for as long as needed (E above the
 * buffer's non-NULL count: repetition).
 *   rate matching      e[b][k] = in[b][idx[k]], idx from the rule above
 *   de-rate-matching   its transpose: d_llr[b][q] = the sum of every e[b][k] with idx[k] == q, added in
 *                      ascending k in the buffer's own precision, starting from d_llr[b][q] itself with
 *                      `accumulate` (HARQ combining of a retransmission into the soft buffer) and from
 *                      +0.0 without; a position no k selects keeps its value (accumulate) or is 0.0.
 *                      No atomics: the same bits on every run.  The output is td_decode_device's input.
 * Ncb = 0 means Kw; otherwise Kpi <= Ncb <= Kw, else TD_EINVAL.  The first call builds and uploads the
 * handle's tables; the launches then allocate nothing (they may be captured into a hipGraph).  It may be
 * called again with another Ncb (it waits for the device first).
 * TD_EINVAL: a null pointer, rv outside 0..3, E < 1, elem_size other than 1, 4 or 8 bytes, B < 0, a bad
 * Ncb, a launch or an info call on a handle without tables.  B = 0 is a no-op.  Asynchronous on `stream`.
 */
int td_rm_set(td_handle* h, int Ncb);
/* The layout the handle's tables were built for (any pointer may be null); n_nonnull = the non-NULL
 * entries of w[0..Ncb). */
int td_rm_info(td_handle* h, int* R, int* Kpi, int* Kw, int* Ncb, int* n_nonnull);
/* d_in [B][3K+12] -> d_e [B][E], elements of elem_size bytes (1: uint8 bits, 4: float, 8: double). */
int td_rate_match(td_handle* h, const void* d_in, int elem_size, int B, int rv, int E, void* d_e, void* stream);
/* d_e [B][E] -> d_llr [B][3K+12]; both double for TD_F64, float for TD_F32, int8 for TD_FIXED.  In int8
 * each position is the sum of its e in ascending k saturated to [-127, 127] after every addition, starting
 * from d_llr itself (-128 read as -127) with `accumulate` and from 0 without; a position no k selects
 * keeps its value (accumulate) or is 0. */
int td_rate_dematch(td_handle* h, const void* d_e, int B, int rv, int E, void* d_llr, int accumulate, void* stream);
/*
 * The receive front end in one pass: received symbols -> the handle's soft buffer, with no LLR array in
 * between.  d_yi, d_yq [B][E / modulation] double symbols, codeword b's own E / modulation of them.  By
 * definition, byte for byte:
 *   demap    transmitted value k of codeword b is element b E + k of what td_demodulate(d_yi, d_yq,
 *            B E / modulation, modulation, Kf, .) writes: bit k % modulation of symbol
 *            b (E / modulation) + k / modulation;
 *   convert  that value goes through td_llr_convert to the handle's precision (steps_per_unit is used only on
 *            a TD_FIXED handle and ignored otherwise);
 *   combine  d_llr [B][3K+12] is what td_rate_dematch(h, e, B, rv, E, d_llr, accumulate, stream) gives on
 *            those e: sums in ascending k in the buffer's precision, int8 saturated to +-127 after every
 *            addition with -128 in the prior buffer read as -127, unselected positions kept (accumulate) or
 *            zero, no atomics, the same bytes on every run.
 * It uses the tables of td_rm_set, allocates nothing and may be captured into a hipGraph.  Asynchronous on
 * `stream`.  B = 0 is a no-op.  NaN symbols: unspecified, as for td_llr_convert.
 * TD_EINVAL: everything td_rate_dematch rejects (a null pointer, rv outside 0..3, E < 1, B < 0, a handle
 * without tables), modulation not 1, 2, 3, 4 or 6, E not a multiple of modulation (LTE's E always is one),
 * a TD_FIXED handle with steps_per_unit not finite or <= 0.
 */
int td_demod_dematch(td_handle* h, const double* d_yi, const double* d_yq, int B, int rv, int E, int modulation,
                     double Kf, double steps_per_unit, void* d_llr, int accumulate, void* stream);
/* Host only (no GPU, no handle): idx[k] = the stream position of e_k, k < E.  1 <= K <= 10000. */
int td_rm_index_host(int K, int Ncb, int rv, int E, int32_t* idx);

/*
 * The transmit side on device-resident bits (an extension: the reference encodes one frame per call on the
 * host, TurboEnCoding, log_map.cpp:530-583, which the compat layer keeps).  With these the chain closes on
 * the GPU: td_crc_attach -> td_encode_device -> td_rate_match -> td_modulate -> (the caller's channel) ->
 * td_demod_dematch (= td_demodulate -> td_llr_convert -> td_rate_dematch) -> td_decode_device.  They work
 * on a handle of any precision and use only its K, f1, f2, device and QPP table.
 *
 * td_encode_device: d_info [B][K] uint8 (any non-zero byte is a 1, as td_crc24_host reads them) ->
 * d_coded [B][3K+12] uint8, each 0 or 1, in the stream layout of encoderm_turbo (log_map.cpp:566-578):
 * (x, p1, p2) per info bit, then the first encoder's three tail (x, p) pairs, then the second encoder's.
 * It is the layout td_rate_match (elem_size 1) and td_modulate take.  Both constituent encoders are the
 * RSC 13/15 of encode_bit (log_map.cpp:247-269), zero start, trellis-terminated; the second one reads
 * u[pi(i)].  Asynchronous on `stream`, allocates nothing, may be captured into a hipGraph.  Pointers need
 * only byte alignment; the bytes do not depend on it.  B = 0 is a no-op.  Any K the handle allows
 * (1 .. 10000).  TD_EINVAL: a null handle or pointer, B < 0.
 */
int td_encode_device(td_handle* h, const uint8_t* d_info, int B, uint8_t* d_coded, void* stream);
/* Builds and uploads the per-position syndrome table (td_crc24_syndromes) for (K, poly): poly = the
 * generator's 24 low-order coefficients, 0x800063 gCRC24B, 0x864CFB gCRC24A (td_stop_params.crc_poly's
 * convention).  Like td_rm_set it may synchronise and allocate.  It may be called again with another poly.
 * The table is independent of the stop rules' (td_set_early_stop and its siblings): setting or clearing a
 * rule does not disturb it, nor the reverse.  A failed call leaves the previous table in place.
 * TD_EINVAL: a null handle, poly == 0, coefficients above the 24 low-order ones, K <= 24. */
int td_crc_set(td_handle* h, uint32_t poly);
/* In place: bits K-24 .. K-1 of every row of d_bits [B][K] become the CRC-24 of bits 0 .. K-25 (most
 * significant remainder bit first, each byte 0 or 1), whatever they held; bits 0 .. K-25 are only read.
 * Afterwards td_crc24_host(row, K, poly) == 0.  Asynchronous on `stream`, allocates nothing, may be
 * captured.  B = 0 is a no-op.  TD_EINVAL: a null handle or pointer, B < 0, a call before td_crc_set. */
int td_crc_attach(td_handle* h, uint8_t* d_bits, int B, void* stream);
/* d_rem[b] = td_crc24_host(row b of d_bits [B][K], K, poly): 0 = the block passes.  Launch and argument
 * rules as td_crc_attach. */
int td_crc_check(td_handle* h, const uint8_t* d_bits, int B, uint32_t* d_rem, void* stream);

/*
 * Scrambling (3GPP TS 36.211 7.2, used by 6.3.1 PDSCH and 5.3.1 PUSCH): the length-31 Gold sequence
 *   x1(n+31) = x1(n+3) ^ x1(n), x1(0) = 1, x1(1..30) = 0;
 *   x2(n+31) = x2(n+3) ^ x2(n+2) ^ x2(n+1) ^ x2(n), x2(i) = bit i of c_init, i < 31;
 *   c(n) = x1(n+1600) ^ x2(n+1600).
 * The calls take no handle and run on the current device.  They are asynchronous on `stream`, allocate nothing
 * and may be captured into a hipGraph; N = 0 or len = 0 is a no-op.  TD_EINVAL: a null pointer, N < 0, len < 0
 * or len >= 2^31, an unknown precision.  Data pointers need only element alignment; d_seq is 4-byte aligned.
 *
 * td_gold_sequence: d_cinit [N] uint32 (bit 31 ignored) -> d_seq [N][W], W = (len + 31) / 32 words: bit g of
 * row n is (d_seq[n W + (g >> 5)] >> (g & 31)) & 1 = c(g) for c_init = d_cinit[n]; bits >= len of the last
 * word are 0.  Every thread jumps to its own offset (31 x 31 GF(2) matrices, built at compile time); none walks
 * the sequence from 0.
 */
int td_gold_sequence(const uint32_t* d_cinit, int N, long long len, uint32_t* d_seq, void* stream);
/* Host only (no GPU): the same W words for one c_init. */
int td_gold_sequence_host(uint32_t cinit, long long len, uint32_t* seq);
/* d_out[n][g] = (d_in[n][g] != 0) ^ c_n(g), each byte 0 or 1; [N][len] uint8; d_out may equal d_in. */
int td_scramble(const uint8_t* d_in, const uint32_t* d_seq, int N, long long len, uint8_t* d_out, void* stream);
/* Soft values [N][len] in `precision` (TD_F64 / TD_F32 / TD_FIXED int8): where c_n(g) = 1 the value's sign is
 * flipped (IEEE negation, so 0.0 -> -0.0; int8: -128 read as -127, then negated), else copied.  In place
 * allowed. */
int td_descramble_llr(const void* d_in, int precision, const uint32_t* d_seq, int N, long long len, void* d_out,
                      void* stream);

/*
 * Transport blocks (3GPP TS 36.212 5.1.2 code block segmentation with filler bits, 5.1.4.1.2 per-block rate
 * matching sizes, 5.1.5 concatenation): the layer between a PDSCH / PUSCH transport block and the calls above,
 * which take [B][K] rows of one K.  A td_tb owns only tables and is independent of any td_handle: the decode
 * handles stay the caller's, one for K_minus and one for K_plus, created with the caller's own f1 / f2 (the LTE
 * (K, f1, f2) table is not part of this library).  Not covered: HARQ bookkeeping beyond `accumulate`, the
 * PUSCH channel interleaver, c_init from RNTI / cell / slot (the caller passes it).
 *
 * The chain, transmit: td_tb_segment -> td_encode_device (two handles) -> td_tb_rate_match -> td_scramble (with
 * td_gold_sequence's words) -> td_modulate.  Receive: td_tb_demod_dematch (symbols -> the two soft buffers,
 * descrambled, in one launch) -> td_decode_device (two handles) -> td_tb_concat; or, call by call,
 * td_demodulate -> td_descramble_llr -> td_llr_convert -> td_tb_rate_dematch, which gives the same bytes.
 *
 * Plan (5.1.2): B = A + 24 bits (the transport block and its gCRC24A), Z = 6144.  B <= Z: L = 0, C = 1,
 * B' = B; else L = 24, C = ceil(B / (Z - L)), B' = B + C L.  K_plus = the smallest code block size with
 * C K >= B' (sizes by rule: 40..512 step 8, 528..1024 step 16, 1056..2048 step 32, 2112..6144 step 64).
 * C = 1: C_plus = 1, K_minus = C_minus = 0.  Else K_minus = the next size below K_plus, C_minus =
 * floor((C K_plus - B') / (K_plus - K_minus)), C_plus = C - C_minus.  F = C_plus K_plus + C_minus K_minus - B'
 * filler bits (at most 63) open block 0.  Blocks r < C_minus have size K_minus, the others K_plus; each carries
 * K_r - L bits of the B-bit sequence in order and, when C > 1, its gCRC24B in its last 24.
 *
 * Layout, block-major: block r of transport block n is row r N + n of the K_minus array [C_minus][N][K_minus]
 * when r < C_minus, else row (r - C_minus) N + n of the K_plus array [C_plus][N][K_plus].  Each array is one
 * batch for one decode handle (td_encode_device, td_decode_device, ... with B = C_minus N or C_plus N), and
 * the rows that share the filler or an E are contiguous ranges.  The pointer of an array whose class is
 * empty (C_minus = 0) may be null.
 */
typedef struct td_tb td_tb;
typedef struct td_tb_plan {
    int A, B, L, C, K_plus, K_minus, C_plus, C_minus, F;
} td_tb_plan;
typedef struct td_tb_params {
    int A;               /* transport block size in bits, 1 .. 1048576 */
    int Ncb_cap;         /* soft buffer limit: a block's Ncb = min(Ncb_cap, its Kw); 0 = the whole buffer,
                            otherwise at least Kpi of K_plus */
    int device;
    double filler_llr;   /* what td_tb_rate_dematch writes for a filler bit: finite and <= 0 (the hard decision
                            is LLR < 0 -> 0, so a known 0 is negative) */
} td_tb_params;
/* Host only (no GPU).  TD_EINVAL: A outside 1 .. 1048576, a null pointer. */
int td_tb_plan_host(int A, td_tb_plan* out);
/* Host only.  5.1.4.1.2 with G' = G / NlQm and gamma = G' mod C: blocks r < n_lo = C - gamma send
 * E_lo = NlQm floor(G' / C) values, the others E_hi = NlQm ceil(G' / C).  Any pointer of the three may be
 * null.  TD_EINVAL: a null plan, G or NlQm < 1, G >= 2^31, G no multiple of NlQm, G' < C. */
int td_tb_rm_sizes_host(const td_tb_plan* p, long long G, int NlQm, int* E_lo, int* E_hi, int* n_lo);
/* Host only: td_rm_index_host for a block whose first F bits are filler (0 <= F <= 63, F < K): their d0 and
 * d1, stream positions 3k and 3k+1 with k < F, are <NULL> in the circular buffer and never selected; d2 stays,
 * as in the standard.  k0(rv) is unchanged; only the non-NULL count and ordinals change.  F = 0:
 * td_rm_index_host. */
int td_rm_index_host_filler(int K, int Ncb, int F, int rv, int E, int32_t* idx);
/* Builds and uploads the tables: the gCRC24A syndromes of length B, the gCRC24B syndromes of K_minus and
 * K_plus, rank / pos of every class of block (K_minus, K_plus; with the filler's <NULL>s for block 0, and
 * without).  It allocates and synchronises; after it no call does, every call is asynchronous on its stream
 * and may be captured into a hipGraph, and pointers need only element alignment.
 * TD_EINVAL: a null pointer, a bad A, Ncb_cap < 0 or 0 < Ncb_cap < Kpi(K_plus), filler_llr not finite or > 0,
 * a bad device ordinal.  TD_ENODEV: no gfx950 device. */
int td_tb_create(td_tb** out, const td_tb_params* p);
int td_tb_destroy(td_tb* t);
int td_tb_get_plan(const td_tb* t, td_tb_plan* out);
/*
 * The four device calls take N transport blocks each (N = 0 is a no-op).  TD_EINVAL -- a null td_tb, a null
 * pointer of a non-empty class, N < 0, rv outside 0..3, G or NlQm that td_tb_rm_sizes_host rejects, an unknown
 * precision -- changes nothing.
 *
 * td_tb_segment: d_tb [N][A] uint8 (any non-zero byte is a 1) -> the code blocks, every byte 0 or 1: F zeros
 * open block 0, the blocks carry the A bits and their gCRC24A in order, and when C > 1 every block ends in the
 * gCRC24B of its first K_r - 24 bits (the filler counted as zeros).  Two launches.
 */
int td_tb_segment(td_tb* t, const uint8_t* d_tb, int N, uint8_t* d_cb_minus, uint8_t* d_cb_plus, void* stream);
/* d_coded_minus / d_coded_plus [rows][3K+12] uint8 = td_encode_device of the two arrays -> d_f [N][G]: row n is
 * e_0 | e_1 | ... | e_{C-1} (5.1.5), e_r[k] = coded_r[idx_r[k]], k < E_r (td_tb_rm_sizes_host), idx_r =
 * td_rm_index_host_filler(K_r, Ncb_r, r == 0 ? F : 0, rv, E_r).  One gather, one launch. */
int td_tb_rate_match(td_tb* t, const uint8_t* d_coded_minus, const uint8_t* d_coded_plus, int N, int rv, long long G,
                     int NlQm, uint8_t* d_f, void* stream);
/* The transpose: d_f [N][G] soft values -> the blocks' soft buffers [rows][3K+12], all double (precision
 * TD_F64), float (TD_F32) or int8 (TD_FIXED), with td_rate_dematch's arithmetic per block: sums in ascending
 * k in the buffer's precision, int8 saturated to +-127 after every addition with -128 in the prior buffer read
 * as -127, an unselected position kept (accumulate) or zero, no atomics, the same bytes on every run.  In
 * block 0's rows, positions 3k and 3k+1 with k < F are always written with filler_llr as td_llr_convert
 * would give it (int8: clamp(rint(filler_llr), -127, 127)).  d_f is what td_demodulate -> td_llr_convert give
 * on the whole [N][G] array.  One launch. */
int td_tb_rate_dematch(td_tb* t, const void* d_f, int precision, int N, int rv, long long G, int NlQm, void* d_llr_minus,
                       void* d_llr_plus, int accumulate, void* stream);
/* Received symbols -> the blocks' soft buffers in one launch.  d_yi, d_yq [N][G / modulation] doubles; d_seq
 * [N][(G + 31) / 32] words of td_gold_sequence, or null for no descrambling.  The result is, byte for byte,
 * td_demodulate of all N G / modulation symbols with Kf, then (d_seq non-null) td_descramble_llr of that [N][G]
 * double array, then td_llr_convert to `precision` with steps_per_unit, then td_tb_rate_dematch with the same
 * t, precision, N, rv, G, NlQm and accumulate -- filler positions included -- without the [N][G] arrays in
 * between.  The inputs are only read.  TD_EINVAL: everything td_tb_rate_dematch rejects, a null d_yi or d_yq,
 * modulation not 1, 2, 3, 4 or 6, NlQm no multiple of modulation, and TD_FIXED with a steps_per_unit that is
 * not finite or <= 0.  Allocates nothing and may be captured. */
int td_tb_demod_dematch(td_tb* t, const double* d_yi, const double* d_yq, int precision, int N, int rv, long long G,
                        int NlQm, int modulation, double Kf, double steps_per_unit, const uint32_t* d_seq,
                        void* d_llr_minus, void* d_llr_plus, int accumulate, void* stream);
/* d_bits_minus / d_bits_plus [rows][K] uint8 = the decoders' hard decisions -> d_tb [N][A] (0 or 1), filler
 * and CRCs stripped; d_cb_rem [N][C] = td_crc24_host of block r under gCRC24B with its first F bits (r = 0)
 * taken as 0, and 0 when C = 1; d_tb_rem [N] = the gCRC24A remainder of the reassembled B bits.  Either
 * remainder pointer may be null.  One launch, two with d_tb_rem. */
int td_tb_concat(td_tb* t, const uint8_t* d_bits_minus, const uint8_t* d_bits_plus, int N, uint8_t* d_tb,
                 uint32_t* d_cb_rem, uint32_t* d_tb_rem, void* stream);

/* Last error message of this thread ("" if none). */
const char* td_last_error(void);
/* Number of visible HIP devices (0 on a host without a GPU; never fails). */
int td_device_count(void);
/* ABI version of the loaded library (TD_ABI_VERSION). */
int td_abi_version(void);

/*
 * Host evaluation of the exact bucket form of E_algorithm used on the device (no GPU needed):
 * max(x,y) + table(|y-x|) through the 29-bucket LUT the kernels read from LDS.  Lets CPU
 * tests prove LUT == log_map.cpp:779-801 for every threshold.  algo = enum td_algo, or
 * TD_MAXSTAR_WINDOW_FAST: the windowed schedule's one-read table (td_set_window_maxstar).
 */
#define TD_MAXSTAR_WINDOW_FAST 2
double td_maxstar_host_f64(double x, double y, int algo);
float td_maxstar_host_f32(float x, float y, int algo);

/* Trellis tables as built by td_create's gen_trellis restatement: nextstat[8][2],
 * laststat[8][2], nextout[8][4] (ITTC/log_map.h:58-66). For tests. */
int td_trellis_tables(int* nextstat, int* laststat, int* nextout);
/* QPP permutation exactly as gen_qpp_index (log_map.cpp:616-624). For tests. */
int td_qpp_table(int K, int f1, int f2, int* pi);

#ifdef __cplusplus
}
#endif
#endif
