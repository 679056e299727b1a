// td_api.cpp -- the C ABI of libturbo_mi355x.so (include/turbo_mi355x.h).
//
// Host side of the decoder: builds the code tables (TurboCodingInit, log_map.cpp:349-434),
// owns the device workspace, and launches the gfx950 kernels of td_kernels.hip.  There is no
// CPU fallback: every decode runs on an MI355X or fails with a status code.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "td_crc.h"
#include "td_encode.h"
#include "td_fixed.h"
#include "td_kernels.h"
#include "td_gold_core.h"
#include "td_ratematch.h"
#include "td_scramble.h"
#include "td_tb.h"

#ifndef TD_SYS2_IN_TURBO
#define TD_SYS2_IN_TURBO 1   // exact schedule: sys2 = sys1 o pi formed inside the turbo kernel (no demux_perm launch)
#endif
#ifndef TD_PLACEMENT_DEFAULT
#define TD_PLACEMENT_DEFAULT 24   // td_reserve's workspace candidates (TD_PLACEMENT_TRIALS overrides)
#endif
#include "td_tables.h"
#include "turbo_mi355x.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what)
{
    return fail(TD_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define TD_HIP(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

struct td_handle {
    td_params p{};
    td::Trellis tr{};
    td::LaneTables lane{};
    std::vector<int> pi;
    int* d_pi = nullptr;
    int* d_pinv = nullptr;
    void* d_lut = nullptr;
    void* d_qlut = nullptr;        // the windowed schedule's one-read max* table (build_qlut), handle precision
    td::LaneTables* d_lane = nullptr;
    unsigned* d_slots = nullptr;   // per-CU occupancy bits of the turbo kernel (wg_pos)
    unsigned long long* d_clk = nullptr;   // the last decode's clock sample (td_clock_read)
    bool clk_valid = false;                // the last decode was eager (a captured one leaves no sample)
    // td_decode_host's device staging (input stream, bits, optional Le), grown on demand and kept: the
    // drop-in's TurboDecoding decodes one frame per call, so per-call allocations would be per frame
    void* d_hin = nullptr;
    uint8_t* d_hbits = nullptr;
    void* d_hle = nullptr;
    size_t hin_b = 0, hbits_b = 0, hle_b = 0;
    int32_t* d_hiters = nullptr;   // td_decode_host_stop's per-codeword iteration counts
    size_t hiters_b = 0;
    std::vector<uint8_t> h_hbits;
    void* d_ws = nullptr;   // decode workspace
    std::vector<float> place_ms;   // td_reserve's placement trials (ms of one probe iteration each)
    int place_pick = -1;
    double place_wall_ms = 0, place_held = 0;   // the search's wall time and peak bytes held
    size_t ws_bytes = 0;
    size_t elem = 8;
    void* stamps = nullptr;     // td_debug_set_stamps
    bool prof = false;          // td_profile_enable
    std::vector<std::array<hipEvent_t, 3>> ev;   // one triple per profiled decode
    size_t nev = 0;
    // frame generator (td_synth_seed / td_synth_frames): glibc rand() stream state
    uint32_t lfg_win[31] = {};                   // x[n-31 .. n-1] before the next draw
    uint32_t lfg_win0[31] = {};                  // the window right after srand(seed)
    std::vector<uint32_t> lfg_jump;              // 31x31: window after K+2 draws (one frame)
    bool lfg_seeded = false;
    unsigned long long lfg_frames = 0;
    uint32_t* d_win = nullptr;
    int win_cap = 0;
    int modulation = 1;                          // td_synth_modulation (MODULATION)
    int role_cus = 0;                            // CU count for the kernel's role rotation (wg_pos)
    int occ3 = 1;                                // TD_OCC3=0: never three workgroups per CU
    // decoding schedule (td_set_window): window 0 = exact full trellis
    td::WindowParams wp{0, 0, 0, 0, 1.0, 0};
    int win_run = 0, win_run_a = 0, win_parts = 0;   // td_debug_window_layout (tests, measurements)
    int win_exact_table = 0;                         // td_set_window_maxstar
    void* d_wws = nullptr;   // windowed-schedule buffers (second extrinsic pair, NII metrics)
    size_t wws_bytes = 0;
    td::WindowStreams wstr{};                    // the windowed schedule's extra streams (batch parts)
    // Workspace ordering across streams: every decode uses the same d_ws / d_wws, so a decode
    // issued on a stream other than the previous decode's first waits (on the device) for that
    // decode to finish with the workspace.  Decodes on one handle therefore never overlap; callers
    // that want concurrent decodes use one handle per stream.
    // early termination (td_set_early_stop): rule 0 = off
    td_stop_params stop{TD_STOP_NONE, 1, 0};
    uint32_t* d_crc = nullptr;      // [K] CRC syndromes by natural bit position (td_crc.h), built by td_set_early_stop
                                    // or td_set_window_stop (a handle has a rule of one kind at most); a fixed
                                    // handle's are td_set_fixed_stop's, by interleaved position
    // early termination of the windowed schedule (td_set_window_stop): rule 0 = off
    td_stop_params wstop{TD_STOP_NONE, 1, 0};
    bool clk_stopped = false;       // the last decode ran the stopping windowed kernels (no clock sample)
    hipEvent_t ws_free = nullptr;   // recorded after the last decode's kernels
    hipStream_t ws_stream = nullptr;
    bool ws_pending = false;
    // rate matching (td_rm_set): the host tables and their device copies, allocated once for the
    // largest Ncb (3K+12 and Kw ints), so a later td_rm_set only uploads
    td::RmTables rm;
    int32_t* d_rm_rank = nullptr;
    int32_t* d_rm_pos = nullptr;
    bool rm_set = false;
    // CRC attach / check (td_crc_set): [K] syndromes by natural bit position, a table of its own -- the stop
    // rules' d_crc is theirs (a fixed handle's is in interleaved order), so neither setter disturbs the other
    uint32_t* d_crc_tab = nullptr;
    uint32_t crc_tab_poly = 0;   // 0 = td_crc_set not called yet
    // the fixed-point decoder (TD_FIXED): the extrinsic's clamp and scale (td_set_fixed)
    td_fixed_params fxp{255, 3};
    // the fixed-point decoder's correction table (td_set_fixed_maxstar): off = Max-Log-MAP
    bool fms_on = false;
    td_fixed_maxstar_params fms{};
    // early termination of the fixed-point decoder (td_set_fixed_stop): rule 0 = off; its CRC table is d_crc
    td_stop_params fstop{TD_STOP_NONE, 1, 0};
    // the fixed-point decoder's sub-block schedule (td_set_fixed_window): window 0 = the exact schedule
    td_fixed_window_params fwin{0, 0};
    // early termination of the sub-block schedule (td_set_fixed_window_stop): rule 0 = off; its CRC table is d_crc
    // (a fixed handle has a rule of one kind at most: td_set_fixed_stop's needs window 0, this one a window)
    td_stop_params fwstop{TD_STOP_NONE, 1, 0};
    // next-iteration initialisation of the sub-block schedule (td_set_fixed_window_nii): its state follows the
    // workspace's carve while it is on
    bool fnii = false;
    // td_debug_workspace_fill: the byte every fresh scratch allocation is filled with; -1 = disarmed
    int poison = -1;
};

namespace td {

bool build_lane_tables(const Trellis& t, LaneTables& lt)
{
    auto A = [](int l) { return (l & 1) ^ (((l >> 1) & 1) * 2) ^ (((l >> 2) & 1) * 7); };
    auto rotr = [](int s) { return (s >> 1) | ((s & 1) << 2); };
    const int m[3] = {1, 2, 7};   // DPP partner masks: quad_perm xor1, quad_perm xor2, row_half_mirror
    for (int ph = 0; ph < 3; ++ph)
        for (int l = 0; l < 8; ++l) {
            int s = A(l);
            for (int r = 0; r < ph; ++r) s = rotr(s);
            lt.state[ph][l] = s;
        }
    for (int ph = 0; ph < 3; ++ph) {
        const int nx = (ph + 1) % 3;
        for (int l = 0; l < 8; ++l) {
            // alpha i -> i+1: this slot computes state j (labeling nx) from its own value (ps)
            // and the partner slot's (pp), both at labeling ph
            const int j = lt.state[nx][l], ps = lt.state[ph][l], pp = lt.state[ph][l ^ m[ph]];
            const int p0 = t.laststat[j][0], p1 = t.laststat[j][1];
            if (!((ps == p0 && pp == p1) || (ps == p1 && pp == p0))) return false;
            const int us = ps == p0 ? 0 : 1;
            // parity sign o and input u select G: (u == 1) == (o == +1) -> P, else Q
            const int os = t.nextout[ps][2 * us + 1], op = t.nextout[pp][2 * (1 - us) + 1];
            lt.a_sg[ph][l] = us ? 1 : -1;
            lt.a_sel[ph][l] = ((us == 1) == (os == 1)) ? 0 : 1;
            lt.a_pg[ph][l] = us ? -1 : 1;
            lt.a_psel[ph][l] = (((1 - us) == 1) == (op == 1)) ? 0 : 1;
            lt.a_j[ph][l] = j;
            lt.a_swap[ph][l] = us;
            // beta i+1 -> i: this slot computes state jb (labeling ph) from successors at labeling nx
            const int jb = lt.state[ph][l], ns = lt.state[nx][l], np = lt.state[nx][l ^ m[ph]];
            const int n0 = t.nextstat[jb][0], n1 = t.nextstat[jb][1];
            if (!((ns == n0 && np == n1) || (ns == n1 && np == n0))) return false;
            const int ub = ns == n0 ? 0 : 1;
            const int obs = t.nextout[jb][2 * ub + 1], obp = t.nextout[jb][2 * (1 - ub) + 1];
            lt.b_sg[ph][l] = ub ? 1 : -1;
            lt.b_sel[ph][l] = ((ub == 1) == (obs == 1)) ? 0 : 1;
            lt.b_pg[ph][l] = ub ? -1 : 1;
            lt.b_psel[ph][l] = (((1 - ub) == 1) == (obp == 1)) ? 0 : 1;
        }
    }
    return true;
}

}  // namespace td

namespace {

template <typename T>
void fill_common(td::DecodeParams<T>& dp, const td_handle* h)
{
    std::memcpy(dp.nextstat, h->tr.nextstat, sizeof dp.nextstat);
    std::memcpy(dp.laststat, h->tr.laststat, sizeof dp.laststat);
    std::memcpy(dp.nextout, h->tr.nextout, sizeof dp.nextout);
    dp.lane = h->d_lane;
    dp.lut = static_cast<const td::LutEntry<T>*>(h->d_lut);
    dp.qlut = static_cast<const T*>(h->d_qlut);
    dp.algo = h->p.algo;
    dp.role_cus = h->role_cus;
    dp.occ3 = h->occ3;
    dp.cu_slots = h->d_slots;
}

// The windowed beta kernel reads each wide array in whole segments of S rows by DMA (td_kernels.hip,
// sw_beta_kernel), up to S - 1 rows past the last step of the last 64-codeword group: every wide array
// carries that much slack (S x 64 x 8 bytes at most).
constexpr size_t kWideSlack = 4096;

// Workspace carve for G groups of the handle's K.  The alpha scratch (astore) belongs to the exact
// schedule only, the tempmax stream (tmstore) to its Max-Log-MAP form only (log-MAP forms tempmax on
// chip since round 4); the windowed schedule uses neither (its buffers: win_carve).  An absent region
// has size 0 (its pointer stays inside the allocation and is never dereferenced).
struct Carve {
    size_t sys1, par1, sys2, par2, ext12, ext21, astore, tmstore, total;
};

Carve carve(int G, int K, size_t elem, int algo, bool exact)
{
    const int L = K + td::kMemory;
    // codewords: groups of 8 (exact schedule) or the windowed schedule's wide groups of 64
    const size_t ncw = exact ? (size_t)G * 8 : ((size_t)G * 8 + 63) / 64 * 64;
    const size_t slack = exact ? 0 : kWideSlack;
    const size_t arrL = align_up(ncw * L * elem + slack, 256);
    const size_t arrK = align_up(ncw * K * elem + slack, 256);
    const size_t arrA = exact ? align_up(td::astore_elems(G, L) * elem, 256) : 0;
    const size_t arrT = exact && algo == TD_ALGO_MAXLOG ? arrL : 0;
    Carve c{};
    c.sys1 = 0;
    c.par1 = c.sys1 + arrL;
    c.sys2 = c.par1 + arrL;
    c.par2 = c.sys2 + arrL;
    c.ext12 = c.par2 + arrL;
    c.ext21 = c.ext12 + arrK;
    c.astore = c.ext21 + arrK;
    c.tmstore = c.astore + arrA;
    c.total = c.tmstore + arrT;
    return c;
}
Carve carve_for(const td_handle* h, int G) { return carve(G, h->p.K, h->elem, h->p.algo, h->wp.window == 0); }

hipError_t ws_malloc(void** p, size_t size) { return hipMalloc(p, size); }
hipError_t ws_release(void* p) { return hipFree(p); }

// td_debug_workspace_fill, armed: a scratch buffer that was just allocated gets the handle's byte before
// anything is enqueued on it (the device is idle after the call: the caller's streams need not be the null
// stream).  Disarmed: nothing, one compare.
hipError_t poison_fresh(const td_handle* h, void* p, size_t size)
{
    if (h->poison < 0 || !p || !size) return hipSuccess;
    const hipError_t e = hipMemset(p, h->poison, size);
    return e != hipSuccess ? e : hipDeviceSynchronize();
}

// the workspace for G groups in the handle's current layout (grown, never shrunk)
int ensure_ws(td_handle* h, int G)
{
    const Carve c = carve_for(h, G);
    if (c.total <= h->ws_bytes) return TD_OK;
    if (h->d_ws) {
        TD_HIP(hipDeviceSynchronize());
        TD_HIP(ws_release(h->d_ws));
        h->d_ws = nullptr;
        h->ws_bytes = 0;
    }
    if (ws_malloc(&h->d_ws, c.total) != hipSuccess) {
        h->d_ws = nullptr;
        return fail(TD_ENOMEM, "hipMalloc of the decode workspace failed (" + std::to_string(c.total) + " B)");
    }
    h->ws_bytes = c.total;
    TD_HIP(poison_fresh(h, h->d_ws, h->ws_bytes));
    return TD_OK;
}

// Workspace placement (td_reserve, exact schedule).  The turbo kernel's speed depends on the
// physical pages behind its workspace: on MI355X, decoders with fresh workspaces of the same size
// ran in two modes 6-7 % apart (config 2: 17.3 vs 18.5 ms a launch), fixed for the life of the
// allocation and unchanged by shifting the carve inside it by 4 KiB .. 128 MiB
// (scripts/spread_probe.py, scripts/ws_offset_probe.py); a physically contiguous allocation
// (hipDeviceMallocContiguous) always landed in the slow mode.  td_reserve therefore allocates
// candidates, all held until the choice (so each one gets fresh pages), times one turbo iteration
// on each (best of two launches; zeroed workspace, results discarded; 2.20 vs 2.32 ms in the two modes at config 2) and
// keeps the fastest.  It stops once the fast mode has been seen (placement_fast_seen below), at
// TD_PLACEMENT_TRIALS candidates (environment, default 24; 1 = a plain allocation), holding at most
// kPlaceLive of them at a time (below).  Results never depend on the placement.
template <typename T>
float probe_ws(const td_handle* h, char* ws, int G, hipStream_t st, hipEvent_t e0, hipEvent_t e1, int warm)
{
    const Carve c = carve(G, h->p.K, sizeof(T), h->p.algo, true);
    td::DecodeParams<T> dp{};
    fill_common(dp, h);
    dp.sys1 = reinterpret_cast<T*>(ws + c.sys1);
    dp.par1 = reinterpret_cast<T*>(ws + c.par1);
    dp.sys2 = reinterpret_cast<T*>(ws + c.sys2);
    dp.par2 = reinterpret_cast<T*>(ws + c.par2);
    dp.ext12 = reinterpret_cast<T*>(ws + c.ext12);
    dp.ext21 = reinterpret_cast<T*>(ws + c.ext21);
    dp.astore = reinterpret_cast<T*>(ws + c.astore);
    dp.tmstore = reinterpret_cast<T*>(ws + c.tmstore);
    dp.pi = h->d_pi;
    dp.pinv = h->d_pinv;
    dp.K = h->p.K;
    dp.L = h->p.K + td::kMemory;
    dp.nT = (dp.L + td::window_steps() - 1) / td::window_steps();
    dp.G = G;
    dp.B = 8 * G;
    dp.iters = 1;
    dp.sys2_in_turbo = TD_SYS2_IN_TURBO;
    if (hipMemsetAsync(ws, 0, c.total, st) != hipSuccess) return -1.f;
    // untimed launches first (the first probe of a process also brings the clocks up), then the
    // best of two timed ones
    for (int w = 0; w < warm; ++w)
        if (td::launch_turbo<T>(dp, st, true) != hipSuccess) return -1.f;
    float best = -1.f;
    for (int r = 0; r < 2; ++r) {
        float ms = -1.f;
        if (hipEventRecord(e0, st) != hipSuccess || td::launch_turbo<T>(dp, st, true) != hipSuccess ||
            hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
            hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
            return -1.f;
        best = best < 0 ? ms : std::min(best, ms);
    }
    return best;
}

// Stop rule of the placement search: the fast mode has been seen once (a) some candidate runs >= 4 %
// below the median of all candidates probed so far (at least three, so that the median is a mode and
// not an average of the two), or (b) at least three candidates run >= 4 % slower than the best one
// (the slow mode confirmed three times, so the best is not merely the fast side of one straggler).
// A slow straggler never stops the search: with every candidate in the slow mode the median is
// slow too and nothing is 4 % below it.  (Until round 3 the rule was "two candidates differ by
// 4 %", which an upward outlier among slow candidates satisfied.)  Neither rule is tried before
// kPlaceMin candidates: some boxes show three levels (e.g. 2.23 / 2.28-2.30 / 2.38-2.41 ms probes;
// decodes 17.5 / 17.8-18.2 / 18.5 ms, in probe order), and a middle-level candidate is already 4 %
// below a slow median; with eight probed, the fastest level is almost always among them.
#ifndef TD_PLACEMENT_MIN
#define TD_PLACEMENT_MIN 8
#endif
int placement_min()
{
    int m = TD_PLACEMENT_MIN;
    if (const char* e = std::getenv("TD_PLACEMENT_MIN")) m = std::atoi(e);
    return std::max(m, 3);
}
bool placement_fast_seen(const std::vector<float>& ms)
{
    std::vector<float> v;
    for (float x : ms)
        if (x > 0 && x < 1e29f) v.push_back(x);
    if ((int)v.size() < placement_min()) return false;
    std::sort(v.begin(), v.end());
    const float med = v.size() % 2 ? v[v.size() / 2] : 0.5f * (v[v.size() / 2 - 1] + v[v.size() / 2]);
    if (v.front() < 0.96f * med) return true;
    int slower = 0;
    for (float x : v) slower += x >= 1.04f * v.front();
    return slower >= 3;
}

// What the search may hold at once (round 6, VERDICT round 5: rounds 3-5 held every candidate until
// the choice, up to 64 GiB at config 2 for a 2.6 GB workspace).  At most kPlaceLive candidates are
// live: once that many are held and the fast mode has not been seen, the slowest is released before
// the next is allocated, and a spacer of kPlaceSpacerBytes is taken first so that the next candidate
// does not get the released pages back in the same order.  Peak hold: kPlaceLive workspaces plus the
// spacers (< 0.5 workspace at config 2), at most half the free device memory.  The kept candidate is
// always live (only the slowest is released).  The search's wall time and peak bytes held are
// recorded (td_debug_placement_cost).
#ifndef TD_PLACE_LIVE
#define TD_PLACE_LIVE 3
#endif
#ifndef TD_PLACE_SPACER_MIB
#define TD_PLACE_SPACER_MIB 48
#endif
constexpr int kPlaceLive = TD_PLACE_LIVE;
constexpr size_t kPlaceSpacerBytes = (size_t)TD_PLACE_SPACER_MIB << 20;

int place_ws(td_handle* h, int G)
{
    int trials = TD_PLACEMENT_DEFAULT;
    if (const char* e = std::getenv("TD_PLACEMENT_TRIALS")) trials = std::atoi(e);
    const Carve c = carve_for(h, G);
    // a workspace that is big enough is kept as it is, placed or not (a reserve
    // after a decode that grew it must not free it and search again)
    if (h->d_ws && c.total <= h->ws_bytes) return TD_OK;
    if (trials <= 1 || h->wp.window || 8 * G < 1024) return ensure_ws(h, G);
    if (h->d_ws) {
        TD_HIP(hipDeviceSynchronize());
        TD_HIP(ws_release(h->d_ws));
        h->d_ws = nullptr;
        h->ws_bytes = 0;
    }
    // every HIP object of the search is released on every exit path, error returns included
    struct Search {
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        std::vector<std::pair<float, void*>> cand;   // live candidates
        std::vector<void*> spacers;
        ~Search()
        {
            if (st) (void)hipStreamSynchronize(st);
            for (auto& x : cand)
                if (x.second) (void)ws_release(x.second);
            for (void* p : spacers) (void)hipFree(p);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (st) (void)hipStreamDestroy(st);
        }
    } s;
    const auto t_start = std::chrono::steady_clock::now();
    TD_HIP(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
    TD_HIP(hipEventCreate(&s.e0));
    TD_HIP(hipEventCreate(&s.e1));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const size_t live_max = std::max<size_t>(1, std::min<size_t>(kPlaceLive, free_b / 2 / std::max<size_t>(c.total, 1)));
    std::vector<float> ms_all;
    size_t held = 0, peak = 0;
    for (int i = 0; i < trials; ++i) {
        if (s.cand.size() >= live_max) {
            if (live_max < 2) break;   // no room to compare
            size_t worst = 0;
            for (size_t k = 1; k < s.cand.size(); ++k)
                if (s.cand[k].first > s.cand[worst].first) worst = k;
            TD_HIP(hipStreamSynchronize(s.st));
            (void)ws_release(s.cand[worst].second);
            s.cand.erase(s.cand.begin() + (long)worst);
            held -= c.total;
            void* sp = nullptr;
            if (kPlaceSpacerBytes && hipMalloc(&sp, kPlaceSpacerBytes) == hipSuccess) {
                s.spacers.push_back(sp);
                held += kPlaceSpacerBytes;
            }
        }
        void* p = nullptr;
        if (ws_malloc(&p, c.total) != hipSuccess) break;   // out of memory: choose among those we have
        held += c.total;
        peak = std::max(peak, held);
        s.cand.emplace_back(1e30f, p);
        // the first candidate also brings the clocks up: with 4 untimed launches its probe still read
        // 3-6 % slow (2.11, then 2.06 / 2.06 ms against 1.96-2.03 for the rest; round 6), so a fast
        // early candidate looked slow and was the first released; 24 launches (~50 ms at config 2) settle them
        const int warm = i == 0 ? 24 : 1;
        const float ms = h->elem == 8 ? probe_ws<double>(h, static_cast<char*>(p), G, s.st, s.e0, s.e1, warm)
                                      : probe_ws<float>(h, static_cast<char*>(p), G, s.st, s.e0, s.e1, warm);
        s.cand.back().first = ms < 0 ? 1e30f : ms;
        ms_all.push_back(s.cand.back().first);
        if (placement_fast_seen(ms_all)) break;
    }
    (void)hipGetLastError();
    if (s.cand.empty()) return ensure_ws(h, G);
    size_t best = 0;
    for (size_t i = 1; i < s.cand.size(); ++i)
        if (s.cand[i].first < s.cand[best].first) best = i;
    h->place_ms = ms_all;
    h->place_pick = -1;   // index into ms_all of the kept candidate
    for (size_t i = 0; i < ms_all.size(); ++i)
        if (ms_all[i] == s.cand[best].first) {
            h->place_pick = (int)i;
            break;
        }
    h->place_held = (double)peak;
    h->place_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    h->d_ws = s.cand[best].second;
    s.cand[best].second = nullptr;   // kept; the guard frees the others and the spacers
    h->ws_bytes = c.total;
    TD_HIP(poison_fresh(h, h->d_ws, h->ws_bytes));
    return TD_OK;
}

int groups_for(int B) { return (B + 7) / 8; }   // groups of 8 codewords, one workgroup each

// the windowed schedule's buffers: the workspace's extrinsic pair plus a second pair (concurrent
// schedule), the alpha checkpoints of each decoder and the NII metrics [2 parity][2 dec][B][nS][2][8],
// grown on demand
struct WinCarve {
    size_t arrK, arrC, nii, arrT, arrS, total;
};
WinCarve win_carve(const td_handle* h, int B)
{
    const size_t elem = h->elem;
    const int K = h->p.K, L = K + td::kMemory, G = groups_for(B);
    WinCarve c{};
    c.arrK = align_up(((size_t)B + 63) / 64 * 64 * K * elem + kWideSlack, 256);   // wide groups of 64 codewords
    c.nii = (size_t)2 * 2 * (((size_t)B + 63) / 64 * 64) * td::window_subblocks(L, h->wp.window) * 16 * elem;
    c.arrC = align_up(td::window_ckpt_elems(B, L, h->wp.window, elem == 4) * elem, 256);
    c.nii = align_up(c.nii, 256);
    c.arrT = align_up(td::window_bits_bytes(B, K), 256);
    c.arrS = align_up(td::window_stop_bytes(B), 256);   // early termination: stop_at, evidence (always carved)
    c.total = 2 * c.arrK + 2 * c.arrC + c.nii + c.arrT + c.arrS;
    return c;
}

// grow the windowed-schedule buffers to `need` bytes (never inside a decode that is being
// captured: td_reserve sizes them for the handle's window settings beforehand)
int ensure_wws(td_handle* h, size_t need)
{
    if (need > h->wws_bytes) {
        if (h->d_wws) {
            TD_HIP(hipDeviceSynchronize());
            TD_HIP(hipFree(h->d_wws));
            h->d_wws = nullptr;
            h->wws_bytes = 0;
        }
        if (hipMalloc(&h->d_wws, need) != hipSuccess) {
            h->d_wws = nullptr;
            return fail(TD_ENOMEM, "hipMalloc of the windowed-schedule buffers failed (" + std::to_string(need) + " B)");
        }
        h->wws_bytes = need;
        TD_HIP(poison_fresh(h, h->d_wws, need));
    }
    return TD_OK;
}

template <typename T>
int window_bufs(td_handle* h, const td::DecodeParams<T>& dp, td::WindowBufs<T>& wb)
{
    const WinCarve c = win_carve(h, dp.B);
    const size_t arrK = c.arrK, arrC = c.arrC;
    const int rc = ensure_wws(h, c.total);
    if (rc) return rc;
    char* w = static_cast<char*>(h->d_wws);
    wb.ext12[0] = dp.ext12;
    wb.ext21[0] = dp.ext21;
    wb.ext12[1] = reinterpret_cast<T*>(w);
    wb.ext21[1] = reinterpret_cast<T*>(w + arrK);
    wb.ckpt[0] = reinterpret_cast<T*>(w + 2 * arrK);
    wb.ckpt[1] = reinterpret_cast<T*>(w + 2 * arrK + arrC);   // the concurrent SISOs run together
    wb.nii = reinterpret_cast<T*>(w + 2 * arrK + 2 * arrC);
    wb.bitsT = reinterpret_cast<uint8_t*>(w + 2 * arrK + 2 * arrC + c.nii);
    wb.stop_at = reinterpret_cast<int*>(w + 2 * arrK + 2 * arrC + c.nii + c.arrT);
    wb.stop_ev = reinterpret_cast<unsigned*>(wb.stop_at) + ((size_t)dp.B + 63) / 64 * 64;
    return TD_OK;
}

// The windowed schedule's extra streams and their fork / join events (its batch parts 1..; part 0
// runs on the caller's stream), made by td_set_window on the handle's device -- never inside a
// decode, which may be under stream capture.  All or nothing: a failure releases
// whatever was made and leaves the handle without them.
void release_wstr(td::WindowStreams& w)
{
    for (int i = 1; i < td::kSwMaxParts; ++i) {
        if (w.st[i]) (void)hipStreamDestroy(w.st[i]);
        if (w.fork[i]) (void)hipEventDestroy(w.fork[i]);
        if (w.join[i]) (void)hipEventDestroy(w.join[i]);
    }
    w = td::WindowStreams{};
}

int ensure_wstr(td_handle* h)
{
    if (h->wstr.st[1]) return TD_OK;
    td::WindowStreams w{};
    hipError_t e = hipSuccess;
    for (int i = 1; i < td::kSwMaxParts && e == hipSuccess; ++i) {
        e = hipStreamCreateWithFlags(&w.st[i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&w.fork[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&w.join[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        release_wstr(w);
        return hip_fail(e, "td_set_window: stream / event creation");
    }
    h->wstr = w;
    return TD_OK;
}

template <typename T>
int decode_device_t(td_handle* h, const void* d_llr, int B, uint8_t* d_bits, int all_iters, void* d_le,
                    int32_t* d_iters, hipStream_t st)
{
    const int G = groups_for(B);
    int rc = ensure_ws(h, G);
    if (rc) return rc;
    const Carve c = carve_for(h, G);
    char* ws = static_cast<char*>(h->d_ws);
    td::DecodeParams<T> dp{};
    fill_common(dp, h);
    dp.sys1 = reinterpret_cast<T*>(ws + c.sys1);
    dp.par1 = reinterpret_cast<T*>(ws + c.par1);
    dp.sys2 = reinterpret_cast<T*>(ws + c.sys2);
    dp.par2 = reinterpret_cast<T*>(ws + c.par2);
    dp.ext12 = reinterpret_cast<T*>(ws + c.ext12);
    dp.ext21 = reinterpret_cast<T*>(ws + c.ext21);
    dp.astore = reinterpret_cast<T*>(ws + c.astore);
    dp.tmstore = reinterpret_cast<T*>(ws + c.tmstore);
    dp.llr_out = nullptr;
    dp.pi = h->d_pi;
    dp.pinv = h->d_pinv;
    dp.bits = d_bits;
    dp.le_dump = static_cast<T*>(d_le);
    dp.stamps = static_cast<unsigned long long*>(h->stamps);
    dp.clk = h->d_clk;
    dp.K = h->p.K;
    dp.L = h->p.K + td::kMemory;
    dp.nT = (dp.L + td::window_steps() - 1) / td::window_steps();
    dp.G = G;
    dp.B = B;
    dp.iters = h->p.iterations;
    dp.all_iters = all_iters ? 1 : 0;
    dp.sys2_in_turbo = (TD_SYS2_IN_TURBO && !h->wp.window) ? 1 : 0;
    td::WindowBufs<T> wb{};
    if (h->wp.window) {   // sized before anything is enqueued (a growth synchronises the device)
        if (!h->wstr.st[1]) return fail(TD_EINVAL, "td_decode_device: the windowed schedule's streams are missing");
        rc = window_bufs<T>(h, dp, wb);
        if (rc) return rc;
    }
    // A decode captured into a hipGraph neither waits on nor records the workspace event: an event
    // recorded outside the capture would break its isolation, and one recorded inside it could not
    // be waited on by a later eager decode.  Replays are therefore not ordered against eager
    // decodes on the same handle (the caller orders them, e.g. on one stream).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    TD_HIP(hipStreamIsCapturing(st, &cap));
    const bool capturing = cap != hipStreamCaptureStatusNone;
    if (!capturing) {
        if (!h->ws_free) TD_HIP(hipEventCreateWithFlags(&h->ws_free, hipEventDisableTiming));
        if (h->ws_pending && st != h->ws_stream) TD_HIP(hipStreamWaitEvent(st, h->ws_free, 0));
    }
    hipEvent_t* ev = nullptr;
    if (h->prof && !capturing) {
        if (h->nev == h->ev.size()) {
            std::array<hipEvent_t, 3> tri{};
            for (auto& x : tri) TD_HIP(hipEventCreate(&x));
            h->ev.push_back(tri);
        }
        ev = h->ev[h->nev].data();   // claimed (nev advanced) only once all three are recorded
        TD_HIP(hipEventRecord(ev[0], st));
    }
    hipError_t e = h->wp.window ? td::launch_window_demux<T>(dp, static_cast<const T*>(d_llr), st)
                                : td::launch_demux<T>(dp, static_cast<const T*>(d_llr), st);
    if (e != hipSuccess) return hip_fail(e, "launch_demux");
    if (ev) TD_HIP(hipEventRecord(ev[1], st));
    const bool wstop = h->wp.window && h->wstop.rule != TD_STOP_NONE;
    if (wstop) {
        const td::StopParams sp{h->wstop.rule, h->wstop.min_iters, h->d_crc, d_iters};
        e = td::launch_window<T>(dp, h->wp, wb, st, h->wstr, &sp);
    } else if (h->wp.window) {
        e = td::launch_window<T>(dp, h->wp, wb, st, h->wstr);   // streams made by td_set_window
    } else if (h->stop.rule != TD_STOP_NONE) {
        const td::StopParams sp{h->stop.rule, h->stop.min_iters, h->d_crc, d_iters};
        e = td::launch_turbo<T>(dp, st, false, &sp);
    } else {
        e = td::launch_turbo<T>(dp, st);
    }
    // no rule of either kind (td_set_early_stop, td_set_window_stop): every codeword took them all
    if (e == hipSuccess && d_iters && h->stop.rule == TD_STOP_NONE && !wstop)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_iters), h->p.iterations, (size_t)B, st);
    if (e != hipSuccess) return hip_fail(e, h->wp.window ? "launch_window" : "launch_turbo");
    h->clk_valid = !capturing;
    h->clk_stopped = wstop;
    if (ev) {
        TD_HIP(hipEventRecord(ev[2], st));
        ++h->nev;
    }
    if (!capturing) {
        TD_HIP(hipEventRecord(h->ws_free, st));
        h->ws_stream = st;
        h->ws_pending = true;
    }
    return TD_OK;
}

bool is_fixed(const td_handle* h) { return h->p.precision == TD_FIXED; }

int not_fixed(const td_handle* h, const char* who)
{
    if (!is_fixed(h)) return TD_OK;
    return fail(TD_EINVAL, std::string(who) + ": not available on a fixed-point handle (TD_FIXED)");
}

// the fixed-point decoder's workspace for B codewords: a plain allocation, grown and never shrunk
int ensure_fixed_ws(td_handle* h, int B)
{
    td::FxCarve c = td::fx_carve(B, h->p.K, h->p.iterations);
    if (h->fnii) c.total += td::fx_nii_bytes(B, h->p.K, h->fwin.window);   // sized for the current window's sub-blocks
    if (c.total <= h->ws_bytes) return TD_OK;
    if (h->d_ws) {
        TD_HIP(hipDeviceSynchronize());
        TD_HIP(ws_release(h->d_ws));
        h->d_ws = nullptr;
        h->ws_bytes = 0;
    }
    if (ws_malloc(&h->d_ws, c.total) != hipSuccess) {
        h->d_ws = nullptr;
        return fail(TD_ENOMEM, "hipMalloc of the decode workspace failed (" + std::to_string(c.total) + " B)");
    }
    h->ws_bytes = c.total;
    TD_HIP(poison_fresh(h, h->d_ws, h->ws_bytes));
    return TD_OK;
}

// td_decode_device on a TD_FIXED handle: the workspace event and profiling protocol of decode_device_t
int decode_fixed(td_handle* h, const void* d_llr, int B, uint8_t* d_bits, int all_iters, void* d_le, int32_t* d_iters,
                 hipStream_t st)
{
    if (!td::launch_fixed_demux || !td::launch_fixed_decode)
        return fail(TD_EHIP, "td_decode_device: this build has no td_fixed.hip");
    int rc = ensure_fixed_ws(h, B);
    if (rc) return rc;
    const td::FxCarve c = td::fx_carve(B, h->p.K, h->p.iterations);
    char* ws = static_cast<char*>(h->d_ws);
    td::fx::FxArgs a{};
    a.xs = reinterpret_cast<int8_t*>(ws + c.xs);
    a.xp1 = reinterpret_cast<int8_t*>(ws + c.xp1);
    a.xp2 = reinterpret_cast<int8_t*>(ws + c.xp2);
    a.ext12 = reinterpret_cast<int16_t*>(ws + c.ext12);
    a.ext21 = reinterpret_cast<int16_t*>(ws + c.ext21);
    a.ckpt = reinterpret_cast<int32_t*>(ws + c.ckpt);
    a.bitsT = reinterpret_cast<uint8_t*>(ws + c.bitsT);
    a.le = static_cast<int16_t*>(d_le);
    a.pi = h->d_pi;
    a.pinv = h->d_pinv;
    a.K = h->p.K;
    a.L = h->p.K + td::kMemory;
    a.B = B;
    a.iters = h->p.iterations;
    a.all_iters = all_iters ? 1 : 0;
    a.le_max = h->fxp.le_max;
    a.scale_q = h->fxp.ext_scale_q;
    a.Bp = c.Bp;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    TD_HIP(hipStreamIsCapturing(st, &cap));
    const bool capturing = cap != hipStreamCaptureStatusNone;
    if (!capturing) {
        if (!h->ws_free) TD_HIP(hipEventCreateWithFlags(&h->ws_free, hipEventDisableTiming));
        if (h->ws_pending && st != h->ws_stream) TD_HIP(hipStreamWaitEvent(st, h->ws_free, 0));
    }
    hipEvent_t* ev = nullptr;
    if (h->prof && !capturing) {
        if (h->nev == h->ev.size()) {
            std::array<hipEvent_t, 3> tri{};
            for (auto& x : tri) TD_HIP(hipEventCreate(&x));
            h->ev.push_back(tri);
        }
        ev = h->ev[h->nev].data();
        TD_HIP(hipEventRecord(ev[0], st));
    }
    // the table travels as kernel arguments: nothing on the device to allocate or to copy
    td::fx::MaxStar ms{};
    if (h->fms_on) {
        for (int j = 0; j < 4; ++j) {
            ms.lo |= (uint32_t)h->fms.corr[j] << (8 * j);
            ms.hi |= (uint32_t)h->fms.corr[4 + j] << (8 * j);
        }
        ms.shift = h->fms.shift;
    }
    const td::fx::MaxStar* m = h->fms_on ? &ms : nullptr;
    uint32_t* d_nii = h->fnii ? reinterpret_cast<uint32_t*>(ws + c.total) : nullptr;   // ensure_fixed_ws sized it
    hipError_t e = td::launch_fixed_demux(a, static_cast<const int8_t*>(d_llr), st);
    if (e != hipSuccess) return hip_fail(e, "launch_fixed_demux");
    if (ev) TD_HIP(hipEventRecord(ev[1], st));
    // the schedule's rule: a fixed handle has one of the two at most (td_set_fixed_stop needs window 0)
    const td_stop_params& rule = h->fwin.window ? h->fwstop : h->fstop;
    const bool hda = rule.rule == TD_STOP_HDA;
    td::fx::FxStop s{};
    s.rule = rule.rule;
    s.first = std::max(hda ? 2 : 1, rule.min_iters);
    s.syn = hda ? nullptr : reinterpret_cast<const int*>(h->d_crc);
    s.used = reinterpret_cast<int32_t*>(ws + c.used);
    const td::fx::FxWindow w{h->fwin.window, h->fwin.overlap};
    const bool stops = rule.rule != TD_STOP_NONE;
    e = td::launch_fixed_decode(a, w.window ? &w : nullptr, stops ? &s : nullptr, m, reinterpret_cast<uint32_t*>(ws + c.ev),
                                reinterpret_cast<uint16_t*>(ws + c.hist), d_nii, d_bits, d_iters, st);
    if (e == hipSuccess && !stops && d_iters)   // no rule: every codeword takes them all
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_iters), h->p.iterations, (size_t)B, st);
    if (e != hipSuccess) return hip_fail(e, "launch_fixed_turbo");
    h->clk_valid = false;
    if (ev) {
        TD_HIP(hipEventRecord(ev[2], st));
        ++h->nev;
    }
    if (!capturing) {
        TD_HIP(hipEventRecord(h->ws_free, st));
        h->ws_stream = st;
        h->ws_pending = true;
    }
    return TD_OK;
}

template <typename T>
int siso_host_t(td_handle* h, const void* recs, const void* La, int terminated, void* LLR, int L, int B)
{
    const int G = groups_for(B);
    const int W = td::window_steps();
    const int nT = (L + W - 1) / W;
    const size_t eL = (size_t)G * L * 8 * sizeof(T);
    const size_t eA = td::astore_elems(G, L) * sizeof(T);
    const size_t inR = (size_t)B * 2 * L * sizeof(T), inA = (size_t)B * L * sizeof(T);
    char* buf = nullptr;
    // zero permutation tables (the bare SISO writes no extrinsic), with the loader's spare ints
    const size_t eP = ((size_t)L + td::kPermPad) * sizeof(int);
    const size_t total = 5 * align_up(eL, 256) + align_up(eA, 256) + align_up(inR, 256) + 2 * align_up(inA, 256) +
                         align_up(eP, 256);
    if (hipMalloc(&buf, total) != hipSuccess) return fail(TD_ENOMEM, "hipMalloc (siso) failed");
    if (poison_fresh(h, buf, total) != hipSuccess) {
        (void)hipFree(buf);
        return fail(TD_EHIP, "td_siso_host: the debug fill of its scratch failed");
    }
    size_t o = 0;
    auto take = [&](size_t n) {
        char* p = buf + o;
        o += align_up(n, 256);
        return p;
    };
    td::DecodeParams<T> dp{};
    fill_common(dp, h);
    dp.sys1 = reinterpret_cast<T*>(take(eL));
    dp.par1 = reinterpret_cast<T*>(take(eL));
    T* la_ws = reinterpret_cast<T*>(take(eL));
    dp.llr_out = reinterpret_cast<T*>(take(eL));
    dp.astore = reinterpret_cast<T*>(take(eA));
    dp.tmstore = reinterpret_cast<T*>(take(eL));
    T* d_recs = reinterpret_cast<T*>(take(inR));
    T* d_la = reinterpret_cast<T*>(take(inA));
    T* d_llr = reinterpret_cast<T*>(take(inA));
    int* d_zero_perm = reinterpret_cast<int*>(take(eP));
    dp.pi = d_zero_perm;
    dp.pinv = d_zero_perm;
    dp.K = L - td::kMemory;
    dp.L = L;
    dp.nT = nT;
    dp.G = G;
    dp.B = B;
    dp.iters = 1;
    int rc = TD_OK;
    hipError_t e = hipMemset(d_zero_perm, 0, eP);
    if (e == hipSuccess) e = hipMemcpy(d_recs, recs, inR, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_la, La, inA, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = td::launch_siso<T>(dp, d_recs, d_la, la_ws, terminated, d_llr, nullptr);
    if (e == hipSuccess) e = hipMemcpy(LLR, d_llr, inA, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = hip_fail(e, "siso");
    (void)hipFree(buf);
    return rc;
}


// ---- glibc rand() stream (srandom_r / random_r, TYPE_3: degree 31, separation 3) as the
// window of the recurrence x[n] = x[n-31] + x[n-3] (mod 2^32), rand() = x[n] >> 1.
void glibc_window(unsigned seed, uint32_t* win)
{
    int32_t tbl[31];
    if (seed == 0) seed = 1;
    tbl[0] = (int32_t)seed;
    long word = (long)seed;
    for (int i = 1; i < 31; ++i) {   // srandom_r: 16807 * x mod (2^31 - 1), Schrage's method
        const long hi = word / 127773, lo = word % 127773;
        word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        tbl[i] = (int32_t)word;
    }
    int f = 3, b = 0;
    for (int k = 0; k < 310; ++k) {   // srandom_r discards 10 * 31 outputs
        tbl[f] = (int32_t)((uint32_t)tbl[f] + (uint32_t)tbl[b]);
        f = (f + 1) % 31;
        b = (b + 1) % 31;
    }
    for (int j = 0; j < 31; ++j) win[j] = (uint32_t)tbl[(f + j) % 31];   // tbl[f] = x[n-31]
}

// M = A^e where A advances the window by one draw (mod 2^32 arithmetic wraps in uint32_t)
std::vector<uint32_t> lfg_power(unsigned long long e)
{
    auto mul = [](const std::vector<uint32_t>& X, const std::vector<uint32_t>& Y) {
        std::vector<uint32_t> Z(31 * 31, 0);
        for (int i = 0; i < 31; ++i)
            for (int k = 0; k < 31; ++k) {
                const uint32_t x = X[i * 31 + k];
                if (!x) continue;
                for (int j = 0; j < 31; ++j) Z[i * 31 + j] += x * Y[k * 31 + j];
            }
        return Z;
    };
    std::vector<uint32_t> A(31 * 31, 0), R(31 * 31, 0);
    for (int j = 0; j < 30; ++j) A[j * 31 + j + 1] = 1;   // W'[j] = W[j+1]
    A[30 * 31 + 0] = 1;                                    // W'[30] = W[0] + W[28]
    A[30 * 31 + 28] = 1;
    for (int i = 0; i < 31; ++i) R[i * 31 + i] = 1;
    while (e) {
        if (e & 1) R = mul(R, A);
        A = mul(A, A);
        e >>= 1;
    }
    return R;
}

void lfg_apply(const std::vector<uint32_t>& M, const uint32_t* w, uint32_t* out)
{
    for (int i = 0; i < 31; ++i) {
        uint32_t acc = 0;
        for (int k = 0; k < 31; ++k) acc += M[i * 31 + k] * w[k];
        out[i] = acc;
    }
}

}  // namespace

extern "C" {

const char* td_last_error(void) { return g_err.c_str(); }

int td_abi_version(void) { return TD_ABI_VERSION; }

int td_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int td_trellis_tables(int* nextstat, int* laststat, int* nextout)
{
    td::Trellis t;
    if (!td::build_trellis(13, 15, t)) return fail(TD_EINVAL, "bad generator");
    if (nextstat) std::memcpy(nextstat, t.nextstat, sizeof t.nextstat);
    if (laststat) std::memcpy(laststat, t.laststat, sizeof t.laststat);
    if (nextout) std::memcpy(nextout, t.nextout, sizeof t.nextout);
    return TD_OK;
}

int td_qpp_table(int K, int f1, int f2, int* pi)
{
    if (K < 1 || K > 10000 || !pi) return fail(TD_EINVAL, "td_qpp_table: K out of range");
    td::build_qpp(K, f1, f2, pi);
    return TD_OK;
}

double td_maxstar_host_f64(double x, double y, int algo)
{
    static td::LutEntry<double> lut[td::kLutSize];
    static double q[td::kQRows];
    static bool init = (td::build_lut<double>(lut), td::build_qlut<double>(q), true);
    (void)init;
    if (algo == TD_ALGO_MAXLOG) return x > y ? x : y;
    if (algo == TD_MAXSTAR_WINDOW_FAST) return td::maxstar_qlut_host<double>(x, y, q);
    return td::maxstar_lut_host<double>(x, y, lut);
}

float td_maxstar_host_f32(float x, float y, int algo)
{
    static td::LutEntry<float> lut[td::kLutSize];
    static float q[td::kQRows];
    static bool init = (td::build_lut<float>(lut), td::build_qlut<float>(q), true);
    (void)init;
    if (algo == TD_ALGO_MAXLOG) return x > y ? x : y;
    if (algo == TD_MAXSTAR_WINDOW_FAST) return td::maxstar_qlut_host<float>(x, y, q);
    return td::maxstar_lut_host<float>(x, y, lut);
}

int td_create(td_handle** out, const td_params* p)
{
    if (!out || !p) return fail(TD_EINVAL, "td_create: null argument");
    *out = nullptr;
    if (p->K < 1 || p->K > 10000) return fail(TD_EINVAL, "td_create: K must be in [1, 10000] (MAX_FRAME_LENGTH)");
    if (p->iterations < 1 || p->iterations > 64) return fail(TD_EINVAL, "td_create: iterations must be in [1, 64]");
    if (p->algo != TD_ALGO_LOGMAP && p->algo != TD_ALGO_MAXLOG) return fail(TD_EINVAL, "td_create: bad algo");
    if (p->precision != TD_F64 && p->precision != TD_F32 && p->precision != TD_FIXED)
        return fail(TD_EINVAL, "td_create: bad precision");
    if (p->precision == TD_FIXED && p->algo != TD_ALGO_MAXLOG)
        return fail(TD_EINVAL, "td_create: TD_FIXED decodes with TD_ALGO_MAXLOG only");
    if (p->precision == TD_FIXED && p->K < 8) return fail(TD_EINVAL, "td_create: TD_FIXED needs K >= 8");
    // the QPP table must be a permutation (gen_qpp_index does not check; a bad f1/f2 silently
    // breaks the reference -- here it is an error)
    std::vector<int> pi(p->K);
    td::build_qpp(p->K, p->f1, p->f2, pi.data());
    {
        std::vector<char> seen(p->K, 0);
        for (int v : pi) {
            if (v < 0 || v >= p->K || seen[v]) return fail(TD_EINVAL, "td_create: f1/f2 do not give a QPP permutation of K");
            seen[v] = 1;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(TD_ENODEV, "td_create: no HIP device visible");
    if (p->device < 0 || p->device >= ndev) return fail(TD_EINVAL, "td_create: device ordinal out of range");
    hipDeviceProp_t prop;
    TD_HIP(hipGetDeviceProperties(&prop, p->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(TD_ENODEV, std::string("td_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    TD_HIP(hipSetDevice(p->device));

    td_handle* h = new td_handle();
    h->p = *p;
    h->elem = p->precision == TD_F64 ? sizeof(double) : p->precision == TD_F32 ? sizeof(float) : sizeof(int8_t);
    {
        h->role_cus = prop.multiProcessorCount;
        const char* o3 = std::getenv("TD_OCC3");      // 0: large batches stay on two workgroups per CU
        h->occ3 = (o3 && std::atoi(o3) == 0) ? 0 : 1;
    }
    {
        td::LutEntry<double> l64[td::kLutSize];
        td::LutEntry<float> l32[td::kLutSize];
        td::build_lut<double>(l64);
        td::build_lut<float>(l32);
        if (!td::lut_vhi_is_next_vlo(l64) || !td::lut_vhi_is_next_vlo(l32) ||
            !td::lut_one_threshold_per_bucket<double>() || !td::lut_one_threshold_per_bucket<float>()) {
            delete h;
            return fail(TD_EINVAL, "td_create: max* table does not have the chained form the kernels read");
        }
    }
    if (!td::build_trellis(13, 15, h->tr) || !td::build_lane_tables(h->tr, h->lane) || !td::trellis_is_lte(h->tr)) {   // G_ROW_1/2, log_map.h:35-36
        delete h;
        return fail(TD_EINVAL, "td_create: trellis does not fit the rotating-label kernel");
    }
    h->pi = std::move(pi);
    // the permutation tables carry td::kPermPad spare (zero) ints: the loader stages whole windows
    if (hipMalloc(&h->d_pi, sizeof(int) * (p->K + td::kPermPad)) != hipSuccess ||
        hipMalloc(&h->d_pinv, sizeof(int) * (p->K + td::kPermPad)) != hipSuccess ||
        hipMalloc(&h->d_lut, sizeof(td::LutEntry<double>) * td::kLutSize) != hipSuccess ||
        hipMalloc(&h->d_qlut, sizeof(double) * td::kQRows) != hipSuccess ||
        hipMalloc(&h->d_lane, sizeof(td::LaneTables)) != hipSuccess ||
        hipMalloc(&h->d_slots, sizeof(unsigned) * td::kCuSlotKeys) != hipSuccess ||
        hipMalloc(&h->d_clk, 4 * sizeof(unsigned long long)) != hipSuccess) {
        td_destroy(h);
        return fail(TD_ENOMEM, "td_create: hipMalloc failed");
    }
    hipError_t e = hipMemset(h->d_pi, 0, sizeof(int) * (p->K + td::kPermPad));
    if (e == hipSuccess) e = hipMemset(h->d_pinv, 0, sizeof(int) * (p->K + td::kPermPad));
    if (e == hipSuccess) e = hipMemcpy(h->d_pi, h->pi.data(), sizeof(int) * p->K, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->d_slots, 0, sizeof(unsigned) * td::kCuSlotKeys);
    if (e == hipSuccess) e = hipMemset(h->d_clk, 0, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpy(h->d_lane, &h->lane, sizeof(td::LaneTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        std::vector<int> inv(p->K);
        for (int i = 0; i < p->K; ++i) inv[h->pi[i]] = i;
        e = hipMemcpy(h->d_pinv, inv.data(), sizeof(int) * p->K, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        if (p->precision == TD_F64) {
            td::LutEntry<double> lut[td::kLutSize];
            td::build_lut<double>(lut);
            double q[td::kQRows];
            td::build_qlut<double>(q);
            e = hipMemcpy(h->d_lut, lut, sizeof lut, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(h->d_qlut, q, sizeof q, hipMemcpyHostToDevice);
        } else {
            td::LutEntry<float> lut[td::kLutSize];
            td::build_lut<float>(lut);
            float q[td::kQRows];
            td::build_qlut<float>(q);
            e = hipMemcpy(h->d_lut, lut, sizeof lut, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(h->d_qlut, q, sizeof q, hipMemcpyHostToDevice);
        }
    }
    if (e != hipSuccess) {
        td_destroy(h);
        return hip_fail(e, "td_create: table upload");
    }
    *out = h;
    return TD_OK;
}

int td_destroy(td_handle* h)
{
    if (!h) return TD_OK;
    (void)hipSetDevice(h->p.device);
    if (h->d_ws) (void)ws_release(h->d_ws);
    if (h->d_pi) (void)hipFree(h->d_pi);
    if (h->d_pinv) (void)hipFree(h->d_pinv);
    if (h->d_lut) (void)hipFree(h->d_lut);
    if (h->d_qlut) (void)hipFree(h->d_qlut);
    if (h->d_lane) (void)hipFree(h->d_lane);
    if (h->d_slots) (void)hipFree(h->d_slots);
    if (h->d_clk) (void)hipFree(h->d_clk);
    if (h->d_hin) (void)hipFree(h->d_hin);
    if (h->d_hbits) (void)hipFree(h->d_hbits);
    if (h->d_hle) (void)hipFree(h->d_hle);
    if (h->d_hiters) (void)hipFree(h->d_hiters);
    if (h->d_crc) (void)hipFree(h->d_crc);
    if (h->d_win) (void)hipFree(h->d_win);
    if (h->d_wws) (void)hipFree(h->d_wws);
    if (h->d_rm_rank) (void)hipFree(h->d_rm_rank);
    if (h->d_rm_pos) (void)hipFree(h->d_rm_pos);
    if (h->d_crc_tab) (void)hipFree(h->d_crc_tab);
    release_wstr(h->wstr);
    for (auto& tri : h->ev)
        for (auto& e : tri) (void)hipEventDestroy(e);
    if (h->ws_free) (void)hipEventDestroy(h->ws_free);
    delete h;
    return TD_OK;
}

int td_reserve(td_handle* h, int B)
{
    if (!h || B < 1) return fail(TD_EINVAL, "td_reserve: bad argument");
    TD_HIP(hipSetDevice(h->p.device));
    if (is_fixed(h)) return ensure_fixed_ws(h, B);   // a plain allocation: no placement search
    const int rc = place_ws(h, groups_for(B));
    if (rc || !h->wp.window) return rc;
    return ensure_wws(h, win_carve(h, B).total);   // the windowed schedule's buffers as well
}

int td_decode_device_stop(td_handle* h, const void* d_llr, int B, uint8_t* d_bits, int all_iters, void* d_le,
                          int32_t* d_iters, void* stream)
{
    if (!h || !d_llr || !d_bits || B < 1) return fail(TD_EINVAL, "td_decode_device: bad argument");
    TD_HIP(hipSetDevice(h->p.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (is_fixed(h)) return decode_fixed(h, d_llr, B, d_bits, all_iters, d_le, d_iters, st);
    if (h->p.precision == TD_F64) return decode_device_t<double>(h, d_llr, B, d_bits, all_iters, d_le, d_iters, st);
    return decode_device_t<float>(h, d_llr, B, d_bits, all_iters, d_le, d_iters, st);
}

int td_decode_device(td_handle* h, const void* d_llr, int B, uint8_t* d_bits, int all_iters, void* d_le,
                     void* stream)
{
    return td_decode_device_stop(h, d_llr, B, d_bits, all_iters, d_le, nullptr, stream);
}

int td_set_early_stop(td_handle* h, const td_stop_params* s)
{
    if (!h) return fail(TD_EINVAL, "td_set_early_stop: null handle");
    if (const int nf = not_fixed(h, "td_set_early_stop")) return nf;
    if (!s || s->rule == TD_STOP_NONE) {
        h->stop = td_stop_params{TD_STOP_NONE, 1, 0};
        return TD_OK;
    }
    if (s->rule != TD_STOP_HDA && s->rule != TD_STOP_CRC) return fail(TD_EINVAL, "td_set_early_stop: unknown rule");
    if (s->min_iters < 1 || s->min_iters > h->p.iterations)
        return fail(TD_EINVAL, "td_set_early_stop: min_iters must be in [1, iterations]");
    if (h->wp.window)
        return fail(TD_EINVAL, "td_set_early_stop: the handle's schedule is windowed (td_set_window): its rule is set by "
                               "td_set_window_stop");
    if (s->rule == TD_STOP_CRC) {
        if (s->crc_poly == 0 || (s->crc_poly & ~td::kCrc24Mask))
            return fail(TD_EINVAL, "td_set_early_stop: crc_poly must be the 24 low-order coefficients, non-zero");
        if (h->p.K <= 24) return fail(TD_EINVAL, "td_set_early_stop: TD_STOP_CRC needs K > 24");
        TD_HIP(hipSetDevice(h->p.device));
        // the table lives on the device from here on: a decode allocates nothing for the rule
        if (!h->d_crc && hipMalloc(reinterpret_cast<void**>(&h->d_crc), (size_t)h->p.K * sizeof(uint32_t)) != hipSuccess) {
            h->d_crc = nullptr;
            return fail(TD_ENOMEM, "td_set_early_stop: hipMalloc failed");
        }
        std::vector<uint32_t> tab((size_t)h->p.K);
        td::crc24_syndromes(h->p.K, s->crc_poly, tab.data());
        TD_HIP(hipDeviceSynchronize());   // no decode of this handle still reads the previous table
        TD_HIP(hipMemcpy(h->d_crc, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    h->stop = *s;
    return TD_OK;
}

int td_set_window_stop(td_handle* h, const td_stop_params* s)
{
    if (!h) return fail(TD_EINVAL, "td_set_window_stop: null handle");
    if (const int nf = not_fixed(h, "td_set_window_stop")) return nf;
    if (!h->wp.window)
        return fail(TD_EINVAL, "td_set_window_stop: the handle's schedule is not windowed (td_set_window first; the exact "
                               "schedule's rule is td_set_early_stop)");
    if (!s || s->rule == TD_STOP_NONE) {
        h->wstop = td_stop_params{TD_STOP_NONE, 1, 0};
        return TD_OK;
    }
    if (s->rule != TD_STOP_HDA && s->rule != TD_STOP_CRC) return fail(TD_EINVAL, "td_set_window_stop: unknown rule");
    if (s->min_iters < 1 || s->min_iters > h->p.iterations)
        return fail(TD_EINVAL, "td_set_window_stop: min_iters must be in [1, iterations]");
    if (s->rule == TD_STOP_CRC) {
        if (s->crc_poly == 0 || (s->crc_poly & ~td::kCrc24Mask))
            return fail(TD_EINVAL, "td_set_window_stop: crc_poly must be the 24 low-order coefficients, non-zero");
        if (h->p.K <= 24) return fail(TD_EINVAL, "td_set_window_stop: TD_STOP_CRC needs K > 24");
        TD_HIP(hipSetDevice(h->p.device));
        // the table lives on the device from here on: a decode allocates nothing for the rule
        if (!h->d_crc && hipMalloc(reinterpret_cast<void**>(&h->d_crc), (size_t)h->p.K * sizeof(uint32_t)) != hipSuccess) {
            h->d_crc = nullptr;
            return fail(TD_ENOMEM, "td_set_window_stop: hipMalloc failed");
        }
        std::vector<uint32_t> tab((size_t)h->p.K);
        td::crc24_syndromes(h->p.K, s->crc_poly, tab.data());
        TD_HIP(hipDeviceSynchronize());   // no decode of this handle still reads the previous table
        TD_HIP(hipMemcpy(h->d_crc, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    h->wstop = *s;
    return TD_OK;
}

// td_set_fixed_stop and td_set_fixed_window_stop: `who` is the entry point, `rule` the handle's member that it
// sets, `window` the schedule that it needs and `other` its message on a handle with the other one.  The
// sub-block setter refuses a handle without a window before anything else, the rule's off included; the
// exact one refuses a window only for a rule that it would otherwise set.
static int set_fixed_rule(td_handle* h, const td_stop_params* s, const std::string& who, td_stop_params td_handle::*rule,
                          bool window, const char* other)
{
    if (!h) return fail(TD_EINVAL, who + ": null handle");
    if (!is_fixed(h)) return fail(TD_EINVAL, who + ": the handle is not fixed-point (TD_FIXED)");
    const bool wrong = (h->fwin.window != 0) != window;
    if (window && wrong) return fail(TD_EINVAL, who + other);
    if (!s || s->rule == TD_STOP_NONE) {
        h->*rule = td_stop_params{TD_STOP_NONE, 1, 0};
        return TD_OK;
    }
    if (s->rule != TD_STOP_HDA && s->rule != TD_STOP_CRC) return fail(TD_EINVAL, who + ": unknown rule");
    if (wrong) return fail(TD_EINVAL, who + other);
    if (s->min_iters < 1 || s->min_iters > h->p.iterations)
        return fail(TD_EINVAL, who + ": min_iters must be in [1, iterations]");
    if (s->rule == TD_STOP_CRC) {
        if (s->crc_poly == 0 || (s->crc_poly & ~td::kCrc24Mask))
            return fail(TD_EINVAL, who + ": crc_poly must be the 24 low-order coefficients, non-zero");
        if (h->p.K <= 24) return fail(TD_EINVAL, who + ": TD_STOP_CRC needs K > 24");
        TD_HIP(hipSetDevice(h->p.device));
        // the table lives on the device from here on: a decode allocates nothing for the rule
        if (!h->d_crc && hipMalloc(reinterpret_cast<void**>(&h->d_crc), (size_t)h->p.K * sizeof(uint32_t)) != hipSuccess) {
            h->d_crc = nullptr;
            return fail(TD_ENOMEM, who + ": hipMalloc failed");
        }
        std::vector<uint32_t> syn((size_t)h->p.K), tab((size_t)h->p.K);
        td::crc24_syndromes(h->p.K, s->crc_poly, syn.data());
        for (int i = 0; i < h->p.K; ++i) tab[i] = syn[h->pi[i]];   // in the order SISO2 meets the bits (FxStop)
        TD_HIP(hipDeviceSynchronize());   // no decode of this handle still reads the previous table
        TD_HIP(hipMemcpy(h->d_crc, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    h->*rule = *s;
    return TD_OK;
}

int td_set_fixed_stop(td_handle* h, const td_stop_params* s)
{
    return set_fixed_rule(h, s, "td_set_fixed_stop", &td_handle::fstop, false,
                          ": the TD_FIXED handle has a sub-block schedule (td_set_fixed_window); "
                          "its rule is set by td_set_fixed_window_stop");
}

int td_set_fixed_window_stop(td_handle* h, const td_stop_params* s)
{
    return set_fixed_rule(h, s, "td_set_fixed_window_stop", &td_handle::fwstop, true,
                          ": the TD_FIXED handle's schedule is not the sub-block one "
                          "(td_set_fixed_window first; the exact schedule's rule is td_set_fixed_stop)");
}

uint32_t td_crc24_host(const uint8_t* bits, int K, uint32_t poly)
{
    if (!bits || K < 1) return 0;
    return td::crc24_bits(bits, K, poly);
}

int td_crc24_syndromes(int K, uint32_t poly, uint32_t* table)
{
    if (K < 1 || !table) return fail(TD_EINVAL, "td_crc24_syndromes: bad argument");
    td::crc24_syndromes(K, poly, table);
    return TD_OK;
}

int td_set_fixed(td_handle* h, const td_fixed_params* f)
{
    if (!h) return fail(TD_EINVAL, "td_set_fixed: null handle");
    if (!is_fixed(h)) return fail(TD_EINVAL, "td_set_fixed: the handle is not fixed-point (TD_FIXED)");
    if (!f) {
        h->fxp = td_fixed_params{255, 3};
        return TD_OK;
    }
    if (f->le_max < 1 || f->le_max > 255) return fail(TD_EINVAL, "td_set_fixed: le_max must be in [1, 255]");
    if (f->ext_scale_q < 1 || f->ext_scale_q > 4)
        return fail(TD_EINVAL, "td_set_fixed: ext_scale_q must be in [1, 4] (quarters; 4 = no scaling)");
    h->fxp = *f;
    return TD_OK;
}

int td_set_fixed_maxstar(td_handle* h, const td_fixed_maxstar_params* m)
{
    if (!h) return fail(TD_EINVAL, "td_set_fixed_maxstar: null handle");
    if (!is_fixed(h)) return fail(TD_EINVAL, "td_set_fixed_maxstar: the handle is not fixed-point (TD_FIXED)");
    if (!m) {
        h->fms_on = false;
        return TD_OK;
    }
    if (m->shift < 0 || m->shift > 8) return fail(TD_EINVAL, "td_set_fixed_maxstar: shift must be in [0, 8]");
    for (int j = 0; j < 8; ++j)
        if (m->corr[j] > 63) return fail(TD_EINVAL, "td_set_fixed_maxstar: every entry of corr must be in [0, 63]");
    if (m->corr[7] != 0) return fail(TD_EINVAL, "td_set_fixed_maxstar: corr[7] must be 0");
    h->fms = *m;
    h->fms_on = true;
    return TD_OK;
}

int td_fixed_maxstar_table(double steps_per_unit, int shift, td_fixed_maxstar_params* out)
{
    if (!out) return fail(TD_EINVAL, "td_fixed_maxstar_table: null output");
    if (!(steps_per_unit > 0.0 && steps_per_unit <= 32.0))
        return fail(TD_EINVAL, "td_fixed_maxstar_table: steps_per_unit must be in (0, 32]");
    const double s = 2.0 * steps_per_unit;   // metric steps per nat
    if (shift < 0) {
        shift = 0;
        while (shift <= 8 && !(s * std::log1p(std::exp(-7.0 * std::ldexp(1.0, shift) / s)) < 1.0)) ++shift;
    }
    if (shift > 8) return fail(TD_EINVAL, "td_fixed_maxstar_table: the rule gives a shift above 8");
    td_fixed_maxstar_params t{};
    t.shift = shift;
    for (int j = 0; j < 7; ++j) {
        const double c = std::floor(s * std::log1p(std::exp(-(j + 0.5) * std::ldexp(1.0, shift) / s)) + 0.5);
        if (c > 63.0) return fail(TD_EINVAL, "td_fixed_maxstar_table: the rule gives an entry above 63");
        t.corr[j] = (uint8_t)c;
    }
    t.corr[7] = 0;
    *out = t;
    return TD_OK;
}

int td_set_fixed_window(td_handle* h, const td_fixed_window_params* w)
{
    if (!h) return fail(TD_EINVAL, "td_set_fixed_window: null handle");
    if (!is_fixed(h)) return fail(TD_EINVAL, "td_set_fixed_window: the handle is not fixed-point (TD_FIXED)");
    if (!w || w->window == 0) {
        h->fwin = td_fixed_window_params{0, 0};
        h->fwstop = td_stop_params{TD_STOP_NONE, 1, 0};   // the sub-block schedule's rule goes with it
        h->fnii = false;                                  // and its next-iteration initialisation
        return TD_OK;
    }
    if (w->window < td::fx::kW || w->window % td::fx::kW)
        return fail(TD_EINVAL, "td_set_fixed_window: the window of a TD_FIXED handle must be 0 or a multiple of 16");
    if (w->overlap < 0 || w->overlap > 3 * (long long)w->window)
        return fail(TD_EINVAL, "td_set_fixed_window: the overlap of a TD_FIXED handle must be in [0, 3*window]");
    if (h->fstop.rule != TD_STOP_NONE)
        return fail(TD_EINVAL, "td_set_fixed_window: the TD_FIXED handle has an early-termination rule "
                               "(td_set_fixed_stop); turn it off first");
    if (h->fnii && w->overlap % td::fx::kW)
        return fail(TD_EINVAL, "td_set_fixed_window: with next-iteration initialisation on (td_set_fixed_window_nii) the "
                               "overlap must be a multiple of 16");
    h->fwin = *w;
    return TD_OK;
}

int td_set_fixed_window_nii(td_handle* h, int on)
{
    if (!h) return fail(TD_EINVAL, "td_set_fixed_window_nii: null handle");
    if (!is_fixed(h)) return fail(TD_EINVAL, "td_set_fixed_window_nii: the handle is not fixed-point (TD_FIXED)");
    if (!h->fwin.window)
        return fail(TD_EINVAL, "td_set_fixed_window_nii: the TD_FIXED handle's schedule is not the sub-block one "
                               "(td_set_fixed_window first)");
    if (on && h->fwin.overlap % td::fx::kW)
        return fail(TD_EINVAL, "td_set_fixed_window_nii: the overlap must be a multiple of 16 (td_set_fixed_window)");
    h->fnii = on != 0;
    return TD_OK;
}

int td_set_window(td_handle* h, const td_window_params* w)
{
    if (!h) return fail(TD_EINVAL, "td_set_window: null handle");
    if (const int nf = not_fixed(h, "td_set_window")) return nf;
    if (!w || w->window == 0) {
        h->wp = td::WindowParams{0, 0, 0, 0, 1.0, 0, 0, 0, 0};
        h->wstop = td_stop_params{TD_STOP_NONE, 1, 0};   // the windowed schedule's rule goes with it
        return TD_OK;
    }
    if (w->window < 3 || w->window > 10000) return fail(TD_EINVAL, "td_set_window: window must be 0 or in [3, 10000]");
    if (h->stop.rule != TD_STOP_NONE)
        return fail(TD_EINVAL, "td_set_window: the handle has the exact schedule's early-termination rule "
                               "(td_set_early_stop); turn it off first (the windowed schedule's is td_set_window_stop)");
    if (w->overlap < 0 || w->overlap > 3 * w->window)
        return fail(TD_EINVAL, "td_set_window: overlap must be in [0, 3*window]");
    if (!(w->ext_scale > 0.0) || !(w->ext_scale <= 4.0))
        return fail(TD_EINVAL, "td_set_window: ext_scale must be in (0, 4]");
    TD_HIP(hipSetDevice(h->p.device));
    const int rc = ensure_wstr(h);
    if (rc) return rc;
    h->wp = td::WindowParams{w->window, w->overlap, w->nii ? 1 : 0, w->concurrent ? 1 : 0, w->ext_scale,
                             h->win_run, h->win_run_a, h->win_parts, h->win_exact_table};
    return TD_OK;
}

int td_set_window_maxstar(td_handle* h, int form)
{
    if (!h) return fail(TD_EINVAL, "td_set_window_maxstar: null handle");
    if (const int nf = not_fixed(h, "td_set_window_maxstar")) return nf;
    if (form != TD_WMAXSTAR_FAST && form != TD_WMAXSTAR_EXACT)
        return fail(TD_EINVAL, "td_set_window_maxstar: form must be TD_WMAXSTAR_FAST or TD_WMAXSTAR_EXACT");
    h->win_exact_table = form == TD_WMAXSTAR_EXACT ? 1 : 0;
    h->wp.exact_table = h->win_exact_table;
    return TD_OK;
}

int td_debug_window_layout(td_handle* h, int run, int run_a, int parts)
{
    if (!h) return fail(TD_EINVAL, "td_debug_window_layout: null handle");
    if (run < 0 || run_a < 0 || parts < 0 || parts > td::kSwMaxParts)
        return fail(TD_EINVAL, "td_debug_window_layout: run, run_a >= 0 and 0 <= parts <= 4");
    h->win_run = run;
    h->win_run_a = run_a;
    h->win_parts = parts;
    if (h->wp.window) {
        h->wp.run = run;
        h->wp.run_a = run_a;
        h->wp.parts = parts;
    }
    return TD_OK;
}

int td_profile_enable(td_handle* h, int on)
{
    if (!h) return fail(TD_EINVAL, "td_profile_enable: null handle");
    h->prof = on != 0;
    h->nev = 0;
    return TD_OK;
}

int td_profile_read(td_handle* h, float* demux_ms, float* decode_ms, int* launches)
{
    if (!h || !h->prof) return fail(TD_EINVAL, "td_profile_read: profiling not enabled");
    TD_HIP(hipSetDevice(h->p.device));
    double sa = 0, sb = 0;
    for (size_t k = 0; k < h->nev; ++k) {
        float a = 0, b = 0;
        TD_HIP(hipEventSynchronize(h->ev[k][2]));
        TD_HIP(hipEventElapsedTime(&a, h->ev[k][0], h->ev[k][1]));
        TD_HIP(hipEventElapsedTime(&b, h->ev[k][1], h->ev[k][2]));
        sa += a;
        sb += b;
    }
    const int n = (int)h->nev;
    if (demux_ms) *demux_ms = n ? (float)(sa / n) : 0.f;
    if (decode_ms) *decode_ms = n ? (float)(sb / n) : 0.f;
    if (launches) *launches = n;
    h->nev = 0;
    return TD_OK;
}

int td_clock_read(td_handle* h, double* sclk_ghz, double* span_ms)
{
    if (!h) return fail(TD_EINVAL, "td_clock_read: null handle");
    if (const int nf = not_fixed(h, "td_clock_read")) return nf;
    if (!h->clk_valid) return fail(TD_EINVAL, "td_clock_read: the last decode was captured into a graph");
    if (h->clk_stopped)
        return fail(TD_EINVAL, "td_clock_read: the last decode ran the windowed schedule with early termination "
                               "(td_set_window_stop), which takes no clock sample");
    TD_HIP(hipSetDevice(h->p.device));
    if (h->ws_pending && h->ws_free) TD_HIP(hipEventSynchronize(h->ws_free));   // this handle's last decode only
    unsigned long long v[4] = {};
    TD_HIP(hipMemcpy(v, h->d_clk, sizeof v, hipMemcpyDeviceToHost));
    const double cyc = (double)(v[2] - v[0]), ticks = (double)(v[3] - v[1]);   // s_memrealtime: 100 MHz
    if (v[3] <= v[1] || v[2] <= v[0]) return fail(TD_EINVAL, "td_clock_read: no decode recorded yet");
    if (sclk_ghz) *sclk_ghz = cyc / ticks * 0.1;
    if (span_ms) *span_ms = ticks * 1e-5;
    return TD_OK;
}

int td_debug_set_stamps(td_handle* h, void* d_buf)
{
    if (!h) return fail(TD_EINVAL, "td_debug_set_stamps: null handle");
    if (const int nf = not_fixed(h, "td_debug_set_stamps")) return nf;
    h->stamps = d_buf;
    return TD_OK;
}

int td_debug_placement(td_handle* h, float* ms, int cap, int* pick)
{
    if (!h) return fail(TD_EINVAL, "td_debug_placement: null handle");
    const int n = (int)h->place_ms.size();
    for (int i = 0; i < n && i < cap && ms; ++i) ms[i] = h->place_ms[i];
    if (pick) *pick = h->place_pick;
    return n;
}

int td_debug_placement_cost(td_handle* h, double* wall_ms, double* held_bytes)
{
    if (!h) return fail(TD_EINVAL, "td_debug_placement_cost: null handle");
    if (wall_ms) *wall_ms = h->place_wall_ms;
    if (held_bytes) *held_bytes = h->place_held;
    return TD_OK;
}

int td_debug_workspace_bytes(td_handle* h, unsigned long long* bytes)
{
    if (!h || !bytes) return fail(TD_EINVAL, "td_debug_workspace_bytes: null argument");
    *bytes = (unsigned long long)h->ws_bytes;
    return TD_OK;
}

int td_debug_workspace_fill(td_handle* h, int byte, unsigned long long* filled)
{
    if (!h) return fail(TD_EINVAL, "td_debug_workspace_fill: null handle");
    if (byte < -1 || byte > 255) return fail(TD_EINVAL, "td_debug_workspace_fill: byte must be -1 or in [0, 255]");
    if (filled) *filled = 0;
    if (byte < 0) {
        h->poison = -1;
        return TD_OK;
    }
    TD_HIP(hipSetDevice(h->p.device));
    TD_HIP(hipDeviceSynchronize());   // no decode still runs on what is about to be overwritten
    // the scratch only: the tables (d_pi, d_pinv, d_lut, d_qlut, d_lane, d_slots, d_crc, d_rm_*) and the
    // generator's d_win hold what later launches read as it is
    const std::pair<void*, size_t> bufs[] = {
        {h->d_ws, h->ws_bytes},    {h->d_wws, h->wws_bytes},          {h->d_hin, h->hin_b},
        {h->d_hbits, h->hbits_b},  {h->d_hle, h->hle_b},              {h->d_hiters, h->hiters_b},
    };
    unsigned long long n = 0;
    for (const auto& b : bufs) {
        if (!b.first || !b.second) continue;
        TD_HIP(hipMemset(b.first, byte, b.second));
        n += b.second;
    }
    TD_HIP(hipDeviceSynchronize());
    h->poison = byte;
    if (filled) *filled = n;
    return TD_OK;
}

int td_debug_placement_rule(const float* ms, int n)
{
    if (!ms || n < 0) return fail(TD_EINVAL, "td_debug_placement_rule: bad argument");
    return placement_fast_seen(std::vector<float>(ms, ms + n)) ? 1 : 0;
}

int td_window_steps(void) { return td::window_steps(); }

int td_debug_stamp_slots(void)
{
#ifdef TD_STAMPS
    return td::kGroupWaves * 16;   // [wave][slot] (td_kernels.hip kStampSlots)
#else
    return 0;
#endif
}

int td_decode_host(td_handle* h, const void* llr, int B, int* out, void* le)
{
    return td_decode_host_stop(h, llr, B, out, le, nullptr);
}

int td_decode_host_stop(td_handle* h, const void* llr, int B, int* out, void* le, int* iters_used)
{
    if (!h || !llr || !out || B < 1) return fail(TD_EINVAL, "td_decode_host: bad argument");
    TD_HIP(hipSetDevice(h->p.device));
    const int K = h->p.K, L = K + td::kMemory, it = h->p.iterations;
    const size_t n = 3 * (size_t)K + 4 * td::kMemory;
    const size_t in_b = (size_t)B * n * h->elem;
    const size_t bits_b = (size_t)B * it * K;
    const size_t le_b = le ? (size_t)B * it * 2 * L * (is_fixed(h) ? sizeof(int16_t) : h->elem) : 0;
    // staging buffers kept by the handle (grown on demand), so a warm per-frame caller allocates nothing
    auto grow = [h](void** p, size_t& cap, size_t need) {
        if (need <= cap) return hipSuccess;
        if (*p) (void)hipFree(*p);
        *p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(p, need);
        if (e != hipSuccess) return e;
        cap = need;
        return poison_fresh(h, *p, need);
    };
    if (grow(&h->d_hin, h->hin_b, in_b) != hipSuccess || grow(reinterpret_cast<void**>(&h->d_hbits), h->hbits_b, bits_b) != hipSuccess ||
        (le && grow(&h->d_hle, h->hle_b, le_b) != hipSuccess) ||
        (iters_used && grow(reinterpret_cast<void**>(&h->d_hiters), h->hiters_b, (size_t)B * sizeof(int32_t)) != hipSuccess))
        return fail(TD_ENOMEM, "td_decode_host: hipMalloc failed");
    TD_HIP(hipMemcpy(h->d_hin, llr, in_b, hipMemcpyHostToDevice));
    const int rc = td_decode_device_stop(h, h->d_hin, B, h->d_hbits, 1, le ? h->d_hle : nullptr,
                                         iters_used ? h->d_hiters : nullptr, nullptr);
    if (rc) return rc;
    h->h_hbits.resize(bits_b);
    TD_HIP(hipMemcpy(h->h_hbits.data(), h->d_hbits, bits_b, hipMemcpyDeviceToHost));   // waits for the decode (null stream)
    if (le) TD_HIP(hipMemcpy(le, h->d_hle, le_b, hipMemcpyDeviceToHost));
    if (iters_used) TD_HIP(hipMemcpy(iters_used, h->d_hiters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < bits_b; ++i) out[i] = h->h_hbits[i];
    return TD_OK;
}

int td_siso_host(td_handle* h, const void* recs, const void* La, int terminated, void* LLR, int L, int B)
{
    if (!h || !recs || !La || !LLR || L < 1 || B < 1) return fail(TD_EINVAL, "td_siso_host: bad argument");
    if (const int nf = not_fixed(h, "td_siso_host")) return nf;
    TD_HIP(hipSetDevice(h->p.device));
    int rc = h->p.precision == TD_F64 ? siso_host_t<double>(h, recs, La, terminated, LLR, L, B)
                                      : siso_host_t<float>(h, recs, La, terminated, LLR, L, B);
    if (!rc) {
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail(e, "td_siso_host");
    }
    return rc;
}


int td_rand_window(unsigned seed, unsigned long long draws, uint32_t* win)
{
    if (!win) return fail(TD_EINVAL, "td_rand_window: null output");
    uint32_t w0[31];
    glibc_window(seed, w0);
    lfg_apply(lfg_power(draws), w0, win);
    return TD_OK;
}

int td_synth_seed(td_handle* h, unsigned seed)
{
    if (!h) return fail(TD_EINVAL, "td_synth_seed: null handle");
    glibc_window(seed, h->lfg_win);
    std::memcpy(h->lfg_win0, h->lfg_win, sizeof h->lfg_win);
    if (h->lfg_jump.empty()) h->lfg_jump = lfg_power((unsigned long long)h->p.K + 2);   // K bits + 2 AWGN seeds
    h->lfg_seeded = true;
    h->lfg_frames = 0;
    return TD_OK;
}

int td_synth_seek(td_handle* h, unsigned long long frame)
{
    if (!h || !h->lfg_seeded) return fail(TD_EINVAL, "td_synth_seek: call td_synth_seed first");
    lfg_apply(lfg_power(frame * ((unsigned long long)h->p.K + 2)), h->lfg_win0, h->lfg_win);
    h->lfg_frames = frame;
    return TD_OK;
}

int td_synth_frames(td_handle* h, double ebn0_db, int B, uint8_t* d_info, double* d_llr, void* stream)
{
    if (!h || B < 1 || !d_info || !d_llr) return fail(TD_EINVAL, "td_synth_frames: bad argument");
    if (!h->lfg_seeded) return fail(TD_EINVAL, "td_synth_frames: call td_synth_seed first");
    TD_HIP(hipSetDevice(h->p.device));
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (B > h->win_cap) {
        if (h->d_win) (void)hipFree(h->d_win);
        h->d_win = nullptr;
        h->win_cap = 0;
        if (hipMalloc(&h->d_win, sizeof(uint32_t) * 31 * (size_t)B) != hipSuccess)
            return fail(TD_ENOMEM, "td_synth_frames: hipMalloc failed");
        h->win_cap = B;
    }
    std::vector<uint32_t> wins((size_t)B * 31);
    for (int b = 0; b < B; ++b) {
        std::memcpy(&wins[(size_t)b * 31], h->lfg_win, sizeof h->lfg_win);
        uint32_t next[31];
        lfg_apply(h->lfg_jump, h->lfg_win, next);
        std::memcpy(h->lfg_win, next, sizeof next);
    }
    h->lfg_frames += (unsigned long long)B;
    TD_HIP(hipMemcpyAsync(h->d_win, wins.data(), wins.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const int K = h->p.K, n = 3 * K + 4 * td::kMemory, M = h->modulation;
    const int nsym = n / M;                                                         // SYMBOL_NUM, main.cpp:15
    const double rate = (double)K / (double)nsym;                                   // main.cpp:47
    const double sigma = std::pow(10.0, -ebn0_db / 20) * std::sqrt(0.5 / (rate * M));   // main.cpp:174
    td::SynthParams sp{K, n, B, M, h->d_pi, h->d_win, sigma, 1 / (2 * std::pow(sigma, 2)), d_info, d_llr};
    TD_HIP(td::launch_synth(sp, st));
    // the host window buffer must outlive the async copy
    TD_HIP(hipStreamSynchronize(st));
    return TD_OK;
}

int td_synth_modulation(td_handle* h, int modulation)
{
    if (!h) return fail(TD_EINVAL, "td_synth_modulation: null handle");
    const int n = 3 * h->p.K + 4 * td::kMemory;
    if (modulation != 1 && modulation != 2 && modulation != 3 && modulation != 4 && modulation != 6)
        return fail(TD_EINVAL, "td_synth_modulation: modulation must be 1, 2, 3, 4 or 6 bits per symbol");
    if (n % modulation)
        return fail(TD_EINVAL, "td_synth_modulation: 3K+12 = " + std::to_string(n) + " is not a whole number of symbols");
    h->modulation = modulation;
    return TD_OK;
}

int td_modulate(const uint8_t* d_bits, long long nsym, int modulation, double* d_si, double* d_sq, void* stream)
{
    if (!d_bits || !d_si || !d_sq || nsym < 0) return fail(TD_EINVAL, "td_modulate: bad argument");
    if (nsym == 0) return TD_OK;
    const hipError_t e = td::launch_modulate(d_bits, nsym, modulation, d_si, d_sq, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(TD_EINVAL, "td_modulate: modulation must be 1, 2, 3, 4 or 6");
    TD_HIP(e);
    return TD_OK;
}

int td_demodulate(const double* d_yi, const double* d_yq, long long nsym, int modulation, double Kf, double* d_llr,
                  void* stream)
{
    if (!d_yi || !d_yq || !d_llr || nsym < 0) return fail(TD_EINVAL, "td_demodulate: bad argument");
    if (nsym == 0) return TD_OK;
    const hipError_t e = td::launch_demodulate(d_yi, d_yq, nsym, modulation, Kf, d_llr, static_cast<hipStream_t>(stream));
    if (e == hipErrorInvalidValue) return fail(TD_EINVAL, "td_demodulate: modulation must be 1, 2, 3, 4 or 6");
    TD_HIP(e);
    return TD_OK;
}

namespace {

// steps_per_unit finite and > 0, judged on its bits: the library is built with -fno-honor-nans, under which
// a floating-point comparison may let a NaN through
bool steps_ok(double s)
{
    uint64_t u;
    std::memcpy(&u, &s, sizeof u);
    return (u >> 63) == 0 && ((u >> 52) & 0x7FF) != 0x7FF && (u << 1) != 0;
}

}  // namespace

int td_llr_convert(const double* d_in, long long n, int precision, double steps_per_unit, void* d_out, void* stream)
{
    if (!d_in || !d_out) return fail(TD_EINVAL, "td_llr_convert: null pointer");
    if (n < 0) return fail(TD_EINVAL, "td_llr_convert: negative n");
    if (precision != TD_F64 && precision != TD_F32 && precision != TD_FIXED)
        return fail(TD_EINVAL, "td_llr_convert: precision must be TD_F64, TD_F32 or TD_FIXED");
    if (precision == TD_FIXED && !steps_ok(steps_per_unit))
        return fail(TD_EINVAL, "td_llr_convert: steps_per_unit must be finite and positive");
    if (n == 0) return TD_OK;
    TD_HIP(td::launch_llr_convert(d_in, n, precision, steps_per_unit, d_out, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

// ---- scrambling (td_gold_core.h, td_scramble.h) ----

int td_gold_sequence_host(uint32_t cinit, long long len, uint32_t* seq)
{
    if (!seq) return fail(TD_EINVAL, "td_gold_sequence_host: null pointer");
    if (len < 0 || len > td::gold::kGoldMaxLen) return fail(TD_EINVAL, "td_gold_sequence_host: len must be in [0, 2^31)");
    if (len == 0) return TD_OK;
    td::gold::gold_words(td::gold::kGoldTables, cinit, len, 0, (len + 31) / 32, seq);
    return TD_OK;
}

namespace {

// the checks the three device calls share; rc < 0: nothing to do
int scramble_args(const char* who, bool pointers, int N, long long len)
{
    const std::string w(who);
    if (!pointers) return fail(TD_EINVAL, w + ": null pointer");
    if (N < 0) return fail(TD_EINVAL, w + ": negative N");
    if (len < 0 || len > td::gold::kGoldMaxLen) return fail(TD_EINVAL, w + ": len must be in [0, 2^31)");
    return N == 0 || len == 0 ? -1 : TD_OK;
}

}  // namespace

int td_gold_sequence(const uint32_t* d_cinit, int N, long long len, uint32_t* d_seq, void* stream)
{
    if (const int rc = scramble_args("td_gold_sequence", d_cinit && d_seq, N, len)) return rc < 0 ? TD_OK : rc;
    if (!td::launch_gold_sequence) return fail(TD_EHIP, "td_gold_sequence: this build has no td_scramble.hip");
    TD_HIP(td::launch_gold_sequence(d_cinit, N, len, d_seq, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_scramble(const uint8_t* d_in, const uint32_t* d_seq, int N, long long len, uint8_t* d_out, void* stream)
{
    if (const int rc = scramble_args("td_scramble", d_in && d_seq && d_out, N, len)) return rc < 0 ? TD_OK : rc;
    if (!td::launch_scramble) return fail(TD_EHIP, "td_scramble: this build has no td_scramble.hip");
    TD_HIP(td::launch_scramble(d_in, d_seq, N, len, d_out, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_descramble_llr(const void* d_in, int precision, const uint32_t* d_seq, int N, long long len, void* d_out, void* stream)
{
    if (precision != TD_F64 && precision != TD_F32 && precision != TD_FIXED)
        return fail(TD_EINVAL, "td_descramble_llr: precision must be TD_F64, TD_F32 or TD_FIXED");
    if (const int rc = scramble_args("td_descramble_llr", d_in && d_seq && d_out, N, len)) return rc < 0 ? TD_OK : rc;
    if (!td::launch_descramble_llr) return fail(TD_EHIP, "td_descramble_llr: this build has no td_scramble.hip");
    const int es = precision == TD_F64 ? 8 : precision == TD_F32 ? 4 : 1;
    TD_HIP(td::launch_descramble_llr(d_in, es, d_seq, N, len, d_out, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_count_errors(td_handle* h, const uint8_t* d_bits, int iters, const uint8_t* d_info, int B, int* d_err,
                    void* stream)
{
    if (!h || !d_bits || !d_info || !d_err || B < 1 || iters < 1) return fail(TD_EINVAL, "td_count_errors: bad argument");
    TD_HIP(hipSetDevice(h->p.device));
    TD_HIP(td::launch_count_errors(d_bits, d_info, h->p.K, iters, B, d_err, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_rm_set(td_handle* h, int Ncb)
{
    if (!h) return fail(TD_EINVAL, "td_rm_set: null handle");
    td::RmTables t;
    if (!td::rm_build(h->p.K, Ncb, t)) {
        const int Kpi = 32 * ((h->p.K + 4 + 31) / 32);
        return fail(TD_EINVAL, "td_rm_set: Ncb = " + std::to_string(Ncb) + " is neither 0 nor in [Kpi, Kw] = [" +
                                   std::to_string(Kpi) + ", " + std::to_string(3 * Kpi) + "]");
    }
    TD_HIP(hipSetDevice(h->p.device));
    if (!h->d_rm_rank && hipMalloc(&h->d_rm_rank, sizeof(int32_t) * t.rank.size()) != hipSuccess)
        return fail(TD_ENOMEM, "td_rm_set: hipMalloc failed");
    if (!h->d_rm_pos && hipMalloc(&h->d_rm_pos, sizeof(int32_t) * t.Kw) != hipSuccess)
        return fail(TD_ENOMEM, "td_rm_set: hipMalloc failed");
    TD_HIP(hipDeviceSynchronize());   // launches that still read the previous tables
    h->rm_set = false;
    TD_HIP(hipMemcpy(h->d_rm_rank, t.rank.data(), sizeof(int32_t) * t.rank.size(), hipMemcpyHostToDevice));
    TD_HIP(hipMemcpy(h->d_rm_pos, t.pos.data(), sizeof(int32_t) * t.pos.size(), hipMemcpyHostToDevice));
    h->rm = std::move(t);
    h->rm_set = true;
    return TD_OK;
}

int td_rm_info(td_handle* h, int* R, int* Kpi, int* Kw, int* Ncb, int* n_nonnull)
{
    if (!h) return fail(TD_EINVAL, "td_rm_info: null handle");
    if (!h->rm_set) return fail(TD_EINVAL, "td_rm_info: call td_rm_set first");
    if (R) *R = h->rm.R;
    if (Kpi) *Kpi = h->rm.Kpi;
    if (Kw) *Kw = h->rm.Kw;
    if (Ncb) *Ncb = h->rm.Ncb;
    if (n_nonnull) *n_nonnull = h->rm.Nnn;
    return TD_OK;
}

namespace {

// the argument checks td_rate_match and td_rate_dematch share; fills the launch's view of the tables
int rm_launch_params(const char* who, td_handle* h, const void* a, const void* b, int B, int rv, int E, td::RmParams& p)
{
    const std::string w(who);
    if (!h || !a || !b) return fail(TD_EINVAL, w + ": null argument");
    if (!h->rm_set) return fail(TD_EINVAL, w + ": call td_rm_set first");
    if (rv < 0 || rv > 3) return fail(TD_EINVAL, w + ": rv must be in 0..3");
    if (E < 1) return fail(TD_EINVAL, w + ": E must be at least 1");
    if (B < 0) return fail(TD_EINVAL, w + ": negative B");
    p = td::RmParams{h->p.K, h->rm.R, h->rm.ND, h->rm.Nnn, h->rm.c0[rv], E, B, h->d_rm_rank, h->d_rm_pos};
    return TD_OK;
}

}  // namespace

int td_rate_match(td_handle* h, const void* d_in, int elem_size, int B, int rv, int E, void* d_e, void* stream)
{
    td::RmParams p;
    if (const int rc = rm_launch_params("td_rate_match", h, d_in, d_e, B, rv, E, p)) return rc;
    if (elem_size != 1 && elem_size != 4 && elem_size != 8)
        return fail(TD_EINVAL, "td_rate_match: elem_size must be 1, 4 or 8 bytes");
    if (B == 0) return TD_OK;
    if (!td::launch_rate_match) return fail(TD_EHIP, "td_rate_match: this build has no td_ratematch.hip");
    TD_HIP(hipSetDevice(h->p.device));
    TD_HIP(td::launch_rate_match(p, d_in, elem_size, d_e, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_rate_dematch(td_handle* h, const void* d_e, int B, int rv, int E, void* d_llr, int accumulate, void* stream)
{
    td::RmParams p;
    if (const int rc = rm_launch_params("td_rate_dematch", h, d_e, d_llr, B, rv, E, p)) return rc;
    if (B == 0) return TD_OK;
    if (!td::launch_rate_dematch<double> || !td::launch_rate_dematch<float>)
        return fail(TD_EHIP, "td_rate_dematch: this build has no td_ratematch.hip");
    TD_HIP(hipSetDevice(h->p.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (is_fixed(h)) {
        if (!td::launch_fixed_dematch) return fail(TD_EHIP, "td_rate_dematch: this build has no td_fixed.hip");
        TD_HIP(td::launch_fixed_dematch(p, static_cast<const int8_t*>(d_e), static_cast<int8_t*>(d_llr), accumulate, st));
    } else if (h->p.precision == TD_F64)
        TD_HIP(td::launch_rate_dematch<double>(p, static_cast<const double*>(d_e), static_cast<double*>(d_llr), accumulate, st));
    else
        TD_HIP(td::launch_rate_dematch<float>(p, static_cast<const float*>(d_e), static_cast<float*>(d_llr), accumulate, st));
    return TD_OK;
}

int td_demod_dematch(td_handle* h, const double* d_yi, const double* d_yq, int B, int rv, int E, int modulation,
                     double Kf, double steps_per_unit, void* d_llr, int accumulate, void* stream)
{
    td::RmParams p;
    if (const int rc = rm_launch_params("td_demod_dematch", h, d_yi, d_llr, B, rv, E, p)) return rc;
    if (!d_yq) return fail(TD_EINVAL, "td_demod_dematch: null argument");
    const int M = modulation;
    if (M != 1 && M != 2 && M != 3 && M != 4 && M != 6)
        return fail(TD_EINVAL, "td_demod_dematch: modulation must be 1, 2, 3, 4 or 6");
    if (E % M) return fail(TD_EINVAL, "td_demod_dematch: E = " + std::to_string(E) + " is not a whole number of symbols");
    if (is_fixed(h) && !steps_ok(steps_per_unit))
        return fail(TD_EINVAL, "td_demod_dematch: steps_per_unit must be finite and positive");
    if (B == 0) return TD_OK;
    if (!td::launch_demod_dematch<double> || !td::launch_demod_dematch<float> || !td::launch_demod_dematch<int8_t>)
        return fail(TD_EHIP, "td_demod_dematch: this build has no td_ratematch.hip");
    TD_HIP(hipSetDevice(h->p.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (is_fixed(h))
        TD_HIP(td::launch_demod_dematch<int8_t>(p, d_yi, d_yq, M, Kf, steps_per_unit, static_cast<int8_t*>(d_llr), accumulate, st));
    else if (h->p.precision == TD_F64)
        TD_HIP(td::launch_demod_dematch<double>(p, d_yi, d_yq, M, Kf, steps_per_unit, static_cast<double*>(d_llr), accumulate, st));
    else
        TD_HIP(td::launch_demod_dematch<float>(p, d_yi, d_yq, M, Kf, steps_per_unit, static_cast<float*>(d_llr), accumulate, st));
    return TD_OK;
}

namespace {

// td_rm_index_host and td_rm_index_host_filler
int rm_index(const char* who, int K, int Ncb, int F, int rv, int E, int32_t* idx)
{
    const std::string w(who);
    if (!idx) return fail(TD_EINVAL, w + ": null idx");
    if (rv < 0 || rv > 3) return fail(TD_EINVAL, w + ": rv must be in 0..3");
    if (E < 1) return fail(TD_EINVAL, w + ": E must be at least 1");
    td::RmTables t;
    if (!td::rm_build(K, Ncb, t, F))
        return fail(TD_EINVAL, w + ": K must be in [1, 10000], Ncb 0 or in [Kpi, Kw], F in [0, 63] and below K");
    size_t j = (size_t)t.c0[rv];
    for (int k = 0; k < E; ++k) {
        idx[k] = t.pos[j];
        if (++j == (size_t)t.Nnn) j = 0;
    }
    return TD_OK;
}

}  // namespace

int td_rm_index_host(int K, int Ncb, int rv, int E, int32_t* idx)
{
    return rm_index("td_rm_index_host", K, Ncb, 0, rv, E, idx);
}

int td_rm_index_host_filler(int K, int Ncb, int F, int rv, int E, int32_t* idx)
{
    return rm_index("td_rm_index_host_filler", K, Ncb, F, rv, E, idx);
}


int td_encode_device(td_handle* h, const uint8_t* d_info, int B, uint8_t* d_coded, void* stream)
{
    if (!h) return fail(TD_EINVAL, "td_encode_device: null handle");
    if (!d_info || !d_coded) return fail(TD_EINVAL, "td_encode_device: null pointer");
    if (B < 0) return fail(TD_EINVAL, "td_encode_device: negative B");
    if (B == 0) return TD_OK;
    if (!td::launch_encode) return fail(TD_EHIP, "td_encode_device: this build has no td_encode.hip");
    TD_HIP(hipSetDevice(h->p.device));
    const td::EncParams p{h->p.K, B, h->d_pi, d_info, d_coded, h->role_cus};
    TD_HIP(td::launch_encode(p, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_crc_set(td_handle* h, uint32_t poly)
{
    if (!h) return fail(TD_EINVAL, "td_crc_set: null handle");
    if (poly == 0 || (poly & ~td::kCrc24Mask))
        return fail(TD_EINVAL, "td_crc_set: poly must be the 24 low-order coefficients, non-zero");
    if (h->p.K <= 24) return fail(TD_EINVAL, "td_crc_set: a CRC-24 needs K > 24");
    TD_HIP(hipSetDevice(h->p.device));
    if (!h->d_crc_tab && hipMalloc(reinterpret_cast<void**>(&h->d_crc_tab), (size_t)h->p.K * sizeof(uint32_t)) != hipSuccess) {
        h->d_crc_tab = nullptr;
        return fail(TD_ENOMEM, "td_crc_set: hipMalloc failed");
    }
    std::vector<uint32_t> tab((size_t)h->p.K);
    td::crc24_syndromes(h->p.K, poly, tab.data());
    TD_HIP(hipDeviceSynchronize());   // launches that still read the previous table
    TD_HIP(hipMemcpy(h->d_crc_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->crc_tab_poly = poly;
    return TD_OK;
}

namespace {

// the argument checks td_crc_attach and td_crc_check share
int crc_launch_params(const char* who, td_handle* h, const void* a, const void* b, int B, td::CrcParams& p)
{
    const std::string w(who);
    if (!h) return fail(TD_EINVAL, w + ": null handle");
    if (!a || !b) return fail(TD_EINVAL, w + ": null pointer");
    if (B < 0) return fail(TD_EINVAL, w + ": negative B");
    if (!h->crc_tab_poly) return fail(TD_EINVAL, w + ": call td_crc_set first");
    p = td::CrcParams{h->p.K, B, h->d_crc_tab, h->role_cus};
    return TD_OK;
}

}  // namespace

int td_crc_attach(td_handle* h, uint8_t* d_bits, int B, void* stream)
{
    td::CrcParams p;
    if (const int rc = crc_launch_params("td_crc_attach", h, d_bits, d_bits, B, p)) return rc;
    if (B == 0) return TD_OK;
    if (!td::launch_crc_attach) return fail(TD_EHIP, "td_crc_attach: this build has no td_encode.hip");
    TD_HIP(hipSetDevice(h->p.device));
    TD_HIP(td::launch_crc_attach(p, d_bits, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_crc_check(td_handle* h, const uint8_t* d_bits, int B, uint32_t* d_rem, void* stream)
{
    td::CrcParams p;
    if (const int rc = crc_launch_params("td_crc_check", h, d_bits, d_rem, B, p)) return rc;
    if (B == 0) return TD_OK;
    if (!td::launch_crc_check) return fail(TD_EHIP, "td_crc_check: this build has no td_encode.hip");
    TD_HIP(hipSetDevice(h->p.device));
    TD_HIP(td::launch_crc_check(p, d_bits, d_rem, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

}  // extern "C"

// ---- transport blocks (td_tb_core.h, td_tb.h) ----

// Owns only tables.  Classes of code block: [K_plus?][with the filler's <NULL>s?]; the filler class exists
// for the size of block 0 when F > 0.
struct td_tb {
    td_tb_params p{};
    td::tb::Plan plan{};
    int cus = 0;
    uint32_t* d_syn_a = nullptr;
    uint32_t* d_syn_b[2] = {nullptr, nullptr};
    struct Class {
        bool set = false;
        int K = 0, R = 0, ND = 0, Nnn = 0, c0[4] = {};
        int32_t* d_rank = nullptr;
        int32_t* d_pos = nullptr;
    } cls[2][2];
};

namespace {

// finite and <= 0, judged on the bits (steps_ok's reason)
bool filler_ok(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return ((u >> 52) & 0x7FF) != 0x7FF && ((u >> 63) != 0 || (u << 1) == 0);
}

// the filler's int8: td_llr_convert's at one step a unit; x is finite and <= 0
int8_t filler_i8(double x)
{
    const double r = std::rint(x);
    return (int8_t)(int)(r < -127.0 ? -127.0 : r);
}

template <typename T>
hipError_t upload(T*& d, const std::vector<T>& v)
{
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(T) * v.size());
    if (e != hipSuccess) {
        d = nullptr;
        return e;
    }
    return hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

void to_c(const td::tb::Plan& p, td_tb_plan* o)
{
    *o = td_tb_plan{p.A, p.B, p.L, p.C, p.K_plus, p.K_minus, p.C_plus, p.C_minus, p.F};
}

// one launch's view; rv < 0: the calls that read no rate-matching table
td::TbTables tb_view(const td_tb* t, int rv)
{
    td::TbTables v{};
    v.plan = t->plan;
    v.syn_a = t->d_syn_a;
    v.syn_b[0] = t->d_syn_b[0], v.syn_b[1] = t->d_syn_b[1];
    v.cus = t->cus;
    if (rv >= 0)
        for (int s = 0; s < 2; ++s)
            for (int f = 0; f < 2; ++f) {
                const td_tb::Class& c = t->cls[s][f];
                if (c.set) v.cls[s][f] = td::TbRmClass{c.K, c.R, c.ND, c.Nnn, c.c0[rv], c.d_rank, c.d_pos};
            }
    return v;
}

// the checks the four device calls share: the handle, N, and a pointer for every non-empty class
int tb_args(const char* who, const td_tb* t, int N, const void* minus, const void* plus)
{
    const std::string w(who);
    if (!t) return fail(TD_EINVAL, w + ": null td_tb");
    if (N < 0) return fail(TD_EINVAL, w + ": negative N");
    if (!plus || (t->plan.C_minus > 0 && !minus)) return fail(TD_EINVAL, w + ": null pointer for a non-empty class of blocks");
    return TD_OK;
}

int tb_rm_args(const char* who, const td_tb* t, int rv, long long G, int NlQm, td::tb::RmSizes& sz)
{
    const std::string w(who);
    if (rv < 0 || rv > 3) return fail(TD_EINVAL, w + ": rv must be in 0..3");
    if (!td::tb::rm_sizes(t->plan.C, G, NlQm, sz))
        return fail(TD_EINVAL, w + ": G must be a multiple of NlQm >= 1 below 2^31 with G / NlQm >= C");
    return TD_OK;
}

}  // namespace

extern "C" {

int td_tb_plan_host(int A, td_tb_plan* out)
{
    if (!out) return fail(TD_EINVAL, "td_tb_plan_host: null pointer");
    td::tb::Plan p;
    if (!td::tb::plan(A, p)) return fail(TD_EINVAL, "td_tb_plan_host: A must be in [1, 1048576]");
    to_c(p, out);
    return TD_OK;
}

int td_tb_rm_sizes_host(const td_tb_plan* p, long long G, int NlQm, int* E_lo, int* E_hi, int* n_lo)
{
    if (!p) return fail(TD_EINVAL, "td_tb_rm_sizes_host: null plan");
    td::tb::RmSizes s;
    if (!td::tb::rm_sizes(p->C, G, NlQm, s))
        return fail(TD_EINVAL, "td_tb_rm_sizes_host: G must be a multiple of NlQm >= 1 below 2^31 with G / NlQm >= C >= 1");
    if (E_lo) *E_lo = s.E_lo;
    if (E_hi) *E_hi = s.E_hi;
    if (n_lo) *n_lo = s.n_lo;
    return TD_OK;
}

int td_tb_create(td_tb** out, const td_tb_params* p)
{
    if (!out || !p) return fail(TD_EINVAL, "td_tb_create: null argument");
    *out = nullptr;
    td::tb::Plan plan;
    if (!td::tb::plan(p->A, plan)) return fail(TD_EINVAL, "td_tb_create: A must be in [1, 1048576]");
    const int Kpi_plus = 32 * ((plan.K_plus + 4 + 31) / 32);
    if (p->Ncb_cap < 0 || (p->Ncb_cap > 0 && p->Ncb_cap < Kpi_plus))
        return fail(TD_EINVAL, "td_tb_create: Ncb_cap must be 0 or at least Kpi of K_plus = " + std::to_string(Kpi_plus));
    if (!filler_ok(p->filler_llr)) return fail(TD_EINVAL, "td_tb_create: filler_llr must be finite and <= 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(TD_ENODEV, "td_tb_create: no HIP device visible");
    if (p->device < 0 || p->device >= ndev) return fail(TD_EINVAL, "td_tb_create: device ordinal out of range");
    hipDeviceProp_t prop;
    TD_HIP(hipGetDeviceProperties(&prop, p->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(TD_ENODEV, std::string("td_tb_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    TD_HIP(hipSetDevice(p->device));

    td_tb* t = new td_tb();
    t->p = *p, t->plan = plan, t->cus = prop.multiProcessorCount;
    hipError_t e;
    {
        std::vector<uint32_t> syn((size_t)plan.B);
        td::crc24_syndromes(plan.B, 0x864CFBu, syn.data());
        e = upload(t->d_syn_a, syn);
    }
    const int Ks[2] = {plan.K_minus, plan.K_plus};
    const int filler_size = plan.C_minus > 0 ? 0 : 1;   // block 0's
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        if (s == 0 && plan.C_minus == 0) continue;
        if (plan.L) {
            std::vector<uint32_t> syn((size_t)Ks[s]);
            td::crc24_syndromes(Ks[s], 0x800063u, syn.data());
            e = upload(t->d_syn_b[s], syn);
        }
        for (int f = 0; f < 2 && e == hipSuccess; ++f) {
            if (f == 1 && (plan.F == 0 || s != filler_size)) continue;
            td::RmTables rm;
            const int Kw = 3 * 32 * ((Ks[s] + 4 + 31) / 32);
            if (!td::rm_build(Ks[s], p->Ncb_cap == 0 || p->Ncb_cap > Kw ? 0 : p->Ncb_cap, rm, f ? plan.F : 0)) {
                td_tb_destroy(t);
                return fail(TD_EINVAL, "td_tb_create: no circular buffer for K = " + std::to_string(Ks[s]));
            }
            td_tb::Class& c = t->cls[s][f];
            c.K = rm.K, c.R = rm.R, c.ND = rm.ND, c.Nnn = rm.Nnn;
            for (int rv = 0; rv < 4; ++rv) c.c0[rv] = rm.c0[rv];
            e = upload(c.d_rank, rm.rank);
            if (e == hipSuccess) e = upload(c.d_pos, rm.pos);
            c.set = e == hipSuccess;
        }
    }
    if (e != hipSuccess) {
        td_tb_destroy(t);
        return e == hipErrorOutOfMemory ? fail(TD_ENOMEM, "td_tb_create: hipMalloc failed") : hip_fail(e, "td_tb_create: table upload");
    }
    *out = t;
    return TD_OK;
}

int td_tb_destroy(td_tb* t)
{
    if (!t) return TD_OK;
    (void)hipSetDevice(t->p.device);
    if (t->d_syn_a) (void)hipFree(t->d_syn_a);
    for (int s = 0; s < 2; ++s) {
        if (t->d_syn_b[s]) (void)hipFree(t->d_syn_b[s]);
        for (int f = 0; f < 2; ++f) {
            if (t->cls[s][f].d_rank) (void)hipFree(t->cls[s][f].d_rank);
            if (t->cls[s][f].d_pos) (void)hipFree(t->cls[s][f].d_pos);
        }
    }
    delete t;
    return TD_OK;
}

int td_tb_get_plan(const td_tb* t, td_tb_plan* out)
{
    if (!t || !out) return fail(TD_EINVAL, "td_tb_get_plan: null argument");
    to_c(t->plan, out);
    return TD_OK;
}

int td_tb_segment(td_tb* t, const uint8_t* d_tb, int N, uint8_t* d_cb_minus, uint8_t* d_cb_plus, void* stream)
{
    if (const int rc = tb_args("td_tb_segment", t, N, d_cb_minus, d_cb_plus)) return rc;
    if (!d_tb) return fail(TD_EINVAL, "td_tb_segment: null d_tb");
    if (N == 0) return TD_OK;
    if (!td::launch_tb_segment) return fail(TD_EHIP, "td_tb_segment: this build has no td_tb.hip");
    TD_HIP(hipSetDevice(t->p.device));
    TD_HIP(td::launch_tb_segment(tb_view(t, -1), d_tb, N, d_cb_minus, d_cb_plus, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_tb_rate_match(td_tb* t, const uint8_t* d_coded_minus, const uint8_t* d_coded_plus, int N, int rv, long long G,
                     int NlQm, uint8_t* d_f, void* stream)
{
    if (const int rc = tb_args("td_tb_rate_match", t, N, d_coded_minus, d_coded_plus)) return rc;
    if (!d_f) return fail(TD_EINVAL, "td_tb_rate_match: null d_f");
    td::tb::RmSizes sz;
    if (const int rc = tb_rm_args("td_tb_rate_match", t, rv, G, NlQm, sz)) return rc;
    if (N == 0) return TD_OK;
    if (!td::launch_tb_rate_match) return fail(TD_EHIP, "td_tb_rate_match: this build has no td_tb.hip");
    TD_HIP(hipSetDevice(t->p.device));
    TD_HIP(td::launch_tb_rate_match(tb_view(t, rv), sz, G, d_coded_minus, d_coded_plus, N, d_f, static_cast<hipStream_t>(stream)));
    return TD_OK;
}

int td_tb_rate_dematch(td_tb* t, const void* d_f, int precision, int N, int rv, long long G, int NlQm, void* d_llr_minus,
                       void* d_llr_plus, int accumulate, void* stream)
{
    if (const int rc = tb_args("td_tb_rate_dematch", t, N, d_llr_minus, d_llr_plus)) return rc;
    if (!d_f) return fail(TD_EINVAL, "td_tb_rate_dematch: null d_f");
    if (precision != TD_F64 && precision != TD_F32 && precision != TD_FIXED)
        return fail(TD_EINVAL, "td_tb_rate_dematch: precision must be TD_F64, TD_F32 or TD_FIXED");
    td::tb::RmSizes sz;
    if (const int rc = tb_rm_args("td_tb_rate_dematch", t, rv, G, NlQm, sz)) return rc;
    if (N == 0) return TD_OK;
    if (!td::launch_tb_rate_dematch<double> || !td::launch_tb_rate_dematch<float> || !td::launch_tb_rate_dematch<int8_t>)
        return fail(TD_EHIP, "td_tb_rate_dematch: this build has no td_tb.hip");
    TD_HIP(hipSetDevice(t->p.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const td::TbTables v = tb_view(t, rv);
    const double x = t->p.filler_llr;
    if (precision == TD_F64)
        TD_HIP(td::launch_tb_rate_dematch<double>(v, sz, G, static_cast<const double*>(d_f), N, static_cast<double*>(d_llr_minus),
                                                  static_cast<double*>(d_llr_plus), x, accumulate, st));
    else if (precision == TD_F32)
        TD_HIP(td::launch_tb_rate_dematch<float>(v, sz, G, static_cast<const float*>(d_f), N, static_cast<float*>(d_llr_minus),
                                                 static_cast<float*>(d_llr_plus), (float)x, accumulate, st));
    else
        TD_HIP(td::launch_tb_rate_dematch<int8_t>(v, sz, G, static_cast<const int8_t*>(d_f), N, static_cast<int8_t*>(d_llr_minus),
                                                  static_cast<int8_t*>(d_llr_plus), filler_i8(x), accumulate, st));
    return TD_OK;
}

int td_tb_demod_dematch(td_tb* t, const double* d_yi, const double* d_yq, int precision, int N, int rv, long long G,
                        int NlQm, int modulation, double Kf, double steps_per_unit, const uint32_t* d_seq,
                        void* d_llr_minus, void* d_llr_plus, int accumulate, void* stream)
{
    if (const int rc = tb_args("td_tb_demod_dematch", t, N, d_llr_minus, d_llr_plus)) return rc;
    if (!d_yi || !d_yq) return fail(TD_EINVAL, "td_tb_demod_dematch: null symbols");
    if (precision != TD_F64 && precision != TD_F32 && precision != TD_FIXED)
        return fail(TD_EINVAL, "td_tb_demod_dematch: precision must be TD_F64, TD_F32 or TD_FIXED");
    const int M = modulation;
    if (M != 1 && M != 2 && M != 3 && M != 4 && M != 6)
        return fail(TD_EINVAL, "td_tb_demod_dematch: modulation must be 1, 2, 3, 4 or 6");
    td::tb::RmSizes sz;
    if (const int rc = tb_rm_args("td_tb_demod_dematch", t, rv, G, NlQm, sz)) return rc;
    if (NlQm % M)
        return fail(TD_EINVAL, "td_tb_demod_dematch: NlQm = " + std::to_string(NlQm) + " is not a multiple of the modulation");
    if (precision == TD_FIXED && !steps_ok(steps_per_unit))
        return fail(TD_EINVAL, "td_tb_demod_dematch: steps_per_unit must be finite and positive");
    if (N == 0) return TD_OK;
    if (!td::launch_tb_demod_dematch<double> || !td::launch_tb_demod_dematch<float> || !td::launch_tb_demod_dematch<int8_t>)
        return fail(TD_EHIP, "td_tb_demod_dematch: this build has no td_tb.hip");
    TD_HIP(hipSetDevice(t->p.device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const td::TbTables v = tb_view(t, rv);
    const td::TbDemodArgs a{d_yi, d_yq, d_seq, M, Kf, steps_per_unit};
    const double x = t->p.filler_llr;
    if (precision == TD_F64)
        TD_HIP(td::launch_tb_demod_dematch<double>(v, sz, G, a, N, static_cast<double*>(d_llr_minus),
                                                   static_cast<double*>(d_llr_plus), x, accumulate, st));
    else if (precision == TD_F32)
        TD_HIP(td::launch_tb_demod_dematch<float>(v, sz, G, a, N, static_cast<float*>(d_llr_minus),
                                                  static_cast<float*>(d_llr_plus), (float)x, accumulate, st));
    else
        TD_HIP(td::launch_tb_demod_dematch<int8_t>(v, sz, G, a, N, static_cast<int8_t*>(d_llr_minus),
                                                   static_cast<int8_t*>(d_llr_plus), filler_i8(x), accumulate, st));
    return TD_OK;
}

int td_tb_concat(td_tb* t, const uint8_t* d_bits_minus, const uint8_t* d_bits_plus, int N, uint8_t* d_tb,
                 uint32_t* d_cb_rem, uint32_t* d_tb_rem, void* stream)
{
    if (const int rc = tb_args("td_tb_concat", t, N, d_bits_minus, d_bits_plus)) return rc;
    if (!d_tb) return fail(TD_EINVAL, "td_tb_concat: null d_tb");
    if (N == 0) return TD_OK;
    if (!td::launch_tb_concat) return fail(TD_EHIP, "td_tb_concat: this build has no td_tb.hip");
    TD_HIP(hipSetDevice(t->p.device));
    TD_HIP(td::launch_tb_concat(tb_view(t, -1), d_bits_minus, d_bits_plus, N, d_tb, d_cb_rem, d_tb_rem,
                                static_cast<hipStream_t>(stream)));
    return TD_OK;
}

}  // extern "C"
