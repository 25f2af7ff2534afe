// k_quant_prof.h -- the observation scaffolding of the quantization search and nothing that computes: the phase and hand-over profiling macros
// (PH_*, HO_*: empty unless a profiling build defines LHIP_PHASE_PROF / LHIP_HANDOFF_PROF) and the counters the host simulations keep
// (LHIP_ROUND_COUNT, LHIP_NOISE_LINES_COUNT, LHIP_PIPE_COUNT, LHIP_SS).  The product library compiles every one of them to nothing.
#pragma once
#include "lhip_defs.h"
namespace lhip {
// optional phase profiling (build with -DLHIP_PHASE_PROF; never in the product library)
#if defined(LHIP_PHASE_PROF) && !defined(LHIP_HOSTSIM)
#define PH_BEGIN() const unsigned long long ph_t0_ = __builtin_amdgcn_s_memtime()
#define PH_END(L, id) do { if (lane == 0) { (L).prof[id] += (unsigned int)(__builtin_amdgcn_s_memtime() - ph_t0_); (L).prof[32 + id] += 1; } } while (0)
#define PH_MARK(L, id, t) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); if (lane == 0) { (L).prof[id] += (unsigned int)(n_ - (t)); (L).prof[32 + id] += 1; } (t) = n_; } while (0)
#define PH_NOW() __builtin_amdgcn_s_memtime()
#else
#define PH_BEGIN() do {} while (0)
#define PH_END(L, id) do {} while (0)
#define PH_MARK(L, id, t) do {} while (0)
#define PH_NOW() 0ull
#endif
enum { PH_INIT, PH_XRPOW, PH_XMIN, PH_QUANTIZE, PH_COUNT, PH_NOISE, PH_BALANCE, PH_SFSTORE, PH_HUFFDIV, PH_PUBLISH, PH_COPY, PH_TOTAL,
       PH_C_LOAD, PH_C_QUADS, PH_C_MAX, PH_C_SUMS, PH_C_FIN, PH_N_WALK, PH_N_TERMS, PH_N_SUMS, PH_Q_MASK, PH_Q_LINES, PH_N, PH_DRAIN = 29 /* 22..28 belong to psyA's stamps */,
       PH_N_LINES = 30, PH_N_FOLD = 31 /* calc_noise: per-line terms / systolic fold; PH_N_TERMS is then the per-band part */ };

#if defined(LHIP_HOSTSIM)
// how many evaluations (quantize + count) ran with the short and with the full round count: lhip_debug_read(10), for the tests that must
// see both forms at work
struct RoundStats { long head = 0, full = 0; };      // (atomic adds: the simulations may run on several host threads)
inline RoundStats& round_stats() { static RoundStats t; return t; }
#define LHIP_ROUND_COUNT(f) do { if (lane == 0) __atomic_fetch_add(&round_stats().f, 1L, __ATOMIC_RELAXED); } while (0)
#else
#define LHIP_ROUND_COUNT(f) do { } while (0)
#endif

#if defined(LHIP_HOSTSIM)
// how many calc_noise calls ran with 7, with 9 and with 3 lines per lane: lhip_debug_read(12), for the tests that must see the form a configuration takes
// (the 64-lane simulation counts; the one-lane one has no lanes to share the lines among and reports zeros)
struct NoiseLineStats { long n7 = 0, n9 = 0, n3 = 0; };
inline NoiseLineStats& noise_line_stats() { static NoiseLineStats t; return t; }
#define LHIP_NOISE_LINES_COUNT(f) do { if (lane == 0) __atomic_fetch_add(&noise_line_stats().f, 1L, __ATOMIC_RELAXED); } while (0)
#else
#define LHIP_NOISE_LINES_COUNT(f) do { } while (0)
#endif

// -DLHIP_HANDOFF_PROF (without LHIP_PHASE_PROF): the production code with four clock reads per counted evaluation and fire-and-forget LDS adds --
// what the hand-over costs when nothing else is instrumented (tests/tools/handoff_prof.py).  acc: 0 owner: posted -> calc_noise finished, 1 owner: waited,
// 2 evaluations, 3 helper: request seen -> reply written, 4 helper's evaluations, 5 posted -> seen by the helper, 6 reply written -> seen by the owner
#if defined(LHIP_HANDOFF_PROF) && !defined(LHIP_PHASE_PROF)
#define HO_NOW() __builtin_amdgcn_s_memtime()
#define HO_ADD(CS_, I_, V_) do { if (lane == 0) __hip_atomic_fetch_add(&(CS_).acc[I_], (unsigned int)(V_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } while (0)
#define HO_ON 1
#else
#define HO_ON 0
#endif

#if defined(LHIP_WAVESIM)
// how often each way was taken (printed at exit with LAMEJS_PIPE_STATS=1: the simulation must exercise both)
struct PipeStats { long piped = 0, committed = 0; ~PipeStats() { if (getenv("LAMEJS_PIPE_STATS")) fprintf(stderr, "count helper: %ld evaluations counted on the helper wave, %ld of the calc_noise calls made beside them committed\n", piped, committed); } };
inline PipeStats& pipe_stats() { static PipeStats t; return t; }
#define LHIP_PIPE_COUNT(f) do { if (lane == 0) pipe_stats().f++; } while (0)
#else
#define LHIP_PIPE_COUNT(f) do { } while (0)
#endif

#if defined(LHIP_HOSTSIM)
// LAMEJS_SEARCH_STATS=1 (host simulations; tools/search_stats.py): the shape of the search per granule-channel -- evaluations of the bin search and of the
// step-up after it, and, per outer-loop round, the length of the `while (bits > huff_bits) gain++` run in front of the evaluation that fits, with how often
// PrevNoise.sfb_count1 (what the next evaluation's 0/1 shortcut is decided with) changed inside a run.  Prices evaluating the gains of a run side by side.
struct SearchStats {
    long bs[40] = {0}, bsup[40] = {0}, run[40] = {0}, run_cnt1_moved[40] = {0}, rounds = 0, evals = 0, searches = 0, run_steps = 0, run_steps_cnt1_moved = 0, run_steps_zo = 0;
    long bsdir[8][3][2] = {{{0}}};      // bin search: evaluation index (0 .. 7) x direction of the last move (0 none, 1 up, 2 down) x this evaluation's verdict (0: bits <= desired, 1: over)
    long mfail[24] = {0}, mfit[24] = {0};      // first evaluation of a round by its margin (huff_bits - the last evaluation's bits), buckets of 8 bits
    bool on = getenv("LAMEJS_SEARCH_STATS") != nullptr;
    ~SearchStats() {
        if (!on) return;
        fprintf(stderr, "search stats: %ld granule-channel searches, %ld evaluations, %ld outer-loop rounds; %ld evaluations inside gain++ runs (%ld of them with sfb_count1 moved by the evaluation before, %ld with a live 0/1 shortcut)\n", searches, evals, rounds, run_steps, run_steps_cnt1_moved, run_steps_zo);
        auto pr = [](const char* nm, const long* h) { fprintf(stderr, "  %s:", nm); for (int i = 0; i < 40; i++) if (h[i]) fprintf(stderr, " %d:%ld", i, h[i]); fprintf(stderr, "\n"); };
        pr("bin-search evaluations per search", bs); pr("step-up evaluations after it", bsup); pr("gain++ run length per outer-loop round (0 = the first evaluation fits)", run);
        pr("runs in which sfb_count1 moved, by run length", run_cnt1_moved);
        fprintf(stderr, "  bin-search evaluations, index / last move (- up down): under/over:"); for (int i = 0; i < 8; i++) for (int d = 0; d < 3; d++) if (bsdir[i][d][0] + bsdir[i][d][1]) fprintf(stderr, " %d%c:%ld/%ld", i, "-ud"[d], bsdir[i][d][0], bsdir[i][d][1]); fprintf(stderr, "\n");
        fprintf(stderr, "  first evaluation of a round, by margin huff_bits - previous bits (bucket of 8 bits: fails / fits):"); for (int i = 0; i < 24; i++) if (mfail[i] + mfit[i]) fprintf(stderr, " %d:%ld/%ld", 8 * (i - 4), mfail[i], mfit[i]); fprintf(stderr, "\n");
    }
};
inline SearchStats& search_stats() { static SearchStats t; return t; }
#define LHIP_SS(...) do { if (lane == 0 && search_stats().on) { SearchStats& ss_ = search_stats(); __VA_ARGS__; } } while (0)
#else
#define LHIP_SS(...) do { } while (0)
#endif
}  // namespace lhip
