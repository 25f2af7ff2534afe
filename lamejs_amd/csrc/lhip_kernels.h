// lhip_kernels.h -- HIP builds only: the __global__ wrappers of the kb_* bodies, their grid helpers, kernel timing and the LAUNCH macros.
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// kernel launch layer
// ===========================================================================================
// Workgroups are handed to the 8 XCDs round-robin (workgroup b runs on XCD b % 8) and every XCD has its own L2.  Kernels whose
// neighbouring work items read the same data (a granule and its successor: overlapping PCM windows, the polyphase output that
// two MDCT granules share, the carried thresholds) number their items so that neighbours run on ONE XCD, back to back:
// item = (b % 8) * ceil(n / 8) + b / 8.  Launch XCD_GRID(n) workgroups; -1 = no item for this workgroup.
#define XCD_GRID(n) (8 * (((n) + 7) / 8))
static __device__ __forceinline__ int xcd_item(int b, int n) { const int it = (b & 7) * ((n + 7) >> 3) + (b >> 3); return it < n && (b >> 3) < ((n + 7) >> 3) ? it : -1; }
__global__ __launch_bounds__(64) void g_load(Tables T, Workspace W, const StreamDesc* SD, const StreamIO* IO) { kb_load(T, W, SD, IO, blockIdx.x, threadIdx.x); }
__global__ __launch_bounds__(64) void g_save(Tables T, Workspace W, const StreamDesc* SD, const StreamIO* IO) { kb_save(T, W, SD, IO, blockIdx.x, threadIdx.x); }
// psy channels chn0 .. chn0 + nch - 1 of every granule slot: (0, C) for L / R; joint stereo then runs (2, 2) for mid / side, which
// read what the L / R pass left in W.fht / W.hpf
// Waves per workgroup of the two psychoacoustic kernels, whose work item is one wave: four waves of consecutive items per workgroup (they share nothing but the
// launch; neighbouring items -- which read the same windows, twiddles and spreading rows, and overlapping PCM -- stay on one XCD, now on one CU and its L1).  Measured
// (round 6, profiles/r06_ab_waves_per_workgroup.txt): g_psyA 2.78 -> 2.59 ms, g_psyB 1.07 -> 1.01 ms per 1e5 two-channel frames (one channel 1.36 -> 1.28, 0.61 -> 0.58);
// 2 waves half of that, 8 slower than 1.  The filterbank kernels do not move and the bit packer loses 6 % (its waves end at very different times): they stay one wave per
// workgroup.  (Occupancy is not what changed: 4 - 5 resident waves per SIMD before and after -- SQ_WAVE_CYCLES counts in units of four clocks, calibrated on g_quant's known 4.)
#ifndef LHIP_WPB
#define LHIP_WPB 4
#endif
enum { WPB = LHIP_WPB };
#define XCD_GRID_W(n) XCD_GRID(((n) + WPB - 1) / WPB)
static __device__ __forceinline__ int xcd_wave_item(int n, int* lane) {
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    *lane = (int)(threadIdx.x & 63);
    const int g = xcd_item(blockIdx.x, (n + WPB - 1) / WPB);
    const int it = g * WPB + wv;
    return (g >= 0 && it < n) ? it : -1;
}
#define WAVE_LDS(TYPE, NAME) __shared__ TYPE NAME##_[WPB]; TYPE& NAME = NAME##_[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))]
// PART 0: all of kb_psyA in one launch.  A lazy batch (BatchPlan::psy_lazy) launches PART 1 (high-pass + sub-block peaks: all the scans need), the scans,
// and then PART 2 in its lazy form, which knows the block types and leaves out the short-block side nobody reads.
template <int PART> __global__ __launch_bounds__(64 * WPB) void g_psyA(Tables T, Workspace W, const StreamDesc* SD, const StreamIO* IO, int chn0, int nch) {
    WAVE_LDS(PsyALds, L);
    int lane;
    const int it = xcd_wave_item(W.ngslots * nch, &lane);
    if (it >= 0) kb_psyA<PART, PART == 2>(T, W, SD, IO, it / nch, chn0 + it % nch, lane, L);
}
__global__ __launch_bounds__(256) void g_prep(Tables T, Workspace W, const StreamDesc* SD, const StreamIO* IO, int nstreams) {
    kb_prep(T, W, SD, IO, nstreams, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}
__global__ __launch_bounds__(256) void g_count_rejected(const StreamIO* IO, int nstreams, int C, float limit, unsigned long long* ctr) {
    const unsigned long long bad = kb_count_rejected(IO, nstreams, C, limit, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
    if (bad) atomicAdd(ctr, bad);
}
__global__ __launch_bounds__(64) void g_scan_raw(Tables T, Workspace W, const StreamDesc* SD, int ngs) { const int g = blockIdx.x * 64 + threadIdx.x; if (g < ngs) kb_scan_raw(T, W, SD, g); }
__global__ __launch_bounds__(64) void g_scan_attack(Tables T, Workspace W, const StreamDesc* SD, int ngs) { const int g = blockIdx.x * 64 + threadIdx.x; if (g < ngs) kb_scan_attack(T, W, SD, g); }
__global__ __launch_bounds__(64) void g_scan_blocktype(Tables T, Workspace W, const StreamDesc* SD, int ngs) { const int g = blockIdx.x * 64 + threadIdx.x; if (g < ngs) kb_scan_blocktype(T, W, SD, g); }
__global__ __launch_bounds__(ATH_NT) void g_scan_ath(Tables T, Workspace W, const StreamDesc* SD) { __shared__ AthLds L; kb_scan_ath(T, W, SD, blockIdx.x, threadIdx.x, L); }
template <int NCH, int LAZY> __global__ __launch_bounds__(64 * WPB) void g_psyB(Tables T, PowBase pb, Workspace W, const StreamDesc* SD, int par) {
    WAVE_LDS(PsyBLdsT<NCH>, L);
    int lane;
    const int it = xcd_wave_item(W.ngslots, &lane);
    if (it >= 0) kb_psyB<NCH, LAZY>(T, pb, W, SD, it, lane, L, par);
}
__global__ __launch_bounds__(64, 4) void g_poly(Tables T, Workspace W, const StreamDesc* SD, const StreamIO* IO, int nitems) {
    __shared__ PolyLds L;
    const int it = xcd_item(blockIdx.x, (nitems + POLY_PER_WAVE - 1) / POLY_PER_WAVE);
    if (it >= 0) kb_polyphase(T, W, SD, IO, it, nitems, threadIdx.x, L);
}
__global__ __launch_bounds__(64) void g_mdct(Tables T, Workspace W, const StreamDesc* SD) {
    __shared__ MdctLds L;
    const int it = xcd_item(blockIdx.x, W.ngslots);
    if (it >= 0) kb_mdct(T, W, SD, it, threadIdx.x, L);
}
// quantization kernels: 8 waves (= 8 frames) per workgroup share one copy of the lookup tables in LDS
#ifdef LHIP_PHASE_PROF
enum { QWAVES = 7 };      /* the profiling counters take LDS: 7 waves keep two workgroups per CU */
#else
enum { QWAVES = 8 };
#endif
// (two workgroups must fit in the 160 KB of LDS of a CU, or occupancy silently halves: static_assert in g_quant)
#ifndef LHIP_QOCC
#define LHIP_QOCC 4     /* waves per SIMD the quantization kernels are register-budgeted for */
#endif
// Persistent workgroups: each wave draws the next frame slot from a global dispenser until none is left, so a
// workgroup never idles on its slowest frame (frames differ a lot in the number of quantization rounds they need) and
// the table copy in LDS is made once per workgroup, not once per 8 frames.
LHIP_DEV int next_frame_slot(int32_t* ctr) {
    int v = 0;
    if ((threadIdx.x & 63) == 0) v = atomicAdd(ctr, 1);
    return __builtin_amdgcn_readfirstlane(v);
}
struct QArgs { Tables T; PowBase pb; Workspace W; const StreamDesc* SD; int chain, nfs, ctr; };
#define LHIP_QUANT_BOUNDS __launch_bounds__(64 * QWAVES, LHIP_QOCC)
// SKIP: the batch kernels exist in two forms -- with the search's dead last round of pairs skipped where the granule-channel's spectrum allows it (GI::tail0,
// k_quant_count.h), and without any of that code: the host launches the second where the configuration's lowpass leaves lines above 512 in every long block (320 kbps),
// which would only carry the first form's larger code (measured: + 1 % of such a step)
template <int SKIP> __global__ LHIP_QUANT_BOUNDS void g_quant(QArgs a_unused) {
    __shared__ QuantTabs Q;
    __shared__ QuantLds L[QWAVES];
    __shared__ TailShare TS;
#ifndef LHIP_PHASE_PROF
    static_assert(QWAVES * sizeof(QuantLds) + sizeof(QuantTabs) + sizeof(TailShare) <= 80 * 1024, "g_quant: LDS budget for 2 workgroups per CU exceeded");
#endif
    const QArgs* A = (const QArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    q_copy_tabs(A->T, Q, threadIdx.x, 64 * QWAVES);
    if (threadIdx.x == 0) TS.drawing = QWAVES;
    if (threadIdx.x < QWAVES) TS.offer[threadIdx.x].state = 0;
    const bool tail_help_on = A->T.channels_out == 2;       // a one-channel frame is one chain: nothing to offer
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef LHIP_PHASE_PROF
    L[wv].prof[threadIdx.x & 63] = 0;                 // per-wave cycle sums, flushed once at the end (a flush per frame would
#endif                                                // itself congest the memory pipeline it is trying to observe)
#if defined(LHIP_PHASE_PROF) || defined(LHIP_WAVE_TIMES)
    const unsigned long long wave_t0_ = wall_clock64();
#endif
    int hint[3] = {-1, -1, -1};                       // stream and bin-search results of this wave's previous frame (kb_quant: speculation seed)
    for (;;) {
        const int fslot = next_frame_slot(A->W.work_ctr + A->ctr);
        if (fslot >= A->nfs) break;
        // the speculative pass (chain == 0): the frame program with the second channel of every granule on offer to the workgroup's idle waves
        // (k_quant_tail.h); with the reservoir the frames are a chain and this kernel is not launched (g_resv_stream)
        kb_quant_th<SKIP>(A->T, A->pb, A->W, A->SD, fslot, threadIdx.x & 63, L[wv], Q, hint, TS, wv);
        hint[0] = __builtin_amdgcn_readfirstlane(hint[0]); hint[1] = __builtin_amdgcn_readfirstlane(hint[1]); hint[2] = __builtin_amdgcn_readfirstlane(hint[2]);
    }
    // the dispenser is empty: stay and take the second channels that this workgroup's waves still have ahead of them
    if (tail_help_on) tail_help<SKIP>(A->T, A->pb, A->W, A->SD, threadIdx.x & 63, L, wv, QWAVES, Q, TS);
#ifdef LHIP_PHASE_PROF
    atomicAdd((unsigned long long*)A->W.prof + (threadIdx.x & 63), (unsigned long long)L[wv].prof[threadIdx.x & 63]);
#endif
#if defined(LHIP_PHASE_PROF) || defined(LHIP_WAVE_TIMES)
    {
        const int wid = blockIdx.x * QWAVES + wv;
        if ((threadIdx.x & 63) == 0 && wid < 8192) { A->W.prof[64 + 2 * wid] = wave_t0_; A->W.prof[64 + 2 * wid + 1] = wall_clock64(); }
    }
#endif
}
// Latency path for small stereo batches: one workgroup of two waves per frame, one wave per channel (kb_quant<1>).  A single
// frame is one wave's serially dependent search; with fewer frames than SIMDs the chip is idle anyway, so the two channels
// of a granule -- independent given the granule's bit budget -- run side by side.
template <int SKIP> __global__ __launch_bounds__(128, LHIP_QOCC) void g_quant_pair(QArgs a_unused) {
    __shared__ QuantTabs Q;
    __shared__ QuantLds L[2];
    __shared__ int mbox[4];
    const QArgs* A = (const QArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    q_copy_tabs(A->T, Q, threadIdx.x, 128);
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    kb_quant<1, 0, SKIP>(A->T, A->pb, A->W, A->SD, blockIdx.x, A->chain, threadIdx.x & 63, L[wv], Q, wv, mbox);
}
// Fast table sets (quality 7): the speculative pass as the bin search alone (k_quant_fast.h), persistent like g_quant.  PAIR == 1 (two channels): the waves
// 2p, 2p + 1 of a workgroup are a pair -- wave 2p draws the pair's frame slots, each wave quantizes one channel; pairs never wait for each other.  PAIR == 0
// (one channel): every wave draws its own frames.  The grid is what the device holds of THIS kernel (run_pipeline: occupancy query), not 2 x CUs.
enum { QF_WAVES = 8 };
template <int PAIR, int SKIP> __global__ __launch_bounds__(64 * QF_WAVES, LHIP_QOCC) void g_quant_fast(QArgs a_unused) {
    __shared__ QuantTabs Q;
    __shared__ QuantLds L[QF_WAVES];
    __shared__ FastPair FP[QF_WAVES / 2];
#ifndef LHIP_PHASE_PROF         // (the profiling build's QuantLds carries the phase counters: one workgroup of this kernel per CU there, and its phases are not profiled)
    static_assert(QF_WAVES * sizeof(QuantLds) + sizeof(QuantTabs) + sizeof(FP) <= 80 * 1024, "g_quant_fast: LDS budget for 2 workgroups per CU exceeded");
#endif
    static_assert(sizeof(FP) / sizeof(int) <= 64 * QF_WAVES, "the pair records are zeroed by one store per thread");
    const QArgs* A = (const QArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    q_copy_tabs(A->T, Q, threadIdx.x, 64 * QF_WAVES);
    if (threadIdx.x < sizeof(FP) / sizeof(int)) ((int*)FP)[threadIdx.x] = 0;
    __syncthreads();
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int hint[3] = {-1, -1, -1};                       // stream and bin-search results of this wave's previous frame (kb_quant_fast: speculation seed)
    for (int round = 1;; round++) {
        int fslot;
        if constexpr (PAIR != 0) {
            FastPair& fp = FP[wv >> 1];
            if ((wv & 1) == 0) { fslot = next_frame_slot(A->W.work_ctr + A->ctr); fast_pair_publish_slot(fp, round, fslot, lane); }
            else fslot = fast_pair_await_slot(fp, round, lane);
            if (fslot >= A->nfs) break;
            kb_quant_fast<1, SKIP>(A->T, A->pb, A->W, A->SD, fslot, lane, L[wv], Q, hint, wv & 1, &fp, round);
        } else {
            fslot = next_frame_slot(A->W.work_ctr + A->ctr);
            if (fslot >= A->nfs) break;
            kb_quant_fast<0, SKIP>(A->T, A->pb, A->W, A->SD, fslot, lane, L[wv], Q, hint);
        }
        hint[0] = __builtin_amdgcn_readfirstlane(hint[0]); hint[1] = __builtin_amdgcn_readfirstlane(hint[1]); hint[2] = __builtin_amdgcn_readfirstlane(hint[2]);
    }
}
__global__ __launch_bounds__(256) void g_validate_fast(Tables T, Workspace W, const StreamDesc* SD, int nfs) {
    __shared__ ValidateShare S;
    const int t = blockIdx.x * 256 + threadIdx.x, fslot = t >> 2;        // four lanes per frame slot (kb_validate_fast_quad)
    kb_validate_fast_quad(T, W, SD, fslot < nfs ? fslot : 0, t & 3, fslot < nfs, S);
}
// ---- seed-chain validation + repair without the host (persistent, grid barriers) ------------------------------------------
// One launch replaces the host's loop "validate -> read the flagged count back -> repair -> ...": every workgroup walks the same
// phases, separated by grid barriers, until a validation pass flags nothing.  Counters per iteration live in two parity slots of
// W.nflagged (zeroed for the next-but-one iteration by workgroup 0); the verdicts of all waves are the same because they read
// the counters after the barrier.  Launched cooperatively when the grid has more than one workgroup (co-residency is what a grid
// barrier needs); a single workgroup (batches of up to 64 frames) needs no cross-workgroup barrier at all.
enum { FX_NFLAG = 0, FX_NSLOW = 1, FX_WORK_REPAIR = 2, FX_WORK_SLOW = 3, FX_PARITY_STRIDE = 8, FX_BAR = 24, FX_STATS = 32 };
LHIP_DEV void grid_barrier(int32_t* bar, int nblocks) {
    __syncthreads();
    if (nblocks > 1 && threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                    // this workgroup's records / flags -> L2 and beyond
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int gen = __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(bar, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1) {
            __hip_atomic_store(bar, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_add(bar + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            // (bounded: 2^26 looks of ~0.12 us = 8 s -- two hundred times the longest launch this can stand behind; a grid that is not co-resident faults instead of hanging the device)
            for (int n = 0; __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen; n++) { if (n > (1 << 26)) __builtin_trap(); __builtin_amdgcn_s_sleep(4); }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                    // this CU's L1 must not serve stale records
    }
    __syncthreads();
}
// Two workgroups per CU at 128 registers (like g_quant) rather than one at 256: the phases of this kernel are spread over all its waves, and twice the
// waves beat the 128 B per lane the smaller budget spills (round 4, profiles/r04_pass9_ab_fixup_two_workgroups_per_cu.txt: validation + repair
// 0.32 -> 0.27 ms per 1e5 two-channel frames, `bursts` 2.2 -> 2.0 ms).  LHIP_FIXUP_OCC=2 builds the old shape.
#ifndef LHIP_FIXUP_OCC
#define LHIP_FIXUP_OCC 4
#endif
template <int SKIP> __global__ __launch_bounds__(64 * QWAVES, LHIP_FIXUP_OCC) void g_fixup(QArgs a_unused) {
    __shared__ QuantTabs Q;
    __shared__ QuantLds L[QWAVES];
    const QArgs* A = (const QArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int nfs = A->nfs, nblocks = gridDim.x, nthr = 64 * QWAVES;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int32_t* base = A->W.nflagged;
    bool tabs = false;
    int repaired = 0, iters = 0, failed = 0;
    for (int it = 0;; it++) {
        int32_t* ctr = base + FX_PARITY_STRIDE * (it & 1);
        Workspace W = A->W;
        W.nflagged = ctr;                                                     // kb_validate(_fast) count into this iteration's slots
        if (blockIdx.x == 0 && threadIdx.x < FX_PARITY_STRIDE) base[FX_PARITY_STRIDE * ((it + 1) & 1) + threadIdx.x] = 0;   // next iteration's
        // V: memo-only replay, one thread per frame slot.  The first pass has been made by g_validate_fast, a plain launch in front
        // of this kernel (it needs no LDS, so it runs at full occupancy; the kernel boundary orders it): in the usual case -- nothing
        // flagged -- this kernel reads two counters and ends without a single grid barrier.
        // Later passes only look at the successors of the frames the last repair phase re-quantized (stamped in W.reval): a frame's
        // verdict depends on its own records and on its predecessor's, and nothing else has changed.  (On material where most
        // replays miss the memo -- `bursts`: 98 % -- a second pass over everything cost another 4 ms.)
        if (it > 0) {
            for (int f = blockIdx.x * nthr + threadIdx.x; f < nfs; f += nblocks * nthr) kb_validate_fast(A->T, W, A->SD, f, it);
            grid_barrier(base + FX_BAR, nblocks);
        }
        // (the counters are read by every lane and asserted wave-uniform: every decision below must be scalar control flow)
        const int nslow = __builtin_amdgcn_readfirstlane(__hip_atomic_load(ctr + FX_NSLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        // Static work split over all waves of the grid (the work of these phases is rare and tiny).  NOT an atomic dispenser: a
        // `for (;;) { i = next_frame_slot(ctr); if (i >= n) break; ... }` loop nested in this iteration loop was compiled into an
        // exec-masked loop whose first-active-lane read of the dispensed index span forever on hardware (seen on ROCm 7.2, gfx950).
        const int gw = blockIdx.x * QWAVES + wv, nw = nblocks * QWAVES;
        if (nslow > 0) {                                                      // frames whose replay asked for a gain never evaluated
            if (!tabs) { q_copy_tabs(A->T, Q, threadIdx.x, nthr); __syncthreads(); tabs = true; }
            for (int i = gw; i < nslow; i += nw)
                kb_validate<SKIP>(A->T, A->pb, W, A->SD, __builtin_amdgcn_readfirstlane(W.slow_list[i]), lane, L[wv], Q);
            grid_barrier(base + FX_BAR, nblocks);
        }
        const int nflag = __builtin_amdgcn_readfirstlane(__hip_atomic_load(ctr + FX_NFLAG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (nflag == 0) break;
        repaired += nflag; iters++;
        if (iters > nfs + 2) { failed = 1; break; }                           // cannot happen: every pass finalises at least the first flagged frame
        // R: re-quantize the flagged frames with the chain-implied seeds.  Wave gw owns the frame slots congruent to gw modulo the
        // number of waves (lane = every nw-th slot): flagged frames come in runs (a burst upsets the seeds of the frames after it),
        // and a frame is one wave's serial search of 1-2 ms, so a run must land on different waves -- owning 64 CONSECUTIVE slots
        // made one wave re-quantize a whole run back to back (8.7 ms for 49 frames on the `bursts` material).
        if (!tabs) { q_copy_tabs(A->T, Q, threadIdx.x, nthr); __syncthreads(); tabs = true; }
        for (int b0 = gw; b0 < nfs; b0 += 64 * nw) {
            int flagged = 0;
            const int f = b0 + nw * lane;
            if (f < nfs) {
                const StreamDesc* sd = A->SD + W.fslot_stream[f];
                const int k = f - sd->fslot0 - 1;
                if (k >= 0) flagged = W.seed_flag[sd->out_slot0 + k] == 1;
            }
            uint64_t m = __ballot(flagged);
            while (m) {
                const int l = (int)__builtin_ctzll(m);
                m &= m - 1;
                const int fr = b0 + nw * l;
                kb_quant<0, 0, SKIP>(A->T, A->pb, W, A->SD, fr, 1, lane, L[wv], Q);
                if (lane == 0) {                                              // its successor (same stream) is what the next pass re-checks
                    const StreamDesc* sd = A->SD + W.fslot_stream[fr];
                    const int k = fr - sd->fslot0 - 1;
                    if (k + 1 < sd->nframes) W.reval[sd->out_slot0 + k + 1] = it + 1;
                }
            }
        }
        grid_barrier(base + FX_BAR, nblocks);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { base[FX_STATS + 0] = repaired; base[FX_STATS + 1] = iters; base[FX_STATS + 2] = failed; }
}
__global__ __launch_bounds__(64) void g_bits(Tables T, Workspace W, const StreamDesc* SD) {
    __shared__ BitsLds L;
    kb_bits(T, W, SD, blockIdx.x, threadIdx.x, L);
}
__global__ __launch_bounds__(64) void g_resv_flush(Tables T, Workspace W, const StreamDesc* SD) {
    __shared__ BitsLds L;
    if (SD[blockIdx.x].flush) kb_resv_flush(T, W, blockIdx.x, threadIdx.x, L, W.io[blockIdx.x].state->rv, W.out_bytes + blockIdx.x);
}
// the music CRC of { infoTag } streams (k_crc.h): one wave per span of a stream's bytes, then one wave per stream folds its spans.  Launched only for a
// batch of such streams, behind the last kernel that writes output bytes.
__global__ __launch_bounds__(64) void g_out_crc(const CrcDesc* D, int nstreams, uint32_t* partial) {
    const int s = crc_find_stream(D, nstreams, (int)blockIdx.x);
    kb_out_crc(D, s, (int)blockIdx.x - D[s].part0, threadIdx.x, partial);
}
// WAV sample types (k_ingest.h): one wave per tile of a stream's new samples, in front of the call's first reader; refused samples of the float types are
// counted where g_count_rejected counts those of Float32 calls
__global__ __launch_bounds__(64) void g_ingest(const IngestDesc* D, int nstreams, float limit, unsigned long long* ctr) {
    __shared__ __attribute__((aligned(16))) uint8_t L[ING_WINDOW];
    const int s = ingest_find_stream(D, nstreams, (int)blockIdx.x);
    const unsigned bad = kb_ingest(D, s, (int64_t)blockIdx.x - D[s].blk0, threadIdx.x, L, limit);
    if (ctr && bad && threadIdx.x == 0) atomicAdd(ctr, (unsigned long long)bad);
}
// ReplayGain of { replayGain } streams (k_gain.h): a lane per position of a stream's row (history ++ new samples), then a wave per 64 completed windows of a stream.
// Launched only for a batch of such streams, once the call's samples exist.
__global__ __launch_bounds__(GAIN_STAGE_NT) void g_gain_stage(Tables T, Workspace W, const StreamDesc* SD, const StreamIO* IO, const GainDesc* D, int nstreams) {
    const int s = gain_find_stream<true>(D, nstreams, (int)blockIdx.x);
    kb_gain_stage(T, W, SD, IO, D, s, (int64_t)((int)blockIdx.x - D[s].blk0) * GAIN_STAGE_NT + threadIdx.x);
}
template <int CH> __global__ __launch_bounds__(64) void g_gain(const GainDesc* D, int nstreams) {
    __shared__ float L[64 * CH * GAIN_STRIDE];
    const int s = gain_find_stream<false>(D, nstreams, (int)blockIdx.x);
    kb_gain<CH>(D, s, (int)blockIdx.x - D[s].wave0, threadIdx.x, L);
}
__global__ __launch_bounds__(64) void g_out_crc_fold(const CrcDesc* D, const uint32_t* partial, uint32_t* out) { kb_crc_fold(D, blockIdx.x, threadIdx.x, partial, out); }
#ifndef LHIP_FRAME_PIPE
#define LHIP_FRAME_PIPE 1      /* 0: the Huffman counts of the outer loop on the searching wave itself (A/B builds) */
#endif
static constexpr bool g_frame_pipe = LHIP_FRAME_PIPE != 0;
// the per-stream reservoir program (kb_resv_stage): one workgroup of RS_WAVES waves per stream
// (two waves per SIMD: 256 registers instead of the 264 an unbounded build takes -- the second workgroup per CU is what lets 512 streams
//  run side by side; the mode's throughput is streams in flight x one frame per 184 us)
__global__ __launch_bounds__(64 * RS_WAVES, 2) void g_resv_stream(QArgs a_unused) {
    __shared__ QuantTabs Q;
    __shared__ __attribute__((aligned(16))) unsigned char U[RS_WAVES][RS_LDS_PER_WAVE];
    __shared__ ResvState RV;
    __shared__ int mbox[4];
    __shared__ int32_t nout;
    __shared__ CountShare CS[2];
    const QArgs* A = (const QArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, st = blockIdx.x;
    q_copy_tabs(A->T, Q, threadIdx.x, 64 * RS_WAVES);
    static_assert(sizeof(ResvState) % 4 == 0, "the reservoir record is copied as words");
    ResvState* grv = &A->W.io[st].state->rv;
    for (int i = threadIdx.x; i < (int)(sizeof(ResvState) / 4); i += 64 * RS_WAVES) ((uint32_t*)&RV)[i] = ((const uint32_t*)grv)[i];
    if (threadIdx.x == 0) nout = 0;
    __syncthreads();
    const int F = __builtin_amdgcn_readfirstlane(A->SD[st].nframes);
    for (int k = 0; k <= F; k++)
        for (int stage = 0; stage < RS_STAGES; stage++) {
            kb_resv_stage<1>(stage, A->T, A->pb, A->W, A->SD, st, k, F, wv, lane, U[wv], Q, mbox, RV, &nout, (g_frame_pipe && A->ctr) ? CS : nullptr);     // A->ctr: the host's verdict on count helpers (run_pipeline)
            __syncthreads();
        }
    if (wv == 3 && A->SD[st].flush) kb_resv_flush(A->T, A->W, st, lane, *(BitsLds*)U[3], RV, &nout);
    __syncthreads();
    for (int i = threadIdx.x; i < (int)(sizeof(ResvState) / 4); i += 64 * RS_WAVES) ((uint32_t*)grv)[i] = ((const uint32_t*)&RV)[i];
    if (threadIdx.x == 0) A->W.out_bytes[st] = nout;
}
// one workgroup of FR_WAVES waves per stream, one frame per stream (see kb_frame_stage)
template <int RESV> __global__ __launch_bounds__(64 * FR_WAVES) void g_frame(QArgs a_unused, const StreamIO* IO) {
    __shared__ QuantTabs Q;
    __shared__ __attribute__((aligned(16))) unsigned char U[FR_WAVES][FR_LDS_PER_WAVE];
    __shared__ int mbox[12];
    __shared__ CountShare CS[2];
    const QArgs* A = (const QArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < 2) CS[threadIdx.x].state = CS_IDLE;
#if defined(LHIP_PHASE_PROF) || defined(LHIP_HANDOFF_PROF)
    if (threadIdx.x < 8) CS[0].acc[threadIdx.x] = 0;
#endif
#ifdef LHIP_PHASE_PROF
    if (blockIdx.x == 0 && threadIdx.x == 0) { A->W.prof[FRAME_PROF_BASE + FR_STAGES + 1] = wall_clock64(); A->W.prof[FRAME_PROF_BASE + FR_STAGES + 3] = __builtin_amdgcn_s_memtime(); }
#endif
    q_copy_tabs(A->T, Q, threadIdx.x, 64 * FR_WAVES);       // (first read by the quantization stage: the barriers in between order it)
    // Unrolled: every stage runs once, and as a loop the compiler hoisted the constants and addresses of ALL stage bodies in front of it and carried them across
    // the stages -- 60 to 150 values parked in scratch memory (308 - 1264 bytes of scratch per lane as the bodies grew; past ~0.5 KB the launch itself got 20 us
    // slower: the runtime allocates scratch that large afresh per dispatch).  Unrolled, g_frame<1> needs no scratch at all.
#pragma clang loop unroll(full)
    for (int stage = 0; stage < FR_STAGES; stage++) {
#ifdef LHIP_PHASE_PROF
        // profiling build (tests/tools/frame_prof.py): when every stage of stream 0's frame starts, and the quantization phases of its wave 0
        if (blockIdx.x == 0 && threadIdx.x == 0) A->W.prof[FRAME_PROF_BASE + stage] = __builtin_amdgcn_s_memtime();
        if (stage == FS_QUANT) ((QuantLds*)U[wv])->prof[lane] = 0;
#endif
        if (frame_stage_empty<RESV>(stage, A->T)) continue;
        kb_frame_stage<RESV, 1>(stage, A->T, A->pb, A->W, A->SD, IO, blockIdx.x, wv, FR_WAVES, lane, U[wv], Q, mbox, g_frame_pipe ? CS : nullptr);
#ifdef LHIP_PHASE_PROF
        // when each wave finished its part of the two stages whose work is dealt over waves (cycles after the stage's start)
        if ((stage == FS_PSYA_POLY || stage == FS_BITS_SAVE) && blockIdx.x == 0 && lane == 0)
            A->W.prof[FRAME_PROF_BASE + (stage == FS_PSYA_POLY ? 40 : 48) + wv] = __builtin_amdgcn_s_memtime() - A->W.prof[FRAME_PROF_BASE + stage];
        if (stage == FS_QUANT && blockIdx.x == 0 && wv == 0 && (lane < 22 || (lane > 28 && lane != 54))) A->W.prof[lane] = ((QuantLds*)U[wv])->prof[lane];      // (22 .. 28, 54: psyA's phases, PSY_FLUSH)
        if (stage == FS_QUANT && blockIdx.x == 0 && wv == 2 && lane < 5) {     // the count helper of wave 0: its five count phases (cycles, calls)
            A->W.prof[FRAME_PROF_BASE + 16 + lane] = ((QuantLds*)U[wv])->prof[PH_C_LOAD + lane]; A->W.prof[FRAME_PROF_BASE + 24 + lane] = ((QuantLds*)U[wv])->prof[32 + PH_C_LOAD + lane];
        }
        if (stage == FS_QUANT && blockIdx.x == 0 && wv == 0 && lane < 8) A->W.prof[FRAME_PROF_BASE + 32 + lane] = CS[0].acc[lane];      // the hand-over's legs
#endif
        __syncthreads();
    }
#ifdef LHIP_PHASE_PROF
    if (blockIdx.x == 0 && threadIdx.x == 0) { A->W.prof[FRAME_PROF_BASE + FR_STAGES] = __builtin_amdgcn_s_memtime(); A->W.prof[FRAME_PROF_BASE + FR_STAGES + 2] = wall_clock64(); }
#elif defined(LHIP_HANDOFF_PROF)
    // (tests/tools/handoff_prof.py: the legs of wave 0's hand-overs, summed over the calls of the process; the product never zeroes or reads these words)
    if (blockIdx.x == 0 && threadIdx.x < 8) atomicAdd(A->W.prof + 32 + threadIdx.x, (unsigned long long)CS[0].acc[threadIdx.x]);
#endif
}
// optional per-kernel timing with HIP events on the launch stream (bench.py roofline accounting)
enum { KT_LOAD, KT_PREP, KT_PSYA, KT_SCAN, KT_PSYB, KT_POLY, KT_MDCT, KT_QUANT, KT_VALIDATE, KT_REPAIR, KT_BITS, KT_SAVE, KT_COUNT, KT_OUT_CRC, KT_INGEST, KT_GAIN_STAGE, KT_GAIN, KT_N };
static const char* const g_kt_names[KT_N] = {"load", "prep", "psyA", "scan", "psyB", "polyphase", "mdct", "quant", "validate", "repair", "bits", "save", "count_rejected", "out_crc", "ingest", "gain_stage", "gain"};
// The switch is process-wide (bench.py turns it on for one extra, untimed step); the events of a batch belong to the calling
// thread (a batch runs entirely inside one run_batch call), the accumulators are shared by all devices and guarded by g_kt_mu.
static std::atomic<bool> g_kt_on{false};
static std::mutex g_kt_mu;
static double g_kt_ms[KT_N];
static int64_t g_kt_calls[KT_N];
struct KtPending { int id; hipEvent_t a, b; };
static thread_local std::vector<KtPending> g_kt_pending;
static void kt_begin(int id, void* st) {
    if (!g_kt_on) return;
    KtPending p; p.id = id;
    hipEventCreate(&p.a); hipEventCreate(&p.b);
    hipEventRecord(p.a, (hipStream_t)st);
    g_kt_pending.push_back(p);
}
static void kt_end(void* st) { if (g_kt_on && !g_kt_pending.empty()) hipEventRecord(g_kt_pending.back().b, (hipStream_t)st); }
static void kt_collect() {
    std::lock_guard<std::mutex> lk(g_kt_mu);
    for (auto& p : g_kt_pending) {
        float ms = 0.f;
        hipEventSynchronize(p.b);
        hipEventElapsedTime(&ms, p.a, p.b);
        g_kt_ms[p.id] += ms; g_kt_calls[p.id]++;
        hipEventDestroy(p.a); hipEventDestroy(p.b);
    }
    g_kt_pending.clear();
}
// LAMEJS_HIP_TRACE=1: synchronise after every launch and name it on stderr (locating a kernel that does not come back)
static const bool g_trace = []() { const char* e = getenv("LAMEJS_HIP_TRACE"); return e && e[0] == '1'; }();
#define TRACE_SYNC(kern, st) do { if (g_trace) { fprintf(stderr, "[lhip] %s launched...", #kern); fflush(stderr); hipError_t t_ = hipStreamSynchronize((hipStream_t)(st)); fprintf(stderr, " %s\n", hipGetErrorString(t_)); } } while (0)
#define LAUNCHB(id, kern, nblk, nthr, st, ...) do { if ((nblk) > 0) { kt_begin(id, st); hipLaunchKernelGGL(kern, dim3(nblk), dim3(nthr), 0, (hipStream_t)(st), __VA_ARGS__); kt_end(st); TRACE_SYNC(kern, st); \
    hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { set_err(std::string(#kern) + ": " + hipGetErrorString(e_)); return false; } } } while (0)
#define LAUNCH(id, kern, nblk, st, ...) do { if ((nblk) > 0) { kt_begin(id, st); hipLaunchKernelGGL(kern, dim3(nblk), dim3(64), 0, (hipStream_t)(st), __VA_ARGS__); kt_end(st); TRACE_SYNC(kern, st); \
    hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { set_err(std::string(#kern) + ": " + hipGetErrorString(e_)); return false; } } } while (0)

// lhip_create: the quantization kernels' tables gathered once into an HBM image (q_copy_tabs)
__global__ __launch_bounds__(256) void g_build_qtabs(Tables T, QuantTabs* img) { q_load_tabs(T, *img, threadIdx.x, 256); }

// Test hooks (lhip_debug_quant_probe, lhip_debug_bits_probe): the kernels g_quant_probe and g_bits_probe are compiled apart, from lhip_probe.cpp (which says why)
// into the code object lhip_quant_probe.co beside this library; it is loaded per device on first use and launched through the module interface.  Returns "" or
// what went wrong; a library without the file beside it (the profiling and experiment builds of tools/) has no probe, and says so.
static std::string probe_launch_kernel(int phys_device, const char* kernel, void* arg, int grid, int block, void* stream) {
    static std::mutex mu;
    static std::map<int, hipModule_t> loaded;
    static std::map<std::pair<int, std::string>, hipFunction_t> fns;
    std::lock_guard<std::mutex> lk(mu);
    auto fit = fns.find({phys_device, kernel});
    if (fit == fns.end()) {
        Dl_info di;
        if (!dladdr((const void*)&lhip_version, &di) || !di.dli_fname) return "cannot find the library's own path";
        std::string path(di.dli_fname);
        const size_t cut = path.rfind('/');
        path = (cut == std::string::npos ? std::string() : path.substr(0, cut + 1)) + "lhip_quant_probe.co";
        auto it = loaded.find(phys_device);
        if (it == loaded.end()) {
            hipModule_t mod = nullptr;
            const hipError_t e = hipModuleLoad(&mod, path.c_str());
            if (e != hipSuccess) return path + ": " + hipGetErrorString(e);
            it = loaded.emplace(phys_device, mod).first;
        }
        hipFunction_t fn = nullptr;
        const hipError_t e = hipModuleGetFunction(&fn, it->second, kernel);
        if (e != hipSuccess) return path + ": " + kernel + ": " + hipGetErrorString(e);
        fit = fns.emplace(std::make_pair(phys_device, std::string(kernel)), fn).first;
    }
    void* params[] = {arg};
    const hipError_t e = hipModuleLaunchKernel(fit->second, (unsigned)grid, 1, 1, (unsigned)block, 1, 1, 0, (hipStream_t)stream, params, nullptr);
    return e != hipSuccess ? std::string(hipGetErrorString(e)) : std::string();
}
static std::string probe_launch(int phys_device, const ProbeArgs& a, void* stream) {
    ProbeArgs arg = a;
    return probe_launch_kernel(phys_device, "g_quant_probe", &arg, a.grid, 64, stream);
}
static std::string bits_probe_launch(int phys_device, const BitsProbeArgs& a, void* stream) {
    BitsProbeArgs arg = a;
    return probe_launch_kernel(phys_device, "g_bits_probe", &arg, a.grid, a.form == 0 ? 64 : 64 * a.T.mode_gr * a.T.channels_out, stream);
}
