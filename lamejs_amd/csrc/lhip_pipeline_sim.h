// lhip_pipeline_sim.h -- run_pipeline of the CPU simulations (-DLHIP_HOSTSIM: one lane; with -DLHIP_WAVESIM: 64 lanes as fibers, workgroups as
// in the kernels): the same kernel bodies in the launch order of lhip_pipeline_hip.h.  Exactly one of the two is included (lhip_batch.h).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// WAVE_RUN: one wave of a kernel body.  Scalar simulation: the body runs once with lane 0 (NL = 1); wave simulation
// (-DLHIP_WAVESIM): its 64 lanes run as fibers and meet at every wave primitive (lhip_wave.h).
#ifdef LHIP_WAVESIM
#define WAVE_RUN(...) wsim::run([&](int lane_) { __VA_ARGS__; })
#else
#define WAVE_RUN(...) do { const int lane_ = 0; __VA_ARGS__; } while (0)
#endif
// QUANT_RUN: frame slot `b` once more through the quantization, as run_pipeline chose for the batch (`pair`)
#ifdef LHIP_WAVESIM
#define QUANT_RUN(chain_) do { if (pair) wsim::run_block(2, [&](int wave_, int lane_) { kb_quant<1, 0, 1>(T, ts.pb10, W, dSD, b, chain_, lane_, LQ2[wave_], QT, wave_, mbox); }); \
                       else WAVE_RUN(kb_quant<0, 0, 1>(T, ts.pb10, W, dSD, b, chain_, lane_, LQ, QT)); } while (0)
#else
#define QUANT_RUN(chain_) WAVE_RUN(kb_quant<0, 0, 1>(T, ts.pb10, W, dSD, b, chain_, lane_, LQ, QT))
#endif
// g_gain_stage and g_gain over a launch's descriptors (also lhip_debug_gain_windows)
static void gain_sim_run(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, const GainDesc* D, int S, int stage_blocks, int waves) {
    static thread_local float LG[LHIP_NL * 2 * GAIN_STRIDE];
    for (int b = 0; b < stage_blocks; b++) { const int s = gain_find_stream<true>(D, S, b); for (int t = 0; t < GAIN_STAGE_NT; t++) kb_gain_stage(T, W, SD, IO, D, s, (int64_t)(b - D[s].blk0) * GAIN_STAGE_NT + t); }
    for (int b = 0; b < waves; b++) {
        const int s = gain_find_stream<false>(D, S, b);
        if (D[s].channels == 2) WAVE_RUN(kb_gain<2>(D, s, b - D[s].wave0, lane_, LG)); else WAVE_RUN(kb_gain<1>(D, s, b - D[s].wave0, lane_, LG));
    }
}
// g_quant_probe (lhip_debug_quant_probe; k_quant_probe.h): `grid` waves, each with an LDS record of its own that serves its records one after the other
enum { PROBE_SIM_WAVES = 3 };
static void quant_probe_sim_run(const Tables& T, const PowBase& pb, const ProbeIn* in, ProbeOut* out, int n, int grid) {
    static thread_local QuantLds LP[PROBE_SIM_WAVES]; static thread_local QuantTabs QT;
    q_load_tabs(T, QT, 0, 1);
    for (int b = 0; b < grid; b++)
        for (int r = b; r < n; r += grid) WAVE_RUN(kb_quant_probe(T, pb, in, out, r, lane_, LP[b], QT));
}
// g_bits_probe (lhip_debug_bits_probe; k_bits_probe.h): `grid` workgroups, each with LDS of its own that serves its frames one after the other.  form 0: kb_bits on one
// wave.  form 1: kb_bits_mw on GR * C waves -- a real workgroup in the wave simulation; the one-lane simulation, whose waves run one after the other, goes through
// kb_bits_mw's pieces (kb_bits_mw_t) (image cleared and inputs fetched | packed | copied out) wave by wave, which is what the two meeting points order.
static void bits_probe_sim_run(const Tables& T, const Workspace& W, const StreamDesc* SD, int n, int grid, int form) {
    static thread_local BitsLds LB[PROBE_SIM_WAVES][4];
    const int np = T.mode_gr * T.channels_out;
    for (int b = 0; b < grid; b++)
        for (int r = b; r < n; r += grid) {
            if (form == 0) { WAVE_RUN(kb_bits(T, W, SD, r, lane_, LB[b][0])); continue; }
#ifdef LHIP_WAVESIM
            int meet[2] = {0, 0};
            wsim::run_block(np, [&](int wave_, int lane_) { kb_bits_mw(T, W, SD, r, lane_, LB[b][wave_], LB[b][0].w, wave_, np, meet); });
#else
            for (int part = 0; part < np; part++) kb_bits_mw_t<1>(T, W, SD, r, 0, LB[b][part], LB[b][0].w, part, np, nullptr);
            for (int part = 0; part < np; part++) kb_bits_mw_t<2>(T, W, SD, r, 0, LB[b][part], LB[b][0].w, part, np, nullptr);
            for (int part = 0; part < np; part++) kb_bits_mw_t<4>(T, W, SD, r, 0, LB[b][part], LB[b][0].w, part, np, nullptr);
#endif
        }
}
static inline bool g_kt_on_() { return false; }
static bool collect_kernel_times(void*) { return true; }
static bool collect_repair_stats(Context*, BatchPlan&, bool, const int32_t*) { return true; }      // (run_pipeline counted them itself)
// P.paths: the simulations record what they simulate -- the scalar one has no two-waves-per-frame program and no count helpers, the wave
// simulation always runs the count helpers, and neither has g_fixup's two launch forms (the repair is the host loop below): no FIXUP bit.
// A fast table set's speculative pass is kb_quant_fast (QUANT_FAST): frame by frame in the scalar simulation, g_quant_fast's workgroup of
// pairs (two channels) or of single waves (one channel) in the wave simulation.
static bool run_pipeline(Context* ctx, BatchPlan& P) {
    const TableSet& ts = *P.ts; const Tables& T = ts.T; Workspace& W = P.W; const std::vector<StreamDesc>& sd = P.sd;
    const StreamDesc* dSD = P.dSD; const StreamIO* dIO = P.dIO;
    const int S = P.S, C = T.channels_out, ngs = P.ngs, nfs = P.nfs, nfr = P.nfr; const bool resv = P.resv, use_frame = P.use_frame;
    int64_t& repaired = P.repaired; int64_t& iters = P.iters;
    if (P.count_f32) g_rejected = (int64_t)kb_count_rejected(dIO, S, T.channels_in, T.pcm_limit, 0, 1);
    if (P.ingest_tiles > 0) {       // g_ingest, workgroup by workgroup
        P.paths |= LHIP_PATH_INGEST;
        alignas(16) static thread_local uint8_t LI[ING_WINDOW];
        unsigned long long bad = 0;
        for (int b = 0; b < P.ingest_tiles; b++) { const int s = ingest_find_stream(P.dING, S, b); WAVE_RUN(const unsigned r = kb_ingest(P.dING, s, (int64_t)b - P.dING[s].blk0, lane_, LI, T.pcm_limit); if (lane_ == 0) bad += r); }
        if (P.count_rej) g_rejected += (int64_t)bad;
    }
    // (thread_local: with LHIP_HOSTSIM_DEVICES > 1 host threads batch on different contexts at the same time)
    static thread_local PsyALds LA; static thread_local PsyBLds4 LB; static thread_local MdctLds LM; static thread_local PolyLds LP; static thread_local QuantLds LQ; static thread_local BitsLds LBi; static thread_local QuantTabs QT;
    q_load_tabs(T, QT, 0, 1);
    if (use_frame) {
        P.paths |= resv ? LHIP_PATH_FRAME_RESV : LHIP_PATH_FRAME;
        // the one-frame-per-stream program (kb_frame_stage), stage by stage; the wave simulation runs it as a real workgroup
        const int NW = FR_WAVES;
        alignas(16) static thread_local unsigned char UL[FR_WAVES][FR_LDS_PER_WAVE]; static thread_local int fmbox[12]; static thread_local CountShare fcs[2];
        for (int s = 0; s < S; s++) {
            fcs[0].state = CS_IDLE; fcs[1].state = CS_IDLE;      // per workgroup, as g_frame does (a stream's owners leave CS_QUIT behind)
#ifdef LHIP_WAVESIM
            wsim::run_block(NW, [&](int wave_, int lane_) {
                for (int stage = 0; stage < FR_STAGES; stage++) {
                    if (resv ? frame_stage_empty<1>(stage, T) : frame_stage_empty<0>(stage, T)) continue;
                    if (resv) kb_frame_stage<1, 1>(stage, T, ts.pb10, W, dSD, dIO, s, wave_, NW, lane_, UL[wave_], QT, fmbox, fcs);
                    else kb_frame_stage<0, 1>(stage, T, ts.pb10, W, dSD, dIO, s, wave_, NW, lane_, UL[wave_], QT, fmbox, fcs);
                    wg_barrier();
                }
            });
#else
            for (int stage = 0; stage < FR_STAGES; stage++)
                for (int wv = 0; wv < NW; wv++) {
                    if (resv) kb_frame_stage<1, 0>(stage, T, ts.pb10, W, dSD, dIO, s, wv, NW, 0, UL[wv], QT, fmbox);
                    else kb_frame_stage<0, 0>(stage, T, ts.pb10, W, dSD, dIO, s, wv, NW, 0, UL[wv], QT, fmbox);
                }
#endif
        }
        if (resv) for (int s = 0; s < S; s++) if (sd[s].flush) P.paths |= LHIP_PATH_RESV_FLUSH;
        if (resv) for (int s = 0; s < S; s++) if (sd[s].flush) WAVE_RUN(kb_resv_flush(T, W, s, lane_, LBi, dIO[s].state->rv, W.out_bytes + s));
    } else {
    P.paths |= LHIP_PATH_SEPARATE | (T.rs_ratio != 1 ? LHIP_PATH_PREP : 0) | (T.psy_channels == 4 ? LHIP_PATH_PSY4 : 0);
    for (int s = 0; s < S; s++) WAVE_RUN(kb_load(T, W, dSD, dIO, s, lane_));
    if (T.rs_ratio != 1) kb_prep(T, W, dSD, dIO, S, 0, 1);
    const bool lazy = P.psy_lazy;      // (as lhip_pipeline_hip.h: part 1, the scans, then part 2 in its lazy form)
    if (lazy) {
        for (int b = 0; b < ngs * C; b++) WAVE_RUN(kb_psyA<1>(T, W, dSD, dIO, b / C, b % C, lane_, LA));
        if (T.psy_channels == 4) for (int b = 0; b < ngs * 2; b++) WAVE_RUN(kb_psyA<1>(T, W, dSD, dIO, b / 2, 2 + b % 2, lane_, LA));
    } else {
        for (int b = 0; b < ngs * C; b++) WAVE_RUN(kb_psyA(T, W, dSD, dIO, b / C, b % C, lane_, LA));
        if (T.psy_channels == 4) for (int b = 0; b < ngs * 2; b++) WAVE_RUN(kb_psyA(T, W, dSD, dIO, b / 2, 2 + b % 2, lane_, LA));
    }
    for (int b = 0; b < ngs; b++) kb_scan_raw(T, W, dSD, b);
    for (int b = 0; b < ngs; b++) kb_scan_attack(T, W, dSD, b);
    for (int b = 0; b < ngs; b++) kb_scan_blocktype(T, W, dSD, b);
    if (lazy) {
        for (int b = 0; b < ngs * C; b++) WAVE_RUN((kb_psyA<2, 1>(T, W, dSD, dIO, b / C, b % C, lane_, LA)));
        if (T.psy_channels == 4) for (int b = 0; b < ngs * 2; b++) WAVE_RUN((kb_psyA<2, 1>(T, W, dSD, dIO, b / 2, 2 + b % 2, lane_, LA)));
    }
#ifdef LHIP_WAVESIM
    { static thread_local AthLds LAth; for (int s = 0; s < S; s++) wsim::run_block(ATH_NT / 64, [&](int wave_, int lane_) { kb_scan_ath(T, W, dSD, s, 64 * wave_ + lane_, LAth); }); }
#else
    { static thread_local AthLds LAth; for (int s = 0; s < S; s++) kb_scan_ath(T, W, dSD, s, 0, LAth); }
#endif
    if (!resv && lazy) for (int b = 0; b < ngs; b++) WAVE_RUN((kb_psyB<4, 1>(T, ts.pb10, W, dSD, b, lane_, LB, -1)));
    else if (!resv) for (int b = 0; b < ngs; b++) WAVE_RUN(kb_psyB<4>(T, ts.pb10, W, dSD, b, lane_, LB, -1));
    for (int b = 0; b < (ngs * C + POLY_PER_WAVE - 1) / POLY_PER_WAVE; b++) WAVE_RUN(kb_polyphase(T, W, dSD, dIO, b, ngs * C, lane_, LP));
    for (int b = 0; b < ngs; b++) WAVE_RUN(kb_mdct(T, W, dSD, b, lane_, LM));
    if (resv) {
        // the per-stream reservoir program (kb_resv_stage), as g_resv_stream runs it; the wave simulation as a real workgroup of four waves
#ifdef LHIP_WAVESIM
        P.paths |= LHIP_PATH_RESV_STREAM_HELPERS;
#else
        P.paths |= LHIP_PATH_RESV_STREAM_NOHELPERS;
#endif
        alignas(16) static thread_local unsigned char RU[RS_WAVES][RS_LDS_PER_WAVE]; static thread_local int rmbox[4]; static thread_local CountShare rcs[2];
        for (int s = 0; s < S; s++) {
            ResvState RV = dIO[s].state->rv;
            int32_t nout = 0;
            const int F = sd[s].nframes;
#ifdef LHIP_WAVESIM
            wsim::run_block(RS_WAVES, [&](int wave_, int lane_) {
                for (int k = 0; k <= F; k++)
                    for (int stage = 0; stage < RS_STAGES; stage++) { kb_resv_stage<1>(stage, T, ts.pb10, W, dSD, s, k, F, wave_, lane_, RU[wave_], QT, rmbox, RV, &nout, rcs); wg_barrier(); }
                if (wave_ == 3 && sd[s].flush) kb_resv_flush(T, W, s, lane_, *(BitsLds*)RU[3], RV, &nout);
            });
#else
            for (int k = 0; k <= F; k++)
                for (int stage = 0; stage < RS_STAGES; stage++)
                    for (int wv = 0; wv < RS_WAVES; wv++) kb_resv_stage<0>(stage, T, ts.pb10, W, dSD, s, k, F, wv, 0, RU[wv], QT, rmbox, RV, &nout);
            if (sd[s].flush) kb_resv_flush(T, W, s, 0, *(BitsLds*)RU[3], RV, &nout);
#endif
            dIO[s].state->rv = RV;
            W.out_bytes[s] = nout;
        }
    } else {
#ifdef LHIP_WAVESIM
    // small stereo batches: the two-waves-per-frame latency kernel (kb_quant<1>), as run_batch chooses on the device
    static thread_local QuantLds LQ2[2]; static thread_local int mbox[4];
    static const int pair_max = []() { const char* e = getenv("LAMEJS_HIP_PAIR_MAX_FRAMES"); return e ? atoi(e) : 12; }();
    const bool pair = (C == 2 && nfs <= pair_max);
#endif
    const bool fastq = ts.fast && fast_quant_allowed();
    // the launch record (lhip_debug_read(11)): what is simulated -- one 8-wave workgroup, or the pair program's one workgroup of two waves per frame slot, in the
    // wave simulation; the three striding "waves" of the scalar one as one workgroup of 3.  Both run the SKIP = 1 bodies, which decide per granule-channel: `skip`
    // reports the table set's skip_tail, the form the device launches for it.
#ifdef LHIP_WAVESIM
    P.ql.workgroups = (!fastq && pair) ? nfs : 1; P.ql.waves = (!fastq && pair) ? 2 : 8; P.ql.kernel = fastq ? QL_FAST : pair ? QL_PAIR : QL_PERSISTENT; P.ql.pair = fastq ? C == 2 : pair;
#else
    P.ql.workgroups = 1; P.ql.waves = 3; P.ql.kernel = fastq ? QL_FAST : QL_PERSISTENT; P.ql.pair = fastq && C == 2;
#endif
    P.ql.nfs = nfs; P.ql.skip = ts.skip_tail;
#ifdef LHIP_WAVESIM
    P.paths |= fastq ? LHIP_PATH_QUANT_FAST : pair ? LHIP_PATH_QUANT_PAIR : LHIP_PATH_QUANT_PERSISTENT;
#else
    P.paths |= fastq ? LHIP_PATH_QUANT_FAST : LHIP_PATH_QUANT_PERSISTENT;
#endif
    if (fastq) {
#if defined(LHIP_WAVESIM)
        // g_quant_fast as a real 8-wave workgroup: the frame slots drawn from a shared counter, by every wave (one channel) or by wave 0 of every pair
        static thread_local QuantLds LF[8]; static thread_local FastPair FP[4];
        int ctr = 0;
        memset(FP, 0, sizeof FP);
        wsim::run_block(8, [&](int wave_, int lane_) {
            int hint[3] = {-1, -1, -1};
            for (int round = 1;; round++) {
                int f = 0;
                if (C == 2) {
                    FastPair& fp = FP[wave_ >> 1];
                    if ((wave_ & 1) == 0) { if (lane_ == 0) f = ctr++; f = wave_bcast(f, 0); fast_pair_publish_slot(fp, round, f, lane_); }
                    else f = fast_pair_await_slot(fp, round, lane_);
                    if (f >= nfs) break;
                    kb_quant_fast<1, 1>(T, ts.pb10, W, dSD, f, lane_, LF[wave_], QT, hint, wave_ & 1, &fp, round);
                } else {
                    if (lane_ == 0) f = ctr++;
                    f = wave_bcast(f, 0);
                    if (f >= nfs) break;
                    kb_quant_fast<0, 1>(T, ts.pb10, W, dSD, f, lane_, LF[wave_], QT, hint);
                }
            }
        });
#else
        // three "persistent waves" striding over the frame slots, each with its own seed hint (as the general pass below)
        int hints[3][3] = {{-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}};
        for (int b = 0; b < nfs; b++) WAVE_RUN(kb_quant_fast<0, 1>(T, ts.pb10, W, dSD, b, lane_, LQ, QT, hints[b % 3]));
#endif
    } else
#if defined(LHIP_WAVESIM)
    if (!pair) {   // the persistent kernel as a real 8-wave workgroup: frames drawn from a shared counter (kb_quant_th, what g_quant runs for one- and
                    // two-channel streams alike), then -- two channels -- the waves help each other (k_quant_tail.h)
        static thread_local QuantLds LQ8[8]; static thread_local TailShare TS;
        int ctr = 0;
        TS.drawing = 8; for (int w = 0; w < 8; w++) TS.offer[w].state = 0;
        wsim::run_block(8, [&](int wave_, int lane_) {
            int hint[3] = {-1, -1, -1};
            for (;;) {
                int f = 0;
                if (lane_ == 0) f = ctr++;
                f = wave_bcast(f, 0);
                if (f >= nfs) break;
                kb_quant_th<1>(T, ts.pb10, W, dSD, f, lane_, LQ8[wave_], QT, hint, TS, wave_);
            }
            if (C == 2) tail_help<1>(T, ts.pb10, W, dSD, lane_, LQ8, wave_, 8, QT, TS);
        });
    } else
#endif
    {   // the speculative pass as three "persistent waves" striding over the frame slots, each with its own seed hint -- what g_quant's
        // waves do with the frames they draw (kb_quant: `hint`), so that the simulations cover that path too
        int hints[3][3] = {{-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}};
        for (int b = 0; b < nfs; b++) {
#ifdef LHIP_WAVESIM
            if (pair) { QUANT_RUN(0); continue; }
            int hl[64][3];                                     // every lane fiber updates its own copy; they must agree (wave-uniform)
            for (int l = 0; l < 64; l++) for (int q = 0; q < 3; q++) hl[l][q] = hints[b % 3][q];
            WAVE_RUN(kb_quant<0, 0, 1>(T, ts.pb10, W, dSD, b, 0, lane_, LQ, QT, -1, nullptr, nullptr, hl[lane_]));
            for (int l = 1; l < 64; l++) for (int q = 0; q < 3; q++) if (hl[l][q] != hl[0][q]) { set_err("wavesim: seed hint not wave-uniform"); return false; }
            for (int q = 0; q < 3; q++) hints[b % 3][q] = hl[0][q];
#else
            WAVE_RUN(kb_quant<0, 0, 1>(T, ts.pb10, W, dSD, b, 0, lane_, LQ, QT, -1, nullptr, nullptr, hints[b % 3]));
#endif
        }
    }
    for (;;) {
        W.nflagged[0] = 0; W.nflagged[1] = 0;
        for (int b = 0; b < nfs; b++) kb_validate_fast(T, W, dSD, b);
        for (int i = 0; i < W.nflagged[1]; i++) WAVE_RUN(kb_validate<1>(T, ts.pb10, W, dSD, W.slow_list[i], lane_, LQ, QT));
        const int nf = W.nflagged[0];
        if (nf == 0) break;
        repaired += nf; iters++;
        for (int b = 0; b < nfs; b++) QUANT_RUN(1);
        if (iters > nfr + 2) { set_err("seed-chain repair did not converge"); return false; }
    }
    for (int b = 0; b < nfs; b++) WAVE_RUN(kb_bits(T, W, dSD, b, lane_, LBi));
    }
    for (int s = 0; s < S; s++) WAVE_RUN(kb_save(T, W, dSD, dIO, s, lane_));
    }
    if (P.crc_mode == 2) {         // g_out_crc and g_out_crc_fold, workgroup by workgroup
        P.paths |= LHIP_PATH_OUT_CRC;
        const CrcDesc* D = (const CrcDesc*)ctx->ws.crc_desc.p; uint32_t* part = (uint32_t*)ctx->ws.crc_part.p;
        for (int b = 0; b < P.crc_parts; b++) { const int s = crc_find_stream(D, S, b); WAVE_RUN(kb_out_crc(D, s, b - D[s].part0, lane_, part)); }
        for (int s = 0; s < S; s++) WAVE_RUN(kb_crc_fold(D, s, lane_, part, P.crc_dst));
    }
    if (P.gain.stage_blocks > 0) {      // g_gain_stage and g_gain, workgroup by workgroup
        P.paths |= LHIP_PATH_GAIN;
        gain_sim_run(T, W, dSD, dIO, P.dGD, S, P.gain.stage_blocks, P.gain.waves);
    }
    return true;
}
#undef QUANT_RUN
#undef WAVE_RUN
