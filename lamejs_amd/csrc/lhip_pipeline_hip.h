// lhip_pipeline_hip.h -- run_pipeline of the product: the HIP launch sequence of one batch on the context's stream, and what only a device
// build has around it (kernel timing, repair statistics left on the device).  Exactly one of this and lhip_pipeline_sim.h is included (lhip_batch.h).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
static inline bool g_kt_on_() { return g_kt_on; }
static_assert(FX_STATS_OFF == FX_STATS * 4, "counter block layout");
static bool collect_kernel_times(void* st) { if (g_kt_on) { if (!rt::sync(st)) return false; kt_collect(); } return true; }
// (an asynchronous batch leaves its repair statistics on the device: lhip_last_batch_stats fetches them)
static bool collect_repair_stats(Context* ctx, BatchPlan& P, bool fetch_fx, const int32_t* fx) {
    g_stat_pending = nullptr;
    if (fetch_fx) {
        P.repaired = fx[0]; P.iters = fx[1];
        if (fx[2]) { set_err("seed-chain repair did not converge"); return false; }
    } else if (P.nfr > 0) g_stat_pending = ctx;
    return true;
}
// LAMEJS_HIP_QUANT_GRID_MAX=<n>, n >= 1 (read once per process; a test hook): at most n workgroups for the persistent speculative quantization launches,
// g_quant_fast and g_quant -- with n = 1 every wave (pair) of the one workgroup takes frame after frame at a few frames already.  Unset or < 1: no cap.
// No other kernel's grid is touched (g_quant_pair is one workgroup per frame, g_fixup's grid decides its launch form, g_resv_stream's is the streams).
static int quant_grid_cap(int grid) {
    static const int cap = []() { const char* e = getenv("LAMEJS_HIP_QUANT_GRID_MAX"); return e ? atoi(e) : 0; }();
    return cap >= 1 && grid > cap ? cap : grid;
}
static bool run_pipeline(Context* ctx, BatchPlan& P) {
    const TableSet& ts = *P.ts; const Tables& T = ts.T; Workspace& W = P.W; const std::vector<StreamDesc>& sd = P.sd;
    const StreamDesc* dSD = P.dSD; const StreamIO* dIO = P.dIO;
    const int S = P.S, C = T.channels_out, ngs = P.ngs, nfs = P.nfs, nfr = P.nfr; const bool resv = P.resv, use_frame = P.use_frame;
    WorkSet& ws = ctx->ws; void* st = ctx->stream; const int64_t in_total = P.in_total;
    if (P.count_rej) {
        if (!ws.rejected.ensure(64) || !rt::dzero(ws.rejected.p, 8, st)) return false;
        int64_t nb = (in_total + 255) / 256;
        if (nb > 2048) nb = 2048;
        if (nb < 1) nb = 1;
        if (P.count_f32) LAUNCHB(KT_COUNT, g_count_rejected, (int)nb, 256, st, dIO, S, T.channels_in, T.pcm_limit, (unsigned long long*)ws.rejected.p);
        g_rej_pending = ctx;
    }
    // WAV sample types: the call's new samples become Float32 planes (dIO points at them) before anything reads them; the float types are cleaned and counted here
    if (P.ingest_tiles > 0) {
        P.paths |= LHIP_PATH_INGEST;
        LAUNCH(KT_INGEST, g_ingest, P.ingest_tiles, st, P.dING, S, T.pcm_limit, P.count_rej ? (unsigned long long*)ws.rejected.p : (unsigned long long*)nullptr);
    }
    if (use_frame) {
        QArgs qa; qa.T = T; qa.pb = ts.pb10; qa.W = W; qa.SD = dSD; qa.chain = 0; qa.nfs = nfs; qa.ctr = 0;
        P.paths |= resv ? LHIP_PATH_FRAME_RESV : LHIP_PATH_FRAME;
        if (resv) LAUNCHB(KT_QUANT, g_frame<1>, S, 64 * FR_WAVES, st, qa, dIO); else LAUNCHB(KT_QUANT, g_frame<0>, S, 64 * FR_WAVES, st, qa, dIO);
        if (resv) { bool any_flush = false; for (int i = 0; i < S; i++) any_flush |= sd[i].flush != 0; if (any_flush) { P.paths |= LHIP_PATH_RESV_FLUSH; LAUNCH(KT_BITS, g_resv_flush, S, st, T, W, dSD); } }
    } else {
    P.paths |= LHIP_PATH_SEPARATE | (T.rs_ratio != 1 ? LHIP_PATH_PREP : 0) | (T.psy_channels == 4 ? LHIP_PATH_PSY4 : 0);
    LAUNCH(KT_LOAD, g_load, S, st, T, W, dSD, dIO);
    if (T.rs_ratio != 1) {          // only the resampler materialises samples; otherwise the consumers convert the caller's Int16 themselves
        int64_t nb = (in_total / C + 255) / 256;
        if (nb > 8192) nb = 8192;
        if (nb < 1) nb = 1;
        LAUNCHB(KT_PREP, g_prep, (int)nb, 256, st, T, W, dSD, dIO, S);
    }
    // A lazy batch (plan_batch) runs the high-pass + sub-block peaks first, then the scans, and everything else of psyA once the block types are known:
    // the short-block side is then computed only for the calls a short granule (or the stream state) reads it from
    const bool lazy = P.psy_lazy;
    if (lazy) {
        LAUNCHB(KT_PSYA, g_psyA<1>, XCD_GRID_W(ngs * C), 64 * WPB, st, T, W, dSD, dIO, 0, C);
        if (T.psy_channels == 4) LAUNCHB(KT_PSYA, g_psyA<1>, XCD_GRID_W(ngs * 2), 64 * WPB, st, T, W, dSD, dIO, 2, 2);
    } else {
        LAUNCHB(KT_PSYA, g_psyA<0>, XCD_GRID_W(ngs * C), 64 * WPB, st, T, W, dSD, dIO, 0, C);
        if (T.psy_channels == 4) LAUNCHB(KT_PSYA, g_psyA<0>, XCD_GRID_W(ngs * 2), 64 * WPB, st, T, W, dSD, dIO, 2, 2);
    }
    LAUNCH(KT_SCAN, g_scan_raw, (ngs + 63) / 64, st, T, W, dSD, ngs);
    LAUNCH(KT_SCAN, g_scan_attack, (ngs + 63) / 64, st, T, W, dSD, ngs);
    LAUNCH(KT_SCAN, g_scan_blocktype, (ngs + 63) / 64, st, T, W, dSD, ngs);
    if (lazy) {
        LAUNCHB(KT_PSYA, g_psyA<2>, XCD_GRID_W(ngs * C), 64 * WPB, st, T, W, dSD, dIO, 0, C);
        if (T.psy_channels == 4) LAUNCHB(KT_PSYA, g_psyA<2>, XCD_GRID_W(ngs * 2), 64 * WPB, st, T, W, dSD, dIO, 2, 2);
    }
    // g_scan_ath (needs psyA's loudness, feeds psyB and the quantizer) is one workgroup per stream: it runs on a side
    // stream while polyphase + MDCT (which need neither) keep the chip busy.  With per-kernel timing on, everything stays
    // on the launch stream so that the HIP events bracket each kernel.
    bool forked = false;
    struct AuxJoin {           // an error return between fork and join must not leave g_scan_ath running on the shared workspace
        void* aux = nullptr;
        ~AuxJoin() { if (aux) (void)hipStreamSynchronize((hipStream_t)aux); }
    } aux_guard;
    if (!g_kt_on) {
        if (!ws.aux_stream) {
            hipStream_t a; hipEvent_t e1, e2;
            if (hipStreamCreateWithFlags(&a, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&e2, hipEventDisableTiming) == hipSuccess) { ws.aux_stream = a; ws.ev_fork = e1; ws.ev_join = e2; }
        }
        if (ws.aux_stream && hipEventRecord((hipEvent_t)ws.ev_fork, (hipStream_t)st) == hipSuccess &&
            hipStreamWaitEvent((hipStream_t)ws.aux_stream, (hipEvent_t)ws.ev_fork, 0) == hipSuccess) {
            LAUNCHB(KT_SCAN, g_scan_ath, S, ATH_NT, ws.aux_stream, T, W, dSD);
            aux_guard.aux = ws.aux_stream;
            HIPCK(hipEventRecord((hipEvent_t)ws.ev_join, (hipStream_t)ws.aux_stream));
            forked = true;
        }
    }
    if (!forked) LAUNCHB(KT_SCAN, g_scan_ath, S, ATH_NT, st, T, W, dSD);
    LAUNCH(KT_POLY, g_poly, XCD_GRID((ngs * C + POLY_PER_WAVE - 1) / POLY_PER_WAVE), st, T, W, dSD, dIO, ngs * C);
    LAUNCH(KT_MDCT, g_mdct, XCD_GRID(ngs), st, T, W, dSD);
    if (forked) { HIPCK(hipStreamWaitEvent((hipStream_t)st, (hipEvent_t)ws.ev_join, 0)); aux_guard.aux = nullptr; }
    if (resv) {
        // bit reservoir: psyB -> quantization -> bit packing of a stream's frames are a serial chain: one workgroup per stream walks them
        // (qa.ctr = 1: the idle waves of a workgroup count for the quantizing ones -- only while every workgroup has a CU to itself: with two
        //  per CU a helper shares its SIMD with the other workgroup's searching wave and the speculative work costs more than it hides --
        //  512 streams: 2.37 M frames/s without helpers, 2.21 M with, profiles/r05_pass4_* / r05_pass5_*)
        QArgs qa; qa.T = T; qa.pb = ts.pb10; qa.W = W; qa.SD = dSD; qa.chain = 2; qa.nfs = nfs; qa.ctr = S <= ctx->num_cus ? 1 : 0;
        P.paths |= qa.ctr ? LHIP_PATH_RESV_STREAM_HELPERS : LHIP_PATH_RESV_STREAM_NOHELPERS;
        LAUNCHB(KT_QUANT, g_resv_stream, S, 64 * RS_WAVES, st, qa);
    } else {
    if (T.psy_channels == 4) { if (lazy) LAUNCHB(KT_PSYB, (g_psyB<4, 1>), XCD_GRID_W(ngs), 64 * WPB, st, T, ts.pb10, W, dSD, -1); else LAUNCHB(KT_PSYB, (g_psyB<4, 0>), XCD_GRID_W(ngs), 64 * WPB, st, T, ts.pb10, W, dSD, -1); }
    else { if (lazy) LAUNCHB(KT_PSYB, (g_psyB<2, 1>), XCD_GRID_W(ngs), 64 * WPB, st, T, ts.pb10, W, dSD, -1); else LAUNCHB(KT_PSYB, (g_psyB<2, 0>), XCD_GRID_W(ngs), 64 * WPB, st, T, ts.pb10, W, dSD, -1); }
    // persistent quantization kernels: as many workgroups as can be resident (2 per CU), frames dispensed dynamically
    int qgrid = (nfs + QWAVES - 1) / QWAVES;
    if (qgrid > ctx->num_cus * 2) qgrid = ctx->num_cus * 2;
    qgrid = quant_grid_cap(qgrid);
#ifdef LHIP_PHASE_PROF
    const bool pair = false;
#else
    // Two waves per frame while that still leaves SIMDs under-subscribed.  Measured on MI355X (stereo 128 kbps, ms per batch,
    // persistent / pair): 600 frames 3.40 / 2.20, 1000: 3.52 / 2.41, 2000: 3.66 / 3.61, 4000: 4.82 / 5.15 -> cross-over at
    // about 2000 frames = 8 x CUs; LAMEJS_HIP_PAIR_MAX_FRAMES overrides the threshold for experiments.
    static const int pair_max = []() { const char* e = getenv("LAMEJS_HIP_PAIR_MAX_FRAMES"); return e ? atoi(e) : -1; }();
    const bool pair = (C == 2 && nfs <= (pair_max >= 0 ? pair_max : 6 * ctx->num_cus));
#endif
    const bool fastq = ts.fast && fast_quant_allowed();
    P.paths |= fastq ? LHIP_PATH_QUANT_FAST : pair ? LHIP_PATH_QUANT_PAIR : LHIP_PATH_QUANT_PERSISTENT;
    if (fastq) {
        // a fast table set (quality 7): the bin-search-only kernel, one wave per channel at every batch size; as many workgroups as the device holds of it
        QArgs qa; qa.T = T; qa.pb = ts.pb10; qa.W = W; qa.SD = dSD; qa.chain = 0; qa.nfs = nfs; qa.ctr = 0;
        const void* const fns[4] = {(const void*)g_quant_fast<0, 0>, (const void*)g_quant_fast<0, 1>, (const void*)g_quant_fast<1, 0>, (const void*)g_quant_fast<1, 1>};
        int& wg_per_cu = ctx->qfast_wg_per_cu[(C == 2 ? 2 : 0) + (ts.skip_tail ? 1 : 0)];
        if (wg_per_cu == 0) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fns[(C == 2 ? 2 : 0) + (ts.skip_tail ? 1 : 0)], 64 * QF_WAVES, 0) != hipSuccess || nb < 1) nb = 1;
            wg_per_cu = nb;
        }
        const int per_wg = C == 2 ? QF_WAVES / 2 : QF_WAVES;      // frames in flight per workgroup
        int fq = (nfs + per_wg - 1) / per_wg;
        if (fq > ctx->num_cus * wg_per_cu) fq = ctx->num_cus * wg_per_cu;
        fq = quant_grid_cap(fq);
        P.ql.workgroups = fq; P.ql.waves = QF_WAVES; P.ql.nfs = nfs; P.ql.kernel = QL_FAST; P.ql.pair = C == 2; P.ql.skip = ts.skip_tail;
        if (C == 2) { if (ts.skip_tail) LAUNCHB(KT_QUANT, (g_quant_fast<1, 1>), fq, 64 * QF_WAVES, st, qa); else LAUNCHB(KT_QUANT, (g_quant_fast<1, 0>), fq, 64 * QF_WAVES, st, qa); }
        else { if (ts.skip_tail) LAUNCHB(KT_QUANT, (g_quant_fast<0, 1>), fq, 64 * QF_WAVES, st, qa); else LAUNCHB(KT_QUANT, (g_quant_fast<0, 0>), fq, 64 * QF_WAVES, st, qa); }
    } else
    { QArgs qa; qa.T = T; qa.pb = ts.pb10; qa.W = W; qa.SD = dSD; qa.chain = 0; qa.nfs = nfs; qa.ctr = 0;
      P.ql.workgroups = pair ? nfs : qgrid; P.ql.waves = pair ? 2 : QWAVES; P.ql.nfs = nfs; P.ql.kernel = pair ? QL_PAIR : QL_PERSISTENT; P.ql.pair = pair; P.ql.skip = ts.skip_tail;
      // (which form is a matter of speed only: the skip itself is decided per granule-channel from its spectrum)
      if (pair) { if (ts.skip_tail) LAUNCHB(KT_QUANT, (g_quant_pair<1>), nfs, 128, st, qa); else LAUNCHB(KT_QUANT, (g_quant_pair<0>), nfs, 128, st, qa); }
      else { if (ts.skip_tail) LAUNCHB(KT_QUANT, (g_quant<1>), qgrid, 64 * QWAVES, st, qa); else LAUNCHB(KT_QUANT, (g_quant<0>), qgrid, 64 * QWAVES, st, qa); } }
    if (nfr > 0) {
        // validation of the seed chain + repair of the flagged frames, decided on the device (no host round trip in the pipeline)
        QArgs qa; qa.T = T; qa.pb = ts.pb10; qa.W = W; qa.SD = dSD; qa.chain = 1; qa.nfs = nfs; qa.ctr = 0;
        LAUNCHB(KT_VALIDATE, g_validate_fast, (nfs + 63) / 64, 256, st, T, W, dSD, nfs);
        // as many workgroups as can be resident (two per CU): the memo-miss re-validation (a quarter to a third of the frames of steady
        // material) is spread over all of them -- a quarter-chip grid was tried and doubled this stage's time
        int fgrid = (nfs + 63) / 64;
        if (ctx->fixup_wg_per_cu == 0) {      // once per context: how many of this build's g_fixup workgroups a CU really holds (a grid barrier needs them all resident)
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)g_fixup<1>, 64 * QWAVES, 0) != hipSuccess || nb < 1) nb = 1;
            ctx->fixup_wg_per_cu = nb < LHIP_FIXUP_OCC / 2 ? nb : LHIP_FIXUP_OCC / 2;
        }
        if (fgrid > ctx->num_cus * ctx->fixup_wg_per_cu) fgrid = ctx->num_cus * ctx->fixup_wg_per_cu;
        if (fgrid < 1) fgrid = 1;
        P.paths |= fgrid == 1 ? LHIP_PATH_FIXUP_SINGLE : LHIP_PATH_FIXUP_COOP;
        const void* fixup_fn = ts.skip_tail ? (const void*)g_fixup<1> : (const void*)g_fixup<0>;
        if (fgrid == 1) { if (ts.skip_tail) LAUNCHB(KT_VALIDATE, g_fixup<1>, 1, 64 * QWAVES, st, qa); else LAUNCHB(KT_VALIDATE, g_fixup<0>, 1, 64 * QWAVES, st, qa); }
        else {
            kt_begin(KT_VALIDATE, st);
            void* kargs[] = {(void*)&qa};
            // An aliased context (tests, LHIP_ALIAS_DEVICES) runs on a stream the library created, and its batches come from worker threads: after a cooperative
            // launch on such a stream from a thread that has since ended, ROCm 7.2's own exit handler crashes inside the HSA runtime (seen on gfx950: every variant
            // without the cooperative launch, or on the null stream, or from the main thread, exits cleanly).  So there the launch goes through the null
            // stream, ordered behind / in front of the context's stream by two events.
            hipStream_t cst = (hipStream_t)st;
            if (ctx->own_stream) {
                if (!ctx->ev_coop[0]) { if (!rt::event_create(&ctx->ev_coop[0]) || !rt::event_create(&ctx->ev_coop[1])) return false; }
                if (!rt::event_record(ctx->ev_coop[0], st) || !rt::stream_wait_event(nullptr, ctx->ev_coop[0])) return false;
                cst = nullptr;
            }
            hipError_t e_ = hipLaunchCooperativeKernel(fixup_fn, dim3(fgrid), dim3(64 * QWAVES), kargs, 0, cst);
            if (ctx->own_stream && e_ == hipSuccess) { if (!rt::event_record(ctx->ev_coop[1], nullptr) || !rt::stream_wait_event(st, ctx->ev_coop[1])) return false; }
            kt_end(st);
            TRACE_SYNC(g_fixup_cooperative, st);
            if (e_ != hipSuccess) { set_err(std::string("g_fixup (cooperative launch): ") + hipGetErrorString(e_)); return false; }
        }
    }
    LAUNCH(KT_BITS, g_bits, nfs, st, T, W, dSD);
    }
    LAUNCH(KT_SAVE, g_save, S, st, T, W, dSD, dIO);
    }
    // { infoTag } streams whose bytes stay on the device: their music CRC, behind the last writer of output bytes
    if (P.crc_mode == 2) {
        P.paths |= LHIP_PATH_OUT_CRC;
        LAUNCH(KT_OUT_CRC, g_out_crc, P.crc_parts, st, (const CrcDesc*)ws.crc_desc.p, S, (uint32_t*)ws.crc_part.p);
        LAUNCH(KT_OUT_CRC, g_out_crc_fold, S, st, (const CrcDesc*)ws.crc_desc.p, (const uint32_t*)ws.crc_part.p, P.crc_dst);
    }
    // { replayGain } streams: the samples of the call exist by now (caller's samples / g_ingest's planes / the resampler's plane) -- rows, then one lane per completed window
    if (P.gain.stage_blocks > 0) {
        P.paths |= LHIP_PATH_GAIN;
        LAUNCHB(KT_GAIN_STAGE, g_gain_stage, P.gain.stage_blocks, GAIN_STAGE_NT, st, T, W, dSD, dIO, P.dGD, S);
        if (C == 2) LAUNCH(KT_GAIN, g_gain<2>, P.gain.waves, st, P.dGD, S); else LAUNCH(KT_GAIN, g_gain<1>, P.gain.waves, st, P.dGD, S);
    }
    return true;
}
