// lhip_context.h -- what lives per device and per stream on the host: DevBuf / PinBuf, WorkSet, Context, lhip_stream.
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// per-device context: HIP stream + grow-only workspace
// ===========================================================================================
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        rt::dfree(p);
        cap = n + n / 4 + 4096;
        p = rt::dmalloc(cap);
        if (!p) { cap = 0; set_err("hipMalloc(workspace) failed"); return false; }
        return true;
    }
    ~DevBuf() { rt::dfree(p); }
};

// grow-only pinned host staging (small host-buffer calls: one copy in, one copy out -- run_batch)
struct PinBuf {
    void* p = nullptr; size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        rt::host_free_pinned(p);
        cap = n + n / 4 + 4096;
        p = rt::host_alloc_pinned(cap);
        if (!p) { cap = 0; return false; }
        return true;
    }
    void release() { rt::host_free_pinned(p); p = nullptr; cap = 0; }
    // (not freed by a destructor: the contexts live in a process-wide map, so that would run during static destruction, after the HIP runtime --
    //  and a profiler hooked into it -- has begun to shut down: `rocprofv3 -- python bench.py` ended in a segmentation fault at exit.  The orderly
    //  way out releases them: lhip_destroy of a context's last stream, while the runtime is certainly still up.)
};

// Everything a batch in flight owns: the workspace arrays, the descriptor / host-I/O staging, and the side stream + events of the ATH scan.
// (Round 4 measured a second set with two batches in flight -- the persistent quantization kernels side by side or one behind the other -- as
// slower than one batch at a time in every form, profiles/r04_pass5_ab_*.txt, and removed it: DESIGN.md, measured and discarded.)
struct WorkSet {
    DevBuf pcm, peaks, loud, eb_l, mask_idx, eb_s, ecb_s, att_raw, uselong, ul_tmp, last_attack, tent, prev_short, blocktype,
        ath_adjust, ath_limit, E, sb, xr, side, l3, seed, seed_flag, nflagged, slow_list, frame_bytes, desc, in16, rejected, out8, prof, fht, hpf, tot_ener, reval, att_clean, nb1, nb2, fr, out_bytes, vdig, small;
    DevBuf crc_desc, crc_part, crc_out;     // { infoTag } streams only (g_out_crc): per-stream descriptors, span remainders, results
    DevBuf ingest, ingest_desc;             // WAV sample types only (g_ingest): the Float32 planes of the call's new samples, per-stream descriptors
    DevBuf gain_rows, gain_desc;            // { replayGain } streams only (g_gain_stage, g_gain): history ++ new samples per stream and channel, per-stream descriptors
    PinBuf pin_in, pin_out;     // small host-buffer calls (run_batch): everything that travels in / out, staged once in pinned memory
    // last batch (for debug taps)
    Workspace lastW; int lastC = 0, lastCp = 0; bool have_last = false;
    // side stream for the one kernel that cannot fill the chip (the ATH recurrence: one workgroup per stream); it runs
    // beside the filterbank kernels, which do not depend on it
    void* aux_stream = nullptr; void* ev_fork = nullptr; void* ev_join = nullptr;
};

struct Context {
    int device = 0;
    void* stream = nullptr;
    std::mutex mu;
    void* ev_coop[2] = {nullptr, nullptr};      // aliased contexts: the events that order the cooperative launch (null stream) with the context's own stream
    bool own_stream = false;    // `stream` was created by the library (aliased contexts only) and is destroyed by lhip_debug_release_context
    int live_streams = 0;       // streams created on this context and not yet destroyed (guarded by mu): the last one out releases the pinned staging buffers
    std::map<std::string, std::shared_ptr<TableSet>> tables;
    WorkSet ws;
    int num_cus = 256;
    int qfast_wg_per_cu[4] = {0, 0, 0, 0};    // resident workgroups per CU of g_quant_fast<PAIR, SKIP> (index 2 PAIR + SKIP; occupancy query at the first launch): its persistent grid is sized by it
    int fixup_wg_per_cu = 0;    // resident g_fixup workgroups per CU (occupancy query at the first cooperative launch)
    // large host-buffer calls (the drop-in's encodeBuffer with a long Int16Array): chunks of the call are copied in on this stream
    // while the chunk before is being encoded and the one before that is copied out (encode_host_chunked)
    void* copy_stream = nullptr; void* ev_in[2] = {nullptr, nullptr}; void* ev_done[2] = {nullptr, nullptr};
    DevBuf chunk_crc;           // ... and, for { infoTag } streams, the music CRCs of the call's pieces (read back once, after the last unit)
    DevBuf chunk_in, chunk_out, chunk_fx, state_bak;     // staging halves (sized for the largest chunk a call has reached so far), the per-chunk repair verdicts, the stream state a failed call gives back
    std::mutex chunk_mu;        // one chunked call at a time per device (they share the two staging halves); taken BEFORE mu, never inside it
};

static std::mutex g_ctx_mu;
static std::map<int, std::unique_ptr<Context>> g_ctx;
static Context* g_last_batch_ctx = nullptr;      // the context of the process's most recent batch (under g_ctx_mu; contexts are never destroyed): what lhip_debug_read taps

static Context* get_context(int device) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto it = g_ctx.find(device);
    if (it != g_ctx.end()) return it->second.get();
    std::unique_ptr<Context> c(new Context());
    c->device = device;
#ifndef LHIP_HOSTSIM
    { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, rt::phys(device)) == hipSuccess && n > 0) c->num_cus = n; }
    // an aliased context (LHIP_ALIAS_DEVICES) gets a HIP stream of its own: on the null stream two contexts of one physical device would simply queue up
    if (rt::alias_n() && device > 0 && hipSetDevice(0) == hipSuccess) { void* st = nullptr; if (rt::stream_create(&st)) { c->stream = st; c->own_stream = true; } }
#endif
    Context* r = c.get();
    g_ctx[device] = std::move(c);
    return r;
}

struct lhip_stream {
    uint32_t magic = 0x4c484950;
    Context* ctx = nullptr;
    std::shared_ptr<TableSet> ts;
    StreamState* d_state = nullptr;
    int mf_size = MF_INIT;
    int mf_samples_to_encode = 576 + 1152;
    int slot_lag = 0;
    int64_t frame_num = 0;
    int64_t rs_n_in = 0;           // resampling streams: input samples received so far
    // non-integer ratio (Tables::rs_frac): what the reference's resampler carries from call to call besides the last 32 samples (device, rs_old)
    double rs_itime = 0;           // gfc.itime (the same for both channels: it moves with the call lengths only)
    double rs_inbuf_nsamples = 0;  // gfc.in_buffer_nsamples: the largest call so far (fractional after a flush bunch) ...
    int64_t rs_inbuf_len = 0;      // ... and the length of the persistent input buffer allocated for it (Lame.js:1373-1379)
    bool rs_flushed = false;       // flush() has run: the reference's resampler holds NaN from then on, the stream ends there
    std::unique_ptr<TagTotals> tag;   // { infoTag } streams: what the tag frame will report (lhip_infotag.h); null otherwise
    std::unique_ptr<GainRec> gain;    // { replayGain } streams: the analysis' device record and sample count (lhip_gain.h); null otherwise
    ~lhip_stream() { rt::dfree(d_state); magic = 0; }
};
