// lhip_batch.h -- one batch of frames: Job, the length arithmetic, and run_batch as phases (plan, bind the workspace, stage descriptors and input,
// run the pipeline, fetch outputs, stream bookkeeping).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// batch encode
// ===========================================================================================
struct Job {
    lhip_stream* s; const void* l; const void* r; size_t n; uint8_t* out; size_t cap; int64_t written;
    int F; int64_t bytes;
    int64_t n_out;              // samples this call appends to the encoder's buffer (== n unless resampling)
    bool flush = false;         // bit reservoir: the stream ends with this call (its bitstream is padded to the end of the last frame)
    double rs_len = -1;         // non-integer ratio, flush only: the reference's (possibly fractional) length of this bunch of zeros; n = ceil(rs_len)
    double rs_used = 0;         // non-integer ratio: num_used of the pass (== the call's length for every call that is accepted; a flush pass may end on a whole frame)
    int f32 = 0, inter = 0;     // sample format of l / r: Float32 (else Int16); interleaved (l holds channels * n samples, r is ignored)
    bool count_rejected = false;   // Float32 by device pointer from the caller: count the samples the read sites refuse
    int type = 0;               // sample type of l / r (format & ~LHIP_PCM_INTERLEAVED); f32 == (type == LHIP_PCM_F32).  The WAV types (>= LHIP_PCM_U8) become Float32 planes first (k_ingest.h)
    void set_format(int format) { type = format & ~LHIP_PCM_INTERLEAVED; f32 = type == LHIP_PCM_F32; inter = (format & LHIP_PCM_INTERLEAVED) != 0; }
};
static_assert(LHIP_PCM_U8 == ING_U8 && LHIP_PCM_S24 == ING_S24 && LHIP_PCM_S32 == ING_S32 && LHIP_PCM_F32N == ING_F32N && LHIP_PCM_F64N == ING_F64N && LHIP_PCM_F64 == ING_F64, "k_ingest.h states the header's sample types");
// bytes per sample of a sample type / the formats of the C ABI / the types that g_ingest (or, for a small host call, the host) turns into Float32 planes
static inline size_t fmt_bps(int type) { return type == LHIP_PCM_S16 ? 2 : type == LHIP_PCM_F32 ? 4 : (size_t)ingest_bps(type); }
static inline bool fmt_ok(int format) {
    const int t = format & ~LHIP_PCM_INTERLEAVED;
    return format >= 0 && (t == LHIP_PCM_S16 || t == LHIP_PCM_F32 || t == LHIP_PCM_U8 || t == LHIP_PCM_S24 || t == LHIP_PCM_S32 || t == LHIP_PCM_F32N || t == LHIP_PCM_F64N || t == LHIP_PCM_F64);
}
static inline int fmt_type(int format) { return format & ~LHIP_PCM_INTERLEAVED; }
static inline bool fmt_ingest(int type) { return type >= LHIP_PCM_U8; }

// resampling by the integer ratio r: output sample m exists once m*r + 16 < (input samples received) -- see kb_resample_elem
static int64_t rs_outputs(int64_t n_in_total, int r) { return n_in_total > 16 ? (n_in_total - 16 + r - 1) / r : 0; }

// Resampling by a non-integer ratio (extension { fractionalResample }).  One pass of fill_buffer_resample (Lame.js:1769-1813) over `len` input
// samples with the clock at `itime`, as far as it depends on lengths only: how many outputs it delivers and how much input it uses, by the
// reference's own loop in f64.  A pass that ends at the loop's `break` used the whole input (num_used == len); one that delivers a whole
// frame first leaves num_used = j + 15.5 -- from then on the reference's buffer positions are fractional and its samples NaN.
struct FracPass { int k; double num_used; int j_last; };
static FracPass frac_pass(const Tables& T, double itime, double len) {
    const int frame = 576 * T.mode_gr;
    int k, j = 0;
    for (k = 0; k < frame; k++) {
        j = (int)floor(k * T.resample_ratio - itime);
        if ((31 + j - 15.5) >= len) break;
    }
    const double reach = 31 + j - 15.5;
    return FracPass{k, len < reach ? len : reach, j};
}
// a call of at most this many samples is consumed whole whatever came before: itime <= 15.5 after any whole pass
static int64_t frac_call_limit(const Tables& T) { return (int64_t)floor((576 * T.mode_gr - 1) * T.resample_ratio - 15.5) + 15; }
static std::string frac_refusal(const Tables& T, size_t n) {
    return "fractionalResample: the reference does not consume a call of " + std::to_string(n) + " samples whole at this point of the stream (its resampler would turn to fractional "
           "positions and NaN samples); nothing was consumed -- calls of at most " + std::to_string(frac_call_limit(T)) + " samples are always accepted for this configuration";
}
// the padding bit of the next frame and the accumulator after it (Encoder.js:442-446), as frame_padding / run_batch's bookkeeping have them
static int host_next_padding(const Tables& T, int* slot_lag) {
    if (T.frac_SpF == 0) return 0;
    int64_t m = (int64_t)*slot_lag % T.out_samplerate; if (m < 0) m += T.out_samplerate;
    const int pad = (m - T.frac_SpF) < 0 ? 1 : 0;
    m = (m - T.frac_SpF) % T.out_samplerate; if (m < 0) m += T.out_samplerate;
    *slot_lag = (int)m;
    return pad;
}

static int64_t batch_bytes(const TableSet& ts, int slot_lag, int F) {
    int64_t npad = 0;
    const Tables& T = ts.T;
    if (T.frac_SpF != 0 && F > 0) {
        const int64_t sr = T.out_samplerate;
        int64_t m0 = slot_lag % sr; if (m0 < 0) m0 += sr;
        const int64_t need = (int64_t)F * T.frac_SpF - m0;
        npad = need > 0 ? (need + sr - 1) / sr : 0;
    }
    return (int64_t)F * ts.base_frame_bytes + npad;
}
// whole frames (and their bytes: exact without the bit reservoir) that a call with `nsamples` more input samples completes on this stream
static int call_frames(const lhip_stream* s, size_t nsamples) {
    const Tables& T = s->ts->T;
    const int frame = 576 * T.mode_gr, mf_needed = 1024 + frame - 272;
    int64_t n_out;
    if (T.rs_frac) {                         // non-integer ratio: 0 or 1 frame, or -1 for a call that would be refused
        if (nsamples == 0) return 0;
        const FracPass fp = frac_pass(T, s->rs_itime, (double)nsamples);
        if (fp.k >= frame || s->rs_flushed) return -1;
        n_out = fp.k;
    } else n_out = T.rs_ratio == 1 ? (int64_t)nsamples : rs_outputs(s->rs_n_in + (int64_t)nsamples, T.rs_ratio) - rs_outputs(s->rs_n_in, T.rs_ratio);
    const int64_t total = (int64_t)s->mf_size + n_out;
    return total >= mf_needed ? (int)((total - mf_needed) / frame) + 1 : 0;
}

static std::atomic<int> g_spec_start{180}, g_spec_step{4};   // seed assumed by the speculative quantization pass (test hook)
#ifdef LHIP_PHASE_PROF
// profiling build: where the host side of a batch spends its time (seconds, summed; [7] = batches) -- lhip_debug_read(9)
static double g_call_prof[8];
#define CALL_STAMP(i) do { const auto n_ = std::chrono::steady_clock::now(); g_call_prof[i] += std::chrono::duration<double>(n_ - cp_t_).count(); cp_t_ = n_; } while (0)
#else
#define CALL_STAMP(i) do {} while (0)
#endif
enum { FX_STATS_OFF = 32 * 4 };      // byte offset of the repair statistics inside the counter block (FX_STATS of g_fixup)
// Small host-buffer calls (the drop-in's own 1152-sample call pattern, small encodeBatch calls): everything that travels is laid out as ONE
// device block   [ output bytes | counters (nflagged, out_bytes) | seed_flag | reval | descriptors | Int16 input ]
// mirrored in pinned host memory, so that a call is ONE copy in (counters arrive as the zeros they must start from), the kernels, ONE copy
// out (bytes + counters) and one synchronisation -- instead of three pageable copies in, five memsets and two to three copies out, each of
// which is a stream operation the frame's single launch waits behind (profiles/r05_*frame_prof*.txt).
// The pinned input mirror (WorkSet::pin_in) starts at the counters: device offset o of the block is offset pin(o) of the mirror.
enum { SMALL_CALL_BYTES = 1 << 20 };
struct CallLayout {
    size_t desc_sd, desc_io, desc_fm, desc_gm, desc_bytes;      // the descriptor block (stage_inputs)
    size_t sm_out, sm_nfl, sm_ob, sm_sf, sm_rv, sm_desc, sm_in, sm_end, copy_in, copy_out;
    void set(int S, int nfs, int ngs, size_t FR, int64_t out_total, size_t in_bytes) {
        auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        desc_sd = 0; desc_io = a16(desc_sd + (size_t)S * sizeof(StreamDesc)); desc_fm = a16(desc_io + (size_t)S * sizeof(StreamIO));
        desc_gm = a16(desc_fm + (size_t)nfs * 4); desc_bytes = desc_gm + (size_t)ngs * 4;
        sm_out = 0; sm_nfl = a16((size_t)out_total + 64); sm_ob = sm_nfl + 256; sm_sf = a16(sm_ob + (size_t)S * 4 + 64); sm_rv = sm_sf + a16(FR * 4);
        sm_desc = sm_rv + a16(FR * 4); sm_in = a16(sm_desc + desc_bytes); sm_end = sm_in + in_bytes + 64;
        copy_in = sm_end - 64 - sm_nfl;      // counters (zeros) + descriptors + input: one copy from pinned memory
        copy_out = sm_sf;                    // [output bytes | counters | out_bytes]: one copy back
    }
    size_t pin(size_t o) const { return o - sm_nfl; }
};
// what the phases of run_batch hand on
struct BatchPlan {
    TableSet* ts = nullptr;
    bool dev_io = false, resv = false, count_rej = false, use_frame = false, small = false;
    bool psy_lazy = false;                         // a large batch without the bit reservoir on the separate kernels: psyA in two parts around the scans, the short-block side only where it is read (plan_batch)
    bool count_f32 = false;                        // ... of count_rej: Float32 samples, counted by g_count_rejected (the WAV float types are counted where they are converted)
    // WAV sample types (k_ingest.h): streams whose samples g_ingest converts, its grid, the floats of all planes, the descriptors on the device
    int ingest = 0, ingest_tiles = 0; size_t ingest_floats = 0; const IngestDesc* dING = nullptr;
    int S = 0, nfs = 0, ngs = 0, nfr = 0, maxF = 0;
    uint32_t paths = 0;                            // LHIP_PATH_*: one bit per launch decision run_pipeline really takes for this batch (host-side record only)
    QuantLaunch ql;                                // ... and the shape of its speculative quantization launch (lhip_debug_read(11))
    int64_t pcm_plane = 0, in_total = 0, out_total = 0, repaired = 0, iters = 0;
    size_t in_bytes = 0, FR = 1;                   // in_bytes: host input as it travels: every job's samples in its format, jobs 4-byte aligned
    std::vector<StreamDesc> sd; std::vector<StreamIO> io;
    std::vector<int64_t> out_rel;                  // a stream's output offset inside the output area (sd.out_off becomes the absolute address in stage_inputs)
    CallLayout L; Workspace W;
    const StreamDesc* dSD = nullptr; const StreamIO* dIO = nullptr;
    // { infoTag } streams: where this call's music CRCs come from -- 0: no such stream, 1: the host's table CRC over the pinned mirror (small calls),
    // 2: g_out_crc over the bytes in HBM (crc_parts workgroups; results to crc_dst on the device, fetched into crc unless the caller keeps a log)
    int crc_mode = 0, crc_parts = 0;
    uint32_t* crc_dst = nullptr;
    std::vector<uint32_t> crc;                     // per stream
    // { replayGain } streams (lhip_gain.h): the two launches' plan and its descriptors on the device; gain.d is empty for a batch without the option
    GainPlan gain; const GainDesc* dGD = nullptr;
};

static bool plan_batch(Context* ctx, std::vector<Job>& jobs, bool dev_io, BatchPlan& P) {
    TableSet& ts = *jobs[0].s->ts;
    const Tables& T = ts.T;
    const int Cin = T.channels_in;                 // channels the caller hands over (2 with C == 1: downmix); everything that sizes or copies INPUT goes by it
    const int GR = T.mode_gr, frame = 576 * GR, mf_needed = 1024 + frame - 272;   // calcNeeded (Lame.js:1517-1530)
    const int S = (int)jobs.size();
    const bool resv = !T.disable_reservoir;       // bit reservoir (extension): the frames of a stream are a serial chain (g_resv_stream), output sizes known to the device only
    P.ts = &ts; P.dev_io = dev_io; P.S = S; P.resv = resv;
    P.sd.resize(S); P.io.resize(S);
    for (int i = 0; i < S; i++) {
        Job& j = jobs[i];
        lhip_stream* s = j.s;
        if (s->ts.get() != &ts) { set_err("batch: all streams must share one configuration"); return false; }
        if (T.rs_frac) {                     // non-integer ratio: the outputs of this call by the reference's own loop; a call it would not consume whole is refused
            FracPass fp = frac_pass(T, s->rs_itime, j.rs_len >= 0 ? j.rs_len : (double)j.n);
            if (j.n == 0 && j.rs_len < 0) fp = FracPass{0, 0.0, 0};      // an empty call is no call (Lame.js:1497)
            if ((fp.k >= frame && j.rs_len < 0) || (s->rs_flushed && j.n > 0)) { j.written = LHIP_ERR_INTERNAL; set_err(s->rs_flushed ? std::string("fractionalResample: the stream has been flushed") : frac_refusal(T, j.n)); return false; }
            j.n_out = fp.k; j.rs_used = fp.num_used;
        } else
        j.n_out = T.rs_ratio == 1 ? (int64_t)j.n : rs_outputs(s->rs_n_in + (int64_t)j.n, T.rs_ratio) - rs_outputs(s->rs_n_in, T.rs_ratio);
        const int64_t total = (int64_t)s->mf_size + j.n_out;
        if (total > 0x7fffffff || (int64_t)j.n > 0x7fffffff) { set_err("too many samples in one call"); return false; }
        j.F = total >= mf_needed ? (int)((total - mf_needed) / frame) + 1 : 0;
        j.bytes = batch_bytes(ts, s->slot_lag, j.F);
        if (resv)     // upper bound (the real count comes back from the device): the call's own frames, what earlier frames left in the
                      // reservoir (main data up to 511 bytes ahead of its header) and in the header queue, the flush padding
            j.bytes = (int64_t)j.F * (ts.base_frame_bytes + 1) + (j.F > 0 || j.flush ? 512 + RESV_HQ * RESV_HDR : 0) + (j.flush ? 1440 + RESV_HQ * RESV_HDR : 0);
        if ((size_t)j.bytes > j.cap) { j.written = LHIP_ERR_BUFFER_TOO_SMALL; set_err("output buffer too small"); return false; }
        StreamDesc& d = P.sd[i];
        memset(&d, 0, sizeof d);
        d.nframes = j.F; d.fslot0 = P.nfs; d.gslot0 = P.ngs; d.out_slot0 = P.nfr;
        d.pcm_off = P.pcm_plane; d.out_off = P.out_total; d.seg_len = (int)total; d.first_call = s->frame_num == 0;
        d.slot_lag = s->slot_lag; d.frame_num0 = s->frame_num; d.flush = (resv && j.flush) ? 1 : 0;
        P.nfs += j.F + 1; P.ngs += GR * j.F + 1; P.nfr += j.F;
        if (j.F > P.maxF) P.maxF = j.F;
        P.pcm_plane += (total + 63) & ~(int64_t)63;
        P.in_total += (int64_t)j.n; P.out_total += (j.bytes + 15) & ~(int64_t)15;
        if (fmt_ingest(j.type)) {      // raw bytes travel, or (a small call) the Float32 planes the host makes of them: room for either, 16-byte aligned
            const size_t b = fmt_bps(j.type);
            P.in_bytes += (j.n * (size_t)Cin * (b > 4 ? b : 4) + 15) & ~(size_t)15;
            if (j.n > 0) { P.ingest++; P.ingest_floats += (size_t)Cin * ((j.n + 3) & ~(size_t)3); }
        } else
        P.in_bytes += (j.n * (size_t)Cin * fmt_bps(j.type) + 3) & ~(size_t)3;
        P.count_f32 |= j.count_rejected && j.f32 && j.n > 0;
        P.count_rej |= j.count_rejected && (j.f32 || (fmt_ingest(j.type) && ingest_is_float(j.type))) && j.n > 0;
    }
    // at most one frame per stream: the whole frame program in one launch (kb_frame_stage); LAMEJS_HIP_NO_FRAME_KERNEL=1 keeps the separate kernels
    static const bool no_frame = []() { const char* e = getenv("LAMEJS_HIP_NO_FRAME_KERNEL"); return e && e[0] == '1'; }();
    // (one workgroup per stream at one wave per SIMD: beyond one stream per CU the separate kernels, each at full occupancy, are faster --
    //  bit-reservoir mode over 2048 streams: 0.7 M frames/s with this kernel, measured; the launch set of the separate kernels costs ~0.5 ms whatever S)
    P.use_frame = P.maxF <= 1 && !no_frame && S <= ctx->num_cus;
    // Short-block psychoacoustics only where a short granule (or the stream state) reads them: that needs the block types, so psyA runs in two launches around
    // the scans and reads its window twice -- worth it from a throughput-sized batch on (6 x CUs frame slots, where the quantization leaves the pair kernel; never
    // below 1024), and not with the bit reservoir, whose short pre-echo control reads the previous call's short thresholds whatever the block type.  Below the
    // threshold W.E holds all 122 entries of every call (lhip_debug_read(2)); in a lazy batch the short entries of a call nobody reads them from are zero.
    // LAMEJS_PSY_LAZY_MIN_FRAMES=<n> (read per batch; a test hook): the threshold in frame slots -- 0: always, a huge value: never.
    {
        const char* e = getenv("LAMEJS_PSY_LAZY_MIN_FRAMES");
        int64_t thr = 6 * (int64_t)ctx->num_cus < 1024 ? 1024 : 6 * (int64_t)ctx->num_cus;
        if (e && *e) { thr = atoll(e); if (thr < 0) thr = 0; }
        P.psy_lazy = !P.use_frame && !resv && (int64_t)P.nfs >= thr;
    }
    return true;
}
// every workspace array once: the buffer grows to `bytes` and W.name points at it
static bool bind_workspace(Context* ctx, BatchPlan& P) {
    WorkSet& ws = ctx->ws; const Tables& T = P.ts->T; Workspace& W = P.W; CallLayout& L = P.L;
    const int C = T.channels_out, S = P.S, nfs = P.nfs, ngs = P.ngs, nfr = P.nfr;
    memset(&W, 0, sizeof W);
    W.spec_start = g_spec_start; W.spec_step = g_spec_step; W.mode_gr = T.mode_gr;
    W.nstreams = S; W.nframes_total = nfr; W.nfslots = nfs; W.ngslots = ngs; W.pcm_plane = P.pcm_plane;
    const int Cp = T.psy_channels;
    const size_t GC = (size_t)ngs * C, GP = (size_t)ngs * Cp, FR = P.FR = (size_t)(nfr > 0 ? nfr : 1);
#define BIND(name, type, bytes) do { if (!ws.name.ensure(bytes)) return false; W.name = (type*)ws.name.p; } while (0)
    BIND(pcm, float, T.rs_ratio != 1 ? (size_t)P.pcm_plane * C * 4 + 64 : 64);
    BIND(peaks, float, GP * PK_STRIDE * 4); BIND(loud, float, GC * 4); BIND(eb_l, float, GP * EBL_STRIDE * 4); BIND(mask_idx, int32_t, GP * EBL_STRIDE * 4);
    BIND(eb_s, float, GP * EBS_STRIDE * 4); BIND(ecb_s, float, GP * EBS_STRIDE * 4); BIND(att_raw, int32_t, GP * 4); BIND(uselong, int32_t, GC * 4); BIND(ul_tmp, int32_t, GP * 4); BIND(last_attack, int32_t, GP * 4);
    BIND(tent, int32_t, GC * 4); BIND(prev_short, int32_t, GC * 4); BIND(blocktype, int32_t, GC * 4); BIND(ath_adjust, double, (size_t)nfs * 8);
    BIND(ath_limit, double, (size_t)nfs * 8); BIND(E, float, GP * E_STRIDE * 4); BIND(sb, float, GC * SB_STRIDE * 4); BIND(xr, float, GC * 576 * 4);
    BIND(att_clean, int32_t, GP * 4); BIND(nb1, float, GP * EBL_STRIDE * 4); BIND(nb2, float, GP * EBL_STRIDE * 4); BIND(fr, FrameResv, FR * sizeof(FrameResv)); BIND(out_bytes, int32_t, (size_t)S * 4 + 64);
    BIND(fht, float, Cp == 4 ? (size_t)ngs * 2 * FHT_STRIDE * 4 : 64); BIND(hpf, float, Cp == 4 ? (size_t)ngs * 2 * 576 * 4 : 64); BIND(tot_ener, float, (size_t)ngs * 4 * 4);
    BIND(side, GrSide, FR * 2 * C * sizeof(GrSide)); BIND(l3, int16_t, FR * 2 * C * 576 * 2); BIND(seed, int32_t, (size_t)nfs * C * 2 * 4);
    BIND(vdig, uint32_t, FR * 2 * C * VD_WORDS * 4);
    BIND(seed_flag, int32_t, FR * 4); BIND(reval, int32_t, FR * 4); BIND(nflagged, int32_t, 256); BIND(slow_list, int32_t, (size_t)nfs * 4); BIND(frame_bytes, int32_t, FR * 4);
    BIND(prof, unsigned long long, PROF_BYTES);
#undef BIND
    W.vdig_n = (int64_t)FR * 2 * C; W.work_ctr = W.nflagged + 16; W.out = nullptr;
    L.set(S, nfs, ngs, FR, P.out_total, P.in_bytes);
    static const bool no_small = []() { const char* e = getenv("LAMEJS_HIP_NO_SMALL_CALLS"); return e && e[0] == '1'; }();
    P.small = !P.dev_io && !no_small && L.sm_end <= SMALL_CALL_BYTES;
    if (P.small && !(ws.pin_in.ensure(L.pin(L.sm_end)) && ws.pin_out.ensure(L.copy_out))) P.small = false;       // no pinned memory: the general path
    if (P.small) {          // the counters and flags of a small call live in its block
        if (!ws.small.ensure(L.sm_end)) return false;
        uint8_t* const smb = (uint8_t*)ws.small.p;
        W.nflagged = (int32_t*)(smb + L.sm_nfl); W.work_ctr = W.nflagged + 16; W.out_bytes = (int32_t*)(smb + L.sm_ob);
        W.seed_flag = (int32_t*)(smb + L.sm_sf); W.reval = (int32_t*)(smb + L.sm_rv);
    } else if (!P.dev_io && !(ws.in16.ensure(P.in_bytes + 64) && ws.out8.ensure((size_t)P.out_total + 64))) return false;
    if (P.small) P.paths |= LHIP_PATH_SMALL_CALL;
    if (P.ts->tag.on) { P.crc_mode = P.small ? 1 : 2; P.crc.assign((size_t)S, 0u); }
    return true;
}
// { infoTag } streams whose bytes stay on the device: one descriptor per stream for g_out_crc (the byte count of a bit-reservoir stream is read on the device)
static bool stage_crc(Context* ctx, const std::vector<Job>& jobs, BatchPlan& P, uint32_t* crc_log) {
    WorkSet& ws = ctx->ws; const int S = P.S;
    std::vector<CrcDesc> cd((size_t)S);
    int64_t parts = 0;
    for (int i = 0; i < S; i++) {
        CrcDesc& d = cd[i];
        d.base = P.io[i].out; d.n = jobs[i].bytes; d.n_dev = P.resv ? P.W.out_bytes + i : nullptr;      // (jobs[i].bytes: exact, or the reservoir's upper bound)
        d.part0 = (int32_t)parts; d.nparts = (int32_t)((jobs[i].bytes + CRC_SPAN_BYTES - 1) / CRC_SPAN_BYTES);
        parts += d.nparts;
    }
    if (parts > 0x7fffffff) { set_err("too many output bytes in one call for the Info tag's CRC"); return false; }
    P.crc_parts = (int)parts;
    if (!ws.crc_desc.ensure((size_t)S * sizeof(CrcDesc)) || !ws.crc_part.ensure((size_t)parts * 4 + 64) || !ws.crc_out.ensure((size_t)S * 4 + 64)) return false;
    if (!rt::h2d(ws.crc_desc.p, cd.data(), (size_t)S * sizeof(CrcDesc), ctx->stream)) return false;
    P.crc_dst = crc_log ? crc_log : (uint32_t*)ws.crc_out.p;
    return true;
}
// { replayGain } streams: every stream of the batch analyses the n_out samples this call appends to its buffer (Lame.js:1609-1613) -- rows and descriptors
static bool stage_gain(Context* ctx, const std::vector<Job>& jobs, BatchPlan& P) {
    WorkSet& ws = ctx->ws; const int S = P.S;
    std::vector<GainRec*> recs((size_t)S); std::vector<int64_t> n((size_t)S);
    for (int i = 0; i < S; i++) { recs[i] = jobs[i].s->gain.get(); n[i] = jobs[i].n_out; }
    if (!gain_plan(recs.data(), n.data(), S, P.gain)) return false;
    if (P.gain.stage_blocks == 0) return true;
    if (!ws.gain_rows.ensure(P.gain.row_floats * 4 + 64) || !ws.gain_desc.ensure((size_t)S * sizeof(GainDesc))) return false;
    gain_bind_rows(P.gain, (float*)ws.gain_rows.p);
    if (!rt::h2d(ws.gain_desc.p, P.gain.d.data(), (size_t)S * sizeof(GainDesc), ctx->stream)) return false;
    P.dGD = (const GainDesc*)ws.gain_desc.p;
    return true;
}
static bool stage_inputs(Context* ctx, std::vector<Job>& jobs, BatchPlan& P) {
    WorkSet& ws = ctx->ws; void* st = ctx->stream; const Tables& T = P.ts->T; Workspace& W = P.W; const CallLayout& L = P.L;
    std::vector<StreamDesc>& sd = P.sd; std::vector<StreamIO>& io = P.io; std::vector<int64_t>& out_rel = P.out_rel;
    const int S = P.S, Cin = T.channels_in, GR = T.mode_gr, nfs = P.nfs, ngs = P.ngs; const size_t FR = P.FR; const bool small = P.small, dev_io = P.dev_io, resv = P.resv;
    uint8_t* const smb = (uint8_t*)ws.small.p;
    std::vector<int32_t> fmap(nfs), gmap(ngs);
    out_rel.resize(S);
    size_t in_off = 0;                            // bytes
    uint8_t* const pin = small ? (uint8_t*)ws.pin_in.p : nullptr;       // mirrors the device block from L.sm_nfl on
    if (small) memset(pin, 0, L.pin(L.sm_desc));                       // the counters start from zero
    for (int i = 0; i < S; i++) {
        Job& j = jobs[i];
        for (int k = 0; k <= j.F; k++) fmap[sd[i].fslot0 + k] = i;
        for (int k = 0; k <= GR * j.F; k++) gmap[sd[i].gslot0 + k] = i;
        StreamIO& o = io[i];
        o.state = j.s->d_state; o.n_new = (int)j.n_out; o.mf_size = j.s->mf_size; o.n_in = (int)j.n;
        o.rs_p0 = T.rs_ratio <= 1 ? 0 : (int)(rs_outputs(j.s->rs_n_in, T.rs_ratio) * T.rs_ratio - 16 - j.s->rs_n_in);
        o.rs_itime = j.s->rs_itime;
        out_rel[i] = sd[i].out_off;
        const size_t bps = fmt_bps(j.type);
        const bool il = j.inter && Cin == 2;          // (one channel: interleaved is planar)
        const bool ing = fmt_ingest(j.type);
        o.f32 = j.f32 ? 1 : 0; o.stride = il ? 2 : 1;
        if (ing && small) {          // a small call: the host converts while it fills the pinned block -- Float32 planes, no launch
            uint8_t* base = smb + L.sm_in; uint8_t* hbase = pin + L.pin(L.sm_in);
            float* h0 = (float*)(hbase + in_off); float* h1 = Cin == 2 ? h0 + j.n : nullptr;
            const bool one = Cin == 2 && !il && (!j.r || j.r == j.l);          // right == left: the samples exist once
            (void)ingest_host(j.type, j.l, j.r, j.n, one ? 1 : Cin, il, h0, h1, T.pcm_limit);
            o.f32 = 1; o.stride = 1;
            o.src[0] = base + in_off; o.src[1] = (Cin == 2 && !one) ? base + in_off + j.n * 4 : o.src[0];
            in_off = (in_off + j.n * 4 * (size_t)Cin + 15) & ~(size_t)15;
            o.out = smb + L.sm_out + sd[i].out_off;
            continue;
        }
        if (dev_io) {
            o.src[0] = j.l; o.src[1] = il ? (const void*)((const uint8_t*)j.l + bps) : ((Cin == 2 && j.r) ? j.r : j.l); o.out = j.out;
        } else {
            uint8_t* base = small ? smb + L.sm_in : (uint8_t*)ws.in16.p;
            uint8_t* hbase = small ? pin + L.pin(L.sm_in) : nullptr;
            const size_t plane = j.n * bps * (il ? 2 : 1);          // an interleaved call is ONE copy
            o.src[0] = base + in_off;
            if (small) memcpy(hbase + in_off, j.l, plane);
            else if (!rt::h2d((void*)o.src[0], j.l, plane, st)) return false;
            if (il) o.src[1] = base + in_off + bps;
            in_off += plane;
            if (Cin == 2 && !il) {
                o.src[1] = base + in_off;
                if (small) memcpy(hbase + in_off, j.r ? j.r : j.l, plane);
                else if (!rt::h2d((void*)o.src[1], j.r ? j.r : j.l, plane, st)) return false;
                in_off += plane;
            } else if (!il) o.src[1] = o.src[0];
            in_off = ing ? (in_off + 15) & ~(size_t)15 : (in_off + 3) & ~(size_t)3;
            o.out = (small ? smb + L.sm_out : (uint8_t*)ws.out8.p) + sd[i].out_off;
        }
    }
    // WAV sample types: o.src[] are the raw samples on the device by now; g_ingest's descriptors are made of them and the stream reads the planes instead
    if (P.ingest && !small) {
        if (!ws.ingest.ensure(P.ingest_floats * 4 + 64) || !ws.ingest_desc.ensure((size_t)S * sizeof(IngestDesc))) return false;
        std::vector<IngestDesc> id((size_t)S);
        float* plane = (float*)ws.ingest.p;
        int64_t blk = 0;
        for (int i = 0; i < S; i++) {
            const Job& j = jobs[i]; StreamIO& o = io[i]; IngestDesc& d = id[i];
            memset(&d, 0, sizeof d);
            d.blk0 = (int32_t)blk; d.type = j.type;
            if (!fmt_ingest(j.type) || j.n == 0) continue;
            const bool il = j.inter && Cin == 2;
            const bool two = Cin == 2 && !il && o.src[1] != o.src[0];
            const size_t pl = (j.n + 3) & ~(size_t)3;
            d.src[0] = (const uint8_t*)o.src[0]; d.src[1] = two ? (const uint8_t*)o.src[1] : nullptr;
            d.dst[0] = plane; d.dst[1] = (il || two) ? plane + pl : plane;
            d.inter = il ? 1 : 0; d.narr = two ? 2 : 1; d.nelem = (int64_t)j.n * (il ? 2 : 1); d.tiles = ingest_tiles(j.type, d.nelem);
            blk += d.tiles * d.narr;
            o.f32 = 1; o.stride = 1; o.src[0] = d.dst[0]; o.src[1] = d.dst[1];
            plane += pl * (size_t)Cin;
        }
        if (blk > 0x7fffffff) { set_err("too many samples in one call"); return false; }
        P.ingest_tiles = (int)blk;
        if (!rt::h2d(ws.ingest_desc.p, id.data(), (size_t)S * sizeof(IngestDesc), st)) return false;
        P.dING = (const IngestDesc*)ws.ingest_desc.p;
    }
    // All descriptors travel in ONE host-to-device copy (a small pageable copy costs ~10 us of host time each, and a 1-frame
    // call is only ~0.4 ms long): [StreamDesc x S | StreamIO x S | frame-slot map | granule-slot map], 16-byte aligned parts.
    // The out pointer per stream is carried in StreamIO; kb_bits reads W.out + sd.out_off, so W.out is a zero base and
    // out_off holds the absolute address (the device address space is 64-bit).
    if (!small && !ws.desc.ensure(L.desc_bytes)) return false;
    uint8_t* const ddesc = small ? smb + L.sm_desc : (uint8_t*)ws.desc.p;
    {
        std::vector<uint8_t> stage_v;
        uint8_t* stage = nullptr;
        if (small) stage = pin + L.pin(L.sm_desc);
        else { stage_v.assign(L.desc_bytes, 0); stage = stage_v.data(); }
        if (small) memset(stage, 0, L.sm_in - L.sm_desc);
        for (int i = 0; i < S; i++) sd[i].out_off = (int64_t)(uintptr_t)io[i].out;
        memcpy(stage + L.desc_sd, sd.data(), (size_t)S * sizeof(StreamDesc));
        memcpy(stage + L.desc_io, io.data(), (size_t)S * sizeof(StreamIO));
        memcpy(stage + L.desc_fm, fmap.data(), (size_t)nfs * 4);
        memcpy(stage + L.desc_gm, gmap.data(), (size_t)ngs * 4);
        if (small) { if (!rt::h2d(smb + L.sm_nfl, pin, L.copy_in, st)) return false; }      // counters (zeros) + descriptors + input: one copy from pinned memory
        else if (!rt::h2d(ddesc, stage, L.desc_bytes, st)) return false;
    }
    W.fslot_stream = (const int32_t*)(ddesc + L.desc_fm); W.gslot_stream = (const int32_t*)(ddesc + L.desc_gm);
    if (!small) {
        if (!rt::dzero(ws.seed_flag.p, FR * 4, st)) return false;
        if (!rt::dzero(ws.reval.p, FR * 4, st)) return false;
        if (resv && !rt::dzero(ws.out_bytes.p, (size_t)S * 4, st)) return false;
        if (!rt::dzero(ws.nflagged.p, 256, st)) return false;
    }
#if defined(LHIP_PHASE_PROF) || defined(LHIP_WAVE_TIMES)
    if (!rt::dzero(ws.prof.p, PROF_BYTES, st)) return false;      // (the product never reads these counters)
#endif
    P.dSD = (const StreamDesc*)(ddesc + L.desc_sd);
    P.dIO = (const StreamIO*)(ddesc + L.desc_io);
    W.io = P.dIO;
    return true;
}
static bool fetch_outputs(Context* ctx, std::vector<Job>& jobs, BatchPlan& P, bool want_sync, int32_t* fx_dst, bool fetch_fx, int32_t (&fx)[3], bool fetch_crc) {
    WorkSet& ws = ctx->ws; void* st = ctx->stream; const Workspace& W = P.W; const CallLayout& L = P.L;
    const int S = P.S, nfr = P.nfr; const bool small = P.small, dev_io = P.dev_io, resv = P.resv;
    const uint8_t* const smb = (const uint8_t*)ws.small.p;
    if (fx_dst) {
        if (nfr > 0) { if (!rt::d2d(fx_dst, (const uint8_t*)W.nflagged + FX_STATS_OFF, 12, st)) return false; }
        else if (!rt::dzero(fx_dst, 12, st)) return false;
    }
    // ---- outputs ----
    if (small) {
        // one copy out: [output bytes | counters | out_bytes], then the callers' buffers are filled from the pinned mirror
        const uint8_t* po = (const uint8_t*)ws.pin_out.p;
        if (!rt::d2h(ws.pin_out.p, smb, L.copy_out, st) || !rt::sync(st)) return false;
        memcpy(fx, po + L.sm_nfl + FX_STATS_OFF, sizeof fx);
        if (resv) for (int i = 0; i < S; i++) jobs[i].bytes = ((const int32_t*)(po + L.sm_ob))[i];
        for (int i = 0; i < S; i++) if (jobs[i].bytes > 0) memcpy(jobs[i].out, po + L.sm_out + P.out_rel[i], (size_t)jobs[i].bytes);
        if (P.crc_mode == 1) for (int i = 0; i < S; i++) P.crc[i] = crc16r_host(po + L.sm_out + P.out_rel[i], (size_t)jobs[i].bytes);      // { infoTag }: the bytes are here anyway
    } else {
        if (fetch_fx && !rt::d2h(fx, (const int32_t*)ws.nflagged.p + FX_STATS_OFF / 4, sizeof fx, st)) return false;
        std::vector<int32_t> ob;
        if (resv) {                                   // how much each stream really wrote
            ob.assign((size_t)S, 0);
            if (!rt::d2h(ob.data(), ws.out_bytes.p, (size_t)S * 4, st) || !rt::sync(st)) return false;
            for (int i = 0; i < S; i++) jobs[i].bytes = ob[i];
        }
        if (fetch_crc && !rt::d2h(P.crc.data(), P.crc_dst, (size_t)S * 4, st)) return false;      // { infoTag }: rides with the copies back; a device-pointer call waits for it
        if (!dev_io) {
            for (int i = 0; i < S; i++)
                if (jobs[i].bytes > 0 && !rt::d2h(jobs[i].out, P.io[i].out, (size_t)jobs[i].bytes, st)) return false;
            if (!rt::sync(st)) return false;
        } else if (want_sync || fetch_crc) {
            if (!rt::sync(st)) return false;
        }
    }
    return true;
}
// host-side stream bookkeeping (Lame.js:1629-1661)
static void advance_streams(std::vector<Job>& jobs, const Tables& T) {
    const int frame = 576 * T.mode_gr;
    for (int i = 0; i < (int)jobs.size(); i++) {
        Job& j = jobs[i];
        lhip_stream* s = j.s;
        const int64_t total = (int64_t)s->mf_size + j.n_out;
        if (j.n > 0) {
            if (s->mf_samples_to_encode < 1) s->mf_samples_to_encode = 576 + 1152;
            s->mf_samples_to_encode += (int)j.n_out;
        }
        s->rs_n_in += (int64_t)j.n;
        if (T.rs_frac) {                     // Lame.js:1813 (num_used == the call's length: the pass used it whole), 1373-1379
            const double len = j.rs_len >= 0 ? j.rs_len : (double)j.n;
            s->rs_itime += j.rs_used - j.n_out * T.resample_ratio;
            if (s->rs_inbuf_len == 0 || s->rs_inbuf_nsamples < len) { s->rs_inbuf_len = (int64_t)floor(len); s->rs_inbuf_nsamples = len; }
        }
        s->mf_samples_to_encode -= frame * j.F;
        s->mf_size = (int)(total - (int64_t)frame * j.F);
        if (T.frac_SpF != 0 && j.F > 0) {
            int64_t m = ((int64_t)s->slot_lag - (int64_t)j.F * T.frac_SpF) % T.out_samplerate;
            if (m < 0) m += T.out_samplerate;
            s->slot_lag = (int)m;
        }
        s->frame_num += j.F;
        j.written = j.bytes;
    }
}

#ifdef LHIP_HOSTSIM
#include "lhip_pipeline_sim.h"
#else
#include "lhip_pipeline_hip.h"
#endif

// fx_dst (device, optional): where this batch's repair verdict (three words: repaired frames, iterations, "did not converge") is copied on the launch
// stream while ctx->mu is still held -- the chunked host path logs one per unit, and another thread's batch on the same device must not get in between
// crc_log (device, optional; { infoTag } streams): where this batch's music CRCs (one word per stream) are left instead of being fetched -- the caller reads its log once
// and does the streams' tag accounting itself (tag_account)
static bool run_batch(Context* ctx, std::vector<Job>& jobs, bool dev_io, bool want_sync, int32_t* fx_dst = nullptr, uint32_t* crc_log = nullptr) {
    if (jobs.empty()) return true;
#ifdef LHIP_PHASE_PROF
    auto cp_t_ = std::chrono::steady_clock::now();
    g_call_prof[7] += 1;
#endif
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rt::set_device(ctx->device)) return false;
    BatchPlan P;
    if (!plan_batch(ctx, jobs, dev_io, P) || !bind_workspace(ctx, P)) return false;
    CALL_STAMP(0);                                  // plan + workspace
    if (!stage_inputs(ctx, jobs, P)) return false;
    if (P.crc_mode == 2 && !stage_crc(ctx, jobs, P, crc_log)) return false;
    if (P.ts->gain_on && !stage_gain(ctx, jobs, P)) return false;
    CALL_STAMP(1);                                  // input copies, descriptors, counters zeroed: enqueued

    g_rejected = 0; g_rej_pending = nullptr;
    if (!run_pipeline(ctx, P)) return false;
    if (P.gain.stage_blocks > 0) { for (int i = 0; i < P.S; i++) if (P.gain.d[i].n > 0) { GainRec& g = *jobs[i].s->gain; g.samples += P.gain.d[i].n; g.cur ^= 1; } }      // (enqueued: the records move on)
    CALL_STAMP(2);                                  // kernels enqueued
    // repair statistics live on the device; they travel with the final synchronisation when there is one, else they are fetched
    // when somebody asks (lhip_last_batch_stats)
    int32_t fx[3] = {0, 0, 0};
    const bool fetch_fx = P.nfr > 0 && (!dev_io || want_sync || g_kt_on_());
    if (!fetch_outputs(ctx, jobs, P, want_sync, fx_dst, fetch_fx, fx, P.crc_mode == 2 && !crc_log) || !collect_kernel_times(ctx->stream)) return false;
    CALL_STAMP(3);                                  // output copies + synchronisation
    advance_streams(jobs, P.ts->T);
    if (P.crc_mode && !crc_log) for (int i = 0; i < P.S; i++) tag_account(*jobs[i].s->tag, jobs[i].F, jobs[i].bytes, P.crc[i], P.ts->T.brate);
    if (!collect_repair_stats(ctx, P, fetch_fx, fx)) return false;
    g_stat_frames = P.nfr; g_stat_repaired = P.repaired; g_stat_iters = P.iters; g_last_paths = P.paths; g_last_quant = P.ql;
    WorkSet& ws = ctx->ws;
    ws.lastW = P.W; ws.lastC = P.ts->T.channels_out; ws.lastCp = P.ts->T.psy_channels; ws.have_last = true;
    { std::lock_guard<std::mutex> lk(g_ctx_mu); g_last_batch_ctx = ctx; }
    return true;
}
