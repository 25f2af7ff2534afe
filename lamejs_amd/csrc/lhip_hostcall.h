// lhip_hostcall.h -- host-buffer calls: the chunked / pipelined path for long inputs and many streams, and the Float32 scan of host samples.
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// Host-buffer calls with many frames (what encodeBuffer() hands over when a caller passes a long Int16Array): the call is cut into
// chunks of whole frames' worth of samples; chunk k + 1 travels to the device (copy stream) while chunk k is encoded (launch stream)
// and the bytes of chunk k - 1 travel back -- PCIe needs about a sixth of the encode time, so it hides behind it.  Any chunking of a
// sample stream gives the same bytes (the library's basic contract), so the result is what one batch gives.  Not for the bit
// reservoir (its byte counts are only known after each launch).
enum { HOST_CHUNK_FRAMES = 8192 };
// chunk schedule: the first chunk is small (its copy is the part of the call nothing overlaps), every later one twice the one before up
// to a cap -- a chunk's copy still fits inside the encode of the chunk before it, and large chunks keep the persistent quantization
// kernel's waves busy (at 8192 frames a wave draws two frames and every launch ends on its slowest one: 1e5 stereo frames took 72.5 ms
// in 8192-frame chunks, 58.3 ms with 8192 doubling to 32768, 60.0 ms as one batch with nothing overlapped; tests/tools/dropin_sweep.py).
// Two-channel streams take chunks of twice the frames (a stereo frame is four to five times the work of a mono frame, so a chunk's fixed
// costs -- the launch tails -- weigh the same at twice the size, and its copy hides as well): 16384 doubling to 65536 measured 52.0 ms
// against 53.8 ms with the mono schedule on the final code of round 3, mono the other way round (11.96 vs 12.52 ms;
// profiles/r03_dropin_host_chunk_sweep.txt).  LAMEJS_HIP_HOST_CHUNK_FRAMES=first[,cap[,growth]] overrides both (tuning, tests).
struct ChunkSchedule { size_t first = HOST_CHUNK_FRAMES, cap = 4 * HOST_CHUNK_FRAMES, growth = 2; bool fixed = false; };
static const ChunkSchedule& host_chunk_schedule() {
    static const ChunkSchedule cs = []() {           // read once (function-local static: initialised exactly once, whichever thread comes first)
        ChunkSchedule c;
        if (const char* e = getenv("LAMEJS_HIP_HOST_CHUNK_FRAMES")) {
            char* end = nullptr;
            const unsigned long v = strtoul(e, &end, 10);
            if (v >= 1 && v <= (1ul << 20)) { c.first = v; c.cap = v; c.fixed = true; }
            if (end && *end == ',') {
                const unsigned long w = strtoul(end + 1, &end, 10); if (w >= c.first && w <= (1ul << 20)) c.cap = w;
                if (end && *end == ',') { const unsigned long gr = strtoul(end + 1, nullptr, 10); if (gr >= 2 && gr <= 8) c.growth = gr; }
            }
        }
        return c;
    }();
    return cs;
}
// One piece of host input for one stream: `n` samples per channel from l / r; its frames' bytes go to the stream's destination (running).
struct HostPiece { int si; const void* l; const void* r; size_t n; };
// The overlapped host path, in general form: `units` are processed in order, each a batch of pieces (one per stream at most) -- unit k + 1
// travels to the device (copy stream) while unit k is encoded (launch stream) and the bytes of unit k - 1 travel back.  For ONE long stream
// the units are consecutive sample ranges of its input (encode_host_chunked); for MANY streams (lhip_encode_batch with host buffers,
// BASELINE configs[4] through the JavaScript encodeBatch) they are groups of streams.  dst[si] / cap[si]: stream si's output buffer;
// written[si] receives its byte count.  A failed call gives every stream back as it found it.
static int encode_host_pipelined(Context* ctx, const std::vector<lhip_stream*>& strs, const std::vector<std::vector<HostPiece>>& units, int format,
                                 uint8_t* const* dst, int64_t* written) {
    std::lock_guard<std::mutex> chunk_lk(ctx->chunk_mu);
    const size_t NS = strs.size();
    const Tables& T = strs[0]->ts->T;
    const int C = T.channels_in;                   // this function only moves INPUT: a downmix stream hands over two channels
    const size_t obytes = (size_t)(strs[0]->ts->base_frame_bytes + 1);
    const size_t spf = (size_t)576 * T.mode_gr * T.rs_ratio;             // input samples per frame
    // staging halves sized for the largest unit of THIS call: samples per channel (pieces back to back, each rounded up to 64) and output bytes
    size_t in_max = 0, out_max = 0;
    for (const auto& u : units) {
        size_t a = 0, o = 0;
        for (const HostPiece& pc : u) { a += (pc.n + 63) & ~(size_t)63; o += ((pc.n / spf + 3) * obytes + 63) & ~(size_t)63; }
        if (a > in_max) in_max = a;
        if (o > out_max) out_max = o;
    }
    const size_t stride = in_max, out_chunk = out_max + 64;
    const size_t bps = fmt_bps(fmt_type(format));
    const bool il = (format & LHIP_PCM_INTERLEAVED) && C == 2;
    // { infoTag } streams: every piece's music CRC stays on the device in the call's log (run_batch: crc_log) and the totals of the streams are brought up to date
    // once, after the last unit -- a failed call has then changed none of them
    const bool tagged = strs[0]->ts->tag.on != 0;
    struct TagRec { int si, F; int64_t bytes; };
    std::vector<TagRec> tag_recs;
    size_t npieces = 0;
    for (const auto& u : units) npieces += u.size();
    // what a failed call must give back: the host-side counters and the device-side state record of every stream (a call that fails in unit
    // k > 0 would otherwise leave streams k units further on with `out` half written -- "a failed call consumes nothing" has to hold here too)
    struct Snap { int mf, ste, lag; int64_t fn, rs; };
    std::vector<Snap> snap(NS);
    for (size_t i = 0; i < NS; i++) snap[i] = Snap{strs[i]->mf_size, strs[i]->mf_samples_to_encode, strs[i]->slot_lag, strs[i]->frame_num, strs[i]->rs_n_in};
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!rt::set_device(ctx->device)) return LHIP_ERR_INTERNAL;
        if (!ctx->copy_stream) {
            void* cs = nullptr; void* e[4] = {nullptr, nullptr, nullptr, nullptr};
            if (!rt::stream_create(&cs)) return LHIP_ERR_INTERNAL;
            for (int i = 0; i < 4; i++) if (!rt::event_create(&e[i])) return LHIP_ERR_INTERNAL;
            ctx->ev_in[0] = e[0]; ctx->ev_in[1] = e[1]; ctx->ev_done[0] = e[2]; ctx->ev_done[1] = e[3]; ctx->copy_stream = cs;
        }
        if (!ctx->chunk_in.ensure(2 * C * stride * bps + 64) || !ctx->chunk_out.ensure(2 * out_chunk) || !ctx->chunk_fx.ensure(units.size() * 16 + 16) || (tagged && !ctx->chunk_crc.ensure(npieces * 4 + 16)) ||
            !ctx->state_bak.ensure(NS * sizeof(StreamState))) return LHIP_ERR_INTERNAL;
        for (size_t i = 0; i < NS; i++)
            if (!rt::d2d((uint8_t*)ctx->state_bak.p + i * sizeof(StreamState), strs[i]->d_state, sizeof(StreamState), ctx->stream)) return LHIP_ERR_INTERNAL;
    }
    void* cs = ctx->copy_stream; void* ks = ctx->stream;
    int64_t frames_all = 0, repaired_all = 0, iters_all = 0;
    uint32_t paths_all = 0;
    std::vector<int64_t> total(NS, 0);
    struct Pending { uint8_t* dst; const uint8_t* src; int64_t bytes; };
    std::vector<Pending> pending; int pending_par = 0; bool have_pending = false;      // the unit whose output is still on the device
    auto fail = [&](const char* what, int64_t code = LHIP_ERR_INTERNAL) -> int {      // wait for everything in flight, then put the streams back where the call found them
        const std::string why = what ? std::string(what) : g_err;
        (void)rt::sync(cs); (void)rt::sync(ks);
        for (size_t i = 0; i < NS; i++) {
            (void)rt::d2d(strs[i]->d_state, (const uint8_t*)ctx->state_bak.p + i * sizeof(StreamState), sizeof(StreamState), ks);
            if (strs[i]->gain) strs[i]->gain->moved = true;      // (the units already analysed are in its histogram: lhip_replay_gain refuses from here on)
            strs[i]->mf_size = snap[i].mf; strs[i]->mf_samples_to_encode = snap[i].ste; strs[i]->slot_lag = snap[i].lag; strs[i]->frame_num = snap[i].fn; strs[i]->rs_n_in = snap[i].rs;
        }
        (void)rt::sync(ks);
        set_err(why);
        return (int)code;
    };
    auto drain = [&]() -> bool {               // copy the pending unit's bytes out; ALWAYS waits for that unit's kernels (its input half is reused next)
        if (!have_pending) return true;
        have_pending = false;
        if (!rt::stream_wait_event(cs, ctx->ev_done[pending_par])) return false;
        for (const Pending& q : pending) if (q.bytes > 0 && !rt::d2h(q.dst, q.src, (size_t)q.bytes, cs)) return false;
        return rt::sync(cs);
    };
    // LAMEJS_HIP_TRACE_CHUNKS=1: host-side timeline of the call on stderr (ms since the call began: after the input copies were issued, after the
    // kernels were enqueued, after the previous unit's bytes arrived) -- where a slow caller-side buffer shows
    static const bool trace_chunks = []() { const char* e = getenv("LAMEJS_HIP_TRACE_CHUNKS"); return e && e[0] == '1'; }();
    const auto t_call = std::chrono::steady_clock::now();
    auto ms_now = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    for (size_t k = 0; k < units.size(); k++) {
        const int par = (int)(k & 1);
        const std::vector<HostPiece>& u = units[k];
        const double t_a = trace_chunks ? ms_now() : 0.0;
        uint8_t* d_in = (uint8_t*)ctx->chunk_in.p + (size_t)par * C * stride * bps;
        uint8_t* d_out = (uint8_t*)ctx->chunk_out.p + (size_t)par * out_chunk;
        // buffer `par` was last used by unit k - 2: its kernels are done (drain() waited for them before unit k - 1 was enqueued)
        // (copies straight from the caller's pageable memory: measured as fast as copies through pinned staging filled by four host
        //  threads -- 72.5 vs 73.2 ms per 1e5 stereo frames at 8192-frame chunks -- so there is no staging layer)
        std::vector<Job> jobs(u.size());
        size_t io = 0, oo = 0;
        for (size_t j = 0; j < u.size(); j++) {
            const HostPiece& pc = u[j];
            const size_t ocap = ((pc.n / spf + 3) * obytes + 63) & ~(size_t)63;
            if (il) {                                      // interleaved two-channel input: one copy, read with stride 2
                if (!rt::h2d(d_in + 2 * io * bps, pc.l, 2 * pc.n * bps, cs)) return fail(nullptr);
                jobs[j] = Job{strs[pc.si], d_in + 2 * io * bps, nullptr, pc.n, d_out + oo, ocap, 0, 0, 0, 0};
            } else {
                if (!rt::h2d(d_in + io * bps, pc.l, pc.n * bps, cs)) return fail(nullptr);
                if (C == 2 && !rt::h2d(d_in + (stride + io) * bps, pc.r ? pc.r : pc.l, pc.n * bps, cs)) return fail(nullptr);
                jobs[j] = Job{strs[pc.si], d_in + io * bps, C == 2 ? d_in + (stride + io) * bps : nullptr, pc.n, d_out + oo, ocap, 0, 0, 0, 0};
            }
            jobs[j].set_format(format);
            io += (pc.n + 63) & ~(size_t)63; oo += ocap;
        }
        if (!rt::event_record(ctx->ev_in[par], cs) || !rt::stream_wait_event(ks, ctx->ev_in[par])) return fail(nullptr);
        const double t_b = trace_chunks ? ms_now() : 0.0;
        // (this unit's repair verdict stays on the device until the call ends: run_batch copies it into the call's log -- stream-ordered, under the context's
        //  lock -- and the log is read back once after the last unit)
        if (!run_batch(ctx, jobs, true, false, (int32_t*)ctx->chunk_fx.p + 4 * k, tagged ? (uint32_t*)ctx->chunk_crc.p + tag_recs.size() : nullptr)) { int64_t code = LHIP_ERR_INTERNAL; for (const Job& j : jobs) if (j.written < 0) { code = j.written; break; } return fail(nullptr, code); }
#ifdef LHIP_HOSTSIM
        // tests: a failure injected after unit k has been consumed (the streams must come back as the call found them)
        if (const char* e = getenv("LHIP_HOSTSIM_FAIL_CHUNK")) if (e[0] && (size_t)atoi(e) == k) return fail("injected failure (LHIP_HOSTSIM_FAIL_CHUNK)");
        repaired_all += g_stat_repaired; iters_all += g_stat_iters;
#endif
        if (!rt::event_record(ctx->ev_done[par], ks)) return fail(nullptr);
        const double t_c = trace_chunks ? ms_now() : 0.0;
        if (!drain()) return fail(nullptr);             // unit k - 1, while unit k is being encoded
        if (trace_chunks) fprintf(stderr, "[lhip unit %zu: %zu piece(s)] begin %.2f  copies issued %.2f  kernels enqueued %.2f  previous unit's bytes home %.2f ms\n", k, u.size(), t_a, t_b, t_c, ms_now());
        pending.clear();
        for (size_t j = 0; j < u.size(); j++) {
            const int si = u[j].si;
            pending.push_back(Pending{dst[si] + total[si], jobs[j].out, jobs[j].written});
            total[si] += jobs[j].written;
            if (tagged) tag_recs.push_back(TagRec{si, jobs[j].F, jobs[j].written});
        }
        pending_par = par; have_pending = true;
        frames_all += g_stat_frames; paths_all |= g_last_paths;
    }
    if (!drain()) return fail(nullptr);
    if (trace_chunks) fprintf(stderr, "[lhip units] last unit's bytes home %.2f ms\n", ms_now());
#ifndef LHIP_HOSTSIM
    {
        std::vector<int32_t> fx(4 * units.size(), 0);
        if (!rt::d2h(fx.data(), ctx->chunk_fx.p, fx.size() * 4, ks) || !rt::sync(ks)) return fail(nullptr);
        bool bad = false;
        for (size_t k = 0; k < units.size(); k++) { repaired_all += fx[4 * k]; iters_all += fx[4 * k + 1]; bad |= fx[4 * k + 2] != 0; }
        if (bad) return fail("seed-chain repair did not converge");
    }
    g_stat_pending = nullptr;
#endif
    if (tagged) {
        std::vector<uint32_t> crcs(tag_recs.size(), 0u);
        if (!rt::d2h(crcs.data(), ctx->chunk_crc.p, crcs.size() * 4, ks) || !rt::sync(ks)) return fail(nullptr);
        for (size_t i = 0; i < tag_recs.size(); i++) tag_account(*strs[tag_recs[i].si]->tag, tag_recs[i].F, tag_recs[i].bytes, crcs[i], T.brate);
    }
    g_stat_frames = frames_all; g_stat_repaired = repaired_all; g_stat_iters = iters_all;     // lhip_last_batch_stats: the whole call
    g_last_paths = paths_all;                                                                 // lhip_debug_last_paths: every path one of its units took
    for (size_t i = 0; i < NS; i++) written[i] = total[i];
    return 0;
}

// ONE long stream: consecutive sample ranges of the call (chunk schedule above)
static int64_t encode_host_chunked(lhip_stream* s, int format, const void* left, const void* right, size_t nsamples, uint8_t* out, size_t out_cap) {
    const Tables& T = s->ts->T;
    const ChunkSchedule& cfg = host_chunk_schedule();
    const size_t mul = (!cfg.fixed && T.channels_out == 2) ? 2 : 1;      // (the schedule follows the encode's cost: output channels)
    const size_t spf = (size_t)576 * T.mode_gr * T.rs_ratio;
    // the whole call must fit the caller's buffer BEFORE anything is consumed (a failed call consumes nothing)
    if ((size_t)batch_bytes(*s->ts, s->slot_lag, call_frames(s, nsamples)) > out_cap) { set_err("output buffer too small"); return LHIP_ERR_BUFFER_TOO_SMALL; }
    std::vector<std::vector<HostPiece>> units;
    const bool il = (format & LHIP_PCM_INTERLEAVED) && T.channels_in == 2;
    const size_t step = fmt_bps(fmt_type(format)) * (il ? 2 : 1);       // bytes from one sample position of the call to the next
    {
        const size_t cap = cfg.cap * mul * spf;
        size_t p = 0, cur = cfg.first * mul * spf;
        while (p < nsamples) {
            size_t m = nsamples - p < cur ? nsamples - p : cur;
            if (nsamples - p - m < m / 4 && nsamples - p <= cap) m = nsamples - p;     // no short chunk at the end: a launch for a few frames costs a whole tail
            units.push_back({HostPiece{0, (const uint8_t*)left + p * step, (right && !il) ? (const uint8_t*)right + p * step : nullptr, m}});
            p += m;
            cur = cfg.growth * cur < cap ? cfg.growth * cur : cap;
        }
    }
    int64_t w = 0;
    uint8_t* d = out;
    const int rc = encode_host_pipelined(s->ctx, {s}, units, format, &d, &w);
    return rc < 0 ? rc : w;
}

// MANY streams with host buffers (lhip_encode_batch): groups of streams as units -- a group's copies hide behind the encode of the group before
static int encode_host_groups(lhip_stream* const* streams, size_t n, int format, const void* const* l, const void* const* r, const size_t* ns,
                              uint8_t* const* out, const size_t* cap, int64_t* written) {
    const Tables& T = streams[0]->ts->T;
    const size_t spf = (size_t)576 * T.mode_gr * T.rs_ratio;
    for (size_t i = 0; i < n; i++)
        if ((size_t)batch_bytes(*streams[i]->ts, streams[i]->slot_lag, call_frames(streams[i], ns[i])) > cap[i]) {
            for (size_t k = 0; k < n; k++) if (written) written[k] = LHIP_ERR_BUFFER_TOO_SMALL;
            set_err("output buffer too small"); return LHIP_ERR_BUFFER_TOO_SMALL;
        }
    // groups of about 2 x the first chunk of the one-stream schedule (16384 one-channel frames): large enough for the persistent kernel,
    // small enough that the first group's copy -- the part nothing overlaps -- stays short
    const size_t target = 2 * host_chunk_schedule().first * spf;
    std::vector<std::vector<HostPiece>> units(1);
    size_t acc = 0;
    for (size_t i = 0; i < n; i++) {
        if (acc >= target) { units.emplace_back(); acc = 0; }
        units.back().push_back(HostPiece{(int)i, l[i], r ? r[i] : nullptr, ns[i]});
        acc += ns[i];
    }
    std::vector<lhip_stream*> strs(streams, streams + n);
    std::vector<int64_t> w(n, 0);
    const int rc = encode_host_pipelined(streams[0]->ctx, strs, units, format, out, w.data());
    for (size_t i = 0; i < n; i++) if (written) written[i] = rc < 0 ? (int64_t)rc : w[i];
    return rc;
}

// Float32 input through a host pointer: the whole call is looked at before anything is consumed.  A sample that is not finite or lies beyond
// +-131072 refuses the call (the reference encodes NaN and infinities into garbage; here they never reach a kernel).  `count` elements.
static bool scan_f32(const void* p, size_t count, float limit, size_t* where) {
    const float* f = (const float*)p;
    for (size_t i = 0; i < count; i++) if (!((f[i] < 0 ? -f[i] : f[i]) <= limit)) { *where = i; return false; }
    return true;
}
// the host-pointer entries' check of one stream's input; on refusal lhip_last_error() names stream, channel, index and value
// (channels: INPUT channels; limit: the stream's Tables::pcm_limit -- 131072, or less where its gains exceed 1)
// the formats whose host calls are looked at first: the float types (an integer type cannot leave the contract)
static inline bool fmt_scanned(int format) { const int t = fmt_type(format); return t == LHIP_PCM_F32 || (fmt_ingest(t) && ingest_is_float(t)); }
// the WAV float types (k_ingest.h): the converted value decides, by the conversion the kernel makes
static bool scan_ingest(int type, const void* p, size_t count, float limit, size_t* where) {
    const size_t bps = fmt_bps(type);
    for (size_t i = 0; i < count; i++) { unsigned bad = 0; (void)ingest_value<false>(type, (const uint8_t*)p + i * bps, limit, &bad); if (bad) { *where = i; return false; } }
    return true;
}
static bool host_samples_ok(size_t stream_idx, int channels, float limit, int format, const void* left, const void* right, size_t n) {
    if (!fmt_scanned(format) || n == 0 || !left) return true;
    const bool il = (format & LHIP_PCM_INTERLEAVED) && channels == 2;
    if (fmt_type(format) != LHIP_PCM_F32) {
        const int type = fmt_type(format);
        size_t w = 0; int ch = 0; const void* bad = nullptr;
        if (!scan_ingest(type, left, il ? 2 * n : n, limit, &w)) { bad = left; if (il) ch = (int)(w & 1); }
        else if (!il && channels == 2 && right && right != left && !scan_ingest(type, right, n, limit, &w)) { bad = right; ch = 1; }
        if (!bad) return true;
        double v;
        if (type == LHIP_PCM_F32N) { float x; memcpy(&x, (const uint8_t*)bad + 4 * w, 4); v = x; } else memcpy(&v, (const uint8_t*)bad + 8 * w, 8);
        char txt[288];
        snprintf(txt, sizeof txt, "%s sample outside the contract (finite, |%s| <= %g): stream %zu, channel %d, index %zu, value %g; nothing was consumed",
                 type == LHIP_PCM_F32N ? "normalised Float32" : type == LHIP_PCM_F64N ? "normalised Float64" : "Float64", type == LHIP_PCM_F64 ? "x" : "32768 x", (double)limit, stream_idx, ch, il ? w / 2 : w, v);
        set_err(txt);
        return false;
    }
    size_t w = 0;
    int ch = 0;
    const void* bad = nullptr;
    if (!scan_f32(left, il ? 2 * n : n, limit, &w)) { bad = left; if (il) { ch = (int)(w & 1); } }
    else if (!il && channels == 2 && right && right != left && !scan_f32(right, n, limit, &w)) { bad = right; ch = 1; }
    if (!bad) return true;
    char txt[256];
    snprintf(txt, sizeof txt, "Float32 sample outside the contract (finite, |x| <= %g): stream %zu, channel %d, index %zu, value %g; nothing was consumed",
             (double)limit, stream_idx, ch, il ? w / 2 : w, (double)((const float*)bad)[w]);
    set_err(txt);
    return false;
}
