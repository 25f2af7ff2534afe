// C-ABI implementation of include/lamejs_hip.h: stream objects, HBM workspace management and
// the kernel pipeline for one batch of frames -- the one file that is compiled; the concerns live in the headers included below (layout of csrc/).  Compiled by hipcc for gfx950 (the product), and
// by g++ with -DLHIP_HOSTSIM for the test-only CPU simulation of the kernel logic (tests/hostsim).
//
// Pipeline per batch:  load carried state -> psyA (parallel over granule-channels)
// -> scan (per stream) -> psyB (parallel) -> polyphase -> MDCT -> quantize (parallel over frames,
// speculative bin-search seed) -> validate seed chain [-> repair flagged frames]* -> bit-pack -> save state.
#include "../../include/lamejs_hip.h"
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
#include "k_psy.h"
#include "k_fb.h"
#include "k_quant.h"
#if !defined(LHIP_HOSTSIM) || defined(LHIP_WAVESIM)
#include "k_quant_tail.h"      // how a launch of the persistent quantization kernel ends (the one-lane simulation has no workgroups: it runs kb_quant)
#endif
#include "k_quant_fast.h"      // the speculative pass of a fast table set (quality 7): the bin search alone
#include "k_quant_probe.h"     // test hook: the search's pure functions over caller-supplied records (lhip_debug_quant_probe)
#include "k_bits.h"
#include "k_bits_probe.h"      // test hook: the bit packer over caller-supplied frames (lhip_debug_bits_probe)
#include "k_crc.h"
#include "k_ingest.h"
#include "k_gain.h"

#include <string>
#include <vector>
#include <map>
#include <mutex>
#include <thread>
#include <atomic>
#include <memory>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <cmath>
#if defined(LHIP_HOSTSIM) && defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>      // lhip_debug_ingest poisons the bytes in front of its input (tests/tools/wavpcm_bounds.c)
#define LHIP_ASAN_POISON 1
#endif

using namespace lhip;

#include "lhip_rt.h"
#include "k_state.h"
#include "k_frame.h"
#ifndef LHIP_HOSTSIM
#include <dlfcn.h>             // lhip_debug_quant_probe finds its kernel's code object beside the library
#include "lhip_kernels.h"
#endif
#include "lhip_gain.h"
#include "lhip_infotag.h"
#include "lhip_tables.h"
#include "lhip_context.h"
#include "lhip_batch.h"
#include "lhip_hostcall.h"
#include "lhip_fracflush.h"

// ---- lhip_debug_math: the device's arithmetic, operation by operation ----
// op 10: records of 2 doubles [a, b] -> [div_by_f32(a, (float)b, RN(1 / (float)b)), a / (float)b]: calc_noise's division by xmin through the reciprocal
// against the division itself (must be bit-identical for finite a >= 0 and a positive Float32 divisor)
LHIP_DEV void math_op10(const double* in, double* out) {
    const double a = in[0], b = (double)(float)in[1], rb = recip_for_div(b);
    out[0] = rb != 0.0 ? div_by_f32(a, b, rb) : a / b;
    out[1] = a / b;
}

// op 8: records of 21 doubles [istep, xa0..4, xb0..4, adj_a0..4, adj_b0..4] (f32 values) -> [0, floor(x istep) x 10, floor(x istep + adj) x 10]
LHIP_DEV void math_op8(const double* in, double* out) {
    float xa[5], xb[5], ja[5], jb[5]; int ra[5], rb[5], va[5], vb[5];
    const float istep = (float)in[0];
    for (int k = 0; k < 5; k++) { xa[k] = (float)in[1 + k]; xb[k] = (float)in[6 + k]; ja[k] = (float)in[11 + k]; jb[k] = (float)in[16 + k]; }
    q_floor_prod(xa, xb, istep, ra, rb);
    q_floor_fma(xa, xb, istep, ja, jb, va, vb);
    out[0] = 0;
    for (int k = 0; k < 5; k++) { out[1 + k] = ra[k]; out[6 + k] = rb[k]; out[11 + k] = va[k]; out[16 + k] = vb[k]; }
}
#ifndef LHIP_HOSTSIM
__global__ void g_math(int op, const double* in, double* out, size_t n, PowBase pb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (op == 8) { if (21 * i + 21 <= n) math_op8(in + 21 * i, out + 21 * i); return; }
    if (op == 10) { if (2 * i + 2 <= n) math_op10(in + 2 * i, out + 2 * i); return; }
    if (i >= n) return;
    const double x = in[i];
    double r = 0;
    switch (op) {
        case 0: r = v8_log10(x); break;
        case 1: r = v8_pow_base(pb, x); break;
        case 2: r = d_sqrt(x); break;
        case 3: r = 1.0 / x; break;
        case 4: r = (double)(float)x; break;
        case 5: r = (double)js_toint32(x); break;
        case 6: r = x / 3.0 + x * 0.1; break;
        case 7: r = v8_log10_pos(x); break;
        case 11: r = (double)ma_index16(x) + 1000.0 * (double)js_toint32(v8_log10_pos(x) * 16.0); break;   // mask_add's table index: shortcut (-1: none) + 1000 * the logarithm's
        case 9: {   // calc_noise's shortcut: noise_class(x) + 1000 * class from the f64 logarithm + 1e6 * class from its Float32 copy
            const double l = v8_log10_pos(x > 1E-20 ? x : 1E-20);
            r = (double)noise_class(x) + 1000.0 * (double)noise_class_of_log(l) + 1e6 * (double)noise_class_of_log((double)(float)l);
        } break;
    }
    out[i] = r;
}
#endif

// { infoTag }: the placeholder of the tag frame goes out in front of the audio of the stream's first call
static size_t tag_pending_bytes(const lhip_stream* s) { return (s->tag && !s->tag->placed) ? (size_t)s->ts->tag.size : 0; }

// { infoTag }: the first call of such a stream (an encode call with samples, or the flush: ns == nullptr) returns the tag frame's placeholder in front of
// its audio -- LAME's contract.  The host writes it where the caller's buffer begins and the call proper sees the buffer behind it; the bytes count
// as written, and the stream as served, only when the call succeeded (a failed call consumes nothing).  inner(out, cap, written) -> code.
template <class Fn>
static int tagged_call(lhip_stream* const* streams, size_t n, const size_t* ns, uint8_t* const* out, const size_t* cap, int64_t* written, bool dev_io, Fn&& inner) {
    bool any = false;
    if (streams && out && cap)
        for (size_t i = 0; i < n && !any; i++) any = streams[i] && streams[i]->magic == 0x4c484950 && streams[i]->tag && !streams[i]->tag->placed && (!ns || ns[i] > 0);
    if (!any) return inner(out, cap, written);
    std::vector<uint8_t*> o(out, out + n); std::vector<size_t> c(cap, cap + n); std::vector<size_t> pre(n, 0); std::vector<int64_t> w(n, 0);
    for (size_t i = 0; i < n; i++) {
        lhip_stream* s = streams[i];
        if (!(s && s->magic == 0x4c484950 && s->tag && !s->tag->placed && (!ns || ns[i] > 0))) continue;
        for (size_t k = 0; k < i; k++) if (streams[k] == s) { s = nullptr; break; }      // (a handle twice in one batch: the call proper reports it)
        if (!s) continue;
        pre[i] = (size_t)s->ts->tag.size;
        if (!out[i] || cap[i] < pre[i]) { set_err("output buffer too small"); for (size_t k = 0; k < n; k++) if (written) written[k] = LHIP_ERR_BUFFER_TOO_SMALL; return LHIP_ERR_BUFFER_TOO_SMALL; }
        std::vector<uint8_t> ph(pre[i]);
        tag_placeholder(s->ts->T, s->ts->tag, ph.data());
        if (!dev_io) memcpy(out[i], ph.data(), pre[i]);
        else {
            Context* ctx = s->ctx;
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (!rt::set_device(ctx->device) || !rt::h2d(out[i], ph.data(), pre[i], ctx->stream)) return LHIP_ERR_INTERNAL;
        }
        o[i] += pre[i]; c[i] -= pre[i];
    }
    const int rc = inner(o.data(), c.data(), w.data());
    for (size_t i = 0; i < n; i++) {
        if (w[i] >= 0 && pre[i]) { w[i] += (int64_t)pre[i]; streams[i]->tag->placed = true; }
        if (written) written[i] = w[i];
    }
    return rc;
}

// ===========================================================================================
// C ABI
// ===========================================================================================
extern "C" {

int lhip_device_count(void) { return rt::device_count(); }

static std::atomic<uint64_t> g_dev_mask{0};
static std::atomic<unsigned> g_dev_rr{0};
int lhip_set_devices(uint64_t mask) {
    const int n = rt::device_count();
    if (n <= 0) { set_err("no HIP device available (this library has no CPU fallback)"); return LHIP_ERR_INTERNAL; }
    const uint64_t all = n >= 64 ? ~0ull : ((1ull << n) - 1);
    if (mask & ~all) { set_err("lhip_set_devices: mask names a device that does not exist"); return LHIP_ERR_INTERNAL; }
    g_dev_mask = mask; g_dev_rr = 0;
    return mask ? __builtin_popcountll(mask) : n;
}

int lhip_stream_device(const lhip_stream* s) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    return s->ctx->device;
}

int lhip_device_identity(int device, char* pci_bus_id, char* uuid_hex, size_t cap) {
    if (!pci_bus_id || !uuid_hex || cap < 2) { set_err("null argument"); return LHIP_ERR_INTERNAL; }
    pci_bus_id[0] = 0; uuid_hex[0] = 0;
#ifdef LHIP_HOSTSIM
    snprintf(pci_bus_id, cap, "hostsim:%d", device < 0 ? 0 : device); snprintf(uuid_hex, cap, "hostsim-%d", device < 0 ? 0 : device);
    return 0;
#else
    if (device < 0 && hipGetDevice(&device) != hipSuccess) { set_err("hipGetDevice failed"); return LHIP_ERR_INTERNAL; }
    const int pd = rt::phys(device);
    if (hipDeviceGetPCIBusId(pci_bus_id, (int)cap, pd) != hipSuccess) { set_err("hipDeviceGetPCIBusId failed"); return LHIP_ERR_INTERNAL; }
    hipUUID u;
    if (hipDeviceGetUuid(&u, pd) == hipSuccess) {
        size_t o = 0;
        for (int i = 0; i < 16 && o + 3 <= cap; i++) o += (size_t)snprintf(uuid_hex + o, cap - o, "%02x", (unsigned)(unsigned char)u.bytes[i]);
    }
    return 0;
#endif
}

const char* lhip_last_error(void) { return g_err.c_str(); }
const char* lhip_version(void) {
#ifdef LHIP_HOSTSIM
    return "lamejs_amd 0.1 (HOST SIMULATION - tests only)";
#else
    return "lamejs_amd 0.1 (HIP gfx950)";
#endif
}

int lhip_create(const lhip_config* cfg, const void* tables, size_t tables_bytes, lhip_stream** out) {
    if (!cfg || !tables || !out) { set_err("null argument"); return LHIP_ERR_INTERNAL; }
    *out = nullptr;
    if (rt::device_count() <= 0) { set_err("no HIP device available (this library has no CPU fallback)"); return LHIP_ERR_INTERNAL; }
    int dev = cfg->device;
    const uint64_t mask = g_dev_mask;
    if (mask) {
        if (dev >= 0 && !((mask >> dev) & 1)) { set_err("device excluded by lhip_set_devices"); return LHIP_ERR_INTERNAL; }
        if (dev < 0) {                       // deal streams round-robin over the allowed devices
            unsigned k = g_dev_rr++ % (unsigned)__builtin_popcountll(mask);
            for (dev = 0; dev < 64; dev++) if ((mask >> dev) & 1) { if (k == 0) break; k--; }
        }
    }
#ifndef LHIP_HOSTSIM
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) { set_err("hipGetDevice failed"); return LHIP_ERR_INTERNAL; } }
#else
    if (dev < 0) dev = 0;
#endif
    if (dev >= rt::device_count()) { set_err("no such HIP device"); return LHIP_ERR_INTERNAL; }
    Context* ctx = get_context(dev);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rt::set_device(dev)) return LHIP_ERR_INTERNAL;
    std::string key((const char*)tables, tables_bytes);
    std::shared_ptr<TableSet> ts;
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        ts = it->second;
        // the same checks build_tables makes of the blob against the requested configuration
        if (ts->T.channels_in != (cfg->channels == 1 ? 1 : 2) || ts->T.in_samplerate != cfg->samplerate) { set_err("tables blob does not match the requested configuration"); return LHIP_ERR_INTERNAL; }
    } else {
        ts = std::make_shared<TableSet>();
        ts->device = dev;
        if (!build_tables(*ts, tables, tables_bytes, *cfg, ctx->stream)) return ts->bad_option ? -3 : LHIP_ERR_INTERNAL;      // (-3: an option's value outside the contract, with a message)
        ctx->tables[key] = ts;
    }
    std::unique_ptr<lhip_stream> s(new lhip_stream());
    s->ctx = ctx; s->ts = ts;
    if (ts->tag.on) s->tag.reset(new TagTotals());
    if (ts->gain_on) { s->gain.reset(gain_create(ts->T.out_samplerate, ts->T.channels_out, ctx->stream)); if (!s->gain) return LHIP_ERR_INTERNAL; }
    s->slot_lag = ts->T.frac_SpF;
    // initial carried state (PsyModel.js:2566-2596 psymodel_init, Lame.js:168-171 lame_init_old)
    std::unique_ptr<StreamState> h(new StreamState());
    memset(h.get(), 0, sizeof(StreamState));
    for (int ch = 0; ch < 4; ch++) {                      // psy state exists for L, R, mid, side (PsyModel.js:2566-2596)
        for (int i = 0; i < E_STRIDE; i++) h->E[ch][i] = 1e20f;
        for (int i = 0; i < EBS_STRIDE; i++) h->ecb_s[ch][i] = 1.0f;
        for (int i = 0; i < 9; i++) h->peaks[ch][i] = 10.f;
        for (int i = 0; i < EBL_STRIDE; i++) h->nb1[ch][i] = h->nb2[ch][i] = 1e20f;
    }
    for (int i = 0; i < 19; i++) h->rv.pefirbuf[i] = (float)(700 * ts->T.mode_gr * ts->T.channels_out);      // Lame.js:1120
    for (int ch = 0; ch < 2; ch++) {
        h->tent[ch] = NORM_TYPE;
        h->last_bt[ch] = -1;
        h->seed[ch][0] = 180; h->seed[ch][1] = 4;
    }
    h->ath_adjust = 0.01; h->ath_limit = 1.0;
    s->d_state = (StreamState*)rt::dmalloc(sizeof(StreamState));
    if (!s->d_state) { set_err("hipMalloc(stream state) failed"); return LHIP_ERR_INTERNAL; }
    if (!rt::h2d(s->d_state, h.get(), sizeof(StreamState), ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
    ctx->live_streams++;
    *out = s.release();
    return 0;
}

void lhip_destroy(lhip_stream* s) {
    if (!s || s->magic != 0x4c484950) return;
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    rt::set_device(ctx->device);
    std::shared_ptr<TableSet> ts = s->ts;
    delete s;
    if (--ctx->live_streams == 0) { (void)rt::sync(ctx->stream); ctx->ws.pin_in.release(); ctx->ws.pin_out.release(); }      // (grow-only while streams live; a later stream allocates them again)
    // the cache entry goes with the last stream that uses it (one reference is the map's, one is `ts` here)
    if (ts.use_count() == 2)
        for (auto it = ctx->tables.begin(); it != ctx->tables.end(); ++it) if (it->second == ts) { ctx->tables.erase(it); break; }
}

size_t lhip_max_output_bytes(const lhip_stream* s, size_t nsamples) {
    if (!s || s->magic != 0x4c484950) return 0;
    const size_t frame = 576 * (size_t)s->ts->T.mode_gr;
    return (nsamples / frame + 3 + (FRAME / frame)) * (size_t)(s->ts->base_frame_bytes + 1) + (s->ts->T.disable_reservoir ? 0 : 4096) + tag_pending_bytes(s);      // reservoir: slack for the per-launch bound
}

int64_t lhip_encode_output_bytes(const lhip_stream* s, size_t nsamples) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!s->ts->T.disable_reservoir) return (int64_t)lhip_max_output_bytes(s, nsamples);      // data-dependent: only a bound exists
    const int F = call_frames(s, nsamples);
    if (F < 0) { set_err(s->rs_flushed ? std::string("fractionalResample: the stream has been flushed") : frac_refusal(s->ts->T, nsamples)); return LHIP_ERR_INTERNAL; }      // the call would be refused
    return batch_bytes(*s->ts, s->slot_lag, F) + (nsamples > 0 ? (int64_t)tag_pending_bytes(s) : 0);
}

int lhip_output_bytes_is_exact(const lhip_stream* s) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    return s->ts->T.disable_reservoir ? 1 : 0;
}

static int encode_many(lhip_stream* const* streams, size_t n, int format, const void* const* l, const void* const* r,
                       const size_t* ns, uint8_t* const* out, const size_t* cap, int64_t* written, bool dev_io, bool sync, bool flush_stream = false) {
    if (n == 0) return 0;
    std::vector<Job> jobs(n);
    for (size_t i = 0; i < n; i++) {
        if (!streams[i] || streams[i]->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
        if (streams[i]->ctx != streams[0]->ctx) { set_err("batch: streams on different devices"); return LHIP_ERR_INTERNAL; }
        jobs[i] = Job{streams[i], l[i], r ? r[i] : nullptr, ns[i], out[i], cap[i], 0, 0, 0, 0};
        jobs[i].set_format(format);
        jobs[i].count_rejected = dev_io && (jobs[i].f32 || (fmt_ingest(jobs[i].type) && ingest_is_float(jobs[i].type)));
        // WAV sample types by device pointer: the kernel reads 4- and 8-byte elements as such (U8 and S24 lie anywhere)
        if (dev_io && fmt_ingest(jobs[i].type) && fmt_bps(jobs[i].type) >= 4 && ns[i] > 0) {
            const uintptr_t m = (uintptr_t)fmt_bps(jobs[i].type) - 1;
            const bool two = streams[i]->ts->T.channels_in == 2 && !jobs[i].inter && jobs[i].r;
            if (((uintptr_t)jobs[i].l & m) || (two && ((uintptr_t)jobs[i].r & m))) {
                char txt[160];
                snprintf(txt, sizeof txt, "stream %zu: device pointer of a %zu-byte sample type is not a multiple of %zu; nothing was consumed", i, m + 1, m + 1);
                set_err(txt);
                for (size_t k = 0; k < n; k++) if (written) written[k] = LHIP_ERR_INTERNAL;
                return LHIP_ERR_INTERNAL;
            }
        }
    }
    // Bit reservoir (extension): the frames of a stream are a serial chain, walked by one workgroup per stream inside the launch
    // (g_resv_stream); a stream that ends with this call (flush) has its bitstream padded by the same launch -- decided per stream
    // (an already flushed stream in a flush batch has nothing to encode and is not flushed again).  The byte counts are only known
    // on the device, so these calls always synchronise.
    bool resv = false;
    for (size_t i = 0; i < n; i++) if (!streams[i]->ts->T.disable_reservoir) { resv = true; jobs[i].flush = flush_stream && ns[i] > 0; }
    // Non-integer-ratio streams (extension { fractionalResample }): a call the reference would not consume whole is refused before anything is
    // consumed on ANY stream of the batch.  Their batches may mix configurations (a caller with many low-bitrate streams has one frame per
    // stream and call at most): the streams are then launched configuration by configuration, in order of first appearance.
    // So is any other batch whose streams do not share one table blob (protected beside unprotected streams, say): a launch works with one table set.
    // Such a call synchronises, and a refusal in a later group leaves the earlier groups encoded -- written[] says which.
    bool any_frac = false, mixed = false;
    for (size_t i = 0; i < n; i++) { any_frac |= streams[i]->ts->T.rs_frac != 0; mixed |= streams[i]->ts.get() != streams[0]->ts.get(); }
    if (any_frac) {
        for (size_t i = 0; i < n; i++)
            if (streams[i]->ts->T.rs_frac && ns[i] > 0 && call_frames(streams[i], ns[i]) < 0) {
                set_err(streams[i]->rs_flushed ? std::string("fractionalResample: the stream has been flushed") : frac_refusal(streams[i]->ts->T, ns[i]));
                for (size_t k = 0; k < n; k++) if (written) written[k] = LHIP_ERR_INTERNAL;
                return LHIP_ERR_INTERNAL;
            }
    }
    {
        if (mixed) {
            std::vector<char> done(n, 0);
            for (size_t i = 0; i < n; i++) {
                if (done[i]) continue;
                std::vector<Job> group; std::vector<size_t> idx;
                for (size_t k = i; k < n; k++) if (!done[k] && streams[k]->ts.get() == streams[i]->ts.get()) { group.push_back(jobs[k]); idx.push_back(k); done[k] = 1; }
                const bool ok = run_batch(streams[0]->ctx, group, dev_io, true);
                for (size_t g = 0; g < idx.size(); g++) if (written) written[idx[g]] = ok ? group[g].written : (group[g].written < 0 ? group[g].written : LHIP_ERR_INTERNAL);
                if (!ok) { for (auto& j : group) if (j.written < 0) return (int)j.written; return LHIP_ERR_INTERNAL; }
            }
            return 0;
        }
    }
    const bool ok = run_batch(streams[0]->ctx, jobs, dev_io, sync || resv);
    for (size_t i = 0; i < n; i++) if (written) written[i] = ok ? jobs[i].written : (jobs[i].written < 0 ? jobs[i].written : LHIP_ERR_INTERNAL);
    if (!ok) { for (auto& j : jobs) if (j.written < 0) return (int)j.written; return LHIP_ERR_INTERNAL; }
    return 0;
}

int64_t lhip_encode_pcm(lhip_stream* s, int format, const void* left, const void* right, size_t nsamples, uint8_t* out, size_t out_cap) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!fmt_ok(format)) { set_err("unknown sample format"); return LHIP_ERR_INTERNAL; }
    if (nsamples == 0) return 0;
    if (!left) { set_err("null input"); return LHIP_ERR_INTERNAL; }
    if (!host_samples_ok(0, s->ts->T.channels_in, s->ts->T.pcm_limit, format, left, right, nsamples)) return LHIP_ERR_INTERNAL;
    int64_t w = 0;
    const int rc = tagged_call(&s, 1, &nsamples, &out, &out_cap, &w, false, [&](uint8_t* const* o, const size_t* c, int64_t* wr) -> int {
        static const bool no_chunk = []() { const char* e = getenv("LAMEJS_HIP_NO_HOST_CHUNKS"); return e && e[0] == '1'; }();
        const Tables& T = s->ts->T;
        if (!no_chunk && T.disable_reservoir && !T.rs_frac && nsamples > (size_t)2 * host_chunk_schedule().first * 576 * T.mode_gr * T.rs_ratio) {
            wr[0] = encode_host_chunked(s, format, left, right, nsamples, o[0], c[0]);
            return wr[0] < 0 ? (int)wr[0] : 0;
        }
        return encode_many(&s, 1, format, &left, &right, &nsamples, o, c, wr, false, true);
    });
    return rc < 0 ? rc : w;
}
int64_t lhip_encode(lhip_stream* s, const int16_t* left, const int16_t* right, size_t nsamples, uint8_t* out, size_t out_cap) {
    return lhip_encode_pcm(s, LHIP_PCM_S16, left, right, nsamples, out, out_cap);
}

int64_t lhip_flush(lhip_stream* s, uint8_t* out, size_t out_cap) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (s->ts->T.rs_frac) return frac_flush(s, out, out_cap);
    const size_t z = flush_zeros(s);
    if (z == 0) { s->mf_samples_to_encode = 0; return 0; }
    std::vector<int16_t> zeros(z, 0);
    const void* l = zeros.data();
    const void* r = zeros.data();
    int64_t w = 0;
    const double end_padding = flush_end_padding(s);
    const int rc = tagged_call(&s, 1, nullptr, &out, &out_cap, &w, false, [&](uint8_t* const* o, const size_t* c, int64_t* wr) -> int {
        return encode_many(&s, 1, LHIP_PCM_S16, &l, &r, &z, o, c, wr, false, true, true); });
    if (rc < 0) return rc;                 // nothing was consumed (e.g. -1: the call can be repeated with a larger buffer)
    s->mf_samples_to_encode = 0;
    if (s->tag) { s->tag->padding = end_padding; s->tag->flushed = true; }
    return w;
}

static int encode_batch_pcm_inner(lhip_stream* const* streams, size_t nstreams, int format, const void* const* left, const void* const* right,
                                  const size_t* nsamples, uint8_t* const* out, const size_t* out_cap, int64_t* written);
int lhip_encode_batch_pcm(lhip_stream* const* streams, size_t nstreams, int format, const void* const* left, const void* const* right,
                          const size_t* nsamples, uint8_t* const* out, const size_t* out_cap, int64_t* written) {
    return tagged_call(streams, nstreams, nsamples, out, out_cap, written, false, [&](uint8_t* const* o, const size_t* c, int64_t* wr) -> int {
        return encode_batch_pcm_inner(streams, nstreams, format, left, right, nsamples, o, c, wr); });
}
static int encode_batch_pcm_inner(lhip_stream* const* streams, size_t nstreams, int format, const void* const* left, const void* const* right,
                                  const size_t* nsamples, uint8_t* const* out, const size_t* out_cap, int64_t* written) {
    if (!fmt_ok(format)) { set_err("unknown sample format"); return LHIP_ERR_INTERNAL; }
    if (fmt_scanned(format) && streams && left && nsamples)       // every stream's samples are looked at before any stream consumes anything
        for (size_t i = 0; i < nstreams; i++)
            if (streams[i] && streams[i]->magic == 0x4c484950 && !host_samples_ok(i, streams[i]->ts->T.channels_in, streams[i]->ts->T.pcm_limit, format, left[i], right ? right[i] : nullptr, nsamples[i])) {
                for (size_t k = 0; k < nstreams; k++) if (written) written[k] = LHIP_ERR_INTERNAL;
                return LHIP_ERR_INTERNAL;
            }
    // many streams with a lot of input: groups of streams go through the overlapped host path (copies behind the encode of the group before)
    if (nstreams > 1 && streams && left && nsamples && out && out_cap) {
        static const bool no_chunk = []() { const char* e = getenv("LAMEJS_HIP_NO_HOST_CHUNKS"); return e && e[0] == '1'; }();
        bool ok = !no_chunk;
        size_t total = 0;
        for (size_t i = 0; i < nstreams && ok; i++) {
            ok = streams[i] && streams[i]->magic == 0x4c484950 && streams[i]->ctx == streams[0]->ctx && streams[i]->ts.get() == streams[0]->ts.get() && left[i] && nsamples[i] > 0;
            if (ok) for (size_t k = 0; k < i; k++) if (streams[k] == streams[i]) { ok = false; break; }      // (a handle twice in one batch: the plain path reports it)
            total += nsamples[i];
        }
        if (ok && streams[0]->ts->T.disable_reservoir && !streams[0]->ts->T.rs_frac) {
            const Tables& T = streams[0]->ts->T;
            if (total > (size_t)4 * host_chunk_schedule().first * 576 * T.mode_gr * T.rs_ratio) return encode_host_groups(streams, nstreams, format, left, right, nsamples, out, out_cap, written);
        }
    }
    return encode_many(streams, nstreams, format, left, right, nsamples, out, out_cap, written, false, true);
}
int lhip_encode_batch(lhip_stream* const* streams, size_t nstreams, const int16_t* const* left, const int16_t* const* right,
                      const size_t* nsamples, uint8_t* const* out, const size_t* out_cap, int64_t* written) {
    return lhip_encode_batch_pcm(streams, nstreams, LHIP_PCM_S16, (const void* const*)left, (const void* const*)right, nsamples, out, out_cap, written);
}

int lhip_flush_batch(lhip_stream* const* streams, size_t nstreams, uint8_t* const* out, const size_t* out_cap, int64_t* written) {
    std::vector<std::vector<int16_t>> zs(nstreams);
    std::vector<const void*> l(nstreams);
    std::vector<size_t> ns(nstreams);
    bool any_frac = false;
    for (size_t i = 0; i < nstreams; i++) any_frac |= streams[i] && streams[i]->magic == 0x4c484950 && streams[i]->ts->T.rs_frac;
    if (any_frac) {                          // non-integer-ratio streams end with a few frames each, partly made on the host (frac_flush): one after the other
        int rc = 0;
        for (size_t i = 0; i < nstreams; i++) {
            const int64_t w = lhip_flush(streams[i], out[i], out_cap[i]);
            if (written) written[i] = w;
            if (w < 0 && rc == 0) rc = (int)w;
        }
        return rc;
    }
    for (size_t i = 0; i < nstreams; i++) {
        if (!streams[i] || streams[i]->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
        ns[i] = flush_zeros(streams[i]);
        zs[i].assign(ns[i] ? ns[i] : 1, 0);
        l[i] = zs[i].data();
    }
    std::vector<double> end_padding(nstreams);
    for (size_t i = 0; i < nstreams; i++) end_padding[i] = flush_end_padding(streams[i]);
    const int rc = tagged_call(streams, nstreams, ns.data(), out, out_cap, written, false, [&](uint8_t* const* o, const size_t* c, int64_t* wr) -> int {
        return encode_many(streams, nstreams, LHIP_PCM_S16, l.data(), l.data(), ns.data(), o, c, wr, false, true, true); });
    if (rc >= 0) for (size_t i = 0; i < nstreams; i++) {
        streams[i]->mf_samples_to_encode = 0;
        if (streams[i]->tag && ns[i] > 0) { streams[i]->tag->padding = end_padding[i]; streams[i]->tag->flushed = true; }
    }
    return rc;
}

int lhip_encode_batch_device(lhip_stream* const* streams, size_t nstreams, const int16_t* const* d_left, const int16_t* const* d_right,
                             const size_t* nsamples, uint8_t* const* d_out, const size_t* out_cap, int64_t* written, int sync) {
    return lhip_encode_batch_device_pcm(streams, nstreams, LHIP_PCM_S16, (const void* const*)d_left, (const void* const*)d_right, nsamples, d_out, out_cap, written, sync);
}
int lhip_encode_batch_device_pcm(lhip_stream* const* streams, size_t nstreams, int format, const void* const* d_left, const void* const* d_right,
                                 const size_t* nsamples, uint8_t* const* d_out, const size_t* out_cap, int64_t* written, int sync) {
    if (!fmt_ok(format)) { set_err("unknown sample format"); return LHIP_ERR_INTERNAL; }
    return tagged_call(streams, nstreams, nsamples, d_out, out_cap, written, true, [&](uint8_t* const* o, const size_t* c, int64_t* wr) -> int {
        return encode_many(streams, nstreams, format, d_left, d_right, nsamples, o, c, wr, true, sync != 0); });
}
int64_t lhip_last_batch_rejected_samples(void) {
    if (g_rej_pending) {                       // the count is on the device: wait for the batch and fetch it
        Context* ctx = g_rej_pending;
        g_rej_pending = nullptr;
        std::lock_guard<std::mutex> lk(ctx->mu);
        unsigned long long v = 0;
        if (!rt::set_device(ctx->device) || !rt::d2h(&v, ctx->ws.rejected.p, sizeof v, ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
        g_rejected = (int64_t)v;
    }
    return g_rejected;
}

// ---- frame-range sharding of ONE stream (second mode): speculate the state at a cut, verify it, transplant on a miss ----
struct StateHdr { uint32_t magic, bytes; int32_t mf_size, mf_samples_to_encode, slot_lag, config; int64_t frame_num, rs_n_in; };
// what must agree between the stream a state blob came from and the stream it is put into
static int32_t state_config_tag(const Tables& T) {
    // FNV-1a over everything that selects a different table set or state layout (MPEG-2 and MPEG-2.5 share version and
    // samplerate_index, so the rates themselves are part of it)
    const int32_t f[] = {T.channels_out, T.mode, T.disable_reservoir != 0, T.samplerate_index, T.version, T.bitrate_index, T.rs_ratio,
                         T.out_samplerate, T.in_samplerate, T.brate, T.mode_gr, T.psy_channels};
    uint32_t h = 2166136261u;
    for (int32_t v : f) for (int b = 0; b < 4; b++) { h ^= (uint32_t)(v >> (8 * b)) & 0xffu; h *= 16777619u; }
    return (int32_t)h;
}
size_t lhip_state_bytes(const lhip_stream* s) {
    if (!s || s->magic != 0x4c484950) return 0;
    return sizeof(StateHdr) + sizeof(StreamState);
}
int lhip_state_get(lhip_stream* s, void* buf, size_t cap) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (s->ts->T.rs_frac) { set_err("lhip_state_get: not for fractionalResample streams (call-sequence streams: the resampler's clock is not part of the state record)"); return LHIP_ERR_INTERNAL; }
    if (!buf || cap < lhip_state_bytes(s)) { set_err("state buffer too small"); return LHIP_ERR_BUFFER_TOO_SMALL; }
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rt::set_device(ctx->device)) return LHIP_ERR_INTERNAL;
    StateHdr h; memset(&h, 0, sizeof h);
    h.magic = 0x5453484cu; h.bytes = (uint32_t)lhip_state_bytes(s);
    h.mf_size = s->mf_size; h.mf_samples_to_encode = s->mf_samples_to_encode; h.slot_lag = s->slot_lag; h.frame_num = s->frame_num; h.rs_n_in = s->rs_n_in;
    h.config = state_config_tag(s->ts->T);
    memcpy(buf, &h, sizeof h);
    if (!rt::set_device(ctx->device) || !rt::d2h((uint8_t*)buf + sizeof h, s->d_state, sizeof(StreamState), ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
    // Canonical form: fields no later launch can read are zeroed, so that "equal blobs = equal futures" also holds the other way round
    // for streams that reached the same point through different call sizes (kb_save never clears the samples beyond mf_size, the
    // resampler tail and the reservoir record are dead without resampler / reservoir).
    {
        const Tables& T = s->ts->T;
        StreamState* S = (StreamState*)((uint8_t*)buf + sizeof h);
        for (int ch = 0; ch < 2; ch++) {
            const int live = ch < T.channels_out ? s->mf_size : 0;
            for (int i = live; i < MF_NEEDED; i++) S->pcm_tail[ch][i] = 0.f;
        }
        if (T.rs_ratio == 1) memset(S->rs_old, 0, sizeof S->rs_old);
        if (T.disable_reservoir) { memset(S->nb1, 0, sizeof S->nb1); memset(S->nb2, 0, sizeof S->nb2); memset(&S->rv, 0, sizeof S->rv); }
    }
    return 0;
}
int lhip_state_set(lhip_stream* s, const void* buf, size_t n) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    StateHdr h;
    if (s->ts->T.rs_frac) { set_err("lhip_state_set: not for fractionalResample streams"); return LHIP_ERR_INTERNAL; }
    if (!buf || n < sizeof h) { set_err("state blob too small"); return LHIP_ERR_INTERNAL; }
    memcpy(&h, buf, sizeof h);
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (h.magic != 0x5453484cu || h.bytes != lhip_state_bytes(s) || n < h.bytes || h.config != state_config_tag(s->ts->T)) { set_err("state blob does not belong to this build / configuration"); return LHIP_ERR_INTERNAL; }
    if (!rt::set_device(ctx->device)) return LHIP_ERR_INTERNAL;
    if (!rt::set_device(ctx->device) || !rt::h2d(s->d_state, (const uint8_t*)buf + sizeof h, sizeof(StreamState), ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
    s->mf_size = h.mf_size; s->mf_samples_to_encode = h.mf_samples_to_encode; s->slot_lag = h.slot_lag; s->frame_num = h.frame_num; s->rs_n_in = h.rs_n_in;
    if (s->tag) s->tag->moved = true;          // (state blobs do not carry the tag's totals)
    if (s->gain) s->gain->moved = true;        // (... nor the gain analysis' history and histogram)
    return 0;
}
size_t lhip_seek_tail_samples(const lhip_stream* s) {
    if (!s || s->magic != 0x4c484950) return 0;
    return (size_t)(MF_INIT + 576 * s->ts->T.mode_gr);
}
// Put a FRESH stream where a stream that has consumed `sample_pos` input samples stands, as far as that is known without encoding:
// the buffered samples (the lhip_seek_tail_samples() samples in front of sample_pos), the frame counter and the padding
// accumulator.  Everything the encoder derives from earlier audio (masking history, filterbank overlap, attack / block-type
// chains, ATH adjustment, bin-search seeds) starts from its initial value and converges while a few warm-up frames are encoded.
int lhip_seek(lhip_stream* s, int64_t sample_pos, const int16_t* tail_left, const int16_t* tail_right) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    const Tables& T = s->ts->T;
    const int frame = 576 * T.mode_gr, ntail = MF_INIT + frame;
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (T.rs_ratio != 1 || !T.disable_reservoir) { set_err("lhip_seek: not for resampling or bit-reservoir streams"); return LHIP_ERR_INTERNAL; }
    if (s->frame_num != 0 || s->mf_size != MF_INIT) { set_err("lhip_seek: the stream has been used"); return LHIP_ERR_INTERNAL; }
    if (sample_pos < 2 * frame || sample_pos % frame != 0 || !tail_left) { set_err("lhip_seek: position must be a whole number (>= 2) of frames"); return LHIP_ERR_INTERNAL; }
    if (T.channels_in == 2 && !tail_right) { set_err("lhip_seek: a two-channel stream needs both tails"); return LHIP_ERR_INTERNAL; }
    // the tails as the kernels would have left them: behind gains and mix (the host's copy of pcm_new_at / pcm_mix, lhip_layout.h)
    const bool down = T.in_mix == 2;
    std::vector<float> t((size_t)2 * MF_NEEDED, 0.f);
    for (int ch = 0; ch < T.channels_out; ch++) {
        const int16_t* src = (ch == 1 && tail_right) ? tail_right : tail_left;
        const bool do_g2 = ch ? T.do_scale_right : T.do_scale_left;
        const double g2 = ch ? T.scale_right : T.scale_left;
        for (int i = 0; i < ntail; i++) {
            float v = (float)src[i];
            if (T.do_scale) v = (float)((double)v * T.scale);
            if (do_g2) v = (float)((double)v * g2);
            if (down) {
                float b = (float)tail_right[i];
                if (T.do_scale_right) b = (float)((double)b * T.scale_right);
                v = (float)(0.5 * ((double)v + (double)b));
            }
            t[(size_t)ch * MF_NEEDED + i] = v;
        }
    }
    if (!rt::set_device(ctx->device) || !rt::h2d((uint8_t*)s->d_state + offsetof(StreamState, pcm_tail), t.data(), sizeof(float) * 2 * MF_NEEDED, ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
    const int64_t k = sample_pos / frame;                     // the stream has emitted k - 1 frames
    s->frame_num = k - 1;
    if (s->tag) s->tag->moved = true;
    if (s->gain) s->gain->moved = true;
    s->rs_n_in = sample_pos;
    s->mf_size = ntail;
    s->mf_samples_to_encode = 576 + 1152 + frame;
    if (T.frac_SpF != 0) {
        int64_t m = ((int64_t)T.frac_SpF - (k - 1) * (int64_t)T.frac_SpF) % T.out_samplerate;     // slot_lag starts at frac_SpF, one decrement per frame
        if (m < 0) m += T.out_samplerate;
        s->slot_lag = (int)m;
    }
    return 0;
}

// Test hooks (extension { fractionalResample }): the host arithmetic of a non-integer-ratio stream alone, nothing is encoded or consumed.
int64_t lhip_frac_call_limit(const lhip_stream* s) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    return s->ts->T.rs_frac ? frac_call_limit(s->ts->T) : 0;
}
int lhip_debug_frac_call(const lhip_stream* s, size_t nsamples, int32_t* k, int32_t* frames) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    const Tables& T = s->ts->T;
    if (!T.rs_frac) { set_err("not a fractionalResample stream"); return LHIP_ERR_INTERNAL; }
    const FracPass fp = frac_pass(T, s->rs_itime, (double)nsamples);
    if (k) *k = fp.k;
    const int F = call_frames(s, nsamples);
    if (frames) *frames = F;
    if (F < 0) { set_err(frac_refusal(T, nsamples)); return LHIP_ERR_INTERNAL; }
    return 0;
}
int lhip_debug_frac_flush(const lhip_stream* s, int32_t* bytes, int32_t* clean, int cap) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!s->ts->T.rs_frac) { set_err("not a fractionalResample stream"); return LHIP_ERR_INTERNAL; }
    std::vector<FracStep> steps;
    if (!frac_flush_plan(s, steps)) return LHIP_ERR_INTERNAL;
    int n = 0;
    for (const FracStep& st : steps) if (st.frame) { if (n < cap) { if (bytes) bytes[n] = st.bytes; if (clean) clean[n] = st.clean ? 1 : 0; } n++; }
    return n;
}

// Test hook (aliased contexts, LHIP_ALIAS_DEVICES): gives back what context `device` holds beyond its streams' lifetime -- the HIP stream the library created
// for it, the side stream and events of the ATH scan -- while the runtime is up.  Only with no live stream on the context.
int lhip_debug_release_context(int device) {
#ifndef LHIP_HOSTSIM
    Context* ctx = get_context(device);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->live_streams != 0) { set_err("lhip_debug_release_context: the context still has streams"); return LHIP_ERR_INTERNAL; }
    if (!rt::set_device(ctx->device)) return LHIP_ERR_INTERNAL;
    (void)hipStreamSynchronize((hipStream_t)ctx->stream);
    WorkSet& ws = ctx->ws;
    if (ws.aux_stream) { (void)hipStreamSynchronize((hipStream_t)ws.aux_stream); (void)hipStreamDestroy((hipStream_t)ws.aux_stream); (void)hipEventDestroy((hipEvent_t)ws.ev_fork); (void)hipEventDestroy((hipEvent_t)ws.ev_join); ws.aux_stream = ws.ev_fork = ws.ev_join = nullptr; }
    if (ctx->own_stream) { (void)hipStreamDestroy((hipStream_t)ctx->stream); ctx->stream = nullptr; ctx->own_stream = false; }
#else
    (void)device;
#endif
    return 0;
}

int lhip_set_hip_stream(int device, void* hip_stream) {
#ifndef LHIP_HOSTSIM
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return LHIP_ERR_INTERNAL; }
#else
    if (device < 0) device = 0;
#endif
    Context* ctx = get_context(device);
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->stream = hip_stream;
    return 0;
}

void lhip_last_batch_stats(int64_t* frames, int64_t* repaired_frames, int64_t* repair_iterations) {
#ifndef LHIP_HOSTSIM
    if (g_stat_pending) {                      // asynchronous batch: wait for it and fetch the device-side counters
        Context* ctx = g_stat_pending;
        g_stat_pending = nullptr;
        std::lock_guard<std::mutex> lk(ctx->mu);
        int32_t fx[3] = {0, 0, 0};
        WorkSet& ws = ctx->ws;
        void* st = ctx->stream;
        if (rt::set_device(ctx->device) && rt::d2h(fx, (const int32_t*)ws.nflagged.p + FX_STATS, sizeof fx, st) && rt::sync(st)) {
            g_stat_repaired = fx[0]; g_stat_iters = fx[1];
            if (fx[2]) set_err("seed-chain repair did not converge");
        }
    }
#endif
    if (frames) *frames = g_stat_frames;
    if (repaired_frames) *repaired_frames = g_stat_repaired;
    if (repair_iterations) *repair_iterations = g_stat_iters;
}

int lhip_debug_last_paths(uint32_t* mask) {
    if (!mask) { set_err("lhip_debug_last_paths: null argument"); return LHIP_ERR_INTERNAL; }
    *mask = g_last_paths;
    return 0;
}

int64_t lhip_debug_read(int what, void* dst, size_t cap) {
    if (what == 11) {                                   // the speculative quantization launch of this thread's last batch (QuantLaunch, lhip_rt.h): eight int32
        if (!dst) { set_err("lhip_debug_read: null argument"); return LHIP_ERR_INTERNAL; }
        const size_t n = cap < sizeof g_last_quant ? cap : sizeof g_last_quant; memcpy(dst, &g_last_quant, n); return (int64_t)n;
    }
#ifdef LHIP_HOSTSIM
    if (what == 10) {                                   // evaluations so far with the short / the full round count (RoundStats, k_quant_prof.h)
        const int64_t v[2] = {(int64_t)__atomic_load_n(&round_stats().head, __ATOMIC_RELAXED), (int64_t)__atomic_load_n(&round_stats().full, __ATOMIC_RELAXED)};
        const size_t n = cap < sizeof v ? cap : sizeof v; memcpy(dst, v, n); return (int64_t)n;
    }
    if (what == 12) {                                   // calc_noise calls so far with 7 / with 9 / with 3 lines per lane (NoiseLineStats, k_quant_prof.h; the 64-lane simulation counts)
        const int64_t v[3] = {(int64_t)__atomic_load_n(&noise_line_stats().n7, __ATOMIC_RELAXED), (int64_t)__atomic_load_n(&noise_line_stats().n9, __ATOMIC_RELAXED), (int64_t)__atomic_load_n(&noise_line_stats().n3, __ATOMIC_RELAXED)};
        const size_t n = cap < sizeof v ? cap : sizeof v; memcpy(dst, v, n); return (int64_t)n;
    }
#endif
#ifdef LHIP_PHASE_PROF
    if (what == 9) { const size_t n = cap < sizeof g_call_prof ? cap : sizeof g_call_prof; memcpy(dst, g_call_prof, n); return (int64_t)n; }
#endif
    Context* ctx = nullptr;
    // (the most recent batch of the process, whichever context ran it: walking the contexts for one that has run a batch found a released aliased context's stale workspace)
    { std::lock_guard<std::mutex> lk(g_ctx_mu); ctx = g_last_batch_ctx; }
    if (!ctx) { set_err("no batch has run"); return LHIP_ERR_INTERNAL; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    rt::set_device(ctx->device);
    const WorkSet& ws = ctx->ws;
    const Workspace& W = ws.lastW;
    const size_t GC = (size_t)W.ngslots * ws.lastC;
    const void* src = nullptr; size_t n = 0;
    switch (what) {
        case 0: src = W.xr; n = GC * 576 * 4; break;
        case 1: src = W.blocktype; n = GC * 4; break;
        case 2: src = W.E; n = (size_t)W.ngslots * ws.lastCp * E_STRIDE * 4; break;
        case 3: src = W.ath_adjust; n = (size_t)W.nfslots * 8; break;
        case 4: src = W.side; n = (size_t)W.nframes_total * 2 * ws.lastC * sizeof(GrSide); break;
        case 5: src = W.sb; n = GC * SB_STRIDE * 4; break;
        case 6: src = W.peaks; n = GC * PK_STRIDE * 4; break;
        case 7: src = W.prof; n = PROF_BYTES; break;
        case 8: src = W.nflagged; n = 256; break;           // validation counters of the last batch: [0] frames flagged by the first pass, [1] frames its memo could not decide, [32..34] repair statistics
        default: set_err("unknown tap"); return LHIP_ERR_INTERNAL;
    }
    if (n > cap) n = cap;
    if (!rt::d2h(dst, src, n, ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
    return (int64_t)n;
}

// ---- the Info tag (extension { infoTag }; lhip_infotag.h) ----
int lhip_stream_info(const lhip_stream* s, lhip_stream_info_t* info) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!info) { set_err("lhip_stream_info: null argument"); return LHIP_ERR_INTERNAL; }
    if (!s->tag) { set_err("lhip_stream_info: the stream was not created with the infoTag option (its totals are not kept)"); return LHIP_ERR_INTERNAL; }
    const TagTotals& v = *s->tag;
    info->frames = v.frames; info->audio_bytes = v.bytes; info->music_crc = v.crc & 0xffff; info->delay = s->ts->tag.delay;
    info->padding = v.padding < 0 ? -1 : (int32_t)v.padding; info->tag_bytes = s->ts->tag.size;
    return 0;
}
int64_t lhip_info_tag(lhip_stream* s, uint8_t* out, size_t cap) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!s->tag) { set_err("lhip_info_tag: the stream was not created with the infoTag option"); return LHIP_ERR_INTERNAL; }
    if (s->tag->moved) { set_err("lhip_info_tag: the stream was moved with lhip_seek or lhip_state_set; state blobs do not carry the tag's totals (combining the tags of shards is not supported)"); return LHIP_ERR_INTERNAL; }
    if (!s->tag->flushed) { set_err("lhip_info_tag: the stream has not been flushed (the tag reports the totals and the end padding of the complete stream)"); return LHIP_ERR_INTERNAL; }
    const size_t n = (size_t)s->ts->tag.size;
    if (!out || cap < n) { set_err("output buffer too small"); return LHIP_ERR_BUFFER_TOO_SMALL; }
    uint32_t radio = 0;
    if (s->gain) {          // { replayGain }: the radio field, when at least one window is complete
        int32_t tenth = 0; int64_t windows = 0, samples = 0;
        const int rc = lhip_replay_gain(s, &tenth, &windows, &samples);
        if (rc < 0) return rc;
        if (rc == 0) radio = gain_tag_field(tenth);
    }
    tag_write(s->ts->T, s->ts->tag, *s->tag, out, radio);
    return (int64_t)n;
}
// Test hooks.  lhip_debug_crc_span: the bytes one workgroup of the CRC kernel covers.  lhip_debug_crc16: the kernel (in the simulations: its body) over a
// caller's buffer, placed `misalign` bytes past a 16-byte boundary -- always the device path, whatever n is.  lhip_debug_info_toc: the seek-table
// bookkeeping alone, fed ncalls batches of frames[i] frames of `kbps`.
size_t lhip_debug_crc_span(void) { return (size_t)CRC_SPAN_BYTES; }
int lhip_debug_crc16(const void* bytes, size_t n, size_t misalign, uint32_t* crc) {
    if ((!bytes && n) || !crc || misalign > 15 || n > (size_t)1 << 40) { set_err("lhip_debug_crc16: bad argument"); return LHIP_ERR_INTERNAL; }
    if (rt::device_count() <= 0) { set_err("no HIP device available (this library has no CPU fallback)"); return LHIP_ERR_INTERNAL; }
    CrcDesc d;
    d.n = (int64_t)n; d.n_dev = nullptr; d.part0 = 0; d.nparts = (int32_t)((n + CRC_SPAN_BYTES - 1) / CRC_SPAN_BYTES);
    uint8_t* buf = (uint8_t*)rt::dmalloc(n + 32);
    uint8_t* aux = (uint8_t*)rt::dmalloc(sizeof(CrcDesc) + 16 + (size_t)d.nparts * 4);      // [descriptor | result | span remainders]
    bool ok = buf && aux;
    if (ok) {
        d.base = buf + ((16 - ((uintptr_t)buf & 15)) & 15) + misalign;
        CrcDesc* dD = (CrcDesc*)aux; uint32_t* dOut = (uint32_t*)(aux + sizeof(CrcDesc)); uint32_t* dPart = dOut + 4;
        ok = rt::h2d((void*)d.base, bytes, n, nullptr) && rt::h2d(dD, &d, sizeof d, nullptr) && rt::sync(nullptr);
#ifndef LHIP_HOSTSIM
        if (ok) {
            if (d.nparts > 0) hipLaunchKernelGGL(g_out_crc, dim3(d.nparts), dim3(64), 0, 0, (const CrcDesc*)dD, 1, dPart);
            hipLaunchKernelGGL(g_out_crc_fold, dim3(1), dim3(64), 0, 0, (const CrcDesc*)dD, (const uint32_t*)dPart, dOut);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) { set_err(std::string("g_out_crc: ") + hipGetErrorString(e)); ok = false; }
        }
#else
        if (ok) {
#ifdef LHIP_WAVESIM
            for (int b = 0; b < d.nparts; b++) wsim::run([&](int lane_) { kb_out_crc(dD, crc_find_stream(dD, 1, b), b, lane_, dPart); });
            wsim::run([&](int lane_) { kb_crc_fold(dD, 0, lane_, dPart, dOut); });
#else
            for (int b = 0; b < d.nparts; b++) kb_out_crc(dD, crc_find_stream(dD, 1, b), b, 0, dPart);
            kb_crc_fold(dD, 0, 0, dPart, dOut);
#endif
        }
#endif
        uint32_t r = 0;
        ok = ok && rt::d2h(&r, dOut, 4, nullptr) && rt::sync(nullptr);
        *crc = r & 0xffff;
    } else set_err("hipMalloc failed");
    rt::dfree(buf); rt::dfree(aux);
    return ok ? 0 : LHIP_ERR_INTERNAL;
}
// Test hook.  lhip_debug_ingest: the kernel g_ingest (in the simulations: its body) over the caller's samples, in a device buffer that ends with them and
// starts `misalign` bytes in front of them past a 16-byte boundary; the planes are buffers of exactly nsamples floats.
int lhip_debug_ingest(int format, int channels, const void* bytes, size_t nsamples, size_t misalign, float* left, float* right, int64_t* rejected) {
    const int type = fmt_type(format);
    if (!fmt_ok(format) || !fmt_ingest(type) || (channels != 1 && channels != 2) || (!bytes && nsamples) || !left || (channels == 2 && !right) || !rejected || misalign > 15 ||
        nsamples > (size_t)1 << 31 || (fmt_bps(type) >= 4 && misalign % fmt_bps(type))) { set_err("lhip_debug_ingest: bad argument"); return LHIP_ERR_INTERNAL; }
    if (rt::device_count() <= 0) { set_err("no HIP device available (this library has no CPU fallback)"); return LHIP_ERR_INTERNAL; }
    const size_t bps = fmt_bps(type), nb = nsamples * bps * (size_t)channels;
    const bool il = (format & LHIP_PCM_INTERLEAVED) && channels == 2;
    *rejected = 0;
    if (nsamples == 0) return 0;
    // [16 bytes | misalign bytes | the samples]: the block ends with the samples; in a simulation built with AddressSanitizer everything in front of them that
    // can be poisoned is (whole 8-byte granules: the piece in front of the window, and the first half of the head piece where misalign >= 8), so a wide load
    // of the ragged head is seen as well as one past the tail.  One block per plane, exactly nsamples floats: a store past the left plane is not in the right one.
    uint8_t* buf = (uint8_t*)rt::dmalloc(16 + misalign + nb);          // (device allocations are 256-byte aligned; the simulations': 16)
    float* pl = (float*)rt::dmalloc(nsamples * 4);
    float* pr = channels == 2 ? (float*)rt::dmalloc(nsamples * 4) : nullptr;
    uint8_t* aux = (uint8_t*)rt::dmalloc(sizeof(IngestDesc) + 16);
    bool ok = buf && pl && (pr || channels == 1) && aux && ((uintptr_t)buf & 15) == 0;
    uint8_t* const smp = buf ? buf + 16 + misalign : nullptr;
#if defined(LHIP_HOSTSIM) && defined(LHIP_ASAN_POISON)
    if (ok) ASAN_POISON_MEMORY_REGION(buf, 16 + (misalign & ~(size_t)7));
#endif
    if (ok) {
        IngestDesc d; memset(&d, 0, sizeof d);
        d.type = type; d.blk0 = 0; d.inter = il ? 1 : 0; d.narr = (channels == 2 && !il) ? 2 : 1;
        d.src[0] = smp; d.src[1] = d.narr == 2 ? smp + nsamples * bps : nullptr;
        d.dst[0] = pl; d.dst[1] = channels == 2 ? pr : pl;
        d.nelem = (int64_t)nsamples * (il ? 2 : 1); d.tiles = ingest_tiles(type, d.nelem);
        const int grid = (int)(d.tiles * d.narr);
        IngestDesc* dD = (IngestDesc*)aux; unsigned long long* dC = (unsigned long long*)(aux + sizeof(IngestDesc));
        unsigned long long zero = 0, cnt = 0;
        ok = rt::h2d(smp, bytes, nb, nullptr) && rt::h2d(dD, &d, sizeof d, nullptr) && rt::h2d(dC, &zero, 8, nullptr) && rt::sync(nullptr);
#ifndef LHIP_HOSTSIM
        if (ok) {
            hipLaunchKernelGGL(g_ingest, dim3(grid), dim3(64), 0, 0, (const IngestDesc*)dD, 1, PCM_F32_LIMIT, dC);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) { set_err(std::string("g_ingest: ") + hipGetErrorString(e)); ok = false; }
        }
#else
        if (ok) {
            alignas(16) static thread_local uint8_t LI[ING_WINDOW];
            for (int b = 0; b < grid; b++) {
#ifdef LHIP_WAVESIM
                wsim::run([&](int lane_) { const unsigned r = kb_ingest(dD, 0, b, lane_, LI, PCM_F32_LIMIT); if (lane_ == 0) *dC += r; });
#else
                *dC += kb_ingest(dD, 0, b, 0, LI, PCM_F32_LIMIT);
#endif
            }
        }
#endif
        ok = ok && rt::d2h(left, pl, nsamples * 4, nullptr) && (channels == 1 || rt::d2h(right, pr, nsamples * 4, nullptr)) && rt::d2h(&cnt, dC, 8, nullptr) && rt::sync(nullptr);
        *rejected = (int64_t)cnt;
    } else set_err("hipMalloc failed");
#if defined(LHIP_HOSTSIM) && defined(LHIP_ASAN_POISON)
    if (buf) ASAN_UNPOISON_MEMORY_REGION(buf, 16 + misalign);
#endif
    rt::dfree(buf); rt::dfree(pl); rt::dfree(pr); rt::dfree(aux);
    return ok ? 0 : LHIP_ERR_INTERNAL;
}
// ---- ReplayGain (extension { replayGain }; k_gain.h, lhip_gain.h) ----
static int gain_fetch(lhip_stream* s, const char* who, std::vector<uint32_t>& A, GainState& gs) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!s->gain) { set_err(std::string(who) + ": the stream was not created with the replayGain option"); return LHIP_ERR_INTERNAL; }
    if (s->gain->moved) { set_err(std::string(who) + ": the stream was moved with lhip_seek or lhip_state_set (or a chunked call failed half way); state blobs do not carry the analysis' history and histogram"); return LHIP_ERR_INTERNAL; }
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    A.assign(GAIN_BINS, 0u);
    if (!rt::set_device(ctx->device) || !rt::d2h(&gs, s->gain->state(), sizeof gs, ctx->stream) || !rt::d2h(A.data(), s->gain->bins(), (size_t)GAIN_BINS * 4, ctx->stream) || !rt::sync(ctx->stream)) return LHIP_ERR_INTERNAL;
    return 0;
}
int lhip_replay_gain(lhip_stream* s, int32_t* tenth_db, int64_t* windows, int64_t* samples) {
    if (!tenth_db || !windows || !samples) { set_err("lhip_replay_gain: null argument"); return LHIP_ERR_INTERNAL; }
    std::vector<uint32_t> A; GainState gs;
    const int rc = gain_fetch(s, "lhip_replay_gain", A, gs);
    if (rc < 0) return rc;
    *samples = gs.samples;
    return gain_result(A.data(), tenth_db, windows);
}
int lhip_debug_gain_histogram(lhip_stream* s, uint32_t* A) {
    if (!A) { set_err("lhip_debug_gain_histogram: null argument"); return LHIP_ERR_INTERNAL; }
    std::vector<uint32_t> v; GainState gs;
    const int rc = gain_fetch(s, "lhip_debug_gain_histogram", v, gs);
    if (rc < 0) return rc;
    memcpy(A, v.data(), (size_t)GAIN_BINS * 4);
    return 0;
}
// Test hook: the two kernels (in the simulations: their bodies) over n samples per channel as ONE call of a fresh stream at output rate fs; bins / energies
// receive floor(n / window) entries: each window's histogram bin and lsum + rsum.
int lhip_debug_gain_windows(int fs, int channels, const float* l, const float* r, size_t n, int32_t* bins, double* energies) {
    const int ri = gain_rate_index(fs);
    if (ri < 0 || (channels != 1 && channels != 2) || !l || (channels == 2 && !r) || n == 0 || n > 0x7fffffff || !bins || !energies) { set_err("lhip_debug_gain_windows: bad argument"); return LHIP_ERR_INTERNAL; }
    if (rt::device_count() <= 0) { set_err("no HIP device available (this library has no CPU fallback)"); return LHIP_ERR_INTERNAL; }
    const size_t nwin = n / (size_t)gain_window(ri);
    std::unique_ptr<GainRec> g(gain_create(fs, channels, nullptr));
    float* src = (float*)rt::dmalloc((size_t)channels * n * 4);                // exactly the samples: a read past them is outside the block
    int32_t* dB = (int32_t*)rt::dmalloc(nwin * 4 + 4); double* dE = (double*)rt::dmalloc(nwin * 8 + 8);
    StreamIO* dIO = (StreamIO*)rt::dmalloc(sizeof(StreamIO)); StreamDesc* dSD = (StreamDesc*)rt::dmalloc(sizeof(StreamDesc)); GainDesc* dGD = (GainDesc*)rt::dmalloc(sizeof(GainDesc));
    GainPlan P; GainRec* rec = g.get(); const int64_t nn = (int64_t)n;
    bool ok = g && src && dB && dE && dIO && dSD && dGD && gain_plan(&rec, &nn, 1, P, dB, dE);
    float* rows = ok ? (float*)rt::dmalloc(P.row_floats * 4) : nullptr;       // exactly the rows
    ok = ok && rows;
    if (ok) {
        gain_bind_rows(P, rows);
        Tables T; memset(&T, 0, sizeof T);                                    // a stream without gains, mix or resampler: the samples are used as given
        T.channels_out = channels; T.channels_in = channels; T.rs_ratio = 1; T.pcm_limit = PCM_F32_LIMIT; T.scale = 1.0;
        Workspace W; memset(&W, 0, sizeof W);
        StreamDesc sd; memset(&sd, 0, sizeof sd);
        StreamIO io; memset(&io, 0, sizeof io);
        io.src[0] = src; io.src[1] = channels == 2 ? src + n : src; io.f32 = 1; io.stride = 1; io.n_new = (int32_t)n; io.n_in = (int32_t)n;
        ok = rt::h2d(src, l, n * 4, nullptr) && (channels == 1 || rt::h2d(src + n, r, n * 4, nullptr)) && rt::h2d(dIO, &io, sizeof io, nullptr) && rt::h2d(dSD, &sd, sizeof sd, nullptr) &&
             rt::h2d(dGD, P.d.data(), sizeof(GainDesc), nullptr) && rt::sync(nullptr);
#ifndef LHIP_HOSTSIM
        if (ok) {
            hipLaunchKernelGGL(g_gain_stage, dim3(P.stage_blocks), dim3(GAIN_STAGE_NT), 0, 0, T, W, (const StreamDesc*)dSD, (const StreamIO*)dIO, (const GainDesc*)dGD, 1);
            if (P.waves > 0) { if (channels == 2) hipLaunchKernelGGL(g_gain<2>, dim3(P.waves), dim3(64), 0, 0, (const GainDesc*)dGD, 1); else hipLaunchKernelGGL(g_gain<1>, dim3(P.waves), dim3(64), 0, 0, (const GainDesc*)dGD, 1); }
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) { set_err(std::string("g_gain: ") + hipGetErrorString(e)); ok = false; }
        }
#else
        if (ok) gain_sim_run(T, W, dSD, dIO, dGD, 1, P.stage_blocks, P.waves);
#endif
        ok = ok && rt::d2h(bins, dB, nwin * 4, nullptr) && rt::d2h(energies, dE, nwin * 8, nullptr) && rt::sync(nullptr);
    } else if (g) set_err("hipMalloc failed");
    rt::dfree(src); rt::dfree(dB); rt::dfree(dE); rt::dfree(dIO); rt::dfree(dSD); rt::dfree(dGD); rt::dfree(rows);
    return ok ? (int)nwin : LHIP_ERR_INTERNAL;
}
// Test hook.  lhip_debug_quant_probe: the kernel g_quant_probe (in the simulations: its body, k_quant_probe.h) over n caller-supplied records with the tables of
// stream s.  Every index the kernel forms from a record is checked here first: the block type, the gain, the step of every band in each of the scalefactor
// states the probe visits (the pow20 table), the quantized lines (pow43), and that the numbers are finite (a NaN line has no quantized value).
static const char* probe_check_record(const ProbeIn& I, const int32_t* pretab) {
    if (I.block_type < 0 || I.block_type > 3) return "block_type outside 0..3";
    if (I.global_gain < 0 || I.global_gain > 255) return "global_gain outside 0..255";
    if ((I.scalefac_scale | 1) != 1 || (I.preflag | 1) != 1) return "scalefac_scale / preflag outside 0..1";
    const bool sh = I.block_type == SHORT_TYPE;
    if (sh && I.preflag) return "preflag on a short block (pretab has long bands only)";
    for (int w = 0; w < 3; w++) if (I.subblock_gain[w] < 0 || I.subblock_gain[w] > 7 || (!sh && I.subblock_gain[w])) return "subblock_gain outside 0..7 (0 unless the block is short)";
    if (!(I.ath_adjust > 0.0) || !(I.ath_adjust < 1e30)) return "ath_adjust not positive and finite";
    for (int i = 0; i < 576; i++) if (!(std::fabs((double)I.xr[i]) < 1e30)) return "xr not finite";
    for (int i = 0; i < E_STRIDE; i++) if (!(I.ratio[i] >= 0.f) || !(I.ratio[i] < 3e38f)) return "ratio negative or not finite";
    const int psymax = sh ? 3 * SBPSY_s : SBPSY_l;
    for (int sfb = 0; sfb < SFBMAX; sfb++) if (I.scalefac[sfb] < 0 || I.scalefac[sfb] > 255) return "scalefac outside 0..255";
    for (int sfb = 0; sfb < psymax; sfb++) {
        // the states of calls a-d, e and f: the scalefactor as given, and with its lowest bit flipped
        for (int flip = 0; flip < 2; flip++) {
            const int sf = I.scalefac[sfb] ^ flip;
            const int st = I.global_gain - ((sf + (I.preflag ? pretab[sfb] : 0)) << (I.scalefac_scale + 1)) - (sh ? I.subblock_gain[sfb % 3] : 0) * 8;
            if (st < -Q_MAX2 || st > Q_MAX) return "a band's step outside the pow20 table";
        }
    }
    if (I.flags & ~1) return "unknown flag";
    if (I.flags & 1) for (int i = 0; i < 576; i++) if (I.ix_in[i] < 0 || I.ix_in[i] > IXMAX_VAL) return "ix_in outside 0..IXMAX_VAL";
    return nullptr;
}
int lhip_debug_quant_probe(lhip_stream* s, const void* in, size_t n, void* out, int max_workgroups) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!in || !out || n == 0 || n > (size_t)1 << 20 || max_workgroups < 0) { set_err("lhip_debug_quant_probe: bad argument"); return LHIP_ERR_INTERNAL; }
    if (s->ts->fast) { set_err("lhip_debug_quant_probe: a quality 7 stream (its table set never calls calc_noise)"); return LHIP_ERR_INTERNAL; }
    const lhtb_entry* pt = find_entry(s->ts->blob.data(), "pretab");
    if (!pt || pt->dtype != 1 || pt->count < (uint32_t)SBMAX_l) { set_err("lhip_debug_quant_probe: tables blob without pretab"); return LHIP_ERR_INTERNAL; }
    const int32_t* pretab = (const int32_t*)(s->ts->blob.data() + pt->offset);
    const ProbeIn* rec = (const ProbeIn*)in;
    for (size_t i = 0; i < n; i++) {
        ProbeIn I; memcpy(&I, rec + i, sizeof I);       // (the caller's buffer need not be aligned)
        if (const char* why = probe_check_record(I, pretab)) { set_err("lhip_debug_quant_probe: record " + std::to_string(i) + ": " + why); return LHIP_ERR_INTERNAL; }
    }
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rt::set_device(ctx->device)) return LHIP_ERR_INTERNAL;
    void* st = ctx->stream;
    ProbeIn* dIn = (ProbeIn*)rt::dmalloc(n * sizeof(ProbeIn));
    ProbeOut* dOut = (ProbeOut*)rt::dmalloc(n * sizeof(ProbeOut));
    bool ok = dIn && dOut;
    if (ok) {
        ok = rt::h2d(dIn, in, n * sizeof(ProbeIn), st) && rt::dzero(dOut, n * sizeof(ProbeOut), st);
        const int nn = (int)n;
#ifndef LHIP_HOSTSIM
        if (ok) {
            const int grid = max_workgroups > 0 ? (nn < max_workgroups ? nn : max_workgroups) : (nn < 1024 ? nn : 1024);
            ProbeArgs a; a.T = s->ts->T; a.pb = s->ts->pb10; a.in = dIn; a.out = dOut; a.n = nn; a.grid = grid;
            const std::string e = probe_launch(rt::phys(ctx->device), a, st);
            if (!e.empty()) { set_err("g_quant_probe: " + e); ok = false; }
        }
#else
        if (ok) {
            ok = rt::sync(st);
            const int cap = max_workgroups > 0 && max_workgroups < PROBE_SIM_WAVES ? max_workgroups : PROBE_SIM_WAVES;
            if (ok) quant_probe_sim_run(s->ts->T, s->ts->pb10, dIn, dOut, nn, nn < cap ? nn : cap);
        }
#endif
        ok = ok && rt::d2h(out, dOut, n * sizeof(ProbeOut), st) && rt::sync(st);
    } else set_err("hipMalloc failed");
    rt::dfree(dIn); rt::dfree(dOut);
    return ok ? 0 : LHIP_ERR_INTERNAL;
}
// Test hook.  lhip_debug_bits_probe: the bit packer -- kb_bits (form 0) or kb_bits_mw (form 1), k_bits.h -- over n caller-supplied frames with the tables of stream s
// (k_bits_probe.h: how the frames are laid out for it).  Every index and every width the packer forms from a record is checked here first, and so is what
// kb_bits_mw takes on trust: that a granule-channel occupies the bits its side record announces.
struct BitsProbeTabs { const int32_t *xlen, *linmax, *off, *hlen, *sfb_l, *sfb_s, *slen1, *slen2; };
// bits of the pairs [a, b) under table t, or -1 with *why set
static int bits_probe_region(const BitsProbeTabs& H, int t, int a, int b, const int16_t* q, const char** why) {
    if (a >= b) return 0;
    if (t < 0 || t > 31 || (t != 0 && H.off[t] < 0)) { *why = "table_select: no such table"; return -1; }
    int bits = 0;
    const int lin = t > 15 ? H.xlen[t] : 0, vmax = t == 0 ? 0 : t > 15 ? 15 + H.linmax[t] : H.xlen[t] - 1;
    for (int i = a; i < b; i += 2) {
        int x1 = q[i] < 0 ? -q[i] : q[i], x2 = q[i + 1] < 0 ? -q[i + 1] : q[i + 1];
        if (x1 > vmax || x2 > vmax || x1 > IXMAX_VAL || x2 > IXMAX_VAL) { *why = "l3: a value above its table's largest (or above 8206)"; return -1; }
        if (t == 0) continue;
        if (t > 15) { if (x1 > 14) { bits += lin; x1 = 15; } if (x2 > 14) { bits += lin; x2 = 15; } }
        bits += H.hlen[H.off[t] + x1 * (t > 15 ? 16 : H.xlen[t]) + x2];
    }
    return bits;
}
// the bits granule-channel gc of a frame will occupy, or -1 with *why set
static int bits_probe_check_gc(const Tables& T, const BitsProbeTabs& H, const GrSide& G, const int16_t* q, int gr, const char** why) {
    const int GR = T.mode_gr;
    if (G.big_values < 0 || G.big_values > 576 || (G.big_values & 1)) { *why = "big_values odd or outside 0..576"; return -1; }
    if (G.count1 < G.big_values || G.count1 > 576 || ((G.count1 - G.big_values) & 3)) { *why = "count1 outside big_values..576 or not whole quadruples"; return -1; }
    if (G.block_type < 0 || G.block_type > 3) { *why = "block_type outside 0..3"; return -1; }
    if (G.global_gain < 0 || G.global_gain > 255) { *why = "global_gain outside 0..255"; return -1; }
    if ((G.preflag | 1) != 1 || (G.scalefac_scale | 1) != 1 || (G.count1table_select | 1) != 1) { *why = "preflag / scalefac_scale / count1table_select outside 0..1"; return -1; }
    for (int w = 0; w < 3; w++) if (G.subblock_gain[w] < 0 || G.subblock_gain[w] > 7) { *why = "subblock_gain outside 0..7"; return -1; }
    if (G.mode_ext < 0 || G.mode_ext > 3) { *why = "mode_ext outside 0..3"; return -1; }
    if (G.sfbmax < 0 || G.sfbmax > SFBMAX) { *why = "sfbmax outside 0..39"; return -1; }
    if (G.sfbdivide < 0 || G.sfbdivide > G.sfbmax) { *why = "sfbdivide outside 0..sfbmax"; return -1; }
    if (G.scfsi < 0 || G.scfsi > 15) { *why = "scfsi outside 0..15"; return -1; }
    const bool sh = G.block_type == SHORT_TYPE;
    int part2 = 0;
    if (GR == 2) {
        if (G.scalefac_compress < 0 || G.scalefac_compress > 15) { *why = "scalefac_compress outside 0..15"; return -1; }
        const int s1 = H.slen1[G.scalefac_compress], s2 = H.slen2[G.scalefac_compress];
        for (int sfb = 0; sfb < G.sfbmax; sfb++) {
            const int v = G.scalefac[sfb], n = sfb < G.sfbdivide ? s1 : s2;
            if (v == -1 && gr == 1) continue;                 // a band shared through scfsi: no field
            if (v < 0 || v >= (1 << n)) { *why = "scalefac: a value that does not fit its slen"; return -1; }
            part2 += n;
        }
    } else {
        const bool pre = G.preflag != 0;
        if (pre ? (G.scalefac_compress < 500 || G.scalefac_compress > 511) : (G.scalefac_compress < 0 || G.scalefac_compress > 399)) { *why = "scalefac_compress outside 0..399 (preflag: 500..511)"; return -1; }
        const int sc = G.scalefac_compress - (pre ? 500 : 0);
        const int sl[4] = {pre ? sc / 3 : (sc >> 4) / 5, pre ? sc % 3 : (sc >> 4) % 5, pre ? 0 : (sc >> 2) & 3, pre ? 0 : sc & 3};
        const int np[4] = {pre ? (sh ? 18 : 11) : (sh ? 9 : 6), pre ? (sh ? 18 : 10) : (sh ? 9 : 5), pre ? 0 : (sh ? 9 : 5), pre ? 0 : (sh ? 9 : 5)};
        for (int p = 0, i = 0; p < 4; p++)
            for (int k = 0; k < np[p]; k++, i++) {
                if (G.scalefac[i] >= (1 << sl[p])) { *why = "scalefac: a value that does not fit its slen"; return -1; }
                part2 += sl[p];
            }
    }
    int part3 = 0, b;
    if (sh) {
        int r1 = 3 * H.sfb_s[3]; if (r1 > G.big_values) r1 = G.big_values;
        const int ts[2] = {G.table_select[0] == 14 ? 16 : G.table_select[0], G.table_select[1] == 14 ? 16 : G.table_select[1]};
        if ((b = bits_probe_region(H, ts[0], 0, r1, q, why)) < 0) return -1; part3 += b;
        if ((b = bits_probe_region(H, ts[1], r1, G.big_values, q, why)) < 0) return -1; part3 += b;
        for (int i = 0; i < 2; i++) if (ts[i] < 0 || ts[i] > 31 || ts[i] == 4) { *why = "table_select: no such table"; return -1; }      // (written to the side info whatever the regions hold)
    } else {
        // (a start / stop block's counts are not transmitted: 7 and 13 in the encoder's records; only the index is bounded there)
        const bool norm = G.block_type == NORM_TYPE;
        if (G.region0_count < 0 || G.region1_count < 0 || (norm && (G.region0_count > 15 || G.region1_count > 7)) || G.region0_count + G.region1_count + 2 > SBMAX_l) { *why = "region0_count / region1_count: an index past sfb_l"; return -1; }
        int r1 = H.sfb_l[G.region0_count + 1], r2 = H.sfb_l[G.region0_count + G.region1_count + 2];
        if (r1 > G.big_values) r1 = G.big_values;
        if (r2 > G.big_values) r2 = G.big_values;
        int ts[3];
        for (int i = 0; i < 3; i++) { ts[i] = G.table_select[i] == 14 ? 16 : G.table_select[i]; if (ts[i] < 0 || ts[i] > 31 || ts[i] == 4) { *why = "table_select: no such table"; return -1; } }
        if ((b = bits_probe_region(H, ts[0], 0, r1, q, why)) < 0) return -1; part3 += b;
        if ((b = bits_probe_region(H, ts[1], r1, r2, q, why)) < 0) return -1; part3 += b;
        if ((b = bits_probe_region(H, ts[2], r2, G.big_values, q, why)) < 0) return -1; part3 += b;
    }
    const int32_t* c1 = H.hlen + H.off[32 + G.count1table_select];
    for (int i = G.big_values; i < G.count1; i += 4) {
        int p = 0;
        for (int k = 0; k < 4; k++) { const int v = q[i + k]; if (v < -1 || v > 1) { *why = "l3: a value above 1 in the count1 region"; return -1; } p = 2 * p + (v != 0); }
        part3 += c1[p];
    }
    for (int i = G.count1; i < 576; i++) if (q[i] != 0) { *why = "l3: a non-zero value at or above count1"; return -1; }
    if (G.part2_length < 0 || G.part2_3_length < 0 || G.part2_length + G.part2_3_length > 4095) { *why = "part2_length + part2_3_length outside 0..4095"; return -1; }
    if (G.part2_length + G.part2_3_length != part2 + part3) { *why = "part2_length + part2_3_length is not what the record occupies"; return -1; }
    return part2 + part3;
}
int lhip_debug_bits_probe(lhip_stream* s, const void* in, size_t n, void* out, int form, int max_workgroups) {
    if (!s || s->magic != 0x4c484950) { set_err("bad stream handle"); return LHIP_ERR_BAD_HANDLE; }
    if (!in || !out || n == 0 || n > (size_t)BITS_PROBE_MAX_RECORDS || max_workgroups < 0 || (form | 1) != 1) { set_err("lhip_debug_bits_probe: bad argument"); return LHIP_ERR_INTERNAL; }
    const Tables& T = s->ts->T;
    if (!T.disable_reservoir) { set_err("lhip_debug_bits_probe: a bit reservoir stream (its frames are not self-contained)"); return LHIP_ERR_INTERNAL; }
    const uint8_t* blob = s->ts->blob.data();
    BitsProbeTabs H;
    {
        const char* names[8] = {"ht_xlen", "ht_linmax", "ht_off", "ht_hlen", "sfb_l", "sfb_s", "slen1_tab", "slen2_tab"};
        const int32_t** dst[8] = {&H.xlen, &H.linmax, &H.off, &H.hlen, &H.sfb_l, &H.sfb_s, &H.slen1, &H.slen2};
        for (int i = 0; i < 8; i++) {
            const lhtb_entry* e = find_entry(blob, names[i]);
            if (!e || e->dtype != 1) { set_err(std::string("lhip_debug_bits_probe: tables blob without ") + names[i]); return LHIP_ERR_INTERNAL; }
            *dst[i] = (const int32_t*)(blob + e->offset);
        }
    }
    const int C = T.channels_out, GR = T.mode_gr, NGC = GR * C, nn = (int)n;
    const size_t rec_bytes = (size_t)NGC * (sizeof(GrSide) + 576 * 2);
    const int base = (int)s->ts->base_frame_bytes;
    if (base + 1 > BITS_PROBE_FRAME_BYTES) { set_err("lhip_debug_bits_probe: frame larger than the record"); return LHIP_ERR_INTERNAL; }
    // the workspace's arrays as the packer indexes them (two granule places per frame whatever GR), one StreamDesc and one output window per record
    std::vector<GrSide> side((size_t)nn * 2 * C);
    std::vector<int16_t> l3((size_t)nn * 2 * C * 576);
    std::vector<StreamDesc> sd(nn);
    std::vector<int32_t> fslot(nn), pads(nn);
    std::vector<int64_t> win(nn);
    memset((void*)side.data(), 0, side.size() * sizeof(GrSide));
    memset((void*)sd.data(), 0, sd.size() * sizeof(StreamDesc));
    int64_t out_bytes = 0;
    int lag = T.frac_SpF;                                        // a fresh stream's (lhip_create)
    for (int r = 0; r < nn; r++) {
        const uint8_t* rec = (const uint8_t*)in + (size_t)r * rec_bytes;
        memcpy((void*)&side[(size_t)r * 2 * C], rec, (size_t)NGC * sizeof(GrSide));         // (the caller's buffer need not be aligned)
        memcpy(&l3[(size_t)r * 2 * C * 576], rec + (size_t)NGC * sizeof(GrSide), (size_t)NGC * 576 * 2);
        pads[r] = host_next_padding(T, &lag);
        int bits = 8 * T.sideinfo_len;
        for (int gc = 0; gc < NGC; gc++) {
            const char* why = nullptr;
            const int b = bits_probe_check_gc(T, H, side[(size_t)r * 2 * C + gc], &l3[((size_t)r * 2 * C + gc) * 576], gc / C, &why);
            if (b < 0) { set_err("lhip_debug_bits_probe: record " + std::to_string(r) + " granule-channel " + std::to_string(gc) + ": " + why); return LHIP_ERR_INTERNAL; }
            bits += b;
        }
        if (bits > 8 * (base + pads[r])) { set_err("lhip_debug_bits_probe: record " + std::to_string(r) + ": the frame's parts exceed the frame's bits"); return LHIP_ERR_INTERNAL; }
        // frame r of a stream starts r * base + (the padded frames before it) bytes in, and r frames hold at most r paddings: the window begins BITS_PROBE_SLACK
        // bytes before the unpadded place and ends as many behind the fully padded one
        win[r] = out_bytes;
        out_bytes += (int64_t)base + 1 + r + 2 * BITS_PROBE_SLACK;
        fslot[r] = r;
        sd[r].nframes = nn; sd[r].fslot0 = -1; sd[r].gslot0 = -1; sd[r].out_slot0 = 0; sd[r].slot_lag = T.frac_SpF;
        sd[r].out_off = win[r] + BITS_PROBE_SLACK - (int64_t)r * base;
    }
    Context* ctx = s->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!rt::set_device(ctx->device)) return LHIP_ERR_INTERNAL;
    void* st = ctx->stream;
    GrSide* dSide = (GrSide*)rt::dmalloc(side.size() * sizeof(GrSide));
    int16_t* dL3 = (int16_t*)rt::dmalloc(l3.size() * 2);
    StreamDesc* dSD = (StreamDesc*)rt::dmalloc(sd.size() * sizeof(StreamDesc));
    int32_t* dFslot = (int32_t*)rt::dmalloc((size_t)nn * 4);
    int32_t* dFB = (int32_t*)rt::dmalloc((size_t)nn * 4);
    uint8_t* dOut = (uint8_t*)rt::dmalloc((size_t)out_bytes);
    std::vector<uint8_t> hOut((size_t)out_bytes);
    std::vector<int32_t> hFB(nn);
    bool ok = dSide && dL3 && dSD && dFslot && dFB && dOut;
    if (ok) {
        ok = rt::h2d(dSide, side.data(), side.size() * sizeof(GrSide), st) && rt::h2d(dL3, l3.data(), l3.size() * 2, st) && rt::h2d(dSD, sd.data(), sd.size() * sizeof(StreamDesc), st) &&
             rt::h2d(dFslot, fslot.data(), (size_t)nn * 4, st) && rt::dzero(dFB, (size_t)nn * 4, st) && rt::dzero(dOut, (size_t)out_bytes, st);
        Workspace W; memset((void*)&W, 0, sizeof W);
        W.nstreams = nn; W.nframes_total = nn; W.nfslots = nn;
        W.fslot_stream = dFslot; W.side = dSide; W.l3 = dL3; W.out = dOut; W.frame_bytes = dFB;
#ifndef LHIP_HOSTSIM
        if (ok) {
            BitsProbeArgs a; memset((void*)&a, 0, sizeof a);
            a.T = T; a.W = W; a.SD = dSD; a.n = nn; a.form = form;
            a.grid = max_workgroups > 0 ? (nn < max_workgroups ? nn : max_workgroups) : (nn < 1024 ? nn : 1024);
            const std::string e = bits_probe_launch(rt::phys(ctx->device), a, st);
            if (!e.empty()) { set_err("g_bits_probe: " + e); ok = false; }
        }
#else
        if (ok) {
            ok = rt::sync(st);
            const int cap = max_workgroups > 0 && max_workgroups < PROBE_SIM_WAVES ? max_workgroups : PROBE_SIM_WAVES;
            if (ok) bits_probe_sim_run(T, W, dSD, nn, nn < cap ? nn : cap, form);
        }
#endif
        ok = ok && rt::d2h(hOut.data(), dOut, (size_t)out_bytes, st) && rt::d2h(hFB.data(), dFB, (size_t)nn * 4, st) && rt::sync(st);
    } else set_err("hipMalloc failed");
    rt::dfree(dSide); rt::dfree(dL3); rt::dfree(dSD); rt::dfree(dFslot); rt::dfree(dFB); rt::dfree(dOut);
    if (!ok) return LHIP_ERR_INTERNAL;
    // where did each frame land?  A frame begins with the sync byte 0xff, everything before it in its window is still zero
    for (int r = 0; r < nn; r++) {
        BitsProbeOut O; memset(&O, 0, sizeof O);
        const int64_t wlen = (int64_t)base + 1 + r + 2 * BITS_PROBE_SLACK;
        const uint8_t* w = hOut.data() + win[r];
        int64_t first = 0;
        while (first < wlen && w[first] == 0) first++;
        O.nbytes = hFB[r];
        O.offset = (int64_t)r * base - BITS_PROBE_SLACK + first;
        if (O.nbytes < 0 || O.nbytes > BITS_PROBE_FRAME_BYTES || first + O.nbytes > wlen) O.status = -1;
        else {
            memcpy(O.bytes, w + first, (size_t)O.nbytes);
            for (int64_t i = first + O.nbytes; i < wlen; i++) if (w[i] != 0) O.status = -2;       // bytes written behind the frame
        }
        memcpy((uint8_t*)out + (size_t)r * sizeof O, &O, sizeof O);
    }
    return 0;
}
int lhip_debug_info_toc(const int64_t* frames, size_t ncalls, int kbps, uint8_t* toc) {
    if ((!frames && ncalls) || !toc || kbps <= 0) { set_err("lhip_debug_info_toc: bad argument"); return LHIP_ERR_INTERNAL; }
    std::unique_ptr<TagTotals> v(new TagTotals());
    for (size_t i = 0; i < ncalls; i++) { if (frames[i] < 0) { set_err("lhip_debug_info_toc: bad argument"); return LHIP_ERR_INTERNAL; } tag_toc_add(*v, frames[i], kbps); }
    tag_toc(*v, toc);
    return v->pos;
}

int lhip_kernel_timing(int enable) {
#ifndef LHIP_HOSTSIM
    std::lock_guard<std::mutex> lk(g_kt_mu);
    g_kt_on = enable != 0;
    for (int i = 0; i < KT_N; i++) { g_kt_ms[i] = 0; g_kt_calls[i] = 0; }
    return KT_N;
#else
    (void)enable; return 0;
#endif
}

int lhip_kernel_times(int idx, const char** name, double* total_ms, int64_t* launches) {
#ifndef LHIP_HOSTSIM
    if (idx < 0 || idx >= KT_N) return -1;
    std::lock_guard<std::mutex> lk(g_kt_mu);
    if (name) *name = g_kt_names[idx];
    if (total_ms) *total_ms = g_kt_ms[idx];
    if (launches) *launches = g_kt_calls[idx];
    return 0;
#else
    (void)idx; (void)name; (void)total_ms; (void)launches; return -1;
#endif
}

int lhip_debug_set_spec_seed(int start, int step) {
    if (start < 0 || start > 255 || step < 1 || step > 255) return LHIP_ERR_INTERNAL;
    g_spec_start = start; g_spec_step = step;
    return 0;
}

int lhip_debug_math(int op, const double* in, double* out, size_t n) {
#ifndef LHIP_HOSTSIM
    double *din = nullptr, *dout = nullptr;
    if (hipMalloc((void**)&din, n * 8) != hipSuccess || hipMalloc((void**)&dout, n * 8) != hipSuccess) { set_err("hipMalloc failed"); return LHIP_ERR_INTERNAL; }
    hipMemcpy(din, in, n * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(g_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, din, dout, n, pow_log2_parts(10.0));
    hipError_t e = hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost);
    hipFree(din); hipFree(dout);
    if (e != hipSuccess) { set_err(hipGetErrorString(e)); return LHIP_ERR_INTERNAL; }
    return 0;
#else
    const PowBase pb = pow_log2_parts(10.0);
    if (op == 8) { for (size_t i = 0; 21 * i + 21 <= n; i++) math_op8(in + 21 * i, out + 21 * i); return 0; }
    if (op == 10) { for (size_t i = 0; 2 * i + 2 <= n; i++) math_op10(in + 2 * i, out + 2 * i); return 0; }
    for (size_t i = 0; i < n; i++) {
        const double x = in[i];
        switch (op) {
            case 0: out[i] = v8_log10(x); break;
            case 1: out[i] = v8_pow_base(pb, x); break;
            case 2: out[i] = d_sqrt(x); break;
            case 3: out[i] = 1.0 / x; break;
            case 4: out[i] = (double)(float)x; break;
            case 5: out[i] = (double)js_toint32(x); break;
            case 7: out[i] = v8_log10_pos(x); break;
            case 11: out[i] = (double)ma_index16(x) + 1000.0 * (double)js_toint32(v8_log10_pos(x) * 16.0); break;
            case 9: { const double l = v8_log10_pos(x > 1E-20 ? x : 1E-20);
                      out[i] = (double)noise_class(x) + 1000.0 * (double)noise_class_of_log(l) + 1e6 * (double)noise_class_of_log((double)(float)l); } break;
            default: out[i] = x / 3.0 + x * 0.1; break;
        }
    }
    return 0;
#endif
}

}  // extern "C"
