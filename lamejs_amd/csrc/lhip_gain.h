// lhip_gain.h -- ReplayGain (extension { replayGain }; k_gain.h has the kernels): what a stream built with the option keeps (GainRec: the device record and
// the host's copy of its sample count), how a batch is cut into the two launches' descriptors, and the end of the analysis -- the percentile walk over the
// histogram (GainAnalysis.js:515-532), RadioGain (BitStream.js:781-787) and the Info tag's radio field (VBRTag.js:640-661).
// Host code; Tables, StreamDesc, StreamIO, StreamState and the state blobs do not know the option.
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
struct GainRec {
    uint8_t* d = nullptr;       // device: GainState | GAIN_BINS counts | two history buffers (gain_state_bytes)
    int ri = 0, channels = 1;   // row of the rate table; output channels
    int cur = 0;                // which history buffer holds the last call's samples
    int64_t samples = 0;        // samples analysed so far (host copy: it is the sum of the calls' n_out)
    bool moved = false;         // lhip_seek / lhip_state_set, or a failed chunked call, put the stream somewhere the record does not describe
    GainState* state() const { return (GainState*)d; }
    uint32_t* bins() const { return (uint32_t*)(d + sizeof(GainState)); }
    float* hist(int which, int c) const { return (float*)(d + sizeof(GainState) + (size_t)GAIN_BINS * 4) + ((size_t)which * channels + c) * gain_keep(ri); }
    ~GainRec() { rt::dfree(d); }
};
static GainRec* gain_create(int out_samplerate, int channels, void* stream) {
    const int ri = gain_rate_index(out_samplerate);
    if (ri < 0) { set_err("ReplayGain: no filter for this output sample rate"); return nullptr; }
    std::unique_ptr<GainRec> g(new GainRec());
    g->ri = ri; g->channels = channels;
    const size_t nb = gain_state_bytes(ri, channels);
    g->d = (uint8_t*)rt::dmalloc(nb);
    if (!g->d) { set_err("hipMalloc(ReplayGain state) failed"); return nullptr; }
    if (!rt::dzero(g->d, nb, stream)) return nullptr;
    return g.release();
}

// one launch pair's plan: a descriptor per stream of the batch, the grids, and where the rows live
struct GainPlan { std::vector<GainDesc> d; std::vector<size_t> off; int stage_blocks = 0, waves = 0; size_t row_floats = 0; };
// stream i of the batch analyses n[i] new samples.  Rows are laid out one behind the other, exactly as long as they are; their addresses are set once the workspace is bound (gain_bind_rows).
static bool gain_plan(GainRec* const* recs, const int64_t* n, int S, GainPlan& P, int32_t* dbg_bin = nullptr, double* dbg_energy = nullptr) {
    P.d.assign((size_t)S, GainDesc{}); P.off.assign((size_t)2 * S, 0);
    int64_t blocks = 0, waves = 0; size_t floats = 0;
    for (int i = 0; i < S; i++) {
        GainRec& g = *recs[i]; GainDesc& d = P.d[i];
        const int window = gain_window(g.ri), keep = gain_keep(g.ri);
        d.state = g.state(); d.bins = g.bins(); d.ri = g.ri; d.channels = g.channels; d.samples = g.samples;
        d.h = (int32_t)(g.samples < keep ? g.samples : keep); d.n = (int32_t)n[i];
        const int64_t total = (int64_t)d.h + d.n;
        d.keep = (int32_t)(total < keep ? total : keep);
        d.win0 = g.samples / window;                                    // windows complete so far = the first one this call can complete
        d.nwin = (int32_t)((g.samples + n[i]) / window - d.win0);
        d.blk0 = (int32_t)blocks; d.wave0 = (int32_t)waves;
        d.dbg_bin = dbg_bin; d.dbg_energy = dbg_energy;
        for (int c = 0; c < 2; c++) {
            const int cc = c < g.channels ? c : 0;
            d.hist_old[c] = g.hist(g.cur, cc); d.hist_new[c] = g.hist(g.cur ^ 1, cc);
            P.off[2 * i + c] = floats + (size_t)cc * (size_t)total;                    // (the row's address: gain_bind_rows)
        }
        if (d.n > 0) {
            blocks += (total + GAIN_STAGE_NT - 1) / GAIN_STAGE_NT; waves += (d.nwin + LHIP_NL - 1) / LHIP_NL;
            floats += (size_t)g.channels * (size_t)total;
        }
    }
    if (blocks > 0x7fffffff || waves > 0x7fffffff) { set_err("too many samples in one call"); return false; }
    P.stage_blocks = (int)blocks; P.waves = (int)waves; P.row_floats = floats;
    return true;
}
static void gain_bind_rows(GainPlan& P, float* rows) { for (size_t i = 0; i < P.d.size(); i++) for (int c = 0; c < 2; c++) P.d[i].row[c] = rows + P.off[2 * i + c]; }
// GainAnalysis.js:515-532 analyzeResult and BitStream.js:783-785: 0 and *tenth_db = RadioGain, or 1 (no window complete: the reference asserts there)
static int gain_result(const uint32_t* A, int32_t* tenth_db, int64_t* windows) {
    int64_t elems = 0;
    for (int i = 0; i < GAIN_BINS; i++) elems += A[i];
    *windows = elems; *tenth_db = 0;
    if (elems == 0) return 1;
    int64_t upper = (int64_t)ceil((double)elems * (1. - 0.95));          // RMS_PERCENTILE; the reference's expression (1 - 0.95 is a little above 0.05)
    int i = GAIN_BINS;
    while (i-- > 0) if ((upper -= A[i]) <= 0) break;
    const double gain = 64.82 - (double)i / 100.;                       // PINK_REF - i / STEPS_per_dB
    *tenth_db = (int32_t)floor(gain * 10.0 + 0.5);
    return 0;
}
// the Info tag's radio ReplayGain field: name code 1 (radio), originator 3 (determined automatically), sign, nine bits of tenths of a dB
static uint32_t gain_tag_field(int32_t tenth_db) {
    int32_t g = tenth_db > 0x1FE ? 0x1FE : (tenth_db < -0x1FE ? -0x1FE : tenth_db);
    return 0x2000u | 0x0C00u | (g < 0 ? 0x200u : 0u) | (uint32_t)(g < 0 ? -g : g);
}
