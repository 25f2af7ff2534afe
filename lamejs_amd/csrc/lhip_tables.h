// lhip_tables.h -- a configuration's table blob on the device: parsed, checked against the supported envelope, index tables derived (TableSet).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// tables (shared between streams with identical blobs)
// ===========================================================================================
struct lhtb_entry { char name[32]; uint32_t dtype, count, offset, pad; };

struct TableSet {
    Tables T;               // device pointers
    PowBase pb10;
    std::vector<uint8_t> blob;
    void* d_blob = nullptr;
    void* d_extra = nullptr;
    void* d_qtabs = nullptr;
    int device = 0;
    int base_frame_bytes = 0;
    bool bad_option = false;  // build_tables refused an option of the blob -- input gains, frame protection, header flags, the Info tag, ReplayGain (lhip_create: -3)
    InfoTagCfg tag;           // { infoTag } (lhip_infotag.h): host-side only, no kernel sees it
    bool skip_tail = false;   // the lowpass zeroes the polyphase bands 28..31 (lines 504..575): long blocks end below line 512, launch the batch kernels that skip the dead round of pairs
    int gain_on = 0;          // { replayGain } (lhip_gain.h): the streams of this blob analyse the samples they consume; host-side only
    bool fast = false;        // { quality: 7 }: no noise shaping and no Huffman region search -- a batch's speculative quantization pass is g_quant_fast (k_quant_fast.h)
    ~TableSet() { rt::dfree(d_blob); rt::dfree(d_extra); rt::dfree(d_qtabs); }
};

// LAMEJS_HIP_NO_FAST_QUANT=1 (read once per process): fast table sets go through the general quantization kernels, which read the same switches (the A/B
// of g_quant_fast, and a second yardstick for it)
static bool fast_quant_allowed() { static const bool off = []() { const char* e = getenv("LAMEJS_HIP_NO_FAST_QUANT"); return e && e[0] == '1'; }(); return !off; }

static const lhtb_entry* find_entry(const uint8_t* b, const char* name) {
    uint32_t n; memcpy(&n, b + 8, 4);
    const lhtb_entry* e = (const lhtb_entry*)(b + 16);
    for (uint32_t i = 0; i < n; i++) if (strncmp(e[i].name, name, 32) == 0) return &e[i];
    return nullptr;
}

// the blob's header, its upload, and every configuration value and array pointer it names
static bool parse_blob(TableSet& ts, const void* blob, size_t nbytes, void* stream) {
    if (nbytes < 16) { set_err("tables blob too small"); return false; }
    uint32_t magic, total;
    memcpy(&magic, blob, 4); memcpy(&total, (const uint8_t*)blob + 12, 4);
    if (magic != 0x4254484cu || total > nbytes) { set_err("tables blob: bad magic/size"); return false; }
    ts.blob.assign((const uint8_t*)blob, (const uint8_t*)blob + total);
    const uint8_t* b = ts.blob.data();
    ts.d_blob = rt::dmalloc(total);
    if (!ts.d_blob) { set_err("hipMalloc(tables) failed"); return false; }
    if (!rt::h2d(ts.d_blob, b, total, stream)) return false;
    Tables& T = ts.T;
    memset(&T, 0, sizeof T);
    bool ok = true;
    auto arr = [&](const char* name, uint32_t dtype, int* count) -> const void* {
        const lhtb_entry* e = find_entry(b, name);
        if (!e || e->dtype != dtype) { set_err(std::string("tables blob: entry missing: ") + name); ok = false; return nullptr; }
        if (count) *count = (int)e->count;
        return (const uint8_t*)ts.d_blob + e->offset;
    };
    auto host_arr = [&](const char* name) -> const void* { const lhtb_entry* e = find_entry(b, name); return e ? b + e->offset : nullptr; };
    bool optional = false;               // an entry that only blobs built with the option have: missing is -1, not an error
    auto named = [&](const char* names_key, const char* key) -> int {
        const lhtb_entry* e = find_entry(b, names_key);
        if (!e) { ok = false; return 0; }
        const int32_t* chars = (const int32_t*)(b + e->offset);
        std::string all;
        for (uint32_t i = 0; i < e->count && chars[i]; i++) all.push_back((char)chars[i]);
        size_t pos = 0; int idx = 0;
        while (pos <= all.size()) {
            size_t c = all.find(',', pos);
            if (c == std::string::npos) c = all.size();
            if (all.compare(pos, c - pos, key) == 0) return idx;
            idx++; pos = c + 1;
        }
        if (optional) return -1;
        set_err(std::string("tables blob: config key missing: ") + key); ok = false; return 0;
    };
    const int32_t* ci = (const int32_t*)host_arr("cfg_i");
    const double* cd = (const double*)host_arr("cfg_d");
    if (!ci || !cd) { set_err("tables blob: cfg arrays missing"); return false; }
#define CI(f) T.f = ci[named("cfg_i_names", #f)]
#define CD(f) T.f = cd[named("cfg_d_names", #f)]
    CI(channels_out); CI(mode); CI(mode_gr); CI(version); CI(samplerate_index); CI(bitrate_index); CI(brate);
    CI(out_samplerate); CI(sideinfo_len); CI(frac_SpF); CI(noise_shaping); CI(noise_shaping_amp);
    CI(noise_shaping_stop); CI(subblock_gain); CI(use_best_huffman); CI(full_outer_loop); CI(substep_shaping);
    CI(sfb21_extra); CI(quant_comp); CI(quant_comp_short); CI(short_blocks_coupled); CI(useTemporal);
    CI(ATH_useAdjust); CI(athaa_loudapprox); CI(copyright); CI(original); CI(emphasis); CI(extension);
    CI(error_protection); CI(npart_l); CI(npart_s); CI(in_samplerate); CI(rs_filter_l); CI(rs_bpc);
    CI(disable_reservoir);
    CD(resample_ratio);
    CD(scale); CD(attackthre); CD(attackthre_s); CD(interChRatio); CD(masking_lower_long); CD(masking_lower_short);
    CD(ATH_aaSensitivityP); CD(ATH_floor); CD(decay); CD(ma_max_i1); CD(ma_max_i2); CD(ma_max_m); CD(VO_SCALE);
    CD(msfix); CD(ATHlower);
    // input gains and downmix (extension): entries that exist only in blobs built with { downmix, scale, scaleLeft, scaleRight }.  Without them:
    // as many channels come in as go out, the preset's scale is in force by the plain comparison (which agrees with the reference's NEQ for
    // every preset value), no per-channel gain.
    optional = true;
#define CIO(f, dflt) { const int k_ = named("cfg_i_names", #f); T.f = k_ >= 0 ? ci[k_] : (dflt); }
#define CDO(f, dflt) { const int k_ = named("cfg_d_names", #f); T.f = k_ >= 0 ? cd[k_] : (dflt); }
    CIO(channels_in, T.channels_out); CIO(do_scale, (!(T.scale == 0.0) && !(T.scale == 1.0)) ? 1 : 0); CIO(do_scale_left, 0); CIO(do_scale_right, 0);
    CDO(scale_left, 0.0); CDO(scale_right, 0.0);
    // the Info tag (extension { infoTag }): entries only a blob built with the option has; they stay on the host (TableSet::tag)
    {
        InfoTagCfg& G = ts.tag;
#define CTAG(f, key) { const int k_ = named("cfg_i_names", key); G.f = k_ >= 0 ? ci[k_] : 0; }
        CTAG(on, "info_tag"); CTAG(quality, "tag_quality"); CTAG(method, "tag_method"); CTAG(lowpass, "tag_lowpass"); CTAG(flags, "tag_flags");
        CTAG(misc, "tag_misc"); CTAG(preset, "tag_preset"); CTAG(delay, "tag_delay");
#undef CTAG
        const lhtb_entry* tv = find_entry(b, "tag_version");
        if (G.on && (!tv || tv->dtype != 1 || tv->count != 9)) { set_err("tables blob: entry missing: tag_version"); ok = false; }
        else if (G.on) for (int i = 0; i < 9; i++) G.version[i] = (uint8_t)((const int32_t*)(b + tv->offset))[i];
    }
    { const int k_ = named("cfg_i_names", "replay_gain"); ts.gain_on = k_ >= 0 ? ci[k_] : 0; }      // { replayGain }: only a blob built with the option has the entry
#undef CIO
#undef CDO
    optional = false;
#undef CI
#undef CD
#define AF(f) T.f = (const float*)arr(#f, 2, nullptr)
#define AI(f) T.f = (const int32_t*)arr(#f, 1, nullptr)
#define AD(f) T.f = (const double*)arr(#f, 3, nullptr)
    AF(rs_blackfilt);
    AF(amp_filter); AF(ATH_l); AF(ATH_s); AF(ATH_psfb21); AF(ATH_psfb12); AF(ATH_cb_l); AF(ATH_cb_s); AF(eql_w);
    AF(pow43); AF(adj43); AF(ipow20); AF(pow20); AF(longfact); AF(shortfact); AF(rnumlines_l); AF(bo_l_weight);
    AF(bo_s_weight); AF(s3_ll); AF(s3_ss); AF(window); AF(window_s); AF(mld_l); AF(mld_s);
    AI(sfb_l); AI(sfb_s); AI(psfb21); AI(psfb12); AI(bv_scf); AI(numlines_l); AI(numlines_s); AI(bo_l); AI(bm_l);
    AI(bo_s); AI(bm_s); AI(s3ind); AI(s3ind_s); AI(fft_rv_tbl); AI(mdct_order); AI(pretab); AI(scfsi_band);
    AI(slen1_n); AI(slen2_n); AI(slen1_tab); AI(slen2_tab); AI(scale_short); AI(scale_long); AI(huf_tbl_noESC);
    AI(ht_xlen); AI(ht_linmax); AI(ht_off); AI(ht_code); AI(ht_hlen); AI(largetbl); AI(table23); AI(table56);
    AI(t32l); AI(t33l);
    T.version_bytes = (const int32_t*)arr("version_bytes", 1, &T.n_version_bytes);
    AD(fht_twiddle); AD(fht_costab); AD(enwindow); AD(mdct_win); AD(ma_tab); AD(ma_table1); AD(ma_table2);
    AD(ma_table3); AD(hpf_fircoef);
#undef AF
#undef AI
#undef AD
    return ok;
}
static bool check_envelope(TableSet& ts, const lhip_config& cfg) {
    Tables& T = ts.T;
    const uint8_t* b = ts.blob.data();
    // MPEGMode: 0 stereo, 1 joint stereo (an extension -- the reference's Mp3Encoder never asks for it, index.js:105), 3 mono
    if (!((T.mode == 0 && T.channels_out == 2) || (T.mode == 1 && T.channels_out == 2) || (T.mode == 3 && T.channels_out == 1))) { set_err("configuration outside the supported envelope (channel mode)"); return false; }
    T.psy_channels = (T.mode == 1) ? 4 : T.channels_out;
    // ---- envelope checks: fail loudly rather than produce different bytes than the reference ----
    // (cfg.channels counts INPUT channels: a downmix blob has channels_in = 2, channels_out = 1)
    if (!(T.channels_in == T.channels_out || (T.channels_in == 2 && T.channels_out == 1))) { set_err("tables blob: channels_in does not fit channels_out"); return false; }
    if (T.channels_in != (cfg.channels == 1 ? 1 : 2) || T.in_samplerate != cfg.samplerate || T.brate <= 0) { set_err("tables blob does not match the requested configuration"); return false; }
    // input gains: samples behind the gains must stay inside the range every kernel was proven for, |x| <= PCM_F32_LIMIT
    {
        T.do_scale = T.do_scale != 0; T.do_scale_left = T.do_scale_left != 0; T.do_scale_right = T.do_scale_right != 0;
        if (T.channels_in == 1) T.do_scale_right = 0;                       // one input channel: scale_right is dead
        const bool down = T.channels_in == 2 && T.channels_out == 1;
        if (!std::isfinite(T.scale) || !std::isfinite(T.scale_left) || !std::isfinite(T.scale_right)) { set_err("input gains: scale, scale_left and scale_right must be finite"); ts.bad_option = true; return false; }
        if (T.scale < 0) { set_err("input gains: scale must not be negative (the reference asserts scale >= 0)"); ts.bad_option = true; return false; }
        const double gl = (T.do_scale ? T.scale : 1.0) * (T.do_scale_left ? T.scale_left : 1.0);
        const double gr = ((T.do_scale && !down) ? T.scale : 1.0) * (T.do_scale_right ? T.scale_right : 1.0);     // the reference's downmix exception: `scale` never reaches the right samples
        const double g = fmax(1.0, fmax(fabs(gl), fabs(gr)));
        if (g > 4.0) { set_err("input gains: the combined gain of a channel must not exceed 4 in magnitude (Int16 full scale then ends exactly at the sample limit, 131072)"); ts.bad_option = true; return false; }
        T.pcm_limit = (float)((double)PCM_F32_LIMIT / g);
        T.in_mix = down ? 2 : ((T.do_scale_left || T.do_scale_right) ? 1 : 0);
    }
    // resampling (Lame.js:1849): only integer decimation ratios, where the reference's filter is a fixed 33-tap FIR
    // (extension: a blob built with { fractionalResample } carries the reference's set-up for a non-integer ratio -- filter_l = 31 and all
    //  2 * bpc + 1 windows; such a stream is a call-sequence stream, see frac_pass)
    T.rs_ratio = 1; T.rs_frac = 0;
    if (T.resample_ratio < .9999 || T.resample_ratio > 1.0001) {
        const int r = T.out_samplerate > 0 ? T.in_samplerate / T.out_samplerate : 0;
        const lhtb_entry* bf = find_entry(b, "rs_blackfilt");
        const bool nonint = !(fabs(T.resample_ratio - floor(.5 + T.resample_ratio)) < .0001);
        if (T.rs_filter_l == RS_TAPS - 2 && nonint && T.out_samplerate > 0 && T.resample_ratio == (double)T.in_samplerate / T.out_samplerate &&
            T.rs_bpc >= 1 && T.rs_bpc <= 320 && bf && bf->count == (uint32_t)(2 * T.rs_bpc + 1) * (RS_TAPS - 1) && T.disable_reservoir) {
            T.rs_ratio = 0; T.rs_frac = 1;
        } else if (r < 2 || r * T.out_samplerate != T.in_samplerate || T.rs_filter_l != RS_TAPS - 1 || T.rs_bpc != 1) {
            set_err("configuration outside the supported envelope (resampling by a non-integer ratio)"); return false;
        } else T.rs_ratio = r;
    }
    if ((T.version != 1 && T.version != 0) || T.mode_gr != (T.version == 1 ? 2 : 1) || T.quant_comp != 9 || T.quant_comp_short != 9 || T.sfb21_extra ||
        T.substep_shaping != 0 || T.noise_shaping_amp > 2 || T.use_best_huffman > 1 || T.athaa_loudapprox != 2 || T.full_outer_loop != 0) {
        set_err("configuration outside the supported envelope (MPEG-1/2/2.5 CBR, the switches of quality 3 or 7)"); return false;
    }
    ts.fast = T.noise_shaping == 0 && T.use_best_huffman == 0;
    // frame protection and header flags (extension { protect, copyright, original, privateBit, emphasis }): the side information of a protected stream is
    // two bytes longer (Lame.js:1109-1110) -- every budget reads sideinfo_len, so it must be the mode's value plus exactly what the flag says
    {
        const int base = T.version == 1 ? (T.channels_out == 1 ? 4 + 17 : 4 + 32) : (T.channels_out == 1 ? 4 + 9 : 4 + 17);
        if ((T.error_protection != 0 && T.error_protection != 1) || T.sideinfo_len != base + 2 * T.error_protection) {
            set_err("frame protection: sideinfo_len must be the mode's " + std::to_string(base) + " bytes, plus 2 exactly when error_protection is set"); ts.bad_option = true; return false;
        }
        if ((T.copyright & ~1) || (T.original & ~1) || (T.extension & ~1) || !(T.emphasis == 0 || T.emphasis == 1 || T.emphasis == 3)) {
            set_err("header flags: copyright, original and extension are 0 or 1, emphasis is 0, 1 or 3 (2 is reserved)"); ts.bad_option = true; return false;
        }
        // the stand-in frames of a non-integer-ratio stream's flush are written by the host without a CRC of their own
        if (T.error_protection && T.rs_frac) { set_err("frame protection cannot be combined with fractionalResample (the flush's stand-in frames carry no pinned CRC)"); ts.bad_option = true; return false; }
    }
    // the Info tag (extension { infoTag }): the frame must hold the tag behind its side information -- LAME switches the tag off silently where it does not, here
    // the stream is refused -- and the flush of a non-integer-ratio stream is partly host stand-ins with a fractional padding: no totals to report
    if (ts.tag.on) {
        InfoTagCfg& G = ts.tag;
        if (G.on != 1) { set_err("Info tag: info_tag is 0 or 1"); ts.bad_option = true; return false; }
        if (T.rs_frac) { set_err("the Info tag cannot be combined with fractionalResample (the flush's frames are partly host stand-ins and its padding is fractional)"); ts.bad_option = true; return false; }
        G.size = T.out_samplerate > 0 ? (int)(((int64_t)(T.version + 1) * 72000 * T.brate) / T.out_samplerate) : 0;
        if (T.sideinfo_len + TAG_BODY_BYTES > G.size || G.size > TAG_MAX_FRAME) {
            set_err("Info tag: a frame of " + std::to_string(G.size) + " bytes cannot hold the tag (" + std::to_string(T.sideinfo_len) + " bytes of header and side information + " +
                    std::to_string((int)TAG_BODY_BYTES) + ", at most " + std::to_string((int)TAG_MAX_FRAME) + ")");
            ts.bad_option = true; return false;
        }
    }
    // ReplayGain (extension { replayGain }): the analysis reads the samples behind the resampler where the kernels leave them -- a non-integer-ratio stream's flush is
    // partly host stand-ins that no kernel sees, so there is no complete sample stream to analyse
    if (ts.gain_on) {
        if (ts.gain_on != 1) { set_err("ReplayGain: replay_gain is 0 or 1"); ts.bad_option = true; return false; }
        if (T.rs_frac) { set_err("ReplayGain cannot be combined with fractionalResample (the flush's frames are partly host stand-ins: the analysed sample stream would be incomplete)"); ts.bad_option = true; return false; }
        if (gain_rate_index(T.out_samplerate) < 0) { set_err("ReplayGain: no filter for an output sample rate of " + std::to_string(T.out_samplerate)); ts.bad_option = true; return false; }
    }
    return true;
}
// derived index tables
static bool derive_index_tables(TableSet& ts, void* stream) {
    Tables& T = ts.T;
    const uint8_t* b = ts.blob.data();
    auto host_arr = [&](const char* name) -> const void* { const lhtb_entry* e = find_entry(b, name); return e ? b + e->offset : nullptr; };
    const int32_t* h_s3ind = (const int32_t*)host_arr("s3ind");
    const int32_t* h_s3ind_s = (const int32_t*)host_arr("s3ind_s");
    const int32_t* h_nl = (const int32_t*)host_arr("numlines_l");
    const int32_t* h_ns = (const int32_t*)host_arr("numlines_s");
    const int32_t* h_bo_l = (const int32_t*)host_arr("bo_l");
    const int32_t* h_bo_s = (const int32_t*)host_arr("bo_s");
    std::vector<int32_t> extra(4 * CBANDS, 0);
    int k = 0, j = 0;
    for (int p = 0; p < T.npart_l; p++) { extra[p] = k; k += h_s3ind[2 * p + 1] - h_s3ind[2 * p] + 1; extra[2 * CBANDS + p] = j; j += h_nl[p]; }
    if (j != HBLKSIZE) { set_err("long partitions do not cover 513 lines"); return false; }
    T.n_s3_ll = k;
    if (k > PSYB_S3_LDS) { set_err("configuration outside the supported envelope (spreading table larger than g_psyB's LDS copy)"); return false; }
    k = 0; j = 0;
    for (int p = 0; p < T.npart_s; p++) { extra[CBANDS + p] = k; k += h_s3ind_s[2 * p + 1] - h_s3ind_s[2 * p] + 1; extra[3 * CBANDS + p] = j; j += h_ns[p]; }
    if (j != HBLKSIZE_s) { set_err("short partitions do not cover 129 lines"); return false; }
    // convert_partition2scalefac walks partitions and bands together (PsyModel.js:644-734): band sb adds partitions
    // up to min(bo[sb], npart), then splits the partition it stopped at with band sb+1.  Where bo[] does not grow
    // (8 kHz short blocks) the walk stops at max(entry, bo[sb]) rather than bo[sb]; the kernel works per band from the
    // stopping points, so hand it those instead of the raw bo[] (identical wherever bo[] is strictly increasing).
    auto walk = [&](const int32_t* bo, int nb, int npart, int32_t* stop) {
        int b = 0, sb = 0;
        for (; sb < nb; ++b, ++sb) {
            const int lim = bo[sb] < npart ? bo[sb] : npart;
            if (b < lim) b = lim;
            stop[sb] = b;
            if (b >= npart) { ++sb; break; }
        }
        for (; sb < nb; ++sb) stop[sb] = npart;              // bands the walk never reaches (zero-filled by the kernel)
    };
    extra.resize(4 * CBANDS + SBMAX_l + SBMAX_s);
    walk(h_bo_l, SBMAX_l, T.npart_l, extra.data() + 4 * CBANDS);
    walk(h_bo_s, SBMAX_s, T.npart_s, extra.data() + 4 * CBANDS + SBMAX_l);
    // the polyphase band filter by output index (k_fb.h poly_slot): amp_by_out[order[band]] = amp_filter[band] where it scales at all
    const size_t amp_at = (extra.size() + 1) & ~(size_t)1;                   // 8-byte aligned
    extra.resize(amp_at + 64);
    {
        const float* h_af = (const float*)host_arr("amp_filter");
        // the band filter (lowpass and highpass: { lowpass, lowpassWidth, highpass, highpassWidth }): products of two cosine ramps, so every value lies in [0, 1]
        for (int band = 0; band < 32; band++)
            if (!std::isfinite(h_af[band]) || h_af[band] < 0.f || h_af[band] > 1.f) { set_err("band filter: amp_filter[" + std::to_string(band) + "] is not a finite value in [0, 1]"); ts.bad_option = true; return false; }
        ts.skip_tail = (double)h_af[28] < 1e-12 && (double)h_af[29] < 1e-12 && (double)h_af[30] < 1e-12 && (double)h_af[31] < 1e-12;      // (k_fb.h: such a band is zero-filled)
        const int32_t* h_order = (const int32_t*)host_arr("mdct_order");
        double amp[32];
        for (int i = 0; i < 32; i++) amp[i] = 1.0;
        T.amp_mask = 0;
        for (int band = 0; band < 32; band++) {
            const double af = (double)h_af[band];
            const int ob = h_order[band];
            if (ob < 0 || ob > 31) { set_err("mdct_order is not a permutation of 0..31"); return false; }
            if (!(af < 1e-12) && af < 1.0) { amp[ob] = af; T.amp_mask |= 1 << ob; }
        }
        memcpy(extra.data() + amp_at, amp, sizeof amp);
    }
    // calc_noise's systolic fold (k_quant_noise.h): lane l owns the lines n l .. n l + n - 1 of the (re-ordered) spectrum, n = noise_nln; per lane,
    // bit k = line n l + k is the first line of its scalefactor band, bit 16 + k = it is the last one ([0..63] long, [64..127] short blocks);
    // then the widest band among bands 0 .. b: 24 entries for long blocks, 40 for short ones (band = 3 * sfb + window).
    // noise_nln: calc_noise reads the sums of the bands below psymax only -- 21 long or 3 * 12 short ones, sfb21_extra being refused above --
    // so the lines from sfb_l[21] and 3 * sfb_s[12] on are never needed: 7 lines per lane (448 lines) where both borders fit, else all 576
    // with 9.  (6 would fit 48 kHz, but an even lane stride brings LDS bank conflicts.)
    const size_t fold_at = extra.size();
    extra.resize(fold_at + 128 + 24 + 40 + 289);
    {
        const int32_t* h_sl = (const int32_t*)host_arr("sfb_l");
        const int32_t* h_ss = (const int32_t*)host_arr("sfb_s");
        std::vector<int> band_l(576), band_s(576);
        for (int d = 0, sfb = 0; d < 576; d++) { while (sfb < SBMAX_l - 1 && h_sl[sfb + 1] <= d) sfb++; band_l[d] = sfb; }
        for (int d = 0, sfb = 0; d < 576; d++) {
            while (sfb < SBMAX_s - 1 && 3 * h_ss[sfb + 1] <= d) sfb++;
            const int st = h_ss[sfb], w = h_ss[sfb + 1] - st;
            band_s[d] = 3 * sfb + (w > 0 ? (d - 3 * st) / w : 0);
        }
        const int nln = (h_sl[SBPSY_l] <= 64 * 7 && 3 * h_ss[SBPSY_s] <= 64 * 7) ? 7 : 9;
        T.noise_nln = nln;
        for (int sh = 0; sh < 2; sh++) {
            const std::vector<int>& b = sh ? band_s : band_l;
            for (int ln = 0; ln < 64; ln++) {
                uint32_t m = 0;
                for (int kk = 0; kk < nln; kk++) {
                    const int jj = nln * ln + kk;
                    if (jj == 0 || b[jj - 1] != b[jj]) m |= 1u << kk;
                    if (jj == 575 || b[jj + 1] != b[jj]) m |= 1u << (16 + kk);
                }
                // the short window (3 lines per lane, lines 0..191): the same marks at bits 12 + k and 28 + k (the 9-line form uses 0..8 and 16..24)
                for (int kk = 0; kk < 3; kk++) {
                    const int jj = 3 * ln + kk;
                    if (jj == 0 || b[jj - 1] != b[jj]) m |= 1u << (12 + kk);
                    if (b[jj + 1] != b[jj]) m |= 1u << (28 + kk);
                }
                extra[fold_at + 64 * sh + ln] = (int32_t)m;
            }
            // the highest band that ends at or below line 192
            int hb = -1;
            for (int jj = 0; jj < 192; jj++) if (b[jj + 1] != b[jj]) hb = b[jj];
            T.noise_hib3[sh] = hb;
        }
        int mx = 0;
        for (int i = 0; i < 24; i++) { if (i < SBMAX_l) { const int w = h_sl[i + 1] - h_sl[i]; if (mx < w) mx = w; } extra[fold_at + 128 + i] = mx; }
        mx = 0;
        for (int i = 0; i < 40; i++) { if (i < 3 * SBMAX_s) { const int w = h_ss[i / 3 + 1] - h_ss[i / 3]; if (mx < w) mx = w; } extra[fold_at + 128 + 24 + i] = mx; }
        // count_bits, NORM blocks (Takehiro.js:575-590): everything it derives from big_values = 2 e in one word -- the region borders
        // a1 = sfb_l[r0 + 1], a2 = sfb_l[r0 + r1 + 2] (10 bits each), the region counts r0 = bv_scf[i - 2], r1 = bv_scf[i - 1] (4 + 3 bits) and
        // PrevNoise.sfb_count1 = the band of line i - 1, plus one (5 bits)
        {
            const int32_t* h_bv = (const int32_t*)host_arr("bv_scf");
            extra[fold_at + 128 + 24 + 40] = 0;
            for (int e = 1; e <= 288; e++) {
                const int i = 2 * e, r0 = h_bv[i - 2], r1 = h_bv[i - 1];
                if (r0 < 0 || r0 > 15 || r1 < 0 || r1 > 7 || r0 + r1 + 2 > SBMAX_l) { set_err("bv_scf outside the range count_bits' region table is packed for"); return false; }
                const int a1 = h_sl[r0 + 1], a2 = h_sl[r0 + r1 + 2];
                extra[fold_at + 128 + 24 + 40 + e] = (int32_t)((uint32_t)a1 | ((uint32_t)a2 << 10) | ((uint32_t)r0 << 20) | ((uint32_t)r1 << 24) | ((uint32_t)(band_l[i - 1] + 1) << 27));
            }
        }
    }
    // psyA's partition energies as a systolic fold (k_psy_a.h): lane l owns the FFT lines 8 l .. 8 l + 7; per lane three words -- marks
    // (bit k: line 8 l + k is the first of its partition, bit 8 + k: the last one, counting line 512 as part of the spectrum) and
    // the partition numbers of its eight lines, a byte each
    const size_t psyfold_at = extra.size();
    extra.resize(psyfold_at + 3 * 64);
    {
        std::vector<int> part(514, 0);
        for (int p = 0, jj = 0; p < T.npart_l; p++) for (int i = 0; i < h_nl[p] && jj < 513; i++) part[jj++] = p;
        part[513] = -1;
        int mx = 0;
        for (int p = 0; p < T.npart_l; p++) if (mx < h_nl[p]) mx = h_nl[p];
        T.psy_maxlen_l = mx;
        for (int ln = 0; ln < 64; ln++) {
            uint32_t m = 0, w[2] = {0, 0};
            for (int kk = 0; kk < 8; kk++) {
                const int jj = 8 * ln + kk;
                if (jj == 0 || part[jj - 1] != part[jj]) m |= 1u << kk;
                if (part[jj + 1] != part[jj]) m |= 1u << (8 + kk);
                w[kk >> 2] |= (uint32_t)part[jj] << (8 * (kk & 3));
            }
            extra[psyfold_at + 3 * ln] = (int32_t)m; extra[psyfold_at + 3 * ln + 1] = (int32_t)w[0]; extra[psyfold_at + 3 * ln + 2] = (int32_t)w[1];
        }
        const float* h_eql = (const float*)host_arr("eql_w");
        for (int i = 0; i < BLKSIZE / 2; i++) if (!(h_eql[i] >= 0.f)) { set_err("eql_w has a negative entry (the loudness sum's error bound needs non-negative terms)"); return false; }
    }
    ts.d_extra = rt::dmalloc(extra.size() * 4);
    if (!ts.d_extra) { set_err("hipMalloc failed"); return false; }
    if (!rt::h2d(ts.d_extra, extra.data(), extra.size() * 4, stream)) return false;
    if (!rt::sync(stream)) return false;
    T.s3off_l = (const int32_t*)ts.d_extra; T.s3off_s = T.s3off_l + CBANDS; T.lineoff_l = T.s3off_l + 2 * CBANDS; T.lineoff_s = T.s3off_l + 3 * CBANDS;
    T.bo_l = T.s3off_l + 4 * CBANDS; T.bo_s = T.bo_l + SBMAX_l;
    T.amp_by_out = (const double*)(T.s3off_l + amp_at);
    T.fold_marks = T.s3off_l + fold_at; T.wpre = T.fold_marks + 128; T.bvtab = T.wpre + 64;
    T.psy_fold = T.s3off_l + psyfold_at;
    return true;
}
static bool build_tables(TableSet& ts, const void* blob, size_t nbytes, const lhip_config& cfg, void* stream) {
    if (!parse_blob(ts, blob, nbytes, stream) || !check_envelope(ts, cfg) || !derive_index_tables(ts, stream)) return false;
    Tables& T = ts.T;
    // the quantization kernels' LDS tables as one image (q_copy_tabs)
    ts.d_qtabs = rt::dmalloc(sizeof(QuantTabs));
    if (!ts.d_qtabs) { set_err("hipMalloc failed"); return false; }
    if (!rt::dzero(ts.d_qtabs, sizeof(QuantTabs), stream)) return false;          // padding bytes: a defined image
#ifdef LHIP_HOSTSIM
    q_load_tabs(T, *(QuantTabs*)ts.d_qtabs, 0, 1);
#else
    hipLaunchKernelGGL(g_build_qtabs, dim3(1), dim3(256), 0, (hipStream_t)stream, T, (QuantTabs*)ts.d_qtabs);
    { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) { set_err(std::string("g_build_qtabs: ") + hipGetErrorString(e_)); return false; } }
    if (!rt::sync(stream)) return false;
#endif
    T.qtabs_img = ts.d_qtabs;
    ts.pb10 = pow_log2_parts(10.0);
    ts.base_frame_bytes = (int)((double)((T.version + 1) * 72000 * T.brate) / T.out_samplerate);
    // kb_bits assembles a frame in BitsLds (and zeroes one word past its last one): the largest frame of this configuration must fit
    if ((8 * (ts.base_frame_bytes + (T.frac_SpF != 0 ? 1 : 0)) + 31) / 32 + 1 > (int)BITS_LDS_WORDS) {
        set_err("configuration outside the supported envelope (frame larger than the bit-packing buffer)"); return false;
    }
    return true;
}
