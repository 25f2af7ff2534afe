// k_state.h -- kernel bodies that move a stream's carried state and samples: kb_load, the resamplers and kb_prep, kb_count_rejected, kb_save.
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// device-resident per-stream state (what the reference carries from frame to frame)
// ===========================================================================================
// load carried state into the stream's carry slots and build its sample segment (tail + new samples)
// (`part` of `nparts`: the copies are dealt round-robin over the waves of a workgroup that calls this with several -- the one-frame launch)
LHIP_DEV void kb_load(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, int st, int lane, int part = 0, int nparts = 1) {
    const int C = T.channels_out;
    const StreamDesc sd = SD[st];
    const StreamIO io = IO[st];
    const StreamState* S = io.state;
    int job = 0;
#define LOAD_JOB() (nparts == 1 || (job++ % nparts) == part)
    for (int ch = 0; ch < C; ch++) {
        if (T.rs_ratio != 1 && LOAD_JOB()) {                     // resampling: the segment is materialised (PcmSrc::plane)
            float* seg = W.pcm + (int64_t)ch * W.pcm_plane + sd.pcm_off;
            for (int i = lane; i < io.mf_size; i += LHIP_NL) seg[i] = S->pcm_tail[ch][i];
        }
        const int64_t o = (int64_t)sd.gslot0 * C + ch;
        if (LOAD_JOB()) for (int i = lane; i < SB_STRIDE; i += LHIP_NL) W.sb[o * SB_STRIDE + i] = S->sb[ch][i];
        if (LOAD_JOB() && lane == 0) {
            W.loud[o] = S->loud[ch];
            W.tent[o] = S->tent[ch];
            W.blocktype[o] = S->last_bt[ch];
            W.seed[((int64_t)sd.fslot0 * C + ch) * 2 + 0] = S->seed[ch][0];
            W.seed[((int64_t)sd.fslot0 * C + ch) * 2 + 1] = S->seed[ch][1];
        }
    }
    const int Cp = T.psy_channels;
    for (int chn = 0; chn < Cp; chn++) {                         // psy channels: L, R and -- joint stereo -- mid, side
        const int64_t o = (int64_t)sd.gslot0 * Cp + chn;
        if (LOAD_JOB()) for (int i = lane; i < E_STRIDE; i += LHIP_NL) W.E[o * E_STRIDE + i] = S->E[chn][i];
        if (LOAD_JOB()) for (int i = lane; i < EBS_STRIDE; i += LHIP_NL) W.ecb_s[o * EBS_STRIDE + i] = S->ecb_s[chn][i];
        if (LOAD_JOB()) {
            for (int i = lane; i < PK_STRIDE; i += LHIP_NL) W.peaks[o * PK_STRIDE + i] = S->peaks[chn][i];
            if (lane == 0) W.last_attack[o] = S->last_attack[chn];
        }
        if (!T.disable_reservoir && LOAD_JOB()) for (int i = lane; i < EBL_STRIDE; i += LHIP_NL) { W.nb1[o * EBL_STRIDE + i] = S->nb1[chn][i]; W.nb2[o * EBL_STRIDE + i] = S->nb2[chn][i]; }
    }
    if (LOAD_JOB()) {
        if (Cp == 4) for (int i = lane; i < 4; i += LHIP_NL) W.tot_ener[(int64_t)sd.gslot0 * 4 + i] = S->tot_ener[i];
        if (lane == 0) { W.ath_adjust[sd.fslot0] = S->ath_adjust; W.ath_limit[sd.fslot0] = S->ath_limit; }
    }
#undef LOAD_JOB
}

// fill_buffer_resample (Lame.js:1719-1843) for an integer ratio r.  There filter_l = 32, bpc = 1, every clock value
// is an integer, the window offset is 0 and the filter index is always 1, so the reference computes a plain decimating
// FIR that does not depend on how the input was chunked:
//     out[m] = sum_{i=0..32} x[m*r + i - 16] * blackfilt[1][i]        (x[<0] = 0; f64 accumulation in tap order)
// and emits out[m] as soon as m*r + 16 < (samples received so far).  `p0` is the position of tap 0 of this call's
// first output relative to this call's first input sample; positions < 0 are the carried tail of earlier calls.
// (gains and downmix happen in front of fill_buffer, Lame.js:1551-1584: the filter reads mixed samples -- pcm_new_at -- and `old` holds mixed samples)
template <int F32>
LHIP_DEV void kb_resample_elem(const Tables& T, float* dst, const PcmSrc& P, const float* old, int p0, int64_t t) {
    const float* coef = T.rs_blackfilt + T.rs_bpc * RS_TAPS;
    const int64_t p = (int64_t)p0 + t * T.rs_ratio;
    double xvalue = 0.0;
    for (int i = 0; i < RS_TAPS; i++) {
        const int64_t q = p + i;
        float y;
        if (q < 0) y = old[(RS_TAPS - 1) + q];
        else y = pcm_new_at<F32>(P, q);
        xvalue += (double)y * (double)coef[i];
    }
    dst[t] = (float)xvalue;
}

// fill_buffer_resample (Lame.js:1769-1800) for a NON-integer ratio (extension { fractionalResample }: Tables::rs_frac).  There filter_l = 31,
// BLACKSIZE = 32 and filter_l / 2 = 15.5: output k of a call sits at input time k * ratio - itime (itime: the resampler's clock at the start
// of the call -- a function of the call lengths alone, kept by the host), its window is row joff of the 2 * bpc + 1 precomputed ones, and
// tap i reads input trunc(i + j - 15.5): truncation toward zero (the reference's `0 | ...`), so input 0 is read twice where i + j - 15.5 is
// -0.5 and +0.5.  That is why call boundaries show in the bytes and such a stream is a call-sequence stream.  The host only asks for outputs
// whose taps lie inside the call (j + 15.5 < n_in, at most 31 samples back into the carried tail); the clamps keep a wrong record in bounds.
template <int F32>
LHIP_DEV void kb_resample_frac_elem(const Tables& T, float* dst, const PcmSrc& P, const float* old, double itime, int n_in, int64_t k) {
    enum { BLACKSIZE = RS_TAPS - 1 };
    const int bpc = T.rs_bpc;
    const double time0 = (double)k * T.resample_ratio;
    const int j = (int)floor(time0 - itime);
    const double offset = (time0 - itime - (j + .5));
    int joff = (int)floor((offset * 2 * bpc) + bpc + .5);
    joff = joff < 0 ? 0 : (joff > 2 * bpc ? 2 * bpc : joff);
    const float* coef = T.rs_blackfilt + (int64_t)joff * BLACKSIZE;
    double xvalue = 0.0;
    for (int i = 0; i < BLACKSIZE; i++) {
        const int j2 = (int)(i + j - 15.5);
        float y = 0.f;
        if (j2 < 0) { if (j2 >= -BLACKSIZE) y = old[BLACKSIZE + j2]; }
        else if (j2 < n_in) y = pcm_new_at<F32>(P, j2);
        xvalue += (double)y * (double)coef[i];
    }
    dst[k] = (float)xvalue;
}

// Resampling configurations only: the new output-rate samples of every stream, grid-stride over (stream, channel, sample).
// (Without resampling nothing is materialised: the consumers convert the caller's Int16 where they stage it, PcmSrc.)
LHIP_DEV void kb_prep_stream(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, int st, int64_t tid, int64_t nthreads) {
    const int C = T.channels_out;
    const StreamIO io = IO[st];
    const int64_t off = SD[st].pcm_off + io.mf_size;
    for (int ch = 0; ch < C; ch++) {
        float* dst = W.pcm + (int64_t)ch * W.pcm_plane + off;
        const PcmSrc P = pcm_source_new(T, io, ch);
        const float* old = io.state->rs_old[ch];
        if (io.f32) {                                            // the sample type is decided outside the tap loops
            if (T.rs_frac) for (int64_t i = tid; i < io.n_new; i += nthreads) kb_resample_frac_elem<1>(T, dst, P, old, io.rs_itime, io.n_in, i);
            else for (int64_t i = tid; i < io.n_new; i += nthreads) kb_resample_elem<1>(T, dst, P, old, io.rs_p0, i);
        } else {
            if (T.rs_frac) for (int64_t i = tid; i < io.n_new; i += nthreads) kb_resample_frac_elem<0>(T, dst, P, old, io.rs_itime, io.n_in, i);
            else for (int64_t i = tid; i < io.n_new; i += nthreads) kb_resample_elem<0>(T, dst, P, old, io.rs_p0, i);
        }
    }
}
LHIP_DEV void kb_prep(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, int nstreams, int64_t tid, int64_t nthreads) {
    for (int st = 0; st < nstreams; st++) kb_prep_stream(T, W, SD, IO, st, tid, nthreads);
}

// Float32 input by device pointer (lhip_encode_batch_device_pcm): the host cannot see the values, the read sites read a sample outside the
// contract as +0 (pcm_f32_clean) -- this counts them, once per (stream, channel, sample) the caller handed over, for lhip_last_batch_rejected_samples.  A pass of its own
// over the call's input (4.6 KB per two-channel frame), launched for such calls only: the read sites stay free of atomics, and several of them
// read a sample more than once.  C: INPUT channels -- source positions are counted, both source channels of a downmix; limit: Tables::pcm_limit.
LHIP_DEV unsigned long long kb_count_rejected(const StreamIO* IO, int nstreams, int C, float limit, int64_t tid, int64_t nthreads) {
    unsigned long long bad = 0;
    for (int st = 0; st < nstreams; st++) {
        const StreamIO io = IO[st];
        if (!io.f32) continue;
        for (int ch = 0; ch < C; ch++) {
            if (ch && io.src[1] == io.src[0]) continue;          // right == left (or no right plane): the samples exist once, as for the host entries' scan
            const float* src = (const float*)(ch ? io.src[1] : io.src[0]);
            for (int64_t i = tid; i < io.n_in; i += nthreads) { const float v = src[i * io.stride]; bad += !((v < 0 ? -v : v) <= limit); }
        }
    }
    return bad;
}

LHIP_DEV void kb_save(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, int st, int lane, int part = 0, int nparts = 1) {
    const int C = T.channels_out;
    const StreamDesc sd = SD[st];
    const StreamIO io = IO[st];
    StreamState* S = io.state;
    const int F = sd.nframes;
    const int frame = 576 * T.mode_gr;
    const int total = io.mf_size + io.n_new, keep = total - frame * F;
    int job = 0;
#define SAVE_JOB() (nparts == 1 || (job++ % nparts) == part)
    for (int ch = 0; ch < C; ch++) {
        // new tail = segment[frame * F ...): read through the same accessor the kernels use.  In place: a chunk of 64 is read
        // completely before it is written, and later chunks only read positions above everything written so far
        if (SAVE_JOB()) {
            const PcmSrc P = pcm_source(T, W, sd, io, ch);
            for (int base = 0; base < keep; base += LHIP_NL) {
                const int i = base + lane;
                float v = 0.f;
                if (i < keep) v = pcm_at(P, frame * F + i);
                wave_sync();
                if (i < keep) S->pcm_tail[ch][i] = v;
                wave_sync();
            }
        }
        if (F == 0) continue;
        const int64_t o = (int64_t)(sd.gslot0 + T.mode_gr * F) * C + ch;
        if (SAVE_JOB()) for (int i = lane; i < SB_STRIDE; i += LHIP_NL) S->sb[ch][i] = W.sb[o * SB_STRIDE + i];
        if (SAVE_JOB() && lane == 0) {
            S->loud[ch] = W.loud[o];
            S->tent[ch] = W.tent[o];
            S->last_bt[ch] = W.blocktype[o];
            Seed s;                                               // bit reservoir: the frames were quantized in order and left their seeds in W.seed
            if (T.disable_reservoir) s = seed_before(W, sd, C, F, 0, ch);
            else { s.start = W.seed[((int64_t)(sd.fslot0 + F) * C + ch) * 2]; s.step = W.seed[((int64_t)(sd.fslot0 + F) * C + ch) * 2 + 1]; }
            S->seed[ch][0] = s.start; S->seed[ch][1] = s.step;
        }
    }
    if (F > 0) {
        const int Cp = T.psy_channels;
        for (int chn = 0; chn < Cp; chn++) {
            const int64_t o = (int64_t)(sd.gslot0 + T.mode_gr * F) * Cp + chn;
            if (SAVE_JOB()) for (int i = lane; i < E_STRIDE; i += LHIP_NL) S->E[chn][i] = W.E[o * E_STRIDE + i];
            if (SAVE_JOB()) for (int i = lane; i < EBS_STRIDE; i += LHIP_NL) S->ecb_s[chn][i] = W.ecb_s[o * EBS_STRIDE + i];
            if (SAVE_JOB()) {
                for (int i = lane; i < PK_STRIDE; i += LHIP_NL) S->peaks[chn][i] = i < 9 ? W.peaks[o * PK_STRIDE + i] : 0.f;   // 9 peaks; the pad words are never written by anybody (stale workspace bytes must not reach the state record)
                if (lane == 0) S->last_attack[chn] = W.last_attack[o];
            }
            if (!T.disable_reservoir && SAVE_JOB()) for (int i = lane; i < EBL_STRIDE; i += LHIP_NL) { S->nb1[chn][i] = W.nb1[o * EBL_STRIDE + i]; S->nb2[chn][i] = W.nb2[o * EBL_STRIDE + i]; }
        }
        if (SAVE_JOB()) {
            if (Cp == 4) for (int i = lane; i < 4; i += LHIP_NL) S->tot_ener[i] = W.tot_ener[(int64_t)(sd.gslot0 + T.mode_gr * F) * 4 + i];
            if (lane == 0) { S->ath_adjust = W.ath_adjust[sd.fslot0 + F]; S->ath_limit = W.ath_limit[sd.fslot0 + F]; }
        }
    }
    if (T.rs_ratio != 1 && SAVE_JOB()) {
        // the last 32 input samples seen so far (carried tail ++ this call's input), as the scaled floats the filter reads
        for (int ch = 0; ch < C; ch++) {
            const PcmSrc P = pcm_source_new(T, io, ch);
            for (int base = 0; base < RS_TAPS - 1; base += LHIP_NL) {
                const int i = base + lane;
                float v = 0.f;
                if (i < RS_TAPS - 1) {
                    const int64_t q = (int64_t)io.n_in - (RS_TAPS - 1) + i;
                    if (q < 0) v = S->rs_old[ch][(RS_TAPS - 1) + q];
                    else v = io.f32 ? pcm_new_at<1>(P, q) : pcm_new_at<0>(P, q);
                }
                wave_sync();
                if (i < RS_TAPS - 1) S->rs_old[ch][i] = v;
                wave_sync();
            }
        }
    }
#undef SAVE_JOB
}
