// lhip_fracflush.h -- what flush() feeds: the zeros of an ordinary stream (flush_zeros) and the planned flush of a non-integer-ratio stream.
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// gfp.encoder_padding as lame_encode_flush sets it (Lame.js:1393-1412) -- a double where the reference's number can be fractional (16 / r for r = 3);
// -1 for a stream that has nothing to flush
static double flush_end_padding(const lhip_stream* s) {
    if (s->mf_samples_to_encode < 1) return -1;
    const Tables& T = s->ts->T;
    const int frame = 576 * T.mode_gr;
    double samples_to_encode = s->mf_samples_to_encode - 1152;
    if (T.in_samplerate != T.out_samplerate) samples_to_encode += 16. * T.out_samplerate / T.in_samplerate;
    double end_padding = frame - fmod(samples_to_encode, (double)frame);
    if (end_padding < 576) end_padding += frame;
    return end_padding;
}
static size_t flush_zeros(lhip_stream* s) {
    // Lame.js:1381-1443: the flush loop feeds bunches of at most 1152 zeros (fill_buffer takes them one frame at a
    // time) until `frames_left` bunches have each completed at least one frame; the total number of zeros is what
    // the batch path needs, the frames follow from it
    if (s->mf_samples_to_encode < 1) return 0;
    const Tables& T = s->ts->T;
    const int frame = 576 * T.mode_gr, mf_needed = 1024 + frame - 272, r = T.rs_ratio;
    // doubles where the reference's numbers can be fractional (16/r for r = 3)
    double samples_to_encode = s->mf_samples_to_encode - 1152;
    if (T.in_samplerate != T.out_samplerate) samples_to_encode += 16. * T.out_samplerate / T.in_samplerate;
    double end_padding = frame - fmod(samples_to_encode, (double)frame);
    if (end_padding < 576) end_padding += frame;
    double frames_left = (samples_to_encode + end_padding) / frame;
    int mf = s->mf_size;
    int64_t n_in = s->rs_n_in;
    size_t zeros = 0;
    while (frames_left > 0) {
        int64_t bunch = (int64_t)(mf_needed - mf) * r;           // bunch *= in_samplerate; bunch /= out_samplerate (exact: integer ratio)
        if (bunch > 1152) bunch = 1152;
        if (bunch < 1) bunch = 1;
        int emitted = 0;
        if (r == 1) {
            for (int rem = (int)bunch; rem > 0;) {
                const int n = rem < frame ? rem : frame;
                mf += n; rem -= n;
                if (mf >= mf_needed) { emitted++; mf -= frame; }
            }
        } else {
            // the fill loop adds at most one frame of resampled samples per pass and encodes whenever mf_needed is reached
            mf += (int)(rs_outputs(n_in + bunch, r) - rs_outputs(n_in, r));
            n_in += bunch;
            while (mf >= mf_needed) { emitted++; mf -= frame; }
        }
        zeros += (size_t)bunch;
        if (emitted) frames_left--;
    }
    return zeros;
}

// ---- flush of a non-integer-ratio stream (extension { fractionalResample }) ----
// lame_encode_flush (Lame.js:1393-1443) feeds bunches of zeros of (mf_needed - mf_size) * in / out samples -- a fractional length -- until
// frames_left bunches have each completed a frame.  Everything about it that depends on lengths only is mirrored here in f64: per fill pass
// its outputs and num_used (frac_pass), and WHERE the reference's samples turn NaN: a tap or a carried-tail copy at a fractional position
// (after a non-integer num_used) or beyond the end of its persistent input buffer (as long as the largest call so far) reads `undefined`.
// A flush frame is CLEAN while no NaN lies in its input window [0, mf_needed): it is encoded by the kernels like any frame (the pass goes to
// the device with its zeros and its fractional length).  From the first frame that is not, the reference encodes its own NaN samples
// (near-empty frames); NaN never enters a kernel here -- those frames are emitted as silent frames of the reference's length and header.
struct FracStep { double len; int k; bool device, frame, clean; int bytes, padding; };
static bool frac_flush_plan(const lhip_stream* s, std::vector<FracStep>& steps) {
    const Tables& T = s->ts->T;
    const int frame = 576 * T.mode_gr, mf_needed = 1024 + frame - 272, B = RS_TAPS - 1;
    steps.clear();
    if (s->mf_samples_to_encode < 1) return true;
    double samples_to_encode = s->mf_samples_to_encode - 1152;
    samples_to_encode += 16. * T.out_samplerate / T.in_samplerate;
    double end_padding = frame - fmod(samples_to_encode, (double)frame);
    if (end_padding < 576) end_padding += frame;
    double frames_left = (samples_to_encode + end_padding) / frame;
    int mf = s->mf_size, lag = s->slot_lag, guard = 0;
    double itime = s->rs_itime, inbuf_ns = s->rs_inbuf_nsamples;
    int64_t inbuf_len = s->rs_inbuf_len;
    bool old_nan[RS_TAPS - 1] = {false}, alive = true;
    std::vector<char> mf_nan((size_t)mf_needed + 2 * frame + 64, 0);
    auto in_nan = [&](double idx) { return idx != floor(idx) || idx < 0 || idx >= (double)inbuf_len; };      // inbuf[idx] is undefined -> NaN in a Float32Array
    while (frames_left > 0) {
        double bunch = mf_needed - mf;
        bunch *= T.in_samplerate;
        bunch /= T.out_samplerate;
        if (bunch > 1152) bunch = 1152;
        if (bunch < 1) bunch = 1;
        if (inbuf_len == 0 || inbuf_ns < bunch) { inbuf_len = (int64_t)floor(bunch); inbuf_ns = bunch; }       // update_inbuffer_size: new Float32Array(bunch)
        double nsamples = bunch, pos = 0;
        bool emitted = false;
        while (nsamples > 0) {
            if (++guard > 256) { set_err("fractionalResample: the flush does not terminate"); return false; }
            const double len = nsamples;
            const FracPass fp = frac_pass(T, itime, len);
            bool any_nan = false;
            for (int k = 0; k < fp.k; k++) {
                const int j = (int)floor(k * T.resample_ratio - itime);
                bool nan = false;
                for (int i = 0; i < B; i++) {
                    const int j2 = (int)(i + j - 15.5);
                    nan |= j2 < 0 ? (j2 >= -B ? old_nan[B + j2] : true) : in_nan(pos + j2);
                }
                mf_nan[(size_t)mf + k] = nan; any_nan |= nan;
            }
            {   // the carried tail (Lame.js:1816-1840), positions only
                const double nu = fp.num_used;
                bool nn[RS_TAPS - 1];
                if (nu >= B) for (int i = 0; i < B; i++) nn[i] = in_nan(pos + nu + i - B);
                else {
                    const double n_shift = B - nu;
                    int i = 0;
                    for (; i < n_shift; ++i) { const double q = i + nu; nn[i] = (q != floor(q) || q >= B) ? true : old_nan[(int)q]; }
                    for (int jj = 0; i < B; ++i, ++jj) nn[i] = in_nan(pos + jj);
                }
                memcpy(old_nan, nn, sizeof nn);
                itime += nu - fp.k * T.resample_ratio;
                nsamples -= nu; pos += nu;
            }
            FracStep st{len, fp.k, false, false, false, 0, 0};
            const bool first = len == bunch;                                      // the pass starts at the bunch's first sample (a later one starts at a fractional position)
            mf += fp.k;
            st.frame = mf >= mf_needed;
            if (st.frame) { st.clean = true; for (int p = 0; p < mf_needed; p++) if (mf_nan[p]) { st.clean = false; break; } }
            st.device = alive && first && (st.frame ? st.clean : !any_nan);
            if (st.frame && !st.device) st.clean = false;                        // (emitted as a silent frame)
            if (!st.device || any_nan || fp.num_used != floor(fp.num_used)) alive = false;
            if (st.frame) {
                st.padding = host_next_padding(T, &lag);
                st.bytes = s->ts->base_frame_bytes + st.padding;
                mf -= frame;
                memmove(mf_nan.data(), mf_nan.data() + frame, mf_nan.size() - frame);
                emitted = true;
            }
            steps.push_back(st);
        }
        frames_left -= emitted ? 1 : 0;
    }
    return true;
}
static int64_t frac_flush(lhip_stream* s, uint8_t* out, size_t out_cap) {
    const Tables& T = s->ts->T;
    std::vector<FracStep> steps;
    if (s->rs_flushed) return 0;
    if (!frac_flush_plan(s, steps)) return LHIP_ERR_INTERNAL;
    size_t total = 0;
    for (const FracStep& st : steps) total += (size_t)st.bytes;
    if (total > out_cap) { set_err("output buffer too small"); return LHIP_ERR_BUFFER_TOO_SMALL; }      // nothing was consumed
    std::vector<int16_t> zeros(1152 + 8, 0);
    int64_t w = 0;
    for (const FracStep& st : steps) {
        if (st.device) {
            std::vector<Job> jobs(1);
            jobs[0] = Job{s, zeros.data(), zeros.data(), (size_t)ceil(st.len), out + w, out_cap - (size_t)w, 0, 0, 0, 0};
            jobs[0].rs_len = st.len;
            if (!run_batch(s->ctx, jobs, false, true)) return jobs[0].written < 0 ? jobs[0].written : LHIP_ERR_INTERNAL;
            if (jobs[0].written != st.bytes) { set_err("fractionalResample: the flush plan and the launch disagree"); return LHIP_ERR_INTERNAL; }
            w += jobs[0].written;
        } else if (st.frame) {
            // a silent frame: the header the reference writes (BitStream.js:259-281; mode_ext 0), side information and main data zero
            uint8_t* f = out + w;
            memset(f, 0, (size_t)st.bytes);
            const int sync = T.out_samplerate < 16000 ? 0xffe : 0xfff;
            f[0] = (uint8_t)(sync >> 4);
            f[1] = (uint8_t)(((sync & 15) << 4) | (T.version << 3) | (1 << 1) | (T.error_protection ? 0 : 1));
            f[2] = (uint8_t)((T.bitrate_index << 4) | (T.samplerate_index << 2) | (st.padding << 1) | T.extension);
            f[3] = (uint8_t)((T.mode << 6) | (T.copyright << 3) | (T.original << 2) | T.emphasis);
            int lag = s->slot_lag; (void)host_next_padding(T, &lag); s->slot_lag = lag;
            s->frame_num++;
            w += st.bytes;
        }
    }
    s->mf_samples_to_encode = 0;
    s->rs_flushed = true;
    return w;
}
