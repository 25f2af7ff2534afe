/*
 * Host-side parameter resolution and table construction for the MI355X encode path.
 *
 * Given the three public knobs of the drop-in API -- (channels, samplerate, kbps) --
 * this module resolves every scalar the hot path needs and builds every lookup
 * table with the host's own Math.* (V8), so the numbers are bit-identical to what
 * the reference computes at `new Mp3Encoder(...)` time.  The result is packed into
 * one "LHTB" blob (see packBlob) that the C-ABI library uploads to HBM once.
 *
 * Behaviour restated (not copied) from the reference's one-time init:
 *   index.js:100-111        fixed Mp3Encoder configuration
 *   Lame.js:747-1371        lame_init_params (CBR, vbr_off branch only)
 *   Lame.js:470-558         polyphase high-pass and low-pass amplitudes (amp_filter)
 *   Lame.js:560-690         quality map (quality 3; 7 with { quality: 7 })
 *   Presets.js:226-358      ABR preset row applied for CBR
 *   QuantizePVT.js:247-414  ATH per sfb, pow43/adj43/ipow20/pow20, long/shortfact
 *   Takehiro.js:1141-1172   bv_scf region split table
 *   PsyModel.js:2249-2822   partitions, spreading functions, ATH per partition, eql_w
 *   FFT.js:226-242          analysis windows; FFT.js:31-115 twiddle recurrence
 *
 * Supported envelope (everything else throws): CBR, every MPEG-1 / MPEG-2 / MPEG-2.5 sample rate
 * 1 or 2 channels, with out_samplerate == in_samplerate or an integer multiple below it (resampling by a non-integer
 * ratio makes the reference feed itself NaN samples; refused unless { fractionalResample: true } asks for the call-sequence-exact
 * extension, see resolveParams).
 */
'use strict';

const C = require('./constants.json');

const SBMAX_l = 22, SBMAX_s = 13, SBPSY_l = 21, SBPSY_s = 12, PSFB21 = 6, PSFB12 = 6;
const CBANDS = 64, BLKSIZE = 1024, BLKSIZE_s = 256, HBLKSIZE = 513;
const IXMAX_VAL = 8206, PRECALC_SIZE = IXMAX_VAL + 2, Q_MAX = 256 + 1, Q_MAX2 = 116;
const FLOAT_MAX = 3.4028235e+38;
const MODE_STEREO = 0, MODE_JOINT_STEREO = 1, MODE_MONO = 3;

function f32(n) { return new Float32Array(n); }
function i32(n) { return new Int32Array(n); }

/* ------------------------------------------------------------------ */
/* parameter resolution                                                */
/* ------------------------------------------------------------------ */

function nearestBitrateFullIndex(bitrate) {
    const t = C.full_bitrate_table;
    let upper = 16, lower = 16, upper_k = t[16], lower_k = t[16];
    for (let b = 0; b < 16; b++) {
        if (Math.max(bitrate, t[b + 1]) != bitrate) {
            upper_k = t[b + 1]; upper = b + 1; lower_k = t[b]; lower = b;
            break;
        }
    }
    return (upper_k - bitrate) > (bitrate - lower_k) ? lower : upper;
}

function suggestedSampleFreq(lowpassfreq, in_rate) {
    /* same decision table as the reference's out_samplerate chooser, Lame.js:285-364 */
    const grid = [48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000];
    let s = 44100;
    for (const g of grid) { if (in_rate >= g) { s = g; break; } }
    if (lowpassfreq == -1) return s;
    const cuts = [[15960, 44100], [15250, 32000], [11220, 24000], [9970, 22050],
        [7230, 16000], [5420, 12000], [4510, 11025], [3970, 8000]];
    for (const [lim, fs] of cuts) if (lowpassfreq <= lim) s = fs;
    if (in_rate < s) {
        const up = [[44100, 48000], [32000, 44100], [24000, 32000], [22050, 24000],
            [16000, 22050], [12000, 16000], [11025, 12000], [8000, 11025]];
        for (const [lim, fs] of up) if (in_rate > lim) return fs;
        return 8000;
    }
    return s;
}

function resolveParams(channels, samplerate, kbps, opts) {
    const p = {};
    p.channels_in = channels;
    p.mode = (channels == 1) ? MODE_MONO : MODE_STEREO;      /* index.js:105, Lame.js:759-761 */
    /* extension (SURVEY.md 8f #3): the reference's joint-stereo path, which its Mp3Encoder never selects (index.js:105) */
    if (opts && opts.jointStereo && channels == 2) p.mode = MODE_JOINT_STEREO;
    /* extension (SURVEY.md 8f #4): the bit reservoir, which index.js:108 switches off */
    p.disable_reservoir = (opts && opts.reservoir) ? 0 : 1;
    /* extension { downmix }: two channels in, MPEGMode.MONO out -- everything below resolves as the reference does for that mode
     * (channels_out = 1, mono side info, presets and lowpass); the mix itself is Lame.js:1579-1584 */
    if (opts && opts.downmix) {
        if (channels != 2) throw new TypeError('lamejs_amd: { downmix } needs two input channels');
        if (opts.jointStereo) throw new TypeError('lamejs_amd: { downmix } and { jointStereo } cannot be combined');
        p.mode = MODE_MONO;
    }
    p.channels_out = (p.mode == MODE_MONO) ? 1 : 2;
    p.in_samplerate = samplerate;
    let brate = kbps;

    /* extension { outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth }: gfp.out_samplerate, lowpassfreq, lowpasswidth, highpassfreq and
     * highpasswidth of the reference's core (LAME's --resample, --lowpass, --lowpass-width, --highpass, --highpass-width), which its wrapper leaves at
     * lame_init's values (0, 0, -1, 0, -1: Lame.js:147-150).  Whole numbers of Hz; lowpass -1 switches the filter off (LAME's convention) */
    const fopt = (k, min, what, minusOne) => {
        if (!opts || opts[k] === undefined || opts[k] === null) return null;
        const v = opts[k];
        if (typeof v != 'number' || !Number.isInteger(v) || !(v >= min || (minusOne && v === -1)))
            throw new RangeError('lamejs_amd: { ' + k + ' } must be ' + what);
        return v;
    };
    const userOut = fopt('outSampleRate', 1, 'one of the MPEG sample rates 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000');
    const userLow = fopt('lowpass', 1, 'a whole number of Hz >= 1, or -1 (no lowpass)', true);
    const lowpasswidth = fopt('lowpassWidth', 0, 'a whole number of Hz >= 0');
    const highpassfreq = fopt('highpass', 1, 'a whole number of Hz >= 1');
    const highpasswidth = fopt('highpassWidth', 0, 'a whole number of Hz >= 0');
    if (highpasswidth !== null && highpassfreq === null)
        throw new RangeError('lamejs_amd: { highpassWidth } needs { highpass } (the reference ignores a width without a frequency)');
    if (userOut !== null) {
        if (![48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000].includes(userOut))
            throw new RangeError('lamejs_amd: { outSampleRate } must be one of the MPEG sample rates 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000');
        if (userOut > samplerate) throw new RangeError('lamejs_amd: { outSampleRate: ' + userOut + ' } is above the input rate ' + samplerate + ' (upsampling is not supported)');
        if (samplerate % userOut != 0)
            throw new RangeError('lamejs_amd: { outSampleRate: ' + userOut + ' } is not the input rate ' + samplerate + ' divided by a whole number (the ratio ' + samplerate / userOut +
                ' is not supported, with or without { fractionalResample })');
    }
    p.filter_options = (userOut !== null || userLow !== null || lowpasswidth !== null || highpassfreq !== null) ? 1 : 0;

    /* lowpass from bitrate (Lame.js:838-885), unless the caller set one */
    let lowpassfreq;
    if (userLow === null) {
        let lowpass = C.lowpass_freq_map[nearestBitrateFullIndex(brate)][1];
        if (p.mode == MODE_MONO) lowpass *= 1.5;
        lowpassfreq = lowpass | 0;
    } else lowpassfreq = userLow;
    /* Lame.js:887-896: the output rate follows from the lowpass only where the caller set none */
    let out_samplerate = userOut;
    if (out_samplerate === null) {
        if (2 * lowpassfreq > samplerate) lowpassfreq = samplerate / 2;
        out_samplerate = suggestedSampleFreq(lowpassfreq | 0, samplerate);
    }
    lowpassfreq = Math.min(20500, lowpassfreq);
    lowpassfreq = Math.min(out_samplerate / 2, lowpassfreq);
    p.out_samplerate = out_samplerate;
    p.lowpassfreq = lowpassfreq;
    if (highpassfreq !== null) {
        /* Lame.js:508-515: below this the reference disables the highpass with a warning -- through System.err, which it does not define: it throws */
        const top = highpassfreq + Math.max(highpasswidth === null ? -1 : highpasswidth, 0);
        if (2. * top / out_samplerate < .9 * (.75 / 31.0)) {
            let min = 1;
            while (2. * min / out_samplerate < .9 * (.75 / 31.0)) min++;
            throw new RangeError('lamejs_amd: { highpass: ' + highpassfreq + ' } is too low for a stream of ' + out_samplerate + ' Hz: highpass + highpassWidth must be at least ' + min + ' Hz');
        }
        /* a highpass at or above the lowpass leaves no band: the reference would encode silence */
        if (lowpassfreq > 0 && !(top < lowpassfreq))
            throw new RangeError('lamejs_amd: { highpass } + { highpassWidth } = ' + top + ' Hz must lie below the lowpass, ' + lowpassfreq + ' Hz');
    }

    /* resampler set-up (Lame.js:943, 1719-1763).  By default only integer ratios are in the envelope: for any other ratio the
     * reference's filter_l / 2 is 15.5, and once a fill pass delivers a whole frame its buffer positions become fractional, typed-array
     * reads return undefined and the encoder is fed NaN samples (at the latest in flush()).
     * extension { fractionalResample: true }: such a configuration is accepted as a CALL-SEQUENCE stream -- every encodeBuffer() call the
     * reference consumes whole (always true up to fractionalCallLimit() samples) gives the reference's bytes for the same sequence of
     * call lengths; longer calls are refused (DESIGN_EXTENSIONS.md 5). */
    p.resample_ratio = samplerate / out_samplerate;
    p.rs_filter_l = 0; p.rs_bpc = 0; p.rs_blackfilt = f32(1);
    if (p.resample_ratio < .9999 || p.resample_ratio > 1.0001) {
        const ratio = p.resample_ratio;
        const intratio = (Math.abs(ratio - Math.floor(.5 + ratio)) < .0001) ? 1 : 0;
        if (!intratio && !(opts && opts.fractionalResample))
            throw new Error('lamejs_amd: (' + channels + ',' + samplerate + ',' + kbps + ') would resample to ' + out_samplerate +
                ' Hz by the non-integer ratio ' + ratio + '; the reference feeds itself NaN samples there (fractional buffer positions), not supported' +
                ' without the option { fractionalResample: true } (call-sequence-exact, calls of limited length)');
        if (!intratio && opts.reservoir)
            throw new Error('lamejs_amd: { fractionalResample } and { reservoir } cannot be combined');
        if (!intratio && p.filter_options)
            throw new Error('lamejs_amd: { fractionalResample } cannot be combined with { lowpass, lowpassWidth, highpass, highpassWidth } where the stream resamples by a non-integer ratio' +
                ' ({ outSampleRate } gives such a configuration an integer ratio)');
        const gcd = (i, j) => (j != 0 ? gcd(j, i % j) : i);
        let bpc = out_samplerate / gcd(out_samplerate, samplerate);
        if (bpc > 320) bpc = 320;                                            /* LameInternalFlags.BPC */
        let fcn = 1.00 / ratio;
        if (fcn > 1.00) fcn = 1.00;
        let filter_l = 31;
        if (0 == filter_l % 2) --filter_l;
        filter_l += intratio;
        const BLACKSIZE = filter_l + 1;
        const blackman = function (x, fcn, l) {                               /* Lame.js:1698-1717 */
            const wcn = (Math.PI * fcn);
            x /= l;
            if (x < 0) x = 0;
            if (x > 1) x = 1;
            const x2 = x - .5;
            const bkwn = 0.42 - 0.5 * Math.cos(2 * x * Math.PI) + 0.08 * Math.cos(4 * x * Math.PI);
            if (Math.abs(x2) < 1e-9) return (wcn / Math.PI);
            else return (bkwn * Math.sin(l * wcn * x2) / (Math.PI * l * x2));
        };
        const bf = f32((2 * bpc + 1) * BLACKSIZE);
        for (let j = 0; j <= 2 * bpc; j++) {
            let sum = 0.;
            const offset = (j - bpc) / (2. * bpc);
            const row = bf.subarray(j * BLACKSIZE, (j + 1) * BLACKSIZE);
            for (let i = 0; i <= filter_l; i++) sum += row[i] = blackman(i - offset, fcn, filter_l);   /* adds the unrounded f64 */
            for (let i = 0; i <= filter_l; i++) row[i] /= sum;
        }
        p.rs_filter_l = filter_l; p.rs_bpc = bpc; p.rs_blackfilt = bf;
    }
    /* SmpFrqIndex (Lame.js:369-403): MPEG-1 for 32/44.1/48 kHz, "version 0" (LSF) for MPEG-2 and MPEG-2.5 rates */
    const SFI = { 44100: [1, 0], 48000: [1, 1], 32000: [1, 2], 22050: [0, 0], 24000: [0, 1], 16000: [0, 2],
        11025: [0, 0], 12000: [0, 1], 8000: [0, 2] };
    if (!SFI[out_samplerate])
        throw new Error('lamejs_amd: unsupported sample rate ' + out_samplerate);
    p.version = SFI[out_samplerate][0];
    const sr_idx = SFI[out_samplerate][1];
    p.samplerate_index = sr_idx;
    p.mode_gr = out_samplerate <= 24000 ? 1 : 2;            /* Lame.js:936 */
    p.framesize = 576 * p.mode_gr;

    /* nearest legal bitrate + index (Lame.js:408-444); MPEG-2.5 rates use their own bitrate row */
    {
        const bt = C.bitrate_table[out_samplerate < 16000 ? 2 : p.version];
        let best = bt[1];
        for (let i = 2; i <= 14; i++)
            if (bt[i] > 0 && Math.abs(bt[i] - brate) < Math.abs(best - brate)) best = bt[i];
        brate = best;
        p.bitrate_index = bt.indexOf(brate);
    }
    p.brate = brate;

    /* polyphase highpass and lowpass: amp_filter (Lame.js:1004-1040, 470-558) */
    let highpass1 = 0, highpass2 = 0, lowpass1 = 0, lowpass2 = 0;
    if (highpassfreq !== null) {
        highpass1 = 2. * highpassfreq;
        highpass2 = (highpasswidth !== null) ? 2. * (highpassfreq + highpasswidth) : (1 + 0.00) * 2. * highpassfreq;
        highpass1 /= out_samplerate; highpass2 /= out_samplerate;
    }
    if (lowpassfreq > 0) {
        lowpass2 = 2. * lowpassfreq;
        if (lowpasswidth !== null) {
            lowpass1 = 2. * (lowpassfreq - lowpasswidth);
            if (lowpass1 < 0) lowpass1 = 0;
        } else lowpass1 = (1 - 0.00) * 2. * lowpassfreq;
        lowpass1 /= out_samplerate; lowpass2 /= out_samplerate;
    }
    {
        let lowpass_band = 32, minband = 999, highpass_band = -1, maxband = -1;
        if (lowpass1 > 0) {
            for (let band = 0; band <= 31; band++) {
                const freq = band / 31.0;
                if (freq >= lowpass2) lowpass_band = Math.min(lowpass_band, band);
                if (lowpass1 < freq && freq < lowpass2) minband = Math.min(minband, band);
            }
            lowpass1 = ((minband == 999 ? lowpass_band : minband) - .75) / 31.0;
            lowpass2 = lowpass_band / 31.0;
        }
        if (highpass2 > 0) {             /* (never below .9 * .75 / 31 here: refused above) */
            for (let band = 0; band <= 31; band++) {
                const freq = band / 31.0;
                if (freq <= highpass1) highpass_band = Math.max(highpass_band, band);
                if (highpass1 < freq && freq < highpass2) maxband = Math.max(maxband, band);
            }
            highpass1 = highpass_band / 31.0;
            highpass2 = ((maxband == -1 ? highpass_band : maxband) + .75) / 31.0;
        }
        const filter_coef = (x) => (x > 1.0 ? 0.0 : (x <= 0.0 ? 1.0 : Math.cos(Math.PI / 2 * x)));      /* Lame.js:239-246 */
        p.amp_filter = f32(32);
        for (let band = 0; band < 32; band++) {
            const freq = band / 31.0;
            let fc1 = 1.0, fc2 = 1.0;
            if (highpass2 > highpass1) fc1 = filter_coef((highpass2 - freq) / (highpass2 - highpass1 + 1e-20));
            if (lowpass2 > lowpass1) fc2 = filter_coef((freq - lowpass1) / (lowpass2 - lowpass1 + 1e-20));
            p.amp_filter[band] = (fc1 * fc2);
        }
    }

    /* scalefactor band edges (Lame.js:1079-1101); note the fractional pseudo-band
     * starts truncated by the Int32 store -- that truncation is the reference's behaviour */
    {
        const j = sr_idx + 3 * p.version + 6 * (out_samplerate < 16000 ? 1 : 0);
        p.sfb_l = i32(SBMAX_l + 1); p.sfb_s = i32(SBMAX_s + 1);
        p.psfb21 = i32(PSFB21 + 1); p.psfb12 = i32(PSFB12 + 1);
        for (let i = 0; i < SBMAX_l + 1; i++) p.sfb_l[i] = C.sfBandIndex[j].l[i];
        for (let i = 0; i < PSFB21 + 1; i++) {
            const size = (p.sfb_l[22] - p.sfb_l[21]) / PSFB21;
            p.psfb21[i] = p.sfb_l[21] + i * size;
        }
        p.psfb21[PSFB21] = 576;
        for (let i = 0; i < SBMAX_s + 1; i++) p.sfb_s[i] = C.sfBandIndex[j].s[i];
        for (let i = 0; i < PSFB12 + 1; i++) {
            const size = (p.sfb_s[13] - p.sfb_s[12]) / PSFB12;
            p.psfb12[i] = p.sfb_s[12] + i * size;
        }
        p.psfb12[PSFB12] = 192;
    }
    /* Lame.js:1103-1110 */
    if (p.version == 1) p.sideinfo_len = (p.channels_out == 1) ? 4 + 17 : 4 + 32;
    else p.sideinfo_len = (p.channels_out == 1) ? 4 + 9 : 4 + 17;
    /* extension { protect, copyright, original, privateBit, emphasis }: gfp.error_protection (LAME's -p) and the header's flag bits
     * (BitStream.js:273-285), which the reference's wrapper leaves at lame_init's values.  A protected frame carries a CRC-16 behind the header:
     * two more bytes of side information (Lame.js:1109-1110), so 16 bits less for every frame's main data.  emphasis 2 is reserved. */
    {
        const given = (k) => !!opts && opts[k] !== undefined && opts[k] !== null;
        const flag = (k, dflt) => {
            if (!given(k)) return dflt;
            const v = opts[k];
            if (v !== true && v !== false && v !== 0 && v !== 1) throw new RangeError('lamejs_amd: { ' + k + ' } must be true or false');
            return v ? 1 : 0;
        };
        p.error_protection = flag('protect', 0);
        p.copyright = flag('copyright', 0);
        p.original = flag('original', 1);                    /* lame_init_old: original = 1 */
        p.extension = flag('privateBit', 0);
        p.emphasis = 0;
        if (given('emphasis')) {
            if (opts.emphasis !== 0 && opts.emphasis !== 1 && opts.emphasis !== 3) throw new RangeError('lamejs_amd: { emphasis } must be 0 (none), 1 (50/15 us) or 3 (CCITT J.17); 2 is reserved');
            p.emphasis = opts.emphasis;
        }
        if (p.error_protection) {
            if (p.rs_filter_l == 31) throw new Error('lamejs_amd: { protect } and { fractionalResample } cannot be combined for (' + channels + ',' + samplerate + ',' + kbps + ')');
            p.sideinfo_len += 2;
        }
        /* extension { infoTag }: the stream starts with room for the Info/LAME tag frame and the library keeps the totals the tag reports (frames, bytes,
         * seek table, music CRC, delay and padding); the frame itself is written by the host once the stream has been flushed.  The flush of a
         * non-integer-ratio stream is partly host stand-ins and its padding fractional: lhip_create refuses the tag there (-3), as it refuses a
         * configuration whose frames are too small to hold it */
        p.info_tag = flag('infoTag', 0);
        /* extension { replayGain }: the stream analyses the samples its encoder consumes (the reference core's gfc.findReplayGain, Lame.js:1609-1613) on the
         * device; lhip_replay_gain reports the track gain and, with { infoTag }, the tag's radio field carries it.  lhip_create refuses it (-3) where the stream
         * resamples by a non-integer ratio */
        p.replay_gain = flag('replayGain', 0);
    }

    /* CBR: ABR preset row for this bitrate (Lame.js:1202-1230, Presets.js:270-357) */
    const row = C.abr_switch_map[nearestBitrateFullIndex(brate)];
    /* kbps quant q_s safejoint nsmsfix st_lrm st_s ns-bass scale msk ath_lwr ath_curve interch sfscale */
    let exp_nspsytune = 0;
    if (row[3] > 0) exp_nspsytune |= 2;
    p.noise_shaping = (row[13] > 0) ? 2 : 0;
    if (Math.abs(row[7]) > 0) throw new Error('ns-bass presets not supported');
    p.quant_comp = row[1];
    p.quant_comp_short = row[2];
    p.attackthre = row[5];
    p.attackthre_s = row[6];
    p.scale = row[8];
    /* extension { scale, scaleLeft, scaleRight }: gfp.scale / scale_left / scale_right (Lame.js:1551-1576).  The user's scale replaces the
     * preset's, which is written only while gfp.scale is still -1 (Presets.js:313-316); a gain is in force when the reference's tolerant
     * NEQ says so (BitStream.js:22-30), not `!=` */
    {
        const given = (k) => !!opts && opts[k] !== undefined && opts[k] !== null;
        const num = (k) => { const v = opts[k]; if (typeof v != 'number') throw new TypeError('lamejs_amd: { ' + k + ' } must be a number'); return v; };
        p.input_options = given('downmix') && opts.downmix || given('scale') || given('scaleLeft') || given('scaleRight') ? 1 : 0;
        if (given('scale')) p.scale = num('scale');
        p.scale_left = given('scaleLeft') ? num('scaleLeft') : 0.;          /* LameGlobalFlags.js:34, 38 */
        p.scale_right = given('scaleRight') ? num('scaleRight') : 0.;
        const EQ = (a, b) => (Math.abs(a) > Math.abs(b)) ? (Math.abs(a - b) <= Math.abs(a) * 1e-6) : (Math.abs(a - b) <= Math.abs(b) * 1e-6);
        const inForce = (g) => (!EQ(g, 0) && !EQ(g, 1.0)) ? 1 : 0;
        p.do_scale = inForce(p.scale); p.do_scale_left = inForce(p.scale_left); p.do_scale_right = inForce(p.scale_right);
    }
    const maskingadjust = row[9];
    const maskingadjust_short = (row[9] > 0) ? row[9] * .9 : row[9] * 1.1;
    p.ATHlower = -row[10] / 10.;
    p.ATHcurve = row[11];
    p.interChRatio = row[12];
    /* Presets.js:288-292 (nsmsfix); Lame.js:1322: < 0 -> 0; PsyModel.js:2738-2744: 0 -> NS_MSFIX (3.5), or 1.0 with safejoint */
    p.msfix = row[4];
    if (p.msfix < 0) p.msfix = 0;
    if (!(Math.abs(p.msfix) > 0.0)) p.msfix = ((exp_nspsytune & 2) != 0) ? 1.0 : 3.5;
    p.mask_adjust = maskingadjust;
    p.mask_adjust_short = maskingadjust_short;
    /* CBRNewIterationLoop.js:56-65: masking_lower = 10^(0.1 * mask_adjust[_short]) */
    p.masking_lower_long = Math.pow(10.0, p.mask_adjust * 0.1);
    p.masking_lower_short = Math.pow(10.0, p.mask_adjust_short * 0.1);

    /* quality 3 (Lame.js:626-636) */
    p.psymodel = 1;
    if (p.noise_shaping == 0) p.noise_shaping = 1;
    p.noise_shaping_amp = 1;
    p.noise_shaping_stop = 1;
    p.subblock_gain = 1;
    p.use_best_huffman = 1;
    p.full_outer_loop = 0;
    p.substep_shaping = 0;
    p.sfb21_extra = 0;
    /* extension { quality }: LAME's -f, quality 7 of the reference's encoder core (its wrapper always asks for 3) -- the psychoacoustic model still
     * decides block switching and mid/side, the quantization is the bin search alone: no noise shaping (even where the preset row asked for
     * type 2), no amplification, no Huffman region search; subblock_gain stays at lame_init_params' -1 (Lame.js:145, 577-588).  8 is resolved
     * to 7 as lame_init_qval does (Lame.js:574-576).  The other levels differ in more than switches and are not in the envelope. */
    p.quality = 3;
    if (opts && opts.quality !== undefined && opts.quality !== null) {
        if (opts.quality !== 3 && opts.quality !== 7 && opts.quality !== 8) throw new RangeError('lamejs_amd: { quality } must be 3, 7 or 8 (8 is encoded as 7)');
        p.quality = opts.quality == 8 ? 7 : opts.quality;
    }
    if (p.quality == 7) {
        p.psymodel = 1;
        p.noise_shaping = 0;
        p.noise_shaping_amp = 0;
        p.noise_shaping_stop = 0;
        p.subblock_gain = -1;
        p.use_best_huffman = 0;
        p.full_outer_loop = 0;
    }

    p.ATH_useAdjust = 3;
    p.ATH_aaSensitivityP = Math.pow(10.0, 0.0 / -10.0);
    /* short_block_allowed -> coupled for (joint) stereo (Lame.js:1302-1317) */
    p.short_blocks_coupled = (p.mode == MODE_STEREO || p.mode == MODE_JOINT_STEREO) ? 1 : 0;
    p.exp_nspsytune = exp_nspsytune | 1;
    p.ATHtype = 4;
    p.athaa_loudapprox = 2;
    if (p.interChRatio < 0) p.interChRatio = 0;
    p.useTemporal = 1;
    p.frac_SpF = (((p.version + 1) * 72000 * brate) % out_samplerate) | 0;

    return p;
}

/* ------------------------------------------------------------------ */
/* ATH                                                                 */
/* ------------------------------------------------------------------ */

function ATHformula_GB(f, value) {
    if (f < -.3) f = 3410;
    f /= 1000;
    f = Math.max(0.1, f);
    return 3.640 * Math.pow(f, -0.8) - 6.800 * Math.exp(-0.6 * Math.pow(f - 3.4, 2.0))
        + 6.000 * Math.exp(-0.15 * Math.pow(f - 8.7, 2.0))
        + (0.6 + 0.04 * value) * 0.001 * Math.pow(f, 4.0);
}

function buildTables(p) {
    const T = {};
    const sfreq0 = p.out_samplerate;
    const ATHformula = (f) => ATHformula_GB(f, p.ATHcurve);     /* ATHtype 4 */
    const ATHmdct = (f) => {
        let ath = ATHformula(f);
        ath -= 100;                                             /* NSATHSCALE */
        return Math.pow(10.0, ath / 10.0 + p.ATHlower);
    };

    /* --- ATH per scalefactor band (QuantizePVT.js:247-328) --- */
    T.ATH_l = f32(SBMAX_l); T.ATH_s = f32(SBMAX_s); T.ATH_psfb21 = f32(PSFB21); T.ATH_psfb12 = f32(PSFB12);
    const bandMin = (dst, k, start, end, div) => {
        dst[k] = FLOAT_MAX;
        for (let i = start; i < end; i++) dst[k] = Math.min(dst[k], ATHmdct(i * sfreq0 / div));
    };
    for (let sfb = 0; sfb < SBMAX_l; sfb++) bandMin(T.ATH_l, sfb, p.sfb_l[sfb], p.sfb_l[sfb + 1], 2 * 576);
    for (let sfb = 0; sfb < PSFB21; sfb++) bandMin(T.ATH_psfb21, sfb, p.psfb21[sfb], p.psfb21[sfb + 1], 2 * 576);
    for (let sfb = 0; sfb < SBMAX_s; sfb++) {
        bandMin(T.ATH_s, sfb, p.sfb_s[sfb], p.sfb_s[sfb + 1], 2 * 192);
        T.ATH_s[sfb] *= (p.sfb_s[sfb + 1] - p.sfb_s[sfb]);
    }
    for (let sfb = 0; sfb < PSFB12; sfb++) {
        bandMin(T.ATH_psfb12, sfb, p.psfb12[sfb], p.psfb12[sfb + 1], 2 * 192);
        T.ATH_psfb12[sfb] *= (p.sfb_s[13] - p.sfb_s[12]);
    }
    T.ATH_floor = 10. * Math.log10(ATHmdct(-1.));

    /* --- quantizer power tables (QuantizePVT.js:343-358) --- */
    T.pow43 = f32(PRECALC_SIZE); T.adj43 = f32(PRECALC_SIZE);
    T.ipow20 = f32(Q_MAX); T.pow20 = f32(Q_MAX + Q_MAX2 + 1);
    T.pow43[0] = 0.0;
    for (let i = 1; i < PRECALC_SIZE; i++) T.pow43[i] = Math.pow(i, 4.0 / 3.0);
    {
        let i;
        for (i = 0; i < PRECALC_SIZE - 1; i++)
            T.adj43[i] = ((i + 1) - Math.pow(0.5 * (T.pow43[i] + T.pow43[i + 1]), 0.75));
        T.adj43[i] = 0.5;
    }
    for (let i = 0; i < Q_MAX; i++) T.ipow20[i] = Math.pow(2.0, (i - 210) * -0.1875);
    for (let i = 0; i <= Q_MAX + Q_MAX2; i++) T.pow20[i] = Math.pow(2.0, (i - 210 - Q_MAX2) * 0.25);

    /* --- region split table (Takehiro.js:1141-1172) --- */
    T.bv_scf = i32(576);
    for (let i = 2; i <= 576; i += 2) {
        let scfb_anz = 0, bv;
        while (p.sfb_l[++scfb_anz] < i);
        bv = C.subdv_table[scfb_anz][0];
        while (p.sfb_l[bv + 1] > i) bv--;
        if (bv < 0) bv = C.subdv_table[scfb_anz][0];
        T.bv_scf[i - 2] = bv;
        bv = C.subdv_table[scfb_anz][1];
        while (p.sfb_l[bv + T.bv_scf[i - 2] + 2] > i) bv--;
        if (bv < 0) bv = C.subdv_table[scfb_anz][1];
        T.bv_scf[i - 1] = bv;
    }

    /* --- long/shortfact (QuantizePVT.js:362-409) --- */
    {
        const dec = (sh) => { let i = (p.exp_nspsytune >> sh) & 63; if (i >= 32) i -= 64; return i; };
        const bass = Math.pow(10, dec(2) / 4.0 / 10.0);
        const alto = Math.pow(10, dec(8) / 4.0 / 10.0);
        const treble = Math.pow(10, dec(14) / 4.0 / 10.0);
        const sfb21 = treble * Math.pow(10, dec(20) / 4.0 / 10.0);
        T.longfact = f32(SBMAX_l); T.shortfact = f32(SBMAX_s);
        for (let i = 0; i < SBMAX_l; i++) T.longfact[i] = i <= 6 ? bass : i <= 13 ? alto : i <= 20 ? treble : sfb21;
        for (let i = 0; i < SBMAX_s; i++) T.shortfact[i] = i <= 5 ? bass : i <= 10 ? alto : i <= 11 ? treble : sfb21;
    }

    /* --- psychoacoustic partitions (PsyModel.js:2363-2460, 2537-2760) --- */
    const LN_TO_LOG10 = 0.2302585093, LOG10 = 2.30258509299404568402, DELBARK = .34;
    const freq2bark = (freq) => {
        if (freq < 0) freq = 0;
        freq = freq * 0.001;
        return 13.0 * Math.atan(.76 * freq) + 3.5 * Math.atan(freq * freq / (7.5 * 7.5));
    };
    const s3_func = (bark) => {
        let tempx = bark, x, tempy;
        if (tempx >= 0) tempx *= 3; else tempx *= 1.5;
        if (tempx >= 0.5 && tempx <= 2.5) { const t = tempx - 0.5; x = 8.0 * (t * t - 2.0 * t); } else x = 0.0;
        tempx += 0.474;
        tempy = 15.811389 + 7.5 * tempx - 17.5 * Math.sqrt(1.0 + tempx * tempx);
        if (tempy <= -60.0) return 0.0;
        tempx = Math.exp((x + tempy) * LN_TO_LOG10);
        tempx /= .6609193;
        return tempx;
    };
    const bval = f32(CBANDS), bval_width = f32(CBANDS), norm = f32(CBANDS);

    function init_numline(numlines, bo, bm, bo_w, mld, blksize, scalepos, deltafreq, sbmax) {
        const b_frq = f32(CBANDS + 1);
        const sample_freq_frac = sfreq0 / (sbmax > 15 ? 2 * 576 : 2 * 192);
        const partition = i32(HBLKSIZE);
        const sfreq = sfreq0 / blksize;
        let i, j = 0, ni = 0;
        for (i = 0; i < CBANDS; i++) {
            const bark1 = freq2bark(sfreq * j);
            b_frq[i] = sfreq * j;
            let j2;
            for (j2 = j; freq2bark(sfreq * j2) - bark1 < DELBARK && j2 <= blksize / 2; j2++);
            numlines[i] = j2 - j;
            ni = i + 1;
            while (j < j2) partition[j++] = i;
            if (j > blksize / 2) { j = blksize / 2; ++i; break; }
        }
        b_frq[i] = sfreq * j;
        for (let sfb = 0; sfb < sbmax; sfb++) {
            const start = scalepos[sfb], end = scalepos[sfb + 1];
            let i1 = 0 | Math.floor(.5 + deltafreq * (start - .5));
            if (i1 < 0) i1 = 0;
            let i2 = 0 | Math.floor(.5 + deltafreq * (end - .5));
            if (i2 > blksize / 2) i2 = blksize / 2;
            bm[sfb] = (partition[i1] + partition[i2]) / 2;
            bo[sfb] = partition[i2];
            const f_tmp = sample_freq_frac * end;
            bo_w[sfb] = (f_tmp - b_frq[bo[sfb]]) / (b_frq[bo[sfb] + 1] - b_frq[bo[sfb]]);
            if (bo_w[sfb] < 0) bo_w[sfb] = 0; else if (bo_w[sfb] > 1) bo_w[sfb] = 1;
            /* stereo demasking threshold of the band (PsyModel.js:2432-2438) */
            let arg = freq2bark(sfreq * scalepos[sfb] * deltafreq);
            arg = (Math.min(arg, 15.5) / 15.5);
            mld[sfb] = Math.pow(10.0, 1.25 * (1 - Math.cos(Math.PI * arg)) - 2.5);
        }
        j = 0;
        for (let k = 0; k < ni; k++) {
            const w = numlines[k];
            bval[k] = .5 * (freq2bark(sfreq * j) + freq2bark(sfreq * (j + w - 1)));
            bval_width[k] = freq2bark(sfreq * (j + w - .5)) - freq2bark(sfreq * (j - .5));
            j += w;
        }
        return ni;
    }

    function init_s3_values(s3ind, npart) {
        const s3 = []; for (let i = 0; i < CBANDS; i++) s3.push(f32(CBANDS));
        for (let i = 0; i < npart; i++)
            for (let j = 0; j < npart; j++) {
                const v = s3_func(bval[i] - bval[j]) * bval_width[j];
                s3[i][j] = v * norm[i];
            }
        let nz = 0;
        for (let i = 0; i < npart; i++) {
            let j;
            for (j = 0; j < npart; j++) if (s3[i][j] > 0.0) break;
            s3ind[2 * i] = j;
            for (j = npart - 1; j > 0; j--) if (s3[i][j] > 0.0) break;
            s3ind[2 * i + 1] = j;
            nz += (s3ind[2 * i + 1] - s3ind[2 * i] + 1);
        }
        const out = f32(nz);
        let k = 0;
        for (let i = 0; i < npart; i++)
            for (let j = s3ind[2 * i]; j <= s3ind[2 * i + 1]; j++) out[k++] = s3[i][j];
        return out;
    }

    T.numlines_l = i32(CBANDS); T.numlines_s = i32(CBANDS); T.rnumlines_l = f32(CBANDS);
    T.bo_l = i32(SBMAX_l); T.bm_l = i32(SBMAX_l); T.bo_s = i32(SBMAX_s); T.bm_s = i32(SBMAX_s);
    T.bo_l_weight = f32(SBMAX_l); T.bo_s_weight = f32(SBMAX_s);
    T.mld_l = f32(SBMAX_l); T.mld_s = f32(SBMAX_s);
    T.s3ind = i32(2 * CBANDS); T.s3ind_s = i32(2 * CBANDS);
    T.ATH_cb_l = f32(CBANDS); T.ATH_cb_s = f32(CBANDS);

    const bvl_a = 13, bvl_b = 24, snr_l_a = 0, snr_l_b = 0, snr_s_a = -8.25, snr_s_b = -4.5;
    T.npart_l = init_numline(T.numlines_l, T.bo_l, T.bm_l, T.bo_l_weight, T.mld_l, BLKSIZE, p.sfb_l,
        BLKSIZE / (2.0 * 576), SBMAX_l);
    for (let i = 0; i < T.npart_l; i++) {
        let snr = snr_l_a;
        if (bval[i] >= bvl_a)
            snr = snr_l_b * (bval[i] - bvl_a) / (bvl_b - bvl_a) + snr_l_a * (bvl_b - bval[i]) / (bvl_b - bvl_a);
        norm[i] = Math.pow(10.0, snr / 10.0);
        T.rnumlines_l[i] = T.numlines_l[i] > 0 ? 1.0 / T.numlines_l[i] : 0;
    }
    T.s3_ll = init_s3_values(T.s3ind, T.npart_l);
    {
        let j = 0;
        for (let i = 0; i < T.npart_l; i++) {
            let x = FLOAT_MAX;
            for (let k = 0; k < T.numlines_l[i]; k++, j++) {
                const freq = sfreq0 * j / (1000.0 * BLKSIZE);
                let level = ATHformula(freq * 1000) - 20;
                level = Math.pow(10., 0.1 * level);
                level *= T.numlines_l[i];
                if (x > level) x = level;
            }
            T.ATH_cb_l[i] = x;
        }
    }
    T.npart_s = init_numline(T.numlines_s, T.bo_s, T.bm_s, T.bo_s_weight, T.mld_s, BLKSIZE_s, p.sfb_s,
        BLKSIZE_s / (2.0 * 192), SBMAX_s);
    {
        let j = 0;
        for (let i = 0; i < T.npart_s; i++) {
            let snr = snr_s_a;
            if (bval[i] >= bvl_a)
                snr = snr_s_b * (bval[i] - bvl_a) / (bvl_b - bvl_a) + snr_s_a * (bvl_b - bval[i]) / (bvl_b - bvl_a);
            norm[i] = Math.pow(10.0, snr / 10.0);
            let x = FLOAT_MAX;
            for (let k = 0; k < T.numlines_s[i]; k++, j++) {
                const freq = sfreq0 * j / (1000.0 * BLKSIZE_s);
                let level = ATHformula(freq * 1000) - 20;
                level = Math.pow(10., 0.1 * level);
                level *= T.numlines_s[i];
                if (x > level) x = level;
            }
            T.ATH_cb_s[i] = x;
        }
    }
    T.s3_ss = init_s3_values(T.s3ind_s, T.npart_s);
    /* spread only from npart_l bands (PsyModel.js:2718-2721) */
    for (let b = 0; b < T.npart_l; b++)
        if (T.s3ind[2 * b + 1] > T.npart_l - 1) T.s3ind[2 * b + 1] = T.npart_l - 1;

    /* mask_add shortcuts (PsyModel.js:376-380) */
    T.ma_max_i1 = Math.pow(10, (8 + 1) / 16.0);
    T.ma_max_i2 = Math.pow(10, (23 + 1) / 16.0);
    T.ma_max_m = Math.pow(10, 15 / 10.0);

    /* FFT analysis windows (FFT.js:226-242) */
    T.window = f32(BLKSIZE); T.window_s = f32(BLKSIZE_s / 2);
    for (let i = 0; i < BLKSIZE; i++)
        T.window[i] = (0.42 - 0.5 * Math.cos(2 * Math.PI * (i + .5) / BLKSIZE)
            + 0.08 * Math.cos(4 * Math.PI * (i + .5) / BLKSIZE));
    for (let i = 0; i < BLKSIZE_s / 2; i++)
        T.window_s[i] = (0.5 * (1.0 - Math.cos(2.0 * Math.PI * (i + 0.5) / BLKSIZE_s)));

    /* FHT twiddles: the f64 recurrence of FFT.js:72-111, unrolled into a table.
     * pass t (k4 = 4,16,64,256 -> kx = 2,8,32,128), entry i = 1..kx-1 holds (c1,s1,c2,s2) as the
     * butterflies of that i see them.  Offsets: pass0 @0 (1 entry), pass1 @1 (7), pass2 @8 (31), pass3 @39 (127) */
    T.fht_twiddle = new Float64Array(4 * 166);
    {
        let off = 0, kx = 2;
        for (let t = 0; t < 4; t++, kx <<= 2) {
            const ct = C.fht_costab[2 * t], st = C.fht_costab[2 * t + 1];
            let c1 = ct, s1 = st;
            for (let i = 1; i < kx; i++) {
                const c2 = 1 - (2 * s1) * s1;
                const s2 = (2 * s1) * c1;
                T.fht_twiddle.set([c1, s1, c2, s2], 4 * off); off++;
                const c2b = c1;
                c1 = c2b * ct - s1 * st;
                s1 = c2b * st + s1 * ct;
            }
        }
    }

    /* temporal masking decay for short-block xmin smoothing (PsyModel.js:2701-2703) */
    T.decay = Math.exp(-1.0 * LOG10 / (0.01 * sfreq0 / 192.0));

    /* equal-loudness weights (PsyModel.js:2735-2752) */
    T.eql_w = f32(BLKSIZE / 2);
    {
        const freq_inc = p.out_samplerate / BLKSIZE;
        let eql_balance = 0.0, freq = 0.0;
        for (let i = 0; i < BLKSIZE / 2; ++i) {
            freq += freq_inc;
            T.eql_w[i] = 1. / Math.pow(10, ATHformula(freq) / 10);
            eql_balance += T.eql_w[i];
        }
        eql_balance = 1.0 / eql_balance;
        for (let i = BLKSIZE / 2; --i >= 0;) T.eql_w[i] *= eql_balance;
    }
    T.VO_SCALE = (1. / (14752 * 14752) / (BLKSIZE / 2));
    return T;
}

/* ------------------------------------------------------------------ */
/* blob packing                                                        */
/* ------------------------------------------------------------------ */

const DT_I32 = 1, DT_F32 = 2, DT_F64 = 3;
const ENTRY_BYTES = 48;           /* char name[32]; u32 dtype,count,offset,pad */

function packBlob(entries) {
    /* entries: [name, typedArray] ; layout: header(16) | directory | 8-byte aligned payloads */
    const n = entries.length;
    let off = 16 + n * ENTRY_BYTES;
    off = (off + 7) & ~7;
    const offs = [];
    for (const [, a] of entries) { offs.push(off); off += (a.byteLength + 7) & ~7; }
    const buf = Buffer.alloc(off);
    buf.writeUInt32LE(0x4254484c, 0);  /* 'LHTB' */
    buf.writeUInt32LE(1, 4);
    buf.writeUInt32LE(n, 8);
    buf.writeUInt32LE(off, 12);
    entries.forEach(([name, a], k) => {
        const e = 16 + k * ENTRY_BYTES;
        if (name.length > 31) throw new Error('name too long: ' + name);
        buf.write(name, e, 'ascii');
        const dt = (a instanceof Int32Array) ? DT_I32 : (a instanceof Float32Array) ? DT_F32 :
            (a instanceof Float64Array) ? DT_F64 : 0;
        if (!dt) throw new Error('bad array type for ' + name);
        buf.writeUInt32LE(dt, e + 32);
        buf.writeUInt32LE(a.length, e + 36);
        buf.writeUInt32LE(offs[k], e + 40);
        Buffer.from(a.buffer, a.byteOffset, a.byteLength).copy(buf, offs[k]);
    });
    return buf;
}

function I(v) { return Int32Array.from(Array.isArray(v) ? v : [v]); }
function D(v) { return Float64Array.from(Array.isArray(v) ? v : [v]); }

function huffmanEntries() {
    /* flatten ht[0..33]: per table xlen, linmax, offset into shared code/len pools (-1 = absent) */
    const xlen = [], linmax = [], off = [], code = [], hlen = [];
    const seen = new Map();
    C.ht.forEach((h, t) => {
        xlen.push(h.xlen); linmax.push(h.linmax);
        if (!h.hlen) { off.push(-1); return; }
        const key = JSON.stringify(h.hlen) + JSON.stringify(h.table);
        if (seen.has(key)) { off.push(seen.get(key)); return; }
        const o = hlen.length;
        seen.set(key, o); off.push(o);
        for (let i = 0; i < h.hlen.length; i++) { hlen.push(h.hlen[i]); code.push(h.table ? h.table[i] : 0); }
    });
    return [['ht_xlen', I(xlen)], ['ht_linmax', I(linmax)], ['ht_off', I(off)],
        ['ht_code', I(code)], ['ht_hlen', I(hlen)],
        ['largetbl', I(C.largetbl)], ['table23', I(C.table23)], ['table56', I(C.table56)],
        ['t32l', I(C.ht[32].hlen)], ['t33l', I(C.ht[33].hlen)]];
}

function buildBlob(channels, samplerate, kbps, opts) {
    const p = resolveParams(channels, samplerate, kbps, opts);
    const T = buildTables(p);
    const cfg_i = {
        channels_out: p.channels_out, mode: p.mode, mode_gr: p.mode_gr, version: p.version,
        samplerate_index: p.samplerate_index, bitrate_index: p.bitrate_index, brate: p.brate,
        out_samplerate: p.out_samplerate, sideinfo_len: p.sideinfo_len, frac_SpF: p.frac_SpF,
        noise_shaping: p.noise_shaping, noise_shaping_amp: p.noise_shaping_amp,
        noise_shaping_stop: p.noise_shaping_stop, subblock_gain: p.subblock_gain,
        use_best_huffman: p.use_best_huffman, full_outer_loop: p.full_outer_loop,
        substep_shaping: p.substep_shaping, sfb21_extra: p.sfb21_extra,
        quant_comp: p.quant_comp, quant_comp_short: p.quant_comp_short,
        short_blocks_coupled: p.short_blocks_coupled, useTemporal: p.useTemporal,
        ATH_useAdjust: p.ATH_useAdjust, athaa_loudapprox: p.athaa_loudapprox,
        copyright: p.copyright, original: p.original, emphasis: p.emphasis, extension: p.extension,
        error_protection: p.error_protection, npart_l: T.npart_l, npart_s: T.npart_s,
        in_samplerate: p.in_samplerate, rs_filter_l: p.rs_filter_l, rs_bpc: p.rs_bpc,
        disable_reservoir: p.disable_reservoir
    };
    const cfg_d = {
        scale: p.scale, attackthre: p.attackthre, attackthre_s: p.attackthre_s,
        interChRatio: p.interChRatio, masking_lower_long: p.masking_lower_long,
        masking_lower_short: p.masking_lower_short, ATH_aaSensitivityP: p.ATH_aaSensitivityP,
        ATH_floor: T.ATH_floor, decay: T.decay, ma_max_i1: T.ma_max_i1, ma_max_i2: T.ma_max_i2,
        ma_max_m: T.ma_max_m, VO_SCALE: T.VO_SCALE, resample_ratio: p.resample_ratio,
        msfix: p.msfix, ATHlower: p.ATHlower
    };
    /* input gains / downmix: named entries that exist only when an option asks for them (a blob without is the bytes it always was;
     * the library defaults them) */
    if (p.input_options) {
        Object.assign(cfg_i, { channels_in: p.channels_in, do_scale: p.do_scale, do_scale_left: p.do_scale_left, do_scale_right: p.do_scale_right });
        Object.assign(cfg_d, { scale_left: p.scale_left, scale_right: p.scale_right });
    }
    /* { infoTag }: what the tag frame reports besides the stream's totals, resolved here as putLameVBR does (VBRTag.js:576-732) -- named entries that
     * exist only with the option (a blob without it is the bytes it always was).  quality: 100 - 10 VBR_q - quality with lame_init's VBR_q = 4 and
     * the stream's quality (3, or 7 with { quality }); method 1 (CBR); lowpass in units of 100 Hz; flags: ATHtype + (exp_nspsytune << 4), i.e. the nspsytune and the
     * safe-joint bit; misc: noise_shaping + (stereoMode << 2) + (nonOptimal << 5) + (sourceFreq << 6) by VBRTag.js:686-732 -- a downmix is MONO,
     * unequal channel gains, a disabled reservoir below 320 kbps and an input rate of at most 32 kHz are "non-optimal"; preset: the bitrate that
     * selected the ABR preset row (Lame.js:1216-1218, Presets.js:415); delay: Encoder.ENCDELAY */
    let tagVersion = null;
    if (p.info_tag) {
        const VBR_q = 4, quality = p.quality;
        const stereoMode = p.mode == MODE_MONO ? 0 : p.mode == MODE_STEREO ? 1 : 3;
        const sourceFreq = samplerate <= 32000 ? 0 : samplerate == 48000 ? 2 : samplerate > 48000 ? 3 : 1;
        const nonOptimal = (p.scale_left < p.scale_right || p.scale_left > p.scale_right || (p.disable_reservoir && p.brate < 320) || p.ATHtype == 0 || samplerate <= 32000) ? 1 : 0;
        const lp = p.lowpassfreq / 100.0 + .5;
        Object.assign(cfg_i, { info_tag: 1, tag_quality: Math.max(0, 100 - 10 * VBR_q - quality), tag_method: 1, tag_lowpass: 0 | (lp > 255 ? 255 : lp),
            tag_flags: (p.ATHtype + (p.exp_nspsytune << 4)) & 0xff, tag_misc: (p.noise_shaping + (stereoMode << 2) + (nonOptimal << 5) + (sourceFreq << 6)) & 0xff,
            tag_preset: p.brate, tag_delay: 576 });
        tagVersion = 'LAME' + C.lame_short_version.split('.').slice(0, 2).join('.') + 'r';          /* Version.js:56-59 getLameVeryShortVersion */
        if (tagVersion.length != 9) throw new Error('lamejs_amd: the very short version string must have 9 characters');
    }
    /* { replayGain }: one named entry that exists only with the option (a blob without it is the bytes it always was) */
    if (p.replay_gain) Object.assign(cfg_i, { replay_gain: 1 });
    const entries = [];
    entries.push(['cfg_i_names', Int32Array.from(Buffer.from(Object.keys(cfg_i).join(',') + '\0', 'ascii'))]);
    entries.push(['cfg_i', I(Object.values(cfg_i))]);
    entries.push(['cfg_d_names', Int32Array.from(Buffer.from(Object.keys(cfg_d).join(',') + '\0', 'ascii'))]);
    entries.push(['cfg_d', D(Object.values(cfg_d))]);
    const push = (n, a) => entries.push([n, a]);
    push('amp_filter', p.amp_filter);
    push('rs_blackfilt', p.rs_blackfilt);
    push('sfb_l', p.sfb_l); push('sfb_s', p.sfb_s); push('psfb21', p.psfb21); push('psfb12', p.psfb12);
    push('ATH_l', T.ATH_l); push('ATH_s', T.ATH_s); push('ATH_psfb21', T.ATH_psfb21); push('ATH_psfb12', T.ATH_psfb12);
    push('ATH_cb_l', T.ATH_cb_l); push('ATH_cb_s', T.ATH_cb_s); push('eql_w', T.eql_w);
    push('pow43', T.pow43); push('adj43', T.adj43); push('ipow20', T.ipow20); push('pow20', T.pow20);
    push('bv_scf', T.bv_scf); push('longfact', T.longfact); push('shortfact', T.shortfact);
    push('numlines_l', T.numlines_l); push('numlines_s', T.numlines_s); push('rnumlines_l', T.rnumlines_l);
    push('bo_l', T.bo_l); push('bm_l', T.bm_l); push('bo_s', T.bo_s); push('bm_s', T.bm_s);
    push('bo_l_weight', T.bo_l_weight); push('bo_s_weight', T.bo_s_weight);
    push('mld_l', T.mld_l); push('mld_s', T.mld_s);
    push('s3ind', T.s3ind); push('s3ind_s', T.s3ind_s); push('s3_ll', T.s3_ll); push('s3_ss', T.s3_ss);
    push('window', T.window); push('window_s', T.window_s); push('fht_twiddle', T.fht_twiddle);
    push('fht_costab', D(C.fht_costab)); push('fft_rv_tbl', I(C.fft_rv_tbl));
    push('enwindow', D(C.enwindow));
    push('mdct_win', D([].concat(C.mdct_win[0], C.mdct_win[1], C.mdct_win[2], C.mdct_win[3])));
    push('mdct_order', I(C.mdct_order));
    push('ma_tab', D(C.ma_tab)); push('ma_table1', D(C.ma_table1)); push('ma_table2', D(C.ma_table2));
    push('ma_table3', D(C.ma_table3)); push('hpf_fircoef', D(C.hpf_fircoef));
    push('pretab', I(C.pretab)); push('scfsi_band', I(C.scfsi_band));
    push('slen1_n', I(C.slen1_n)); push('slen2_n', I(C.slen2_n));
    push('slen1_tab', I(C.slen1_tab)); push('slen2_tab', I(C.slen2_tab));
    push('scale_short', I(C.scale_short)); push('scale_long', I(C.scale_long));
    push('huf_tbl_noESC', I(C.huf_tbl_noESC));
    /* ancillary "version" bytes as the reference emits them: string chars coerced by >> (BitStream.js:180-204) */
    push('version_bytes', I(C.lame_short_version.split('').map(ch => (ch >> 0) & 0xff)));
    huffmanEntries().forEach(e => entries.push(e));
    /* what the blob was generated FROM: the first 8 bytes of sha256(tables.js ++ constants.json) -- a cached blob is stale when its generator
     * has changed, whatever the files' modification times say after a checkout (lamejs_amd/__init__.py tables_blob, __graft_entry__.py) */
    if (tagVersion) push('tag_version', I(tagVersion.split('').map(ch => ch.charCodeAt(0))));
    push('src_sha256_64', sourceHash());
    return { blob: packBlob(entries), params: p, tables: T };
}

function sourceHash() {
    const fs = require('fs'), path = require('path');
    const h = require('crypto').createHash('sha256');
    h.update(fs.readFileSync(__filename)); h.update(fs.readFileSync(path.join(__dirname, 'constants.json')));
    const d = h.digest();
    return Int32Array.from([d.readInt32LE(0), d.readInt32LE(4)]);
}

/* { fractionalResample }: the longest encodeBuffer() call that is accepted whatever calls came before (0: the configuration does not
 * resample by a non-integer ratio, any length goes).  The reference consumes a call whole while floor((framesize - 1) * ratio - itime)
 * + 15.5 >= length, and its clock itime never exceeds 15.5 after a call it consumed whole (Lame.js:1769-1813). */
function fractionalCallLimit(p) {
    if (p.rs_filter_l != 31) return 0;
    return Math.floor((p.framesize - 1) * p.resample_ratio - 15.5) + 15;
}

module.exports = { buildBlob, resolveParams, buildTables, packBlob, sourceHash, fractionalCallLimit };

if (require.main === module) {
    /* CLI: node tables.js <channels> <samplerate> <kbps> <out.bin> [joint] [reservoir] [fracresample] [downmix] [scale=G] [scaleLeft=G] [scaleRight=G]
     *      [protect] [copyright] [original=0|1] [privateBit] [emphasis=E] [infoTag] [replayGain] [quality=3|7|8]
     *      [outrate=HZ] [lowpass=HZ|-1] [lowpasswidth=HZ] [highpass=HZ] [highpasswidth=HZ] */
    const [ch, sr, kb, out] = process.argv.slice(2), flags = process.argv.slice(6);
    const opts = { jointStereo: flags.includes('joint'), reservoir: flags.includes('reservoir'), fractionalResample: flags.includes('fracresample') };
    if (flags.includes('downmix')) opts.downmix = true;
    for (const f of flags) { const m = /^(scale|scaleLeft|scaleRight)=(.+)$/.exec(f); if (m) opts[m[1]] = Number(m[2]); }
    for (const k of ['protect', 'copyright', 'privateBit', 'infoTag', 'replayGain']) if (flags.includes(k)) opts[k] = true;
    for (const f of flags) { const m = /^(original|emphasis|quality)=(.+)$/.exec(f); if (m) opts[m[1]] = Number(m[2]); }
    {
        const W = { outrate: 'outSampleRate', lowpass: 'lowpass', lowpasswidth: 'lowpassWidth', highpass: 'highpass', highpasswidth: 'highpassWidth' };
        for (const f of flags) { const m = /^(outrate|lowpass|lowpasswidth|highpass|highpasswidth)=(.+)$/.exec(f); if (m) opts[W[m[1]]] = Number(m[2]); }
    }
    const r = buildBlob(+ch, +sr, +kb, opts);
    require('fs').writeFileSync(out, r.blob);
    console.log('wrote', out, r.blob.length, 'bytes');
}
