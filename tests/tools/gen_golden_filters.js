/*
 * TEST TOOL (needs the reference's sources; LAMEJS_REF names their directory): goldens for the output sample rate and the polyphase filter settings (tests/golden/golden_filters.json).
 *
 * gfp.out_samplerate, lowpassfreq, lowpasswidth, highpassfreq and highpasswidth are settings of the reference's encoder core that its public Mp3Encoder
 * leaves at lame_init's values (Lame.js:147-150), so this generator wires the UNMODIFIED modules itself, as tests/tools/gen_golden_quality.js does, and sets
 * the five fields (with mode, quality, disable_reservoir and error_protection where a case asks) before lame_init_params.  What lame_init_params resolved --
 * out_samplerate, lowpassfreq, brate, version, resample_ratio and all 32 amp_filter values -- is recorded per case beside the bytes.
 *
 * Streams of 12 output frames (12 * framesize * resample_ratio input samples) on the corpora of tests/tools/pcm_gen.js, by the names of gen_golden_quality.js.
 * Every stream is also encoded without the five settings (where the reference can: a triple it resamples by a non-integer ratio feeds itself NaN) and must
 * differ; a highpass case must close band 0; a width case must have a band strictly between 0 and 1.
 * { infoTag, replayGain } of a case are this project's host-side options: the reference stream recorded for it is the audio behind the tag's placeholder.
 * usage: node tests/tools/gen_golden_filters.js          (required as a module it only exports refEncoder and CONFIGS: tests/js_filters_check.js)
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const { material, REF } = require('./gen_golden_quality.js');
const S = path.join(REF, 'src', 'js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);
const FIELDS = { outSampleRate: 'out_samplerate', lowpass: 'lowpassfreq', lowpassWidth: 'lowpasswidth', highpass: 'highpassfreq', highpassWidth: 'highpasswidth' };

/* opts: the five settings, and { quality, jointStereo, reservoir, downmix, protect } */
function refEncoder(channels, samplerate, kbps, opts) {
    const req = (n) => require(path.join(S, n + '.js'));
    const Lame = req('Lame'), Presets = req('Presets'), GainAnalysis = req('GainAnalysis'), QuantizePVT = req('QuantizePVT'), Quantize = req('Quantize');
    const Takehiro = req('Takehiro'), Reservoir = req('Reservoir'), MPEGMode = req('MPEGMode'), BitStream = req('BitStream'), Version = req('Version'), VBRTag = req('VBRTag');
    function Stub() { this.setModules = function () {}; }
    const lame = new Lame(), gaud = new Stub(), ga = new GainAnalysis(), bs = new BitStream();
    const p = new Presets(), qupvt = new QuantizePVT(), qu = new Quantize(), vbr = new VBRTag();
    const ver = new Version(), id3 = new Stub(), rv = new Reservoir(), tak = new Takehiro();
    const parse = new Stub(), mpg = {};
    lame.setModules(ga, bs, p, qupvt, qu, vbr, ver, id3, mpg);
    bs.setModules(ga, mpg, ver, vbr);
    id3.setModules(bs, ver);
    p.setModules(lame);
    qu.setModules(bs, rv, qupvt, tak);
    qupvt.setModules(tak, rv, lame.enc.psy);
    rv.setModules(bs);
    tak.setModules(qupvt);
    vbr.setModules(lame, bs, ver);
    gaud.setModules(parse, mpg);
    parse.setModules(ver, id3, p);
    global.CRC_writeheader = bs.CRC_writeheader;
    global.byte = (x) => x;
    const gfp = lame.lame_init();
    gfp.num_channels = channels;
    gfp.in_samplerate = samplerate;
    gfp.brate = kbps;
    gfp.mode = opts.downmix ? MPEGMode.MONO : (opts.jointStereo && channels == 2) ? MPEGMode.JOINT_STEREO : MPEGMode.STEREO;
    gfp.quality = opts.quality === undefined ? 3 : opts.quality;
    gfp.bWriteVbrTag = false;
    gfp.disable_reservoir = !opts.reservoir;
    gfp.write_id3tag_automatic = false;
    if (opts.protect) gfp.error_protection = 1;
    for (const k in FIELDS) if (opts[k] !== undefined) gfp[FIELDS[k]] = opts[k];
    const rc = lame.lame_init_params(gfp);
    if (rc != 0) throw new Error('lame_init_params rc=' + rc);
    let maxSamples = 1152, mp3buf_size = 0 | (1.25 * maxSamples + 7200), mp3buf = new Int8Array(mp3buf_size);
    return {
        gfp, gfc: gfp.internal_flags,
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if (left.length > maxSamples) { maxSamples = left.length; mp3buf_size = 0 | (1.25 * maxSamples + 7200); mp3buf = new Int8Array(mp3buf_size); }
            const n = lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, mp3buf_size);
            return new Int8Array(mp3buf.subarray(0, n));
        },
        flush() {
            const n = lame.lame_encode_flush(gfp, mp3buf, 0, mp3buf_size);
            return new Int8Array(mp3buf.subarray(0, n));
        }
    };
}

const UNEVEN = [1, 17, 777, 4096, 4096, 777, 17, 1, 4042];      /* sums to 12 * 1152 */
const LP12 = { lowpass: 12000, outSampleRate: 44100 };
/* [name, channels in, samplerate, kbps, options, corpus, call lengths (null: twelve calls of one output frame's input each)] */
const CONFIGS = [
    /* the settings checked on the unmodified reference when the options were proposed */
    ['lp12000_out44100_128', 2, 44100, 128, LP12, 'bursts', null],
    ['lp12000_w2000_out44100_128', 2, 44100, 128, { lowpass: 12000, lowpassWidth: 2000, outSampleRate: 44100 }, 'bursts', null],
    ['lp_off_128', 2, 44100, 128, { lowpass: -1 }, 'bursts', null],
    ['lp19000_128', 2, 44100, 128, { lowpass: 19000 }, 'bursts', null],
    ['hp500_128', 2, 44100, 128, { highpass: 500 }, 'bursts', null],
    ['hp2000_w500_128', 2, 44100, 128, { highpass: 2000, highpassWidth: 500 }, 'bursts', null],
    ['out44100_44100_96', 2, 44100, 96, { outSampleRate: 44100 }, 'bursts', null],
    ['out48000_48000_112', 2, 48000, 112, { outSampleRate: 48000 }, 'bursts', null],
    ['out22050_44100_128', 2, 44100, 128, { outSampleRate: 22050 }, 'bursts', null],
    ['out22050_44100_320', 2, 44100, 320, { outSampleRate: 22050 }, 'bursts', null],
    ['out16000_48000_64', 2, 48000, 64, { outSampleRate: 16000 }, 'bursts', null],
    /* (192000 Hz, one channel, 64 kbps: the reference's own choice is 48000 Hz already, so the row alone would be the default's bytes -- taken with two channels,
     *  where the default is 24000 Hz, and with one channel and a lowpass beside it) */
    ['out48000_192000_64', 2, 192000, 64, { outSampleRate: 48000 }, 'bursts', null],
    ['out48000_lp15000_192000_64_mono', 1, 192000, 64, { outSampleRate: 48000, lowpass: 15000 }, 'bursts', null],
    ['out8000_48000_16_mono', 1, 48000, 16, { outSampleRate: 8000 }, 'bursts', null],
    /* further settings */
    ['mono_lp8000_out44100_64', 1, 44100, 64, { lowpass: 8000, outSampleRate: 44100 }, 'bursts', null],
    ['lp14000_hp1000_out44100_128', 2, 44100, 128, { lowpass: 14000, highpass: 1000, outSampleRate: 44100 }, 'bursts', null],
    ['out44100_88200_128', 2, 88200, 128, { outSampleRate: 44100 }, 'bursts', null],
    ['lp16000_320', 2, 44100, 320, { lowpass: 16000 }, 'bursts', null],
    ['lp_off_48000_320', 2, 48000, 320, { lowpass: -1 }, 'bursts', null],
    ['lpw1000_auto_128', 2, 44100, 128, { lowpassWidth: 1000 }, 'bursts', null],
    ['lp5000_w6000_out44100_128', 2, 44100, 128, { lowpass: 5000, lowpassWidth: 6000, outSampleRate: 44100 }, 'bursts', null],
    ['hp1000_w0_128', 2, 44100, 128, { highpass: 1000, highpassWidth: 0 }, 'bursts', null],
    ['hp8000_lp_off_128', 2, 44100, 128, { highpass: 8000, lowpass: -1 }, 'bursts', null],
    ['hp400_22050_48', 2, 22050, 48, { highpass: 400 }, 'bursts', null],
    ['mono_hp200_lp3000_11025_16', 1, 11025, 16, { highpass: 200, lowpass: 3000, outSampleRate: 11025 }, 'bursts', null],
    ['mono_lp_off_8000_8', 1, 8000, 8, { lowpass: -1 }, 'sine', null],
    ['out24000_48000_128', 2, 48000, 128, { outSampleRate: 24000 }, 'bursts', null],
    ['out11025_44100_32_mono', 1, 44100, 32, { outSampleRate: 11025 }, 'bursts', null],
    ['hp500_sine_128', 2, 44100, 128, { highpass: 500 }, 'sine', null],
    ['lp_off_silent3_128', 2, 44100, 128, { lowpass: -1 }, 'silent3', null],
    ['lp12000_wavexcerpt_128', 2, 44100, 128, LP12, 'wavexcerpt', null],
    /* call lengths */
    ['lp12000_uneven_calls', 2, 44100, 128, LP12, 'bursts', UNEVEN],
    ['hp500_uneven_calls', 2, 44100, 128, { highpass: 500 }, 'bursts', UNEVEN],
    /* with the other options */
    ['joint_lp12000_mixed_128', 2, 44100, 128, Object.assign({ jointStereo: true }, LP12), 'mixed', null],
    ['joint_hp500_centre_128', 2, 44100, 128, { jointStereo: true, highpass: 500 }, 'centre_bursts', null],
    ['resv_hp500_128', 2, 44100, 128, { reservoir: true, highpass: 500 }, 'bursts', null],
    ['resv_out22050_44100_128', 2, 44100, 128, { reservoir: true, outSampleRate: 22050 }, 'bursts', null],
    ['downmix_lp10000_out44100_64', 2, 44100, 64, { downmix: true, lowpass: 10000, outSampleRate: 44100 }, 'bursts', null],
    ['protect_hp2000_w500_128', 2, 44100, 128, { protect: true, highpass: 2000, highpassWidth: 500 }, 'bursts', null],
    ['q7_hp500_128', 2, 44100, 128, { quality: 7, highpass: 500 }, 'bursts', null],
    ['q7_out22050_44100_320', 2, 44100, 320, { quality: 7, outSampleRate: 22050 }, 'bursts', null],
    ['tag_gain_lp12000_w2000_out44100_128', 2, 44100, 128, { infoTag: true, replayGain: true, lowpass: 12000, lowpassWidth: 2000, outSampleRate: 44100 }, 'bursts', null]
];

function run(ch, sr, kbps, opts, L, R, lens) {
    const enc = refEncoder(ch, sr, kbps, opts);
    const parts = [], bytes = [];
    let p = 0;
    for (const m of lens) {
        const b = ch == 2 ? enc.encodeBuffer(L.subarray(p, p + m), R.subarray(p, p + m)) : enc.encodeBuffer(L.subarray(p, p + m));
        p += m;
        bytes.push(b.length); parts.push(Buffer.from(b.buffer, b.byteOffset, b.length));
    }
    const f = enc.flush(), fb = Buffer.from(f.buffer, f.byteOffset, f.length);
    return { enc, parts, bytes, fb, whole: Buffer.concat(parts.concat([fb])) };
}

module.exports = { refEncoder, material, CONFIGS, FIELDS };
if (require.main === module) {
const cases = [];
for (const [name, ch, sr, kbps, opts, corpus, lens0] of CONFIGS) {
    const probe = refEncoder(ch, sr, kbps, opts);
    const ratio = probe.gfc.resample_ratio, framesize = probe.gfp.framesize;
    if (ratio != Math.floor(ratio)) throw new Error(name + ': the reference resolved the ratio ' + ratio);
    const per = framesize * ratio, N = 12 * per;
    const lens = lens0 || new Array(12).fill(per);
    if (lens.reduce((a, b) => a + b, 0) != N) throw new Error('call lengths of ' + name);
    const [L, R] = material(corpus, N, ch);
    const h = crypto.createHash('md5'); h.update(buf(L)); if (R) h.update(buf(R));
    const r = run(ch, sr, kbps, opts, L, R, lens);
    const plainOpts = Object.assign({}, opts); for (const k in FIELDS) delete plainOpts[k];
    let plain_md5 = null;                 /* null: the reference cannot encode the triple without the settings (non-integer ratio: NaN samples, or it throws) */
    try {
        const q = refEncoder(ch, sr, kbps, plainOpts), pr = q.gfc.resample_ratio;
        if (pr == Math.floor(pr)) plain_md5 = md5(run(ch, sr, kbps, plainOpts, L, R, lens).whole);
    } catch (e) { plain_md5 = null; }
    if (plain_md5 !== null && plain_md5 == md5(r.whole)) throw new Error(name + ': the bytes do not differ from the stream without the settings');
    const g = r.enc.gfc, gp = r.enc.gfp, af = Float32Array.from(g.amp_filter);
    if (af.length != 32) throw new Error(name + ': amp_filter has ' + af.length + ' values');
    if (opts.highpass !== undefined && !(af[0] < 1e-12)) throw new Error(name + ': the highpass leaves band 0 open (' + af[0] + ')');
    if ((opts.lowpassWidth > 0 || opts.highpassWidth > 0) && !Array.from(af).some((v) => v > 0 && v < 1)) throw new Error(name + ': no band strictly between 0 and 1');
    const settings = {}; for (const k in FIELDS) if (opts[k] !== undefined) settings[k] = opts[k];
    const o = { name, channels: ch, samplerate: sr, kbps, settings, corpus, nsamples: N, ref_channels_out: g.channels_out,
                ref: { out_samplerate: gp.out_samplerate, lowpassfreq: gp.lowpassfreq, brate: gp.brate, version: gp.version, resample_ratio: g.resample_ratio, mode_gr: g.mode_gr },
                amp_filter_bits: Array.from(new Uint32Array(af.buffer)), open_bands: Array.from(af).map((v) => (v < 1e-12 ? 0 : 1)).join(''),
                frames: null, call_lens: lens, call_bytes: r.bytes, enc_md5: md5(Buffer.concat(r.parts)), flush_len: r.fb.length, flush_md5: md5(r.fb),
                all_md5: md5(r.whole), plain_all_md5: plain_md5, pcm_md5: h.digest('hex') };
    for (const k of ['jointStereo', 'reservoir', 'downmix', 'protect', 'infoTag', 'replayGain']) if (opts[k] !== undefined) o[k] = +opts[k];
    if (opts.quality !== undefined) o.quality = opts.quality;
    /* frames: a CBR stream of whole frames */
    {
        const BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320], BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160];
        const SR = { 3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000] };
        let pos = 0, n = 0;
        while (pos + 4 <= r.whole.length) {
            const hd = r.whole.readUInt32BE(pos);
            if ((hd >>> 21) != 0x7ff) throw new Error(name + ': lost sync at ' + pos);
            const v = (hd >>> 19) & 3, bri = (hd >>> 12) & 15, sri = (hd >>> 10) & 3, pad = (hd >>> 9) & 1;
            if (SR[v][sri] != gp.out_samplerate || (v == 3 ? BR1 : BR2)[bri] != gp.brate) throw new Error(name + ': a frame header disagrees with the resolved rate / bitrate');
            pos += Math.floor((v == 3 ? 144000 : 72000) * gp.brate / gp.out_samplerate) + pad;
            n++;
        }
        if (pos != r.whole.length) throw new Error(name + ': the stream does not end on a frame boundary');
        o.frames = n;
    }
    cases.push(o);
    console.log(name, 'out', gp.out_samplerate, 'lowpass', gp.lowpassfreq, 'brate', gp.brate, 'v', gp.version, 'ratio', g.resample_ratio, 'frames', o.frames, 'bands', o.open_bands, o.all_md5.slice(0, 8), 'plain', String(plain_md5).slice(0, 8));
}
{
    const by = {}; cases.forEach((c) => { by[c.name] = c; });
    if (by.lp12000_uneven_calls.all_md5 != by.lp12000_out44100_128.all_md5 || by.hp500_uneven_calls.all_md5 != by.hp500_128.all_md5) throw new Error('uneven calls change the stream');
    if (by.tag_gain_lp12000_w2000_out44100_128.all_md5 != by.lp12000_w2000_out44100_128.all_md5) throw new Error('the tag case is not the plain stream');
}
fs.writeFileSync(path.join(OUT, 'golden_filters.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_filters.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified modules wired as index.js:73-111; gfp.out_samplerate, lowpassfreq, lowpasswidth, highpassfreq, highpasswidth (and mode, quality, ' +
               'disable_reservoir, error_protection) set before lame_init_params; globals CRC_writeheader (the BitStream\'s own method) and byte (identity) defined, under node ' + process.version, cases }, null, 1));
console.log('wrote', cases.length, 'cases');
}
