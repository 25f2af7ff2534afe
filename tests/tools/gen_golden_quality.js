/*
 * TEST TOOL (needs /root/reference): goldens for the fast encoding mode, quality 7 (tests/golden/golden_quality.json).
 *
 * gfp.quality is a setting of the reference's encoder core that its public Mp3Encoder fixes at 3 (index.js:107), so this generator wires the
 * UNMODIFIED modules itself, as index.js:73-111 does, and sets gfp.quality (with mode, disable_reservoir and error_protection where a case asks)
 * before lame_init_params, whose lame_init_qval resolves the switches (Lame.js:560-690; 8 becomes 7).  tests/tools/ref_harness.js stays as it is.
 * For { protect } the two identifiers the reference's CRC path looks up as globals are supplied as gen_golden_protection.js supplies them.
 *
 * Streams of 12 * 1152 input samples: the corpora of tests/tools/pcm_gen.js, their "centre" variants (L = A + (B >> 3), R = A - (B >> 3)), `mixed`
 * (six frames of the centre variant, then six of independent channels: M/S and L/R frames in one stream), `silent3` (three frames of digital
 * silence in front: granules without energy) and the first samples of the reference's own fixtures testdata/Left44100.wav / Right44100.wav.
 * Every stream is also encoded at quality 3 and must differ from it; the switches lame_init_qval left in gfc are recorded per case.
 * usage: node tests/tools/gen_golden_quality.js          (required as a module it only exports refEncoder and material: tests/js_quality_check.js)
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./pcm_gen.js');
const REF = process.env.LAMEJS_REF || '/root/reference';
const S = path.join(REF, 'src', 'js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);

/* opts: { quality, jointStereo, reservoir, downmix, protect } */
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
    gfp.quality = opts.quality;
    gfp.bWriteVbrTag = false;
    gfp.disable_reservoir = !opts.reservoir;
    gfp.write_id3tag_automatic = false;
    if (opts.protect) gfp.error_protection = 1;
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

/* walk the frames of a whole CBR stream: [frames, frames with mode_ext == 2 (M/S), joint-stereo frames with mode_ext == 0 (L/R)] */
function walk(mp3) {
    const BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320], BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160];
    const SR = { 3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000] };
    let pos = 0, n = 0, ms = 0, lr = 0;
    while (pos + 4 <= mp3.length) {
        const h = mp3.readUInt32BE(pos);
        if ((h >>> 21) != 0x7ff) throw new Error('lost sync at ' + pos);
        const ver = (h >>> 19) & 3, bri = (h >>> 12) & 15, sri = (h >>> 10) & 3, pad = (h >>> 9) & 1, mode = (h >>> 6) & 3, ext = (h >>> 4) & 3;
        if (mode == 1) { if (ext == 2) ms++; else if (ext == 0) lr++; else throw new Error('unexpected mode_ext ' + ext); }
        pos += Math.floor((ver == 3 ? 144000 : 72000) * (ver == 3 ? BR1 : BR2)[bri] / SR[ver][sri]) + pad;
        n++;
    }
    if (pos != mp3.length) throw new Error('stream does not end on a frame boundary');
    return [n, ms, lr];
}

function centre(A, B) {
    const L = new Int16Array(A.length), R = new Int16Array(A.length);
    for (let i = 0; i < A.length; i++) {
        const d = B[i] >> 3;
        L[i] = Math.max(-32768, Math.min(32767, A[i] + d));
        R[i] = Math.max(-32768, Math.min(32767, A[i] - d));
    }
    return [L, R];
}
const WAV = {};
function wav(name) { return WAV[name] || (WAV[name] = gen.readWav(fs.readFileSync(path.join(REF, 'testdata', name))).samples); }
/* the corpora by name (tests/quality_cases.py builds the same arrays; the md5 of the PCM pins them) */
function material(corpus, N, ch) {
    if (corpus == 'wavexcerpt') return [wav('Left44100.wav').slice(0, N), ch == 2 ? wav('Right44100.wav').slice(0, N) : null];
    if (corpus == 'mixed') {
        const [A, B] = gen.bursts(N, 2), [CL, CR] = centre(A, B), h = N / 2;
        const L = new Int16Array(N), R = new Int16Array(N);
        L.set(CL.subarray(0, h), 0); R.set(CR.subarray(0, h), 0); L.set(A.subarray(h), h); R.set(B.subarray(h), h);
        return [L, R];
    }
    if (corpus == 'silent3') {
        const [A, B] = gen.bursts(N, ch), z = 3 * 1152;
        A.fill(0, 0, z); if (B) B.fill(0, 0, z);
        return [A, B || null];
    }
    let [L, R] = gen[corpus.replace('centre_', '')](N, ch);
    if (corpus.startsWith('centre_')) [L, R] = centre(L, R);
    return [L, R || null];
}

const Q7 = { quality: 7 };
const EVEN = new Array(12).fill(1152), UNEVEN = [1, 17, 777, 4096, 4096, 777, 17, 1, 4042];      /* both sum to 12 * 1152 */
/* [name, channels in, samplerate, kbps, options, corpus, call lengths] */
const CONFIGS = [
    ['q7_stereo_44100_128', 2, 44100, 128, Q7, 'bursts', EVEN],
    ['q7_mono_44100_64', 1, 44100, 64, Q7, 'bursts', EVEN],
    ['q7_stereo_48000_320', 2, 48000, 320, Q7, 'bursts', EVEN],
    /* one granule per frame */
    ['q7_stereo_22050_48', 2, 22050, 48, Q7, 'bursts', EVEN],
    ['q7_mono_16000_32', 1, 16000, 32, Q7, 'bursts', EVEN],
    /* the global gain near its upper clamp */
    ['q7_mono_8000_8', 1, 8000, 8, Q7, 'sine', EVEN],
    ['q7_stereo_44100_48_resample_int', 2, 44100, 48, Q7, 'bursts', EVEN],
    ['q7_joint_centre_bursts_128', 2, 44100, 128, { quality: 7, jointStereo: true }, 'centre_bursts', EVEN],
    ['q7_joint_centre_sine_128', 2, 44100, 128, { quality: 7, jointStereo: true }, 'centre_sine', EVEN],
    ['q7_joint_mixed_128', 2, 44100, 128, { quality: 7, jointStereo: true }, 'mixed', EVEN],
    ['q7_resv_mono_128', 1, 44100, 128, { quality: 7, reservoir: true }, 'bursts', EVEN],
    ['q7_resv_stereo_128', 2, 44100, 128, { quality: 7, reservoir: true }, 'bursts', EVEN],
    ['q7_resv_joint_mixed_128', 2, 44100, 128, { quality: 7, reservoir: true, jointStereo: true }, 'mixed', EVEN],
    ['q7_resv_mono_22050_32', 1, 22050, 32, { quality: 7, reservoir: true }, 'sine', EVEN],
    ['q7_downmix_128', 2, 44100, 128, { quality: 7, downmix: true }, 'bursts', EVEN],
    ['q7_protect_128', 2, 44100, 128, { quality: 7, protect: true }, 'bursts', EVEN],
    ['q7_uneven_calls', 2, 44100, 128, Q7, 'bursts', UNEVEN],
    ['q7_joint_uneven_calls', 2, 44100, 128, { quality: 7, jointStereo: true }, 'mixed', UNEVEN],
    ['q7_silent3_stereo_128', 2, 44100, 128, Q7, 'silent3', EVEN],
    ['q7_silent3_mono_22050_32', 1, 22050, 32, Q7, 'silent3', EVEN],
    ['q7_sine_stereo_128', 2, 44100, 128, Q7, 'sine', EVEN],
    ['q7_wavexcerpt_stereo_128', 2, 44100, 128, Q7, 'wavexcerpt', EVEN],
    ['q7_wavexcerpt_mono_64', 1, 44100, 64, Q7, 'wavexcerpt', EVEN],
    ['q7_wavexcerpt_joint_192', 2, 44100, 192, { quality: 7, jointStereo: true }, 'wavexcerpt', EVEN],
    ['q8_stereo_44100_128', 2, 44100, 128, { quality: 8 }, 'bursts', EVEN]
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

module.exports = { refEncoder, material, REF };
if (require.main === module) {
const cases = [];
for (const [name, ch, sr, kbps, opts, corpus, lens] of CONFIGS) {
    const N = lens.reduce((a, b) => a + b, 0);
    if (N != 12 * 1152) throw new Error('call lengths of ' + name);
    const [L, R] = material(corpus, N, ch);
    const h = crypto.createHash('md5'); h.update(buf(L)); if (R) h.update(buf(R));
    const r = run(ch, sr, kbps, opts, L, R, lens), q3 = run(ch, sr, kbps, Object.assign({}, opts, { quality: 3 }), L, R, lens);
    if (Buffer.compare(r.whole, q3.whole) == 0) throw new Error(name + ': the bytes do not differ from quality 3');
    const [frames, ms, lr] = walk(r.whole), g = r.enc.gfc;
    if (r.enc.gfp.quality != 7) throw new Error(name + ': gfp.quality is ' + r.enc.gfp.quality + ' after lame_init_params');
    if (/joint_mixed|joint_uneven/.test(name) && !(ms > 0 && lr > 0)) throw new Error(name + ': M/S ' + ms + ', L/R ' + lr + ' -- both kinds of frame must occur');
    const o = { name, channels: ch, samplerate: sr, kbps, quality: opts.quality, corpus, nsamples: N, ref_channels_out: g.channels_out, out_samplerate: r.enc.gfp.out_samplerate,
                ref_switches: { noise_shaping: g.noise_shaping, noise_shaping_amp: g.noise_shaping_amp, noise_shaping_stop: g.noise_shaping_stop, use_best_huffman: g.use_best_huffman,
                                subblock_gain: g.subblock_gain, psymodel: g.psymodel, full_outer_loop: g.full_outer_loop },
                frames, ms_frames: ms, lr_frames: lr, call_lens: lens, call_bytes: r.bytes, enc_md5: md5(Buffer.concat(r.parts)), flush_len: r.fb.length, flush_md5: md5(r.fb),
                all_md5: md5(r.whole), q3_all_md5: md5(q3.whole), pcm_md5: h.digest('hex') };
    for (const k of ['jointStereo', 'reservoir', 'downmix', 'protect']) if (opts[k] !== undefined) o[k] = +opts[k];
    cases.push(o);
    console.log(name, 'out', o.out_samplerate, 'frames', frames, 'M/S', ms, 'L/R', lr, 'bytes', r.whole.length, o.all_md5.slice(0, 8), 'q3', o.q3_all_md5.slice(0, 8), JSON.stringify(o.ref_switches));
}
{
    const by = {}; cases.forEach((c) => { by[c.name] = c; });
    if (by.q8_stereo_44100_128.all_md5 != by.q7_stereo_44100_128.all_md5) throw new Error('quality 8 is not quality 7');
    if (by.q7_uneven_calls.all_md5 != by.q7_stereo_44100_128.all_md5) throw new Error('uneven calls change the stream');
}
fs.writeFileSync(path.join(OUT, 'golden_quality.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_quality.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified modules wired as index.js:73-111; gfp.quality (and mode, disable_reservoir, error_protection) set before lame_init_params; ' +
               'globals CRC_writeheader (the BitStream\'s own method) and byte (identity) defined, under node ' + process.version, cases }, null, 1));
console.log('wrote', cases.length, 'cases');
}
