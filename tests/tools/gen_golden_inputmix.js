/*
 * TEST TOOL (needs /root/reference): goldens for the input gains and the stereo-to-mono downmix (tests/golden/golden_inputmix.json).
 *
 * The reference's lame_encode_buffer_sample applies gfp.scale, gfp.scale_left / gfp.scale_right and -- two channels in, MPEGMode.MONO out --
 * the downmix 0.5 * (l + r) (Lame.js:1551-1584).  Its public Mp3Encoder offers none of them, so this generator wires the UNMODIFIED modules
 * itself, as index.js:73-111 does, and sets gfp.mode, gfp.scale, gfp.scale_left and gfp.scale_right before lame_init_params.
 *
 * Streams of 12 frames from the corpora of tests/tools/pcm_gen.js.  Calls: 1152 samples eight times, one call of three frames plus 391
 * samples, flush; the configuration that resamples by a non-integer ratio takes 576-sample calls only.  `kind` f32: Float32Array input with
 * fractional values, v = (a * 16 + k) / 16 as tests/tools/gen_golden_floatpcm.js derives it (bit-identical in numpy).
 * `kind` q20 / even4: Int16 samples shaped so that every value BEHIND gains and mix is a whole number -- l = 20 * floor(l / 20) (then
 * fround(l * 0.95) = 19 k exactly) with r of k's parity; l even and r a multiple of 4 -- which is what lets the Int16-only oracle, fed the
 * premix, be checked against these bytes (tests/inputmix_cases.py).
 * usage: node tests/tools/gen_golden_inputmix.js
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./pcm_gen.js');
const REF = process.env.LAMEJS_REF || '/root/reference';
const S = path.join(REF, 'src', 'js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);

/* opts: { downmix, scale, scaleLeft, scaleRight } -- undefined leaves the field as lame_init leaves it */
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
    const gfp = lame.lame_init();
    gfp.num_channels = channels;
    gfp.in_samplerate = samplerate;
    gfp.brate = kbps;
    gfp.mode = opts.downmix ? MPEGMode.MONO : MPEGMode.STEREO;
    gfp.quality = 3;
    gfp.bWriteVbrTag = false;
    gfp.disable_reservoir = true;
    gfp.write_id3tag_automatic = false;
    if (opts.scale !== undefined) gfp.scale = opts.scale;
    if (opts.scaleLeft !== undefined) gfp.scale_left = opts.scaleLeft;
    if (opts.scaleRight !== undefined) gfp.scale_right = opts.scaleRight;
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

function floatPcm(a, right) {
    const f = new Float32Array(a.length);
    for (let i = 0; i < a.length; i++) f[i] = (a[i] * 16 + (right ? (i * 5 + 1) & 15 : (i * 7 + 3) & 15)) / 16;
    return f;
}

/* [name, channels in, samplerate, kbps, options, corpus, kind] */
const CONFIGS = [
    ['downmix_44100_128_quirk', 2, 44100, 128, { downmix: true }, 'bursts', 's16'],
    ['downmix_44100_320', 2, 44100, 320, { downmix: true }, 'sine', 's16'],
    /* (MPEGMode.MONO raises the lowpass by 1.5, Lame.js:838-885: these two keep their sample rate in a downmix, the two after them resample) */
    ['downmix_48000_64', 2, 48000, 64, { downmix: true }, 'bursts', 's16'],
    ['downmix_44100_96', 2, 44100, 96, { downmix: true, fractionalResample: true }, 'sine', 's16'],
    ['downmix_44100_32_resample_int', 2, 44100, 32, { downmix: true }, 'bursts', 's16'],
    ['downmix_44100_48_resample_frac', 2, 44100, 48, { downmix: true, fractionalResample: true }, 'sine', 's16'],
    ['downmix_16000_32_lsf', 2, 16000, 32, { downmix: true }, 'bursts', 's16'],
    ['downmix_8000_8', 2, 8000, 8, { downmix: true }, 'sine', 's16'],
    ['gains_lr_128', 2, 44100, 128, { scaleLeft: 0.5, scaleRight: 0.25 }, 'bursts', 's16'],
    ['gains_lr_320', 2, 44100, 320, { scaleLeft: 0.5, scaleRight: 0.25 }, 'sine', 's16'],
    ['downmix_flip_left_double_right', 2, 44100, 128, { downmix: true, scaleLeft: -1, scaleRight: 2 }, 'sine', 's16'],
    ['downmix_f32', 2, 44100, 128, { downmix: true }, 'sine', 'f32'],
    ['downmix_gains_f32', 2, 44100, 64, { downmix: true, scale: 0.8, scaleLeft: 1, scaleRight: 0.5 }, 'bursts', 'f32'],
    ['gains_f32', 2, 44100, 128, { scale: 0.8, scaleLeft: 0.5, scaleRight: 0.25 }, 'bursts', 'f32']
];
for (const sc of [0.5, 1, 0, 1.0000005, 4]) for (const ch of [1, 2])
    CONFIGS.push(['scale_' + sc + (ch == 1 ? '_mono' : '_stereo'), ch, 44100, 128, { scale: sc }, ch == 1 ? 'sine' : 'bursts', 's16']);

CONFIGS.push(['whole_downmix_quirk', 2, 44100, 128, { downmix: true }, 'bursts', 'q20']);
CONFIGS.push(['whole_downmix_resample_int', 2, 44100, 32, { downmix: true }, 'sine', 'q20']);
CONFIGS.push(['whole_gains_lr', 2, 44100, 128, { scale: 1, scaleLeft: 0.5, scaleRight: 0.25 }, 'bursts', 'even4']);
CONFIGS.push(['whole_downmix_flip', 2, 44100, 128, { downmix: true, scale: 1, scaleLeft: -1, scaleRight: 2 }, 'sine', 'even4']);
function shape(kind, A, B) {
    const L = new Int16Array(A.length), R = new Int16Array(A.length);
    for (let i = 0; i < A.length; i++) {
        if (kind == 'q20') { const k = Math.floor(A[i] / 20); L[i] = 20 * k; let r = B[i] - ((k + B[i]) & 1); if (r < -32768) r += 2; R[i] = r; }
        else { L[i] = (A[i] >> 2) & ~1; R[i] = (B[i] >> 2) & ~3; }
    }
    return [L, R];
}

const cases = [];
for (const [name, ch, sr, kbps, opts, corpus, kind] of CONFIGS) {
    const lens = name.endsWith('_frac') ? new Array(23).fill(576) : new Array(8).fill(1152).concat([3 * 1152 + 391]);
    const N = lens.reduce((a, b) => a + b, 0);
    const [A, B] = gen[corpus](N, ch);
    const shaped = (kind == 'q20' || kind == 'even4') ? shape(kind, A, B) : null;
    const L = shaped ? shaped[0] : kind == 'f32' ? floatPcm(A, false) : A, R = ch == 2 ? (shaped ? shaped[1] : kind == 'f32' ? floatPcm(B, true) : B) : null;
    const h = crypto.createHash('md5'); h.update(buf(L)); if (R) h.update(buf(R));
    const enc = refEncoder(ch, sr, kbps, opts);
    const parts = [], bytes = [];
    let p = 0;
    for (const m of lens) {
        const b = ch == 2 ? enc.encodeBuffer(L.subarray(p, p + m), R.subarray(p, p + m)) : enc.encodeBuffer(L.subarray(p, p + m));
        p += m;
        bytes.push(b.length); parts.push(Buffer.from(b.buffer, b.byteOffset, b.length));
    }
    const f = enc.flush(), fb = Buffer.from(f.buffer, f.byteOffset, f.length);
    const o = { name, channels: ch, samplerate: sr, kbps, downmix: opts.downmix ? 1 : 0, frac: opts.fractionalResample ? 1 : 0, corpus, kind, nsamples: N,
                ref_scale: enc.gfp.scale, ref_channels_out: enc.gfc.channels_out, out_samplerate: enc.gfp.out_samplerate,
                call_lens: lens, call_bytes: bytes, enc_md5: md5(Buffer.concat(parts)), flush_len: fb.length, flush_md5: md5(fb), pcm_md5: h.digest('hex') };
    for (const k of ['scale', 'scaleLeft', 'scaleRight']) if (opts[k] !== undefined) o[k] = opts[k];
    cases.push(o);
    console.log(name, 'scale', enc.gfp.scale, 'out', enc.gfp.out_samplerate, 'bytes', Buffer.concat(parts).length, '+', fb.length, o.enc_md5.slice(0, 8));
}
fs.writeFileSync(path.join(OUT, 'golden_inputmix.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_inputmix.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified modules wired as index.js:73-111, gfp.mode / scale / scale_left / scale_right set before lame_init_params, under node ' + process.version, cases }, null, 1));
console.log('wrote', cases.length, 'cases');
