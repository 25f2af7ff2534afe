/*
 * TEST TOOL (needs /root/reference): goldens for Float32 PCM input (tests/golden/golden_floatpcm.json).
 *
 * The reference's lame_encode_buffer stores the numbers it is given into a Float32Array and encodes those (Lame.js:1506-1510), so a
 * Float32Array with fractional parts or with values beyond 16 bits is encoded as given.  This generator drives the UNMODIFIED reference --
 * its public Mp3Encoder, and tests/tools/ref_harness.js (unmodified modules, wired as index.js wires them) for joint stereo and the bit
 * reservoir -- with such input.  The oracle takes Int16 only, so these bytes are what pins fractional input.
 *
 * Float PCM comes out bit-identical here and in numpy (tests/pcmformats_cases.py: float_pcm): it is derived from the Int16 corpora of
 * tests/tools/pcm_gen.js by exact dyadic arithmetic on integers, v = (a * K + k) / 2^m with k = (i * 7 + 3) & 15 (left), (i * 5 + 1) & 15
 * (right) -- at most 22 significant bits, no transcendental on the float side:
 *   frac : (a * 16 + k) / 16              Int16 range with fractional parts
 *   unit : (a * 16 + k) / 2^19            the range [-1, 1] (unscaled Web Audio data: analog silence, the ATH paths)
 *   hot  : (a * 16 * M + k) / 16          M = 12 (sine) / 6 (bursts): peaks in (65536, 131072]
 *   ints : a                              integer-valued floats inside the Int16 range
 * usage: node tests/tools/gen_golden_floatpcm.js
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const { refEncoder, refPublic } = require('./ref_harness.js');
const gen = require('./pcm_gen.js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const HOT = { sine: 12, bursts: 6 };

function floatPcm(kind, corpus, a, right) {
    const f = new Float32Array(a.length);
    for (let i = 0; i < a.length; i++) {
        const k = right ? (i * 5 + 1) & 15 : (i * 7 + 3) & 15;
        if (kind == 'frac') f[i] = (a[i] * 16 + k) / 16;
        else if (kind == 'unit') f[i] = (a[i] * 16 + k) / 524288;
        else if (kind == 'hot') f[i] = (a[i] * 16 * HOT[corpus] + k) / 16;
        else f[i] = a[i];
    }
    return f;
}
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);

/* [name, channels, samplerate, kbps, options, corpus, call pattern] */
const ODD = [1, 777, 1151, 1, 2305, 333, 4001, 1, 777, 1153];
const CONFIGS = [
    ['m1_128_mono', 1, 44100, 128, {}, 'sine', 'one'],
    ['m1_128_stereo', 2, 44100, 128, {}, 'bursts', 'calls1152'],
    ['m1_320_stereo', 2, 44100, 320, {}, 'sine', 'odd'],
    ['m1_320_mono', 1, 44100, 320, {}, 'bursts', 'calls1152'],
    ['m1_48k_stereo', 2, 48000, 192, {}, 'bursts', 'odd'],
    ['lsf_mono', 1, 16000, 32, {}, 'sine', 'calls1152'],
    ['resample_int_mono', 1, 44100, 32, {}, 'bursts', 'odd'],
    ['resample_frac_stereo', 2, 44100, 96, { fractionalResample: true }, 'sine', 'calls576'],
    ['joint_stereo', 2, 44100, 128, { jointStereo: true }, 'bursts', 'calls1152'],
    ['reservoir_stereo', 2, 44100, 128, { reservoir: true }, 'sine', 'odd'],
    ['reservoir_mono', 1, 44100, 128, { reservoir: true }, 'bursts', 'calls1152']
];
const N = 14 * 1152;
function callLens(pattern, n) {
    const lens = [];
    if (pattern == 'one') return [n];
    for (let p = 0, i = 0; p < n; i++) {
        let m = pattern == 'calls1152' ? 1152 : pattern == 'calls576' ? 576 : ODD[i % ODD.length];
        if (m > n - p) m = n - p;
        lens.push(m); p += m;
    }
    return lens;
}

const cases = [];
for (const kind of ['frac', 'unit', 'hot', 'ints'])
    for (const [name, ch, sr, kbps, opts, corpus, pattern] of CONFIGS) {
        const [A, B] = gen[corpus](N, ch);
        const L = floatPcm(kind, corpus, A, false), R = ch == 2 ? floatPcm(kind, corpus, B, true) : null;
        const h = crypto.createHash('md5'); h.update(buf(L)); if (R) h.update(buf(R));
        const wrapper = opts.jointStereo || opts.reservoir;
        const enc = wrapper ? refEncoder(ch, sr, kbps, opts) : new (refPublic().Mp3Encoder)(ch, sr, kbps);
        const lens = callLens(pattern, N), parts = [], bytes = [];
        let p = 0, peak = 0;
        for (let i = 0; i < N; i++) peak = Math.max(peak, Math.abs(L[i]), R ? Math.abs(R[i]) : 0);
        for (const m of lens) {
            const b = ch == 2 ? enc.encodeBuffer(L.subarray(p, p + m), R.subarray(p, p + m)) : enc.encodeBuffer(L.subarray(p, p + m));
            p += m;
            bytes.push(b.length); parts.push(Buffer.from(b.buffer, b.byteOffset, b.length));
        }
        const f = enc.flush(), fb = Buffer.from(f.buffer, f.byteOffset, f.length);
        cases.push({ kind, name, channels: ch, samplerate: sr, kbps, joint: opts.jointStereo ? 1 : 0, reservoir: opts.reservoir ? 1 : 0, frac: opts.fractionalResample ? 1 : 0,
                     corpus, pattern, nsamples: N, peak, call_lens: lens, call_bytes: bytes, enc_md5: md5(Buffer.concat(parts)), flush_len: fb.length, flush_md5: md5(fb),
                     all_md5: md5(Buffer.concat(parts.concat([fb]))), pcm_md5: h.digest('hex') });
        console.log(kind, name, 'peak', peak, 'bytes', Buffer.concat(parts).length, '+', fb.length);
    }
fs.writeFileSync(path.join(OUT, 'golden_floatpcm.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_floatpcm.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified (joint / reservoir cases: its modules wired as index.js:73-111 by tests/tools/ref_harness.js), Float32Array input, under node ' + process.version, cases }, null, 1));
console.log('wrote', cases.length, 'cases');
