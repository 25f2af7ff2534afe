/*
 * TEST: { outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth } of lamejs_amd/js against the goldens of the unmodified reference
 * (tests/golden/golden_filters.json: the five gfp fields set, every case in its own calls), encodeBatch over encoders of different option sets in ONE call
 * (each stream its single-stream bytes) and the RangeErrors.  Where the reference's sources exist (tests/tools/gen_golden_filters.js wires them; the
 * single-file build under oracle/_ref fixes the five fields and is not used) three seeded streams are also encoded beside the LIVE reference, call by call.
 * usage: node js_filters_check.js [seed]    -> one JSON line
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./tools/pcm_gen.js');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const seed = +(process.argv[2] || 20401);
const G = JSON.parse(fs.readFileSync(path.join(__dirname, 'golden', 'golden_filters.json'), 'utf8')).cases;
const res = { families: {}, calls: 0, mismatches: 0, goldens: 0, range_errors: 0, refusals: 0, live: 0 };
const bytes = (b) => Buffer.from(b.buffer, b.byteOffset, b.length);
const cat = (parts) => Buffer.concat(parts.map(bytes));
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
function note(name, ok) { res.calls++; if (!ok) res.mismatches++; const f = res.families[name] || (res.families[name] = { calls: 0, mismatches: 0 }); f.calls++; if (!ok) f.mismatches++; }

function centre(A, B) {
    const L = new Int16Array(A.length), R = new Int16Array(A.length);
    for (let i = 0; i < A.length; i++) { const d = B[i] >> 3; L[i] = Math.max(-32768, Math.min(32767, A[i] + d)); R[i] = Math.max(-32768, Math.min(32767, A[i] - d)); }
    return [L, R];
}
function raw(name, n) { const b = fs.readFileSync(path.join(__dirname, 'golden', name)); return new Int16Array(b.buffer.slice(b.byteOffset, b.byteOffset + 2 * n)); }
/* the corpora of tests/tools/gen_golden_quality.js (the wav excerpt from the committed samples); the md5 of the PCM pins them */
function material(corpus, N, ch, s) {
    if (corpus == 'wavexcerpt') return [raw('left44100_full.s16', N), ch == 2 ? raw('right44100_full.s16', N) : null];
    if (corpus == 'mixed') {
        const [A, B] = gen.bursts(N, 2, s), [CL, CR] = centre(A, B), h = N / 2, L = new Int16Array(N), R = new Int16Array(N);
        L.set(CL.subarray(0, h), 0); R.set(CR.subarray(0, h), 0); L.set(A.subarray(h), h); R.set(B.subarray(h), h);
        return [L, R];
    }
    if (corpus == 'silent3') { const [A, B] = gen.bursts(N, ch, s); A.fill(0, 0, 3 * 1152); if (B) B.fill(0, 0, 3 * 1152); return [A, B || null]; }
    let [L, R] = gen[corpus.replace('centre_', '')](N, ch, s);
    if (corpus.startsWith('centre_')) [L, R] = centre(L, R);
    return [L, R || null];
}
const optsOf = (c) => { const o = Object.assign({}, c.settings); if (c.quality !== undefined) o.quality = c.quality; for (const k of ['jointStereo', 'reservoir', 'downmix', 'protect', 'infoTag', 'replayGain']) if (c[k]) o[k] = true; return o; };
function encodeCalls(enc, ch, L, R, lens) {
    const parts = []; let p = 0;
    for (const m of lens) { parts.push(ch == 2 ? enc.encodeBuffer(L.subarray(p, p + m), R.subarray(p, p + m)) : enc.encodeBuffer(L.subarray(p, p + m))); p += m; }
    return parts;
}

/* every golden in its own calls: byte counts per call (not for the reservoir, whose split into calls is the library's; an { infoTag } stream's placeholder is
 * taken off the front), md5 of the calls' bytes, the flush */
for (const c of G) {
    const [L, R] = material(c.corpus, c.nsamples, c.channels);
    const h = crypto.createHash('md5'); h.update(Buffer.from(L.buffer, L.byteOffset, L.byteLength)); if (R) h.update(Buffer.from(R.buffer, R.byteOffset, R.byteLength));
    note('goldens', h.digest('hex') == c.pcm_md5);
    const enc = new lamejs.Mp3Encoder(c.channels, c.samplerate, c.kbps, optsOf(c));
    let parts = encodeCalls(enc, c.channels, L, R, c.call_lens).map(bytes);
    const fl = enc.flush();
    if (c.infoTag) { const cut = enc.streamInfo().tagBytes, k = parts.findIndex((b) => b.length > 0); parts[k] = parts[k].subarray(cut); note('goldens', cut > 0); }
    note('goldens', md5(Buffer.concat(parts.concat([bytes(fl)]))) == c.all_md5);
    if (!c.reservoir) note('goldens', JSON.stringify(parts.map((b) => b.length)) == JSON.stringify(c.call_bytes) && md5(Buffer.concat(parts)) == c.enc_md5 && md5(bytes(fl)) == c.flush_md5);
    res.goldens++;
}
/* encodeBatch: a plain encoder and four encoders of different option sets -- other filters, another output rate, another MPEG version -- in ONE call,
 * three calls of unequal length, then flushBatch */
{
    const by = {}; G.forEach((c) => { by[c.name] = c; });
    const cs = [by.hp2000_w500_128, by.lp_off_128, by.out22050_44100_128, by.lp12000_w2000_out44100_128];
    const [L, R] = material('bursts', 12 * 1152, 2);
    const encs = [new lamejs.Mp3Encoder(2, 44100, 128)].concat(cs.map((c) => new lamejs.Mp3Encoder(2, 44100, 128, optsOf(c))));
    const out = encs.map(() => []), cuts = [5000, 1152, 7672];          /* sums to 12 * 1152 */
    let p = 0;
    for (const m of cuts) {
        const got = lamejs.encodeBatch(encs, encs.map(() => L.subarray(p, p + m)), encs.map(() => R.subarray(p, p + m)));
        got.forEach((b, i) => out[i].push(b)); p += m;
    }
    lamejs.flushBatch(encs).forEach((b, i) => out[i].push(b));
    note('batch_mixed', md5(cat(out[0])) == cs[0].plain_all_md5);
    cs.forEach((c, i) => note('batch_mixed', md5(cat(out[i + 1])) == c.all_md5));
}
/* beside the live reference, where its sources are here */
{
    const ref = require('./tools/gen_golden_filters.js'), q = require('./tools/gen_golden_quality.js');
    if (fs.existsSync(path.join(q.REF, 'src', 'js', 'Lame.js'))) {
        for (const [ch, sr, kb, o, corpus] of [[2, 44100, 160, { lowpass: 13000, lowpassWidth: 1500, highpass: 700, outSampleRate: 44100 }, 'bursts'],
            [1, 48000, 40, { outSampleRate: 24000, highpass: 600, highpassWidth: 100 }, 'sine'], [2, 32000, 96, { lowpass: -1, jointStereo: true }, 'mixed']]) {
            const per = 1152 * (sr / (o.outSampleRate || sr)) * ((o.outSampleRate || sr) <= 24000 ? 0.5 : 1), n = 9 * per;
            const [L, R] = material(corpus, n, ch, seed + kb), a = ref.refEncoder(ch, sr, kb, o), b = new lamejs.Mp3Encoder(ch, sr, kb, o);
            for (let p = 0; p < n; p += per) {
                const x = ch == 2 ? a.encodeBuffer(L.subarray(p, p + per), R.subarray(p, p + per)) : a.encodeBuffer(L.subarray(p, p + per));
                const y = ch == 2 ? b.encodeBuffer(L.subarray(p, p + per), R.subarray(p, p + per)) : b.encodeBuffer(L.subarray(p, p + per));
                note('live', Buffer.compare(bytes(x), bytes(y)) == 0);
            }
            note('live', Buffer.compare(bytes(a.flush()), bytes(b.flush())) == 0);
            res.live++;
        }
    }
}
/* RangeErrors: wrong types, values outside the rules; an Error (not a RangeError) where the reference's own choice is a non-integer ratio */
const RANGE = [{ lowpass: '12000' }, { lowpass: 0 }, { lowpass: -2 }, { lowpass: 12000.5 }, { lowpass: NaN }, { lowpass: true }, { lowpassWidth: -1 }, { lowpassWidth: '5' }, { highpass: 0 }, { highpass: 100 },
    { highpass: 480 }, { highpass: 17000 }, { highpass: 16000, highpassWidth: 1000 }, { highpassWidth: 100 }, { highpass: 500, highpassWidth: 0.5 }, { outSampleRate: 44000 }, { outSampleRate: 48000 },
    { outSampleRate: 32000 }, { outSampleRate: 32000, fractionalResample: true }, { outSampleRate: '44100' }, { outSampleRate: 22050.5 }, { outSampleRate: false }, { highpass: 12000, lowpass: 12000, outSampleRate: 44100 }];
for (const o of RANGE)
    try { new lamejs.Mp3Encoder(2, 44100, 128, o); } catch (e) { if (e instanceof RangeError) res.range_errors++; }
note('refusals', res.range_errors == RANGE.length);
try { new lamejs.Mp3Encoder(2, 44100, 128, { lowpass: 12000 }); } catch (e) { if (!(e instanceof RangeError) && /non-integer ratio/.test(e.message)) res.refusals++; }
try { new lamejs.Mp3Encoder(2, 44100, 128, { highpass: 481 }).flush(); res.refusals++; } catch (e) { /* 481 Hz is the minimum at 44.1 kHz: accepted */ }
note('refusals', res.refusals == 2);
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 ? 0 : 1);
