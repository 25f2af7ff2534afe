/*
 * TEST: { quality } of lamejs_amd/js against the goldens of the unmodified reference (tests/golden/golden_quality.json: gfp.quality = 7, every case in
 * its own calls), quality 8 as 7, encodeBatch over encoders of both qualities in ONE call (each stream its single-stream bytes), a { pendingFrames }
 * quality-7 encoder (same byte STREAM) and the RangeErrors.  Where the reference's sources exist (tests/tools/gen_golden_quality.js wires them; the
 * single-file build under oracle/_ref fixes quality 3 and is not used) a seeded stream is also encoded beside the LIVE reference, call by call.
 * usage: node js_quality_check.js [seed]    -> one JSON line
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./tools/pcm_gen.js');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const seed = +(process.argv[2] || 20302);
const G = JSON.parse(fs.readFileSync(path.join(__dirname, 'golden', 'golden_quality.json'), 'utf8')).cases;
const res = { families: {}, calls: 0, mismatches: 0, goldens: 0, range_errors: 0, live: 0 };
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
const optsOf = (c) => { const o = { quality: c.quality }; for (const k of ['jointStereo', 'reservoir', 'downmix', 'protect']) if (c[k]) o[k] = true; return o; };
function encodeCalls(enc, ch, L, R, lens) {
    const parts = []; let p = 0;
    for (const m of lens) { parts.push(ch == 2 ? enc.encodeBuffer(L.subarray(p, p + m), R.subarray(p, p + m)) : enc.encodeBuffer(L.subarray(p, p + m))); p += m; }
    return parts;
}

/* every golden in its own calls: byte counts per call (not for the reservoir, whose split into calls is the library's), md5 of the calls' bytes, the flush */
for (const c of G) {
    const [L, R] = material(c.corpus, c.nsamples, c.channels);
    const h = crypto.createHash('md5'); h.update(Buffer.from(L.buffer, L.byteOffset, L.byteLength)); if (R) h.update(Buffer.from(R.buffer, R.byteOffset, R.byteLength));
    note('goldens', h.digest('hex') == c.pcm_md5);
    const enc = new lamejs.Mp3Encoder(c.channels, c.samplerate, c.kbps, optsOf(c));
    const parts = encodeCalls(enc, c.channels, L, R, c.call_lens), fl = enc.flush();
    note(c.quality == 8 ? 'quality8' : 'goldens', md5(Buffer.concat([cat(parts), bytes(fl)])) == c.all_md5);
    if (!c.reservoir) note('goldens', JSON.stringify(parts.map((b) => b.length)) == JSON.stringify(c.call_bytes) && md5(cat(parts)) == c.enc_md5 && md5(bytes(fl)) == c.flush_md5);
    res.goldens++;
}
/* encodeBatch: a quality-3, a quality-7 and a quality-7 joint-stereo encoder in ONE call, three calls of unequal length, then flushBatch */
{
    const by = {}; G.forEach((c) => { by[c.name] = c; });
    const c7 = by.q7_stereo_44100_128, cj = by.q7_joint_mixed_128;
    const [L, R] = material(c7.corpus, c7.nsamples, 2), [JL, JR] = material(cj.corpus, cj.nsamples, 2);
    const mk = () => [new lamejs.Mp3Encoder(2, 44100, 128), new lamejs.Mp3Encoder(2, 44100, 128, { quality: 7 }), new lamejs.Mp3Encoder(2, 44100, 128, { quality: 7, jointStereo: true })];
    const encs = mk(), out = [[], [], []], cuts = [5000, 1152, 7672];          /* three batch calls; sums to 12 * 1152 */
    let p = 0;
    for (const m of cuts) {
        const got = lamejs.encodeBatch(encs, [L.subarray(p, p + m), L.subarray(p, p + m), JL.subarray(p, p + m)], [R.subarray(p, p + m), R.subarray(p, p + m), JR.subarray(p, p + m)]);
        got.forEach((b, i) => out[i].push(b)); p += m;
    }
    lamejs.flushBatch(encs).forEach((b, i) => out[i].push(b));
    note('batch_mixed', md5(cat(out[0])) == c7.q3_all_md5);
    note('batch_mixed', md5(cat(out[1])) == c7.all_md5);
    note('batch_mixed', md5(cat(out[2])) == cj.all_md5);
    /* { pendingFrames }: the byte STREAM is the reference's */
    const pend = new lamejs.Mp3Encoder(2, 44100, 128, { quality: 7, pendingFrames: 4 });
    const parts = encodeCalls(pend, 2, L, R, c7.call_lens); parts.push(pend.flush());
    note('pending', md5(cat(parts)) == c7.all_md5);
}
/* beside the live reference, where its sources are here */
{
    const ref = require('./tools/gen_golden_quality.js');
    if (fs.existsSync(path.join(ref.REF, 'src', 'js', 'Lame.js'))) {
        for (const [ch, sr, kb, o, corpus] of [[2, 44100, 160, { quality: 7 }, 'bursts'], [1, 24000, 40, { quality: 7 }, 'sine'], [2, 32000, 96, { quality: 8, jointStereo: true }, 'mixed']]) {
            const n = 9 * 1152, [L, R] = material(corpus, n, ch, seed + kb), a = ref.refEncoder(ch, sr, kb, o), b = new lamejs.Mp3Encoder(ch, sr, kb, o);
            for (let p = 0; p < n; p += 1152) {
                const x = ch == 2 ? a.encodeBuffer(L.subarray(p, p + 1152), R.subarray(p, p + 1152)) : a.encodeBuffer(L.subarray(p, p + 1152));
                const y = ch == 2 ? b.encodeBuffer(L.subarray(p, p + 1152), R.subarray(p, p + 1152)) : b.encodeBuffer(L.subarray(p, p + 1152));
                note('live', Buffer.compare(bytes(x), bytes(y)) == 0);
            }
            note('live', Buffer.compare(bytes(a.flush()), bytes(b.flush())) == 0);
            res.live++;
        }
    }
}
for (const q of [0, 5, 9, '7', 7.5, true])
    try { new lamejs.Mp3Encoder(2, 44100, 128, { quality: q }); } catch (e) { if (e instanceof RangeError && /3, 7 or 8/.test(e.message)) res.range_errors++; }
note('refusals', res.range_errors == 6);
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 ? 0 : 1);
