/*
 * TEST: lamejs_amd/js with { fractionalResample: true } beside the LIVE unmodified reference (its sources, or oracle/_ref/lame.all.js where
 * they do not exist) on fresh pseudo-random PCM: 8 triples x 20 calls of 576 samples.  Every encodeBuffer() must return the reference's bytes
 * call by call; the flush is compared by the clean / not-clean rule -- frame count, lengths and headers equal, a frame whose input window
 * held no NaN in the reference byte for byte, every other one all zero behind its header.  Also: a call beyond the limit throws and changes
 * nothing, { pendingFrames } is refused, and one encodeBatch over all 8 encoders equals the single calls.
 * usage: node tests/js_fracresample_check.js [seed]        (LAMEJS_HIP_LIB selects the library)
 */
'use strict';
const path = require('path');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js'));
const { hookedRef } = require('./tools/frac_ref.js');
const gen = require('./tools/pcm_gen.js');
const TRIPLES = [[2, 44100, 96], [1, 44100, 48], [2, 48000, 112], [2, 48000, 96], [1, 22050, 16], [2, 32000, 48], [1, 44100, 8], [2, 24000, 48]];
const NCALLS = 20, LEN = 576;
const seed = process.argv[2] ? +process.argv[2] : (Date.now() & 0x7fffffff);
const eq = (a, b) => a.length == b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) == 0;
function noise(n, ch, s) {
    const u = gen.lcg(s), L = new Int16Array(n), R = ch == 2 ? new Int16Array(n) : null;
    for (let i = 0; i < n; i++) { const a = i % 9000 < 2500 ? 14000 : 600; L[i] = Math.round(a * (2 * u() - 1)); if (R) R[i] = Math.round(a * 0.7 * (2 * u() - 1)); }
    return [L, R];
}
let calls = 0, bad = 0, cleanFlush = 0, dirtyFlush = 0, refused = 0;
const batchEnc = [], batchPcm = [], batchWant = [];
TRIPLES.forEach(([ch, sr, kb], ti) => {
    const [L, R] = noise(LEN * NCALLS, ch, seed + 977 * ti);
    const ref = hookedRef(ch, sr, kb), enc = new lamejs.Mp3Encoder(ch, sr, kb, { fractionalResample: true });
    let threw = false;
    try { new lamejs.Mp3Encoder(ch, sr, kb, { fractionalResample: true, pendingFrames: 4 }); } catch (e) { threw = /pendingFrames/.test(e.message); }
    if (!threw) { bad++; console.error('pendingFrames was not refused', ch, sr, kb); }
    const want = [];
    for (let c = 0; c < NCALLS; c++) {
        const l = L.subarray(c * LEN, (c + 1) * LEN), r = R ? R.subarray(c * LEN, (c + 1) * LEN) : undefined;
        if (c == 7) {      /* a call the reference would not consume whole: throws, consumes nothing */
            const n = enc.callLimit() + 200;
            try { enc.encodeBuffer(new Int16Array(n), R ? new Int16Array(n) : undefined); } catch (e) { if (e instanceof RangeError && e.message.includes(String(enc.callLimit()))) refused++; }
        }
        const a = ref.encodeBuffer(l, r), b = enc.encodeBuffer(l, r);
        want.push(a);
        calls++;
        if (!eq(a, b)) { bad++; console.error('encodeBuffer differs', ch, sr, kb, 'call', c, a.length, b.length); }
    }
    if (ref.frames.some((f) => f.nan_in_window)) { bad++; console.error('the reference met NaN before flush()', ch, sr, kb); }
    const nEnc = ref.frames.length;
    ref.flush();
    const ff = ref.frames.slice(nEnc), got = enc.flush();
    let p = 0;
    if (got.length != ff.reduce((s, f) => s + f.bytes, 0)) { bad++; console.error('flush length differs', ch, sr, kb, got.length); }
    else for (const f of ff) {
        const g = Buffer.from(got.buffer, got.byteOffset + p, f.bytes); p += f.bytes;
        if (g.subarray(0, 4).toString('hex') != f.header_hex) { bad++; console.error('flush header differs', ch, sr, kb); }
        if (!f.nan_in_window) { cleanFlush++; if (Buffer.compare(g, f.data) != 0) { bad++; console.error('clean flush frame differs', ch, sr, kb); } }
        else { dirtyFlush++; if (g.subarray(4).some((x) => x != 0)) { bad++; console.error('stand-in frame is not silent', ch, sr, kb); } }
    }
    batchEnc.push(new lamejs.Mp3Encoder(ch, sr, kb, { fractionalResample: true })); batchPcm.push([L, R]); batchWant.push(want);
});
/* one encodeBatch per round over all 8 encoders (8 configurations in one call) == the single calls */
for (let c = 0; c < NCALLS; c++) {
    const outs = lamejs.encodeBatch(batchEnc, batchPcm.map(([L]) => L.subarray(c * LEN, (c + 1) * LEN)), batchPcm.map(([L, R]) => (R || L).subarray(c * LEN, (c + 1) * LEN)));
    outs.forEach((o, i) => { if (!eq(o, batchWant[i][c])) { bad++; console.error('encodeBatch differs', TRIPLES[i], 'call', c); } });
}
console.log(JSON.stringify({ seed, triples: TRIPLES.length, calls, mismatches: bad, clean_flush_frames: cleanFlush, stand_in_flush_frames: dirtyFlush, refused_long_calls: refused }));
process.exit(bad ? 1 : 0);
