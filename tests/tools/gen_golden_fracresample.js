/*
 * TEST TOOL (needs the reference): goldens for the { fractionalResample } extension -- the 49 (channels, sample rate, kbps) triples the
 * reference resamples by a non-integer ratio, fed in calls it consumes whole.  The UNMODIFIED reference runs (tests/tools/frac_ref.js: a hook
 * on lame_encode_mp3_frame that only looks); per case the generator records the call lengths, per call the output-rate samples the
 * resampler delivered (k) and the bytes returned, the md5 of all encodeBuffer() returns, and per flush frame its length, header, md5 and
 * whether NaN lay in its input window.
 * Two CONDITIONS, not measurements -- a case that violates one is not written and the generator fails: the reference shows no NaN before
 * flush(), and the first flush frame's window is NaN-free.
 * Cases: all 49 triples x 576-sample calls; the 23 triples profiles/r03_reference_noninteger_resample.txt marks "never" x 1152-sample calls;
 * six triples x both corpora with two odd call lengths in [577, limit] mixed within one stream; per distinct ratio one "bad call" case: a
 * call of limit + 200 samples after three good ones -- the reference turns fractional there (NaN in its buffer within the next two calls,
 * verified), lamejs_amd must refuse it and leave the stream untouched: the expected bytes come from a reference run WITHOUT that call.
 * Output: tests/golden/golden_fracresample.json.    usage: node tests/tools/gen_golden_fracresample.js
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const { hookedRef, fractionalTriples } = require('./frac_ref.js');
const gen = require('./pcm_gen.js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
function pcmMd5(L, R) { const h = crypto.createHash('md5'); h.update(Buffer.from(L.buffer, L.byteOffset, L.byteLength)); if (R) h.update(Buffer.from(R.buffer, R.byteOffset, R.byteLength)); return h.digest('hex'); }

/* one reference run over the given call lengths; `skip`: index of a call that is NOT made (its samples are passed over) */
function run(t, corpus, lens, skip, withFlush) {
    const total = lens.reduce((a, b) => a + b, 0);
    const [L, R] = gen[corpus](total, t.ch);
    const e = hookedRef(t.ch, t.sr, t.kb);
    const parts = [], call_bytes = [], call_k = [];
    let p = 0, nanAt = -1;
    lens.forEach((n, c) => {
        if (c !== skip) {
            const mf0 = e.gfc.mf_size, f0 = e.frames.length;
            const o = e.encodeBuffer(L.subarray(p, p + n), R ? R.subarray(p, p + n) : undefined);
            parts.push(Buffer.from(o.buffer, o.byteOffset, o.length));
            call_bytes.push(o.length);
            call_k.push(e.gfc.mf_size - mf0 + e.gfp.framesize * (e.frames.length - f0));
            if (e.frames.length - f0 > 1 && skip !== -2) throw new Error('a call completed more than one frame');
            if (nanAt < 0 && (e.nanBuffered() || e.frames.some((f) => f.nan_in_window))) nanAt = c;
        }
        p += n;
    });
    const nEnc = e.frames.length;
    let flush = null;
    if (withFlush) {
        const f = e.flush();
        flush = e.frames.slice(nEnc).map((fr) => ({ bytes: fr.bytes, header_hex: fr.header_hex, nan_in_window: fr.nan_in_window, md5: fr.md5 }));
        if (f.length != flush.reduce((a, fr) => a + fr.bytes, 0)) throw new Error('flush(): the frames do not add up to the returned bytes');
    }
    const enc = Buffer.concat(parts);
    return { L, R, total, enc_md5: md5(enc), enc_len: enc.length, call_bytes, call_k, nanAt, flush };
}

const triples = fractionalTriples();
if (triples.length != 49) throw new Error('expected 49 non-integer-resample triples, found ' + triples.length);
const never = new Set(fs.readFileSync(path.join(__dirname, '..', '..', 'profiles', 'r03_reference_noninteger_resample.txt'), 'utf8').split('\n')
    .filter((l) => /^\d/.test(l) && l.split('|')[1].trim() == 'never, 0').map((l) => { const m = l.trim().split(/\s+/); return m[0] + ' ' + m[1] + ' ' + m[2]; }));
if (never.size != 23) throw new Error('expected 23 "never" triples, found ' + never.size);

const cases = [];
let cleanFlush = 0, allFlush = 0;
/* `lensOf(n)`: the call lengths of the case with n calls.  Whether the first flush frame is clean depends on where the stream stands when
 * flush() comes (its first bunch of zeros may be longer than the reference's input buffer, which is as long as the largest call): the case
 * takes the smallest number of calls >= 12 for which both conditions hold, and there must be one below 24. */
function add(kind, t, corpus, lensOf, extra) {
    let r = null, lens = null;
    for (let n = 12; n < 24; n++) {
        lens = lensOf(n);
        r = run(t, corpus, lens, -1, true);
        if (r.nanAt >= 0) throw new Error(`CONDITION violated: NaN before flush() in ${t.ch} ${t.sr} ${t.kb} ${kind} (call ${r.nanAt})`);
        if (r.flush.length && !r.flush[0].nan_in_window) break;
        r = null;
    }
    if (!r) throw new Error(`CONDITION violated: first flush frame not clean in ${t.ch} ${t.sr} ${t.kb} ${kind} for any of 12 .. 23 calls`);
    allFlush += r.flush.length; cleanFlush += r.flush.filter((f) => !f.nan_in_window).length;
    cases.push(Object.assign({ kind, channels: t.ch, samplerate: t.sr, kbps: t.kb, out_samplerate: t.out, call_limit: t.limit, corpus, nsamples: r.total, pcm_md5: pcmMd5(r.L, r.R),
        call_lens: lens, call_k: r.call_k, call_bytes: r.call_bytes, enc_md5: r.enc_md5, enc_len: r.enc_len, flush: r.flush }, extra || {}));
}
triples.forEach((t, i) => add('calls576', t, i % 2 ? 'bursts' : 'sine', (n) => Array(n).fill(576)));
triples.filter((t) => never.has(t.ch + ' ' + t.sr + ' ' + t.kb)).forEach((t, i) => add('calls1152', t, i % 2 ? 'sine' : 'bursts', (n) => Array(n).fill(1152)));
/* one triple per distinct (ratio, frame size): the first of each */
const perRatio = [];
for (const t of triples) if (!perRatio.some((u) => u.ratio == t.ratio)) perRatio.push(t);
const oddSix = [[2, 44100, 96], [2, 48000, 112], [1, 48000, 48], [1, 22050, 16], [2, 32000, 48], [1, 44100, 8]].map(([ch, sr, kb]) => triples.find((t) => t.ch == ch && t.sr == sr && t.kb == kb));
for (const t of oddSix) for (const corpus of ['sine', 'bursts']) {
    const a = 577 + 2 * Math.floor((t.limit - 577) / 6), b = t.limit - (t.limit % 2 ? 0 : 1);
    add('odd', t, corpus, (n) => { const lens = []; for (let i = 0; i < n; i++) lens.push([a, b, b, a, 577, b][i % 6]); return lens; });
}
for (const t of perRatio) {
    const good = 576, bad = t.limit + 200;
    let r = null, w = null, lens = null;
    for (let n = 10; n < 22 && !r; n++) {      /* (the number of calls by the same rule as in add()) */
        lens = Array(n).fill(good); lens[3] = bad;
        w = run(t, 'sine', lens, -2, false);      /* (-2: every call is made, and the long one may complete several frames) */
        if (!(w.nanAt >= 3 && w.nanAt <= 5)) throw new Error(`bad-call case ${t.ch} ${t.sr} ${t.kb}: the reference shows NaN at call ${w.nanAt}, expected within two calls of the long one`);
        r = run(t, 'sine', lens, 3, true);
        if (r.nanAt >= 0) throw new Error('CONDITION violated: NaN before flush() in the run without the long call');
        if (r.flush[0].nan_in_window) r = null;
    }
    if (!r) throw new Error('CONDITION violated: first flush frame not clean (bad-call case)');
    allFlush += r.flush.length; cleanFlush += r.flush.filter((f) => !f.nan_in_window).length;
    cases.push({ kind: 'badcall', channels: t.ch, samplerate: t.sr, kbps: t.kb, out_samplerate: t.out, call_limit: t.limit, corpus: 'sine', nsamples: r.total, pcm_md5: pcmMd5(r.L, r.R),
        call_lens: lens, bad_call: 3, reference_nan_at_call: w.nanAt, note: 'reference turns fractional here', call_k: r.call_k, call_bytes: r.call_bytes, enc_md5: r.enc_md5, enc_len: r.enc_len, flush: r.flush });
}
fs.writeFileSync(path.join(OUT, 'golden_fracresample.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_fracresample.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified, modules wired as index.js:73-111, under node ' + process.version,
    ratios: perRatio.length, flush_frames: allFlush, flush_frames_clean: cleanFlush, cases }));
console.log('wrote', cases.length, 'cases (' + perRatio.length + ' distinct ratios);', cleanFlush, 'of', allFlush, 'flush frames are clean');
