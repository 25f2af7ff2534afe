/*
 * TEST: the sample types of lamejs_amd/js beside the LIVE unmodified reference (tests/tools/ref_harness.js), call by call.
 * The reference's lame_encode_buffer stores the numbers it is given into a Float32Array and encodes that, so a Float32Array, a Float64Array
 * or a plain Array with fractional values, or with values beyond 16 bits, must give its bytes -- not those of Int16Array.from(input).
 * Families: Float32Array (fractional; beyond 16 bits), Float64Array, Array, Int16Array, encodeInterleaved (Float32Array, Int16Array),
 * encodeBatch with mixed array types and { interleaved: true }, a { pendingFrames } encoder that switches from Int16 to Float32 mid-stream
 * (same byte STREAM), a refused sample (RangeError, nothing consumed), and a refused
 * batch over { pendingFrames } encoders (what they hold back is neither encoded nor lost).
 * usage: node js_pcmformats_check.js [seed]    -> one JSON line
 */
'use strict';
const path = require('path');
const gen = require('./tools/pcm_gen.js');
const { refPublic } = require('./tools/ref_harness.js');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const Ref = refPublic().Mp3Encoder;
const seed = +(process.argv[2] || 20261);
const CALLS = 12, N = 1152 * CALLS;
const res = { families: {}, calls: 0, mismatches: 0, differs_from_int16_coercion: 0 };
const eq = (a, b) => a.length == b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) == 0;
const cat = (parts) => Buffer.concat(parts.map((b) => Buffer.from(b.buffer, b.byteOffset, b.length)));

/* sine + noise at `amp` with fractional parts, as doubles */
function pcm(amp, ch, s) {
    const u = gen.lcg(s), L = new Float64Array(N), R = ch == 2 ? new Float64Array(N) : null;
    for (let i = 0; i < N; i++) {
        L[i] = amp * (0.6 * Math.sin(2 * Math.PI * 440 * i / 44100) + 0.3 * (2 * u() - 1));
        if (R) R[i] = amp * (0.5 * Math.sin(2 * Math.PI * 660 * i / 44100) + 0.3 * (2 * u() - 1));
    }
    return [L, R];
}
function note(name, ok) { res.calls++; if (!ok) res.mismatches++; const f = res.families[name] || (res.families[name] = { calls: 0, mismatches: 0 }); f.calls++; if (!ok) f.mismatches++; }
/* both encoders fed the same arrays call by call (mk: how the call's slice is handed over), flush included */
function sideBySide(name, ch, sr, kbps, L, R, mk, opts) {
    const ref = new Ref(ch, sr, kbps), ours = opts ? new lamejs.Mp3Encoder(ch, sr, kbps, opts) : new lamejs.Mp3Encoder(ch, sr, kbps);
    const coerced = new Ref(ch, sr, kbps);
    let differs = false;
    for (let c = 0; c < CALLS; c++) {
        const l = mk(L, c), r = R ? mk(R, c) : undefined;
        const a = ch == 2 ? ref.encodeBuffer(l, r) : ref.encodeBuffer(l), b = ch == 2 ? ours.encodeBuffer(l, r) : ours.encodeBuffer(l);
        const k = ch == 2 ? coerced.encodeBuffer(Int16Array.from(l), Int16Array.from(r)) : coerced.encodeBuffer(Int16Array.from(l));
        differs = differs || !eq(a, k);
        note(name, eq(a, b));
    }
    note(name, eq(ref.flush(), ours.flush()));
    return differs;
}
const slice = (T) => (A, c) => T.from(A.subarray(1152 * c, 1152 * (c + 1)));
const asArray = (A, c) => Array.from(A.subarray(1152 * c, 1152 * (c + 1)));

for (const amp of [1.0, 20000, 32768, 110000]) {
    const [L, R] = pcm(amp, 2, seed + amp);
    if (sideBySide('Float32Array', 2, 44100, 128, L, R, slice(Float32Array))) res.differs_from_int16_coercion++;
}
{ const [L] = pcm(20000, 1, seed + 1); sideBySide('Float64Array', 1, 44100, 128, L, null, slice(Float64Array)); }
{ const [L, R] = pcm(90000, 2, seed + 2); sideBySide('Array', 2, 48000, 192, L, R, asArray); }
{ const [L, R] = pcm(20000, 2, seed + 3); sideBySide('Int16Array', 2, 44100, 128, L, R, slice(Int16Array)); }
{ const [L] = pcm(30000.5, 1, seed + 4); sideBySide('Float32Array_resample', 1, 44100, 32, L, null, slice(Float32Array)); }
{ const [L, R] = pcm(25000, 2, seed + 5); sideBySide('Float32Array_320kbps', 2, 44100, 320, L, R, slice(Float32Array)); }

/* encodeInterleaved: the reference fed the planes */
for (const T of [Float32Array, Int16Array]) {
    const [L, R] = pcm(21000, 2, seed + 6), ref = new Ref(2, 44100, 128), ours = new lamejs.Mp3Encoder(2, 44100, 128);
    for (let c = 0; c < CALLS; c++) {
        const l = slice(T)(L, c), r = slice(T)(R, c), il = new T(2 * 1152);
        for (let i = 0; i < 1152; i++) { il[2 * i] = l[i]; il[2 * i + 1] = r[i]; }
        note('encodeInterleaved', eq(ref.encodeBuffer(l, r), ours.encodeInterleaved(il)));
    }
    note('encodeInterleaved', eq(ref.flush(), ours.flush()));
}
/* encodeBatch with mixed array types: one launch, every stream the reference's bytes; then { interleaved: true } */
{
    const P = [pcm(15000, 2, seed + 7), pcm(70000, 2, seed + 8), pcm(0.9, 2, seed + 9)], mks = [slice(Int16Array), slice(Float32Array), asArray];
    const refs = P.map(() => new Ref(2, 44100, 128)), encs = P.map(() => new lamejs.Mp3Encoder(2, 44100, 128));
    for (let c = 0; c < CALLS; c++) {
        const ls = P.map((p, i) => mks[i](p[0], c)), rs = P.map((p, i) => mks[i](p[1], c));
        const got = lamejs.encodeBatch(encs, ls, rs);
        refs.forEach((r, i) => note('encodeBatch_mixed', eq(r.encodeBuffer(ls[i], rs[i]), got[i])));
    }
    const fl = lamejs.flushBatch(encs);
    refs.forEach((r, i) => note('encodeBatch_mixed', eq(r.flush(), fl[i])));
    const refs2 = P.map(() => new Ref(2, 44100, 128)), encs2 = P.map(() => new lamejs.Mp3Encoder(2, 44100, 128));
    for (let c = 0; c < CALLS; c++) {
        const ls = P.map((p) => slice(Float32Array)(p[0], c)), rs = P.map((p) => slice(Float32Array)(p[1], c));
        const ils = ls.map((l, i) => { const a = new Float32Array(2304); for (let k = 0; k < 1152; k++) { a[2 * k] = l[k]; a[2 * k + 1] = rs[i][k]; } return a; });
        const got = lamejs.encodeBatch(encs2, ils, null, { interleaved: true });
        refs2.forEach((r, i) => note('encodeBatch_interleaved', eq(r.encodeBuffer(ls[i], rs[i]), got[i])));
    }
}
/* { pendingFrames }: Int16 calls, then Float32 calls: the byte STREAM is the reference's */
{
    const [L, R] = pcm(18000, 2, seed + 10), ref = new Ref(2, 44100, 128), ours = new lamejs.Mp3Encoder(2, 44100, 128, { pendingFrames: 5 });
    const a = [], b = [];
    for (let c = 0; c < CALLS; c++) {
        const T = c < 4 ? Int16Array : Float32Array, l = slice(T)(L, c), r = slice(T)(R, c);
        a.push(ref.encodeBuffer(l, r)); b.push(ours.encodeBuffer(l, r));
    }
    a.push(ref.flush()); b.push(ours.flush());
    note('pendingFrames_switch', Buffer.compare(cat(a), cat(b)) == 0);
    res.pending_nonempty_calls = b.filter((x) => x.length > 0).length;
}
/* a refused sample: RangeError, nothing consumed -- the next calls give the bytes of a run without the bad call */
{
    const [L, R] = pcm(20000, 2, seed + 11), ref = new Ref(2, 44100, 128);
    res.range_errors = 0;
    for (const opts of [undefined, { pendingFrames: 3 }]) {
        const ours = opts ? new lamejs.Mp3Encoder(2, 44100, 128, opts) : new lamejs.Mp3Encoder(2, 44100, 128), a = [], b = [];
        const r2 = new Ref(2, 44100, 128);
        for (let c = 0; c < CALLS; c++) {
            const l = slice(Float32Array)(L, c), r = slice(Float32Array)(R, c);
            if (c == 2 || c == 7) {
                const bad = Float32Array.from(l); bad[100 + c] = c == 2 ? NaN : Infinity;
                try { ours.encodeBuffer(bad, r); } catch (e) { if (e instanceof RangeError && /index 10[27]/.test(e.message)) res.range_errors++; }
            }
            a.push(r2.encodeBuffer(l, r)); b.push(ours.encodeBuffer(l, r));
        }
        a.push(r2.flush()); b.push(ours.flush());
        note('refused_sample', Buffer.compare(cat(a), cat(b)) == 0);
    }
    void ref;
}
/* a refused BATCH over { pendingFrames } encoders: what they hold back must not be encoded (and lost) by the refused call */
{
    const P = [pcm(16000, 2, seed + 12), pcm(17000, 2, seed + 13)], refs = P.map(() => new Ref(2, 44100, 128));
    const encs = P.map(() => new lamejs.Mp3Encoder(2, 44100, 128, { pendingFrames: 4 })), a = P.map(() => []), b = P.map(() => []);
    res.batch_range_errors = 0;
    for (let c = 0; c < CALLS; c++) {
        const ls = P.map((p) => slice(Float32Array)(p[0], c)), rs = P.map((p) => slice(Float32Array)(p[1], c));
        if (c < 6) { P.forEach((_, i) => { a[i].push(refs[i].encodeBuffer(ls[i], rs[i])); b[i].push(encs[i].encodeBuffer(ls[i], rs[i])); }); continue; }      /* (2 frames are held back after call 5) */
        if (c == 6) {
            const bad = Float32Array.from(rs[1]); bad[9] = -Infinity;
            try { lamejs.encodeBatch(encs, ls, [rs[0], bad]); } catch (e) { if (e instanceof RangeError && /stream 1/.test(e.message) && /index 9/.test(e.message)) res.batch_range_errors++; }
        }
        const got = lamejs.encodeBatch(encs, ls, rs);
        P.forEach((_, i) => { a[i].push(refs[i].encodeBuffer(ls[i], rs[i])); b[i].push(got[i]); });
    }
    const fl = lamejs.flushBatch(encs);
    P.forEach((_, i) => { a[i].push(refs[i].flush()); b[i].push(fl[i]); note('refused_batch_pending', Buffer.compare(cat(a[i]), cat(b[i])) == 0); });
}
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 ? 0 : 1);
