/*
 * TEST: { downmix, scale, scaleLeft, scaleRight } of lamejs_amd/js beside the LIVE unmodified reference, call by call.  The reference's public
 * Mp3Encoder offers none of these, so its modules -- from its own single-file build oracle/_ref/lame.all.js, handed out by
 * tests/tools/ref_bundle.js -- are wired here as index.js:73-111 wires them, with gfp.mode = MONO for a downmix and gfp.scale / scale_left /
 * scale_right set before lame_init_params.  Nothing else of the reference is read.
 * Families: downmix (Int16Array, Float32Array with fractions), downmix through encodeInterleaved, per-channel gains on a stereo stream, user
 * scale on a mono stream, encodeBatch over three downmix streams of unequal lengths, a { pendingFrames } downmix encoder (same byte STREAM),
 * { fractionalResample } with a downmix (576-sample calls; flush by length), and the two TypeErrors.
 * usage: node js_inputmix_check.js [seed]    -> one JSON line
 */
'use strict';
const path = require('path');
const gen = require('./tools/pcm_gen.js');
const M = require('./tools/ref_bundle.js').load().__modules;
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const seed = +(process.argv[2] || 20272);
const CALLS = 10;
const res = { families: {}, calls: 0, mismatches: 0, type_errors: 0 };
const bytes = (b) => Buffer.from(b.buffer, b.byteOffset, b.length);
const eq = (a, b) => a.length == b.length && Buffer.compare(bytes(a), bytes(b)) == 0;
const cat = (parts) => Buffer.concat(parts.map(bytes));
function note(name, ok) { res.calls++; if (!ok) res.mismatches++; const f = res.families[name] || (res.families[name] = { calls: 0, mismatches: 0 }); f.calls++; if (!ok) f.mismatches++; }

function refEncoder(channels, samplerate, kbps, opts) {
    function Stub() { this.setModules = function () {}; }
    const lame = new M.Lame(), gaud = new Stub(), ga = new M.GainAnalysis(), bs = new M.BitStream();
    const p = new M.Presets(), qupvt = new M.QuantizePVT(), qu = new M.Quantize(), vbr = new M.VBRTag();
    const ver = new M.Version(), id3 = new Stub(), rv = new M.Reservoir(), tak = new M.Takehiro();
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
    gfp.num_channels = channels; gfp.in_samplerate = samplerate; gfp.brate = kbps;
    gfp.mode = opts.downmix ? M.MPEGMode.MONO : M.MPEGMode.STEREO;
    gfp.quality = 3; gfp.bWriteVbrTag = false; gfp.disable_reservoir = true; gfp.write_id3tag_automatic = false;
    if (opts.scale !== undefined) gfp.scale = opts.scale;
    if (opts.scaleLeft !== undefined) gfp.scale_left = opts.scaleLeft;
    if (opts.scaleRight !== undefined) gfp.scale_right = opts.scaleRight;
    if (lame.lame_init_params(gfp) != 0) throw new Error('lame_init_params failed');
    let cap = 0 | (1.25 * 1152 + 7200), mp3buf = new Int8Array(cap);
    return {
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if ((0 | (1.25 * left.length + 7200)) > cap) { cap = 0 | (1.25 * left.length + 7200); mp3buf = new Int8Array(cap); }
            return new Int8Array(mp3buf.subarray(0, lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, cap)));
        },
        flush() { return new Int8Array(mp3buf.subarray(0, lame.lame_encode_flush(gfp, mp3buf, 0, cap))); }
    };
}

/* sine + noise with fractional parts, as doubles */
function pcm(amp, n, s) {
    const u = gen.lcg(s), L = new Float64Array(n), R = new Float64Array(n);
    for (let i = 0; i < n; i++) {
        L[i] = amp * (0.6 * Math.sin(2 * Math.PI * 440 * i / 44100) + 0.3 * (2 * u() - 1));
        R[i] = amp * (0.5 * Math.sin(2 * Math.PI * 660 * i / 44100 + 0.4) + 0.3 * (2 * u() - 1));
    }
    return [L, R];
}
const cut = (T, A, p, n) => T.from(A.subarray(p, p + n));
function sideBySide(name, ch, sr, kbps, opts, T, amp, s, how, len, flushExact) {
    const n = len || 1152, [L, R] = pcm(amp, n * CALLS, s);
    const ref = refEncoder(ch, sr, kbps, opts), ours = new lamejs.Mp3Encoder(ch, sr, kbps, opts);
    for (let c = 0; c < CALLS; c++) {
        const l = cut(T, L, n * c, n), r = cut(T, R, n * c, n);
        const a = ch == 2 ? ref.encodeBuffer(l, r) : ref.encodeBuffer(l);
        let b;
        if (how == 'interleaved') { const il = new T(2 * n); for (let i = 0; i < n; i++) { il[2 * i] = l[i]; il[2 * i + 1] = r[i]; } b = ours.encodeInterleaved(il); }
        else b = ch == 2 ? ours.encodeBuffer(l, r) : ours.encodeBuffer(l);
        note(name, eq(a, b));
    }
    const fa = ref.flush(), fb = ours.flush();
    note(name, flushExact === false ? fa.length == fb.length : eq(fa, fb));
}

sideBySide('downmix', 2, 44100, 128, { downmix: true }, Int16Array, 20000, seed + 1);
sideBySide('downmix', 2, 44100, 64, { downmix: true, scale: 0.8, scaleLeft: 1, scaleRight: 0.5 }, Float32Array, 30000.5, seed + 2);
sideBySide('downmix', 2, 44100, 320, { downmix: true }, Float32Array, 0.9, seed + 3);
sideBySide('downmix', 2, 44100, 32, { downmix: true, scaleLeft: -1, scaleRight: 2 }, Int16Array, 9000, seed + 4);
sideBySide('downmix_interleaved', 2, 44100, 128, { downmix: true }, Int16Array, 18000, seed + 5, 'interleaved');
sideBySide('downmix_interleaved', 2, 16000, 32, { downmix: true, scaleRight: 0.25 }, Float32Array, 25000.25, seed + 6, 'interleaved');
sideBySide('gains', 2, 44100, 128, { scaleLeft: 0.5, scaleRight: 0.25 }, Int16Array, 22000, seed + 7);
sideBySide('gains', 2, 44100, 192, { scale: 4 }, Float32Array, 8000.5, seed + 8);
sideBySide('gains', 1, 44100, 128, { scale: 0.5, scaleRight: 3 }, Int16Array, 22000, seed + 9);
sideBySide('gains', 2, 44100, 128, { scale: 1.0000005 }, Int16Array, 22000, seed + 10);
sideBySide('fractional', 2, 44100, 48, { downmix: true, fractionalResample: true }, Int16Array, 15000, seed + 11, 'planar', 576, false);

/* encodeBatch: three downmix streams of unequal lengths per round, one launch; then their flushes */
{
    const opts = { downmix: true, scaleRight: 0.5 }, lens = [1152, 2 * 1152 + 7, 777];
    const P = lens.map((n, i) => pcm(12000 + 3000 * i, n * 4, seed + 20 + i)), refs = P.map(() => refEncoder(2, 44100, 128, opts)), encs = P.map(() => new lamejs.Mp3Encoder(2, 44100, 128, opts));
    for (let c = 0; c < 4; c++) {
        const T = c % 2 ? Float32Array : Int16Array;
        const ls = P.map((p, i) => cut(T, p[0], lens[i] * c, lens[i])), rs = P.map((p, i) => cut(T, p[1], lens[i] * c, lens[i]));
        const got = lamejs.encodeBatch(encs, ls, rs);
        refs.forEach((r, i) => note('batch', eq(r.encodeBuffer(ls[i], rs[i]), got[i])));
    }
    const fl = lamejs.flushBatch(encs);
    refs.forEach((r, i) => note('batch', eq(r.flush(), fl[i])));
}
/* { pendingFrames }: the pending buffers hold source samples of both channels; the byte STREAM is the reference's */
{
    const opts = { downmix: true }, [L, R] = pcm(18000, 1152 * CALLS, seed + 30), ref = refEncoder(2, 44100, 128, opts);
    const ours = new lamejs.Mp3Encoder(2, 44100, 128, { downmix: true, pendingFrames: 4 }), a = [], b = [];
    for (let c = 0; c < CALLS; c++) {
        const T = c < 5 ? Int16Array : Float32Array, l = cut(T, L, 1152 * c, 1152), r = cut(T, R, 1152 * c, 1152);
        a.push(ref.encodeBuffer(l, r)); b.push(ours.encodeBuffer(l, r));
    }
    a.push(ref.flush()); b.push(ours.flush());
    note('pending', Buffer.compare(cat(a), cat(b)) == 0);
    res.pending_empty_calls = b.filter((x) => x.length == 0).length;
}
for (const mk of [() => new lamejs.Mp3Encoder(1, 44100, 128, { downmix: true }), () => new lamejs.Mp3Encoder(2, 44100, 128, { downmix: true, jointStereo: true })])
    try { mk(); } catch (e) { if (e instanceof TypeError) res.type_errors++; }
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 ? 0 : 1);
