/*
 * TEST: { protect, copyright, original, privateBit, emphasis } of lamejs_amd/js beside the LIVE unmodified reference, call by call.  The
 * reference's public Mp3Encoder offers none of these and its CRC path needs two identifiers defined: tests/tools/ref_bundle_protect.js
 * evaluates the reference's own single-file build with them and wires its modules as index.js:73-111 does.
 * Families: protect (stereo, mono, MPEG-2, MPEG-2.5, joint stereo, reservoir, downmix, Float32 input, interleaved), the flag bits alone,
 * everything at once, encodeBatch over protected and unprotected encoders of two configurations in ONE call, a { pendingFrames } protected
 * encoder (same byte STREAM), and the RangeErrors.  Every protected frame of ours is also checked against a bitwise ISO 11172-3 CRC-16.
 * usage: node js_protection_check.js [seed]    -> one JSON line
 */
'use strict';
const path = require('path');
const gen = require('./tools/pcm_gen.js');
const { refEncoder } = require('./tools/ref_bundle_protect.js');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const seed = +(process.argv[2] || 20282);
const CALLS = 8;
const res = { families: {}, calls: 0, mismatches: 0, crc_frames: 0, crc_bad: 0, range_errors: 0 };
const bytes = (b) => Buffer.from(b.buffer, b.byteOffset, b.length);
const eq = (a, b) => a.length == b.length && Buffer.compare(bytes(a), bytes(b)) == 0;
const cat = (parts) => Buffer.concat(parts.map(bytes));
function note(name, ok) { res.calls++; if (!ok) res.mismatches++; const f = res.families[name] || (res.families[name] = { calls: 0, mismatches: 0 }); f.calls++; if (!ok) f.mismatches++; }

function isoCrc(msg) {
    let crc = 0xffff;
    for (const b of msg) for (let i = 7; i >= 0; i--) { const top = ((crc >> 15) & 1) ^ ((b >> i) & 1); crc = (crc << 1) & 0xffff; if (top) crc ^= 0x8005; }
    return crc;
}
/* every frame of a whole stream of OURS: protection bit as asked, stored CRC == ISO CRC */
function checkCrc(mp3, protect, sideinfoLen) {
    const BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320], BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160];
    const SR = { 3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000] };
    let pos = 0;
    while (pos + 6 <= mp3.length) {
        const h = mp3.readUInt32BE(pos), ver = (h >>> 19) & 3;
        if ((h >>> 21) != 0x7ff) { res.crc_bad++; return; }
        if (!((h >>> 16) & 1) != !!protect) res.crc_bad++;
        if (protect) {
            const msg = [mp3[pos + 2], mp3[pos + 3]];
            for (let i = 6; i < sideinfoLen; i++) msg.push(mp3[pos + i]);
            res.crc_frames++;
            if (isoCrc(msg) != mp3.readUInt16BE(pos + 4)) res.crc_bad++;
        }
        pos += Math.floor((ver == 3 ? 144000 : 72000) * (ver == 3 ? BR1 : BR2)[(h >>> 12) & 15] / SR[ver][(h >>> 10) & 3]) + ((h >>> 9) & 1);
    }
    if (pos != mp3.length) res.crc_bad++;
}

/* bursts of noise over a sine, with fractional parts, as doubles */
function pcm(amp, n, s) {
    const u = gen.lcg(s), L = new Float64Array(n), R = new Float64Array(n);
    for (let i = 0; i < n; i++) {
        const g = (i % 5000) >= 3000 && (i % 5000) < 3600 ? 1 : 0.05;
        L[i] = amp * (0.3 * Math.sin(2 * Math.PI * 440 * i / 44100) + g * 0.6 * (2 * u() - 1));
        R[i] = amp * (0.3 * Math.sin(2 * Math.PI * 440 * i / 44100 + 0.1) + g * 0.5 * (2 * u() - 1));
    }
    return [L, R];
}
const cut = (T, A, p, n) => T.from(A.subarray(p, p + n));
function sideBySide(name, ch, sr, kbps, opts, T, amp, s, how, len) {
    const n = len || 1152, [L, R] = pcm(amp, n * CALLS, s);
    const ref = refEncoder(ch, sr, kbps, opts), ours = new lamejs.Mp3Encoder(ch, sr, kbps, opts), mine = [];
    for (let c = 0; c < CALLS; c++) {
        const l = cut(T, L, n * c, n), r = cut(T, R, n * c, n);
        const a = ch == 2 ? ref.encodeBuffer(l, r) : ref.encodeBuffer(l);
        let b;
        if (how == 'interleaved') { const il = new T(2 * n); for (let i = 0; i < n; i++) { il[2 * i] = l[i]; il[2 * i + 1] = r[i]; } b = ours.encodeInterleaved(il); }
        else b = ch == 2 ? ours.encodeBuffer(l, r) : ours.encodeBuffer(l);
        mine.push(b);
        note(name, eq(a, b));
    }
    const fa = ref.flush(), fb = ours.flush();
    mine.push(fb);
    note(name, eq(fa, fb));
    checkCrc(cat(mine), opts.protect, ref.sideinfoLen);
}

const P = { protect: true };
sideBySide('protect', 2, 44100, 128, P, Int16Array, 20000, seed + 1);
sideBySide('protect', 1, 44100, 128, P, Int16Array, 20000, seed + 2);
sideBySide('protect', 2, 48000, 320, P, Float32Array, 25000.5, seed + 3);
sideBySide('protect', 2, 22050, 48, P, Int16Array, 20000, seed + 4, 'interleaved');
sideBySide('protect', 1, 8000, 8, P, Int16Array, 20000, seed + 5, 'planar', 777);
sideBySide('protect', 2, 44100, 48, P, Int16Array, 20000, seed + 6);
sideBySide('protect', 2, 44100, 128, { protect: true, jointStereo: true }, Int16Array, 20000, seed + 7);
sideBySide('protect', 2, 44100, 128, { protect: true, jointStereo: true, reservoir: true }, Int16Array, 20000, seed + 8);
sideBySide('protect', 1, 44100, 64, { protect: true, reservoir: true }, Float32Array, 18000.25, seed + 9, 'planar', 2000);
sideBySide('protect', 2, 44100, 128, { protect: true, downmix: true }, Int16Array, 20000, seed + 10);
sideBySide('flags', 2, 44100, 128, { copyright: true }, Int16Array, 20000, seed + 11);
sideBySide('flags', 1, 44100, 128, { original: false }, Int16Array, 20000, seed + 12);
sideBySide('flags', 2, 22050, 48, { privateBit: true }, Int16Array, 20000, seed + 13);
sideBySide('flags', 1, 8000, 8, { emphasis: 1 }, Int16Array, 20000, seed + 14);
sideBySide('flags', 2, 44100, 192, { emphasis: 3, copyright: true, original: true, privateBit: false }, Int16Array, 20000, seed + 15);
sideBySide('everything', 2, 44100, 128, { protect: true, copyright: true, original: false, privateBit: true, emphasis: 3, jointStereo: true, reservoir: true }, Int16Array, 20000, seed + 16, 'planar', 1500);

/* encodeBatch: protected and unprotected encoders of two configurations in ONE call, unequal lengths; then their flushes */
{
    const cfgs = [[2, 44100, 128, P], [2, 44100, 128, {}], [2, 22050, 48, P], [2, 22050, 48, { copyright: true }], [2, 44100, 128, P]], lens = [1152, 2 * 1152 + 7, 777, 1152, 3000];
    const D = cfgs.map((c, i) => pcm(12000 + 3000 * i, lens[i] * 4, seed + 20 + i)), refs = cfgs.map((c) => refEncoder(c[0], c[1], c[2], c[3])), encs = cfgs.map((c) => new lamejs.Mp3Encoder(c[0], c[1], c[2], c[3]));
    const mine = cfgs.map(() => []);
    for (let c = 0; c < 4; c++) {
        const T = c % 2 ? Float32Array : Int16Array;
        const ls = D.map((p, i) => cut(T, p[0], lens[i] * c, lens[i])), rs = D.map((p, i) => cut(T, p[1], lens[i] * c, lens[i]));
        const got = lamejs.encodeBatch(encs, ls, rs);
        refs.forEach((r, i) => { note('batch_mixed', eq(r.encodeBuffer(ls[i], rs[i]), got[i])); mine[i].push(got[i]); });
    }
    const fl = lamejs.flushBatch(encs);
    refs.forEach((r, i) => { note('batch_mixed', eq(r.flush(), fl[i])); mine[i].push(fl[i]); checkCrc(cat(mine[i]), cfgs[i][3].protect, r.sideinfoLen); });
}
/* { pendingFrames }: the byte STREAM is the reference's */
{
    const [L, R] = pcm(18000, 1152 * CALLS, seed + 30), ref = refEncoder(2, 44100, 128, P);
    const ours = new lamejs.Mp3Encoder(2, 44100, 128, { protect: true, pendingFrames: 4 }), a = [], b = [];
    for (let c = 0; c < CALLS; c++) {
        const l = cut(Int16Array, L, 1152 * c, 1152), r = cut(Int16Array, R, 1152 * c, 1152);
        a.push(ref.encodeBuffer(l, r)); b.push(ours.encodeBuffer(l, r));
    }
    a.push(ref.flush()); b.push(ours.flush());
    note('pending', Buffer.compare(cat(a), cat(b)) == 0);
    checkCrc(cat(b), true, ref.sideinfoLen);
}
for (const o of [{ emphasis: 2 }, { protect: 'yes' }, { copyright: 2 }])
    try { new lamejs.Mp3Encoder(2, 44100, 128, o); } catch (e) { if (e instanceof RangeError) res.range_errors++; }
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 && res.crc_bad == 0 ? 0 : 1);
