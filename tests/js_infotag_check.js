/*
 * TEST: { infoTag } of lamejs_amd/js beside the LIVE unmodified reference (tests/tools/ref_harness.js: its modules wired as index.js:73-111 does,
 * internals exposed).  The reference's tag writer does not run, but the music CRC it keeps while encoding does (BitStream.js:927 ->
 * gfc.nMusicCRC), and so do gfp.frameNum, gfp.encoder_delay and gfp.encoder_padding after the flush: per stream, the audio behind our placeholder
 * is the reference's bytes call by call, and streamInfo() is what the reference holds.  Families: plain (stereo, mono, MPEG-2, Float32 input),
 * joint stereo, reservoir, encodeBatch over tagged beside untagged encoders, a { pendingFrames } tagged encoder (same byte STREAM).  Then a FILE is
 * assembled as INTEGRATION.md says -- the stream written, offset 0 overwritten with infoTagFrame() -- and parsed: every frame header walks to the end
 * of the file, the first frame carries "Info", the frame and byte counts, the music CRC of the bytes behind it (bitwise CRC-16 here) and a tag CRC
 * over the bytes in front of that field.
 * usage: node js_infotag_check.js [seed]    -> one JSON line
 */
'use strict';
const path = require('path');
const gen = require('./tools/pcm_gen.js');
const harness = require('./tools/ref_harness.js');
/* the live reference with its internals: tests/tools/ref_harness.js where the reference's sources are; where only its single-file build is
 * (oracle/_ref/lame.all.js), that build's modules wired the same way (index.js:73-111) -- the harness's own stand-in there hides gfp */
function refEncoder(channels, samplerate, kbps, opts) {
    const r = harness.refEncoder(channels, samplerate, kbps, opts);
    if (r.gfp) return r;
    const M = require('./tools/ref_bundle.js').load().__modules;
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
    gfp.mode = (opts && opts.jointStereo && channels == 2) ? M.MPEGMode.JOINT_STEREO : M.MPEGMode.STEREO;
    gfp.quality = 3; gfp.bWriteVbrTag = false; gfp.disable_reservoir = !(opts && opts.reservoir); gfp.write_id3tag_automatic = false;
    if (lame.lame_init_params(gfp) != 0) throw new Error('lame_init_params failed');
    let cap = 0 | (1.25 * 1152 + 7200), mp3buf = new Int8Array(cap);
    return {
        gfp, gfc: gfp.internal_flags,
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if ((0 | (1.25 * left.length + 7200)) > cap) { cap = 0 | (1.25 * left.length + 7200); mp3buf = new Int8Array(cap); }
            return new Int8Array(mp3buf.subarray(0, lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, cap)));
        },
        flush() { return new Int8Array(mp3buf.subarray(0, lame.lame_encode_flush(gfp, mp3buf, 0, cap))); }
    };
}
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const seed = +(process.argv[2] || 20293);
const CALLS = 8;
const res = { families: {}, calls: 0, mismatches: 0, files: 0, file_bad: 0, refused: 0 };
const bytes = (b) => Buffer.from(b.buffer, b.byteOffset, b.length);
const eq = (a, b) => a.length == b.length && Buffer.compare(bytes(a), bytes(b)) == 0;
const cat = (parts) => Buffer.concat(parts.map(bytes));
function note(name, ok) { res.calls++; if (!ok) res.mismatches++; const f = res.families[name] || (res.families[name] = { calls: 0, mismatches: 0 }); f.calls++; if (!ok) f.mismatches++; }

function crc16(buf) {
    let crc = 0;
    for (const b of buf) { crc ^= b; for (let i = 0; i < 8; i++) crc = (crc & 1) ? (crc >>> 1) ^ 0xA001 : crc >>> 1; }
    return crc;
}
const BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320], BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160];
const SR = { 3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000] };
function frameBytes(h) { const ver = (h >>> 19) & 3; return Math.floor((ver == 3 ? 144000 : 72000) * (ver == 3 ? BR1 : BR2)[(h >>> 12) & 15] / SR[ver][(h >>> 10) & 3]) + ((h >>> 9) & 1); }
/* a file as the documentation assembles it; info: the reference's totals */
function checkFile(file, info) {
    res.files++;
    let pos = 0, frames = 0, bad = 0;
    while (pos + 4 <= file.length) { const h = file.readUInt32BE(pos); if ((h >>> 21) != 0x7ff) { bad++; break; } pos += frameBytes(h); frames++; }
    if (pos != file.length) bad++;
    const h0 = file.readUInt32BE(0), n0 = frameBytes(h0), mpeg1 = ((h0 >>> 19) & 3) == 3, mono = ((h0 >>> 6) & 3) == 3;
    const off = 4 + (mpeg1 ? (mono ? 17 : 32) : (mono ? 9 : 17));
    if (file.toString('ascii', off, off + 4) != 'Info' || file.readUInt32BE(off + 4) != 0xF) bad++;
    if (file.readUInt32BE(off + 8) != info.frames || file.readUInt32BE(off + 8) != frames - 1 || file.readUInt32BE(off + 12) != file.length) bad++;
    const p = off + 116;
    if (file.toString('ascii', p + 4, p + 13) != 'LAME3.98r') bad++;
    const d = (file[p + 25] << 16) | (file[p + 26] << 8) | file[p + 27];
    if ((d >> 12) != info.delay || (d & 0xfff) != Math.floor(info.padding)) bad++;
    if (file.readUInt16BE(p + 36) != info.crc || file.readUInt16BE(p + 36) != crc16(file.subarray(n0))) bad++;
    if (file.readUInt16BE(p + 38) != crc16(file.subarray(0, p + 38))) bad++;
    if (bad) res.file_bad++;
}

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
const refInfo = (ref) => ({ frames: ref.gfp.frameNum, crc: ref.gfc.nMusicCRC, delay: ref.gfp.encoder_delay, padding: ref.gfp.encoder_padding });
function sameInfo(si, ref, nbytes) {
    const r = refInfo(ref);
    return si.frames == r.frames && si.musicCrc == r.crc && si.delay == r.delay && si.padding == Math.floor(r.padding) && si.audioBytes == nbytes;
}
function sideBySide(name, ch, sr, kbps, opts, T, amp, s, len) {
    const n = len || 1152, [L, R] = pcm(amp, n * CALLS, s);
    const ref = refEncoder(ch, sr, kbps, opts), ours = new lamejs.Mp3Encoder(ch, sr, kbps, Object.assign({ infoTag: true }, opts)), mine = [];
    const nt = ours.streamInfo().tagBytes;
    let total = 0;
    for (let c = 0; c < CALLS; c++) {
        const l = cut(T, L, n * c, n), r = cut(T, R, n * c, n);
        const a = ch == 2 ? ref.encodeBuffer(l, r) : ref.encodeBuffer(l);
        let b = ch == 2 ? ours.encodeBuffer(l, r) : ours.encodeBuffer(l);
        mine.push(b);
        if (c == 0) b = b.subarray(nt);                    /* the placeholder goes out with the first call */
        total += a.length;
        note(name, opts.reservoir ? true : eq(a, b));      /* (with the reservoir only the stream is the reference's, not its split into calls) */
    }
    const fa = ref.flush(), fb = ours.flush();
    mine.push(fb);
    total += fa.length;
    const si = ours.streamInfo();
    note(name, sameInfo(si, ref, total) && cat(mine).length == total + nt);
    const file = Buffer.from(cat(mine));
    bytes(ours.infoTagFrame()).copy(file, 0);
    checkFile(file, refInfo(ref));
}

sideBySide('plain', 2, 44100, 128, {}, Int16Array, 20000, seed + 1);
sideBySide('plain', 1, 44100, 128, {}, Int16Array, 20000, seed + 2);
sideBySide('plain', 2, 48000, 320, {}, Float32Array, 25000.5, seed + 3);
sideBySide('plain', 2, 22050, 64, {}, Int16Array, 20000, seed + 4, 777);
sideBySide('plain', 1, 8000, 24, {}, Int16Array, 20000, seed + 5, 100);
sideBySide('joint', 2, 44100, 128, { jointStereo: true }, Int16Array, 20000, seed + 6);
sideBySide('reservoir', 2, 44100, 128, { reservoir: true }, Int16Array, 20000, seed + 7);
sideBySide('reservoir', 2, 44100, 128, { jointStereo: true, reservoir: true }, Int16Array, 20000, seed + 8, 5000);

/* encodeBatch: tagged beside untagged encoders in ONE call, unequal lengths; then their flushes */
{
    const tagged = [true, false, true], lens = [1152, 2 * 1152 + 7, 3000];
    const D = lens.map((n, i) => pcm(12000 + 3000 * i, n * 4, seed + 20 + i)), refs = lens.map(() => refEncoder(2, 44100, 128, {}));
    const encs = tagged.map((t) => new lamejs.Mp3Encoder(2, 44100, 128, t ? { infoTag: true } : {}));
    const mine = lens.map(() => []), totals = lens.map(() => 0);
    for (let c = 0; c < 4; c++) {
        const ls = D.map((p, i) => cut(Int16Array, p[0], lens[i] * c, lens[i])), rs = D.map((p, i) => cut(Int16Array, p[1], lens[i] * c, lens[i]));
        const got = lamejs.encodeBatch(encs, ls, rs);
        refs.forEach((r, i) => { const a = r.encodeBuffer(ls[i], rs[i]); totals[i] += a.length; mine[i].push(got[i]); note('batch_mixed', eq(a, tagged[i] && c == 0 ? got[i].subarray(417) : got[i])); });
    }
    const fl = lamejs.flushBatch(encs);
    refs.forEach((r, i) => {
        const a = r.flush(); totals[i] += a.length; mine[i].push(fl[i]);
        note('batch_mixed', eq(a, fl[i]));
        if (!tagged[i]) return;
        note('batch_mixed', sameInfo(encs[i].streamInfo(), r, totals[i]));
        const file = Buffer.from(cat(mine[i])); bytes(encs[i].infoTagFrame()).copy(file, 0); checkFile(file, refInfo(r));
    });
}
/* { pendingFrames }: the byte STREAM is the reference's behind the placeholder */
{
    const [L, R] = pcm(18000, 1152 * CALLS, seed + 30), ref = refEncoder(2, 44100, 128, {});
    const ours = new lamejs.Mp3Encoder(2, 44100, 128, { infoTag: true, pendingFrames: 4 }), a = [], b = [];
    for (let c = 0; c < CALLS; c++) {
        const l = cut(Int16Array, L, 1152 * c, 1152), r = cut(Int16Array, R, 1152 * c, 1152);
        a.push(ref.encodeBuffer(l, r)); b.push(ours.encodeBuffer(l, r));
    }
    a.push(ref.flush()); b.push(ours.flush());
    note('pending', Buffer.compare(cat(a), cat(b).subarray(417)) == 0 && sameInfo(ours.streamInfo(), ref, cat(a).length));
    const file = Buffer.from(cat(b)); bytes(ours.infoTagFrame()).copy(file, 0); checkFile(file, refInfo(ref));
}
for (const c of [[1, 8000, 8, { infoTag: true }], [2, 22050, 32, { infoTag: true, fractionalResample: true }]])
    try { new lamejs.Mp3Encoder(c[0], c[1], c[2], c[3]); } catch (e) { if (/Info tag/.test(e.message)) res.refused++; }
try { const e = new lamejs.Mp3Encoder(2, 44100, 128, { infoTag: true }); e.infoTagFrame(); } catch (e) { if (/not been flushed/.test(e.message)) res.refused++; }
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 && res.file_bad == 0 ? 0 : 1);
