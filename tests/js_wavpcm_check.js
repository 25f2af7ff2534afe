/*
 * TEST: Mp3Encoder.encodePcm / encodeBatch(..., { format }) / WavHeader.readFormat of lamejs_amd/js beside the LIVE unmodified reference
 * (tests/tools/ref_harness.js), call by call.  The reference is fed Float32Array.from(mapped values): what a caller who widens the samples of a WAV
 * file on the host hands it -- (b - 128) * 256, v / 256, v / 65536, x * 32768.  Families: every format interleaved and planar, one and two channels;
 * encodeBatch with { format }; a { pendingFrames } encoder (same byte STREAM); a refused sample (RangeError, nothing consumed); readFormat on
 * hand-built headers with fmt chunks of 16, 18 and 40 bytes, and on headers it must refuse.
 * usage: node js_wavpcm_check.js [seed]    -> one JSON line
 */
'use strict';
const path = require('path');
const gen = require('./tools/pcm_gen.js');
const { refPublic } = require('./tools/ref_harness.js');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const Ref = refPublic().Mp3Encoder;
const seed = +(process.argv[2] || 20301);
const CALLS = 8;
const res = { families: {}, calls: 0, mismatches: 0, range_errors: 0, headers_ok: 0, headers_refused: 0 };
const eq = (a, b) => a.length == b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) == 0;
const cat = (parts) => Buffer.concat(parts.map((b) => Buffer.from(b.buffer, b.byteOffset, b.length)));
function note(name, ok) { res.calls++; if (!ok) res.mismatches++; const f = res.families[name] || (res.families[name] = { calls: 0, mismatches: 0 }); f.calls++; if (!ok) f.mismatches++; }

const BPS = { u8: 1, s16: 2, s24: 3, s32: 4, f32: 4, f64: 8 };
/* n elements of `format` (a sine plus noise at about a third of full scale, 32-bit and float values with low-order bits that get rounded) -> { bytes, mapped } */
function elements(format, n, s) {
    const u = gen.lcg(s), bytes = Buffer.alloc(n * BPS[format]), mapped = new Float64Array(n);
    for (let i = 0; i < n; i++) {
        const x = 0.3 * Math.sin(2 * Math.PI * 440 * i / 44100) + 0.1 * (2 * u() - 1);
        switch (format) {
            case 'u8': { const b = Math.max(0, Math.min(255, Math.round(128 + 127 * x * 2))); bytes.writeUInt8(b, i); mapped[i] = (b - 128) * 256; break; }
            case 's16': { const v = Math.round(32767 * x); bytes.writeInt16LE(v, 2 * i); mapped[i] = v; break; }
            case 's24': { const v = Math.round(8388607 * x); bytes.writeIntLE(v, 3 * i, 3); mapped[i] = v / 256; break; }
            case 's32': { const v = Math.round(2147483647 * x); bytes.writeInt32LE(v, 4 * i); mapped[i] = v / 65536; break; }
            case 'f32': { const v = Math.fround(x); bytes.writeFloatLE(v, 4 * i); mapped[i] = v * 32768; break; }
            default: { bytes.writeDoubleLE(x, 8 * i); mapped[i] = x * 32768; }
        }
    }
    return { bytes, mapped };
}
function sideBySide(name, format, ch, sr, kbps, inter, opts) {
    const ref = new Ref(ch, sr, kbps), ours = opts ? new lamejs.Mp3Encoder(ch, sr, kbps, opts) : new lamejs.Mp3Encoder(ch, sr, kbps);
    const a = [], b = [];
    for (let c = 0; c < CALLS; c++) {
        const n = opts ? 1152 : [1152, 777, 1153, 2305][c % 4], E = elements(format, n * ch, seed + 31 * c + ch), bps = BPS[format];
        let l, r;
        if (ch == 1) l = Float32Array.from(E.mapped);
        else if (inter) { l = new Float32Array(n); r = new Float32Array(n); for (let i = 0; i < n; i++) { l[i] = E.mapped[2 * i]; r[i] = E.mapped[2 * i + 1]; } }
        else { l = Float32Array.from(E.mapped.subarray(0, n)); r = Float32Array.from(E.mapped.subarray(n)); }
        /* (the bytes at an odd offset of their buffer: packed data lies anywhere) */
        const shifted = Buffer.alloc(E.bytes.length + 1); E.bytes.copy(shifted, 1);
        const u8 = bps % 4 ? shifted.subarray(1) : E.bytes;
        a.push(ch == 2 ? ref.encodeBuffer(l, r) : ref.encodeBuffer(l));
        b.push(ours.encodePcm(u8, format, { interleaved: inter }));
        if (!opts) note(name, eq(a[c], b[c]));
    }
    a.push(ref.flush()); b.push(ours.flush());
    note(name, opts ? Buffer.compare(cat(a), cat(b)) == 0 : eq(a[CALLS], b[CALLS]));
}
for (const format of Object.keys(BPS)) {
    sideBySide(format, format, 2, 44100, 128, true);
    sideBySide(format, format, 2, 44100, 128, false);
    sideBySide(format, format, 1, 44100, 64, true);
}
sideBySide('s24_resample', 's24', 1, 44100, 32, true);
sideBySide('pending', 's24', 2, 44100, 128, true, { pendingFrames: 4 });
sideBySide('pending', 'f64', 2, 44100, 128, false, { pendingFrames: 4 });

/* encodeBatch with { format } */
for (const [format, inter] of [['s24', true], ['s32', false], ['u8', true]]) {
    const NS = [1152 * 3 + 5, 777, 1152 * 2], refs = NS.map(() => new Ref(2, 44100, 128)), encs = NS.map(() => new lamejs.Mp3Encoder(2, 44100, 128));
    const E = NS.map((n, i) => elements(format, 2 * n, seed + 77 + i)), bps = BPS[format];
    const want = NS.map((n, i) => {
        const l = new Float32Array(n), r = new Float32Array(n);
        for (let k = 0; k < n; k++) { l[k] = E[i].mapped[inter ? 2 * k : k]; r[k] = E[i].mapped[inter ? 2 * k + 1 : n + k]; }
        return refs[i].encodeBuffer(l, r);
    });
    const got = inter ? lamejs.encodeBatch(encs, E.map((e) => e.bytes), { interleaved: true, format: format })
        : lamejs.encodeBatch(encs, E.map((e, i) => e.bytes.subarray(0, NS[i] * bps)), E.map((e, i) => e.bytes.subarray(NS[i] * bps)), { format: format });
    NS.forEach((_, i) => note('batch', eq(want[i], got[i])));
    const fl = lamejs.flushBatch(encs);
    NS.forEach((_, i) => note('batch', eq(refs[i].flush(), fl[i])));
}

/* a refused sample: RangeError, nothing consumed */
for (const format of ['f32', 'f64']) {
    const ref = new Ref(2, 44100, 128), ours = new lamejs.Mp3Encoder(2, 44100, 128), a = [], b = [];
    for (let c = 0; c < 4; c++) {
        const E = elements(format, 2 * 1152, seed + 99 + c), l = new Float32Array(1152), r = new Float32Array(1152);
        for (let i = 0; i < 1152; i++) { l[i] = E.mapped[2 * i]; r[i] = E.mapped[2 * i + 1]; }
        if (c == 1 || c == 3) {
            const bad = Buffer.from(E.bytes);
            if (format == 'f32') bad.writeFloatLE(c == 1 ? NaN : 4.5, 4 * 201); else bad.writeDoubleLE(c == 1 ? Infinity : -1e300, 8 * 201);
            try { ours.encodePcm(bad, format); } catch (e) { if (e instanceof RangeError && /channel 1/.test(e.message) && /index 100/.test(e.message)) res.range_errors++; }
        }
        a.push(ref.encodeBuffer(l, r)); b.push(ours.encodePcm(E.bytes, format));
    }
    a.push(ref.flush()); b.push(ours.flush());
    note('refused_sample', Buffer.compare(cat(a), cat(b)) == 0);
}
try { new lamejs.Mp3Encoder(1, 44100, 128).encodePcm(Buffer.alloc(6), 's25'); } catch (e) { if (e instanceof TypeError) res.type_errors = 1; }

/* WavHeader.readFormat on hand-built headers */
function wav(fmtLen, code, bits, ch, sr, sub, extraChunk, dataLen) {
    const parts = [], bps = bits / 8;
    const fmt = Buffer.alloc(8 + fmtLen);
    fmt.write('fmt ', 0); fmt.writeUInt32LE(fmtLen, 4); fmt.writeUInt16LE(code, 8); fmt.writeUInt16LE(ch, 10); fmt.writeUInt32LE(sr, 12);
    fmt.writeUInt32LE(sr * ch * bps, 16); fmt.writeUInt16LE(ch * bps, 20); fmt.writeUInt16LE(bits, 22);
    if (fmtLen == 18) fmt.writeUInt16LE(0, 24);
    if (fmtLen == 40) { fmt.writeUInt16LE(22, 24); fmt.writeUInt16LE(bits, 26); fmt.writeUInt32LE(3, 28); fmt.writeUInt16LE(sub, 32); Buffer.from('000000001000800000aa00389b71', 'hex').copy(fmt, 34); }
    parts.push(fmt);
    if (extraChunk) { const x = Buffer.alloc(8 + 5 + 1); x.write('LIST', 0); x.writeUInt32LE(5, 4); parts.push(x); }      /* odd length: padded to even */
    const d = Buffer.alloc(8 + dataLen); d.write('data', 0); d.writeUInt32LE(dataLen, 4); parts.push(d);
    const body = Buffer.concat(parts), head = Buffer.alloc(12);
    head.write('RIFF', 0); head.writeUInt32LE(4 + body.length, 4); head.write('WAVE', 8);
    const all = Buffer.concat([head, body]);
    return new DataView(all.buffer, all.byteOffset, all.length);
}
const good = [[16, 1, 8, 1, 'u8'], [16, 1, 16, 2, 's16'], [16, 1, 24, 2, 's24'], [18, 1, 32, 2, 's32'], [18, 3, 32, 1, 'f32'], [16, 3, 64, 2, 'f64'], [40, 0xFFFE, 24, 2, 's24', 1], [40, 0xFFFE, 32, 2, 'f32', 3], [40, 0xFFFE, 32, 1, 's32', 1]];
for (const [fmtLen, code, bits, ch, want, sub] of good)
    for (const extra of [false, true]) {
        const w = lamejs.WavHeader.readFormat(wav(fmtLen, code, bits, ch, 48000, sub || 0, extra, 96));
        const off = 12 + 8 + fmtLen + (extra ? 14 : 0) + 8;
        if (w.format == want && w.channels == ch && w.sampleRate == 48000 && w.dataOffset == off && w.dataLen == 96) res.headers_ok++;
    }
for (const dv of [wav(16, 6, 8, 1, 8000, 0, false, 8), wav(16, 1, 12, 1, 8000, 0, false, 8), wav(16, 3, 16, 1, 8000, 0, false, 8), wav(20, 1, 16, 1, 8000, 0, false, 8), wav(40, 0xFFFE, 16, 2, 8000, 7, false, 8),
                  wav(16, 1, 16, 3, 8000, 0, false, 8), wav(18, 0xFFFE, 16, 2, 8000, 1, false, 8)])
    try { lamejs.WavHeader.readFormat(dv); } catch (e) { res.headers_refused++; }
/* an EXTENSIBLE header whose valid bits are fewer than its container's is refused; a data length beyond the view is cut to whole sample frames */
{
    const dv = wav(40, 0xFFFE, 24, 2, 48000, 1, false, 8); dv.setUint16(38, 20, true);
    try { lamejs.WavHeader.readFormat(dv); } catch (e) { res.headers_refused++; }
    const st = wav(16, 1, 24, 2, 48000, 0, false, 100); st.setUint32(40, 0xFFFFFFFF, true);
    const w = lamejs.WavHeader.readFormat(st);
    res.clamped = (w.dataOffset == 44 && w.dataLen == 96) ? 1 : 0;
}
/* { pendingFrames }: the float contract is the library's -- a double above the limit is refused although it would round onto it; nothing is held back of the call */
{
    const ours = new lamejs.Mp3Encoder(1, 44100, 128, { pendingFrames: 4 }), plain = new lamejs.Mp3Encoder(1, 44100, 128);
    const b = Buffer.alloc(8 * 1152); b.writeDoubleLE(4.0000001, 8 * 7);
    res.pending_range_errors = 0;
    for (const e of [ours, plain]) try { e.encodePcm(b, 'f64'); } catch (x) { if (x instanceof RangeError && /index 7/.test(x.message)) res.pending_range_errors++; }
    b.writeDoubleLE(131071.999999999 / 32768, 8 * 7);          /* just below: rounds onto the limit, accepted */
    ours.encodePcm(b, 'f64'); plain.encodePcm(b, 'f64');
    note('pending_limit', Buffer.compare(cat([ours.flush()]), cat([plain.flush()])) == 0);
}
/* readHeader is what it was */
{ const w = lamejs.WavHeader.readHeader(wav(16, 1, 16, 2, 44100, 0, false, 64)); res.read_header_same = (w.channels == 2 && w.sampleRate == 44100 && w.dataOffset == 44 && w.dataLen == 64) ? 1 : 0; }
console.log(JSON.stringify(res));
process.exit(res.mismatches == 0 ? 0 : 1);
