/*
 * TEST: { replayGain } of lamejs_amd/js against tests/golden/golden_replaygain.json (recorded from the live reference by tests/tools/gen_golden_replaygain.js).
 * Per golden case -- calls of 1152 samples, flushed -- replayGain() reports the reference's windows and samples, and its RadioGain as tenthDb where the case is
 * margin_ok (within one tenth of a dB elsewhere: a window may sit one histogram step from the reference's).  Then: the same stream as one call; two encoders of
 * different lengths through encodeBatch / flushBatch; a { pendingFrames } encoder; the Info tag's radio field with and without the option; the refusals.
 * usage: node js_replaygain_check.js    -> one JSON line
 */
'use strict';
const fs = require('fs'), path = require('path');
const gen = require('./tools/pcm_gen.js');
const lamejs = require(path.join(__dirname, '..', 'lamejs_amd', 'js', 'index.js'));
const G = JSON.parse(fs.readFileSync(path.join(__dirname, 'golden', 'golden_replaygain.json'), 'utf8'));
const res = { cases: 0, mismatches: 0, exact_tenth: 0, cut_same: 0, batch_same: 0, pending_same: 0, tag_fields: 0, refused: 0, notes: [] };
const bad = (what) => { res.mismatches++; res.notes.push(what); };
const byName = (n) => G.cases.find((c) => c.name == n);
const optsOf = (c, more) => Object.assign({ replayGain: true }, c.downmix ? { downmix: true } : {}, c.jointStereo ? { jointStereo: true } : {}, c.reservoir ? { reservoir: true } : {}, more || {});
const same = (a, b) => a.tenthDb === b.tenthDb && a.windows === b.windows && a.samples === b.samples;
function run(c, call, more) {
    const [L, R] = gen[c.corpus](c.nsamples, c.channels);
    const enc = new lamejs.Mp3Encoder(c.channels, c.samplerate, c.kbps, optsOf(c, more));
    const parts = [];
    for (let p = 0; p < c.nsamples; p += call) parts.push(c.channels == 2 ? enc.encodeBuffer(L.subarray(p, p + call), R.subarray(p, p + call)) : enc.encodeBuffer(L.subarray(p, p + call)));
    parts.push(enc.flush());
    return { enc, gain: enc.replayGain(), bytes: Buffer.concat(parts.map((b) => Buffer.from(b.buffer, b.byteOffset, b.length))) };
}

const NAMES = ['mono_48000_64', 'stereo_48000_128', 'resample_48000_24000_stereo_64', 'downmix_48000_96', 'stereo_16000_48_mpeg2', 'mono_8000_16_mpeg25'];
const first = {};
for (const name of NAMES) {
    const c = byName(name), r = run(c, 1152);
    res.cases++;
    first[name] = r;
    if (r.gain.windows != c.windows || r.gain.samples != c.fed) bad(name + ': windows / samples ' + JSON.stringify(r.gain));
    if (r.gain.tenthDb === c.RadioGain) res.exact_tenth++;
    else if (c.margin_ok || Math.abs(r.gain.tenthDb - c.RadioGain) > 1) bad(name + ': tenthDb ' + r.gain.tenthDb + ', reference ' + c.RadioGain);
}
/* one call */
for (const name of NAMES.slice(1, 4)) {
    const c = byName(name), r = run(c, c.nsamples);
    if (same(r.gain, first[name].gain) && Buffer.compare(r.bytes, first[name].bytes) == 0) res.cut_same++; else bad(name + ': one call differs');
}
/* a batch of two streams of different lengths */
{
    const c = byName('stereo_48000_128'), [L, R] = gen[c.corpus](c.nsamples, 2), M = c.nsamples - 3 * 1152 - 77;
    const a = new lamejs.Mp3Encoder(2, c.samplerate, c.kbps, optsOf(c)), b = new lamejs.Mp3Encoder(2, c.samplerate, c.kbps, optsOf(c));
    lamejs.encodeBatch([a, b], [L, L.subarray(0, M)], [R, R.subarray(0, M)]);
    lamejs.flushBatch([a, b]);
    const solo = new lamejs.Mp3Encoder(2, c.samplerate, c.kbps, optsOf(c));
    solo.encodeBuffer(L.subarray(0, M), R.subarray(0, M)); solo.flush();
    if (same(a.replayGain(), first[c.name].gain) && same(b.replayGain(), solo.replayGain()) && b.replayGain().samples < a.replayGain().samples) res.batch_same++; else bad('batch differs');
}
/* { pendingFrames }: the samples reach the library in other pieces */
{
    const c = byName('stereo_16000_48_mpeg2'), r = run(c, 1152, { pendingFrames: 4 });
    if (same(r.gain, first[c.name].gain) && Buffer.compare(r.bytes, first[c.name].bytes) == 0) res.pending_same++; else bad('pendingFrames differs');
}
/* the tag's radio field */
{
    const c = byName('stereo_48000_128');
    const radio = (frame) => {
        const f = Buffer.from(frame.buffer, frame.byteOffset, frame.length), off = 4 + 32 + 116 + 19;       /* MPEG-1, two channels, unprotected */
        return { peak: f.readUInt32BE(off - 4), radio: f.readUInt16BE(off), audiophile: f.readUInt16BE(off + 2) };
    };
    const w = run(c, 1152, { infoTag: true }), t = radio(w.enc.infoTagFrame()), g = w.gain.tenthDb;
    const want = 0x2000 | 0x0C00 | (g < 0 ? 0x200 : 0) | Math.min(Math.abs(g), 0x1FE);
    if (t.radio == want && t.peak == 0 && t.audiophile == 0 && same(w.gain, first[c.name].gain)) res.tag_fields++; else bad('tag radio field ' + JSON.stringify(t) + ' want ' + want);
    const [L, R] = gen[c.corpus](c.nsamples, 2), plain = new lamejs.Mp3Encoder(2, c.samplerate, c.kbps, { infoTag: true });
    plain.encodeBuffer(L, R); plain.flush();
    const t0 = radio(plain.infoTagFrame());
    if (t0.radio == 0 && t0.peak == 0 && t0.audiophile == 0) res.tag_fields++; else bad('tag without the option ' + JSON.stringify(t0));
    try { plain.replayGain(); bad('replayGain() without the option did not throw'); } catch (e) { if (/replayGain option/.test(e.message)) res.refused++; else bad(e.message); }
}
try { new lamejs.Mp3Encoder(2, 22050, 32, { fractionalResample: true, replayGain: true }); bad('fractionalResample + replayGain was accepted'); }
catch (e) { if (/ReplayGain cannot be combined with fractionalResample/.test(e.message)) res.refused++; else bad(e.message); }
{
    const enc = new lamejs.Mp3Encoder(2, 44100, 128, { replayGain: true });
    enc.setState(enc.getState());
    try { enc.replayGain(); bad('replayGain() after setState did not throw'); } catch (e) { if (/moved/.test(e.message)) res.refused++; else bad(e.message); }
}
console.log(JSON.stringify(res));
process.exit(res.mismatches ? 1 : 0);
