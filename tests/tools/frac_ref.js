/*
 * TEST INFRASTRUCTURE: the UNMODIFIED reference with a hook on Encoder.lame_encode_mp3_frame, for the configurations it resamples by a
 * non-integer ratio (extension { fractionalResample } of lamejs_amd).  The reference's own code runs; the hook only LOOKS: per frame it
 * scans the frame's input window -- mfbuf[ch][0 .. mf_needed), everything the psychoacoustic model and the filterbank of that frame read --
 * for NaN and records the bytes the frame came out as.  Works from the reference's sources where they exist and from its single-file build
 * (oracle/_ref/lame.all.js, tests/tools/ref_bundle.js) where they do not.
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const harness = require('./ref_harness.js');

function wireFromBundle(channels, samplerate, kbps) {
    const M = require('./ref_bundle.js').load().__modules;
    function Stub() { this.setModules = function () {}; }
    const lame = new M.Lame(), gaud = new Stub(), ga = new M.GainAnalysis(), bs = new M.BitStream();
    const p = new M.Presets(), qupvt = new M.QuantizePVT(), qu = new M.Quantize(), vbr = new M.VBRTag();
    const ver = new M.Version(), id3 = new Stub(), rv = new M.Reservoir(), tak = new M.Takehiro();
    const parse = new Stub(), mpg = {};
    lame.setModules(ga, bs, p, qupvt, qu, vbr, ver, id3, mpg);
    bs.setModules(ga, mpg, ver, vbr); id3.setModules(bs, ver); p.setModules(lame); qu.setModules(bs, rv, qupvt, tak);
    qupvt.setModules(tak, rv, lame.enc.psy); rv.setModules(bs); tak.setModules(qupvt); vbr.setModules(lame, bs, ver);
    gaud.setModules(parse, mpg); parse.setModules(ver, id3, p);
    const gfp = lame.lame_init();
    gfp.num_channels = channels; gfp.in_samplerate = samplerate; gfp.brate = kbps; gfp.mode = M.MPEGMode.STEREO; gfp.quality = 3;
    gfp.bWriteVbrTag = false; gfp.disable_reservoir = true; gfp.write_id3tag_automatic = false;
    if (lame.lame_init_params(gfp) != 0) throw new Error('lame_init_params failed');
    let maxSamples = 1152, mp3buf_size = 0 | (1.25 * maxSamples + 7200), mp3buf = new Int8Array(mp3buf_size);
    return {
        lame, gfp, gfc: gfp.internal_flags,
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if (left.length > maxSamples) { maxSamples = left.length; mp3buf_size = 0 | (1.25 * maxSamples + 7200); mp3buf = new Int8Array(mp3buf_size); }
            const n = lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, mp3buf_size);
            return new Int8Array(mp3buf.subarray(0, n));
        },
        flush() { const n = lame.lame_encode_flush(gfp, mp3buf, 0, mp3buf_size); return new Int8Array(mp3buf.subarray(0, n)); }
    };
}

/* an encoder of the unmodified reference whose frames are watched: e.frames = [{ bytes, header_hex, nan_in_window, md5, data }] in order */
function hookedRef(channels, samplerate, kbps) {
    const haveSrc = fs.existsSync(path.join(harness.REF, 'src', 'js', 'index.js'));
    const e = haveSrc ? harness.refEncoder(channels, samplerate, kbps) : wireFromBundle(channels, samplerate, kbps);
    const enc = e.lame.enc, orig = enc.lame_encode_mp3_frame, gfp = e.gfp, gfc = e.gfc;
    const mf_needed = 1024 + gfp.framesize - 272;
    e.frames = [];
    enc.lame_encode_mp3_frame = function (g, inbuf_l, inbuf_r, mp3buf, mp3bufPos, mp3buf_size) {
        let nan = false;
        for (let i = 0; i < mf_needed && !nan; i++) nan = inbuf_l[i] !== inbuf_l[i] || (gfc.channels_out == 2 && inbuf_r[i] !== inbuf_r[i]);
        const ret = orig.call(enc, g, inbuf_l, inbuf_r, mp3buf, mp3bufPos, mp3buf_size);
        const data = Buffer.from(new Int8Array(mp3buf.subarray(mp3bufPos, mp3bufPos + Math.max(ret, 0))).buffer);
        e.frames.push({ bytes: ret, header_hex: data.subarray(0, 4).toString('hex'), nan_in_window: nan, md5: crypto.createHash('md5').update(data).digest('hex'), data });
        return ret;
    };
    e.nanBuffered = function () { for (let ch = 0; ch < gfc.channels_out; ch++) for (let i = 0; i < gfc.mf_size; i++) if (gfc.mfbuf[ch][i] !== gfc.mfbuf[ch][i]) return true; return false; };
    return e;
}

/* the 49 triples of profiles/r03_reference_noninteger_resample.txt, computed: every triple tables.js refuses by default for its ratio */
function fractionalTriples() {
    const tables = require('../../lamejs_amd/js/tables.js');
    const RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000];
    const KBPS = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 192, 224, 256, 320];
    const out = [];
    for (const ch of [1, 2]) for (const sr of RATES) for (const kb of KBPS) {
        let p = null;
        try { p = tables.resolveParams(ch, sr, kb, { fractionalResample: true }); } catch (err) { continue; }
        if (p.rs_filter_l == 31) out.push({ ch, sr, kb, out: p.out_samplerate, ratio: p.resample_ratio, framesize: p.framesize, limit: tables.fractionalCallLimit(p) });
    }
    return out;
}

module.exports = { hookedRef, fractionalTriples };
