/*
 * TEST INFRASTRUCTURE: the UNMODIFIED reference bundle (oracle/_ref/lame.all.js, see tests/tools/ref_bundle.js) evaluated so that its CRC path
 * runs.  BitStream.js:408 calls `CRC_writeheader` as a free identifier (the function is a method of the BitStream object) and
 * BitStream.js:255-256 write `(byte)(crc >> 8)`, a call of `byte` in JavaScript.  The bundle is evaluated as the body of a function whose two
 * parameters carry those names -- the BitStream's own method and the identity --, so nothing leaks into the globals and the file is not touched.
 * refEncoder() repeats the wiring of index.js:73-111 and sets gfp.error_protection / copyright / original / extension / emphasis (and mode,
 * disable_reservoir) before lame_init_params.
 */
'use strict';
const fs = require('fs');
const { bundlePath } = require('./ref_bundle.js');

let cached = null;
function load() {
    if (cached) return cached;
    const p = bundlePath();
    if (!p) throw new Error('reference bundle not found (make -C oracle ref_js)');
    let src = fs.readFileSync(p, 'utf8');
    const anchor = 'lamejs.Mp3Encoder = Mp3Encoder;';
    const at = src.lastIndexOf(anchor);
    if (at < 0) throw new Error('reference bundle: unexpected layout');
    const hook = 'lamejs.__modules = { Lame: Lame, Presets: Presets, GainAnalysis: GainAnalysis, QuantizePVT: QuantizePVT, Quantize: Quantize, ' +
                 'Takehiro: Takehiro, Reservoir: Reservoir, MPEGMode: MPEGMode, BitStream: BitStream, Version: Version, VBRTag: VBRTag };\n';
    src = src.slice(0, at) + hook + src.slice(at);
    let method = null;
    const crcWriteheader = function (gfc, header) { if (!method) method = new cached.__modules.BitStream().CRC_writeheader; return method(gfc, header); };
    cached = (new Function('CRC_writeheader', 'byte', src + '\nreturn lamejs;'))(crcWriteheader, (x) => x);
    return cached;
}

/* opts: { protect, copyright, original, privateBit, emphasis, jointStereo, reservoir, downmix } */
function refEncoder(channels, samplerate, kbps, opts) {
    const M = load().__modules;
    opts = opts || {};
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
    gfp.mode = opts.downmix ? M.MPEGMode.MONO : (opts.jointStereo && channels == 2) ? M.MPEGMode.JOINT_STEREO : M.MPEGMode.STEREO;
    gfp.quality = 3; gfp.bWriteVbrTag = false; gfp.disable_reservoir = !opts.reservoir; gfp.write_id3tag_automatic = false;
    if (opts.protect) gfp.error_protection = 1;
    if (opts.copyright !== undefined) gfp.copyright = opts.copyright ? 1 : 0;
    if (opts.original !== undefined) gfp.original = opts.original ? 1 : 0;
    if (opts.privateBit !== undefined) gfp.extension = opts.privateBit ? 1 : 0;
    if (opts.emphasis !== undefined) gfp.emphasis = opts.emphasis;
    if (lame.lame_init_params(gfp) != 0) throw new Error('lame_init_params failed');
    let cap = 0 | (1.25 * 1152 + 7200), mp3buf = new Int8Array(cap);
    return {
        sideinfoLen: gfp.internal_flags.sideinfo_len,
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if ((0 | (1.25 * left.length + 7200)) > cap) { cap = 0 | (1.25 * left.length + 7200); mp3buf = new Int8Array(cap); }
            return new Int8Array(mp3buf.subarray(0, lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, cap)));
        },
        flush() { return new Int8Array(mp3buf.subarray(0, lame.lame_encode_flush(gfp, mp3buf, 0, cap))); }
    };
}

module.exports = { load, refEncoder };
