/*
 * TEST TOOL (needs /root/reference): goldens for the Info/LAME tag frame (tests/golden/golden_infotag.json).
 *
 * The reference's tag WRITER (VBRTag.js) does not run -- it still holds Java -- but what the tag reports is computed by code that does run,
 * unmodified: the running music CRC (BitStream.js:927 -> gfc.nMusicCRC), gfp.encoder_delay, gfp.encoder_padding after lame_encode_flush
 * (Lame.js:1409-1412), gfp.frameNum, the version string and the settings lowpassfreq / quality / VBR_q / ATHtype / exp_nspsytune /
 * noise_shaping / preset.  This generator records them per case, beside the total bytes and their md5.
 *
 * The modules come from where tests/tools/ref_harness.js finds the reference (its REF) and are wired as index.js:73-111 does; the options its
 * public Mp3Encoder does not offer (mode, disable_reservoir, error_protection, scale_left / scale_right) are set before lame_init_params.  The
 * protected cases run through tests/tools/ref_bundle_protect.js' evaluation of the reference bundle, which supplies the two identifiers
 * the reference's CRC path looks up as globals (see there).
 *
 * Every recorded nMusicCRC is checked here against an independent bitwise CRC-16 (reflected polynomial 0xA001, initial value 0, no final XOR) of
 * the bytes the encoder returned; on a mismatch nothing is written.
 * usage: node tests/tools/gen_golden_infotag.js
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./pcm_gen.js');
const { REF } = require('./ref_harness.js');
const S = path.join(REF, 'src', 'js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);

function modules(protect) {
    if (protect) return require('./ref_bundle_protect.js').load().__modules;
    const req = (n) => require(path.join(S, n + '.js'));
    const M = {};
    for (const n of ['Lame', 'Presets', 'GainAnalysis', 'QuantizePVT', 'Quantize', 'Takehiro', 'Reservoir', 'MPEGMode', 'BitStream', 'Version', 'VBRTag']) M[n] = req(n);
    return M;
}

/* opts: { jointStereo, reservoir, protect, downmix, scaleLeft, scaleRight } */
function refEncoder(channels, samplerate, kbps, opts) {
    const M = modules(opts.protect);
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
    if (opts.scaleLeft !== undefined) gfp.scale_left = opts.scaleLeft;
    if (opts.scaleRight !== undefined) gfp.scale_right = opts.scaleRight;
    if (lame.lame_init_params(gfp) != 0) throw new Error('lame_init_params failed');
    let cap = 0 | (1.25 * 1152 + 7200), mp3buf = new Int8Array(cap);
    return {
        gfp, gfc: gfp.internal_flags, version: ver.getLameVeryShortVersion(),
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if ((0 | (1.25 * left.length + 7200)) > cap) { cap = 0 | (1.25 * left.length + 7200); mp3buf = new Int8Array(cap); }
            return new Int8Array(mp3buf.subarray(0, lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, cap)));
        },
        flush() { return new Int8Array(mp3buf.subarray(0, lame.lame_encode_flush(gfp, mp3buf, 0, cap))); }
    };
}

/* CRC-16, reflected polynomial 0xA001, initial value 0, no final XOR -- bit by bit */
function crc16(bytes) {
    let crc = 0;
    for (const b of bytes) {
        crc ^= b;
        for (let i = 0; i < 8; i++) crc = (crc & 1) ? (crc >>> 1) ^ 0xA001 : crc >>> 1;
    }
    return crc;
}

function centre(A, B) {
    const L = new Int16Array(A.length), R = new Int16Array(A.length);
    for (let i = 0; i < A.length; i++) {
        const d = B[i] >> 3;
        L[i] = Math.max(-32768, Math.min(32767, A[i] + d));
        R[i] = Math.max(-32768, Math.min(32767, A[i] - d));
    }
    return [L, R];
}

/* calls of `m` samples, then what is left */
function cut(N, m) { const a = []; for (let p = 0; p < N; p += m) a.push(Math.min(m, N - p)); return a; }
const N1 = 12 * 1152 + 37, N2 = 12 * 576 + 37;      /* about twelve frames and an odd remainder, for two- and one-granule streams */
/* (every configuration here has frames large enough for the tag: floor((version + 1) * 72000 * brate / out_samplerate) >= sideinfo_len + 156)
 * [name, channels in, samplerate, kbps, options, corpus, samples, call lengths] */
const CONFIGS = [
    ['stereo_44100_128', 2, 44100, 128, {}, 'bursts', N1, cut(N1, 1152)],
    ['mono_44100_128', 1, 44100, 128, {}, 'bursts', N1, cut(N1, 1152)],
    ['mono_48000_64', 1, 48000, 64, {}, 'sine', N1, cut(N1, 1152)],
    ['stereo_48000_320', 2, 48000, 320, {}, 'bursts', N1, cut(N1, 2000)],
    ['stereo_22050_64_mpeg2', 2, 22050, 64, {}, 'bursts', N2, cut(N2, 700)],
    ['mono_16000_40_mpeg2', 1, 16000, 40, {}, 'sine', N2, cut(N2, 576)],
    ['mono_8000_24_mpeg25', 1, 8000, 24, {}, 'bursts', N2, cut(N2, 576)],
    ['stereo_12000_64_mpeg25', 2, 12000, 64, {}, 'sine', N2, cut(N2, 1000)],
    ['stereo_48000_64_resample_int', 2, 48000, 64, {}, 'bursts', 2 * N2, cut(2 * N2, 1152)],
    ['joint_128', 2, 44100, 128, { jointStereo: true }, 'centre_bursts', N1, cut(N1, 1152)],
    ['resv_stereo_128', 2, 44100, 128, { reservoir: true }, 'bursts', N1, cut(N1, 1152)],
    ['resv_mono_22050_56', 1, 22050, 56, { reservoir: true }, 'sine', N2, cut(N2, 576)],
    ['joint_resv_128', 2, 44100, 128, { jointStereo: true, reservoir: true }, 'centre_bursts', N1, cut(N1, 5000)],
    ['protect_stereo_128', 2, 44100, 128, { protect: true }, 'bursts', N1, cut(N1, 1152)],
    ['protect_mono_22050_56', 1, 22050, 56, { protect: true }, 'bursts', N2, cut(N2, 576)],
    ['protect_joint_resv_128', 2, 44100, 128, { protect: true, jointStereo: true, reservoir: true }, 'centre_sine', N1, cut(N1, 1152)],
    ['downmix_unequal_gains', 2, 44100, 128, { downmix: true, scaleLeft: 0.5, scaleRight: 0.25 }, 'bursts', N1, cut(N1, 1152)],
    ['gains_lr_reservoir_320', 2, 44100, 320, { scaleLeft: 0.5, scaleRight: 0.25, reservoir: true }, 'sine', N1, cut(N1, 1152)],
    ['calls_of_100', 1, 44100, 64, {}, 'sine', N1, cut(N1, 100)],
    ['calls_of_100_stereo_resv', 2, 44100, 128, { reservoir: true }, 'sine', N1, cut(N1, 100)],
    ['one_call', 2, 44100, 128, {}, 'sine', N1, [N1]],
    ['one_call_mono_mpeg2', 1, 22050, 56, {}, 'bursts', N2, [N2]]
];

const cases = [];
for (const [name, ch, sr, kbps, opts, corpus, N, lens] of CONFIGS) {
    if (lens.reduce((a, b) => a + b, 0) != N) throw new Error('call lengths of ' + name);
    let [L, R] = gen[corpus.replace('centre_', '')](N, ch);
    if (corpus.startsWith('centre_')) [L, R] = centre(L, R);
    const h = crypto.createHash('md5'); h.update(buf(L)); if (R) h.update(buf(R));
    const enc = refEncoder(ch, sr, kbps, opts);
    const parts = [], bytes = [];
    let p = 0;
    for (const m of lens) {
        const b = ch == 2 ? enc.encodeBuffer(L.subarray(p, p + m), R.subarray(p, p + m)) : enc.encodeBuffer(L.subarray(p, p + m));
        p += m;
        bytes.push(b.length); parts.push(Buffer.from(b.buffer, b.byteOffset, b.length));
    }
    const f = enc.flush(), fb = Buffer.from(f.buffer, f.byteOffset, f.length);
    const whole = Buffer.concat(parts.concat([fb]));
    const own = crc16(whole);
    if (own != enc.gfc.nMusicCRC) { console.error(name + ': nMusicCRC ' + enc.gfc.nMusicCRC + ' is not the bitwise CRC-16 of the bytes, ' + own + ' -- nothing written'); process.exit(1); }
    const g = enc.gfp;
    const o = { name, channels: ch, samplerate: sr, kbps, corpus, nsamples: N, call_lens: lens, call_bytes: bytes, enc_md5: md5(Buffer.concat(parts)), flush_len: fb.length,
                flush_md5: md5(fb), all_md5: md5(whole), total_bytes: whole.length, pcm_md5: h.digest('hex'),
                nMusicCRC: enc.gfc.nMusicCRC, encoder_delay: g.encoder_delay, encoder_padding: g.encoder_padding, frameNum: g.frameNum, version_string: enc.version,
                lowpassfreq: g.lowpassfreq, quality: g.quality, VBR_q: g.VBR_q, ATHtype: g.ATHtype, exp_nspsytune: g.exp_nspsytune, noise_shaping: enc.gfc.noise_shaping, preset: g.preset,
                out_samplerate: g.out_samplerate, ref_brate: g.brate, ref_sideinfo_len: enc.gfc.sideinfo_len, ref_channels_out: enc.gfc.channels_out };
    for (const k of ['jointStereo', 'reservoir', 'protect', 'downmix']) if (opts[k]) o[k] = 1;
    for (const k of ['scaleLeft', 'scaleRight']) if (opts[k] !== undefined) o[k] = opts[k];
    cases.push(o);
    console.log(name, 'out', g.out_samplerate, 'frames', g.frameNum, 'bytes', whole.length, 'crc', own.toString(16), 'delay', g.encoder_delay, 'padding', g.encoder_padding,
                'lowpass', g.lowpassfreq, 'preset', g.preset, 'zero-byte calls', bytes.filter((x) => x == 0).length);
}
fs.writeFileSync(path.join(OUT, 'golden_infotag.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_infotag.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified modules wired as index.js:73-111; mode / disable_reservoir / error_protection / scale_left / scale_right set before ' +
               'lame_init_params; every nMusicCRC equal to a bitwise CRC-16 (0xA001 reflected, initial value 0) of the returned bytes, under node ' + process.version, cases }, null, 1));
console.log('wrote', cases.length, 'cases');
