/*
 * TEST TOOL (needs /root/reference): goldens for CRC frame protection and the header's flag bits (tests/golden/golden_protection.json).
 *
 * gfp.error_protection (LAME's -p), gfp.copyright, gfp.original, gfp.extension (the private bit) and gfp.emphasis are settings of the reference's
 * encoder core that its public Mp3Encoder leaves at lame_init's values, so this generator wires the UNMODIFIED modules itself, as index.js:73-111
 * does, and sets them before lame_init_params (which derives sideinfo_len from error_protection, Lame.js:1103-1110).
 *
 * The reference's CRC path is one identifier short of running: BitStream.js:408 calls `CRC_writeheader` as a free identifier (the function is a
 * method of the BitStream object) and BitStream.js:255-256 write `(byte)(crc >> 8)`, which JavaScript reads as a call of `byte`.  Both are
 * supplied as globals here -- the BitStream's own method and the identity -- and nothing of the reference is modified.
 *
 * Streams of 12 * 1152 input samples from the corpora of tests/tools/pcm_gen.js (the bursts: short blocks; 44.1 kHz rates: padding frames).
 * Calls: twelve of 1152 samples and flush; one stream with uneven call lengths.  Every protected frame the reference wrote is also checked here
 * against an independent bitwise CRC-16 as ISO 11172-3 defines it (polynomial 0x8005, preset 0xffff, header bytes 2, 3 and the side information).
 * usage: node tests/tools/gen_golden_protection.js
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./pcm_gen.js');
const REF = process.env.LAMEJS_REF || '/root/reference';
const S = path.join(REF, 'src', 'js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);

/* opts: { protect, copyright, original, privateBit, emphasis, jointStereo, reservoir, downmix } */
function refEncoder(channels, samplerate, kbps, opts) {
    const req = (n) => require(path.join(S, n + '.js'));
    const Lame = req('Lame'), Presets = req('Presets'), GainAnalysis = req('GainAnalysis'), QuantizePVT = req('QuantizePVT'), Quantize = req('Quantize');
    const Takehiro = req('Takehiro'), Reservoir = req('Reservoir'), MPEGMode = req('MPEGMode'), BitStream = req('BitStream'), Version = req('Version'), VBRTag = req('VBRTag');
    function Stub() { this.setModules = function () {}; }
    const lame = new Lame(), gaud = new Stub(), ga = new GainAnalysis(), bs = new BitStream();
    const p = new Presets(), qupvt = new QuantizePVT(), qu = new Quantize(), vbr = new VBRTag();
    const ver = new Version(), id3 = new Stub(), rv = new Reservoir(), tak = new Takehiro();
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
    /* the two identifiers the reference's CRC path looks up as globals (see the header comment) */
    global.CRC_writeheader = bs.CRC_writeheader;
    global.byte = (x) => x;
    const gfp = lame.lame_init();
    gfp.num_channels = channels;
    gfp.in_samplerate = samplerate;
    gfp.brate = kbps;
    gfp.mode = opts.downmix ? MPEGMode.MONO : (opts.jointStereo && channels == 2) ? MPEGMode.JOINT_STEREO : MPEGMode.STEREO;
    gfp.quality = 3;
    gfp.bWriteVbrTag = false;
    gfp.disable_reservoir = !opts.reservoir;
    gfp.write_id3tag_automatic = false;
    if (opts.protect) gfp.error_protection = 1;
    if (opts.copyright !== undefined) gfp.copyright = opts.copyright ? 1 : 0;
    if (opts.original !== undefined) gfp.original = opts.original ? 1 : 0;
    if (opts.privateBit !== undefined) gfp.extension = opts.privateBit ? 1 : 0;
    if (opts.emphasis !== undefined) gfp.emphasis = opts.emphasis;
    const rc = lame.lame_init_params(gfp);
    if (rc != 0) throw new Error('lame_init_params rc=' + rc);
    let maxSamples = 1152, mp3buf_size = 0 | (1.25 * maxSamples + 7200), mp3buf = new Int8Array(mp3buf_size);
    return {
        gfp, gfc: gfp.internal_flags,
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            if (left.length > maxSamples) { maxSamples = left.length; mp3buf_size = 0 | (1.25 * maxSamples + 7200); mp3buf = new Int8Array(mp3buf_size); }
            const n = lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, mp3buf_size);
            return new Int8Array(mp3buf.subarray(0, n));
        },
        flush() {
            const n = lame.lame_encode_flush(gfp, mp3buf, 0, mp3buf_size);
            return new Int8Array(mp3buf.subarray(0, n));
        }
    };
}

/* ISO 11172-3 CRC-16, bit by bit */
function isoCrc(bytes) {
    let crc = 0xffff;
    for (const b of bytes) for (let i = 7; i >= 0; i--) {
        const top = ((crc >> 15) & 1) ^ ((b >> i) & 1);
        crc = (crc << 1) & 0xffff;
        if (top) crc ^= 0x8005;
    }
    return crc;
}
/* walk the frames of a whole stream: [frames, protected frames whose stored CRC is the ISO one, padded frames] */
function walk(mp3, sideinfo_len) {
    const BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320], BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160];
    const SR = { 3: [44100, 48000, 32000], 2: [22050, 24000, 16000], 0: [11025, 12000, 8000] };
    let pos = 0, n = 0, good = 0, padded = 0;
    while (pos + 6 <= mp3.length) {
        const h = mp3.readUInt32BE(pos);
        if ((h >>> 21) != 0x7ff) throw new Error('lost sync at ' + pos);
        const ver = (h >>> 19) & 3, prot = !((h >>> 16) & 1), bri = (h >>> 12) & 15, sri = (h >>> 10) & 3, pad = (h >>> 9) & 1;
        if (prot) {
            const msg = [mp3[pos + 2], mp3[pos + 3]];
            for (let i = 6; i < sideinfo_len; i++) msg.push(mp3[pos + i]);
            if (isoCrc(msg) == mp3.readUInt16BE(pos + 4)) good++;
        }
        padded += pad;
        pos += Math.floor((ver == 3 ? 144000 : 72000) * (ver == 3 ? BR1 : BR2)[bri] / SR[ver][sri]) + pad;
        n++;
    }
    if (pos != mp3.length) throw new Error('stream does not end on a frame boundary');
    return [n, good, padded];
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

const P = { protect: true };
const EVEN = new Array(12).fill(1152), UNEVEN = [1, 1151, 777, 2305, 333, 1153, 4000, 575, 1152, 2377];      /* both sum to 12 * 1152 */
/* [name, channels in, samplerate, kbps, options, corpus, call lengths] */
const CONFIGS = [
    /* every value of sideinfo_len (38, 23, 15) and both granule counts */
    ['protect_stereo_44100_128', 2, 44100, 128, P, 'bursts', EVEN],
    ['protect_mono_44100_128', 1, 44100, 128, P, 'bursts', EVEN],
    ['protect_stereo_48000_320', 2, 48000, 320, P, 'bursts', EVEN],
    /* (stereo 22.05 kHz at 32 kbps resamples to 16 kHz by a non-integer ratio: { protect } is refused there; 48 kbps keeps the sample rate) */
    ['protect_stereo_22050_48', 2, 22050, 48, P, 'bursts', EVEN],
    ['protect_mono_22050_32', 1, 22050, 32, P, 'bursts', EVEN],
    ['protect_mono_8000_8', 1, 8000, 8, P, 'bursts', EVEN],
    ['protect_stereo_44100_48_resample_int', 2, 44100, 48, P, 'bursts', EVEN],
    ['protect_joint_128', 2, 44100, 128, { protect: true, jointStereo: true }, 'centre_bursts', EVEN],
    ['protect_joint_resv_128', 2, 44100, 128, { protect: true, jointStereo: true, reservoir: true }, 'centre_bursts', EVEN],
    ['protect_stereo_resv_128', 2, 44100, 128, { protect: true, reservoir: true }, 'bursts', EVEN],
    ['protect_mono_resv_128', 1, 44100, 128, { protect: true, reservoir: true }, 'bursts', EVEN],
    ['protect_mono_resv_22050_32', 1, 22050, 32, { protect: true, reservoir: true }, 'bursts', EVEN],
    ['protect_downmix_128', 2, 44100, 128, { protect: true, downmix: true }, 'bursts', EVEN],
    ['protect_uneven_calls', 2, 44100, 128, P, 'bursts', UNEVEN],
    ['protect_mono_uneven_calls_resv', 1, 44100, 64, { protect: true, reservoir: true }, 'sine', UNEVEN],
    /* the flag bits alone */
    ['flag_copyright', 2, 44100, 128, { copyright: true }, 'bursts', EVEN],
    ['flag_not_original', 1, 44100, 128, { original: false }, 'bursts', EVEN],
    ['flag_private', 2, 22050, 48, { privateBit: true }, 'bursts', EVEN],
    ['flag_emphasis_1', 1, 8000, 8, { emphasis: 1 }, 'bursts', EVEN],
    /* everything at once */
    ['everything', 2, 44100, 128, { protect: true, copyright: true, original: false, privateBit: true, emphasis: 3, jointStereo: true, reservoir: true }, 'centre_bursts', UNEVEN]
];

const cases = [];
for (const [name, ch, sr, kbps, opts, corpus, lens] of CONFIGS) {
    const N = lens.reduce((a, b) => a + b, 0);
    if (N != 12 * 1152) throw new Error('call lengths of ' + name);
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
    const [frames, good, padded] = walk(whole, enc.gfc.sideinfo_len);
    if (opts.protect && good != frames) throw new Error(name + ': ' + good + ' of ' + frames + ' frames carry the ISO CRC');
    if (!opts.protect && good != 0) throw new Error(name + ': unprotected stream with protected frames');
    const o = { name, channels: ch, samplerate: sr, kbps, corpus, nsamples: N, ref_sideinfo_len: enc.gfc.sideinfo_len, ref_channels_out: enc.gfc.channels_out,
                out_samplerate: enc.gfp.out_samplerate, frames, padded_frames: padded, header1: whole[1], header2: whole[2] & ~2, header3: whole[3] & ~0x30,
                call_lens: lens, call_bytes: bytes, enc_md5: md5(Buffer.concat(parts)), flush_len: fb.length, flush_md5: md5(fb), pcm_md5: h.digest('hex') };
    for (const k of ['protect', 'copyright', 'original', 'privateBit', 'emphasis', 'jointStereo', 'reservoir', 'downmix']) if (opts[k] !== undefined) o[k] = +opts[k];
    cases.push(o);
    console.log(name, 'sideinfo_len', o.ref_sideinfo_len, 'out', o.out_samplerate, 'frames', frames, 'crc ok', good, 'padded', padded, 'bytes', whole.length, o.enc_md5.slice(0, 8));
}
fs.writeFileSync(path.join(OUT, 'golden_protection.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_protection.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified modules wired as index.js:73-111; gfp.error_protection / copyright / original / extension / emphasis (and mode, disable_reservoir) set before ' +
               'lame_init_params; globals CRC_writeheader (the BitStream\'s own method) and byte (identity) defined, under node ' + process.version, cases }, null, 1));
console.log('wrote', cases.length, 'cases');
