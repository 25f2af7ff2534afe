/*
 * Drop-in replacement for the encode path of zhuker/lamejs:
 *     const { Mp3Encoder, WavHeader } = require('lamejs_amd/js');
 *     const enc = new Mp3Encoder(channels, sampleRate, kbps);
 *     const bytes = enc.encodeBuffer(left[, right]);   // Int8Array, possibly empty
 *     const tail  = enc.flush();
 * Same constructor arguments, same return types and the same byte stream as the reference
 * (src/js/index.js:66-136, 138-196).  Parameter resolution and every lookup table are computed here,
 * in JavaScript (tables.js), with the engine's own Math.*; the per-frame hot path -- psychoacoustic
 * model, polyphase + MDCT, CBR iteration loop, bitstream formatting -- runs as hand-written HIP
 * kernels on an MI355X behind the C ABI of include/lamejs_hip.h, reached through a thin N-API addon.
 * GPU efficiency comes from batching: pass many frames per encodeBuffer() call (the reference API
 * already allows any length).  There is no CPU fallback.
 * Extension: new Mp3Encoder(2, sampleRate, kbps, { jointStereo: true }) encodes in the reference core's joint-stereo mode (per frame
 * mid/side or left/right), which the reference's own wrapper never selects (index.js:105 hard-codes MPEGMode.STEREO); { reservoir: true }
 * uses the bit reservoir (index.js:108 switches it off).  With the reservoir the frames of a stream are a serial chain -- a launch
 * encodes one frame per stream -- so that mode only uses the GPU well through encodeBatch() over many streams.
 * Extension for callers that feed 1152 samples per call (every usage the reference documents): { pendingFrames: N } lets the encoder
 * hold back up to N frames' worth of input and encode them in ONE launch -- a frame alone is one wavefront's serial search (0.2 - 0.8 ms),
 * sixty-four together take hardly longer.  The BYTE STREAM is the reference's (any chunking of the samples gives the same bytes); only
 * WHICH call returns which bytes changes: calls return empty arrays until N frames are pending, then all their frames at once, and
 * flush() returns the rest.  Off by default: without it every call returns exactly the bytes the reference's call returns.
 * Extension { downmix, scale, scaleLeft, scaleRight }: the reference core's input gains and stereo-to-mono downmix (Lame.js:1551-1584), which
 * its wrapper does not offer -- new Mp3Encoder(2, 44100, 64, { downmix: true, scale: 0.8, scaleLeft: 1, scaleRight: 0.5 }) takes two channels
 * (encodeBuffer(l, r), encodeInterleaved, encodeBatch, { pendingFrames } holding source samples of both) and writes a mono stream, mixed where
 * the samples are read on the device; byte for byte what the reference's core gives for MPEGMode.MONO with those gains.  `scale` replaces the
 * preset's (0.95 at and below 128 kbps).  { downmix } with one channel or with { jointStereo } is a TypeError; a gain beyond 4 in magnitude,
 * a negative scale or a gain that is not finite is refused at construction.
 * Extension { protect, copyright, original, privateBit, emphasis }: the frame header's settings, which the reference's wrapper leaves at their defaults.
 * new Mp3Encoder(2, 44100, 128, { protect: true }) writes CRC-protected frames (LAME's -p): the reference core's bytes for gfp.error_protection = 1 --
 * same frame sizes, two more bytes of side information per frame, a CRC-16 as ISO 11172-3 defines it.  copyright: true, original: false,
 * privateBit: true and emphasis: 0 | 1 | 3 set the header bits of those names; any other value (emphasis 2 is reserved) is a RangeError.  Accepted
 * wherever { downmix } is, encodeBatch() of protected and unprotected encoders included; not with a { fractionalResample } stream that resamples.
 * Extension { infoTag: true }: the encoder writes a FILE, as LAME does: the first call that returns anything returns, in front of its audio, the placeholder of
 * an Info/LAME tag frame (a valid header, then zeros; the audio behind it is byte for byte the stream without the option); enc.streamInfo() gives
 * { frames, audioBytes, musicCrc, delay, padding (-1 before flush()), tagBytes }; after flush(), enc.infoTagFrame() returns the finished frame -- frame and byte
 * counts, a 100-point seek table, encoder delay and end padding for gapless playback, the CRC-16 of the audio, LAME's extension fields -- as an Int8Array
 * to be written over the placeholder at offset 0.  With every option above, encodeBatch() of tagged beside untagged encoders and { pendingFrames }
 * included; refused at construction where a frame is too small to hold the tag (8 kHz at 8 kbps, say) and on a { fractionalResample } stream that resamples.
 * Extension { replayGain: true }: the samples the encoder consumes (behind gains, downmix and resampler; the zeros of flush() included; left and right of a
 * joint-stereo stream) are analysed on the GPU as the reference core's ReplayGain analysis does -- the published filters, windows of a twentieth of a second,
 * the 95th percentile of their levels -- and enc.replayGain() returns { tenthDb, windows, samples }: the track gain in tenths of a dB.  The result does not
 * depend on how the stream is cut into calls; nothing is read back until replayGain() or infoTagFrame() asks.  With { infoTag } the tag frame's radio
 * ReplayGain field carries the value (peak amplitude and the audiophile field stay zero).  With every option above, encodeBatch() of such encoders beside
 * others and { pendingFrames } included; refused at construction on a { fractionalResample } stream that resamples; not after seek() / setState().
 * Extension { quality: 7 }: LAME's -f, the fast mode of the reference's encoder core (its wrapper always asks for quality 3): block switching and mid/side
 * decisions as always, the quantization of a granule is the bin search for its step size alone -- no noise shaping, no Huffman region search -- so the
 * bytes are those of the reference core with gfp.quality = 7, and a batch is quantized by a kernel of its own (g_quant_fast).  8 is encoded as 7, as the
 * core does; 3 is the default; any other value is a RangeError.  With every option above, encodeBatch() of encoders of both qualities included.
 * Extension { outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth }: the reference core's gfp.out_samplerate, lowpassfreq, lowpasswidth, highpassfreq
 * and highpasswidth (LAME's --resample, --lowpass, --lowpass-width, --highpass, --highpass-width), whole numbers of Hz.  outSampleRate is one of the nine MPEG
 * rates, the input rate or the input rate divided by a whole number: new Mp3Encoder(2, 44100, 96, { outSampleRate: 44100 }) is a plain stream without
 * resampling (the default picks 32000 Hz there, a non-integer ratio).  lowpass replaces the bitrate's band limit (-1: no lowpass) and, without outSampleRate,
 * chooses the output rate as the core does; the widths give the filters a cosine transition instead of a hard edge.  A highpass below the stream's minimum
 * (about 480 Hz at 44.1 kHz), at or above the lowpass, a width without its highpass, upsampling, a non-integer ratio and any value that is not a whole
 * number are RangeErrors.  With every option above, encodeBatch() of encoders with different settings included; not with a { fractionalResample } stream
 * that resamples by a non-integer ratio.
 * Extension { fractionalResample: true }: the 49 (channels, sample rate, kbps) triples the reference resamples by a non-integer ratio -- refused
 * by default, because the reference feeds itself NaN samples there once a call is long enough -- are accepted as call-sequence streams: every
 * encodeBuffer() gives the reference's bytes for the same sequence of call lengths; a call longer than the reference consumes whole throws
 * (enc.callLimit() samples are always accepted: 1585 for 44100 -> 32000 Hz, never less than 576); a call completes at most one frame -- the
 * throughput is in encodeBatch() over many such streams, of any mix of configurations; the flush frames the reference makes of its own NaN
 * samples are replaced by silent frames of equal length and header, and the stream ends with flush().  Not with { pendingFrames }
 * (re-chunking changes the bytes) or { reservoir }; no seek / getState / setState.  For every other triple the option changes nothing.
 * Samples.  encodeBuffer() takes what the reference takes: its lame_encode_buffer stores whatever numbers it is given into a Float32Array
 * (Lame.js:1506-1510) and encodes that.  An Int16Array goes to the GPU as it is; a Float32Array as it is (fractional parts and values beyond 16
 * bits included: the reference's bytes for those values); anything else (Array, Float64Array, other typed arrays) through Float32Array.from,
 * which is the reference's own store.  The one deviation: a sample that is not finite or lies beyond +-131072 throws a RangeError and
 * consumes nothing (the reference encodes NaN into garbage).  Extension encodeInterleaved(samples): channels * n samples as they lie in a
 * WAV file (L R L R ...), Int16Array or Float32Array, read in place by the kernels.
 */
'use strict';
const path = require('path');
const tables = require('./tables.js');

let addon = null;
let defaultDevice = -1;                         // -1: the HIP runtime's current device
function loadAddon() {
    if (!addon) addon = require(path.join(__dirname, 'addon', 'lhip_napi.node'));
    return addon;
}

/* The table blob of a configuration is a pure function of (channels, samplerate, kbps, options): built once per process and shared by
 * every encoder of that configuration (1024 streams of BASELINE config 5 = one build, not 1024; the library shares the uploaded copy
 * between streams with identical blobs as well).  Configurations outside the envelope throw in buildBlob and are not cached. */
const blobCache = new Map();
function tablesBlob(channels, samplerate, kbps, opts) {
    const key = [channels, samplerate, kbps, opts && opts.jointStereo ? 1 : 0, opts && opts.reservoir ? 1 : 0, opts && opts.fractionalResample ? 1 : 0,
        opts && opts.downmix ? 1 : 0, opts ? String(opts.scale) : '', opts ? String(opts.scaleLeft) : '', opts ? String(opts.scaleRight) : '',
        opts ? ['protect', 'copyright', 'original', 'privateBit', 'emphasis'].map((k) => String(opts[k])).join(',') : '', opts && opts.infoTag ? 1 : 0, opts && opts.replayGain ? 1 : 0,
        opts ? typeof opts.quality + String(opts.quality) : '',
        opts ? ['outSampleRate', 'lowpass', 'lowpassWidth', 'highpass', 'highpassWidth'].map((k) => typeof opts[k] + String(opts[k])).join(',') : ''].join('|');     /* (quality and the filter options with their type: '7' is refused, not served 7's blob; pendingFrames is host-side only) */
    let blob = blobCache.get(key);
    if (!blob) { blob = tables.buildBlob(channels, samplerate, kbps, opts).blob; blobCache.set(key, blob); }
    return blob;
}

/* one call's arrays in one sample type: Int16Array if all of them are, otherwise Float32Array (Int16 values are exact in Float32) */
const isPcm = (a) => a instanceof Int16Array || a instanceof Float32Array;
const toF32 = (a) => (a instanceof Float32Array ? a : Float32Array.from(a));
function sameType(arrays) {
    return arrays.every((a) => a instanceof Int16Array) ? arrays : arrays.map(toF32);
}
const PCM_LIMIT = 131072;
function checkF32(a, what) {
    for (let i = 0; i < a.length; i++)
        if (!(Math.abs(a[i]) <= PCM_LIMIT)) throw new RangeError('lamejs_amd: Float32 sample outside the contract (finite, |x| <= 131072): ' + what + ' index ' + i + ', value ' + a[i] + '; nothing was consumed');
}

/* Sample types a WAV file stores (include/lamejs_hip.h: LHIP_PCM_*), by the names encodePcm() and encodeBatch(..., { format }) take.  'f32' and 'f64'
 * are the NORMALISED types: floats in [-1, 1], full scale = 32768. */
const PCM_TYPES = { u8: [4, 1], s16: [0, 2], s24: [8, 3], s32: [12, 4], f32: [16, 4], f64: [20, 8] };
function pcmType(format) {
    const t = PCM_TYPES[format];
    if (!t) throw new TypeError("lamejs_amd: format must be one of 'u8', 's16', 's24', 's32', 'f32', 'f64'");
    return t;
}
function asBytes(b) {
    if (b instanceof Uint8Array) return b;
    if (b instanceof ArrayBuffer) return new Uint8Array(b);
    if (ArrayBuffer.isView(b)) return new Uint8Array(b.buffer, b.byteOffset, b.byteLength);
    throw new TypeError('lamejs_amd: bytes must be a Uint8Array, a Buffer, an ArrayBuffer or a view of one');
}
/* the value the encoder sees for element e of `bytes` (the header's table): what { pendingFrames } holds back of such input, as Float32 */
function pcmValue(dv, format, e) {
    switch (format) {
        case 'u8': return (dv.getUint8(e) - 128) * 256;
        case 's16': return dv.getInt16(2 * e, true);
        case 's24': return ((dv.getUint8(3 * e) | (dv.getUint8(3 * e + 1) << 8) | (dv.getInt8(3 * e + 2) << 16))) / 256;
        case 's32': return dv.getInt32(4 * e, true) / 65536;
        case 'f32': return dv.getFloat32(4 * e, true) * 32768;
        default: return dv.getFloat64(8 * e, true) * 32768;
    }
}
/* the float types' contract as the library applies it: the value (a double: compared BEFORE it is rounded to Float32) must be finite and within the limit */
function checkPcm(dv, format, count, where) {
    if (format != 'f32' && format != 'f64') return;
    for (let e = 0; e < count; e++) {
        const v = pcmValue(dv, format, e);
        if (!(Math.abs(v) <= PCM_LIMIT)) throw new RangeError('lamejs_amd: sample outside the contract (finite, |32768 x| <= 131072): ' + where(e) + ', value ' + v / 32768 + '; nothing was consumed');
    }
}

function Mp3Encoder(channels, samplerate, kbps, opts) {
    if (arguments.length != 3 && !(arguments.length == 4 && opts !== null && typeof opts == 'object')) {
        opts = undefined;
        console.error('WARN: Mp3Encoder(channels, samplerate, kbps) not specified');
        channels = 1; samplerate = 44100; kbps = 128;
    }
    const native = loadAddon();
    const blob = tablesBlob(channels, samplerate, kbps, opts);
    /* a stream that resamples by a non-integer ratio is a call-sequence stream: holding input back would change its bytes */
    const fractional = !!(opts && opts.fractionalResample) && tables.fractionalCallLimit(tables.resolveParams(channels, samplerate, kbps, opts)) > 0;
    if (fractional && opts.pendingFrames > 1)
        throw new Error('lamejs_amd: { pendingFrames } cannot be combined with { fractionalResample } for (' + channels + ',' + samplerate + ',' + kbps + '): the bytes of such a stream depend on the call lengths');
    const handle = native.create(blob, channels, samplerate, kbps, defaultDevice);
    const hooks = { handle: handle, channels: channels, drain: null, pending: () => 0 };
    Object.defineProperty(this, '_lhip', { value: hooks, enumerable: false });

    /* { pendingFrames: N }: input held back until N frames' worth has accumulated (see the header comment) */
    const pendMax = opts && opts.pendingFrames > 1 ? 1152 * (opts.pendingFrames | 0) : 0;
    let pendL = pendMax ? new Int16Array(pendMax + 1152) : null, pendR = pendMax && channels == 2 ? new Int16Array(pendMax + 1152) : null, pendN = 0;
    const EMPTY = () => new Int8Array(0);
    function drain() {
        if (pendN == 0) return EMPTY();
        const out = native.encode(handle, pendL.subarray(0, pendN), pendR ? pendR.subarray(0, pendN) : null);
        pendN = 0;
        return out;
    }
    /* what is held back belongs in front of anything that reaches the native handle by another way (encodeBatch / flushBatch drain it first and
     * return its bytes in front of their own; getState / setState / seek refuse while input is pending: the state would not contain it) */
    if (pendMax) { hooks.drain = drain; hooks.pending = () => pendN; }
    const noPending = (what) => { if (pendN > 0) throw new Error(what + ': ' + pendN + ' samples are held back by { pendingFrames }; call flush() first'); };
    /* { pendingFrames }: Int16 input is held back in Int16 buffers; at the first other input what is held back moves into Float32 buffers, which
     * then serve for the rest of the stream (Int16 values are exact in Float32: the byte stream does not change) */
    function pendToF32() {
        const l = new Float32Array(pendL.length); l.set(pendL.subarray(0, pendN)); pendL = l;
        if (pendR) { const r = new Float32Array(pendR.length); r.set(pendR.subarray(0, pendN)); pendR = r; }
    }
    this.encodeBuffer = function (left, right) {
        if (channels == 1) right = null;
        [left, right] = sameType(right ? [left, right] : [left]);
        if (!pendMax) return native.encode(handle, left, right || null);
        if (right && right.length != left.length) throw new TypeError('right must be an Int16Array of the same length');       /* (the native path's own check and message) */
        if (left instanceof Float32Array) {                      /* checked before it is held back: a refused sample consumes nothing */
            checkF32(left, 'left'); if (right) checkF32(right, 'right');
            if (pendL instanceof Int16Array) pendToF32();
        }
        if (left.length > pendL.length - pendN) {                /* does not fit beside what is pending: encode that first, then this */
            const a = drain(), b = left.length >= pendMax ? native.encode(handle, left, right || null) : null;
            if (b) { const r = new Int8Array(a.length + b.length); r.set(a, 0); r.set(b, a.length); return r; }
            pendL.set(left, 0); if (pendR) pendR.set(right || left, 0); pendN = left.length;
            return a;
        }
        pendL.set(left, pendN); if (pendR) pendR.set(right || left, pendN); pendN += left.length;
        return pendN >= pendMax ? drain() : EMPTY();
    };
    /* Extension: channels * n samples interleaved (L R L R ...), Int16Array or Float32Array (anything else through Float32Array.from) */
    this.encodeInterleaved = function (samples) {
        if (!isPcm(samples)) samples = Float32Array.from(samples);
        if (samples.length % channels) throw new TypeError('interleaved samples: the length must be a multiple of the channel count');
        if (!pendMax) return native.encode(handle, samples, null, channels);
        if (channels == 1) return this.encodeBuffer(samples);
        const n = samples.length / 2, l = new samples.constructor(n), r = new samples.constructor(n);      /* held back per channel, like everything { pendingFrames } holds back */
        for (let i = 0; i < n; i++) { l[i] = samples[2 * i]; r[i] = samples[2 * i + 1]; }
        return this.encodeBuffer(l, r);
    };
    /* Extension: PCM as a WAV file stores it -- encodePcm(bytes, format[, { interleaved = true }]).  format: 'u8', 's16', 's24', 's32', 'f32', 'f64' (the two
     * float names: samples in [-1, 1]); interleaved (L R L R ..., as in the file) or the left plane followed by the right one.  The bytes travel as they
     * are and a kernel converts them; only a call small enough for one pinned block (a few frames) is converted by the host while it fills that block, and a
     * call of a float type is scanned by the library first.  A float sample that is not finite or lies beyond +-4 is a RangeError and
     * consumes nothing.  With { pendingFrames } the input is held back as the Float32 values it stands for. */
    this.encodePcm = function (bytes, format, o) {
        const [type, bps] = pcmType(format), u8 = asBytes(bytes), inter = !(o && o.interleaved === false);
        if (u8.length % (bps * channels)) throw new TypeError('encodePcm: the byte length must be a whole number of sample frames');
        if (!pendMax) return native.encodePcm(handle, u8, type, channels, inter);
        const n = u8.length / (bps * channels), dv = new DataView(u8.buffer, u8.byteOffset, u8.byteLength);
        const l = new Float32Array(n), r = channels == 2 ? new Float32Array(n) : null;
        checkPcm(dv, format, u8.length / bps, (e) => 'channel ' + (r ? (inter ? e & 1 : (e < n ? 0 : 1)) : 0) + ', index ' + (r && inter ? e >> 1 : e % n));      /* as the library does: before the rounding */
        for (let i = 0; i < n; i++) {
            l[i] = pcmValue(dv, format, r && inter ? 2 * i : i);
            if (r) r[i] = pcmValue(dv, format, inter ? 2 * i + 1 : n + i);
        }
        return this.encodeBuffer(l, r);
    };
    this.flush = function () {
        if (!pendMax || pendN == 0) return native.flush(handle);
        const a = drain(), b = native.flush(handle);
        const r = new Int8Array(a.length + b.length); r.set(a, 0); r.set(b, a.length);
        return r;
    };
    /* Extension -- frame-range sharding of ONE stream (include/lamejs_hip.h, lhip_seek ...; DESIGN.md 7): a fresh encoder is put
     * at input sample `samplePos` (a whole number >= 2 of frames) with the seekTailSamples() samples in front of it, encodes a few
     * warm-up frames whose bytes are thrown away, and its getState() at the cut is compared with the getState() of the encoder that
     * came from the left; equal states = equal futures, otherwise setState() transplants the true one. */
    this.seekTailSamples = function () { return native.seekTailSamples(handle); };
    this.seek = function (samplePos, tailLeft, tailRight) { noPending('seek'); native.seek(handle, samplePos, tailLeft, channels == 1 ? null : (tailRight || null)); };
    this.getState = function () { noPending('getState'); return native.stateGet(handle); };
    this.setState = function (state) { noPending('setState'); native.stateSet(handle, state); };
    /* { fractionalResample }: the encodeBuffer() length that is accepted whatever calls came before (0: any length goes) */
    this.callLimit = function () { return native.callLimit(handle); };
    /* { infoTag }: the stream's totals so far; after flush() the finished Info/LAME tag frame, to be written over the placeholder at offset 0 */
    this.streamInfo = function () { return native.streamInfo(handle); };
    this.infoTagFrame = function () { noPending('infoTagFrame'); return native.infoTag(handle); };
    /* { replayGain }: { tenthDb, windows, samples } -- the track gain in tenths of a dB (null while no window of ceil(rate / 20) samples is complete), the
     * complete windows and the samples analysed so far (samples still held back by { pendingFrames } are not among them) */
    this.replayGain = function () { return native.replayGain(handle); };
}

/* RIFF/WAVE header reader with the reference's field names (index.js:138-193) */
function WavHeader() { this.dataOffset = 0; this.dataLen = 0; this.channels = 0; this.sampleRate = 0; }
WavHeader.readHeader = function (dataView) {
    const tag = (o) => String.fromCharCode(dataView.getUint8(o), dataView.getUint8(o + 1), dataView.getUint8(o + 2), dataView.getUint8(o + 3));
    const w = new WavHeader();
    if (tag(0) != 'RIFF' || tag(8) != 'WAVE' || tag(12) != 'fmt ') return;
    const fmtLen = dataView.getUint32(16, true);
    if (fmtLen != 16 && fmtLen != 18) throw 'extended fmt chunk not implemented';
    w.channels = dataView.getUint16(22, true);
    w.sampleRate = dataView.getUint32(24, true);
    let pos = 20 + fmtLen, len = 0;
    for (;;) {
        const id = tag(pos);
        len = dataView.getUint32(pos + 4, true);
        if (id == 'data') break;
        pos += len + 8;
    }
    w.dataLen = len;
    w.dataOffset = pos + 8;
    return w;
};
/* Extension: what encodePcm() needs to know of a WAV file -- { format, channels, sampleRate, dataOffset, dataLen }, format one of encodePcm's names.
 * `fmt ` chunks of 16, 18 and 40 bytes: PCM (1), IEEE float (3), and WAVE_FORMAT_EXTENSIBLE (0xFFFE) by the first two bytes of its sub-format;
 * 8, 16, 24 and 32 bits for PCM, 32 and 64 for float.  Anything else throws. */
WavHeader.readFormat = function (dataView) {
    const tag = (o) => String.fromCharCode(dataView.getUint8(o), dataView.getUint8(o + 1), dataView.getUint8(o + 2), dataView.getUint8(o + 3));
    if (dataView.byteLength < 28 || tag(0) != 'RIFF' || tag(8) != 'WAVE' || tag(12) != 'fmt ') throw new Error('readFormat: not a RIFF/WAVE file with a leading fmt chunk');
    const fmtLen = dataView.getUint32(16, true);
    if (fmtLen != 16 && fmtLen != 18 && fmtLen != 40) throw new Error('readFormat: fmt chunk of ' + fmtLen + ' bytes not supported');
    let code = dataView.getUint16(20, true);
    const channels = dataView.getUint16(22, true), sampleRate = dataView.getUint32(24, true), bits = dataView.getUint16(34, true);
    if (code == 0xFFFE) {
        if (fmtLen != 40 || dataView.getUint16(36, true) < 22) throw new Error('readFormat: WAVE_FORMAT_EXTENSIBLE needs a fmt chunk of 40 bytes');
        code = dataView.getUint16(44, true);              /* the sub-format GUID starts with the format code */
        const valid = dataView.getUint16(38, true);
        if (valid != 0 && valid != bits) throw new Error('readFormat: ' + valid + ' valid bits in a container of ' + bits + ' not supported');
    }
    const format = code == 1 ? { 8: 'u8', 16: 's16', 24: 's24', 32: 's32' }[bits] : code == 3 ? { 32: 'f32', 64: 'f64' }[bits] : undefined;
    if (!format) throw new Error('readFormat: format code ' + code + ' with ' + bits + ' bits per sample not supported');
    if (channels != 1 && channels != 2) throw new Error('readFormat: ' + channels + ' channels not supported');
    if (dataView.getUint16(32, true) != channels * PCM_TYPES[format][1]) throw new Error('readFormat: block align does not match the sample type (padded containers are not supported)');
    let pos = 20 + fmtLen;
    for (;;) {
        if (pos + 8 > dataView.byteLength) throw new Error('readFormat: no data chunk');
        const len = dataView.getUint32(pos + 4, true);
        if (tag(pos) == 'data') {
            /* a length beyond the view (0xFFFFFFFF in a streamed file, a truncated file): what is there, in whole sample frames */
            const frame = channels * PCM_TYPES[format][1], have = dataView.byteLength - (pos + 8);
            return { format: format, channels: channels, sampleRate: sampleRate, dataOffset: pos + 8, dataLen: len <= have ? len : have - have % frame };
        }
        pos += 8 + len + (len & 1);
    }
};

module.exports.Mp3Encoder = Mp3Encoder;
module.exports.WavHeader = WavHeader;
module.exports.deviceCount = function () { return loadAddon().deviceCount(); };

/*
 * Extensions (not part of the reference API) for callers with many independent streams (BASELINE config 5):
 *   setDevice(d)                          encoders constructed afterwards live on HIP device d (deal streams round-robin
 *                                         over deviceCount() GPUs; streams never exchange data)
 *   encodeBatch(encoders, lefts[, rights][, { interleaved: true }])
 *                                         one launch for all the encoders' new samples -> Int8Array per encoder, the same
 *                                         bytes each encoder's own encodeBuffer() would have returned.  Int16 if every array is an
 *                                         Int16Array, otherwise the whole batch as Float32 (still one launch); interleaved: lefts[i]
 *                                         holds channels * n samples (L R L R ...), rights is ignored
 *                                         { format: 'u8' | 's16' | 's24' | 's32' | 'f32' | 'f64' }: the arrays are Uint8Arrays of samples
 *                                         of that type (see Mp3Encoder.encodePcm); a refused float sample is a RangeError
 *   flushBatch(encoders)                  likewise for flush()
 *   setDevices(mask)                      let the library deal new encoders round-robin over the GPUs named by the bit mask
 * The encoders of one call must share the channel count and the device; encoders of one configuration share a launch, other configurations and
 * options (protected beside unprotected encoders, say) get a launch each inside the same call.
 */
module.exports.setDevice = function (d) { defaultDevice = d | 0; };
/* setDevices(mask): bit d = HIP device d may be used; encoders constructed with the default device (-1) are then dealt round-robin
 * over the allowed GPUs by the library (lhip_set_devices); returns how many devices are allowed.  mask 0 restores the default. */
module.exports.setDevices = function (mask) { defaultDevice = -1; return loadAddon().setDevices(mask); };
/* encoders constructed with { pendingFrames }: what they hold back is encoded first and its bytes are returned in front of the batch's own */
function drainPending(encoders) { return encoders.map((e) => (e._lhip.pending() > 0 ? e._lhip.drain() : null)); }
function prepend(heads, outs) {
    return outs.map((b, i) => { const a = heads[i]; if (!a || a.length == 0) return b; const r = new Int8Array(a.length + b.length); r.set(a, 0); r.set(b, a.length); return r; });
}
module.exports.encodeBatch = function (encoders, lefts, rights, opts) {
    if (rights && !Array.isArray(rights) && typeof rights == 'object' && opts === undefined) { opts = rights; rights = null; }
    const hs = encoders.map((e) => e._lhip.handle);
    const channels = encoders.length > 0 ? encoders[0]._lhip.channels : 1;
    const inter = !!(opts && opts.interleaved);
    const nl = lefts.length;
    if (opts && opts.format !== undefined) {          /* { format }: Uint8Arrays of samples as a WAV file stores them (Mp3Encoder.encodePcm); they travel as they are */
        const [type, bps] = pcmType(opts.format);
        /* a refused sample consumes nothing, held-back input included: where something is held back, the float types are looked at before it is encoded */
        if ((opts.format == 'f32' || opts.format == 'f64') && encoders.some((e) => e._lhip.pending() > 0))
            lefts.concat(channels == 2 && rights && !inter ? rights : []).forEach((b, i) => {
                const u8 = asBytes(b), dv = new DataView(u8.buffer, u8.byteOffset, u8.byteLength);
                checkPcm(dv, opts.format, u8.length / bps, (e) => 'array ' + i + ', element ' + e);
            });
        const heads = drainPending(encoders);
        return prepend(heads, loadAddon().encodeBatch(hs, lefts.map(asBytes), channels == 2 && rights && !inter ? rights.map(asBytes) : null, inter ? channels : 0, type));
    }
    const all = sameType(lefts.concat(channels == 2 && rights && !inter ? rights : []).map((a) => (isPcm(a) ? a : Float32Array.from(a))));
    const L = all.slice(0, nl), R = all.length > nl ? all.slice(nl) : null;
    /* checked BEFORE anything held back by { pendingFrames } is encoded: a refused sample consumes nothing, held-back input included */
    if (L.length > 0 && L[0] instanceof Float32Array) { L.forEach((a, i) => checkF32(a, 'stream ' + i + ', left')); if (R) R.forEach((a, i) => checkF32(a, 'stream ' + i + ', right')); }
    const heads = drainPending(encoders);
    return prepend(heads, loadAddon().encodeBatch(hs, L, R, inter ? channels : 0));
};
module.exports.flushBatch = function (encoders) { const heads = drainPending(encoders); return prepend(heads, loadAddon().flushBatch(encoders.map((e) => e._lhip.handle))); };
