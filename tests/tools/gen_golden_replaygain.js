/*
 * TEST TOOL (needs /root/reference): goldens for the ReplayGain analysis (tests/golden/golden_replaygain.json), from the live reference.
 *
 * The reference's core has the analysis (GainAnalysis.js, called from lame_encode_buffer_sample on the samples it has just put into mfbuf,
 * Lame.js:1609-1613), but it cannot run as the encoder calls it.  Nothing of the reference is edited; this harness supplies from outside what is missing:
 *   - common.Arrays.ill (a typo for fill in InitGainAnalysis) is set to Arrays.fill;
 *   - the bare names nobody defines -- MAX_ORDER, GAIN_ANALYSIS_OK, GAIN_ANALYSIS_ERROR, INIT_GAIN_ANALYSIS_OK, INIT_GAIN_ANALYSIS_ERROR,
 *     GAIN_NOT_ENOUGH_SAMPLES (GainAnalysis.js), GainAnalysis and NEQ (BitStream.js) -- become globals with the values GainAnalysis.js:114-121 gives them;
 *   - lame_init_params switches the analysis off whenever bWriteVbrTag is false: gfc.findReplayGain = true and InitGainAnalysis after it;
 *   - `i = cursamples / 8; while (i-- != 0)` never ends unless cursamples is a multiple of eight: the module handed to Lame and BitStream is a wrapper whose
 *     AnalyzeSamples gives the real one eight samples per call, and throws when a piece is not a multiple of eight (a case that cannot run fails, it does not hang).
 * That runs the seven output rates whose window is a multiple of eight end to end.  At 44100 and 22050 Hz (windows 2205 and 1103) the module hangs at the first
 * window's end; there it runs for the first 2200 / 1096 samples, and rgdata's filter outputs and running sums are recorded: they pin those coefficient rows and
 * the arithmetic bit for bit.
 *
 * Per case: the non-zero histogram bins in front of GetTitleGain, RadioGain, the samples analysed (`fed`) and their md5 (Float32, left then right), every
 * window's bin in order for the `bins` cases, margin_ok (moving the percentile bin by +-2 does not change RadioGain), and -- from this file's own restatement
 * of the arithmetic, checked here against the live module window by window -- in how many windows a recursion restarted from zero state wf samples in front
 * of the window (wf: lamejs_amd/csrc/k_gain.h) lands in another bin than the recursion run through (`restart_diff`): the tests' cap for the device comes from it.
 * usage: node tests/tools/gen_golden_replaygain.js
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const gen = require('./pcm_gen.js');
const { REF } = require('./ref_harness.js');
const S = path.join(REF, 'src', 'js');
const OUT = path.join(__dirname, '..', 'golden');
const md5 = (b) => crypto.createHash('md5').update(b).digest('hex');
const buf = (b) => Buffer.from(b.buffer, b.byteOffset, b.byteLength);

/* ---- what the reference leaves undefined ---- */
const common = require(path.join(S, 'common.js'));
common.Arrays.ill = common.Arrays.fill;
const GainAnalysisModule = require(path.join(S, 'GainAnalysis.js'));
Object.assign(global, { MAX_ORDER: 10, GAIN_ANALYSIS_OK: 1, GAIN_ANALYSIS_ERROR: 0, INIT_GAIN_ANALYSIS_OK: 1, INIT_GAIN_ANALYSIS_ERROR: 0, GAIN_NOT_ENOUGH_SAMPLES: -24601,
                        GainAnalysis: GainAnalysisModule });
global.NEQ = function (a, b) { return !((Math.abs(a) > Math.abs(b)) ? (Math.abs(a - b) <= Math.abs(a) * 1e-6) : (Math.abs(a - b) <= Math.abs(b) * 1e-6)); };      /* BitStream.js:22-30 */

/* the library's table: window, wf and -- for this file's restatement -- the coefficients, which the exact comparison with the live module below pins */
function rateTable() {
    const src = fs.readFileSync(path.join(__dirname, '..', '..', 'lamejs_amd', 'csrc', 'k_gain.h'), 'utf8');
    const t = {};
    const re = /\{(\d+), (\d+), (\d+),\s*\{([^}]*)\},\s*\{([^}]*)\}\}/g;
    let m;
    while ((m = re.exec(src))) t[+m[1]] = { window: +m[2], wf: +m[3], ky: m[4].split(',').map(Number), kb: m[5].split(',').map(Number) };
    if (Object.keys(t).length != 9) throw new Error('k_gain.h: nine rates expected');
    return t;
}
const RT = rateTable();

function refEncoder(channels, samplerate, kbps, opts, log) {
    const req = (n) => require(path.join(S, n + '.js'));
    const M = {};
    for (const n of ['Lame', 'Presets', 'QuantizePVT', 'Quantize', 'Takehiro', 'Reservoir', 'MPEGMode', 'BitStream', 'Version', 'VBRTag']) M[n] = req(n);
    function Stub() { this.setModules = function () {}; }
    const real = new GainAnalysisModule();
    /* the wrapper handed to Lame and BitStream as their `ga` */
    const ga = {
        InitGainAnalysis: (rg, f) => real.InitGainAnalysis(rg, f),
        AnalyzeSamples(rg, l, lp, r, rp, n, nch) {
            if (n % 8) throw new Error('a piece of ' + n + ' samples is not a multiple of eight: the reference cannot analyse this case');
            for (let c = 0; c < nch; c++) { const a = c ? r : l, p = c ? rp : lp; for (let i = 0; i < n; i++) log.samples[c].push(a[p + i]); }
            for (let o = 0; o < n; o += 8) {
                if (log.stopAt && log.fed + 8 > log.stopAt) throw new Error('fed past the point where the module hangs');
                const before = log.bins ? Int32Array.from(rg.A) : null;
                if (real.AnalyzeSamples(rg, l, lp + o, r, rp + o, 8, nch) != 1) throw new Error('AnalyzeSamples failed');
                log.fed += 8;
                if (before && rg.totsamp == 0) { for (let i = 0; i < before.length; i++) if (rg.A[i] != before[i]) log.bins.push(i); }
            }
            return 1;
        },
        GetTitleGain(rg) { log.hist = Int32Array.from(rg.A); return real.GetTitleGain(rg); }
    };
    const lame = new M.Lame(), gaud = new Stub(), bs = new M.BitStream();
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
    if (lame.lame_init_params(gfp) != 0) throw new Error('lame_init_params failed');
    const gfc = gfp.internal_flags;
    gfc.findReplayGain = true;
    if (real.InitGainAnalysis(gfc.rgdata, gfp.out_samplerate) != 1) throw new Error('InitGainAnalysis failed');
    let cap = 0 | (1.25 * 1152 + 7200), mp3buf = new Int8Array(cap);
    return {
        gfp, gfc,
        encodeBuffer(left, right) {
            if (channels == 1) right = left;
            return lame.lame_encode_buffer(gfp, left, right, left.length, mp3buf, 0, cap);
        },
        flush() { return lame.lame_encode_flush(gfp, mp3buf, 0, cap); }
    };
}

/* ---- this file's restatement: both filters from zero state at `a`, the reference's operation order and Float32 stores ---- */
function filt(R, x, a, b) {
    const n = b - a, xs = new Float64Array(n + 10), ys = new Float64Array(n + 10), os = new Float64Array(n + 10), ky = R.ky, kb = R.kb;
    for (let i = 0; i < n; i++) xs[i + 10] = x[a + i];
    for (let k = 10; k < n + 10; k++) {
        ys[k] = Math.fround(1e-10 + xs[k] * ky[0] - ys[k - 1] * ky[1] + xs[k - 1] * ky[2] - ys[k - 2] * ky[3] + xs[k - 2] * ky[4] - ys[k - 3] * ky[5] + xs[k - 3] * ky[6]
            - ys[k - 4] * ky[7] + xs[k - 4] * ky[8] - ys[k - 5] * ky[9] + xs[k - 5] * ky[10] - ys[k - 6] * ky[11] + xs[k - 6] * ky[12] - ys[k - 7] * ky[13]
            + xs[k - 7] * ky[14] - ys[k - 8] * ky[15] + xs[k - 8] * ky[16] - ys[k - 9] * ky[17] + xs[k - 9] * ky[18] - ys[k - 10] * ky[19] + xs[k - 10] * ky[20]);
        os[k] = Math.fround(ys[k] * kb[0] - os[k - 1] * kb[1] + ys[k - 1] * kb[2] - os[k - 2] * kb[3] + ys[k - 2] * kb[4]);
    }
    return os.subarray(10);
}
function wsum(o, a, window) {
    let s = 0, k = 0;
    for (; k + 8 <= window; k += 8) {
        const q = (j) => o[a + k + j] * o[a + k + j];
        s += q(0) + q(1) + q(2) + q(3) + q(4) + q(5) + q(6) + q(7);
    }
    for (; k < window; k++) s += o[a + k] * o[a + k];
    return s;
}
function binOf(e, window) { const val = 100. * 10. * Math.log10(e / window * 0.5 + 1.e-37); return val <= 0 ? 0 : Math.min(0 | val, 11999); }
function bins(R, chans, restart) {
    const n = chans[0].length, nwin = Math.floor(n / R.window), out = [];
    const thru = restart === null ? chans.map((c) => filt(R, c, 0, n)) : null;
    for (let k = 0; k < nwin; k++) {
        const sums = chans.map((c, ci) => {
            if (thru) return wsum(thru[ci], k * R.window, R.window);
            const a = Math.max(0, k * R.window - restart);
            return wsum(filt(R, c, a, (k + 1) * R.window), k * R.window - a, R.window);
        });
        out.push(binOf(sums[0] + sums[sums.length - 1], R.window));
    }
    return out;
}
function radio(hist) {
    let elems = 0;
    for (const v of hist) elems += v;
    let upper = 0 | Math.ceil(elems * (1. - 0.95)), i;
    for (i = hist.length; i-- > 0;) if ((upper -= hist[i]) <= 0) break;
    return { i, at: (j) => Math.floor((64.82 - j / 100.) * 10.0 + 0.5) | 0 };
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

/* [name, channels in, samplerate, kbps, options, corpus, frames of 1152 samples, record every window's bin]  -- calls of 1152 samples, flushed */
const CONFIGS = [
    ['mono_48000_64', 1, 48000, 64, {}, 'sine', 24, true],
    ['stereo_48000_128', 2, 48000, 128, {}, 'bursts', 30, false],
    ['stereo_48000_320', 2, 48000, 320, {}, 'sine', 24, false],
    ['joint_48000_128', 2, 48000, 128, { jointStereo: true }, 'centre_sine', 24, false],
    ['resv_stereo_48000_128', 2, 48000, 128, { reservoir: true }, 'sine', 24, false],
    ['downmix_48000_96', 2, 48000, 96, { downmix: true }, 'bursts', 24, false],
    ['resample_48000_24000_stereo_64', 2, 48000, 64, {}, 'bursts', 40, false],
    ['stereo_32000_96', 2, 32000, 96, {}, 'sine', 20, false],
    ['mono_32000_48', 1, 32000, 48, {}, 'sine', 20, false],
    ['stereo_24000_64_mpeg2', 2, 24000, 64, {}, 'sine', 16, false],
    ['mono_16000_32_mpeg2', 1, 16000, 32, {}, 'bursts', 12, false],
    ['stereo_16000_48_mpeg2', 2, 16000, 48, {}, 'bursts', 12, true],
    ['stereo_12000_32_mpeg25', 2, 12000, 32, {}, 'bursts', 10, false],
    ['mono_11025_24_mpeg25', 1, 11025, 24, {}, 'bursts', 10, false],
    ['mono_8000_16_mpeg25', 1, 8000, 16, {}, 'bursts', 8, false],
    ['stereo_8000_24_mpeg25', 2, 8000, 24, {}, 'sine', 8, false]
];
/* the two rates whose window is no multiple of eight: [name, channels, samplerate, kbps, corpus, call lengths] -- no flush, the module stops in front of the first window's end */
const PARTIAL = [
    ['stereo_44100_128_first_2200', 2, 44100, 128, 'sine', [1152, 1048]],
    ['mono_22050_32_first_1096', 1, 22050, 32, 'bursts', [1096]]
];

function pcmOf(corpus, N, ch) {
    let [L, R] = gen[corpus.replace('centre_', '')](N, ch);
    if (corpus.startsWith('centre_')) [L, R] = centre(L, R);
    return [L, R];
}

/* one case at a given length */
function runCase([name, ch, sr, kbps, opts, corpus, , wantBins], frames) {
    const N = frames * 1152;
    const [L, R] = pcmOf(corpus, N, ch);
    const log = { fed: 0, samples: [[], []], bins: [], hist: null };
    const enc = refEncoder(ch, sr, kbps, opts, log);
    for (let p = 0; p < N; p += 1152) enc.encodeBuffer(L.subarray(p, p + 1152), ch == 2 ? R.subarray(p, p + 1152) : null);
    enc.flush();
    const fs_out = enc.gfp.out_samplerate, Rt = RT[fs_out], C = enc.gfc.channels_out;
    if (!log.hist) throw new Error(name + ': GetTitleGain was not reached');
    const chans = []; for (let c = 0; c < C; c++) chans.push(Float32Array.from(log.samples[c]));
    /* this file's restatement against the live module, window by window */
    const thru = bins(Rt, chans, null);
    if (thru.length != log.bins.length || thru.some((b, k) => b != log.bins[k])) throw new Error(name + ': the restatement differs from the live module -- nothing written');
    const rest = bins(Rt, chans, Rt.wf);
    let diff = 0, worst = 0;
    for (let k = 0; k < thru.length; k++) { if (rest[k] != thru[k]) diff++; worst = Math.max(worst, Math.abs(rest[k] - thru[k])); }
    const nz = {}; log.hist.forEach((v, i) => { if (v) nz[i] = v; });
    const r = radio(log.hist);
    if (r.at(r.i) != enc.gfc.RadioGain) throw new Error(name + ': RadioGain ' + enc.gfc.RadioGain + ' is not what the histogram gives, ' + r.at(r.i));
    const h = crypto.createHash('md5'); for (const c of chans) h.update(buf(c));
    const pm = crypto.createHash('md5'); pm.update(buf(L)); if (R) pm.update(buf(R));
    const o = { name, channels: ch, samplerate: sr, kbps, corpus, nsamples: N, call: 1152, out_samplerate: fs_out, channels_out: C, fed: log.fed, windows: thru.length,
                histogram: nz, RadioGain: enc.gfc.RadioGain, percentile_bin: r.i, margin_ok: (r.at(r.i - 2) == r.at(r.i) && r.at(r.i + 2) == r.at(r.i)) ? 1 : 0,
                restart_diff: diff, restart_worst: worst, analysed_md5: h.digest('hex'), pcm_md5: pm.digest('hex') };
    if (wantBins) o.bins = log.bins;
    for (const k of ['jointStereo', 'reservoir', 'downmix']) if (opts[k]) o[k] = 1;
    console.log(name, 'frames', frames, 'out', fs_out, 'fed', log.fed, 'windows', thru.length, 'RadioGain', enc.gfc.RadioGain, 'margin_ok', o.margin_ok, 'restart differs in', diff, 'worst', worst);
    return o;
}
/* tenth_db is compared exactly only where the percentile bin is not within two bins of a rounding step of RadioGain (margin_ok), and three quarters of the
 * cases must be such: a case whose first length is not takes the first of its length + 2, + 4, + 6 frames that is -- the choice looks at the reference alone */
const cases = [];
for (const cfg of CONFIGS) {
    let pick = null;
    for (const extra of [0, 2, 4, 6]) { const o = runCase(cfg, cfg[6] + extra); if (!pick) pick = o; if (o.margin_ok) { pick = o; break; } }
    cases.push(pick);
}
if (4 * cases.filter((c) => c.margin_ok).length < 3 * cases.length) throw new Error('fewer than three quarters of the cases are margin_ok');
const partial = [];
for (const [name, ch, sr, kbps, corpus, lens] of PARTIAL) {
    const N = lens.reduce((a, b) => a + b, 0);
    const [L, R] = pcmOf(corpus, N, ch);
    const log = { fed: 0, samples: [[], []], bins: null, hist: null, stopAt: N };
    const enc = refEncoder(ch, sr, kbps, {}, log);
    let p = 0;
    for (const m of lens) { enc.encodeBuffer(L.subarray(p, p + m), ch == 2 ? R.subarray(p, p + m) : null); p += m; }
    const rg = enc.gfc.rgdata, C = enc.gfc.channels_out;
    if (log.fed != N || rg.totsamp != N) throw new Error(name + ': fed ' + log.fed + ', totsamp ' + rg.totsamp);
    const h = crypto.createHash('md5'); for (let c = 0; c < C; c++) h.update(buf(Float32Array.from(log.samples[c])));
    const bitsOf = (a) => Array.from(new Int32Array(Float32Array.from(a).buffer));
    const f64bits = (x) => { const b = Buffer.alloc(8); b.writeDoubleLE(x); return b.toString('hex'); };
    const o = { name, channels: ch, samplerate: sr, kbps, corpus, nsamples: N, call_lens: lens, out_samplerate: enc.gfp.out_samplerate, channels_out: C, fed: N, analysed_md5: h.digest('hex'),
                lstep_md5: md5(buf(Float32Array.from(rg.lstepbuf.subarray(10, 10 + N)))), lout_md5: md5(buf(Float32Array.from(rg.loutbuf.subarray(10, 10 + N)))),
                rstep_md5: md5(buf(Float32Array.from(rg.rstepbuf.subarray(10, 10 + N)))), rout_md5: md5(buf(Float32Array.from(rg.routbuf.subarray(10, 10 + N)))),
                lout_tail_bits: bitsOf(rg.loutbuf.subarray(10 + N - 16, 10 + N)), lsum_hex: f64bits(rg.lsum), rsum_hex: f64bits(rg.rsum) };
    partial.push(o);
    console.log(name, 'out', o.out_samplerate, 'fed', N, 'lsum', rg.lsum, 'rsum', rg.rsum);
}
const wf = {}; for (const k of Object.keys(RT)) wf[k] = RT[k].wf;
fs.writeFileSync(path.join(OUT, 'golden_replaygain.json'), JSON.stringify({ generator: 'tests/tools/gen_golden_replaygain.js',
    reference: 'zhuker/lamejs v1.2.1, unmodified modules wired as index.js:73-111; Arrays.ill, the undefined names of GainAnalysis.js / BitStream.js and findReplayGain supplied from ' +
               'outside, AnalyzeSamples fed eight samples per call; restart_diff from the generator\'s own restatement, equal to the live module window by window, under node ' + process.version,
    wf, cases, partial }, null, 1));
console.log('wrote', cases.length, '+', partial.length, 'cases');
