/*
 * TEST TOOL (needs the reference, sources or single-file build): the resampler windows of a { fractionalResample } blob against a LIVE
 * instance of the unmodified reference -- gfc.blackfilt as its fill_buffer_resample builds it in its first call -- bit for bit, all
 * 2 * bpc + 1 rows of 32 taps, for one (channels, sample rate, kbps) triple per distinct ratio; bpc, filter_l and the ratio too.
 * Prints one JSON line { ratios, rows, mismatches }.      usage: node tests/tools/check_fracresample_tables.js
 */
'use strict';
const { hookedRef, fractionalTriples } = require('./frac_ref.js');
const tables = require('../../lamejs_amd/js/tables.js');
const perRatio = [];
for (const t of fractionalTriples()) if (!perRatio.some((u) => u.ratio == t.ratio)) perRatio.push(t);
let rows = 0, bad = 0;
for (const t of perRatio) {
    const p = tables.resolveParams(t.ch, t.sr, t.kb, { fractionalResample: true });
    const e = hookedRef(t.ch, t.sr, t.kb);
    e.encodeBuffer(new Int16Array(64), t.ch == 2 ? new Int16Array(64) : undefined);
    const bf = e.gfc.blackfilt, bpc = p.rs_bpc;
    if (p.rs_filter_l != 31 || e.gfc.resample_ratio !== p.resample_ratio || p.rs_blackfilt.length != (2 * bpc + 1) * 32) bad++;
    for (let j = 0; j <= 2 * bpc; j++) {
        rows++;
        if (!bf[j] || bf[j].length != 32) { bad++; continue; }
        for (let i = 0; i < 32; i++) if (!Object.is(bf[j][i], p.rs_blackfilt[j * 32 + i])) { bad++; break; }
    }
    if (bf[2 * bpc + 1] !== undefined && bf[2 * bpc + 1] !== null) bad++;      /* the reference built exactly 2 * bpc + 1 rows */
}
console.log(JSON.stringify({ ratios: perRatio.length, rows, mismatches: bad }));
process.exit(bad ? 1 : 0);
