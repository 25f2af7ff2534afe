// k_quant_probe.h -- TEST HOOK (lhip_debug_quant_probe): the quantization search's pure functions over caller-supplied records.  The body calls the device
// functions of k_quant.h that the shipped kernels call -- q_ath_pseudo, q_init_outer_loop, q_init_xrpow, q_calc_xmin, q_pecalc, q_count_bits<NPL>,
// q_count_bits<NPL_HEAD>, q_calc_noise_ -- and restates none of them; what it adds is the plumbing between a record and a wave's LDS record.  No
// shipped kernel calls anything in this file, and the probe touches no stream state: its inputs and outputs are the caller's records alone.
// The record layouts are the ones include/lamejs_hip.h states (little-endian, natural alignment).
#pragma once
#include "k_quant.h"

namespace lhip {

enum { PROBE_IN_BYTES = 4144, PROBE_OUT_BYTES = 6352, PROBE_NOISE_CALLS = 8 };

struct ProbeIn {
    float xr[576];                 // natural order, as lhip_debug_read(0) gives it
    float ratio[E_STRIDE];         // the E layout of lhip_debug_read(2)
    double ath_adjust;
    int32_t block_type, global_gain, scalefac_scale, preflag, subblock_gain[3], scalefac[SFBMAX];
    int32_t flags, pad_;           // bit 0: ix_in is given
    int16_t ix_in[576];            // magnitudes, quantizer line order
};
struct ProbeEval {                 // one quantize + count at the record's gain, all scalefactors zero
    int32_t bits, big_values, count1, count1table_select, table_select[3], region0_count, region1_count, ran;
    int16_t ix[576];
};
struct ProbeNoise {                // one calc_noise call
    double max_noise;
    int32_t over_count, over_SSD, ran, pad_;
    float distort[SFBMAX + 1];
};
struct ProbeOut {
    double xrpow_max, pe;
    int32_t active, max_nonzero_coeff, tail0, pad_;
    float xr[576];                 // after the analog-silence rule, quantizer line order
    float xmin[SFBMAX + 1];
    ProbeEval ev[2];               // [0] q_count_bits<NPL>, [1] q_count_bits<NPL_HEAD> (only where tail0 is set)
    ProbeNoise nz[PROBE_NOISE_CALLS];   // calls a .. h
};
// the kernel's one argument (g_quant_probe, lhip_probe.cpp); `grid` = the workgroups launched
struct ProbeArgs { Tables T; PowBase pb; const ProbeIn* in; ProbeOut* out; int n, grid; };
static_assert(sizeof(ProbeIn) == PROBE_IN_BYTES && sizeof(ProbeOut) == PROBE_OUT_BYTES, "the record layouts of include/lamejs_hip.h");
static_assert(offsetof(ProbeIn, ix_in) % 4 == 0 && offsetof(ProbeOut, ev) % 8 == 0 && sizeof(ProbeEval) % 8 == 0 && offsetof(ProbeEval, ix) % 4 == 0, "word copies of the quantized lines");

// The body: in the simulations, and in the HIP translation unit that holds the kernel (lhip_probe.cpp); lhip_api.cpp's HIP build needs the records alone.
#if defined(LHIP_HOSTSIM) || defined(LHIP_PROBE_BODY)
// an evaluation's fields; a refused gain (LARGE_BITS) leaves everything but `bits` and `ran` as the host zeroed it
LHIP_DEV void probe_put_eval(ProbeEval& e, const GI& g, int bits, int lane, const QuantLds& L) {
    if (lane == 0) { e.bits = bits; e.ran = 1; }
    if (bits == LARGE_BITS) return;
    if (lane == 0) {
        e.big_values = g.big_values; e.count1 = g.count1; e.count1table_select = g.count1table_select;
        for (int i = 0; i < 3; i++) e.table_select[i] = g.table_select[i];
        e.region0_count = g.region0_count; e.region1_count = g.region1_count;
    }
    for (int i = lane; i < 288; i += LHIP_NL) ((uint32_t*)e.ix)[i] = ((const uint32_t*)L.ixw)[i];
}

LHIP_DEV void kb_quant_probe(const Tables& T, const PowBase& pb10, const ProbeIn* in, ProbeOut* out, int r, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = lane_anew(lane);
    const ProbeIn& I = in[r];
    ProbeOut& O = out[r];
    const double ath_adjust = unid(I.ath_adjust);
    const int bt = uni(I.block_type), gain = uni(I.global_gain), flags = uni(I.flags);
    // ---- 1. init ----
    GI g;
    q_ath_pseudo(T, pb10, ath_adjust, lane, L, Q);
    XrSrc X; X.a = I.xr; X.b = nullptr; X.side = 0;
    q_init_outer_loop(T, pb10, ath_adjust, g, bt, X, nullptr, 0, lane, L, Q);
    const int active = q_init_xrpow(g, lane, L, Q);
    for (int i = lane; i < 576; i += LHIP_NL) O.xr[i] = L.xr[i];
    if (lane == 0) { O.active = active; O.xrpow_max = g.xrpow_max; }
    if (!active) { wave_sync(); return; }
    // ---- 2. xmin, perceptual entropy ----
    const double masking_lower = (bt != SHORT_TYPE) ? T.masking_lower_long : T.masking_lower_short;
    q_calc_xmin(T, ath_adjust, masking_lower, I.ratio, g, lane, L, Q, 1);
    uni_gi(g);
    LHIP_LANE_ONCE(sfb, 0, g.psymax) O.xmin[sfb] = L.xmin[sfb];
    {
        const double pe = q_pecalc(I.ratio, bt == SHORT_TYPE, masking_lower);
        if (lane == 0) { O.max_nonzero_coeff = g.max_nonzero_coeff; O.tail0 = g.tail0; O.pe = pe; }
    }
    // ---- 3. one evaluation at the record's gain, scalefactors zero (the bin search's state) ----
    for (int i = lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0u;
    wave_sync();
    PrevNoise pn; pn.gain = 0; pn.sfb_count1 = 0;
    int asg = 0, bits;
    GI w = g; w.global_gain = gain;
    bits = q_count_bits<NPL>(T, w, L.sfw, L.ixw, 0, pn, &asg, lane, L, Q);
    uni_gi(w); bits = uni(bits);
    wave_sync();
    probe_put_eval(O.ev[0], w, bits, lane, L);
    if (g.tail0) {
        // the short round count: what the unit before left in the words 256..287 is there, and is zeroed as q_unit zeroes it
        for (int i = 256 + lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0x1fff1fffu;
        wave_sync();
        for (int i = 256 + lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0u;
        wave_sync();
        w = g; w.global_gain = gain;
        bits = q_count_bits<NPL_HEAD>(T, w, L.sfw, L.ixw, 0, pn, &asg, lane, L, Q);
        uni_gi(w); bits = uni(bits);
        wave_sync();
        probe_put_eval(O.ev[1], w, bits, lane, L);
    }
    // ---- 4. calc_noise with the record's scalefactor state, on ix_in or on the lines of step 3 (all zero where the gain was refused) ----
    w = g; w.global_gain = gain; w.scalefac_scale = uni(I.scalefac_scale); w.preflag = uni(I.preflag);
    w.subblock_gain[0] = uni(I.subblock_gain[0]); w.subblock_gain[1] = uni(I.subblock_gain[1]); w.subblock_gain[2] = uni(I.subblock_gain[2]); w.subblock_gain[3] = 0;
    LHIP_LANE_ONCE(i, 0, SFBMAX) L.sfw[i] = I.scalefac[i];
    int cached_calls = bits != LARGE_BITS;
    if (flags & 1) {
        for (int i = lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = ((const uint32_t*)I.ix_in)[i];
        wave_sync();
        // calc_noise trusts that the lines were quantized at this gain from this xrpow (may_big); the caller's lines need not have been -- an amplified
        // band's xrpow was scaled -- so values beyond the part of pow43 staged in LDS are announced through xrpow_max
        int mx = 0;
        for (int i = lane; i < 576; i += LHIP_NL) if (mx < L.ixw[i]) mx = L.ixw[i];
        mx = wave_max(mx);
        if (mx >= QT_N - 1) w.xrpow_max = 1e30;
        cached_calls = 1;
    }
    wave_sync();
    // g, h: the border of the 3-line body -- the highest band that ends at or below line 192 alone fresh, then the band above it alone
    const int b3 = uni(T.noise_hib3[bt == SHORT_TYPE]);
    const int ncalls = !cached_calls ? 2 : (b3 >= 0 && b3 + 1 < g.psymax) ? PROBE_NOISE_CALLS : 6;
#pragma nounroll
    for (int k = 0; k < ncalls; k++) {
        // a: fresh, max_noise wanted; b: fresh, not wanted; c: fills an empty cache; d: every band cached; e: band 0 alone is fresh; f: a mix; g, h: above
        const int use_pn = k >= 2, need_max = (k == 0 || k == 3 || k == 5 || k == 7);
        if (k == 2) {
            LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) { L.pn_step[i] = 0; L.pn_dist[i] = 0.f; L.pn_x[i] = 1.0; L.pn_cls[i] = 0; }
            pn.gain = 0; pn.sfb_count1 = 0;
        }
        if (k == 4 && lane == 0) L.sfw[0] ^= 1;
        if (k == 5) { LHIP_LANE_ONCE(sfb, 0, g.psymax) if (sfb % 3 == 0) L.sfw[sfb] ^= 1; }
        if (k >= 6 && lane == 0) L.sfw[b3 + (k - 6)] ^= 1;
        wave_sync();
        NoiseRes nr;
        q_calc_noise_(T, w, L.sfw, L.ixw, &nr, use_pn, pn, need_max, lane, L, Q);
        ProbeNoise& N = O.nz[k];
        if (lane == 0) { N.max_noise = nr.max_noise; N.over_count = nr.over_count; N.over_SSD = nr.over_SSD; N.ran = 1; }
        LHIP_LANE_ONCE(sfb, 0, g.psymax) N.distort[sfb] = L.distort[sfb];
        wave_sync();
    }
}
#endif

}  // namespace lhip
