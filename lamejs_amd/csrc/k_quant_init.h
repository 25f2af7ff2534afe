// k_quant_init.h -- from the MDCT output to a granule-channel ready for the search: init_outer_loop with the analog-silence rule, init_xrpow,
// the ordered band sums (fold_band_sums) and calc_xmin with the limits derived beside it (max_nonzero_coeff, firstcut, tail0).
#pragma once
#include "k_quant_tabs.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// init_outer_loop (Quantize.js:204-306) incl. psfb21_analogsilence (147-202)
// xr_g: this granule-channel's MDCT output in HBM (natural order)
// ---------------------------------------------------------------------------------------------
// xr_wb != nullptr: lines zeroed by the analog-silence rule are also zeroed in HBM, so that a later pass over the
// same granule (kb_validate) can skip the rule (`skip_silence`); the rule is idempotent.
// Where the lines come from: the channel's own MDCT output, or -- frames that joint stereo codes M/S -- mid / side of both
// channels' outputs (ms_convert, Quantize.js:76-83).  M/S granules are never written back (the L / R lines must survive for the
// other channel and for later passes), so they never skip the silence rule either.
struct XrSrc { const float* a; const float* b; int side; };       // b == nullptr: a is the spectrum; else a = left, b = right
LHIP_DEV XrSrc xr_source(const Workspace& W, int C, int gslot, int ch, int ms) {
    XrSrc X;
    if (!ms) { X.a = W.xr + ((int64_t)gslot * C + ch) * 576; X.b = nullptr; X.side = 0; }
    else { X.a = W.xr + (int64_t)gslot * C * 576; X.b = X.a + 576; X.side = ch; }
    return X;
}
LHIP_DEV float xr_at(const XrSrc& X, int i) {
    if (!X.b) return X.a[i];
    const double l = X.a[i], r = X.b[i];
    return X.side ? (float)((l - r) * (LHIP_SQRT2 * 0.5)) : (float)((l + r) * (LHIP_SQRT2 * 0.5));
}
// The analog-silence thresholds of a frame (Quantize.js:147-202: athAdjust of the pseudo bands' ATH, scaled by the band factor of
// sfb21 / sfb12): functions of the frame's ATH adjustment alone, so they are formed once per frame -- [0..5] for long blocks,
// [6..11] for short ones -- and not once per granule and channel.
LHIP_DEV void q_ath_pseudo(const Tables& T, const PowBase& pb10, double ath_adjust, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = lane_anew(lane);
    wave_sync();
    LHIP_LANE_ONCE(e, 0, PSFB21 + PSFB12) {
        double a = athAdjust(T, pb10, ath_adjust, Q.ath_psfb[e], T.ATH_floor);
        const double f = (double)Q.fact_psfb[e < PSFB21 ? 0 : 1];
        if (f > 1e-12) a *= f;
        L.ath_pseudo[e] = a;
    }
    wave_sync();
}

// the lines of a granule-channel from HBM, in the order the quantizer keeps them (short blocks: the three windows of a band as
// consecutive runs).  All loads of a lane are issued before the first one is needed (a lane-strided loop compiles to one load per
// trip, each waited for by itself: nine round trips to memory).
LHIP_DEV void q_load_lines(const XrSrc& X, int is_short, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
#if LHIP_NL == 1
    for (int d = 0; d < 576; d++) {
        int src = d;
        if (is_short) {
            const int sw = Q.l2s_short[d], sfb = sw / 3, win = sw - 3 * sfb;
            const int st = Q.sfb_s[sfb], w = Q.sfb_s[sfb + 1] - st;
            src = 3 * (st + (d - 3 * st - win * w)) + win;
        }
        L.xr[d] = xr_at(X, src);
    }
    (void)lane;
#else
    enum { NV = 576 / LHIP_NL };
    int src[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int d = lane + LHIP_NL * k;
        src[k] = d;
        if (is_short) {
            const int sw = Q.l2s_short[d], sfb = sw / 3, win = sw - 3 * sfb;
            const int st = Q.sfb_s[sfb], w = Q.sfb_s[sfb + 1] - st;
            src[k] = 3 * (st + (d - 3 * st - win * w)) + win;
        }
    }
    float va[NV], vb[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) { va[k] = X.a[src[k]]; vb[k] = 0.f; }
    if (X.b) {
#pragma unroll
        for (int k = 0; k < NV; k++) vb[k] = X.b[src[k]];
    }
#pragma unroll
    for (int k = 0; k < NV; k++) { LHIP_PIN_LOADED(va[k]); LHIP_PIN_LOADED(vb[k]); }
#pragma unroll
    for (int k = 0; k < NV; k++) {
        float v = va[k];
        if (X.b) { const double l = va[k], r = vb[k]; v = X.side ? (float)((l - r) * (LHIP_SQRT2 * 0.5)) : (float)((l + r) * (LHIP_SQRT2 * 0.5)); }
        L.xr[lane + LHIP_NL * k] = v;
    }
#endif
}

// ath_ready: L.ath_pseudo holds this frame's thresholds (q_ath_pseudo); only read when the silence rule runs
LHIP_DEV void q_init_outer_loop(const Tables& T, const PowBase& pb10, double ath_adjust, GI& g, int block_type,
                                const XrSrc& xr_g, float* xr_wb, int skip_silence, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    unsigned long long tmi_ = PH_NOW(); (void)tmi_;
    (void)pb10; (void)ath_adjust;
#if defined(LHIP_PHASE_PROF) && !defined(LHIP_HOSTSIM)
    __builtin_amdgcn_s_waitcnt(0);           // profiling build only: everything this wave still has in flight (stores of the previous granule)
    PH_MARK(L, PH_DRAIN, tmi_);
#endif
    g.part2_3_length = 0; g.big_values = 0; g.count1 = 0; g.global_gain = 210; g.scalefac_compress = 0;
    g.block_type = block_type;
    g.table_select[0] = g.table_select[1] = g.table_select[2] = 0;
    g.subblock_gain[0] = g.subblock_gain[1] = g.subblock_gain[2] = g.subblock_gain[3] = 0;
    g.region0_count = 0; g.region1_count = 0; g.preflag = 0; g.scalefac_scale = 0; g.count1table_select = 0;
    g.part2_length = 0; g.sfb_lmax = SBPSY_l; g.sfb_smin = SBPSY_s;
    g.psy_lmax = T.sfb21_extra ? SBMAX_l : SBPSY_l;
    g.psymax = g.psy_lmax; g.sfbmax = g.sfb_lmax; g.sfbdivide = 11;
    g.count1bits = 0; g.max_nonzero_coeff = 575; g.xrpow_max = 0; g.firstcut = 64; g.tail0 = 0;
    int nsfb;
    if (block_type == SHORT_TYPE) {
        g.sfb_smin = 0; g.sfb_lmax = 0;
        g.psymax = 3 * ((T.sfb21_extra ? SBMAX_s : SBPSY_s));
        g.sfbmax = 3 * SBPSY_s;
        g.sfbdivide = g.sfbmax - 18;
        g.psy_lmax = 0;
        nsfb = 3 * SBMAX_s;
        LHIP_LANE_ONCE(i, 0, nsfb) {
            const int sfb = i / 3, win = i - 3 * sfb;
            const int w = Q.sfb_s[sfb + 1] - Q.sfb_s[sfb];
            L.width[i] = (int16_t)w; L.window[i] = (int16_t)win; L.start[i] = (int16_t)(3 * Q.sfb_s[sfb] + win * w);
        }
        if (lane == 0) L.start[nsfb] = 576;
        q_load_lines(xr_g, 1, lane, L, Q);       // re-ordered: within each short sfb the three windows become consecutive runs
    } else {
        nsfb = SBMAX_l;
        LHIP_LANE_ONCE(i, 0, SBMAX_l) {
            L.width[i] = (int16_t)(Q.sfb_l[i + 1] - Q.sfb_l[i]); L.window[i] = 3; L.start[i] = (int16_t)Q.sfb_l[i];
        }
        if (lane == 0) L.start[SBMAX_l] = 576;
        q_load_lines(xr_g, 0, lane, L, Q);
    }
    LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) { L.sfw[i] = 0; L.sfb[i] = 0; }
    wave_sync();
    PH_MARK(L, PH_COPY, tmi_);

    // analog silence in the pseudo bands above sfb21 / sfb12: zero trailing lines below the adjusted ATH (thresholds: q_ath_pseudo)
    if (skip_silence) return;
    if (block_type != SHORT_TYPE) {
        const int lo = Q.psfb21[0];
        int top = lo - 1;                       // highest line that is NOT below its threshold
        for (int j = lo + lane; j < 576; j += LHIP_NL) {
            int gsfb = 0;                       // pseudo band of line j: the number of inner borders at or below it
#pragma unroll
            for (int q = 1; q < PSFB21; q++) gsfb += (Q.psfb21[q] <= j);
            if (!(d_abs((double)L.xr[j]) < L.ath_pseudo[gsfb])) top = j;   // ascending j per lane
        }
        top = wave_max(top);
        for (int j = lo + lane; j < 576; j += LHIP_NL) if (j > top) { L.xr[j] = 0; if (xr_wb) xr_wb[j] = 0; }
        PH_MARK(L, PH_PUBLISH, tmi_);
    } else {
        const int s12 = Q.sfb_s[12], w12 = Q.sfb_s[13] - s12;
        for (int block = 0; block < 3; block++) {
            const int lo = s12 * 3 + w12 * block;
            int top = lo - 1;
            for (int j = lo + lane; j < lo + w12; j += LHIP_NL) {
                const int rel = j - lo + Q.psfb12[0];
                int gsfb = 0;
#pragma unroll
                for (int q = 1; q < PSFB12; q++) gsfb += (Q.psfb12[q] <= rel);
                if (!(d_abs((double)L.xr[j]) < L.ath_pseudo[PSFB21 + gsfb])) top = j;
            }
            top = wave_max(top);
            for (int j = lo + lane; j < lo + w12; j += LHIP_NL) if (j > top) { L.xr[j] = 0; if (xr_wb) xr_wb[3 * (s12 + (j - lo)) + block] = 0; }
        }
    }
    wave_sync();
}

// init_xrpow (Quantize.js:92-138); returns 1 if the granule has energy
LHIP_DEV int q_init_xrpow(GI& g, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    float m = 0.f;
    double sum = 0;
    for (int i = lane; i < 576; i += LHIP_NL) {
        const double tmp = d_abs((double)L.xr[i]);
        sum += tmp;
        const float v = (float)d_sqrt(tmp * d_sqrt(tmp));
        L.xrpow[i] = v;
        m = fmax_nonneg(m, v);
    }
    m = wave_maxf_pos(m);
    g.xrpow_max = m;
    // `sum > 1e-20` only separates digital silence from signal; the reduction order cannot change the verdict
    // except within 1e-14 (relative) of the threshold itself
    const int has = wave_sumd(sum) > 1E-20;
    wave_sync();
    return has;
}

// the first band that reaches past max_nonzero_coeff (quantize_xrpow's walk ends inside it, Takehiro.js:212-250); 64 if none does
LHIP_DEV void q_set_firstcut(GI& g, int lane, const QuantLds& L) {
    const int sfbmax = (g.block_type == SHORT_TYPE) ? 38 : 21;
    uint64_t m = 0;
    LHIP_LANE_ONCE(sfb, 0, (sfbmax) + 1) if (L.start[sfb] + L.width[sfb] > g.max_nonzero_coeff) m |= 1ull << sfb;
    m = wave_lane_bits(m);
    g.firstcut = m ? (int)__builtin_ctzll(m) : 64;
}

// Ordered (line order) f64 sums of per-line terms over scalefactor bands, all bands at once, as a systolic fold:
// lane l owns NLN consecutive lines and folds their terms, in order, onto the running sum handed over by lane l-1
// (reset at band starts); ceil(longest band / NLN) + 1 hand-overs reproduce the strictly sequential sums exactly.
// Result: L.nsum[band] for every band whose length is <= maxlen.
enum { NLN_FOLD = 576 / LHIP_NL };
LHIP_DEV void fold_band_sums(double (&tq)[NLN_FOLD], const uint8_t* l2s, int maxlen, int lane, QuantLds& L) {
#if LHIP_NL == 1
    (void)maxlen; (void)lane;
    double sacc = 0.0;
    for (int j = 0; j < 576; j++) {
        if (j == 0 || l2s[j - 1] != l2s[j]) sacc = 0.0;
        sacc += tq[j];
        if (j == 575 || l2s[j + 1] != l2s[j]) L.nsum[l2s[j]] = sacc;
    }
#else
    unsigned endm = 0;
    double keep[NLN_FOLD]; int bnd[NLN_FOLD];
    int prevb = (lane == 0) ? -1 : (int)l2s[NLN_FOLD * lane - 1];
#pragma unroll
    for (int k = 0; k < NLN_FOLD; k++) {
        const int j = NLN_FOLD * lane + k;
        bnd[k] = l2s[j];
        keep[k] = (bnd[k] != prevb) ? 0.0 : 1.0;       // fma(sum, keep, t): `sum + t` or a fresh `t`, one rounding either way
        prevb = bnd[k];
    }
    const int nextb = (lane == LHIP_NL - 1) ? -1 : (int)l2s[NLN_FOLD * (lane + 1)];
#pragma unroll
    for (int k = 0; k < NLN_FOLD; k++) if (bnd[k] != (k + 1 < NLN_FOLD ? bnd[k + 1 < NLN_FOLD ? k + 1 : k] : nextb)) endm |= 1u << k;
    const int nsteps = (maxlen + NLN_FOLD - 1) / NLN_FOLD + 1;
    double carry = 0.0;
    for (int st = 0; st + 1 < nsteps; st++) {
        double sacc = carry;
#pragma unroll
        for (int k = 0; k < NLN_FOLD; k++) sacc = __builtin_fma(sacc, keep[k], tq[k]);
        carry = wave_shr1d(sacc, 0.0);
    }
    {
        double sacc = carry;
#pragma unroll
        for (int k = 0; k < NLN_FOLD; k++) { sacc = __builtin_fma(sacc, keep[k], tq[k]); tq[k] = sacc; }
    }
#pragma unroll
    for (int k = 0; k < NLN_FOLD; k++) if ((endm >> k) & 1u) L.nsum[bnd[k]] = tq[k];
#endif
    wave_sync();
}

// The granule-channel's own spectrum decides whether the last round of pairs (lines 512..575) is dead: true exactly when all of them
// compare equal to zero.  Not derived from max_nonzero_coeff -- the reference's 575 for short blocks stays what it is (firstcut and the
// walk depend on it), and a short block's windows 1 and 2 put lines there that a long block at the same bitrate never has.
LHIP_DEV int q_tail_is_zero(int lane, const QuantLds& L) {
    int nz = 0;
    for (int k = 512 + lane; k < 576; k += LHIP_NL) if (!((double)L.xr[k] == 0)) nz = 1;
    return !wave_any(nz);
}

// calc_xmin (QuantizePVT.js:569-719), CBR flavour; want_tail0: also set g.tail0 (the kernels that skip the dead round of pairs)
LHIP_DEV void q_calc_xmin(const Tables& T, double ath_adjust, double masking_lower, const float* ratio /*E layout*/,
                          GI& g, int lane, QuantLds& L, const QuantTabs& Q, const int want_tail0 = 0) {
    lane = fresh_lane(lane);
    // band energies en0 = sum of xr^2 in line order: terms with all lanes busy, then the ordered fold
    {
        double tq[NLN_FOLD];
#pragma unroll
        for (int k = 0; k < NLN_FOLD; k++) { const double x = L.xr[NLN_FOLD * lane + k]; tq[k] = x * x; }
        int maxw = 0;
        const int nb = (g.block_type != SHORT_TYPE) ? g.psy_lmax : 3 * SBPSY_s;
        LHIP_LANE_ONCE(b, 0, nb) if (maxw < L.width[b]) maxw = L.width[b];
        maxw = wave_max(maxw);
        fold_band_sums(tq, line2sfb(Q, g.block_type), maxw, lane, L);
    }
    if (g.block_type != SHORT_TYPE) {
        LHIP_LANE_ONCE(gsfb, 0, g.psy_lmax) {
            double xmin = ath_adjust * (double)T.ATH_l[gsfb];
            const double en0 = L.nsum[gsfb];
            const double en = ratio[E_EN_L + gsfb];
            if (en > 0.0) {
                const double x = en0 * (double)ratio[E_THM_L + gsfb] * masking_lower / en;
                if (xmin < x) xmin = x;
            }
            const float xm = (float)(xmin * (double)T.longfact[gsfb]);
            L.xmin[gsfb] = xm; L.rxmin[gsfb] = recip_for_div((double)xm);
        }
        int t = -1;
        for (int k = lane; k < 576; k += LHIP_NL) if (!((double)L.xr[k] == 0)) t = k;
        t = wave_max(t);
        g.max_nonzero_coeff = (t >= 575) ? 575 : t + 1;
        if (want_tail0) g.tail0 = t < 512;
    } else {
        LHIP_LANE_ONCE(sfb, 0, SBPSY_s) {       // psymax/3 bands, 3 windows each
            const double tmpATH = ath_adjust * (double)T.ATH_s[sfb];
            float px[3];
            for (int b = 0; b < 3; b++) {
                const int gs = 3 * sfb + b;
                double xmin = tmpATH;
                const double en0 = L.nsum[gs];
                const double en = ratio[E_EN_S + sfb * 3 + b];
                if (en > 0.0) {
                    const double x = en0 * (double)ratio[E_THM_S + sfb * 3 + b] * masking_lower / en;
                    if (xmin < x) xmin = x;
                }
                px[b] = (float)(xmin * (double)T.shortfact[sfb]);
            }
            if (T.useTemporal) {
                if ((double)px[0] > (double)px[1]) px[1] = (float)((double)px[1] + ((double)px[0] - (double)px[1]) * T.decay);
                if ((double)px[1] > (double)px[2]) px[2] = (float)((double)px[2] + ((double)px[1] - (double)px[2]) * T.decay);
            }
            L.xmin[3 * sfb] = px[0]; L.xmin[3 * sfb + 1] = px[1]; L.xmin[3 * sfb + 2] = px[2];
            L.rxmin[3 * sfb] = recip_for_div((double)px[0]); L.rxmin[3 * sfb + 1] = recip_for_div((double)px[1]); L.rxmin[3 * sfb + 2] = recip_for_div((double)px[2]);
        }
        g.max_nonzero_coeff = 575;
        if (want_tail0) g.tail0 = q_tail_is_zero(lane, L);
    }
    q_set_firstcut(g, lane, L);
    wave_sync();
}

// What calc_xmin (QuantizePVT.js:569-719, q_calc_xmin) leaves behind that quantization reads: max_nonzero_coeff, and this code base's two facts derived
// with it -- the first band reaching past it (q_set_firstcut) and "the lines 512..575 are all zero" (GI::tail0).  The thresholds themselves (L.xmin,
// L.rxmin) are read by calc_noise alone: a search that never calls it (a fast table set, the validation's replay) asks for the limits alone.
LHIP_DEV void q_search_limits(GI& g, int lane, QuantLds& L, const int want_tail0) {
    lane = fresh_lane(lane);
    if (g.block_type != SHORT_TYPE) {
        int t = -1;
        for (int k = lane; k < 576; k += LHIP_NL) if (!((double)L.xr[k] == 0)) t = k;
        t = wave_max(t);
        g.max_nonzero_coeff = (t >= 575) ? 575 : t + 1;
        if (want_tail0) g.tail0 = t < 512;
    } else {
        g.max_nonzero_coeff = 575;
        if (want_tail0) g.tail0 = q_tail_is_zero(lane, L);
    }
    q_set_firstcut(g, lane, L);
    wave_sync();
}
}  // namespace lhip
