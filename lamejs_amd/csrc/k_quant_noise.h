// k_quant_noise.h -- calc_noise: the per-line error terms and their systolic fold into band sums (q_noise_band_sums), the per-band part
// with the noise cache, and the deferred cache write of a speculative call (NoiseCommit / q_noise_commit).
#pragma once
#include "k_quant_count.h"
namespace lhip {
#if LHIP_NL != 1
// calc_noise's line pass and systolic fold (step 2 of q_calc_noise_, which says how the fold reproduces the reference's sums): the squared
// errors of the lines 0 .. 64 NLN - 1, NLN consecutive lines per lane, summed per band into L.nsum.  NLN = 9 covers the spectrum.  NLN = 3 is the short
// window (lines 0..191) of a call whose fresh bands all end at or below line 192 -- the other bands' values come from the cache; its marks sit 12 bits up
// in the same words of fold_marks.  NLN = 7
// stops at line 448: q_calc_noise_ reads L.nsum[sfb] for sfb < psymax alone -- 21 long bands or 36 short ones, sfb21_extra being refused -- and
// Tables::noise_nln is 7 only where every such band ends at or below line 448.  A band cut off by line 448 gets no end mark in
// QuantTabs::fold_marks (built for the same NLN), so its partial sum is never stored.  (L.nsum's other readers, q_calc_xmin and the
// perceptual entropies, fill it themselves: fold_band_sums, q_frame_pe.)
template <int NLN>
LHIP_DEV void q_noise_band_sums(const Tables& T, const GI& g, const int16_t* ix, int may_big, int maxlen, int lane, QuantLds& L, const QuantTabs& Q,
                                unsigned long long& tm_) {
    static_assert(LHIP_NL == 64 && (NLN == 3 || NLN == 7 || NLN == 9), "QuantTabs::fold_marks is laid out for 3 and for 7 or 9 lines on each of 64 lanes");
    enum { MS = NLN == 3 ? 12 : 0 };                 // the short window's marks sit 12 bits up in the same words
    if (NLN == 3) LHIP_NOISE_LINES_COUNT(n3); else if (NLN == 7) LHIP_NOISE_LINES_COUNT(n7); else LHIP_NOISE_LINES_COUNT(n9);
    double tq[NLN], keep[NLN];
    int lastb[NLN];
    const uint32_t marks = Q.fold_marks[g.block_type == SHORT_TYPE][lane];
    const uint8_t* l2s = line2sfb(Q, g.block_type);
    // Terms are computed for every line below 64 NLN, evaluated band or not: a cached band's sum is never read.
    // keep[k] = 0 at a band start, 1 elsewhere: fma(sum, keep, t) is `sum + t` or `t` with ONE rounding, i.e.
    // exactly the reference's `noise += t` (or a fresh sum); no contraction is involved, the fma is explicit.
    // |xr| - pow43 * step: the product of two Float32 values is exact in f64, so the explicit fma's single rounding is the
    // reference's (a product, then a difference).
    // !may_big (the usual case): every quantized value is below QT_N (q_calc_noise_), nothing to clamp; else the clamped look-up is
    // replaced in the pass that follows
#define NOISE_TERMS(IDX) _Pragma("unroll") for (int k = 0; k < NLN; k++) { \
        const int j = NLN * lane + k; \
        const int bnd = l2s[j]; \
        const float bstep = L.bstep[bnd]; \
        const float xa = L.xr[j]; const int iv = ix[j]; \
        const float pw = Q.pow43[IDX]; \
        const double x = __builtin_fma(-(double)pw, (double)bstep, d_abs((double)xa)); \
        tq[k] = x * x; \
        keep[k] = one_unless_bit(marks, MS + k); \
        lastb[k] = bnd; \
    }
    if (!may_big) { NOISE_TERMS(iv) } else { NOISE_TERMS(iv < QT_N ? iv : QT_N - 1) }
#undef NOISE_TERMS
    if (may_big) {                                   // rare: quantized values beyond the part of pow43 staged in LDS
#pragma unroll
        for (int k = 0; k < NLN; k++) {
            const int j = NLN * lane + k;
            const int iv = ix[j];
            if (iv >= QT_N) {
                const double x = __builtin_fma(-(double)T.pow43[iv], (double)L.bstep[lastb[k]], d_abs((double)L.xr[j]));
                tq[k] = x * x;
            }
        }
    }
    PH_MARK(L, PH_N_LINES, tm_);
    const int nsteps = (maxlen + NLN - 1) / NLN + 1;
    double carry = 0.0;
    for (int st = 0; st + 1 < nsteps; st++) {
        double sacc = carry;
#pragma unroll
        for (int k = 0; k < NLN; k++) sacc = __builtin_fma(sacc, keep[k], tq[k]);
        carry = wave_shr1d(sacc, 0.0);
    }
    {
        double sacc = carry;
#pragma unroll
        for (int k = 0; k < NLN; k++) { sacc = __builtin_fma(sacc, keep[k], tq[k]); tq[k] = sacc; }   // tq := running sums of the last step
    }
#pragma unroll
    for (int k = 0; k < NLN; k++) if ((marks >> (16 + MS + k)) & 1u) L.nsum[lastb[k]] = tq[k];
    wave_sync();
    PH_MARK(L, PH_N_FOLD, tm_);
}
#endif

// ---------------------------------------------------------------------------------------------
// calc_noise (QuantizePVT.js:784-878); distort -> L.distort, cache -> L.pn_*
// The bands' sums in the reference's line order (f64 sums are order-sensitive) as a systolic fold; all gathers hit LDS.
// ---------------------------------------------------------------------------------------------
// need_max: the caller will look at max_noise even if some band is over its threshold (quant_compare only reads max_noise of
// results with over_count == 0, and of `best` only while best.over_count == 0), so the f64 wave maximum is skipped otherwise
// What a calc_noise call would write into the noise cache (PrevNoise / L.pn_*), held by lane = band: a call made SPECULATIVELY (count_bits
// of the same quantization still running on another wave, q_count_bits_piped) must not touch the cache before its evaluation is known to
// be the one the reference makes -- q_noise_commit writes it then; a discarded call leaves no trace the reference could see.
struct NoiseCommit { int fresh, step, cls; float dist; double x; };
LHIP_DEV void q_noise_commit(const GI& g, const NoiseCommit& nc, PrevNoise& pn, int lane, QuantLds& L) {
    lane = fresh_lane(lane);
    LHIP_LANE_ONCE(sfb, 0, g.psymax) {
        if (nc.fresh) { L.pn_step[sfb] = nc.step; L.pn_dist[sfb] = nc.dist; L.pn_x[sfb] = nc.x; L.pn_cls[sfb] = (int16_t)nc.cls; }
    }
    pn.gain = g.global_gain;
    wave_sync();
}
LHIP_DEV void q_calc_noise_(const Tables& T, const GI& g, const int32_t* scalefac, const int16_t* ix, NoiseRes* res,
                           int use_pn, PrevNoise& pn, int need_max, int lane, QuantLds& L, const QuantTabs& Q, NoiseCommit* defer = nullptr) {
    lane = fresh_lane(lane);
    unsigned long long tm_ = PH_NOW(); (void)tm_;
    // 1) per band: its step and whether the cache answers for it.  The reference walks a start line from band to band and sums the
    //    first band that reaches past max_nonzero_coeff over its useful part only, every later band over nothing
    //    (QuantizePVT.js:806-830).  Summing every evaluated band over its WHOLE width gives the same sums: from
    //    max_nonzero_coeff on xr is zero (it is the first of the spectrum's trailing zeros) and so is the quantized value
    //    ((int)(0 * istep + adj43[0]) = 0, cached values by induction), hence every skipped line would add (|0| - pow43[0] * step)^2 = +0
    //    to a non-negative sum -- so there is no range bookkeeping here at all.
    // One error formula serves the three branches of calc_noise_core (QuantizePVT.js:725-767): a band that starts above count1 holds
    // only zeros and one that starts above big_values only 0/1, and pow43[0] = 0, pow43[1] = 1, so |xr| - pow43[ix] * step is bit for
    // bit `xr` (squared), `|xr| - ix01[ix]` and `|xr| - pow43[ix] * step` there.
    const int is_short = g.block_type == SHORT_TYPE;
    // quantized values are <= xrpow_max * ipow20(gain) + 1 (the working copy was quantized at this gain): below QT_N - 1
    // no line can need the part of pow43 that is not staged in LDS
    const int may_big = !(g.xrpow_max * ipow20(Q, g.global_gain) < (double)(QT_N - 1));
#if LHIP_NL == 1
    // one-lane build: the same band by band (a band next to a step of the class function takes the logarithm by itself; where the
    // shortcut is taken it equals the logarithm's verdict, so the wave-wide fallback of the 64-lane program gives the same numbers)
    const uint8_t* l2s = line2sfb(Q, g.block_type);
    int over = 0, ssd = 0;
    uint64_t m_fresh = 0;
    (void)may_big; (void)is_short;
    for (int sfb = 0; sfb < g.psymax; sfb++) {
        const int s = sf_step(Q, g, scalefac, L.window, sfb);
        if (!(use_pn && L.pn_step[sfb] == s)) m_fresh |= 1ull << sfb;
        L.qmode[sfb] = s;
        L.bstep[sfb] = Q.pow20[s + Q_MAX2];
    }
    PH_MARK(L, PH_N_WALK, tm_);
    {
        double sacc = 0.0;
        for (int j = 0; j < 576; j++) {
            const int bnd = l2s[j];
            if (j == 0 || l2s[j - 1] != bnd) sacc = 0.0;
            const double x = __builtin_fma(-pow43v(T, Q, ix[j]), (double)L.bstep[bnd < SFBMAX + 1 ? bnd : SFBMAX], d_abs((double)L.xr[j]));
            sacc += x * x;
            if (j == 575 || l2s[j + 1] != bnd) L.nsum[bnd] = sacc;
        }
    }
    PH_MARK(L, PH_N_FOLD, tm_);
    for (int sfb = 0; sfb < g.psymax; sfb++) {
        int cls;
        if (!((m_fresh >> sfb) & 1)) { L.distort[sfb] = L.pn_dist[sfb]; cls = L.pn_cls[sfb]; }
        else {
            const double noise = L.nsum[sfb], b = (double)L.xmin[sfb], rb = L.rxmin[sfb];
            const double x = rb != 0.0 ? div_by_f32(noise, b, rb) : noise / b;
            L.distort[sfb] = (float)x;
            if (use_pn) { L.pn_step[sfb] = L.qmode[sfb]; const double nf = (double)(float)noise; L.pn_dist[sfb] = (float)(rb != 0.0 ? div_by_f32(nf, b, rb) : nf / b); }
            cls = need_max ? -1 : noise_class(x);          // the logarithm will be formed anyway: no shortcut
            int cls_cache = cls;
            if (cls < 0) {
                const double l = v8_log10_pos(x > 1E-20 ? x : 1E-20);
                cls = noise_class_of_log(l); cls_cache = noise_class_of_log((double)(float)l);
            }
            if (use_pn) { L.pn_x[sfb] = x; L.pn_cls[sfb] = (int16_t)cls_cache; }
            else L.nsum[sfb] = x;                          // (no cache in this call: the value for the max_noise pass below)
        }
        if (cls > 0) { ssd += cls * cls; over++; }
    }
    PH_MARK(L, PH_N_TERMS, tm_);
    if (use_pn) pn.gain = g.global_gain;
    res->over_count = over; res->over_SSD = ssd;
    res->max_noise = 0.0;
    if (need_max || over == 0) {
        double max_noise = -20.0;
        for (int sfb = 0; sfb < g.psymax; sfb++) {
            const bool fresh = (m_fresh >> sfb) & 1;
            const double x = (fresh && !use_pn) ? L.nsum[sfb] : L.pn_x[sfb];
            const double l = v8_log10_pos(x > 1E-20 ? x : 1E-20);
            const double nl = fresh ? l : (double)(float)l;
            if (nl > max_noise) max_noise = nl;
        }
        res->max_noise = max_noise;
    }
#else
    int my_step = 0, my_fresh = 0;                        // lane = band: kept in registers for the per-band part after the fold
    LHIP_LANE_ONCE(sfb, 0, g.psymax) {
        my_step = sf_step(Q, g, scalefac, L.window, sfb);
        my_fresh = !(use_pn && L.pn_step[sfb] == my_step);
        L.bstep[sfb] = Q.pow20[my_step + Q_MAX2];
    }
    // the longest chain the fold must carry: the widest evaluated band (an upper bound -- the widest band up to the highest evaluated one)
    const uint64_t m_fresh = wave_ballot(my_fresh);
    const int hib = m_fresh ? 63 - (int)__builtin_clzll(m_fresh) : 0;
    const int maxlen = m_fresh ? (int)(is_short ? Q.wpre_short[hib] : Q.wpre_long[hib]) : 0;
    wave_sync();
    PH_MARK(L, PH_N_WALK, tm_);
    // 2) squared errors summed per band in the reference's line order (f64 sums are order-sensitive) as a
    //    systolic fold: lane l owns NLN consecutive lines and folds their terms, in order, onto the running sum
    //    handed over by lane l-1 (reset at band starts).  One hand-over step extends every band's chain by one
    //    lane, so ceil(longest band / NLN) + 1 steps reproduce the strictly sequential sums exactly, while the
    //    terms themselves are computed once, all lanes busy.
    //    NLN is the table set's, or 3 for the short window: wave-uniform branches per call pick the body.  The table set's value is read from the kernel's arguments (Tables::noise_nln, a
    //    scalar load that does not depend on the band pass above), not from its copy in QuantTabs: a branch on a value in LDS adds a third
    //    dependent LDS round trip to the line pass, which cost most of what the two lines save (profiles/noise_lines_ab_parent_vs_result.txt).
    if (m_fresh && hib <= T.noise_hib3[is_short]) q_noise_band_sums<3>(T, g, ix, may_big, maxlen, lane, L, Q, tm_);   // every fresh band ends at or below line 192
    else if (T.noise_nln == 7) q_noise_band_sums<7>(T, g, ix, may_big, maxlen, lane, L, Q, tm_);
    else q_noise_band_sums<9>(T, g, ix, may_big, maxlen, lane, L, Q, tm_);
    // 3) per band: distortion ratio x = noise / xmin (div_by_f32: the division's result from the reciprocal calc_xmin left), its class
    //    (over? tmp) -- without the logarithm wherever that is safe (noise_class, lhip_math.h) -- and the cache.  The reference caches
    //    the Float32 copy of the noise and divides it by xmin again in every later call; that quotient is formed here, once.  Lanes whose
    //    band sits next to a step of the class function (or outside the shortcut's range) make the whole wave take the logarithm for
    //    this call (about one call in a hundred); the logarithm is also taken when the caller will read max_noise (need_max) or the
    //    result turns out to have no distorted band.
    double x = 1.0;                                   // this lane's band: noise / xmin (cached bands: as last evaluated)
    int cls = 0;                                      // class used by THIS call
    const int fresh = my_fresh;
    LHIP_LANE_ONCE(sfb, 0, g.psymax) {
        if (!fresh) {
            L.distort[sfb] = L.pn_dist[sfb];
            x = L.pn_x[sfb];
            cls = L.pn_cls[sfb];
        } else {
            const double noise = L.nsum[sfb], b = (double)L.xmin[sfb], rb = L.rxmin[sfb];
            const double nf = (double)(float)noise;
            x = div_by_f32(noise, b, rb);
            double xf = div_by_f32(nf, b, rb);
            if (rb == 0.0) { x = noise / b; xf = nf / b; }         // never on sane material: an xmin outside div_by_f32's proof
            L.distort[sfb] = (float)x;
            if (defer) { defer->step = my_step; defer->dist = (float)xf; }
            else if (use_pn) { L.pn_step[sfb] = my_step; L.pn_dist[sfb] = (float)xf; }
            cls = need_max ? -1 : noise_class(x);          // the logarithm will be formed anyway: no shortcut
        }
    }
    PH_MARK(L, PH_N_TERMS, tm_);
    int cls_cache = cls;                              // class the reference will derive from its Float32 copy in later calls
    int have_log = 0;
    double nl = -20.0;                                // noise_log as this call sees it (only valid when have_log)
    if (wave_any(cls < 0)) {
        LHIP_LANE_ONCE(sfb, 0, g.psymax) {
            const double l = v8_log10_pos(x > 1E-20 ? x : 1E-20);       // operand >= 1e-20 (a NaN compares false and becomes 1e-20 too)
            const double lf = (double)(float)l;
            nl = fresh ? l : lf;
            if (fresh) { cls = noise_class_of_log(l); cls_cache = noise_class_of_log(lf); }
        }
        have_log = 1;
    }
    int over = 0, ssd = 0;
    if (defer) { defer->fresh = 0; LHIP_LANE_ONCE(sfb, 0, g.psymax) { defer->fresh = use_pn && fresh; defer->x = x; defer->cls = cls_cache; } }
    LHIP_LANE_ONCE(sfb, 0, g.psymax) {
        if (!defer && use_pn && fresh) { L.pn_x[sfb] = x; L.pn_cls[sfb] = (int16_t)cls_cache; }
        if (cls > 0) { ssd = cls * cls; over = 1; }
    }
    if (use_pn && !defer) pn.gain = g.global_gain;
    {   // over <= 39 bands and over_SSD <= 39 * 400^2 < 2^25: one packed integer reduction
        const int os = wave_sum((ssd << 6) | over);
        res->over_count = os & 63; res->over_SSD = os >> 6;
    }
    res->max_noise = 0.0;
    if (need_max || res->over_count == 0) {
        double max_noise = -20.0;
        if (!have_log) {
            LHIP_LANE_ONCE(sfb, 0, g.psymax) {
                const double l = v8_log10_pos(x > 1E-20 ? x : 1E-20);
                nl = fresh ? l : (double)(float)l;
            }
        }
        LHIP_LANE_ONCE(sfb, 0, g.psymax) max_noise = nl;
        res->max_noise = wave_maxd(max_noise);
    }
#endif
    wave_sync();
    PH_MARK(L, PH_N_SUMS, tm_);
}

LHIP_DEV void q_calc_noise(const Tables& T, const GI& g, const int32_t* scalefac, const int16_t* ix, NoiseRes* res,
                           int use_pn, PrevNoise& pn, int need_max, int lane, QuantLds& L, const QuantTabs& Q) {
    PH_BEGIN();
    q_calc_noise_(T, g, scalefac, ix, res, use_pn, pn, need_max, lane, L, Q);
    PH_END(L, PH_NOISE);
}
}  // namespace lhip
