// k_quant_amp.h -- what the outer loop does between two evaluations: scale_bitcount, loop_break, the amplification of the distorted bands
// (amp_scalefac_bands, inc_scalefac_scale, inc_subblock_gain) and balance_noise that drives them.
#pragma once
#include "k_quant_count.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// scale_bitcount (Takehiro.js:980-1030), MPEG-1, no mixed blocks.  returns 1 on failure
// ---------------------------------------------------------------------------------------------
LHIP_DEV int q_scale_bitcount(const QuantTabs& Q, GI& g, int32_t* scalefac, int lane) {
    lane = fresh_lane(lane);
    const int sh = (g.block_type == SHORT_TYPE) ? 24 : 16;       // scale_short / scale_long byte of Q.sbc
    if (g.block_type != SHORT_TYPE && 0 == g.preflag) {
        int bad = 0;
        LHIP_LANE_ONCE(sfb, 11, SBPSY_l) if (scalefac[sfb] < Q.pretab[sfb]) bad = 1;
        if (!wave_any(bad)) {
            g.preflag = 1;
            wave_sync();
            LHIP_LANE_ONCE(sfb, 11, SBPSY_l) scalefac[sfb] -= Q.pretab[sfb];
            wave_sync();
        }
    }
    // slen1_n / slen2_n are powers of two, and "every value < 2^b" is "the OR of the values < 2^b": the two maxima
    // of the reference become one OR reduction of (part 1 | part 2 << 8)
    int m12 = 0;
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax) {
        const int v = scalefac[sfb];
        m12 |= (sfb < g.sfbdivide) ? v : (v << 8);
    }
    m12 = wave_or(m12);
    const int m1 = m12 & 0xff, m2 = m12 >> 8;
    // first k with the smallest tab[k] among the admissible ones == minimum of (tab[k], k) pairs; one lane per k
    int best = 0x7fffffff;
    LHIP_LANE_ONCE(k, 0, 16) {
        const uint32_t e = Q.sbc[k];
        if (m1 < (int)(e & 0xffu) && m2 < (int)((e >> 8) & 0xffu)) { const int v = (int)((e >> sh) & 0xffu) * 16 + k; if (v < best) best = v; }
    }
    best = wave_min(best);
    g.part2_length = LARGE_BITS;
    if (best != 0x7fffffff) { g.part2_length = best >> 4; g.scalefac_compress = best & 15; }
    return g.part2_length == LARGE_BITS;
}

// scale_bitcount_lsf (Takehiro.js:1046-1132), MPEG-2/2.5, no mixed blocks, no intensity stereo.  The four
// partitions of nr_of_sfb_block[table][row] are runs of the linear scalefactor index (a short band contributes its
// three windows), every max_range_sfac_tab entry is 2^n-1 and log2tab is the bit length, so the four partition maxima
// of the reference become one OR reduction with a byte per partition.  On failure nothing is written (the reference
// leaves scalefac_compress / part2_length as they were); returns 1 on failure.
LHIP_DEV int q_scale_bitcount_lsf(GI& g, const int32_t* scalefac, int lane) {
    lane = fresh_lane(lane);
    const bool pre = g.preflag != 0, sh = g.block_type == SHORT_TYPE;
    // nr_of_sfb_block[0][0..1] = {6,5,5,5} {9,9,9,9}; nr_of_sfb_block[2][0..1] = {11,10,0,0} {18,18,0,0}
    const int n0 = pre ? (sh ? 18 : 11) : (sh ? 9 : 6), n1 = pre ? (sh ? 18 : 10) : (sh ? 9 : 5);
    const int n2 = pre ? 0 : (sh ? 9 : 5), n3 = n2;
    const uint32_t range = pre ? 0x00000307u : 0x07070f0fu;      // max_range_sfac_tab[0] / [2], partition p in byte p
    const int b1 = n0, b2 = n0 + n1, b3 = b2 + n2, end = b3 + n3;
    uint32_t m = 0;
    LHIP_LANE_ONCE(i, 0, end) {
        int v = scalefac[i];
        if (v < 0) v = 0;
        const int part = (i >= b1) + (i >= b2) + (i >= b3);
        m |= (uint32_t)v << (8 * part);
    }
    m = (uint32_t)wave_or((int)m);
    int over = 0, slen[4];
    for (int p = 0; p < 4; p++) {
        const uint32_t mp = (m >> (8 * p)) & 0xffu;
        if (mp > ((range >> (8 * p)) & 0xffu)) over = 1;
        slen[p] = mp ? 32 - __builtin_clz(mp) : 0;
    }
    if (!over) {
        g.scalefac_compress = pre ? 500 + slen[0] * 3 + slen[1] : ((slen[0] * 5 + slen[1]) << 4) + (slen[2] << 2) + slen[3];
        g.part2_length = slen[0] * n0 + slen[1] * n1 + slen[2] * n2 + slen[3] * n3;
    }
    return over;
}

LHIP_DEV int q_scale_bitcount_any(const Tables& T, const QuantTabs& Q, GI& g, int32_t* scalefac, int lane) {   // Quantize.js:814-817, 840-843
    return T.mode_gr == 2 ? q_scale_bitcount(Q, g, scalefac, lane) : q_scale_bitcount_lsf(g, scalefac, lane);
}

// ---------------------------------------------------------------------------------------------
// amplification helpers (Quantize.js:453-460, 597-778)
// ---------------------------------------------------------------------------------------------
LHIP_DEV int q_loop_break(const GI& g, const int32_t* scalefac, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    int z = 0;
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax)
        if (scalefac[sfb] + band_sbgain(g, L.window, sfb) == 0) z = 1;
    return !wave_any(z);
}

// multiply xrpow of the flagged bands (bit sfb of m_amp) by `amp`, tracking xrpow_max.  Branch-free: an unflagged pair is
// multiplied by 1.0 (exact through the f32 -> f64 -> f32 round trip) and takes part in the maximum like the flagged ones --
// xrpow_max already bounds every unflagged line, so the update `if (max > xrpow_max)` sees the same verdict.
template <int NR>
LHIP_DEV void q_amplify_rounds(GI& g, double amp, uint64_t m_amp, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    float m = 0.f;
    const uint8_t* l2s = line2sfb(Q, g.block_type);
    struct F2 { float x, y; };
    F2 xx[NR]; int bnd[NR];
#pragma unroll
    for (int j = 0; j < NR; j++) {                             // pairs never straddle a band
        const int p = 2 * (lane + LHIP_NL * j);
        xx[j].x = 0.f; xx[j].y = 0.f; bnd[j] = 0;
        if (p < 576) { xx[j] = *(const F2*)(L.xrpow + p); bnd[j] = l2s[p]; }
    }
#pragma unroll
    for (int j = 0; j < NR; j++) {
        const int p = 2 * (lane + LHIP_NL * j);
        const double a = ((m_amp >> bnd[j]) & 1) ? amp : 1.0;
        xx[j].x = (float)((double)xx[j].x * a); xx[j].y = (float)((double)xx[j].y * a);
        if (p < 576) *(F2*)(L.xrpow + p) = xx[j];
        m = fmax_nonneg(m, fmax_nonneg(xx[j].x, xx[j].y));      // xrpow values are >= +0
    }
    m = wave_maxf_pos(m);
    if ((double)m > g.xrpow_max) g.xrpow_max = m;
    wave_sync();
}
// (zero lines stay zero under any amplification and add nothing to the maximum)
template <int SKIP>
LHIP_DEV void q_amplify_flagged(GI& g, double amp, uint64_t m_amp, int lane, QuantLds& L, const QuantTabs& Q) {
    if constexpr (SKIP != 0) {
        if (g.tail0) { q_amplify_rounds<NPL_HEAD>(g, amp, m_amp, lane, L, Q); return; }
    }
    q_amplify_rounds<NPL>(g, amp, m_amp, lane, L, Q);
}

// amp_scalefac_bands (Quantize.js:597-669) + loop_break (453-460) + the scalefactor statistics scale_bitcount starts with
// (Takehiro.js:980-1005), in ONE pass over the bands: the amplification decision, the incremented scalefactor, "is any band
// still at zero" and, for MPEG-1 long blocks, "could the pretab be subtracted" / the two range maxima all look at the same
// scalefac[sfb].  *all_nonzero = loop_break's verdict; *pre_bad / *m12 feed q_scale_bitcount_from (values BEFORE a preflag
// subtraction, which that function applies itself when it is due).
template <int SKIP>
LHIP_DEV void q_amp_scalefac_bands(const Tables& T, GI& g, int32_t* scalefac, int* all_nonzero, int* pre_bad, int* m12_out,
                                   int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    const double ifqstep34 = (g.scalefac_scale == 0) ? 1.29683955465100964055 : 1.68179283050742922612;
    float tr = 0.f;
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax) if (tr < L.distort[sfb]) tr = L.distort[sfb];
    double trigger = wave_maxf_pos(tr);
    // noise_shaping_amp == 1 with a distorted band: the trigger is sqrt(max distortion) (Quantize.js:612-617).  For Float32 values d and M,
    // d < RN(sqrt(M)) <=> d * d < M with the square formed exactly in f64: a Float32 can only equal the correctly rounded root if it IS
    // the root (a 53-bit neighbour of an irrational root is no 24-bit number, and d * d = M means d = sqrt(M)), so no Float32 lies between
    // the root and its rounding -- the comparison needs no square root (a dozen f64 instructions per call, on every lane)
    const int by_square = T.noise_shaping_amp == 1 && trigger > 1.0;
    const double max_dist = trigger;
    switch (T.noise_shaping_amp) {
        case 2: break;
        case 1:
            if (!(trigger > 1.0)) trigger *= .95;
            break;
        default:
            if (trigger > 1.0) trigger = 1.0;
            else trigger *= .95;
            break;
    }
    uint64_t m_amp = 0;                                  // bit sfb: band is amplified
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax) {
        const double d = (double)L.distort[sfb];
        const int below = by_square ? (d * d < max_dist) : (d < trigger);
        if (!below) m_amp |= 1ull << sfb;
    }
    m_amp = wave_lane_bits(m_amp);
    if (T.noise_shaping_amp == 2 && m_amp) m_amp = 1ull << __builtin_ctzll(m_amp);     // amplify exactly one band
    int z = 0, bad = 0, m12 = 0;
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax) {
        const int v = scalefac[sfb] + (int)((m_amp >> sfb) & 1);
        scalefac[sfb] = v;
        if (v + band_sbgain(g, L.window, sfb) == 0) z = 1;
        if (sfb >= 11 && sfb < SBPSY_l && v < Q.pretab[sfb]) bad = 1;
        m12 |= (sfb < g.sfbdivide) ? v : (v << 8);
    }
    {   // three one-bit / small-field facts in one OR reduction: bits 0-15 m12, bit 16 z, bit 17 bad
        const int r = wave_or(m12 | (z << 16) | (bad << 17));
        *m12_out = r & 0xffff; *all_nonzero = !((r >> 16) & 1); *pre_bad = (r >> 17) & 1;
    }
    q_amplify_flagged<SKIP>(g, ifqstep34, m_amp, lane, L, Q);
}

// scale_bitcount (MPEG-1) continuing from the statistics of q_amp_scalefac_bands: pre_bad = some band 11..20 is below its
// pretab entry, m12 = OR of the scalefactors of part 1 | part 2 << 8.  Same result as q_scale_bitcount on the same scalefactors.
LHIP_DEV int q_scale_bitcount_from(const QuantTabs& Q, GI& g, int32_t* scalefac, int pre_bad, int m12, int lane) {
    lane = fresh_lane(lane);
    const int sh = (g.block_type == SHORT_TYPE) ? 24 : 16;
    if (g.block_type != SHORT_TYPE && 0 == g.preflag && !pre_bad) {
        g.preflag = 1;
        wave_sync();
        LHIP_LANE_ONCE(sfb, 11, SBPSY_l) scalefac[sfb] -= Q.pretab[sfb];
        wave_sync();
        m12 = 0;                                              // the statistics change with the subtraction: take them again
        LHIP_LANE_ONCE(sfb, 0, g.sfbmax) { const int v = scalefac[sfb]; m12 |= (sfb < g.sfbdivide) ? v : (v << 8); }
        m12 = wave_or(m12);
    }
    const int m1 = m12 & 0xff, m2 = m12 >> 8;
    int best = 0x7fffffff;
    LHIP_LANE_ONCE(k, 0, 16) {
        const uint32_t e = Q.sbc[k];
        if (m1 < (int)(e & 0xffu) && m2 < (int)((e >> 8) & 0xffu)) { const int v = (int)((e >> sh) & 0xffu) * 16 + k; if (v < best) best = v; }
    }
    best = wave_min(best);
    g.part2_length = LARGE_BITS;
    if (best != 0x7fffffff) { g.part2_length = best >> 4; g.scalefac_compress = best & 15; }
    return g.part2_length == LARGE_BITS;
}

template <int SKIP>
LHIP_DEV void q_inc_scalefac_scale(const Tables& T, GI& g, int32_t* scalefac, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    uint64_t m_amp = 0;
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax) {
        int s = scalefac[sfb];
        if (g.preflag != 0) s += Q.pretab[sfb];
        if ((s & 1) != 0) { s++; m_amp |= 1ull << sfb; }
        scalefac[sfb] = s >> 1;
    }
    m_amp = wave_lane_bits(m_amp);
    wave_sync();
    g.preflag = 0;
    g.scalefac_scale = 1;
    q_amplify_flagged<SKIP>(g, 1.29683955465100964055, m_amp, lane, L, Q);
}

// inc_subblock_gain (Quantize.js:705-778); returns 1 on failure.  Short blocks only (sfb_lmax == 0).
LHIP_DEV int q_inc_subblock_gain(const Tables& T, GI& g, int32_t* scalefac, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    for (int window = 0; window < 3; window++) {
        int s1 = 0, s2 = 0;
        LHIP_LANE_ONCE3(sfb, window, g.sfbmax) {
            const int v = scalefac[sfb];
            if (sfb < g.sfbdivide) { if (s1 < v) s1 = v; } else { if (s2 < v) s2 = v; }
        }
        s1 = wave_max(s1); s2 = wave_max(s2);
        if (s1 < 16 && s2 < 8) continue;
        if (sbgain(g, window) >= 7) return 1;
        if (window == 0) g.subblock_gain[0]++; else if (window == 1) g.subblock_gain[1]++; else g.subblock_gain[2]++;
        // per band of this window: either lower the scalefactor or scale xrpow by IPOW20(210 + (s << ..))
        // (bands are handled one amplitude at a time; at most 13 bands + the sfb12 tail per window)
        wave_sync();
        for (int sfb = window; sfb < g.sfbmax + 3; sfb += 3) {   // last iteration: sfb == sfbmax + window, the sfb12 tail
            double amp;
            int doamp = 0;
            int s = (sfb < g.sfbmax) ? scalefac[sfb] : 0;
            wave_sync();                              // every lane has read the scalefactor before lane 0 rewrites it
            if (sfb < g.sfbmax) {
                s = s - (4 >> g.scalefac_scale);
                if (s >= 0) { if (lane == 0) scalefac[sfb] = s; }
                else {
                    if (lane == 0) scalefac[sfb] = 0;
                    amp = ipow20(Q, 210 + s * (1 << (g.scalefac_scale + 1)));      // s < 0 here: a multiplication, not a shift of a negative value
                    doamp = 1;
                }
            } else { amp = ipow20(Q, 202); doamp = 1; }
            wave_sync();
            if (uni(doamp)) {
                float m = 0.f;
                const int st = L.start[sfb], w = L.width[sfb];
                for (int i = st + lane; i < st + w; i += LHIP_NL) {
                    const float v = (float)((double)L.xrpow[i] * amp);
                    L.xrpow[i] = v;
                    m = fmax_nonneg(m, v);
                }
                m = wave_maxf_pos(m);
                if ((double)m > g.xrpow_max) g.xrpow_max = m;
            }
        }
        wave_sync();
    }
    return 0;
}

// balance_noise (Quantize.js:793-846); returns 1 to continue the outer loop
template <int SKIP>
LHIP_DEV int q_balance_noise(const Tables& T, GI& g, int32_t* scalefac, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    int all_nonzero, pre_bad, m12;
    q_amp_scalefac_bands<SKIP>(T, g, scalefac, &all_nonzero, &pre_bad, &m12, lane, L, Q);
    int status = all_nonzero;                                  // loop_break (Quantize.js:453-460)
    if (status) return 0;
    status = T.mode_gr == 2 ? q_scale_bitcount_from(Q, g, scalefac, pre_bad, m12, lane) : q_scale_bitcount_lsf(g, scalefac, lane);
    if (!status) return 1;
    if (T.noise_shaping > 1) {
        if (0 == g.scalefac_scale) {
            q_inc_scalefac_scale<SKIP>(T, g, scalefac, lane, L, Q);
            status = 0;
        } else if (g.block_type == SHORT_TYPE && T.subblock_gain > 0) {
            status = (q_inc_subblock_gain(T, g, scalefac, lane, L, Q) || q_loop_break(g, scalefac, lane, L, Q));
        }
    }
    if (!status) status = q_scale_bitcount_any(T, Q, g, scalefac, lane);
    return !status;
}
}  // namespace lhip
