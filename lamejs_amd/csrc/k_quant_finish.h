// k_quant_finish.h -- how a granule-channel ends after the search (iteration_finish_one): best_scalefac_store with scfsi_calc (Takehiro.js:809-943)
// and best_huffman_divide with recalc_divide_sub (Takehiro.js:698-800), the region splits priced from per-band Huffman statistics.
#pragma once
#include "k_quant_count.h"
#include "k_quant_amp.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// iteration_finish_one: best_scalefac_store (Takehiro.js:862-943), scfsi_calc (809-855),
// best_huffman_divide (727-800)
// ---------------------------------------------------------------------------------------------
LHIP_DEV void q_best_scalefac_store(const Tables& T, GI& g, int gr, int ch, int gr0_block_type, int* scfsi /*[4]*/,
                                    int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    int32_t* sf = L.sfb;
    int recalc = 0;
    {
        // bands whose quantized lines are all zero get scalefactor -2 (Takehiro.js:870-882): every lane flags the
        // bands of its non-zero pairs (a pair never straddles a band), then one lane per band reads its flag
        LHIP_LANE_ONCE(sfb, 0, (SFBMAX) + 1) L.qmode[sfb] = 0;
        wave_sync();
        const uint8_t* l2s = line2sfb(Q, g.block_type);
        for (int p = 2 * lane; p < 576; p += 2 * LHIP_NL)
            if (*(const uint32_t*)(L.ixw + p) != 0) L.qmode[l2s[p]] = 1;
        wave_sync();
        int any = 0;
        LHIP_LANE_ONCE(sfb, 0, g.sfbmax) if (!L.qmode[sfb]) { sf[sfb] = -2; any = 1; }
        if (wave_any(any)) recalc = -2;
        wave_sync();
    }
    if (0 == g.scalefac_scale && 0 == g.preflag) {
        int s = 0;
        LHIP_LANE_ONCE(sfb, 0, g.sfbmax) if (sf[sfb] > 0) s |= sf[sfb];
        s = wave_or(s);
        if (0 == (s & 1) && s != 0) {
            LHIP_LANE_ONCE(sfb, 0, g.sfbmax) if (sf[sfb] > 0) sf[sfb] >>= 1;
            g.scalefac_scale = recalc = 1;
            wave_sync();
        }
    }
    if (0 == g.preflag && g.block_type != SHORT_TYPE && T.mode_gr == 2) {
        int bad = 0;
        LHIP_LANE_ONCE(sfb, 11, SBPSY_l) if (sf[sfb] < T.pretab[sfb] && sf[sfb] != -2) bad = 1;
        if (!wave_any(bad)) {
            LHIP_LANE_ONCE(sfb, 11, SBPSY_l) if (sf[sfb] > 0) sf[sfb] -= T.pretab[sfb];
            g.preflag = recalc = 1;
            wave_sync();
        }
    }
    for (int i = 0; i < 4; i++) scfsi[i] = 0;
    if (T.mode_gr == 2 && gr == 1 && uni(gr0_block_type) != SHORT_TYPE && g.block_type != SHORT_TYPE) {
        // scfsi_calc (Takehiro.js:809-855), one lane per scalefactor band: a group is shared with granule 0 when no
        // band of it differs (bands already marked negative do not count as different)
        const int8_t* g0 = L.sf_gr0[ch];
        uint64_t m_diff = 0;
        LHIP_LANE_ONCE(sfb, 0, SBPSY_l) if ((int)g0[sfb] != sf[sfb] && sf[sfb] >= 0) m_diff |= 1ull << sfb;
        m_diff = wave_lane_bits(m_diff);
        uint64_t m_same = 0;
        for (int i = 0; i < 4; i++) {
            const int b0 = T.scfsi_band[i], b1 = T.scfsi_band[i + 1];
            const uint64_t rng = ((1ull << b1) - 1) & ~((1ull << b0) - 1);
            if ((m_diff & rng) == 0) { scfsi[i] = 1; m_same |= rng; }
        }
        wave_sync();
        LHIP_LANE_ONCE(sfb, 0, SBPSY_l) if ((m_same >> sfb) & 1) sf[sfb] = -1;
        wave_sync();
        // slen1_n / slen2_n are powers of two: the two maxima of the reference reduce to ORs (negative markers count as 0)
        uint64_t m_cnt = 0;
        int or12 = 0;
        LHIP_LANE_ONCE(sfb, 0, SBPSY_l) {
            const int v = sf[sfb];
            if (v != -1) m_cnt |= 1ull << sfb;
            const int vp = v > 0 ? v : 0;
            or12 |= (sfb < 11) ? vp : (vp << 8);
        }
        m_cnt = wave_lane_bits(m_cnt);
        or12 = wave_or(or12);
        const int c1 = __builtin_popcountll(m_cnt & 0x7ffull), c2 = __builtin_popcountll(m_cnt >> 11);
        const int s1 = or12 & 0xff, s2 = or12 >> 8;
        int best = 0x7fffffff;                         // first i with the smallest cost == minimum of (cost, i)
        LHIP_LANE_ONCE(i, 0, 16)
            if (s1 < T.slen1_n[i] && s2 < T.slen2_n[i]) { const int c = (T.slen1_tab[i] * c1 + T.slen2_tab[i] * c2) * 16 + i; if (c < best) best = c; }
        best = wave_min(best);
        if (best != 0x7fffffff && g.part2_length > (best >> 4)) { g.part2_length = best >> 4; g.scalefac_compress = best & 15; }
        recalc = 0;
    }
    wave_sync();
    LHIP_LANE_ONCE(sfb, 0, g.sfbmax) if (sf[sfb] == -2) sf[sfb] = 0;
    wave_sync();
    if (uni(recalc) != 0) q_scale_bitcount_any(T, Q, g, sf, lane);
}

// Range maxima over whole bands in O(1): hmax[t][b] = maximum of the band maxima (row 0 of the statistics) of the bands
// b .. b + 2^t - 1, bands past SBMAX_l counting as 0; any range is covered by two (overlapping) power-of-two windows.
LHIP_DEV void q_band_max_tables(int lane, QuantLds& L) {
    LHIP_LANE_ONCE(b, 0, 24) L.hmax[0][b] = (int16_t)(b < SBMAX_l ? L.hd.bstat[0][b + 1] : 0);     // quantized values are <= IXMAX_VAL
    wave_sync();
#pragma unroll
    for (int t = 1; t < 5; t++) {
        LHIP_LANE_ONCE(b, 0, 24) {
            const int h = 1 << (t - 1);
            const int a = L.hmax[t - 1][b], c = (b + h < 24) ? (int)L.hmax[t - 1][b + h] : 0;
            L.hmax[t][b] = (int16_t)(a > c ? a : c);
        }
        wave_sync();
    }
}
LHIP_DEV int q_band_range_max(const QuantLds& L, int lo, int hi) {      // bands [lo, hi); 0 for an empty range
    const int len = hi - lo;
    const int t = 31 - (int)__builtin_clz((unsigned)(len > 0 ? len : 1));
    const int a = L.hmax[t][lo < 23 ? lo : 23], c = L.hmax[t][hi - (1 << t) >= 0 ? hi - (1 << t) : 0];
    const int m = a > c ? a : c;
    return len > 0 ? m : 0;
}

// Huffman statistics per scalefactor band over the pairs below `limit`, then turned into prefix sums over
// bands so that any union of whole bands [b0, b1) costs O(1):
// row 0 max (kept per band), 1 t1, 2 table23 (packed), 3 table56 (packed), 4..6 t7-9, 7..9 t10-12, 10..12 t13-15,
// 13 largetbl hi, 14 largetbl lo, 15 number of escaped values.  A row is only meaningful for regions whose
// maximum admits the table group, which is exactly when the reference would look at it.
LHIP_DEV void q_band_stats(const Tables& T, const int16_t* ix, int limit, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    // One lane per run of consecutive pairs (5 on the device): every pair contributes its 17 code lengths, the
    // lane keeps running sums, an exclusive wave scan of the lane totals turns them into prefix sums over ALL
    // pairs, and the lanes owning the last pair of a band publish the prefix there.  Sums are packed two per
    // word (a total is at most 288 x 21 < 2^16).  A length is only added when the PAIR admits the table; a row
    // is only read for regions whose maximum admits it, where that is the same thing.
    enum { PPL = (288 + LHIP_NL - 1) / LHIP_NL, NW = 9 };
    LHIP_LANE_ONCE(bnd, 0, (SBMAX_l + 1) + 1) L.hd.bstat[0][bnd] = 0;
    wave_sync();
    uint32_t pre[PPL][NW];
    uint32_t run[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) run[w] = 0;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int q = PPL * lane + j, p = 2 * q;
        if (q < 288 && p < limit) {
            const uint32_t w2 = *(const uint32_t*)(ix + p);
            const int x = (int)(w2 & 0xffffu), y = (int)(w2 >> 16), m = x > y ? x : y;
            if (m > 0) lds_max(&L.hd.bstat[0][Q.l2s_long[p] + 1], m);
            const int xc = x < 15 ? x : 15, yc = y < 15 ? y : 15, e = xc * 16 + yc;
            uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
            if (m <= 1) c0 = Q.hlen[HL_T1 + x * 2 + y];
            if (m <= 2) { const int k = x * 3 + y; c0 |= (uint32_t)Q.hlen[HL_T2 + k] << 16; c1 = Q.hlen[HL_T3 + k]; }
            if (m <= 3) { const int k = x * 4 + y; c1 |= (uint32_t)Q.hlen[HL_T5 + k] << 16; c2 = Q.hlen[HL_T6 + k]; }
            if (m <= 5) { const int k = x * 6 + y; c2 |= (uint32_t)Q.hlen[HL_T7 + k] << 16; c3 = Q.hlen[HL_T8 + k] | ((uint32_t)Q.hlen[HL_T9 + k] << 16); }
            if (m <= 7) { const int k = x * 8 + y; c4 = Q.hlen[HL_T10 + k] | ((uint32_t)Q.hlen[HL_T11 + k] << 16); c5 = Q.hlen[HL_T12 + k]; }
            if (m <= 15) { c5 |= (uint32_t)Q.hlen[HL_T13 + e] << 16; c6 = Q.hlen[HL_T14 + e] | ((uint32_t)Q.hlen[HL_T15 + e] << 16); }
            const uint32_t c7 = Q.hlen[HL_EHI + e] | ((uint32_t)Q.hlen[HL_ELO + e] << 16);
            const uint32_t c8 = (uint32_t)((x > 14) + (y > 14));
            run[0] += c0; run[1] += c1; run[2] += c2; run[3] += c3; run[4] += c4; run[5] += c5; run[6] += c6; run[7] += c7; run[8] += c8;
        }
#pragma unroll
        for (int w = 0; w < NW; w++) pre[j][w] = run[w];
    }
    uint32_t base[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) { int tot; base[w] = (uint32_t)wave_excl_scan((int)run[w], lane, &tot); }
    // word layout: 0: t1 | t2<<16   1: t3 | t5<<16   2: t6 | t7<<16   3: t8 | t9<<16   4: t10 | t11<<16
    //              5: t12 | t13<<16  6: t14 | t15<<16  7: esc_hi | esc_lo<<16   8: escaped values
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int q = PPL * lane + j, p = 2 * q;
        if (q < 288 && (p + 2 == 576 || Q.l2s_long[p] != Q.l2s_long[p + 2])) {
            const int col = Q.l2s_long[p] + 1;
            uint32_t v[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) v[w] = base[w] + pre[j][w];
            L.hd.bstat[1][col] = (int)(v[0] & 0xffffu);
            L.hd.bstat[2][col] = (int)((v[0] & 0xffff0000u) | (v[1] & 0xffffu));          // t2 << 16 | t3 (count_bit_noESC_from2 packing)
            L.hd.bstat[3][col] = (int)((v[1] & 0xffff0000u) | (v[2] & 0xffffu));          // t5 << 16 | t6
            L.hd.bstat[4][col] = (int)(v[2] >> 16); L.hd.bstat[5][col] = (int)(v[3] & 0xffffu); L.hd.bstat[6][col] = (int)(v[3] >> 16);
            L.hd.bstat[7][col] = (int)(v[4] & 0xffffu); L.hd.bstat[8][col] = (int)(v[4] >> 16); L.hd.bstat[9][col] = (int)(v[5] & 0xffffu);
            L.hd.bstat[10][col] = (int)(v[5] >> 16); L.hd.bstat[11][col] = (int)(v[6] & 0xffffu); L.hd.bstat[12][col] = (int)(v[6] >> 16);
            L.hd.bstat[13][col] = (int)(v[7] & 0xffffu); L.hd.bstat[14][col] = (int)(v[7] >> 16); L.hd.bstat[15][col] = (int)v[8];
        }
    }
    LHIP_LANE_ONCE(k, 1, 16) L.hd.bstat[k][0] = 0;
    wave_sync();
    q_band_max_tables(lane, L);
}

// choose_table for the union of whole bands [b0, b1) from the statistics above (bits are added to *bits).
// Called with lane-varying ranges, so it is written branch-free (selects), like the region planning of count_bits.
LHIP_DEV int q_choose_from_stats(const Tables& T, int b0, int b1, int* bits, const QuantLds& L, const QuantTabs& Q) {
    (void)T; (void)Q;
    const int mx = q_band_range_max(L, b0, b1);
    const int kind = (mx == 0) ? 0 : (mx == 1) ? 1 : (mx <= 3) ? 2 : (mx <= 15) ? 4 : (mx <= IXMAX_VAL) ? 5 : 6;
    const int t1 = (mx <= 1) ? mx : (mx == 2) ? 2 : (mx == 3) ? 5 : (mx <= 5) ? 7 : (mx <= 7) ? 10 : 13;
    const int rowA = (kind == 1) ? 1 : (kind == 2) ? (mx == 2 ? 2 : 3) : (kind == 4) ? (mx <= 5 ? 4 : mx <= 7 ? 7 : 10) : 13;
    int choice, choice2, lb1, lb2;
    esc_choice(mx > 15 ? mx - 15 : 1, &choice, &choice2, &lb1, &lb2);
    const int sA = L.hd.bstat[rowA][b1] - L.hd.bstat[rowA][b0];
    const int sB = L.hd.bstat[rowA + 1][b1] - L.hd.bstat[rowA + 1][b0];
    const int sC = L.hd.bstat[rowA + 2][b1] - L.hd.bstat[rowA + 2][b0];
    int c0 = sA, c1 = sB, c2 = sC, ta = t1, tb = t1 + 1;
    if (kind == 2) { c0 = (int)((unsigned)sA >> 16); c1 = sA & 0xffff; }
    if (kind == 5) { c0 = sA + sC * lb1; c1 = sB + sC * lb2; ta = choice; tb = choice2; }
    int bsum = c0, t = ta;
    if ((kind == 2 || kind == 4 || kind == 5) && bsum > c1) { bsum = c1; t = tb; }
    if (kind == 4 && bsum > c2) { bsum = c2; t = t1 + 2; }
    if (kind == 0) { bsum = 0; t = 0; }
    if (kind == 6) { *bits = LARGE_BITS; return -1; }
    *bits += bsum;
    return t;
}

// recalc_divide_sub (Takehiro.js:698-725); region 2 = bands r2.. up to big_values, from the band statistics.
// The cost of region 2 for every split point r2 is independent of the loop state, so lane r2 evaluates it; the
// reference's running comparison (its `break`s depend on the best length so far) is then replayed over those.
LHIP_DEV void q_recalc_divide_sub(const Tables& T, const GI& c2, GI& g, int lane, QuantLds& L, const QuantTabs& Q) {
    const int bigv = c2.big_values;
    LHIP_LANE_ONCE(r2, 2, SBMAX_l + 1) {
        int bits2 = 0;
        const int tbl = q_choose_from_stats(T, r2, SBMAX_l, &bits2, L, Q);
        L.r2_bits[r2] = bits2; L.r2_tbl[r2] = tbl;
    }
    wave_sync();
    int best = -1, cur = g.part2_3_length;
    for (int r2 = 2; r2 < SBMAX_l + 1; r2++) {
        if (Q.sfb_l[r2] >= bigv) break;
        int bits = L.r01_bits[r2 - 2] + c2.count1bits;
        if (cur <= bits) break;
        bits += L.r2_bits[r2];
        if (cur <= bits) continue;
        cur = bits; best = r2;
    }
    best = uni(best);
    if (best >= 0) {
        g = c2;
        g.part2_3_length = uni(cur);
        g.region0_count = L.r01_div[best - 2];
        g.region1_count = best - 2 - L.r01_div[best - 2];
        g.table_select[0] = L.r0_tbl[best - 2];
        g.table_select[1] = L.r1_tbl[best - 2];
        g.table_select[2] = L.r2_tbl[best];
    }
    wave_sync();
}

LHIP_DEV void q_best_huffman_divide(const Tables& T, GI& g, int lane, QuantLds& L, const QuantTabs& Q) {
    if (g.block_type == SHORT_TYPE && T.mode_gr == 1) return;     // Takehiro.js:735-737
    lane = fresh_lane(lane);
    const int16_t* ix = L.ixw;
    GI c2 = g;
    if (g.block_type == NORM_TYPE) {
        // recalc_divide_init: every (region0, region1) split evaluated from the per-band statistics
        q_band_stats(T, ix, g.big_values, lane, L, Q);
        const int bigv = g.big_values;
        LHIP_LANE_ONCE(s, 0, 24) { L.r01_bits[s] = LARGE_BITS; L.r01_div[s] = 0; L.r0_tbl[s] = 0; L.r1_tbl[s] = 0; }
        // all 16 x 8 splits in parallel; candidate bits go to cand[r0 + r1][r0]
        for (int c = lane; c < 128; c += LHIP_NL) {
            const int r0 = c >> 3, r1 = c & 7, sidx = r0 + r1;
            if (sidx > 20) continue;
            int bits = LARGE_BITS;
            if (Q.sfb_l[r0 + 1] < bigv && Q.sfb_l[r0 + r1 + 2] < bigv) {
                bits = 0;
                q_choose_from_stats(T, 0, r0 + 1, &bits, L, Q);
                q_choose_from_stats(T, r0 + 1, r0 + r1 + 2, &bits, L, Q);
            }
            L.hd.cand[sidx][r0] = (int16_t)(bits > 0x7fff ? 0x7fff : bits);
        }
        wave_sync();
        // lane s: the first r0 (ascending) with the strictly smallest bits wins, as in the reference's loop order
        LHIP_LANE_ONCE(sidx, 0, (20) + 1) {
            int bb = 0x7fff, bd = -1;               // 0x7fff == no valid split (the reference keeps LARGE_BITS there)
            for (int r0 = (sidx > 7 ? sidx - 7 : 0); r0 < 16 && r0 <= sidx; r0++)
                if (bb > L.hd.cand[sidx][r0]) { bb = L.hd.cand[sidx][r0]; bd = r0; }
            if (bd >= 0) {
                int dummy = 0;
                L.r01_bits[sidx] = bb; L.r01_div[sidx] = bd;
                L.r0_tbl[sidx] = q_choose_from_stats(T, 0, bd + 1, &dummy, L, Q);
                L.r1_tbl[sidx] = q_choose_from_stats(T, bd + 1, sidx + 2, &dummy, L, Q);
            }
        }
        wave_sync();
        q_recalc_divide_sub(T, c2, g, lane, L, Q);
    }
    int i = c2.big_values;
    if (i == 0 || (ix[i - 2] | ix[i - 1]) > 1) return;
    i = g.count1 + 2;
    if (i > 576) return;
    c2 = g;
    c2.count1 = i;
    // quads from count1 + 2 down to the old big_values (all values <= 1 there)
    const int nq = (i - c2.big_values + 3) >> 2;
    int a12 = 0;
    for (int k = lane; k < nq; k += LHIP_NL) {
        const int e = i - 4 * k;
        const int p = ((ix[e - 4] * 2 + ix[e - 3]) * 2 + ix[e - 2]) * 2 + ix[e - 1];
        a12 += Q.t32l[p] + (Q.t33l[p] << 16);
    }
    a12 = wave_sum(a12);
    int a1 = a12 & 0xffff, a2 = a12 >> 16;
    i -= 4 * nq;
    c2.big_values = i;
    c2.count1table_select = 0;
    if (a1 > a2) { a1 = a2; c2.count1table_select = 1; }
    c2.count1bits = a1;
    if (c2.block_type == NORM_TYPE) {
        if (c2.big_values != g.big_values) q_band_stats(T, ix, c2.big_values, lane, L, Q);   // statistics must honour the new limit
        q_recalc_divide_sub(T, c2, g, lane, L, Q);
    } else {
        c2.part2_3_length = a1;
        a1 = Q.sfb_l[7 + 1];
        if (a1 > i) a1 = i;
        if (a1 > 0) c2.table_select[0] = q_choose_table(T, ix, 0, a1, &c2.part2_3_length, lane, L, Q);
        if (i > a1) c2.table_select[1] = q_choose_table(T, ix, a1, i, &c2.part2_3_length, lane, L, Q);
        if (g.part2_3_length > c2.part2_3_length) g = c2;
    }
}
}  // namespace lhip
