// CBR quantization / noise-shaping loop as a wave program: one 64-lane wavefront owns one frame
// and runs granule 0 (all channels) then granule 1, exactly as the reference's
// CBRNewIterationLoop.iteration_loop does (CBRNewIterationLoop.js:25-90).  Inside a
// granule-channel the *control flow* of the reference (Quantize.js outer_loop 871-1052,
// bin_search_StepSize 322-381, balance_noise 793-846, ...) is executed uniformly by all lanes,
// while every loop over the 576 spectral lines / the scalefactor bands is spread over the lanes:
//   - quantize x^(3/4) lines (Takehiro.js:102-314): five pairs per lane, per-band decisions as ballots
//   - Huffman bit counting (Takehiro.js:319-628): region maxima and packed length sums by
//     integer wave reductions (exact, order-free)
//   - noise per scalefactor band (QuantizePVT.js:725-878): nine consecutive lines per lane, the bands' f64 sums in the
//     reference's line order as a systolic fold over the lanes (f64 sums are order-sensitive, so they are never tree-reduced);
//     the per-band rest (distortion ratio, class, cache) one lane per band
// State (GrInfo scalars) is wave-uniform and lives in registers; spectra and per-band arrays live in LDS.
//
// Map of the files.  The stages up to the search itself are headers of their own, included below in dependency order, each with what it holds.
// This file holds what runs around the search: iteration_finish_one (q_best_scalefac_store, q_best_huffman_divide), the seed chain and a frame's
// bit budget, the granule-channel program q_unit with the frame program kb_quant, and the seed-chain validation (kb_validate, kb_validate_fast*).
// Beside it, included by the translation unit: k_quant_tail.h (how a persistent launch ends), k_quant_fast.h (the quality-7 pass) and
// k_quant_probe.h (the test hook over the search's pure functions).
#pragma once
#include "k_quant_prof.h"       // observation scaffolding: PH_* / HO_* profiling macros, the host simulations' counters
#include "k_quant_tabs.h"       // GI, the LDS table image (QuantTabs), the per-wave LDS record (QuantLds), small helpers
#include "k_quant_init.h"       // init_outer_loop, init_xrpow, ordered band sums, calc_xmin and the search limits
#include "k_quant_count.h"      // quantize_xrpow, Huffman region plans, noquant_count_bits / count_bits
#include "k_quant_noise.h"      // calc_noise
#include "k_quant_helper.h"     // count_bits on a helper wave (latency kernels)
#include "k_quant_amp.h"        // scale_bitcount, amplification, balance_noise
#include "k_quant_search.h"     // quant_compare, the bin-search step (bs_advance), the memo flush, bin_search_StepSize + outer_loop (q_outer_loop)
#include "k_quant_framebits.h"  // frame_bits_of, frame_padding (all that k_bits.h needs)

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

// Huffman statistics per scalefactor band over the pairs below `limit`, then turned into prefix sums over
// bands so that any union of whole bands [b0, b1) costs O(1):
// row 0 max (kept per band), 1 t1, 2 table23 (packed), 3 table56 (packed), 4..6 t7-9, 7..9 t10-12, 10..12 t13-15,
// 13 largetbl hi, 14 largetbl lo, 15 number of escaped values.  A row is only meaningful for regions whose
// maximum admits the table group, which is exactly when the reference would look at it.
LHIP_DEV void q_band_max_tables(int lane, QuantLds& L);
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

// ---------------------------------------------------------------------------------------------
// Bin-search seed chain (Quantize.js:324-326, 377-378: gfc.OldValue / gfc.CurrentStep).
// The seed of a granule-channel is a function of the bin-search results of the two most recent
// *active* granules of that channel: start = gain[p1], step = (start_of_p1 - gain[p1] >= 4) ? 4 : 2
// with start_of_p1 = gain[p2].  Frames are quantized speculatively (kb_quant with chain == 0 uses the
// reset seed), then kb_validate re-runs every bin search with the chain-implied seed and flags
// frames whose result differs; flagged frames are re-quantized with chain == 1 until none is left.
// ---------------------------------------------------------------------------------------------
struct Seed { int start, step; };

// seed seen by granule (k, gr) of channel ch, derived from the records of all earlier granules
LHIP_DEV Seed seed_before(const Workspace& W, const StreamDesc& sd, int C, int k, int gr, int ch) {
    const int32_t* carry = W.seed + ((int64_t)sd.fslot0 * C + ch) * 2;
    int g1 = -1, g2 = -1;                                    // gains of the last / second-to-last active granule
    const int GR = W.mode_gr;                                 // side records are laid out [frame][2][C] whatever GR is
    for (int q = GR * k + gr - 1; q >= 0; q--) {
        const GrSide* r = W.side + (((int64_t)sd.out_slot0 + q / GR) * 2 + q % GR) * C + ch;
        if (r->active) {
            if (g1 < 0) g1 = r->bs_gain;
            else { g2 = r->bs_gain; break; }
        }
    }
    Seed s;
    if (g1 < 0) { s.start = carry[0]; s.step = carry[1]; }
    else {
        const int prev_start = (g2 < 0) ? carry[0] : g2;
        s.start = g1;
        s.step = (prev_start - g1 >= 4) ? 4 : 2;
    }
    return s;
}

// perceptual entropy of one channel of one psy call (pecalc_l / pecalc_s, PsyModel.js:845-905) from the maskings E (layout E_*)
LHIP_DEV double q_pecalc(const float* E, int is_short, double masking_lower) {
    const double regcoef_s[12] = {11.8, 13.6, 17.2, 32, 46.5, 51.3, 57.5, 67.1, 71.5, 84.6, 97.6, 130};
    const double regcoef_l[21] = {6.8, 5.8, 5.8, 6.4, 6.5, 9.9, 12.1, 14.4, 15, 18.9, 21.6, 26.9, 34.2, 40.2, 46.8, 56.5, 60.7, 73.9, 85.7, 93.4, 126.1};
    const double LOG10 = 2.30258509299404568402;
    double pe;
    if (is_short) {
        pe = const_here(1236.28 / 4);
        for (int sb = 0; sb < SBMAX_s - 1; sb++)
            for (int sblock = 0; sblock < 3; sblock++) {
                const double thm = E[E_THM_S + sb * 3 + sblock];
                if (thm > 0.0) {
                    const double x = thm * masking_lower, en = E[E_EN_S + sb * 3 + sblock];
                    if (en > x) {
                        if (en > x * 1e10) pe += regcoef_s[sb] * const_here(10.0 * LOG10);
                        else pe += regcoef_s[sb] * v8_log10(en / x);
                    }
                }
            }
    } else {
        pe = const_here(1124.23 / 4);
        for (int sb = 0; sb < SBMAX_l - 1; sb++) {
            const double thm = E[E_THM_L + sb];
            if (thm > 0.0) {
                const double x = thm * masking_lower, en = E[E_EN_L + sb];
                if (en > x) {
                    if (en > x * 1e10) pe += regcoef_l[sb] * const_here(10.0 * LOG10);
                    else pe += regcoef_l[sb] * v8_log10(en / x);
                }
            }
        }
    }
    return pe;
}

// Joint stereo: M/S or L/R for frame k of the stream (Encoder.js:520-561).  M/S when the perceptual entropy of the mid / side pair,
// summed over the frame's granules, is not larger than that of left / right, and both channels have the same block type in the
// first and in the last granule.  The entropies belong to the psy calls of this frame: maskings of the call before (slot - 1),
// block types of the granule, and the masking_lower the previous frame's last channel left behind (gfc.masking_lower; 1 before
// the first frame -- Lame.js:175).  Returns mode_ext: 0 or 2 (wave-uniform).
// The frame's perceptual entropies into L.nsum[granule * 4 + psy channel] (PsyModel.js:1352-1380): maskings of the psy call before
// (slot - 1), block types of the granule, and the masking_lower the previous frame's last channel left behind (gfc.masking_lower;
// 1 before the first frame -- Lame.js:175).
LHIP_DEV void q_frame_pe(const Tables& T, const Workspace& W, const StreamDesc& sd, int k, int lane, QuantLds& L) {
    const int GR = T.mode_gr, C = T.channels_out, Cp = T.psy_channels;
    const int bt_prev = W.blocktype[(int64_t)(sd.gslot0 + GR * k) * C + (C - 1)];    // carry slot for k == 0: -1 on a fresh stream
    const double ml = bt_prev < 0 ? 1.0 : (bt_prev != SHORT_TYPE ? T.masking_lower_long : T.masking_lower_short);
    wave_sync();
    LHIP_LANE_ONCE(it, 0, 4 * GR) {                                                  // lane = granule * 4 + psy channel
        const int gr = it >> 2, chn = it & 3;
        if (chn < Cp) {
            const int gs = sd.gslot0 + 1 + GR * k + gr;
            const int bt0 = W.blocktype[(int64_t)gs * C], bt1 = W.blocktype[(int64_t)gs * C + (C - 1)];
            const int type = chn < 2 ? (chn ? bt1 : bt0) : ((bt0 == SHORT_TYPE || bt1 == SHORT_TYPE) ? SHORT_TYPE : NORM_TYPE);
            L.nsum[it] = q_pecalc(W.E + ((int64_t)(gs - 1) * Cp + chn) * E_STRIDE, type == SHORT_TYPE, ml);
        }
    }
    wave_sync();
}

// Joint stereo: M/S or L/R for frame k of the stream (Encoder.js:520-561).  M/S when the perceptual entropy of the mid / side pair,
// summed over the frame's granules, is not larger than that of left / right, and both channels have the same block type in the
// first and in the last granule.  Returns mode_ext: 0 or 2 (wave-uniform); the entropies stay in L.nsum.
LHIP_DEV int q_ms_decision(const Tables& T, const Workspace& W, const StreamDesc& sd, int k, int lane, QuantLds& L) {
    const int GR = T.mode_gr;
    q_frame_pe(T, W, sd, k, lane, L);
    double sum_ms = 0., sum_lr = 0.;
    for (int gr = 0; gr < GR; gr++)
        for (int ch = 0; ch < 2; ch++) { sum_ms += L.nsum[4 * gr + 2 + ch]; sum_lr += L.nsum[4 * gr + ch]; }
    int ms = 0;
    if (sum_ms <= 1.00 * sum_lr) {
        const int g0 = sd.gslot0 + 1 + GR * k, g1 = g0 + GR - 1;
        if (W.blocktype[(int64_t)g0 * 2] == W.blocktype[(int64_t)g0 * 2 + 1] && W.blocktype[(int64_t)g1 * 2] == W.blocktype[(int64_t)g1 * 2 + 1]) ms = 2;
    }
    return uni(ms);
}

// on_pe (QuantizePVT.js:421-484) with ResvMaxBits (Reservoir.js:190-229), the bit reservoir in use.  The reference computes in JS
// numbers (doubles) except where it stores into Int32Arrays (targ_bits, add_bits): those stores truncate.  Returns max_bits.
LHIP_DEV double q_on_pe_resv(const Tables& T, const double* pe, int* targ, int mean_bits, int cbr, int ResvSize_i, int ResvMax_i) {
    const int C = T.channels_out;
    double ResvSize = ResvSize_i, ResvMax = ResvMax_i, tbits, add_b, extra_bits, max_bits, bits;
    int add_bits[2] = {0, 0};
    if (cbr != 0) ResvSize += mean_bits;
    tbits = mean_bits;
    if (ResvSize * 10 > ResvMax * 9) { add_b = ResvSize - (ResvMax * 9) / 10; tbits += add_b; }
    else { add_b = 0; tbits -= .1 * mean_bits; }
    extra_bits = (ResvSize < (ResvMax * 6) / 10 ? ResvSize : (ResvMax * 6) / 10);
    extra_bits -= add_b;
    if (extra_bits < 0) extra_bits = 0;
    max_bits = tbits + extra_bits;
    if (max_bits > MAX_BITS_PER_GRANULE) max_bits = MAX_BITS_PER_GRANULE;
    bits = 0;
    for (int ch = 0; ch < C; ++ch) {
        const double t = tbits / C;
        targ[ch] = js_toint32(t < MAX_BITS_PER_CHANNEL ? t : (double)MAX_BITS_PER_CHANNEL);
        add_bits[ch] = js_toint32((double)targ[ch] * pe[ch] / 700.0 - targ[ch]);
        if (add_bits[ch] > mean_bits * 3 / 4) add_bits[ch] = mean_bits * 3 / 4;
        if (add_bits[ch] < 0) add_bits[ch] = 0;
        if (add_bits[ch] + targ[ch] > MAX_BITS_PER_CHANNEL) add_bits[ch] = (MAX_BITS_PER_CHANNEL - targ[ch]) > 0 ? MAX_BITS_PER_CHANNEL - targ[ch] : 0;
        bits += add_bits[ch];
    }
    if (bits > extra_bits)
        for (int ch = 0; ch < C; ++ch) add_bits[ch] = js_toint32(extra_bits * add_bits[ch] / bits);
    for (int ch = 0; ch < C; ++ch) { targ[ch] += add_bits[ch]; extra_bits -= add_bits[ch]; }
    bits = 0;
    for (int ch = 0; ch < C; ++ch) bits += targ[ch];
    if (bits > MAX_BITS_PER_GRANULE)
        for (int ch = 0; ch < C; ++ch) {
            targ[ch] = js_toint32((double)targ[ch] * MAX_BITS_PER_GRANULE);
            targ[ch] = js_toint32((double)targ[ch] / bits);
        }
    return max_bits;
}

// reduce_side (QuantizePVT.js:486-534): M/S granules move bits from the side to the mid channel by the energy ratio; the
// reference's targ_bits is an Int32Array, so every store truncates
LHIP_DEV void q_reduce_side(int* targ, double ms_ener_ratio, int mean_bits, double max_bits) {
    double fac = .33 * (.5 - ms_ener_ratio) / .5;
    if (fac < 0) fac = 0;
    if (fac > .5) fac = .5;
    int move_bits = js_toint32(fac * .5 * (targ[0] + targ[1]));
    if (move_bits > MAX_BITS_PER_CHANNEL - targ[0]) move_bits = MAX_BITS_PER_CHANNEL - targ[0];
    if (move_bits < 0) move_bits = 0;
    if (targ[1] >= 125) {
        if (targ[1] - move_bits > 125) {
            if (targ[0] < mean_bits) targ[0] += move_bits;
            targ[1] -= move_bits;
        } else {
            targ[0] += targ[1] - 125;
            targ[1] = 125;
        }
    }
    move_bits = targ[0] + targ[1];
    if (move_bits > max_bits) {
        targ[0] = js_toint32((max_bits * targ[0]) / move_bits);
        targ[1] = js_toint32((max_bits * targ[1]) / move_bits);
    }
}

// returns max_bits of on_pe (tbits + extra_bits, extra_bits = 0 here, capped at the per-granule limit)
LHIP_DEV int targ_bits_for(const Tables& T, int mean_bits, int gr, int ResvSize, int* targ) {
    // on_pe + ResvMaxBits(cbr = gr) with the reservoir disabled (QuantizePVT.js:421-484, Reservoir.js:190-229)
    const int C = uni_here(T.channels_out);
    int rs = ResvSize, tbits, bits = 0;
    if (gr != 0) rs += mean_bits;
    tbits = mean_bits;
    if (rs * 10 > 0) tbits += rs;
    for (int ch = 0; ch < C; ++ch) {
        const double t = (double)tbits / C;
        targ[ch] = js_toint32(t < MAX_BITS_PER_CHANNEL ? t : (double)MAX_BITS_PER_CHANNEL);
        bits += targ[ch];
    }
    if (bits > MAX_BITS_PER_GRANULE)
        for (int ch = 0; ch < C; ++ch) {
            targ[ch] = js_toint32((double)targ[ch] * MAX_BITS_PER_GRANULE);
            targ[ch] = js_toint32((double)targ[ch] / bits);
        }
    return tbits < MAX_BITS_PER_GRANULE ? tbits : MAX_BITS_PER_GRANULE;
}

// One granule-channel of a frame, from the spectrum to the published record: init_outer_loop .. best_huffman_divide (the body of the
// reference's per-channel loop, Quantize.js:1406-1466 CBR_iteration_loop + iteration_finish_one) on the calling wave's LDS record.
// `used` = the bin-search seed, `gr0_bt` = this channel's block type in granule 0 (scfsi); L.sf_gr0[ch] is written by granule 0 and read
// by granule 1 of the same channel.  Returns the bits spent (part2_3 + part2), the seed the next granule of this channel starts from
// (valid if `active`) and the block type.
struct UnitOut { int bits; Seed next; int block_type; int active; };
// Inlined at every call site: behind a call (one copy of the code for kb_quant's, the owner's and the helper's site) g_quant was a third slower -- spills around the call.
// SKIP == 1 (the batch kernels): a granule-channel whose lines 512..575 are all zero runs its per-pair rounds without the last one (GI::tail0)
template <int SKIP = 0>
LHIP_DEV UnitOut q_unit(const Tables& T, const PowBase& pb10, const Workspace& W, int C, int Cp, int fidx, int gslot, int gr, int ch, int mode_ext,
                        double ath_adjust, int targ_ch, Seed used, int gr0_bt, int lane, QuantLds& L, const QuantTabs& Q, CountShare* cs = nullptr) {
    lane = lane_anew(lane);        // (here and below: lane-derived LDS / HBM addresses are formed where they are used, not parked in scratch across the search)
    UnitOut u; u.next = used;
    GI g;
#if defined(LHIP_HOSTSIM)
    // simulations only: what the unit before left in the words 256..287 of the working spectrum is made visible -- at 44.1 / 48 kHz those lines lie in the
    // last band, beyond big_values and count1, where a stale value of ordinary size changes no byte; a unit that runs without the last round must zero them
    if (SKIP) { for (int i = 256 + lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0x1fff1fffu; wave_sync(); }
#endif
    const int bt = W.blocktype[(int64_t)gslot * C + ch];
    const double masking_lower = (bt != SHORT_TYPE) ? T.masking_lower_long : T.masking_lower_short;
    const float* ratio = W.E + ((int64_t)(gslot - 1) * Cp + ch + mode_ext) * E_STRIDE;   // thresholds of the previous psy call (mid / side: channels 2, 3)
    { PH_BEGIN(); q_init_outer_loop(T, pb10, ath_adjust, g, bt, xr_source(W, C, gslot, ch, mode_ext == 2), mode_ext == 2 ? nullptr : W.xr + ((int64_t)gslot * C + ch) * 576, 0, lane, L, Q); PH_END(L, PH_INIT); }
    int active = 0, bs_gain = 0;
    if (q_init_xrpow(g, lane, L, Q)) {
        active = 1;
        { PH_BEGIN(); q_calc_xmin(T, ath_adjust, masking_lower, ratio, g, lane, L, Q, SKIP); PH_END(L, PH_XMIN); }
        if constexpr (SKIP != 0) {
            // L.ixw outlives a granule-channel: no evaluation of this search writes the words 256..287, so they must not keep what the
            // unit before left there.  `kept`, the published spectrum and everything read after the search cover all 576 lines as before.
            if (g.tail0) { for (int i = 256 + lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0u; wave_sync(); }
        }
        int16_t* kept = cs ? cs->kept : W.l3 + (((int64_t)fidx * 2 + gr) * C + ch) * 576;
        { PH_BEGIN(); q_outer_loop<SKIP>(T, g, targ_ch, used.start, used.step, &bs_gain, kept, W.side + ((int64_t)fidx * 2 + gr) * C + ch, W.vdig + ((int64_t)fidx * 2 + gr) * C + ch, W.vdig_n, lane, L, Q, cs); PH_END(L, PH_XRPOW); }   // (profiling builds: the whole search in the otherwise unused slot)
        uni_gi(g); bs_gain = uni(bs_gain);
        lane = lane_anew(lane);
        wave_sync();                                    // the kept spectrum was written by other lanes of this wave
#if LHIP_NL == 1
        for (int i = lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = ((const uint32_t*)kept)[i];
#else
        {   // all of a lane's words in flight at once (a lane-strided loop waits for every load by itself)
            uint32_t kw[NPL];
#pragma unroll
            for (int j = 0; j < NPL; j++) { const int i = lane + LHIP_NL * j; kw[j] = ((const uint32_t*)kept)[i < 288 ? i : 287]; }
#pragma unroll
            for (int j = 0; j < NPL; j++) LHIP_PIN_LOADED(kw[j]);
#pragma unroll
            for (int j = 0; j < NPL; j++) { const int i = lane + LHIP_NL * j; if (i < 288) ((uint32_t*)L.ixw)[i] = kw[j]; }
        }
#endif
        wave_sync();
        Seed nx; nx.step = (used.start - bs_gain >= 4) ? 4 : 2; nx.start = bs_gain;
        u.next = nx;
    } else {
        for (int i = lane; i < 576; i += LHIP_NL) L.ixw[i] = 0;
        wave_sync();
    }
    int scfsi[4];
    { PH_BEGIN(); q_best_scalefac_store(T, g, gr, ch, gr0_bt, scfsi, lane, L, Q); PH_END(L, PH_SFSTORE); }
    uni_gi(g);
    if (T.use_best_huffman == 1) { PH_BEGIN(); q_best_huffman_divide(T, g, lane, L, Q); PH_END(L, PH_HUFFDIV); }
    uni_gi(g);
    u.bits = g.part2_3_length + g.part2_length;
    u.block_type = g.block_type;
    if (gr == 0) { LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) L.sf_gr0[ch][i] = (int8_t)L.sfb[i]; }
    // ---- publish the record and the signed quantized spectrum ----
    // (q_unit_fast, k_quant_fast.h, carries the same statements and must change with these: as one function called from both units they cost
    // g_quant_fast one or two vector registers and the latency kernels one, profiles/quant_split_shared_sites_resources.txt)
    lane = lane_anew(lane);
    GrSide* out = W.side + ((int64_t)fidx * 2 + gr) * C + ch;
    if (lane == 0) {
        out->part2_3_length = g.part2_3_length; out->part2_length = g.part2_length; out->big_values = g.big_values;
        out->count1 = g.count1; out->global_gain = g.global_gain; out->scalefac_compress = g.scalefac_compress;
        out->block_type = g.block_type;
        for (int i = 0; i < 3; i++) { out->table_select[i] = g.table_select[i]; out->subblock_gain[i] = g.subblock_gain[i]; }
        out->region0_count = g.region0_count; out->region1_count = g.region1_count; out->preflag = g.preflag;
        out->scalefac_scale = g.scalefac_scale; out->count1table_select = g.count1table_select;
        out->sfbmax = g.sfbmax; out->sfbdivide = g.sfbdivide;
        out->active = active; out->bs_start = used.start; out->bs_step_in = used.step; out->bs_gain = bs_gain;
        W.vdig[((int64_t)fidx * 2 + gr) * C + ch] = vd_head(active, used.start, used.step, bs_gain);      // digest word VD_HEAD
        out->targ_bits = targ_ch;
        out->mode_ext = uni_here(mode_ext);      // (formed here: hoisted to the frame's start as a vector copy, it would be the one value the search spills)
        out->scfsi = scfsi[0] | (scfsi[1] << 1) | (scfsi[2] << 2) | (scfsi[3] << 3);
    }
    LHIP_LANE_ONCE(i, 0, SFBMAX) out->scalefac[i] = L.sfb[i];
    if (!active && lane == 0) { out->bs_ntab = 0; out->bs_state = 0; }
    int16_t* l3o = W.l3 + (((int64_t)fidx * 2 + gr) * C + ch) * 576;
    for (int i = lane; i < 576; i += LHIP_NL) {
        const int v = L.ixw[i];
        l3o[i] = (int16_t)(((double)L.xr[i] < 0) ? -v : v);
    }
    wave_sync();
    u.active = active;
    return u;
}

// One wave per frame slot.  chain == 0: speculative reset seed (exact for the first frame of a stream
// batch, whose seed is the carried one); chain == 1: chain-implied seed (repair pass, flagged frames only);
// chain == 2: the frames of the stream are quantized in order (bit reservoir: the persistent per-stream kernel), the seed is what the
// frame before left in W.seed[fslot - 1] and this frame leaves its own in W.seed[fslot] (no walk back through the side records).
// rvp (RESV only): the stream's reservoir record -- in global memory (one-frame launches) or in the LDS of the per-stream kernel.
// PAIR == 1 (latency path for small stereo batches, g_quant_pair): the workgroup is two waves, wave `my_ch` does that
// channel only -- the channels of a granule are independent given the granule's bit budget -- and the two meet once per
// granule to exchange the bits they used (ResvSize feeds the next granule's budget) through `mbox` in LDS.
// RESV == 1: the bit-reservoir extension (Tables::disable_reservoir == 0) -- a separate instantiation, so that the usual path carries none
// of its state (the entropies, the reservoir record) through the frame
template <int PAIR = 0, int RESV = 0, int SKIP = 0>
LHIP_DEV void kb_quant(const Tables& T, const PowBase& pb10, const Workspace& W, const StreamDesc* SD, int fslot,
                       int chain, int lane, QuantLds& L, const QuantTabs& Q, int my_ch = -1, int* mbox = nullptr, const ResvState* rvp = nullptr,
                       int* hint = nullptr, CountShare* cs = nullptr, const int* later_granules_ready = nullptr) {
    const int C = T.channels_out;
    const int st = W.fslot_stream[fslot];
    const StreamDesc sd = SD[st];
    const int k = fslot - sd.fslot0 - 1;
    if (k < 0) return;
    const int fidx = sd.out_slot0 + k;                    // dense frame index
    if (chain == 1 && !W.seed_flag[fidx]) return;
#ifdef LHIP_PHASE_PROF
    const unsigned long long ph_total0_ = __builtin_amdgcn_s_memtime();     // L.prof is zeroed / flushed once per wave by g_quant
#endif
    const double ath_adjust = W.ath_adjust[fslot];        // after adjust_ATH of this frame
    const int padding = frame_padding(T, sd, k);
    const int mean_bits = (frame_bits_of(T, padding) - T.sideinfo_len * 8) / T.mode_gr;
    // per-channel state as named scalars: a dynamically indexed local array would live in scratch memory,
    // and everything read back from scratch counts as divergent for the compiler
    Seed seed0, seed1;
    seed0.start = seed1.start = W.spec_start; seed0.step = seed1.step = W.spec_step;
    if (chain == 2) {
        const int32_t* ps = W.seed + (int64_t)(fslot - 1) * C * 2;
        seed0.start = uni(ps[0]); seed0.step = uni(ps[1]);
        if (C > 1) { seed1.start = uni(ps[2]); seed1.step = uni(ps[3]); }
    } else if (chain || k == 0) {
        seed0 = seed_before(W, sd, C, k, 0, 0);
        if (C > 1) seed1 = seed_before(W, sd, C, k, 0, 1);
    } else if (hint && hint[0] == st) {
        // speculation with a better guess than the reset seed: the gains this wave's previous frame OF THE SAME STREAM ended on (any seed
        // is legitimate here -- the validation replays the search with the chain-implied one); a steady stream's chain seeds look like this
        if (hint[1] >= 0) { seed0.start = hint[1]; seed0.step = 2; }
        if (C > 1 && hint[2] >= 0) { seed1.start = hint[2]; seed1.step = 2; }
    }
    int gr0_bt0 = 0, gr0_bt1 = 0;
    const int Cp = T.psy_channels;
    const int mode_ext = (T.mode == 1) ? q_ms_decision(T, W, sd, k, lane, L) : 0;      // joint stereo: this frame M/S (2) or L/R (0)
    // Bit reservoir (extension): the frame starts from the reservoir the previous frame left (one frame per stream and launch), its
    // budget follows the perceptual entropies (on_pe), and ResvFrameEnd's verdict goes to the bit packer, which commits it.
    constexpr bool resv = RESV != 0;
    const ResvState* rv = resv ? rvp : nullptr;
    int ResvSize = resv ? uni(rv->ResvSize) : 0;
    int ResvMax = 0;
    double pe_use[2][2] = {{0., 0.}, {0., 0.}};
    float pefir_new = 0.f;
    if constexpr (resv) {
        // ResvFrameBegin (Reservoir.js:130-180; brate <= 320, not strict_ISO)
        const int frameLength = frame_bits_of(T, padding), resvLimit = (8 * 256) * T.mode_gr - 8, maxmp3buf = 8 * 1440;
        ResvMax = maxmp3buf - frameLength;
        if (ResvMax > resvLimit) ResvMax = resvLimit;
        if (ResvMax < 0) ResvMax = 0;
        // the entropies of the maskings in use, scaled by the 19-frame FIR of their sums (Encoder.js:600-626; pefirbuf is a Float32Array)
        if (T.mode != 1) q_frame_pe(T, W, sd, k, lane, L);
        double f = 0.0;
        for (int gr = 0; gr < T.mode_gr; gr++)
            for (int ch = 0; ch < C; ch++) { pe_use[gr][ch] = L.nsum[4 * gr + ch + mode_ext]; f += pe_use[gr][ch]; }
        pefir_new = (float)f;
        {
            const double fircoef[9] = {-0.0207887 * 5, -0.0378413 * 5, -0.0432472 * 5, -0.031183 * 5, 7.79609e-18 * 5, 0.0467745 * 5,
                                       0.10091 * 5, 0.151365 * 5, 0.187098 * 5};
            // buffer after the shift: b[i] = old[i + 1] for i < 18, b[18] = the new sum
            f = rv->pefirbuf[10];
            for (int i = 0; i < 9; i++) f += ((double)rv->pefirbuf[i + 1] + (double)(i == 0 ? pefir_new : rv->pefirbuf[19 - i])) * fircoef[i];
        }
        f = (670 * 5 * T.mode_gr * C) / f;
        for (int gr = 0; gr < T.mode_gr; gr++)
            for (int ch = 0; ch < C; ch++) pe_use[gr][ch] *= f;
        wave_sync();
    }
    q_ath_pseudo(T, pb10, ath_adjust, lane, L, Q);          // the frame's analog-silence thresholds, both block kinds
    for (int gr = 0; gr < T.mode_gr; gr++) {
        const int gslot = sd.gslot0 + 1 + T.mode_gr * k + gr;
        // one-frame launch: the thresholds granule 1 quantizes against (psyB of granule 0) are computed by other waves WHILE granule 0 is
        // quantized; a one-channel frame has no workgroup barrier between its granules to order that, so it waits for their flag here
        if (gr > 0 && later_granules_ready) { (void)wg_wait_not(later_granules_ready, 0, 0, lane); wg_acquire(); }
        int targ[2] = {0, 0};
        const double max_bits = resv ? q_on_pe_resv(T, pe_use[gr], targ, mean_bits, gr, ResvSize, ResvMax) : (double)targ_bits_for(T, mean_bits, gr, ResvSize, targ);
        if (mode_ext == 2) {
            // Encoder.js:482-486: side / (mid + side) of the total energies the psy call of this granule handed back (one call of delay)
            const float* te = W.tot_ener + (int64_t)(gslot - 1) * 4;
            double r = (double)te[2] + (double)te[3];
            if (r > 0) r = (double)te[3] / r;
            q_reduce_side(targ, r, mean_bits, max_bits);
        }
        const int targ0 = uni(targ[0]), targ1 = uni(targ[1]);
        for (int ch = 0; ch < C; ch++) {
            if (PAIR && ch != my_ch) continue;
            const UnitOut u = q_unit<SKIP>(T, pb10, W, C, Cp, fidx, gslot, gr, ch, mode_ext, ath_adjust, ch == 0 ? targ0 : targ1, ch == 0 ? seed0 : seed1,
                                           ch == 0 ? gr0_bt0 : gr0_bt1, lane, L, Q, cs);
            if (u.active) { if (ch == 0) seed0 = u.next; else seed1 = u.next; }
            if (!PAIR) ResvSize = uni(ResvSize - u.bits);
            else if (lane == 0) mbox[2 * gr + ch] = u.bits;
            if (gr == 0) { if (ch == 0) gr0_bt0 = u.block_type; else gr0_bt1 = u.block_type; }
        }
        if (PAIR) {                                   // both waves have published this granule: take the other channel's bits
            if (cs) wg_store(&cs->state, CS_BARRIER, lane);     // (this wave's count helper keeps the barrier's count)
            wg_barrier();
            ResvSize = uni(ResvSize - (mbox[2 * gr] + mbox[2 * gr + 1]));
        }
    }
    if constexpr (resv) if (lane == 0 && (!PAIR || my_ch == 0)) {
        // ResvFrameEnd (Reservoir.js:243-293); main_data_begin is a double there (fractions of a byte survive in it)
        const double mdb0 = rv->main_data_begin;
        int rs = ResvSize + mean_bits * T.mode_gr, over_bits, stuffingBits = 0;
        if ((over_bits = rs % 8) != 0) stuffingBits += over_bits;
        over_bits = (rs - stuffingBits) - ResvMax;
        if (over_bits > 0) stuffingBits += over_bits;
        const double mdb_bytes = (mdb0 * 8 < stuffingBits ? mdb0 * 8 : (double)stuffingBits) / 8;
        FrameResv fr;
        fr.drain_pre = js_toint32(8 * mdb_bytes);
        stuffingBits -= fr.drain_pre;
        rs -= fr.drain_pre;
        fr.main_data_begin = mdb0 - mdb_bytes;
        fr.drain_post = stuffingBits;
        rs -= stuffingBits;
        fr.ResvSize = rs; fr.ResvMax = ResvMax; fr.pefir_new = pefir_new; fr.pad_ = 0;
        W.fr[fidx] = fr;
    }
    if (hint) { hint[0] = st; hint[1] = seed0.start; hint[2] = C > 1 ? seed1.start : -1; }
    if (chain == 1 && lane == 0) W.seed_flag[fidx] = 0;
    if (chain == 2 && lane == 0) {                            // OldValue / CurrentStep after this frame (every wave of a pair its own channel)
        int32_t* ps = W.seed + (int64_t)fslot * C * 2;
        if (!PAIR || my_ch == 0) { ps[0] = seed0.start; ps[1] = seed0.step; }
        if (C > 1 && (!PAIR || my_ch == 1)) { ps[2] = seed1.start; ps[3] = seed1.step; }
    }
#ifdef LHIP_PHASE_PROF
    if (lane == 0) { L.prof[PH_TOTAL] += (unsigned int)(__builtin_amdgcn_s_memtime() - ph_total0_); L.prof[32 + PH_TOTAL] += 1; }
#endif
}

// Replay the bin searches of a frame with the chain-implied seeds; flag the frame if any result differs.
// The search only asks for count_bits(gain) with all-zero scalefactors; the speculative pass left a memo of every
// such evaluation (GrSide::bs_tab), so most replays are pure scalar look-ups and the spectrum is only re-quantized
// on a miss.
template <int SKIP>
LHIP_DEV void kb_validate(const Tables& T, const PowBase& pb10, const Workspace& W, const StreamDesc* SD, int fslot,
                          int lane, QuantLds& L, const QuantTabs& Q) {
    const int C = T.channels_out;
    const int st = W.fslot_stream[fslot];
    const StreamDesc sd = SD[st];
    const int k = fslot - sd.fslot0 - 1;
    if (k < 0) return;
    const int fidx = sd.out_slot0 + k;
    if (uni(W.seed_flag[fidx]) != 2) return;                  // only frames the memo-only pass could not decide
    const double ath_adjust = W.ath_adjust[fslot];
    int bad = 0;
    for (int gr = 0; gr < T.mode_gr && !bad; gr++) {
        const int gslot = sd.gslot0 + 1 + T.mode_gr * k + gr;
        for (int ch = 0; ch < C && !bad; ch++) {
            const GrSide* rec = W.side + ((int64_t)fidx * 2 + gr) * C + ch;
            if (!rec->active) continue;
            const Seed s = seed_before(W, sd, C, k, gr, ch);
            if (s.start == rec->bs_start && s.step == rec->bs_step_in) continue;     // already quantized with this seed
            const int ntab = uni(rec->bs_ntab);
            // memo entry per lane (device) / linear search (host simulation)
            int my_ent = 0, my_asg = 0;
            LHIP_LANE_ONCE(i, 0, ntab) { my_ent = rec->bs_tab[i]; my_asg = rec->bs_asg[i]; }
            GI g;
            PrevNoise pn_none; pn_none.gain = 0; pn_none.sfb_count1 = 0;
            int inited = 0;
            // bin_search_StepSize (Quantize.js:322-381), part2_length == 0 at this point
            const int desired_rate = uni(rec->targ_bits);
            int gain = uni(s.start), CurrentStep = uni(s.step), flagGoneOver = 0, Direction = 0, up = 0;
            GI g0;                                          // conditionally assigned fields as init_outer_loop leaves them
            g0.table_select[0] = g0.table_select[1] = g0.table_select[2] = 0; g0.region0_count = 0; g0.region1_count = 0;
            int cstate = pack_cond_fields(g0, 0);
            for (;;) {
                int nBits = -1, asg = 0;
#if LHIP_NL == 1
                for (int i = 0; i < ntab; i++) if ((int)((uint32_t)rec->bs_tab[i] >> 24) == gain) { nBits = rec->bs_tab[i] & 0xffffff; asg = rec->bs_asg[i]; break; }
                (void)my_ent; (void)my_asg;
#else
                {
                    const uint64_t hit = wave_ballot(lane < ntab && (int)((uint32_t)my_ent >> 24) == gain);
                    if (hit) {
                        const int src = (int)__builtin_ctzll(hit);
                        nBits = wave_bcast(my_ent, src) & 0xffffff;
                        asg = wave_bcast(my_asg, src);
                    }
                }
#endif
                if (nBits < 0) {
                    if (!inited) {
                        const int ms = uni(rec->mode_ext) == 2;        // M/S granules were not written back: the silence rule runs again
                        if (ms) q_ath_pseudo(T, pb10, ath_adjust, lane, L, Q);
                        q_init_outer_loop(T, pb10, ath_adjust, g, W.blocktype[(int64_t)gslot * C + ch],
                                          xr_source(W, C, gslot, ch, ms), nullptr, ms ? 0 : 1, lane, L, Q);
                        q_init_xrpow(g, lane, L, Q);
                        // max_nonzero_coeff is set by calc_xmin in the reference before the bin search.  This mirrors q_search_limits (k_quant_init.h)
                        // and must change with it: calling it here moves g_fixup<1>'s scratch (92 -> 80 bytes), and the kernel is to stay as it was
                        if (g.block_type != SHORT_TYPE) {
                            int t = -1;
                            for (int i = lane; i < 576; i += LHIP_NL) if (!((double)L.xr[i] == 0)) t = i;
                            t = wave_max(t);
                            g.max_nonzero_coeff = (t >= 575) ? 575 : t + 1;
                            if (SKIP) g.tail0 = t < 512;
                        } else if (SKIP) g.tail0 = q_tail_is_zero(lane, L);         // as q_calc_xmin sets it (only the bit count is used here: stale words 256..287 of L.ixw are never read)
                        q_set_firstcut(g, lane, L);
                        inited = 1;
                    }
                    g.global_gain = gain;
                    nBits = q_count_bits_rounds<SKIP>(T, g, L.sfb, L.ixw, 0, pn_none, &asg, lane, L, Q);
                }
                nBits = uni(nBits);
                cstate = apply_cond_fields(cstate, uni(asg));
                if (!bs_advance(nBits, desired_rate, gain, CurrentStep, flagGoneOver, Direction, up)) break;
            }
            // the gain AND the path-dependent leftovers (table_select of empty regions, region counts) must be what the
            // speculative pass produced
            if (gain != rec->bs_gain || cstate != (rec->bs_state & ~15)) bad = 1;
        }
    }
    if (lane == 0) {
        W.seed_flag[fidx] = bad ? 1 : 0;
        if (bad) {
#ifdef LHIP_HOSTSIM
            W.nflagged[0] += 1;
#else
            atomicAdd(W.nflagged, 1);
#endif
        }
    }
}

// The chain-implied seed from the digests (what seed_before derives from the side records): gains of the last two active granules of the channel.
LHIP_DEV Seed seed_before_dig(const Workspace& W, const StreamDesc& sd, int C, int k, int gr, int ch) {
    const int32_t* carry = W.seed + ((int64_t)sd.fslot0 * C + ch) * 2;
    int g1 = -1, g2 = -1;
    const int GR = W.mode_gr;
    for (int q = GR * k + gr - 1; q >= 0; q--) {
        const uint32_t h = W.vdig[(((int64_t)sd.out_slot0 + q / GR) * 2 + q % GR) * C + ch];
        if (vd_active(h)) {
            if (g1 < 0) g1 = vd_gain(h);
            else { g2 = vd_gain(h); break; }
        }
    }
    Seed s;
    if (g1 < 0) { s.start = carry[0]; s.step = carry[1]; }
    else {
        const int prev_start = (g2 < 0) ? carry[0] : g2;
        s.start = g1;
        s.step = (prev_start - g1 >= 4) ? 4 : 2;
    }
    return s;
}

// Memo-only replay of ONE granule-channel's bin search with the chain-implied seed: a few scalar look-ups in the granule-channels' DIGESTS
// (W.vdig: seed used, resulting gain, target, the first VD_ENT memo entries; word-major, so the threads of a wave read neighbouring
// words) -- the side records, 464 bytes apart with the memo at their far end, are only read by a search with more than VD_ENT memoised
// evaluations.  Returns 0 consistent, 1 re-quantize the frame with the chain-implied seed, 2 undecided (a gain the speculative pass never
// evaluated) -> kb_validate decides.
LHIP_DEV int validate_fast_gc(const Tables& T, const Workspace& W, const StreamDesc& sd, int k, int fidx, int gr, int ch) {
    const int C = T.channels_out;
    const int64_t dn = W.vdig_n;
    const int64_t gc = ((int64_t)fidx * 2 + gr) * C + ch;
    const uint32_t* dig = W.vdig + gc;
    const uint32_t h = dig[0];
    if (!vd_active(h)) return 0;
    const Seed s = seed_before_dig(W, sd, C, k, gr, ch);
    if (s.start == vd_start(h) && s.step == vd_step(h)) return 0;
    const uint32_t tw = dig[VD_TARG * dn];
    const int ntab = (int)(tw >> 24), desired_rate = (int)(tw & 0xffffffu);
    const GrSide* rec = W.side + gc;
    int32_t et[VD_ENT], ea[VD_ENT];
#pragma unroll
    for (int i = 0; i < VD_ENT; i++) { et[i] = -1; ea[i] = 0; if (i < ntab) { et[i] = (int32_t)dig[(VD_TAB + 2 * i) * dn]; ea[i] = (int32_t)dig[(VD_TAB + 2 * i + 1) * dn]; } }
    int gain = s.start, CurrentStep = s.step, flagGoneOver = 0, Direction = 0, up = 0;
    GI g0;
    g0.table_select[0] = g0.table_select[1] = g0.table_select[2] = 0; g0.region0_count = 0; g0.region1_count = 0;
    int cstate = pack_cond_fields(g0, 0);
    for (;;) {
        int nBits = -1, asg = 0;
#pragma unroll
        for (int i = VD_ENT - 1; i >= 0; i--) if (i < ntab && (int)((uint32_t)et[i] >> 24) == gain) { nBits = et[i] & 0xffffff; asg = ea[i]; }   // the FIRST entry with that gain, as the record walk finds it
        if (nBits < 0 && ntab > VD_ENT)      // a long search: the entries beyond the digest are in the side record
            for (int i = VD_ENT; i < ntab; i++) { const int e = rec->bs_tab[i]; if ((int)((uint32_t)e >> 24) == gain) { nBits = e & 0xffffff; asg = rec->bs_asg[i]; break; } }
        if (nBits < 0) return 2;
        cstate = apply_cond_fields(cstate, asg);
        if (!bs_advance(nBits, desired_rate, gain, CurrentStep, flagGoneOver, Direction, up)) break;
    }
    return (gain != vd_gain(h) || cstate != (int)(dig[VD_STATE * dn] & ~15u)) ? 1 : 0;
}

// The frame's verdict from its granule-channels' (a definite "re-quantize" wins over "undecided": the re-quantization settles every
// granule-channel of the frame) -> W.seed_flag, the counters and the list of undecided frames.
LHIP_DEV void validate_fast_publish(const Workspace& W, int fslot, int fidx, int any1, int any2) {
    const int verdict = any1 ? 1 : any2 ? 2 : 0;
    W.seed_flag[fidx] = verdict;
    if (verdict) {
#ifdef LHIP_HOSTSIM
        const int pos = W.nflagged[verdict - 1]; W.nflagged[verdict - 1] += 1;
#else
        const int pos = atomicAdd(W.nflagged + (verdict - 1), 1);
#endif
        if (verdict == 2) W.slow_list[pos] = fslot;
    }
}

// One thread per frame (the persistent repair kernel's later passes, the host simulation).
// only_pass > 0: just the frames stamped for that pass (successors of frames the previous repair pass re-quantized)
LHIP_DEV void kb_validate_fast(const Tables& T, const Workspace& W, const StreamDesc* SD, int fslot, int only_pass = 0) {
    const int C = T.channels_out;
    const StreamDesc sd = SD[W.fslot_stream[fslot]];
    const int k = fslot - sd.fslot0 - 1;
    if (k < 0) return;
    const int fidx = sd.out_slot0 + k;
    if (only_pass > 0 && W.reval[fidx] != only_pass) return;
    int any1 = 0, any2 = 0;
    for (int gr = 0; gr < T.mode_gr && !any1; gr++)
        for (int ch = 0; ch < C && !any1; ch++) { const int v = validate_fast_gc(T, W, sd, k, fidx, gr, ch); any1 |= (v == 1); any2 |= (v == 2); }
    validate_fast_publish(W, fslot, fidx, any1, any2);
}

#ifndef LHIP_HOSTSIM
// The first pass over a whole batch (g_validate_fast): FOUR lanes per frame, one per granule-channel -- a frame's check is a chain of
// dependent look-ups (the two previous granules' digests, then the memo), and one thread per frame left the chip with a wave and a half
// per SIMD waiting on them (0.27 ms per 1e5 two-channel frames); the quad's verdicts meet through DPP and its first lane publishes.
struct ValidateShare { int total[2], base[2], woff[4][2]; };      // g_validate_fast: 256 threads = 4 waves
LHIP_DEV void kb_validate_fast_quad(const Tables& T, const Workspace& W, const StreamDesc* SD, int fslot, int sub, bool live, ValidateShare& S) {
    const int C = T.channels_out;
    int v = 0, fidx = 0;
    bool has = false;
    if (live) {
        const StreamDesc sd = SD[W.fslot_stream[fslot]];
        const int k = fslot - sd.fslot0 - 1;
        if (k >= 0) {
            has = true;
            fidx = sd.out_slot0 + k;
            const int gr = sub / C, ch = sub - gr * C;
            if (gr < T.mode_gr) v = validate_fast_gc(T, W, sd, k, fidx, gr, ch);
        }
    }
    // OR over the four lanes of the quad (bit 0: some granule-channel says "re-quantize", bit 1: some is undecided)
    int m = (v == 1 ? 1 : 0) | (v == 2 ? 2 : 0);
    m |= __builtin_amdgcn_mov_dpp(m, 0xB1, 0xF, 0xF, true);      // quad_perm [1,0,3,2]
    m |= __builtin_amdgcn_mov_dpp(m, 0x4E, 0xF, 0xF, true);      // quad_perm [2,3,0,1]
    // The quad's first lane publishes.  The counters are bumped ONCE PER WORKGROUP: on steady material a quarter to a third of the frames are
    // "undecided" (profiles/r04_pass6_validate_stats.txt), and 23-32 k returning atomics on one address serialise in the L2 -- that, not the
    // replay, was this kernel's time (0.26 ms stereo / 0.37 ms mono per 1e5 frames, in proportion to the undecided frames).  Every wave ranks
    // its publishing lanes with ballots, the waves meet in LDS, one thread per counter talks to global memory, and the list slots follow from
    // the ranks.  (The order of W.slow_list is immaterial: g_fixup spreads its entries over its waves.)
    const bool pub = has && sub == 0;
    const int verdict = pub ? ((m & 1) ? 1 : (m & 2) ? 2 : 0) : 0;
    if (pub) W.seed_flag[fidx] = verdict;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const uint64_t b1 = __ballot(verdict == 1), b2 = __ballot(verdict == 2);
    if (threadIdx.x < 2) S.total[threadIdx.x] = 0;
    __syncthreads();
    if (lane == 0) {                                 // this wave's offsets inside the workgroup's share (LDS atomics: cheap, returning)
        S.woff[wv][0] = b1 ? atomicAdd(&S.total[0], (int)__builtin_popcountll(b1)) : 0;
        S.woff[wv][1] = b2 ? atomicAdd(&S.total[1], (int)__builtin_popcountll(b2)) : 0;
    }
    __syncthreads();
    if (threadIdx.x < 2) { const int n = S.total[threadIdx.x]; S.base[threadIdx.x] = n ? atomicAdd(W.nflagged + threadIdx.x, n) : 0; }
    __syncthreads();
    if (verdict == 2) W.slow_list[S.base[1] + S.woff[wv][1] + (int)__builtin_popcountll(b2 & ((1ull << lane) - 1))] = fslot;
}
#endif

}  // namespace lhip
