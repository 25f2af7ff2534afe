// k_quant_count.h -- one evaluation of the search: quantize_xrpow into registers and LDS, the Huffman region plans, noquant_count_bits and
// count_bits over the pairs of the lanes (q_count_bits_rounds picks the round count of the granule-channel).
#pragma once
#include "k_quant_tabs.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// quantize_xrpow (Takehiro.js:171-314) -> ix ; `use_prev` = the prev_noise cache (pn_* in LDS) is live
// ---------------------------------------------------------------------------------------------
// Lane l owns the PAIRS 2(l + 64 j), +1 (bands start and end on even lines, so a pair never straddles a band):
// xrpow comes in as one 8-byte load and ix goes out as one 32-bit store per pair, and the quantized values stay in
// registers (vx, vy) for the Huffman bit count that follows -- no LDS round trip between the two.
enum { NPL = (288 + LHIP_NL - 1) / LHIP_NL };
// The pairs 256..287 (lines 512..575) are the last round, on half the lanes.  Up to 256 kbps the encoder's lowpass leaves those lines
// exactly zero in a long block, so they quantize to zero whatever the gain: with GI::tail0 set the per-pair functions run NR = NPL_HEAD
// rounds, and the words 256..287 of the working spectrum are zeroed once per granule-channel instead (q_unit).
enum { NPL_HEAD = 256 / LHIP_NL };

template <int NR>
LHIP_DEV void q_quantize(const Tables& T, const GI& g, const int32_t* scalefac, int16_t* ix, int use_prev,
                         int pn_gain, int pn_sfb_count1, int (&vx)[NR], int (&vy)[NR], int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    const double istep = ipow20(Q, g.global_gain);
    // every truncated product is <= xrpow_max * istep: below QT_N no lane can need the part of adj43 that is not staged in LDS
    const int may_big = !(g.xrpow_max * istep < (double)QT_N);
    const int sfbmax = (g.block_type == SHORT_TYPE) ? 38 : 21;
    const int prev_data_use = use_prev && (g.global_gain == pn_gain);
    // per-band decision as wave-uniform bit masks: cached (keep old values) / 0-1 shortcut; the first
    // non-cached band reaching past max_nonzero_coeff (sstar) is quantized partially and ends the walk
    unsigned long long tm_ = PH_NOW(); (void)tm_;
    // the lines first: their LDS latency passes while the band masks are formed
    float xa[NR], xb[NR];
#pragma unroll
    for (int j = 0; j < NR; j++) {
        const int p = 2 * (lane + LHIP_NL * j);
        xa[j] = 0.f; xb[j] = 0.f;
        if (p < 576) { struct F2 { float x, y; }; const F2 xx = *(const F2*)(L.xrpow + p); xa[j] = xx.x; xb[j] = xx.y; }   // 8-byte aligned: p is even
    }
    uint64_t m_cached = 0, m_zo = 0;                     // bit sfb, produced by lane sfb (sfbmax < 64)
    if (use_prev) {                                      // bin-search rounds have no cache and no 0/1 shortcut: nothing to decide
        LHIP_LANE_ONCE(sfb, 0, (sfbmax) + 1) {
            int step = -1;
            const int pstep = L.pn_step[sfb];
            if (prev_data_use || g.block_type == NORM_TYPE) step = sf_step(Q, g, scalefac, L.window, sfb);
            if (prev_data_use && pstep == step) m_cached |= 1ull << sfb;
            else if (pn_sfb_count1 > 0 && sfb >= pn_sfb_count1 && pstep > 0 && step >= pstep) m_zo |= 1ull << sfb;
        }
    }
    m_cached = wave_lane_bits(m_cached); m_zo = wave_lane_bits(m_zo);
    // the bands reaching past max_nonzero_coeff are firstcut .. sfbmax; the walk ends in the first of them that is not cached
    const uint64_t m_cut = (use_prev && g.firstcut <= sfbmax) ? ((~0ull << g.firstcut) & ((2ull << sfbmax) - 1) & ~m_cached) : 0;
    const int sstar = m_cut ? (int)__builtin_ctzll(m_cut) : 99;
    // The reference stops quantizing inside band sstar (at max_nonzero_coeff, rounded to a pair) and fills the rest with
    // zeros.  Every line from max_nonzero_coeff on has xrpow == 0 (it is the first of the spectrum's trailing zeros, or
    // 575 with a full last band) and quantizes to 0 by either formula, and the kept values of cached bands are zero there
    // by induction, so that walk needs no masks here; what remains of it is that the partial band never takes the 0/1
    // shortcut.
    if (sstar <= sfbmax) m_zo &= ~(1ull << sstar);
    PH_MARK(L, PH_Q_MASK, tm_);
    const uint8_t* l2s = line2sfb(Q, g.block_type);
    const int need_old = (m_cached != 0);
    const float istep_f = Q.ipow20[g.global_gain];     // the Float32Array value itself; `istep` above is its f64 image
    // staged, branch-light form: all loads of a stage are independent so they overlap (LDS latency is the cost here); the two
    // truncations of every line are q_floor_prod / q_floor_fma (lhip_math.h)
    int ra[NR], rb[NR];
    q_floor_prod(xa, xb, istep_f, ra, rb);                                 // 0 <= x <= 8206: truncation == ToInt32
    float aa[NR], ab[NR];
    if (!may_big) {                                                        // every product is below QT_N (see may_big): nothing to clamp
#pragma unroll
        for (int j = 0; j < NR; j++) { aa[j] = Q.adj43[ra[j]]; ab[j] = Q.adj43[rb[j]]; }
    } else {                                                               // rare: large quantized values
#pragma unroll
        for (int j = 0; j < NR; j++) { aa[j] = Q.adj43[ra[j] < QT_N ? ra[j] : QT_N - 1]; ab[j] = Q.adj43[rb[j] < QT_N ? rb[j] : QT_N - 1]; }
#pragma unroll
        for (int j = 0; j < NR; j++) {
            if (ra[j] >= QT_N) aa[j] = T.adj43[ra[j]];
            if (rb[j] >= QT_N) ab[j] = T.adj43[rb[j]];
        }
    }
    // no masking at the end of the spectrum: zero xrpow quantizes to (int)(0 + adj43[0]) = 0 (see above)
    q_floor_fma(xa, xb, istep_f, aa, ab, vx, vy);
    if (!need_old && m_zo == 0) {
        // the common round (every bin-search round and most others): no cached band, no 0/1 shortcut
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const int p = 2 * (lane + LHIP_NL * j);
            if (p < 576) *(uint32_t*)(ix + p) = (uint32_t)vx[j] | ((uint32_t)vy[j] << 16);
        }
    } else if (m_zo == 0) {
        // cached bands keep their values, nothing else
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const int p = 2 * (lane + LHIP_NL * j);
            int sf = 0; uint32_t oldw = 0;
            if (p < 576) { sf = l2s[p]; oldw = *(const uint32_t*)(ix + p); }
            const int cached = (int)((m_cached >> sf) & 1);
            const int va = cached ? (int)(oldw & 0xffffu) : vx[j], vb = cached ? (int)(oldw >> 16) : vy[j];
            vx[j] = va; vy[j] = vb;
            if (p < 576) *(uint32_t*)(ix + p) = (uint32_t)va | ((uint32_t)vb << 16);
        }
    } else {
        // 0/1 shortcut (Takehiro.js:187-210): ix = (compareval0 > xrpow) ? 0 : 1 with compareval0 = (1 - 0.4054) / istep in f64.  xrpow is a
        // Float32 value, so the f64 comparison is a Float32 one against zo_thr, the smallest Float32 not below compareval0:
        // compareval0 > x  <=>  x < zo_thr
        const double compareval0 = (1.0 - 0.4054) / istep;
        float zo_thr = (float)compareval0;
        if ((double)zo_thr < compareval0) zo_thr = f32_next_up(zo_thr);
        // the previous values are only fetched when some band is cached
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const int p = 2 * (lane + LHIP_NL * j);
            int sf = 0; uint32_t oldw = 0;
            if (p < 576) { sf = l2s[p]; if (need_old) oldw = *(const uint32_t*)(ix + p); }
            const int cached = (int)((m_cached >> sf) & 1), zo = (int)((m_zo >> sf) & 1);
            int va = vx[j], vb = vy[j];
            if (zo) { va = (xa[j] < zo_thr) ? 0 : 1; vb = (xb[j] < zo_thr) ? 0 : 1; }
            const int oa = (int)(oldw & 0xffffu), ob = (int)(oldw >> 16);
            va = cached ? oa : va;
            vb = cached ? ob : vb;
            vx[j] = va; vy[j] = vb;
            if (p < 576) *(uint32_t*)(ix + p) = (uint32_t)va | ((uint32_t)vb << 16);
        }
    }
    wave_sync();
    PH_MARK(L, PH_Q_LINES, tm_);
}

// ---------------------------------------------------------------------------------------------
// Huffman table choice for a set of pairs (Takehiro.js:336-516).  Region description for the one-pass counter.
// ---------------------------------------------------------------------------------------------
struct RegionPlan { int kind, t1, xlen, lb1, lb2, choice, choice2, o0, o1, o2; };   // kind 0 empty/zero, 1 t1, 2 table23/56, 4 triple, 5 ESC, 6 overflow

// ESC table pair for a maximum > 15 (Takehiro.js:479-497): linmax of table t is 2^linbits - 1, so "linmax >= mx"
// is "linbits >= bit length of mx"; linbits of tables 16..23 = 1,2,3,4,6,8,10,13 and of 24..31 = 4,5,6,7,8,9,11,13.
LHIP_DEV void esc_choice(int mx15, int* choice, int* choice2, int* lb1, int* lb2) {
    const int bl = 32 - __builtin_clz((unsigned)mx15);            // 1..13
    const int c24 = bl <= 4 ? 0 : bl <= 9 ? bl - 4 : bl <= 11 ? 6 : 7;
    int f16 = bl <= 4 ? bl - 1 : 4 + ((bl - 5) >> 1);
    if (f16 > 7) f16 = 7;
    int c16 = c24 - 8 + 8;                                         // choice2 - 8 - 16 == c24
    if (c16 < f16) c16 = f16;
    // c16 can reach 8 only if c24 == 8, which cannot happen (c24 <= 7)
    *choice2 = 24 + c24; *choice = 16 + c16;
    *lb1 = (int)((0xDA864321u >> (4 * c16)) & 15u);
    *lb2 = (int)((0xDB987654u >> (4 * c24)) & 15u);
}

// plan of a Huffman region whose largest value is m (Takehiro.js:336-346 choose_table / 479-497 ESC pair), as stored in
// QuantTabs::plan.  plan word: kind | t0 << 3 | t1 << 9 | t2 << 15 | lbA << 21 | lbB << 25
LHIP_DEV int plan_index(int m) { return m <= 15 ? m : (m <= IXMAX_VAL ? 15 + (32 - __builtin_clz((unsigned)(m - 15) | 1u)) : 29); }
LHIP_DEV void q_fill_plans(QuantTabs& Q, int tid, int nthr) {
    for (int e = tid; e < 30; e += nthr) {
        const int m = e <= 15 ? e : (e < 29 ? 15 + (1 << (e - 16)) : IXMAX_VAL + 1);
        // first candidate table for maxima 0..15 (huf_tbl_noESC, Takehiro.js:336-346), one nibble per value
        const int mc = m < 15 ? m : 15;
        const int tn = (int)((mc < 8 ? (0xAA775210u >> (4 * mc)) : (0xDDDDDDDDu >> (4 * (mc - 8)))) & 15u);
        const int kind = (m == 0) ? 0 : (m == 1) ? 1 : (m <= 3) ? 2 : (m <= 15) ? 4 : (m <= IXMAX_VAL) ? 5 : 6;
        int choice, choice2, lb1, lb2;
        esc_choice(m > 15 ? m - 15 : 1, &choice, &choice2, &lb1, &lb2);
        const int esc = (kind == 5);
        int xl = (tn == 1) ? 2 : (tn == 2) ? 3 : (tn == 5) ? 4 : (tn == 7) ? 6 : (tn == 10) ? 8 : 16;
        int oA = hl_off(tn), oB = hl_off(tn + 1), oC = hl_off(tn + 2 > 15 ? 15 : tn + 2);
        if (esc) { oA = HL_EHI; oB = HL_ELO; oC = HL_EHI; xl = 16; }
        if (kind == 0 || kind == 6) { oA = oB = oC = 0; xl = 0; }
        const int t0 = esc ? choice : tn, t1 = esc ? choice2 : tn + 1, t2 = tn + 2;
        Q.plan[e].d0 = (uint32_t)oA | ((uint32_t)oB << 16);
        Q.plan[e].d1 = (uint32_t)oC | ((uint32_t)xl << 16);
        Q.plan[e].pw = (uint32_t)kind | ((uint32_t)t0 << 3) | ((uint32_t)t1 << 9) | ((uint32_t)t2 << 15) |
                       ((uint32_t)(esc ? lb1 : 0) << 21) | ((uint32_t)(esc ? lb2 : 0) << 25);
    }
}

LHIP_DEV RegionPlan plan_region_(const QuantTabs& Q, int mx) {
    (void)Q;
    RegionPlan r; r.kind = 0; r.t1 = 0; r.xlen = 0; r.lb1 = r.lb2 = 0; r.choice = r.choice2 = 0; r.o0 = r.o1 = r.o2 = 0;
    if (mx == 0) return r;
    if (mx == 1) { r.kind = 1; r.t1 = 1; r.xlen = 2; r.o0 = HL_T1; return r; }
    if (mx <= 3) { r.kind = 2; r.t1 = (mx == 2) ? 2 : 5; r.xlen = (mx == 2) ? 3 : 4; return r; }
    if (mx <= 15) {
        r.kind = 4;
        if (mx <= 5) { r.t1 = 7; r.xlen = 6; r.o0 = HL_T7; r.o1 = HL_T8; r.o2 = HL_T9; }
        else if (mx <= 7) { r.t1 = 10; r.xlen = 8; r.o0 = HL_T10; r.o1 = HL_T11; r.o2 = HL_T12; }
        else { r.t1 = 13; r.xlen = 16; r.o0 = HL_T13; r.o1 = HL_T14; r.o2 = HL_T15; }
        return r;
    }
    if (mx > IXMAX_VAL) { r.kind = 6; return r; }
    r.kind = 5;
    esc_choice(mx - 15, &r.choice, &r.choice2, &r.lb1, &r.lb2);
    return r;
}

// contribution of one pair to the (up to three) length sums of its region
LHIP_DEV void pair_bits(const QuantTabs& Q, const RegionPlan& r, int x, int y, int& s0, int& s1, int& s2) {
    switch (r.kind) {
        case 1: s0 += Q.hlen[r.o0 + x * 2 + y]; break;
        case 2: { const int q = (r.t1 == 2) ? x * 3 + y : x * 4 + y, oa = (r.t1 == 2) ? HL_T2 : HL_T5, ob = (r.t1 == 2) ? HL_T3 : HL_T6;
                  s0 += ((int)Q.hlen[oa + q] << 16) | (int)Q.hlen[ob + q]; } break;      // packed t1 | t1 + 1 as count_bit_noESC_from2 does
        case 4: { const int q = x * r.xlen + y; s0 += Q.hlen[r.o0 + q]; s1 += Q.hlen[r.o1 + q]; s2 += Q.hlen[r.o2 + q]; } break;
        case 5: {
            int n = 0;
            if (x != 0) { if (x > 14) { x = 15; n++; } x *= 16; }
            if (y != 0) { if (y > 14) { y = 15; n++; } x += y; }
            s0 += (int)Q.hlen[HL_EHI + x] + n * r.lb1; s1 += (int)Q.hlen[HL_ELO + x] + n * r.lb2;
        } break;
        default: break;
    }
}

// final table + bits from the wave-reduced sums (same tie-breaking as count_bit_* in the reference)
LHIP_DEV int finish_region(const RegionPlan& r, int s0, int s1, int s2, int* bits) {
    switch (r.kind) {
        case 0: return 0;
        case 1: *bits += s0; return 1;
        case 2: { int t1 = r.t1, sum2 = s0 & 0xffff, sum = s0 >> 16; if (sum > sum2) { sum = sum2; t1++; } *bits += sum; return t1; }
        case 4: { int t = r.t1; if (s0 > s1) { s0 = s1; t++; } if (s0 > s2) { s0 = s2; t = r.t1 + 2; } *bits += s0; return t; }
        case 5: { int c = r.choice; if (s0 > s1) { s0 = s1; c = r.choice2; } *bits += s0; return c; }
        default: *bits = LARGE_BITS; return -1;
    }
}

// choose_table over pairs [a, b): cooperative; adds to *bits, returns table
LHIP_DEV int q_choose_table(const Tables& T, const int16_t* ix, int a, int b, int* bits, int lane, const QuantLds& L, const QuantTabs& Q) {
    int mx = 0;
    for (int p = a + 2 * lane; p < b; p += 2 * LHIP_NL) { const int x1 = ix[p], x2 = ix[p + 1]; if (mx < x1) mx = x1; if (mx < x2) mx = x2; }
    mx = wave_max(mx);
    const RegionPlan r = plan_region_(Q, mx);
    int s0 = 0, s1 = 0, s2 = 0;
    if (r.kind >= 1 && r.kind <= 5)
        for (int p = a + 2 * lane; p < b; p += 2 * LHIP_NL) pair_bits(Q, r, ix[p], ix[p + 1], s0, s1, s2);
    s0 = wave_sum(s0);
    if (r.kind >= 4) s1 = wave_sum(s1);
    if (r.kind == 4) s2 = wave_sum(s2);
    return finish_region(r, s0, s1, s2, bits);
}

// Conditionally assigned GrInfo fields (Takehiro.js:566-612: table_select[r] only for a non-empty region, the region
// counts only for long blocks with big_values > 0).  Their values after a bin search depend on the gains it visited, so
// they are part of what the seed-chain validation must reproduce.  mask bits: 1/2/4 table_select[0/1/2], 8 region counts.
LHIP_DEV int pack_cond_fields(const GI& g, int mask) {
    return mask | ((g.table_select[0] + 1) << 4) | ((g.table_select[1] + 1) << 10) | ((g.table_select[2] + 1) << 16) |
           (g.region0_count << 22) | (g.region1_count << 26);
}
LHIP_DEV int apply_cond_fields(int state, int asg) {
    if (asg & 1) state = (state & ~(63 << 4)) | (asg & (63 << 4));
    if (asg & 2) state = (state & ~(63 << 10)) | (asg & (63 << 10));
    if (asg & 4) state = (state & ~(63 << 16)) | (asg & (63 << 16));
    if (asg & 8) state = (state & ~(0x3ff << 22)) | (asg & (0x3ff << 22));
    return state & ~15;
}   // scalar part of CalcNoiseData (arrays are L.pn_*)

// noquant_count_bits (Takehiro.js:521-628); updates g, returns bits.  pn_sfb_count1 as in/out.
// *asg_mask: which conditionally assigned fields this call wrote (see pack_cond_fields).
template <int NR>
LHIP_DEV int q_noquant_count_bits(const Tables& T, GI& g, const int16_t* ix, int (&vx)[NR], int (&vy)[NR], int use_prev, int* pn_sfb_count1, int* asg_mask, int lane, QuantLds& L, const QuantTabs& Q) {
    *asg_mask = 0;
    lane = fresh_lane(lane);
    unsigned long long tm_ = PH_NOW(); (void)tm_;
    int i = ((g.max_nonzero_coeff + 2) >> 1) << 1;
    if (i > 576) i = 576;
    if (use_prev) *pn_sfb_count1 = 0;
    // the lane's pairs arrive in registers from q_quantize; pairs at or above the max_nonzero_coeff bound are zero already
    // (xr, hence xrpow, is zero from max_nonzero_coeff on -- see q_quantize)
    // count1 boundary (highest pair with a non-zero value) and the end of the big-values region (the quad scan of
    // Takehiro.js:540-560 stops at the first quad, counted from the top, that holds a value > 1).
    int firstbig;
#if LHIP_NL == 1
    {
        int top = 0;
        for (int j = 0; j < NR; j++) if ((vx[j] | vy[j]) != 0) top = 2 * (lane + LHIP_NL * j) + 2;
        i = top;
        const int nq = i >> 2;
        firstbig = nq;
        for (int k = 0; k < nq; k++) {
            const int e = i - 4 * k;
            if (((ix[e - 1] | ix[e - 2] | ix[e - 3] | ix[e - 4]) & 0x7fff) > 1) { firstbig = k; break; }
        }
    }
#else
    {
        // Pair lane + 64 j is bit `lane` of ballot j, so the two boundaries are "highest set bit" questions
        // answered on the scalar unit: no reduction chain, no second pass over the spectrum.
        int tp = -1, bp = -1;                    // highest non-zero pair / highest pair with a value > 1
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const uint64_t nz = wave_ballot((vx[j] | vy[j]) != 0), bg = wave_ballot((vx[j] | vy[j]) > 1);
            if (nz) tp = 64 * j + 63 - (int)__builtin_clzll(nz);
            if (bg) bp = 64 * j + 63 - (int)__builtin_clzll(bg);
        }
        i = 2 * tp + 2;
        const int P = tp + 1, nq = i >> 2;
        firstbig = (P - 1 - bp) >> 1;
        if (firstbig > nq) firstbig = nq;
    }
#endif
    g.count1 = i;
    PH_MARK(L, PH_C_LOAD, tm_);
    int a12 = 0;
    for (int k = lane; k < firstbig; k += LHIP_NL) {
        const int e = i - 4 * k;                 // even: the two pairs of the quad as two aligned 32-bit words; values are 0/1 here
        const uint32_t w0 = *(const uint32_t*)(ix + e - 4), w1 = *(const uint32_t*)(ix + e - 2);
        const int p = (int)(((w0 & 1u) << 3) | ((w0 >> 16) << 2) | ((w1 & 1u) << 1) | (w1 >> 16));
        a12 += Q.t32l[p] + (Q.t33l[p] << 16);
    }
    // the quads' two candidate lengths (packed) are reduced together with the region sums below: one reduction chain less per call
    i -= 4 * firstbig;
    g.big_values = i;
    int a1, a2, bits;
#define COUNT1_FINISH(A12) do { const int c1_ = (A12) & 0xffff, c2_ = (int)((unsigned)(A12) >> 16); bits = c1_; g.count1table_select = 0; \
                                if (c1_ > c2_) { bits = c2_; g.count1table_select = 1; } g.count1bits = bits; } while (0)
    PH_MARK(L, PH_C_QUADS, tm_);
    if (i == 0) { const int t = wave_sum(a12); COUNT1_FINISH(t); return bits; }
    int use2 = 0, cnt1_norm = 0;
    if (g.block_type == SHORT_TYPE) {
        a1 = 3 * Q.sfb_s[3];
        if (a1 > g.big_values) a1 = g.big_values;
        a2 = g.big_values;
    } else if (g.block_type == NORM_TYPE) {
        const uint32_t bt = Q.bvtab[i >> 1];               // one look-up: region counts, region borders, sfb_count1
        g.region0_count = (int)((bt >> 20) & 15u); g.region1_count = (int)((bt >> 24) & 7u);
        a1 = (int)(bt & 1023u); a2 = (int)((bt >> 10) & 1023u);
        cnt1_norm = (int)(bt >> 27);
        if (a2 < i) use2 = 1;
    } else {
        g.region0_count = 7;
        g.region1_count = SBMAX_l - 1 - 7 - 1;
        a1 = Q.sfb_l[7 + 1];
        a2 = i;
        if (a1 > a2) a1 = a2;
    }
    if (a1 > i) a1 = i;
    if (a2 > i) a2 = i;
    *asg_mask = (g.block_type != SHORT_TYPE ? 8 : 0) | (use2 ? 4 : 0) | (0 < a1 ? 1 : 0) | (a1 < a2 ? 2 : 0);
    // region maxima: region of a pair = number of boundaries at or below it
    int m0 = 0, m1 = 0, m2 = 0;
    int rj[NR];                                                    // region of the lane's pairs (3: at or beyond big_values), kept for the length sums
#pragma unroll
    for (int j = 0; j < NR; j++) {
        rj[j] = 3;
        if (2 * LHIP_NL * j >= i) continue;                         // wave-uniform: every pair of this round of lanes lies beyond big_values
        const int p = 2 * (lane + LHIP_NL * j);
        const int r = (p >= a1) + (p >= a2) + (p >= i);             // a1 <= a2 <= i
        const int m = vx[j] > vy[j] ? vx[j] : vy[j];
        const int mr0 = (r == 0) ? m : 0, mr1 = (r == 1) ? m : 0, mr2 = (r == 2) ? m : 0;
        m0 = m0 > mr0 ? m0 : mr0; m1 = m1 > mr1 ? m1 : mr1; m2 = m2 > mr2 ? m2 : mr2;
        rj[j] = r;
    }
    { int mm[3] = {m0, m1, m2}; wave_max_n(mm); m0 = mm[0]; m1 = mm[1]; m2 = mm[2]; }
    // Data-driven length sums: every region publishes the pool offsets of its (up to three) candidate tables and
    // its row stride; a pair then costs three byte gathers whatever its region's table group is, and all regions
    // are handled in ONE pass.  Region r is planned (and later finished) by lane r, branch-free: there is no
    // scalar per-region control flow left.
    struct LanePlan { int kind, t0, t1, t2, lbA, lbB; };
    // one plan per lane on the device (a scalar struct: an array indexed by r / 64 would live in scratch memory and cost a
    // memory round trip per access); the one-lane host simulation holds all three
#if LHIP_NL == 1
    LanePlan lp[3]; int pv[3];
#define LP_(r) lp[r]
#define PV_(r) pv[r]
#else
    LanePlan lp1; int pv1 = 0;
    lp1.kind = 0; lp1.t0 = lp1.t1 = lp1.t2 = lp1.lbA = lp1.lbB = 0;
#define LP_(r) lp1
#define PV_(r) pv1
#endif
    LHIP_LANE_ONCE(r, 0, 3) {
        const int m = (r == 0) ? m0 : (r == 1) ? m1 : (r == 2) ? m2 : 0;
        const QuantTabs::PlanEnt pe = Q.plan[plan_index(m)];          // the whole plan is a function of the maximum: one look-up
        L.rdesc[r][0] = pe.d0;
        L.rdesc[r][1] = pe.d1;
        LanePlan& q = LP_(r);
        q.kind = (int)(pe.pw & 7u); q.t0 = (int)((pe.pw >> 3) & 63u); q.t1 = (int)((pe.pw >> 9) & 63u); q.t2 = (int)((pe.pw >> 15) & 63u);
        q.lbA = (int)((pe.pw >> 21) & 15u); q.lbB = (int)((pe.pw >> 25) & 15u);
    }
    wave_sync();
    PH_MARK(L, PH_C_MAX, tm_);
    // field width: a lane owns at most NPL pairs (5 x 21 bits < 2^10); the one-lane host simulation owns all 288
#if LHIP_NL == 1
    typedef uint64_t acc_t; enum { FB = 21 };
#else
    typedef uint32_t acc_t; enum { FB = 10 };
#endif
    const acc_t FM = ((acc_t)1 << FB) - 1;
    acc_t accA = 0, accB = 0, accC = 0, accN = 0;
    const int any_esc = (m0 > 15) | (m1 > 15) | (m2 > 15);          // escaped values only cost extra bits in ESC regions
#if LHIP_NL == 1
#pragma unroll
    for (int j = 0; j < NR; j++) {
        const int p = 2 * (lane + LHIP_NL * j);
        if (p < i) {
            const int r = (p >= a1) + (p >= a2);
            const uint64_t d = *(const uint64_t*)L.rdesc[r];
            const uint32_t d0 = (uint32_t)d, d1 = (uint32_t)(d >> 32);
            const int x = vx[j], y = vy[j];
            const int idx = (x < 15 ? x : 15) * (int)(d1 >> 16) + (y < 15 ? y : 15);
            const int sh = FB * r;
            accA += (acc_t)Q.hlen[(d0 & 0xffffu) + idx] << sh;
            accB += (acc_t)Q.hlen[(d0 >> 16) + idx] << sh;
            accC += (acc_t)Q.hlen[(d1 & 0xffffu) + idx] << sh;
            if (any_esc) accN += (acc_t)((x > 14) + (y > 14)) << sh;
        }
    }
    (void)rj;
#else
    // a pair at a time (descriptor of its region, three byte gathers, three multiply-adds): measured 1 % faster per launch than the
    // same work in stages (all descriptors, all gathers, all sums), which keeps fifteen more values live
    if (any_esc) {
#pragma unroll
        for (int j = 0; j < NR; j++) {
            if (rj[j] < 3) {
                const int r = rj[j];
                const uint64_t d = *(const uint64_t*)L.rdesc[r];
                const uint32_t d0 = (uint32_t)d, d1 = (uint32_t)(d >> 32);
                const int x = vx[j], y = vy[j];
                const int idx = (x < 15 ? x : 15) * (int)(d1 >> 16) + (y < 15 ? y : 15);
                const unsigned mult = 1u << (FB * r);                   // field of region r; 24-bit multiply-add accumulates in one instruction
                accA = mul24((unsigned)Q.hlen[(d0 & 0xffffu) + idx], mult) + accA;
                accB = mul24((unsigned)Q.hlen[(d0 >> 16) + idx], mult) + accB;
                accC = mul24((unsigned)Q.hlen[(d1 & 0xffffu) + idx], mult) + accC;
                accN = mul24((unsigned)((x > 14) + (y > 14)), mult) + accN;
            }
        }
    } else {
        // no region holds a value above 15 (three calls in four at stereo 128 kbps): nothing to clamp, no escapes to count
#pragma unroll
        for (int j = 0; j < NR; j++) {
            if (rj[j] < 3) {
                const int r = rj[j];
                const uint64_t d = *(const uint64_t*)L.rdesc[r];
                const uint32_t d0 = (uint32_t)d, d1 = (uint32_t)(d >> 32);
                const int idx = vx[j] * (int)(d1 >> 16) + vy[j];
                const unsigned mult = 1u << (FB * r);
                accA = mul24((unsigned)Q.hlen[(d0 & 0xffffu) + idx], mult) + accA;
                accB = mul24((unsigned)Q.hlen[(d0 >> 16) + idx], mult) + accB;
                accC = mul24((unsigned)Q.hlen[(d1 & 0xffffu) + idx], mult) + accC;
            }
        }
    }
#endif
    // unpack to (A|B<<16), (C|N<<16) per region: wave totals stay below 2^16 (<= 288 pairs x 21 bits = 6048)
#define FLD(A, R) ((uint32_t)(((A) >> (FB * (R))) & FM))
    int qq[7] = {(int)(FLD(accA, 0) | (FLD(accB, 0) << 16)), (int)(FLD(accC, 0) | (FLD(accN, 0) << 16)), (int)(FLD(accA, 1) | (FLD(accB, 1) << 16)),
                 (int)(FLD(accC, 1) | (FLD(accN, 1) << 16)), (int)(FLD(accA, 2) | (FLD(accB, 2) << 16)), (int)(FLD(accC, 2) | (FLD(accN, 2) << 16)), a12};
    wave_sum_n(qq);                       // six packed region sums and the count1 quads' pair, reduced side by side
    const int q0 = qq[0], q1 = qq[1], q2 = qq[2], q3 = qq[3], q4 = qq[4], q5 = qq[5];
    COUNT1_FINISH(qq[6]);
#undef COUNT1_FINISH
#undef FLD
    PH_MARK(L, PH_C_SUMS, tm_);
    // finish (Takehiro.js count_bit_noESC / _from2 / _from3 / count_bit_ESC tie-breaking): lane r picks the cheapest
    // admissible candidate of region r; result packed as table | overflow << 6 | bits << 8
    LHIP_LANE_ONCE(r, 0, 3) {
        const LanePlan& q = LP_(r);
        const int qa = (r == 0) ? q0 : (r == 1) ? q2 : q4, qc = (r == 0) ? q1 : (r == 1) ? q3 : q5;
        const int n = (int)((unsigned)qc >> 16);
        const int c0 = (qa & 0xffff) + n * q.lbA, c1 = (int)((unsigned)qa >> 16) + n * q.lbB, c2 = qc & 0xffff;
        int b = c0, t = q.t0;
        if ((q.kind == 2 || q.kind == 4 || q.kind == 5) && b > c1) { b = c1; t = q.t1; }
        if (q.kind == 4 && b > c2) { b = c2; t = q.t2; }
        if (q.kind == 0) { b = 0; t = 0; }
        if (q.kind == 6) { b = 0; t = 63; }              // table_select := -1 (never emitted: overflow cannot pass count_bits)
        PV_(r) = t | ((q.kind == 6) << 6) | (b << 8);
    }
#if LHIP_NL == 1
    const int pv0 = pv[0], pv1_ = pv[1], pv2 = pv[2];
#else
    const int pv0 = wave_bcast(pv1, 0), pv1_ = wave_bcast(pv1, 1), pv2 = wave_bcast(pv1, 2);
#endif
    // the reference evaluates region 2 first (NORM only), then 0, then 1; an overflowing region *sets* bits
#define APPLY(PV, SLOT) do { const int t_ = (PV) & 63; if ((PV) & 64) bits = LARGE_BITS; else bits += (PV) >> 8; g.table_select[SLOT] = (t_ == 63) ? -1 : t_; } while (0)
    if (use2) APPLY(pv2, 2);
    if (0 < a1) APPLY(pv0, 0);
    if (a1 < a2) APPLY(pv1_, 1);
#undef APPLY
#undef LP_
#undef PV_
    // first band whose start is >= big_values (PrevNoise.sfb_count1): one table look-up instead of a walk
    if (use_prev && g.block_type == NORM_TYPE) *pn_sfb_count1 = cnt1_norm;       // big_values > 0 here (the table's entry)
    PH_MARK(L, PH_C_FIN, tm_);
    return bits;
}

struct PrevNoise { int gain, sfb_count1; };

// count_bits (Takehiro.js:630-660)
// `use_pn` selects the prev_noise cache; pn is passed by reference with a flag (never as a nullable pointer to a
// local: a select between private addresses is a per-lane value for the compiler and makes the control flow divergent)
template <int NR>
LHIP_DEV int q_count_bits(const Tables& T, GI& g, const int32_t* scalefac, int16_t* ix, int use_pn, PrevNoise& pn, int* asg, int lane, QuantLds& L, const QuantTabs& Q) {
    *asg = 0;
    {   // Takehiro.js:635-638: `xrpow_max > IXMAX_VAL / IPOW20(gain)`.  The division is only needed when the product is
        // within rounding of the bound: fl(x * ip) <= 8206 (1 - 2^-50) implies x < fl(8206 / ip)
        const double ip = ipow20(Q, g.global_gain);
        if (g.xrpow_max * ip > (double)IXMAX_VAL * (1.0 - 0x1p-50)) {
            const double w = (double)IXMAX_VAL / ip;
            if (g.xrpow_max > w) return LARGE_BITS;
        }
    }
    int vx[NR], vy[NR];
    { PH_BEGIN(); q_quantize<NR>(T, g, scalefac, ix, use_pn, use_pn ? pn.gain : 0, use_pn ? pn.sfb_count1 : 0, vx, vy, lane, L, Q); PH_END(L, PH_QUANTIZE); }
    int cnt1 = pn.sfb_count1;
    PH_BEGIN();
    int amask = 0;
    const int r = q_noquant_count_bits<NR>(T, g, ix, vx, vy, use_pn, &cnt1, &amask, lane, L, Q);
    *asg = pack_cond_fields(g, amask);
    if (use_pn) pn.sfb_count1 = cnt1;
    PH_END(L, PH_COUNT);
    return r;
}
// one evaluation with the round count the granule-channel needs, chosen by one scalar branch: each form keeps its own interleaved schedule,
// and the short one holds fewer live registers.  SKIP == 0 (the latency kernels): the full form only, not one instruction more in their loop
template <int SKIP>
LHIP_DEV int q_count_bits_rounds(const Tables& T, GI& g, const int32_t* scalefac, int16_t* ix, int use_pn, PrevNoise& pn, int* asg, int lane, QuantLds& L, const QuantTabs& Q) {
    if constexpr (SKIP != 0) {
        if (g.tail0) { LHIP_ROUND_COUNT(head); return q_count_bits<NPL_HEAD>(T, g, scalefac, ix, use_pn, pn, asg, lane, L, Q); }
    }
    LHIP_ROUND_COUNT(full);
    return q_count_bits<NPL>(T, g, scalefac, ix, use_pn, pn, asg, lane, L, Q);
}
}  // namespace lhip
