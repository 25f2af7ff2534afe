// k_quant_tabs.h -- what every stage of the search holds on to: the granule state GI (wave-uniform scalars), the read-only table image staged in
// LDS (QuantTabs, q_load_tabs / q_copy_tabs), the per-wave LDS record (QuantLds) and the small look-up helpers.
#pragma once
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
#include "k_quant_prof.h"
namespace lhip {
struct GI {   // wave-uniform scalar part of the reference's GrInfo
    double xrpow_max;
    int part2_3_length, big_values, count1, global_gain, scalefac_compress, block_type;
    int table_select[3], subblock_gain[4];
    int region0_count, region1_count, preflag, scalefac_scale, count1table_select;
    int part2_length, sfb_lmax, sfb_smin, psy_lmax, sfbmax, psymax, sfbdivide;
    int count1bits, max_nonzero_coeff;
    int firstcut;               // first band reaching past max_nonzero_coeff (64: none): fixed once max_nonzero_coeff is (q_set_firstcut)
    int tail0;                  // every line of 512..575 is +-0 (q_calc_xmin): the pairs 256..287 quantize to zero and their round is not issued (NPL_HEAD)
};

struct NoiseRes { double max_noise; int over_count, over_SSD, bits; };

// Re-asserts that the granule state is wave-uniform (it is by construction: every lane executes the same
// decisions).  The compiler's divergence analysis loses that fact at joins of lane-guarded code, and once one
// loop-carried scalar counts as divergent every decision of the loop turns into exec-masked vector code.
LHIP_DEV void uni_gi(GI& g) {
    g.xrpow_max = unid(g.xrpow_max);
    g.part2_3_length = uni(g.part2_3_length); g.big_values = uni(g.big_values); g.count1 = uni(g.count1); g.global_gain = uni(g.global_gain);
    g.scalefac_compress = uni(g.scalefac_compress); g.block_type = uni(g.block_type);
    for (int i = 0; i < 3; i++) g.table_select[i] = uni(g.table_select[i]);
    for (int i = 0; i < 4; i++) g.subblock_gain[i] = uni(g.subblock_gain[i]);
    g.region0_count = uni(g.region0_count); g.region1_count = uni(g.region1_count); g.preflag = uni(g.preflag); g.scalefac_scale = uni(g.scalefac_scale);
    g.count1table_select = uni(g.count1table_select); g.part2_length = uni(g.part2_length); g.sfb_lmax = uni(g.sfb_lmax); g.sfb_smin = uni(g.sfb_smin);
    g.psy_lmax = uni(g.psy_lmax); g.sfbmax = uni(g.sfbmax); g.psymax = uni(g.psymax); g.sfbdivide = uni(g.sfbdivide);
    g.count1bits = uni(g.count1bits); g.max_nonzero_coeff = uni(g.max_nonzero_coeff); g.firstcut = uni(g.firstcut); g.tail0 = uni(g.tail0);
}

// Read-only tables staged once per workgroup in LDS (shared by the waves of the block): everything the
// inner loops gather from -- avoids ~1 us HBM/L2 round trips inside serially dependent code.
enum { QT_N = 256 };
// Layout of the Huffman code-length pool (bytes): the table sizes are fixed by ISO 11172-3, so the offsets are
// compile-time constants (tables 4 and 14 do not exist in the standard; the reference keeps a 256-entry row 14).
enum { HL_T1 = 0, HL_T2 = 4, HL_T3 = 13, HL_T5 = 22, HL_T6 = 38, HL_T7 = 54, HL_T8 = 90, HL_T9 = 126, HL_T10 = 162, HL_T11 = 226,
       HL_T12 = 290, HL_T13 = 354, HL_T14 = 610, HL_T15 = 866, HL_EHI = 1122, HL_ELO = 1378, HL_END = 1634 };
LHIP_DEV int hl_off(int t) {
    switch (t) {
        case 1: return HL_T1; case 2: return HL_T2; case 3: return HL_T3; case 5: return HL_T5; case 6: return HL_T6;
        case 7: return HL_T7; case 8: return HL_T8; case 9: return HL_T9; case 10: return HL_T10; case 11: return HL_T11;
        case 12: return HL_T12; case 13: return HL_T13; case 14: return HL_T14; case 15: return HL_T15; default: return 0;
    }
}
struct alignas(16) QuantTabs {
    float pow43[QT_N], adj43[QT_N];
    float ipow20[Q_MAX], pow20[Q_MAX + Q_MAX2 + 1];
    int32_t sfb_l[SBMAX_l + 1], sfb_s[SBMAX_s + 1], pretab[SBMAX_l];
    uint16_t hoff[16];
    uint8_t hlen[HL_END];        // code-length pool: tables 1-3, 5-15, then the two ESC length tables (layout: hl_off)
    uint8_t t32l[16], t33l[16];
    uint8_t l2s_long[576], l2s_short[576];
    uint32_t bvtab[289];         // count_bits, NORM blocks, by big_values / 2: region borders, region counts, sfb_count1 (Tables::bvtab)
    uint8_t huf_tbl_noESC[16], ht_xlen[34];
    uint16_t ht_linmax[34];
    // Huffman region plans by region maximum (count_bits): entries 0..15 = the maximum itself, 16..28 = bit length 1..13
    // of (maximum - 15), 29 = beyond IXMAX_VAL.  d0/d1 = pool offsets of the candidate length tables | row stride (what
    // the pairs gather with), pw = kind | candidate table numbers | linbits of the two ESC candidates (plan_word)
    struct PlanEnt { uint32_t d0, d1, pw; } plan[30];
    // scale_bitcount candidates (Takehiro.js:980-1030): row k = slen1_n | slen2_n << 8 | scale_long << 16 | scale_short << 24
    uint32_t sbc[16];
    // calc_noise's systolic fold (lane l owns the lines n l .. n l + n - 1, n = noise_nln: 7 or 9, Tables::noise_nln): bit k = line n l + k is the
    // first of its scalefactor band, bit 16 + k = it is the last one; bits 12 + k and 28 + k: the same for the short window's lines 3 l + k, k < 3;
    // [0] long blocks, [1] short blocks.  wpre: widest band among bands 0 .. b (long / short).
    uint32_t fold_marks[2][64];
    int32_t noise_nln;
    uint16_t wpre_long[24], wpre_short[40];
    // analog silence (Quantize.js:147-202): pseudo-band borders above sfb21 / sfb12, their ATH values ([0..5] long, [6..11] short) and the
    // two band factors they are scaled with
    int16_t psfb21[PSFB21 + 1], psfb12[PSFB12 + 1];
    float ath_psfb[PSFB21 + PSFB12], fact_psfb[2];
};

LHIP_DEV void q_fill_plans(QuantTabs& Q, int tid, int nthr);

LHIP_DEV void q_load_tabs(const Tables& T, QuantTabs& Q, int tid, int nthr) {
    q_fill_plans(Q, tid, nthr);
    for (int i = tid; i < QT_N; i += nthr) { Q.pow43[i] = T.pow43[i]; Q.adj43[i] = T.adj43[i]; }
    for (int i = tid; i < Q_MAX; i += nthr) Q.ipow20[i] = T.ipow20[i];
    for (int i = tid; i < Q_MAX + Q_MAX2 + 1; i += nthr) Q.pow20[i] = T.pow20[i];
    for (int i = tid; i < 16; i += nthr) { Q.t32l[i] = (uint8_t)T.t32l[i]; Q.t33l[i] = (uint8_t)T.t33l[i]; }
    for (int i = tid; i < SBMAX_l + 1; i += nthr) Q.sfb_l[i] = T.sfb_l[i];
    for (int i = tid; i < SBMAX_s + 1; i += nthr) Q.sfb_s[i] = T.sfb_s[i];
    for (int i = tid; i < SBMAX_l; i += nthr) Q.pretab[i] = T.pretab[i];
    for (int i = tid; i < 16; i += nthr)
        Q.sbc[i] = (uint32_t)T.slen1_n[i] | ((uint32_t)T.slen2_n[i] << 8) | ((uint32_t)T.scale_long[i] << 16) | ((uint32_t)T.scale_short[i] << 24);
    for (int i = tid; i < 289; i += nthr) Q.bvtab[i] = (uint32_t)T.bvtab[i];
    for (int i = tid; i < 15; i += nthr) Q.huf_tbl_noESC[i] = (uint8_t)T.huf_tbl_noESC[i];
    for (int i = tid; i < 34; i += nthr) { Q.ht_xlen[i] = (uint8_t)T.ht_xlen[i]; Q.ht_linmax[i] = (uint16_t)T.ht_linmax[i]; }
    // Huffman code-length pool
    if (tid == 0) { Q.hoff[0] = 0; Q.hoff[4] = 0; }
    for (int t = 1; t < 16; t++) {
        if (t == 4) continue;
        const int xl = T.ht_xlen[t];
        const int n = (t == 14) ? 256 : xl * xl, off = hl_off(t);
        if (tid == 0) Q.hoff[t] = (uint16_t)off;
        for (int i = tid; i < n; i += nthr) Q.hlen[off + i] = (uint8_t)T.ht_hlen[T.ht_off[t] + i];
    }
    for (int i = tid; i < 256; i += nthr) { Q.hlen[HL_EHI + i] = (uint8_t)(T.largetbl[i] >> 16); Q.hlen[HL_ELO + i] = (uint8_t)(T.largetbl[i] & 0xffff); }
    for (int d = tid; d < 576; d += nthr) {
        int sfb = 0;
        while (T.sfb_l[sfb + 1] <= d) sfb++;
        Q.l2s_long[d] = (uint8_t)sfb;
        sfb = 0;
        while (3 * T.sfb_s[sfb + 1] <= d) sfb++;
        const int st = T.sfb_s[sfb], w = T.sfb_s[sfb + 1] - st;
        const int r = d - 3 * st, win = r / w, l = st + (r - win * w);
        Q.l2s_short[d] = (uint8_t)(3 * sfb + win);
        (void)l;
    }
    for (int e = tid; e < PSFB21 + 1; e += nthr) Q.psfb21[e] = (int16_t)T.psfb21[e];
    for (int e = tid; e < PSFB12 + 1; e += nthr) Q.psfb12[e] = (int16_t)T.psfb12[e];
    for (int e = tid; e < PSFB21 + PSFB12; e += nthr) Q.ath_psfb[e] = e < PSFB21 ? T.ATH_psfb21[e] : T.ATH_psfb12[e - PSFB21];
    if (tid == 0) { Q.fact_psfb[0] = T.longfact[21]; Q.fact_psfb[1] = T.shortfact[12]; }
    for (int e = tid; e < 2 * 64; e += nthr) Q.fold_marks[e >> 6][e & 63] = (uint32_t)T.fold_marks[e];
    if (tid == 0) Q.noise_nln = T.noise_nln;
    for (int e = tid; e < 24; e += nthr) Q.wpre_long[e] = (uint16_t)T.wpre[e];
    for (int e = tid; e < 40; e += nthr) Q.wpre_short[e] = (uint16_t)T.wpre[24 + e];
}

// The tables do not change after lhip_create: they are gathered ONCE per configuration into an image in HBM (g_build_qtabs) and a workgroup
// copies that image flat -- 16 bytes per thread and step -- instead of repeating q_load_tabs' gathers from fifteen source tables, which cost a
// one-frame launch 19 us of dependent global loads before its first stage (profiles/r05_pass1_frame_prof_*.txt).
LHIP_DEV void q_copy_tabs(const Tables& T, QuantTabs& Q, int tid, int nthr) {
    static_assert(sizeof(QuantTabs) % 16 == 0, "QuantTabs is copied in 16-byte pieces");
    struct alignas(16) V4 { uint32_t a, b, c, d; };
    const V4* src = (const V4*)T.qtabs_img;
    V4* dst = (V4*)&Q;
    for (int i = tid; i < (int)(sizeof(QuantTabs) / 16); i += nthr) dst[i] = src[i];
}

struct QuantLds {
    float xr[576];
    union {                      // xrpow is dead once the outer loop has finished; the Huffman-split scratch reuses it
        float xrpow[576];
        struct { int32_t bstat[16][SBMAX_l + 2]; int16_t cand[21][16]; } hd;   // cand: bits clipped to 0x7fff (LARGE_BITS marker)
    };
    int16_t ixw[576];            // l3_enc of the working copy (cod_info_w)
    int32_t sfw[SFBMAX + 1], sfb[SFBMAX + 1];     // scalefac working / kept
    int16_t width[SFBMAX + 1], window[SFBMAX + 1], start[SFBMAX + 2];
    float xmin[SFBMAX + 1], distort[SFBMAX + 1];
    double rxmin[SFBMAX + 1];                    // 1 / xmin, correctly rounded (0: xmin outside the range div_by_f32 is proven for): calc_noise divides by xmin in every call
    int32_t pn_step[SFBMAX + 1];
    float pn_dist[SFBMAX + 1];                   // the cache of the reference's Float32 noise, as what every later call derives from it: (float)(noise / xmin)
    // the cache of the reference's Float32 noise_log, without the logarithm: pn_x = the band's noise / xmin (f64) as last evaluated,
    // pn_cls = noise_class of the Float32 copy of its logarithm (lhip_math.h); the logarithm itself is only formed when max_noise is read
    union {                      // pn_x is dead once the outer loop has finished; the Huffman split's range-maximum tables reuse it
        double pn_x[SFBMAX + 1];
        int16_t hmax[5][24];     // hmax[t][b] = largest quantized value in the bands b .. b + 2^t - 1 (q_band_max_tables)
    };
    int16_t pn_cls[SFBMAX + 1];
    int32_t qmode[SFBMAX + 1];
    float bstep[SFBMAX + 1];                     // calc_noise: POW20 of the band's step (what the per-line pass reads)
    int8_t sf_gr0[2][SFBMAX + 1];                 // final gr0 scalefactors per channel (for scfsi): -2..15
    union {                      // calc_noise band sums live only inside the outer loop, the split tables only after it
        struct { int32_t r01_bits[24], r01_div[24], r0_tbl[24], r1_tbl[24], r2_bits[24], r2_tbl[24]; };
        double nsum[SFBMAX + 1];
        struct { int32_t bs_tab[BS_TAB_MAX], bs_asg[BS_TAB_MAX]; } memo;   // bin-search memo, flushed to the side record before the first calc_noise
    };
    alignas(8) uint32_t rdesc[4][2];   // per Huffman region: offsets of its candidate length tables | row stride
    int32_t gkeep[24];                 // the mutable scalars of the kept quantization (cod_info) while the outer loop runs on cod_info_w
    double ath_pseudo[PSFB21 + PSFB12];   // this frame's analog-silence thresholds (q_ath_pseudo): [0..5] long blocks, [6..11] short blocks
#ifdef LHIP_PHASE_PROF
    unsigned int prof[64];           // per-frame cycle sums fit 32 bits
#endif
};

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
LHIP_DEV double ipow20(const QuantTabs& Q, int x) { return (double)Q.ipow20[x]; }
LHIP_DEV double pow20(const QuantTabs& Q, int x) { return (double)Q.pow20[x + Q_MAX2]; }
LHIP_DEV double pow43v(const Tables& T, const QuantTabs& Q, int i) {
    float v = Q.pow43[i < QT_N ? i : QT_N - 1];
    if (i >= QT_N) v = T.pow43[i];          // rare: large quantized values
    return (double)v;
}
LHIP_DEV double adj43v(const Tables& T, const QuantTabs& Q, int i) {
    float v = Q.adj43[i < QT_N ? i : QT_N - 1];
    if (i >= QT_N) v = T.adj43[i];
    return (double)v;
}
LHIP_DEV const uint8_t* line2sfb(const QuantTabs& Q, int block_type) { return block_type == SHORT_TYPE ? Q.l2s_short : Q.l2s_long; }
LHIP_DEV const uint8_t* hlen_of(const QuantTabs& Q, int t) { return Q.hlen + Q.hoff[t]; }

// QuantizePVT.js:541-561
LHIP_DEV double athAdjust(const Tables& T, const PowBase& pb10, double a, double x, double athFloor) {
    const double o = 90.30873362, p = 94.82444863;
    double u = v8_log10(x) * 10.0;
    const double v = a * a;
    double w = 0.0;
    u -= athFloor;
    if (v > 1E-20) w = 1. + v8_log10(v) * const_here(10.0 / o);
    if (w < 0) w = 0.;
    u *= w;
    u += athFloor + const_here(o) - const_here(p);
    return v8_pow_base(pb10, 0.1 * u);
}

LHIP_DEV int sbgain(const GI& g, int w) {   // subblock_gain[w] without a dynamically indexed register array
    return w == 0 ? g.subblock_gain[0] : w == 1 ? g.subblock_gain[1] : w == 2 ? g.subblock_gain[2] : g.subblock_gain[3];
}

// the band's sub-block gain: only short blocks have one (every other block type keeps its bands in "window 3", whose gain stays 0 --
// nothing ever increments subblock_gain[3]), so long blocks neither fetch the window nor select among the gains
LHIP_DEV int band_sbgain(const GI& g, const int16_t* window, int sfb) { return g.block_type == SHORT_TYPE ? sbgain(g, window[sfb]) : 0; }
LHIP_DEV int sf_step(const QuantTabs& Q, const GI& g, const int32_t* scalefac, const int16_t* window, int sfb) {
    return g.global_gain - ((scalefac[sfb] + (g.preflag != 0 ? Q.pretab[sfb] : 0)) << (g.scalefac_scale + 1))
           - band_sbgain(g, window, sfb) * 8;
}
}  // namespace lhip
