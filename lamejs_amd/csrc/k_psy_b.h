// k_psy_b.h -- kb_psyB, the thresholds that need the scans' results (PsyModel.js:1226-1342, 692-767, 525-543), with its LDS record and the mask_add tables and index
// (PsyModel.js:403-473).
#pragma once
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// kb_psyB: one wave per psy call (all channels).
// ---------------------------------------------------------------------------------------------
// NCH = psy channels the instantiation can hold: 2 (mono / stereo), or 4 for joint stereo (L, R, mid, side) -- a separate kernel so that
// the usual configurations keep their 3.5 KB of LDS per wave
struct PsyBTabs { double mt1[25], mt2[10], mt3[14], mtab[9]; };     // mask_add tables: looked up inside a serially dependent chain
// The long-block spreading is a chain per partition (lane) whose every step needs three operands of ANOTHER partition k -- its energy times
// its tonality factor, its ATH share -- and one entry of the lane's own spreading row.  Fetched from global memory inside the chain (one step
// ahead) they left the wave in s_waitcnt for 70 % of its cycles: a step computes for ~150 cycles, a load from L2 takes several hundred.  They are
// staged in LDS before the chains start: ebm[k] = eb_l[k] * mtab[mask_idx[k]] and athc[k] = ATH_cb_l[k] * ATH.adjust (the products the chain
// formed at every use: same operands, same operation) and the spreading rows s3_ll, which overlay the arrays only the later phases use.
enum { PSYB_S3_LDS = 1024 };
template <int NCH> struct PsyBLdsT : PsyBTabs {
    double ebm[CBANDS], athc[CBANDS];
    float thr_l[NCH][CBANDS + 2];
    union {
        struct { float thr_s[NCH][3][CBANDS + 2]; float E[NCH][E_STRIDE]; };     // short limiting onwards
        float s3[PSYB_S3_LDS];                                                   // long spreading: T.s3_ll
    };
};
typedef PsyBLdsT<2> PsyBLds;
typedef PsyBLdsT<4> PsyBLds4;

// js_toint32(v8_log10_pos(ratio) * 16.0), the table index of mask_add (PsyModel.js:403-473), for 1 <= ratio < 2^20 -- without the
// logarithm where that is safe: the index is a step function of ratio with steps at 10^(k / 16), and away from the steps any
// approximation of 16 log10(ratio) with an error below the distance to the next integer gives the same integer.
// t = log2_f32((float)ratio) * 16 log10(2): error < 2e-5 (one ulp of v_log_f32 at |log2| <= 20, the conversion of ratio, the f32
// multiply); returns -1 within 2e-4 of an integer (the caller then takes the logarithm, as before; about 1 operand in 2500).
LHIP_DEV int ma_index16(double ratio) {
    const float t = fast_log2f((float)ratio) * 4.81647993062369912f;
    const float k = __builtin_floorf(t);
    const float fr = t - k;
    // (written so that a ratio beyond Float32 or a NaN -- t infinite or NaN, fr NaN -- fails the test and takes the logarithm as well)
    int i = -1;
    if (fr >= 2e-4f && fr <= 1.0f - 2e-4f) i = (int)k;
#ifdef LHIP_HOSTSIM
    if (i >= 0 && i != js_toint32(v8_log10_pos(ratio) * 16.0)) { fprintf(stderr, "hostsim: ma_index16 disagrees with the logarithm at %a\n", ratio); abort(); }
#endif
    return i;
}
LHIP_DEV int ma_index16_exact(double ratio) {
    int i = ma_index16(ratio);
    if (i < 0) i = js_toint32(v8_log10_pos(ratio) * 16.0);
    return i;
}

LHIP_DEV double mask_add_l(const Tables& T, const PsyBTabs& L, double ath_cb, double m1, double m2, int b) {
    // PsyModel.js:403-473 (long blocks).  Every logarithm here has a positive, finite, normal operand -- `ratio` lies in
    // [1, ma_max_i2) and m1 / m2 in (1, ma_max_m) on the paths that take it -- so the branch-free v8_log10_pos applies (lhip_math.h)
    double ratio;
    if (m2 > m1) {
        if (m2 < (m1 * T.ma_max_i2)) ratio = m2 / m1;
        else return (m1 + m2);
    } else {
        if (m1 >= (m2 * T.ma_max_i2)) return (m1 + m2);
        ratio = m1 / m2;
    }
    m1 += m2;
    if ((b + 3) <= 3 + 3) {
        if (ratio >= T.ma_max_i1) return m1;
        const int i = ma_index16_exact(ratio);
        return m1 * L.mt2[i];
    }
    const int i = ma_index16_exact(ratio);
    m2 = ath_cb;
    if (m1 < T.ma_max_m * m2) {
        if (m1 > m2) {
            double f = 1.0;
            if (i <= 13) f = L.mt3[i];
            const double r = v8_log10_pos(m1 / m2) * (10.0 / 15.0);
            return m1 * ((L.mt1[i] - f) * r + f);
        }
        if (i > 13) return m1;
        return m1 * L.mt3[i];
    }
    return m1 * L.mt1[i];
}


// NS_INTERP (PsyModel.js:828-842).  r = constant * pcfact; pcfact is 0 with the reservoir disabled, where this returns y unchanged
LHIP_DEV double ns_interp(double x, double y, double r) {
    if (r >= 1.0) return x;
    if (r <= 0.0) return y;
    if (y > 0.0) return v8_pow(x / y, r) * y;
    return 0.0;
}

// par >= 0 (bit reservoir): only the psy calls with q % mode_gr == par -- the second granule's short-block pre-echo control looks at
// the first one's finished thresholds, so the two are launched one after the other
// resv_size / resv_max (bit reservoir only): ResvSize / ResvMax as the previous frame left them -- handed in by the caller, which knows
// where the stream's reservoir record lives (the persistent per-stream kernel keeps it in LDS and pipelines the previous frame's bit
// packing with this call, so this function must not read the record itself)
// LAZY = 1 (batches whose psyA ran lazily: reservoir disabled): the short limiting, convert_partition2scalefac_s and the short pre-echo control only where
// psy_need_s says the call's short thresholds are read; elsewhere the E_EN_S / E_THM_S entries of W.E are written as zeros.
template <int NCH, int LAZY = 0> LHIP_DEV void kb_psyB(const Tables& T, const PowBase& pb10, const Workspace& W, const StreamDesc* SD, int gslot, int lane, PsyBLdsT<NCH>& L, int par = -1,
                                         int resv_size = 0, int resv_max = 0) {
    const int C = T.channels_out, Cp = T.psy_channels;      // Cp <= NCH: the launch picks the instantiation by Tables::psy_channels
    const int st = W.gslot_stream[gslot];
    const StreamDesc sd = SD[st];
    const int q = gslot - sd.gslot0 - 1;
    if (q < 0) return;
    if (par >= 0 && q % T.mode_gr != par) return;
    const bool shortw = LAZY ? psy_need_s(T, W, sd, gslot) != 0 : true;
    // PsyModel.js:1036-1038: share of the reservoir in use, as the previous frame left it (0 with the reservoir disabled)
    double pcfact = 0.0;
    if (!T.disable_reservoir) pcfact = resv_max == 0 ? 0.0 : (double)resv_size / resv_max * 0.5;
    const int fs = sd.fslot0 + q / T.mode_gr;            // ATH.adjust as left by the previous frame
    const double ath_adjust = W.ath_adjust[fs];
    for (int i = lane; i < 25; i += LHIP_NL) {
        L.mt1[i] = T.ma_table1[i];
        if (i < 10) L.mt2[i] = T.ma_table2[i];
        if (i < 14) L.mt3[i] = T.ma_table3[i];
        if (i < 9) L.mtab[i] = T.ma_tab[i];
    }
    wave_sync();

    for (int i = lane; i < T.n_s3_ll; i += LHIP_NL) L.s3[i] = T.s3_ll[i];
    LHIP_LANE_ONCE(k, 0, T.npart_l) L.athc[k] = (double)T.ATH_cb_l[k] * ath_adjust;
    for (int ch = 0; ch < Cp; ch++) {
        const int64_t o = (int64_t)gslot * Cp + ch;
        const float* eb_l = W.eb_l + o * EBL_STRIDE;
        const int32_t* midx = W.mask_idx + o * EBL_STRIDE;
        LHIP_LANE_ONCE(k, 0, T.npart_l) L.ebm[k] = (double)eb_l[k] * L.mtab[midx[k]];
        wave_sync();
        // long-block spreading with additive masking (PsyModel.js:1274-1320); thr = ecb (pcfact == 0)
        // The additive-masking chain is serial in the partition's spreading row; all of its operands are in LDS (see PsyBLdsT).
        LHIP_LANE_ONCE(b, 0, T.npart_l) {                        // npart_l < CBANDS = 64
            const int k0 = T.s3ind[2 * b], k1 = T.s3ind[2 * b + 1], j0 = T.s3off_l[b];
            double ecb = (double)L.s3[j0] * L.ebm[k0];
            for (int kk = k0 + 1; kk <= k1; kk++)
                ecb = mask_add_l(T, L, L.athc[kk], ecb, (double)L.s3[j0 + (kk - k0)] * L.ebm[kk], kk - b);
            ecb *= 0.158489319246111;
            float thr = (float)ecb;
            if (!T.disable_reservoir) {   // long-block pre-echo control (PsyModel.js:1300-1318): dead with the reservoir disabled (pcfact == 0)
                const float n1 = W.nb1[(o - Cp) * EBL_STRIDE + b], n2 = W.nb2[(o - Cp) * EBL_STRIDE + b];
                if (pcfact > 0.0 && !W.prev_short[(int64_t)gslot * C + (ch & 1)]) {
                    const double a = 2 * (double)n1, b2 = 16 * (double)n2, m = a < b2 ? a : b2;
                    thr = (float)ns_interp(ecb < m ? ecb : m, ecb, pcfact);
                }
                W.nb2[o * EBL_STRIDE + b] = n1;
                W.nb1[o * EBL_STRIDE + b] = (float)ecb;
            }
            L.thr_l[ch][b] = thr;
        }
        wave_sync();                                  // the next channel refills ebm
    }
    // (the spreading rows are dead: their LDS is thr_s / E from here on)
    if (shortw) for (int ch = 0; ch < Cp; ch++) {
        const int64_t o = (int64_t)gslot * Cp + ch;
        // short-block limiting by the two previous sub-blocks (compute_masking_s, 762-775)
        const int pshort = W.prev_short[(int64_t)gslot * C + (ch & 1)];      // blocktype_old[chn & 1] (PsyModel.js:767)
        for (int it = lane; it < 3 * T.npart_s; it += LHIP_NL) {
            const int sblock = it / T.npart_s, b = it - sblock * T.npart_s;
            const float* e0 = W.ecb_s + o * EBS_STRIDE;
            const float* em = W.ecb_s + (o - Cp) * EBS_STRIDE;      // previous psy call (or carry)
            const float ecb = e0[sblock * CBANDS + b];
            const float nb1 = sblock >= 1 ? e0[(sblock - 1) * CBANDS + b] : em[2 * CBANDS + b];
            const float nb2 = sblock >= 2 ? e0[(sblock - 2) * CBANDS + b] : em[(sblock + 1) * CBANDS + b];
            double x = 2 * (double)nb1;
            float thr = (float)((double)ecb < x ? (double)ecb : x);
            if (pshort) {
                x = 16 * (double)nb2;
                const double y = thr;
                thr = (float)(x < y ? x : y);
            }
            L.thr_s[ch][sblock][b] = thr;
        }
    }
    wave_sync();

    for (int ch = 0; ch < Cp; ch++) {
        const int64_t o = (int64_t)gslot * Cp + ch;
        const float* eb_l = W.eb_l + o * EBL_STRIDE;
        float* Eo = L.E[ch];
        // convert_partition2scalefac_l (PsyModel.js:692-734): lane per scalefactor band
        for (int sb = lane; sb < SBMAX_l; sb += LHIP_NL) {
            const int npart = T.npart_l;
            const int bstart = sb == 0 ? 0 : T.bo_l[sb - 1];      // partition shared with the previous band
            float en_f = 0.f, thm_f = 0.f;
            // band sb exists only if the walk has not run past npart before reaching it
            if (sb == 0 || bstart < npart) {
                double enn = 0.0, thmm = 0.0;
                int b = bstart;
                if (sb > 0) {
                    const double w_next = 1.0 - (double)T.bo_l_weight[sb - 1];
                    enn = w_next * (double)eb_l[b];
                    thmm = w_next * (double)L.thr_l[ch][b];
                    b++;
                }
                const int bo = T.bo_l[sb];
                const int b_lim = bo < npart ? bo : npart;
                while (b < b_lim) { enn += (double)eb_l[b]; thmm += (double)L.thr_l[ch][b]; b++; }
                en_f = (float)enn; thm_f = (float)thmm;
                if (b < npart) {
                    const double w_curr = T.bo_l_weight[sb];
                    en_f = (float)((double)en_f + w_curr * (double)eb_l[b]);
                    thm_f = (float)((double)thm_f + w_curr * (double)L.thr_l[ch][b]);
                }
            }
            Eo[E_EN_L + sb] = en_f;
            Eo[E_THM_L + sb] = thm_f;
        }
        // convert_partition2scalefac_s (644-687)
        if (!shortw) for (int it = lane; it < 3 * SBMAX_s; it += LHIP_NL) { Eo[E_EN_S + it] = 0.f; Eo[E_THM_S + it] = 0.f; }
        if (shortw) for (int it = lane; it < 3 * SBMAX_s; it += LHIP_NL) {
            const int sblock = it / SBMAX_s, sb = it - sblock * SBMAX_s;
            const float* ebs = W.eb_s + o * EBS_STRIDE + sblock * CBANDS;
            const float* thr = L.thr_s[ch][sblock];
            const int npart = T.npart_s;
            const int bstart = sb == 0 ? 0 : T.bo_s[sb - 1];
            float en_f = 0.f, thm_f = 0.f;
            if (sb == 0 || bstart < npart) {
                double enn = 0.0, thmm = 0.0;
                int b = bstart;
                if (sb > 0) {
                    const double w_next = 1.0 - (double)T.bo_s_weight[sb - 1];
                    enn = w_next * (double)ebs[b];
                    thmm = w_next * (double)thr[b];
                    b++;
                }
                const int bo = T.bo_s[sb];
                const int b_lim = bo < npart ? bo : npart;
                while (b < b_lim) { enn += (double)ebs[b]; thmm += (double)thr[b]; b++; }
                en_f = (float)enn; thm_f = (float)thmm;
                if (b < npart) {
                    const double w_curr = T.bo_s_weight[sb];
                    en_f = (float)((double)en_f + w_curr * (double)ebs[b]);
                    thm_f = (float)((double)thm_f + w_curr * (double)thr[b]);
                }
            }
            Eo[E_EN_S + sb * 3 + sblock] = en_f;
            Eo[E_THM_S + sb * 3 + sblock] = thm_f;                 // as converted; the pre-echo control follows
        }
    }
    wave_sync();
    if (shortw) for (int ch = 0; ch < Cp; ch++) {
        // short-block pre-echo control (PsyModel.js:1226-1267), one lane per band, the three sub-blocks in order: x0.8, the two
        // attack-driven interpolations towards the previous sub-block's finished threshold (sub-block 0: the previous CALL's
        // sub-block 2) -- identities when pcfact == 0 -- and the pulse halving.  ns_attacks holds only 0 / 1, so
        // the reference's `>= 2` and `== 3` alternatives never fire.
        const int64_t o = (int64_t)gslot * Cp + ch;
        const float* pk = W.peaks + o * PK_STRIDE;            // en_subshort[3..11]
        const int att = W.att_clean[o];
        float* Eo = L.E[ch];
        LHIP_LANE_ONCE(sb, 0, SBMAX_s) {
            float prev = pcfact > 0.0 ? W.E[(o - Cp) * E_STRIDE + E_THM_S + sb * 3 + 2] : 0.f;      // (only read where the previous call is complete)
            for (int sblock = 0; sblock < 3; sblock++) {
                double thmm = Eo[E_THM_S + sb * 3 + sblock];
                thmm *= 0.8;
                if ((att >> (sblock + 1)) & 1) { const double p = ns_interp(prev, thmm, 0.6 * pcfact); thmm = thmm < p ? thmm : p; }
                if ((att >> sblock) & 1) { const double p = ns_interp(prev, thmm, 0.3 * pcfact); thmm = thmm < p ? thmm : p; }
                const double e3 = pk[sblock * 3 + 0], e4 = pk[sblock * 3 + 1], e5 = pk[sblock * 3 + 2];
                const double enn = e3 + e4 + e5;
                if (e5 * 6 < enn) {
                    thmm *= 0.5;
                    if (e4 * 6 < enn) thmm *= 0.5;
                }
                prev = (float)thmm;
                Eo[E_THM_S + sb * 3 + sblock] = prev;
            }
        }
    }
    wave_sync();
    const int nthm = shortw ? SBMAX_l + 3 * SBMAX_s : SBMAX_l;      // thresholds the channel-mixing steps below go over
    // inter-channel masking (PsyModel.js:525-543): stereo mode with ratio > 0
    if ((T.mode == 0 || T.mode == 1) && T.interChRatio > 0.0 && C > 1) {
        const double r_ = T.interChRatio;
        float nl[2] = {0.f, 0.f};
        for (int i = lane; i < nthm; i += LHIP_NL) {
            const int idx = E_THM_L + i;                       // thm.l then thm.s are contiguous
            const double l = L.E[0][idx], r = L.E[1][idx];
            nl[0] = (float)(l + r * r_);
            nl[1] = (float)(r + l * r_);
            L.E[0][idx] = nl[0];
            L.E[1][idx] = nl[1];
        }
        wave_sync();
    }
    if constexpr (NCH == 4) if (Cp == 4) {
        // joint stereo (PsyModel.js:1336-1342): msfix1 (548-582), then ns_msfix (591-636) with the ATH.adjust the previous frame left.
        // One lane per band (thm.l then thm.s are contiguous in E, and so are en.l / en.s); both steps only touch the band's own
        // four thresholds, so they run back to back in the lane.
        const double msfix = T.msfix;
        const bool do_ns = d_abs(msfix) > 0.0;
        const double athlower_l = do_ns ? v8_pow_base(pb10, T.ATHlower * ath_adjust) : 0.0;
        const double athlower_s = athlower_l * ((double)BLKSIZE_s / BLKSIZE);
        for (int i = lane; i < nthm; i += LHIP_NL) {
            const int it = E_THM_L + i, ie = E_EN_L + i;
            const bool lng = i < SBMAX_l;
            const int sb = lng ? i : (i - SBMAX_l) / 3;
            float t0 = L.E[0][it], t1 = L.E[1][it], t2 = L.E[2][it], t3 = L.E[3][it];
            if (!((double)t0 > 1.58 * (double)t1 || (double)t1 > 1.58 * (double)t0)) {
                const double m = lng ? (double)T.mld_l[sb] : (double)T.mld_s[sb];
                double mld = m * (double)L.E[3][ie];
                const double lo1 = (double)t3 < mld ? (double)t3 : mld;
                const double rmid = (double)t2 > lo1 ? (double)t2 : lo1;
                mld = m * (double)L.E[2][ie];
                const double lo2 = (double)t2 < mld ? (double)t2 : mld;
                const double rside = (double)t3 > lo2 ? (double)t3 : lo2;
                t2 = (float)rmid; t3 = (float)rside;
            }
            if (do_ns) {
                const double ath = lng ? (double)T.ATH_cb_l[T.bm_l[sb]] * athlower_l : (double)T.ATH_cb_s[T.bm_s[sb]] * athlower_s;
                const double a0 = (double)t0 > ath ? (double)t0 : ath, a1 = (double)t1 > ath ? (double)t1 : ath;
                const double thmLR = a0 < a1 ? a0 : a1;
                double thmM = (double)t2 > ath ? (double)t2 : ath, thmS = (double)t3 > ath ? (double)t3 : ath;
                if (thmLR * (msfix * 2.0) < thmM + thmS) {
                    const double f = thmLR * (msfix * 2.0) / (thmM + thmS);
                    thmM *= f;
                    thmS *= f;
                }
                t2 = (float)(thmM < (double)t2 ? thmM : (double)t2);
                t3 = (float)(thmS < (double)t3 ? thmS : (double)t3);
            }
            L.E[2][it] = t2; L.E[3][it] = t3;
        }
        wave_sync();
    }
    for (int ch = 0; ch < Cp; ch++)
        for (int i = lane; i < E_STRIDE; i += LHIP_NL) W.E[((int64_t)gslot * Cp + ch) * E_STRIDE + i] = L.E[ch][i];
}
}  // namespace lhip
