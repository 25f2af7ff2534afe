// k_quant_budget.h -- what a frame's granule-channels start from: the bin-search seed chain (Quantize.js:324-326, 377-378), the perceptual entropies and
// the M/S decision (PsyModel.js:845-905, Encoder.js:520-561), on_pe / reduce_side (QuantizePVT.js:421-534) with ResvMaxBits (Reservoir.js:190-229).
#pragma once
#include "k_quant_tabs.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// Bin-search seed chain (Quantize.js:324-326, 377-378: gfc.OldValue / gfc.CurrentStep).
// The seed of a granule-channel is a function of the bin-search results of the two most recent
// *active* granules of that channel: start = gain[p1], step = (start_of_p1 - gain[p1] >= 4) ? 4 : 2
// with start_of_p1 = gain[p2].  Frames are quantized speculatively (kb_quant with chain == 0 uses the
// reset seed), then kb_validate re-runs every bin search with the chain-implied seed and flags
// frames whose result differs; flagged frames are re-quantized with chain == 1 until none is left.
// ---------------------------------------------------------------------------------------------
struct Seed { int start, step; };

// What the seed chain reads of an earlier granule-channel -- was it active, and the gain its bin search ended on -- from its side record or from the
// head word of its digest (W.vdig: the memo-only validation, which does not touch the records)
LHIP_DEV const GrSide* seed_entry(const GrSide* side, int64_t gc) { return side + gc; }
LHIP_DEV uint32_t seed_entry(const uint32_t* vdig, int64_t gc) { return vdig[gc]; }
LHIP_DEV int seed_entry_active(const GrSide* r) { return r->active; }
LHIP_DEV int seed_entry_gain(const GrSide* r) { return r->bs_gain; }
LHIP_DEV int seed_entry_active(uint32_t h) { return vd_active(h); }
LHIP_DEV int seed_entry_gain(uint32_t h) { return vd_gain(h); }

// seed seen by granule (k, gr) of channel ch, derived from all earlier granules of the channel as SRC holds them: the side records, or
// &Workspace::vdig for the digests
template <auto SRC = &Workspace::side>
LHIP_DEV Seed seed_before(const Workspace& W, const StreamDesc& sd, int C, int k, int gr, int ch) {
    const int32_t* carry = W.seed + ((int64_t)sd.fslot0 * C + ch) * 2;
    int g1 = -1, g2 = -1;                                    // gains of the last / second-to-last active granule
    const int GR = W.mode_gr;                                 // side records and digests are laid out [frame][2][C] whatever GR is
    for (int q = GR * k + gr - 1; q >= 0; q--) {
        const auto e = seed_entry(W.*SRC, (((int64_t)sd.out_slot0 + q / GR) * 2 + q % GR) * C + ch);
        if (seed_entry_active(e)) {
            if (g1 < 0) g1 = seed_entry_gain(e);
            else { g2 = seed_entry_gain(e); break; }
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
}  // namespace lhip
