// k_quant_fast.h -- the speculative quantization pass of a FAST table set (quality 7, LAME's -f: noise_shaping == 0 and use_best_huffman == 0):
// the reference's outer_loop returns right after bin_search_StepSize (Quantize.js:886-888) and iteration_finish_one has no best_huffman_divide.
//
// The general program (k_quant_frame.h, k_quant_search.h: q_unit / q_outer_loop) computes exactly that for such a table set -- it reads the switches -- but it is one body for
// every setting: the noise loop, the amplification, the Huffman region search and the count helpers are compiled into every kernel that holds it, and
// they set its registers and its code size.  This file is the same granule-channel with nothing but what the fast mode runs, built from the q_*
// functions of k_quant.h by calling them: load the lines, x^(3/4) and the energy test, what calc_xmin leaves behind that quantization reads
// (q_search_limits), the bin search over count_bits with all-zero scalefactors (q_bin_search), best_scalefac_store / scfsi, the record.  It leaves
// GrSide, the bin-search memo (bs_tab, bs_asg, bs_ntab, bs_state) and the digest words (W.vdig) exactly as q_unit / q_outer_loop leave them, so
// g_validate_fast, g_fixup (whose repair pass keeps the general body) and g_bits run behind it unchanged.
//
// One wave per CHANNEL at every batch size (kb_quant_fast<1>): the channels of a granule are independent given the granule's bit budget -- the
// reference's loop (Quantize.js:1406-1466) passes nothing between them but the reservoir count afterwards -- so the two waves of a pair meet once per
// granule to exchange the bits they used, through a FastPair record in LDS.  The waves of a pair are neighbours in one persistent workgroup
// (g_quant_fast, lhip_kernels.h); pairs do not wait for each other: no workgroup barrier inside the frame loop.
#pragma once
namespace lhip {

// bin_search_StepSize (Quantize.js:322-381) and nothing behind it: the two states ST_BS / ST_BSUP of q_outer_loop, on the granule state itself (the
// general loop works on a copy, cod_info_w, and copies it back when noise_shaping == 0).  The working spectrum L.ixw ends as the quantization at the
// gain found; the scalefactors stay the zeros q_init_outer_loop wrote.  Memo and digest: as q_outer_loop writes them.
template <int SKIP>
LHIP_DEV void q_bin_search(const Tables& T, GI& g, int targ_bits, int bs_start, int bs_step, int* bs_gain_out, GrSide* rec, uint32_t* dig, int64_t dn,
                           int lane, QuantLds& L, const QuantTabs& Q) {
    lane = fresh_lane(lane);
    PrevNoise pn; pn.gain = 0; pn.sfb_count1 = 0;
    targ_bits = uni(targ_bits); bs_start = uni(bs_start); bs_step = uni(bs_step);
    uni_gi(g);
    int CurrentStep = bs_step, flagGoneOver = 0, Direction = 0, up = 0, nbs = 0;
    const int desired_rate = targ_bits - g.part2_length;
    g.global_gain = bs_start;
    for (;;) {
        uni_gi(g); CurrentStep = uni(CurrentStep); flagGoneOver = uni(flagGoneOver); Direction = uni(Direction); up = uni(up); nbs = uni(nbs);
        int asg = 0;
        const int nBits = q_count_bits_rounds<SKIP>(T, g, L.sfw, L.ixw, 0, pn, &asg, lane, L, Q);
        if (nbs < BS_TAB_MAX) { if (lane == 0) { L.memo.bs_tab[nbs] = (g.global_gain << 24) | nBits; L.memo.bs_asg[nbs] = asg; } nbs++; }
        if (bs_advance(nBits, desired_rate, g.global_gain, CurrentStep, flagGoneOver, Direction, up)) continue;
        g.part2_3_length = nBits;
        break;
    }
    *bs_gain_out = g.global_gain;                            // OldValue[ch] after this granule
    q_flush_bs_memo(g, targ_bits, nbs, rec, dig, dn, lane, L);
}

// One granule-channel of a fast table set, from the spectrum to the published record: q_unit without what such a table set never runs.
template <int SKIP>
LHIP_DEV UnitOut q_unit_fast(const Tables& T, const PowBase& pb10, const Workspace& W, int C, int fidx, int gslot, int gr, int ch, int mode_ext,
                             double ath_adjust, int targ_ch, Seed used, int gr0_bt, int lane, QuantLds& L, const QuantTabs& Q) {
    lane = lane_anew(lane);
    UnitOut u; u.next = used;
    GI g;
#if defined(LHIP_HOSTSIM)
    // simulations only (as q_unit): stale values in the words no evaluation of a tail0 search writes must not survive into the record
    if (SKIP) { for (int i = 256 + lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0x1fff1fffu; wave_sync(); }
#endif
    const int bt = W.blocktype[(int64_t)gslot * C + ch];
    q_init_outer_loop(T, pb10, ath_adjust, g, bt, xr_source(W, C, gslot, ch, mode_ext == 2), mode_ext == 2 ? nullptr : W.xr + ((int64_t)gslot * C + ch) * 576, 0, lane, L, Q);
    int active = 0, bs_gain = 0;
    GrSide* out = W.side + ((int64_t)fidx * 2 + gr) * C + ch;
    if (q_init_xrpow(g, lane, L, Q)) {
        active = 1;
        q_search_limits(g, lane, L, SKIP);
        if constexpr (SKIP != 0) {
            if (g.tail0) { for (int i = 256 + lane; i < 288; i += LHIP_NL) ((uint32_t*)L.ixw)[i] = 0u; wave_sync(); }
        }
        q_bin_search<SKIP>(T, g, targ_ch, used.start, used.step, &bs_gain, out, W.vdig + ((int64_t)fidx * 2 + gr) * C + ch, W.vdig_n, lane, L, Q);
        uni_gi(g); bs_gain = uni(bs_gain);
        lane = lane_anew(lane);
        Seed nx; nx.step = (used.start - bs_gain >= 4) ? 4 : 2; nx.start = bs_gain;
        u.next = nx;
    } else {
        for (int i = lane; i < 576; i += LHIP_NL) L.ixw[i] = 0;
        wave_sync();
    }
    int scfsi[4];
    q_best_scalefac_store(T, g, gr, ch, gr0_bt, scfsi, lane, L, Q);
    uni_gi(g);
    u.bits = g.part2_3_length + g.part2_length;
    u.block_type = g.block_type;
    if (gr == 0) { LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) L.sf_gr0[ch][i] = (int8_t)L.sfb[i]; }
    // ---- publish the record and the signed quantized spectrum: q_unit's statements (k_quant_frame.h), a second copy to be changed with them (see there) ----
    lane = lane_anew(lane);
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
        out->mode_ext = uni_here(mode_ext);
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

// The meeting place of the two waves of a pair (LDS, zeroed before the first frame).  `round` counts the frames the pair has drawn, from 1, and every word a
// wave waits on only ever grows.  Wave 0 of the pair draws the frame slot and hands it to wave 1, which acknowledges it: wave 0 does not hand over the next
// slot before that, so it is at most one frame ahead (between granules it needs its partner anyway) and the bits are kept per parity of the round.
struct FastPair { int slot, slot_seq, slot_ack, pad_, done[2][2], bits[2][2][2]; };

LHIP_DEV void fast_pair_wait(const int* p, int round, int lane) {
    long spins = 0;
    while (wg_load(p, lane) < round) { wg_idle(); LHIP_SPIN_GUARD(spins); }
    wg_acquire();
}
LHIP_DEV void fast_pair_publish_slot(FastPair& fp, int round, int fslot, int lane) {
    fast_pair_wait(&fp.slot_ack, round - 1, lane);
    if (lane == 0) fp.slot = fslot;
    wg_store(&fp.slot_seq, round, lane);
}
LHIP_DEV int fast_pair_await_slot(FastPair& fp, int round, int lane) {
    fast_pair_wait(&fp.slot_seq, round, lane);
    const int fslot = wg_load(&fp.slot, lane);
    wg_store(&fp.slot_ack, round, lane);
    return fslot;
}

// The frame program of the speculative pass (kb_quant with chain == 0, no reservoir) around q_unit_fast.  PAIR == 0: one wave, the frame's channels in turn
// (one-channel streams; the one-lane simulation).  PAIR == 1: wave `my_ch` of a pair does that channel of every granule.
template <int PAIR, int SKIP>
LHIP_DEV void kb_quant_fast(const Tables& T, const PowBase& pb10, const Workspace& W, const StreamDesc* SD, int fslot, int lane, QuantLds& L,
                            const QuantTabs& Q, int* hint, int my_ch = -1, FastPair* fp = nullptr, int round = 0) {
    lane = lane_anew(lane);
    const int C = T.channels_out;
    const int st = uni(W.fslot_stream[fslot]);
    const StreamDesc sd = SD[st];
    const int k = uni(fslot - sd.fslot0 - 1);
    if (k < 0) return;
    const int fidx = uni(sd.out_slot0 + k);
    const double ath_adjust = unid(W.ath_adjust[fslot]);
    const int padding = uni(frame_padding(T, sd, k));
    const int mean_bits = uni((frame_bits_of(T, padding) - T.sideinfo_len * 8) / T.mode_gr);
    Seed seed0, seed1;
    seed0.start = seed1.start = W.spec_start; seed0.step = seed1.step = W.spec_step;
    if (k == 0) {
        seed0 = seed_before(W, sd, C, k, 0, 0);
        if (C > 1) seed1 = seed_before(W, sd, C, k, 0, 1);
        seed0.start = uni(seed0.start); seed0.step = uni(seed0.step); seed1.start = uni(seed1.start); seed1.step = uni(seed1.step);
    } else if (hint[0] == st) {
        // (any seed is legitimate here: the validation replays the search with the chain-implied one)
        if (hint[1] >= 0) { seed0.start = hint[1]; seed0.step = 2; }
        if (C > 1 && hint[2] >= 0) { seed1.start = hint[2]; seed1.step = 2; }
    }
    int gr0_bt0 = 0, gr0_bt1 = 0;
    const int mode_ext = (T.mode == 1) ? q_ms_decision(T, W, sd, k, lane, L) : 0;      // (each wave of a pair for itself: a few band sums)
    int ResvSize = 0;
    q_ath_pseudo(T, pb10, ath_adjust, lane, L, Q);
    for (int gr = 0; gr < T.mode_gr; gr++) {
        const int gslot = sd.gslot0 + 1 + T.mode_gr * k + gr;
        int targ[2] = {0, 0};
        const double max_bits = (double)targ_bits_for(T, mean_bits, gr, ResvSize, targ);
        if (mode_ext == 2) {
            const float* te = W.tot_ener + (int64_t)(gslot - 1) * 4;
            double r = (double)te[2] + (double)te[3];
            if (r > 0) r = (double)te[3] / r;
            q_reduce_side(targ, r, mean_bits, max_bits);
        }
        const int targ0 = uni(targ[0]), targ1 = uni(targ[1]);
        for (int ch = 0; ch < C; ch++) {
            if (PAIR && ch != my_ch) continue;
            const UnitOut u = q_unit_fast<SKIP>(T, pb10, W, C, fidx, gslot, gr, ch, mode_ext, ath_adjust, ch == 0 ? targ0 : targ1, ch == 0 ? seed0 : seed1,
                                                ch == 0 ? gr0_bt0 : gr0_bt1, lane, L, Q);
            if (u.active) { if (ch == 0) seed0 = u.next; else seed1 = u.next; }
            if (!PAIR) ResvSize = uni(ResvSize - u.bits);
            else if (lane == 0) fp->bits[round & 1][gr][ch] = u.bits;
            if (gr == 0) { if (ch == 0) gr0_bt0 = u.block_type; else gr0_bt1 = u.block_type; }
        }
        if (PAIR && gr + 1 < T.mode_gr) {             // the other channel's bits feed the next granule's budget; behind the last granule nothing reads them
            wg_store(&fp->done[gr][my_ch], round, lane);
            fast_pair_wait(&fp->done[gr][my_ch ^ 1], round, lane);
            ResvSize = uni(ResvSize - (wg_load(&fp->bits[round & 1][gr][0], lane) + wg_load(&fp->bits[round & 1][gr][1], lane)));
        }
    }
    hint[0] = st; hint[1] = seed0.start; hint[2] = C > 1 ? seed1.start : -1;
}

}  // namespace lhip
