// k_quant_search.h -- the search itself: quant_compare, the kept quantization's scalars in LDS (gi_keep_*) and bin_search_StepSize + outer_loop
// as one state machine (q_outer_loop).
#pragma once
#include "k_quant_helper.h"
#include "k_quant_amp.h"
namespace lhip {
LHIP_DEV int q_quant_compare(const NoiseRes& best, const NoiseRes& calc) {   // Quantize.js:481-568 case 9
    int better;
    if (best.over_count > 0) {
        better = calc.over_SSD <= best.over_SSD;
        if (calc.over_SSD == best.over_SSD) better = calc.bits < best.bits;
    } else {
        better = ((calc.max_noise < 0) && ((calc.max_noise * 10 + calc.bits) <= (best.max_noise * 10 + best.bits)));
    }
    if (best.over_count == 0) better = better && calc.bits < best.bits;
    return better;
}

// The kept quantization's scalars live in LDS while the outer loop runs (only part2_3_length is read there): the loop carries
// one GrInfo (the working copy) in scalar registers instead of two, which is most of what used to spill.  Fields the loop never
// changes (block type, band limits, max_nonzero_coeff) are the same in both copies and are not stored.
LHIP_DEV void gi_keep_store(QuantLds& L, const GI& w, int lane) {
    lane = fresh_lane(lane);
    if (lane == 0) {
        int32_t* k = L.gkeep;
        k[0] = w.part2_3_length; k[1] = w.big_values; k[2] = w.count1; k[3] = w.global_gain; k[4] = w.scalefac_compress;
        k[5] = w.table_select[0]; k[6] = w.table_select[1]; k[7] = w.table_select[2];
        k[8] = w.subblock_gain[0]; k[9] = w.subblock_gain[1]; k[10] = w.subblock_gain[2]; k[11] = w.subblock_gain[3];
        k[12] = w.region0_count; k[13] = w.region1_count; k[14] = w.preflag; k[15] = w.scalefac_scale; k[16] = w.count1table_select;
        k[17] = w.part2_length; k[18] = w.count1bits;
        union { double d; int32_t i[2]; } u; u.d = w.xrpow_max; k[19] = u.i[0]; k[20] = u.i[1];
    }
}
LHIP_DEV void gi_keep_load(const QuantLds& L, GI& g) {
    const int32_t* k = L.gkeep;
    g.part2_3_length = uni(k[0]); g.big_values = uni(k[1]); g.count1 = uni(k[2]); g.global_gain = uni(k[3]); g.scalefac_compress = uni(k[4]);
    g.table_select[0] = uni(k[5]); g.table_select[1] = uni(k[6]); g.table_select[2] = uni(k[7]);
    g.subblock_gain[0] = uni(k[8]); g.subblock_gain[1] = uni(k[9]); g.subblock_gain[2] = uni(k[10]); g.subblock_gain[3] = uni(k[11]);
    g.region0_count = uni(k[12]); g.region1_count = uni(k[13]); g.preflag = uni(k[14]); g.scalefac_scale = uni(k[15]); g.count1table_select = uni(k[16]);
    g.part2_length = uni(k[17]); g.count1bits = uni(k[18]);
    union { double d; int32_t i[2]; } u; u.i[0] = uni(k[19]); u.i[1] = uni(k[20]); g.xrpow_max = u.d;
}

// One step of bin_search_StepSize (Quantize.js:322-381): the evaluation at `gain` counted nBits.  `up` = the halving phase is over and only the
// `gain++` tail is left.  Returns 1 if the search goes on (evaluate at the new `gain`), 0 if `gain` is its result.  The fast pass (q_bin_search) and
// both replays (kb_validate, validate_fast_gc) call it; q_outer_loop carries the same statements inside its state machine (see there).
LHIP_DEV int bs_advance(int nBits, int desired_rate, int& gain, int& CurrentStep, int& flagGoneOver, int& Direction, int& up) {
    if (!up) {
        if (CurrentStep == 1 || nBits == desired_rate) up = 1;
        else {
            int step;
            if (nBits > desired_rate) {
                if (Direction == 2) flagGoneOver = 1;
                if (flagGoneOver) CurrentStep /= 2;
                Direction = 1;
                step = CurrentStep;
            } else {
                if (Direction == 1) flagGoneOver = 1;
                if (flagGoneOver) CurrentStep /= 2;
                Direction = 2;
                step = -CurrentStep;
            }
            gain += step;
            if (gain < 0) { gain = 0; flagGoneOver = 1; }
            if (gain > 255) { gain = 255; flagGoneOver = 1; }
            return 1;
        }
    }
    if (nBits > desired_rate && gain < 255) { gain++; return 1; }
    return 0;
}

// The end of a bin search: its memo (L.memo, nbs entries) goes to the side record in one burst, with the conditionally assigned fields of `g` as the
// search left them, and in the digest's compact form (`dig` / `dn`: see q_outer_loop)
LHIP_DEV void q_flush_bs_memo(const GI& g, int targ_bits, int nbs, GrSide* rec, uint32_t* dig, int64_t dn, int lane, QuantLds& L) {
    wave_sync();
    LHIP_LANE_ONCE(i, 0, nbs) {
        const int32_t e = L.memo.bs_tab[i], a = L.memo.bs_asg[i];
        rec->bs_tab[i] = e; rec->bs_asg[i] = a;
        if (i < VD_ENT) { dig[(VD_TAB + 2 * i) * dn] = (uint32_t)e; dig[(VD_TAB + 2 * i + 1) * dn] = (uint32_t)a; }
    }
    if (lane == 0) {
        const int state = pack_cond_fields(g, 0);
        rec->bs_ntab = nbs; rec->bs_state = state;
        dig[VD_TARG * dn] = (uint32_t)targ_bits | ((uint32_t)nbs << 24); dig[VD_STATE * dn] = (uint32_t)state;
    }
    wave_sync();
}

// outer_loop (Quantize.js:871-1052).  g = kept copy (cod_info); seeds in/out via start/step.
// bin_search_StepSize (Quantize.js:322-381) + outer_loop (Quantize.js:871-1052) as ONE state machine, so that the
// three big building blocks -- count_bits, calc_noise, balance_noise -- are each instantiated exactly once
// (code size decides instruction-cache behaviour here).  Everything runs on the working copy `w`
// (ixw / sfw); `g` (kept spectrum in HBM / sfb) is the kept quantization, exactly the reference's cod_info / cod_info_w pair
// with the roles of the first copy swapped (bin search on w, then g = w).
// `kept` (HBM, this granule-channel's slot of W.l3) receives the quantized spectrum of the kept copy whenever a better
// quantization is found; it is read back into L.ixw once the loop has finished (the working copy is dead then).
// `dig` / `dn`: the granule-channel's validation digest (word w at dig[w * dn]; lhip_layout.h VD_*): the bin-search memo in the compact,
// coalesced form the one-thread-per-frame validation reads
// `cs` (latency kernels only): the record through which a helper wave takes the Huffman count of the outer loop's evaluations while this wave
// runs calc_noise beside it (q_count_bits_piped); nullptr: everything on this wave
template <int SKIP = 0>
LHIP_DEV void q_outer_loop(const Tables& T, GI& g, int targ_bits, int bs_start, int bs_step, int* bs_gain_out,
                           int16_t* kept, GrSide* rec, uint32_t* dig, int64_t dn, int lane, QuantLds& L, const QuantTabs& Q, CountShare* cs = nullptr) {
    lane = fresh_lane(lane);
    enum { ST_BS, ST_BSUP, ST_A, ST_B };
    NoiseRes best, ni;
    PrevNoise pn; pn.gain = 0; pn.sfb_count1 = 0;
    best.max_noise = 0; best.over_count = 0; best.over_SSD = 0; best.bits = 0;
    LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) { L.pn_step[i] = 0; L.pn_dist[i] = 0.f; L.pn_x[i] = 1.0; L.pn_cls[i] = 0; L.distort[i] = 0.f; }
    wave_sync();
    targ_bits = uni(targ_bits); bs_start = uni(bs_start); bs_step = uni(bs_step);
    uni_gi(g);
    GI w = g;
    // bin-search state
    int CurrentStep = bs_step, flagGoneOver = 0, Direction = 0;
    const int desired_rate = targ_bits - w.part2_length;
    w.global_gain = bs_start;
    // outer-loop state
    int best_part2_3_length = 9999999, age = 0, maxggain = 255, huff_bits = 0, first = 1;
    int kept_p23 = g.part2_3_length;                        // cod_info.part2_3_length (the one kept field the loop reads)
    const int search_limit = 3;
    int st = ST_BS, nbs = 0;
    int ss_nbs = 0, ss_nup = 0, ss_run = 0, ss_moved = 0, ss_first_ = 0, ss_prev_bits_ = 0; (void)ss_nbs; (void)ss_nup; (void)ss_run; (void)ss_moved; (void)ss_first_; (void)ss_prev_bits_;
    LHIP_SS(ss_.searches++);
    for (;;) {
        uni_gi(w); kept_p23 = uni(kept_p23); st = uni(st); CurrentStep = uni(CurrentStep); flagGoneOver = uni(flagGoneOver); Direction = uni(Direction);
        best_part2_3_length = uni(best_part2_3_length); age = uni(age); maxggain = uni(maxggain); huff_bits = uni(huff_bits); first = uni(first);
        pn.gain = uni(pn.gain); pn.sfb_count1 = uni(pn.sfb_count1);
        best.max_noise = unid(best.max_noise); best.over_count = uni(best.over_count); best.over_SSD = uni(best.over_SSD); best.bits = uni(best.bits);
        int asg = 0;
        const int cnt1_seen = pn.sfb_count1;                  // what this evaluation's 0/1 shortcut is decided with
        int nBits, spec = 0;
        NoiseCommit nc; nc.fresh = 0; nc.step = 0; nc.cls = 0; nc.dist = 0.f; nc.x = 0.0;
#if LHIP_NL != 1
        if (cs != nullptr && st >= ST_A) nBits = q_count_bits_piped(T, w, L.sfw, L.ixw, pn, &asg, *cs, &ni, &nc, best.over_count == 0, &spec, lane, L, Q);
        else
#endif
        nBits = q_count_bits_rounds<SKIP>(T, w, L.sfw, L.ixw, st >= ST_A, pn, &asg, lane, L, Q);   // the only call site (but for the two-wave form above)
        LHIP_SS(ss_.evals++; if (st == ST_BS) ss_nbs++; else if (st == ST_BSUP) ss_nup++;
                if (st >= ST_A && ss_run > 0) { ss_.run_steps++; if (ss_moved) ss_.run_steps_cnt1_moved++; if (cnt1_seen > 0) ss_.run_steps_zo++; });
        // memo of the bin search: collected in LDS and written to the side record in one burst when the search ends (a global
        // store per step would sit in front of every later memory wait of the wave -- the VMEM counter retires in order)
        if (st <= ST_BSUP && nbs < BS_TAB_MAX) { if (lane == 0) { L.memo.bs_tab[nbs] = (w.global_gain << 24) | nBits; L.memo.bs_asg[nbs] = asg; } nbs++; }
        LHIP_SS(if (st <= ST_BSUP) { const int i_ = (ss_nbs + ss_nup - 1) < 7 ? (ss_nbs + ss_nup - 1) : 7; ss_.bsdir[i_ < 0 ? 0 : i_][st == ST_BSUP ? 1 : Direction][nBits > desired_rate]++; });
        // The bin-search step, written out as it always was: the second copy of bs_advance (`up` there is st == ST_BSUP here), to be changed with it.
        // Calling bs_advance here costs the latency kernels three vector registers (g_quant_pair 137 -> 140, g_frame<1> 193 -> 195, g_resv_stream
        // 226 -> 228: profiles/quant_split_shared_sites_resources.txt), and they may not grow.
        if (st == ST_BS) {
            if (CurrentStep == 1 || nBits == desired_rate) st = ST_BSUP;
            else {
                int step;
                if (nBits > desired_rate) {
                    if (Direction == 2) flagGoneOver = 1;
                    if (flagGoneOver) CurrentStep /= 2;
                    Direction = 1;
                    step = CurrentStep;
                } else {
                    if (Direction == 1) flagGoneOver = 1;
                    if (flagGoneOver) CurrentStep /= 2;
                    Direction = 2;
                    step = -CurrentStep;
                }
                w.global_gain += step;
                if (w.global_gain < 0) { w.global_gain = 0; flagGoneOver = 1; }
                if (w.global_gain > 255) { w.global_gain = 255; flagGoneOver = 1; }
                continue;
            }
        }
        if (st == ST_BSUP) {
            if (nBits > desired_rate && w.global_gain < 255) { w.global_gain++; continue; }
            w.part2_3_length = nBits;
            LHIP_SS(ss_.bs[ss_nbs < 39 ? ss_nbs : 39]++; ss_.bsup[ss_nup < 39 ? ss_nup : 39]++);
            *bs_gain_out = w.global_gain;                    // OldValue[ch] after this granule
            q_flush_bs_memo(w, targ_bits, nbs, rec, dig, dn, lane, L);
            if (0 == T.noise_shaping) {
                g = w;
                for (int i = lane; i < 288; i += LHIP_NL) ((uint32_t*)kept)[i] = ((const uint32_t*)L.ixw)[i];
                LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) L.sfb[i] = L.sfw[i];
                wave_sync();
                return;
            }
        } else if (st == ST_A) {
            w.part2_3_length = nBits;
            LHIP_SS(if (ss_run == 0 && ss_first_) { int b_ = (huff_bits - ss_prev_bits_) / 8 + 4; b_ = b_ < 0 ? 0 : b_ > 23 ? 23 : b_; if (nBits > huff_bits) ss_.mfail[b_]++; else ss_.mfit[b_]++; } ss_first_ = 0);
            if (nBits > huff_bits && w.global_gain <= maxggain) { LHIP_SS(ss_run++; ss_moved = (pn.sfb_count1 != cnt1_seen)); w.global_gain++; continue; }
            if (w.global_gain > maxggain) break;
            if (best.over_count == 0) {
                // The reference's second loop (Quantize.js:1004-1013) starts by counting again at the SAME gain.  That evaluation
                // has the same inputs as the one just made -- spectrum, gain, scalefactors, the noise cache (only calc_noise
                // writes it) -- except PrevNoise.sfb_count1, which the one just made has rewritten and which steers the 0/1
                // shortcut of quantize_xrpow.  If it was rewritten with the value it had, the second evaluation is the first
                // one again (same bits, same assignments, same spectrum) and is not made.
                st = ST_B;
                if (pn.sfb_count1 != cnt1_seen) continue;
                if (nBits > best_part2_3_length && w.global_gain <= maxggain) { LHIP_SS(ss_run++; ss_moved = (pn.sfb_count1 != cnt1_seen)); w.global_gain++; continue; }
                if (w.global_gain > maxggain) break;
            }
        } else {   // ST_B
            w.part2_3_length = nBits;
            if (nBits > best_part2_3_length && w.global_gain <= maxggain) { LHIP_SS(ss_run++; ss_moved = (pn.sfb_count1 != cnt1_seen)); w.global_gain++; continue; }
            if (w.global_gain > maxggain) break;
        }
        LHIP_SS(if (st >= ST_A) { ss_.rounds++; ss_.run[ss_run < 39 ? ss_run : 39]++; }  ss_run = 0; ss_moved = 0);
        if (spec) { q_noise_commit(w, nc, pn, lane, L); LHIP_PIPE_COUNT(committed); }          // made beside the count, on exactly these inputs: now it counts
        else q_calc_noise(T, w, L.sfw, L.ixw, &ni, 1, pn, best.over_count == 0, lane, L, Q);                 // the only call site
        ni.bits = w.part2_3_length;
        int keep;
        if (first) keep = 1;
        else keep = q_quant_compare(best, ni);
        if (keep) {
            if (!first) best_part2_3_length = kept_p23;           // value BEFORE the copy (reference quirk)
            best = ni;
            gi_keep_store(L, w, lane);                            // cod_info = cod_info_w
            kept_p23 = w.part2_3_length;
            for (int i = lane; i < 288; i += LHIP_NL) ((uint32_t*)kept)[i] = ((const uint32_t*)L.ixw)[i];
            LHIP_LANE_ONCE(i, 0, (SFBMAX) + 1) L.sfb[i] = L.sfw[i];
            wave_sync();
            age = 0;
        } else if (T.full_outer_loop == 0) {
            if (++age > search_limit && best.over_count == 0) break;
        }
        if (!first && !((w.global_gain + w.scalefac_scale) < 255)) break;
        first = 0;
        int bal_;
        { PH_BEGIN(); bal_ = q_balance_noise<SKIP>(T, w, L.sfw, lane, L, Q); PH_END(L, PH_BALANCE); }       // the only call site
        if (!bal_) break;
        maxggain = (w.scalefac_scale != 0) ? 254 : 255;
        huff_bits = targ_bits - w.part2_length;
        if (huff_bits <= 0) break;
        LHIP_SS(ss_first_ = 1; ss_prev_bits_ = w.part2_3_length);
        st = ST_A;
    }
    wave_sync();
    { const GI inv = w; g = inv; gi_keep_load(L, g); }       // the invariant fields are the working copy's, the rest comes back from LDS
}
}  // namespace lhip
