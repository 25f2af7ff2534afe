// k_quant_frame.h -- the programs: q_unit, one granule-channel from the spectrum to its published record (Quantize.js:1406-1466), and kb_quant, a frame
// (CBRNewIterationLoop.js:25-90) with ResvFrameBegin / ResvFrameEnd (Reservoir.js:130-180, 243-293).
#pragma once
#include "k_quant_search.h"
#include "k_quant_framebits.h"
#include "k_quant_finish.h"
#include "k_quant_budget.h"
namespace lhip {
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
}  // namespace lhip
