// k_quant_validate.h -- the seed-chain validation: the bin search of bin_search_StepSize (Quantize.js:322-381) replayed with the chain-implied seed, from the
// side records with re-quantization on a memo miss (kb_validate) and from the digests alone (kb_validate_fast, kb_validate_fast_quad).
#pragma once
#include "k_quant_search.h"
#include "k_quant_budget.h"
namespace lhip {
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
    const Seed s = seed_before<&Workspace::vdig>(W, sd, C, k, gr, ch);
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
