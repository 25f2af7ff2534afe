// k_quant_helper.h -- count_bits on a second wave (latency kernels): the hand-over record CountShare, the helper's loop (q_count_helper) and
// the owner's side (q_count_bits_piped), which runs calc_noise speculatively beside the count.
#pragma once
#include "k_quant_noise.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// count_bits on a second wave (latency kernels: a workgroup per frame with idle waves -- g_frame).
// One evaluation of the outer loop is  quantize -> count_bits -> [fits?] -> calc_noise  and calc_noise needs the quantized values but
// nothing count_bits produces.  So the owner of a granule-channel quantizes, hands the Huffman count of that quantization (noquant_count_bits,
// Takehiro.js:521-628: a pure function of the quantized values, the block type and the region fields it may leave untouched) to a
// helper wave through a record in LDS, and runs calc_noise itself MEANWHILE -- speculatively: its cache writes are held back
// (NoiseCommit) until the count is in and the loop's decisions say that this evaluation is the one calc_noise follows
// (Quantize.js:986-1018); otherwise the result is dropped and nothing of it remains (calc_noise's other outputs -- distort, the band sums
// -- are rewritten by the next call before anybody reads them).  Same values, same order of the reference's decisions; only the clock changes.
// CountShare::state: CS_REQ request posted (owner), CS_DONE reply posted (helper), CS_BARRIER the owner is about to wait at a workgroup
// barrier and the helper must keep the count, CS_QUIT the owner's frame is finished.
// ---------------------------------------------------------------------------------------------
// The hand-over is on the search's critical path, so it is three LDS words each way: the request is the state word itself (CS_REQ | block
// type << 8 -- the count reads nothing else of the granule's state: the quantized values are in the owner's record), the reply packs what
// noquant_count_bits assigns (w[0] bits | count1 << 17; w[1] big_values | count1bits << 10 | count1table_select << 23 | region0_count << 24 |
// region1_count << 28; w[2] table_select[0..2] + 1 at 6 bits each | sfb_count1 << 18 | the mask of conditionally assigned fields << 24: the
// owner takes the region counts and table_select[r] only where the reference's count assigns them, Takehiro.js:566-612).
struct CountShare { int state; uint32_t w[3];
    int16_t kept[576];          // the search's kept copy of the quantized spectrum (q_outer_loop's `kept`): in LDS where a wave is alone with its memory latencies
                                // (the batched kernel keeps it in HBM -- the granule-channel's slot of W.l3 -- and reads it back once per search)
#if defined(LHIP_PHASE_PROF) || defined(LHIP_HANDOFF_PROF)
    unsigned long long t_post, t_reply; unsigned int acc[8];      // profiling builds: the hand-over's legs (q_count_helper)
#endif
};

enum { CS_IDLE = 0, CS_REQ = 1, CS_DONE = 2, CS_BARRIER = 8, CS_QUIT = 9 };

#if LHIP_NL != 1
// the helper: serves one owner's requests until it is told to leave.  Lo = the owner's LDS record (the quantized values), L = this wave's own (scratch).
LHIP_DEV void q_count_helper(const Tables& T, CountShare& cs, const QuantLds& Lo, QuantLds& L, const QuantTabs& Q, int lane) {
    for (;;) {
        const int s = wg_wait_not(&cs.state, CS_IDLE, CS_DONE, lane);       // a request, a barrier to keep, or the end
        if (s == CS_QUIT) break;
        if (s == CS_BARRIER) { wg_store(&cs.state, CS_IDLE, lane); wg_barrier(); continue; }     // (the owner posts again only after the barrier)
#ifdef LHIP_PHASE_PROF
        const unsigned long long hp_seen_ = __builtin_amdgcn_s_memtime();
#endif
#if HO_ON
        const unsigned long long ho_h0_ = HO_NOW();
#endif
        wg_acquire();
        lane = lane_anew(lane);
        GI g;
        g.block_type = uni(s >> 8); g.max_nonzero_coeff = 0;
        g.region0_count = 0; g.region1_count = 0; g.table_select[0] = g.table_select[1] = g.table_select[2] = 0;
        g.count1table_select = 0; g.count1bits = 0; g.count1 = 0; g.big_values = 0;
        int cnt1 = 0, amask = 0;
        int vx[NPL], vy[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = lane + LHIP_NL * j;
            const uint32_t w = i < 288 ? ((const uint32_t*)Lo.ixw)[i] : 0u;
            vx[j] = (int)(w & 0xffffu); vy[j] = (int)(w >> 16);
        }
#ifdef LHIP_PHASE_PROF
        const unsigned long long hp_start_ = __builtin_amdgcn_s_memtime();
#endif
        const int bits = uni(q_noquant_count_bits<NPL>(T, g, Lo.ixw, vx, vy, 1, &cnt1, &amask, lane, L, Q));
#ifdef LHIP_PHASE_PROF
        const unsigned long long hp_end_ = __builtin_amdgcn_s_memtime();
#endif
        uni_gi(g);
        const uint32_t w0 = (uint32_t)bits | ((uint32_t)g.count1 << 17);
        const uint32_t w1 = (uint32_t)g.big_values | ((uint32_t)g.count1bits << 10) | ((uint32_t)g.count1table_select << 23) | ((uint32_t)g.region0_count << 24) | ((uint32_t)g.region1_count << 28);
        const uint32_t w2 = (uint32_t)(g.table_select[0] + 1) | ((uint32_t)(g.table_select[1] + 1) << 6) | ((uint32_t)(g.table_select[2] + 1) << 12) | ((uint32_t)uni(cnt1) << 18) | ((uint32_t)uni(amask) << 24);
        if (lane == 0) { cs.w[0] = w0; cs.w[1] = w1; cs.w[2] = w2; }
#ifdef LHIP_PHASE_PROF
        if (lane == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); cs.acc[0] += (unsigned int)(hp_seen_ - cs.t_post); cs.acc[1] += (unsigned int)(hp_start_ - hp_seen_);
                         cs.acc[2] += (unsigned int)(hp_end_ - hp_start_); cs.acc[3] += (unsigned int)(now_ - hp_end_); cs.acc[7] += 1; cs.t_reply = now_; }
#endif
#if HO_ON
        const unsigned long long ho_h1_ = HO_NOW();
        if (lane == 0) cs.t_reply = ho_h1_;
#endif
        wg_store(&cs.state, CS_DONE, lane);
#if HO_ON
        HO_ADD(cs, 3, ho_h1_ - ho_h0_); HO_ADD(cs, 4, 1); HO_ADD(cs, 5, ho_h0_ - cs.t_post);
#endif
    }
}
// the owner's side: q_count_bits (use_pn = 1) with the count on the helper and calc_noise run beside it.  *spec = 1: `ni` / `nc` hold a calc_noise
// of this quantization that has not been committed (q_noise_commit)
LHIP_DEV int q_count_bits_piped(const Tables& T, GI& g, const int32_t* scalefac, int16_t* ix, PrevNoise& pn, int* asg, CountShare& cs,
                                NoiseRes* ni, NoiseCommit* nc, int need_max, int* spec, int lane, QuantLds& L, const QuantTabs& Q) {
    *asg = 0; *spec = 0;
    {   // Takehiro.js:635-638 (see q_count_bits)
        const double ip = ipow20(Q, g.global_gain);
        if (g.xrpow_max * ip > (double)IXMAX_VAL * (1.0 - 0x1p-50)) {
            const double w = (double)IXMAX_VAL / ip;
            if (g.xrpow_max > w) return LARGE_BITS;
        }
    }
    {
        int vx[NPL], vy[NPL];
        PH_BEGIN(); q_quantize<NPL>(T, g, scalefac, ix, 1, pn.gain, pn.sfb_count1, vx, vy, lane, L, Q); PH_END(L, PH_QUANTIZE);
        (void)vx; (void)vy;                          // the helper reads the pairs back from LDS
    }
#ifdef LHIP_PHASE_PROF
    if (lane == 0) cs.t_post = __builtin_amdgcn_s_memtime();
#endif
#if HO_ON
    const unsigned long long ho_t0_ = HO_NOW();
    if (lane == 0) cs.t_post = ho_t0_;
#endif
    wg_store(&cs.state, CS_REQ | (g.block_type << 8), lane);
    LHIP_PIPE_COUNT(piped);
    { PH_BEGIN(); q_calc_noise_(T, g, scalefac, ix, ni, 1, pn, need_max, lane, L, Q, nc); PH_END(L, PH_NOISE); }
    *spec = 1;
#if HO_ON
    const unsigned long long ho_t1_ = HO_NOW();
#endif
    PH_BEGIN();
#ifdef LHIP_PHASE_PROF
    const unsigned long long op_wait0_ = __builtin_amdgcn_s_memtime();
#endif
    (void)wg_wait_not(&cs.state, CS_REQ | (g.block_type << 8), CS_REQ | (g.block_type << 8), lane);       // the only thing it can become is CS_DONE
#ifdef LHIP_PHASE_PROF
    if (lane == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); cs.acc[4] += (unsigned int)(now_ - cs.t_reply); cs.acc[5] += (unsigned int)(op_wait0_ - cs.t_post); cs.acc[6] += (unsigned int)(now_ - op_wait0_); }
#endif
#if HO_ON
    const unsigned long long ho_t2_ = HO_NOW();
#endif
    wg_acquire();
    const uint32_t w0 = (uint32_t)uni((int)cs.w[0]), w1 = (uint32_t)uni((int)cs.w[1]), w2 = (uint32_t)uni((int)cs.w[2]);
#if HO_ON
    HO_ADD(cs, 0, ho_t1_ - ho_t0_); HO_ADD(cs, 1, ho_t2_ - ho_t1_); HO_ADD(cs, 2, 1); HO_ADD(cs, 6, ho_t2_ - cs.t_reply);
#endif
    const int bits = (int)(w0 & 0x1ffffu), amask = (int)((w2 >> 24) & 15u);
    static_assert(LARGE_BITS < (1 << 17), "the reply packs the bit count in 17 bits");
    g.count1 = (int)(w0 >> 17); g.big_values = (int)(w1 & 1023u); g.count1bits = (int)((w1 >> 10) & 0x1fffu); g.count1table_select = (int)((w1 >> 23) & 1u);
    if (amask & 8) { g.region0_count = (int)((w1 >> 24) & 15u); g.region1_count = (int)(w1 >> 28); }       // (region1_count is 13 for start / stop blocks: four bits)
    if (amask & 1) g.table_select[0] = (int)(w2 & 63u) - 1;
    if (amask & 2) g.table_select[1] = (int)((w2 >> 6) & 63u) - 1;
    if (amask & 4) g.table_select[2] = (int)((w2 >> 12) & 63u) - 1;
    *asg = pack_cond_fields(g, amask);
    pn.sfb_count1 = (int)((w2 >> 18) & 63u);
    PH_END(L, PH_COUNT);                             // (profiling builds: the part of the count the owner still had to wait for)
    return bits;
}
#endif
}  // namespace lhip
