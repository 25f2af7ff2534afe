// k_psy_scan.h -- the four per-stream scans between psyA and psyB: raw attack flags, attack clean-up and the block-type chain (PsyModel.js:1105-1204, 784-826)
// and the ATH auto-adjust recurrence (Encoder.js:166-243).
#pragma once
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
namespace lhip {
// ---------------------------------------------------------------------------------------------
// kb_scan: one wave per stream.  Phase 1 (parallel): raw attack flags per (psy call, channel).
// Phase 2 (lane 0): attack clean-up / block-type chain and the ATH auto-adjust recurrence.
// ---------------------------------------------------------------------------------------------
LHIP_DEV int attack_flags_raw(const Tables& T, const float* cur, const float* prev, int chn) {
    // PsyModel.js:1105-1181 under the fractional-index port bug: only i in {0,3,6,9}
    const double thr = (chn == 3) ? T.attackthre_s : T.attackthre;
    float ai[4];
    ai[0] = (float)((double)prev[6] / (double)prev[4]);
    const double refv[3] = {(double)prev[7], (double)cur[1], (double)cur[4]};
    for (int t = 0; t < 3; t++) {
        double p = cur[3 * t];
        const double r = refv[t];
        if (p > r) p = p / r;
        else if (r > p * 10.0) p = r / (p * 10.0);
        else p = 0.0;
        ai[t + 1] = (float)p;
    }
    double en_short[4];
    en_short[0] = 0.0;
    for (int i = 0; i < 3; i++) en_short[0] += (double)prev[i + 6];
    en_short[1] = 0.0 + (double)cur[0]; en_short[2] = 0.0 + (double)cur[3]; en_short[3] = 0.0 + (double)cur[6];
    int a[4];
    for (int j = 0; j < 4; j++) a[j] = ((double)ai[j] > thr) ? 1 : 0;
    for (int i = 1; i < 4; i++) {
        double ratio;
        if (en_short[i - 1] > en_short[i]) ratio = en_short[i - 1] / en_short[i];
        else ratio = en_short[i] / en_short[i - 1];
        if (ratio < 1.7) { a[i] = 0; if (i == 1) a[0] = 0; }
    }
    return a[0] | (a[1] << 1) | (a[2] << 2) | (a[3] << 3);
}

// raw attack flags of one psy call, all channels (parallel over granule slots)
LHIP_DEV void kb_scan_raw(const Tables& T, const Workspace& W, const StreamDesc* SD, int gslot) {
    const int Cp = T.psy_channels;
    const StreamDesc sd = SD[W.gslot_stream[gslot]];
    if (gslot - sd.gslot0 - 1 < 0) return;
    for (int ch = 0; ch < Cp; ch++) {
        const int64_t o = (int64_t)gslot * Cp + ch;
        W.att_raw[o] = attack_flags_raw(T, W.peaks + o * PK_STRIDE, W.peaks + (o - Cp) * PK_STRIDE, ch);
    }
}

// lastAttacks after the psy call in `gslot` (PsyModel.js:1183-1196, 1268), resolved by looking back:
// a0' = a0 & !last, a1' = a1 & !a0', a2' = a2 & !a1'  ->  the value only depends on the previous call
// when a0 = a1 = a2 = 1, so the walk almost always stops at once.
LHIP_DEV int last_attack_after(const Workspace& W, int C, int gcarry, int gslot, int ch) {
    int flips = 0, g = gslot;
    for (;;) {
        if (g == gcarry) { const int v = W.last_attack[(int64_t)g * C + ch] != 0; return flips ? !v : v; }
        const int raw = W.att_raw[(int64_t)g * C + ch];
        const int a0 = raw & 1, a1 = (raw >> 1) & 1, a2 = (raw >> 2) & 1;
        int v;
        if (!a2) v = 0;
        else if (!a1) v = 1;
        else if (!a0) v = 0;
        else { flips ^= 1; g--; continue; }        // a2' = !last(g-1)
        return flips ? !v : v;
    }
}

// per granule slot: attack clean-up -> uselongblock (coupled), lastAttacks (parallel over granule slots)
LHIP_DEV void kb_scan_attack(const Tables& T, const Workspace& W, const StreamDesc* SD, int gslot) {
    const int C = T.channels_out, Cp = T.psy_channels;
    const StreamDesc sd = SD[W.gslot_stream[gslot]];
    if (gslot - sd.gslot0 - 1 < 0) return;
    int ul[2] = {1, 1};
    for (int ch = 0; ch < Cp; ch++) {
        const int last = last_attack_after(W, Cp, sd.gslot0, gslot - 1, ch);
        const int raw = W.att_raw[(int64_t)gslot * Cp + ch];
        int a0 = raw & 1, a1 = (raw >> 1) & 1, a2 = (raw >> 2) & 1, a3 = (raw >> 3) & 1;
        if (a0 != 0 && last != 0) a0 = 0;
        if ((a0 + a1 + a2 + a3) != 0) {            // lastAttacks == 3 never happens
            if (ch < 2) ul[ch] = 0;
            else ul[0] = ul[1] = 0;                 // an attack in mid or side switches both channels (PsyModel.js:1198-1204)
            if (a1 != 0 && a0 != 0) a1 = 0;
            if (a2 != 0 && a1 != 0) a2 = 0;
            if (a3 != 0 && a2 != 0) a3 = 0;
        }
        W.att_clean[(int64_t)gslot * Cp + ch] = a0 | (a1 << 1) | (a2 << 2) | (a3 << 3);
        W.ul_tmp[(int64_t)gslot * Cp + ch] = a2;   // lastAttacks after this call (published below)
    }
    if (T.short_blocks_coupled && !(ul[0] != 0 && ul[1] != 0)) ul[0] = ul[1] = 0;
    for (int ch = 0; ch < C; ch++) W.uselong[(int64_t)gslot * C + ch] = ul[ch];
}

// per granule slot: block_type_set chain from the (coupled) uselongblock flags of this and the two
// previous calls (PsyModel.js:784-826) (parallel over granule slots)
LHIP_DEV void kb_scan_blocktype(const Tables& T, const Workspace& W, const StreamDesc* SD, int gslot) {
    const int C = T.channels_out;
    const StreamDesc sd = SD[W.gslot_stream[gslot]];
    const int q = gslot - sd.gslot0 - 1;
    if (q < 0) return;
    for (int ch = 0; ch < C; ch++) {
        // tentative type left by the previous call
        int old;
        if (q == 0) old = W.tent[(int64_t)sd.gslot0 * C + ch];
        else {
            const int ul1 = W.uselong[(int64_t)(gslot - 1) * C + ch];
            int pshort;
            if (q == 1) pshort = W.tent[(int64_t)sd.gslot0 * C + ch] == SHORT_TYPE;
            else pshort = W.uselong[(int64_t)(gslot - 2) * C + ch] == 0;
            old = ul1 ? (pshort ? STOP_TYPE : NORM_TYPE) : SHORT_TYPE;
        }
        const int ul = W.uselong[(int64_t)gslot * C + ch];
        W.prev_short[(int64_t)gslot * C + ch] = (old == SHORT_TYPE) ? 1 : 0;
        int bt = NORM_TYPE;
        if (ul != 0) { if (old == SHORT_TYPE) bt = STOP_TYPE; }
        else {
            bt = SHORT_TYPE;
            if (old == NORM_TYPE) old = START_TYPE;
            if (old == STOP_TYPE) old = SHORT_TYPE;
        }
        W.blocktype[(int64_t)gslot * C + ch] = old;
        W.tent[(int64_t)gslot * C + ch] = bt;
    }
    const int Cp = T.psy_channels;
    for (int ch = 0; ch < Cp; ch++) W.last_attack[(int64_t)gslot * Cp + ch] = W.ul_tmp[(int64_t)gslot * Cp + ch];
}

// ATH auto-adjust recurrence (Encoder.js:166-243), one 1024-thread workgroup per stream.
// The recurrence (adjust, adjustLimit) <- F_k(adjust, adjustLimit) is serial in general (repeated f64
// multiplications during a loudness descent cannot be re-associated), but two consecutive "loud" frames
// (max_pow > 0.03125) force the state to (1, 1) whatever came before.  Frames are processed in chunks of
// ATH_NT x ATH_SEG; inside a chunk every thread owns a contiguous segment: pass A evaluates each segment from its
// first such reset point onwards (no dependence on other threads), then the segment prefixes are filled in
// as soon as the state at the end of the previous segment is known (at most ATH_NT rounds, 1 in the common case).
// Nothing but the segment end states is staged: max_pow is recomputed from the per-granule loudness (L2-resident).
#if defined(LHIP_HOSTSIM) && defined(LHIP_WAVESIM)
// TEST-ONLY: the wave simulator runs the scan as a workgroup of two waves with two-frame segments, so that a few hundred frames walk
// through several chunks, multi-frame segments, reset points, prefix rounds and the chunk carry (the device: 1024 threads x 16)
enum { ATH_NT = 128, ATH_SEG = 2 };
LHIP_DEV void block_sync() { wg_barrier(); }
LHIP_DEV int block_any(int p) { static int any_ = 0; wg_barrier(); if (p) any_ = 1; wg_barrier(); const int r = any_; wg_barrier(); any_ = 0; return r; }
#elif defined(LHIP_HOSTSIM)
enum { ATH_NT = 1, ATH_SEG = 1 << 20 };
LHIP_DEV void block_sync() {}
LHIP_DEV int block_any(int p) { return p != 0; }
#else
enum { ATH_NT = 1024, ATH_SEG = 16 };
LHIP_DEV void block_sync() { __syncthreads(); }
LHIP_DEV int block_any(int p) { return __syncthreads_or(p); }
#endif
struct AthLds { double e_adj[ATH_NT + 1], e_lim[ATH_NT + 1]; int known[ATH_NT + 1], first_reset[ATH_NT + 1]; double c_adj, c_lim, c_mp; };

LHIP_DEV void ath_step(const Tables& T, double max_pow, double& adj, double& lim) {
    if (T.ATH_useAdjust == 0) { adj = 1.0; return; }
    if (max_pow > 0.03125) {
        if (adj >= 1.0) adj = 1.0;
        else if (adj < lim) adj = lim;
        lim = 1.0;
    } else {
        const double adj_lim_new = 31.98 * max_pow + 0.000625;
        if (adj >= adj_lim_new) {
            adj *= adj_lim_new * 0.075 + 0.925;
            if (adj < adj_lim_new) adj = adj_lim_new;
        } else {
            if (lim >= adj_lim_new) adj = adj_lim_new;
            else if (adj < lim) adj = lim;
        }
        lim = adj_lim_new;
    }
}

// max_pow of frame k of the stream (Encoder.js:420-440): loudness of the two psy calls before the frame's granules
LHIP_DEV double ath_max_pow(const Tables& T, const Workspace& W, const StreamDesc& sd, int C, int k) {
    const int GR = T.mode_gr;
    const int64_t g0 = (int64_t)(sd.gslot0 + GR * k) * C, g1 = g0 + C;
    double max_pow = W.loud[g0], gr2_max = (GR == 2) ? (double)W.loud[g1] : 0.0;
    if (C == 2) { max_pow += (double)W.loud[g0 + 1]; if (GR == 2) gr2_max += (double)W.loud[g1 + 1]; }
    else { max_pow += max_pow; gr2_max += gr2_max; }
    if (GR == 2) max_pow = max_pow > gr2_max ? max_pow : gr2_max;      // Encoder.js:187-189: only with two granules
    max_pow *= 0.5;
    max_pow *= T.ATH_aaSensitivityP;
    return max_pow;
}

LHIP_DEV void kb_scan_ath(const Tables& T, const Workspace& W, const StreamDesc* SD, int st, int tid, AthLds& L) {
    const int C = T.channels_out;
    const StreamDesc sd = SD[st];
    if (tid == 0) { L.c_adj = W.ath_adjust[sd.fslot0]; L.c_lim = W.ath_limit[sd.fslot0]; L.c_mp = 0.0; }   // state carried into the chunk; 0: previous frame unknown / not loud
    block_sync();
    for (int k0 = 0; k0 < sd.nframes; k0 += ATH_NT * ATH_SEG) {
        const int rem = sd.nframes - k0;
        const int n = rem < ATH_NT * ATH_SEG ? rem : ATH_NT * ATH_SEG;
        const int seglen = (n + ATH_NT - 1) / ATH_NT;
        const int s0 = tid * seglen < n ? tid * seglen : n, s1 = (tid + 1) * seglen < n ? (tid + 1) * seglen : n;
        const double cadj = L.c_adj, clim = L.c_lim, prev_mp = L.c_mp;
        // pass A: from the first reset point of the segment to its end
        {
            int fr = -1;
            if (T.ATH_useAdjust != 0) {
                double pm = (s0 < s1) ? (s0 > 0 ? ath_max_pow(T, W, sd, C, k0 + s0 - 1) : prev_mp) : 0.0;
                for (int k = s0; k < s1; k++) {
                    const double m = ath_max_pow(T, W, sd, C, k0 + k);
                    if (pm > 0.03125 && m > 0.03125) { fr = k; break; }
                    pm = m;
                }
            } else if (s0 < s1) fr = s0;
            double a = 1.0, l = 1.0;
            if (fr >= 0) {
                l = (T.ATH_useAdjust != 0) ? 1.0 : clim;
                W.ath_adjust[sd.fslot0 + 1 + k0 + fr] = 1.0; W.ath_limit[sd.fslot0 + 1 + k0 + fr] = l;
                for (int k = fr + 1; k < s1; k++) {
                    ath_step(T, ath_max_pow(T, W, sd, C, k0 + k), a, l);
                    W.ath_adjust[sd.fslot0 + 1 + k0 + k] = a; W.ath_limit[sd.fslot0 + 1 + k0 + k] = l;
                }
            }
            L.first_reset[tid] = fr;
            L.known[tid + 1] = (fr >= 0) || (s0 >= s1);      // empty segments are all at the tail: nobody waits for their state
                                                             // (forwarding it one thread per round cost a 1-frame call 1023 rounds)
            L.e_adj[tid + 1] = a; L.e_lim[tid + 1] = l;
            if (tid == 0) { L.known[0] = 1; L.e_adj[0] = cadj; L.e_lim[0] = clim; }
        }
        block_sync();
        // prefix rounds: a segment's frames before its first reset need the state at the end of the previous segment
        int done = (s0 >= s1);
        for (int round = 0; round < ATH_NT + 1; round++) {
            int progressed = 0;
            if (!done && L.known[tid]) {
                double a = L.e_adj[tid], l = L.e_lim[tid];
                const int fr = L.first_reset[tid];
                const int stop = fr >= 0 ? fr : s1;
                for (int k = s0; k < stop; k++) {
                    ath_step(T, ath_max_pow(T, W, sd, C, k0 + k), a, l);
                    W.ath_adjust[sd.fslot0 + 1 + k0 + k] = a; W.ath_limit[sd.fslot0 + 1 + k0 + k] = l;
                }
                if (fr < 0) { L.e_adj[tid + 1] = a; L.e_lim[tid + 1] = l; }
                done = 1; progressed = 1;
            }
            block_sync();
            if (progressed && L.first_reset[tid] < 0) L.known[tid + 1] = 1;
            // empty segments simply forward the state
            if (s0 >= s1 && L.known[tid] && !L.known[tid + 1]) { L.e_adj[tid + 1] = L.e_adj[tid]; L.e_lim[tid + 1] = L.e_lim[tid]; L.known[tid + 1] = 1; }
            block_sync();
            if (!block_any(!done || !L.known[tid + 1])) break;
        }
        // carry: state after the last frame of the chunk = end state of the last non-empty segment
        if (s0 < s1 && s1 == n) { L.c_adj = L.e_adj[tid + 1]; L.c_lim = L.e_lim[tid + 1]; L.c_mp = ath_max_pow(T, W, sd, C, k0 + n - 1); }
        block_sync();
    }
}
}  // namespace lhip
