// k_psy_a.h -- kb_psyA, everything of L3psycho_anal_ns that is a pure function of the PCM window (PsyModel.js:241-319, 906-992, 1051-1121; FFT.js:185-221), with its LDS
// record, the PSY_* profiling macros and what decides whether a granule needs its short-block or its transform part (psy_need_s / psy_need_f).
#pragma once
#include <type_traits>
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
#include "k_psy_fht.h"
namespace lhip {
// LDS of one psy-A wave.  The energies overwrite the lower halves of the FHT buffers they are computed from
// (fe = fz[0..512], fes[b] = fs[b][0..128]) and the partition arrays live in the then-dead upper half of fz:
// 7.2 KB instead of 12.3 KB per wave, i.e. LDS no longer caps the kernel at 3 waves per SIMD.
struct PsyALds {
    float fz[BLKSIZE + BLKSIZE / 32];              // long FHT buffer (padded layout, fzp); after the energies: [0..512] fe, [516..] eb/mx/av/ebs
    float fs[3][BLKSIZE_s];                        // short FHT buffers: one padded buffer of 3 x 256 points (fzp over the flat index b * 256 + j) ...
    float fs_pad[3 * BLKSIZE_s / 32];              // ... which therefore extends into this; after the energies: fs[b][0..128] = fes
};
static_assert(offsetof(PsyALds, fs_pad) == offsetof(PsyALds, fs) + sizeof(float) * 3 * BLKSIZE_s, "the short transform buffer is one flat padded array");
#define PSYA_FE(L) ((L).fz)
#define PSYA_FES(L, b) ((L).fs[b])
#define PSYA_EB(L) ((L).fz + 516)
#define PSYA_MX(L) ((L).fz + 516 + CBANDS)
#define PSYA_AV(L) ((L).fz + 516 + 2 * CBANDS)
#define PSYA_EBS(L, b) ((L).fz + 516 + (3 + (b)) * CBANDS)

#if defined(LHIP_PHASE_PROF) && !defined(LHIP_HOSTSIM)
#define PSY_STAMP(i) psy_t_[i] = __builtin_amdgcn_s_memtime()      /* stamp 2 sits inside the `ch < 2` branch: the mid / side waves keep stamp 1's time there */
#define PSY_FLUSH() do { if (lane == 0 && ((gslot & 63) == 0 || (W.ngslots <= 4 && ch == 0 && gslot - sd.gslot0 == 1))) {   /* a sample of the waves: a flush per wave congests what it measures */ if (psy_t_[2] == 0) psy_t_[2] = psy_t_[1]; \
    for (int i_ = 0; i_ < 7; i_++) atomicAdd((unsigned long long*)W.prof + 22 + i_, psy_t_[i_ + 1] - psy_t_[i_]); atomicAdd((unsigned long long*)W.prof + 54, 1ull); } } while (0)
#define PSY_DECL() unsigned long long psy_t_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#else
#define PSY_STAMP(i) do {} while (0)
#define PSY_FLUSH() do {} while (0)
#define PSY_DECL() do {} while (0)
#endif
// (float)((sum of the LHIP_NL * K non-negative values, lane l holding [l K, (l + 1) K)) * scale + add) when that Float32 does not depend
// on the order of the additions: *out is set and 1 returned if both ends of the error band of an any-order sum round to the same
// Float32 (wave-uniform verdict); 0: the caller must form the sum in the reference's order.  scale > 0, add >= 0.
template <int K> LHIP_DEV int guarded_f32_of_sum(const double (&p)[K], double scale, double add, float* out) {
#if LHIP_NL == 1
    (void)p; (void)scale; (void)add; (void)out;
    return 0;                                         // the one-lane build always takes the sequential sum
#else
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) s += p[k];
    s = wave_sumd(s);
    // any-order sum vs the reference's sequential one: both within (n - 1) u (n = 512, u = 2^-53) of the exact sum, then one rounding
    // each for `* scale` and `+ add` on either side: 2e-13 covers it with a margin of 1.7
    const float lo = (float)((s * (1.0 - 2e-13)) * scale + add), hi = (float)((s * (1.0 + 2e-13)) * scale + add);
    *out = lo;
#ifdef LHIP_WAVESIM
    if (lo == hi) {       // the simulation checks the claim on everything it encodes: the guarded value IS the sequential sum's
        const float ref = (float)(wave_seq_sum<K>(p) * scale + add);
        if (ref != lo) { fprintf(stderr, "wavesim: guarded_f32_of_sum disagrees with the sequential sum (%a vs %a)\n", (double)lo, (double)ref); abort(); }
    }
#endif
    return lo == hi;
#endif
}

// Who reads the short-block side of the psy call in granule slot `gslot` (both wave-uniform; W.blocktype must be final: behind g_scan_blocktype).
// Its short thresholds (E_EN_S / E_THM_S of W.E[gslot]) are read by the quantization of slot gslot + 1 -- q_calc_xmin for a SHORT_TYPE granule, q_frame_pe
// for L / R of that type and for mid / side when either channel has it -- and, for the stream's last call of the batch, by a later batch through the stream
// state (kb_save): psy_need_s.  Taking the OR over the channels also covers the inter-channel masking and the mid / side thresholds, which mix the channels.
// Its short spectra up to ecb_s are read by its own short limiting and by the next call's (the two previous sub-blocks): psy_need_f.
// Neither holds with the bit reservoir, whose short pre-echo control reads the previous call's thresholds whatever the block type.
LHIP_DEV int psy_need_s(const Tables& T, const Workspace& W, const StreamDesc& sd, int gslot) {
    if (gslot >= sd.gslot0 + T.mode_gr * sd.nframes) return 1;
    const int C = T.channels_out;
    int s = 0;
    for (int ch = 0; ch < C; ch++) s |= W.blocktype[(int64_t)(gslot + 1) * C + ch] == SHORT_TYPE;
    return uni(s);
}
LHIP_DEV int psy_need_f(const Tables& T, const Workspace& W, const StreamDesc& sd, int gslot) {
    if (psy_need_s(T, W, sd, gslot)) return 1;
    return psy_need_s(T, W, sd, gslot + 1);             // (not the last slot of its stream, or the line above had returned)
}

// kb_psyA's staging of a window that lies wholly in the call's new samples, per sample format (F32: Float32 / Int16; UNIT: stride 1 known
// at compile time -- <0, 1, 0> is the Int16 planar loop as it always was) and per input treatment (MIX: PcmSrc::mix -- 1 the channel's own gain
// follows `scale`, 2 downmix).  The downmix instance is unrolled by hand: the trip count (16) is known, and left as one load per source and
// trip each trip would wait out two memory latencies -- eight loads in flight per source instead
template <int F32, int UNIT, int MIX>
LHIP_DEV void psya_stage_new(const PcmSrc& P, int first, int lane, float* fz) {
    typedef typename std::conditional<F32 != 0, float, int16_t>::type elem_t;
    const int str = UNIT ? 1 : P.stride;
    const elem_t* src = (const elem_t*)P.src + (int64_t)first * str;
    if (MIX == 2) {
        const elem_t* src2 = (const elem_t*)P.src2 + (int64_t)first * str;
        enum { STG = 8 };
        for (int i0 = lane; i0 < BLKSIZE; i0 += LHIP_NL * STG) {
            typename std::conditional<F32 != 0, float, int>::type ra[STG], rb[STG];
#pragma unroll
            for (int k = 0; k < STG; k++) {
                int i = i0 + LHIP_NL * k;
                if (i >= BLKSIZE) i = BLKSIZE - 1;                // (one lane: the last trips of the scalar build; never on a 64-lane wave)
                ra[k] = src[i * str]; rb[k] = src2[i * str];
            }
#pragma unroll
            for (int k = 0; k < STG; k++) { LHIP_PIN_LOADED(ra[k]); LHIP_PIN_LOADED(rb[k]); }
#pragma unroll
            for (int k = 0; k < STG; k++) {
                const int i = i0 + LHIP_NL * k;
                float v = F32 ? pcm_f32_clean((float)ra[k], P.limit) : (float)ra[k];
                if (P.do_scale) v = (float)((double)v * P.scale);
                v = pcm_mix(P, v, F32 ? pcm_f32_clean((float)rb[k], P.limit) : (float)rb[k]);
                if (i < BLKSIZE) fz[i] = v;
            }
        }
        return;
    }
    for (int i = lane; i < BLKSIZE; i += LHIP_NL) {
        float v = F32 ? pcm_f32_clean((float)src[i * str], P.limit) : (float)src[i * str];
        if (P.do_scale) v = (float)((double)v * P.scale);
        if (MIX) v = pcm_mix(P, v, 0.f);
        fz[i] = v;
    }
}

// one wave per (granule slot >= 1 of a stream, psy channel).  ch = 0, 1: L, R.  Joint stereo adds ch = 2, 3 (mid, side) in a second
// launch: their high-passed samples and their spectra are linear combinations of the L / R ones (PsyModel.js:1113-1121, 258-273),
// which the L / R waves leave in W.hpf / W.fht; everything from the energies on is the same code for all four.
// PART (one-frame launches, where a wave is alone with its latencies and other waves of the workgroup idle): 1 = only the high-pass + sub-block peaks
// (they need the samples and nothing else, and nothing below needs them), 2 = everything else; 0 = all of it on one wave (the batched kernel);
// 3 = everything else up to the loudness (what the scans and the search of the frame's first granule need), 4 = the rest -- partition energies, tonality,
// short spreading: psyB's inputs -- later, on the same wave and the same LDS record (nothing but LDS carries over).
// LAZY = 1 (batches that run part 1, the scans and then part 2 as launches of their own: the block types are final when part 2 starts): the short-block
// side -- short windowing and transforms, short energies, partitions and spreading, ecb_s / eb_s -- only where psy_need_f says somebody reads it; the
// branches are scalar (the verdict is wave-uniform).  Peaks, loudness and every long-block value do not depend on it.
template <int PART = 0, int LAZY = 0>
LHIP_DEV void kb_psyA(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, int gslot, int ch, int lane, PsyALds& L) {
    static_assert(LAZY == 0 || PART == 2, "the lazy form reads the block types: it exists for part 2 behind the scans only");
    const int C = T.channels_out, Cp = T.psy_channels;
    const int st = W.gslot_stream[gslot];
    const StreamDesc sd = SD[st];
    const int q = gslot - sd.gslot0 - 1;              // local psy call index
    if (q < 0) return;                                // carry slot: nothing to compute
    // The call's 1024-sample window (segment index 576 q + 304 onwards) is converted ONCE into the long FHT buffer: the high-pass,
    // the short windowing and the long windowing all read it from LDS; the long windowing then runs in place (every lane takes its
    // samples into registers before anybody writes).  The caller's Int16 is read coalesced, 2 bytes per sample, exactly once.
    if (PART != 4 && ch < 2) {
        const PcmSrc P = pcm_source(T, W, sd, IO[st], ch);
        const int b0 = 576 * q + 304;
        if (!P.plane && b0 >= P.mf) {
            // the usual case, wave-uniform: the whole window lies in this call's new samples -- no per-sample decisions
            if (!P.mix) {
                if (!P.f32 && P.stride == 1) psya_stage_new<0, 1, 0>(P, b0 - P.mf, lane, L.fz);
                else if (!P.f32) psya_stage_new<0, 0, 0>(P, b0 - P.mf, lane, L.fz);
                else psya_stage_new<1, 0, 0>(P, b0 - P.mf, lane, L.fz);
            } else if (P.mix == 1) {
                if (!P.f32) psya_stage_new<0, 0, 1>(P, b0 - P.mf, lane, L.fz);
                else psya_stage_new<1, 0, 1>(P, b0 - P.mf, lane, L.fz);
            } else {
                if (!P.f32) psya_stage_new<0, 0, 2>(P, b0 - P.mf, lane, L.fz);
                else psya_stage_new<1, 0, 2>(P, b0 - P.mf, lane, L.fz);
            }
        } else {
            for (int i = lane; i < BLKSIZE; i += LHIP_NL) L.fz[i] = pcm_at(P, b0 + i);
        }
        wave_sync();
    }
#define buf(i) L.fz[i]
    const int64_t o = (int64_t)gslot * Cp + ch;
    PSY_DECL();
    PSY_STAMP(0);

    const bool shortw = LAZY ? psy_need_f(T, W, sd, gslot) != 0 : true;      // the short spectra of this call are read (always, in the eager form)
    if (PART == 4) goto psya_tail;
    // --- fs/4 high-pass, 9 sub-block peaks (PsyModel.js:1051-1069, 1122-1132) ---
    if (PART == 0 || PART == 1) {
        const float* fir = L.fz + 397;                // 576 - 350 - 21 + 192
        // Each lane filters NINE CONSECUTIVE outputs: they share 30 input samples, read and widened once (a lane that took
        // output lane + 64 k of each sub-block instead would read 198).  The magnitudes go through LDS (the short FHT buffers are
        // free until the windowing) so that lane l then holds value l of each 64-sample sub-block for the nine wave maxima.
        // Per output the sums are formed exactly as in PsyModel.js:1051-1069 (same operands, same order).
        enum { HO = (576 + LHIP_NL - 1) / LHIP_NL };      // outputs per lane: 9
        float* mag = &L.fs[0][0];
        if (ch >= 2) {
            const float* hl = W.hpf + (int64_t)gslot * 2 * 576;
            for (int i = lane; i < 576; i += LHIP_NL) {
                const double l = hl[i], r = hl[576 + i];
                float v = (ch == 2) ? (float)(l + r) : (float)(l - r);
                mag[i] = v < 0 ? -v : v;
            }
        } else {
            double x[HO + 21];
#pragma unroll
            for (int t = 0; t < HO + 21; t++) { const int n = HO * lane + t; x[t] = (n < 576 + 21) ? (double)fir[n] : 0.0; }
#pragma unroll
            for (int k = 0; k < HO; k++) {
                double sum1 = x[k + 10], sum2 = 0.0;
#pragma unroll
                for (int j = 0; j < 9; j += 2) {
                    sum1 += T.hpf_fircoef[j] * (x[k + j] + x[k + 21 - j]);
                    sum2 += T.hpf_fircoef[j + 1] * (x[k + j + 1] + x[k + 21 - j - 1]);
                }
                float v = (float)(sum1 + sum2);
                if (Cp == 4 && HO * lane + k < 576) W.hpf[((int64_t)gslot * 2 + ch) * 576 + HO * lane + k] = v;
                v = v < 0 ? -v : v;
                if (HO * lane + k < 576) mag[HO * lane + k] = v;
            }
        }
        wave_sync();
        enum { KP = (64 + LHIP_NL - 1) / LHIP_NL };
        float pk[9];
#pragma unroll
        for (int sbk = 0; sbk < 9; sbk++) {
            float m = 1.0f;
            for (int u = 0; u < KP; u++) { const float v = mag[sbk * 64 + lane + LHIP_NL * u]; if (m < v) m = v; }
            pk[sbk] = m;
        }
        wave_sync();                                  // the magnitudes are dead: the short windowing refills L.fs
        {   // nine maxima of values >= 1: IEEE order == integer order of the bit patterns; reduced side by side (one DPP step serves all nine)
            int pb[9];
#pragma unroll
            for (int sbk = 0; sbk < 9; sbk++) __builtin_memcpy(&pb[sbk], &pk[sbk], 4);
            wave_max_n(pb);
#pragma unroll
            for (int sbk = 0; sbk < 9; sbk++) __builtin_memcpy(&pk[sbk], &pb[sbk], 4);
        }
        if (lane == 0) {
#pragma unroll
            for (int sbk = 0; sbk < 9; sbk++) W.peaks[o * PK_STRIDE + sbk] = pk[sbk];
        }
    }
    if (PART == 1) return;

    PSY_STAMP(1);
    if (ch >= 2) {
        // mid / side spectra from the L / R ones (compute_ffts, PsyModel.js:258-273): (l + r) * SQRT2 * 0.5, rounded to f32
        const float* fl = W.fht + (int64_t)gslot * 2 * FHT_STRIDE;
        const int nfht = shortw ? FHT_STRIDE : BLKSIZE;
        for (int i = lane; i < nfht; i += LHIP_NL) {
            const double l = fl[i], r = fl[FHT_STRIDE + i];
            const float v = (ch == 2) ? (float)((l + r) * LHIP_SQRT2 * 0.5) : (float)((l - r) * LHIP_SQRT2 * 0.5);
            if (i < BLKSIZE) L.fz[fzp(i)] = v; else (&L.fs[0][0])[fzp(i - BLKSIZE)] = v;
        }
        wave_sync();
    } else {
    // --- windowing + first radix-4 stage (FFT.js:185-221 long, 140-180 short) ---
    if (shortw) for (int it = lane; it < 3 * (BLKSIZE_s / 8); it += LHIP_NL) {
        const int b = it / (BLKSIZE_s / 8), j = it - b * (BLKSIZE_s / 8);
        const int k = (576 / 3) * (b + 1);
        const int i = T.fft_rv_tbl[j << 2] & 0xff;
        float* x = &L.fs[0][0] + fzp(b * BLKSIZE_s + 4 * j);        // padded layout: x[0..3] stay together, the second group sits 128 + 4 words on
        double f0, f1, f2, f3, w;
        f0 = (double)T.window_s[i] * (double)buf(i + k);
        w = (double)T.window_s[0x7f - i] * (double)buf(i + k + 0x80);
        f1 = f0 - w; f0 = f0 + w;
        f2 = (double)T.window_s[i + 0x40] * (double)buf(i + k + 0x40);
        w = (double)T.window_s[0x3f - i] * (double)buf(i + k + 0xc0);
        f3 = f2 - w; f2 = f2 + w;
        x[0] = (float)(f0 + f2); x[2] = (float)(f0 - f2); x[1] = (float)(f1 + f3); x[3] = (float)(f1 - f3);
        f0 = (double)T.window_s[i + 0x01] * (double)buf(i + k + 0x01);
        w = (double)T.window_s[0x7e - i] * (double)buf(i + k + 0x81);
        f1 = f0 - w; f0 = f0 + w;
        f2 = (double)T.window_s[i + 0x41] * (double)buf(i + k + 0x41);
        w = (double)T.window_s[0x3e - i] * (double)buf(i + k + 0xc1);
        f3 = f2 - w; f2 = f2 + w;
        x[fzo(BLKSIZE_s / 2) + 0] = (float)(f0 + f2); x[fzo(BLKSIZE_s / 2) + 2] = (float)(f0 - f2);
        x[fzo(BLKSIZE_s / 2) + 1] = (float)(f1 + f3); x[fzo(BLKSIZE_s / 2) + 3] = (float)(f1 - f3);
    }
    {   // long window, in place: all samples of the lane's items first, then -- after everybody has read -- the butterflies
        enum { KL = (BLKSIZE / 8 + LHIP_NL - 1) / LHIP_NL };
        float xin[KL][8];
#pragma unroll
        for (int u = 0; u < KL; u++) {
            const int jj = lane + LHIP_NL * u;
            if (jj < BLKSIZE / 8) {
                const int i = T.fft_rv_tbl[jj] & 0xff;
                xin[u][0] = buf(i); xin[u][1] = buf(i + 0x200); xin[u][2] = buf(i + 0x100); xin[u][3] = buf(i + 0x300);
                xin[u][4] = buf(i + 0x001); xin[u][5] = buf(i + 0x201); xin[u][6] = buf(i + 0x101); xin[u][7] = buf(i + 0x301);
            }
        }
        wave_sync();
#pragma unroll
        for (int u = 0; u < KL; u++) {
            const int jj = lane + LHIP_NL * u;
            if (jj < BLKSIZE / 8) {
                const int i = T.fft_rv_tbl[jj] & 0xff;
                float* x = L.fz + fzp(4 * jj);
                double f0, f1, f2, f3, w;
                f0 = (double)T.window[i] * (double)xin[u][0];
                w = (double)T.window[i + 0x200] * (double)xin[u][1];
                f1 = f0 - w; f0 = f0 + w;
                f2 = (double)T.window[i + 0x100] * (double)xin[u][2];
                w = (double)T.window[i + 0x300] * (double)xin[u][3];
                f3 = f2 - w; f2 = f2 + w;
                x[0] = (float)(f0 + f2); x[2] = (float)(f0 - f2); x[1] = (float)(f1 + f3); x[3] = (float)(f1 - f3);
                f0 = (double)T.window[i + 0x001] * (double)xin[u][4];
                w = (double)T.window[i + 0x201] * (double)xin[u][5];
                f1 = f0 - w; f0 = f0 + w;
                f2 = (double)T.window[i + 0x101] * (double)xin[u][6];
                w = (double)T.window[i + 0x301] * (double)xin[u][7];
                f3 = f2 - w; f2 = f2 + w;
                x[fzo(BLKSIZE / 2) + 0] = (float)(f0 + f2); x[fzo(BLKSIZE / 2) + 2] = (float)(f0 - f2);
                x[fzo(BLKSIZE / 2) + 1] = (float)(f1 + f3); x[fzo(BLKSIZE / 2) + 3] = (float)(f1 - f3);
            }
        }
    }
    wave_sync();

    PSY_STAMP(2);
    // --- remaining FHT passes; twiddle table offsets 0,1,8,39 (pass t has kx-1 entries) ---
    {
        int off = 0;
#pragma unroll
        for (int k1 = 4, kx = 2; k1 < BLKSIZE; k1 <<= 2, kx <<= 2) {
            fht_pass(L.fz, BLKSIZE, k1, kx, lane, LHIP_NL, 0, T.fht_twiddle + 4 * off);
            if (k1 < BLKSIZE_s && shortw) fht_pass_blocks(&L.fs[0][0], 3, BLKSIZE_s, k1, kx, lane, LHIP_NL, T.fht_twiddle + 4 * off);
            wave_sync();
            off += kx - 1;
        }
    }
    if (Cp == 4) {                                    // joint stereo: the spectra the mid / side waves combine
        float* fo = W.fht + ((int64_t)gslot * 2 + ch) * FHT_STRIDE;
        const int nfht = shortw ? FHT_STRIDE : BLKSIZE;          // (the mid / side waves of the slot reach the same verdict and read no further)
        for (int i = lane; i < nfht; i += LHIP_NL) fo[i] = (i < BLKSIZE) ? L.fz[fzp(i)] : (&L.fs[0][0])[fzp(i - BLKSIZE)];
    }
    }   // ch < 2

    PSY_STAMP(3);
    // --- energies (PsyModel.js:274-296), written over the lower halves of the transform buffers ---
    {
        enum { KE = (BLKSIZE / 2 + 1 + LHIP_NL - 1) / LHIP_NL, KS = (3 * (BLKSIZE_s / 2 + 1) + LHIP_NL - 1) / LHIP_NL };
        float el[KE], es[KS];
#pragma unroll
        for (int u = 0; u < KE; u++) {
            const int j = lane + LHIP_NL * u;
            el[u] = 0.f;
            if (j == 0) { const float e0 = L.fz[0]; el[u] = (float)((double)e0 * (double)e0); }
            else if (j <= BLKSIZE / 2) { const double re = L.fz[fzp(j)], im = L.fz[fzp(BLKSIZE - j)]; el[u] = (float)((re * re + im * im) * 0.5); }
        }
#pragma unroll
        for (int u = 0; u < KS; u++) es[u] = 0.f;
        if (shortw) {
#pragma unroll
        for (int u = 0; u < KS; u++) {
            const int it = lane + LHIP_NL * u;
            if (it < 3 * (BLKSIZE_s / 2 + 1)) {
                const int b = it / (BLKSIZE_s / 2 + 1), j = it - b * (BLKSIZE_s / 2 + 1);
                const float* fsf = &L.fs[0][0];
                if (j == 0) { const float e0 = fsf[fzp(b * BLKSIZE_s)]; es[u] = (float)((double)e0 * (double)e0); }
                else { const double re = fsf[fzp(b * BLKSIZE_s + j)], im = fsf[fzp(b * BLKSIZE_s + BLKSIZE_s - j)]; es[u] = (float)((re * re + im * im) * 0.5); }
            }
        }
        }
        wave_sync();                                  // every lane has read its operands before anything is overwritten
#pragma unroll
        for (int u = 0; u < KE; u++) { const int j = lane + LHIP_NL * u; if (j <= BLKSIZE / 2) PSYA_FE(L)[j] = el[u]; }
        if (shortw) {
#pragma unroll
        for (int u = 0; u < KS; u++) {
            const int it = lane + LHIP_NL * u;
            if (it < 3 * (BLKSIZE_s / 2 + 1)) { const int b = it / (BLKSIZE_s / 2 + 1), j = it - b * (BLKSIZE_s / 2 + 1); PSYA_FES(L, b)[j] = es[u]; }
        }
        }
    }
    wave_sync();

    PSY_STAMP(4);
    // --- loudness: strictly sequential f64 sum (PsyModel.js:241-249), products in parallel, ordered fold ---
    {
        enum { K = (BLKSIZE / 2) / LHIP_NL };
        double pr[K];
#pragma unroll
        for (int k = 0; k < K; k++) { const int i = K * lane + k; pr[k] = (double)PSYA_FE(L)[i] * (double)T.eql_w[i]; }
        // The reference's sum is strictly sequential, and only its Float32 rounding is ever read.  All terms are >= 0, so a sum in ANY
        // order lies within (n - 1) u of the exact sum, as the reference's own does: the two differ by less than 1.2e-13 (relative).
        // A tree sum (8 adds per lane + a wave reduction instead of 64 hand-over steps) therefore rounds to the reference's Float32
        // whenever both ends of its 2e-13 error band round to the same Float32; when they do not (about one call in 10^5) the
        // sequential fold decides.  (T.eql_w >= 0 is checked where the table is loaded.)
        if (ch < 2) {                                 // no loudness for mid / side (PsyModel.js:319)
            float lf;
            if (!guarded_f32_of_sum<K>(pr, T.VO_SCALE, 0.0, &lf)) lf = (float)(wave_seq_sum<K>(pr) * T.VO_SCALE);
            if (lane == 0) W.loud[(int64_t)gslot * C + ch] = lf;
        }
        if (Cp == 4) {
            // total energy: lines 11 .. 512 summed in ascending order (PsyModel.js:300-307); the leading zeros change nothing
#pragma unroll
            for (int k = 0; k < K; k++) { const int i = K * lane + k; pr[k] = (i >= 11) ? (double)PSYA_FE(L)[i] : 0.0; }
            const double last = (double)PSYA_FE(L)[BLKSIZE / 2];
            float tf;
            if (!guarded_f32_of_sum<K>(pr, 1.0, last, &tf)) tf = (float)(wave_seq_sum<K>(pr) + last);
            if (lane == 0) W.tot_ener[(int64_t)gslot * 4 + ch] = tf;
        }
    }

    PSY_STAMP(5);
    if (PART == 3) return;
psya_tail:
    // --- long partitions: energy, max, average (calc_energy, PsyModel.js:906-928) ---
#if LHIP_NL == 1
    LHIP_LANE_ONCE(b, 0, T.npart_l) {                        // npart_l < CBANDS = 64
        double ebb = 0, m = 0;
        int j = T.lineoff_l[b];
        for (int i = 0; i < T.numlines_l[b]; ++i, ++j) {
            const double el = PSYA_FE(L)[j];
            ebb += el;
            if (m < el) m = el;
        }
        PSYA_EB(L)[b] = (float)ebb;
        PSYA_MX(L)[b] = (float)m;
        PSYA_AV(L)[b] = (float)(ebb * (double)T.rnumlines_l[b]);
    }
#else
    {
        // The partitions tile the 513 lines, and a partition's energy is the f64 sum of its lines in ascending order: a systolic fold
        // (as calc_noise's band sums, k_quant_noise.h) -- lane l owns the lines 8 l .. 8 l + 7 and folds them, in order, onto the running sum
        // lane l - 1 hands over, the chain restarting at every partition's first line; ceil(longest partition / 8) + 1 hand-overs give
        // every partition's strictly sequential sum (one lane per partition walking its lines took as many trips as the longest
        // partition has lines: 83 at 44.1 kHz).  Line 512 is added by lane 63 at the end -- it is the last line of the last partition.
        // The maxima are order-free: every lane reduces its lines per partition and merges through an LDS integer maximum (energies
        // are >= 0: IEEE order == integer order of the bit patterns).
        enum { KF = 8 };
        static_assert(BLKSIZE / 2 == KF * LHIP_NL, "psy_fold is laid out for 8 lines per lane");
        const int32_t* pf = T.psy_fold + 3 * lane;
        const uint32_t marks = (uint32_t)pf[0], pw0 = (uint32_t)pf[1], pw1 = (uint32_t)pf[2];
        LHIP_LANE_ONCE(b, 0, CBANDS) PSYA_MX(L)[b] = 0.f;
        double tq[KF], keep[KF];
        float ev[KF];
#pragma unroll
        for (int k = 0; k < KF; k++) { ev[k] = PSYA_FE(L)[KF * lane + k]; tq[k] = (double)ev[k]; keep[k] = one_unless_bit(marks, k); }
        const float e512 = PSYA_FE(L)[BLKSIZE / 2];
        wave_sync();                                  // the maxima start from zero
        {   // maxima: running maximum inside the lane, flushed where a partition ends (or the lane does)
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < KF; k++) {
                m = ((marks >> k) & 1u) ? ev[k] : fmax_nonneg(m, ev[k]);
                const int bnd = (int)(((k < 4 ? pw0 : pw1) >> (8 * (k & 3))) & 0xffu);
                float mm = m;
                if (lane == LHIP_NL - 1 && k == KF - 1 && !((marks >> (8 + k)) & 1u)) mm = fmax_nonneg(mm, e512);     // line 512 belongs to the same partition
                if (((marks >> (8 + k)) & 1u) || k == KF - 1) { int32_t bits; __builtin_memcpy(&bits, &mm, 4); lds_max((int32_t*)&PSYA_MX(L)[bnd], bits); }
            }
            if (lane == LHIP_NL - 1 && ((marks >> (8 + KF - 1)) & 1u)) {       // line 512 is a partition of its own (the last one)
                int32_t bits; __builtin_memcpy(&bits, &e512, 4); lds_max((int32_t*)&PSYA_MX(L)[T.npart_l - 1], bits);
            }
        }
        const int nsteps = (T.psy_maxlen_l + KF - 1) / KF + 1;
        double carry = 0.0;
        for (int st = 0; st + 1 < nsteps; st++) {
            double sacc = carry;
#pragma unroll
            for (int k = 0; k < KF; k++) sacc = __builtin_fma(sacc, keep[k], tq[k]);
            carry = wave_shr1d(sacc, 0.0);
        }
        {
            double sacc = carry;
#pragma unroll
            for (int k = 0; k < KF; k++) { sacc = __builtin_fma(sacc, keep[k], tq[k]); tq[k] = sacc; }   // tq := running sums of the last step
        }
#pragma unroll
        for (int k = 0; k < KF; k++) {
            const int bnd = (int)(((k < 4 ? pw0 : pw1) >> (8 * (k & 3))) & 0xffu);
            if ((marks >> (8 + k)) & 1u) { PSYA_EB(L)[bnd] = (float)tq[k]; PSYA_AV(L)[bnd] = (float)(tq[k] * (double)T.rnumlines_l[bnd]); }
        }
        if (lane == LHIP_NL - 1) {                    // the partition line 512 closes
            const int bl = T.npart_l - 1;
            const double ebb = ((marks >> (8 + KF - 1)) & 1u) ? (double)e512 : tq[KF - 1] + (double)e512;
            PSYA_EB(L)[bl] = (float)ebb; PSYA_AV(L)[bl] = (float)(ebb * (double)T.rnumlines_l[bl]);
        }
    }
#endif
    // --- short partitions: energy per sub-block (compute_masking_s first loop, 740-750) ---
    if (shortw) for (int it = lane; it < 3 * T.npart_s; it += LHIP_NL) {
        const int sblock = it / T.npart_s, b = it - sblock * T.npart_s;
        double ebb = 0;
        int j = T.lineoff_s[b];
        for (int i = 0; i < T.numlines_s[b]; ++i, ++j) ebb += (double)PSYA_FES(L, sblock)[j];
        PSYA_EBS(L, sblock)[b] = (float)ebb;
    }
    wave_sync();

    PSY_STAMP(6);
    // --- tonality index (calc_mask_index_l, PsyModel.js:930-992) ---
    for (int b = lane; b < CBANDS; b += LHIP_NL) {
        int k = 0;
        float ebv = 0.f;
        if (b < T.npart_l) {
            const int last = T.npart_l - 1;
            const int lo = b > 0 ? b - 1 : b, hi = b < last ? b + 1 : b;
            double a, m;
            int nl;
            if (b == 0) { a = (double)PSYA_AV(L)[0] + (double)PSYA_AV(L)[1]; nl = T.numlines_l[0] + T.numlines_l[1] - 1; }
            else if (b == last) { a = (double)PSYA_AV(L)[b - 1] + (double)PSYA_AV(L)[b]; nl = T.numlines_l[b - 1] + T.numlines_l[b] - 1; }
            else { a = (double)PSYA_AV(L)[b - 1] + (double)PSYA_AV(L)[b] + (double)PSYA_AV(L)[b + 1]; nl = T.numlines_l[b - 1] + T.numlines_l[b] + T.numlines_l[b + 1] - 1; }
            if (a > 0.0) {
                m = PSYA_MX(L)[lo];
                for (int t = lo + 1; t <= hi; t++) if (m < (double)PSYA_MX(L)[t]) m = PSYA_MX(L)[t];
                a = 20.0 * (m * (double)(hi - lo + 1) - a) / (a * nl);
                k = js_toint32(a);
                if (k > 8) k = 8;
            }
            ebv = PSYA_EB(L)[b];
        }
        W.eb_l[o * EBL_STRIDE + b] = ebv;
        W.mask_idx[o * EBL_STRIDE + b] = k;
    }
    // --- short spreading (compute_masking_s second loop before limiting, 752-760) ---
    // lane = partition; its spreading row is fetched once (independent loads) and applied to the three sub-blocks
    if (shortw) for (int b = lane; b < CBANDS; b += LHIP_NL) {
        float ecbv[3] = {0.f, 0.f, 0.f}, ebv[3] = {0.f, 0.f, 0.f};
        if (b < T.npart_s) {
            enum { MT = 12 };                         // rows are at most 12 long for every MPEG-1 rate; longer rows take the tail loop
            const int k0 = T.s3ind_s[2 * b], k1 = T.s3ind_s[2 * b + 1], j0 = T.s3off_s[b];
            float cf[MT];
#pragma unroll
            for (int u = 0; u < MT; u++) cf[u] = (k0 + u <= k1) ? T.s3_ss[j0 + u] : 0.f;
            for (int sblock = 0; sblock < 3; sblock++) {
                const float* e = PSYA_EBS(L, sblock);
                double ecb = (double)cf[0] * (double)e[k0];
#pragma unroll
                for (int u = 1; u < MT; u++) if (k0 + u <= k1) ecb += (double)cf[u] * (double)e[k0 + u];
                for (int kk = k0 + MT; kk <= k1; kk++) ecb += (double)T.s3_ss[j0 + (kk - k0)] * (double)e[kk];
                ecbv[sblock] = (float)ecb;
                ebv[sblock] = e[b];
            }
        }
        for (int sblock = 0; sblock < 3; sblock++) {
            W.ecb_s[o * EBS_STRIDE + sblock * CBANDS + b] = ecbv[sblock];
            W.eb_s[o * EBS_STRIDE + sblock * CBANDS + b] = ebv[sblock];
        }
    }
    PSY_STAMP(7);
    if (PART == 0 || PART == 2) PSY_FLUSH();
#undef buf
}
}  // namespace lhip
