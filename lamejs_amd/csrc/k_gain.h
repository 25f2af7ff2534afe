// k_gain.h -- ReplayGain analysis of the samples the encoder consumes (extension { replayGain }; GainAnalysis.js, Lame.js:1609-1613): per output channel
// the 10th-order "Yule" filter and the 2nd-order Butterworth high-pass of the published ReplayGain design, both in f64 with every output stored as Float32;
// the energy of the second filter's output over windows of ceil(fs / 20) samples; one histogram count per window at trunc(1000 log10(energy / window / 2 + 1e-37)).
//
// The reference runs the recursion through the whole stream.  Here the result is a pure function of the sample stream, whatever calls cut it into: window k
// covers the absolute samples [k window, (k + 1) window), and its energy comes from a recursion that starts from zero state GAIN wf samples in front of the
// window -- or at sample 0 of the stream, where that comes first (never over imagined zeros in front of it: the 1e-10 term would leave a state).  So the
// first windows of a stream are the reference's bit for bit, and all others differ from it by the rounding noise of two trajectories that have converged
// (DESIGN_EXTENSIONS.md 4.11 has the pole moduli and how wf follows from them).  The operations, their order and the Float32 stores are the reference's;
// within a window the squares are added in groups of eight from the window's first sample, each group as one sum, then what is left one by one.
//
// kb_gain_stage   one lane per sample: `history ++ this call's new samples` per channel, contiguous, into the context's workspace; the new samples are read
//                 where the encoder reads them (pcm_new_at on the caller's samples or g_ingest's planes; the plane g_prep fills behind the resampler).  The
//                 last wf + window - 1 samples of that row are the next call's history: they go to the OTHER of the stream's two history buffers, so no lane
//                 writes what another lane of the launch reads.
// kb_gain         one wave per LHIP_NL windows of one stream that complete in this call, a lane per window, both channels of a window in the same lane (two
//                 independent chains: the recursion is latency-bound).  All lanes of a wave walk the same number of steps, ending on their window's last
//                 sample, so whether a step is inside the window is wave-uniform; a lane whose recursion may not start yet (stream start) holds its state at
//                 zero.  A lane's samples are wf + window consecutive floats, 9.6 KB from its neighbour's: the wave fetches GAIN_TILE samples of every row
//                 with consecutive lanes on consecutive addresses and turns them through LDS (row stride GAIN_TILE + 1: no bank conflicts), then every lane
//                 reads its own row.  The filter state lives in registers: the step loop is unrolled by the filter order, so the delay line is renamed, not moved.
#pragma once
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"

namespace lhip {

enum { GAIN_BINS = 12000, GAIN_ORDER = 10, GAIN_TILE = 40, GAIN_STRIDE = GAIN_TILE + 1, GAIN_RATES = 9, GAIN_STAGE_NT = 256 };
static_assert(GAIN_TILE % GAIN_ORDER == 0, "the step loop is unrolled by the filter order");

// per output sample rate: the window ceil(fs / 20), the warm-up wf in front of a window (a multiple of 64; DESIGN_EXTENSIONS.md 4.11), the 21 coefficients of
// the Yule filter (b0, a1, b1, a2, ... b10, as the reference lists them) and the 5 of the Butterworth high-pass (b0, a1, b1, a2, b2)
struct GainRate { int fs, window, wf; double yule[21], butter[5]; };
struct GainRates { GainRate r[GAIN_RATES]; };
constexpr GainRates gain_rates() {
    return GainRates{{
        {48000, 2400, 2112,
         {0.03857599435200, -3.84664617118067, -0.02160367184185, 7.81501653005538, -0.00123395316851, -11.34170355132042, -0.00009291677959,
          13.05504219327545, -0.01655260341619, -12.28759895145294, 0.02161526843274, 9.48293806319790, -0.02074045215285, -5.87257861775999,
          0.00594298065125, 2.75465861874613, 0.00306428023191, -0.86984376593551, 0.00012025322027, 0.13919314567432, 0.00288463683916},
         {0.98621192462708, -1.97223372919527, -1.97242384925416, 0.97261396931306, 0.98621192462708}},
        {44100, 2205, 1984,
         {0.05418656406430, -3.47845948550071, -0.02911007808948, 6.36317777566148, -0.00848709379851, -8.54751527471874, -0.00851165645469,
          9.47693607801280, -0.00834990904936, -8.81498681370155, 0.02245293253339, 6.85401540936998, -0.02596338512915, -4.39470996079559,
          0.01624864962975, 2.19611684890774, -0.00240879051584, -0.75104302451432, 0.00674613682247, 0.13149317958808, -0.00187763777362},
         {0.98500175787242, -1.96977855582618, -1.97000351574484, 0.97022847566350, 0.98500175787242}},
        {32000, 1600, 1472,
         {0.15457299681924, -2.37898834973084, -0.09331049056315, 2.84868151156327, -0.06247880153653, -2.64577170229825, 0.02163541888798,
          2.23697657451713, -0.05588393329856, -1.67148153367602, 0.04781476674921, 1.00595954808547, 0.00222312597743, -0.45953458054983,
          0.03174092540049, 0.16378164858596, -0.01390589421898, -0.05032077717131, 0.00651420667831, 0.02347897407020, -0.00881362733839},
         {0.97938932735214, -1.95835380975398, -1.95877865470428, 0.95920349965459, 0.97938932735214}},
        {24000, 1200, 1152,
         {0.30296907319327, -1.61273165137247, -0.22613988682123, 1.07977492259970, -0.08587323730772, -0.25656257754070, 0.03282930172664,
          -0.16276719120440, -0.00915702933434, -0.22638893773906, -0.02364141202522, 0.39120800788284, -0.00584456039913, -0.22138138954925,
          0.06276101321749, 0.04500235387352, -0.00000828086748, 0.02005851806501, 0.00205861885564, 0.00302439095741, -0.02950134983287},
         {0.97531843204928, -1.95002759149878, -1.95063686409857, 0.95124613669835, 0.97531843204928}},
        {22050, 1103, 1024,
         {0.33642304856132, -1.49858979367799, -0.25572241425570, 0.87350271418188, -0.11828570177555, 0.12205022308084, 0.11921148675203,
          -0.80774944671438, -0.07834489609479, 0.47854794562326, -0.00469977914380, -0.12453458140019, -0.00589500224440, -0.04067510197014,
          0.05724228140351, 0.08333755284107, 0.00832043980773, -0.04237348025746, -0.01635381384540, 0.02977207319925, -0.01760176568150},
         {0.97316523498161, -1.94561023566527, -1.94633046996323, 0.94705070426118, 0.97316523498161}},
        {16000, 800, 832,
         {0.44915256608450, -0.62820619233671, -0.14351757464547, 0.29661783706366, -0.22784394429749, -0.37256372942400, -0.01419140100551,
          0.00213767857124, 0.04078262797139, -0.42029820170918, -0.12398163381748, 0.22199650564824, 0.04097565135648, 0.00613424350682,
          0.10478503600251, 0.06747620744683, -0.01863887810927, 0.05784820375801, -0.03193428438915, 0.03222754072173, 0.00541907748707},
         {0.96454515552826, -1.92783286977036, -1.92909031105652, 0.93034775234268, 0.96454515552826}},
        {12000, 600, 768,
         {0.56619470757641, -1.04800335126349, -0.75464456939302, 0.29156311971249, 0.16242137742230, -0.26806001042947, 0.16744243493672,
          0.00819999645858, -0.18901604199609, 0.45054734505008, 0.30931782841830, -0.33032403314006, -0.27562961986224, 0.06739368333110,
          0.00647310677246, -0.04784254229033, 0.08647503780351, 0.01639907836189, -0.03788984554840, 0.01807364323573, -0.00588215443421},
         {0.96009142950541, -1.91858953033784, -1.92018285901082, 0.92177618768381, 0.96009142950541}},
        {11025, 552, 704,
         {0.58100494960553, -0.51035327095184, -0.53174909058578, -0.31863563325245, -0.14289799034253, -0.20256413484477, 0.17520704835522,
          0.14728154134330, 0.02377945217615, 0.38952639978999, 0.15558449135573, -0.23313271880868, -0.25344790059353, -0.05246019024463,
          0.01628462406333, -0.02505961724053, 0.06920467763959, 0.02442357316099, -0.03721611395801, 0.01818801111503, -0.00749618797172},
         {0.95856916599601, -1.91542108074780, -1.91713833199203, 0.91885558323625, 0.95856916599601}},
        {8000, 400, 576,
         {0.53648789255105, -0.25049871956020, -0.42163034350696, -0.43193942311114, -0.00275953611929, -0.03424681017675, 0.04267842219415,
          -0.04678328784242, -0.10214864179676, 0.26408300200955, 0.14590772289388, 0.15113130533216, -0.02459864859345, -0.17556493366449,
          -0.11202315195388, -0.18823009262115, -0.04060034127000, 0.05477720428674, 0.04788665548180, 0.04704409688120, -0.02217936801134},
         {0.94597685600279, -1.88903307939452, -1.89195371200558, 0.89487434461664, 0.94597685600279}},
    }};
}
// the table's row of an output sample rate; -1: not one of the nine (cannot happen for a stream the library accepts)
static inline int gain_rate_index(int fs) {
    constexpr GainRates G = gain_rates();
    for (int i = 0; i < GAIN_RATES; i++) if (G.r[i].fs == fs) return i;
    return -1;
}
static inline int gain_window(int ri) { constexpr GainRates G = gain_rates(); return G.r[ri].window; }
static inline int gain_wf(int ri) { constexpr GainRates G = gain_rates(); return G.r[ri].wf; }
// samples of history a stream keeps per channel: what the window that ends with the next call's first sample needs
static inline int gain_keep(int ri) { return gain_wf(ri) + gain_window(ri) - 1; }

// What a stream carries on the device (allocated by lhip_create only with the option; neither StreamState nor the state blobs know it):
//   GainState | histogram, GAIN_BINS x u32 | history buffer 0 | history buffer 1        (a history buffer: channels x gain_keep() floats)
struct GainState { int64_t samples, windows; };
static inline size_t gain_state_bytes(int ri, int channels) { return sizeof(GainState) + (size_t)GAIN_BINS * 4 + (size_t)2 * channels * gain_keep(ri) * 4; }

// One stream of one launch.  The row of channel c is row[c][0 .. h + n): h samples of history (absolute samples [samples - h, samples)) and the call's n new ones.
//   stage:  lanes blk0 * GAIN_STAGE_NT ... cover the h + n positions;  hist_old[c] holds the h history samples, hist_new[c] receives the last `keep` of the row
//   gain:   windows win0 .. win0 + nwin - 1 complete in this call (absolute numbers); waves wave0 .. of the launch take LHIP_NL of them each
struct GainDesc {
    GainState* state; uint32_t* bins;
    const float* hist_old[2]; float* hist_new[2]; float* row[2];
    int32_t* dbg_bin; double* dbg_energy;      // test hook (lhip_debug_gain_windows): per window of the call, else null
    int64_t samples, win0;                     // samples analysed before this call; first window that completes in it
    int32_t h, n, keep, nwin, ri, channels, blk0, wave0;
};

// workgroup / wave b of a launch -> its stream: the last one whose first number is <= b (they ascend; a stream without work has none)
template <bool STAGE> LHIP_DEV int gain_find_stream(const GainDesc* D, int nstreams, int b) {
    int lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((STAGE ? D[mid].blk0 : D[mid].wave0) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// position i (0 <= i < h + n) of stream st's rows, both channels
LHIP_DEV void kb_gain_stage(const Tables& T, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, const GainDesc* D, int st, int64_t i) {
    const GainDesc& d = D[st];
    const int64_t total = (int64_t)d.h + d.n;
    if (i >= total) return;
    if (i == 0) { d.state->samples = d.samples + d.n; d.state->windows = d.win0 + d.nwin; }
    const int64_t k = i - d.h;                 // >= 0: new sample k of the call
    const int64_t to = i - (total - d.keep);   // >= 0: position in the next call's history
    for (int c = 0; c < d.channels; c++) {
        float v;
        if (k < 0) v = d.hist_old[c][i];
        else if (T.rs_ratio != 1) v = W.pcm[(int64_t)c * W.pcm_plane + SD[st].pcm_off + IO[st].mf_size + k];
        else {
            const PcmSrc P = pcm_source_new(T, IO[st], c);
            v = P.f32 ? pcm_new_at<1>(P, k) : pcm_new_at<0>(P, k);
        }
        d.row[c][i] = v;
        if (to >= 0) d.hist_new[c][to] = v;
    }
}

// one step of both filters for one channel: x = the new sample; xs / ys / bs: the last ten inputs, Yule outputs and (two of them used) Butterworth outputs
// as circular delay lines whose newest entry is at P (a compile-time constant: the caller unrolls by GAIN_ORDER).  Returns the Butterworth output (Float32).
template <int P> LHIP_DEV float gain_step(const double (&ky)[21], const double (&kb)[5], float x, bool on, float (&xs)[GAIN_ORDER], float (&ys)[GAIN_ORDER], float (&bs)[2]) {
#define GX(j) ((double)xs[(P + GAIN_ORDER - (j)) % GAIN_ORDER])      /* x[n - j - 1], j = 0 .. 9 */
#define GY(j) ((double)ys[(P + GAIN_ORDER - (j)) % GAIN_ORDER])
    const double y = 1e-10 + (double)x * ky[0] - GY(0) * ky[1] + GX(0) * ky[2] - GY(1) * ky[3] + GX(1) * ky[4] - GY(2) * ky[5] + GX(2) * ky[6]
                     - GY(3) * ky[7] + GX(3) * ky[8] - GY(4) * ky[9] + GX(4) * ky[10] - GY(5) * ky[11] + GX(5) * ky[12] - GY(6) * ky[13] + GX(6) * ky[14]
                     - GY(7) * ky[15] + GX(7) * ky[16] - GY(8) * ky[17] + GX(8) * ky[18] - GY(9) * ky[19] + GX(9) * ky[20];
    const float yf = on ? (float)y : 0.f;
    // the high-pass reads the Yule outputs y[n], y[n - 1], y[n - 2] and its own last two
    const double o = (double)yf * kb[0] - (double)bs[(P + 2 - 0) % 2] * kb[1] + GY(0) * kb[2] - (double)bs[(P + 2 - 1) % 2] * kb[3] + GY(1) * kb[4];
#undef GX
#undef GY
    const float of = on ? (float)o : 0.f;
    xs[(P + 1) % GAIN_ORDER] = on ? x : 0.f;
    ys[(P + 1) % GAIN_ORDER] = yf;
    bs[(P + 1) % 2] = of;
    return of;
}

// the squares of a window, in the reference's order for pieces that are multiples of eight: groups of eight from the window's first sample, each added to
// the sum as one parenthesised sum, then the rest one by one.  idx: position inside the window (wave-uniform); ngrp: 8 * (window / 8)
struct GainSum { double sum, grp; };
LHIP_DEV void gain_add(GainSum& s, float o, int idx, int ngrp) {
    const double q = (double)o * (double)o;
    if (idx >= ngrp) { s.sum += q; return; }
    s.grp = (idx & 7) ? s.grp + q : q;
    if ((idx & 7) == 7) s.sum += s.grp;
}

// wave `wv` of stream st (windows win0 + wv * LHIP_NL ...); lds: LHIP_NL * CH * GAIN_STRIDE floats
template <int CH> LHIP_DEV void kb_gain(const GainDesc* D, int st, int wv, int lane, float* lds) {
    constexpr GainRates G = gain_rates();
    const GainDesc& d = D[st];
    const int ri = d.ri, window = G.r[ri].window, wf = G.r[ri].wf, ngrp = window & ~7;
    double ky[21], kb[5];
    for (int j = 0; j < 21; j++) ky[j] = G.r[ri].yule[j];
    for (int j = 0; j < 5; j++) kb[j] = G.r[ri].butter[j];
    const int64_t total = (int64_t)d.h + d.n, abs0 = d.samples - d.h;          // the rows hold the absolute samples [abs0, abs0 + total)
    const int nrows = LHIP_NL * CH;
    // every lane ends on its window's last sample after `steps` steps (a whole number of tiles: the surplus in front is spent holding zero state)
    const int steps = (wf + window + GAIN_TILE - 1) / GAIN_TILE * GAIN_TILE;
    {
        const int w = wv * LHIP_NL + lane;                  // the call's window number: a lane is a window
        const bool have = w < d.nwin;
        const int64_t wstart = (d.win0 + w) * (int64_t)window - abs0;      // in row coordinates; >= 0 for a window that completes in this call
        const int64_t first = have ? (wstart - wf > 0 ? wstart - wf : 0) : 0;      // where this lane's recursion starts: wf in front, or at the stream's (== the row's) first sample
        const int64_t base = wstart + window - steps;       // row position of step 0 (may be negative)
        float xs[CH][GAIN_ORDER], ys[CH][GAIN_ORDER], bs[CH][2];
        GainSum acc[CH];
        for (int c = 0; c < CH; c++) { for (int j = 0; j < GAIN_ORDER; j++) xs[c][j] = ys[c][j] = 0.f; bs[c][0] = bs[c][1] = 0.f; acc[c].sum = 0.0; acc[c].grp = 0.0; }
        for (int t0 = 0; t0 < steps; t0 += GAIN_TILE) {
            // the tile: GAIN_TILE samples of every row of the wave, consecutive lanes on consecutive samples of a row; outside [0, total) a zero that no active step reads
            wave_sync();
            for (int e = lane; e < nrows * GAIN_TILE; e += LHIP_NL) {
                const int r = e / GAIN_TILE, col = e - r * GAIN_TILE, rl = r / CH, rc = r - rl * CH;
                const int rw = wv * LHIP_NL + rl;
                const int64_t p = (d.win0 + rw) * (int64_t)window - abs0 + window - steps + t0 + col;
                float v = 0.f;
                if (rw < d.nwin && p >= 0 && p < total) v = (rc ? d.row[1] : d.row[0])[p];
                lds[r * GAIN_STRIDE + col] = v;
            }
            wave_sync();
            const float* mine = lds + lane * CH * GAIN_STRIDE;
            for (int q = 0; q < GAIN_TILE; q += GAIN_ORDER) {
#define GAIN_STEP(PP) { const int t = t0 + q + PP; const bool on = have && base + t >= first; const int idx = t - (steps - window); \
                        for (int c = 0; c < CH; c++) { const float o = gain_step<PP>(ky, kb, mine[c * GAIN_STRIDE + q + PP], on, xs[c], ys[c], bs[c]); if (idx >= 0) gain_add(acc[c], o, idx, ngrp); } }
                GAIN_STEP(0) GAIN_STEP(1) GAIN_STEP(2) GAIN_STEP(3) GAIN_STEP(4) GAIN_STEP(5) GAIN_STEP(6) GAIN_STEP(7) GAIN_STEP(8) GAIN_STEP(9)
#undef GAIN_STEP
            }
        }
        if (have) {
            const double e = acc[0].sum + (CH == 2 ? acc[CH - 1].sum : acc[0].sum);      // lsum + rsum; one channel: rsum = lsum
            const double val = 100. * 10. * v8_log10(e / (double)window * 0.5 + 1.e-37);
            int bin = val <= 0 ? 0 : (int)val;                   // (val is finite and below 2^31: e <= 2 window (4 * 131072)^2 ... far below)
            if (bin >= GAIN_BINS) bin = GAIN_BINS - 1;
#ifdef LHIP_HOSTSIM
            d.bins[bin]++;
#else
            atomicAdd(d.bins + bin, 1u);
#endif
            if (d.dbg_bin) { d.dbg_bin[w] = bin; d.dbg_energy[w] = e; }
        }
    }
}

}  // namespace lhip
