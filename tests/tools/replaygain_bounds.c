/* TEST TOOL (tests/test_replaygain_cpu.py::test_bounds_under_asan): built with -fsanitize=address together with lhip_api.cpp as a simulation
 * (-DLHIP_HOSTSIM, and once more with -DLHIP_WAVESIM), so that every load and store of the bodies of g_gain_stage and g_gain is checked.
 * lhip_debug_gain_windows puts the samples and the rows (history ++ new samples, per channel) into heap blocks of exactly their size, so a read or a write one
 * float past either is seen; the stream entry (lhip_encode_pcm on a { replayGain } stream) reads the caller's samples from blocks that END with the call's last
 * sample and keeps its history in a block that ends with the second history buffer.  Shapes: a call of one sample, calls that end exactly on a window boundary,
 * calls shorter and longer than the history that is kept (the history shifts / is replaced whole), a stream whose calls never complete a window.
 * usage: replaygain_bounds <tables blob of (2, 8000, 24) built with replayGain> */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lamejs_hip.h"

static uint32_t rnd_state = 4711u;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static int fail(const char* what, long a, long b) { fprintf(stderr, "replaygain_bounds: %s (%ld, %ld): %s\n", what, a, b, lhip_last_error()); return 1; }

int main(int argc, char** argv) {
    static const int RATES[] = {48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000};
    static const int WINDOW[] = {2400, 2205, 1600, 1200, 1103, 800, 600, 552, 400};
    if (argc < 2) { fprintf(stderr, "usage: replaygain_bounds <tables blob>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    long tb = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* tables = malloc((size_t)tb);
    if (fread(tables, 1, (size_t)tb, f) != (size_t)tb) return 2;
    fclose(f);
    long checks = 0;
    /* the kernels over one array: one sample, one short of a window, exactly one, two and 65 windows (a second wave), one more */
    for (int ri = 0; ri < 9; ri++)
        for (int ch = 1; ch <= 2; ch++) {
            const int w = WINDOW[ri];
            const long NS[] = {1, 7, w - 1, w, w + 1, 2 * w, 3 * w + 17, (ri == 8 ? 65L * w : 4L * w)};
            for (size_t ni = 0; ni < sizeof NS / sizeof NS[0]; ni++) {
                const long n = NS[ni], nwin = n / w;
                float* l = (float*)malloc((size_t)n * 4);
                float* r = (float*)malloc((size_t)n * 4);
                int32_t* bins = (int32_t*)malloc((size_t)(nwin ? nwin : 1) * 4);
                double* en = (double*)malloc((size_t)(nwin ? nwin : 1) * 8);
                for (long i = 0; i < n; i++) { l[i] = (float)((int)(rnd() % 20001) - 10000); r[i] = (float)((int)(rnd() % 2001) - 1000); }
                if (lhip_debug_gain_windows(RATES[ri], ch, l, ch == 2 ? r : NULL, (size_t)n, bins, en) != (int)nwin) return fail("lhip_debug_gain_windows", RATES[ri], n);
                for (long k = 0; k < nwin; k++) if (bins[k] < 3000 || bins[k] > 9000 || !(en[k] > 0)) return fail("window result", k, bins[k]);
                free(l); free(r); free(bins); free(en);
                checks++;
            }
        }
    /* a stream: 8 kHz, two channels, window 400, 975 samples of history */
    {
        static const int CALLS[] = {1, 399, 400, 1, 7, 9, 11, 381, 401, 974, 975, 976, 1152, 3000, 1, 1, 2398};
        lhip_config cfg; memset(&cfg, 0, sizeof cfg);
        cfg.channels = 2; cfg.samplerate = 8000; cfg.kbps = 24; cfg.device = 0;
        lhip_stream* s = NULL;
        if (lhip_create(&cfg, tables, (size_t)tb, &s) != 0) return fail("lhip_create", 0, 0);
        long total = 0;
        for (size_t ci = 0; ci < sizeof CALLS / sizeof CALLS[0]; ci++) {
            const int n = CALLS[ci];
            int16_t* l = (int16_t*)malloc((size_t)n * 2);
            int16_t* r = (int16_t*)malloc((size_t)n * 2);
            for (int i = 0; i < n; i++) { l[i] = (int16_t)((int)(rnd() % 20001) - 10000); r[i] = (int16_t)((int)(rnd() % 2001) - 1000); }
            const size_t cap = lhip_max_output_bytes(s, (size_t)n);
            uint8_t* out = (uint8_t*)malloc(cap);
            if (lhip_encode_pcm(s, LHIP_PCM_S16, l, r, (size_t)n, out, cap) < 0) return fail("lhip_encode_pcm", (long)ci, n);
            total += n;
            int32_t tenth = 0; int64_t windows = -1, samples = -1;
            const int rc = lhip_replay_gain(s, &tenth, &windows, &samples);
            if (rc < 0 || samples != total || windows != total / 400 || (rc == 1) != (windows == 0)) return fail("lhip_replay_gain", (long)windows, (long)samples);
            free(l); free(r); free(out);
            checks++;
        }
        lhip_destroy(s);
    }
    free(tables);
    printf("replaygain_bounds OK: %ld checks\n", checks);
    return 0;
}
