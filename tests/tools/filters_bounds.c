/* TEST TOOL (tests/test_filters_cpu.py::test_bounds_under_sanitizers): built with -fsanitize=address,undefined together with lhip_api.cpp as a simulation
 * (-DLHIP_HOSTSIM, and once more with -DLHIP_WAVESIM), so that every load and store of the kernel bodies is checked in the states the options
 * { outSampleRate, lowpass, lowpassWidth, highpass, highpassWidth } add: zero polyphase bands at the bottom of the spectrum, all 32 bands open, other
 * resampling ratios and input rates.  Streams of bursts over a quiet tone with three frames of digital silence in front, in heap blocks that end with
 * the last sample: one batch call, then the same samples in calls of 1152 and of uneven lengths (the one-frame program and short batches), whose
 * bytes must be the batch call's.
 * usage: filters_bounds <channels> <samplerate> <kbps> <tables blob> [... more such quadruples] */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "lamejs_hip.h"

static uint32_t rnd_state = 20403u;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static int fail(const char* what, int a, int b) { fprintf(stderr, "filters_bounds: %s (%d, %d): %s\n", what, a, b, lhip_last_error()); return 1; }

static void* slurp(const char* path, size_t* n) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    long tb = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* p = malloc((size_t)tb);
    if (fread(p, 1, (size_t)tb, f) != (size_t)tb) exit(2);
    fclose(f);
    *n = (size_t)tb;
    return p;
}

/* the stream in calls of lens[] (cycled) -> bytes, the flush included */
static long encode(const lhip_config* cfg, const void* blob, size_t nblob, const int16_t* L, const int16_t* R, size_t n, const int* lens, int nlens, uint8_t* out, size_t cap) {
    lhip_stream* h = NULL;
    if (lhip_create(cfg, blob, nblob, &h) != 0) return -1;
    long total = 0;
    size_t p = 0;
    for (int i = 0; p < n; i++) {
        size_t m = (size_t)lens[i % nlens];
        if (m > n - p) m = n - p;
        /* every call's input in a block of its own that ends with its last sample */
        int16_t* l = (int16_t*)malloc(m * 2); int16_t* r = (int16_t*)malloc(m * 2);
        memcpy(l, L + p, m * 2); memcpy(r, R + p, m * 2);
        const int64_t w = lhip_encode(h, l, cfg->channels == 2 ? r : l, m, out + total, cap - (size_t)total);
        free(l); free(r);
        if (w < 0) { lhip_destroy(h); return -1; }
        total += (long)w; p += m;
    }
    const int64_t w = lhip_flush(h, out + total, cap - (size_t)total);
    lhip_destroy(h);
    return w < 0 ? -1 : total + (long)w;
}

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 1) % 4) { fprintf(stderr, "usage: filters_bounds <channels> <samplerate> <kbps> <tables blob> [...]\n"); return 2; }
    long streams = 0;
    for (int a = 1; a + 3 < argc; a += 4) {
        lhip_config cfg; memset(&cfg, 0, sizeof cfg);
        cfg.channels = atoi(argv[a]); cfg.samplerate = atoi(argv[a + 1]); cfg.kbps = atoi(argv[a + 2]); cfg.device = -1;
        const size_t n = (size_t)(14 * 1152 + 391) * (size_t)(cfg.samplerate > 48000 ? cfg.samplerate / 48000 : 1);      /* (about as many frames whatever the input rate) */
        size_t nblob = 0;
        void* blob = slurp(argv[a + 3], &nblob);
        int16_t* L = (int16_t*)malloc(n * 2); int16_t* R = (int16_t*)malloc(n * 2);
        for (size_t i = 0; i < n; i++) {
            const int loud = (i % 5000) >= 3000 && (i % 5000) < 3600;
            const int tone = (int)(i % 100) * 60 - 3000;
            L[i] = i < 3 * 1152 ? 0 : (int16_t)(tone + (loud ? (int)(rnd() % 24000) - 12000 : (int)(rnd() % 600) - 300));
            R[i] = i < 3 * 1152 ? 0 : (int16_t)(tone / 2 + (loud ? (int)(rnd() % 20000) - 10000 : (int)(rnd() % 400) - 200));
        }
        const size_t cap = (n / 576 + 8) * 1500 + 16384;
        uint8_t* whole = (uint8_t*)malloc(cap); uint8_t* parts = (uint8_t*)malloc(cap);
        const int ONE[] = {(int)n}, FRAMES[] = {1152}, UNEVEN[] = {1, 17, 777, 4096, 2305};
        const long nw = encode(&cfg, blob, nblob, L, R, n, ONE, 1, whole, cap);
        if (nw <= 0) return fail("batch call", cfg.channels, cfg.samplerate);
        for (int k = 0; k < 2; k++) {
            const long np = encode(&cfg, blob, nblob, L, R, n, k ? UNEVEN : FRAMES, k ? 5 : 1, parts, cap);
            if (np != nw || memcmp(whole, parts, (size_t)nw) != 0) return fail("the stream in calls differs from the stream in one call", cfg.channels, k);
        }
        free(whole); free(parts); free(L); free(R); free(blob);
        streams += 3;
    }
    printf("filters_bounds OK: %ld streams\n", streams);
    return 0;
}
